"""Checkpoint files and the epoch-end BN averaging on the host (no GPU): utils.checkpoint's
load_ckpt / save_checkpoint (reference utils/checkpoint.py), dp.all_reduce_norm over two gloo
ranks (utils/allreduce_norm.py), the evaluation-dataset hook of YoloxConfig and the CLI's
argument check."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pixeltable-yolox_amd")


def _nano(num_classes):
    from yolox_amd.config import named_config
    cfg = named_config("yolox_nano")
    cfg.num_classes = num_classes
    return cfg.get_model()


# ------------------------------------------------------------------ load_ckpt
def test_load_ckpt_copies_equal_shapes_and_keeps_the_rest(capsys):
    from yolox_amd.utils.checkpoint import load_ckpt
    from yolox_amd.weights import synthetic_state_dict
    src = _nano(80)
    ckpt = synthetic_state_dict(src.state_dict(), seed=5)
    model = _nano(3)
    init = {k: v.clone() for k, v in model.state_dict().items()}
    cls = {f"head.cls_preds.{i}.{n}" for i in range(3) for n in ("weight", "bias")}
    assert cls <= set(init) and all(init[k].shape != ckpt[k].shape for k in cls)
    missing = "backbone.backbone.stem.conv.conv.weight"
    assert not torch.equal(init[missing], ckpt[missing])
    del ckpt[missing]
    assert load_ckpt(model, ckpt) is model
    got = model.state_dict()
    assert set(got) == set(init)
    for k, v in got.items():
        if k in cls or k == missing:
            assert torch.equal(v, init[k]), k
        else:
            assert torch.equal(v, ckpt[k]), k
    # the biases kept are the config's prior-probability initialisation
    assert torch.allclose(got["head.cls_preds.0.bias"], torch.full((3,), -4.59511985))
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 7
    assert sum(missing in ln and "not in the checkpoint" in ln for ln in out) == 1
    for k in cls:
        (ln,) = [ln for ln in out if f" {k} " in ln]
        assert str(tuple(ckpt[k].shape)) in ln and str(tuple(init[k].shape)) in ln


# ------------------------------------------------------------------ save_checkpoint
def test_save_checkpoint_files(tmp_path):
    from yolox_amd.utils.checkpoint import save_checkpoint
    d = tmp_path / "run" / "name"  # created by the save, parents included
    state = {"start_epoch": 1, "model": {"w": torch.arange(6.0).view(2, 3)}}
    save_checkpoint(state, False, str(d), "latest")
    assert sorted(os.listdir(d)) == ["latest_ckpt.pth"]
    save_checkpoint(state, True, str(d), "epoch_1")
    assert sorted(os.listdir(d)) == ["best_ckpt.pth", "epoch_1_ckpt.pth", "latest_ckpt.pth"]  # no temporary left
    assert (d / "best_ckpt.pth").read_bytes() == (d / "epoch_1_ckpt.pth").read_bytes()
    # one state under two names: the same bytes (the trainer's last_epoch / epoch_<n> / best files)
    assert (d / "latest_ckpt.pth").read_bytes() == (d / "epoch_1_ckpt.pth").read_bytes()
    got = torch.load(d / "best_ckpt.pth", weights_only=True)
    assert got["start_epoch"] == 1 and torch.equal(got["model"]["w"], state["model"]["w"])


def test_save_checkpoint_keeps_the_old_file_when_the_write_fails(tmp_path):
    """A write that dies half way leaves the previous latest_ckpt.pth whole and no temporary."""
    from yolox_amd.utils.checkpoint import save_checkpoint
    save_checkpoint({"start_epoch": 1}, False, str(tmp_path), "latest")
    before = (tmp_path / "latest_ckpt.pth").read_bytes()
    with pytest.raises(Exception):
        save_checkpoint({"start_epoch": 2, "bad": lambda: 0}, False, str(tmp_path), "latest")  # not picklable
    assert os.listdir(tmp_path) == ["latest_ckpt.pth"]
    assert (tmp_path / "latest_ckpt.pth").read_bytes() == before


def test_trainer_shaped_state_round_trips_weights_only(tmp_path):
    """What Trainer.save_ckpt writes: model, SGD(nesterov, foreach) state after one step, the
    scalars and a GradScaler dict -- read back with weights_only=True, as resume and
    from_pretrained read it."""
    from yolox_amd.trainer import get_optimizer
    from yolox_amd.utils.checkpoint import save_checkpoint
    model = _nano(3)
    opt = get_optimizer(model, lr=0.01)
    assert opt.defaults["nesterov"] and opt.defaults["foreach"]
    for i, p in enumerate(model.parameters()):
        p.grad = torch.full_like(p, 1e-3 * (i % 5 + 1))
    opt.step()
    scaler = {"scale": 65536.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000,
              "_growth_tracker": 3}
    state = {"start_epoch": 2, "model": model.state_dict(), "optimizer": opt.state_dict(), "best_ap": 0.25,
             "curr_ap": None, "scaler": scaler}
    save_checkpoint(state, True, str(tmp_path), "last_epoch")
    save_checkpoint(state, False, str(tmp_path), "epoch_2")
    assert (tmp_path / "epoch_2_ckpt.pth").read_bytes() == (tmp_path / "best_ckpt.pth").read_bytes()
    got = torch.load(tmp_path / "best_ckpt.pth", map_location="cpu", weights_only=True)
    assert set(got) == set(state)
    assert (got["start_epoch"], got["best_ap"], got["curr_ap"], got["scaler"]) == (2, 0.25, None, scaler)
    assert list(got["model"]) == list(state["model"])
    for k, v in state["model"].items():
        assert torch.equal(got["model"][k], v) and got["model"][k].dtype == v.dtype, k
    want = state["optimizer"]
    assert got["optimizer"]["param_groups"] == want["param_groups"] and len(want["param_groups"]) == 3
    assert set(got["optimizer"]["state"]) == set(want["state"]) and len(want["state"]) == len(list(model.parameters()))
    for i, s in want["state"].items():
        assert torch.equal(got["optimizer"]["state"][i]["momentum_buffer"], s["momentum_buffer"])
    # and it loads: a fresh model + optimizer continue from it
    model2 = _nano(3)
    opt2 = get_optimizer(model2, lr=0.5)
    model2.load_state_dict(got["model"])
    opt2.load_state_dict(got["optimizer"])
    assert opt2.param_groups[0]["lr"] == 0.01 and opt2.param_groups[1]["weight_decay"] == 5e-4
    for p, p2 in zip(model.parameters(), model2.parameters()):
        assert torch.equal(opt2.state[p2]["momentum_buffer"], opt.state[p]["momentum_buffer"])


# ------------------------------------------------------------------ all_reduce_norm
class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 4, 1)
        self.bn1 = nn.BatchNorm2d(4)
        self.block = nn.Sequential(nn.Conv2d(4, 6, 1), nn.BatchNorm2d(6))


def _fill(net, rank):
    """Rank-dependent values in every tensor; ``num_batches_tracked`` 3 and 7 (mean 5)."""
    with torch.no_grad():
        for i, (k, v) in enumerate(net.state_dict().items()):
            if v.dtype.is_floating_point:
                v.copy_(torch.arange(v.numel(), dtype=torch.float32).view_as(v) * (rank + 1) + i + 10.0 * rank)
            else:
                v.fill_(3 + 4 * rank)


def _norm_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from yolox_amd.dp import all_reduce_norm
        net = _Net()
        _fill(net, rank)
        all_reduce_norm(net)
        q.put((rank, {k: (str(v.dtype), v.tolist()) for k, v in net.state_dict().items()}))
    finally:
        dist.destroy_process_group()


def test_all_reduce_norm_gloo_world2():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_norm_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    nets = [_Net(), _Net()]
    for r, n in enumerate(nets):
        _fill(n, r)
    sd0, sd1 = nets[0].state_dict(), nets[1].state_dict()
    norm_keys = [k for k in sd0 if k.startswith(("bn1.", "block.1."))]
    assert len(norm_keys) == 10
    for rank in range(2):
        for k, (dtype, vals) in res[rank].items():
            got = torch.tensor(vals, dtype=sd0[k].dtype)
            assert dtype == str(sd0[k].dtype), k
            if k in norm_keys:
                if k.endswith("num_batches_tracked"):
                    assert dtype == "torch.int64" and got.item() == 5
                else:  # the mean of two float32 values: (a + b) / 2, one rounding of the sum
                    assert torch.equal(got, (sd0[k] + sd1[k]) / 2), (rank, k)
                    assert not torch.equal(got, sd0[k])
            else:  # conv weights and biases stay this rank's own
                assert torch.equal(got, (sd0, sd1)[rank][k]), (rank, k)


def test_all_reduce_norm_is_a_noop_without_a_world(tmp_path):
    from yolox_amd.dp import all_reduce_norm
    net = _Net()
    _fill(net, 1)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    all_reduce_norm(net)  # no process group
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'pg'}", rank=0, world_size=1)
    try:
        all_reduce_norm(net)  # a world of one
    finally:
        dist.destroy_process_group()
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]) and v.dtype == before[k].dtype, k


# ------------------------------------------------------------------ config, CLI
def test_eval_loader_falls_back_to_the_configs_dataset():
    from yolox_amd.config import YoloxConfig, named_config
    assert named_config("yolox_s").get_eval_dataset(testdev=False, legacy=False) is None
    with pytest.raises(NotImplementedError):
        named_config("yolox_s").get_eval_loader(2, False)
    asked = []

    class _Set:
        def __len__(self):
            return 5

    class _Cfg(YoloxConfig):
        def get_eval_dataset(self, **kwargs):
            asked.append(kwargs)
            return _Set()

    cfg = _Cfg("mine", test_size=(96, 128))
    loader = cfg.get_eval_loader(2, False, legacy=True)
    assert isinstance(loader.dataset, _Set) and len(loader) == 3 and loader.size == (96, 128) and loader.legacy
    assert asked == [{"testdev": False, "legacy": True}]
    mine = _Set()
    assert cfg.get_eval_loader(2, False, dataset=mine).dataset is mine and len(asked) == 1
    assert cfg.get_evaluator(2, False).dataloader.dataset.__class__ is _Set


@pytest.mark.parametrize("flags", [["--resume"], ["--ckpt", "x"], ["-e", "3"], ["--resume", "--ckpt", "x", "-e", "3"]])
def test_cli_accepts_the_checkpoint_flags(flags):
    from yolox_amd.cli import check_args, make_parser
    args = make_parser().parse_args(["-c", "yolox_s"] + flags)
    check_args(args)
    assert args.resume == ("--resume" in flags)
    assert args.ckpt == ("x" if "--ckpt" in flags else None)
    assert args.start_epoch == (3 if "-e" in flags else None)


def test_cli_still_refuses_cache_and_a_missing_config():
    from yolox_amd.cli import check_args, make_parser
    with pytest.raises(NotImplementedError):
        check_args(make_parser().parse_args(["-c", "yolox_s", "--cache"]))
    with pytest.raises(AttributeError):
        check_args(make_parser().parse_args(["--resume"]))
