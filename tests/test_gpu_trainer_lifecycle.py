"""The trainer's epoch ends on the device (reference core/trainer.py:131-179, 217-237, 312-429):
checkpoint files, best checkpoint, --resume, --ckpt fine-tuning, the epoch-end evaluation and two
ranks.  Setup (trainer_lifecycle_common): yolox_s at 128 x 128, batch 2, a dataset of 4 (two
iterations per epoch), two epochs (one warm-up, one no-aug), evaluation every epoch over three
ragged images, deterministic (no multiscale redraws), by-shape training tiles.

The weight-gradient kernels sum with fp32 atomics, so two training runs are not bit-identical:
every comparison here is between a file and live state, or between two loads of one file, and is
exact.  The inference plans of both evaluations in the live-EMA test are fp32 eager plans with the
default tiles (plans pick tiles by timing only when Plan.autotune is called; nothing here does)."""
import json
import os
import random
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXPECTED_FILES = sorted(f"{n}_ckpt.pth" for n in ("latest", "last_mosaic_epoch", "last_epoch", "epoch_1", "epoch_2"))


@pytest.fixture(scope="module", autouse=True)
def _by_shape_tiles():
    old = os.environ.get("YOLOX_AMD_TRAIN_TUNE")
    os.environ["YOLOX_AMD_TRAIN_TUNE"] = "0"  # read when a train graph is built
    yield
    if old is None:
        os.environ.pop("YOLOX_AMD_TRAIN_TUNE", None)
    else:
        os.environ["YOLOX_AMD_TRAIN_TUNE"] = old


def _trainer(cfg, args):
    from yolox_amd.trainer import Trainer
    random.seed(cfg.seed)
    torch.manual_seed(cfg.seed)
    return Trainer(cfg, args)


def _load(path):
    return torch.load(path, map_location="cuda", weights_only=True)


def _momentum(trainer):
    """The fused step's momentum views in the optimizer state_dict's index order."""
    return [trainer.fused.bufs[id(p)] for g in trainer.optimizer.param_groups for p in g["params"]]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """One two-epoch fp32 run with the evaluation dataset; the tests below only read it."""
    from trainer_lifecycle_common import make_args, make_config, spy_on_eval
    out = tmp_path_factory.mktemp("run")
    cfg = make_config(out)
    evals = spy_on_eval(cfg)
    trainer = _trainer(cfg, make_args())
    trainer.train()
    torch.cuda.synchronize()
    return {"dir": out / "yolox_s", "out": out, "cfg": cfg, "trainer": trainer, "evals": evals}


# ------------------------------------------------------------------ 1. files and contents
def test_files_and_contents(run):
    trainer, d = run["trainer"], run["dir"]
    assert sorted(os.listdir(d)) == EXPECTED_FILES  # no best (AP without ground truth), no temporaries
    latest = _load(d / "latest_ckpt.pth")
    assert latest["start_epoch"] == 2 and "scaler" not in latest
    assert set(latest) == {"start_epoch", "model", "optimizer", "best_ap", "curr_ap"}
    live = trainer.ema_model.ema.state_dict()
    assert list(latest["model"]) == list(live)
    for k, v in live.items():
        assert torch.equal(latest["model"][k], v) and latest["model"][k].dtype == v.dtype, k
    state = latest["optimizer"]["state"]
    bufs = _momentum(trainer)
    assert sorted(state) == list(range(len(bufs)))
    for i, b in enumerate(bufs):
        assert torch.equal(state[i]["momentum_buffer"], b), i
    assert any(float(b.abs().max()) > 0 for b in bufs)
    assert _load(d / "last_mosaic_epoch_ckpt.pth")["start_epoch"] == 1
    assert _load(d / "epoch_1_ckpt.pth")["start_epoch"] == 1
    last = _load(d / "last_epoch_ckpt.pth")
    assert last["start_epoch"] == 2 and last["curr_ap"] == run["evals"][1][1][0][0]


def test_fp16_run_saves_the_live_scaler(tmp_path):
    """--fp16, no evaluation dataset: the evaluation is skipped, the files are still written."""
    from trainer_lifecycle_common import make_args, make_config
    trainer = _trainer(make_config(tmp_path, val=False), make_args(fp16=True))
    trainer.train()
    assert trainer.evaluator is None
    assert sorted(os.listdir(tmp_path / "yolox_s")) == EXPECTED_FILES
    latest = _load(tmp_path / "yolox_s" / "latest_ckpt.pth")
    assert latest["scaler"]["scale"] == trainer.scaler.get_scale()
    assert latest["scaler"]["_growth_tracker"] == int(trainer.scaler._growth_tracker.item())
    assert latest["scaler"] == trainer.scaler.state_dict()
    last = _load(tmp_path / "yolox_s" / "last_epoch_ckpt.pth")
    assert last["curr_ap"] is None and last["best_ap"] == 0 and last["start_epoch"] == 2


# ------------------------------------------------------------------ 2. best checkpoint
def test_best_checkpoint_follows_the_best_ap(tmp_path):
    from trainer_lifecycle_common import make_args, make_config
    cfg = make_config(tmp_path)
    aps = [0.2, 0.1]
    cfg.eval = lambda model, evaluator, dist, half=False, return_outputs=False: ((aps.pop(0), 0.3, "stub"), {})
    trainer = _trainer(cfg, make_args())
    trainer.train()
    d = tmp_path / "yolox_s"
    assert not aps and trainer.best_ap == 0.2
    assert sorted(os.listdir(d)) == sorted(EXPECTED_FILES + ["best_ckpt.pth"])
    assert (d / "best_ckpt.pth").read_bytes() == (d / "epoch_1_ckpt.pth").read_bytes()
    best, last = _load(d / "best_ckpt.pth"), _load(d / "last_epoch_ckpt.pth")
    assert (best["start_epoch"], best["best_ap"], best["curr_ap"]) == (1, 0.2, 0.2)
    assert (last["start_epoch"], last["best_ap"], last["curr_ap"]) == (2, 0.2, 0.1)


# ------------------------------------------------------------------ 3. resume
def test_resume_restores_live_state(run):
    from trainer_lifecycle_common import make_args, make_config
    path = run["dir"] / "epoch_1_ckpt.pth"
    ckpt = _load(path)
    ckpt["best_ap"] = 0.125  # resume must take it from the file
    path2 = run["out"] / "resume_from.pth"
    torch.save(ckpt, path2)
    trainer = _trainer(make_config(run["out"]), make_args(resume=True, ckpt=str(path2)))
    trainer.before_train()
    assert trainer.start_epoch == 1 and trainer.best_ap == 0.125 and trainer.no_aug
    model = trainer.model.state_dict()
    ema = trainer.ema_model.ema.state_dict()
    assert list(model) == list(ckpt["model"]) == list(ema)
    for k, v in ckpt["model"].items():
        assert torch.equal(model[k], v), k
        assert torch.equal(ema[k], v) and ema[k].data_ptr() != model[k].data_ptr(), k
    assert trainer.max_iter == 2 and trainer.ema_model.updates == trainer.max_iter * trainer.start_epoch
    loaded = [ckpt["optimizer"]["state"][i]["momentum_buffer"] for i in range(len(trainer.fused.params))]
    for b, want in zip(_momentum(trainer), loaded):
        assert torch.equal(b, want)
    assert any(float(w.abs().max()) > 0 for w in loaded)
    # one iteration of the resumed epoch
    trainer.epoch, trainer.iter = trainer.start_epoch, 0
    trainer.before_epoch()
    trainer.train_one_iter()
    torch.cuda.synchronize()
    changed = 0
    for p, b, want in zip(trainer.fused.params, _momentum(trainer), loaded):
        held = trainer.optimizer.state[p]["momentum_buffer"]
        assert held.data_ptr() == b.data_ptr() and held.shape == p.shape
        changed += int(not torch.equal(held, want))
    assert changed > 0
    saved = trainer.optimizer.state_dict()["state"]
    assert all(torch.equal(saved[i]["momentum_buffer"], b) for i, b in enumerate(_momentum(trainer)))
    lr = trainer.lr_scheduler.update_lr(trainer.start_epoch * trainer.max_iter + 1)
    assert [g["lr"] for g in trainer.optimizer.param_groups] == [lr] * 3
    assert float(trainer.last[2]) == float(trainer.last[2]) and trainer.ema_model.updates == 3
    assert sorted(os.listdir(run["dir"])) == EXPECTED_FILES  # nothing written before an epoch end


def test_resume_start_epoch_override_and_missing_file(run, tmp_path):
    from trainer_lifecycle_common import make_args, make_config
    # -e 1 over <output_dir>/<name>/latest_ckpt.pth (start_epoch 2 in the file)
    trainer = _trainer(make_config(run["out"]), make_args(resume=True, start_epoch=1))
    trainer.before_train()
    assert trainer.start_epoch == 0 and trainer.ema_model.updates == 0 and not trainer.no_aug
    latest = _load(run["dir"] / "latest_ckpt.pth")
    for k, v in trainer.model.state_dict().items():
        assert torch.equal(v, latest["model"][k]), k
    missing = _trainer(make_config(tmp_path), make_args(resume=True))
    with pytest.raises(FileNotFoundError):
        missing.before_train()
    assert not os.path.exists(tmp_path / "yolox_s")


# ------------------------------------------------------------------ 4. fine-tune
def test_finetune_from_an_80_class_checkpoint(run, tmp_path):
    from trainer_lifecycle_common import make_args, make_config
    path = run["dir"] / "last_epoch_ckpt.pth"
    ckpt = _load(path)["model"]
    trainer = _trainer(make_config(tmp_path, val=False, num_classes=3), make_args(ckpt=str(path)))
    trainer.before_train()
    assert trainer.start_epoch == 0 and len(trainer.optimizer.state) == 0 and trainer.best_ap == 0
    assert trainer.ema_model.updates == 0
    got = trainer.model.state_dict()
    cls = {f"head.cls_preds.{i}.{n}" for i in range(3) for n in ("weight", "bias")}
    assert list(got) == list(ckpt)
    for k, v in got.items():
        if k in cls:
            assert v.shape[0] == 3 and ckpt[k].shape[0] == 80
        else:
            assert torch.equal(v, ckpt[k]), k
    for i in range(3):  # the config's initialisation: prior probability 1e-2
        assert torch.allclose(got[f"head.cls_preds.{i}.bias"], torch.full((3,), -4.59511985, device="cuda"))
    trainer.epoch, trainer.iter = 0, 0
    trainer.before_epoch()
    trainer.train_one_iter()
    loss = float(trainer.last[2])
    assert loss == loss and abs(loss) != float("inf")
    assert len(trainer.optimizer.state) == len(trainer.fused.params)


# ------------------------------------------------------------------ 5. evaluation
def test_evaluation_sees_the_live_ema_and_restores_modes(run):
    """The epoch-2 evaluation ran on the EMA the fused step had been updating in place since the
    epoch-1 evaluation folded it into inference plans; a model loaded from the file written right
    after must detect exactly the same."""
    from PIL import Image
    from trainer_lifecycle_common import VAL_IDS, make_config

    from yolox_amd.models import Yolox, YoloxModule
    trainer, evals = run["trainer"], run["evals"]
    assert len(evals) == 2 and all(m is trainer.ema_model.ema for m, _ in evals)
    (ap, ap50, summary), per_image = evals[1][1]
    assert sorted(per_image) == VAL_IDS and all(len(d["bboxes"]) > 0 for d in per_image.values())
    assert "Average forward time" in summary
    assert evals[0][1][1] != per_image  # the EMA moved between the two evaluations
    cfg = make_config(run["out"])
    model = YoloxModule.load_checkpoint(str(run["dir"] / "last_epoch_ckpt.pth"), cfg).to("cuda")
    ev = cfg.get_evaluator(batch_size=2, is_distributed=False)
    (ap2, ap50_2, _), per_image2 = cfg.eval(model, ev, False, return_outputs=True)
    assert per_image2 == per_image
    assert (ap2, ap50_2) == (ap, ap50)
    assert all(m.training is True for m in trainer.model.modules())
    assert all(m.training is False for m in trainer.ema_model.ema.modules())
    cfg = make_config(run["out"])
    yolox = Yolox.from_pretrained(str(run["dir"] / "last_epoch_ckpt.pth"), config=cfg, device="cuda")
    images = [Image.fromarray(a) for a in cfg.val.imgs]
    dets = yolox(images, threshold=0.0)
    assert len(dets) == len(images)


def test_evaluation_without_ema_restores_the_training_model(tmp_path):
    """EMA off: the training model itself is evaluated, in eval mode for the call only."""
    from trainer_lifecycle_common import make_args, make_config, spy_on_eval
    cfg = make_config(tmp_path, ema=False, max_epoch=1, no_aug_epochs=0, save_history_ckpt=False)
    evals = spy_on_eval(cfg)
    trainer = _trainer(cfg, make_args())
    trainer.train()
    assert len(evals) == 1 and evals[0][0] is trainer.model and trainer.ema_model is None
    assert all(m.training is True for m in trainer.model.modules())
    d = tmp_path / "yolox_s"
    # epoch + 1 == max_epoch - no_aug_epochs holds at the one epoch: last_mosaic_epoch is written too
    assert sorted(os.listdir(d)) == ["last_epoch_ckpt.pth", "last_mosaic_epoch_ckpt.pth", "latest_ckpt.pth"]
    last = _load(d / "last_epoch_ckpt.pth")
    for k, v in trainer.model.state_dict().items():
        assert torch.equal(last["model"][k], v), k


# ------------------------------------------------------------------ 6. two ranks
def test_two_ranks(tmp_path):
    """Two gloo ranks on the one GPU, batch 2 per rank (global batch 4 over a dataset of 8: two
    iterations per epoch), an output directory per rank."""
    from trainer_lifecycle_common import VAL_IDS
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", YOLOX_AMD_TRAIN_TUNE="0")
    procs = [subprocess.Popen(["timeout", "-k", "10", "240", sys.executable,
                               os.path.join(HERE, "trainer_lifecycle_worker.py"), "--rank", str(r), "--port",
                               str(port), "--out", str(tmp_path / f"r{r}")], env=env) for r in range(2)]
    try:
        rcs = [p.wait(timeout=300) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0, 0]
    res = [json.load(open(tmp_path / f"r{r}" / "result.json")) for r in range(2)]
    assert res[0]["files"] == EXPECTED_FILES and res[1]["files"] == []
    assert res[0]["image_ids"] == [VAL_IDS, VAL_IDS]  # both shards reached rank 0, at both epoch ends
    assert res[0]["scored"] == [True, True]
    assert all(r["training_flags"] for r in res)
    bn = [torch.load(tmp_path / f"r{r}" / "bn.pt", weights_only=True) for r in range(2)]
    assert list(bn[0]["after"]) == list(bn[1]["after"]) and len(bn[0]["after"]) > 100
    for k, v in bn[0]["after"].items():
        assert torch.equal(v, bn[1]["after"][k]), k
    # and they were rank-local before the epoch-end average (broadcast_buffers=False)
    assert any(not torch.equal(v, bn[1]["before"][k]) for k, v in bn[0]["before"].items())
