"""YOLOX-Darknet53 on the host (no GPU): config, module tree, checkpoint layout, planner, and the
plain-torch restatement the GPU tests compare against."""
import json
import os

import numpy as np
import pytest
import torch

import darknet_torch as DT
from conftest import GOLDEN


def synthetic(eval_mode=True):
    from yolox_amd.config import named_config
    from yolox_amd.weights import synthetic_state_dict
    m = named_config("yolox_darknet").get_model()
    m.load_state_dict(synthetic_state_dict(m.state_dict(), seed=0, bn_stats="yolox_darknet"))
    return m.eval() if eval_mode else m


def test_state_dict_matches_reference_checkpoint_layout():
    from yolox_amd.config import named_config
    with open(os.path.join(GOLDEN, "state_dict_shapes_darknet.json")) as f:
        ref = [(k, tuple(s)) for k, s in json.load(f)["yolox_darknet"]]
    m = named_config("yolox_darknet").get_model()
    mine = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert dict(mine) == dict(ref) and len(mine) == len(ref) == 528
    backbone = lambda kv: [k for k, _ in kv if k.startswith("backbone.")]  # noqa: E731
    assert backbone(mine) == backbone(ref)  # the new modules' registration order too
    assert "backbone.backbone.stem.0.conv.weight" in dict(mine)
    assert dict(mine)["backbone.out1.0.conv.weight"] == (256, 768, 1, 1)
    assert dict(mine)["backbone.out2.0.conv.weight"] == (128, 384, 1, 1)


def test_named_config_and_dash_alias():
    from yolox_amd.config import YoloxConfig, YoloxDarknet, named_config
    from yolox_amd.models import YoloxProcessor
    a = YoloxConfig.get_named_config("yolox-darknet")
    assert a is YoloxConfig.get_named_config("yolox_darknet") and isinstance(a, YoloxDarknet)
    assert (a.depth, a.width, a.num_classes, a.test_size) == (1.0, 1.0, 80, (640, 640))
    c = named_config("yolox-darknet")
    assert isinstance(c, YoloxDarknet) and c is not a and c.name == "yolox_darknet"
    assert YoloxProcessor("yolox_darknet").config.test_size == (640, 640)


def test_get_model_topology_and_initialisation():
    from yolox_amd.config import named_config
    from yolox_amd.models import Darknet, ResLayer, YoloFpn, YoloxModule
    m = named_config("yolox_darknet").get_model()
    assert isinstance(m, YoloxModule) and isinstance(m.backbone, YoloFpn) and isinstance(m.backbone.backbone, Darknet)
    assert m.training
    bns = [x for x in m.modules() if isinstance(x, torch.nn.BatchNorm2d)]
    assert bns and all(b.eps == 1e-3 and b.momentum == 0.03 for b in bns)
    assert torch.allclose(m.head.cls_preds[0].bias, torch.full((80,), -4.59511985))
    assert sum(isinstance(x, ResLayer) for x in m.modules()) == 1 + 2 + 8 + 8 + 4
    assert all(isinstance(x, torch.nn.LeakyReLU) and x.negative_slope == 0.1
               for x in m.modules() if type(x).__name__ in ("SiLU", "ReLU", "LeakyReLU"))
    assert m.compute_dtype == torch.float32 and m.device.type == "cpu"
    assert m.to(torch.bfloat16).compute_dtype == torch.bfloat16
    # the PAFPN presets keep reading the Focus stem's conv
    s = named_config("yolox_nano").get_model()
    assert s.compute_dtype == s.backbone.backbone.stem.conv.conv.weight.dtype == torch.float32
    d21 = Darknet(21, out_features=("stem", "dark5"))
    assert [len(getattr(d21, k)) for k in ("stem", "dark2", "dark3", "dark4", "dark5")] == [3, 2, 3, 3, 7]


def test_synthetic_state_dict_round_trips():
    from yolox_amd.weights import load_bn_stats, synthetic_state_dict
    m = synthetic()
    sd = synthetic_state_dict(m.state_dict(), seed=0, bn_stats="yolox_darknet")
    stats = load_bn_stats("yolox_darknet")
    assert len(stats) == 170 and set(stats) <= set(sd)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    k = "backbone.backbone.dark5.7.conv2.bn.running_var"
    assert torch.equal(sd[k], stats[k]) and bool((stats[k] > 0).all())


def test_bn_stats_table_is_found_with_the_fixtures(tmp_path, monkeypatch):
    """The yolox_darknet table is reference-run data kept under tests/golden/; load_bn_stats looks in the
    package's data/, then YOLOX_AMD_BN_STATS_DIR, then there, and names the places when a table is missing."""
    import shutil
    from yolox_amd import weights as W
    assert W.bn_stats_dirs()[0] == W.DATA_DIR and os.path.samefile(W.bn_stats_dirs()[-1], GOLDEN)
    assert os.path.isfile(os.path.join(GOLDEN, "bn_stats_yolox_darknet.npz"))
    assert len(W.load_bn_stats("yolox_s")) > 0  # the presets' tables stay in the package
    shutil.copy(os.path.join(GOLDEN, "bn_stats_yolox_darknet.npz"), tmp_path / "bn_stats_elsewhere.npz")
    with pytest.raises(FileNotFoundError, match="YOLOX_AMD_BN_STATS_DIR"):
        W.load_bn_stats("elsewhere")
    monkeypatch.setenv("YOLOX_AMD_BN_STATS_DIR", str(tmp_path))
    assert len(W.load_bn_stats("elsewhere")) == 170


def test_train_mode_forward_is_refused_before_any_device_work():
    from yolox_amd.models import Darknet, ResLayer, YoloFpn
    m = synthetic(eval_mode=False)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="ResLayer|Darknet|YoloFpn"):
        m(x, torch.zeros(1, 4, 5))
    for block, inp, name in ((ResLayer(64), torch.zeros(1, 64, 8, 8), "ResLayer"), (Darknet(21), x, "Darknet"),
                             (YoloFpn(), x, "YoloFpn"), (m.backbone.backbone.dark3[1], torch.zeros(1, 256, 8, 8), "ResLayer")):
        assert block.training
        with pytest.raises(NotImplementedError, match=name):
            block(inp)
    # eval mode on the host: the usual refusal of a non-ROCm device, not the training one
    with pytest.raises(RuntimeError, match="ROCm device"):
        ResLayer(64).eval()(torch.zeros(1, 64, 8, 8))
    with pytest.raises(RuntimeError, match="ROCm device"):
        m.eval()(x)


def test_reference_layout_checkpoint_loads(tmp_path):
    from yolox_amd.config import named_config
    from yolox_amd.models import Yolox, YoloxModule
    from yolox_amd.weights import synthetic_state_dict
    with open(os.path.join(GOLDEN, "state_dict_shapes_darknet.json")) as f:
        shapes = {k: tuple(s) for k, s in json.load(f)["yolox_darknet"]}
    sd = synthetic_state_dict(shapes, seed=4)  # keys and shapes as the reference's module tree has them
    torch.save({"model": sd}, tmp_path / "yolox_darknet.pth")
    m = YoloxModule.load_checkpoint(str(tmp_path / "yolox_darknet.pth"), named_config("yolox_darknet"))
    assert not m.training
    for k in ("backbone.backbone.stem.0.conv.weight", "backbone.out2.4.bn.running_mean", "head.stems.2.conv.weight"):
        assert torch.equal(m.state_dict()[k], sd[k]), k
    with pytest.raises(ValueError, match="config must be provided"):
        Yolox.from_pretrained(str(tmp_path / "yolox_darknet.pth"))
    with pytest.raises(RuntimeError, match="ROCm device"):
        Yolox.from_pretrained(str(tmp_path / "yolox_darknet.pth"), config=named_config("yolox_darknet"), device="cpu")


def test_planner_topology_and_flops(monkeypatch):
    """One launch per BaseConv (no fusions), the stem as OP_STEM_RGB or, with the switch off, rgb_pack +
    conv; the two concats are two-source convs with the upsampled map first."""
    from yolox_amd import _native as N
    from yolox_amd import engine as E
    m = synthetic()

    def plan(dtype):
        ctx = E.PlanCtx(1, dtype, torch.device("cpu"))
        feats = m.backbone.plan(ctx, ctx.image(640, 640))
        m.head.plan(ctx, feats, E.OutBuffer(sum(f.lh * f.lw for f in feats), 85))
        return ctx, feats

    ctx, feats = plan(torch.bfloat16)
    assert [(f.ch, f.lh) for f in feats] == [(128, 80), (256, 40), (512, 20)]
    kinds = [o.kind for o in ctx.ops]
    n_base = sum(1 for x in m.modules() if type(x).__name__ == "BaseConv")
    assert ctx.ops[0].kind == N.OP_STEM_RGB and kinds.count(N.OP_STEM_RGB) == 1 and kinds.count(N.OP_SPP) == 1
    assert kinds.count(N.OP_HEAD) == 3
    # every BaseConv but the stem is one conv op, except the head's cls0 | reg0 pairs (stacked)
    assert kinds.count(N.OP_CONV) == n_base - 1 - 3
    two = [o for o in ctx.ops if o.kind == N.OP_CONV and len(o.args["srcs"]) == 2]
    assert [(o.args["cin"], [s.ch for s in o.args["srcs"]], [s.up for s in o.args["srcs"]]) for o in two] == [
        (768, [256, 512], [1, 0]), (384, [128, 256], [1, 0])]
    assert all(o.args["act"] == N.ACT_LRELU for o in ctx.ops if o.kind == N.OP_CONV and not o.args["dst_f32"])
    gflop = ctx.flops / 1e9
    assert 180 < gflop < 190, gflop  # 185.3 GFLOPs at 640 x 640 (the published model card's figure)
    fp32, _ = plan(torch.float32)  # float32 plans take the stem kernel too, and the two pred convs per level
    assert fp32.ops[0].kind == N.OP_STEM_RGB and N.OP_HEAD not in [o.kind for o in fp32.ops]
    monkeypatch.setattr(E, "_RGB_STEM", False)
    off, _ = plan(torch.bfloat16)
    assert [o.kind for o in off.ops[:2]] == [N.OP_RGB_PACK, N.OP_CONV]
    assert off.ops[1].args["cin"] == 16 and off.ops[1].args["spec"].cin_pad == 16 and off.ops[1].args["spec"].cin_g == 3
    assert off.flops == ctx.flops and len(off.ops) == len(ctx.ops) + 1
    fp32, _ = plan(torch.float32)
    assert [o.kind for o in fp32.ops[:2]] == [N.OP_RGB_PACK, N.OP_CONV]


def test_new_entry_points_refuse_bad_arguments_without_a_device():
    import ctypes
    from yolox_amd import _native as N
    lib = N.lib()
    assert ctypes.sizeof(N.Op) == lib.yxh_sizeof_op() and lib.yxh_abi_version() == 21
    assert (N.OP_STEM_RGB, N.OP_RGB_PACK) == (6, 7)
    assert lib.yxh_rgb_stem_conv(None, None) == N.EINVAL and b"null" in lib.yxh_last_error()
    assert lib.yxh_rgb_pack(None, N.NHWC, N.U8, 1, 4, 4, None, N.BF16, None) == N.EINVAL
    assert lib.yxh_rgb_stem_pack(None, None, None, None, None, 1e-3, 32, N.BF16, None, None, None) == N.EINVAL
    op = N.Op()
    op.kind = N.OP_STEM_RGB
    assert lib.yxh_run_ops(ctypes.byref(op), 1, None) == N.EINVAL and b"op 0" in lib.yxh_last_error()


def test_torch_restatement_reproduces_the_reference_fixture(golden):
    """The reference's own CPU forward (fixture) against the restatement on the package's module tree,
    float32 on the host.  Bars: the 1e-3 of tests/test_gpu_model.py tightened to CPU torch -- measured
    2.2e-7 (boxes, relative), 1.3e-5 (probabilities) and 3.3e-5 of a 4.4-4.8 range (FPN maps)."""
    d = golden("fwd_yolox_darknet_96x128.npz")
    m = synthetic()
    x = torch.from_numpy(d["input_u8"]).permute(0, 3, 1, 2).float()
    out, feats = DT.yolox(m, x)
    out, ref = out.numpy(), d["output"]
    assert out.shape == ref.shape == (2, 12 * 16 + 6 * 8 + 3 * 4, 85)
    assert np.abs(out[..., :4] - ref[..., :4]).max() / np.abs(ref[..., :4]).max() < 1e-5
    assert np.abs(out[..., 4:] - ref[..., 4:]).max() < 1e-4
    for i, f in enumerate(feats):
        r = d[f"fpn{i}"]
        assert f.shape == r.shape
        assert np.abs(f.numpy() - r).max() / np.abs(r).max() < 1e-4, i
