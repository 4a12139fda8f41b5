"""YOLOX-Darknet53 on the device: the HIP plan against the reference's fixture (float32), against
itself across compute dtypes, stem paths, input formats and execution forms, the new blocks'
standalone forwards against the plain-torch restatement (tests/darknet_torch.py, on the host), and the
serving API.  Shapes: batch 2 at 96 x 128 (the fixture) and 64 x 64."""
import os

import numpy as np
import pytest
import torch

import darknet_torch as DT
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURE = "fwd_yolox_darknet_96x128.npz"
FILES = [os.path.join(GOLDEN, "images", f"{n}.jpg") for n in ("000000000001", "000000000009")]
SIZE = (96, 128)


@pytest.fixture(scope="module")
def models():
    from yolox_amd.models import YoloxModule
    cache = {}

    def get(dtype):
        if dtype not in cache:
            cache[dtype] = YoloxModule.synthetic("yolox_darknet", seed=0, device="cuda", dtype=dtype)
        return cache[dtype]

    return get


@pytest.fixture(scope="module")
def host_model():
    from yolox_amd.config import named_config
    from yolox_amd.weights import synthetic_state_dict
    m = named_config("yolox_darknet").get_model()
    m.load_state_dict(synthetic_state_dict(m.state_dict(), seed=0, bn_stats="yolox_darknet"))
    return m.eval()


@pytest.fixture(scope="module")
def fixture_u8():
    with np.load(os.path.join(GOLDEN, FIXTURE)) as z:
        return torch.from_numpy(np.array(z["input_u8"]))


@pytest.fixture(scope="module")
def fp32_out(models, fixture_u8):
    """The float32 device output of the fixture's input (computed once, never modified)."""
    return models(torch.float32)(fixture_u8.permute(0, 3, 1, 2).float()).clone()


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-6))


def test_fp32_forward_matches_reference_fixture(golden, models, fp32_out, fixture_u8):
    """Decoded rows and the three FPN maps against the reference's own CPU forward, at the float32 bars
    of tests/test_gpu_model.py (1e-3 of the box range, 1e-3 on probabilities; 1e-3 of each map's range)."""
    d = golden(FIXTURE)
    out, ref = fp32_out.cpu().numpy(), d["output"]
    assert out.shape == ref.shape
    feats = models(torch.float32).backbone(fixture_u8.permute(0, 3, 1, 2).float().cuda())
    errs = [rel(f.cpu().numpy(), d[f"fpn{i}"]) for i, f in enumerate(feats)]
    print(f"box rel {rel(out[..., :4], ref[..., :4]):.3g} prob abs {np.abs(out[..., 4:] - ref[..., 4:]).max():.3g} "
          f"fpn rel {errs}")
    assert rel(out[..., :4], ref[..., :4]) < 1e-3
    assert np.abs(out[..., 4:] - ref[..., 4:]).max() < 1e-3
    for i, f in enumerate(feats):
        assert tuple(f.shape) == d[f"fpn{i}"].shape and errs[i] < 1e-3, (i, errs)


# twice the distance between the restatement with 16-bit storage (folded weights and every activation map
# rounded, tests/darknet_torch.py) and the float32 restatement, measured once on the host on the
# fixture's input: bf16 p_max 0.0917, p99 0.0359, box p99 0.00763, xy 0.0981; fp16 p_max 0.00951,
# p99 0.00437, box p99 0.000842, xy 0.0144
LOW_PRECISION_BARS = {torch.bfloat16: dict(p_max=0.184, p_p99=0.072, box_p99=0.0153, xy_max=0.196),
                      torch.float16: dict(p_max=0.0190, p_p99=0.0088, box_p99=0.00168, xy_max=0.0288)}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_low_precision_forward_against_fp32(models, fp32_out, fixture_u8, dtype):
    out = models(dtype)(fixture_u8.permute(0, 3, 1, 2).float())
    got = DT.metrics(out, fp32_out)
    print(dtype, got)
    assert torch.isfinite(out).all()
    for k, bar in LOW_PRECISION_BARS[dtype].items():
        assert got[k] < bar, (k, got)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_stem_kernel_plan_matches_pack_plan(models, fixture_u8, dtype):
    """yxh_rgb_stem_conv (default) against yxh_rgb_pack + the generic conv: the same 27 products per output
    in another summation order, so float32 differs by accumulation rounding only (1e-4 on probabilities, the
    bar of the Focus stem's analogous test) and a 16-bit plan by what one flipped rounding of a stem output
    can do downstream: the low-precision bars."""
    from yolox_amd import _native as N
    from yolox_amd.engine import Plan
    m = models(dtype)
    x = fixture_u8.cuda()
    fused = Plan(m, 2, *SIZE, dtype, "cuda", N.NHWC, torch.uint8)
    split = Plan(m, 2, *SIZE, dtype, "cuda", N.NHWC, torch.uint8, fuse_stem=False)
    assert [o.kind for o in fused.ctx.ops[:1]] == [N.OP_STEM_RGB]
    assert [o.kind for o in split.ctx.ops[:2]] == [N.OP_RGB_PACK, N.OP_CONV]
    a, b = fused.run(x).clone(), split.run(x).clone()
    got = DT.metrics(a, b)
    print(dtype, got)
    if dtype == torch.float32:
        assert got["p_max"] < 1e-4 and got["box_p99"] < 1e-4
    else:
        for k, bar in LOW_PRECISION_BARS[dtype].items():
            assert got[k] < bar, (k, got)


def test_switch_off_plans_the_pack_path(models, monkeypatch):
    from yolox_amd import _native as N
    from yolox_amd import engine as E
    monkeypatch.setattr(E, "_RGB_STEM", False)
    plan = E.Plan(models(torch.bfloat16), 1, 64, 64, torch.bfloat16, "cuda", N.NHWC, torch.uint8)
    assert [o.kind for o in plan.ctx.ops[:2]] == [N.OP_RGB_PACK, N.OP_CONV]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_nhwc_uint8_input_and_graph_replay(models, fixture_u8, dtype):
    """uint8 NHWC through forward_nhwc equals the float32 NCHW call (the same pixel values), and the
    captured graph's replay equals the eager run, bit for bit."""
    from yolox_amd import _native as N
    m = models(dtype)
    ref = m(fixture_u8.permute(0, 3, 1, 2).float())
    assert torch.equal(m.forward_nhwc(fixture_u8.cuda()), ref)
    plan = m.plan_for(2, *SIZE, N.NHWC, torch.uint8)
    eager = plan.run(fixture_u8.cuda()).clone()
    plan.static_input().copy_(fixture_u8)
    g1 = plan.replay().clone()
    g2 = plan.replay().clone()
    torch.cuda.synchronize()
    assert torch.equal(eager, ref) and torch.equal(g1, eager) and torch.equal(g2, eager)


def test_standalone_blocks_match_restatement(models, host_model):
    """ResLayer(x), Darknet(images) (all five features, 64 x 64) and YoloFpn(images) (96 x 128) in float32
    against the restatement on the host: 1e-3 of each map's range, the float32 bar of the model test."""
    from yolox_amd.models import Darknet
    from yolox_amd.weights import synthetic_images
    m = models(torch.float32)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 128, 9, 13, generator=g)
    res_dev, res_host = m.backbone.backbone.dark2[1], host_model.backbone.backbone.dark2[1]
    with torch.no_grad():
        assert rel(res_dev(x.cuda()).cpu(), DT.res_layer(res_host, x)) < 1e-3
    img = torch.from_numpy(synthetic_images(2, 64, 64, seed=5)).permute(0, 3, 1, 2).float()
    dark = Darknet(53, out_features=Darknet.FEATURES)
    dark.load_state_dict(host_model.backbone.backbone.state_dict())
    for b in dark.modules():
        if isinstance(b, torch.nn.BatchNorm2d):
            b.eps = 1e-3
    with torch.no_grad():
        want = DT.darknet(dark.eval(), img)
        got = dark.cuda()(img.cuda())
    assert list(got) == list(want) == ["stem", "dark2", "dark3", "dark4", "dark5"]
    for k in want:
        assert tuple(got[k].shape) == tuple(want[k].shape)
        assert rel(got[k].cpu(), want[k]) < 1e-3, k
    assert list(m.backbone.backbone(img.cuda())) == ["dark3", "dark4", "dark5"]
    img = torch.from_numpy(synthetic_images(2, *SIZE, seed=6)).permute(0, 3, 1, 2).float()
    with torch.no_grad():
        want = DT.yolo_fpn(host_model.backbone, img)
    got = m.backbone(img.cuda())
    assert len(got) == 3
    for i, (a, b) in enumerate(zip(got, want)):
        assert tuple(a.shape) == tuple(b.shape) and rel(a.cpu(), b) < 1e-3, i


def make_api(module):
    from yolox_amd.config import named_config
    from yolox_amd.models import Yolox, YoloxProcessor
    cfg = named_config("yolox_darknet")
    cfg.test_size = SIZE
    return Yolox(module, YoloxProcessor(cfg))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_stream_equals_call_on_image_files(models, dtype):
    yolox = make_api(models(dtype))
    want = yolox(FILES, threshold=0.01)
    assert len(want) == 2 and any(len(d["labels"]) for d in want)
    assert list(yolox.stream(FILES, threshold=0.01, batch_size=2)) == want
    assert yolox.detect(FILES, threshold=0.01, batch_size=2) == want
    assert (yolox.pipeline(2).scores is not None) == (dtype == torch.bfloat16)


def test_pipeline_with_score_records_equals_one_without(models, monkeypatch):
    from yolox_amd.engine import Plan
    from yolox_amd.serve import Pipeline
    yolox = make_api(models(torch.bfloat16))
    with_records = Pipeline(yolox.module, yolox.processor, 2)
    monkeypatch.setattr(Plan, "enable_scores", lambda self: None)
    without = Pipeline(yolox.module, yolox.processor, 2)
    assert with_records.scores is not None and without.scores is None
    a = list(with_records.run(FILES, 0.01))
    b = list(without.run(FILES, 0.01))
    assert a == b and any(len(d["labels"]) for d in a)
