"""SimOTA assignment, the losses and the loss gradient (csrc/simota.hip) at their edges, against
the reference's own results (tests/golden/simota_edges.npz: get_assignments / get_losses on the
batches of tests/simota_cases.py) and against autograd through the oracle's loss math.

What the batches reach that the 640 / 320 / 128 square, 80-class, random-box tests do not:
lh != lw in both orientations, 1 / 3 / 20 / 80 classes (the unroll-by-8 loop and its tail),
dynamic_k up to 9 and many anchors claimed by several ground truths (tight, sat), sigmoids of
exactly 0 and 1 and the -100 logarithm clamp (sat), duplicated label rows, a ground truth without
an anchor in its own radius, fewer than 10 candidates, L == G, L == 1, images and a whole batch
without labels, predicted edges that equal ground-truth edges (the half-gradient tie), and the
bf16 / f16 gradient outputs.

An image whose assignment the oracle finds decided by rounding (oracle.simota_margins; stored per
image in the fixture, capped by tests/test_oracle.py) is not held to the exact assignment.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import simota_cases as SC

pytestmark = pytest.mark.gpu

ALL = SC.case_names()
GRAD_CASES = ["rand_96x160_c3", "tight_160x96_c20", "sat_96x160_c80", "exact_hit", "all_empty"]
DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}

_runs = {}


def run(name, tag):
    """yolox_losses on the named batch (cached): (losses as floats, assignment on the CPU)."""
    if (name, tag) not in _runs:
        from yolox_amd.models.losses import yolox_losses
        c = SC.get_case(name)
        origin = torch.from_numpy(c["origin"].copy()).cuda() if tag == "l1" else None
        losses, assign = yolox_losses(torch.from_numpy(c["outputs"].copy()).cuda(),
                                      torch.from_numpy(c["labels"].copy()).cuda(), c["hw"], origin_reg=origin)
        torch.cuda.synchronize()
        _runs[name, tag] = ({k: v.item() for k, v in losses.items()}, {k: v.cpu() for k, v in assign.items()})
    return _runs[name, tag]


@pytest.mark.parametrize("name", ALL)
def test_assignment_matches_reference(golden, name):
    from test_gpu_simota import check_image
    d = golden("simota_edges.npz")
    c = SC.get_case(name)
    _, assign = run(name, "l1")
    for b in range(c["labels"].shape[0]):
        if SC.num_gt(c["labels"][b]) == 0:
            assert int(assign["num_fg"][b]) == 0 and not assign["fg_mask"][b].any()
        elif not d[f"{name}.rounding"][b]:
            check_image(assign, b, d[f"{name}.img{b}.fg_mask"], d[f"{name}.img{b}.matched_gt_inds"],
                        d[f"{name}.img{b}.pred_ious"], d[f"{name}.img{b}.num_fg"])


@pytest.mark.parametrize("tag", ["nol1", "l1"])
@pytest.mark.parametrize("name", ALL)
def test_losses_match_reference(golden, name, tag):
    d = golden("simota_edges.npz")
    if d[f"{name}.rounding"].any():
        pytest.skip("batch holds a rounding-decided image (capped by test_oracle.py)")
    losses, _ = run(name, tag)
    for k, ref in zip(SC.LOSS_KEYS, d[f"{name}.{tag}.losses"]):
        print(name, tag, k, losses[k], float(ref))
        assert losses[k] == pytest.approx(float(ref), rel=1e-4, abs=1e-6), k
    if name == "all_empty":
        assert losses["iou_loss"] == 0.0 and losses["cls_loss"] == 0.0 and losses["l1_loss"] == 0.0
        assert losses["num_fg"] == 1.0


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def raw_of(c):
    """Pre-decode head outputs [B, A, 5+C] whose decode gives the batch's boxes (to rounding)."""
    if c["raw"] is not None:
        return torch.from_numpy(c["raw"].copy())
    xs, ys, st = (torch.from_numpy(a.copy()) for a in SC.anchors(c["H"], c["W"]))
    raw = torch.from_numpy(c["outputs"].copy())
    raw[..., 0] = raw[..., 0] / st - xs
    raw[..., 1] = raw[..., 1] / st - ys
    raw[..., 2:4] = torch.log(raw[..., 2:4] / st[:, None])
    return raw


def decode(rawd, c):
    from yolox_amd import _native as N
    B, A, D = rawd.shape
    lhw = (C.c_int32 * 6)(*[v for t in c["hw"] for v in t])
    strides = (C.c_int32 * 3)(*SC.STRIDES)
    preds = torch.empty_like(rawd)
    N.check(N.lib().yxh_head_decode_train(rawd.data_ptr(), B, A, D - 5, lhw, strides, 3, preds.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream))
    return preds, lhw, strides


_grads = {}


def device_grads(name, use_l1):
    """Decode, assign and differentiate the named batch on the device (cached): raw (CPU), the
    losses, the assignment and {dtype: (g_ro, g_cls)} for fp32 / bf16 / f16 gradient outputs."""
    if (name, use_l1) in _grads:
        return _grads[name, use_l1]
    from yolox_amd import _native as N
    from yolox_amd.models.losses import yolox_losses
    c = SC.get_case(name)
    raw = raw_of(c)
    B, A, D = raw.shape
    nc = D - 5
    rawd = raw.cuda()
    preds, lhw, strides = decode(rawd, c)
    labd = torch.from_numpy(c["labels"].copy()).cuda()
    losses, assign = yolox_losses(preds, labd, c["hw"], origin_reg=rawd[..., :4].contiguous() if use_l1 else None)
    gt = torch.full((), 2.0, device="cuda")
    nfg = assign["num_fg"].int().contiguous()
    fgd = assign["fg_mask"].to(torch.uint8).contiguous()
    out = {}
    for dtype, code in DT.items():
        g_ro = torch.full((B, A, 8), float("nan"), device="cuda", dtype=dtype)
        g_cls = torch.full((B, A, nc), float("nan"), device="cuda", dtype=dtype)
        N.check(N.lib().yxh_yolox_loss_bwd(
            preds.data_ptr(), rawd.data_ptr(), labd.data_ptr(), B, A, nc, c["L"], lhw, strides, 3, fgd.data_ptr(),
            assign["matched_gt_inds"].data_ptr(), assign["pred_ious"].data_ptr(), nfg.data_ptr(), gt.data_ptr(),
            int(use_l1), code, g_ro.data_ptr(), g_cls.data_ptr(), torch.cuda.current_stream().cuda_stream))
        out[dtype] = (g_ro, g_cls)
    torch.cuda.synchronize()
    _grads[name, use_l1] = (raw, {k: v.item() for k, v in losses.items()},
                            {k: v.cpu() for k, v in assign.items()},
                            {k: (a.cpu(), b.cpu()) for k, (a, b) in out.items()})
    return _grads[name, use_l1]


@pytest.mark.parametrize("use_l1", [False, True])
@pytest.mark.parametrize("name", GRAD_CASES)
def test_loss_bwd_matches_autograd(oracle, name, use_l1):
    """d (2 * total_loss) / d raw head outputs vs autograd through the oracle's loss math with the
    device's assignment as fixed targets, fp32 outputs (tests/test_gpu_train.py's check, same
    bound) on a non-square batch per generator, the exact-hit batch and the batch without labels."""
    c = SC.get_case(name)
    raw, losses, assign, grads = device_grads(name, use_l1)
    g_ro, g_cls = grads[torch.float32]
    if name == "exact_hit":
        hit = list(c["hit"])
        assert assign["fg_mask"][0, hit].all()
        np.testing.assert_array_equal(assign["pred_ious"][0, hit].numpy(), np.ones(3, np.float32))
    xs, ys, st = (torch.from_numpy(a.copy()) for a in SC.anchors(c["H"], c["W"]))
    ref, ref_total = SC.loss_bwd_reference(oracle, raw, torch.from_numpy(c["labels"].copy()), xs, ys, st, assign,
                                           use_l1, 2.0)
    print(name, use_l1, rel(g_ro[..., :5], ref[..., :5]), rel(g_cls, ref[..., 5:]))
    assert losses["total_loss"] == pytest.approx(ref_total, rel=1e-5)
    assert rel(g_ro[..., :5], ref[..., :5]) < 1e-5
    assert float(g_ro[..., 5:].abs().max()) == 0.0
    assert rel(g_cls, ref[..., 5:]) < 1e-5


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("use_l1", [False, True])
@pytest.mark.parametrize("name", ["rand_96x160_c3", "sat_96x160_c80"])
def test_loss_bwd_16bit_outputs_round_the_fp32_ones(name, use_l1, dtype):
    """The bf16 / f16 instantiations (the 16-bit training step's) store the same fp32 value rounded
    once to nearest even: bit-equal to the fp32 outputs cast with .to(dtype)."""
    _, _, _, grads = device_grads(name, use_l1)
    for got, want in zip(grads[dtype], grads[torch.float32]):
        assert got.dtype == dtype
        assert torch.equal(got.view(torch.int16), want.to(dtype).view(torch.int16))


@pytest.mark.parametrize("H,W,nc", [(96, 160, 3), (160, 96, 20)])
def test_head_decode_train_non_square(H, W, nc):
    """yxh_head_decode_train vs the oracle's decode ((o + grid) * s, exp(o) * s): xy bit-exact
    (one fp32 add and multiply), wh to 1e-6 relative (expf), logits untouched."""
    xs, ys, st = (torch.from_numpy(a.copy()) for a in SC.anchors(H, W))
    g = torch.Generator().manual_seed(H + nc)
    raw = torch.randn(2, xs.shape[0], 5 + nc, generator=g)
    preds, _, _ = decode(raw.cuda(), {"hw": SC.level_hw(H, W)})
    torch.cuda.synchronize()
    preds = preds.cpu()
    assert torch.equal(preds[..., :2], (raw[..., :2] + torch.stack([xs, ys], 1)) * st[:, None])
    np.testing.assert_allclose(preds[..., 2:4].numpy(), (torch.exp(raw[..., 2:4]) * st[:, None]).numpy(),
                               rtol=1e-6, atol=0)
    assert torch.equal(preds[..., 4:], raw[..., 4:])
