"""GIoU through the training path: yxh_yolox_loss_ex / yxh_yolox_loss_bwd_ex (csrc/simota.hip over
csrc/iou_loss.hpp) against the reference head with head.iou_loss = IouLoss("none", "giou")
(tests/golden/iou_loss.npz head.*, written by tests/golden/make_golden_iou.py on the batches of
tests/simota_cases.py), and one YoloxModule training step, eager and captured.

Every batch is the device decode of raw_of(case), as in tests/test_gpu_simota_edges.py, whose
helpers and bars this file reuses: rel=1e-4, abs=1e-6 on the losses (its :69) and rel(...) < 1e-5
on the fp32 gradient (its :158; the reference's own fp32-vs-fp64 noise on these gradients is
at most 1.3e-6, printed by the generator)."""
import pytest
import torch

import simota_cases as SC
from test_gpu_simota_edges import DT, GRAD_CASES, decode, raw_of, rel

pytestmark = pytest.mark.gpu

ALL = SC.case_names()
TYPE = {"iou": 0, "giou": 1}

_runs = {}


def device_run(name, use_l1, lt):
    """Decode, assign, reduce and differentiate the named batch with box loss ``lt`` (cached):
    (losses [6] float32, assignment on the CPU, {dtype: (g_ro, g_cls)} on the CPU)."""
    if (name, use_l1, lt) in _runs:
        return _runs[name, use_l1, lt]
    from yolox_amd import _native as N
    from yolox_amd.models.losses import yolox_losses
    c = SC.get_case(name)
    rawd = raw_of(c).cuda()
    B, A, D = rawd.shape
    nc = D - 5
    preds, lhw, strides = decode(rawd, c)
    labd = torch.from_numpy(c["labels"].copy()).cuda()
    losses, assign = yolox_losses(preds, labd, c["hw"], origin_reg=rawd[..., :4].contiguous() if use_l1 else None,
                                  iou_loss_type=lt)
    gt = torch.ones((), device="cuda")
    nfg = assign["num_fg"].int().contiguous()
    fgd = assign["fg_mask"].to(torch.uint8).contiguous()
    grads = {}
    for dtype, code in DT.items():
        g_ro = torch.full((B, A, 8), float("nan"), device="cuda", dtype=dtype)
        g_cls = torch.full((B, A, nc), float("nan"), device="cuda", dtype=dtype)
        N.check(N.lib().yxh_yolox_loss_bwd_ex(
            preds.data_ptr(), rawd.data_ptr(), labd.data_ptr(), B, A, nc, c["L"], lhw, strides, 3, fgd.data_ptr(),
            assign["matched_gt_inds"].data_ptr(), assign["pred_ious"].data_ptr(), nfg.data_ptr(), gt.data_ptr(),
            int(use_l1), code, g_ro.data_ptr(), g_cls.data_ptr(), torch.cuda.current_stream().cuda_stream, TYPE[lt]))
        grads[dtype] = (g_ro, g_cls)
    torch.cuda.synchronize()
    _runs[name, use_l1, lt] = (torch.stack([losses[k] for k in SC.LOSS_KEYS]).cpu(),
                               {k: v.cpu() for k, v in assign.items()},
                               {k: (a.cpu(), b.cpu()) for k, (a, b) in grads.items()})
    return _runs[name, use_l1, lt]


@pytest.mark.parametrize("use_l1", [False, True])
@pytest.mark.parametrize("name", ALL)
def test_giou_changes_only_the_box_term(golden, name, use_l1):
    """SimOTA is untouched (the assignment, pred_ious and with them the class targets use the plain
    IoU): everything but total_loss and iou_loss is bit-equal to the iou run; the six losses match
    the reference head with GIoU."""
    d = golden("iou_loss.npz")
    li, ai, _ = device_run(name, use_l1, "iou")
    lg, ag, _ = device_run(name, use_l1, "giou")
    for k in ("fg_mask", "matched_gt_inds", "pred_ious", "num_fg"):
        assert torch.equal(ai[k], ag[k]), k
    for k in ("conf_loss", "cls_loss", "l1_loss", "num_fg"):
        i = SC.LOSS_KEYS.index(k)
        assert li[i].item() == lg[i].item(), k
    ref = d[f"head.{name}.{'l1' if use_l1 else 'nol1'}.f32.losses"]
    for i, k in enumerate(SC.LOSS_KEYS):
        print(name, use_l1, k, lg[i].item(), float(ref[i]))
        assert lg[i].item() == pytest.approx(float(ref[i]), rel=1e-4, abs=1e-6), k
    if int(ag["num_fg"].sum()) > 0:
        assert lg[1].item() != li[1].item()  # the box term did change


@pytest.mark.parametrize("use_l1", [False, True])
@pytest.mark.parametrize("name", GRAD_CASES)
def test_giou_loss_bwd_matches_reference(golden, name, use_l1):
    d = golden("iou_loss.npz")
    _, _, gi = device_run(name, use_l1, "iou")
    _, _, gg = device_run(name, use_l1, "giou")
    g_ro, g_cls = gg[torch.float32]
    ref = torch.from_numpy(d[f"head.{name}.{'l1' if use_l1 else 'nol1'}.f32.g_raw5"])
    print(name, use_l1, rel(g_ro[..., :5], ref))
    assert rel(g_ro[..., :5], ref) < 1e-5
    assert float(g_ro[..., 5:].abs().max()) == 0.0
    assert torch.equal(g_cls, gi[torch.float32][1])
    assert torch.equal(g_ro[..., 4], gi[torch.float32][0][..., 4])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", ["rand_96x160_c3", "sat_96x160_c80"])
def test_giou_16bit_gradient_outputs_round_the_fp32_ones(name, dtype):
    for use_l1 in (False, True):
        _, _, grads = device_run(name, use_l1, "giou")
        for got, want in zip(grads[dtype], grads[torch.float32]):
            assert got.dtype == dtype
            assert torch.equal(got.view(torch.int16), want.to(dtype).view(torch.int16))


@pytest.mark.parametrize("name", ["rand_96x160_c3", "exact_hit"])
def test_ex_type_0_is_the_old_entry_point(name):
    """yxh_yolox_loss_ex / _bwd_ex with YXH_IOU_LOSS_IOU against yxh_yolox_loss / _bwd, bit for bit."""
    from yolox_amd import _native as N
    lib, st = N.lib(), torch.cuda.current_stream().cuda_stream
    c = SC.get_case(name)
    rawd = raw_of(c).cuda()
    B, A, D = rawd.shape
    nc, L = D - 5, c["L"]
    preds, lhw, strides = decode(rawd, c)
    labd = torch.from_numpy(c["labels"].copy()).cuda()
    origin = rawd[..., :4].contiguous()
    gt = torch.full((), 2.0, device="cuda")
    res = []
    for ex in (False, True):
        fg = torch.empty(B, A, dtype=torch.uint8, device="cuda")
        matched = torch.empty(B, A, dtype=torch.int32, device="cuda")
        piou = torch.empty(B, A, device="cuda")
        nfg = torch.empty(B, dtype=torch.int32, device="cuda")
        losses = torch.empty(6, device="cuda")
        ws = torch.empty(int(lib.yxh_yolox_loss_workspace_bytes(B, A, L)), dtype=torch.uint8, device="cuda")
        args = [preds.data_ptr(), origin.data_ptr(), labd.data_ptr(), B, A, nc, L, lhw, strides, 3, fg.data_ptr(),
                matched.data_ptr(), piou.data_ptr(), nfg.data_ptr(), losses.data_ptr(), ws.data_ptr(), ws.numel(), st]
        N.check(lib.yxh_yolox_loss_ex(*args, 0) if ex else lib.yxh_yolox_loss(*args))
        g_ro = torch.full((B, A, 8), float("nan"), device="cuda")
        g_cls = torch.full((B, A, nc), float("nan"), device="cuda")
        bargs = [preds.data_ptr(), rawd.data_ptr(), labd.data_ptr(), B, A, nc, L, lhw, strides, 3, fg.data_ptr(),
                 matched.data_ptr(), piou.data_ptr(), nfg.data_ptr(), gt.data_ptr(), 1, 0, g_ro.data_ptr(),
                 g_cls.data_ptr(), st]
        N.check(lib.yxh_yolox_loss_bwd_ex(*bargs, 0) if ex else lib.yxh_yolox_loss_bwd(*bargs))
        torch.cuda.synchronize()
        res.append([v.cpu() for v in (losses, fg, matched, piou, nfg, g_ro, g_cls)])
    for a, b in zip(*res):
        assert not torch.isnan(a.float()).any()
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="iou_loss_type"):
        N.check(lib.yxh_yolox_loss_ex(*args, 2))


def test_train_step_with_giou_eager_and_captured(monkeypatch):
    """One YoloxModule training step of yolox_s at 128 x 128, batch 2, with the reference's switch
    model.head.iou_loss = IouLoss("none", "giou"): out["iou_loss"] is 5 * sum / num_fg of the
    standalone module on the foreground rows (1e-6 relative: the step sums fp32 block trees of up
    to 256 values, the recomputation sums in fp64), the other loss terms are the iou step's bits,
    and a CapturedTrainStep replays the eager step bit for bit.  A head whose iou_loss is not an
    IouLoss with reduction "none" is refused."""
    import yolox_amd.train as T
    from test_gpu_train import _model_and_batch
    from yolox_amd.models import IouLoss
    monkeypatch.setenv("YOLOX_AMD_TRAIN_TUNE", "0")
    monkeypatch.setattr(T, "_TRAIN_TILES", {})
    m, _, x, labels, _ = _model_and_batch()
    m = m.cuda().train()
    xs, ls = x.cuda(), labels.cuda()
    ctx = lambda: torch.autocast("cuda", enabled=False)  # noqa: E731
    with ctx():
        base = {k: float(v.detach()) for k, v in m(xs, ls).items()}
    m.head.iou_loss = IouLoss(reduction="none", loss_type="giou")
    with ctx():
        out = m(xs, ls)
    out["total_loss"].backward()
    torch.cuda.synchronize()
    g = m._train_graph
    fg = g.assign["fg_mask"].bool()
    matched = g.assign["matched_gt_inds"].long()
    nfg = int(g.assign["num_fg"].sum())
    assert nfg > 0
    pred = g.outputs[..., :4][fg]
    tgt = torch.cat([ls[b].float()[matched[b][fg[b]]][:, 1:5] for b in range(xs.shape[0])])
    rows = IouLoss("none", "giou")(pred.contiguous(), tgt.contiguous())
    want = 5.0 * float(rows.double().sum()) / nfg
    assert float(out["iou_loss"]) == pytest.approx(want, rel=1e-6)
    for k in ("conf_loss", "cls_loss", "l1_loss", "num_fg"):
        assert float(out[k]) == base[k], k
    assert float(out["iou_loss"]) != base["iou_loss"]
    eager = {k: float(v.detach()) for k, v in out.items()}
    grads = {n: p.grad.clone() for n, p in m.named_parameters()}
    # the captured step keeps the type it captured
    m2, _, _, _, _ = _model_and_batch()
    m2 = m2.cuda().train()
    m2.head.iou_loss = IouLoss(reduction="none", loss_type="giou")
    with ctx():
        m2(xs, ls)["total_loss"].backward()  # eager warm-up (tiles, repack table); BN statistics move once
        cap = T.CapturedTrainStep(m2, xs, ls)
    # same weights, but m2's BN running statistics do not enter the train-mode forward: same step
    got = cap(xs, ls)
    torch.cuda.synchronize()
    for k in ("total_loss", "iou_loss", "conf_loss", "cls_loss", "l1_loss", "num_fg"):
        assert float(got[k]) == eager[k], k
    for n, p in m2.named_parameters():
        assert torch.equal(p.grad, grads[n]), n
    for bad in (IouLoss("sum", "giou"), torch.nn.L1Loss(reduction="none")):
        m.head.iou_loss = bad
        with pytest.raises(ValueError, match="iou_loss"):
            with ctx():
                m(xs, ls)
