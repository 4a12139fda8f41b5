"""The fused head launch (yxh_head_pred) and the serving score records for any class count
1-80 and every preset's head width (64 / 96 / 128 / 192 / 256 / 320).

T1 op level vs torch fp32; T2 the first 5 + C columns of a C-class launch equal an 80-class
launch's, bit for bit; T3 the score records at op level (incl. planted ties and a NaN class 0);
T4 plan level: column identity, the new widths against the two-conv plan, the serving path and
the training rows.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
FILL = -7.0


def N():
    from yolox_amd import _native
    return _native


class Level:
    """One head level's operands on the device and a yxh_head_desc over them.  The features are
    channel slices of one wider [B, h, w, 2 cin] buffer; the output has 28 rows before and 12
    after the level's."""

    def __init__(self, dtype, cin, h, w, C, seed, B=3):
        self.dtype, self.cin, self.h, self.w, self.C, self.B = dtype, cin, h, w, C, B
        self.a_off, self.A, self.stride = 28, 4 * 7 + h * w + 12, 16.0
        g = torch.Generator().manual_seed(seed)
        self.feats = torch.randn(B, h, w, 2 * cin, generator=g).to(dtype)
        self.w_ro = (torch.randn(5, cin, generator=g) / cin ** 0.5).to(dtype)
        self.w_cl = (torch.randn(C, cin, generator=g) / cin ** 0.5).to(dtype)
        self.b_ro, self.b_cl = torch.randn(5, generator=g) * 0.2, torch.randn(C, generator=g) * 0.2 - 2

    def run(self, mode, C=None, scores=False, v1=False, monkeypatch=None):
        """Launch with the first ``C`` class rows (default all); returns (rows, records | None) on the host."""
        n = N()
        C = self.C if C is None else C
        cin, h, w, B, A = self.cin, self.h, self.w, self.B, self.A
        fd = self.feats.to(DEV)
        wro, bro = self.w_ro.to(DEV), self.b_ro.to(DEV)
        wcl, bcl = self.w_cl[:C].contiguous().to(DEV), self.b_cl[:C].contiguous().to(DEV)
        outd = torch.full((B, A, 5 + C), FILL, device=DEV)
        rec = torch.full((B, A, 8), FILL, device=DEV) if scores else None
        d = n.HeadDesc()
        d.dtype, d.batch, d.h, d.w, d.cin, d.num_classes = n.DTYPE_CODE[self.dtype], B, h, w, cin, C
        esz = fd.element_size()
        for src, off in ((d.reg, 0), (d.cls, cin)):
            src.ptr = fd.data_ptr() + off * esz
            src.channels, src.cstride, src.bstride, src.h, src.w, src.upsample = cin, 2 * cin, h * w * 2 * cin, h, w, 0
        d.w_reg, d.b_reg, d.w_cls, d.b_cls = wro.data_ptr(), bro.data_ptr(), wcl.data_ptr(), bcl.data_ptr()
        d.out, d.out_bstride, d.a_off, d.stride, d.train = outd.data_ptr(), A * (5 + C), self.a_off, self.stride, mode
        if scores:
            d.scores = rec.data_ptr()
        if v1:
            monkeypatch.setenv("YXH_HEAD_V1", "1")
        try:
            n.check(n.lib().yxh_head_pred(ctypes.byref(d), n.stream_ptr()), "head_pred")
        finally:
            if v1:
                monkeypatch.delenv("YXH_HEAD_V1")
        torch.cuda.synchronize()
        return outd.cpu(), (rec.cpu() if scores else None)

    def want(self, mode, C=None):
        """torch fp32 on the same (rounded) operands."""
        C = self.C if C is None else C
        cin, h, w, B = self.cin, self.h, self.w, self.B
        reg, cls = self.feats[..., :cin], self.feats[..., cin:]
        ro = reg.float().reshape(B, h * w, cin) @ self.w_ro.float().T + self.b_ro
        cl = cls.float().reshape(B, h * w, cin) @ self.w_cl[:C].float().T + self.b_cl[:C]
        gy, gx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        want = torch.cat([ro, cl], -1)
        if mode != 2:
            want[..., 0] = (want[..., 0] + gx.reshape(-1)) * self.stride
            want[..., 1] = (want[..., 1] + gy.reshape(-1)) * self.stride
            want[..., 2:4] = torch.exp(want[..., 2:4]) * self.stride
        if mode != 1:
            want[..., 4:] = torch.sigmoid(want[..., 4:])
        return want


BF, HF = torch.bfloat16, torch.float16
# (C, cin, mode, dtype, (h, w)): every C meets >= 2 widths, every width >= 3 class counts and all three modes;
# 6 x 6 and 10 x 10 put 16-pixel groups across image boundaries at B = 3 (36 * 3 = 108: a partial last group)
T1_CASES = [
    (1, 64, 0, BF, (6, 6)), (17, 64, 1, HF, (10, 10)), (64, 64, 2, BF, (4, 8)),
    (3, 96, 0, HF, (10, 10)), (16, 96, 1, BF, (6, 6)), (20, 96, 2, HF, (4, 8)), (48, 96, 0, BF, (6, 6)),
    (1, 128, 1, HF, (4, 8)), (20, 128, 0, BF, (10, 10)), (48, 128, 2, HF, (6, 6)),
    (3, 192, 1, BF, (4, 8)), (17, 192, 0, BF, (6, 6)), (64, 192, 2, HF, (10, 10)),
    (16, 256, 0, HF, (10, 10)), (3, 256, 2, BF, (6, 6)), (64, 256, 1, BF, (4, 8)),
    (1, 320, 2, HF, (6, 6)), (17, 320, 0, BF, (10, 10)), (20, 320, 1, HF, (4, 8)), (48, 320, 0, HF, (6, 6)),
    (64, 320, 0, BF, (10, 10)),
]


@pytest.mark.parametrize("C,cin,mode,dtype,hw", T1_CASES)
def test_head_pred_classes_level(C, cin, mode, dtype, hw, monkeypatch):
    """T1: yxh_head_pred for C classes over cin channels vs torch fp32 on the same rounded operands
    (rtol = atol = 1e-4); rows outside [a_off, a_off + h*w) keep the fill value; for 64 / 128 / 256
    channels the tile kernel (YXH_HEAD_V1=1) gives the same bits."""
    lv = Level(dtype, cin, hw[0], hw[1], C, seed=cin + hw[0] + C)
    got, _ = lv.run(mode)
    a, n = lv.a_off, hw[0] * hw[1]
    torch.testing.assert_close(got[:, a:a + n], lv.want(mode), rtol=1e-4, atol=1e-4)
    assert (got[:, :a] == FILL).all() and (got[:, a + n:] == FILL).all()
    if cin in (64, 128, 256):
        got1, _ = lv.run(mode, v1=True, monkeypatch=monkeypatch)
        assert torch.equal(got1, got)


@pytest.mark.parametrize("cin", [96, 192, 320])
def test_head_pred_tile_kernel_refuses_new_widths(cin, monkeypatch):
    """The tile kernel needs a power-of-two row: the new widths are head_pred2 only."""
    lv = Level(BF, cin, 4, 8, 3, seed=cin)
    with pytest.raises(NotImplementedError, match="head_pred2 only"):
        lv.run(0, v1=True, monkeypatch=monkeypatch)


def test_head_pred_refuses_more_than_80_classes():
    lv = Level(BF, 64, 4, 8, 81, seed=1)
    with pytest.raises(NotImplementedError, match="1-80 classes"):
        lv.run(0)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cin", [64, 128, 256])
def test_head_pred_column_identity(cin, mode):
    """T2: a C-class launch's rows equal, bit for bit, columns [: 5 + C] of the 80-class launch whose
    w_cls / b_cls start with the same C rows (fragment f's MFMA order does not depend on the others)."""
    lv = Level(BF if mode == 0 else HF, cin, 10, 10, 80, seed=cin + mode)
    full, _ = lv.run(mode)
    for C in (1, 20, 64):
        got, _ = lv.run(mode, C=C)
        assert torch.equal(got, full[..., :5 + C]), C


def check_records(rows: np.ndarray, rec: np.ndarray):
    """Each record equals the filter's arithmetic on its own row: first maximum, its index, obj,
    obj * max in fp32, and the box."""
    cls = rows[..., 5:]
    best = cls.max(-1)
    np.testing.assert_array_equal(rec[..., 1], best)
    np.testing.assert_array_equal(rec[..., 2], cls.argmax(-1).astype(np.float32))
    np.testing.assert_array_equal(rec[..., 3], rows[..., 4])
    np.testing.assert_array_equal(rec[..., 0], (rows[..., 4] * best).astype(np.float32))
    np.testing.assert_array_equal(rec[..., 4:8], rows[..., :4])


@pytest.mark.parametrize("C,cin,dtype,hw", [(1, 96, BF, (6, 6)), (3, 320, HF, (10, 10)), (17, 128, BF, (6, 6)),
                                            (20, 192, HF, (4, 8)), (20, 64, BF, (10, 10))])
def test_head_pred_records_level(C, cin, dtype, hw):
    """T3: yxh_head_desc.scores at op level (mode 0): the rows are those of a launch without records,
    the level's records follow from their own rows, records outside the level are untouched."""
    lv = Level(dtype, cin, hw[0], hw[1], C, seed=3 * cin + C)
    plain, _ = lv.run(0)
    rows, rec = lv.run(0, scores=True)
    assert torch.equal(rows, plain)
    a, n = lv.a_off, hw[0] * hw[1]
    check_records(rows[:, a:a + n].numpy(), rec[:, a:a + n].numpy())
    assert (rec[:, :a] == FILL).all() and (rec[:, a + n:] == FILL).all()


def test_head_pred_records_ties_and_nan():
    """T3: equal class scores in different quarter-lanes (a lane holds classes 4 q .. 4 q + 3 of each
    16-class fragment): classes 2 / 9 (lanes 0 / 2) and 5 / 17 (lane 1 / lane 0's second fragment) get
    identical weight rows and biases, so the first index must win the merge; then class 0 is NaN
    (its bias), which starts the scan and is never replaced."""
    lv = Level(BF, 128, 6, 6, 20, seed=77)
    lv.w_cl[9], lv.b_cl[9] = lv.w_cl[2], lv.b_cl[2]
    lv.w_cl[17], lv.b_cl[17] = lv.w_cl[5], lv.b_cl[5]
    lv.b_cl[2] = lv.b_cl[9] = lv.b_cl[5] = lv.b_cl[17] = 6.0  # 8 sigma of a logit above the other classes' -2: these decide
    a, n = lv.a_off, 36
    rows, rec = lv.run(0, scores=True)
    r, s = rows[:, a:a + n].numpy(), rec[:, a:a + n].numpy()
    assert np.array_equal(r[..., 5 + 2], r[..., 5 + 9]) and np.array_equal(r[..., 5 + 5], r[..., 5 + 17])
    check_records(r, s)
    won = set(s[..., 2].reshape(-1).tolist())
    assert won <= {2.0, 5.0} and len(won) == 2, won  # every pixel's maximum is a tied pair: the lower index
    lv.b_cl[0] = float("nan")
    rows, rec = lv.run(0, scores=True)
    r, s = rows[:, a:a + n].numpy(), rec[:, a:a + n].numpy()
    assert np.isnan(r[..., 5]).all()
    check_records(r, s)
    assert (s[..., 2] == 0).all() and np.isnan(s[..., 1]).all() and np.isnan(s[..., 0]).all()


# ------------------------------------------------------------------ T4: plan level (192 x 192, batch 3)
SIZE, BATCH = 192, 3


def _images(seed=21):
    from yolox_amd.weights import synthetic_images
    return torch.from_numpy(synthetic_images(BATCH, SIZE, SIZE, seed=seed)).cuda()


def _plan(m, dtype, **kw):
    from yolox_amd.engine import Plan
    return Plan(m, BATCH, SIZE, SIZE, dtype, "cuda", N().NHWC, torch.uint8, **kw)


def _replay(p, x):
    p.static_input().copy_(x)
    rows = p.replay().clone()
    torch.cuda.synchronize()
    return rows


def _nheads(p):
    return [r.args["train"] for r in p.ctx.ops if r.kind == N().OP_HEAD]


def test_plan_column_identity_20_classes():
    """T4 (a): yolox_s bf16 with 20 classes whose cls_preds are the first 20 rows of the 80-class
    synthetic model's (everything else shared): the replayed rows equal [..., :25] of the 80-class
    plan's rows, bit for bit."""
    from yolox_amd.models import YoloxModule
    m80 = YoloxModule.synthetic("yolox_s", seed=0, device="cuda", dtype=BF)
    m20 = YoloxModule.synthetic("yolox_s", seed=0, device="cuda", dtype=BF, num_classes=20)
    sd80, sd20 = m80.state_dict(), m20.state_dict()
    assert sd80.keys() == sd20.keys()
    for k in sd80:
        assert torch.equal(sd20[k], sd80[k][:20] if "cls_preds" in k else sd80[k]), k
    x = _images()
    p80, p20 = _plan(m80, BF), _plan(m20, BF)
    assert len(_nheads(p80)) == 3 and len(_nheads(p20)) == 3
    r80, r20 = _replay(p80, x), _replay(p20, x)
    assert tuple(r20.shape) == (BATCH, 24 * 24 + 12 * 12 + 6 * 6, 25)
    assert torch.equal(r20, r80[..., :25])


@pytest.mark.parametrize("name,dtype,width", [("yolox_tiny", BF, 96), ("yolox_m", BF, 192), ("yolox_x", HF, 320)])
def test_plan_new_widths_vs_two_conv_plan(name, dtype, width):
    """T4 (b): 3-class models of the presets with head widths 96 / 192 / 320: three OP_HEAD launches
    (none with fuse_head_pred=False), rows within rtol = atol = 1e-4 of the two-conv plan's."""
    from yolox_amd.models import YoloxModule
    m = YoloxModule.synthetic(name, seed=0, device="cuda", dtype=dtype, num_classes=3)
    fused, split = _plan(m, dtype), _plan(m, dtype, fuse_head_pred=False)
    assert _nheads(fused) == [0, 0, 0] and _nheads(split) == []
    assert {r.args["cin"] for r in fused.ctx.ops if r.kind == N().OP_HEAD} == {width}
    x = _images()
    torch.testing.assert_close(_replay(fused, x), _replay(split, x), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("name,dtype,C", [("yolox_s", BF, 20), ("yolox_x", HF, 3)])
def test_plan_serving_records(oracle, name, dtype, C):
    """T4 (c): enable_scores() on a 20-class yolox_s and a 3-class yolox_x: a [3, A, 8] tensor, rows
    bit-identical to a plan without records, and postprocess_device(..., scores=) bit-identical to the
    row-reading filter and to the C oracle (one stream and split), with detections in every image at
    conf 0.01."""
    from yolox_amd.models import YoloxModule
    from yolox_amd.utils.boxes import postprocess_device
    m = YoloxModule.synthetic(name, seed=0, device="cuda", dtype=dtype, num_classes=C)
    x = _images()
    want_rows = _replay(_plan(m, dtype), x)
    p = _plan(m, dtype)
    scores = p.enable_scores()
    assert scores is not None and tuple(scores.shape) == (BATCH, p.anchors, 8)
    rows = _replay(p, x)
    assert torch.equal(rows, want_rows)
    h = rows.cpu().numpy()
    check_records(h, scores.cpu().numpy())
    side = torch.cuda.Stream()
    for conf in (0.01, 0.3):
        want = oracle.postprocess(h.copy(), C, conf, 0.65)
        if conf == 0.01:
            assert all(w is not None and len(w) > 0 for w in want), "no detections: the comparison shows nothing"
        pa, pb, pc = rows.clone(), rows.clone(), rows.clone()
        da, ca = postprocess_device(pa, C, conf, 0.65)
        db, cb = postprocess_device(pb, C, conf, 0.65, scores=scores)
        ev = torch.cuda.Event()
        dc, cc = postprocess_device(pc, C, conf, 0.65, scores=scores, filter_done=ev, rest_stream=side)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert torch.equal(pa, pb) and torch.equal(pa, pc)  # the in-place xyxy rows
        assert torch.equal(ca, cb) and torch.equal(ca, cc)
        n = ca.cpu().numpy()
        for b in range(BATCH):
            assert torch.equal(da[b, :n[b]], db[b, :n[b]]) and torch.equal(da[b, :n[b]], dc[b, :n[b]])
            if want[b] is None:
                assert n[b] == 0
            else:
                np.testing.assert_array_equal(db[b, :n[b]].cpu().numpy(), want[b])


def test_plan_training_rows_320():
    """T4 (d): train=True plans of a 3-class yolox_x fp16: three OP_HEAD launches in mode 1, rows within
    rtol = atol = 1e-4 of the two-conv plan's."""
    from yolox_amd.models import YoloxModule
    m = YoloxModule.synthetic("yolox_x", seed=0, device="cuda", dtype=HF, num_classes=3)
    fused, split = _plan(m, HF, train=True), _plan(m, HF, train=True, fuse_head_pred=False)
    assert _nheads(fused) == [1, 1, 1] and _nheads(split) == []
    x = _images()
    torch.testing.assert_close(_replay(fused, x), _replay(split, x), rtol=1e-4, atol=1e-4)
