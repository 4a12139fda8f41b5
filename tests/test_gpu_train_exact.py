"""The training step's non-MFMA kernels judged per element against float64 (tests/train_exact.py holds the
references, the derivation of every bound and the case tables; tests/test_train_exact_checker.py pins them on the
CPU): BatchNorm statistics / forward / backward and the channel sum (csrc/train_bn.hip), the depthwise gradients
(csrc/train_dw.hip), SPP and upsample backward (csrc/train_bwd.hip).

Every comparison is bit equality on grid operands, or a per-element bound with full-mantissa operands.  Inputs are
NaN-filled buffers around the live view (a read outside it poisons the result), outputs canary-filled ones (a
store outside the view, or an element left unwritten, is named), the reduction workspaces NaN between canary
guards.  Every launch runs twice into fresh outputs, which must agree bit for bit.
"""
import ctypes as C

import pytest
import torch

import grad_exact as ge
import train_exact as te
from test_gpu_ops import DEV, N

pytestmark = pytest.mark.gpu

F32 = torch.float32
_DEV = {}


def stream():
    return torch.cuda.current_stream().cuda_stream


def src_of(buf, channels=None):
    s = N().Src()
    s.ptr = buf.data_ptr()
    s.channels, s.cstride, s.bstride = channels or buf.ch, buf.cstride, buf.bstride
    s.h, s.w = buf.H, buf.W
    return s


def ptr(t):
    return None if t is None else t.data_ptr()


def flat(n, dtype=F32, value=None, fill="canary"):
    """n elements between guards: canary-filled output, or a NaN-fenced input holding `value`"""
    b = ge.Guarded((), n, dtype, DEV, fill=fill)
    return b if value is None else b.set(value.reshape(-1))


def same_bits(first, second, label):
    for name in first:
        a, b = first[name], second[name]
        if a is not None and not torch.equal(a.bits, b.bits):
            at = ge.first_index((a.bits != b.bits).cpu())[0] - ge.GUARD
            raise AssertionError(f"{label}: two runs differ in {name}, first at element {at}")


# ================================================================================================ BatchNorm
def bn_inputs(case, dt, mode):
    key = (case, dt, mode)
    if key not in _DEV:
        ops, dtype = te.bn_operands(case, dt, mode), te.DTYPES[dt]
        off, idle, pad = te.VIEWS[case.view]
        mk = lambda t, d: te.ViewBuf(case.B, case.H, case.W, case.C, d, DEV, off, idle, pad, fill="nan").set(t)  # noqa: E731
        _DEV.clear()  # one case's buffers at a time
        _DEV[key] = dict(y=mk(ops["y"], dtype), dout=mk(ops["dout"], F32),
                         res=mk(ops["res"], dtype) if case.res else None,
                         gamma=flat(case.C, value=ops["gamma"], fill="nan") if case.gamma else None,
                         beta=flat(case.C, value=ops["beta"], fill="nan") if case.beta else None)
    return _DEV[key]


def bn_pass(case, dt, mode):
    """statistics, forward, backward and channel sum of one case into fresh outputs -> the output buffers"""
    n, lib = N(), N().lib()
    dtype, code = te.DTYPES[dt], N().DTYPE_CODE[te.DTYPES[dt]]
    ops, d = te.bn_operands(case, dt, mode), bn_inputs(case, dt, mode)
    Cc, B, M = case.C, case.B, case.M
    off, idle, pad = te.VIEWS[case.view]
    ws = te.Workspace(int(lib.yxh_reduce_workspace_bytes(Cc)), DEV)
    o = dict(ws=ws, stats=flat(4 * Cc), rmean=None, rvar=None, dgamma=flat(Cc), dbeta=flat(Cc), dx=flat(M * Cc, dtype),
             sum=flat(Cc), out=te.ViewBuf(B, case.H, case.W, Cc, dtype, DEV, off, idle, pad))
    if case.running:
        o["rmean"], o["rvar"] = flat(Cc).set(ops["rmean"]), flat(Cc).set(ops["rvar"])
    ys = src_of(d["y"])
    n.check(lib.yxh_bn_stats(code, B, C.byref(ys), ptr(d["gamma"]), ptr(d["beta"]), ptr(o["rmean"]), ptr(o["rvar"]),
                             te.EPS, te.MOMENTUM, o["stats"].data_ptr(), ws.data_ptr(), ws.nbytes, stream()))
    act = case.act if mode == "full" else te.ACT_NONE
    rs, os_ = src_of(d["res"]) if case.res else None, src_of(o["out"])
    n.check(lib.yxh_bn_act_fwd(code, B, C.byref(ys), o["stats"].data_ptr(), act, C.byref(rs) if rs else None,
                               C.byref(os_), stream()))
    gs = src_of(d["dout"])
    n.check(lib.yxh_bn_act_bwd(code, B, C.byref(ys), C.byref(gs), o["stats"].data_ptr(), ptr(d["gamma"]), act,
                               o["dgamma"].data_ptr(), o["dbeta"].data_ptr(), o["dx"].data_ptr(), ws.data_ptr(),
                               ws.nbytes, stream()))
    n.check(lib.yxh_channel_sum(code, B, C.byref(ys), o["sum"].data_ptr(), ws.data_ptr(), ws.nbytes, stream()))
    torch.cuda.synchronize()
    return o


def bn_judge(case, dt, mode, o):
    dtype, Cc, M = te.DTYPES[dt], case.C, case.M
    ops = te.bn_operands(case, dt, mode)
    label = f"BatchNorm {case.id} {dt} {mode}"
    wsg = o["ws"].guards()
    fence = lambda k: [o[k].outside(f"{k}'s buffer"), wsg]  # noqa: E731
    full = mode == "full"
    chain = te.chain(M, Cc, dtype) if full else None
    ref = te.bn_stats_reference(ops["y"], ops["gamma"], ops["beta"], ops["rmean"], ops["rvar"])
    tol = te.bn_stats_tolerance(ref, chain)
    stats = o["stats"].slice.view(4, Cc).cpu()
    worst = {}
    worst["stats"] = te.judge(stats, ref["stats"], tol["stats"], fence("stats"), label + " mean / invstd / scale / shift")
    if case.running:
        for k in ("rmean", "rvar"):
            worst[k] = te.judge(o[k].slice, ref[k], tol[k], fence(k), f"{label} {k}")
    y_sum, tol_sum, _ = te.channel_sum_reference(ops["y"], chain if full else 0.0)
    if full:
        worst["sum"] = te.judge(o["sum"].slice, y_sum, tol_sum, fence("sum"), label + " channel_sum")
    else:
        # the preconditions: M squares (v - v0)**2 <= 16, M operands <= 2, M gradients <= 2, all multiples of 1 / 64
        te.grid_sum_exact(M, 16.0)
        te.assert_grid_exact(y_sum, M, max_product=2.0)
        te.judge_exact(stats[0], ref["mean"].to(F32).to(te.F64), label=label + " mean (one rounding of the exact mean)")
        te.judge_exact(o["sum"].slice, y_sum, fence("sum"), label + " channel_sum")
    act = case.act if full else te.ACT_NONE
    want, tol_out = te.bn_act_fwd_reference(ops["y"], stats, act, ops["res"], dtype)
    worst["out"] = te.judge(o["out"].get(), want, tol_out, [o["out"].outside("out's buffer")], label + " forward")
    b = te.bn_act_bwd_reference(ops["y"], ops["dout"], stats, ops["gamma"], act, dtype,
                                te.chain(M, Cc, dtype))
    assert b["ambiguous"] <= te.AMBIGUOUS_CAP, (label, b["ambiguous"])
    if full:
        worst["dbeta"] = te.judge(o["dbeta"].slice, b["dbeta"], b["tol_dbeta"], fence("dbeta"), label + " dbeta")
    else:
        te.assert_grid_exact(b["dbeta"], M, max_product=2.0)
        te.judge_exact(o["dbeta"].slice, b["dbeta"], fence("dbeta"), label + " dbeta (act 0)")
    worst["dgamma"] = te.judge(o["dgamma"].slice, b["dgamma"], b["tol_dgamma"], fence("dgamma"), label + " dgamma")
    worst["dx"] = te.judge(o["dx"].slice.view(case.B, case.H, case.W, Cc), b["dx"], b["tol_dx"], fence("dx"),
                           label + " dx", judged=b["judged"])
    if case.edge and full:
        want_is = 1 / (te.f32_value(te.EPS) ** 0.5)
        assert abs(float(stats[1, te.EDGE_CONST]) - want_is) <= float(tol["invstd"][te.EDGE_CONST]), stats[1]
        assert bool(torch.isfinite(o["dx"].slice.float()).all())
        assert abs(float(ref["mean"][te.EDGE_SHIFTED]) - 1000) < 0.01 and float(ref["var"][te.EDGE_SHIFTED]) < 2e-4
    return worst


BN_PARAMS = [(c, dt) for c in te.BN_CASES for dt in c.dts]


@pytest.mark.parametrize("case,dt", BN_PARAMS, ids=[f"{c.id}-{dt}" for c, dt in BN_PARAMS])
def test_batchnorm_kernels_exact(case, dt):
    if case in te.CAP_CASES:
        # red_blocks' arithmetic restated: the block cap binds and leaves more than 448 = 7 * 64 partials per
        # channel, so lanes of chan_finalize's eighth chain sum one and others meet its bb < nblk guard
        nch = case.C // te.EPC[te.DTYPES[dt]]
        assert nch >= 256 and (case.M + 7) // 8 > te.RED_CAP
        rpb = -(-case.M // te.RED_CAP)
        nblk = -(-case.M // rpb)
        assert (nblk, rpb) == te.red_plan(case.M, case.C, te.DTYPES[dt]) and 448 < nblk < 512, (nblk, rpb)
    for mode in ("grid", "full"):
        first, second = bn_pass(case, dt, mode), bn_pass(case, dt, mode)
        worst = bn_judge(case, dt, mode, first)
        same_bits({k: v for k, v in first.items() if k != "ws"}, second, f"BatchNorm {case.id} {dt} {mode}")
        ge.check_guards([second["ws"].guards()], "second run")
        print(f"\nBatchNorm {case.id} {dt} {mode}: worst error / bound "
              + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ================================================================================================ depthwise
def dw_run(case, dt, mode):
    n, lib = N(), N().lib()
    dtype, code = te.DTYPES[dt], N().DTYPE_CODE[te.DTYPES[dt]]
    ops = te.dw_operands(case, dt, mode)
    B, H, W, Cc, s, oh, ow = case.B, case.H, case.W, case.C, case.s, case.oh, case.ow
    dyw = case.dyw or (Cc + 7) // 8 * 8
    x = te.ViewBuf(B, H, W, Cc, dtype, DEV, off=16, idle=32, pad_rows=2, fill="nan").set(ops["x"])
    dy = te.ViewBuf(B, oh, ow, Cc, dtype, DEV, off=0, idle=dyw - Cc, pad_rows=1, fill="nan").set(ops["dy"])
    w = flat(9 * Cc, dtype, ops["w"], fill="nan")
    xs, dys = src_of(x), src_of(dy, dyw)
    runs = []
    for _ in range(2):
        o = dict(dw=flat(9 * Cc), dx=te.ViewBuf(B, H, W, Cc, F32, DEV, off=16, idle=32, pad_rows=3),
                 acc=te.ViewBuf(B, H, W, Cc, F32, DEV, off=16, idle=32, pad_rows=3).set(ops["base"]))
        ws = te.Workspace(int(lib.yxh_dw_wgrad_workspace_bytes(B, oh, ow, Cc, 3)), DEV)
        assert ws.nbytes == te.dw_nsplit(B, oh, ow) * Cc * 9 * 4
        if case.wgrad:
            n.check(lib.yxh_dw_wgrad(code, B, C.byref(xs), C.byref(dys), Cc, 3, s, 1, oh, ow, o["dw"].data_ptr(),
                                     ws.data_ptr(), ws.nbytes, stream()))
        for k, accumulate in (("dx", 0), ("acc", 1)):
            n.check(lib.yxh_dw_dgrad(code, B, C.byref(dys), w.data_ptr(), Cc, 3, s, 1, H, W, o[k].data_ptr(),
                                     o[k].cstride, o[k].bstride, accumulate, stream()))
        torch.cuda.synchronize()
        ge.check_guards([ws.guards()], f"depthwise {case.id}")
        if case.wgrad:  # every partial was written, and nothing else: a NaN left over would be one unused
            assert not bool(torch.isnan(ws.live).any()), "a partial of the workspace was never written"
        runs.append(o)
    label = f"depthwise {case.id} {dt} {mode}"
    a = runs[0]
    got_dw = a["dw"].slice.view(Cc, 3, 3)
    guards = {k: [a[k].outside(f"{k}'s buffer")] for k in a}
    if mode == "grid":
        if case.wgrad:
            te.judge_exact(got_dw, ops["dw"], guards["dw"], label + " dw")
        te.judge_exact(a["dx"].get(), ops["dx"], guards["dx"], label + " dx written")
        te.judge_exact(a["acc"].get(), ops["y_acc"], guards["acc"], label + " dx accumulated")
    else:
        if case.wgrad:
            te.judge(got_dw, ops["dw"], ge.tolerance(case.K, ops["Sw"]), guards["dw"], label + " dw")
        te.judge(a["dx"].get(), ops["dx"], ge.tolerance(9, ops["Sx"]), guards["dx"], label + " dx written")
        te.judge(a["acc"].get(), ops["y_acc"], ge.tolerance(9, ops["Sx"], ops["y_acc"], added=True), guards["acc"],
                 label + " dx accumulated")
    same_bits(runs[0], runs[1], label)


DW_PARAMS = [(c, dt) for c in te.DW_CASES for dt in c.dts]


@pytest.mark.parametrize("case,dt", DW_PARAMS, ids=[f"{c.id}-{dt}" for c, dt in DW_PARAMS])
def test_depthwise_gradients_exact(case, dt):
    dw_run(case, dt, "grid")
    if case.full:
        dw_run(case, dt, "full")


def test_depthwise_cases_split_as_stated():
    """dw_wgrad's 4096-pixel blocks restated: the cases reach two and three blocks, full and partial last ones"""
    split = {c[:5]: (te.dw_nsplit(c.B, c.oh, c.ow), c.K % te.DW_BLOCK) for c in te.DW_CASES}
    assert split[(2, 48, 48, 8, 1)] == (2, 512) and split[(2, 64, 64, 8, 1)] == (2, 0)
    assert split[(1, 96, 96, 16, 1)] == (3, 1024) and split[(2, 96, 96, 8, 2)] == (2, 512)


# ================================================================================================ SPP / upsample
SPP_PARAMS = [(c, dt) for c in te.SPP_CASES for dt in te.ALL]


@pytest.mark.parametrize("case,dt", SPP_PARAMS, ids=[f"{c.id}-{dt}" for c, dt in SPP_PARAMS])
def test_spp_bwd_exact(case, dt):
    n, lib = N(), N().lib()
    dtype = te.DTYPES[dt]
    B, H, W, c = case.B, case.H, case.W, case.c
    assert te.spp_cpb(H, W) == te.SPP_CPB.get((H, W), 4)
    ops = te.spp_operands(case, dt)
    # the cat view: x in channels [0, c); the pooled planes and the idle channels hold NaN (the backward pools again)
    cat = te.ViewBuf(B, H, W, c, dtype, DEV, off=0, idle=3 * c + case.idle, fill="nan").set(ops["x"])
    dcat = flat(B * H * W * 4 * c, value=ops["dcat"], fill="nan")
    cs = src_of(cat, 4 * c)
    runs = []
    for _ in range(2):
        dx = flat(B * H * W * c)
        n.check(lib.yxh_spp_bwd(n.DTYPE_CODE[dtype], B, C.byref(cs), c, dcat.data_ptr(), dx.data_ptr(), stream()))
        torch.cuda.synchronize()
        runs.append(dict(dx=dx))
    label = f"spp_bwd {case.id} {dt}"
    te.judge_exact(runs[0]["dx"].slice.view(B, H, W, c), ops["dx"], [runs[0]["dx"].outside("dx's buffer")], label)
    same_bits(runs[0], runs[1], label)


@pytest.mark.parametrize("B,h,w,Cc", te.UPSAMPLE_CASES)
def test_upsample_bwd_exact(B, h, w, Cc):
    n, lib = N(), N().lib()
    g = torch.Generator().manual_seed(h * w + Cc)
    up, prefill = te.grid((B, 2 * h, 2 * w, Cc), g), te.grid((B, h, w, Cc), g)
    want = te.upsample_bwd_reference(up, prefill)
    te.assert_grid_exact(want, 5, max_product=2.0)
    src = flat(up.numel(), value=up, fill="nan")
    runs = []
    for _ in range(2):
        dst = flat(prefill.numel()).set(prefill.reshape(-1))
        n.check(lib.yxh_upsample_bwd(src.data_ptr(), B, h, w, Cc, dst.data_ptr(), stream()))
        torch.cuda.synchronize()
        runs.append(dict(dst=dst))
    label = f"upsample_bwd {(B, h, w, Cc)}"
    te.judge_exact(runs[0]["dst"].slice.view(B, h, w, Cc), want, [runs[0]["dst"].outside("dst's buffer")], label)
    same_bits(runs[0], runs[1], label)
