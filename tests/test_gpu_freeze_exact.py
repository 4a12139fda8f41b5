"""yxh_bn_frozen_stats and yxh_bn_frozen_act_bwd judged per element against float64 (tests/freeze_exact.py holds
the references and the derivation of every bound; tests/test_freeze_exact_checker.py pins them on the CPU).

Inputs are NaN-fenced views (a read outside the live view poisons the result) that must hold the same bits after the
launch (idle channels and padding rows of a sliced view untouched); dx is a canary-guarded dense buffer (a store
outside it, or an element left unwritten, is named).
"""
import ctypes as C

import pytest
import torch

import freeze_exact as fe
import train_exact as te
from test_gpu_ops import DEV, N
from test_gpu_train_exact import flat, ptr, src_of, stream

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("C_,has_gamma,has_beta", fe.STATS_CASES, ids=[f"C{c}-g{g}-b{b}" for c, g, b in fe.STATS_CASES])
def test_frozen_stats_exact(C_, has_gamma, has_beta):
    n, lib = N(), N().lib()
    o = fe.stats_operands(C_, has_gamma, has_beta)
    dev = {k: (flat(C_, value=v, fill="nan") if v is not None else None) for k, v in o.items()}
    before = {k: b.snapshot() for k, b in dev.items() if b is not None}
    stats = flat(4 * C_)
    n.check(lib.yxh_bn_frozen_stats(ptr(dev["gamma"]), ptr(dev["beta"]), ptr(dev["rmean"]), ptr(dev["rvar"]), te.EPS,
                                    C_, stats.data_ptr(), stream()))
    torch.cuda.synchronize()
    want, tol = fe.stats_reference(o)
    got = stats.slice.view(4, C_).cpu()
    label = f"frozen stats C={C_}"
    assert torch.equal(got[0], o["rmean"]), label + ": the mean row is not the running mean"
    worst = te.judge(got[1:], want[1:], tol[1:], [stats.outside("the stats table's buffer")],
                     label + " invstd / scale / shift")
    for k, b in before.items():  # the running statistics and the affine parameters are read only
        assert torch.equal(b, dev[k].snapshot()), f"{label}: {k} was written"
    print(f"\n{label}: worst error / bound {worst:.3f}")


PARAMS = [(dt, C_, view) for dt in te.ALL for C_ in fe.CHANNELS for view in fe.VIEW_NAMES]


@pytest.mark.parametrize("dt,C_,view", PARAMS, ids=[f"{dt}-C{c}-{v}" for dt, c, v in PARAMS])
def test_frozen_act_bwd_exact(dt, C_, view):
    n, lib = N(), N().lib()
    dtype, code = te.DTYPES[dt], N().DTYPE_CODE[te.DTYPES[dt]]
    off, idle, pad = te.VIEWS[view]
    worst = 0.0
    for case in (c for c in fe.cases(dt) if c.C == C_ and c.view == view):
        ops = fe.operands(case, dt)
        mk = lambda t, d: te.ViewBuf(case.B, case.H, case.W, C_, d, DEV, off, idle, pad, fill="nan").set(t)  # noqa: E731
        y, dout = mk(ops["y"], dtype), mk(ops["dout"], torch.float32)
        stats = flat(4 * C_, value=ops["stats"], fill="nan")
        before = [b.snapshot() for b in (y, dout, stats)]
        dx = flat(case.M * C_, dtype)
        ys, gs = src_of(y), src_of(dout)
        n.check(lib.yxh_bn_frozen_act_bwd(code, case.B, C.byref(ys), C.byref(gs), stats.data_ptr(), case.act,
                                          dx.data_ptr(), stream()))
        torch.cuda.synchronize()
        ref = fe.act_bwd_reference(ops["y"], ops["dout"], ops["stats"], case.act, dtype)
        label = f"frozen act bwd {case.id} {dt}"
        assert ref["ambiguous"] <= te.AMBIGUOUS_CAP, (label, ref["ambiguous"])
        worst = max(worst, te.judge(dx.slice.view(case.B, case.H, case.W, C_), ref["dx"], ref["tol"],
                                    [dx.outside("dx's buffer")], label, judged=ref["judged"]))
        for name, b, was in zip(("y", "dout", "stats"), (y, dout, stats), before):
            assert torch.equal(was, b.snapshot()), f"{label}: the {name} buffer (idle channels included) was written"
    print(f"\nfrozen act bwd {dt} C={C_} {view}: worst error / bound {worst:.3f}")
