"""The judge of the BatchNorm, depthwise and SPP / upsample gradient kernels (tests/train_exact.py) pinned on the CPU,
as test_grad_exact_checker.py pins the conv one -- so a pass on the device means what it says:

  references      each vectorised float64 reference against a plain-loop version (and torch's float64 autograd) at
                  tiny shapes; the SPP scan against F.max_pool2d's autograd on tie-free planes
  preconditions   of every case of the GPU lists: grid exactness, the 0.1 % cap on ReLU / LeakyReLU elements
                  without a defined side, the launch arithmetic the cases were chosen for
  bounds          an fp32 emulation of each kernel's formula (rows over lanes and blocks as red_plan says, blocks
                  and chan_finalize in double) stays inside its bound, for every case
  planted faults  a dropped row lane, sum 1 and sum 2 swapped, the biased variance in the running statistic, a
                  partial block left out, the last maximum on a tie, a tap's sign flipped, a store one chunk past
                  a slice, an element left unwritten: each is rejected
"""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

import grad_exact as ge
import train_exact as te

F32, F64 = torch.float32, torch.float64
BN_PARAMS = [(c, dt) for c in te.BN_CASES for dt in c.dts]
BN_IDS = [f"{c.id}-{dt}" for c, dt in BN_PARAMS]


def raises(err, fn, *a, **k):
    try:
        fn(*a, **k)
    except err:
        return True
    return False


# ------------------------------------------------------------------------------------------ references against loops
def _act_py(z, act):
    return {0: z, 1: z / (1 + math.exp(-z)), 2: max(z, 0.0), 3: z if z > 0 else te.LRELU_SLOPE * z}[act]


@pytest.mark.parametrize("B,H,W,act", [(2, 2, 3, 1), (1, 1, 1, 3), (1, 3, 1, 2), (2, 1, 2, 0)])
def test_batchnorm_references_against_loops_and_autograd(B, H, W, act):
    g = torch.Generator().manual_seed(H * 7 + W + act)
    Cc, M = 3, B * H * W
    y = torch.randn(B, H, W, Cc, generator=g) * 2 + 1
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g)
    rm, rv = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    res, dout = torch.randn(B, H, W, Cc, generator=g), torch.randn(B, H, W, Cc, generator=g)
    r = te.bn_stats_reference(y, gamma, beta, rm, rv)
    eps, mo = te.f32_value(te.EPS), te.f32_value(te.MOMENTUM)
    rows = y.double().reshape(M, Cc).tolist()
    for c in range(Cc):
        col = [row[c] for row in rows]
        mean = sum(col) / M
        var = sum((v - mean) ** 2 for v in col) / M
        unb = var * M / (M - 1) if M > 1 else var
        want = dict(mean=mean, var=var, invstd=(var + eps) ** -0.5, scale=float(gamma[c]) * (var + eps) ** -0.5,
                    rmean=(1 - mo) * float(rm[c]) + mo * mean, rvar=(1 - mo) * float(rv[c]) + mo * unb,
                    S1=sum(abs(v - col[0]) for v in col), S2=sum((v - col[0]) ** 2 for v in col))
        want["shift"] = float(beta[c]) - mean * want["scale"]
        for k, v in want.items():
            assert float(r[k][c]) == pytest.approx(v, rel=1e-12, abs=1e-13), (k, c)
    if M > 1:  # torch's own training-mode BatchNorm, float64 (it refuses M == 1)
        rm2, rv2 = rm.double(), rv.double()
        F.batch_norm(y.double().permute(0, 3, 1, 2), rm2, rv2, None, None, True, mo, eps)
        assert float((rm2 - r["rmean"]).abs().max()) < 1e-12 and float((rv2 - r["rvar"]).abs().max()) < 1e-12
    else:
        assert bool((r["var"] == 0).all()) and bool((r["unbiased"] == 0).all())
    stats = r["stats"].to(F32)
    out, _ = te.bn_act_fwd_reference(y, stats, act, res, F32)
    st = stats.double().tolist()
    for b, h, w, c in itertools.product(range(B), range(H), range(W), range(Cc)):
        z = float(y[b, h, w, c]) * st[2][c] + st[3][c]
        assert float(out[b, h, w, c]) == pytest.approx(_act_py(z, act) + float(res[b, h, w, c]), rel=1e-12, abs=1e-13)
    # backward: autograd through the same function of y, with the batch statistics part of the graph
    bw = te.bn_act_bwd_reference(y, dout, r["stats"], gamma, act, F32, torch.full((Cc,), 4.0, dtype=F64))
    x = y.double().reshape(M, Cc).clone().requires_grad_()
    gm, bt = gamma.double().clone().requires_grad_(), beta.double().clone().requires_grad_()
    mean = x.mean(0)
    xhat = (x - mean) / torch.sqrt((x - mean).square().mean(0) + eps)
    te.act64(xhat * gm + bt, act).backward(dout.double().reshape(M, Cc))
    assert float((bw["dgamma"] - gm.grad).abs().max()) < 1e-10 and float((bw["dbeta"] - bt.grad).abs().max()) < 1e-10
    assert float((bw["dx"].reshape(M, Cc) - x.grad).abs().max()) < 1e-10
    s, _, S = te.channel_sum_reference(y, torch.full((Cc,), 4.0, dtype=F64))
    assert float(s[1]) == pytest.approx(sum(row[1] for row in rows), abs=1e-12)
    assert float(S[1]) == pytest.approx(sum(abs(row[1]) for row in rows), abs=1e-12)


def _dw_loops(x, dy, w, s):
    B, H, W, Cc = x.shape
    _, oh, ow, _ = dy.shape
    dw = torch.zeros(Cc, 3, 3, dtype=F64)
    dx = torch.zeros(B, H, W, Cc, dtype=F64)
    for b, oy, ox, ky, kx, c in itertools.product(range(B), range(oh), range(ow), range(3), range(3), range(Cc)):
        iy, ix = oy * s - 1 + ky, ox * s - 1 + kx
        if 0 <= iy < H and 0 <= ix < W:
            dw[c, ky, kx] += dy[b, oy, ox, c] * x[b, iy, ix, c]
            dx[b, iy, ix, c] += dy[b, oy, ox, c] * w[c, ky, kx]
    return dw, dx


@pytest.mark.parametrize("H,W,s", [(4, 5, 1), (5, 4, 2), (6, 6, 2), (1, 3, 1)])
def test_depthwise_references_against_loops_and_autograd(H, W, s):
    g = torch.Generator().manual_seed(H + 10 * s)
    B, Cc = 2, 3
    oh, ow = (H - 1) // s + 1, (W - 1) // s + 1
    x, dy = torch.randn(B, H, W, Cc, generator=g).double(), torch.randn(B, oh, ow, Cc, generator=g).double()
    w = torch.randn(Cc, 3, 3, generator=g).double()
    dw, Sw = te.dw_wgrad_reference(x, dy, s)
    dx, Sx = te.dw_dgrad_reference(dy, w, s, H, W)
    want_dw, want_dx = _dw_loops(x, dy, w, s)
    assert float((dw - want_dw).abs().max()) < 1e-12 and float((dx - want_dx).abs().max()) < 1e-12
    abs_dw, abs_dx = _dw_loops(x.abs(), dy.abs(), w.abs(), s)
    assert float((Sw - abs_dw).abs().max()) < 1e-12 and float((Sx - abs_dx).abs().max()) < 1e-12
    xr, wr = x.permute(0, 3, 1, 2).clone().requires_grad_(), w.view(Cc, 1, 3, 3).clone().requires_grad_()
    F.conv2d(xr, wr, None, s, 1, 1, Cc).backward(dy.permute(0, 3, 1, 2))
    assert float((dw - wr.grad.view(Cc, 3, 3)).abs().max()) < 1e-12
    assert float((dx - xr.grad.permute(0, 2, 3, 1)).abs().max()) < 1e-12


def _spp_loops(x, dcat):
    """per output pixel: scan the clipped window row by row, keep the first maximum"""
    B, H, W, c = x.shape
    dx = dcat[..., :c].double().clone()
    xs = x.tolist()
    for n, k in enumerate(te.SPP_KS):
        r = k // 2
        for b, oy, ox, ch in itertools.product(range(B), range(H), range(W), range(c)):
            best, at = None, None
            for yy in range(max(0, oy - r), min(H - 1, oy + r) + 1):
                for xx in range(max(0, ox - r), min(W - 1, ox + r) + 1):
                    if best is None or xs[b][yy][xx][ch] > best:
                        best, at = xs[b][yy][xx][ch], (yy, xx)
            dx[b, at[0], at[1], ch] += float(dcat[b, oy, ox, (n + 1) * c + ch])
    return dx


@pytest.mark.parametrize("H,W", [(4, 4), (3, 14), (14, 2), (7, 8)])
def test_spp_reference_against_loops_and_max_pool(H, W):
    g = torch.Generator().manual_seed(H * 20 + W)
    B, c = 2, 2
    dcat = te.grid((B, H, W, 4 * c), g)
    tied = te.grid((B, H, W, c), g)  # 33 values on up to 169 pixels: ties everywhere
    assert float((te.spp_bwd_reference(tied, dcat) - _spp_loops(tied.double(), dcat)).abs().max()) == 0.0
    assert float((te.spp_bwd_reference(tied, dcat) - te.spp_bwd_reference(tied, dcat, last=True)).abs().max()) > 0
    free = torch.stack([torch.randperm(H * W * c, generator=g).double().view(H, W, c) for _ in range(B)])
    want = _spp_loops(free, dcat)
    assert float((te.spp_bwd_reference(free, dcat) - want).abs().max()) == 0.0
    xr = free.permute(0, 3, 1, 2).clone().requires_grad_()
    torch.cat([xr] + [F.max_pool2d(xr, k, 1, k // 2) for k in te.SPP_KS], 1).backward(dcat.double().permute(0, 3, 1, 2))
    assert float((want - xr.grad.permute(0, 2, 3, 1)).abs().max()) == 0.0


def test_upsample_reference_against_loops():
    g = torch.Generator().manual_seed(2)
    up, dst = torch.randn(2, 6, 4, 3, generator=g), torch.randn(2, 3, 2, 3, generator=g)
    got = te.upsample_bwd_reference(up, dst)
    for b, y, x, c in itertools.product(range(2), range(3), range(2), range(3)):
        want = float(dst[b, y, x, c]) + sum(float(up[b, 2 * y + i, 2 * x + j, c]) for i in (0, 1) for j in (0, 1))
        assert float(got[b, y, x, c]) == pytest.approx(want, abs=1e-12)


# ------------------------------------------------------------------------------------------ the fp32 emulation
def emu_reduce(terms, dtype, drop=None, drop_block=None):
    """per-channel sum of terms [M, C] (fp32) as chan_reduce + chan_finalize order it: a lane's rows and then the
    lanes in fp32, the blocks in double.  drop = (block, lane, channel): that lane's rows are lost"""
    M, Cc = terms.shape
    nblk, rpb = te.red_plan(M, Cc, dtype)
    lanes = te.row_lanes(Cc, dtype)
    total = torch.zeros(Cc, dtype=F64)
    for rpi in lanes.unique().tolist():
        cols = (lanes == rpi).nonzero().flatten()
        for b in range(nblk):
            if b == drop_block:
                continue
            block = terms[b * rpb:min(M, (b + 1) * rpb)]
            acc = torch.zeros(len(cols), dtype=F32)
            for lane in range(min(rpi, block.shape[0])):
                part = block[lane::rpi, cols].sum(0, dtype=F32)
                if drop is not None and drop[:2] == (b, lane):
                    part[cols.tolist().index(drop[2])] = 0.0
                acc = acc + part
            total[cols] += acc.double()
    return total


def emu_stats(ops, dtype, fault=None, drop=None, drop_block=None):
    v = ops["y"].float().reshape(-1, ops["y"].shape[-1])
    M, Cc = v.shape
    d = v - v[0]
    t1, t2 = emu_reduce(d, dtype, drop, drop_block), emu_reduce(d * d, dtype, drop, drop_block)
    if fault == "swap":
        t1, t2 = t2, t1
    eps, mo = torch.tensor(te.EPS, dtype=F32), torch.tensor(te.MOMENTUM, dtype=F32)
    m1 = t1 / M
    mean = v[0].double() + m1
    var = (t2 / M - m1 * m1).clamp_min(0)
    invstd = (1 / torch.sqrt(var + eps.double())).float()
    gam = ops["gamma"] if ops["gamma"] is not None else torch.ones(Cc)
    bet = ops["beta"] if ops["beta"] is not None else torch.zeros(Cc)
    scale = gam * invstd
    out = dict(stats=torch.stack([mean.float(), invstd, scale, bet - mean.float() * scale]))
    if ops["rmean"] is not None:
        unb = var * M / (M - 1) if M > 1 and fault != "biased" else var
        out["rmean"] = (1 - mo) * ops["rmean"] + mo * mean.float()
        out["rvar"] = (1 - mo) * ops["rvar"] + mo * unb.float()
    return out


F32_SLOPE = torch.tensor(0.1, dtype=F32)


def _act32(z, act):
    if act == te.ACT_SILU:
        return z / (1 + torch.exp(-z))
    if act == te.ACT_RELU:
        return torch.where(z > 0, z, torch.zeros_like(z))
    return torch.where(z > 0, z, z * F32_SLOPE) if act == te.ACT_LRELU else z


def _act_grad32(z, act):
    if act == te.ACT_SILU:
        s = 1 / (1 + torch.exp(-z))
        return s * (1 + z * (1 - s))
    if act == te.ACT_NONE:
        return torch.ones_like(z)
    return torch.where(z > 0, torch.ones_like(z), torch.zeros_like(z) if act == te.ACT_RELU else F32_SLOPE.expand_as(z))


def emu_fwd(ops, stats, act, dtype):
    z = ops["y"].float() * stats[2] + stats[3]
    o = _act32(z, act)
    return (o + ops["res"].float() if ops["res"] is not None else o).to(dtype)


def emu_bwd(ops, stats, act, dtype, drop=None):
    v = ops["y"].float().reshape(-1, stats.shape[1])
    M, Cc = v.shape
    g = ops["dout"].reshape(M, Cc)
    dz = g * _act_grad32(v * stats[2] + stats[3], act)
    t1, t2 = emu_reduce(dz, dtype, drop), emu_reduce(dz * ((v - stats[0]) * stats[1]), dtype, drop)
    inv_m = torch.tensor(1.0 / M, dtype=F32)
    k1 = (ops["gamma"] if ops["gamma"] is not None else torch.ones(Cc)) * stats[1]
    k2, k3 = -k1 * stats[1] * (t2.float() * inv_m), -k1 * (t1.float() * inv_m)
    return dict(dgamma=t2.float(), dbeta=t1.float(), dx=(k1 * dz + k2 * (v - stats[0]) + k3).to(dtype).reshape(ops["y"].shape))


def judge_bn(case, dt, mode, st, fwd=None, bwd=None, total=None):
    """the GPU test's judgement of one case, on emulated results -> the worst ratios"""
    dtype, ops = te.DTYPES[dt], te.bn_operands(case, dt, mode)
    M, Cc = case.M, case.C
    full = mode == "full"
    chain = te.chain(M, Cc, dtype)
    ref = te.bn_stats_reference(ops["y"], ops["gamma"], ops["beta"], ops["rmean"], ops["rvar"])
    tol = te.bn_stats_tolerance(ref, chain if full else None)
    worst = dict(stats=te.judge(st["stats"], ref["stats"], tol["stats"], label="stats"))
    if not full:
        te.grid_sum_exact(M, 16.0)
        te.judge_exact(st["stats"][0], ref["mean"].to(F32).to(F64), label="mean")
    if case.running:
        worst["rmean"] = te.judge(st["rmean"], ref["rmean"], tol["rmean"], label="rmean")
        worst["rvar"] = te.judge(st["rvar"], ref["rvar"], tol["rvar"], label="rvar")
    act = case.act if full else te.ACT_NONE
    if total is not None:
        y_sum, tol_sum, _ = te.channel_sum_reference(ops["y"], chain)
        if full:
            worst["sum"] = te.judge(total, y_sum, tol_sum, label="channel_sum")
        else:
            te.assert_grid_exact(y_sum, M, max_product=2.0)
            te.judge_exact(total, y_sum, label="channel_sum")
    if fwd is not None:
        want, tol_out = te.bn_act_fwd_reference(ops["y"], st["stats"], act, ops["res"], dtype)
        worst["out"] = te.judge(fwd, want, tol_out, label="forward")
    if bwd is not None:
        b = te.bn_act_bwd_reference(ops["y"], ops["dout"], st["stats"], ops["gamma"], act, dtype, chain)
        assert b["ambiguous"] <= te.AMBIGUOUS_CAP, b["ambiguous"]
        if full:
            worst["dbeta"] = te.judge(bwd["dbeta"], b["dbeta"], b["tol_dbeta"], label="dbeta")
        else:
            te.assert_grid_exact(b["dbeta"], M, max_product=2.0)
            te.judge_exact(bwd["dbeta"], b["dbeta"], label="dbeta")
        worst["dgamma"] = te.judge(bwd["dgamma"], b["dgamma"], b["tol_dgamma"], label="dgamma")
        worst["dx"] = te.judge(bwd["dx"], b["dx"], b["tol_dx"], label="dx", judged=b["judged"])
    return worst


def emulate_and_judge(case, dt, mode, **fault):
    dtype, ops = te.DTYPES[dt], te.bn_operands(case, dt, mode)
    act = case.act if mode == "full" else te.ACT_NONE
    st = emu_stats(ops, dtype, **fault)
    clean = emu_stats(ops, dtype)["stats"] if fault else st["stats"]  # downstream kernels: judged on their own
    total = emu_reduce(ops["y"].float().reshape(-1, case.C), dtype, fault.get("drop"), fault.get("drop_block")).float()
    return judge_bn(case, dt, mode, st, emu_fwd(ops, clean, act, dtype), emu_bwd(ops, clean, act, dtype), total)


@pytest.mark.parametrize("case,dt", BN_PARAMS, ids=BN_IDS)
def test_batchnorm_case_preconditions_and_fp32_emulation(case, dt):
    """grid exactness and the ambiguity cap hold on the reference alone (judge_bn asserts both), and plain fp32
    arithmetic in the kernels' order stays inside every bound"""
    assert case.M <= 16384 and case.C % te.EPC[te.DTYPES[dt]] == 0
    for mode in ("grid", "full"):
        worst = emulate_and_judge(case, dt, mode)
        assert max(worst.values()) <= 1.0, worst


def test_case_lists_reach_what_they_were_chosen_for():
    for case in te.CAP_CASES:
        for dt in case.dts:
            nblk, rpb = te.red_plan(case.M, case.C, te.DTYPES[dt])
            assert 448 < nblk < 512 and int(te.row_lanes(case.C, te.DTYPES[dt]).max()) == 1, (case, nblk, rpb)
    lanes = {(c.C, dt): te.row_lanes(c.C, te.DTYPES[dt]) for c, dt in BN_PARAMS}
    idle = {(C, dt) for C, dt in lanes if C // te.EPC[te.DTYPES[dt]] < 256 and 256 % (C // te.EPC[te.DTYPES[dt]])}
    assert {(24, "f32"), (48, "bf16"), (80, "f32"), (320, "f16")} <= idle  # chunk counts that do not divide 256
    assert len(lanes[(1280, "f32")].unique()) == 2 and len(lanes[(2560, "bf16")].unique()) == 2  # two channel groups
    assert any(c.M < int(te.row_lanes(c.C, te.DTYPES[dt]).min()) for c, dt in BN_PARAMS) and any(c.M == 1 for c in te.BN_CASES)
    assert {te.spp_cpb(c.H, c.W) for c in te.SPP_CASES} == {4, 2, 1}
    assert all(te.spp_cpb(H, W) == cpb for (H, W), cpb in te.SPP_CPB.items())
    assert {1706, 1707, 3413, 3414, 6826} <= {c.H * c.W for c in te.SPP_CASES}  # both sides of every threshold
    assert [te.spp_cpb(1, a) for a in (1706, 1707, 3413, 3414, 6826)] == [4, 2, 2, 1, 1] and 6827 * 24 > 160 * 1024
    assert any(c.c % te.spp_cpb(c.H, c.W) for c in te.SPP_CASES) and any(c.idle for c in te.SPP_CASES)
    assert {te.dw_nsplit(c.B, c.oh, c.ow) for c in te.DW_CASES} >= {1, 2, 3}
    assert any(c.C > 64 and c.C % 64 for c in te.DW_CASES) and any(c.C % 8 for c in te.DW_CASES)


@pytest.mark.parametrize("case", te.DW_CASES, ids=[c.id for c in te.DW_CASES])
def test_depthwise_cases_meet_their_conditions(case):
    for dt in case.dts:
        ops = te.dw_operands(case, dt, "grid")  # asserts grid exactness
        assert float((_f32_dw(ops, case) - ops["dw"]).abs().max()) == 0.0
        if case.full:
            ops = te.dw_operands(case, dt, "full")
            te.judge(_f32_dw(ops, case).float(), ops["dw"], ge.tolerance(case.K, ops["Sw"]), label="dw")
            xr = torch.zeros(case.B, case.C, case.H, case.W, requires_grad=True)
            F.conv2d(xr, ops["w"].float().view(case.C, 1, 3, 3), None, case.s, 1, 1, case.C).backward(
                ops["dy"].float().permute(0, 3, 1, 2))
            te.judge(xr.grad.permute(0, 2, 3, 1), ops["dx"], ge.tolerance(9, ops["Sx"]), label="dx")


def _f32_dw(ops, case):
    """torch fp32 autograd of the depthwise conv -> dw [C][3][3] as float64"""
    wr = torch.zeros(case.C, 1, 3, 3, requires_grad=True)
    F.conv2d(ops["x"].float().permute(0, 3, 1, 2), wr, None, case.s, 1, 1, case.C).backward(
        ops["dy"].float().permute(0, 3, 1, 2))
    return wr.grad.view(case.C, 3, 3).double()


# ------------------------------------------------------------------------------------------ planted faults
ODD = next(c for c in te.BN_CASES if c.C == 24 and c.running)       # 42 / 85 row lanes, running statistics
ROWS = next(c for c in te.BN_CASES if c.M == 8192)                  # 32 / 16 blocks of 256 / 512 rows


@pytest.mark.parametrize("dt", te.ALL)
@pytest.mark.parametrize("mode", ["grid", "full"])
def test_planted_reduction_faults_are_rejected(dt, mode):
    clean = emulate_and_judge(ODD, dt, mode)
    assert max(clean.values()) <= 1.0
    bad = (te.PerElementError,)
    assert raises(bad, emulate_and_judge, ODD, dt, mode, drop=(0, 1, 5)), "a dropped row lane of channel 5"
    assert raises(bad, emulate_and_judge, ODD, dt, mode, fault="swap"), "sum 1 and sum 2 swapped"
    assert raises(bad, emulate_and_judge, ODD, dt, mode, fault="biased"), "the biased variance in running_var"
    assert raises(bad, emulate_and_judge, ROWS, dt, mode, drop_block=3), "a partial block left out"
    assert raises(bad, emulate_and_judge, te.CAP_CASES[0], te.CAP_CASES[0].dts[0], mode, drop_block=460), \
        "a partial of the eighth chain left out"


def test_dropped_lane_in_the_backward_sums_is_rejected():
    ops = te.bn_operands(ODD, "f32", "full")
    st = emu_stats(ops, F32)
    bwd = emu_bwd(ops, st["stats"], ODD.act, F32, drop=(0, 2, 7))
    assert raises(te.PerElementError, judge_bn, ODD, "f32", "full", st, bwd=bwd)
    assert max(judge_bn(ODD, "f32", "full", st, bwd=emu_bwd(ops, st["stats"], ODD.act, F32)).values()) <= 1.0


@pytest.mark.parametrize("act", [te.ACT_RELU, te.ACT_LRELU])
def test_elements_without_a_side_are_left_out_of_dx_and_bounded_in_the_sums(act):
    """no case of the GPU list has one (the cap is checked per case), so the rule itself is pinned here: z == 0 at
    two of 24 elements; taking either side there passes, a wrong side anywhere else does not"""
    g = torch.Generator().manual_seed(act)
    y, dout = torch.randn(1, 2, 3, 4, generator=g), torch.randn(1, 2, 3, 4, generator=g)
    y[0, 0, 1, 2] = y[0, 1, 0, 3] = 0.0
    stats = torch.stack([torch.zeros(4), torch.ones(4), torch.ones(4), torch.zeros(4)])
    chain = torch.full((4,), 6.0, dtype=F64)
    b = te.bn_act_bwd_reference(y, dout, stats, None, act, F32, chain)
    assert b["ambiguous"] == pytest.approx(2 / 24) and int((~b["judged"]).sum()) == 2
    slope = 0.0 if act == te.ACT_RELU else te.LRELU_SLOPE
    for side in (1.0, slope):  # the other side at the two elements: dz there, and both sums, change
        d = torch.where(b["judged"], te.act_grad64(y.double(), act), torch.full_like(y, side, dtype=F64)) * dout.double()
        v = y.double().reshape(6, 4)
        db, dg = d.reshape(6, 4).sum(0), (d.reshape(6, 4) * v).sum(0)
        dx = d - db / 6 - y.double() * dg / 6
        te.judge(db.float(), b["dbeta"], b["tol_dbeta"], label="dbeta")
        te.judge(dg.float(), b["dgamma"], b["tol_dgamma"], label="dgamma")
        te.judge(dx.float(), b["dx"], b["tol_dx"], label="dx", judged=b["judged"])
    wrong = b["dx"].clone()
    wrong[0, 1, 1, 1] += (1 - slope) * float(dout[0, 1, 1, 1])  # a defined element on the wrong side
    assert raises(te.PerElementError, te.judge, wrong.float(), b["dx"], b["tol_dx"], judged=b["judged"])


def test_last_maximum_on_a_tie_is_rejected():
    for case in te.SPP_CASES[:5]:
        ops = te.spp_operands(case, "bf16")
        wrong = te.spp_bwd_reference(ops["x"], ops["dcat"], last=True)
        assert raises(te.PerElementError, te.judge_exact, wrong.float(), ops["dx"])
        te.judge_exact(ops["dx"].float(), ops["dx"])


@pytest.mark.parametrize("mode", ["grid", "full"])
def test_flipped_tap_is_rejected(mode):
    case = next(c for c in te.DW_CASES if c.full and "f32" in c.dts)
    ops = te.dw_operands(case, "f32", mode)
    w = ops["w"].clone()
    w[:, 1, 2] = -w[:, 1, 2]
    wrong, _ = te.dw_dgrad_reference(ops["dy"], w, case.s, case.H, case.W)
    wrong_dw = te._dw_wgrad64(ops["x"].double(), ops["dy"].double(), case.s)
    wrong_dw[:, 0, 1] = -wrong_dw[:, 0, 1]
    if mode == "grid":
        assert raises(te.PerElementError, te.judge_exact, wrong.float(), ops["dx"])
        assert raises(te.PerElementError, te.judge_exact, wrong_dw.float(), ops["dw"])
    else:
        assert raises(te.PerElementError, te.judge, wrong.float(), ops["dx"], ge.tolerance(9, ops["Sx"]))
        assert raises(te.PerElementError, te.judge, wrong_dw.float(), ops["dw"], ge.tolerance(case.K, ops["Sw"]))
        te.judge(ops["dx"].float(), ops["dx"], ge.tolerance(9, ops["Sx"]))


@pytest.mark.parametrize("dtype", [F32, torch.bfloat16, torch.float16])
def test_stray_store_and_unwritten_element_are_named(dtype):
    epc = te.EPC[dtype]
    off, idle, pad = te.VIEWS["padded"]
    want = te.grid((2, 3, 4, 16), torch.Generator().manual_seed(1)).double()
    tol = torch.full_like(want, 1e-3)

    def fresh():
        return te.ViewBuf(2, 3, 4, 16, dtype, "cpu", off, idle, pad)

    buf = fresh().set(want)
    assert te.judge(buf.get(), want, tol, [buf.outside("out")]) == 0.0
    buf = fresh().set(want)
    buf.view[1, 5, off + 16:off + 16 + epc] = 1.0  # one chunk past the slice
    assert raises(te.GuardError, te.judge, buf.get(), want, tol, [buf.outside("out")])
    buf = fresh().set(want)
    buf.view[0, 12, off:off + epc] = 1.0  # image 0's first padding row
    assert raises(te.GuardError, te.judge, buf.get(), want, tol, [buf.outside("out")])
    buf = fresh().set(want)
    buf.flat[ge.GUARD - 1] = 1.0  # the element before the view
    assert raises(te.GuardError, te.judge, buf.get(), want, tol, [buf.outside("out")])
    buf = fresh().set(want)
    buf.live.view(torch.int16 if epc == 8 else torch.int32)[1, 7, 3] = buf.canary  # never written
    assert raises(te.PerElementError, te.judge, buf.get(), want, tol, [buf.outside("out")])
