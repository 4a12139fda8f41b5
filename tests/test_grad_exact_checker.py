"""The judge of the gradient kernels (tests/grad_exact.py) pinned on the CPU, as test_conv_exact_checker.py pins the
forward one: the float64 references against cases worked in plain loops, and for every geometry of the GPU lists
the conditions of the mode(s) it is judged in -- so a pass on the device means what it says.

  grid mode            assert_grid_exact holds; torch fp32 on the CPU equals the float64 reference bit for bit;
                       a reference with one operand element changed by 1 / 8, with one border tap of one pixel
                       dropped, or with one pixel counted twice is rejected
  full-mantissa mode   torch fp32 stays at <= 0.25 of the bound; dropping one pixel exceeds the bound at >= 90 %
                       of the elements it changes; with fp32 operands, truncating them to bf16 reaches >= 4 x the
                       bound somewhere
A geometry that cannot meet the second set is judged on grid operands only (full=False in grad_exact.py).
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

import grad_exact as ge

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
TORCH_CAP, DROP_SHARE, TRUNC_FACTOR = 0.25, 0.90, 4.0


def ids(geoms):
    return ["-".join(str(v) for v in g).replace(" ", "") for g in geoms]


def rejected(y_mutant, y):
    """the grid judge, handed a mutant reference's values as the kernel's output, raises"""
    try:
        ge.judge_exact(y_mutant.to(F32), y, label="mutant")
    except ge.PerElementError:
        return True
    return False


def truncate_bf16(t):
    return (t.contiguous().view(torch.int32) & ~0xFFFF).view(F32)


# ------------------------------------------------------------------------------------------ hand-worked references
def wgrad_loops(srcs, dy, cout, k, s, p, cin_store):
    xs = [x.tolist() for x, _ in srcs]
    B, oh, ow = dy.shape[:3]
    H, W = (srcs[0][0].shape[1] << srcs[0][1]), (srcs[0][0].shape[2] << srcs[0][1])
    g = dy.tolist()
    dw = [[[[0.0] * k for _ in range(k)] for _ in range(cin_store)] for _ in range(cout)]
    for n, c, ky, kx in itertools.product(range(cout), range(cin_store), range(k), range(k)):
        si, cc = 0, c
        if c >= srcs[0][0].shape[3]:
            si, cc = 1, c - srcs[0][0].shape[3]
        up = srcs[si][1]
        acc = 0.0
        for b, oy, ox in itertools.product(range(B), range(oh), range(ow)):
            iy, ix = oy * s - p + ky, ox * s - p + kx
            if 0 <= iy < H and 0 <= ix < W:
                acc += g[b][oy][ox][n] * xs[si][b][iy >> up][ix >> up][cc]
        dw[n][c][ky][kx] = acc
    return torch.tensor(dw, dtype=torch.float64)


@pytest.mark.parametrize("k,s,H,W", [(3, 2, 6, 4), (3, 1, 4, 6), (3, 2, 5, 7), (1, 1, 4, 2)])
def test_wgrad_reference_against_loops(k, s, H, W):
    """two sources, the second upsampled, cin_store < cin, a dy wider than cout"""
    g = torch.Generator().manual_seed(H + s)
    p = (k - 1) // 2
    oh, ow = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    srcs = [(torch.randn(2, H, W, 2, generator=g), 0)]
    if H % 2 == 0 and W % 2 == 0:
        srcs.append((torch.randn(2, H // 2, W // 2, 3, generator=g), 1))
    else:
        srcs.append((torch.randn(2, H, W, 3, generator=g), 0))
    dy = torch.randn(2, oh, ow, 4, generator=g)
    dw, S = ge.wgrad_reference(srcs, dy, 3, k, s, p, 4)
    assert dw.shape == (3, 4, k, k) and dw.dtype == torch.float64
    want = wgrad_loops(srcs, dy, 3, k, s, p, 4)
    assert float((dw - want).abs().max()) < 1e-12
    assert float((S - wgrad_loops([(x.abs(), u) for x, u in srcs], dy.abs(), 3, k, s, p, 4)).abs().max()) < 1e-12
    # the same through torch autograd, fp64
    x = ge.cat_sources(srcs).permute(0, 3, 1, 2)
    w = torch.zeros(3, 5, k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, stride=s, padding=p).backward(dy[..., :3].double().permute(0, 3, 1, 2))
    assert float((dw - w.grad[:, :4]).abs().max()) < 1e-12


def dgrad_loops(dy, w, k, s, in_hw):
    p = (k - 1) // 2
    H, W = in_hw
    B, oh, ow, cout = dy.shape
    cin = w.shape[1]
    g, wl = dy.tolist(), w.tolist()
    dx = [[[[0.0] * cin for _ in range(W)] for _ in range(H)] for _ in range(B)]
    for b, oy, ox, ky, kx in itertools.product(range(B), range(oh), range(ow), range(k), range(k)):
        iy, ix = oy * s - p + ky, ox * s - p + kx
        if 0 <= iy < H and 0 <= ix < W:
            for c in range(cin):
                dx[b][iy][ix][c] += sum(g[b][oy][ox][n] * wl[n][c][ky][kx] for n in range(cout))
    return torch.tensor(dx, dtype=torch.float64)


@pytest.mark.parametrize("k,s,H,W", [(3, 2, 6, 4), (3, 2, 5, 7), (3, 1, 4, 5), (1, 1, 3, 2)])
def test_dgrad_reference_against_loops(k, s, H, W):
    g = torch.Generator().manual_seed(H * 3 + s)
    p = (k - 1) // 2
    oh, ow = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = torch.randn(2, oh, ow, 3, generator=g).to(BF16)
    w = torch.randn(3, 2, k, k, generator=g)
    dx, S = ge.dgrad_reference(dy, w, k, s, (H, W))
    assert dx.shape == (2, H, W, 2) and dx.dtype == torch.float64
    wr = w.to(BF16).double()  # rounded once to the compute dtype, as the packer does
    assert float((dx - dgrad_loops(dy.double(), wr, k, s, (H, W))).abs().max()) < 1e-12
    assert float((S - dgrad_loops(dy.double().abs(), wr.abs(), k, s, (H, W))).abs().max()) < 1e-12
    assert float((dx - dgrad_loops(dy.double(), w.double(), k, s, (H, W))).abs().max()) > 1e-6  # (the rounding counts)


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_dgrad_weight_reference_against_loops(dtype):
    g = torch.Generator().manual_seed(4)
    cout, cin, k, c_begin, c_count, cout_pad = 3, 5, 3, 2, 2, 8
    w = torch.randn(cout, cin, k, k, generator=g)
    got = ge.dgrad_weight_reference(w, c_begin, c_count, cout_pad, dtype)
    assert got.shape == (c_count, k, k, cout_pad) and got.dtype == dtype
    for c, ky, kx, n in itertools.product(range(c_count), range(k), range(k), range(cout_pad)):
        want = w[n, c_begin + c, k - 1 - ky, k - 1 - kx].to(dtype) if n < cout else torch.zeros((), dtype=dtype)
        assert got[c, ky, kx, n].view(torch.int16 if dtype != F32 else torch.int32) == \
            want.view(torch.int16 if dtype != F32 else torch.int32), (c, ky, kx, n)


# ------------------------------------------------------------------------------------------ the judge itself
def test_grid_and_precondition():
    g = torch.Generator().manual_seed(0)
    v = ge.grid((4000,), g)
    assert float(v.abs().max()) == 2.0 and float(v.min()) == -2.0
    assert bool(((v * 8).round() == v * 8).all())
    for dt in (BF16, F16):
        assert torch.equal(v.to(dt).float(), v)
    ge.assert_grid_exact(v.double(), 65536)
    with pytest.raises(AssertionError, match="leaves the exact regime"):
        ge.assert_grid_exact(v.double(), 65537)
    with pytest.raises(AssertionError, match="not an fp32 number"):
        ge.assert_grid_exact(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64), 8)


def test_judge_reports_the_first_bad_index_and_names_the_guard():
    y = torch.arange(24, dtype=torch.float64).view(2, 3, 4)
    got = y.float().clone()
    assert ge.judge_exact(got, y) == 0.0
    got[1, 0, 2] += 2.0 ** -20
    got[1, 2, 3] += 1
    with pytest.raises(ge.PerElementError, match=r"2 of 24 elements differ.*first at \(1, 0, 2\)"):
        ge.judge_exact(got, y, label="x")
    got = y.float().clone()
    got[0, 1, 1] = float("nan")
    with pytest.raises(ge.PoisonError, match=r"first at \(0, 1, 1\)"):
        ge.judge_exact(got, y)
    # a guarded slice: a store before it, in its idle channels, or after it names the buffer
    for where in ("front", "idle", "back"):
        d = ge.Guarded((2, 3), 4, F32, "cpu", off=8, idle=16)
        assert d.view.shape == (2, 3, 20) and d.slice.shape == (2, 3, 4)
        assert d.data_ptr() == d.flat.data_ptr() + (ge.GUARD + 8) * 4
        d.set(y.view(2, 3, 4))
        ge.judge_exact(d.slice, y.view(2, 3, 4), guards=[d.outside("dW's buffer")])
        if where == "front":
            d.flat[ge.GUARD - 1] = 0.0
        elif where == "idle":
            d.view[1, 2, 12] = 0.0
        else:
            d.flat[ge.GUARD + d.n] = 0.0
        with pytest.raises(ge.GuardError, match="1 guard elements of dW's buffer overwritten"):
            ge.judge_exact(d.slice, y.view(2, 3, 4), guards=[d.outside("dW's buffer")])
        with pytest.raises(ge.GuardError, match="dW's buffer"):
            ge.judge_bound(d.slice, y.view(2, 3, 4), torch.ones(2, 3, 4, dtype=torch.float64),
                           guards=[d.outside("dW's buffer")])
    w = ge.Workspace(64, "cpu")
    ge.check_guards([w.guards(), w.untouched()])
    w.live[3] = 1.0
    ge.check_guards([w.guards()])
    with pytest.raises(ge.GuardError, match="too small for one partial"):
        ge.check_guards([w.untouched()])
    w.flat[ge.GUARD + 16] = 0.0
    with pytest.raises(ge.GuardError, match="the workspace's guards"):
        ge.check_guards([w.guards()])
    x = ge.Guarded((2, 2, 2), 8, BF16, "cpu", off=16, idle=32, fill="nan")
    assert bool(torch.isnan(x.flat).all())
    x.set(torch.ones(2, 2, 2, 8))
    assert int(torch.isnan(x.flat).sum()) == x.flat.numel() - 64


# ------------------------------------------------------------------------------------------ weight gradient
def wgrad_pixel(geom, x, dy, b, oy, ox, taps=None):
    """the contribution of output pixel (b, oy, ox) to dW (float64), over `taps` [(ky, kx)] or every valid one"""
    out = torch.zeros(geom.cout, geom.cin_store, geom.k, geom.k, dtype=torch.float64)
    for ky in range(geom.k):
        for kx in range(geom.k):
            iy, ix = oy * geom.s - geom.pad + ky, ox * geom.s - geom.pad + kx
            if 0 <= iy < geom.H and 0 <= ix < geom.W and (taps is None or (ky, kx) in taps):
                out[:, :, ky, kx] = torch.outer(dy[b, oy, ox, :geom.cout], x[b, iy, ix, :geom.cin_store])
    return out


def last_valid_tap(k, s, p, o, size):
    return max(t for t in range(k) if 0 <= o * s - p + t < size)


def wgrad_torch32(geom, ops):
    x = ge.cat_sources(list(zip(ops["srcs"], [u for _, u in geom.srcs])), F32).permute(0, 3, 1, 2)
    w = torch.zeros(geom.cout, geom.cin, geom.k, geom.k, requires_grad=True)
    F.conv2d(x, w, stride=geom.s, padding=geom.pad).backward(ops["dy"][..., :geom.cout].float().permute(0, 3, 1, 2))
    return ops["prefill"] + w.grad[:, :geom.cin_store]


@pytest.mark.parametrize("geom", ge.WGRAD_GEOMS, ids=ids(ge.WGRAD_GEOMS))
def test_wgrad_geometry_grid_conditions(geom):
    ops = ge.wgrad_operands(geom, F32, "grid")  # (asserts assert_grid_exact)
    y = ops["y"]
    ge.assert_grid_exact(y, geom.K + 1)
    for dt in (BF16, F16):  # the same values in every compute dtype
        assert all(torch.equal(a.to(dt).float(), a) for a in ops["srcs"] + [ops["dy"]])
    assert ge.judge_exact(wgrad_torch32(geom, ops), y, label="torch fp32") == 0.0
    srcs = [(x, u) for x, (_, u) in zip(ops["srcs"], geom.srcs)]
    x64, dy64 = ge.cat_sources(srcs), ops["dy"].double()
    # one operand element changed by 1 / 8
    for which in ("x", "dy"):
        xs, dy = [x.clone() for x in ops["srcs"]], ops["dy"].clone()
        if which == "x":
            xs[-1][geom.B - 1, -1, -1, 0] += 0.125
        else:
            dy[0, 0, 0, geom.cout - 1] += 0.125
        m, _ = ge.wgrad_reference([(x, u) for x, (_, u) in zip(xs, geom.srcs)], dy, geom.cout, geom.k, geom.s,
                                  geom.pad, geom.cin_store)
        assert rejected(m + ops["prefill"].double(), y), which
    # one border tap of one pixel dropped; one pixel counted twice
    oy, ox = geom.oh - 1, geom.ow - 1
    tap = (last_valid_tap(geom.k, geom.s, geom.pad, oy, geom.H), last_valid_tap(geom.k, geom.s, geom.pad, ox, geom.W))
    assert rejected(y - wgrad_pixel(geom, x64, dy64, geom.B - 1, oy, ox, [tap]), y)
    assert rejected(y + wgrad_pixel(geom, x64, dy64, 0, 0, 0), y)


FULL_WG = [g for g in ge.WGRAD_GEOMS if g.full]


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("geom", FULL_WG, ids=ids(FULL_WG))
def test_wgrad_geometry_full_mantissa_conditions(geom, dtype):
    ops = ge.wgrad_operands(geom, dtype, "full")
    y, tol = ops["y"], ops["tol"]
    r, at = ge.ce.element_ratio(wgrad_torch32(geom, ops), y, tol)
    assert r <= TORCH_CAP, (r, at)
    srcs = [(x, u) for x, (_, u) in zip(ops["srcs"], geom.srcs)]
    x64, dy64 = ge.cat_sources(srcs), ops["dy"].double()
    delta = wgrad_pixel(geom, x64, dy64, geom.B - 1, geom.oh // 2, geom.ow // 2)
    changed = delta != 0
    share = float(((delta.abs() > tol) & changed).sum()) / float(changed.sum())
    assert share >= DROP_SHARE, share
    if dtype == F32:
        m, _ = ge.wgrad_reference([(truncate_bf16(x), u) for x, u in srcs], truncate_bf16(ops["dy"]), geom.cout,
                                  geom.k, geom.s, geom.pad, geom.cin_store)
        worst = float(((m - ops["dw"]).abs() / tol).max())
        assert worst >= TRUNC_FACTOR, worst
    print(f"\n{tuple(geom)}: torch fp32 {r:.4f} of the bound, dropped pixel above it at {share:.3f}")


# ------------------------------------------------------------------------------------------ data gradient
DG_ALL = ge.DGRAD_S2_GEOMS + ge.DGRAD_S1_GEOMS


def dgrad_torch32(geom, ops):
    dy = ops["dy"]
    w = ops["w"].to(dy.dtype).float()
    x = torch.zeros(geom.B, geom.cin, geom.H, geom.W, requires_grad=True)
    F.conv2d(x, w, stride=geom.s, padding=geom.pad).backward(dy.float().permute(0, 3, 1, 2))
    return x.grad.permute(0, 2, 3, 1).contiguous()


def dgrad_pixel(geom, dy64, w64, b, oy, ox, taps=None):
    """the contribution of dy's pixel (b, oy, ox) to dx"""
    out = torch.zeros(geom.B, geom.H, geom.W, geom.cin, dtype=torch.float64)
    for ky in range(geom.k):
        for kx in range(geom.k):
            iy, ix = oy * geom.s - geom.pad + ky, ox * geom.s - geom.pad + kx
            if 0 <= iy < geom.H and 0 <= ix < geom.W and (taps is None or (ky, kx) in taps):
                out[b, iy, ix] = dy64[b, oy, ox] @ w64[:, :, ky, kx]
    return out


@pytest.mark.parametrize("geom", DG_ALL, ids=ids(DG_ALL))
def test_dgrad_geometry_grid_conditions(geom):
    ops = ge.dgrad_operands(geom, F32, "grid")
    dx = ops["dx"]
    ge.assert_grid_exact(dx, geom.K)
    ge.assert_grid_exact(ops["y_acc"], geom.K + 1)
    for dt in (BF16, F16):
        assert torch.equal(ops["dy"].to(dt).float(), ops["dy"]) and torch.equal(ops["w"].to(dt).float(), ops["w"])
    t32 = dgrad_torch32(geom, ops)
    assert ge.judge_exact(t32, dx, label="torch fp32") == 0.0
    assert ge.judge_exact(t32 + ops["base"], ops["y_acc"], label="torch fp32, accumulated") == 0.0
    for which in ("dy", "w"):
        dy, w = ops["dy"].clone(), ops["w"].clone()
        if which == "dy":
            dy[geom.B - 1, -1, -1, geom.cout - 1] += 0.125
        else:
            w[0, geom.cin - 1, 0, geom.k - 1] += 0.125
        assert rejected(ge.dgrad_reference(dy, w, geom.k, geom.s, (geom.H, geom.W))[0], dx), which
    dy64, w64 = ops["dy"].double(), ops["w"].double()
    oy, ox = geom.oh - 1, geom.ow - 1
    tap = (last_valid_tap(geom.k, geom.s, geom.pad, oy, geom.H), last_valid_tap(geom.k, geom.s, geom.pad, ox, geom.W))
    assert rejected(dx - dgrad_pixel(geom, dy64, w64, geom.B - 1, oy, ox, [tap]), dx)
    assert rejected(dx + dgrad_pixel(geom, dy64, w64, 0, 0, 0), dx)


FULL_DG = [g for g in DG_ALL if g.full]


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("geom", FULL_DG, ids=ids(FULL_DG))
def test_dgrad_geometry_full_mantissa_conditions(geom, dtype):
    if dtype == F32 and geom not in ge.DGRAD_S2_GEOMS:
        return  # the stride-1 ids (conv_ws, 281-288) are built for 16-bit operands alone: nothing runs this in fp32
    ops = ge.dgrad_operands(geom, dtype, "full")
    t32 = dgrad_torch32(geom, ops)
    for acc in (False, True):
        y = ops["y_acc"] if acc else ops["dx"]
        tol = ge.dgrad_tolerance(geom, ops, acc)
        r, at = ge.ce.element_ratio(t32 + ops["base"] if acc else t32, y, tol)
        assert r <= TORCH_CAP, (acc, r, at)
        # one output pixel dropped: not written (the write form leaves the canary there; judged here as a zero)
        # or not added
        pix = ops["dx"][geom.B - 1, geom.H // 2, geom.W // 2]
        ptol = tol[geom.B - 1, geom.H // 2, geom.W // 2]
        share = float(((pix.abs() > ptol) & (pix != 0)).sum()) / float((pix != 0).sum())
        assert share >= DROP_SHARE, (acc, share)
        if dtype == F32:
            m, _ = ge.dgrad_reference(truncate_bf16(ops["dy"]), truncate_bf16(ops["w"]), geom.k, geom.s,
                                      (geom.H, geom.W))
            worst = float(((m - ops["dx"]).abs() / tol).max())
            assert worst >= TRUNC_FACTOR, (acc, worst)
        print(f"\n{tuple(geom)} {'accumulate' if acc else 'write'}: torch fp32 {r:.4f} of the bound, dropped pixel "
              f"above it at {share:.3f}")
