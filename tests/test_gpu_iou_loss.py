"""The standalone IouLoss kernels (csrc/iou_loss.hip, csrc/iou_loss.hpp) against the reference's
IouLoss (tests/golden/iou_loss.npz boxes.*, written by tests/golden/make_golden_iou.py).

The bar is measured, not chosen: for each loss type and each quantity the fixture holds the
reference in fp64 and in fp32.  The fp32 reference's deviation from the fp64 one on the 1000
random pairs (loss: max abs; gradients: max abs over max |fp64|) is the noise of computing this
formula in fp32 at all, and the kernel's deviation from fp64, in the same measure, may be at most
4 x that (the kernel's backward groups a few sums differently from autograd's graph).  The edge
table is held to the same numbers, in its own max |fp64|.  On the committed fixture the
reference's noise is 2.7e-6 / 2.9e-6 (loss, iou / giou), 4.4e-6 / 9.8e-7 (d pred) and
4.4e-6 / 1.3e-6 (d target); DESIGN.md section 7 has the table."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TYPES = ("iou", "giou")
QUANT = ("loss", "g_pred", "g_target")
SIZES = (1, 64, 65, 255, 256, 257, 1000)  # the wave edge, the block edge and its tail
MARGIN = 4.0
CANARY = -1234.5


def dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


_runs = {}


def run_none(golden, tag, lt, n=None):
    """IouLoss('none', lt) on the first n rows of boxes.<tag>, gradient of .sum() (cached):
    (loss, d pred, d target) as numpy arrays."""
    if (tag, lt, n) not in _runs:
        from yolox_amd.models import IouLoss
        d = golden("iou_loss.npz")
        p, t = dev(d[f"boxes.{tag}.pred"][:n], True), dev(d[f"boxes.{tag}.target"][:n], True)
        loss = IouLoss(reduction="none", loss_type=lt)(p, t)
        loss.sum().backward()
        torch.cuda.synchronize()
        _runs[tag, lt, n] = tuple(v.detach().cpu().numpy() for v in (loss, p.grad, t.grad))
    return _runs[tag, lt, n]


def measure(x, f64, q, scale64=None):
    """max abs for the loss, max abs over max |fp64| (of scale64 when given) for a gradient."""
    err = float(np.abs(np.asarray(x, np.float64) - f64).max())
    return err if q == "loss" else err / float(np.abs(f64 if scale64 is None else scale64).max())


def ref_noise(d, lt, q):
    return measure(d[f"boxes.rand.{lt}.f32.{q}"], d[f"boxes.rand.{lt}.f64.{q}"], q)


@pytest.mark.parametrize("lt", TYPES)
def test_random_boxes_within_the_reference_noise(golden, lt):
    d = golden("iou_loss.npz")
    got = run_none(golden, "rand", lt)
    for q, x in zip(QUANT, got):
        noise, err = ref_noise(d, lt, q), measure(x, d[f"boxes.rand.{lt}.f64.{q}"], q)
        print(f"rand {lt} {q}: kernel vs fp64 {err:.3e}, fp32 reference vs fp64 {noise:.3e}")
        assert noise > 0
        assert err <= MARGIN * noise, (q, err, noise)


@pytest.mark.parametrize("lt", TYPES)
def test_edge_table(golden, lt):
    d = golden("iou_loss.npz")
    names = [str(n) for n in d["boxes.edge.names"]]
    got = run_none(golden, "edge", lt)
    for q, x in zip(QUANT, got):
        f64, f32 = d[f"boxes.edge.{lt}.f64.{q}"], d[f"boxes.edge.{lt}.f32.{q}"]
        assert np.isfinite(x).all() and np.isfinite(f32).all()
        err = measure(x, f64, q)
        print(f"edge {lt} {q}: kernel vs fp64 {err:.3e} (bound {MARGIN * ref_noise(d, lt, q):.3e})")
        assert err <= MARGIN * ref_noise(d, lt, q), (q, err)
        if q != "loss":
            # every gradient that is exactly 0 in the fp32 reference is exactly 0
            bad = [(names[i], j) for i, j in zip(*np.nonzero((f32 == 0) & (x != 0)))]
            assert not bad, bad
    # the tie rows: torch.max / torch.min hand each side half.  Any other split of a tied edge moves
    # that row's gradient by a share of order 1 of its size; 1e-3 of the row's own max is far above
    # the fp32 noise and far below that.
    gp, gt = got[1], got[2]
    for i, n in enumerate(names):
        if n.startswith(("identical", "shared_")):
            for x, q in ((gp, "g_pred"), (gt, "g_target")):
                f64 = d[f"boxes.edge.{lt}.f64.{q}"][i]
                assert np.abs(x[i] - f64).max() <= 1e-3 * np.abs(f64).max(), (n, q, x[i], f64)
        if n.startswith("identical"):  # the two sides of a full tie get the same bits
            assert np.array_equal(gp[i], gt[i]), n
            assert gp[i][0] == 0 and gp[i][1] == 0


@pytest.mark.parametrize("n", SIZES)
def test_sizes_cut_from_the_fixture(golden, n):
    """The first n rows: each row's result does not depend on n (bit-equal to the 1000-row run), so
    the full set's bound holds for every cut; sum and mean agree with the fp64 sum of the kernel's
    own per-row losses to fp32 rounding (2^-23 relative: the fp64 partials are rounded to fp32 once,
    and the mean once more by its fp32 division by n)."""
    from yolox_amd.models import IouLoss
    d = golden("iou_loss.npz")
    for lt in TYPES:
        full, cut = run_none(golden, "rand", lt), run_none(golden, "rand", lt, n)
        for q, a, b in zip(QUANT, cut, full):
            assert a.shape[0] == n
            assert np.array_equal(a, b[:n]), (lt, q)
            f64 = d[f"boxes.rand.{lt}.f64.{q}"]
            assert measure(a, f64[:n], q, f64) <= MARGIN * ref_noise(d, lt, q)
        p, t = dev(d["boxes.rand.pred"][:n]), dev(d["boxes.rand.target"][:n])
        want = float(cut[0].astype(np.float64).sum())
        s = IouLoss("sum", lt)(p, t)
        m = IouLoss("mean", lt)(p, t)
        assert s.shape == () and m.shape == () and s.dtype == torch.float32
        assert abs(s.item() - want) <= 2.0 ** -23 * abs(want), (lt, n, s.item(), want)
        assert abs(m.item() - want / n) <= 2.0 ** -23 * abs(want / n), (lt, n, m.item(), want / n)


def test_second_reduction_pass_sees_many_partials(golden):
    """N = 65 537 (257 blocks, so the single-block pass strides over more than 256 partials): sum
    and mean against the fp64 sum of the kernel's own per-row output, to fp32 rounding; two runs of
    every reduction are bit-identical."""
    from yolox_amd.models import IouLoss
    d = golden("iou_loss.npz")
    n = 65537
    p = dev(np.tile(d["boxes.rand.pred"], (66, 1))[:n])
    t = dev(np.tile(d["boxes.rand.target"], (66, 1))[:n])
    for lt in TYPES:
        rows = IouLoss("none", lt)(p, t)
        want = float(rows.double().sum().item())
        s, m = IouLoss("sum", lt)(p, t), IouLoss("mean", lt)(p, t)
        assert abs(s.item() - want) <= 2.0 ** -23 * abs(want), (lt, s.item(), want)
        assert abs(m.item() - want / n) <= 2.0 ** -23 * abs(want / n), (lt, m.item(), want / n)
        assert m.item() == pytest.approx(float(rows.double().mean().item()), rel=2.0 ** -23)
        assert torch.equal(rows, IouLoss("none", lt)(p, t))
        assert torch.equal(s, IouLoss("sum", lt)(p, t)) and torch.equal(m, IouLoss("mean", lt)(p, t))


@pytest.mark.parametrize("lt", TYPES)
def test_empty_input(lt):
    from yolox_amd.models import IouLoss
    p = torch.zeros(0, 4, device="cuda", requires_grad=True)
    t = torch.zeros(0, 4, device="cuda")
    none = IouLoss("none", lt)(p, t)
    assert none.shape == (0,) and none.dtype == torch.float32
    s = IouLoss("sum", lt)(p, t)
    assert s.shape == () and s.item() == 0.0
    assert torch.isnan(IouLoss("mean", lt)(p, t)).item()  # torch: the mean of nothing
    s.backward()
    assert p.grad.shape == (0, 4)


@pytest.mark.parametrize("red", ["none", "sum", "mean"])
@pytest.mark.parametrize("lt", TYPES)
def test_backward_with_upstream_gradient(golden, lt, red):
    """loss.backward() with a non-unit upstream gradient (per row for none, 3.5 for sum and mean),
    on a [2, 500, 4] pred that is a strided slice of wider storage and a target whose storage is
    4 bytes off 16-byte alignment; target.requires_grad on and off.  Bound: 4 x the fp32
    reference's noise with the same upstream weights applied to both references."""
    from yolox_amd.models import IouLoss
    d = golden("iou_loss.npz")
    n = 1000
    rng = np.random.default_rng(5)
    w = rng.uniform(0.5, 2.0, n).astype(np.float32) if red == "none" else np.full(n, 3.5, np.float32)
    scale = w.astype(np.float64) / (n if red == "mean" else 1)
    wide = torch.zeros(2, 500, 6, device="cuda")
    wide[..., :4] = dev(d["boxes.rand.pred"]).view(2, 500, 4)
    flat = torch.zeros(4 * n + 1, device="cuda")
    flat[1:] = dev(d["boxes.rand.target"]).view(-1)
    grads = {}
    for tgrad in (True, False):
        p = wide[..., :4].detach().requires_grad_()
        t = flat[1:].view(2, 500, 4).detach().requires_grad_(tgrad)
        assert not p.is_contiguous() and t.data_ptr() % 16 == 4
        loss = IouLoss(red, lt)(p, t)
        assert loss.shape == ((n,) if red == "none" else ())
        (loss * dev(w)).sum().backward() if red == "none" else (loss * 3.5).backward()
        assert p.grad.shape == (2, 500, 4)
        assert (t.grad is not None) == tgrad
        grads[tgrad] = (p.grad.cpu().numpy().reshape(n, 4), t.grad.cpu().numpy().reshape(n, 4) if tgrad else None)
    assert np.array_equal(grads[True][0], grads[False][0])  # g_target null changes nothing else
    for q, x in zip(("g_pred", "g_target"), grads[True]):
        f64 = d[f"boxes.rand.{lt}.f64.{q}"] * scale[:, None]
        f32 = d[f"boxes.rand.{lt}.f32.{q}"].astype(np.float64) * scale[:, None]
        noise, err = measure(f32, f64, q), measure(x, f64, q)
        print(f"{lt} {red} {q}: kernel {err:.3e}, weighted fp32 reference {noise:.3e}")
        assert err <= MARGIN * noise, (q, err, noise)


@pytest.mark.parametrize("lt", TYPES)
def test_16bit_inputs_are_upcast(golden, lt):
    from yolox_amd.models import IouLoss
    d = golden("iou_loss.npz")
    m = IouLoss("none", lt)
    for dt in (torch.bfloat16, torch.float16):
        p = dev(d["boxes.rand.pred"][:257]).to(dt).requires_grad_()
        t = dev(d["boxes.rand.target"][:257]).to(dt)
        out = m(p, t)
        assert out.dtype == dt
        p32 = p.detach().float().requires_grad_()
        want = m(p32, t.float())
        assert torch.equal(out, want.to(dt))
        out.float().sum().backward()
        want.sum().backward()
        assert p.grad.dtype == dt and torch.equal(p.grad, p32.grad.to(dt))
    with pytest.raises(ValueError):
        m(dev(d["boxes.rand.pred"]).double(), dev(d["boxes.rand.target"]).double())


@pytest.mark.parametrize("n", [257, 1000])
def test_canaries_stay_untouched(golden, n):
    """Through the C ABI: 16 bytes in front of and 256 bytes behind out, g_pred and g_target keep
    their fill for every type and reduction, and results equal the module's."""
    from yolox_amd import _native as N
    d = golden("iou_loss.npz")
    lib, st = N.lib(), torch.cuda.current_stream().cuda_stream
    p, t = dev(d["boxes.rand.pred"][:n]), dev(d["boxes.rand.target"][:n])
    go = torch.ones(n, device="cuda")
    ws = torch.empty(int(lib.yxh_iou_loss_workspace_bytes(n)) // 8 + 1, dtype=torch.float64, device="cuda")

    def guarded(k):
        return torch.full((4 + k + 64,), CANARY, device="cuda")

    def intact(buf, k):
        return bool((buf[:4] == CANARY).all() and (buf[4 + k:] == CANARY).all() and (buf[4:4 + k] != CANARY).all())

    for lt in TYPES:
        want = run_none(golden, "rand", lt, n)
        for red in (N.REDUCE_NONE, N.REDUCE_SUM, N.REDUCE_MEAN):
            k = n if red == N.REDUCE_NONE else 1
            out = guarded(k)
            N.check(lib.yxh_iou_loss(p.data_ptr(), t.data_ptr(), n, N.IOU_LOSS_CODE[lt], red, out.data_ptr() + 16,
                                     ws.data_ptr(), ws.numel() * 8, st))
            assert intact(out, k), (lt, red)
            if red == N.REDUCE_NONE:
                assert np.array_equal(out[4:4 + n].cpu().numpy(), want[0])
            for with_t in (True, False):
                gp, gt = guarded(4 * n), guarded(4 * n)
                N.check(lib.yxh_iou_loss_bwd(p.data_ptr(), t.data_ptr(), n, N.IOU_LOSS_CODE[lt], red, go.data_ptr(),
                                             gp.data_ptr() + 16, gt.data_ptr() + 16 if with_t else None, st))
                assert intact(gp, 4 * n), (lt, red)
                if with_t:
                    assert intact(gt, 4 * n), (lt, red)
                else:
                    assert bool((gt == CANARY).all())
                if red == N.REDUCE_NONE:
                    assert np.array_equal(gp[4:4 + 4 * n].cpu().numpy().reshape(n, 4), want[1])
                    if with_t:
                        assert np.array_equal(gt[4:4 + 4 * n].cpu().numpy().reshape(n, 4), want[2])
    # a misaligned row pointer is refused, not read
    assert lib.yxh_iou_loss(p.data_ptr() + 4, t.data_ptr(), n - 1, 0, 0, ws.data_ptr(), None, 0, st) == N.EINVAL
    assert b"16-byte" in lib.yxh_last_error()
    with pytest.raises(ValueError, match="workspace"):
        N.check(lib.yxh_iou_loss(p.data_ptr(), t.data_ptr(), n, 0, N.REDUCE_SUM, ws.data_ptr(), ws.data_ptr(), 0, st))
