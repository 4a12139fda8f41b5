"""The judge of tests/conv_exact.py judged on the CPU: sound on a correct stand-in device, and sensitive to
the slips a conv kernel can make.

The stand-in device is torch fp32 on the same operands (fp32 conv2d, F.silu, one rounding to the destination
dtype).  Soundness: it passes every check at every geometry and dtype.  Sensitivity: each planted slip is
rejected, and by the check named here -- some slips are below the per-element bound in fp16 and only the RMS
check sees them.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_exact as ce

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
GEOMS = [  # cin, cout, k, stride, H, W
    (128, 128, 3, 1, 20, 22), (64, 96, 3, 2, 17, 15), (256, 64, 1, 1, 9, 11), (512, 512, 3, 1, 12, 14),
    (32, 32, 3, 1, 37, 45)]
B = 2


def operands(cin, cout, k, H, W, dtype, seed, stride=1):
    """What a kernel would be handed: NHWC input in the compute dtype, folded weights [cout][k][k][cin] in the
    compute dtype, fp32 bias, and a residual at the output size"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, cin, generator=g).to(dtype)
    w = (torch.randn(cout, k, k, cin, generator=g) / (cin * k * k) ** 0.5).to(dtype)
    b = torch.randn(cout, generator=g) * 0.3
    pad = (k - 1) // 2
    oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    r = torch.randn(B, oh, ow, cout, generator=g).to(dtype)
    return x, w, b, r


def conv32(x, w, b, stride, pad):
    """fp32 pre-activation [B, oh, ow, cout] of the stand-in device"""
    w4 = w.float().permute(0, 3, 1, 2)
    return F.conv2d(x.float().permute(0, 3, 1, 2), w4, b, stride, pad).permute(0, 2, 3, 1)


def stand_in(x, w, b, stride, pad, dtype, residual=None):
    y = F.silu(conv32(x, w, b, stride, pad))
    if residual is not None:
        y = y + residual.float()
    return y.to(dtype)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16", "f32"])
def test_sound_on_the_fp32_stand_in(dtype, geom, residual):
    cin, cout, k, s, H, W = geom
    pad = (k - 1) // 2
    x, w, b, r = operands(cin, cout, k, H, W, dtype, seed=cin + cout + H, stride=s)
    res = r if residual else None
    z, y, S = ce.reference(x, w, b, k, s, pad, "silu", residual=res)
    tol = ce.tolerance(z, y, S, k * k * cin, "silu", dtype, added=residual)
    ref32 = ce.reference32(x, w, b, k, s, pad, "silu", dtype, residual=res)
    got = stand_in(x, w, b, s, pad, dtype, res)
    ratio, rms = ce.judge(got, y, tol, dtype, ref32=ref32, label=str(geom))
    print(f"{geom} {dtype} residual={residual}: per-element {ratio:.3f}, rms {rms}")
    assert ratio <= 1.0
    assert dtype == torch.float32 or rms <= 1.05
    # a different fp32 summation order (the K halves summed apart) moves neither
    zs = conv32(x[..., :cin // 2], w[..., :cin // 2], None, s, pad) + conv32(x[..., cin // 2:], w[..., cin // 2:],
                                                                            b, s, pad)
    got2 = (F.silu(zs) + (res.float() if residual else 0)).to(dtype)
    ratio2, rms2 = ce.judge(got2, y, tol, dtype, ref32=ref32, label=str(geom))
    assert ratio2 <= 1.0 and (dtype == torch.float32 or abs(rms2 - rms) < 1e-3)


# ---------------------------------------------------------------- the planted slips
CIN = COUT = 128
H, W = 20, 22


def trunc(t, dtype):
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero)"""
    assert dtype == torch.bfloat16
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(dtype)


def slip_channel_dropped(x, w, b, r, dt):
    z = conv32(x, w, b, 1, 1)
    x1 = torch.zeros_like(x)
    x1[1, 7:10, 4:7, 17] = x[1, 7:10, 4:7, 17]  # channel 17 as output pixel (1, 8, 5) sees it
    z[1, 8, 5] -= conv32(x1, w, None, 1, 1)[1, 8, 5]
    return (F.silu(z) + r.float()).to(dt)


def slip_partial_16bit(x, w, b, r, dt):
    h = CIN // 2
    part = conv32(x[..., h:], w[..., h:], None, 1, 1).to(dt).float()  # the exchanged partial, in 16 bits
    return (F.silu(conv32(x[..., :h], w[..., :h], b, 1, 1) + part) + r.float()).to(dt)


def slip_double_rounding(x, w, b, r, dt):
    return (F.silu(conv32(x, w, b, 1, 1)).to(dt).float() + r.float()).to(dt)


def slip_silu_of_rounded(x, w, b, r, dt):
    return (F.silu(conv32(x, w, b, 1, 1).to(dt).float()) + r.float()).to(dt)


def slip_bias_rounded(x, w, b, r, dt):
    return (F.silu(conv32(x, w, b.to(dt).float(), 1, 1)) + r.float()).to(dt)


def slip_truncation(x, w, b, r, dt):
    return trunc(F.silu(conv32(x, w, b, 1, 1)) + r.float(), dt)


def slip_border_tap_dropped(x, w, b, r, dt):
    z = conv32(x, w, b, 1, 1)
    w1 = torch.zeros_like(w)
    w1[:, 1, 2] = w[:, 1, 2]  # tap (ky 1, kx 2) at the left border pixel (0, 6, 0)
    z[0, 6, 0] -= conv32(x, w1, None, 1, 1)[0, 6, 0]
    return (F.silu(z) + r.float()).to(dt)


def slip_next_image_as_padding(x, w, b, r, dt):
    xp = F.pad(x.float(), (0, 0, 1, 1, 1, 1))  # [B, H + 2, W + 2, C]
    xp[0, H + 1, 1:W + 1] = x[1, 0].float()  # image 0's bottom padding row = image 1's first row
    z = conv32(xp, w, b, 1, 0)
    return (F.silu(z) + r.float()).to(dt)


def slip_residual_shifted(x, w, b, r, dt):
    return (F.silu(conv32(x, w, b, 1, 1)) + torch.roll(r.float(), 1, dims=2)).to(dt)


SLIPS = {
    "channel_dropped": slip_channel_dropped, "partial_16bit": slip_partial_16bit,
    "double_rounding": slip_double_rounding, "silu_of_rounded": slip_silu_of_rounded,
    "bias_rounded": slip_bias_rounded, "truncation": slip_truncation,
    "border_tap_dropped": slip_border_tap_dropped, "next_image_as_padding": slip_next_image_as_padding,
    "residual_shifted": slip_residual_shifted}
# which check must reject which slip.  bf16: the per-element bound rejects every one.  fp16: the bias rounded
# to 16 bits stays below both checks (0.59x the tolerance, 1-3 % of the RMS) and truncation below the
# per-element bound (0.92x; its RMS ratio unmeasured), so neither is asserted there; the three intermediate
# roundings must be rejected by the RMS check (whatever the per-element bound makes of them).
BF16_PER_ELEMENT = sorted(SLIPS)
F16_PER_ELEMENT = ["channel_dropped", "border_tap_dropped", "next_image_as_padding", "residual_shifted"]
F16_RMS = ["partial_16bit", "double_rounding", "silu_of_rounded"]


_CASE = {}


def case(dtype):
    if dtype not in _CASE:
        x, w, b, r = operands(CIN, COUT, 3, H, W, dtype, seed=7)
        z, y, S = ce.reference(x, w, b, 3, 1, 1, "silu", residual=r)
        tol = ce.tolerance(z, y, S, 9 * CIN, "silu", dtype, added=True)
        ref32 = ce.reference32(x, w, b, 3, 1, 1, "silu", dtype, residual=r)
        _CASE[dtype] = (x, w, b, r, y, tol, ref32)
    return _CASE[dtype]


def test_slip_case_is_sound_without_a_slip():
    for dtype in (torch.bfloat16, torch.float16):
        x, w, b, r, y, tol, ref32 = case(dtype)
        ratio, rms = ce.judge(stand_in(x, w, b, 1, 1, dtype, r), y, tol, dtype, ref32=ref32)
        assert ratio <= 1.0 and rms <= 1.05


@pytest.mark.parametrize("slip", BF16_PER_ELEMENT)
def test_bf16_per_element_bound_rejects(slip):
    dtype = torch.bfloat16
    x, w, b, r, y, tol, ref32 = case(dtype)
    got = SLIPS[slip](x, w, b, r, dtype)
    ratio, at = ce.element_ratio(got, y, tol)
    print(f"bf16 {slip}: per-element {ratio:.3f} at {at}, rms {ce.rms_ratio(got, y, ref32):.4f}")
    assert ratio > 1.0
    with pytest.raises(ce.PerElementError, match="x the tolerance at"):
        ce.judge(got, y, tol, dtype, ref32=ref32, label=slip)


@pytest.mark.parametrize("slip", F16_PER_ELEMENT)
def test_f16_per_element_bound_rejects(slip):
    dtype = torch.float16
    x, w, b, r, y, tol, ref32 = case(dtype)
    got = SLIPS[slip](x, w, b, r, dtype)
    ratio, at = ce.element_ratio(got, y, tol)
    print(f"f16 {slip}: per-element {ratio:.3f} at {at}, rms {ce.rms_ratio(got, y, ref32):.4f}")
    assert ratio > 1.0
    with pytest.raises(ce.PerElementError):
        ce.judge(got, y, tol, dtype, ref32=ref32, label=slip)


@pytest.mark.parametrize("slip", F16_RMS)
def test_f16_rms_check_rejects(slip):
    dtype = torch.float16
    x, w, b, r, y, tol, ref32 = case(dtype)
    got = SLIPS[slip](x, w, b, r, dtype)
    rms = ce.rms_ratio(got, y, ref32)
    print(f"f16 {slip}: per-element {ce.element_ratio(got, y, tol)[0]:.3f}, rms {rms:.4f}")
    assert rms > 1.05
    with pytest.raises((ce.RmsError, ce.PerElementError)):
        ce.judge(got, y, tol, dtype, ref32=ref32, label=slip)
    # and by the RMS check alone: with the per-element bound out of the way it is the one that raises
    with pytest.raises(ce.RmsError, match="above 1.05"):
        ce.judge(got, y, torch.full_like(tol, float("inf")), dtype, ref32=ref32, label=slip)


@pytest.mark.parametrize("slip", ["partial_16bit", "double_rounding", "channel_dropped"])
def test_bf16_rms_check_rejects_too(slip):
    """The ratios that set the 5 %: 1.099 (16-bit partial), 1.22 (double rounding), >= 1.25 (a dropped channel)"""
    dtype = torch.bfloat16
    x, w, b, r, y, tol, ref32 = case(dtype)
    rms = ce.rms_ratio(SLIPS[slip](x, w, b, r, dtype), y, ref32)
    print(f"bf16 {slip}: rms {rms:.4f}")
    assert rms > 1.05


def test_poison_and_guards():
    dtype = torch.bfloat16
    x, w, b, r, y, tol, ref32 = case(dtype)
    got = stand_in(x, w, b, 1, 1, dtype, r)
    bad = got.clone()
    bad[1, 3, 4, 5] = float("nan")
    with pytest.raises(ce.PoisonError, match=r"\(1, 3, 4, 5\)"):
        ce.judge(bad, y, tol, dtype, ref32=ref32)
    guard = torch.full((4096,), 0x7A5C, dtype=torch.int16)
    ce.judge(got, y, tol, dtype, ref32=ref32, guards=[("tail", guard, 0x7A5C)])
    guard[17] = 0x7A5D
    with pytest.raises(ce.GuardError, match="tail"):
        ce.judge(got, y, tol, dtype, ref32=ref32, guards=[("tail", guard, 0x7A5C)])


@pytest.mark.parametrize("act", ["none", "relu", "lrelu"])
def test_other_activations_sound(act):
    for dtype in DTYPES:
        x, w, b, _ = operands(64, 80, 3, 13, 19, dtype, seed=3)
        z, y, S = ce.reference(x, w, b, 3, 1, 1, act)
        tol = ce.tolerance(z, y, S, 9 * 64, act, dtype)
        ref32 = ce.reference32(x, w, b, 3, 1, 1, act, dtype)
        z32 = conv32(x, w, b, 1, 1)
        got = {"none": z32, "relu": F.relu(z32), "lrelu": F.leaky_relu(z32, 0.1)}[act].to(dtype)
        ratio, rms = ce.judge(got, y, tol, dtype, ref32=ref32)
        assert ratio <= 1.0


def test_accumulate_into_fp32_destination():
    dtype = torch.bfloat16
    x, w, b, _ = operands(64, 48, 3, 9, 11, dtype, seed=5)
    base = torch.randn(B, 9, 11, 48, generator=torch.Generator().manual_seed(6))
    z, y, S = ce.reference(x, w, b, 3, 1, 1, "none", accumulate_into=base)
    tol = ce.tolerance(z, y, S, 9 * 64, "none", torch.float32, added=True)
    got = conv32(x, w, b, 1, 1) + base
    ratio, rms = ce.judge(got, y, tol, torch.float32)
    assert ratio <= 1.0 and rms is None
    with pytest.raises(ce.PerElementError):  # the prefilled destination overwritten instead of added to
        ce.judge(conv32(x, w, b, 1, 1), y, tol, torch.float32)
