"""Per-element judge of a forward convolution against a float64 reference of the device's own operands.

`close()` of test_gpu_ops.py compares with torch fp32 on the unrounded input and the unfolded weights, so its
bound has to absorb operand rounding and the BN fold.  Here the reference starts from what the kernel reads --
the input as rounded to the compute dtype, the folded weights and the fp32 bias yxh_fold_bn_pack wrote -- so
what is left is the kernel's own arithmetic, and every term of the bound is derived:

  accumulation   c * (K + 2) * u32 * S     fp32 FMA chains in any order and any K split, plus the bias add;
                                           S = conv(|x|, |w|) + |b|, K = kh * kw * cin, c = 1.1 >= sup |silu'|
                                           (1 for none / relu / lrelu, whose slopes are <= 1)
  SiLU           (2 |z| + 6) * u32 * |silu(z)|
                                           yxh_common.hpp: v * rcp(1 + exp2(v * -log2e)).  The rounded constant
                                           and the product put 2 |z| u32 into the exponent; v_exp_f32 and
                                           v_rcp_f32 are 1 ulp each (2 u32 each), the add and the final multiply
                                           half an ulp each: 2 + 2 + 1 + 1 = 6
  add            u32 * |y|                 the residual / accumulate add (only where there is one)
  output         u_out * |y| + half the smallest subnormal of the destination dtype

All tensors are NHWC ([B, H, W, C]), as the kernels hold them.  Plain module: no GPU, no fixtures.
"""
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
HALF_SUBNORMAL = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -150}
RMS_SLACK = 1.05  # rms(got - y) <= RMS_SLACK * rms(ref32 - y), 16-bit destinations


class PerElementError(AssertionError):
    pass


class RmsError(AssertionError):
    pass


class PoisonError(AssertionError):
    pass


class GuardError(AssertionError):
    pass


def _act(z, act):
    if act == "silu":
        return z * torch.sigmoid(z)
    if act == "relu":
        return torch.relu(z)
    if act == "lrelu":
        return torch.where(z >= 0, z, z * 0.1)
    if act == "none":
        return z
    raise ValueError(f"act {act}")


def unpack_weight(w_packed, cout, k, cin):
    """[cout][kh][kw][cin_pad] as yxh_fold_bn_pack wrote it -> [cout, cin, kh, kw] (torch's layout)"""
    w = w_packed.detach().cpu().reshape(cout, k, k, -1)
    assert w.shape[3] >= cin, (w.shape, cin)
    return w[..., :cin].permute(0, 3, 1, 2).contiguous()


def _conv(x, w, bias, stride, pad, dt):
    return F.conv2d(x.to(dt).permute(0, 3, 1, 2), w.to(dt), None if bias is None else bias.to(dt), stride, pad)


def reference(x, w_packed, bias, k, stride, pad, act, residual=None, accumulate_into=None):
    """float64 from the device's operands.  x [B, H, W, cin] in the compute dtype, w_packed the folded weights
    [cout][k][k][cin_pad], bias fp32 [cout]; residual / accumulate_into [B, oh, ow, cout].
    -> z (pre-activation), y (after activation, residual, accumulate), S (sum of absolute products + |b|)."""
    x = x.detach().cpu()
    bias = bias.detach().cpu()
    w = unpack_weight(w_packed, bias.numel(), k, x.shape[3])
    f64 = torch.float64
    z = _conv(x, w, bias, stride, pad, f64).permute(0, 2, 3, 1).contiguous()
    S = _conv(x.to(f64).abs(), w.to(f64).abs(), bias.to(f64).abs(), stride, pad, f64).permute(0, 2, 3, 1).contiguous()
    y = _act(z, act)
    for add in (residual, accumulate_into):
        if add is not None:
            y = y + add.detach().cpu().to(f64)
    return z, y, S


def reference32(x, w_packed, bias, k, stride, pad, act, out_dtype, residual=None):
    """The reference's own error for the RMS check: torch fp32 conv2d + activation (+ residual) on the same
    operands, rounded once to the destination dtype; returned in float64."""
    x = x.detach().cpu()
    bias = bias.detach().cpu()
    w = unpack_weight(w_packed, bias.numel(), k, x.shape[3])
    f32 = torch.float32
    z = _conv(x, w, bias, stride, pad, f32).permute(0, 2, 3, 1)
    y = F.silu(z) if act == "silu" else _act(z, act)
    if residual is not None:
        y = y + residual.detach().cpu().to(f32)
    return y.to(out_dtype).to(torch.float64)


def tolerance(z, y, S, K, act, out_dtype, added=False):
    """Per-element bound on |got - y| (module docstring).  added: a residual or accumulate add follows."""
    c = 1.1 if act == "silu" else 1.0
    tol = c * (K + 2) * U32 * S
    if act == "silu":
        tol = tol + (2 * z.abs() + 6) * U32 * _act(z, "silu").abs()
    if added:
        tol = tol + U32 * y.abs()
    return tol + U_OUT[out_dtype] * y.abs() + HALF_SUBNORMAL[out_dtype]


def element_ratio(got, y, tol):
    """-> (worst |got - y| / tol, its index (b, y, x, c)); NaN in got counts as infinite"""
    r = (got.detach().cpu().to(torch.float64) - y).abs() / tol
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    i = int(r.argmax())
    idx = []
    for n in reversed(r.shape):
        idx.append(i % n)
        i //= n
    return float(r.max()), tuple(reversed(idx))


def rms_ratio(got, y, ref32):
    e = (got.detach().cpu().to(torch.float64) - y).square().mean().sqrt().item()
    e32 = (ref32 - y).square().mean().sqrt().item()
    return e / e32 if e32 > 0 else (0.0 if e == 0 else float("inf"))


def judge(got, y, tol, out_dtype, ref32=None, guards=(), label=""):
    """The four checks.  got: the destination slice [B, oh, ow, cout]; y, tol from reference / tolerance;
    ref32 from reference32 (16-bit destinations: required); guards: (name, tensor, canary tensor or scalar)
    whose elements must be bit-identical.  -> (per-element ratio, RMS ratio or None)."""
    got = got.detach().cpu()
    assert got.shape == y.shape, (got.shape, y.shape)
    if torch.isnan(got).any():
        bad = torch.isnan(got).nonzero()
        raise PoisonError(f"{label}: {len(bad)} NaN in the output, first at (b, y, x, c) = {tuple(bad[0].tolist())}")
    for name, t, canary in guards:
        same = t == canary
        if not bool(same.all()):
            bad = (~same).nonzero()
            raise GuardError(f"{label}: {len(bad)} guard elements of {name} overwritten, first at "
                             f"{tuple(bad[0].tolist())}")
    ratio, at = element_ratio(got, y, tol)
    if not ratio <= 1.0:
        raise PerElementError(f"{label}: |got - y| = {ratio:.3f} x the tolerance at (b, y, x, c) = {at}: got "
                              f"{float(got[at]):.9g}, want {float(y[at]):.9g}, tolerance {float(tol[at]):.3g}")
    rms = None
    if out_dtype != torch.float32:
        assert ref32 is not None, "a 16-bit destination needs ref32"
        rms = rms_ratio(got, y, ref32)
        if not rms <= RMS_SLACK:
            raise RmsError(f"{label}: rms(got - y) = {rms:.4f} x rms(ref32 - y), above {RMS_SLACK}")
    return ratio, rms
