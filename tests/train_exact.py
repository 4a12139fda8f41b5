"""Judge of the training step's non-MFMA kernels -- BatchNorm statistics / forward / backward and the channel sum
(csrc/train_bn.hip), the depthwise gradients (csrc/train_dw.hip), SPP and upsample backward (csrc/train_bwd.hip) --
against float64 references written from the operation, next to conv_exact.py and grad_exact.py and reusing their
error classes, guarded buffers and per-element judges.  A tensor-wide max-norm is never the criterion.

Two operand modes, as in grad_exact.py:

  grid            every operand is k / 8 with |k| <= 16.  Whatever is a pure sum of operands, or of products of two
                  operands, is then a sum of multiples of 1 / 64 that every order of summation gets exactly, and must
                  equal the float64 reference bit for bit: channel_sum, the batch mean (the shifted sums
                  sum(v - v0) and sum((v - v0)**2), (v - v0)**2 <= 16 = 1024 / 64, are exact for M <= 16384 rows and
                  the mean is one rounding of an exact double), dbeta with act 0, both depthwise gradients, upsample
                  backward and SPP backward.  grid_sum_exact() / assert_grid_exact() are the preconditions,
                  asserted per case.  On grid planes an SPP window of 169 pixels holds at most 33 distinct values:
                  ties are the rule, and only the first maximum in row-major scan order gives the reference's bits.
  full mantissa   randn rounded to the compute dtype, judged per element against a bound derived from the operation
                  count.  u = 2**-24 (half an fp32 ulp, relative), ulp(x) the fp32 spacing at the float64 value x.

Reductions (chan_reduce + chan_finalize).  A channel's rows are split over blocks of rpb rows and, inside a block,
over rpi row lanes (red_plan() / row_lanes() restate the launch arithmetic).  One fp32 chain is a lane's
ceil(rpb / rpi) rows followed by the rpi lanes; the blocks are summed in double.  So a sum of terms t_i carries at
most
      chain * u * sum|t_i|,        chain = ceil(rpb / rpi) + rpi     (+ the roundings of t_i itself)
Statistics, with v0 the channel's first pixel, S1 = sum|v - v0|, S2 = sum (v - v0)**2, m1 = mean - v0:
      e1    = (chain + 1) * u * S1 / M                     (+1: the subtraction v - v0)
      e_var = (chain + 3) * u * S2 / M + 2 |m1| e1 + e1**2  (+3: the subtraction twice and the square)
      r     = e_var / (var + eps),  invstd's relative error from the sums = r / 2 * (1 + r)   (r < 1 / 2 asserted)
What follows the double arithmetic of chan_finalize is a handful of float conversions and multiplies, each half an
ulp; counted in whole ulps of the float64 value (ULPS below):
      mean     1   one conversion                       invstd  1   one conversion
      scale    2   invstd's conversion, one multiply
      shift    4 ulp(mean * scale) + 1 ulp(shift)       mean's conversion (1/2), scale (1 1/2), the product (1/2),
                                                         the ulp's own factor-of-two wobble; then the subtraction
      running  2 ulp((1 - mo) * old) + 2 ulp(mo * new) + 1 ulp(result)
                                                         1 - mo and its product; the conversion and its product; the add
On grid operands the sums are exact and these ulps are the whole bound (the mean: bit equality).  eps and the
momentum enter the reference as the floats the kernel is handed.

Forward, from the device's own scale / shift (the statistics are judged on their own):
      z = v * scale + shift         e_z = u * (2 |v * scale| + |shift|)    two roundings, or one FMA
      out = act(z) (+ res)          tol = lip * e_z + e_act + [u |out| for the residual add] + u_out |out|
                                          + half the smallest subnormal of the destination
      lip = 1.1 >= sup |silu'|, 1 otherwise.  e_act: none / relu 0; lrelu u |out| (the product with 0.1f); silu in
      fp32 (expf, IEEE divide) 8 u |silu(z)|: expf within 3 ulp (OpenCL C's bound for exp, which the device
      library is built to) damped by E / (1 + E) <= 1, the add, the divide; silu in 16 bits FAST_SILU_FWD u |silu(z)|.

Backward.  dz = dout * act'(z), dbeta = sum dz, dgamma = sum dz * xhat, xhat = (v - mean) * invstd,
dx = k1 * dz + k2 * (v - mean) + k3, k1 = gamma * invstd, k2 = -k1 * invstd * dgamma / M, k3 = -k1 * dbeta / M.
      e_g   = silu: G u s (1 + |z|) + e_z / 2, s = sigmoid(z): |d silu' / ds| <= 1 + |z|, |silu''| <= 1 / 2;
              G = 12 in fp32 (s: 8 u as above; 1 - s, the two products, the add) and FAST_SILU_GRAD in 16 bits.
              relu / lrelu: 0, but an element with |z| <= e_z has no defined side: it is left out of dx's
              judgement (AMBIGUOUS_CAP: at most 0.1 % of a case) and enters dbeta / dgamma with
              |dout| * (1 - slope) (* |xhat|) instead
      e_dz  = |dout| e_g + u |dz|
      dbeta   sum e_dz + chain u sum|dz| + 1 ulp
      dgamma  sum (e_dz |xhat| + 3 u |dz xhat|) + chain u sum|dz xhat| + 1 ulp     (3: v - mean, * invstd, * dz)
      dx      |k1| e_dz + |v - mean| |k1 invstd| tol_dgamma / M + |k1| tol_dbeta / M
              + u (4 |k1 dz| + 9 |k2 (v - mean)| + 6 |k3|) + u_out |dx| + half a subnormal
              k1: one product; k2: four more and 1 / M; k3: two more and 1 / M; v - mean; the three terms' two adds
channel_sum   chain u sum|x| + 1 ulp.

Depthwise gradients and their full-mantissa bound, grad_exact.tolerance: (K + 2) u S [+ u |y| onto a prefill],
K the summed products (the output pixels for dw, 9 taps for dx), S the same gradient of the absolute values.

The two constants that no reading of the code gives are the errors of the 16-bit activation paths,
z / (1.0f + __expf(-z)) in bn_act_fwd and act_grad<false> (__expf and __builtin_amdgcn_rcpf); the ROCm tree holds
no device-library document stating them.  tools/silu_error_probe.py measured the kernels themselves on an
MI355X over z in [-20, 20] against float64 (2026-10-21, ROCm 7, gfx950):
      forward   max (|out - silu(z)| - half the 16-bit spacing at out) / (u |silu(z)|) over 4 194 304 z:
                14.12 with bf16 outputs (at z = -18.69), 11.13 with f16 outputs (at z = -11.65)
      gradient  max |dbeta - silu'(z)| / (u s (1 + |z|)) over one pixel with dout = 1, 1 048 576 z:
                15.98 (f16 operands, at z = -19.45), 15.70 (bf16, at z = -17.96)
The error grows with |z| (the exponent's argument is a rounded product), so the figures hold for |z| <= 20 only:
the references assert that of every 16-bit SiLU case.  With a margin of 2x, rounded up: FAST_SILU_FWD = 29,
FAST_SILU_GRAD = 32, i.e. 2**-19 relative -- 1 / 256 of half an ulp of f16 (2**-11), 1 / 2048 of bf16's.  They are
constants of this file, never computed from an output under judgement.

All tensors are NHWC.  Plain module: no GPU, no fixtures (the buffers allocate on the device they are given).
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from conv_exact import GuardError, HALF_SUBNORMAL, PerElementError, PoisonError, U32, U_OUT  # noqa: F401
from grad_exact import GUARD, Guarded, Workspace, assert_grid_exact, check_guards, first_index, grid, judge_exact  # noqa: F401,E501

F64 = torch.float64
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
EPC = {torch.float32: 4, torch.bfloat16: 8, torch.float16: 8}  # elements of a 16-byte chunk
ACT_NONE, ACT_SILU, ACT_RELU, ACT_LRELU = 0, 1, 2, 3
LRELU_SLOPE = float(torch.tensor(0.1, dtype=torch.float32))  # the kernel's 0.1f
FAST_SILU_FWD = 29.0   # measured 14.12 (module docstring), margin 2x
FAST_SILU_GRAD = 32.0  # measured 15.98, margin 2x
FAST_SILU_RANGE = 20.0  # |z| of the measurement
SILU32_FWD, SILU32_GRAD = 8.0, 12.0
AMBIGUOUS_CAP = 1e-3
ULPS = dict(mean=1, invstd=1, scale=2, shift_product=4, shift=1, running_old=2, running_new=2, running=1)
EPS, MOMENTUM = 1e-3, 0.03  # the BatchNorm settings of every YOLOX config


def f32_value(v):
    """the double value of v as a C float argument"""
    return float(torch.tensor(v, dtype=torch.float32))


def ulp(x):
    """fp32 spacing at the float64 values x (that of the smallest normal below it)"""
    e = torch.frexp(x.abs().clamp_min(2.0 ** -126))[1] - 1  # |x| in [2**e, 2**(e + 1))
    return torch.ldexp(torch.ones_like(x), e - 23)


def grid_sum_exact(n, max_term):
    """n terms, multiples of 1 / 64 of magnitude <= max_term, sum exactly in fp32 in any order"""
    assert max_term * n * 64 <= 2 ** 24, f"{n} terms of {max_term} leave the exact regime"


# ---------------------------------------------------------------------------------------------- launch arithmetic
RED_CAP = 512  # chan_reduce blocks per channel group (the library's default)


def red_plan(M, C, dtype):
    """red_blocks() of train_bn.hip restated: -> (blocks = partials per channel, rows per block)"""
    nch = C // EPC[dtype]
    rpi = 1 if nch >= 256 else 256 // nch
    nblk = max(1, min(RED_CAP, (M + rpi * 8 - 1) // (rpi * 8)))
    rpb = (M + nblk - 1) // nblk
    return (M + rpb - 1) // rpb, rpb


def row_lanes(C, dtype):
    """chan_reduce's row lanes per channel: [C] (each group of 256 chunks has its own count)"""
    per = 256 * EPC[dtype]
    out = torch.empty(C, dtype=torch.int64)
    for c0 in range(0, C, per):
        cl = min(C - c0, per)
        out[c0:c0 + cl] = 256 // (cl // EPC[dtype])
    return out


def chain(M, C, dtype):
    """-> [C] float64: the longest fp32 summation chain behind a channel's reduction"""
    _, rpb = red_plan(M, C, dtype)
    rpi = row_lanes(C, dtype)
    return ((rpb + rpi - 1) // rpi + rpi).to(F64)


def spp_cpb(H, W):
    """spp_bwd_launch's channels per block: 24 bytes of LDS per channel and pixel, 160 KiB"""
    hw = H * W
    return 4 if hw * 4 * 24 <= 160 * 1024 else 2 if hw * 2 * 24 <= 160 * 1024 else 1


DW_BLOCK = 4096  # dw_wgrad's output pixels per block


def dw_nsplit(B, oh, ow):
    return (B * oh * ow + DW_BLOCK - 1) // DW_BLOCK


# ---------------------------------------------------------------------------------------------- activations
def act64(z, act):
    if act == ACT_SILU:
        return z * torch.sigmoid(z)
    if act == ACT_RELU:
        return torch.where(z > 0, z, torch.zeros_like(z))
    if act == ACT_LRELU:
        return torch.where(z > 0, z, z * LRELU_SLOPE)
    assert act == ACT_NONE, act
    return z


def act_grad64(z, act):
    if act == ACT_SILU:
        s = torch.sigmoid(z)
        return s * (1 + z * (1 - s))
    if act == ACT_RELU:
        return (z > 0).to(F64)
    if act == ACT_LRELU:
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, LRELU_SLOPE))
    assert act == ACT_NONE, act
    return torch.ones_like(z)


def _rows(t):
    t = t.detach().cpu().to(F64)
    return t.reshape(-1, t.shape[-1])


# ---------------------------------------------------------------------------------------------- BatchNorm references
def bn_stats_reference(y, gamma=None, beta=None, rmean=None, rvar=None, eps=EPS, momentum=MOMENTUM):
    """Training-mode BatchNorm2d statistics of y [B, H, W, C] (compute dtype), float64.  gamma / beta fp32 [C] or
    None (1 / 0); rmean / rvar the running statistics before the step, or None.  The running variance takes the
    unbiased batch variance (M == 1, where torch refuses: the biased one, as the kernel does).
    -> dict: M, mean, var, invstd, scale, shift, stats [4][C], rmean, rvar, and the companion sums S1, S2, m1"""
    x = _rows(y)
    M, C = x.shape
    eps, mo = f32_value(eps), f32_value(momentum)
    mean = x.mean(0)
    var = (x - mean).square().mean(0)
    invstd = 1 / torch.sqrt(var + eps)
    g = torch.ones(C, dtype=F64) if gamma is None else gamma.detach().cpu().to(F64)
    b = torch.zeros(C, dtype=F64) if beta is None else beta.detach().cpu().to(F64)
    scale = g * invstd
    shift = b - mean * scale
    d = x - x[0]
    r = dict(M=M, C=C, eps=eps, mo=mo, mean=mean, var=var, invstd=invstd, scale=scale, shift=shift, beta=b,
             stats=torch.stack([mean, invstd, scale, shift]), S1=d.abs().sum(0), S2=d.square().sum(0),
             m1=mean - x[0], rmean=None, rvar=None)
    if rmean is not None:
        r["rmean_old"], r["rvar_old"] = rmean.detach().cpu().to(F64), rvar.detach().cpu().to(F64)
        r["unbiased"] = var * M / (M - 1) if M > 1 else var
        r["rmean"] = (1 - mo) * r["rmean_old"] + mo * mean
        r["rvar"] = (1 - mo) * r["rvar_old"] + mo * r["unbiased"]
    return r


def bn_stats_tolerance(r, chain_len=None):
    """-> dict of per-channel bounds on mean, invstd, scale, shift (and rmean, rvar) (module docstring).
    chain_len None: grid operands, exact sums (the mean's bound is then unused: it is compared bit for bit)"""
    M, mean, scale, invstd = r["M"], r["mean"], r["scale"], r["invstd"]
    zero = torch.zeros_like(mean)
    if chain_len is None:
        e1, e_var = zero, zero
    else:
        e1 = (chain_len + 1) * U32 * r["S1"] / M
        e_var = (chain_len + 3) * U32 * r["S2"] / M + 2 * r["m1"].abs() * e1 + e1 * e1
    rr = e_var / (r["var"] + r["eps"])
    assert float(rr.max()) < 0.5, "the variance's bound leaves the first-order regime"
    rel = rr / 2 * (1 + rr)
    ms = mean * scale
    t = dict(mean=e1 + ULPS["mean"] * ulp(mean),
             invstd=invstd * rel + ULPS["invstd"] * ulp(invstd),
             scale=scale.abs() * rel + ULPS["scale"] * ulp(scale),
             shift=scale.abs() * e1 + ms.abs() * rel + ULPS["shift_product"] * ulp(ms) + ULPS["shift"] * ulp(r["shift"]))
    if r["rmean"] is not None:
        mo = r["mo"]
        for key, new, e_new in (("rmean", mean, e1), ("rvar", r["unbiased"], e_var * (M / (M - 1) if M > 1 else 1))):
            t[key] = (mo * e_new + ULPS["running_old"] * ulp((1 - mo) * r[key + "_old"])
                      + ULPS["running_new"] * ulp(mo * new) + ULPS["running"] * ulp(r[key]))
    t["stats"] = torch.stack([t["mean"], t["invstd"], t["scale"], t["shift"]])
    return t


def _z(y, stats):
    """-> v [M, C], scale, shift, z, e_z from the fp32 statistics the kernel reads"""
    v = _rows(y)
    st = stats.detach().cpu().to(F64).reshape(4, -1)
    z = v * st[2] + st[3]
    return v, st, z, U32 * (2 * (v * st[2]).abs() + st[3].abs())


def bn_act_fwd_reference(y, stats, act, res, out_dtype):
    """out = act(y * scale + shift) (+ res) from the device's stats [4][C] (fp32).  y, res [B, H, W, C] in the
    compute dtype.  -> (out float64 [B, H, W, C], tol)"""
    v, st, z, e_z = _z(y, stats)
    o = act64(z, act)
    assert act != ACT_SILU or out_dtype == torch.float32 or float(z.abs().max()) <= FAST_SILU_RANGE
    e_act = {ACT_NONE: 0.0, ACT_RELU: 0.0, ACT_LRELU: U32 * o.abs(),
             ACT_SILU: (SILU32_FWD if out_dtype == torch.float32 else FAST_SILU_FWD) * U32 * o.abs()}[act]
    tol = (1.1 if act == ACT_SILU else 1.0) * e_z + e_act
    if res is not None:
        o = o + _rows(res)
        tol = tol + U32 * o.abs()
    tol = tol + U_OUT[out_dtype] * o.abs() + HALF_SUBNORMAL[out_dtype]
    return o.reshape(y.shape), tol.reshape(y.shape)


def bn_act_bwd_reference(y, dout, stats, gamma, act, dtype, chain_len):
    """Backward of act(BN(y)) from the device's stats [4][C].  y [B, H, W, C] in `dtype`, dout fp32, gamma fp32 [C]
    or None.  -> dict: dgamma, dbeta [C], dx [B, H, W, C] float64, their bounds tol_*, `judged` (the dx elements
    with a defined side) and `ambiguous` (the share without)"""
    v, st, z, e_z = _z(y, stats)
    M, C = v.shape
    mean, invstd = st[0], st[1]
    g = _rows(dout)
    gam = torch.ones(C, dtype=F64) if gamma is None else gamma.detach().cpu().to(F64)
    dz = g * act_grad64(z, act)
    xhat = (v - mean) * invstd
    dbeta, dgamma = dz.sum(0), (dz * xhat).sum(0)
    k1 = gam * invstd
    A, Bt, Ct = k1 * dz, -k1 * invstd * dgamma / M * (v - mean), (-k1 * dbeta / M).expand(M, C)
    dx = A + Bt + Ct
    judged = torch.ones_like(z, dtype=torch.bool)
    if act == ACT_SILU:
        assert dtype == torch.float32 or float(z.abs().max()) <= FAST_SILU_RANGE
        s = torch.sigmoid(z)
        e_g = (SILU32_GRAD if dtype == torch.float32 else FAST_SILU_GRAD) * U32 * s * (1 + z.abs()) + e_z / 2
    else:
        e_g = torch.zeros_like(z)
        if act in (ACT_RELU, ACT_LRELU):
            judged = z.abs() > e_z
            e_g = torch.where(judged, e_g, torch.full_like(z, 1.0 if act == ACT_RELU else 1 - LRELU_SLOPE))
    e_dz = g.abs() * e_g + U32 * dz.abs()
    tol_db = e_dz.sum(0) + chain_len * U32 * dz.abs().sum(0) + ulp(dbeta)
    tol_dg = ((e_dz * xhat.abs() + 3 * U32 * (dz * xhat).abs()).sum(0) + chain_len * U32 * (dz * xhat).abs().sum(0)
              + ulp(dgamma))
    tol_dx = (k1.abs() * e_dz + (v - mean).abs() * (k1 * invstd).abs() * tol_dg / M + k1.abs() * tol_db / M
              + U32 * (4 * A.abs() + 9 * Bt.abs() + 6 * Ct.abs()) + U_OUT[dtype] * dx.abs() + HALF_SUBNORMAL[dtype])
    return dict(dgamma=dgamma, dbeta=dbeta, dx=dx.reshape(y.shape), tol_dgamma=tol_dg, tol_dbeta=tol_db,
                tol_dx=tol_dx.reshape(y.shape), judged=judged.reshape(y.shape),
                ambiguous=1.0 - float(judged.to(F64).mean()))


def channel_sum_reference(x, chain_len):
    """-> (sum over pixels [C] float64, tol, S = the same sum of absolute values)"""
    v = _rows(x)
    y, S = v.sum(0), v.abs().sum(0)
    return y, chain_len * U32 * S + ulp(y), S


# ---------------------------------------------------------------------------------------------- depthwise gradients
def _dw_out(n, s):
    return (n + 2 - 3) // s + 1


def _dw_wgrad64(x, dy, s):
    B, H, W, C = x.shape
    _, oh, ow, _ = dy.shape
    assert (oh, ow) == (_dw_out(H, s), _dw_out(W, s)), (x.shape, dy.shape)
    xp = F.pad(x, (0, 0, 1, 1 + s, 1, 1 + s))
    dw = torch.empty(C, 3, 3, dtype=F64)
    for ky in range(3):
        for kx in range(3):
            dw[:, ky, kx] = torch.einsum("bhwc,bhwc->c", dy, xp[:, ky:ky + s * oh:s, kx:kx + s * ow:s, :])
    return dw


def dw_wgrad_reference(x, dy, s):
    """Weight gradient of the depthwise 3x3 stride-s pad-1 conv.  x [B, H, W, C], dy [B, oh, ow, C] in the compute
    dtype -> (dw [C][3][3] float64, S the same gradient of the absolute values)"""
    x, dy = x.detach().cpu().to(F64), dy.detach().cpu().to(F64)
    return _dw_wgrad64(x, dy, s), _dw_wgrad64(x.abs(), dy.abs(), s)


def _dw_dgrad64(dy, w, s, H, W):
    B, oh, ow, C = dy.shape
    assert (oh, ow) == (_dw_out(H, s), _dw_out(W, s)), (dy.shape, H, W)
    dxp = torch.zeros(B, H + 2 + s, W + 2 + s, C, dtype=F64)  # padded row iy + 1 = oy * s + ky
    for ky in range(3):
        for kx in range(3):
            dxp[:, ky:ky + s * oh:s, kx:kx + s * ow:s, :] += dy * w[:, ky, kx]
    return dxp[:, 1:1 + H, 1:1 + W, :].contiguous()


def dw_dgrad_reference(dy, w, s, H, W):
    """Data gradient.  dy [B, oh, ow, C], w [C][3][3], both in the compute dtype -> (dx [B, H, W, C] float64, S)"""
    dy, w = dy.detach().cpu().to(F64), w.detach().cpu().to(F64).reshape(-1, 3, 3)
    return _dw_dgrad64(dy, w, s, H, W), _dw_dgrad64(dy.abs(), w.abs(), s, H, W)


# ---------------------------------------------------------------------------------------------- SPP / upsample backward
SPP_KS = (5, 9, 13)


def spp_argmax(x, k, last=False):
    """For every output pixel of max_pool2d(k, stride 1, pad k // 2) over the planes x [B, H, W, c] (float64): the
    flat index y * W + x of the FIRST maximum in a row-major scan of the window clipped to the plane.  The scan
    is the explicit double loop over the window's rows and columns, taken for all output pixels at once; a later
    candidate wins only if strictly greater.  (last=True: the planted fault, the last maximum.)"""
    B, H, W, c = x.shape
    r = k // 2
    xp = F.pad(x, (0, 0, r, r, r, r), value=-math.inf)
    best = torch.full_like(x, -math.inf)
    arg = torch.full(x.shape, -1, dtype=torch.int64)
    oy, ox = torch.arange(H).view(1, H, 1, 1), torch.arange(W).view(1, 1, W, 1)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            v = xp[:, r + dy:r + dy + H, r + dx:r + dx + W, :]
            win = (v >= best) & (v > -math.inf) if last else v > best
            best = torch.where(win, v, best)
            arg = torch.where(win, ((oy + dy) * W + (ox + dx)).expand_as(arg), arg)
    assert int(arg.min()) >= 0
    return arg, best


def spp_bwd_reference(x, dcat, last=False):
    """SPPBottleneck's concat + max-pool backward.  x [B, H, W, c] (the pooled input, compute dtype), dcat
    [B, H, W, 4c] fp32 (identity, k = 5, 9, 13) -> dx [B, H, W, c] float64"""
    x, g = x.detach().cpu().to(F64), dcat.detach().cpu().to(F64)
    B, H, W, c = x.shape
    dx = g[..., :c].reshape(B, H * W, c).clone()
    for n, k in enumerate(SPP_KS):
        arg, _ = spp_argmax(x, k, last)
        dx.scatter_add_(1, arg.view(B, H * W, c), g[..., (n + 1) * c:(n + 2) * c].reshape(B, H * W, c))
    return dx.view(B, H, W, c)


def upsample_bwd_reference(g, dst):
    """nearest x2 backward: dst [B, h, w, C] + the 2x2 block sums of g [B, 2h, 2w, C]"""
    g, dst = g.detach().cpu().to(F64), dst.detach().cpu().to(F64)
    B, h, w, C = dst.shape
    return dst + g.view(B, h, 2, w, 2, C).sum((2, 4))


# ---------------------------------------------------------------------------------------------- the judge
def judge(got, y, tol, guards=(), label="", judged=None):
    """Per element: |got - y| <= tol wherever `judged` (default: everywhere); no NaN anywhere; the guards keep their
    canary.  -> the worst |got - y| / tol"""
    got = got.detach().cpu()
    assert got.shape == y.shape == tol.shape, (got.shape, y.shape, tol.shape)
    bad = ~torch.isfinite(got.to(F64))
    if bool(bad.any()):
        raise PoisonError(f"{label}: {int(bad.sum())} non-finite values in the output, first at {first_index(bad)}")
    check_guards(guards, label)
    r = (got.to(F64) - y).abs() / tol
    if judged is not None:
        r = torch.where(judged, r, torch.zeros_like(r))
    if not bool((r <= 1.0).all()):
        at = first_index(r == r.max()) if r.dim() else ()
        raise PerElementError(f"{label}: |got - y| = {float(r.max()):.3f} x the bound at {at}: got "
                              f"{float(got[at]):.9g}, want {float(y[at]):.9g}, bound {float(tol[at]):.3g} "
                              f"({int((r > 1).sum())} of {r.numel()} elements out)")
    return float(r.max()) if r.numel() else 0.0


class ViewBuf(Guarded):
    """B images of H x W pixels as the trainer's views hold them: channels [off, off + ch) of rows ch + idle wide
    (a slice of a concat buffer) and pad_rows idle pixel rows after every image (bstride > h * w * cstride: vofs
    then splits (b, pix)); GUARD elements before and after.  fill as Guarded: NaN for inputs, canary for outputs."""

    def __init__(self, B, H, W, ch, dtype, device, off=0, idle=0, pad_rows=0, fill="canary"):
        super().__init__((B, H * W + pad_rows), ch, dtype, device, off=off, idle=idle, fill=fill)
        self.B, self.H, self.W, self.pad_rows = B, H, W, pad_rows
        self.live = self.view[:, :H * W, off:off + ch]

    def set(self, value):
        self.live.copy_(value.to(self.flat.device, self.flat.dtype).reshape(self.B, self.H * self.W, self.ch))
        return self

    def get(self):
        return self.live.reshape(self.B, self.H, self.W, self.ch).cpu()

    cstride = property(lambda self: self.cw)
    bstride = property(lambda self: (self.H * self.W + self.pad_rows) * self.cw)

    def outside(self, name):
        assert self.canary is not None, "NaN-filled input buffers have no canary"
        bits = self.bits.clone()
        bits[GUARD:GUARD + self.n].view(*self.rows, self.cw)[:, :self.H * self.W, self.off:self.off + self.ch] \
            .fill_(self.canary)
        return (name, bits.cpu(), self.canary)


# ---------------------------------------------------------------------------------------------- cases
# Shared by tests/test_gpu_train_exact.py and tests/test_train_exact_checker.py, which checks on the CPU that every
# case meets the conditions it is judged under.
ALL, F32_ONLY, HALVES = ("f32", "bf16", "f16"), ("f32",), ("bf16", "f16")
VIEWS = {"dense": (0, 0, 0), "slice": (16, 32, 0), "padded": (16, 32, 3)}  # channel offset, idle channels, pad rows

BN = namedtuple("BN", "C B H W dts act gamma beta running res view edge", defaults=(ALL, 1, 1, 1, 1, 1, "dense", 0))
BN.M = property(lambda self: self.B * self.H * self.W)
BN.id = property(lambda self: "-".join(str(v) for v in self if not isinstance(v, tuple)))


def _bn_cases():
    cases = []
    n = 0
    # channel counts whose chunk count does not divide 256 (yolox_nano 24, yolox_m 48 / 96 / 192, yolox_x 80 /
    # 160 / 320), with every act, gamma / beta NULL together and apart, running stats and residual on and off
    for C in (24, 48, 80, 96, 160, 192, 320):
        for B, H, W in ((2, 7, 5), (3, 10, 7)):
            gamma, beta = ((1, 1), (0, 0), (1, 0), (0, 1))[(n // 4) % 4]
            cases.append(BN(C, B, H, W, ALL, n % 4, gamma, beta, 1 - (n // 2) % 2, int(n % 3 == 0),
                            ("dense", "slice", "padded")[n % 3]))
            n += 1
    # the second channel group (more than 256 chunks)
    cases += [BN(1280, 2, 3, 3, F32_ONLY), BN(2560, 2, 3, 3, HALVES)]
    # many rows at few channels: the unrolled row loop, its tail, many row lanes
    cases += [BN(32, 2, 64, 64)]
    # the cap on reduction blocks: more than 448 partials per channel reach chan_finalize's eighth chain
    cases += [BN(1024, 1, 65, 64, F32_ONLY, res=0), BN(2048, 1, 65, 64, HALVES, res=0)]
    # fewer rows than row lanes; M == 1: the biased variance in the running statistics
    cases += [BN(64, 1, 1, 1), BN(64, 1, 1, 2), BN(64, 1, 1, 3)]
    # every act through channel-slice views, images back to back and with padding rows between them
    for act in (ACT_NONE, ACT_SILU, ACT_RELU, ACT_LRELU):
        cases += [BN(64, 3, 10, 7, ALL, act, view="slice"), BN(64, 3, 10, 7, ALL, act, view="padded", running=0)]
    cases += [BN(64, 2, 9, 11, ALL, 1, 0, 0, view="slice"), BN(64, 2, 9, 11, ALL, 3, 1, 0, view="padded", res=0),
              BN(64, 2, 9, 11, ALL, 2, 0, 1, view="slice", running=0)]
    # a constant channel and a channel with |mean| >> std, within one fp32 tensor
    cases += [BN(16, 2, 16, 16, F32_ONLY, edge=1)]
    return cases


BN_CASES = _bn_cases()
CAP_CASES = [c for c in BN_CASES if c.C in (1024, 2048)]
EDGE_CONST, EDGE_SHIFTED = 3, 5  # the edge case's channels
_OPS = {}


def _draw(shape, g, mode, dtype, scale=1.0, offset=0.0):
    if mode == "grid":
        return grid(shape, g).to(dtype)
    return (torch.randn(shape, generator=g) * scale + offset).to(dtype)


def bn_operands(case, dt, mode):
    """CPU operands of (case, dtype name, "grid" | "full"), drawn once: y, res [B, H, W, C] in the compute dtype,
    dout fp32, gamma / beta / rmean / rvar fp32 [C] (None where the case passes NULL)"""
    key = ("bn", case, dt, mode)
    if key not in _OPS:
        dtype = DTYPES[dt]
        g = torch.Generator().manual_seed(31 * case.C + 7 * case.M + case.act)
        shape, C = (case.B, case.H, case.W, case.C), case.C
        if mode == "grid":
            y = _draw(shape, g, mode, dtype)
        else:
            y = (torch.randn(shape, generator=g) * (torch.rand(C, generator=g) * 1.5 + 0.5)
                 + torch.randn(C, generator=g) * 2).to(dtype)
            if case.edge:
                y[..., EDGE_CONST] = 1.7
                y[..., EDGE_SHIFTED] = 1000 + 0.01 * torch.randn(shape[:3], generator=g)
        o = dict(y=y, dout=_draw(shape, g, mode, torch.float32), res=_draw(shape, g, mode, dtype) if case.res else None,
                 gamma=(grid((C,), g) if mode == "grid" else torch.rand(C, generator=g) + 0.5) if case.gamma else None,
                 beta=(grid((C,), g) if mode == "grid" else torch.randn(C, generator=g) * 0.5) if case.beta else None,
                 rmean=torch.randn(C, generator=g) if case.running else None,
                 rvar=torch.rand(C, generator=g) + 0.5 if case.running else None)
        _OPS[key] = o
    return _OPS[key]


# depthwise: B, H, W (conv input), C, stride; dts; dyw = channels of the dy view (>= C, whole chunks);
# full: also judged with full-mantissa operands; wgrad: yxh_dw_wgrad takes it too
DW = namedtuple("DW", "B H W C s dts dyw full wgrad", defaults=(ALL, None, False, True))
DW.oh = property(lambda self: _dw_out(self.H, self.s))
DW.ow = property(lambda self: _dw_out(self.W, self.s))
DW.K = property(lambda self: self.B * self.oh * self.ow)
DW.id = property(lambda self: "-".join(str(v) for v in self[:5]))
DW_CASES = [
    DW(2, 48, 48, 8, 1),                    # 4608 output pixels: two blocks, the last of 512 pixels
    DW(2, 64, 64, 8, 1),                    # 8192: exactly two full blocks
    DW(1, 96, 96, 16, 1),                   # three blocks, the last of 1024 pixels
    DW(2, 96, 96, 8, 2),                    # 4608 output pixels at stride 2: two blocks, the last of 512
    DW(1, 9, 10, 72, 1, full=True),         # C > 64, not a multiple of 64: the c < C guard of the last slice
    DW(2, 8, 8, 100, 2),
    DW(2, 7, 9, 12, 1, HALVES, dyw=16),     # dw_dgrad's c0 + EPC > C tail
    DW(2, 9, 6, 20, 2, HALVES, dyw=24, full=True),
    DW(2, 7, 9, 6, 1, F32_ONLY, dyw=8, full=True),
    DW(2, 11, 13, 16, 2, ALL, dyw=32),      # dy as the first C channels of a 2C-wide view
]


def dw_operands(case, dt, mode):
    """x [B, H, W, C], dy [B, oh, ow, C], w [C][3][3] in the compute dtype, base fp32 (the accumulate form's
    grid-valued destination) and the float64 references dw, dx, their S, y_acc = base + dx"""
    key = ("dw", case, dt, mode)
    if key not in _OPS:
        dtype = DTYPES[dt]
        g = torch.Generator().manual_seed(4000 + 13 * case.H * case.W + case.C + case.s)
        x = _draw((case.B, case.H, case.W, case.C), g, mode, dtype)
        dy = _draw((case.B, case.oh, case.ow, case.C), g, mode, dtype)
        w = _draw((case.C, 3, 3), g, mode, dtype, scale=0.3)
        base = grid((case.B, case.H, case.W, case.C), g)
        dw, Sw = dw_wgrad_reference(x, dy, case.s)
        dx, Sx = dw_dgrad_reference(dy, w, case.s, case.H, case.W)
        y_acc = dx + base.to(F64)
        if mode == "grid":
            assert_grid_exact(dw, case.K)
            assert_grid_exact(dx, 9)
            assert_grid_exact(y_acc, 10)
        _OPS[key] = dict(x=x, dy=dy, w=w, base=base, dw=dw, Sw=Sw, dx=dx, Sx=Sx, y_acc=y_acc)
    return _OPS[key]


# SPP backward: B, H, W, c, idle channels of the cat view past 4c.  Planes at the edge of each rule (narrower than
# the 13-wide window in both directions, in one only, one pixel wider, YOLOX's 20x20); near-square planes that
# spp_bwd_launch gives 2 channels and 1 channel per block, and the areas on both sides of each of its LDS thresholds
# (4 channels up to 1706 pixels, 2 up to 3413, 1 up to 6826, the largest plane it takes); c not a multiple of the
# channels per block
SPP = namedtuple("SPP", "B H W c idle", defaults=(0,))
SPP.id = property(lambda self: "-".join(str(v) for v in self))
SPP_CASES = [SPP(2, 4, 4, 8), SPP(2, 5, 13, 8), SPP(2, 13, 5, 24), SPP(1, 14, 14, 8), SPP(2, 20, 20, 24),
             SPP(2, 9, 7, 6), SPP(1, 20, 20, 8, idle=8), SPP(1, 41, 41, 5), SPP(1, 39, 44, 3), SPP(1, 57, 60, 2),
             SPP(1, 2, 853, 5), SPP(1, 3, 569, 3), SPP(1, 1, 3413, 2), SPP(1, 6, 569, 2), SPP(1, 2, 3413, 1)]
SPP_CPB = {(39, 44): 2, (57, 60): 1, (3, 569): 2, (1, 3413): 2, (6, 569): 1, (2, 3413): 1}  # every other plane: 4


def spp_operands(case, dt):
    """grid planes x [B, H, W, c] in the compute dtype, dcat fp32 [B, H, W, 4c] and dx float64"""
    key = ("spp", case, dt)
    if key not in _OPS:
        g = torch.Generator().manual_seed(600 + case.H * case.W + case.c)
        x = grid((case.B, case.H, case.W, case.c), g).to(DTYPES[dt])
        dcat = grid((case.B, case.H, case.W, 4 * case.c), g)
        dx = spp_bwd_reference(x, dcat)
        grid_sum_exact(1 + sum(k * k for k in SPP_KS), 2.0)  # identity + every output of the three windows
        assert bool((dx.to(torch.float32).to(F64) == dx).all())
        _OPS[key] = dict(x=x, dcat=dcat, dx=dx)
    return _OPS[key]


UPSAMPLE_CASES = [(2, 1, 1, 4), (2, 5, 7, 4), (1, 1, 1, 20), (2, 5, 7, 20)]  # B, h, w, C
