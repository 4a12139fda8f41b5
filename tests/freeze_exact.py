"""Judge of the two kernels a frozen (eval-mode) BatchNorm adds to the training step (csrc/train_bn.hip), per element
against float64, next to train_exact.py and on its constants, views, guarded buffers and judge.

yxh_bn_frozen_stats   stats[4][C] = mean, invstd, scale, shift from the RUNNING statistics:
      mean   = running_mean                                     bit equality (a copy)
      invstd = 1 / sqrt(running_var + eps)                      ULPS["invstd"]: the double result's one conversion
      scale  = gamma * invstd                                   ULPS["scale"]
      shift  = beta - mean * scale                              ULPS["shift_product"] ulp(mean * scale) + ULPS["shift"]
  the bars train_exact.ULPS states for yxh_bn_stats' same operations after its (here absent) reduction.  eps enters
  the reference as the float the kernel is handed.

yxh_bn_frozen_act_bwd dx = dout * act'(z) * scale, z = y * scale + shift, from the stats table it is handed:
      e_z   = u (2 |y scale| + |shift|)                         train_exact._z
      e_g   = silu: G u s (1 + |z|) + e_z / 2, G = SILU32_GRAD in fp32, FAST_SILU_GRAD in 16 bits (|z| <= 20
              asserted: the range of that measurement); lrelu / none: 0, an lrelu element with |z| <= e_z has no
              defined side and is left out (at most AMBIGUOUS_CAP of a case, checked on the CPU for every case)
      e_dz  = |dout| e_g + u |dz|                               the product dout * act'
      tol   = |scale| e_dz + u |dx| + u_out |dx| + half a subnormal of dtype     the product with scale, the store
  No reduction: nothing depends on the launch shape.

Plain module: no GPU, no fixtures.
"""
import torch

import train_exact as te
from train_exact import F64, U32, U_OUT, HALF_SUBNORMAL  # noqa: F401

ACTS = (te.ACT_SILU, te.ACT_LRELU, te.ACT_NONE)
CHANNELS = (1, 8, 20, 24, 80, 256)  # one lane's tail, the chunk boundary, yolox_x's odd widths, many chunks
PIXELS = {1: (1, 1, 1), 35: (5, 1, 7), 400: (4, 10, 10)}  # B * H * W -> (B, H, W): more than one image each
VIEW_NAMES = ("dense", "slice", "padded")


def cases(dt):
    """every te.BN case of one dtype: C x pixels x act x view"""
    return [te.BN(C, *PIXELS[m], (dt,), act, view=view)
            for C in CHANNELS for m in PIXELS for act in ACTS for view in VIEW_NAMES]


_OPS = {}


def operands(case, dt):
    """CPU operands, drawn once: y [B, H, W, C] in the compute dtype, dout fp32, stats fp32 [4][C] (rows 2 and 3,
    scale and shift, are what the kernel reads; scale takes both signs)"""
    key = (case, dt)
    if key not in _OPS:
        g = torch.Generator().manual_seed(977 * case.C + 13 * case.M + case.act)
        shape, C = (case.B, case.H, case.W, case.C), case.C
        y = (torch.randn(shape, generator=g) * 1.5).to(te.DTYPES[dt])
        dout = torch.randn(shape, generator=g)
        sign = torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
        scale = (torch.rand(C, generator=g) + 0.5) * sign
        shift = torch.randn(C, generator=g) * 0.5
        stats = torch.stack([torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5, scale, shift])
        _OPS[key] = dict(y=y, dout=dout, stats=stats.to(torch.float32))
    return _OPS[key]


def act_bwd_reference(y, dout, stats, act, dtype):
    """-> dict: dx [B, H, W, C] float64, tol, judged, ambiguous (module docstring)"""
    v, st, z, e_z = te._z(y, stats)
    g = te._rows(dout)
    scale = st[2]
    dz = g * te.act_grad64(z, act)
    dx = dz * scale
    judged = torch.ones_like(z, dtype=torch.bool)
    if act == te.ACT_SILU:
        assert dtype == torch.float32 or float(z.abs().max()) <= te.FAST_SILU_RANGE
        s = torch.sigmoid(z)
        e_g = (te.SILU32_GRAD if dtype == torch.float32 else te.FAST_SILU_GRAD) * U32 * s * (1 + z.abs()) + e_z / 2
    else:
        e_g = torch.zeros_like(z)
        if act in (te.ACT_RELU, te.ACT_LRELU):
            judged = z.abs() > e_z
    e_dz = g.abs() * e_g + U32 * dz.abs()
    tol = scale.abs() * e_dz + U32 * dx.abs() + U_OUT[dtype] * dx.abs() + HALF_SUBNORMAL[dtype]
    return dict(dx=dx.reshape(y.shape), tol=tol.reshape(y.shape), judged=judged.reshape(y.shape),
                ambiguous=1.0 - float(judged.to(F64).mean()))


# ---------------------------------------------------------------------------------------------- frozen statistics
STATS_CASES = [(1, 1, 1), (20, 1, 0), (24, 0, 1), (256, 0, 0), (1280, 1, 1)]  # C, gamma given, beta given


def stats_operands(C, has_gamma, has_beta):
    g = torch.Generator().manual_seed(5000 + C)
    rvar = torch.rand(C, generator=g) * 4
    rvar[0] = 0.0  # invstd = 1 / sqrt(eps)
    if C > 1:
        rvar[1] = 1e-12  # lost against eps 1e-3 in fp32, kept in the double sum
    return dict(rmean=torch.randn(C, generator=g) * 3, rvar=rvar,
                gamma=torch.rand(C, generator=g) + 0.5 if has_gamma else None,
                beta=torch.randn(C, generator=g) * 0.5 if has_beta else None)


def stats_reference(o, eps=te.EPS):
    """-> (stats [4][C] float64, tol [4][C]; row 0, the mean, is compared bit for bit: its bound is 0)"""
    eps = te.f32_value(eps)
    mean, var = o["rmean"].to(F64), o["rvar"].to(F64)
    C = mean.numel()
    invstd = 1 / torch.sqrt(var + eps)
    g = torch.ones(C, dtype=F64) if o["gamma"] is None else o["gamma"].to(F64)
    b = torch.zeros(C, dtype=F64) if o["beta"] is None else o["beta"].to(F64)
    scale = g * invstd
    ms = mean * scale
    shift = b - ms
    tol = torch.stack([torch.zeros(C, dtype=F64), te.ULPS["invstd"] * te.ulp(invstd), te.ULPS["scale"] * te.ulp(scale),
                       te.ULPS["shift_product"] * te.ulp(ms) + te.ULPS["shift"] * te.ulp(shift)])
    return torch.stack([mean, invstd, scale, shift]), tol
