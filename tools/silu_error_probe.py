"""The error of the 16-bit SiLU paths of the training step, measured on the kernels themselves against float64:
the two constants FAST_SILU_FWD / FAST_SILU_GRAD of tests/train_exact.py (which records the result).

  forward   yxh_bn_act_fwd with y = 0, scale = 0 and shift = z hands the activation any fp32 z.  The output is
            rounded to 16 bits, so the fp32 value v behind it is only known to lie within half a spacing of it:
            |v - silu(z)| >= |out - silu(z)| - spacing(out) / 2, and the maximum of that over millions of z -- some
            always sit next to a rounding boundary -- is the measurement, in units of u |silu(z)|, u = 2**-24.
  gradient  yxh_bn_act_bwd over ONE pixel with dout = 1: dbeta = act_grad(z) comes back in fp32, unrounded.
            In units of u * sigmoid(z) * (1 + |z|).
z: uniform in [-20, 20] plus a dense stretch around 0.
Usage: python tools/silu_error_probe.py [millions of z for the forward, default 4]"""
import ctypes as C
import sys

import torch

sys.path.insert(0, "pixeltable-yolox_amd")
from yolox_amd import _native as N  # noqa: E402

U32 = 2.0 ** -24
MANT = {torch.float16: 10, torch.bfloat16: 7}
MIN_NORMAL = {torch.float16: 2.0 ** -14, torch.bfloat16: 2.0 ** -126}


def draw(n, g):
    z = torch.rand(n, generator=g) * 40 - 20
    z[: n // 8] = torch.rand(n // 8, generator=g) * 2 - 1
    return z.to(torch.float32)


def view(t, c):
    s = N.Src()
    s.ptr, s.channels, s.cstride, s.bstride, s.h, s.w = t.data_ptr(), c, c, c, 1, 1
    return s


def stats_of(z):
    st = torch.zeros(4, z.numel())
    st[1], st[3] = 1.0, z
    return st.cuda()


def forward(dtype, n, g, lib, stream):
    z = draw(n, g)
    st, y, out = stats_of(z), torch.zeros(n, dtype=dtype, device="cuda"), torch.empty(n, dtype=dtype, device="cuda")
    ys, os_ = view(y, n), view(out, n)
    N.check(lib.yxh_bn_act_fwd(N.DTYPE_CODE[dtype], 1, C.byref(ys), st.data_ptr(), N.ACT_CODE["silu"], None,
                               C.byref(os_), stream))
    torch.cuda.synchronize()
    got, z64 = out.cpu().double(), z.double()
    want = z64 * torch.sigmoid(z64)
    big = torch.maximum(got.abs(), want.abs()).clamp_min(MIN_NORMAL[dtype])
    spacing = torch.ldexp(torch.ones_like(big), torch.frexp(big)[1] - 1 - MANT[dtype])
    e = ((got - want).abs() - spacing / 2).clamp_min(0) / (U32 * want.abs())
    e = torch.where(want.abs() >= MIN_NORMAL[dtype], e, torch.zeros_like(e))
    i = int(e.argmax())
    return float(e[i]), float(z[i])


def gradient(dtype, n, g, lib, stream, ws):
    z = draw(n, g)
    st, y = stats_of(z), torch.zeros(n, dtype=dtype, device="cuda")
    dout = torch.ones(n, device="cuda")
    dg, db, dx = torch.empty(n, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, dtype=dtype, device="cuda")
    ys, gs = view(y, n), view(dout, n)
    N.check(lib.yxh_bn_act_bwd(N.DTYPE_CODE[dtype], 1, C.byref(ys), C.byref(gs), st.data_ptr(), None,
                               N.ACT_CODE["silu"], dg.data_ptr(), db.data_ptr(), dx.data_ptr(), ws.data_ptr(),
                               ws.numel(), stream))
    torch.cuda.synchronize()
    z64 = z.double()
    s = torch.sigmoid(z64)
    e = (db.cpu().double() - s * (1 + z64 * (1 - s))).abs() / (U32 * s * (1 + z64.abs()))
    i = int(e.argmax())
    return float(e[i]), float(z[i])


def main():
    millions = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    lib, stream = N.lib(), N.stream_ptr(torch.device("cuda"))
    g = torch.Generator().manual_seed(0)
    nb = 1 << 15
    ws = torch.empty(int(lib.yxh_reduce_workspace_bytes(nb)), dtype=torch.uint8, device="cuda")
    for dtype in (torch.float16, torch.bfloat16):
        fwd = max(forward(dtype, 1 << 20, g, lib, stream) for _ in range(millions))
        bwd = max(gradient(dtype, nb, g, lib, stream, ws) for _ in range(32))
        print(f"{dtype}: forward {fwd[0]:.3f} u |silu(z)| at z = {fwd[1]:.6g} over {millions << 20} z; "
              f"gradient {bwd[0]:.3f} u s (1 + |z|) at z = {bwd[1]:.6g} over {32 * nb} z", flush=True)


if __name__ == "__main__":
    main()
