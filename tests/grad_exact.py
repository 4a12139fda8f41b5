"""Judge of the convolution gradient kernels (yxh_conv_wgrad, the data-gradient forms of yxh_conv2d) against
float64 references, next to conv_exact.py and reusing its error classes and per-element judge.

Two operand modes:

  grid            every operand is k / 8 with |k| <= 16 (exact in bf16, f16 and fp32).  A product is a multiple of
                  1 / 64 of magnitude <= 4, so a sum of K of them is a multiple of 1 / 64 of magnitude <= 4 K: with
                  4 * K * 64 <= 2**24 it and every partial sum of it, in any order, is an fp32 number.  MFMA
                  internals, K splits, atomics and the fixed-order reduce then all give the same bits, and a
                  correct kernel equals the float64 reference bit for bit at any such K (assert_grid_exact is the
                  precondition, checked per geometry).
  full mantissa   randn rounded to the compute dtype, judged per element against
                      (K + 2) * u32 * S  [+ u32 * |y| for the add onto a prefill]  + half the smallest subnormal,
                  conv_exact.py's accumulation term with K the number of summed products and S the same
                  gradient of the absolute values.  The bound grows as K * S ~ K**2, so only small-K geometries
                  are judged this way (tests/test_grad_exact_checker.py holds the conditions).

All activations and gradients are NHWC, weights and weight gradients [cout][cin][kh][kw], as the kernels hold them.
Plain module: no GPU, no fixtures (Guarded allocates on the device it is given).
"""
import torch
import torch.nn.functional as F

import conv_exact as ce
from conv_exact import GuardError, PerElementError, PoisonError, U32  # noqa: F401  (one set of error classes)

GUARD = 4096  # elements before and after every guarded slice: a stray access lands in allocated memory
CANARY = {2: 0x7A5C, 4: 0x7A5C7A5C}  # finite in bf16 / fp16 / fp32
GRID_MAX_PRODUCT = 4.0  # (16 / 8) ** 2
HALF_SUBNORMAL32 = ce.HALF_SUBNORMAL[torch.float32]


# ---------------------------------------------------------------------------------------------- operands
def grid(shape, generator):
    """integers in [-16, 16] divided by 8, fp32: exact in bf16 and f16"""
    return torch.randint(-16, 17, tuple(shape), generator=generator).to(torch.float32) / 8


def assert_grid_exact(y64, K, max_product=GRID_MAX_PRODUCT):
    """The precondition of the bit comparison: every reference value is an fp32 number and K products of at most
    max_product, all multiples of 1 / 64, sum exactly in fp32 in any order.  (With a prefill, count it as one more
    product and pass the larger of 4 and its largest magnitude.)"""
    assert bool((y64.to(torch.float32).to(torch.float64) == y64).all()), "a reference value is not an fp32 number"
    assert max_product * K * 64 <= 2 ** 24, f"K = {K} leaves the exact regime: {max_product} * K * 64 > 2**24"


# ---------------------------------------------------------------------------------------------- references
def cat_sources(srcs, dt=torch.float64):
    """[(x [B, h, w, c], upsample), ...] -> the conv input [B, H, W, cin]: nearest x2, concatenation"""
    parts = []
    for x, up in srcs:
        x = x.detach().cpu().to(dt)
        parts.append(x.repeat_interleave(2, 1).repeat_interleave(2, 2) if up else x)
    return torch.cat(parts, 3)


def _wgrad64(x, dy, k, s, p):
    B, H, W, _ = x.shape
    _, oh, ow, _ = dy.shape
    assert oh == (H + 2 * p - k) // s + 1 and ow == (W + 2 * p - k) // s + 1, (x.shape, dy.shape)
    # pad up to what the last tap of the last output pixel reads (torch ignores what is past it, as the conv does)
    xp = F.pad(x, (0, 0, p, p + s, p, p + s))
    dw = torch.empty(dy.shape[3], x.shape[3], k, k, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            xs = xp[:, ky:ky + s * oh:s, kx:kx + s * ow:s, :]
            dw[:, :, ky, kx] = torch.einsum("bhwn,bhwc->nc", dy, xs)
    return dw


def wgrad_reference(srcs, dy, cout, k, s, p, cin_store):
    """float64 weight gradient of the conv over cat(srcs).  srcs [(x, upsample)], dy [B, oh, ow, >= cout] (only the
    first cout channels count).  -> (dW [cout][cin_store][k][k], S the same gradient of the absolute values)"""
    x = cat_sources(srcs)[..., :cin_store]
    g = dy.detach().cpu().to(torch.float64)[..., :cout]
    return _wgrad64(x, g, k, s, p), _wgrad64(x.abs(), g.abs(), k, s, p)


def _dgrad64(dy, w, k, s, in_hw):
    p = (k - 1) // 2
    H, W = in_hw
    _, oh, ow, _ = dy.shape
    assert oh == (H + 2 * p - k) // s + 1 and ow == (W + 2 * p - k) // s + 1, (dy.shape, in_hw)
    op = (H - ((oh - 1) * s - 2 * p + k), W - ((ow - 1) * s - 2 * p + k))
    dx = F.conv_transpose2d(dy.permute(0, 3, 1, 2), w, None, s, p, op)
    assert tuple(dx.shape[2:]) == (H, W)
    return dx.permute(0, 2, 3, 1).contiguous()


def dgrad_reference(dy, w, k, s, in_hw):
    """float64 data gradient (the transposed convolution) of a k x k stride-s conv with pad (k - 1) // 2.
    dy [B, oh, ow, cout] in the compute dtype, w the *unpacked* fp32 weight [cout][cin][k][k], rounded here to
    dy's dtype as yxh_pack_dgrad_weight rounds it.  -> (dx [B, H, W, cin], S of the absolute values)"""
    g = dy.detach().cpu()
    w64 = w.detach().cpu().to(torch.float32).to(g.dtype).to(torch.float64)
    g = g.to(torch.float64)
    return _dgrad64(g, w64, k, s, in_hw), _dgrad64(g.abs(), w64.abs(), k, s, in_hw)


def dgrad_weight_reference(w, c_begin, c_count, cout_pad, dtype):
    """What yxh_pack_dgrad_weight must write: [c_count][kh][kw][cout_pad] in dtype, taps flipped, zeros in
    [cout, cout_pad), one round-to-nearest-even from fp32"""
    w = w.detach().cpu().to(torch.float32)
    cout = w.shape[0]
    out = torch.zeros(c_count, w.shape[2], w.shape[3], cout_pad, dtype=dtype)
    out[..., :cout] = w[:, c_begin:c_begin + c_count].flip(2, 3).permute(1, 2, 3, 0).to(dtype)
    return out


def tolerance(K, S, y=None, added=False):
    """Per-element bound on |got - y| of an fp32 gradient with full-mantissa operands (module docstring)"""
    tol = (K + 2) * U32 * S
    if added:
        tol = tol + U32 * y.abs()
    return tol + HALF_SUBNORMAL32


# ---------------------------------------------------------------------------------------------- the judge
def first_index(mask):
    return tuple(mask.nonzero()[0].tolist())


def judge_exact(got, y, guards=(), label=""):
    """Grid mode: got (fp32) must equal the float64 reference bit for bit (-0.0 and 0.0 are the same gradient).
    guards as in judge_bound.  Raises with the first bad index."""
    got = got.detach().cpu()
    assert got.shape == y.shape, (got.shape, y.shape)
    if torch.isnan(got).any():
        bad = torch.isnan(got)
        raise PoisonError(f"{label}: {int(bad.sum())} NaN in the output, first at {first_index(bad)}")
    check_guards(guards, label)
    bad = got.to(torch.float64) != y
    if bool(bad.any()):
        at = first_index(bad)
        raise PerElementError(f"{label}: {int(bad.sum())} of {bad.numel()} elements differ from the float64 "
                              f"reference, first at {at}: got {float(got[at]):.9g}, want {float(y[at]):.9g}")
    return 0.0


def judge_bound(got, y, tol, guards=(), label=""):
    """Full-mantissa mode: conv_exact.judge on an fp32 destination.  guards: (name, tensor of bits, canary)
    -> the worst |got - y| / tol"""
    return ce.judge(got, y, tol, torch.float32, guards=guards, label=label)[0]


def check_guards(guards, label=""):
    for name, t, canary in guards:
        same = t == canary
        if not bool(same.all()):
            bad = ~same
            raise GuardError(f"{label}: {int(bad.sum())} guard elements of {name} overwritten, first at "
                             f"{first_index(bad)}")


# ---------------------------------------------------------------------------------------------- guarded buffers
def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class Guarded:
    """A slice inside a wider buffer with GUARD elements before and after it.

    Guarded(rows, ch, dtype, device, off=, idle=): `rows` (a shape prefix, e.g. (B, h, w) or ()) of ch + idle
    elements each, the slice being elements [off, off + ch) of every row.  fill "nan" (inputs: a read outside the
    slice poisons the result) or "canary" (outputs: a store outside the slice changes a known bit pattern).
    .view is the whole padded tensor, .slice the live part; data_ptr() that of the slice's first element."""

    def __init__(self, rows, ch, dtype, device, off=0, idle=0, fill="canary"):
        self.rows, self.ch, self.off, self.cw = tuple(rows), ch, off, ch + idle
        n = self.cw
        for r in self.rows:
            n *= r
        self.n = n
        self.flat = torch.empty(n + 2 * GUARD, dtype=dtype, device=device)
        self.bits = _bits(self.flat)
        self.canary = CANARY[self.flat.element_size()]
        if fill == "nan":
            self.flat.fill_(float("nan"))
            self.canary = None
        else:
            self.bits.fill_(self.canary)
        self.view = self.flat[GUARD:GUARD + n].view(*self.rows, self.cw)
        self.slice = self.view[..., off:off + ch]

    def set(self, value):
        self.slice.copy_(value.to(self.flat.device, self.flat.dtype) if torch.is_tensor(value)
                         else torch.full_like(self.slice, value))
        return self

    def data_ptr(self):
        return self.view.data_ptr() + self.off * self.flat.element_size()

    def snapshot(self):
        """the whole buffer's bits on its device (the slice included): two runs of a launch must agree on it"""
        return self.bits.clone()

    def outside(self, name):
        """-> a guard triple for the judge: every element outside the slice still holds the canary.  (The slice
        is overwritten with the canary in a copy of the bits, so one comparison covers guards and idle parts.)"""
        assert self.canary is not None, "NaN-filled input buffers have no canary"
        bits = self.bits.clone()
        bits[GUARD:GUARD + self.n].view(*self.rows, self.cw)[..., self.off:self.off + self.ch].fill_(self.canary)
        return (name, bits.cpu(), self.canary)


class Workspace:
    """`nbytes` of NaN (a partial the reduce reads without its split having written it poisons dW) between two
    canary guards (nothing past workspace_bytes may change)"""

    def __init__(self, nbytes, device):
        assert nbytes % 4 == 0
        self.nbytes, self.n = nbytes, nbytes // 4
        self.flat = torch.empty(self.n + 2 * GUARD, dtype=torch.float32, device=device)
        self.bits = self.flat.view(torch.int32)
        self.canary = CANARY[4]
        self.bits.fill_(self.canary)
        self.live = self.flat[GUARD:GUARD + self.n]
        self.live.fill_(float("nan"))
        self.nan_bits = int(self.bits[GUARD].item()) if self.n else 0

    def data_ptr(self):
        return self.live.data_ptr()

    def guards(self, name="the workspace's guards"):
        g = torch.cat([self.bits[:GUARD], self.bits[GUARD + self.n:]])
        return (name, g.cpu(), self.canary)

    def untouched(self, name="the workspace (too small for one partial: must stay unused)"):
        return (name, self.bits[GUARD:GUARD + self.n].cpu(), self.nan_bits)


# ---------------------------------------------------------------------------------------------- geometries
# Shared by the GPU tests and by tests/test_grad_exact_checker.py, which checks on the CPU that every one of them
# meets the conditions of the mode(s) it is judged in.
PAD_VALUE = 1024.0  # dy's pad channels [cout, dy.channels): finite, exact in every dtype; a tile may read them


class WG(tuple):
    """A weight-gradient geometry: srcs ((channels, upsample), ...), cout, k, stride, H, W (conv input), B;
    dyc: channels of the dy view (>= cout), cin_store (<= cin), full: also judged with full-mantissa operands,
    zero: dW prefilled with zeros instead of grid values"""
    __slots__ = ()

    def __new__(cls, srcs, cout, k, s, H, W, B, dyc=None, cin_store=None, full=True, zero=False):
        cin = sum(c for c, _ in srcs)
        return super().__new__(cls, (tuple(srcs), cout, k, s, H, W, B, dyc or (cout + 7) // 8 * 8, cin_store or cin,
                                     full, zero))

    srcs, cout, k, s, H, W, B, dyc, cin_store, full, zero = (property(lambda self, i=i: self[i]) for i in range(11))
    cin = property(lambda self: sum(c for c, _ in self.srcs))
    pad = property(lambda self: (self.k - 1) // 2)
    oh = property(lambda self: (self.H + 2 * self.pad - self.k) // self.s + 1)
    ow = property(lambda self: (self.W + 2 * self.pad - self.k) // self.s + 1)
    K = property(lambda self: self.B * self.oh * self.ow)  # summed products per dW element
    ne = property(lambda self: self.cout * self.cin_store * self.k * self.k)


def _one(c, up=0):
    return ((c, up),)


WGRAD_GEOMS = [
    # --- pixel-stage edges
    WG(_one(128), 128, 3, 1, 4, 4, 2),                 # 4x4 planes: rows narrower than any stage; K = 32
    WG(_one(128), 128, 1, 1, 2, 2, 2),                 # 2x2 planes, 1x1; K = 8
    WG(_one(32), 64, 3, 1, 9, 13, 3),                  # ow 13: a 32-pixel stage with a tail, B 3, K = 351 (off 64)
    WG(_one(64), 32, 3, 2, 10, 74, 2),                 # stride 2 on even H and W, ow 37; K = 370
    WG(_one(64), 64, 3, 1, 3, 70, 1, zero=True),       # ow 70: a 64-pixel stage with a tail; zero prefill; K = 210
    WG(((96, 0), (32, 0)), 136, 3, 2, 17, 15, 2),      # stride 2 on odd H and W, cout tail 136, split 96 + 32
    # --- channel tails
    WG(_one(16), 24, 3, 1, 12, 12, 1),                 # cout 24 (rows of a 16 / 32-row tile idle), cin 16
    WG(_one(128), 85, 1, 1, 6, 10, 2, dyc=88, zero=True),  # the head preds' 85 rows of an 88-channel dy
    WG(((48, 0), (48, 0)), 64, 1, 1, 6, 7, 3),         # concat split off a stage boundary, B 3
    WG(((80, 0), (80, 0)), 96, 1, 1, 7, 9, 2),
    WG(_one(160), 160, 3, 1, 6, 10, 2),                # tiles 29 / 30
    WG(((80, 0), (80, 0)), 160, 3, 2, 12, 10, 2),
    # --- sources
    WG(((64, 0), (64, 1)), 128, 1, 1, 8, 12, 2),       # the second source upsampled (PAFPN), 1x1
    WG(((64, 0), (64, 1)), 64, 3, 1, 12, 10, 2),       # ... and 3x3
    WG(((32, 1), (32, 0)), 64, 3, 1, 8, 8, 2),         # an upsampled first source
    WG(_one(16), 32, 3, 1, 8, 10, 2, cin_store=12),    # the Focus stem: 12 of 16 channels, 3x3 stride 1
    # --- grid only: many splits with a ragged last one
    WG(_one(64), 64, 3, 1, 40, 44, 2, full=False),     # K = 3520
    WG(_one(128), 128, 3, 1, 20, 20, 4, full=False),   # K = 1600
]


class DG(tuple):
    """A data-gradient geometry of a k x k stride-s conv cin -> cout with pad (k - 1) // 2 over a B x H x W input:
    dy is [B, oh, ow, cout], dx [B, H, W, cin]; full: also judged with full-mantissa operands (K = taps * cout up
    to 2880 meets the conditions: a dropped dx element is a whole sum, not one product)"""
    __slots__ = ()

    def __new__(cls, cin, cout, k, s, H, W, B, full=True):
        return super().__new__(cls, (cin, cout, k, s, H, W, B, full))

    cin, cout, k, s, H, W, B, full = (property(lambda self, i=i: self[i]) for i in range(8))
    pad = property(lambda self: (self.k - 1) // 2)
    oh = property(lambda self: (self.H + 2 * self.pad - self.k) // self.s + 1)
    ow = property(lambda self: (self.W + 2 * self.pad - self.k) // self.s + 1)
    K = property(lambda self: self.k * self.k * self.cout)  # summed products per dx element (at most)


# stride 2: odd and even H and W, cin / cout from 32 to 320 (80, 160, 320 among them), B 2 and 3
DGRAD_S2_GEOMS = [
    DG(32, 32, 3, 2, 17, 15, 3), DG(32, 64, 3, 2, 10, 12, 2), DG(64, 128, 3, 2, 9, 10, 2),
    DG(80, 160, 3, 2, 11, 13, 2), DG(160, 320, 3, 2, 8, 6, 2), DG(320, 320, 3, 2, 5, 7, 2),
    DG(128, 256, 3, 2, 19, 22, 3),
]
# stride 1, conv_ws's fp32-gradient ids (cin == cout): planes below and above one tile, odd widths
DGRAD_S1_GEOMS = [
    DG(64, 64, 3, 1, 3, 5, 2), DG(64, 64, 3, 1, 20, 22, 3), DG(128, 128, 3, 1, 9, 19, 2),
    DG(256, 256, 3, 1, 5, 7, 2), DG(256, 256, 3, 1, 13, 21, 2), DG(80, 80, 3, 1, 11, 19, 2),
    DG(160, 160, 3, 1, 3, 7, 3), DG(160, 160, 3, 1, 10, 18, 2), DG(320, 320, 3, 1, 9, 7, 2),
    DG(320, 320, 3, 1, 5, 33, 2),
]

_OPS = {}


def _draw(shape, g, mode, dtype):
    return (grid(shape, g) if mode == "grid" else torch.randn(shape, generator=g)).to(dtype)


def wgrad_operands(geom, dtype, mode):
    """CPU operands and references of (geometry, compute dtype, "grid" | "full"), built once:
    srcs [x [B, h, w, c] in dtype], dy [B, oh, ow, dyc] in dtype (pad channels = PAD_VALUE), prefill fp32
    [cout][cin_store][k][k], y = prefill + dW (float64), tol (full mode), S"""
    key = ("w", geom, dtype, mode)
    if key not in _OPS:
        g = torch.Generator().manual_seed(1000 + 7 * geom.H * geom.W + geom.cin + 3 * geom.cout)
        xs = [_draw((geom.B, geom.H >> up, geom.W >> up, c), g, mode, dtype) for c, up in geom.srcs]
        dy = _draw((geom.B, geom.oh, geom.ow, geom.dyc), g, mode, dtype)
        dy[..., geom.cout:] = PAD_VALUE
        shape = (geom.cout, geom.cin_store, geom.k, geom.k)
        prefill = torch.zeros(shape) if geom.zero else grid(shape, g)
        dw, S = wgrad_reference([(x, up) for x, (_, up) in zip(xs, geom.srcs)], dy, geom.cout, geom.k, geom.s,
                                geom.pad, geom.cin_store)
        y = dw + prefill.to(torch.float64)
        tol = None
        if mode == "grid":
            assert_grid_exact(y, geom.K + 1)
        else:
            tol = tolerance(geom.K, S, y, added=True)
        _OPS[key] = dict(srcs=xs, dy=dy, prefill=prefill, dw=dw, y=y, S=S, tol=tol)
    return _OPS[key]


def dgrad_operands(geom, dtype, mode):
    """dy [B, oh, ow, cout] in dtype, w fp32 [cout][cin][k][k] (grid values, or randn * 0.05 for the packer to
    round), base fp32 [B, H, W, cin] (the accumulate form's grid-valued destination), dx / S float64, tol"""
    key = ("d", geom, dtype, mode)
    if key not in _OPS:
        g = torch.Generator().manual_seed(2000 + 5 * geom.H * geom.W + geom.cin + 3 * geom.cout)
        dy = _draw((geom.B, geom.oh, geom.ow, geom.cout), g, mode, dtype)
        shape = (geom.cout, geom.cin, geom.k, geom.k)
        w = grid(shape, g) if mode == "grid" else torch.randn(shape, generator=g) * 0.05
        base = grid((geom.B, geom.H, geom.W, geom.cin), g)
        dx, S = dgrad_reference(dy, w, geom.k, geom.s, (geom.H, geom.W))
        y_acc = dx + base.to(torch.float64)
        if mode == "grid":
            assert_grid_exact(dx, geom.K)
            assert_grid_exact(y_acc, geom.K + 1)
        _OPS[key] = dict(dy=dy, w=w, base=base, dx=dx, y_acc=y_acc, S=S)
    return _OPS[key]


def dgrad_tolerance(geom, ops, accumulate):
    """conv_exact.tolerance for an fp32 destination with no activation and a zero bias (S carries no bias term)"""
    y = ops["y_acc"] if accumulate else ops["dx"]
    return ce.tolerance(ops["dx"], y, ops["S"], geom.K, "none", torch.float32, added=accumulate)
