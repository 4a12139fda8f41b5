"""yxh_rgb_stem_conv / yxh_rgb_stem_pack / yxh_rgb_pack on the device.

The conv is judged per element (tests/conv_exact.py) against a float64 F.conv2d of the operands the
kernel reads: the image rounded to the compute dtype, the folded weights and the fp32 bias
yxh_rgb_stem_pack wrote.  Destinations sit between guard regions and, in the wide layout, inside a
96-channel buffer at a channel offset; every byte the kernel must not touch is compared.
"""
import ctypes as C

import pytest
import torch

import conv_exact as CE

pytestmark = pytest.mark.gpu

SIZES = [(1, 1, 1), (2, 8, 8), (3, 33, 47), (2, 64, 96)]  # (B, H, W): 47 and 96 straddle the 64-pixel tile
FORMATS = ["nchw_f32", "nhwc_u8", "nhwc_bf16", "nhwc_f16", "nhwc_f32"]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
COUTS = [16, 32, 64]
ACTS = ["none", "silu", "lrelu"]
GUARD = 4096  # bytes in front of and behind every destination
EPS = 1e-3


def _lib():
    from yolox_amd import _native as N
    return N, N.lib()


def make_image(fmt, B, H, W, seed):
    """-> (device tensor in the format's layout and dtype, the same values as [B, H, W, 3] float32 on the host)"""
    g = torch.Generator().manual_seed(seed)
    if fmt == "nhwc_u8":
        img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    else:
        img = torch.rand(B, H, W, 3, generator=g) * 255.0
        img = img.to({"nhwc_bf16": torch.bfloat16, "nhwc_f16": torch.float16}.get(fmt, torch.float32))
    dev = img.permute(0, 3, 1, 2).contiguous() if fmt == "nchw_f32" else img
    return dev.cuda(), img.float()


def make_params(cout, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, 3, 3, 3, generator=g) * (27 ** -0.5) / 64.0  # images are 0..255
    gamma = torch.rand(cout, generator=g) * 0.4 + 0.4
    beta = torch.randn(cout, generator=g) * 0.5
    mean = torch.randn(cout, generator=g) * 0.3
    var = torch.rand(cout, generator=g) + 0.5
    return w, gamma, beta, mean, var


def pack(params, cout, dtype):
    """yxh_rgb_stem_pack -> (packed weights [round16(cout), 32] in dtype, bias fp32 [round16(cout)]), on the device"""
    N, lib = _lib()
    cpad = (cout + 15) // 16 * 16
    dev = [t.cuda().contiguous() for t in params]
    wp = torch.full((cpad, 32), 7.0, dtype=dtype, device="cuda")
    bp = torch.full((cpad,), 7.0, dtype=torch.float32, device="cuda")
    N.check(lib.yxh_rgb_stem_pack(*[t.data_ptr() for t in dev], EPS, cout, N.DTYPE_CODE[dtype], wp.data_ptr(),
                                  bp.data_ptr(), N.stream_ptr()), "rgb_stem_pack")
    torch.cuda.synchronize()
    return wp, bp


def desc(N, fmt, img, B, H, W, dtype, cout, act, wp, bp, dst_ptr, cstride):
    d = N.StemDesc()
    d.img = img.data_ptr()
    d.layout = N.NCHW if fmt == "nchw_f32" else N.NHWC
    d.img_dtype = N.DTYPE_CODE[img.dtype]
    d.batch, d.h, d.w = B, H, W
    d.dtype, d.cout, d.act = N.DTYPE_CODE[dtype], cout, N.ACT_CODE[act]
    d.weight, d.bias = wp.data_ptr(), bp.data_ptr()
    d.dst, d.dst_cstride, d.dst_bstride = dst_ptr, cstride, H * W * cstride
    return d


def run_case(fmt, B, H, W, dtype, cout, act, wide, seed):
    """One launch (twice, for determinism) into a guarded destination, judged per element."""
    N, lib = _lib()
    img, host = make_image(fmt, B, H, W, seed)
    wp, bp = pack(make_params(cout, seed + 1), cout, dtype)
    cstride, coff = (96, 32) if wide else (cout, 0)
    es = torch.empty((), dtype=dtype).element_size()
    nbytes = B * H * W * cstride * es
    raw = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    before = raw.clone()
    body = raw[GUARD:GUARD + nbytes].view(dtype).view(B, H, W, cstride)
    d = desc(N, fmt, img, B, H, W, dtype, cout, act, wp, bp, body.data_ptr() + coff * es, cstride)
    N.check(lib.yxh_rgb_stem_conv(C.byref(d), N.stream_ptr()), "rgb_stem_conv")
    torch.cuda.synchronize()
    first = raw.clone()
    N.check(lib.yxh_rgb_stem_conv(C.byref(d), N.stream_ptr()), "rgb_stem_conv")
    torch.cuda.synchronize()
    assert torch.equal(raw, first), "two launches differ"
    got = body[..., coff:coff + cout]
    x = host.to(dtype)  # what the kernel stages: the image rounded to the compute dtype
    w_fold = wp[:cout, :27].reshape(cout, 3, 3, 3)  # [cout][ky][kx][c], the packed k order
    z, y, S = CE.reference(x, w_fold, bp[:cout], 3, 1, 1, act)
    tol = CE.tolerance(z, y, S, 27, act, dtype)
    ref32 = None if dtype == torch.float32 else CE.reference32(x, w_fold, bp[:cout], 3, 1, 1, act, dtype)
    mask = torch.ones(B, H, W, cstride, dtype=torch.bool)
    mask[..., coff:coff + cout] = False
    canary = before[GUARD:GUARD + nbytes].view(dtype).view(B, H, W, cstride).cpu().view(torch.uint8)
    body_bytes = body.cpu().view(torch.uint8)
    mask_bytes = mask.repeat_interleave(es, dim=3)
    guards = [("front guard", raw[:GUARD].cpu(), before[:GUARD].cpu()),
              ("back guard", raw[GUARD + nbytes:].cpu(), before[GUARD + nbytes:].cpu()),
              ("untouched channels", body_bytes[mask_bytes], canary[mask_bytes])]
    label = f"{fmt} {B}x{H}x{W} {dtype} cout {cout} {act} {'wide' if wide else 'dense'}"
    return CE.judge(got, y, tol, dtype, ref32, guards, label)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_rgb_stem_conv_per_element(size, fmt, dtype):
    """Every size x image format x compute dtype, each with all three widths; the activation and the
    destination layout rotate so that every (cout, act) and (cout, layout) pair occurs."""
    B, H, W = size
    i = SIZES.index(size) * 15 + FORMATS.index(fmt) * 3 + DTYPES.index(dtype)
    for ci, cout in enumerate(COUTS):
        run_case(fmt, B, H, W, dtype, cout, ACTS[(i + ci) % 3], wide=bool((i // 3 + ci) % 2), seed=100 + i)


@pytest.mark.parametrize("wide", [False, True], ids=["dense", "offset_in_96"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("cout", COUTS)
def test_rgb_stem_conv_widths_acts_layouts(cout, act, wide):
    for dtype in DTYPES:
        run_case("nhwc_u8", 3, 33, 47, dtype, cout, act, wide, seed=7)


def test_rgb_stem_refusals():
    N, lib = _lib()
    img, _ = make_image("nhwc_u8", 1, 8, 8, 0)
    wp, bp = pack(make_params(32, 1), 32, torch.bfloat16)
    out = torch.zeros(1, 8, 8, 32, dtype=torch.bfloat16, device="cuda")
    good = lambda: desc(N, "nhwc_u8", img, 1, 8, 8, torch.bfloat16, 32, "lrelu", wp, bp, out.data_ptr(), 32)  # noqa: E731
    assert lib.yxh_rgb_stem_conv(None, None) == N.EINVAL and b"null" in lib.yxh_last_error()
    for field in ("img", "weight", "bias", "dst"):
        d = good()
        setattr(d, field, None)
        assert lib.yxh_rgb_stem_conv(C.byref(d), N.stream_ptr()) == N.EINVAL, field
        assert b"null" in lib.yxh_last_error()
    d = good()
    d.cout = 24
    assert lib.yxh_rgb_stem_conv(C.byref(d), N.stream_ptr()) == N.EUNSUPPORTED and b"cout 24" in lib.yxh_last_error()
    d = good()
    d.cout = 80
    assert lib.yxh_rgb_stem_conv(C.byref(d), N.stream_ptr()) == N.EUNSUPPORTED
    d = good()
    d.dtype = N.U8
    assert lib.yxh_rgb_stem_conv(C.byref(d), N.stream_ptr()) == N.EINVAL and b"dtype" in lib.yxh_last_error()
    for field, bad in (("h", 0), ("batch", 0), ("layout", 2), ("img_dtype", 9), ("act", N.ACT_DECODE), ("dst_cstride", 16),
                       ("dst", out.data_ptr() + 2)):
        d = good()
        setattr(d, field, bad)
        assert lib.yxh_rgb_stem_conv(C.byref(d), N.stream_ptr()) == N.EINVAL, field
    d = good()
    d.layout = N.NCHW  # NCHW images are float32
    assert lib.yxh_rgb_stem_conv(C.byref(d), N.stream_ptr()) == N.EUNSUPPORTED
    op = N.Op()
    op.kind = N.OP_STEM_RGB
    op.u.stem = good()
    op.u.stem.cout = 24
    assert lib.yxh_run_ops(C.byref(op), 1, N.stream_ptr()) == N.EUNSUPPORTED
    torch.cuda.synchronize()
    assert not out.any()  # every refusal came before a launch
    op.u.stem.cout = 32
    N.check(lib.yxh_run_ops(C.byref(op), 1, N.stream_ptr()), "run_ops")
    torch.cuda.synchronize()
    assert out.any()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("cout", [24, 32])
def test_rgb_stem_pack_matches_host_fold(cout, dtype):
    """[round16(cout)][32], k = (ky*3 + kx)*3 + c, zeros at k >= 27 and in the rows past cout; the fold
    is yxh_stem_pack's: w * gamma / sqrt(var + eps) rounded once, bias beta - mean * scale in fp32.  Bounds
    from the device operations' precision: sqrtf within 1 ulp, the fp32 divide within 2.5 ulp, the product
    half an ulp -- 4 ulp = 8 unit roundoffs on the folded weight, plus the destination's rounding; the bias'
    product carries the scale's 7 roundoffs plus its own and the subtraction's."""
    params = make_params(cout, 5)
    wp, bp = pack(params, cout, dtype)
    w, gamma, beta, mean, var = params
    scale = gamma / torch.sqrt(var + EPS)
    want = (w * scale[:, None, None, None]).permute(0, 2, 3, 1).reshape(cout, 27).double()
    got = wp.cpu().double()
    assert not got[:cout, 27:].any() and not got[cout:].any()
    tol = (CE.U_OUT[dtype] + 8 * CE.U32) * want.abs() + CE.HALF_SUBNORMAL[dtype]
    assert bool(((got[:cout, :27] - want).abs() <= tol).all())
    want_b = (beta - mean * scale).double()
    tol_b = 9 * CE.U32 * (beta.abs() + (mean * scale).abs()).double() + 1e-30
    assert bool(((bp.cpu().double()[:cout] - want_b).abs() <= tol_b).all()) and not bp[cout:].any()
    # no BatchNorm: scale 1, bias 0
    N, lib = _lib()
    wd = w.cuda()
    N.check(lib.yxh_rgb_stem_pack(wd.data_ptr(), None, None, None, None, 0.0, cout, N.DTYPE_CODE[dtype], wp.data_ptr(),
                                  bp.data_ptr(), N.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(wp[:cout, :27].cpu(), w.permute(0, 2, 3, 1).reshape(cout, 27).to(dtype)) and not bp.any()


@pytest.mark.parametrize("dst_dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_rgb_pack_is_exact(fmt, dst_dtype):
    N, lib = _lib()
    for B, H, W in [(1, 1, 1), (3, 33, 47)]:  # 4653 pixels: more than one block, a ragged last one
        img, host = make_image(fmt, B, H, W, 3)
        es = torch.empty((), dtype=dst_dtype).element_size()
        nbytes = B * H * W * 16 * es
        raw = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        N.check(lib.yxh_rgb_pack(img.data_ptr(), N.NCHW if fmt == "nchw_f32" else N.NHWC, N.DTYPE_CODE[img.dtype], B, H, W,
                                 raw[GUARD:].data_ptr(), N.DTYPE_CODE[dst_dtype], N.stream_ptr()), "rgb_pack")
        torch.cuda.synchronize()
        out = raw[GUARD:GUARD + nbytes].view(dst_dtype).view(B, H, W, 16).cpu()
        assert torch.equal(out[..., :3], host.to(dst_dtype)) and not out[..., 3:].any()
        assert bool((raw[:GUARD] == 0xA5).all()) and bool((raw[GUARD + nbytes:] == 0xA5).all())
