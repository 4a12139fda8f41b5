"""The data-gradient kernels the forward judge (test_gpu_conv_exact.py) leaves out, judged per element against a
float64 reference (tests/grad_exact.py): yxh_pack_dgrad_weight bit for bit, then yxh_conv2d over its weights with
a zero bias, no activation and a dense fp32 destination, as the trainer launches it --

  stride 2   the parity-class tiles 215-216 (fp32) / 217-220 (16-bit) over the zero-dilated dy, and the same
             dilated source on conv_igemm (ids 1-9, both slab bits) and on code 0, the untuned route
  stride 1   conv_ws's fp32-gradient ids 281-288 (persistent: grid_cap 0, 1, 2)

Grid operands must give the reference's bits at every K; full-mantissa operands are held to
conv_exact.tolerance with K = taps * cout.  dy sits between NaN guards.  The destination sits between canary
guards; in the write form it is canary-prefilled itself, so an element the kernel does not write is a huge
error; in the YXH_CONV_ACCUMULATE form it holds a grid-valued base.  Every launch runs twice and must give the
same bits.  A tile may refuse only with its family's texts; what ran nowhere must equal NEVER (empty).
"""
import ctypes as C
import re

import pytest
import torch

import grad_exact as ge
from test_gpu_ops import DEV, N
from yolox_amd import tiles as T

pytestmark = pytest.mark.gpu

DT_ID = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}
DT_OF = {v: k for k, v in DT_ID.items()}
SLABS = "2-slab staging not possible"
DILATED = "dilated (upsample == 2) sources run on the register-staged kernel only"
S2_TEXTS = ("dgrad_s2f: fp32 data gradient of a 3x3 s2 p1 conv", "dgrad_s2h: 16-bit data gradient of a 3x3 s2 p1 conv")
WS_TEXTS = ("conv_ws variant built for stride", "conv_ws fp32-gradient tile", "conv_ws is built for bf16/f16")
FORMS = ("write", "accumulate")


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------- the packer
PACK_CASES = [  # cout, cin, k, c_begin, c_count, cout_pad
    (24, 16, 3, 0, 16, 24), (24, 40, 3, 16, 24, 24), (85, 32, 1, 0, 32, 88), (64, 96, 1, 48, 48, 64),
    (21, 24, 3, 8, 16, 32), (64, 64, 3, 0, 64, 64),
]


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("cout,cin,k,c_begin,c_count,cout_pad", PACK_CASES)
def test_pack_dgrad_weight_bit_equal(dt, cout, cin, k, c_begin, c_count, cout_pad):
    """[cout][cin][kh][kw] fp32 -> [c_count][kh][kw][cout_pad]: flipped taps, the second source of a concat
    (c_begin > 0), zeros in [cout, cout_pad), one round-to-nearest-even; nothing outside the output written."""
    n, dtype = N(), DT_OF[dt]
    g = torch.Generator().manual_seed(cout + cin + k)
    w = torch.randn(cout, cin, k, k, generator=g)
    w[0, c_begin, 0, 0] = 1.0 + 2.0 ** -8 + 2.0 ** -20  # above a bf16 tie: truncation would round down
    w[1, c_begin, 0, 0] = 1.0 + 2.0 ** -8               # a bf16 tie: to even (down)
    w[2, c_begin, 0, 0] = 1.0 + 3 * 2.0 ** -8           # a bf16 tie: to even (up)
    want = ge.dgrad_weight_reference(w, c_begin, c_count, cout_pad, dtype)
    wd = w.to(DEV)
    out = ge.Guarded((), want.numel(), dtype, DEV)
    n.check(n.lib().yxh_pack_dgrad_weight(wd.data_ptr(), cout, cin, k, k, c_begin, c_count, cout_pad,
                                          n.DTYPE_CODE[dtype], out.data_ptr(), stream()))
    got = out.slice.cpu().view(want.shape)
    ge.check_guards([out.outside("the packed weights' buffer")])
    iv = torch.int32 if dtype == torch.float32 else torch.int16
    bad = got.view(iv) != want.view(iv)
    assert not bool(bad.any()), f"{int(bad.sum())} elements differ, first at (c, ky, kx, n) = {ge.first_index(bad)}"


# ---------------------------------------------------------------------------------------------- the launches
_DEV = {}


def device_operands(geom, dtype, mode):
    """dy between NaN guards, the packed weights, a zero bias and the accumulate base on the device, once"""
    key = (geom, dtype, mode)
    if key not in _DEV:
        n = N()
        ops = ge.dgrad_operands(geom, dtype, mode)
        dy = ge.Guarded((geom.B, geom.oh, geom.ow), geom.cout, dtype, DEV, fill="nan").set(ops["dy"])
        wd = ops["w"].to(DEV)
        pk = torch.empty(geom.cin * geom.k * geom.k * geom.cout, dtype=dtype, device=DEV)
        n.check(n.lib().yxh_pack_dgrad_weight(wd.data_ptr(), geom.cout, geom.cin, geom.k, geom.k, 0, geom.cin,
                                              geom.cout, n.DTYPE_CODE[dtype], pk.data_ptr(), stream()))
        torch.cuda.synchronize()
        want = ge.dgrad_weight_reference(ops["w"], 0, geom.cin, geom.cout, dtype)
        assert torch.equal(pk.cpu().view(want.shape), want)
        _DEV[key] = (dy, pk, torch.zeros(geom.cin, device=DEV), ops["base"].to(DEV))
    return _DEV[key]


def run_once(geom, dtype, mode, code, form, cap):
    n = N()
    dy, pk, zb, base = device_operands(geom, dtype, mode)
    dx = ge.Guarded((geom.B, geom.H, geom.W), geom.cin, torch.float32, DEV)
    if form == "accumulate":
        dx.set(base)
    d = n.ConvDesc()
    d.dtype, d.batch, d.in_h, d.in_w, d.out_h, d.out_w = n.DTYPE_CODE[dtype], geom.B, geom.H, geom.W, geom.H, geom.W
    d.cin, d.cout, d.kh, d.kw, d.stride, d.pad = geom.cout, geom.cin, geom.k, geom.k, 1, geom.k - 1 - geom.pad
    d.groups, d.nsrc = 1, 1
    s = n.Src()
    s.ptr, s.channels, s.cstride, s.bstride = dy.data_ptr(), geom.cout, geom.cout, geom.oh * geom.ow * geom.cout
    s.h, s.w, s.upsample = geom.oh, geom.ow, 2 if geom.s == 2 else 0
    d.src[0] = s
    d.weight, d.bias, d.dst, d.dst_dtype = pk.data_ptr(), zb.data_ptr(), dx.data_ptr(), n.DTYPE_CODE[torch.float32]
    d.dst_cstride, d.dst_bstride, d.act = geom.cin, geom.H * geom.W * geom.cin, 0
    d.flags, d.tile, d.grid_cap = (n.CONV_ACCUMULATE if form == "accumulate" else 0), code, cap
    n.check(n.lib().yxh_conv2d(C.byref(d), stream()))
    return dx


def launch(geom, dtype, mode, code, form, cap=0):
    """One launch, twice, judged -> the worst |got - y| / tolerance (0 on grid operands); a refusal propagates"""
    label = f"tile {code >> 1} (code {code}) {tuple(geom)} {DT_ID[dtype]} {mode} operands, {form}, grid_cap {cap}"
    ops = ge.dgrad_operands(geom, dtype, mode)
    a = run_once(geom, dtype, mode, code, form, cap)
    b = run_once(geom, dtype, mode, code, form, cap)
    acc = form == "accumulate"
    y = ops["y_acc"] if acc else ops["dx"]
    guards = [a.outside("dx's buffer")]
    if mode == "grid":
        ratio = ge.judge_exact(a.slice, y, guards=guards, label=label)
    else:
        ratio = ge.judge_bound(a.slice, y, ge.dgrad_tolerance(geom, ops, acc), guards=guards, label=label)
    if not torch.equal(a.bits, b.bits):
        at = ge.first_index((a.bits != b.bits).cpu())[0] - ge.GUARD
        raise AssertionError(f"{label}: two runs differ, first at flat element {at} of dx")
    return ratio


class Fam:
    def __init__(self, codes, dtypes, geoms, texts, caps=(0,)):
        self.codes, self.dtypes, self.geoms, self.texts, self.caps = list(codes), dtypes, geoms, texts, caps


FAMILIES = {
    "dgrad_s2_f32": Fam(T.codes(T.DGRAD_S2_F32), ("f32",), ge.DGRAD_S2_GEOMS, S2_TEXTS),
    "dgrad_s2_16": Fam(T.codes(T.DGRAD_S2_16), ("bf16", "f16"), ge.DGRAD_S2_GEOMS, S2_TEXTS),
    # the zero-dilated form on the register-staged kernel (every id, both slab bits) and the untuned route
    "igemm_dilated": Fam([0] + T.codes(T.IGEMM.ids, (0, 1)), ("f32", "bf16", "f16"), ge.DGRAD_S2_GEOMS, (SLABS,)),
    "ws_f32grad": Fam(T.codes(T.WS_WIDE_F32GRAD), ("bf16", "f16"), ge.DGRAD_S1_GEOMS, WS_TEXTS, caps=(0, 1, 2)),
}
CASES = [(f, d) for f, fam in FAMILIES.items() for d in fam.dtypes]
# (family, dtype) -> the (code, form) pairs that no geometry may run
NEVER = {case: set() for case in CASES}


@pytest.mark.parametrize("fam,dt", CASES, ids=[f"{f}-{d}" for f, d in CASES])
def test_dgrad_family_exact(fam, dt):
    f, dtype = FAMILIES[fam], DT_OF[dt]
    assert T.DGRAD_S2_F32 == range(215, 217) and T.DGRAD_S2_16 == range(217, 221) and \
        T.WS_WIDE_F32GRAD == range(281, 289)
    pat = re.compile("|".join(re.escape(t) for t in f.texts))
    ran, worst, failures, launches = set(), (0.0, ""), [], 0
    for geom in f.geoms:
        for mode in ("grid", "full"):
            if mode == "full" and not geom.full:
                continue
            for code in f.codes:
                for form in FORMS:
                    for cap in f.caps:
                        try:
                            r = launch(geom, dtype, mode, code, form, cap)
                        except (NotImplementedError, ValueError) as e:
                            assert pat.search(str(e)), f"code {code} {tuple(geom)} {form}: unexpected refusal: {e}"
                            continue
                        except AssertionError as e:  # judge every launch, report them together
                            failures.append(str(e))
                            ran.add((code, form))
                            continue
                        ran.add((code, form))
                        launches += 1
                        if r > worst[0]:
                            worst = (r, f"code {code} {tuple(geom)} {form} cap {cap}")
    print(f"\ndgrad {fam} {dt}: {launches} launches judged (each run twice), {len(ran)} (code, form) pairs ran; "
          f"worst full-mantissa ratio {worst[0]:.4f} ({worst[1]})")
    assert not failures, f"{len(failures)} launches failed:\n" + "\n".join(failures[:40])
    missing = {(c, form) for c in f.codes for form in FORMS} - ran
    assert missing == NEVER[(fam, dt)], f"never ran: {sorted(missing)}; expected: {sorted(NEVER[(fam, dt)])}"


# ---------------------------------------------------------------------------------------------- the dilated sweep
# What a row that is not flagged YXH_TILE_NO_DILATED may answer to a zero-dilated 3x3 source instead of running it
SWEEP_TEXTS = {
    "igemm": (SLABS,),
    "dgrad_s2": S2_TEXTS + (SLABS,),
    "ws_post": ("conv_ws needs a 3x3 pad-1 conv over one plain source", SLABS),
    "ws1_deep": ("conv_ws1 needs a 1x1 s1 conv", SLABS),
    "ws_wide": ("conv_ws needs a 3x3 pad-1 conv over one plain source", SLABS),
}
SWEEP_GEOM = ge.DGRAD_S2_GEOMS[2]  # 64 -> 128, 9x10, B 2: two K slabs possible in every dtype
# {dtype: the tile ids that ran the dilated source}: conv_igemm and the parity-class tiles of the operand type
SWEEP_RAN = {"f32": set(T.IGEMM.ids) | set(T.DGRAD_S2_F32), "bf16": set(T.IGEMM.ids) | set(T.DGRAD_S2_16),
             "f16": set(T.IGEMM.ids) | set(T.DGRAD_S2_16)}


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_dilated_source_on_every_tile_code(dt):
    """Every code of every row of the tile table handed the zero-dilated dy: a row flagged YXH_TILE_NO_DILATED must
    refuse it (the tuner times whatever returns YXH_OK), any other code refuses with its family's text or is
    exact."""
    dtype = DT_OF[dt]
    ran, failures = set(), []
    for fam in T.FAMILIES:
        flagged = bool(fam.flags & T.NO_DILATED)
        assert flagged or fam.name in SWEEP_TEXTS, fam.name
        pat = re.compile("|".join(re.escape(t) for t in ((DILATED, SLABS) if flagged else SWEEP_TEXTS[fam.name])))
        for code in T.codes(fam.ids, (0, 1)):
            try:
                launch(SWEEP_GEOM, dtype, "grid", code, "write")
            except (NotImplementedError, ValueError) as e:
                if not pat.search(str(e)):
                    failures.append(f"{fam.name} code {code}: unexpected refusal: {e}")
                continue
            except AssertionError as e:
                failures.append(str(e))
                continue
            if flagged:
                failures.append(f"{fam.name} code {code} is flagged YXH_TILE_NO_DILATED and ran a dilated source")
            ran.add(code >> 1)
    assert not failures, f"{len(failures)} codes failed:\n" + "\n".join(failures[:40])
    assert ran == SWEEP_RAN[dt], sorted(ran ^ SWEEP_RAN[dt])
