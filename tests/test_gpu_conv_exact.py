"""Every plain forward-conv tile judged per element against a float64 reference of its own operands
(tests/conv_exact.py), one test per (family, dtype).

Per launch: the source is a channel slice (offset 16) of a buffer 32 channels wider whose idle channels are
NaN, with 4096 NaN elements before and after it -- a tile that reads a neighbour against a zero weight, or past
the tensor, poisons its output.  The destination is a slice (offset 32) of a wider buffer filled with a canary
bit pattern, with the same guards -- a store outside the slice changes a canary.  Every launch runs twice into
fresh buffers and the two results must be bit-equal.  The persistent families also run with grid_cap 1 and 2:
every tile walked by one or two blocks, the ring-wrap counts of their pipelines.

A tile may refuse a launch only with its family's own NotImplementedError / ValueError texts, and the codes
that ran on no geometry must be exactly the withdrawn / not-built ones written out in NEVER.
"""
import re

import pytest
import torch

import conv_exact as ce
from test_gpu_ops import DEV, GLDS_K2_WITHDRAWN, N, WS_WIDE_WITHDRAWN, WS_WITHDRAWN, make_conv, pack, run_conv

pytestmark = pytest.mark.gpu

GUARD = 4096
SRC_OFF, DST_OFF, IDLE = 16, 32, 32
CANARY = {2: 0x7A5C, 4: 0x7A5C7A5C}  # finite in bf16 / fp16 / fp32: an unwritten output is a huge error, not a NaN
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DT_ID = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}

# geometry: (sources ((channels, upsample), ...), cout, k, stride, H, W (conv input), batch)


def g3(cin, cout, s, H, W, B):
    return (((cin, 0),), cout, 3, s, H, W, B)


def g1(cin, cout, H, W, B):
    return (((cin, 0),), cout, 1, 1, H, W, B)


# 3x3: odd widths wider than a 16-pixel tile (19, 21, 22), pixel counts off 16, shapes below one tile (5x7, 9x7),
# B = 3, cout tails (80, 96), stride 2 on odd H and W, (64, 64, 20x22x4): >= 5 of a persistent family's largest tile
G3 = [g3(32, 32, 1, 9, 21, 3), g3(64, 80, 1, 13, 19, 2), g3(128, 128, 1, 20, 22, 2), g3(64, 64, 1, 20, 22, 4),
      g3(128, 96, 2, 17, 15, 2), g3(64, 128, 2, 18, 34, 2), g3(256, 64, 1, 5, 7, 3)]
G3_WS = G3 + [g3(32, 64, 2, 11, 13, 2), g3(256, 32, 2, 9, 7, 2), g3(32, 32, 1, 33, 37, 3), g3(256, 64, 1, 17, 19, 3),
              g3(128, 128, 1, 33, 35, 2)]
G3_WIDE = [g3(80, 80, 1, 11, 19, 2), g3(160, 160, 1, 10, 18, 2), g3(320, 96, 1, 9, 7, 3), g3(320, 320, 2, 13, 11, 2),
           g3(512, 512, 1, 6, 10, 2), g3(16, 80, 1, 12, 20, 2), g3(80, 160, 2, 13, 11, 2), g3(160, 64, 2, 9, 15, 2),
           g3(80, 80, 1, 21, 37, 2), g3(160, 64, 1, 17, 35, 2)]
PAFPN = (((128, 1), (64, 0)), 96, 1, 1, 10, 12, 2)  # an upsampled 128-channel slice | 64 dense channels -> 96
G1 = [g1(64, 80, 8, 9, 3), g1(128, 256, 7, 9, 3), g1(64, 64, 20, 22, 3), g1(256, 5, 6, 6, 2), g1(96, 192, 7, 9, 2),
      g1(512, 1024, 4, 5, 3), g1(1024, 512, 5, 5, 2), PAFPN]
# conv_ws1: a 256-channel shape with cout % 8 == 0, two dense sources, the [upsampled | dense] forms its ids
# 249-252 / 256 are built for, >= 5 of the largest (256-pixel) tile, 5-6 of the 16-pixel tiles of the K-split
# 512 / 1024-channel ids (one block walks them all at grid_cap 1), and shapes below a 16- / 32-pixel tile
G1_WS1 = G1 + [g1(256, 64, 9, 11, 2), (((32, 0), (32, 0)), 64, 1, 1, 9, 11, 2),
               (((128, 1), (128, 0)), 128, 1, 1, 10, 12, 2), (((256, 1), (256, 0)), 256, 1, 1, 6, 10, 3),
               g1(64, 64, 36, 37, 1), g1(512, 256, 9, 10, 1), g1(1024, 128, 8, 10, 1), g1(512, 64, 3, 3, 1),
               g1(1024, 64, 3, 3, 1), g1(256, 64, 3, 5, 1)]
G1_PWF = G1 + [g1(64, 64, 36, 37, 1)]  # 1332 pixels: 6 of the 256-pixel tile

SLABS = "2-slab staging not possible"
WS_TEXTS = ("conv_ws variant built for stride", "padded-K variant", "conv_ws: 16-bit dst, SiLU/no activation",
            "conv_ws tile id", "conv_ws is built for bf16/f16")
WS1_TEXTS = ("conv_ws1 variant built for", "conv_ws1: dense 1x1 over", "does not fit the LDS image",
             "no 16-byte epilogue", "conv_ws1 is built for bf16/f16")
R3_LOCAL_16 = set(range(1, 13)) | {14} | set(range(16, 23)) | {26, 27, 28} | set(range(30, 41))
R3_LOCAL_F32 = {29, 30, 31, 32, 33, 38, 39, 40}


class Fam:
    def __init__(self, ids, geoms, texts, bits=(0,), caps=(0,)):
        self.ids, self.geoms, self.texts, self.bits, self.caps = list(ids), geoms, texts, bits, caps

    def codes(self):
        return [2 * i + b for i in self.ids for b in self.bits]


FAMILIES = {
    "igemm": Fam(range(1, 10), G3 + [G1[0], G1[3], G1[4], PAFPN], (SLABS,), bits=(0, 1)),
    "glds": Fam(range(17, 26), G3 + [G1[0], G1[3], G1[4], PAFPN], (SLABS, "two-slab staging is not built"),
                bits=(0, 1)),
    "rows": Fam(range(33, 52), G3, (SLABS, "2-slab stages not built for stride 2", "160 KiB", "bf16/f16 only"),
                bits=(0, 1)),
    "pw": Fam(range(65, 71), G1, (SLABS, "exceed", "160 KiB", "bf16/f16 only", "conv_pw needs a 1x1 stride-1 conv"),
              bits=(0, 1)),
    "pwr": Fam(range(81, 83), G1, ("conv_pwr needs a 1x1", "bf16/f16 only", "beyond 256")),
    "pwf": Fam(range(97, 105), G1_PWF, ("not a multiple of the", "conv_pwf needs a 1x1 s1 conv over dense sources",
                                       "bf16/f16 only"), caps=(0, 1, 2)),
    "r3": Fam(range(113, 161), G3, ("built for stride", "not a multiple of the", "conv_r3 tile id", "bf16/f16 only")),
    "ws": Fam(range(161, 191), G3_WS, WS_TEXTS, caps=(0, 1, 2)),
    "ws1": Fam(range(201, 211), G1_WS1, WS1_TEXTS, bits=(0, 1), caps=(0, 1, 2)),
    "pw1f": Fam(range(211, 215), G1, ("conv_pw1f: fp32 1x1 s1 conv",)),
    "ws1_deep": Fam(range(241, 259), G1_WS1, WS1_TEXTS, bits=(0, 1), caps=(0, 1, 2)),
    "ws_wide": Fam(list(range(261, 281)) + [289], G3_WIDE, WS_TEXTS, caps=(0, 1, 2)),
}


def never(fam, dtype):
    """The tile codes of (family, dtype) that no geometry may run: withdrawn or not built."""
    f = FAMILIES[fam]
    all_codes = set(f.codes())
    h = dtype != torch.float32
    if fam == "igemm":
        return set()
    if fam == "glds":  # two-slab staging of the wide tiles spilled
        return {2 * t + 1 for t in GLDS_K2_WITHDRAWN}
    if fam == "rows":
        # 16-bit: with 128-byte stages the three-buffer ids 39 / 40 / 41 (204 / 204 / 180 KiB) and the TN-128,
        # 128-pixel ids 44 / 45 (168 KiB) pass 160 KiB of LDS (rows_lds_bytes); fp32: ids 39-51 are not built
        return {2 * t + 1 for t in (39, 40, 41, 44, 45)} if h else {2 * t + b for t in range(39, 52) for b in (0, 1)}
    if fam in ("pw", "pwr", "pwf"):
        return set() if h else all_codes
    if fam == "r3":  # reserved ids 153-160, the spilled 125 / 127 / 135 / 136 / 137; 141 is built for fp32 alone
        built = R3_LOCAL_16 if h else R3_LOCAL_F32
        return {2 * t for t in f.ids if t - 112 not in built}
    if fam == "ws":
        return {2 * t for t in WS_WITHDRAWN} if h else all_codes
    if fam == "ws_wide":
        return {2 * t for t in WS_WIDE_WITHDRAWN} if h else all_codes
    if fam == "ws1":
        return set() if h else all_codes
    if fam == "ws1_deep":  # 247: TN 64 over four channel waves, one fragment per wave: no 16-byte epilogue
        return {2 * 247 + 1} if h else all_codes
    if fam == "pw1f":
        return all_codes if h else set()
    raise KeyError(fam)


# ---------------------------------------------------------------- operands and references, built once
_CONV, _REF = {}, {}


def conv_of(geom, dtype):
    """(conv, bn, packed (w, b) on the device, sources [(guarded buffer, SRC_OFF, ch, up)], the logical input
    [B, H, W, cin] on the CPU in the compute dtype, residual / accumulate base [B, oh, ow, cout] fp32)"""
    key = (geom, dtype)
    if key not in _CONV:
        srcs, cout, k, s, H, W, B = geom
        cin = sum(c for c, _ in srcs)
        conv, bn = make_conv(cin, cout, k, s, seed=cin + cout + k + s)
        packed = pack(conv, bn, dtype, cin)
        g = torch.Generator().manual_seed(H * W + cin)
        bufs, parts = [], []
        for c, up in srcs:
            h, w = H >> up, W >> up
            x = torch.randn(B, h, w, c, generator=g).to(dtype)
            n = B * h * w * (c + IDLE)
            flat = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
            view = flat[GUARD:GUARD + n].view(B, h, w, c + IDLE)
            view[..., SRC_OFF:SRC_OFF + c] = x.to(DEV)
            bufs.append((view, SRC_OFF, c, up))
            parts.append(x.repeat_interleave(2, 1).repeat_interleave(2, 2) if up else x)
        pad = (k - 1) // 2
        oh, ow = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
        base = torch.randn(B, oh, ow, cout, generator=g)
        torch.cuda.synchronize()
        _CONV[key] = (conv, bn, packed, bufs, torch.cat(parts, 3), base)
    return _CONV[key]


def ref_of(geom, dtype, act):
    """float64 (z, act(z), S) and fp32 act(z) of (geometry, dtype, activation), computed once"""
    key = (geom, dtype, act)
    if key not in _REF:
        _, cout, k, s, _, _, _ = geom
        _, _, (w, b), _, x, _ = conv_of(geom, dtype)
        z, ya, S = ce.reference(x, w, b, k, s, (k - 1) // 2, act)
        y32 = ce.reference32(x, w, b, k, s, (k - 1) // 2, act, torch.float32)
        _REF[key] = (z, ya, S, y32)
    return _REF[key]


class Dst:
    """A destination slice at channel DST_OFF of a canary-filled, guarded buffer"""

    def __init__(self, B, oh, ow, cout, dtype, prefill=None):
        self.cout = cout
        cw = DST_OFF + (cout + 7) // 8 * 8 + IDLE
        n = B * oh * ow * cw
        self.flat = torch.empty(n + 2 * GUARD, dtype=dtype, device=DEV)
        self.bits = self.flat.view(torch.int16 if self.flat.element_size() == 2 else torch.int32)
        self.canary = CANARY[self.flat.element_size()]
        self.bits.fill_(self.canary)
        self.view = self.flat[GUARD:GUARD + n].view(B, oh, ow, cw)
        if prefill is not None:
            self.view[..., DST_OFF:DST_OFF + cout] = prefill.to(DEV, dtype)

    def result(self):
        """-> (the slice on the CPU, the whole buffer's bits with the slice reset to the canary)"""
        got = self.view[..., DST_OFF:DST_OFF + self.cout].cpu()
        self.view[..., DST_OFF:DST_OFF + self.cout] = 0
        bits = self.bits.cpu()
        n = self.view.numel()
        sl = bits[GUARD:GUARD + n].view(self.view.shape)[..., DST_OFF:DST_OFF + self.cout]
        assert int(sl.abs().max()) == 0  # (the zeros just written: the slice is where we think it is)
        sl.fill_(self.canary)
        return got, bits


VARIANTS = ("plain", "residual", "f32dst", "accumulate")


def launch(geom, dtype, code, act, variant, cap):
    """One launch, twice, each into a fresh canary buffer, judged.  -> (per-element ratio, RMS ratio or None);
    a tile's refusal propagates as its NotImplementedError / ValueError"""
    srcs, cout, k, s, H, W, B = geom
    n = N()
    conv, bn, packed, bufs, _, base = conv_of(geom, dtype)
    pad = (k - 1) // 2
    oh, ow = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    out_dtype = torch.float32 if variant in ("f32dst", "accumulate") else dtype
    prefill = base if variant in ("residual", "accumulate") else None
    runs = []
    for _ in range(2):
        d = Dst(B, oh, ow, cout, out_dtype, prefill)
        run_conv(bufs, conv, bn, dtype, act=act, out=d.view, out_coff=DST_OFF, tile=code, grid_cap=cap, packed=packed,
                 residual=(d.view, DST_OFF) if variant == "residual" else None,
                 flags=n.CONV_ACCUMULATE if variant == "accumulate" else 0)
        runs.append(d)
    label = f"tile {code >> 1} (code {code}) {geom} {DT_ID[dtype]} {act} {variant} grid_cap {cap}"
    assert torch.equal(runs[0].bits, runs[1].bits), f"{label}: two runs differ"
    got, bits = runs[0].result()
    z, ya, S, y32 = ref_of(geom, dtype, act)
    cin = sum(c for c, _ in srcs)
    y, ref32 = ya, None
    if prefill is not None:
        y = ya + prefill.to(out_dtype).to(torch.float64)  # as the kernel reads it back
    if out_dtype != torch.float32:
        y32 = y32.float()
        ref32 = (y32 + prefill.to(dtype).float() if prefill is not None else y32).to(dtype).to(torch.float64)
    tol = ce.tolerance(z, y, S, k * k * cin, act, out_dtype, added=prefill is not None)
    return ce.judge(got, y, tol, out_dtype, ref32=ref32, guards=[("the destination buffer", bits, runs[0].canary)],
                    label=label)


def plan(geom):
    """(act, variant) pairs of a geometry.  The launches are small enough to run every form everywhere, so each
    id meets them at the channel counts it is built for: SiLU, the other activations, an fp32 destination, the
    accumulate into a prefilled fp32 destination, and on stride 1 the in-place residual"""
    out = [("silu", "plain"), ("none", "plain"), ("relu", "plain"), ("lrelu", "plain"), ("silu", "f32dst"),
           ("none", "f32dst"), ("none", "accumulate")]
    if geom[3] == 1:
        out.append(("silu", "residual"))
    return out


def test_refused_where_a_tile_would_be_wrong():
    """What the judge found: conv_pwf stores whole 4-channel groups, so with cout 5 in 8-byte-aligned rows it
    wrote 3 channels into the neighbouring slice; conv_pw1f has no residual add and dropped one silently."""
    for tid in FAMILIES["pwf"].ids:
        with pytest.raises(NotImplementedError, match="conv_pwf needs"):
            launch(g1(256, 5, 6, 6, 2), torch.bfloat16, 2 * tid, "silu", "plain", 0)
    for tid in FAMILIES["pw1f"].ids:
        with pytest.raises(NotImplementedError, match="conv_pw1f: fp32 1x1 s1 conv"):
            launch(g1(64, 80, 8, 9, 3), torch.float32, 2 * tid, "silu", "residual", 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=[DT_ID[d] for d in DTYPES])
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_family_exact(fam, dtype):
    f = FAMILIES[fam]
    texts = re.compile("|".join(re.escape(t) for t in f.texts))
    ran, worst, worst_rms, failures = set(), (0.0, ""), (0.0, ""), []
    for geom in f.geoms:
        for act, variant in plan(geom):
            for code in f.codes():
                for cap in f.caps:
                    try:
                        r = launch(geom, dtype, code, act, variant, cap)
                    except (NotImplementedError, ValueError) as e:
                        assert texts.search(str(e)), f"tile code {code} {geom}: unexpected refusal: {e}"
                        continue
                    except AssertionError as e:  # judge every launch, report them together
                        failures.append(str(e))
                        ran.add(code)
                        continue
                    ran.add(code)
                    label = f"code {code} {geom} {act} {variant} cap {cap}"
                    if r[0] > worst[0]:
                        worst = (r[0], label)
                    if r[1] is not None and r[1] > worst_rms[0]:
                        worst_rms = (r[1], label)
    print(f"\n{fam} {DT_ID[dtype]}: {len(ran)} codes ran; worst per-element {worst[0]:.3f} ({worst[1]}); "
          f"worst rms {worst_rms[0]:.6f} ({worst_rms[1]})")
    assert not failures, f"{len(failures)} launches failed:\n" + "\n".join(failures[:40])
    missing = set(f.codes()) - ran
    assert missing == never(fam, dtype), (f"never ran: {sorted(missing)}; withdrawn / not built: "
                                          f"{sorted(never(fam, dtype))}")
