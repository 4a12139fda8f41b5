"""Every weight-gradient tile (yxh_conv_wgrad, ids 1-30 and the by-shape tile 0) judged per element against a
float64 reference (tests/grad_exact.py), one test per (family of csrc/wgrad.hip's kWgradFamilies, dtype).

Operands.  Every geometry runs on grid operands (k / 8, |k| <= 16): all products and partial sums are fp32
numbers, so whatever the order -- MFMA internals, K splits, atomics, the fixed-order reduce -- the result must
equal the reference bit for bit, at any K.  The geometries small enough for the derived bound to bite (full=True,
conditions in tests/test_grad_exact_checker.py) also run on randn rounded to the compute dtype.

Views, as the trainer hands them over.  Each source is a channel slice (offset 16) of a buffer 32 channels wider
with NaN in the idle channels and 4096 NaN elements before and after; dy likewise, its pad channels
[cout, dy.channels) holding a large finite value (a tile may read them, never use them).  dW is a slice of a flat
canary buffer (in the trainer the neighbours are other parameters' gradients), prefilled with grid values: both the
atomic path and wgrad_reduce add onto it (one geometry per family starts from zeros).

Workspace, a NaN-filled slice between canary guards:
  none    atomics
  16 MiB  every partial the reduce reads must have been written by its split: no NaN may reach dW
          (and what was written is a whole number of partials, at least one: the workspace was used)
  three   room for exactly three partials of this dW: the capacity clamp (which binds in every family: some
          geometry leaves more than three partials in 16 MiB); nothing past workspace_bytes changes
  small   16 bytes short of one partial: falls back to atomics, the workspace stays bit-untouched
Every launch runs twice into fresh buffers; the two results must be bit-equal on grid operands in every mode, and
with full-mantissa operands whenever the splits go through a workspace.

A tile may refuse a launch only with its family's own texts, and the (tile, workspace mode) pairs that ran on no
geometry must be exactly NEVER -- which is empty.
"""
import ctypes as C
import re

import pytest
import torch

import grad_exact as ge
from test_gpu_ops import DEV, N

pytestmark = pytest.mark.gpu

OFF, IDLE = 16, 32
DT_ID = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}
DT_OF = {v: k for k, v in DT_ID.items()}
WS_MODES = ("none", "16M", "three", "small")
NINE = "need a 3x3 pad-1 conv of stride 1 or 2"

# family: (ids, dtypes, the texts it may refuse with)
FAMILIES = {
    "by_shape": ([0], ("f32", "bf16", "f16"), ()),  # one of 1-4 by shape: may never refuse
    "reg": (range(1, 5), ("f32", "bf16", "f16"), ()),
    "glds": (range(5, 11), ("bf16", "f16"), ()),
    "nine_f32": (range(11, 17), ("f32",), (NINE, "read one plain source", "channels must be whole 4-float chunks")),
    "kmajor": (range(17, 21), ("f32",), ("wgrad tiles 17-20: 16-byte channel chunks",)),
    "nine_kmajor": (range(21, 25), ("f32",), (NINE, "wgrad tiles 21-24: 16-byte channel chunks")),
    "nine_16": (range(25, 31), ("bf16", "f16"), (NINE, "wgrad tiles 25-30: 16-byte channel chunks",
                                                 "wgrad tile 27 is stride-1 only")),
}
CASES = [(f, d) for f, (_, dts, _) in FAMILIES.items() for d in dts]
# (family, dtype) -> the (tile, workspace mode) pairs that no geometry may run
NEVER = {case: set() for case in CASES}

_DEV = {}
PARTIALS = {"16M": 0, "three": 0}  # the most partials a launch left in its workspace, per mode


def view_src(buf, h, w, up=0):
    s = N().Src()
    s.ptr = buf.data_ptr()
    s.channels, s.cstride, s.bstride = buf.ch, buf.cw, h * w * buf.cw
    s.h, s.w, s.upsample = h, w, up
    return s


def device_operands(geom, dtype, mode):
    """the guarded source / dy buffers of (geometry, dtype, mode) on the device, uploaded once (the kernels only
    read them)"""
    key = (geom, dtype, mode)
    if key not in _DEV:
        ops = ge.wgrad_operands(geom, dtype, mode)
        srcs = []
        for x, (c, up) in zip(ops["srcs"], geom.srcs):
            srcs.append(ge.Guarded(x.shape[:3], c, dtype, DEV, off=OFF, idle=IDLE, fill="nan").set(x))
        dy = ge.Guarded((geom.B, geom.oh, geom.ow), geom.dyc, dtype, DEV, off=OFF, idle=IDLE, fill="nan").set(ops["dy"])
        _DEV[key] = (srcs, dy, ops["prefill"].to(DEV))
    return _DEV[key]


def ws_bytes(geom, ws_mode):
    return {"none": 0, "16M": 16 << 20, "three": 3 * geom.ne * 4, "small": geom.ne * 4 - 16}[ws_mode]


def run_once(geom, dtype, mode, tile, ws_mode):
    """one launch into a fresh dW buffer and workspace -> (dW buffer, workspace or None)"""
    n = N()
    srcs, dy, prefill = device_operands(geom, dtype, mode)
    dw = ge.Guarded((), geom.ne, torch.float32, DEV)
    dw.slice.copy_(prefill.reshape(-1))
    ws = ge.Workspace(ws_bytes(geom, ws_mode), DEV) if ws_mode != "none" else None
    d = n.WgradDesc()
    d.dtype, d.batch = n.DTYPE_CODE[dtype], geom.B
    d.in_h, d.in_w, d.out_h, d.out_w = geom.H, geom.W, geom.oh, geom.ow
    d.cin, d.cout, d.kh, d.kw, d.stride, d.pad = geom.cin, geom.cout, geom.k, geom.k, geom.s, geom.pad
    d.nsrc, d.cin_store = len(srcs), geom.cin_store
    for j, (buf, (_, up)) in enumerate(zip(srcs, geom.srcs)):
        d.src[j] = view_src(buf, geom.H >> up, geom.W >> up, up)
    d.dy = view_src(dy, geom.oh, geom.ow)
    d.dw, d.tile = dw.data_ptr(), tile
    if ws is not None:
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.nbytes
    n.check(n.lib().yxh_conv_wgrad(C.byref(d), torch.cuda.current_stream().cuda_stream))
    return dw, ws


def judge_run(geom, ops, mode, dw, ws, ws_mode, label):
    guards = [dw.outside("dW's buffer (the neighbouring gradients)")]
    if ws is not None:
        guards.append(ws.guards())
        if ws_mode == "small":
            guards.append(ws.untouched())
    got = dw.slice.view(geom.cout, geom.cin_store, geom.k, geom.k)
    if mode == "grid":
        ratio = ge.judge_exact(got, ops["y"], guards=guards, label=label)
    else:
        ratio = ge.judge_bound(got, ops["y"], ops["tol"], guards=guards, label=label)
    if ws_mode in ("16M", "three"):  # honoured by every tile: whole partials, at least one, went through it
        written = int((~torch.isnan(ws.live)).sum())
        if written < geom.ne or written % geom.ne:
            raise AssertionError(f"{label}: {written} floats of the workspace written, not whole partials of {geom.ne}")
        PARTIALS[ws_mode] = max(PARTIALS[ws_mode], written // geom.ne)
    return ratio


def launch(geom, dtype, mode, tile, ws_mode):
    """One launch, twice, judged.  -> the worst |got - y| / tolerance (0 on grid operands); a refusal propagates"""
    label = f"tile {tile} {tuple(geom)} {DT_ID[dtype]} {mode} operands, workspace {ws_mode}"
    ops = ge.wgrad_operands(geom, dtype, mode)
    a, wa = run_once(geom, dtype, mode, tile, ws_mode)
    b, wb = run_once(geom, dtype, mode, tile, ws_mode)
    ratio = judge_run(geom, ops, mode, a, wa, ws_mode, label)
    if mode == "grid" or ws_mode in ("16M", "three"):
        if not torch.equal(a.bits, b.bits):
            at = ge.first_index((a.bits != b.bits).cpu())[0] - ge.GUARD
            raise AssertionError(f"{label}: two runs differ, first at dW element {at} (outside [0, {geom.ne}): a "
                                 f"guard)")
        ge.check_guards([wb.guards()] if wb is not None else [], label)
    else:
        ratio = max(ratio, judge_run(geom, ops, mode, b, wb, ws_mode, label + " (second run)"))
    return ratio


def run_family(fam, dtype, geoms, modes=("grid", "full"), ws_modes=WS_MODES):
    ids, _, texts = FAMILIES[fam]
    pat = re.compile("|".join(re.escape(t) for t in texts)) if texts else None
    ran, worst, failures, launches = set(), (0.0, ""), [], 0
    for geom in geoms:
        for mode in modes:
            if mode == "full" and not geom.full:
                continue
            for tile in ids:
                for ws_mode in ws_modes:
                    try:
                        r = launch(geom, dtype, mode, tile, ws_mode)
                    except (NotImplementedError, ValueError) as e:
                        assert pat is not None and pat.search(str(e)), \
                            f"tile {tile} {tuple(geom)} workspace {ws_mode}: unexpected refusal: {e}"
                        continue
                    except AssertionError as e:  # judge every launch, report them together
                        failures.append(str(e))
                        ran.add((tile, ws_mode))
                        continue
                    ran.add((tile, ws_mode))
                    launches += 1
                    if r > worst[0]:
                        worst = (r, f"tile {tile} {tuple(geom)} workspace {ws_mode}")
    return ran, worst, failures, launches


@pytest.mark.parametrize("fam,dt", CASES, ids=[f"{f}-{d}" for f, d in CASES])
def test_wgrad_family_exact(fam, dt):
    dtype = DT_OF[dt]
    PARTIALS.update({"16M": 0, "three": 0})
    ran, worst, failures, launches = run_family(fam, dtype, ge.WGRAD_GEOMS)
    print(f"\nwgrad {fam} {dt}: {launches} launches judged (each run twice), {len(ran)} (tile, workspace) pairs ran; "
          f"worst full-mantissa ratio {worst[0]:.4f} ({worst[1]})")
    print(f"most partials in a workspace: {PARTIALS['16M']} with 16 MiB, {PARTIALS['three']} with room for three")
    assert not failures, f"{len(failures)} launches failed:\n" + "\n".join(failures[:40])
    # the clamp binds somewhere in every family: the many-split geometries want more than three partials
    assert PARTIALS["16M"] > 3 >= PARTIALS["three"] >= 1, PARTIALS
    missing = {(t, w) for t in FAMILIES[fam][0] for w in WS_MODES} - ran
    assert missing == NEVER[(fam, dt)], f"never ran: {sorted(missing)}; expected: {sorted(NEVER[(fam, dt)])}"


def test_focus_stem_form_runs_on_every_tile_that_accepts_it():
    """cin 16 stored as 12 (the Focus stem's 3x3 stride-1 conv): the tuner may give it any of the 30 tiles, and
    every one built for the operand type takes it (the nine-tap fp32 tiles too: one plain source, whole chunks)."""
    stem = [g for g in ge.WGRAD_GEOMS if g.cin_store < g.cin]
    assert stem and all(g.k == 3 and g.s == 1 and g.cin == 16 and g.cin_store == 12 for g in stem)
    for fam, dt in CASES:
        ran, _, failures, _ = run_family(fam, DT_OF[dt], stem, modes=("grid",), ws_modes=("none", "16M"))
        assert not failures, "\n".join(failures)
        assert {t for t, _ in ran} == set(FAMILIES[fam][0]), (fam, dt, sorted(ran))
