"""The id space of yxh_conv_desc.tile: the C family table (csrc/conv_tiles.hpp, read through
yxh_conv_tile_family), its Python mirror (yolox_amd/tiles.py) and the tuners' candidate lists
built from it, which must stay element for element what they were as literals."""
import ctypes

import pytest

from yolox_amd import tiles as T

MAX_ID = 300


def c_families():
    from yolox_amd import _native as N
    lib, rows, f = N.lib(), [], N.TileFamily()
    while lib.yxh_conv_tile_family(len(rows), ctypes.byref(f)) == N.OK:
        rows.append((f.name.decode(), f.first, f.count, f.flags))
        assert len(rows) < 64
    return rows


def test_c_table_is_sorted_disjoint_and_equals_the_python_mirror():
    from yolox_amd import _native as N
    rows = c_families()
    assert b"index" in N.lib().yxh_last_error()  # the walk ended on YXH_EINVAL past the last row
    assert N.lib().yxh_conv_tile_family(-1, ctypes.byref(N.TileFamily())) == N.EINVAL
    assert N.lib().yxh_conv_tile_family(0, None) == N.EINVAL
    for (_, first, count, _), (_, nxt, _, _) in zip(rows, rows[1:]):
        assert count > 0 and first + count <= nxt
    assert rows[0][1] >= 1 and rows[-1][1] + rows[-1][2] - 1 <= MAX_ID
    assert rows == [tuple(f) for f in T.FAMILIES]
    assert len({f.name for f in T.FAMILIES}) == len(T.FAMILIES)


def test_candidate_lists_are_unchanged(monkeypatch):
    """Frozen expectations: the expressions engine.py and train.py held before the lists were built
    from tiles.py.  Equality of lists -- the order decides ties in the tuners."""
    from yolox_amd import engine, train
    tile_candidates = [2 * i + k for i in list(range(1, 10)) + list(range(17, 26)) + list(range(33, 52))
                       + list(range(65, 71)) for k in (0, 1)] + [2 * 81, 2 * 82] + [2 * i for i in range(97, 105)] + [2 * i for i in range(113, 153)] + [2 * i for i in range(161, 197)] + [2 * i + k for i in range(201, 211) for k in (0, 1)] + [2 * i for i in range(221, 237)] + [2 * i + k for i in range(241, 259) for k in (0, 1)] + [2 * i for i in range(261, 281)]
    tile_candidates_16 = [t for t in tile_candidates if (t >> 1) < 17 or (t >> 1) > 96]
    base_tiles = [2 * i + k for i in list(range(1, 10)) + list(range(17, 26)) + list(range(33, 52)) for k in (0, 1)]
    tiles16 = [2 * i for i in list(range(97, 105)) + list(range(161, 191)) + list(range(201, 211))
               + list(range(261, 290)) + list(range(217, 221))]
    conv_tune_tiles_f32 = base_tiles + [2 * (112 + i) for i in (29, 30, 31, 32, 33, 38, 39, 40)] + [2 * i for i in range(211, 217)]
    assert engine.TILE_CANDIDATES == tile_candidates
    assert engine.TILE_CANDIDATES_16 == tile_candidates_16
    assert train._BASE_TILES == base_tiles
    assert train.CONV_TUNE_TILES_F32 == conv_tune_tiles_f32
    # CONV_TUNE_TILES is conv_tune_tiles() of the process's YOLOX_AMD_TRAIN_TILES16
    monkeypatch.setenv("YOLOX_AMD_TRAIN_TILES16", "base")
    assert train.conv_tune_tiles() == base_tiles
    monkeypatch.delenv("YOLOX_AMD_TRAIN_TILES16")
    assert train.conv_tune_tiles() == base_tiles + tiles16
    assert train.CONV_TUNE_TILES in (base_tiles, base_tiles + tiles16)
    assert train.WGRAD_TUNE_TILES == list(range(1, 31))


# every id up to MAX_ID that no row holds.  (153-160 are no gap: the r3 row reserves 48 ids, of which
# conv_r3's own dispatch refuses those it has not built, as it always did.)
GAPS = [(10, 16), (26, 32), (52, 64), (71, 80), (83, 96), (105, 112), (197, 200), (237, 240), (259, 260), (290, 300)]


def test_family_of_gaps_and_range_ends():
    assert T.family_of(0) is None and T.family_of(1) is None
    for lo, hi in GAPS:
        for i in range(lo, hi + 1):
            assert T.family_of(T.code(i)) is None and T.family_of(T.code(i, 1)) is None, i
    for f in T.FAMILIES:
        for i in (f.first, f.first + f.count - 1):
            assert T.family_of(T.code(i)) is f and T.family_of(T.code(i, 1)) is f, (f.name, i)
    covered = sum(f.count for f in T.FAMILIES) + sum(hi - lo + 1 for lo, hi in GAPS)
    assert covered == MAX_ID  # rows and gaps together are exactly ids 1..MAX_ID
    assert T.family_of(T.code(153)) is T.R3 and T.family_of(T.code(160)) is T.R3
    assert T.code(201, 1) == 403 and T.codes(range(1, 3), (0, 1)) == [2, 3, 4, 5]


# ------------------------------------------------------------------ GPU: every code on two tiny convs
SWEEP_GEOMS = {"3x3": (32, 32, 3, 16), "1x1": (64, 64, 1, 16)}  # cin, cout, k, H = W; bf16, s1, batch 1


def sweep(name):
    """{code: status} of every code 2 * id + bit, id 1..MAX_ID, on one of the two convs; asserts what
    holds for each single code on the way."""
    import torch
    from test_gpu_ops import close, make_conv, nhwc, ref_conv, run_conv
    cin, cout, k, hw = SWEEP_GEOMS[name]
    dtype = torch.bfloat16
    conv, bn = make_conv(cin, cout, k, 1, seed=3)
    x = torch.randn(1, cin, hw, hw, generator=torch.Generator().manual_seed(1))
    X, want = nhwc(x, dtype), ref_conv(x, conv, bn, "silu")
    status = {}
    for code in range(2, 2 * MAX_ID + 2):
        try:
            y = run_conv([(X, 0, cin, 0)], conv, bn, dtype, tile=code)  # a fresh zeroed destination
        except ValueError as e:
            status[code] = "EINVAL"
            if T.family_of(code) is None:
                assert "tile" in str(e), (code, str(e))
            continue
        except NotImplementedError:
            status[code] = "EUNSUPPORTED"
            continue
        status[code] = "OK"
        close(y.permute(0, 3, 1, 2), want, dtype)
        assert T.family_of(code) is not None, code
    for code, s in status.items():
        if T.family_of(code) is None:
            assert s == "EINVAL", (code, s)
    return status


def ranges(spans, mul=1):
    return [mul * c for lo, hi in spans for c in range(lo, hi + 1)]


# Recorded by running sweep() on the commit before the family table existed (the ladder of ranges in
# conv.hip), not taken from the table.  Inclusive spans: of tile codes for the 1x1; of ids for the 3x3,
# whose 32 input channels allow no second K slab, so that only even codes (2 * id) get past YXH_EINVAL.
SWEEP_OK = {
    "3x3": ranges([(1, 9), (17, 25), (33, 51), (113, 114), (117, 121), (126, 126), (128, 128), (131, 131),
                   (133, 134), (138, 138), (140, 140), (142, 144), (148, 150), (152, 152), (161, 162),
                   (178, 178)], 2),
    "1x1": ranges([(2, 19), (34, 34), (36, 36), (38, 40), (42, 46), (48, 48), (50, 51), (130, 141), (162, 165),
                   (194, 209), (402, 405), (482, 483), (496, 497)]),
}
SWEEP_EUNSUPPORTED = {
    "3x3": ranges([(65, 70), (81, 82), (97, 104), (115, 116), (122, 124), (129, 130), (132, 132), (139, 139),
                   (145, 147), (151, 151), (163, 168), (171, 177), (179, 196), (201, 236), (241, 258), (261, 269),
                   (271, 272), (274, 274), (276, 276), (279, 289)], 2),
    "1x1": ranges([(35, 35), (37, 37), (41, 41), (47, 47), (49, 49), (66, 103), (226, 393), (406, 473),
                   (484, 495), (498, 517), (522, 579)]),
}


@pytest.mark.gpu
def test_every_tile_code_is_routed_as_before():
    for name in sorted(SWEEP_GEOMS):
        status = sweep(name)
        assert [c for c, s in status.items() if s == "OK"] == SWEEP_OK[name], name
        assert [c for c, s in status.items() if s == "EUNSUPPORTED"] == SWEEP_EUNSUPPORTED[name], name
