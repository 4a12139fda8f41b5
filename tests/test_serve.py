"""The serving pipeline's device-free parts: yxh_detections_pack's argument checks and the host
formatter that turns its packed records into ``Detections`` (yolox_amd/serve.py)."""
import ctypes

import numpy as np


def test_detections_pack_argument_errors_without_a_device():
    from yolox_amd import _native as N
    lib = N.lib()
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf) + 15 & ~15  # any non-null, 16-byte aligned address: never dereferenced

    def call(det=p, counts=p, B=2, A=3, n_valid=2, ratios=p, rows=p, cap=4, offsets=p):
        return lib.yxh_detections_pack(det, counts, B, A, n_valid, ratios, rows, cap, offsets, None)

    cases = [(dict(det=None), b"null"), (dict(counts=None), b"null"), (dict(ratios=None), b"null"),
             (dict(rows=None), b"null"), (dict(offsets=None), b"null"), (dict(B=0), b"batch"),
             (dict(B=-1), b"batch"), (dict(A=0), b"anchors"), (dict(n_valid=-1), b"n_valid"),
             (dict(n_valid=3), b"n_valid"), (dict(cap=-1), b"capacity")]
    for kw, word in cases:
        assert call(**kw) == N.EINVAL, kw
        assert word in lib.yxh_last_error(), (kw, lib.yxh_last_error())


def test_format_detections_equals_the_reference_formatting(oracle):
    """Hand-made det rows of three images (the second without detections), divided by float32(ratio)
    as yxh_detections_pack does: the formatter's Detections equal the oracle's formatting of the
    undivided rows (a CPU fp32 tensor divided by the Python-double ratio) with ==."""
    from yolox_amd.serve import format_detections
    size = (128, 128)
    hws = [(97, 131), (64, 64), (480, 640)]
    tiny = np.float32(1e-45)  # the smallest fp32 denormal
    det = [np.array([[10.5, -3.25, 100.125, 77.0, 0.9, 0.8, 17.0],
                     [-0.0, 1.17549435e-38, tiny, -tiny, 0.33333334, 0.1, 0.0],
                     [3.0e-39, -2.0e-41, 127.99999, 1e-30, 1.0, 1e-20, 79.0]], np.float32),
           None,
           np.array([[1.0, 2.0, 3.0, 4.0, 0.5, 0.25, 3.0]], np.float32)]
    rng = np.random.default_rng(3)
    det[2] = np.concatenate([det[2], np.concatenate([rng.uniform(-20, 150, (40, 4)), rng.uniform(0, 1, (40, 2)),
                                                     rng.integers(0, 80, (40, 1))], 1).astype(np.float32)])
    packed, offsets = [], [0]
    for b, (rows, (h, w)) in enumerate(zip(det, hws)):
        n = 0 if rows is None else len(rows)
        offsets.append(offsets[-1] + n)
        if rows is None:
            continue
        r = np.float32(min(size[0] / h, size[1] / w))
        rec = np.zeros((n, 8), np.float32)
        rec[:, :4] = rows[:, :4] / r
        rec[:, 4:6] = rows[:, 4:6]
        rec.view(np.int32)[:, 6] = rows[:, 6].astype(np.int32)
        rec.view(np.int32)[:, 7] = b
        packed.append(rec)
    got = format_detections(np.concatenate(packed), np.asarray(offsets, np.int32), 3)
    want = [oracle.detections(rows, hw, size) for rows, hw in zip(det, hws)]
    assert got == want
    assert got[1] == {"bboxes": [], "scores": [], "labels": []}
    for g in got:
        assert all(type(v) is int for v in g["labels"]) and all(type(v) is float for v in g["scores"])
        assert all(type(b) is tuple and len(b) == 4 and all(type(v) is float for v in b) for b in g["bboxes"])
    # fewer images than offsets (a short last batch): the rest is dropped
    assert format_detections(np.concatenate(packed), np.asarray(offsets, np.int32), 1) == want[:1]
    assert format_detections(np.zeros((0, 8), np.float32), np.zeros(3, np.int32), 2) == [want[1], want[1]]
