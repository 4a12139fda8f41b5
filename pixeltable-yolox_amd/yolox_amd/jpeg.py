"""Baseline JPEG decoding with the render on the device (include/yoloxhip.h, ``yxh_jpeg_*``).

The Huffman decode is serial and runs on the host in C++ (csrc/jpeg_host.cpp), on a thread pool --
ctypes drops the GIL around every call; dequantisation, IDCT, chroma upsampling and the colour
conversion run as HIP kernels (csrc/jpeg.hip) and reproduce PIL's bytes exactly.  ``JpegDecoder``
is the piece ``serve.Pipeline`` and ``data.StreamedImages`` share: it reads and probes an input,
decodes accepted files straight into the caller's pinned staging, and counts in ``stats`` how many
files went to the device and how many to PIL, with the reason.

``YOLOX_AMD_JPEG=0`` forces PIL everywhere, ``=1`` forces the device path; unset, ``DEFAULT_ON``
decides (DESIGN.md §16 holds the measurement behind it).
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Optional, Sequence

from . import _native as N

__all__ = ["DEFAULT_ON", "JpegDecoder", "Encoded", "device_path_enabled", "exif_orientation"]

DEFAULT_ON = True  # Yolox.stream from files measured 8x PIL's rate, ranges disjoint


def device_path_enabled() -> bool:
    v = os.environ.get("YOLOX_AMD_JPEG", "")
    if v not in ("", "0", "1"):
        raise ValueError(f"YOLOX_AMD_JPEG must be 0 or 1, got {v!r}")
    return DEFAULT_ON if v == "" else v == "1"


class Encoded:
    """An encoded image the device path accepted: its bytes and what the probe read."""

    __slots__ = ("data", "height", "width", "components", "sampling", "coef_bytes")

    def __init__(self, data: bytes, info: N.JpegInfo):
        self.data = data
        self.height, self.width = int(info.height), int(info.width)
        self.components, self.sampling = int(info.components), int(info.sampling)
        self.coef_bytes = int(info.coef_bytes)

    @property
    def rgb_bytes(self) -> int:
        return self.height * self.width * 3

    @property
    def workspace_bytes(self) -> int:
        return int(N.lib().yxh_jpeg_workspace_bytes(self.height, self.width, self.sampling))


def exif_orientation(data: bytes) -> int:
    """The EXIF orientation tag of a JPEG's APP1 segment in front of the scan (1 if there is none):
    what decides whether ``ImageOps.exif_transpose`` would move pixels."""
    p, n = 2, len(data)
    while p + 4 <= n and data[p] == 0xFF:
        m = data[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if m == 0xDA or m == 0xD9:
            break
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            p += 2
            continue
        size = (data[p + 2] << 8) | data[p + 3]
        if size < 2:
            break
        seg = data[p + 4:p + 2 + size]
        p += 2 + size
        if m != 0xE1 or seg[:6] != b"Exif\0\0" or len(seg) < 14:
            continue
        t = seg[6:]
        order = {b"II": "little", b"MM": "big"}.get(bytes(t[:2]))
        if order is None or int.from_bytes(t[2:4], order) != 42:
            continue
        ifd = int.from_bytes(t[4:8], order)
        if ifd + 2 > len(t):
            continue
        for k in range(int.from_bytes(t[ifd:ifd + 2], order)):
            e = ifd + 2 + 12 * k
            if e + 12 > len(t):
                break
            if int.from_bytes(t[e:e + 2], order) == 0x0112:
                return int.from_bytes(t[e + 8:e + 10], order)
    return 1


class JpegDecoder:
    """Reads, probes and entropy-decodes encoded images for the device render.

    ``workers`` sizes the thread pool (``min(16, workers)``, at least 1).  ``enabled``: None follows
    ``YOLOX_AMD_JPEG`` / ``DEFAULT_ON`` at every call, a bool pins it.  ``stats`` counts files only
    (paths and encoded bytes, not arrays or PIL images): ``device`` rendered on the device, ``pil``
    handed to PIL, and ``reasons`` why, by text."""

    def __init__(self, workers: int = 4, enabled: Optional[bool] = None):
        self.workers = min(16, max(1, int(workers)))
        self.enabled = enabled
        self._pool: Optional[ThreadPoolExecutor] = None
        self._lock = threading.Lock()
        self.reset_stats()

    def reset_stats(self) -> None:
        self.stats = {"device": 0, "pil": 0, "reasons": {}}

    @property
    def on(self) -> bool:
        return device_path_enabled() if self.enabled is None else bool(self.enabled)

    def _to_pil(self, reason: str) -> None:
        with self._lock:
            self.stats["pil"] += 1
            self.stats["reasons"][reason] = self.stats["reasons"].get(reason, 0) + 1

    def _executor(self) -> ThreadPoolExecutor:
        if self._pool is None:
            self._pool = ThreadPoolExecutor(self.workers, thread_name_prefix="yxh-jpeg")
        return self._pool

    def close(self) -> None:
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    # ------------------------------------------------------------------ probe
    @staticmethod
    def read(src) -> bytes:
        """The encoded bytes of a path or a bytes-like object."""
        if isinstance(src, (str, os.PathLike)):
            with open(src, "rb") as f:
                return f.read()
        return src if isinstance(src, bytes) else bytes(src)

    def accept(self, data: bytes, gray: bool = False, exif: bool = False) -> Optional[Encoded]:
        """Probe ``data``: an ``Encoded`` if the device path takes it, else None with the reason
        counted.  ``gray``: one-component files are taken too (the caller wants them replicated to
        RGB).  ``exif``: a file whose EXIF orientation is not 1 is left to PIL's ``exif_transpose``."""
        if not self.on:
            self._to_pil("device path off")
            return None
        info = N.JpegInfo()
        rc = N.lib().yxh_jpeg_probe(data, len(data), C.byref(info))
        if rc != N.OK:
            msg = N.lib().yxh_last_error().decode(errors="replace")
            self._to_pil("not a JPEG" if rc == N.EINVAL and data[:2] != b"\xff\xd8" else msg)
            return None
        if info.components == 1 and not gray:
            self._to_pil("grayscale")
            return None
        if exif and exif_orientation(data) != 1:
            self._to_pil("EXIF orientation")
            return None
        return Encoded(data, info)

    # ------------------------------------------------------------------ entropy decode
    @staticmethod
    def _decode_one(job):
        data, ptr, nbytes = job
        image = N.JpegImage()
        rc = N.lib().yxh_jpeg_decode(data, len(data), ptr, nbytes, C.byref(image))
        # the message is thread-local: read it on the thread that made the call
        return image, (None if rc == N.OK else N.lib().yxh_last_error().decode(errors="replace"))

    def decode(self, items: Sequence[Encoded], base_ptr: int, offsets: Sequence[int]) -> list:
        """Entropy-decode ``items`` on the pool, image k's coefficients to ``base_ptr + offsets[k]``
        (caller-owned host memory of at least ``coef_bytes`` each).  -> per item ``(JpegImage,
        None)``, or ``(None, reason)`` for a file the decoder refused (counted as handed to PIL)."""
        jobs = [(e.data, base_ptr + int(o), e.coef_bytes) for e, o in zip(items, offsets)]
        if self.workers > 1 and len(jobs) > 1:
            res = list(self._executor().map(self._decode_one, jobs))
        else:
            res = [self._decode_one(j) for j in jobs]
        out = []
        for image, err in res:
            if err is None:
                with self._lock:
                    self.stats["device"] += 1
                out.append((image, None))
            else:
                self._to_pil(err)
                out.append((None, err))
        return out


def render_batch(coef_ptr: int, desc_ptr: int, batch: int, workspace_ptr: int, dst_ptr: int, stream: int) -> None:
    """One ``yxh_jpeg_render_batch`` call; every pointer is device memory the caller checked."""
    N.check(N.lib().yxh_jpeg_render_batch(coef_ptr, desc_ptr, batch, workspace_ptr, dst_ptr, stream),
            "yxh_jpeg_render_batch")
