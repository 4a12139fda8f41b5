"""Pipelined serving: a stream of images in, a stream of ``Detections`` out (``Yolox.stream``).

``Pipeline`` is the loop ``bench.py`` measures, behind the public API.  Per batch:

* the host packs the image bytes, the letterbox descriptors and the fp32 letterbox ratios into one
  of two pinned staging slots, and one H2D copy on a copy stream moves them -- while the batch
  before runs.  An input that is a path or encoded bytes and a baseline JPEG the device decoder
  takes (``yolox_amd.jpeg``) is not decoded on the host: its Huffman decode runs on a thread pool
  straight into the staging slot, coefficients instead of pixels;
* on the forward stream: ``yxh_jpeg_render_batch`` of those coefficients into the pool regions the
  letterbox descriptors point at, the letterbox straight into the captured plan's input, ``plan.replay()``,
  the NMS filter (fed by the head's score records where the plan emits them);
* on a side stream, beside the next batch's forward: the rest of the NMS, ``yxh_detections_pack``
  (boxes divided by the ratio, rows compacted over the batch), one D2H of the offsets plus the first
  ``capacity_rows`` rows into a pinned result slot, an event;
* the host waits for that event only, and builds the batch's ``Detections`` in one vectorised numpy
  pass.

det / counts / packed rows / result slot / staging / NMS workspaces are double-buffered.  At most
two batches are in flight and a batch's results are consumed before the batch two after it is
submitted: that ordering is what keeps every double buffer safe.
"""
from __future__ import annotations

import ctypes
import io
import os
from collections import deque
from itertools import islice
from typing import Iterable, Iterator, Optional

import numpy as np
import torch

from . import _native as N
from .engine import Plan
from .jpeg import Encoded, JpegDecoder, render_batch
from .models.processor import Detections, letterbox_fill, letterbox_layout
from .utils.boxes import _Workspace, postprocess_device

ROW_BYTES = 32  # yxh_detections_pack's record
C_SIZEOF_JPEG_IMAGE = ctypes.sizeof(N.JpegImage)  # yxh_jpeg_image (N.lib() checks it against the library)


def format_detections(rows: np.ndarray, offsets, n: int) -> list[Detections]:
    """The packed records ``rows`` ([N, 8] float32: four box columns already divided by the ratio,
    obj, cls_conf, then label and image index as int32 bits) and the per-image ``offsets`` ->
    ``Detections`` of images 0 .. n-1, as YoloxProcessor.postprocess builds them: boxes as tuples of
    Python floats, scores as the double product of the two fp32 confidences (exact in float64, so the
    same doubles as the reference's ``.item() * .item()``), labels as Python ints."""
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 8)
    cols = rows[:, :4].astype(np.float64).T  # fp32 -> double is exact: the floats tensor.tolist() gives
    boxes = list(zip(cols[0].tolist(), cols[1].tolist(), cols[2].tolist(), cols[3].tolist()))
    scores = (rows[:, 4].astype(np.float64) * rows[:, 5].astype(np.float64)).tolist()
    labels = rows.view(np.int32)[:, 6].tolist()
    out = []
    for b in range(n):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        out.append(Detections(bboxes=boxes[lo:hi], scores=scores[lo:hi], labels=labels[lo:hi]))
    return out


ENCODED_TYPES = (bytes, bytearray, memoryview)  # an encoded image held in memory


def as_array(im) -> np.ndarray:
    """One input of ``Yolox.stream``: a path, the bytes of an encoded image, a PIL image or an
    H x W x 3 uint8 array -> the array (as-is, like the reference's ``np.array(image)``: nothing is
    converted to RGB)."""
    if isinstance(im, np.ndarray):
        return im
    if isinstance(im, ENCODED_TYPES):
        im = io.BytesIO(im)
    if isinstance(im, (str, os.PathLike, io.BytesIO)):
        from PIL import Image
        with Image.open(im) as f:
            return np.asarray(f)
    return np.asarray(im)


def _align16(n: int) -> int:
    return (n + 15) & ~15


class _Slot:
    """One half of every double buffer."""

    def __init__(self, B: int, A: int, header: int, device):
        self.host: Optional[torch.Tensor] = None   # pinned staging: image bytes, descriptors, ratios
        self.pool: Optional[torch.Tensor] = None   # its device copy
        self.det = torch.empty(B, A, 7, dtype=torch.float32, device=device)
        self.counts = torch.zeros(B, dtype=torch.int32, device=device)
        # offsets [B+1] int32 (padded to `header` bytes) followed by B * A packed rows
        self.packed = torch.zeros(header + B * A * ROW_BYTES, dtype=torch.uint8, device=device)
        self.result = torch.zeros(header + B * A * ROW_BYTES, dtype=torch.uint8, pin_memory=True)
        self.workspace = _Workspace()
        self.h2d_done = torch.cuda.Event()
        self.filter_done = torch.cuda.Event()
        self.done = torch.cuda.Event()
        self.n = 0

    def staging(self, nbytes: int, device, dev_bytes: int = 0) -> None:
        """Room for ``nbytes`` of staging and its device copy; the device side may be asked for more
        (``dev_bytes``: regions only the device writes, behind the copied range)."""
        if self.host is None or self.host.numel() < nbytes:
            size = max(nbytes, 1 << 20) * 5 // 4
            self.host = torch.empty(size, dtype=torch.uint8, pin_memory=True)
        need = max(self.host.numel(), dev_bytes)
        if self.pool is None or self.pool.numel() < need:
            self.pool = torch.empty(need if need == self.host.numel() else need * 5 // 4, dtype=torch.uint8,
                                    device=device)


class Pipeline:
    def __init__(self, module, processor, batch_size: int, capacity_rows: Optional[int] = None,
                 tune: bool = False, jpeg: Optional[JpegDecoder] = None):
        if batch_size < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        if module.device.type != "cuda":
            raise RuntimeError("YoloxModule runs on a ROCm device only; call .to('cuda') first")
        self.module, self.processor = module, processor
        self.device, self.dtype = module.device, module.compute_dtype
        self.batch = B = int(batch_size)
        self.size = th, tw = tuple(int(v) for v in processor.config.test_size)
        self.lib = N.lib()
        with torch.cuda.device(self.device):
            # a plan of its own, not plan_for's cached one: eager run() calls rebind a shared plan's ops
            self.plan = Plan(module, B, th, tw, self.dtype, self.device, N.NHWC, torch.uint8)
            self.input = self.plan.static_input()
            if tune:
                self.plan.autotune()
            self.scores = self.plan.enable_scores()  # None (fp32 modules): the filter reads the rows
            self.plan.capture()
            self.anchors = A = self.plan.anchors
            self.capacity = min(B * A, 64 * B if capacity_rows is None else int(capacity_rows))
            if self.capacity < 0:
                raise ValueError(f"capacity_rows must not be negative, got {capacity_rows}")
            self.header = ((B + 1) * 4 + 15) // 16 * 16
            self.main = torch.cuda.Stream(self.device)
            self.side = torch.cuda.Stream(self.device)
            self.copy = torch.cuda.Stream(self.device)
            self.slots = [_Slot(B, A, self.header, self.device) for _ in range(2)]
            for s in self.slots:  # zero-filled and only ever used at this B (yxh_postprocess_scored's contract)
                s.workspace.buf = torch.zeros(int(self.lib.yxh_postprocess_workspace_bytes(B, A)), dtype=torch.uint8,
                                              device=self.device)
            torch.cuda.synchronize(self.device)  # the fills above ran on the caller's stream
        self.jpeg = jpeg if jpeg is not None else JpegDecoder(workers=16)
        self.k = 0
        self.inflight: deque = deque()

    # ------------------------------------------------------------------ one batch
    def submit(self, arrays: list, threshold: float) -> _Slot:
        """Pack and launch one batch of 1 .. B images; nothing is waited for."""
        assert len(self.inflight) < 2
        slot = self.slots[self.k % 2]
        return self.launch(slot, self.pack(slot, arrays), threshold)

    def pack(self, slot: _Slot, arrays: list) -> tuple:
        """Host half of a batch: the image bytes, the letterbox descriptors and the fp32 ratios into the
        slot's pinned staging.  Returns (n, descriptor offset, ratio offset, total bytes, JPEG part);
        the last is None unless the batch holds ``Encoded`` items (``pack_encoded``)."""
        B, (th, tw) = self.batch, self.size
        n = len(arrays)
        assert 0 < n <= B
        if any(isinstance(a, Encoded) for a in arrays):
            return self.pack_encoded(slot, list(arrays))
        arrays, offs, desc_off = letterbox_layout(arrays, self.size)  # ValueError: nothing launched yet
        ratio_off = desc_off + 16 * n
        total = ratio_off + 4 * B
        slot.staging(total, self.device)
        hn = slot.host.numpy()
        letterbox_fill(hn, arrays, offs, desc_off)
        ratios = np.ones(B, np.float32)  # Python double, rounded once to fp32 (processor.py:45-49)
        ratios[:n] = [min(th / a.shape[0], tw / a.shape[1]) for a in arrays]
        hn[ratio_off:total] = ratios.view(np.uint8)
        return n, desc_off, ratio_off, total, None

    def pack_encoded(self, slot: _Slot, items: list) -> tuple:
        """``pack`` for a batch that mixes arrays and ``Encoded`` JPEGs, in input order.  Copied
        range of the slot: array pixels, letterbox descriptors, ratios, JPEG descriptors,
        coefficients; behind it, on the device only: the regions the JPEGs are rendered into (what
        their letterbox descriptors point at) and the component-plane workspace."""
        B, (th, tw) = self.batch, self.size
        n = len(items)
        enc = [k for k, a in enumerate(items) if isinstance(a, Encoded)]
        plain = [k for k in range(n) if not isinstance(items[k], Encoded)]
        if plain:  # the reference's checks, ValueError before anything is launched
            for k, a in zip(plain, letterbox_layout([items[k] for k in plain], self.size)[0]):
                items[k] = a
        for k in enc:
            e = items[k]
            r = min(th / e.height, tw / e.width)
            if int(e.width * r) <= 0 or int(e.height * r) <= 0:
                raise ValueError(f"image {(e.height, e.width)} resizes to nothing at {self.size}")
        m = len(enc)
        src, off = [0] * n, 0
        for k in plain:
            src[k] = off
            off += _align16(items[k].nbytes)
        desc_off = off
        ratio_off = desc_off + 16 * n
        jdesc_off = _align16(ratio_off + 4 * B)
        off = jdesc_off + C_SIZEOF_JPEG_IMAGE * m
        coef = []
        for k in enc:
            coef.append(off)
            off += _align16(items[k].coef_bytes)
        total = off
        ws = []
        for k in enc:  # device-only regions
            src[k] = off
            off += _align16(items[k].rgb_bytes)
        for k in enc:
            ws.append(off)
            off += items[k].workspace_bytes
        slot.staging(total, self.device, off)
        hn = slot.host.numpy()
        decoded = self.jpeg.decode([items[k] for k in enc], slot.host.data_ptr(), coef)
        if any(err is not None for _, err in decoded):
            # a file the probe took and the entropy decoder refused goes to PIL, which may raise as
            # it always did; the batch is packed again with it as an array
            self.jpeg.stats["device"] -= sum(err is None for _, err in decoded)
            for k, (_, err) in zip(enc, decoded):
                if err is not None:
                    items[k] = as_array(items[k].data)
            return self.pack(slot, items)
        descs = (N.JpegImage * m)()
        for j, (k, (image, _)) in enumerate(zip(enc, decoded)):
            image.coef_offset, image.dst_offset, image.ws_offset = coef[j], src[k], ws[j]
            descs[j] = image
        hn[jdesc_off:jdesc_off + C_SIZEOF_JPEG_IMAGE * m] = np.frombuffer(descs, np.uint8)
        for k in plain:
            a = items[k]
            hn[src[k]:src[k] + a.nbytes] = a.reshape(-1) if a.flags.c_contiguous else np.ascontiguousarray(a).reshape(-1)
        shapes = [(a.height, a.width) if isinstance(a, Encoded) else a.shape[:2] for a in items]
        desc = np.zeros(n, dtype=[("off", "<i8"), ("h", "<i4"), ("w", "<i4")])
        desc["off"] = src
        desc["h"] = [h for h, _ in shapes]
        desc["w"] = [w for _, w in shapes]
        hn[desc_off:ratio_off] = desc.view(np.uint8)
        ratios = np.ones(B, np.float32)
        ratios[:n] = [min(th / h, tw / w) for h, w in shapes]
        hn[ratio_off:ratio_off + 4 * B] = ratios.view(np.uint8)
        return n, desc_off, ratio_off, total, (m, jdesc_off)

    def launch(self, slot: _Slot, packed_at: tuple, threshold: float) -> _Slot:
        """Device half of a batch, asynchronous: H2D, letterbox, forward, NMS, pack, D2H, event."""
        B, A, (th, tw) = self.batch, self.anchors, self.size
        n, desc_off, ratio_off, total, encoded = packed_at
        cfg = self.processor.config
        caller = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self.copy):
            slot.pool[:total].copy_(slot.host[:total], non_blocking=True)
            slot.h2d_done.record(self.copy)
        pool = slot.pool.data_ptr()
        with torch.cuda.stream(self.main):
            if not self.inflight:
                self.main.wait_stream(caller)  # weights the caller's stream was still writing
            self.main.wait_event(slot.h2d_done)
            if encoded is not None:  # coefficients -> RGB, where the letterbox descriptors point
                m, jdesc_off = encoded
                render_batch(pool, pool + jdesc_off, m, pool, pool, self.main.cuda_stream)
            # only the n new images: the other input slots keep their stale contents, n_valid drops them
            N.check(self.lib.yxh_letterbox_batch(pool, pool + desc_off, n, th, tw, N.LB_U8_NHWC,
                                                 self.input.data_ptr(), self.main.cuda_stream), "letterbox")
            out = self.plan.replay()
            postprocess_device(out, cfg.num_classes, float(threshold), cfg.nmsthre, class_agnostic=False,
                               det=slot.det, counts=slot.counts, filter_done=slot.filter_done,
                               rest_stream=self.side, scores=self.scores, workspace=slot.workspace)
        with torch.cuda.stream(self.side):
            packed = slot.packed.data_ptr()
            # the device buffer holds all B * A rows (nothing is ever lost); self.capacity only bounds
            # the first copy to the host
            N.check(self.lib.yxh_detections_pack(slot.det.data_ptr(), slot.counts.data_ptr(), B, A, n,
                                                 pool + ratio_off, packed + self.header, B * A, packed,
                                                 self.side.cuda_stream), "detections_pack")
            nbytes = self.header + self.capacity * ROW_BYTES
            slot.result[:nbytes].copy_(slot.packed[:nbytes], non_blocking=True)
            slot.done.record(self.side)
        slot.n = n
        self.k += 1
        self.inflight.append(slot)
        return slot

    def collect(self) -> list[Detections]:
        """Wait for the oldest batch in flight and format its results."""
        slot = self.inflight.popleft()
        slot.done.synchronize()
        B, hdr = self.batch, self.header
        res = slot.result.numpy()
        offsets = res[:(B + 1) * 4].view(np.int32).copy()
        total = int(offsets[B])
        if total > self.capacity:  # the rows the first copy left on the device (packed holds all B * A)
            lo, hi = hdr + self.capacity * ROW_BYTES, hdr + total * ROW_BYTES
            with torch.cuda.stream(self.copy):
                slot.result[lo:hi].copy_(slot.packed[lo:hi], non_blocking=True)
            self.copy.synchronize()
        rows = res[hdr:hdr + total * ROW_BYTES].view(np.float32).reshape(total, 8)
        return format_detections(rows, offsets, slot.n)

    def drain(self) -> None:
        """Wait for whatever is still in flight (an abandoned or failed stream) and forget it."""
        while self.inflight:
            self.inflight.popleft().done.synchronize()

    # ------------------------------------------------------------------ the stream
    def prepare(self, im):
        """One input -> what ``pack`` takes: an ``Encoded`` for a path or encoded bytes the device
        JPEG decoder accepts (three components: ``as_array`` hands a grayscale file on as 2-D, which
        the reference rejects), else ``as_array``'s array."""
        if isinstance(im, (str, os.PathLike) + ENCODED_TYPES):
            if self.jpeg.on:
                data = self.jpeg.read(im)
                return self.jpeg.accept(data) or as_array(data)
            self.jpeg.accept(b"")  # counted: handed to PIL, the device path is off
        return as_array(im)

    def run(self, inputs: Iterable, threshold: float) -> Iterator[Detections]:
        it = iter(inputs)
        exhausted = False
        try:
            while True:
                while not exhausted and len(self.inflight) < 2:
                    chunk = [self.prepare(im) for im in islice(it, self.batch)]
                    exhausted = len(chunk) < self.batch
                    if chunk:
                        self.submit(chunk, threshold)
                if not self.inflight:
                    return
                # format_detections copies out of the pinned slot: it is free before the next submit
                yield from self.collect()
        finally:
            self.drain()
