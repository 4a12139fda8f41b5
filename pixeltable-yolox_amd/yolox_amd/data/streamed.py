"""The on-demand image pool for datasets on disk: ``StreamedImages`` hands ``GpuMosaicDetection``
the ``pool`` / ``offsets`` / ``shapes`` / ``labels`` that ``ResidentImages`` does, but decodes an
image only when a batch first asks for it and keeps at most ``capacity`` of them in HBM.

Everything ``draw`` needs (resized shapes, labels, ids) comes from the annotation file, so
construction decodes nothing and the random draws do not depend on what is cached.  ``ensure``
runs before a render: the batch's missing images are decoded as RGB at their original size in a
thread pool (PIL releases the GIL in the decoder), packed into pinned staging, uploaded, and one
``yxh_resize_u8_batch`` launch resizes them -- swapping to BGR on the way -- into fixed-size
slots, on the stream the render uses.  With the device JPEG path on (``yolox_amd.jpeg``,
``YOLOX_AMD_JPEG``), a baseline JPEG whose EXIF orientation is 1 skips PIL: its Huffman decode runs
in the decoder's thread pool into the pinned staging, ``yxh_jpeg_render_batch`` turns the
coefficients into the same RGB bytes on the device, and the same resize follows.  Slots are
``align16(H * W * 3)`` bytes of ``img_size``: a resized image never exceeds it, eviction is a table update and the pool never fragments.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor
from typing import Iterable, Optional

import numpy as np

__all__ = ["SlotTable", "StreamedImages"]


class SlotTable:
    """Which image sits in which of ``capacity`` slots, least-recently-used by batch.  Pure
    bookkeeping (no torch): ``assign`` says what to load where, the caller does the loading."""

    def __init__(self, capacity: int):
        if capacity < 1:
            raise ValueError(f"pool capacity must be at least one slot, got {capacity}")
        self.capacity = int(capacity)
        self._slot: OrderedDict = OrderedDict()  # image -> slot, oldest batch first
        self._free = list(range(self.capacity - 1, -1, -1))
        self.requests = self.hits = self.decodes = self.evictions = 0

    def __contains__(self, image) -> bool:
        return image in self._slot

    def __len__(self) -> int:
        return len(self._slot)

    def slot(self, image) -> int:
        return self._slot[image]

    def assign(self, images: Iterable[int]):
        """Make room for one batch: -> (misses [(image, slot)], evicted [image]).  Images already
        present are hits and become the most recent; the batch's own images are never evicted."""
        batch = dict.fromkeys(images)  # distinct, in request order
        if len(batch) > self.capacity:
            raise ValueError(f"the batch needs {len(batch)} distinct images, the pool holds {self.capacity}")
        self.requests += len(batch)
        slots, missing = self._slot, []
        for i in batch:  # this loop is the whole cost of a warm batch
            if i in slots:
                slots.move_to_end(i)
            else:
                missing.append(i)
        self.hits += len(batch) - len(missing)
        misses, evicted = [], []
        for i in missing:
            if self._free:
                s = self._free.pop()
            else:  # the front is the least recent and, hits having moved to the back, not of this batch
                old, s = self._slot.popitem(last=False)
                evicted.append(old)
                self.evictions += 1
            self._slot[i] = s
            misses.append((i, s))
            self.decodes += 1
        return misses, evicted

    def drop(self, images: Iterable[int]) -> None:
        """Forget images whose load failed; their slots are free again."""
        for i in images:
            s = self._slot.pop(i, None)
            if s is not None:
                self._free.append(s)


def _align16(n: int) -> int:
    return (n + 15) & ~15


class StreamedImages:
    """``ResidentImages``'s surface over a ``CocoDataset``, filled on demand (module docstring).

    ``capacity_slots`` or ``capacity_bytes`` bound the pool; the default is
    ``YOLOX_AMD_DATA_CACHE_GB`` (64 if unset), and never more slots than the dataset has images.
    ``workers`` sizes the decode thread pool (min(16, max(1, workers)))."""

    def __init__(self, dataset, device="cuda", capacity_slots: Optional[int] = None,
                 capacity_bytes: Optional[int] = None, workers: int = 4, staging_bytes: int = 256 << 20):
        import torch
        self.dataset = dataset
        self.device = torch.device(device)
        n = len(dataset)
        self.shapes = np.array([dataset.annotations[i][2] for i in range(n)], np.int64).reshape(n, 2)
        if n and self.shapes.min() <= 0:
            i = int(np.argmin(self.shapes.min(1)))
            raise ValueError(f"image {i} resizes to an empty image ({tuple(self.shapes[i])}) at {dataset.img_size}")
        self.offsets = np.full(n, -1, np.int64)  # -1: not in the pool
        self.labels = [np.array(dataset.load_anno(i), copy=True) for i in range(n)]
        self.infos = [dataset.annotations[i][1] for i in range(n)]
        self.ids = [np.array([dataset.ids[i]]) for i in range(n)]
        self.slot_bytes = _align16(int(dataset.img_size[0]) * int(dataset.img_size[1]) * 3)
        if capacity_slots is None:
            if capacity_bytes is None:
                capacity_bytes = int(float(os.environ.get("YOLOX_AMD_DATA_CACHE_GB", "64")) * (1 << 30))
            capacity_slots = int(capacity_bytes) // self.slot_bytes
            if capacity_slots < 1:
                raise ValueError(f"{capacity_bytes} bytes hold no {self.slot_bytes}-byte slot")
        self.table = SlotTable(min(int(capacity_slots), max(n, 1)))
        self.pool = torch.empty(self.table.capacity * self.slot_bytes, dtype=torch.uint8, device=self.device)
        self.workers = min(16, max(1, int(workers)))
        self.staging_bytes = int(staging_bytes)
        self._host = self._dev = None
        from ..jpeg import JpegDecoder
        self.jpeg = JpegDecoder(workers=self.workers)  # .stats: files rendered on the device / handed to PIL
        # RGB from the decoder and the swap on the device; a dataset without load_rgb gives BGR as is
        self._decode, self._swap = ((dataset.load_rgb, True) if hasattr(dataset, "load_rgb")
                                    else (dataset.load_image, False))

    def __len__(self) -> int:
        return len(self.shapes)

    @property
    def nbytes(self) -> int:
        return self.pool.numel()

    @property
    def capacity(self) -> int:
        return self.table.capacity

    @property
    def stats(self) -> dict:
        t = self.table
        return dict(requests=t.requests, hits=t.hits, decodes=t.decodes, evictions=t.evictions)

    def _src_bytes(self, i: int) -> int:
        h, w = self.infos[i]
        return int(h) * int(w) * 3

    def _staging(self, nbytes: int, dev_bytes: int = 0):
        """Pinned staging of ``nbytes`` and its device copy, which may be asked for more
        (``dev_bytes``: what only the device writes, behind the copied range)."""
        import torch
        if self._host is None or self._host.numel() < nbytes:
            have = 0 if self._host is None else self._host.numel()
            nbytes = max(nbytes, min(2 * have, self.staging_bytes))  # grow geometrically up to the round size
            self._host = torch.empty(nbytes, dtype=torch.uint8)
            if self.device.type == "cuda":
                self._host = self._host.pin_memory()
            self._dev = None
        need = max(self._host.numel(), dev_bytes)
        if self._dev is None or self._dev.numel() < need:
            self._dev = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._host, self._dev

    def ensure(self, indices: Iterable[int]) -> None:
        """Make every listed image present in the pool (on the current stream)."""
        misses, evicted = self.table.assign(indices)
        for i in evicted:
            self.offsets[i] = -1
        if not misses:
            return
        try:
            k = 0
            while k < len(misses):  # rounds of whole images that fit the staging buffer
                j, used = k, 0
                while j < len(misses) and (j == k or used + self._src_bytes(misses[j][0]) <= self.staging_bytes):
                    used += _align16(self._src_bytes(misses[j][0]))
                    j += 1
                self._load(misses[k:j], used)
                k = j
        except BaseException:
            lost = [i for i, _ in misses if self.offsets[i] < 0]
            self.table.drop(lost)
            raise

    def _prepare(self, i: int):
        """One missing image for ``_load``: an ``Encoded`` JPEG the device decoder takes (grayscale
        included, which ``convert("RGB")`` replicates; not a file whose EXIF orientation PIL would
        apply), checked against the annotation file like ``load_rgb`` -- or ``load_rgb``'s array."""
        path = self.dataset.image_path(i)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"file named {path} not found")
        e = self.jpeg.accept(self.jpeg.read(path), gray=True, exif=True)
        if e is None:
            return self._decode(i)
        height, width = (int(v) for v in self.infos[i])
        if (e.height, e.width) != (height, width):
            raise ValueError(f"{path} decodes to {e.height}x{e.width}, the annotation file says "
                             f"{height}x{width}")
        return e

    def _load(self, items, nbytes: int, pil_only=frozenset()) -> None:
        """One copy + launch round: decode ``items`` [(image, slot)], upload, resize into the slots.
        ``pil_only``: images the entropy decoder refused in a first attempt."""
        from .. import _native as N
        from ..jpeg import Encoded, render_batch
        from .coco import resize_u8_batch
        images = [i for i, _ in items]
        on_device = self.jpeg.on and hasattr(self.dataset, "image_path") and hasattr(self.dataset, "load_rgb")

        def fetch(i):
            return self._prepare(i) if on_device and i not in pil_only else self._decode(i)

        if self.workers > 1 and len(images) > 1:
            with ThreadPoolExecutor(min(self.workers, len(images))) as ex:
                decoded = list(ex.map(fetch, images))
        else:
            decoded = [fetch(i) for i in images]
        # copied range: decoded pixels or coefficients per image, then the JPEG descriptors; behind
        # it on the device only: the regions the JPEGs are rendered into and the plane workspace
        src, off = [], 0
        for (i, slot), img in zip(items, decoded):
            src.append(off)
            if isinstance(img, Encoded):
                off += _align16(img.coef_bytes)
                continue
            h, w = (int(v) for v in self.infos[i])
            if img.shape != (h, w, 3) or img.dtype != np.uint8:
                raise ValueError(f"image {i} decodes to {img.shape} {img.dtype}, the annotation file says "
                                 f"{h}x{w}x3 uint8")
            off += _align16(img.size)
        enc = [k for k, img in enumerate(decoded) if isinstance(img, Encoded)]
        jdesc_off = off
        nbytes = off = jdesc_off + C.sizeof(N.JpegImage) * len(enc)
        off = _align16(off)
        rgb, ws = {}, {}
        for k in enc:
            rgb[k] = off
            off += _align16(decoded[k].rgb_bytes)
        for k in enc:
            ws[k] = off
            off += decoded[k].workspace_bytes
        host, dev = self._staging(nbytes, off)
        view = host.numpy()
        if enc:
            res = self.jpeg.decode([decoded[k] for k in enc], host.data_ptr(), [src[k] for k in enc])
            refused = {images[k] for k, (_, err) in zip(enc, res) if err is not None}
            if refused:  # PIL takes them (and raises on them, if it must, as it always did)
                self.jpeg.stats["device"] -= len(enc) - len(refused)
                return self._load(items, nbytes, pil_only | refused)
            jd = (N.JpegImage * len(enc))()
            for j, (k, (image, _)) in enumerate(zip(enc, res)):
                image.coef_offset, image.dst_offset, image.ws_offset = src[k], rgb[k], ws[k]
                jd[j] = image
            view[jdesc_off:nbytes] = np.frombuffer(jd, np.uint8)
        descs = []
        for k, ((i, slot), img) in enumerate(zip(items, decoded)):
            h, w = (int(v) for v in self.infos[i])
            if not isinstance(img, Encoded):
                view[src[k]:src[k] + img.size] = img.reshape(-1)
            rh, rw = (int(v) for v in self.shapes[i])
            descs.append(N.ResizeImage(rgb.get(k, src[k]), slot * self.slot_bytes, h, w, rh, rw))
        dev[:nbytes].copy_(host[:nbytes], non_blocking=False)  # staging is free again when this returns
        if enc:
            p = dev.data_ptr()
            render_batch(p, p + jdesc_off, len(enc), p, p, N.stream_ptr(self.device))
        resize_u8_batch(dev, descs, self.pool, swap_rb=self._swap)
        for (i, slot) in items:
            self.offsets[i] = slot * self.slot_bytes
