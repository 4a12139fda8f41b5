"""COCO-format datasets from disk: the reference's ``CocoDataset`` (datasets/coco.py:32-160)
without pycocotools, cv2 or CacheDataset, and the device resize it feeds.

The annotation file is read as JSON; images are decoded with PIL and come out as
``cv2.imread`` gives them (uint8 H x W x 3 BGR, EXIF orientation applied).
``load_resized_img`` is ``cv2.resize(img, (int(w*r), int(h*r)), INTER_LINEAR)`` restated on the
device (``yxh_resize_u8_batch``, csrc/preprocess.hip): only an image that already has its
resized size is returned without a device, so everything else needs libyoloxhip.so on a ROCm
device -- there is no host resize.  JPEG decoding is libjpeg-turbo through PIL, not cv2's build
of it: decode parity against cv2 is unpinned.
"""
from __future__ import annotations

import copy
import json
import os
from typing import Sequence

import numpy as np

from .. import _native as N

__all__ = ["CocoDataset", "remove_useless_info", "resize_u8_batch"]


def remove_useless_info(coco: dict) -> None:
    """datasets/coco.py:13-29 on the JSON dict, in place."""
    coco.pop("info", None)
    coco.pop("licenses", None)
    for img in coco["images"]:
        for k in ("license", "coco_url", "date_captured", "flickr_url"):
            img.pop(k, None)
    for anno in coco.get("annotations", ()):
        anno.pop("segmentation", None)


def resize_u8_batch(src, descs: Sequence[N.ResizeImage], dst, swap_rb: bool = False) -> None:
    """One ``yxh_resize_u8_batch`` launch on the current stream: ``src`` / ``dst`` are uint8 device
    tensors, ``descs`` the per-image descriptors.  Every descriptor is checked against both
    buffers here (the kernel cannot know their sizes)."""
    import torch
    N.require_device(src, "resize source")
    N.require_device(dst, "resize destination")
    if src.dtype != torch.uint8 or dst.dtype != torch.uint8 or not src.is_contiguous() or not dst.is_contiguous():
        raise ValueError("resize buffers must be contiguous uint8 tensors")
    if len(descs) == 0:
        return
    for k, d in enumerate(descs):
        if min(d.src_h, d.src_w, d.dst_h, d.dst_w) <= 0:
            raise ValueError(f"resize image {k}: empty size {d.src_h}x{d.src_w} -> {d.dst_h}x{d.dst_w}")
        if d.src_offset < 0 or d.src_offset + d.src_h * d.src_w * 3 > src.numel():
            raise ValueError(f"resize image {k}: source range outside the {src.numel()}-byte buffer")
        if d.dst_offset < 0 or d.dst_offset % 16 or d.dst_offset + d.dst_h * d.dst_w * 3 > dst.numel():
            raise ValueError(f"resize image {k}: destination range outside the {dst.numel()}-byte buffer "
                             f"or not 16-aligned")
    arr = (N.ResizeImage * len(descs))(*descs)
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    dev_desc = host.to(dst.device, non_blocking=False)
    N.check(N.lib().yxh_resize_u8_batch(src.data_ptr(), dev_desc.data_ptr(), len(descs),
                                        N.RESIZE_SWAP_RB if swap_rb else 0, dst.data_ptr(),
                                        N.stream_ptr(dst.device)), "yxh_resize_u8_batch")


class CocoDataset:
    """COCO dataset class (datasets/coco.py:32-160): ``<data_dir>/annotations/<json_file>`` and
    the images under ``<data_dir>/<name>/``.  ``coco`` is the parsed JSON dict (what
    CocoEvaluator reads its ground truth from)."""

    def __init__(self, data_dir, json_file: str = "instances_train2017.json", name: str = "train2017",
                 img_size=(416, 416), preproc=None, device="cuda"):
        if data_dir is None:
            raise ValueError("CocoDataset needs data_dir (there is no YOLOX_DATADIR fallback here)")
        self.data_dir = data_dir
        self.json_file = json_file
        with open(os.path.join(self.data_dir, "annotations", self.json_file)) as f:
            self.coco = json.load(f)
        remove_useless_info(self.coco)
        self._imgs = {im["id"]: im for im in self.coco["images"]}
        self.ids = list(self._imgs)  # COCO.getImgIds(): the dict's insertion order
        self.num_imgs = len(self.ids)
        cat_ids = list({c["id"]: c for c in self.coco["categories"]})
        self.class_ids = sorted(cat_ids)
        cats = {c["id"]: c for c in self.coco["categories"]}
        self.cats = [cats[i] for i in cat_ids]  # loadCats(getCatIds()): JSON order (the reference's quirk)
        self._classes = tuple(c["name"] for c in self.cats)
        self._anns: dict = {}
        for a in self.coco.get("annotations", ()):
            self._anns.setdefault(a["image_id"], []).append(a)
        self.name = name
        self.img_size = tuple(img_size)
        self.preproc = preproc
        self.device = device
        self.annotations = [self.load_anno_from_ids(i) for i in self.ids]

    def __len__(self) -> int:
        return self.num_imgs

    def load_anno_from_ids(self, id_):
        """coco.py:90-126 -> (labels float64 [n, 5] scaled by r, (height, width), resized size,
        file name)."""
        im_ann = self._imgs[id_]
        width, height = im_ann["width"], im_ann["height"]
        objs = []
        for obj in self._anns.get(id_, ()):
            if obj.get("iscrowd", 0) != 0:  # getAnnIds(iscrowd=False)
                continue
            x1 = np.max((0, obj["bbox"][0]))
            y1 = np.max((0, obj["bbox"][1]))
            x2 = np.min((width, x1 + np.max((0, obj["bbox"][2]))))
            y2 = np.min((height, y1 + np.max((0, obj["bbox"][3]))))
            if obj["area"] > 0 and x2 >= x1 and y2 >= y1:
                objs.append(([x1, y1, x2, y2], self.class_ids.index(obj["category_id"])))
        res = np.zeros((len(objs), 5))
        for ix, (box, cls) in enumerate(objs):
            res[ix, 0:4] = box
            res[ix, 4] = cls
        r = min(self.img_size[0] / height, self.img_size[1] / width)
        res[:, :4] *= r
        file_name = im_ann["file_name"] if "file_name" in im_ann else "{:012}".format(id_) + ".jpg"
        return res, (height, width), (int(height * r), int(width * r)), file_name

    def load_anno(self, index: int) -> np.ndarray:
        return self.annotations[index][0]

    def image_path(self, index: int) -> str:
        return os.path.join(self.data_dir, self.name, self.annotations[index][3])

    def load_rgb(self, index: int) -> np.ndarray:
        """The decoded image, uint8 H x W x 3 RGB (PIL's order), checked against the JSON's size:
        what the streamed pool uploads (the device resize swaps the channels)."""
        from PIL import Image, ImageOps
        path = self.image_path(index)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"file named {path} not found")
        with Image.open(path) as im:
            im = ImageOps.exif_transpose(im)  # cv2.imread applies the EXIF orientation
            img = np.asarray(im.convert("RGB"), dtype=np.uint8)
        height, width = self.annotations[index][1]
        if img.shape[:2] != (height, width):
            raise ValueError(f"{path} decodes to {img.shape[0]}x{img.shape[1]}, the annotation file says "
                             f"{height}x{width}")
        return img

    def load_image(self, index: int) -> np.ndarray:
        """cv2.imread(file): uint8 H x W x 3 BGR (coco.py:141-149)."""
        return np.ascontiguousarray(self.load_rgb(index)[:, :, ::-1])

    def load_resized_img(self, index: int) -> np.ndarray:
        """coco.py:131-139: the image resized by r to (int(h*r), int(w*r)); on the device unless it
        already has that size."""
        import torch
        img = self.load_image(index)
        h, w = img.shape[:2]
        r = min(self.img_size[0] / h, self.img_size[1] / w)
        rh, rw = int(h * r), int(w * r)
        if (rh, rw) == (h, w):
            return img
        if rh <= 0 or rw <= 0:
            raise ValueError(f"{self.image_path(index)} ({h}x{w}) resizes to an empty image at {self.img_size}")
        src = torch.from_numpy(img.reshape(-1)).to(self.device)
        dst = torch.empty(rh * rw * 3, dtype=torch.uint8, device=self.device)
        d = N.ResizeImage(0, 0, h, w, rh, rw)
        resize_u8_batch(src, [d], dst)
        return dst.cpu().numpy().reshape(rh, rw, 3)

    def pull_item(self, index: int):
        """coco.py:155-160."""
        label, origin_image_size, _, _ = self.annotations[index]
        return self.load_resized_img(index), copy.deepcopy(label), origin_image_size, np.array([self.ids[index]])
