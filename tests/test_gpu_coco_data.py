"""COCO-format data on the device: yxh_resize_u8_batch against the oracle's restatement of
cv2.resize (oracle.reference_cpu.letterbox: its [:, :rh, :rw] region is load_resized_img for the
same img_size), CocoDataset.pull_item / the evaluation loader over files, the streamed pool
against the resident one, and the config wiring end to end.  Everything is integer pixels, so
every comparison is exact.  JPEG decoding itself (PIL against cv2) is not pinned."""
import json
import os
import random
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import GOLDEN
from yolox_amd import _native as N
from yolox_amd.data import CocoDataset, GpuMosaicDetection, ResidentImages, StreamedImages, TrainTransform
from yolox_amd.data.coco import resize_u8_batch

pytestmark = pytest.mark.gpu

JPEGS = sorted(os.path.join(GOLDEN, "images", f) for f in os.listdir(os.path.join(GOLDEN, "images"))
               if f.endswith(".jpg"))
# (h, w) -> the resized size at img_size (64, 64) and the path it takes
RAGGED = [((96, 128), (48, 64)),   # area-2x
          ((40, 64), (40, 64)),    # copy
          ((64, 64), (64, 64)),    # copy
          ((20, 31), (41, 64)),    # bilinear, upscale
          ((97, 61), (64, 40)),    # bilinear
          ((33, 130), (16, 64)),   # bilinear
          ((50, 1), (64, 1)),      # bilinear, one pixel wide
          ((1, 50), (1, 64)),      # bilinear, one pixel high
          ((2, 2), (64, 64))]      # bilinear, 32x upscale, every tap clamped
GUARD = 0xA5


def resized_size(h, w, size):
    r = min(size[0] / h, size[1] / w)
    return int(h * r), int(w * r)


def oracle_resize(oracle, img, size):
    rh, rw = resized_size(img.shape[0], img.shape[1], size)
    out = oracle.letterbox(img, size)[:, :rh, :rw]
    return np.ascontiguousarray(out.transpose(1, 2, 0)).astype(np.uint8)


def run_ragged(images, size, misalign, swap):
    """One launch over ``images``: sources packed at offsets pushed off dword alignment by
    ``misalign`` (cycled), destinations 16-aligned with guard gaps and a guard tail.
    -> (results, guard bytes all untouched)."""
    src_off, off = [], 0
    for k, im in enumerate(images):
        off = ((off + 3) & ~3) + misalign[k % len(misalign)]
        src_off.append(off)
        off += im.size
    src = np.full(off + 8, 0x5A, np.uint8)
    for o, im in zip(src_off, images):
        src[o:o + im.size] = im.reshape(-1)
    descs, spans, off = [], [], 32
    for o, im in zip(src_off, images):
        h, w = im.shape[:2]
        rh, rw = resized_size(h, w, size)
        descs.append(N.ResizeImage(o, off, h, w, rh, rw))
        spans.append((off, rh, rw))
        off = ((off + rh * rw * 3 + 15) & ~15) + 16 * (1 + len(descs) % 2)
    dst = torch.full((off + 64,), GUARD, dtype=torch.uint8, device="cuda")
    resize_u8_batch(torch.from_numpy(src).cuda(), descs, dst, swap_rb=swap)
    got = dst.cpu().numpy()
    guard = np.ones(len(got), bool)
    out = []
    for o, rh, rw in spans:
        out.append(got[o:o + rh * rw * 3].reshape(rh, rw, 3))
        guard[o:o + rh * rw * 3] = False
    return out, bool((got[guard] == GUARD).all()) and int(guard.sum()) >= 64 + 32


@pytest.mark.parametrize("swap", [False, True])
def test_resize_kernel_ragged_launch_vs_oracle(oracle, swap):
    rng = np.random.default_rng(5)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w), _ in RAGGED]
    for im, (_, want) in zip(images, RAGGED):
        assert resized_size(im.shape[0], im.shape[1], (64, 64)) == want
    got, guard_ok = run_ragged(images, (64, 64), misalign=(0, 1, 3), swap=swap)
    for im, g in zip(images, got):
        ref = oracle_resize(oracle, im, (64, 64))
        if swap:
            ref = ref[:, :, ::-1]
        bad = np.argwhere(g != ref)
        assert bad.size == 0, f"{im.shape[:2]} -> {g.shape[:2]}: {len(bad)} values differ, first {bad[:4]}"
    assert guard_ok, "a byte outside an image's destination range was written"


@pytest.mark.parametrize("size", [(416, 416), (320, 320)])
def test_resize_kernel_user_sizes_vs_oracle(oracle, size):
    """480 x 640 JPEGs: bilinear at (416, 416), the exact-2x area path at (320, 320)."""
    images = [np.asarray(Image.open(p).convert("RGB")) for p in JPEGS]
    assert len(images) == 3
    got, guard_ok = run_ragged(images, size, misalign=(0, 1), swap=True)
    for im, g in zip(images, got):
        assert np.array_equal(g, oracle_resize(oracle, im, size)[:, :, ::-1])
    assert guard_ok


def test_resize_wrapper_rejects_ranges_outside_the_buffers():
    src = torch.zeros(48, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(64, dtype=torch.uint8, device="cuda")
    for d in (N.ResizeImage(1, 0, 4, 4, 4, 4),      # source runs past the buffer
              N.ResizeImage(0, 32, 4, 4, 4, 4),     # destination runs past the buffer
              N.ResizeImage(0, 8, 4, 4, 2, 2),      # destination not 16-aligned
              N.ResizeImage(0, 0, 4, 4, 0, 4)):     # empty
        with pytest.raises(ValueError):
            resize_u8_batch(src, [d], dst)


# ------------------------------------------------------------------ datasets on disk
PNG_SHAPES = [(96, 128), (20, 31), (97, 61), (33, 130)]
OVERFULL_SEED = 1  # samples 0 and 1 drawn with this seed read 6 distinct images of the 7 (draws are host-only)


def make_dataset(root, split="train2017", json_file="instances_train2017.json", seed=0):
    """The three golden JPEGs and four seeded PNGs, two boxes on each, 80 categories."""
    os.makedirs(os.path.join(root, split), exist_ok=True)
    os.makedirs(os.path.join(root, "annotations"), exist_ok=True)
    rng = np.random.default_rng(seed)
    images, anns = [], []
    files = []
    for p in JPEGS:
        shutil.copy(p, os.path.join(root, split, os.path.basename(p)))
        w, h = Image.open(p).size
        files.append((os.path.basename(p), h, w))
    for k, (h, w) in enumerate(PNG_SHAPES):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, split, f"p{k}.png"))
        files.append((f"p{k}.png", h, w))
    for k, (name, h, w) in enumerate(files):
        img_id = 100 + 7 * k
        images.append(dict(id=img_id, file_name=name, height=h, width=w))
        for j in range(2):
            bw, bh = float(rng.uniform(0.3, 0.8) * w), float(rng.uniform(0.3, 0.8) * h)
            x, y = float(rng.uniform(0, w - bw)), float(rng.uniform(0, h - bh))
            anns.append(dict(id=len(anns) + 1, image_id=img_id, bbox=[x, y, bw, bh], area=bw * bh, iscrowd=0,
                             category_id=int(rng.integers(1, 81))))
    cats = [dict(id=i, name=f"c{i}") for i in range(1, 81)]
    with open(os.path.join(root, "annotations", json_file), "w") as f:
        json.dump(dict(images=images, annotations=anns, categories=cats), f)
    return root


def test_pull_item_resizes_on_the_device(oracle, tmp_path):
    ds = CocoDataset(make_dataset(str(tmp_path)), img_size=(64, 64))
    for i in (0, 3, 4, 6):  # a JPEG (bilinear), PNGs: area-2x, upscale, bilinear
        img, labels, info, img_id = ds.pull_item(i)
        full = ds.load_image(i)
        assert info == full.shape[:2] and int(img_id[0]) == ds.ids[i]
        assert img.shape[:2] == ds.annotations[i][2]
        assert np.array_equal(img, oracle_resize(oracle, full, (64, 64)))
        assert np.array_equal(labels, ds.load_anno(i))


def test_eval_loader_over_files(oracle, tmp_path):
    from yolox_amd.config import named_config
    root = make_dataset(str(tmp_path), "val2017", "instances_val2017.json")
    cfg = named_config("yolox_nano")
    cfg.update(dict(data_dir=root, input_size="(64, 64)", test_size="(64, 64)"))
    loader = cfg.get_eval_loader(2, False)
    imgs, _, (heights, widths), ids = next(iter(loader))
    ds = loader.dataset
    assert isinstance(ds, CocoDataset) and ds.name == "val2017" and len(loader) == 4
    want = np.stack([oracle.letterbox(ds.pull_item(i)[0], (64, 64)) for i in range(2)])
    assert np.array_equal(imgs.cpu().numpy(), want)
    meta = json.load(open(os.path.join(root, "annotations", "instances_val2017.json")))["images"]
    assert heights == [m["height"] for m in meta[:2]] and widths == [m["width"] for m in meta[:2]]
    assert ids == [m["id"] for m in meta[:2]]


def mosaic_pair(ds, capacity):
    kw = dict(preproc=TrainTransform(max_labels=120), device="cuda")
    a = GpuMosaicDetection(ds, (64, 64), rng=random.Random(3), np_rng=np.random.RandomState(3),
                           resident=ResidentImages(ds), **kw)
    b = GpuMosaicDetection(ds, (64, 64), rng=random.Random(3), np_rng=np.random.RandomState(3),
                           resident=StreamedImages(ds, capacity_slots=capacity, workers=4), **kw)
    return a, b


def test_streamed_pool_equals_resident_pool(tmp_path):
    ds = CocoDataset(make_dataset(str(tmp_path)), img_size=(64, 64))
    assert len(ds) == 7
    res, stream = mosaic_pair(ds, 5)
    pool = stream.images
    assert pool.capacity == 5 and pool.nbytes == 5 * 64 * 64 * 3 and pool.stats["decodes"] == 0
    assert np.array_equal(pool.shapes, res.images.shapes)
    for a, b in zip(pool.labels, res.images.labels):
        assert np.array_equal(a, b)
    for k in range(6):  # mosaic + mixup: at most 5 images a sample
        xa, ta = res.get_batch([k])
        xb, tb = stream.get_batch([k])
        assert torch.equal(xa, xb) and torch.equal(ta, tb), f"batch {k}"
    res.close_mosaic()
    stream.close_mosaic()
    for idx in ([6, 2], [0, 5]):
        xa, ta = res.get_batch(idx)
        xb, tb = stream.get_batch(idx)
        assert torch.equal(xa, xb) and torch.equal(ta, tb), f"no-aug batch {idx}"
    for idx in ((True, 4), (False, 3)):  # __getitem__ goes through the same ensure: a mosaic item, a plain one
        (ia, la, fa, da), (ib, lb, fb, db) = res[idx], stream[idx]
        assert torch.equal(ia, ib) and np.array_equal(la, lb) and tuple(fa) == tuple(fb) and int(da[0]) == int(db[0])
    s = pool.stats
    assert s["evictions"] > 0 and s["hits"] > 0 and s["decodes"] < s["requests"], s
    assert s["requests"] == s["hits"] + s["decodes"]
    assert int((pool.offsets >= 0).sum()) == 5 and len(set(pool.offsets[pool.offsets >= 0])) == 5


def test_batch_larger_than_the_pool_is_refused(tmp_path):
    ds = CocoDataset(make_dataset(str(tmp_path)), img_size=(64, 64))
    stream = GpuMosaicDetection(ds, (64, 64), preproc=TrainTransform(max_labels=120), device="cuda",
                                rng=random.Random(OVERFULL_SEED), np_rng=np.random.RandomState(OVERFULL_SEED),
                                resident=StreamedImages(ds, capacity_slots=5))
    drawn = [stream.draw(i) for i in (0, 1)]
    need = len({i for p, _ in drawn for i in (p.indices + [p.cp_index] if p.mix else p.indices)})
    assert need > 5  # what the seed was picked for
    with pytest.raises(ValueError, match=f"needs {need} distinct images"):
        stream.render([p for p, _ in drawn])
    assert stream.images.stats["decodes"] == 0


def test_config_end_to_end(tmp_path):
    from yolox_amd.config import named_config
    from yolox_amd.models import YoloxModule
    from yolox_amd.trainer import InfiniteSampler
    root = make_dataset(str(tmp_path))
    make_dataset(root, "val2017", "instances_val2017.json", seed=1)
    cfg = named_config("yolox_nano")
    cfg.update(dict(data_dir=root, input_size="(64, 64)", test_size="(64, 64)"))
    loader = cfg.get_data_loader(2, False)
    assert isinstance(loader.dataset.images, StreamedImages) and loader.dataset.images.capacity == 7
    random.seed(11)
    np.random.seed(11)
    imgs, targets = loader.next()
    assert imgs.shape == (2, 3, 64, 64) and imgs.dtype == torch.float32 and imgs.is_cuda
    assert targets.shape == (2, 120, 5)
    ds = CocoDataset(root, cfg.train_ann, "train2017", (64, 64))
    hand = GpuMosaicDetection(ds, (64, 64), mosaic=True,
                              preproc=TrainTransform(max_labels=120, flip_prob=cfg.flip_prob, hsv_prob=cfg.hsv_prob),
                              degrees=cfg.degrees, translate=cfg.translate, mosaic_scale=cfg.mosaic_scale,
                              mixup_scale=cfg.mixup_scale, shear=cfg.shear, enable_mixup=cfg.enable_mixup,
                              mosaic_prob=cfg.mosaic_prob, mixup_prob=cfg.mixup_prob, device="cuda")
    it = iter(InfiniteSampler(len(ds), seed=0))
    random.seed(11)
    np.random.seed(11)
    want_imgs, want_targets = hand.get_batch([next(it), next(it)])
    assert torch.equal(targets, want_targets) and torch.equal(imgs, want_imgs)
    model = YoloxModule.synthetic("yolox_nano", seed=0, device="cuda")
    ap50_95, ap50, summary = cfg.get_evaluator(2, False).evaluate(model)
    assert np.isfinite(ap50_95) and np.isfinite(ap50) and isinstance(summary, str)
