"""CocoDataset (yolox_amd/data/coco.py), the pool's slot bookkeeping and the config wiring, on a
CPU-only host.  The reference's own class needs pycocotools and cv2, which are absent, so the
reader is pinned to the formulas of datasets/coco.py:90-126 written out here."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
from PIL import Image

from yolox_amd.config import named_config
from yolox_amd.data import CocoDataset, SlotTable

CATS = [{"id": 7, "name": "seven"}, {"id": 1, "name": "one"}, {"id": 3, "name": "three"}]


def write_json(root, name, images, annotations, categories=CATS, **extra):
    os.makedirs(os.path.join(root, "annotations"), exist_ok=True)
    with open(os.path.join(root, "annotations", name), "w") as f:
        json.dump(dict(images=images, annotations=annotations, categories=categories, **extra), f)


def ann(i, image_id, bbox, cat, area=None, iscrowd=0):
    return dict(id=i, image_id=image_id, bbox=bbox, category_id=cat, iscrowd=iscrowd,
                area=bbox[2] * bbox[3] if area is None else area, segmentation=[[0, 0, 1, 1]])


@pytest.fixture()
def handmade(tmp_path):
    """Three images whose JSON order (9, 4, 12) is not their id order; categories listed 7, 1, 3."""
    root = str(tmp_path)
    rng = np.random.default_rng(0)
    os.makedirs(os.path.join(root, "train2017"))
    rgb = rng.integers(0, 256, (40, 64, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(os.path.join(root, "train2017", "b.png"))
    grey = rng.integers(0, 256, (20, 30), dtype=np.uint8)
    Image.fromarray(grey, mode="L").save(os.path.join(root, "train2017", "c.png"))
    Image.fromarray(rgb[:10, :10]).save(os.path.join(root, "train2017", "wrong.png"))
    images = [dict(id=9, file_name="b.png", height=40, width=64, coco_url="u", license=1, date_captured="d"),
              dict(id=4, height=100, width=50),
              dict(id=12, file_name="c.png", height=20, width=30),
              dict(id=13, file_name="wrong.png", height=12, width=10),
              dict(id=14, file_name="absent.png", height=12, width=10)]
    anns = [ann(1, 9, [-5, 4, 20, 10], 7),            # negative x: clamped to 0, x2 = 0 + 20
            ann(2, 9, [50, 30, 30, 20], 1),           # crosses the right and bottom edges
            ann(3, 9, [1, 1, 5, 5], 3, area=0),       # dropped: area 0
            ann(4, 9, [2, 2, 6, 6], 3, iscrowd=1),    # dropped: crowd
            ann(5, 4, [10.5, 20, 5, 8], 3)]
    write_json(root, "instances_train2017.json", images, anns, info={"year": 1}, licenses=[1])
    return root, rgb, grey


def test_annotation_arithmetic(handmade):
    root, _, _ = handmade
    ds = CocoDataset(root, img_size=(64, 64))
    assert len(ds) == 5 and ds.ids == [9, 4, 12, 13, 14]  # the JSON's order, not sorted
    assert ds.class_ids == [1, 3, 7]
    assert ds._classes == ("seven", "one", "three") and [c["id"] for c in ds.cats] == [7, 1, 3]
    assert "info" not in ds.coco and "licenses" not in ds.coco
    assert set(ds.coco["images"][0]) == {"id", "file_name", "height", "width"}
    assert all("segmentation" not in a for a in ds.coco["annotations"])
    # image 9: 40 x 64 at (64, 64), r = min(64/40, 64/64) = 1
    res, info, resized, name = ds.annotations[0]
    want = np.array([[0, 4, 20, 14, 2], [50, 30, 64, 40, 0]], np.float64)
    assert res.dtype == np.float64 and np.array_equal(res, want)
    assert info == (40, 64) and resized == (40, 64) and name == "b.png"
    assert ds.load_anno(0) is res
    # image 4: 100 x 50, r = min(64/100, 64/50) = 0.64, no file_name
    r = min(64 / 100, 64 / 50)
    res, info, resized, name = ds.annotations[1]
    want = np.array([[10.5, 20, 15.5, 28, 1]], np.float64)
    want[:, :4] *= r
    assert res.dtype == np.float64 and np.array_equal(res, want)
    assert info == (100, 50) and resized == (int(100 * r), int(50 * r)) == (64, 32)
    assert name == "000000000004.jpg"
    # image 12: no annotations
    assert ds.load_anno(2).shape == (0, 5) and ds.load_anno(2).dtype == np.float64
    assert ds.annotations[2][2] == (int(20 * (64 / 30)), int(30 * (64 / 30)))


def test_load_image(handmade):
    root, rgb, grey = handmade
    ds = CocoDataset(root, img_size=(64, 64))
    img = ds.load_image(0)
    assert img.dtype == np.uint8 and img.flags["C_CONTIGUOUS"]
    assert np.array_equal(img, rgb[:, :, ::-1])  # cv2.imread's BGR
    g = ds.load_image(2)
    assert g.shape == (20, 30, 3)
    for c in range(3):
        assert np.array_equal(g[:, :, c], grey)
    with pytest.raises(ValueError, match="wrong.png"):
        ds.load_image(3)
    with pytest.raises(Exception, match=re.escape(os.path.join(root, "train2017", "absent.png"))):
        ds.load_image(4)


def test_pull_item_that_already_fits_needs_no_device(handmade):
    root, rgb, _ = handmade
    ds = CocoDataset(root, img_size=(64, 64))
    img, labels, info, img_id = ds.pull_item(0)  # 40 x 64 at (64, 64): the copy path
    assert np.array_equal(img, ds.load_image(0)) and np.array_equal(img, rgb[:, :, ::-1])
    assert info == (40, 64)
    assert isinstance(img_id, np.ndarray) and np.array_equal(img_id, np.array([9]))
    assert np.array_equal(labels, ds.load_anno(0))
    labels[:] = -1
    assert ds.load_anno(0)[0, 2] == 20  # a copy: the stored labels are untouched


def test_slot_table_lru_by_batch():
    t = SlotTable(4)
    misses, evicted = t.assign([10, 11, 10, 12])
    assert [i for i, _ in misses] == [10, 11, 12] and evicted == []
    assert len({s for _, s in misses}) == 3
    assert (t.requests, t.hits, t.decodes, t.evictions) == (3, 0, 3, 0)
    slots = {i: t.slot(i) for i in (10, 11, 12)}
    misses, evicted = t.assign([11, 13])  # a hit decodes nothing; 13 takes the free slot
    assert [i for i, _ in misses] == [13] and evicted == []
    assert (t.requests, t.hits, t.decodes, t.evictions) == (5, 1, 4, 0)
    assert t.slot(11) == slots[11]
    # full; least recent batch first: 10 and 12 (first batch, 11 was touched since), in that order
    misses, evicted = t.assign([14])
    assert evicted == [10] and misses == [(14, slots[10])]
    misses, evicted = t.assign([15])
    assert evicted == [12] and misses == [(15, slots[12])]
    assert t.evictions == 2 and 10 not in t and 12 not in t
    # the batch's own images are never evicted: 11 is the least recent, but it is in the batch
    misses, evicted = t.assign([11, 20, 21, 22])
    assert 11 in t and t.slot(11) == slots[11]
    assert sorted(evicted) == [13, 14, 15] and [i for i, _ in misses] == [20, 21, 22]
    assert len({t.slot(i) for i in (11, 20, 21, 22)}) == 4
    before = (t.requests, t.hits, t.decodes, t.evictions)
    with pytest.raises(ValueError, match="5 distinct"):
        t.assign([1, 2, 3, 4, 5, 5])
    assert (t.requests, t.hits, t.decodes, t.evictions) == before and 11 in t
    t.drop([20])
    assert 20 not in t
    misses, evicted = t.assign([30])
    assert evicted == [] and len(misses) == 1  # the dropped slot is free again


def test_config_picks_files_directories_and_sizes(tmp_path):
    root = str(tmp_path)
    for k, name in enumerate(("instances_train2017.json", "instances_val2017.json", "instances_test2017.json")):
        write_json(root, name, [dict(id=i, height=10, width=10) for i in range(k + 1)], [])
    cfg = named_config("yolox_nano")
    assert cfg.get_eval_dataset() is None  # data_dir None: as before
    cfg.update(dict(data_dir=root, input_size="(64, 96)", test_size="(96, 64)"))
    ds = cfg.get_dataset()
    assert (ds.json_file, ds.name, ds.img_size, len(ds)) == ("instances_train2017.json", "train2017", (64, 96), 1)
    ds = cfg.get_eval_dataset()
    assert (ds.json_file, ds.name, ds.img_size, len(ds)) == ("instances_val2017.json", "val2017", (96, 64), 2)
    ds = cfg.get_eval_dataset(testdev=True)
    assert (ds.json_file, ds.name, ds.img_size, len(ds)) == ("instances_test2017.json", "test2017", (96, 64), 3)
    assert ds.data_dir == root
    cfg.num_classes = 2  # the files have three categories
    with pytest.raises(ValueError, match="3 categories"):
        cfg.get_eval_dataset()
    with pytest.raises(ValueError, match="3 categories"):
        cfg.get_data_loader(2, False)
    with pytest.raises(ValueError, match="3 categories"):
        cfg.get_eval_loader(2, False)


def test_resize_entry_abi():
    from yolox_amd import _native as N
    lib = N.lib()
    assert N.ABI_VERSION == 21 and lib.yxh_abi_version() == 21  # additive entry: no bump
    assert lib.yxh_sizeof_resize_image() == ctypes.sizeof(N.ResizeImage) == 32
    assert {"yxh_resize_u8_batch", "yxh_sizeof_resize_image"} <= set(N.EXPORTED)
    p = 4096  # never dereferenced: the checks return first
    assert lib.yxh_resize_u8_batch(None, p, 1, 0, p, None) == N.EINVAL
    assert b"null" in lib.yxh_last_error()
    assert lib.yxh_resize_u8_batch(p, None, 1, 0, p, None) == N.EINVAL
    assert lib.yxh_resize_u8_batch(p, p, 1, 0, None, None) == N.EINVAL
    assert lib.yxh_resize_u8_batch(p, p, 0, 0, p, None) == N.EINVAL
    assert b"batch" in lib.yxh_last_error()
    assert lib.yxh_resize_u8_batch(p, p, 1, 2, p, None) == N.EINVAL
    assert b"flags" in lib.yxh_last_error()
    assert lib.yxh_resize_u8_batch(p, p, 1, N.RESIZE_SWAP_RB | 4, p, None) == N.EINVAL
