#!/usr/bin/env python3
"""What the COCO data path costs on the device: the pool's resize kernel and the streamed loader.

A COCO-layout dataset is written under a temporary directory (the three tests/golden/images JPEGs
copied under ``--images`` file names, a generated annotation file), then:

  (a) kernel   ``yxh_resize_u8_batch`` over 160 decoded 480 x 640 images (the most a 32-sample mosaic
               + mixup batch can need) into pool slots at img_size (640, 640) -- a copy, the COCO common
               case -- and (416, 416) -- bilinear -- timed with device events over enough launches to
               fill ``--window`` seconds after warm-up, ``--repeats`` times, alternating with
               ``yxh_letterbox_batch`` (YXH_LB_U8_NHWC) on the same sources and target: the same
               per-pixel arithmetic, at least as many bytes written.  Bytes are the compulsory ones
               (every source byte once, every output byte once) over the median time, against the
               HBM peak (8.0 TB/s spec, 6.29 TB/s measured with a float4 copy).
  (b) loader   ``MosaicBatches.next()`` images/s for yolox_s defaults at batch 32 over one pass of the
               dataset: cold (a new StreamedImages: the pass decodes what it reads), warm (the next pass
               over the same pool) and ResidentImages over the same dataset, alternating in one process,
               ``--repeats`` times, each pass drawing the same seeded samples.  Host clock around the
               pass, ended by a device synchronise.

Needs the GPU.  The report is written to ``--out``.

    python tools/data_bench.py [--out profiles/data/coco_stream.txt]
"""
import argparse
import json
import os
import random
import shutil
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "pixeltable-yolox_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "data", "coco_stream.txt"))
    ap.add_argument("--images", type=int, default=512, help="file names in the on-disk dataset")
    ap.add_argument("--kernel-batch", type=int, default=160)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of launches per timed window")
    ap.add_argument("--skip-loader", action="store_true")
    return ap.parse_args()


def golden_jpegs():
    d = os.path.join(REPO, "tests", "golden", "images")
    return sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith(".jpg"))


def write_dataset(root, count, seed=0):
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "train2017"))
    os.makedirs(os.path.join(root, "annotations"))
    sizes = [Image.open(p).size for p in golden_jpegs()]
    images, anns = [], []
    for i in range(count):
        src = golden_jpegs()[i % len(sizes)]
        name = f"{i + 1:012}.jpg"
        shutil.copy(src, os.path.join(root, "train2017", name))
        w, h = sizes[i % len(sizes)]
        images.append(dict(id=i + 1, file_name=name, height=h, width=w))
        for _ in range(int(rng.integers(1, 8))):
            bw, bh = float(rng.uniform(0.05, 0.6) * w), float(rng.uniform(0.05, 0.6) * h)
            x, y = float(rng.uniform(0, w - bw)), float(rng.uniform(0, h - bh))
            anns.append(dict(id=len(anns) + 1, image_id=i + 1, bbox=[x, y, bw, bh], area=bw * bh, iscrowd=0,
                             category_id=int(rng.integers(1, 81))))
    with open(os.path.join(root, "annotations", "instances_train2017.json"), "w") as f:
        json.dump(dict(images=images, annotations=anns, categories=[dict(id=i, name=f"c{i}") for i in range(1, 81)]),
                  f)


def timed(fn, window):
    """Median-ready time of one call of ``fn`` (ms): device events over enough calls to fill ``window``."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    n = max(3, int(window * 1000.0 / max(start.elapsed_time(end), 1e-3)))
    start.record()
    for _ in range(n):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / n


def spread(xs, fmt="{:.4f}"):
    return f"median {fmt.format(statistics.median(xs))} (min {fmt.format(min(xs))}, max {fmt.format(max(xs))})"


def kernel_section(args, lines):
    from yolox_amd import _native as N
    lib = N.lib()
    dev = torch.device("cuda")
    arrays = [np.asarray(Image.open(p).convert("RGB")) for p in golden_jpegs()]
    arrays = [a for a in arrays if a.shape == (480, 640, 3)]
    B = args.kernel_batch
    src_bytes = 480 * 640 * 3
    host = np.concatenate([arrays[i % len(arrays)].reshape(-1) for i in range(B)])
    src = torch.from_numpy(host).to(dev)
    st = N.stream_ptr(dev)
    lines.append(f"(a) kernel time, {B} images of 480 x 640 x 3 uint8 ({len(arrays)} distinct decoded JPEGs), "
                 f"one launch, {args.repeats} alternating repeats of a {args.window} s window")
    for size in ((640, 640), (416, 416)):
        r = min(size[0] / 480, size[1] / 640)
        rh, rw = int(480 * r), int(640 * r)
        slot = (size[0] * size[1] * 3 + 15) & ~15
        descs = (N.ResizeImage * B)(*[N.ResizeImage(i * src_bytes, i * slot, 480, 640, rh, rw) for i in range(B)])
        d_descs = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
        pool = torch.empty(B * slot, dtype=torch.uint8, device=dev)
        lb = np.zeros(B, dtype=[("off", "<i8"), ("h", "<i4"), ("w", "<i4")])
        lb["off"], lb["h"], lb["w"] = np.arange(B) * src_bytes, 480, 640
        d_lb = torch.from_numpy(lb.view(np.uint8)).to(dev)
        canvas = torch.empty((B, size[0], size[1], 3), dtype=torch.uint8, device=dev)

        def resize(flags=N.RESIZE_SWAP_RB):
            N.check(lib.yxh_resize_u8_batch(src.data_ptr(), d_descs.data_ptr(), B, flags, pool.data_ptr(), st))

        def resize_noswap():
            resize(0)

        def letterbox():
            N.check(lib.yxh_letterbox_batch(src.data_ptr(), d_lb.data_ptr(), B, size[0], size[1], N.LB_U8_NHWC,
                                            canvas.data_ptr(), st))

        cases = {"yxh_resize_u8_batch (swap)": resize, "yxh_resize_u8_batch (no swap)": resize_noswap,
                 "yxh_letterbox_batch u8_nhwc": letterbox}
        for fn in cases.values():  # warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        # the pool's image equals the canvas' top-left region with the channels swapped back
        resize_noswap()
        letterbox()
        torch.cuda.synchronize()
        got = pool.view(B, slot)[:, :rh * rw * 3].reshape(B, rh, rw, 3)
        assert torch.equal(got, canvas[:, :rh, :rw]), "resize and letterbox disagree"
        times = {k: [] for k in cases}
        for _ in range(args.repeats):
            for k, fn in cases.items():
                times[k].append(timed(fn, args.window))
        mode = "copy" if (rh, rw) == (480, 640) else "bilinear"
        lines.append(f"  img_size {size}: resized {rh} x {rw} ({mode})")
        for k, ts in times.items():
            out_bytes = (size[0] * size[1] if "letterbox" in k else rh * rw) * 3
            moved = B * (src_bytes + out_bytes)
            rate = moved / (statistics.median(ts) * 1e-3)
            lines.append(f"    {k:32s} ms {spread(ts)}; {moved / 1e6:.1f} MB compulsory -> {rate / 1e12:.2f} TB/s = "
                         f"{100 * rate / HBM_SPEC:.0f}% of spec, {100 * rate / HBM_MEASURED:.0f}% of measured peak")


def loader_section(args, lines, root):
    from yolox_amd.config import named_config
    from yolox_amd.data import GpuMosaicDetection, MosaicBatches, ResidentImages, StreamedImages, TrainTransform
    from yolox_amd.trainer import InfiniteSampler
    cfg = named_config("yolox_s")
    cfg.data_dir = root
    t0 = time.perf_counter()
    ds = cfg.get_dataset()
    t_json = time.perf_counter() - t0
    passes = len(ds) // args.batch

    def loader(images):
        m = GpuMosaicDetection(
            ds, cfg.input_size, preproc=TrainTransform(max_labels=120, flip_prob=cfg.flip_prob, hsv_prob=cfg.hsv_prob),
            degrees=cfg.degrees, translate=cfg.translate, mosaic_scale=cfg.mosaic_scale, mixup_scale=cfg.mixup_scale,
            shear=cfg.shear, enable_mixup=cfg.enable_mixup, mosaic_prob=cfg.mosaic_prob, mixup_prob=cfg.mixup_prob,
            device="cuda", rng=random.Random(0), np_rng=np.random.RandomState(0), resident=images)
        return MosaicBatches(m, InfiniteSampler(len(ds), seed=0), args.batch)

    def one_pass(ld):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(passes):
            ld.next()
        torch.cuda.synchronize()
        return passes * args.batch / (time.perf_counter() - t)

    t0 = time.perf_counter()
    resident = ResidentImages(ds)
    t_res = time.perf_counter() - t0
    one_pass(loader(resident))  # warm-up: code objects, allocator
    rates = {"streamed cold": [], "streamed warm": [], "resident": []}
    stats = []
    for _ in range(args.repeats):
        pool = StreamedImages(ds, workers=cfg.data_num_workers)
        ld = loader(pool)
        rates["streamed cold"].append(one_pass(ld))
        cold = dict(pool.stats)
        rates["streamed warm"].append(one_pass(ld))
        stats.append((cold, dict(pool.stats)))
        rates["resident"].append(one_pass(loader(resident)))
    lines.append("")
    lines.append(f"(b) MosaicBatches.next() images/s, yolox_s defaults (640 x 640, mosaic + mixup), batch {args.batch}, "
                 f"one pass = {passes} batches over {len(ds)} files, {args.repeats} alternating repeats, "
                 f"{cfg.data_num_workers} decode threads")
    lines.append(f"  annotation file read in {t_json:.2f} s; ResidentImages built (every pull_item) in {t_res:.2f} s; "
                 f"streamed pool {pool.capacity} slots, {pool.nbytes / 1e6:.0f} MB")
    for k, xs in rates.items():
        lines.append(f"    {k:14s} images/s {spread(xs, '{:.0f}')}")
    cold, warm = stats[-1]
    lines.append(f"  last repeat, cold pass: {cold}; after the warm pass: {warm}")


def main():
    args = parse()
    if not torch.cuda.is_available():
        sys.exit("data_bench.py needs the GPU")
    lines = [f"tools/data_bench.py on {torch.cuda.get_device_name(0)}"]
    kernel_section(args, lines)
    if not args.skip_loader:
        with tempfile.TemporaryDirectory() as root:
            write_dataset(root, args.images)
            loader_section(args, lines, root)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
