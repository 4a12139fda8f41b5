#!/usr/bin/env python3
"""What decoding JPEGs on the device costs and buys: the host entropy stage, the render kernels,
and the two users that start from files.

The files are the three tests/golden/images photographs (480 x 640 and 640 x 480), re-encoded with
PIL as 4:2:0 at quality 90 -- COCO's common case -- unless a section says 4:4:4 (the files as they
are).  Every comparison alternates its variants in one process, ``--repeats`` times, and reports
median and range.

  (a) host     ``yxh_jpeg_decode`` (Huffman decode to int16 coefficients) against PIL's full decode
               (``np.asarray(Image.open(...).convert("RGB"))``), images/s on 1, 4 and 16 threads over
               the same in-memory files.
  (b) kernel   ``yxh_jpeg_render_batch`` per call (two launches) for 32 images of 480 x 640, 4:2:0 and
               4:4:4, device events over enough calls to fill ``--window`` seconds.
  (c) serving  ``Yolox.stream`` over ``--images`` file names, yolox_s bf16 (synthetic weights), batch
               32 at 640 x 640: the device path (YOLOX_AMD_JPEG=1) against PIL (=0), and the same
               images handed over as decoded arrays.  Host clock around the whole stream.
  (d) loader   ``MosaicBatches.next()`` images/s over one cold pass of a StreamedImages pool (as
               tools/data_bench.py's (b)), device path against PIL.

Needs the GPU.  The report is written to ``--out``.

    python tools/jpeg_bench.py [--out profiles/jpeg/jpeg_decode.txt]
"""
import argparse
import ctypes as C
import io
import json
import os
import random
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "pixeltable-yolox_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "jpeg", "jpeg_decode.txt"))
    ap.add_argument("--images", type=int, default=512, help="file names on disk for (c) and (d)")
    ap.add_argument("--host-images", type=int, default=192, help="in-memory files per timed pass of (a)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of launches per timed window of (b)")
    ap.add_argument("--skip", default="", help="sections to leave out, e.g. 'cd'")
    return ap.parse_args()


def golden_jpegs():
    d = os.path.join(REPO, "tests", "golden", "images")
    return sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith(".jpg"))


def encoded(sampling: str) -> list:
    """The golden photographs as JPEG bytes: '444' as they are, '420' re-encoded."""
    out = []
    for p in golden_jpegs():
        if sampling == "444":
            with open(p, "rb") as f:
                out.append(f.read())
        else:
            buf = io.BytesIO()
            with Image.open(p) as im:
                im.save(buf, "JPEG", subsampling="4:2:0", quality=90)
            out.append(buf.getvalue())
    return out


def spread(xs, fmt="{:.0f}"):
    return f"median {fmt.format(statistics.median(xs))} (min {fmt.format(min(xs))}, max {fmt.format(max(xs))})"


def disjoint_above(a, b) -> bool:
    return statistics.median(a) > statistics.median(b) and min(a) > max(b)


# ------------------------------------------------------------------ (a)
def host_section(args, lines):
    from yolox_amd import _native as N
    lib = N.lib()
    lines.append(f"(a) host stage, images/s over {args.host_images} in-memory files per pass, "
                 f"{args.repeats} alternating repeats")
    for sampling in ("420", "444"):
        files = encoded(sampling)
        files = [files[i % len(files)] for i in range(args.host_images)]
        info = N.JpegInfo()
        need = 0
        for data in files[:3]:
            N.check(lib.yxh_jpeg_probe(data, len(data), C.byref(info)))
            need = max(need, int(info.coef_bytes))
        local = {}

        def entropy(data):
            import threading
            buf = local.setdefault(threading.get_ident(), np.empty(need, np.uint8))
            image = N.JpegImage()
            N.check(lib.yxh_jpeg_decode(data, len(data), buf.ctypes.data, need, C.byref(image)))

        def pil(data):
            with Image.open(io.BytesIO(data)) as im:
                np.asarray(im.convert("RGB"))

        lines.append(f"  {sampling[0]}:{sampling[1]}:{sampling[2]}, {sum(map(len, files[:3])) // 3} bytes a file on average")
        for threads in (1, 4, 16):
            rates = {"yxh_jpeg_decode": [], "PIL full decode": []}
            with ThreadPoolExecutor(threads) as ex:
                for fn in (entropy, pil):
                    list(ex.map(fn, files[:2 * threads]))  # warm-up
                for _ in range(args.repeats):
                    for name, fn in (("yxh_jpeg_decode", entropy), ("PIL full decode", pil)):
                        t = time.perf_counter()
                        list(ex.map(fn, files))
                        rates[name].append(len(files) / (time.perf_counter() - t))
            for name, xs in rates.items():
                lines.append(f"    {threads:2d} thread(s)  {name:16s} {spread(xs)}"
                             + (f"  = {statistics.median(xs) / threads:.0f} per thread" if threads > 1 else ""))


# ------------------------------------------------------------------ (b)
def timed(fn, window):
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


def kernel_section(args, lines):
    from yolox_amd import _native as N
    lib = N.lib()
    dev = torch.device("cuda")
    B = args.batch
    cases = {}
    for sampling in ("420", "444"):
        files = [d for d in encoded(sampling)]
        descs = (N.JpegImage * B)()
        coefs, off, ws_off, dst_off = [], 0, 0, 0
        k = 0
        while k < B:
            data = files[k % len(files)]
            info = N.JpegInfo()
            N.check(lib.yxh_jpeg_probe(data, len(data), C.byref(info)))
            if (info.height, info.width) != (480, 640):
                files.remove(data)
                continue
            buf = np.empty(int(info.coef_bytes), np.uint8)
            N.check(lib.yxh_jpeg_decode(data, len(data), buf.ctypes.data, buf.nbytes, C.byref(descs[k])))
            descs[k].coef_offset, descs[k].ws_offset, descs[k].dst_offset = off, ws_off, dst_off
            coefs.append(buf)
            off += (buf.nbytes + 15) & ~15
            ws_off += int(lib.yxh_jpeg_workspace_bytes(480, 640, info.sampling))
            dst_off += 480 * 640 * 3
            k += 1
        coef = torch.from_numpy(np.concatenate(coefs)).to(dev)
        desc = torch.from_numpy(np.frombuffer(descs, np.uint8).copy()).to(dev)
        ws = torch.empty(ws_off, dtype=torch.uint8, device=dev)
        dst = torch.empty(dst_off, dtype=torch.uint8, device=dev)
        st = N.stream_ptr(dev)

        def render(coef=coef, desc=desc, ws=ws, dst=dst):
            N.check(lib.yxh_jpeg_render_batch(coef.data_ptr(), desc.data_ptr(), B, ws.data_ptr(), dst.data_ptr(), st))

        for _ in range(3):
            render()
        torch.cuda.synchronize()
        with Image.open(io.BytesIO(files[0])) as im:
            want = np.asarray(im.convert("RGB"))
        assert np.array_equal(dst[:480 * 640 * 3].cpu().numpy().reshape(480, 640, 3), want), "render differs from PIL"
        cases[sampling] = (render, coef.numel() + ws_off * 2 + dst_off)
    times = {k: [] for k in cases}
    for _ in range(args.repeats):
        for k, (fn, _) in cases.items():
            times[k].append(timed(fn, args.window))
    lines.append("")
    lines.append(f"(b) yxh_jpeg_render_batch, {B} images of 480 x 640 in one call (jpeg_idct + jpeg_colour), "
                 f"{args.repeats} alternating repeats of a {args.window} s window")
    for k, ts in times.items():
        moved = cases[k][1]
        med = statistics.median(ts)
        lines.append(f"    {k[0]}:{k[1]}:{k[2]}  ms per call {spread(ts, '{:.4f}')}; {B / med * 1e3:.0f} images/s; "
                     f"{moved / 1e6:.1f} MB compulsory (coefficients in, planes out and in, RGB out) -> "
                     f"{moved / (med * 1e-3) / 1e12:.2f} TB/s")


# ------------------------------------------------------------------ (c), (d)
def write_dataset(root, count, seed=0):
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "train2017"))
    os.makedirs(os.path.join(root, "annotations"))
    files = encoded("420")
    sizes = [Image.open(io.BytesIO(d)).size for d in files]
    images, anns, paths = [], [], []
    for i in range(count):
        name = f"{i + 1:012}.jpg"
        paths.append(os.path.join(root, "train2017", name))
        with open(paths[-1], "wb") as f:
            f.write(files[i % len(files)])
        w, h = sizes[i % len(files)]
        images.append(dict(id=i + 1, file_name=name, height=h, width=w))
        for _ in range(int(rng.integers(1, 8))):
            bw, bh = float(rng.uniform(0.05, 0.6) * w), float(rng.uniform(0.05, 0.6) * h)
            x, y = float(rng.uniform(0, w - bw)), float(rng.uniform(0, h - bh))
            anns.append(dict(id=len(anns) + 1, image_id=i + 1, bbox=[x, y, bw, bh], area=bw * bh, iscrowd=0,
                             category_id=int(rng.integers(1, 81))))
    with open(os.path.join(root, "annotations", "instances_train2017.json"), "w") as f:
        json.dump(dict(images=images, annotations=anns, categories=[dict(id=i, name=f"c{i}") for i in range(1, 81)]),
                  f)
    return paths


def serving_section(args, lines, paths):
    from yolox_amd.config import named_config
    from yolox_amd.models import Yolox, YoloxModule, YoloxProcessor
    cfg = named_config("yolox_s")
    yolox = Yolox(YoloxModule.synthetic("yolox_s", device="cuda", dtype=torch.bfloat16), YoloxProcessor(cfg))
    arrays = [np.asarray(Image.open(p)) for p in paths]

    def run(inputs, setting):
        os.environ["YOLOX_AMD_JPEG"] = setting
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = list(yolox.stream(inputs, threshold=0.25, batch_size=args.batch))
        torch.cuda.synchronize()
        return len(out) / (time.perf_counter() - t), out

    variants = {"files, device path (=1)": (paths, "1"), "files, PIL (=0)": (paths, "0"),
                "decoded arrays": (arrays, "0")}
    results = {}
    for k, (inputs, s) in variants.items():  # warm-up; and the three must agree exactly
        results[k] = run(inputs, s)[1]
    ref = results["decoded arrays"]
    assert all(r == ref for r in results.values()), "the three inputs give different Detections"
    yolox.jpeg.reset_stats()
    rates = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, (inputs, s) in variants.items():
            rates[k].append(run(inputs, s)[0])
    lines.append("")
    lines.append(f"(c) Yolox.stream images/s, yolox_s bf16 synthetic weights, batch {args.batch}, 640 x 640, "
                 f"{len(paths)} files of 4:2:0 q90 (equal Detections checked), {args.repeats} alternating repeats")
    for k, xs in rates.items():
        lines.append(f"    {k:26s} {spread(xs)}")
    lines.append(f"  decoder stats over the timed runs: {yolox.jpeg.stats}")
    dev, pil = rates["files, device path (=1)"], rates["files, PIL (=0)"]
    lines.append(f"  rule (DESIGN §15's): device path default only if its median is above PIL's and the ranges are "
                 f"disjoint -> {'MET' if disjoint_above(dev, pil) else 'NOT met'}")
    os.environ.pop("YOLOX_AMD_JPEG", None)


def loader_section(args, lines, root):
    from yolox_amd.config import named_config
    from yolox_amd.data import GpuMosaicDetection, MosaicBatches, StreamedImages, TrainTransform
    from yolox_amd.trainer import InfiniteSampler
    cfg = named_config("yolox_s")
    cfg.data_dir = root
    ds = cfg.get_dataset()
    passes = len(ds) // args.batch

    def cold_pass(setting):
        os.environ["YOLOX_AMD_JPEG"] = setting
        pool = StreamedImages(ds, workers=cfg.data_num_workers)
        m = GpuMosaicDetection(
            ds, cfg.input_size, preproc=TrainTransform(max_labels=120, flip_prob=cfg.flip_prob, hsv_prob=cfg.hsv_prob),
            degrees=cfg.degrees, translate=cfg.translate, mosaic_scale=cfg.mosaic_scale, mixup_scale=cfg.mixup_scale,
            shear=cfg.shear, enable_mixup=cfg.enable_mixup, mosaic_prob=cfg.mosaic_prob, mixup_prob=cfg.mixup_prob,
            device="cuda", rng=random.Random(0), np_rng=np.random.RandomState(0), resident=pool)
        ld = MosaicBatches(m, InfiniteSampler(len(ds), seed=0), args.batch)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(passes):
            ld.next()
        torch.cuda.synchronize()
        return passes * args.batch / (time.perf_counter() - t), pool

    for s in ("1", "0"):
        cold_pass(s)  # warm-up
    rates = {"device path (=1)": [], "PIL (=0)": []}
    for _ in range(args.repeats):
        for k, s in (("device path (=1)", "1"), ("PIL (=0)", "0")):
            r, pool = cold_pass(s)
            rates[k].append(r)
            if s == "1":
                stats = (dict(pool.stats), dict(pool.jpeg.stats))
    lines.append("")
    lines.append(f"(d) MosaicBatches.next() images/s, cold pass (a new StreamedImages each), yolox_s defaults, batch "
                 f"{args.batch}, {passes} batches over {len(ds)} files, {cfg.data_num_workers} decode threads, "
                 f"{args.repeats} alternating repeats")
    for k, xs in rates.items():
        lines.append(f"    {k:18s} {spread(xs)}")
    lines.append(f"  last device-path pass: pool {stats[0]}, decoder {stats[1]}")
    os.environ.pop("YOLOX_AMD_JPEG", None)


def main():
    args = parse()
    if not torch.cuda.is_available():
        sys.exit("jpeg_bench.py needs the GPU")
    lines = [f"tools/jpeg_bench.py on {torch.cuda.get_device_name(0)}, {os.cpu_count()} CPUs visible"]
    if "a" not in args.skip:
        host_section(args, lines)
    if "b" not in args.skip:
        kernel_section(args, lines)
    if "c" not in args.skip or "d" not in args.skip:
        with tempfile.TemporaryDirectory() as root:
            paths = write_dataset(root, args.images)
            if "c" not in args.skip:
                serving_section(args, lines, paths)
            if "d" not in args.skip:
                loader_section(args, lines, root)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
