#!/usr/bin/env python3
"""Throughput of the two public serving paths, images in to Detections out.

yolox_s bf16 at 640, batches of 32, 64 batches of in-memory 480 x 640 uint8 RGB arrays per repeat:
  (a) call    a loop of ``yolox(chunk)`` over chunks of 32 (PIL images made from the arrays:
              ``Yolox.__call__`` takes paths or PIL images);
  (b) stream  ``yolox.stream(arrays, batch_size=32)`` (yolox_amd/serve.py); ``stream-tuned`` is the same
              after ``yolox.pipeline(32, tune=True)`` (conv tiles autotuned, as bench.py does).
Each path is warmed up, then timed ``--repeats`` (>= 5) times; the median and min / max images/s are
printed, and the ratio of the medians.  A third step times the host stages of one batch of (b) alone
(packing the images into the pinned staging slot, its H2D copy, formatting the results) and the device
half of the batches back to back with no host packing, in ms per batch, to show which stage bounds
the stream.  bench.py's figure (the same pipeline with the input resident
in HBM and the results left on the device) is the ceiling of (b); the gap to it is host packing, the
H2D copy of the raw images and the result formatting.

Without --step this is the driver: every GPU step is a child process of its own under `timeout`, and
the first one that fails ends the run.

    python tools/serve_bench.py [--out profiles/serve/stream_vs_call.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "pixeltable-yolox_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

STEPS = ("call", "stream", "stream-tuned", "stages")


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=STEPS, help="run one measurement in this process (the driver's children)")
    ap.add_argument("--model", default="yolox_s")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=1, help="untimed passes over all batches")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step (driver)")
    ap.add_argument("--out", default=None, help="also write the report to this file (driver)")
    return ap.parse_args()


def run_step(args) -> dict:
    import numpy as np
    import torch
    from PIL import Image

    from yolox_amd.models import Yolox, YoloxModule, YoloxProcessor

    if args.repeats < 5:
        raise SystemExit("--repeats must be at least 5")
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[args.dtype]
    yolox = Yolox(YoloxModule.synthetic(args.model, seed=0, device="cuda", dtype=dtype), YoloxProcessor(args.model))
    rng = np.random.default_rng(7)
    distinct = [rng.integers(0, 256, (args.height, args.width, 3), dtype=np.uint8) for _ in range(2 * args.batch)]
    total = args.batch * args.batches
    arrays = [distinct[i % len(distinct)] for i in range(total)]
    if args.step == "call":
        images = [Image.fromarray(a) for a in distinct]
        chunks = [[images[(i + j) % len(images)] for j in range(args.batch)] for i in range(0, total, args.batch)]

        def once():
            n = 0
            for c in chunks:
                n += len(yolox(c, threshold=args.threshold))
            return n
    else:
        if args.step != "stream":
            yolox.pipeline(args.batch, tune=True)

        def once():
            n = 0
            for _ in yolox.stream(arrays, threshold=args.threshold, batch_size=args.batch):
                n += 1
            return n

    if args.step == "stages":
        return stages(args, yolox, arrays)
    for _ in range(args.warmup):
        assert once() == total
    torch.cuda.synchronize()
    rates = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        n = once()
        torch.cuda.synchronize()
        rates.append(n / (time.perf_counter() - t0))
    return {"step": args.step, "images": total, "images_per_s": [round(r, 1) for r in rates],
            "median": round(statistics.median(rates), 1), "min": round(min(rates), 1), "max": round(max(rates), 1)}


def stages(args, yolox, arrays) -> dict:
    """ms per batch of the stream's host stages, each alone (median of 20)."""
    import numpy as np
    import torch

    from yolox_amd.models.processor import letterbox_fill, letterbox_layout
    from yolox_amd.serve import format_detections

    B = args.batch
    pipe = yolox.pipeline(B)
    dets = list(yolox.stream(arrays[:2 * B], threshold=args.threshold, batch_size=B))
    slot, chunk = pipe.slots[0], arrays[:B]
    pack, h2d, fmt = [], [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    nrows = sum(len(d["labels"]) for d in dets[:B])
    rows = np.zeros((nrows, 8), np.float32)
    offsets = np.concatenate([[0], np.cumsum([len(d["labels"]) for d in dets[:B]])]).astype(np.int32)
    for _ in range(20):
        t0 = time.perf_counter()
        arrs, offs, desc_off = letterbox_layout(chunk, pipe.size)
        letterbox_fill(slot.host.numpy(), arrs, offs, desc_off)
        pack.append((time.perf_counter() - t0) * 1e3)
        nbytes = desc_off + 20 * B
        with torch.cuda.stream(pipe.copy):
            e0.record()
            slot.pool[:nbytes].copy_(slot.host[:nbytes], non_blocking=True)
            e1.record()
        e1.synchronize()
        h2d.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        format_detections(rows, offsets, B)
        fmt.append((time.perf_counter() - t0) * 1e3)
    # the device half alone (tuned plan): the same packed batch launched back to back, two in flight
    packed_at = pipe.pack(slot, chunk)
    other_at = pipe.pack(pipe.slots[1], chunk)
    dev = []
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(40):
            s = pipe.slots[pipe.k % 2]
            pipe.launch(s, packed_at if s is slot else other_at, args.threshold)
            if len(pipe.inflight) == 2:
                pipe.inflight.popleft().done.synchronize()
        pipe.drain()
        dev.append((time.perf_counter() - t0) * 1e3 / 40)
    med = lambda v: round(statistics.median(v), 3)  # noqa: E731
    return {"step": "stages", "device_ms": med(dev), "pack_ms": med(pack), "h2d_ms": med(h2d), "h2d_mib": round(nbytes / 2 ** 20, 1),
            "format_ms": med(fmt), "detections_per_batch": nrows}


def drive(args) -> int:
    passthrough = ["--model", args.model, "--dtype", args.dtype, "--batch", str(args.batch), "--batches",
                   str(args.batches), "--height", str(args.height), "--width", str(args.width), "--threshold",
                   str(args.threshold), "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
    res = {}
    for step in STEPS:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step]
        r = subprocess.run(cmd + passthrough, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:  # a failed, killed or timed-out step: nothing more is started
            print(f"step {step} ended with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
        res[step] = json.loads(r.stdout.strip().splitlines()[-1])
    lines = [f"{args.model} {args.dtype} {args.batch} x {args.batches} images of {args.height}x{args.width} uint8, "
             f"threshold {args.threshold}, {args.repeats} timed repeats after {args.warmup} warm-up pass(es)"]
    for name, label in (("call", "(a) loop of yolox(chunk)"), ("stream", "(b) yolox.stream(...)   "),
                        ("stream-tuned", "(b) with a tuned plan   ")):
        r = res[name]
        lines.append(f"{label}: median {r['median']:9.1f} images/s  min {r['min']:9.1f}  max {r['max']:9.1f}  "
                     f"repeats {r['images_per_s']}")
    lines.append(f"(b) / (a) medians: {res['stream']['median'] / res['call']['median']:.2f}x")
    st = res["stages"]
    lines.append(f"(b) per batch: {args.batch / res['stream']['median'] * 1e3:.3f} ms, tuned "
                 f"{args.batch / res['stream-tuned']['median'] * 1e3:.3f} ms; the device half alone (H2D, letterbox, "
                 f"tuned forward, NMS, pack, D2H; no host packing) {st['device_ms']} ms; host stages alone: packing "
                 f"{st['pack_ms']} ms, H2D of {st['h2d_mib']} MiB {st['h2d_ms']} ms, formatting "
                 f"{st['detections_per_batch']} detections {st['format_ms']} ms")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")
    return 0


def main() -> int:
    args = parse()
    if args.step:
        print(json.dumps(run_step(args)))
        return 0
    return drive(args)


if __name__ == "__main__":
    sys.exit(main())
