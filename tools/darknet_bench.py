#!/usr/bin/env python3
"""YOLOX-Darknet53 baseline on the device (needs an MI355X; there is no CPU path).

Three measurements, each five repeats with the compared forms alternating inside one process, reported
as the median with its range:

  stem     yxh_rgb_stem_conv alone against yxh_rgb_pack + the generic conv (its tile picked by timing every
           applicable candidate once), 640 x 640 uint8 NHWC images, bf16 compute, batch 8; device events
           around a run of launches
  forward  the captured yolox_darknet forward at 640 x 640 bf16, batch 8 and batch 32 (chunked when a
           buffer would pass 2^31 bytes), with plan.flops / time as a fraction of the 2.5 PFLOP/s dense
           bf16 peak: an end-to-end rate over peak, not a kernel's share.  Heuristic tiles: untuned
  stream   Yolox.stream images/s at batch 32 over 640 x 640 uint8 arrays (host wall clock around the
           whole generator, which ends with the last result on the host)

    python tools/darknet_bench.py --out profiles/darknet/darknet53.txt
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "pixeltable-yolox_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from yolox_amd import _native as N  # noqa: E402
from yolox_amd import engine as E  # noqa: E402
from yolox_amd.config import named_config  # noqa: E402
from yolox_amd.models import Yolox, YoloxModule, YoloxProcessor  # noqa: E402
from yolox_amd.weights import synthetic_images  # noqa: E402

PEAK_BF16 = 2.5e15  # dense MFMA FLOP/s
REPEATS = 5


def summary(v):
    return f"median {statistics.median(v):.4f} (range {min(v):.4f} .. {max(v):.4f})"


def time_ops(lib, ops_ptr, n, launches):
    """ms per launch of ``n`` ops starting at ``ops_ptr``, device events around ``launches`` runs"""
    st = N.stream_ptr()
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(launches):
        N.check(lib.yxh_run_ops(ops_ptr, n, st), "run_ops")
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / launches


def pick_tile(lib, plan, index):
    """The fastest applicable tile of conv op ``index`` (each candidate timed over 20 launches)."""
    op = plan._ops[index]
    ptr = C.pointer(op)
    best = (float("inf"), 0)
    for tile in [0] + E.TILE_CANDIDATES_16:
        op.u.conv.tile = tile
        if lib.yxh_run_ops(ptr, 1, N.stream_ptr()) != N.OK:
            continue
        t = time_ops(lib, ptr, 1, 20)
        if t < best[0]:
            best = (t, tile)
    op.u.conv.tile = best[1]
    return best[1]


def bench_stem(model, out, batch=8, hw=640, launches=200):
    lib = N.lib()
    x = torch.from_numpy(synthetic_images(batch, hw, hw, seed=1)).cuda()
    plans = {"kernel": E.Plan(model, batch, hw, hw, torch.bfloat16, "cuda", N.NHWC, torch.uint8),
             "pack+conv": E.Plan(model, batch, hw, hw, torch.bfloat16, "cuda", N.NHWC, torch.uint8, fuse_stem=False)}
    nops = {"kernel": 1, "pack+conv": 2}
    assert plans["kernel"].ctx.ops[0].kind == N.OP_STEM_RGB
    assert [o.kind for o in plans["pack+conv"].ctx.ops[:2]] == [N.OP_RGB_PACK, N.OP_CONV]
    for p in plans.values():
        p.pack_weights()
        p._bind_input(x)
    tile = pick_tile(lib, plans["pack+conv"], 1)
    ptrs = {k: p._ops for k, p in plans.items()}  # the op arrays: the stem is their first op(s)
    for k in plans:  # warm-up
        time_ops(lib, ptrs[k], nops[k], 20)
    times = {k: [] for k in plans}
    for _ in range(REPEATS):
        for k in plans:
            times[k].append(time_ops(lib, ptrs[k], nops[k], launches) * 1e3)
    written = batch * hw * hw * 32 * 2
    out.append(f"stem, batch {batch}, {hw} x {hw} uint8 NHWC, bf16 compute, 3 -> 32 channels, us per launch "
               f"({launches} launches per repeat, {REPEATS} alternating repeats)")
    for k in plans:
        med = statistics.median(times[k])
        extra = f"; conv tile code {tile}" if k == "pack+conv" else ""
        out.append(f"  {k:10s} {summary(times[k])} us   {written / med / 1e6:.2f} TB/s of output written{extra}")
    k_med, f_med = statistics.median(times["kernel"]), statistics.median(times["pack+conv"])
    wins = k_med <= f_med and max(times["kernel"]) <= max(times["pack+conv"]) and min(times["kernel"]) <= min(times["pack+conv"])
    out.append(f"  decision: the kernel's median is {'not above' if k_med <= f_med else 'above'} the fallback's and the "
               f"ranges {'do not overlap the wrong way' if wins else 'overlap the wrong way'}: "
               f"{'kernel' if wins else 'fallback'} is the default")
    return wins


def plan_chunk(model, batch, hw):
    """Images per pass so that no activation buffer reaches 2^31 bytes."""
    probe = E.PlanCtx(1, torch.bfloat16, torch.device("cuda"))
    model.backbone.plan(probe, probe.image(hw, hw))
    per_image = max(b.nelem_image * b.esize for b in probe.buffers)
    chunk = batch
    while chunk > 1 and chunk * per_image >= 1 << 31:
        chunk //= 2
    return chunk


def bench_forward(model, out, hw=640, replays=20):
    out.append(f"captured forward, {hw} x {hw} uint8 NHWC, bf16, heuristic tiles, ms per forward "
               f"({replays} replays per repeat, {REPEATS} repeats)")
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for batch in (8, 32):
        chunk = plan_chunk(model, batch, hw)
        plan = E.Plan(model, batch, hw, hw, torch.bfloat16, "cuda", N.NHWC, torch.uint8, chunk=chunk)
        plan.static_input().copy_(torch.from_numpy(synthetic_images(batch, hw, hw, seed=2)))
        plan.capture()
        for _ in range(3):
            plan.replay()
        torch.cuda.synchronize()
        ms = []
        for _ in range(REPEATS):
            e0.record(stream)
            for _ in range(replays):
                plan.replay()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / replays)
        med = statistics.median(ms)
        out.append(f"  batch {batch:2d} (chunk {chunk}): {summary(ms)} ms   {plan.flops / 1e9 / batch:.1f} GFLOP per image, "
                   f"{plan.flops / (med * 1e-3) / 1e12:.1f} TFLOP/s = {100 * plan.flops / (med * 1e-3) / PEAK_BF16:.1f} % of the "
                   f"dense bf16 peak (whole forward); {batch / (med * 1e-3):.0f} images/s")
        del plan


def bench_stream(model, out, batch=32, images=256, hw=640):
    yolox = Yolox(model, YoloxProcessor(named_config("yolox_darknet")))
    rng = np.random.default_rng(3)
    arrays = [rng.integers(0, 256, (hw, hw, 3), dtype=np.uint8) for _ in range(images)]
    n = sum(1 for _ in yolox.stream(arrays, threshold=0.3, batch_size=batch))  # warm-up: builds the pipeline
    assert n == images
    rates = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        n = sum(1 for _ in yolox.stream(arrays, threshold=0.3, batch_size=batch))
        rates.append(n / (time.perf_counter() - t0))
    out.append(f"Yolox.stream, batch {batch}, {images} uint8 {hw} x {hw} arrays per repeat, images/s: {summary(rates)}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "darknet", "darknet53.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("darknet_bench needs a ROCm device")
    model = YoloxModule.synthetic("yolox_darknet", device="cuda", dtype=torch.bfloat16)
    out = [f"YOLOX-Darknet53 baseline, {torch.cuda.get_device_name(0)}, torch {torch.__version__}", ""]
    bench_stem(model, out)
    out.append("")
    bench_forward(model, out)
    out.append("")
    bench_stream(model, out)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
