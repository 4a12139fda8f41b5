#!/usr/bin/env python3
"""Step time of fine-tuning with frozen modules: yolox_s 640 fp32 batch 8 (bench.py's configs[2] shape), the step
as a captured replay + fused SGD / EMA step (configs[2]'s step form), for

    full                   every parameter trains
    backbone.backbone      freeze_module(model, "backbone.backbone")   CspDarknet frozen, PAFPN + head train
    backbone               freeze_module(model, "backbone")            CspDarknet + PAFPN frozen, the head trains

Alternating repeats on one device: every round times STEPS steps of each variant in turn (host clock around steps
that end in a device synchronise); reported per variant are the median and the range over the rounds, and the conv
/ data-gradient / weight-gradient launches of one eager step (the YOLOX_AMD_TRAIN_LOG record of yolox_amd.train).

``--parent DIR`` (a built checkout of the parent commit) adds the A/B the unfrozen step owes: two child processes,
one per tree, each builds the full step once (tiles tuned, captured) and then times STEPS steps whenever it is told to,
in alternating rounds; the spread of each side is the margin the other is read against.

    python tools/freeze_bench.py [--rounds 7] [--steps 20] [--parent DIR] [--out profiles/freeze/freeze_step.txt]
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --tree DIR (the A/B's children): the checkout whose package and library this process loads
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else REPO
sys.path.insert(0, os.path.join(TREE, "pixeltable-yolox_amd"))
os.environ.setdefault("YOLOX_AMD_TRAIN_LOG", "1")  # the launch record is read in-process, never written

import torch  # noqa: E402

VARIANTS = (("full", None), ("backbone.backbone", "backbone.backbone"), ("backbone", "backbone"))


def build(name, B, S, dev):
    import yolox_amd.train as T
    from yolox_amd.models import YoloxModule
    from yolox_amd.optim import FusedStep
    from yolox_amd.trainer import ModelEMA, get_optimizer, train_one_iter
    from yolox_amd.weights import synthetic_images, synthetic_labels
    model = YoloxModule.synthetic("yolox_s", seed=0, device=dev)
    model.train()
    if name is not None:
        from yolox_amd.utils import freeze_module
        freeze_module(model, name)
    opt = get_optimizer(model, lr=0.01 / 64 * B)
    ema = ModelEMA(model, 0.9998)
    fused = FusedStep(model, opt, ema)
    imgs = torch.from_numpy(synthetic_images(B, S, S, seed=1000)).to(dev).permute(0, 3, 1, 2).float()
    labels = torch.from_numpy(synthetic_labels(B, S, S, seed=2000)).to(dev)
    counts = {}
    for _ in range(3):  # eager: tiles tuned, the repack table recorded; the last one counted
        del T._LAUNCH_LOG[:]
        train_one_iter(model, opt, imgs, labels, ema=ema, fused=fused)
        counts = {k: sum(1 for r in T._LAUNCH_LOG if r[0] == k) for k in ("conv", "dgrad", "wgrad")}
    opt.zero_grad(set_to_none=True)
    cap = T.CapturedTrainStep(model, imgs, labels, dtype=torch.float32)

    def step():
        return train_one_iter(model, opt, imgs, labels, ema=ema, fused=fused, captured=cap)

    for _ in range(3):
        out = step()
    torch.cuda.synchronize()
    frozen = sum(1 for p in model.parameters() if not p.requires_grad)
    return step, counts, frozen, sum(1 for _ in model.parameters()), float(out["total_loss"])


def timed(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def worker(a):
    """A child of the A/B: the full step of --tree, timed once per line read."""
    step = build(None, a.batch, a.size, torch.device("cuda", 0))[0]
    print("ready", flush=True)
    for line in sys.stdin:
        print(f"{timed(step, int(line)):.6f}", flush=True)


def ab_parent(a):
    """-> {label: [ms per step of each round]} for the parent's tree and this one, alternating"""
    import subprocess
    trees = (("parent commit", os.path.abspath(a.parent)), ("this tree", REPO))
    procs = {}
    for label, tree in trees:
        procs[label] = subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), "--tree", tree, "--worker", "--batch", str(a.batch), "--size",
             str(a.size)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=tree)
    ms = {label: [] for label, _ in trees}
    try:
        for label, _ in trees:
            line = procs[label].stdout.readline().strip()
            if line != "ready":
                raise RuntimeError(f"{label}: the child ended before its step was built ({line!r})")
        for _ in range(a.rounds):
            for label, _ in trees:
                procs[label].stdin.write(f"{a.steps}\n")
                procs[label].stdin.flush()
                ms[label].append(float(procs[label].stdout.readline()))
    finally:
        for p in procs.values():
            p.stdin.close()
        for p in procs.values():
            p.wait(timeout=60)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "freeze", "freeze_step.txt"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: A/B of the unfrozen step")
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    dev = torch.device("cuda", 0)
    built = {label: build(name, a.batch, a.size, dev) for label, name in VARIANTS}
    ms = {label: [] for label, _ in VARIANTS}
    for _ in range(a.rounds):
        for label, _ in VARIANTS:
            ms[label].append(timed(built[label][0], a.steps))
    lines = [f"yolox_s {a.size}x{a.size} fp32 batch {a.batch}, captured replay + fused SGD/EMA step, {torch.cuda.get_device_name(0)}",
             f"{a.rounds} alternating rounds of {a.steps} steps per variant; ms per step: median [min .. max]; img/s at the median",
             f"{'frozen':<20}{'frozen tensors':>16}{'ms/step':>28}{'img/s':>9}{'vs full':>9}   launches of one eager step"]
    base = statistics.median(ms["full"])
    for label, _ in VARIANTS:
        _, counts, frozen, total, loss = built[label]
        med = statistics.median(ms[label])
        lines.append(f"{label:<20}{f'{frozen} / {total}':>16}{f'{med:.3f} [{min(ms[label]):.3f} .. {max(ms[label]):.3f}]':>28}"
                     f"{a.batch / med * 1e3:>9.1f}{base / med:>8.2f}x   conv {counts['conv']}, dgrad {counts['dgrad']}, "
                     f"wgrad {counts['wgrad']} (loss {loss:.4f})")
    if a.parent:
        del built
        torch.cuda.empty_cache()
        ab = ab_parent(a)
        lines.append(f"unfrozen step, parent commit against this tree: one process each, {a.rounds} alternating rounds of "
                     f"{a.steps} steps")
        for label, v in ab.items():
            med = statistics.median(v)
            lines.append(f"{label:<20}{'':>16}{f'{med:.3f} [{min(v):.3f} .. {max(v):.3f}]':>28}{a.batch / med * 1e3:>9.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
