"""A/B (GPU box): yolox_s bs32 bf16 forward of a model with few classes, each head level as one
head_pred launch (fuse_head_pred) vs the two 1x1 pred convs, plus a second copy of the off form
(A/A: the noise).  All plans autotuned and graph-captured in ONE process, replays alternated in
rounds so clock and box state are shared.  Usage: python tools/ab_head_pred.py [classes] [rounds]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pixeltable-yolox_amd"))
from yolox_amd import _native as N  # noqa: E402
from yolox_amd.engine import Plan  # noqa: E402
from yolox_amd.models import YoloxModule  # noqa: E402
from yolox_amd.weights import synthetic_images  # noqa: E402

dev = torch.device("cuda:0")
B, S = 32, 640
C = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 11
REP = 100
model = YoloxModule.synthetic("yolox_s", seed=0, device=dev, dtype=torch.bfloat16, num_classes=C)
imgs = torch.from_numpy(synthetic_images(B, S, S, seed=1)).to(dev)
plans = {}
for name, fuse in (("on", True), ("off", False), ("off (A/A)", False)):
    p = Plan(model, B, S, S, torch.bfloat16, dev, N.NHWC, torch.uint8, fuse_head_pred=fuse)
    p.static_input().copy_(imgs)
    p.autotune()
    p.capture()
    plans[name] = p
outs = {k: p.replay().clone() for k, p in plans.items()}
torch.cuda.synchronize()
print(f"{C} classes: max |on - off| {(outs['on'] - outs['off']).abs().max().item():.3g}, "
      f"off == off (A/A): {torch.equal(outs['off'], outs['off (A/A)'])}")
res = {k: [] for k in plans}
s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for r in range(rounds):
    for k, p in plans.items():
        for _ in range(3):
            p.replay()
        s.record()
        for _ in range(REP):
            p.replay()
        e.record()
        e.synchronize()
        res[k].append(s.elapsed_time(e) / REP)
for k, v in res.items():
    heads = sum(1 for o in plans[k].ctx.ops if o.kind == N.OP_HEAD)
    print(f"{k}: forward median {statistics.median(v):.4f} ms, min {min(v):.4f}, max {max(v):.4f} over {len(v)} rounds "
          f"({heads} head_pred launches, {len(plans[k].ctx.ops)} ops)")
