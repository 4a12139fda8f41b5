#!/usr/bin/env python3
"""Golden fixtures of YOLOX-Darknet53, from the REFERENCE's own modules on CPU.

Run in the build container only (needs the reference checkout make_golden.py reads):
    python tests/golden/make_golden_darknet.py

Builds the reference's YoloFpn (yolo_fpn.py) and YoloxHead(80, in_channels=[128, 256, 512],
act="lrelu") inside the reference's YoloxModule, with make_golden.py's seeded weights and BN
calibration, and writes

  tests/golden/bn_stats_yolox_darknet.npz                           calibrated running statistics (found
                                                                    there by yolox_amd.weights.load_bn_stats)
  tests/golden/state_dict_shapes_darknet.json                       keys / shapes (checkpoint contract)
  tests/golden/fwd_yolox_darknet_96x128.npz                         batch-2 96 x 128 eval forward:
                                                                    input_u8, output, fpn0..fpn2
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402
from make_golden import calibrate_bn, load_reference, synthetic_state_dict  # noqa: E402

NAME = "yolox_darknet"
FWD_B, FWD_H, FWD_W = 2, 96, 128


def build(ref) -> nn.Module:
    fpn = G._exec("yolox.models.yolo_fpn", "models/yolo_fpn.py")
    model = ref.yolox.YoloxModule(fpn.YoloFpn(), ref.head.YoloxHead(80, in_channels=[128, 256, 512], act="lrelu"))
    for m in model.modules():  # config.py:162-175
        if isinstance(m, nn.BatchNorm2d):
            m.eps = 1e-3
            m.momentum = 0.03
    model.head.initialize_biases(1e-2)
    model.load_state_dict(synthetic_state_dict(model.state_dict(), seed=0))
    calibrate_bn(model, G.nchw(G.synthetic_images(2, G.CALIB_HW, G.CALIB_HW, G.CALIB_SEED)))
    model.eval()
    return model


def main() -> None:
    if not os.path.isdir(G.REF):
        sys.exit("reference not present: fixtures can only be generated in the build container")
    ref = load_reference()
    model = build(ref)
    sd = model.state_dict()
    path = os.path.join(HERE, "state_dict_shapes_darknet.json")
    with open(path, "w") as f:
        json.dump({NAME: [[k, list(v.shape)] for k, v in sd.items()]}, f)
    print(f"wrote {path} ({len(sd)} keys)")
    stats = {k: v.numpy() for k, v in sd.items() if k.endswith("running_mean") or k.endswith("running_var")}
    path = os.path.join(HERE, f"bn_stats_{NAME}.npz")
    np.savez_compressed(path, **stats)
    print(f"wrote {path} ({len(stats)} tensors)")
    img = G.synthetic_images(FWD_B, FWD_H, FWD_W, seed=7)
    x = G.nchw(img)
    with torch.no_grad():
        feats = model.backbone(x)
        out = model(x)
    G.save(f"fwd_{NAME}_{FWD_H}x{FWD_W}.npz", input_u8=img, output=out.numpy(),
           **{f"fpn{i}": f.numpy() for i, f in enumerate(feats)})


if __name__ == "__main__":
    main()
