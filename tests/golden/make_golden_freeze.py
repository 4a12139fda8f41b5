#!/usr/bin/env python3
"""Golden fixture of a frozen-backbone training step, from the REFERENCE's own modules on CPU.

Run in the build container only (needs the reference checkout make_golden.py reads):
    python tests/golden/make_golden_freeze.py

Builds the reference's yolox_s with make_golden.py's seeded weights and BN calibration (the model of
train_yolox_s_128.npz), puts it in train mode, calls the reference's own
``yolox.utils.model_utils.freeze_module(model.backbone)`` and runs one forward + backward on the inputs
train_yolox_s_128.npz stores (use_l1 False).  Writes

  tests/golden/train_freeze_yolox_s_128.npz   losses (total, iou, l1, conf, cls, num_fg) and the gradient of every
                                              head parameter of at most MAX_NUMEL elements (the preds, the BatchNorms,
                                              stems 0 and 1) and of one 3x3 tower conv (LARGE): what fits under
                                              1 MiB; nothing else (the inputs are the other fixture's)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402

MAX_NUMEL = 33000
LARGE = ("head.cls_convs.0.0.conv.weight",)  # one 3x3 tower weight (147 456 elements) on top: what the size limit leaves


def main() -> None:
    if not os.path.isdir(G.REF):
        sys.exit("reference not present: fixtures can only be generated in the build container")
    ref = G.load_reference()
    mu = G._exec("yolox.utils.model_utils", "utils/model_utils.py")
    d = np.load(os.path.join(HERE, "train_yolox_s_128.npz"))
    model = G.build(ref, "yolox_s")
    model.train()
    model.head.use_l1 = False
    assert mu.freeze_module(model.backbone) is model.backbone
    before = {k: v.clone() for k, v in model.state_dict().items()}
    out = model(G.nchw(d["input_u8"]), torch.from_numpy(d["labels"]))
    out["total_loss"].backward()
    arrays = {}
    for k in ("total_loss", "iou_loss", "l1_loss", "conf_loss", "cls_loss", "num_fg"):
        v = out[k]
        arrays[k] = np.float64(v.item() if torch.is_tensor(v) else v)
    for name, p in model.named_parameters():
        if name.startswith("backbone."):
            assert p.grad is None, name
        else:
            assert p.grad is not None, name
            if p.numel() <= MAX_NUMEL or name in LARGE:
                arrays[f"grad.{name}"] = p.grad.numpy()
    for k, v in model.state_dict().items():  # the frozen half kept its statistics, the head's moved
        if k.startswith("backbone."):
            assert torch.equal(v, before[k]), k
    G.save("train_freeze_yolox_s_128.npz", **arrays)


if __name__ == "__main__":
    main()
