#!/usr/bin/env python3
"""Fixture of the IouLoss tests (tests/golden/iou_loss.npz), from the reference on the CPU.

  boxes.*        the reference's IouLoss (losses.py:7-51), loss_type iou and giou, in fp64 and
                 in fp32: the loss, d sum(loss) / d pred and d sum(loss) / d target for
                   rand  N = 1000 pairs at the 640 scale: targets ~ U(40, 600) centres, sizes
                         U(8, 320); preds = target centre + N(0, 0.35 * size) (a tenth of them far
                         away, disjoint), size * exp(N(0, 0.45)) -- IoU spans 0 to 1
                   edge  the hand-built table below, every row in both argument orders
                 The fp32 reference's deviation from the fp64 one is what the device kernels are
                 measured against (tests/test_gpu_iou_loss.py); this script prints it.
  head.<case>.*  the reference YoloxHead(C, width=0.5) with head.iou_loss = IouLoss("none", "giou"):
                 get_losses on outputs = decode(raw) for every batch of tests/simota_cases.py
                 (raw as tests/test_gpu_simota_edges.py raw_of builds it), use_l1 off and on: the
                 six losses and d total_loss / d raw[..., :5], in fp32 and in fp64.

Run on the CPU with the reference checkout present: python tests/golden/make_golden_iou.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import simota_cases as SC  # noqa: E402
from make_golden import load_reference, save  # noqa: E402

TYPES = ("iou", "giou")
RAND_N = 1000
RAND_SEED = 20

# (name, box a, box b); every value is exact in fp32 (and so are the halves), so a tie in fp32 is
# a tie in fp64.  Each row is stored as (a, b) and as (b, a).
EDGE_ROWS = (
    ("identical", (100, 100, 50, 40), (100, 100, 50, 40)),
    ("identical_small", (320.5, 7.25, 3, 9), (320.5, 7.25, 3, 9)),
    ("disjoint", (100, 100, 20, 20), (300, 250, 30, 40)),
    ("disjoint_x_only", (100, 100, 20, 20), (300, 104, 30, 40)),
    ("touch_x_edge", (100, 100, 20, 20), (120, 100, 20, 30)),       # br_x == tl_x == 110
    ("touch_y_edge", (100, 100, 20, 20), (104, 75, 30, 30)),        # br_y == tl_y == 90
    ("nested", (100, 100, 80, 60), (105, 95, 20, 10)),
    ("shared_left", (100, 100, 40, 40), (90, 105, 20, 30)),         # both left edges at 80
    ("shared_right", (100, 100, 40, 40), (110, 95, 20, 20)),        # both right edges at 120
    ("shared_left_right", (100, 100, 40, 40), (100, 110, 40, 20)),  # equal x extent
    ("shared_left_partial", (100, 100, 40, 40), (95, 130, 30, 40)),  # left edges at 80, overlap in y partial
    ("shared_top", (100, 100, 40, 40), (105, 90, 30, 20)),          # both top edges at 80
    ("shared_bottom", (100, 100, 40, 40), (95, 110, 20, 20)),       # both bottom edges at 120
    ("shared_top_bottom", (100, 100, 40, 40), (110, 100, 20, 40)),  # equal y extent
    ("zero_zero_same_point", (50, 60, 0, 0), (50, 60, 0, 0)),       # area_c = 0: the 1e-16 clamp
    ("zero_zero_apart", (50, 60, 0, 0), (80, 100, 0, 0)),           # giou = -1: the clamp bound
    ("zero_zero_apart_x", (50, 60, 0, 0), (80, 60, 0, 0)),          # area_c = 0 with a distance
    ("zero_target_inside", (100, 100, 40, 40), (105, 95, 0, 0)),
    ("tiny_400_apart", (100, 100, 1e-4, 1e-4), (500, 100, 1e-4, 1e-4)),
    ("tiny_400_apart_diag", (100, 100, 1e-4, 1e-4), (420, 340, 1e-4, 1e-4)),
)


def edge_table():
    names, pred, target = [], [], []
    for name, a, b in EDGE_ROWS:
        names += [name, name + ".swapped"]
        pred += [a, b]
        target += [b, a]
    return names, np.asarray(pred, np.float32), np.asarray(target, np.float32)


def rand_boxes():
    rng = np.random.default_rng(RAND_SEED)
    n = RAND_N
    t = np.stack([rng.uniform(40, 600, n), rng.uniform(40, 600, n), rng.uniform(8, 320, n), rng.uniform(8, 320, n)], 1)
    p = t.copy()
    p[:, :2] += rng.normal(0, 0.35, (n, 2)) * t[:, 2:]
    far = rng.random(n) < 0.1
    p[far, :2] += rng.choice([-1.0, 1.0], (int(far.sum()), 2)) * rng.uniform(1.0, 3.0, (int(far.sum()), 2)) * t[far, 2:]
    p[:, 2:] *= np.exp(rng.normal(0, 0.45, (n, 2)))
    return p.astype(np.float32), t.astype(np.float32)


def ref_iou_loss(ref, pred, target, loss_type, dtype):
    p = torch.from_numpy(pred).to(dtype).requires_grad_()
    t = torch.from_numpy(target).to(dtype).requires_grad_()
    loss = ref.losses.IouLoss(reduction="none", loss_type=loss_type)(p, t)
    loss.sum().backward()
    return loss.detach().numpy(), p.grad.numpy(), t.grad.numpy()


def noise(f32, f64, relative):
    err = float(np.abs(f32.astype(np.float64) - f64).max())
    return err / float(np.abs(f64).max()) if relative else err


def gen_boxes(ref, arrays) -> None:
    names, ep, et = edge_table()
    rp, rt = rand_boxes()
    arrays["boxes.edge.names"] = np.array(names)
    for tag, (p, t) in (("rand", (rp, rt)), ("edge", (ep, et))):
        arrays[f"boxes.{tag}.pred"] = p
        arrays[f"boxes.{tag}.target"] = t
        for lt in TYPES:
            res = {}
            for dn, dtype in (("f64", torch.float64), ("f32", torch.float32)):
                res[dn] = ref_iou_loss(ref, p, t, lt, dtype)
                for q, v in zip(("loss", "g_pred", "g_target"), res[dn]):
                    arrays[f"boxes.{tag}.{lt}.{dn}.{q}"] = v
            iou = 1.0 - res["f64"][0] if lt == "giou" else np.sqrt(np.maximum(1.0 - res["f64"][0], 0.0))
            print(f"boxes.{tag}.{lt}: {'giou' if lt == 'giou' else 'iou'} in [{iou.min():.4f}, {iou.max():.4f}]; "
                  f"fp32 reference vs fp64: loss max abs {noise(res['f32'][0], res['f64'][0], False):.3e}, "
                  f"g_pred / max {noise(res['f32'][1], res['f64'][1], True):.3e}, "
                  f"g_target / max {noise(res['f32'][2], res['f64'][2], True):.3e}")


def raw_of(c):
    """tests/test_gpu_simota_edges.py raw_of: the pre-decode head outputs of the batch."""
    if c["raw"] is not None:
        return torch.from_numpy(c["raw"].copy())
    xs, ys, st = (torch.from_numpy(a.copy()) for a in SC.anchors(c["H"], c["W"]))
    raw = torch.from_numpy(c["outputs"].copy())
    raw[..., 0] = raw[..., 0] / st - xs
    raw[..., 1] = raw[..., 1] / st - ys
    raw[..., 2:4] = torch.log(raw[..., 2:4] / st[:, None])
    return raw


def gen_head(ref, arrays) -> None:
    worst = 0.0
    for name in SC.case_names():
        c = SC.get_case(name)
        raw32 = raw_of(c)
        for use_l1 in (False, True):
            tag = "l1" if use_l1 else "nol1"
            out = {}
            for dn, dtype in (("f32", torch.float32), ("f64", torch.float64)):
                head = ref.head.YoloxHead(c["C"], width=0.5)
                head.iou_loss = ref.losses.IouLoss(reduction="none", loss_type="giou")
                head.use_l1 = use_l1
                xs, ys, st = (torch.from_numpy(a.copy()).to(dtype)[None] for a in SC.anchors(c["H"], c["W"]))
                r = raw32.detach().clone().to(dtype).requires_grad_()
                # get_output_and_grid (yolo_head.py:227-230)
                dec = torch.cat([(r[..., :2] + torch.stack([xs[0], ys[0]], 1)) * st[0][:, None],
                                 torch.exp(r[..., 2:4]) * st[0][:, None], r[..., 4:]], -1)
                lab = torch.from_numpy(c["labels"].copy()).to(dtype)
                res = head.get_losses(None, [xs], [ys], [st], lab, dec, [r[..., :4]] if use_l1 else [], dtype)
                res[0].backward()
                out[dn] = (np.array([v.item() if torch.is_tensor(v) else v for v in res], np.float64),
                           r.grad[..., :5].numpy().copy())
                arrays[f"head.{name}.{tag}.{dn}.losses"] = out[dn][0]
                arrays[f"head.{name}.{tag}.{dn}.g_raw5"] = out[dn][1]
            g32, g64 = out["f32"][1], out["f64"][1]
            nz = noise(g32, g64, True) if np.abs(g64).max() > 0 else 0.0
            worst = max(worst, nz)
            print(f"head.{name}.{tag}: giou losses {np.array2string(out['f32'][0], precision=4)}; "
                  f"fp32 vs fp64 gradient / max {nz:.3e}")
    print(f"head: worst fp32-vs-fp64 gradient noise {worst:.3e}")


def main() -> None:
    torch.manual_seed(0)
    ref = load_reference()
    arrays = {}
    gen_boxes(ref, arrays)
    gen_head(ref, arrays)
    save("iou_loss.npz", **arrays)


if __name__ == "__main__":
    main()
