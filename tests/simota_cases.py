"""Shared inputs of the SimOTA / loss edge tests: the fixture script (tests/golden/make_golden.py
gen_simota_edges), the oracle test (tests/test_oracle.py) and the device test
(tests/test_gpu_simota_edges.py) all regenerate the same batches from seeds here; only labels
and the reference's results are stored (tests/golden/simota_edges.npz).

Anchors are strides 8 / 16 / 32, level-major and row-major (weights.anchor_grid).  Ground truths:
centres ~ U(8, W-8) x U(8, H-8), sizes ~ U(8, W/2) x U(8, H/2), class ~ U{0..C-1}.  Predictions:

  rand   anchor centre + N(0, 4), sizes U(8, 160) (weights.synthetic_head_outputs): boxes unrelated
         to the ground truths, small IoUs, dynamic_k 1-4
  tight  every anchor predicts its nearest ground truth's box + N(0, 1.5) per coordinate (sizes at
         least 2): large IoUs, dynamic_k up to 9-10, many anchors claimed by several ground truths
  sat    tight, then 5 % of the class logits +40 and 5 % -40, 30 % of the objectness logits +40 and
         10 % -120: sigmoids of exactly 0 and 1, the -100 clamp of the logarithm

Generated batches are 4 images (SEEDS) for each generator over SHAPES: non-square both ways, class
counts on both sides of the kernel's unroll by 8, L == G.  Hand-built batches (HAND) hold
duplicated label rows, a ground truth whose centre is off the image (no anchor inside its own
radius), one with 3 candidates of its own, an image and a whole batch without labels, L == 1 with
fewer than 10 candidates in the image, and predictions that equal their ground truth exactly.

Not included: a ground truth for which the whole image has no candidate at all (say a single label
centred at (-300, -300)).  The reference raises there (torch.cat of an empty list), so there is no
reference result to match.
"""
import numpy as np

STRIDES = (8, 16, 32)
GENERATORS = ("rand", "tight", "sat")
SEEDS = (0, 1, 2, 3)
# (H, W, C, G, L)
SHAPES = ((96, 160, 80, 6, 120), (96, 160, 3, 12, 12), (64, 64, 1, 3, 8), (160, 96, 20, 25, 32))
HAND = ("dup_off_corner", "few_candidates", "all_empty", "exact_hit")
LOSS_KEYS = ("total_loss", "iou_loss", "conf_loss", "cls_loss", "l1_loss", "num_fg")


def level_hw(H, W):
    return [(H // s, W // s) for s in STRIDES]


def anchors(H, W):
    """(x_shifts, y_shifts, strides), each float32 [A]."""
    xs, ys, ss = [], [], []
    for s in STRIDES:
        h, w = H // s, W // s
        yv, xv = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        xs.append(xv.reshape(-1))
        ys.append(yv.reshape(-1))
        ss.append(np.full(h * w, s))
    return tuple(np.concatenate(p).astype(np.float32) for p in (xs, ys, ss))


def gen_labels(rng, H, W, C, G, L):
    lab = np.zeros((L, 5), np.float32)
    lab[:G, 0] = rng.integers(0, C, G)
    lab[:G, 1] = rng.uniform(8, W - 8, G)
    lab[:G, 2] = rng.uniform(8, H - 8, G)
    lab[:G, 3] = rng.uniform(8, W / 2, G)
    lab[:G, 4] = rng.uniform(8, H / 2, G)
    return lab


def gen_image(gen, rng, H, W, C, gts):
    """One image's head outputs [A, 5+C] = (cx, cy, w, h, obj logit, class logits) for the
    ground-truth boxes ``gts`` [G, 4]."""
    xs, ys, st = anchors(H, W)
    A = xs.shape[0]
    xc, yc = (xs + 0.5) * st, (ys + 0.5) * st
    if gen == "rand" or len(gts) == 0:
        box = np.stack([xc + rng.normal(0, 4, A), yc + rng.normal(0, 4, A),
                        rng.uniform(8, 160, A), rng.uniform(8, 160, A)], 1)
    else:
        near = np.argmin((xc[:, None] - gts[None, :, 0]) ** 2 + (yc[:, None] - gts[None, :, 1]) ** 2, 1)
        box = gts[near] + rng.normal(0, 1.5, (A, 4))
        box[:, 2:] = np.maximum(box[:, 2:], 2.0)
    cls = rng.normal(-2, 1.5, (A, C))
    obj = rng.normal(0, 1.5, (A, 1))
    if gen == "sat":
        u = rng.random((A, C))
        cls[u < 0.05] = 40.0
        cls[(u >= 0.05) & (u < 0.10)] = -40.0
        u = rng.random((A, 1))
        obj[u < 0.30] = 40.0
        obj[(u >= 0.30) & (u < 0.40)] = -120.0
    return np.concatenate([box, obj, cls], 1).astype(np.float32)


def _case(name, gen, H, W, C, labels, outputs, origin, raw=None):
    return {"name": name, "gen": gen, "H": H, "W": W, "C": C, "L": labels.shape[1], "hw": level_hw(H, W),
            "labels": labels, "outputs": outputs, "origin": origin, "raw": raw}


def generated_case(gen, shape):
    H, W, C, G, L = shape
    labels, outputs, origin = [], [], []
    for seed in SEEDS:
        rng = np.random.default_rng((seed, GENERATORS.index(gen), H, W, C, G))
        lab = gen_labels(rng, H, W, C, G, L)
        out = gen_image(gen, rng, H, W, C, lab[:G, 1:5].astype(np.float64))
        labels.append(lab)
        outputs.append(out)
        origin.append(rng.normal(0, 1, (out.shape[0], 4)).astype(np.float32))
    return _case(f"{gen}_{H}x{W}_c{C}", gen, H, W, C, np.stack(labels), np.stack(outputs), np.stack(origin))


def _hand_rand(name, H, W, C, labels, seed):
    labels = np.asarray(labels, np.float32)
    outputs, origin = [], []
    for b in range(labels.shape[0]):
        rng = np.random.default_rng((seed, b, H, W, C))
        outputs.append(gen_image("rand", rng, H, W, C, np.zeros((0, 4))))
        origin.append(rng.normal(0, 1, (outputs[-1].shape[0], 4)).astype(np.float32))
    return _case(name, None, H, W, C, labels, np.stack(outputs), np.stack(origin))


def exact_hit_case():
    """64x64, one class: three ground truths, each centred on an anchor centre (one per level)
    with w = h = the level's stride, and raw reg outputs (0.5, 0.5, 0, 0) at those anchors, so the
    decoded box equals the ground truth exactly (IoU 1.0, every max / min pair of the IoU ties).
    ``raw`` is the pre-decode head output; ``outputs`` holds the decoded boxes ((raw + grid) * s
    exactly, the drawn w, h where raw holds their logarithm) and ``origin`` is raw's reg part."""
    H = W = 64
    C = 1
    xs, ys, st = anchors(H, W)
    A = xs.shape[0]
    rng = np.random.default_rng((7, H, W, C))
    dxy = rng.normal(0, 4, (A, 2)).astype(np.float32) / st[:, None]
    wh = rng.uniform(8, 160, (A, 2)).astype(np.float32)
    raw = np.zeros((1, A, 5 + C), np.float32)
    raw[0, :, :2] = np.float32(0.5) + dxy
    raw[0, :, 2:4] = np.log(wh / st[:, None])
    raw[0, :, 4] = rng.normal(0, 1.5, A)
    raw[0, :, 5:] = rng.normal(-2, 1.5, (A, C))
    hit = (2 * 8 + 5, 64 + 1 * 4 + 2, 64 + 16 + 1 * 2 + 1)  # (x, y) = (5, 2) / (2, 1) / (1, 1)
    labels = np.zeros((1, 4, 5), np.float32)
    for i, a in enumerate(hit):
        raw[0, a, :4] = (0.5, 0.5, 0.0, 0.0)
        wh[a] = st[a]
        labels[0, i] = (0, (xs[a] + 0.5) * st[a], (ys[a] + 0.5) * st[a], st[a], st[a])
    out = raw.copy()
    out[0, :, 0] = (raw[0, :, 0] + xs) * st
    out[0, :, 1] = (raw[0, :, 1] + ys) * st
    out[0, :, 2:4] = wh
    case = _case("exact_hit", None, H, W, C, labels, out, raw[..., :4].copy(), raw)
    case["hit"] = hit
    return case


def hand_case(name):
    if name == "dup_off_corner":
        lab = np.zeros((3, 8, 5), np.float32)
        lab[0, :5] = [[1, 60, 40, 40, 30]] * 3 + [[2, 300, 40, 30, 30], [0, -3, -3, 30, 30]]
        lab[2, :2] = [[0, 30, 50, 10, 9], [2, 120, 30, 9, 12]]
        return _hand_rand(name, 96, 160, 3, lab, 11)
    if name == "few_candidates":
        return _hand_rand(name, 96, 160, 3, [[[0, -3, -3, 30, 30]]], 12)
    if name == "all_empty":
        return _hand_rand(name, 96, 160, 3, np.zeros((2, 8, 5)), 13)
    if name == "exact_hit":
        return exact_hit_case()
    raise KeyError(name)


_cache = {}


def case_names():
    return [f"{g}_{s[0]}x{s[1]}_c{s[2]}" for g in GENERATORS for s in SHAPES] + list(HAND)


def get_case(name):
    """The named batch (cached; treat the arrays as read-only)."""
    if name not in _cache:
        if name in HAND:
            _cache[name] = hand_case(name)
        else:
            gen = name.split("_")[0]
            shape = next(s for s in SHAPES if name == f"{gen}_{s[0]}x{s[1]}_c{s[2]}")
            _cache[name] = generated_case(gen, shape)
        for v in _cache[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _cache[name]


def num_gt(labels_b):
    return int((labels_b.sum(1) > 0).sum())


def loss_bwd_reference(oracle, raw, labels, xs, ys, st, assign, use_l1, gtot):
    """Autograd reference of yxh_yolox_loss_bwd: d (gtot * total_loss) / d raw head outputs
    through the oracle's loss math (decode, IoU loss, BCE, L1), with the device's assignment
    ``assign`` as fixed targets.  raw [B, A, 5+C] and labels [B, L, 5] are CPU tensors, xs / ys /
    st the anchors [A].  Returns (gradient [B, A, 5+C], total_loss as a float)."""
    import torch
    import torch.nn.functional as F
    B, nc = raw.shape[0], raw.shape[2] - 5
    r = raw.clone().requires_grad_()
    dec = torch.cat([(r[..., :2] + torch.stack([xs, ys], 1)) * st[:, None], torch.exp(r[..., 2:4]) * st[:, None],
                     r[..., 4:]], -1)
    fg = assign["fg_mask"].cpu().bool()
    matched = assign["matched_gt_inds"].cpu().long()
    piou = assign["pred_ious"].cpu()
    num_fg = max(int(fg.sum()), 1)
    tot = 0.0
    for b in range(B):
        f = fg[b]
        gtb = labels[b][matched[b][f]]
        tot = tot + 5.0 * oracle.iou_loss(dec[b, f, :4], gtb[:, 1:5]).sum()
        tot = tot + F.binary_cross_entropy_with_logits(r[b, :, 4], f.float(), reduction="sum")
        tgt = F.one_hot(gtb[:, 0].long(), nc).float() * piou[b][f][:, None]
        tot = tot + F.binary_cross_entropy_with_logits(r[b, f, 5:], tgt, reduction="sum")
        if use_l1:
            s_ = st[f]
            l1t = torch.stack([gtb[:, 1] / s_ - xs[f], gtb[:, 2] / s_ - ys[f], torch.log(gtb[:, 3] / s_ + 1e-8),
                               torch.log(gtb[:, 4] / s_ + 1e-8)], 1)
            tot = tot + (r[b, f, :4] - l1t).abs().sum()
    (gtot * tot / num_fg).backward()
    return r.grad, float(tot.detach()) / num_fg
