"""Plain-torch restatement of the YOLOX-Darknet53 forward, for tests.

Walks the package's module tree (parameters and topology only) with F.conv2d, F.batch_norm and
F.leaky_relu(0.1), following the reference's forwards (network_blocks.py:102-141, darknet.py:80-92,
yolo_fpn.py:57-82, yolo_head.py:140-251).  float32 on whatever device the tensors are on.

``store``: None, or a 16-bit dtype.  With it the restatement models what a 16-bit plan stores: every
BaseConv's weights with BatchNorm folded in float32 and rounded once to ``store`` (bias float32),
every activation map rounded to ``store`` after the activation (and residual add), the pred convs'
weights rounded, float32 accumulation and decode.
"""
import torch
import torch.nn.functional as F


def _q(t, store):
    return t if store is None else t.to(store).float()


def _act(y, name):
    if name == "lrelu":
        return F.leaky_relu(y, 0.1)
    if name == "silu":
        return F.silu(y)
    if name == "relu":
        return F.relu(y)
    raise ValueError(name)


def base_conv(m, x, store=None, residual=None):
    c, bn = m.conv, m.bn
    w = c.weight.detach().float()
    stats = [t.detach().float() for t in (bn.running_mean, bn.running_var, bn.weight, bn.bias)]
    if store is None:
        y = F.conv2d(x, w, None, c.stride, c.padding, 1, c.groups)
        y = F.batch_norm(y, stats[0], stats[1], stats[2], stats[3], False, 0.0, bn.eps)
    else:
        scale = stats[2] / torch.sqrt(stats[1] + bn.eps)
        y = F.conv2d(x, _q(w * scale[:, None, None, None], store), stats[3] - stats[0] * scale, c.stride,
                     c.padding, 1, c.groups)
    y = _act(y, m.act_name)
    if residual is not None:
        y = y + residual
    return _q(y, store)


def res_layer(m, x, store=None):
    return base_conv(m.layer2, base_conv(m.layer1, x, store), store, residual=x)


def spp(m, x, store=None):
    x = base_conv(m.conv1, x, store)
    x = torch.cat([x] + [F.max_pool2d(x, p.kernel_size, p.stride, p.padding) for p in m.m], 1)
    return base_conv(m.conv2, x, store)


def chain(blocks, x, store=None):
    for m in blocks:
        kind = type(m).__name__
        if kind == "BaseConv":
            x = base_conv(m, x, store)
        elif kind == "ResLayer":
            x = res_layer(m, x, store)
        elif kind == "SPPBottleneck":
            x = spp(m, x, store)
        else:
            raise TypeError(kind)
    return x


def darknet(m, x, store=None) -> dict:
    """All five feature maps, in the reference's order."""
    outs = {}
    x = _q(x.float(), store)
    for name in ("stem", "dark2", "dark3", "dark4", "dark5"):
        x = outs[name] = chain(getattr(m, name), x, store)
    return outs


def yolo_fpn(m, x, store=None):
    f = darknet(m.backbone, x, store)
    x2, x1, x0 = [f[k] for k in m.in_features]
    up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")  # noqa: E731
    x1_in = up(base_conv(m.out1_cbl, x0, store))
    out_dark4 = chain(m.out1, torch.cat([x1_in, x1], 1), store)
    x2_in = up(base_conv(m.out2_cbl, out_dark4, store))
    out_dark3 = chain(m.out2, torch.cat([x2_in, x2], 1), store)
    return out_dark3, out_dark4, x0


def head(m, feats, store=None):
    rows = []
    for k, (x, stride) in enumerate(zip(feats, m.strides)):
        x = base_conv(m.stems[k], x, store)
        c = chain(m.cls_convs[k], x, store)
        r = chain(m.reg_convs[k], x, store)
        pred = lambda p, t: F.conv2d(t, _q(p.weight.detach().float(), store), p.bias.detach().float())  # noqa: E731
        out = torch.cat([pred(m.reg_preds[k], r), pred(m.obj_preds[k], r).sigmoid(),
                         pred(m.cls_preds[k], c).sigmoid()], 1)
        h, w = out.shape[2:]
        yv, xv = torch.meshgrid(torch.arange(h, device=out.device), torch.arange(w, device=out.device), indexing="ij")
        grid = torch.stack((xv, yv), 2).view(1, -1, 2).float()
        o = out.flatten(2).permute(0, 2, 1)
        rows.append(torch.cat([(o[..., :2] + grid) * stride, torch.exp(o[..., 2:4]) * stride, o[..., 4:]], -1))
    return torch.cat(rows, 1)


def yolox(m, x, store=None):
    """-> (decoded [B, A, 5 + C] rows, the three FPN maps)."""
    with torch.no_grad():
        feats = yolo_fpn(m.backbone, x, store)
        return head(m.head, feats, store), feats


def metrics(a, b) -> dict:
    """Probability / box distances between two decoded outputs (the measures of
    tests/test_gpu_model.py's low-precision checks)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    dp = (a[..., 4:] - b[..., 4:]).abs().flatten()
    db = ((a[..., :4] - b[..., :4]).abs() / b[..., :4].abs().clamp_min(1.0)).flatten()
    return {"p_max": dp.max().item(), "p_p99": dp.quantile(0.99).item(), "xy_max": (a[..., :2] - b[..., :2]).abs().max().item(),
            "box_p99": db.quantile(0.99).item()}
