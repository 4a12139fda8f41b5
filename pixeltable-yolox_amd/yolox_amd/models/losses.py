"""YOLOX training losses with on-device SimOTA (yxh_yolox_loss_ex) and the standalone
IouLoss module (yxh_iou_loss).

yolox_losses replaces YoloxHead.get_losses (reference yolo_head.py:253-411): the reference
loops over images and ground truths in Python with host syncs; here one call assigns and
reduces the whole batch on the device.  IouLoss is the reference's module of that name
(losses.py:7-51) over the same per-pair device math the batch kernels use.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _native as N

LOSS_KEYS = ("total_loss", "iou_loss", "conf_loss", "cls_loss", "l1_loss", "num_fg")


def _aligned(t: torch.Tensor) -> torch.Tensor:
    """t contiguous with 16-byte aligned storage (each [4] row is one 16-byte load)."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


class _IouLossFn(torch.autograd.Function):
    """pred, target: fp32 [N, 4] on the device, N > 0."""

    @staticmethod
    def forward(ctx, pred, target, loss_type: int, reduction: int):
        pred, target = _aligned(pred.detach()), _aligned(target.detach())
        n, dev = pred.shape[0], pred.device
        lib = N.lib()
        out = torch.empty((n,) if reduction == N.REDUCE_NONE else (), dtype=torch.float32, device=dev)
        ws = None
        if reduction != N.REDUCE_NONE:
            ws = torch.empty(int(lib.yxh_iou_loss_workspace_bytes(n)) // 8, dtype=torch.float64, device=dev)
        N.check(lib.yxh_iou_loss(pred.data_ptr(), target.data_ptr(), n, loss_type, reduction, out.data_ptr(),
                                 ws.data_ptr() if ws is not None else None, ws.numel() * 8 if ws is not None else 0,
                                 N.stream_ptr(dev)), "iou_loss")
        ctx.save_for_backward(pred, target)
        ctx.loss_type, ctx.reduction = loss_type, reduction
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        pred, target = ctx.saved_tensors
        n, dev = pred.shape[0], pred.device
        grad = _aligned(grad.to(torch.float32))
        g_pred = torch.empty_like(pred)
        g_target = torch.empty_like(target) if ctx.needs_input_grad[1] else None
        N.check(N.lib().yxh_iou_loss_bwd(pred.data_ptr(), target.data_ptr(), n, ctx.loss_type, ctx.reduction,
                                         grad.data_ptr(), g_pred.data_ptr(),
                                         g_target.data_ptr() if g_target is not None else None, N.stream_ptr(dev)),
                "iou_loss_bwd")
        return (g_pred if ctx.needs_input_grad[0] else None), g_target, None, None


class IouLoss(nn.Module):
    """The reference's IouLoss (losses.py:7-51) on the device: ``pred`` and ``target`` are
    (cx, cy, w, h) boxes, ``loss_type`` "iou" (1 - iou^2) or "giou", ``reduction`` "none",
    "sum" or "mean".  Gradients flow to ``pred`` and, when it requires them, to ``target``;
    there is no double backward.  fp32 runs natively; fp16 / bf16 inputs are computed in fp32
    and the loss returned in the inputs' type."""

    def __init__(self, reduction="none", loss_type="iou"):
        super().__init__()
        if reduction not in N.REDUCTION_CODE:
            raise ValueError(f"IouLoss: unknown reduction {reduction!r} (none, sum or mean)")
        if loss_type not in N.IOU_LOSS_CODE:
            raise ValueError(f"IouLoss: unknown loss_type {loss_type!r} (iou or giou)")
        self.reduction = reduction
        self.loss_type = loss_type

    def extra_repr(self) -> str:
        return f"reduction={self.reduction!r}, loss_type={self.loss_type!r}"

    def forward(self, pred, target):
        assert pred.shape[0] == target.shape[0]
        for name, t in (("pred", pred), ("target", target)):
            if t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
                raise ValueError(f"IouLoss: {name} must be float32, float16 or bfloat16 (got {t.dtype})")
        if not (pred.is_cuda and target.is_cuda):
            raise RuntimeError("IouLoss runs on a ROCm device only; call .to('cuda') first")
        # attributes may have been reassigned since construction
        if self.reduction not in N.REDUCTION_CODE or self.loss_type not in N.IOU_LOSS_CODE:
            raise ValueError(f"IouLoss: reduction {self.reduction!r}, loss_type {self.loss_type!r}")
        out_dtype = torch.promote_types(pred.dtype, target.dtype)
        pred = pred.view(-1, 4).float()
        target = target.view(-1, 4).float()
        if pred.shape[0] != target.shape[0]:
            raise ValueError(f"IouLoss: {pred.shape[0]} pred boxes against {target.shape[0]} target boxes")
        if pred.shape[0] == 0:
            # as torch: an empty tensor, 0, or nan (the mean of nothing), still attached to the graph
            loss = pred.sum(1) + target.sum(1)
            loss = loss if self.reduction == "none" else (loss.sum() if self.reduction == "sum" else loss.mean())
        else:
            loss = _IouLossFn.apply(pred, target, N.IOU_LOSS_CODE[self.loss_type], N.REDUCTION_CODE[self.reduction])
        return loss.to(out_dtype)


def yolox_losses(outputs: torch.Tensor, labels: torch.Tensor, level_hw: Sequence[tuple[int, int]],
                 strides: Sequence[int] = (8, 16, 32), origin_reg: Optional[torch.Tensor] = None,
                 iou_loss_type: str = "iou"):
    """outputs [B, A, 5+C] (train-mode decoded boxes, raw obj/cls logits), labels
    [B, L, 5].  iou_loss_type: the box loss of the foreground anchors, "iou" or "giou"
    (head.iou_loss.loss_type); the assignment uses the plain IoU either way.
    Returns (losses dict of 0-d tensors, assignment dict)."""
    if iou_loss_type not in N.IOU_LOSS_CODE:
        raise ValueError(f"unknown iou_loss_type {iou_loss_type!r} (iou or giou)")
    N.require_device(outputs, "outputs")
    if outputs.dtype != torch.float32:
        raise ValueError("outputs must be float32")
    B, A, D = outputs.shape
    C = D - 5
    L = labels.shape[1]
    dev = outputs.device
    outputs = outputs.contiguous()
    labels = labels.to(dev, torch.float32).contiguous()
    if origin_reg is not None:
        origin_reg = origin_reg.to(dev, torch.float32).contiguous()
    # level geometry is read on the host by the launcher (host arrays, not device memory)
    hw = torch.tensor([v for h, w in level_hw for v in (h, w)], dtype=torch.int32)
    st = torch.tensor(list(strides), dtype=torch.int32)
    fg = torch.empty(B, A, dtype=torch.uint8, device=dev)
    matched = torch.empty(B, A, dtype=torch.int32, device=dev)
    piou = torch.empty(B, A, dtype=torch.float32, device=dev)
    num_fg = torch.empty(B, dtype=torch.int32, device=dev)
    losses = torch.empty(6, dtype=torch.float32, device=dev)
    lib = N.lib()
    ws = torch.empty(int(lib.yxh_yolox_loss_workspace_bytes(B, A, L)), dtype=torch.uint8, device=dev)
    N.check(lib.yxh_yolox_loss_ex(
        outputs.data_ptr(), origin_reg.data_ptr() if origin_reg is not None else None, labels.data_ptr(), B, A, C,
        L, hw.data_ptr(), st.data_ptr(), len(strides), fg.data_ptr(), matched.data_ptr(), piou.data_ptr(),
        num_fg.data_ptr(), losses.data_ptr(), ws.data_ptr(), ws.numel(), N.stream_ptr(dev),
        N.IOU_LOSS_CODE[iou_loss_type]), "yolox_loss")
    out = {k: losses[i] for i, k in enumerate(LOSS_KEYS)}
    assign = {"fg_mask": fg.bool(), "matched_gt_inds": matched, "pred_ious": piou, "num_fg": num_fg}
    return out, assign
