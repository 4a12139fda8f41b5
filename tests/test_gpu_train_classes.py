"""The HIP training step with a class count that is not a multiple of the kernels' 16-byte dy
chunks (a fine-tuned 3-class head: 4 fp32 / 8 fp16 elements per chunk).  The head's reverse pass
pads the class gradient rows with zeros for the weight / data gradient kernels; losses and every
parameter gradient are pinned to the oracle's autograd at the bound tests/test_gpu_train.py uses
for the other widths (1e-3 of each tensor's max, fp32), and an fp16 autocast step stays finite and
within 5 % of the fp32 loss."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


@pytest.mark.parametrize("num_classes", [3, 6])
def test_train_step_unaligned_class_count_matches_oracle(oracle, num_classes):
    from yolox_amd.config import named_config
    from yolox_amd.weights import synthetic_images, synthetic_labels, synthetic_state_dict
    cfg = named_config("yolox_s")
    cfg.num_classes = num_classes
    m = cfg.get_model()
    sd = synthetic_state_dict(m.state_dict(), seed=3, bn_stats="yolox_s")
    m.load_state_dict(sd)
    x = torch.from_numpy(synthetic_images(2, 64, 64, seed=5)).permute(0, 3, 1, 2).float()
    labels = torch.from_numpy(synthetic_labels(2, 64, 64, max_gt=6, num_classes=num_classes, seed=7))
    assert int(labels[..., 0].max()) < num_classes
    m = m.cuda().train()
    out = m(x.cuda(), labels.cuda())
    out["total_loss"].backward()
    torch.cuda.synchronize()
    sdo = {k: v.clone().float().requires_grad_(v.is_floating_point() and "running" not in k
                                               and "num_batches" not in k) for k, v in sd.items()}
    arch = dataclasses.replace(oracle.ARCHS["yolox_s"], num_classes=num_classes)
    ref = oracle.forward_train(sdo, arch, x, labels, use_l1=False)
    ref["total_loss"].backward()
    for k in ("total_loss", "iou_loss", "conf_loss", "cls_loss", "num_fg"):
        assert float(out[k].detach()) == pytest.approx(float(ref[k]), rel=1e-3, abs=1e-6), k
    for pname, prm in m.named_parameters():
        assert rel(prm.grad, sdo[pname].grad) < 1e-3, pname
    m.load_state_dict(sd)
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16):
        out16 = m(x.cuda().half(), labels.cuda())
    out16["total_loss"].backward()
    torch.cuda.synchronize()
    l16 = float(out16["total_loss"].detach())
    assert np.isfinite(l16) and abs(l16 - float(out["total_loss"].detach())) < 0.05 * float(out["total_loss"].detach())
    assert all(torch.isfinite(prm.grad).all() for prm in m.parameters())
