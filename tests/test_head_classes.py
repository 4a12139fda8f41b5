"""YoloxModule.synthetic(num_classes=): a preset with a fine-tuned model's class count (host only)."""
import pytest
import torch


def _synthetic(**kw):
    from yolox_amd.models import YoloxModule
    try:
        return YoloxModule.synthetic("yolox_s", seed=3, device="cpu", **kw)
    except (RuntimeError, NotImplementedError) as e:  # a build whose synthetic() cannot target the host
        pytest.skip(f"YoloxModule.synthetic cannot build on the host: {e}")


def test_synthetic_num_classes():
    m3, m80 = _synthetic(num_classes=3), _synthetic()
    assert m3.head.num_classes == 3
    assert [p.out_channels for p in m3.head.cls_preds] == [3, 3, 3]
    sd3, sd80 = m3.state_dict(), m80.state_dict()
    assert sd3.keys() == sd80.keys()
    for k, v in sd80.items():  # only cls_preds change shape; everything else (BN statistics too) is the preset's
        if "cls_preds" in k:
            assert sd3[k].shape[0] == 3 and sd3[k].shape[1:] == v.shape[1:], k
        else:
            assert torch.equal(sd3[k], v), k


def test_synthetic_default_keeps_the_preset():
    """No num_classes: the tensors of the state dict synthetic() has always built for this seed."""
    from yolox_amd.config import named_config
    from yolox_amd.weights import synthetic_state_dict
    m = _synthetic()
    assert m.head.num_classes == 80
    cfg = named_config("yolox_s")
    want = synthetic_state_dict(cfg.get_model().state_dict(), seed=3, bn_stats=cfg.name)
    got = m.state_dict()
    assert got.keys() == want.keys()
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    with pytest.raises(ValueError):
        _synthetic(num_classes=0)
