"""IouLoss on the host side: the module's interface (reference losses.py:7-51, yolo_head.py:125),
the ABI-21 entry points and the fixture's contents.  The device checks are
tests/test_gpu_iou_loss.py and tests/test_gpu_train_giou.py."""
import os
import re

import pytest
import torch

import simota_cases as SC
from conftest import REPO

NEW_ENTRIES = ("yxh_iou_loss_workspace_bytes", "yxh_iou_loss", "yxh_iou_loss_bwd", "yxh_yolox_loss_ex",
               "yxh_yolox_loss_bwd_ex")


def test_import_and_attributes():
    from yolox_amd.models import IouLoss
    from yolox_amd.models.losses import IouLoss as same
    assert IouLoss is same
    m = IouLoss()
    assert isinstance(m, torch.nn.Module)
    assert (m.reduction, m.loss_type) == ("none", "iou")
    m = IouLoss(reduction="mean", loss_type="giou")
    assert (m.reduction, m.loss_type) == ("mean", "giou")
    m = IouLoss("sum", "giou")  # the reference's positional order
    assert (m.reduction, m.loss_type) == ("sum", "giou")
    assert not list(m.parameters()) and not list(m.buffers())


@pytest.mark.parametrize("kwargs", [{"loss_type": "diou"}, {"loss_type": "IOU"}, {"reduction": "avg"},
                                    {"reduction": None}])
def test_unknown_type_or_reduction_raises(kwargs):
    from yolox_amd.models import IouLoss
    with pytest.raises(ValueError):
        IouLoss(**kwargs)


def test_input_checks_need_no_device():
    from yolox_amd.models import IouLoss
    m = IouLoss()
    with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
        m(torch.zeros(3, 4), torch.zeros(3, 4))
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        m(torch.zeros(3, 4, dtype=torch.float64), torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(ValueError):
        m(torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, 4))
    with pytest.raises(AssertionError):  # the reference's assert
        m(torch.zeros(3, 4), torch.zeros(2, 4))


def test_head_carries_the_loss_module():
    from yolox_amd.models import IouLoss, YoloxHead
    head = YoloxHead(3, width=0.5)
    assert isinstance(head.iou_loss, IouLoss)
    assert head.iou_loss.reduction == "none" and head.iou_loss.loss_type == "iou"
    keys = list(head.state_dict().keys())
    assert not [k for k in keys if "iou_loss" in k]
    del head.iou_loss
    assert list(head.state_dict().keys()) == keys
    # the reference's way of switching the box loss
    head.iou_loss = IouLoss(reduction="none", loss_type="giou")
    assert list(head.state_dict().keys()) == keys


def test_yolox_losses_rejects_an_unknown_type_before_the_device():
    from yolox_amd.models.losses import yolox_losses
    with pytest.raises(ValueError, match="iou_loss_type"):
        yolox_losses(torch.zeros(1, 21, 8), torch.zeros(1, 2, 5), [(4, 4), (2, 2), (1, 1)], iou_loss_type="diou")
    import inspect
    assert inspect.signature(yolox_losses).parameters["iou_loss_type"].default == "iou"


def test_abi_21_and_new_entries():
    from yolox_amd import _native as N
    assert N.ABI_VERSION == 21
    header = open(os.path.join(REPO, "include", "yoloxhip.h")).read()
    assert re.search(r"#define\s+YXH_ABI_VERSION\s+21\b", header)
    assert re.search(r"YXH_IOU_LOSS_IOU\s*=\s*0\b", header) and re.search(r"YXH_IOU_LOSS_GIOU\s*=\s*1\b", header)
    assert (N.IOU_LOSS_IOU, N.IOU_LOSS_GIOU) == (0, 1)
    lib = N.lib()
    for name in NEW_ENTRIES:
        assert name in N.EXPORTED, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(lib, name), name


def test_argument_errors_without_a_device():
    """Unknown type / reduction -> YXH_EINVAL with a message, n == 0 -> YXH_OK: both return before
    the HIP runtime is touched."""
    from yolox_amd import _native as N
    lib = N.lib()
    assert lib.yxh_iou_loss(None, None, 0, 0, 0, None, None, 0, None) == N.OK
    assert lib.yxh_iou_loss_bwd(None, None, 0, 1, 2, None, None, None, None) == N.OK
    assert lib.yxh_iou_loss_workspace_bytes(0) == 0
    assert lib.yxh_iou_loss_workspace_bytes(1) == 8 and lib.yxh_iou_loss_workspace_bytes(257) == 16
    assert lib.yxh_iou_loss(None, None, 4, 2, 0, None, None, 0, None) == N.EINVAL
    assert b"loss_type 2" in lib.yxh_last_error()
    assert lib.yxh_iou_loss(None, None, 4, 1, 3, None, None, 0, None) == N.EINVAL
    assert b"reduction 3" in lib.yxh_last_error()
    assert lib.yxh_iou_loss_bwd(None, None, 4, -1, 0, None, None, None, None) == N.EINVAL
    assert b"loss_type -1" in lib.yxh_last_error()
    assert lib.yxh_iou_loss_bwd(None, None, 0, 0, 7, None, None, None, None) == N.EINVAL  # checked before n == 0
    assert lib.yxh_iou_loss(None, None, 4, 0, 0, None, None, 0, None) == N.EINVAL
    assert b"null" in lib.yxh_last_error()
    args = [None] * 3 + [1, 21, 3, 2] + [None] * 2 + [3] + [None] * 6 + [0, None]
    assert lib.yxh_yolox_loss_ex(*args, 2) == N.EINVAL
    assert b"iou_loss_type 2" in lib.yxh_last_error()
    bargs = [None] * 3 + [1, 21, 3, 2] + [None] * 2 + [3] + [None] * 5 + [0, 0, None, None, None]
    assert lib.yxh_yolox_loss_bwd_ex(*bargs, 5) == N.EINVAL
    assert b"iou_loss_type 5" in lib.yxh_last_error()


def test_fixture_holds_every_case(golden):
    d = golden("iou_loss.npz")
    for name in SC.case_names():
        for tag in ("nol1", "l1"):
            for dn in ("f32", "f64"):
                assert d[f"head.{name}.{tag}.{dn}.losses"].shape == (6,)
                c = SC.get_case(name)
                assert d[f"head.{name}.{tag}.{dn}.g_raw5"].shape == c["outputs"].shape[:2] + (5,)
    names = [str(n) for n in d["boxes.edge.names"]]
    assert len(names) == d["boxes.edge.pred"].shape[0]
    for n in names:  # every edge row in both argument orders
        if not n.endswith(".swapped"):
            i, j = names.index(n), names.index(n + ".swapped")
            assert (d["boxes.edge.pred"][i] == d["boxes.edge.target"][j]).all()
            assert (d["boxes.edge.target"][i] == d["boxes.edge.pred"][j]).all()
    assert d["boxes.rand.pred"].shape == (1000, 4)
    for tag in ("rand", "edge"):
        for lt in ("iou", "giou"):
            for dn in ("f32", "f64"):
                for q in ("loss", "g_pred", "g_target"):
                    assert f"boxes.{tag}.{lt}.{dn}.{q}" in d
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "iou_loss.npz")) < 1 << 20
