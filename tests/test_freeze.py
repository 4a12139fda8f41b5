"""freeze_module, the freeze config field and the --freeze flag (CPU)."""
import types

import pytest
import torch


def _model():
    from yolox_amd.config import named_config
    return named_config("yolox_s").get_model()


@pytest.mark.parametrize("name", [None, "backbone", "backbone.backbone", "head.stems"])
def test_freeze_module_follows_the_reference_rule(name):
    """yolox/utils/model_utils.py:129-154: requires_grad off where `name` is a substring of the parameter's name,
    .eval() on the sub-modules whose name contains it (and so on everything below them); all of them for None."""
    from yolox_amd.utils import freeze_module
    m = _model()
    assert all(p.requires_grad for p in m.parameters()) and all(s.training for s in m.modules())
    want_frozen = {n for n, _ in m.named_parameters() if name is None or name in n}
    # a child's name extends its parent's, so the matching set is closed under .eval()'s recursion
    want_eval = {n for n, _ in m.named_modules() if name is None or name in n}
    assert want_frozen and want_eval
    out = freeze_module(m, name)
    assert out is m
    assert {n for n, p in m.named_parameters() if not p.requires_grad} == want_frozen
    assert {n for n, s in m.named_modules() if not s.training} == want_eval
    if name == "backbone":
        assert all(n.startswith("backbone.") for n in want_frozen) and m.training and m.head.training
        assert not m.backbone.training and not m.backbone.backbone.dark3[0].bn.training
    if name == "head.stems":
        assert want_frozen == {n for n, _ in m.named_parameters() if n.startswith("head.stems.")}
    if name is None:
        assert not m.training


def test_freeze_module_on_a_submodule_and_exports():
    import yolox_amd.utils as U
    from yolox_amd.utils.model_utils import freeze_module
    assert U.freeze_module is freeze_module
    m = _model()
    assert freeze_module(m.backbone) is m.backbone
    assert all(not p.requires_grad for p in m.backbone.parameters()) and all(p.requires_grad for p in m.head.parameters())
    assert not any(s.training for s in m.backbone.modules()) and all(s.training for s in m.head.modules())
    m.train()  # undoes the eval half, as in torch
    assert m.backbone.training and not next(m.backbone.parameters()).requires_grad


def test_cli_and_config_take_freeze():
    from yolox_amd.cli import make_parser
    from yolox_amd.config import named_config
    args = make_parser().parse_args(["-c", "yolox_s", "--freeze", "backbone", "head.stems", "-b", "4"])
    assert args.freeze == ["backbone", "head.stems"] and args.batch_size == 4
    assert make_parser().parse_args(["-c", "yolox_s"]).freeze is None
    c = named_config("yolox_s")
    assert c.freeze == ()
    c.update({"freeze": "backbone.backbone"})
    assert c.freeze == ("backbone.backbone",)
    c.update({"freeze": "backbone, head.stems"})
    assert c.freeze == ("backbone", "head.stems")
    c.update({"freeze": ["head.stems"]})
    assert c.freeze == ("head.stems",)
    c.update({"freeze": tuple(args.freeze)})
    assert c.freeze == ("backbone", "head.stems")
    c.update({"freeze": ""})
    assert c.freeze == ()


def test_trainer_refuses_a_name_that_matches_nothing():
    from yolox_amd.config import named_config
    from yolox_amd.trainer import Trainer
    c = named_config("yolox_s")
    t = Trainer(c, types.SimpleNamespace(fp16=False, name=None))
    m = c.get_model()
    c.update({"freeze": "neck"})
    with pytest.raises(ValueError, match="neck"):
        t.apply_freeze(m)
    assert all(p.requires_grad for p in m.parameters())
    c.update({"freeze": "head.stems,backbone.backbone.dark5"})
    t.apply_freeze(m)
    frozen = {n for n, p in m.named_parameters() if not p.requires_grad}
    assert frozen and all(n.startswith(("head.stems.", "backbone.backbone.dark5.")) for n in frozen)
    assert not m.head.stems[0].bn.training and m.head.cls_convs[0][0].bn.training


def test_grad_buffer_holds_trainable_parameters_only():
    from yolox_amd.train import GradBuffer
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2)), torch.nn.Parameter(torch.zeros(5))]
    ps[1].requires_grad = False
    gb = GradBuffer(ps, "cpu")
    assert gb.params == [ps[2], ps[0]] and gb.numel == 8
    assert gb.holds(ps[0]) and not gb.holds(ps[1]) and not gb.holds(None)
    gb.publish(gb.begin())
    assert ps[1].grad is None and ps[0].grad is not None and ps[2].grad.shape == (5,)
    assert GradBuffer(ps, "cpu").serial > gb.serial
