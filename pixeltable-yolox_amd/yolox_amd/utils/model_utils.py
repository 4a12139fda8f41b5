"""Module utilities of the reference's ``yolox.utils.model_utils`` that the HIP path honours."""
from __future__ import annotations

from typing import Optional

import torch.nn as nn

__all__ = ["freeze_module", "frozen_names"]


def frozen_names(module: nn.Module, name: Optional[str] = None) -> tuple:
    """(parameter names, sub-module names) that ``freeze_module(module, name)`` touches: those whose
    name contains ``name`` as a substring (no pattern matching), all of them when ``name`` is None."""
    def hit(n: str) -> bool:
        return name is None or name in n

    return ([n for n, _ in module.named_parameters() if hit(n)], [n for n, _ in module.named_modules() if hit(n)])


def freeze_module(module: nn.Module, name: Optional[str] = None) -> nn.Module:
    """model_utils.py:129-154, in place: ``requires_grad = False`` on the parameters whose name contains
    ``name`` and ``.eval()`` on the sub-modules whose name does (so their BatchNorms keep their running
    statistics); everything when ``name`` is None.  Returns ``module``.

        freeze_module(model.backbone)          # CspDarknet + PAFPN
        freeze_module(model, "head.stems")

    The HIP train step (yolox_amd.train) reads both flags: no gradient launches and no BatchNorm statistics
    for what is frozen, ``.grad`` stays None, and FusedStep neither decays nor moves such a parameter.
    ``module.train()`` puts the sub-modules back into train mode; call freeze_module again afterwards."""
    params, mods = frozen_names(module, name)
    table = dict(module.named_parameters())
    for n in params:
        table[n].requires_grad = False
    subs = dict(module.named_modules())
    for n in mods:
        subs[n].eval()
    return module
