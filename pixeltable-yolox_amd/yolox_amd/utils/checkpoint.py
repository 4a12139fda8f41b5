"""Checkpoint files (reference yolox/utils/checkpoint.py): ``load_ckpt`` for fine-tuning from a
checkpoint whose head may have another class count, ``save_checkpoint`` for the trainer's
``<name>_ckpt.pth`` / ``best_ckpt.pth`` files.

Differences from the reference: skipped keys are printed (no logger here), and a file is written
under a temporary name in its directory and renamed into place, so a killed run never leaves a
truncated ``latest_ckpt.pth`` behind.
"""
from __future__ import annotations

import os
import shutil

import torch


def load_ckpt(model, ckpt):
    """checkpoint.py:9-31: load the entries of ``ckpt`` (a state dict) that ``model`` has with an
    equal shape; every other key of the model keeps its value and is reported."""
    load_dict = {}
    for key, v in model.state_dict().items():
        if key not in ckpt:
            print(f"load_ckpt: {key} is not in the checkpoint, kept as initialised", flush=True)
            continue
        v_ckpt = ckpt[key]
        if tuple(v.shape) != tuple(v_ckpt.shape):
            print(f"load_ckpt: shape of {key} is {tuple(v_ckpt.shape)} in the checkpoint vs {tuple(v.shape)} in "
                  "the model, kept as initialised", flush=True)
            continue
        load_dict[key] = v_ckpt
    model.load_state_dict(load_dict, strict=False)
    return model


def _write_atomically(write, filename: str) -> None:
    tmp = f"{filename}.{os.getpid()}.tmp"
    try:
        write(tmp)
        os.replace(tmp, filename)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def save_checkpoint(state, is_best: bool, save_dir: str, model_name: str = "") -> str:
    """checkpoint.py:34-41: ``<save_dir>/<model_name>_ckpt.pth`` (and its copy ``best_ckpt.pth``
    when ``is_best``).  Returns the file's path."""
    os.makedirs(save_dir, exist_ok=True)
    filename = os.path.join(save_dir, model_name + "_ckpt.pth")

    def write(tmp):
        # through a file object: torch.save(path) names the archive's records after the file, so
        # equal states saved under two names (last_epoch / epoch_<n>) would differ in their bytes
        with open(tmp, "wb") as f:
            torch.save(state, f)

    _write_atomically(write, filename)
    if is_best:
        _write_atomically(lambda tmp: shutil.copyfile(filename, tmp), os.path.join(save_dir, "best_ckpt.pth"))
    return filename
