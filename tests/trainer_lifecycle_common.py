"""Shared by tests/test_gpu_trainer_lifecycle.py and its two-rank worker: the tiny training setup
(yolox_s at 128 x 128, batch 2 per rank, two iterations per epoch, two epochs, one of them
no-aug, evaluation every epoch) and the three-image evaluation dataset."""
import types

import numpy as np

from yolox_amd.config import YoloxConfig

VAL_IDS = [10, 11, 12]


class ValSet:
    """pull_item dataset (coco.py:131-160's contract): ragged uint8 images, COCO ground truth
    without annotations (the tests compare detections, not AP)."""
    class_ids = list(range(1, 81))

    def __init__(self, n=3):
        rng = np.random.default_rng(0)
        self.imgs = [rng.integers(0, 256, (int(rng.integers(300, 700)), int(rng.integers(300, 700)), 3),
                                  dtype=np.uint8) for _ in range(n)]
        self.coco = {"images": [{"id": VAL_IDS[0] + i, "height": a.shape[0], "width": a.shape[1]}
                                for i, a in enumerate(self.imgs)],
                     "annotations": [], "categories": [{"id": c, "name": f"c{c}"} for c in self.class_ids]}

    def __len__(self):
        return len(self.imgs)

    def pull_item(self, i):
        a = self.imgs[i]
        return a, np.zeros((0, 5), np.float32), (a.shape[0], a.shape[1]), VAL_IDS[0] + i


class LifecycleConfig(YoloxConfig):
    """yolox_s with an evaluation dataset (``val``; None: no evaluation)."""
    val = None

    def get_eval_dataset(self, **kwargs):
        return self.val


def make_config(output_dir, val=True, **over) -> LifecycleConfig:
    """A fresh config per trainer: get_model / get_optimizer cache on the config."""
    cfg = LifecycleConfig("yolox_s", depth=0.33, width=0.50, input_size=(128, 128), test_size=(128, 128),
                          max_epoch=2, warmup_epochs=1, no_aug_epochs=1, eval_interval=1, deterministic=True,
                          seed=3, output_dir=str(output_dir), print_interval=1,
                          # a model a few steps from its initialisation scores about 1e-4 (the prior
                          # biases): keep its detections so that the evaluations have boxes to compare
                          test_conf=1e-6)
    for k, v in over.items():
        setattr(cfg, k, v)
    cfg.val = ValSet() if val else None
    return cfg


def make_args(**over):
    a = dict(batch_size=2, fp16=False, max_iter=None, dataset_size=4, name=None, resume=False, ckpt=None,
             start_epoch=None)
    a.update(over)
    return types.SimpleNamespace(**a)


def spy_on_eval(cfg) -> list:
    """Record every ``cfg.eval`` call's (model, result)."""
    calls, inner = [], cfg.eval

    def spy(model, evaluator, is_distributed, half=False, return_outputs=False):
        r = inner(model, evaluator, is_distributed, half, return_outputs=return_outputs)
        calls.append((model, r))
        return r

    cfg.eval = spy
    return calls
