"""One rank of tests/test_gpu_trainer_lifecycle.py::test_two_ranks: Trainer.train() under
yolox_amd.dp.DistributedDataParallel (gloo, both ranks on GPU 0), an output directory per rank.
Writes result.json (files written, the image ids each evaluation returned, mode flags) and bn.pt
(the BN buffers before the last epoch-end average and after it)."""
import argparse
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "pixeltable-yolox_amd"))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int)
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--port", type=int)
    ap.add_argument("--out")
    a = ap.parse_args()
    os.environ["YOLOX_AMD_TRAIN_TUNE"] = "0"
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port), RANK=str(a.rank), WORLD_SIZE=str(a.world))
    import torch
    import torch.distributed as dist
    from trainer_lifecycle_common import make_args, make_config, spy_on_eval

    import yolox_amd.dp as dp
    from yolox_amd.trainer import Trainer
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=a.rank, world_size=a.world)
    os.makedirs(a.out, exist_ok=True)
    cfg = make_config(os.path.join(a.out, "ckpt"))
    evals = spy_on_eval(cfg)
    random.seed(cfg.seed)
    torch.manual_seed(cfg.seed)
    trainer = Trainer(cfg, make_args(batch_size=2 * a.world, dataset_size=4 * a.world))

    def bn_buffers():
        return {k: v.detach().cpu().clone() for k, v in trainer.model.module.named_buffers()}

    before = {}
    inner = dp.all_reduce_norm

    def recording(module, *args, **kwargs):
        before.update(bn_buffers())  # the last call's: the end of epoch 2
        return inner(module, *args, **kwargs)

    dp.all_reduce_norm = recording
    trainer.train()
    torch.cuda.synchronize()
    assert trainer.is_distributed and trainer.max_iter == 2
    ckpt_dir = os.path.join(a.out, "ckpt", "yolox_s")
    res = {"rank": a.rank, "files": sorted(os.listdir(ckpt_dir)) if os.path.isdir(ckpt_dir) else [],
           "image_ids": [sorted(r[1]) for _, r in evals], "scored": [r[0][2] is not None for _, r in evals],
           "training_flags": all(m.training for m in trainer.model.modules())
           and not any(m.training for m in trainer.ema_model.ema.modules())}
    torch.save({"before": before, "after": bn_buffers()}, os.path.join(a.out, "bn.pt"))
    with open(os.path.join(a.out, "result.json"), "w") as f:
        json.dump(res, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
