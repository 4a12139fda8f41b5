"""``yolox train`` (reference yolox/cli/train.py:19-143 + cli/utils.py) on the HIP path.

    python -m yolox_amd train -c yolox-s -d 8 -b 64 --fp16 [-o] [--resume] [--ckpt FILE] [-e N]
                              [--freeze NAME ...] [-D key=value ...]

Same flags and meaning as the reference: ``-c`` a named config (or ``module:Class``),
``-d`` processes = GPUs of this machine (one process per GPU, yolox_amd.launch), ``-b`` the
GLOBAL batch (each rank trains on b / d images), ``--fp16`` mixed precision through
autocast + GradScaler, ``-D`` config overrides, ``--resume`` continue from ``--ckpt`` or
``<output_dir>/<name>/latest_ckpt.pth`` (``-e`` overrides the epoch to start at, 1-based),
``--ckpt`` alone fine-tune from a checkpoint's matching weights.  ``--freeze NAME [NAME ...]`` (added; also
``-D freeze=NAME,NAME``) freezes, after the weights are loaded, every parameter and sub-module whose name
contains NAME (``yolox_amd.utils.freeze_module``: ``requires_grad`` off, BatchNorm in eval mode), e.g.
``backbone`` (CspDarknet + PAFPN), ``backbone.backbone`` (CspDarknet) or ``head.stems``; the HIP step then
skips their backward and BatchNorm statistics, the optimizer leaves them alone, and a NAME that matches
nothing is an error.  Every epoch end writes
checkpoints there and, with an evaluation dataset (``YoloxConfig.get_eval_dataset``),
evaluates (yolox_amd.trainer).  ``-D data_dir=/path/to/COCO`` trains on a COCO-layout directory
(``annotations/<train_ann>``, ``train2017/``; yolox_amd.data.CocoDataset streamed through an HBM
pool of ``YOLOX_AMD_DATA_CACHE_GB`` gigabytes, 64 by default) and evaluates on its ``val2017``;
without ``data_dir`` the training data is synthetic and nothing is evaluated.  Added:
``--max-iter`` (stop after that many iterations) and ``--dataset-size`` (length of the synthetic
COCO-shaped dataset).  Loggers and ``--cache`` are out of scope (the HBM pool is the cache).
"""
from __future__ import annotations

import argparse
import importlib
import random
import sys
from typing import Optional

import torch

from .config import YoloxConfig
from .launch import launch


def resolve_config(config_str: str) -> YoloxConfig:
    """cli/utils.py:7-29."""
    config = YoloxConfig.get_named_config(config_str)
    if config is not None:
        return config
    config_class: Optional[type] = None
    classpath = config_str.split(":")
    if len(classpath) == 2:
        try:
            config_class = getattr(importlib.import_module(classpath[0]), classpath[1], None)
        except ImportError:
            pass
    if config_class is None:
        raise ValueError(f"Unknown config class: {config_str}")
    if not issubclass(config_class, YoloxConfig):
        raise ValueError(f"Invalid config class (does not extend `YoloxConfig`): {config_str}")
    return config_class()


def parse_model_config_opts(kv_opts) -> dict:
    """cli/utils.py:32-42."""
    kv = {}
    for item in kv_opts or []:
        if "=" not in item:
            raise ValueError(f"Invalid model configuration option (must be of the form OPT=VALUE): {item}")
        k, v = item.split("=", 1)
        kv[k] = v
    return kv


def make_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser("yolox train")
    p.add_argument("-c", "--config", type=str, help="a builtin config such as yolox_s, or module:Class")
    p.add_argument("-n", "--name", type=str, default=None)
    p.add_argument("--dist-backend", default="nccl", type=str, help="distributed backend (nccl = RCCL)")
    p.add_argument("--dist-url", default=None, type=str)
    p.add_argument("-b", "--batch-size", type=int, default=64, help="global batch size")
    p.add_argument("-d", "--devices", default=None, type=int, help="GPUs (processes) for training")
    p.add_argument("--resume", default=False, action="store_true")
    p.add_argument("--ckpt", default=None, type=str)
    p.add_argument("-e", "--start_epoch", default=None, type=int)
    p.add_argument("--num_machines", default=1, type=int)
    p.add_argument("--machine_rank", default=0, type=int)
    p.add_argument("--fp16", dest="fp16", default=False, action="store_true")
    p.add_argument("--cache", type=str, nargs="?", const="ram")
    p.add_argument("-o", "--occupy", dest="occupy", default=False, action="store_true")
    p.add_argument("-l", "--logger", type=str, default="tensorboard")
    p.add_argument("-D", type=str, metavar="OPT=VALUE", action="append")
    p.add_argument("--max-iter", dest="max_iter", type=int, default=None, help="stop after this many iterations")
    p.add_argument("--dataset-size", dest="dataset_size", type=int, default=118287)
    p.add_argument("--freeze", type=str, nargs="+", default=None, metavar="NAME",
                   help="freeze parameters / sub-modules whose name contains NAME (e.g. backbone, head.stems)")
    return p


def train(config: YoloxConfig, args) -> None:
    """cli/train.py:95-113."""
    if config.seed is not None:
        random.seed(config.seed)
        torch.manual_seed(config.seed)
    trainer = config.get_trainer(args)
    trainer.train()


def check_args(args) -> None:
    """The argument errors of cli/train.py:118-119 plus what this path does not build."""
    if args.config is None:
        raise AttributeError("Please specify a model configuration.")
    if args.cache:
        raise NotImplementedError("--cache: dataset caches are out of scope")


def main(argv: list) -> None:
    """cli/train.py:116-143: resolve and validate the config, then one process per GPU."""
    args = make_parser().parse_args(argv)
    check_args(args)
    config = resolve_config(args.config)
    config.update(parse_model_config_opts(args.D))
    if args.freeze:
        config.update({"freeze": tuple(args.freeze)})
    config.validate()
    if not args.name:
        args.name = config.name
    ngpu = torch.cuda.device_count()  # does not initialise the device on this image
    num_gpu = ngpu if args.devices is None else args.devices
    if args.dist_backend == "nccl":
        assert 0 < num_gpu <= ngpu, f"-d {num_gpu}: {ngpu} GPU(s) visible"
    launch(train, num_gpu, args.num_machines, args.machine_rank, backend=args.dist_backend,
           dist_url="auto" if args.dist_url is None else args.dist_url, args=(config, args))


def cli(argv=None) -> None:
    argv = sys.argv[1:] if argv is None else argv
    if not argv or argv[0] != "train":
        sys.exit("usage: python -m yolox_amd train -c <config> [-d N] [-b B] [--fp16] [--resume] [--ckpt FILE] "
                 "[-e N] [--freeze NAME ...] [-D k=v ...]")
    main(argv[1:])
