"""Shared `main` of the drop-in entry scripts.

Each reference script (8 files under /root/reference) has a same-named script at the
repository root that calls `run(<preset>)`: identical defaults (batch, crop, optimizer,
epochs, callbacks, checkpoint file name), CLI overrides on top.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

from .config import check_accum, check_clip, check_loss, check_mix, config_from_args


def _banner(cfg, strategy):
    import torch
    print(f"Using pddl {__import__('pddl').__version__} (torch {torch.__version__}, HIP {torch.version.hip}), "
          f"strategy={cfg.strategy}, replicas={strategy.num_replicas_in_sync}, "
          f"per-replica batch={strategy.per_replica_batch}, global batch={strategy.global_batch}, "
          f"accum_steps={cfg.accum_steps}, effective global batch={strategy.global_batch * cfg.accum_steps}, "
          f"crop={cfg.crop}, bn={cfg.bn_mode}, optimizer={cfg.optimizer}, "
          f"label_smoothing={cfg.label_smoothing:g}, global_clipnorm={cfg.global_clipnorm}, "
          f"skip_nonfinite={cfg.skip_nonfinite}, "
          f"mixup={cfg.mixup:g}, cutmix={cfg.cutmix:g}, mix_prob={cfg.mix_prob:g}", flush=True)


def model_summary(cfg) -> str:
    from .models.resnet50 import ParamLayout
    L = ParamLayout(cfg.num_classes)
    kinds = [n for n, a in (("MixUp", cfg.mixup), ("CutMix", cfg.cutmix)) if a > 0]
    mix = f"  batch_mix ({' / '.join(kinds)}, p={cfg.mix_prob:g})" if kinds else ""
    return (f'Model: "{cfg.model_name}"\n'
            f"  input_1 (InputLayer) [(None, {cfg.image_size}, {cfg.image_size}, 3)]\n"
            f"  rescaling (Rescaling)  random_crop (RandomCrop {cfg.crop}x{cfg.crop})  random_flip (RandomFlip){mix}\n"
            f"  resnet50 (Functional) (None, 2048)   {L.count() - 2048 * cfg.num_classes - cfg.num_classes:,}\n"
            f"  dense (Dense) (None, {cfg.num_classes})  {2048 * cfg.num_classes + cfg.num_classes:,}\n"
            f"Total params: {L.count():,}\nTrainable params: {L.count(True):,}\n"
            f"Non-trainable params: {L.count(False):,}")


def run(preset: str, argv: Optional[List[str]] = None, extra=None) -> int:
    from .parallel.strategies import make_strategy
    from .train.trainer import Trainer, default_callbacks
    cfg = config_from_args(preset, argv, extra)
    try:
        check_loss(cfg)
        check_mix(cfg)
        check_clip(cfg)
    except ValueError as e:
        sys.stderr.write(f"{e}\n")
        return 2
    if cfg.strategy == "ps":
        if cfg.resume:
            # (the PS job's variables and Adam slots live on the PS roles; the reference has no
            # resume path at all, imagenet-resnet50-ps.py:142-148)
            sys.stderr.write("--resume is not supported for --strategy ps: the parameter-server job restarts from "
                             "--weights (the final PS checkpoint holds the trained variables, no optimizer state)\n")
            return 2
        if cfg.evaluate:
            sys.stderr.write("--evaluate is not supported for --strategy ps: score the PS checkpoint with the single "
                             "or mirrored script (--evaluate --weights <the final PS checkpoint>)\n")
            return 2
        if cfg.optimizer == "lars" or cfg.lr_schedule == "poly":
            what = "--optimizer lars" if cfg.optimizer == "lars" else "--lr-schedule poly"
            sys.stderr.write(f"{what} is not supported for --strategy ps: the parameter servers apply Adam at a "
                             "host-set rate (use the mirrored, multiworker or horovod script for large batches)\n")
            return 2
        if cfg.accum_steps != 1:
            sys.stderr.write("--accum-steps is not supported for --strategy ps: every worker push is one asynchronous "
                             "update on the parameter servers (use the single, mirrored, multiworker or horovod script)\n")
            return 2
        from .parallel.parameter_server import run_ps_job
        return run_ps_job(cfg)
    try:
        check_accum(cfg)
    except ValueError as e:
        sys.stderr.write(f"{e}\n")
        return 2
    if cfg.roctx:
        from .utils import profiling
        profiling.enable(True)
    strategy = make_strategy(cfg)
    trainer = Trainer(cfg, strategy)
    if strategy.is_chief:
        _banner(cfg, strategy)
        if cfg.verbose:
            print(model_summary(cfg), flush=True)
    if cfg.strategy == "multiworker":
        # the reference's informational print (imagenet-resnet50-multiworkers.py:76; 10M-image
        # epoch assumption, Q9) -- printed by every worker, as there
        print("Steps per epoch: ", int((10000000 / strategy.num_replicas_in_sync) / strategy.world), flush=True)
    if cfg.evaluate:
        return _evaluate(cfg, strategy, trainer)
    cbs = default_callbacks(cfg, strategy)
    initial_epoch = 0
    rs = getattr(strategy, "resume_state", None)
    if rs:          # --resume of a periodic checkpoint: epochs, LR and callback state continue
        initial_epoch = int(rs.get("epoch", 0))
        if cfg.lr_schedule != "poly":   # (poly: the rate follows the restored optimizer iteration count)
            trainer.set_lr(float(rs.get("lr", trainer.lr)))
        trainer.resume_state = rs
        if strategy.is_chief:
            print(f"Resuming after epoch {initial_epoch} at lr {trainer.lr:.4g}", flush=True)
    trainer.fit(cfg.epochs, cbs, initial_epoch=initial_epoch)
    if cfg.timeline and hasattr(strategy, "write_timeline"):
        strategy.write_timeline(cfg.timeline)
    if cfg.save:
        fname = os.path.join(cfg.save_dir, cfg.checkpoint_name(n_gpus=strategy.num_replicas_in_sync))
        if strategy.is_chief:
            print("Saving model to ", fname, flush=True)
        trainer.save(fname)
    if cfg.strategy in ("horovod", "multiworker"):
        print("All done for rank", strategy.rank, flush=True)
    _leave_process_group()
    return 0


def _leave_process_group():
    try:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.barrier()
            dist.destroy_process_group()
    except Exception:
        pass


def _evaluate(cfg, strategy, trainer) -> int:
    """--evaluate: Keras `model.evaluate` of the loaded weights over the validation split (bounded
    by --validation-steps / --max-steps).  Nothing is trained and nothing is saved."""
    import json
    import time
    strategy.sync()
    t0 = time.time()
    m = trainer.evaluate(top5=True)
    strategy.sync()
    dt = max(time.time() - t0, 1e-9)
    if strategy.is_chief:
        print(f"evaluate - loss: {m['loss']:.4f} - accuracy: {m['accuracy']:.4f} - top5_accuracy: "
              f"{m['top5_accuracy']:.4f} - {m['images']} images - {m['images'] / dt:.1f} img/s", flush=True)
        if cfg.metrics_jsonl:
            rec = {"evaluate": True, **m, "images_per_sec": m["images"] / dt,
                   "replicas": strategy.num_replicas_in_sync, "label_smoothing": cfg.label_smoothing}
            with open(cfg.metrics_jsonl, "a") as f:
                f.write(json.dumps(rec) + "\n")
    _leave_process_group()
    return 0
