"""One dataclass config with per-entrypoint presets.

The reference hard-codes every constant per script; each preset below reproduces one
script's constants (file:line cited), and every field can be overridden from the CLI
(`parse_args`).
"""
from __future__ import annotations

import argparse
import dataclasses
import math
from dataclasses import dataclass, field
from typing import List, Optional


@dataclass
class TrainConfig:
    # identity
    preset: str = "single"
    model_name: str = "ResNet50_ImageNet"          # imagenet-resnet50.py:61
    # data
    data: str = "synthetic"                        # synthetic | records:<dir>
    image_size: int = 224                          # resize_with_crop target (imagenet-resnet50.py:39)
    crop: int = 244                                # RandomCrop(244,244) (imagenet-resnet50.py:54), Q1
    flip: bool = True                              # RandomFlip("horizontal") (imagenet-resnet50.py:55)
    num_classes: int = 1000
    train_images: int = 1281167                    # ImageNet-1k train split
    val_images: int = 50000
    steps_per_epoch: Optional[int] = None          # PS: 312500 (imagenet-resnet50-ps.py:143)
    validation_steps: Optional[int] = None
    seed: int = 0
    # batch
    batch_size: int = 32                           # per replica (imagenet-resnet50.py:46)
    val_batch_size: Optional[int] = None           # MWMS: 256 per replica (multiworkers.py:72)
    global_batch_mode: str = "per_replica"         # per_replica | global (pretrained MWMS: 32*n_workers global)
    # model
    weights: str = "none"                          # none | imagenet | <path.h5>
    bn_mode: str = "frozen"                        # frozen (training=False, Q3) | train
    precision: str = "bf16"                        # bf16 compute, fp32 master
    # optimizer
    optimizer: str = "adam"                        # imagenet-resnet50.py:62
    lr: float = 1e-3                               # Keras Adam default
    lr_scale_by_size: bool = False                 # hvd: lr = 0.1 * size (imagenet-resnet50-hvd.py:99)
    momentum: float = 0.9
    nesterov: bool = False
    weight_decay: float = 0.0
    beta1: float = 0.9
    beta2: float = 0.999
    adam_eps: float = 1e-7
    lars_eta: float = 1e-3                         # LARS trust coefficient
    lars_eps: float = 0.0                          # LARS: added to the trust ratio's denominator
    label_smoothing: float = 0.0                   # eps of the loss target (1 - eps) * onehot + eps / num_classes
                                                   # (Keras CategoricalCrossentropy(label_smoothing)); training,
                                                   # validation and --evaluate all report this loss
    mixup: float = 0.0                             # additive: mixup alpha (lambda ~ Beta(alpha, alpha)); 0 = off
    cutmix: float = 0.0                            # additive: CutMix alpha; 0 = off (both on: one of the two per batch)
    mix_prob: float = 1.0                          # probability that a training batch is mixed at all
    global_clipnorm: Optional[float] = None        # additive (Keras `global_clipnorm`): the whole gradient is scaled
                                                   # by C / max(|g|, C) before the update; None = off
    skip_nonfinite: bool = False                   # additive: a step whose gradient norm is inf / nan updates nothing
    # training loop
    epochs: int = 50                               # imagenet-resnet50.py:67
    verbose: int = 2
    reduce_lr_patience: int = 5                    # ReduceLROnPlateau (imagenet-resnet50.py:64)
    reduce_lr_factor: float = 0.1
    min_lr: float = 1e-5
    early_stop_patience: int = 10                  # EarlyStopping (imagenet-resnet50.py:65)
    early_stop_min_delta: float = 1e-3
    warmup_epochs: int = 0                         # hvd LearningRateWarmupCallback (hvd.py:115): 3
    lr_schedule: str = "plateau"                   # plateau (the reference's callbacks) | poly: per-step warm-up
                                                   # over warmup_epochs + power-2 decay to lr_end, on the device
    lr_end: float = 1e-4                           # poly: the rate at and after the last step
    # distribution
    strategy: str = "single"                       # single | mirrored | multiworker | horovod | ps
    bucket_mb: float = 32.0                        # gradient bucket size (7-link xGMI tuned); <= 0: autotune
    grad_dtype: str = "fp32"                       # all-reduce dtype
    accum_steps: int = 1                           # micro-batches per update (Horovod's backward_passes_per_step)
    num_ps: int = 1
    num_workers: int = 1
    port_base: int = 12345                         # SlurmClusterResolver(port_base=12345) (multiworkers.py:16)
    min_shard_bytes: int = 256 << 10               # MinSizePartitioner (ps.py:77)
    shard_by: str = "batch"                        # hvd: batch-then-shard (hvd.py:77-78); mwms: element DATA
    ps_overlap: bool = True                        # PS: a worker's push/pull round trip overlaps its next step
    ps_wire: str = "bf16"                          # PS: gradient push / parameter pull element type on GPU roles
                                                   # (bf16 halves the xGMI bytes; fp32 master + Adam on the PS; CPU: fp32)
    # device / output
    device: str = "auto"                           # auto | cpu | cuda
    save: bool = True
    save_dir: str = "."
    checkpoint_every: int = 0                      # additive: periodic checkpoints (0 = off)
    resume: Optional[str] = None
    metrics_jsonl: Optional[str] = None
    data_cache: Optional[str] = None               # tfds / folder data: decoded-image cache directory (--cache)
    baseline_ips: Optional[float] = None           # 1-GPU images/sec: the JSONL log adds scaling efficiency
    timeline: Optional[str] = None                 # chrome-trace JSON of the fusion engine
    graphs: Optional[bool] = None                  # HIP graphs: None = auto (on for Mirrored / local replicas)
    roctx: bool = False                            # roctx ranges per step phase (utils/profiling.py)
    max_steps: Optional[int] = None                # cap steps per epoch (smoke / bench)
    evaluate: bool = False                         # --evaluate: score the validation split and exit (no training)

    def replace(self, **kw) -> "TrainConfig":
        return dataclasses.replace(self, **kw)

    def checkpoint_name(self, n_gpus: Optional[int] = None) -> str:
        """'ImageNet-' + model.name + '-reuse.h5' (imagenet-resnet50.py:69-70); Horovod adds
        '-<N>GPUs' (imagenet-resnet50-hvd.py:127, with the int+str bug Q7 fixed)."""
        if self.preset == "horovod" and n_gpus is not None:
            return f"ImageNet-{self.model_name}-{n_gpus}GPUs-reuse.h5"
        return f"ImageNet-{self.model_name}-reuse.h5"


PRESETS = {
    # imagenet-resnet50.py / imagenet-pretrained-resnet50.py
    "single": dict(strategy="single", model_name="ResNet50_ImageNet", batch_size=32, crop=244),
    "single_pretrained": dict(strategy="single", model_name="ResNet50_ImageNet", batch_size=32, crop=244,
                              weights="imagenet"),
    # imagenet-resnet50-mirror.py:21,54 (global = 32 * replicas)
    "mirrored": dict(strategy="mirrored", model_name="ResNet50_ImageNet_mirror", batch_size=32, crop=244),
    "mirrored_pretrained": dict(strategy="mirrored", model_name="ResNet50_ImageNet_mirror", batch_size=32,
                                crop=244, weights="imagenet"),
    # imagenet-resnet50-multiworkers.py:70,72 (128 / 256 per replica, DATA sharding)
    "multiworker": dict(strategy="multiworker", model_name="ResNet50_ImageNet_Multiworkers", batch_size=128,
                        val_batch_size=256, crop=244, shard_by="element", verbose=1),
    # imagenet-pretrained-resnet50-multiworkers.py:63,65 (global 32 * n_workers)
    "multiworker_pretrained": dict(strategy="multiworker", model_name="ResNet50_Pretrained_ImageNet_Multiworkers",
                                   batch_size=32, crop=244, weights="imagenet", shard_by="element"),
    # imagenet-resnet50-ps.py:77,120,143
    "ps": dict(strategy="ps", model_name="ResNet50_ImageNet_PS", batch_size=32, crop=244,
               steps_per_epoch=312500, validation_steps=1562, num_ps=1, num_workers=1),
    # imagenet-resnet50-hvd.py:25,89,99,115
    "horovod": dict(strategy="horovod", model_name="ResNet50_ImageNet", batch_size=32, crop=160,
                    lr=0.1, lr_scale_by_size=True, warmup_epochs=3, shard_by="batch"),
    # the benchmark configuration (BASELINE.json: synthetic 3x224x224, random init, bf16)
    "bench": dict(strategy="horovod", model_name="ResNet50_ImageNet", batch_size=256, crop=224,
                  lr=1e-3, lr_scale_by_size=False, warmup_epochs=0, save=False, verbose=0),
}


def check_accum(cfg: TrainConfig) -> None:
    """--accum-steps K: what cannot be combined with K > 1 is a configuration error, raised
    before anything is built."""
    k = cfg.accum_steps
    if not isinstance(k, int) or isinstance(k, bool) or k < 1:
        raise ValueError(f"--accum-steps must be an integer >= 1 (got {k!r})")
    if k == 1:
        return
    if cfg.graphs is True:
        raise ValueError("--graphs cannot be combined with --accum-steps > 1: the whole-step graph contains the "
                         "optimizer update (drop --graphs; accumulation runs the eager step)")
    if cfg.bucket_mb <= 0:
        raise ValueError("--bucket-mb 0 (autotune) cannot be combined with --accum-steps > 1: the autotune times "
                         "single steps (pass a bucket size)")
    if cfg.strategy == "ps":
        raise ValueError("--accum-steps > 1 is not supported for --strategy ps: every worker push is one "
                         "asynchronous update on the parameter servers")


def check_loss(cfg: TrainConfig) -> None:
    """--label-smoothing eps: a value outside [0, 1] is a configuration error, raised before
    anything is built."""
    eps = cfg.label_smoothing
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0.0 <= eps <= 1.0:
        raise ValueError(f"--label-smoothing must be a number in [0, 1] (got {eps!r})")


def check_mix(cfg: TrainConfig) -> None:
    """--mixup / --cutmix ALPHA and --mix-prob P: a negative or non-finite alpha, or P outside
    [0, 1], is a configuration error, raised before anything is built."""
    for flag, a in (("--mixup", cfg.mixup), ("--cutmix", cfg.cutmix)):
        if isinstance(a, bool) or not isinstance(a, (int, float)) or not math.isfinite(a) or a < 0:
            raise ValueError(f"{flag} must be a finite number >= 0 (got {a!r})")
    p = cfg.mix_prob
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:
        raise ValueError(f"--mix-prob must be a number in [0, 1] (got {p!r})")


def check_clip(cfg: TrainConfig) -> None:
    """--global-clipnorm C / --skip-nonfinite: a threshold that is no finite number > 0, or either
    option on the parameter server, is a configuration error, raised before anything is built."""
    c = cfg.global_clipnorm
    if c is not None and (isinstance(c, bool) or not isinstance(c, (int, float)) or not math.isfinite(c) or c <= 0):
        raise ValueError(f"--global-clipnorm must be a finite number > 0 (got {c!r})")
    if cfg.strategy == "ps" and (c is not None or cfg.skip_nonfinite):
        raise ValueError("--global-clipnorm / --skip-nonfinite are not supported for --strategy ps: every parameter-"
                         "server shard applies its own Adam to one worker's push, so no process holds a whole "
                         "gradient to take the global norm of")


def make_config(preset: str = "single", **overrides) -> TrainConfig:
    if preset not in PRESETS:
        raise ValueError(f"unknown preset {preset!r}; choose from {sorted(PRESETS)}")
    kw = dict(PRESETS[preset])
    kw.update({k: v for k, v in overrides.items() if v is not None})
    kw["preset"] = preset.split("_")[0] if preset.endswith("_pretrained") else preset
    return TrainConfig(**kw)


def add_cli_args(ap: argparse.ArgumentParser) -> argparse.ArgumentParser:
    """CLI overrides shared by every entry script."""
    a = ap.add_argument
    a("--epochs", type=int)
    a("--batch-size", type=int, dest="batch_size")
    a("--val-batch-size", type=int, dest="val_batch_size")
    a("--crop", type=int)
    a("--image-size", type=int, dest="image_size")
    a("--precision", choices=["bf16", "fp32"])
    a("--bn-mode", choices=["frozen", "train"], dest="bn_mode")
    a("--optimizer", choices=["adam", "sgd", "lars"])
    a("--lr", type=float)
    a("--momentum", type=float)
    a("--weight-decay", type=float, dest="weight_decay")
    a("--nesterov", action="store_true", default=None, help="SGD: Nesterov momentum")
    a("--lars-eta", type=float, dest="lars_eta", help="LARS trust coefficient")
    a("--lars-eps", type=float, dest="lars_eps", help="LARS: added to the trust ratio's denominator")
    a("--label-smoothing", type=float, dest="label_smoothing",
      help="eps in [0, 1]: the loss target is (1 - eps) * onehot + eps / num_classes (0.1 in the large-batch "
           "recipes); loss, val_loss and --evaluate all report the smoothed loss")
    a("--mixup", type=float, metavar="ALPHA",
      help="mixup: each training batch is blended with a permutation of itself, lambda ~ Beta(ALPHA, ALPHA), inside "
           "the preprocess kernel, and the loss takes the matching soft target (0 = off; 0.2 in the usual recipes)")
    a("--cutmix", type=float, metavar="ALPHA",
      help="CutMix: a random box of each image is replaced by its partner's, lambda ~ Beta(ALPHA, ALPHA), the label "
           "weight being the kept area (0 = off; 1.0 in the usual recipes); with --mixup, each mixed batch takes one "
           "of the two with probability 1/2")
    a("--mix-prob", type=float, dest="mix_prob", metavar="P",
      help="probability in [0, 1] that a training batch is mixed (default 1; needs --mixup or --cutmix)")
    a("--global-clipnorm", type=float, dest="global_clipnorm",
      help="C > 0: scale the whole gradient by C / max(|g|, C) before the update (Keras global_clipnorm), the norm "
           "taken on the device in a fixed order; with --accum-steps K the optimizer only runs on the K-th "
           "micro-step, so the norm is that of the folded mean gradient; not with --strategy ps")
    a("--skip-nonfinite", action="store_true", default=None, dest="skip_nonfinite",
      help="a step whose gradient norm is inf / nan leaves parameters and optimizer state untouched (the step "
           "count still advances); not with --strategy ps")
    a("--lr-schedule", choices=["plateau", "poly"], dest="lr_schedule",
      help="plateau: ReduceLROnPlateau (+ the Horovod warm-up); poly: per-step linear warm-up over "
           "--warmup-epochs, then power-2 decay to --lr-end at the last step, computed on the device")
    a("--lr-end", type=float, dest="lr_end")
    a("--warmup-epochs", type=int, dest="warmup_epochs")
    a("--data", type=str)
    a("--cache", type=str, dest="data_cache")
    a("--steps-per-epoch", type=int, dest="steps_per_epoch")
    a("--validation-steps", type=int, dest="validation_steps")
    a("--max-steps", type=int, dest="max_steps")
    a("--evaluate", action="store_true", default=None,
      help="score the validation split (loss, top-1, top-5) with --weights / --resume loaded; trains and saves nothing")
    a("--bucket-mb", type=float, dest="bucket_mb")
    a("--grad-dtype", choices=["fp32", "bf16"], dest="grad_dtype")
    a("--accum-steps", "--backward-passes-per-step", type=int, dest="accum_steps",
      help="gradient accumulation: every K-th step all-reduces and applies ONE update from the mean gradient over "
           "K micro-batches (effective global batch = K x global batch); --steps-per-epoch must be a multiple of K")
    a("--weights", type=str)
    a("--device", choices=["auto", "cpu", "cuda"])
    a("--seed", type=int)
    a("--save-dir", type=str, dest="save_dir")
    a("--no-save", action="store_false", dest="save", default=None)
    a("--resume", type=str)
    a("--checkpoint-every", type=int, dest="checkpoint_every")
    a("--metrics-jsonl", type=str, dest="metrics_jsonl")
    a("--baseline-ips", type=float, dest="baseline_ips")
    a("--timeline", type=str)
    a("--graphs", action="store_true", default=None)
    a("--no-graphs", action="store_false", dest="graphs", default=None)
    a("--roctx", action="store_true", default=None)
    a("--verbose", type=int)
    a("--ps-wire", choices=["fp32", "bf16"], dest="ps_wire",
      help="PS: element type of the gradient push and the parameter pull (GPU roles)")
    a("--ps-sync", action="store_false", dest="ps_overlap", default=None,
      help="PS: block on every push/pull round trip (no overlap with the next step)")
    return ap


def config_from_args(preset: str, argv: Optional[List[str]] = None, extra=None) -> TrainConfig:
    ap = argparse.ArgumentParser(description=f"pddl ResNet-50 training ({preset})")
    add_cli_args(ap)
    if extra is not None:
        extra(ap)
    ns, _ = ap.parse_known_args(argv)
    kw = {k: v for k, v in vars(ns).items() if v is not None and k in TrainConfig.__dataclass_fields__}
    cfg = make_config(preset, **kw)
    cfg._ns = ns  # type: ignore[attr-defined]
    return cfg
