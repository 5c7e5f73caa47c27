"""Flat-buffer optimizers: one fused HIP launch over all trainable parameters.

Adam reproduces TF/Keras `ResourceApplyAdam` (epsilon-hat form; imagenet-resnet50.py:62),
SGD reproduces `keras.optimizers.SGD(momentum, nesterov)` — the north-star optimizer
(BASELINE.json).  LARS (You et al., the MLPerf ResNet-50 form) is the large-batch optimizer:
momentum SGD whose step is scaled per layer by a trust ratio, in two launches over a segment
table of the flat buffer.  On CPU the same update runs as torch ops (reference semantics).
"""
from __future__ import annotations

import math

import torch


def scheduled_lr(lr: float, t: int, warmup_steps: int, total_steps: int, end_lr: float) -> float:
    """Learning rate of step t (1-based): linear warm-up from 0 to `lr` over `warmup_steps`,
    polynomial decay (power 2) to `end_lr` at `total_steps`, `end_lr` after that.  The device
    computes the same expression (opt_hparams_sched_kernel)."""
    if t <= warmup_steps:
        return lr * t / warmup_steps
    if t < total_steps:
        rem = (total_steps - t) / (total_steps - warmup_steps)
        return end_lr + (lr - end_lr) * rem * rem
    return end_lr


GRAD_NORM_CHUNK = 16384  # floats per block of the global-norm pass (kGradNormDefaultChunk)


class FlatOptimizer:
    """On the GPU the step counter and learning rate live in a device buffer
    `hs = {t, lr, lr_t, lr_sched, warmup_steps, total_steps, end_lr, -}` advanced by a
    one-thread kernel, so a captured step (HIP graph) replays correctly; host-side changes (LR
    callbacks, checkpoint restore) are written to it before the next step, outside any capture.
    With a schedule (`set_schedule`) that kernel also derives the step's learning rate from the
    step count, so a per-step schedule costs no host write at all.

    Global-norm clipping and the non-finite skip (`set_grad_clip`, both off by default) add one
    norm pass before the update: `gn = {norm, scale, skip, clip, skip_enabled, clipped steps,
    skipped steps, -}` is a second device buffer, filled by `native.grad_norm` in a fixed
    reduction order (bit-identical on every replica) and read by the update kernel, which
    multiplies `scale = clip / max(norm, clip)` into the gradient scale and does nothing at all
    when `skip` is set.  The threshold is host-written like `lr`, so a captured step replays with
    a changed threshold.  With both off, `gn` is None and a step makes exactly the calls it made
    before."""

    def __init__(self, engine, lr: float):
        self.engine = engine
        self.n = engine.L.n_trainable
        self.params = engine.params[: self.n]
        self.grads = engine.grads
        self.gscale = 1.0
        self.hs = torch.zeros(8, dtype=torch.float32, device=self.params.device) if self.params.is_cuda else None
        self._lr = float(lr)
        self._iterations = 0         # Keras `optimizer.iterations`
        self._dirty = True
        self._sched = None           # (warmup_steps, total_steps, end_lr) or None
        self._clip = None            # global_clipnorm threshold or None
        self._skip_nonfinite = False
        self.gn = None               # device float[8] (a host list on the CPU) while clipping / skipping is on
        self.gn_partials = None      # one float per chunk of the norm pass
        self.gn_chunk = GRAD_NORM_CHUNK

    @property
    def on_gpu(self):
        return self.params.is_cuda

    @property
    def lr(self):
        return self._lr

    @lr.setter
    def lr(self, v):
        self._lr = float(v)
        self._dirty = True

    @property
    def iterations(self):
        return self._iterations

    @iterations.setter
    def iterations(self, v):
        self._iterations = int(v)
        self._dirty = True

    def set_schedule(self, warmup_steps: int, total_steps: int, end_lr: float):
        """Warm-up + polynomial decay of `lr` by step count (`scheduled_lr`), evaluated on the
        device.  Install it before the step is captured into a graph: the capture records which
        hparams kernel runs.  `lr` stays the peak rate; the position is `iterations`."""
        warmup_steps, total_steps = int(warmup_steps), int(total_steps)
        if warmup_steps < 0 or total_steps <= warmup_steps:
            raise ValueError("schedule needs 0 <= warmup_steps < total_steps")
        if total_steps >= 1 << 24:
            raise ValueError("schedule: total_steps must stay below 2**24 (the device step counter is fp32)")
        self._sched = (warmup_steps, total_steps, float(end_lr))
        self._dirty = True

    @property
    def schedule(self):
        return self._sched

    def lr_at(self, t: int) -> float:
        """The learning rate step t runs at (before Adam's bias correction)."""
        return self._lr if self._sched is None else scheduled_lr(self._lr, t, *self._sched)

    @property
    def current_lr(self) -> float:
        """The rate of the most recent step (the base rate before the first)."""
        return self.lr_at(max(self._iterations, 1)) if self._sched is not None else self._lr

    def set_grad_clip(self, global_clipnorm=None, skip_nonfinite=False):
        """`global_clipnorm` C (Keras): the whole gradient is scaled by C / max(norm, C), norm the
        L2 norm of gscale * grads over all trainable parameters; None measures only.
        `skip_nonfinite`: a step whose norm is inf / nan (some non-finite gradient, or an fp32
        overflow of the sum of squares) changes neither the parameters nor the optimizer state;
        `iterations` still advances.  With either on, `clip_stats()` reports the norm.  Turn
        them on before the step is captured into a graph (the capture records the norm pass); a
        later change of the threshold reaches the next replay through `sync_hparams`."""
        if global_clipnorm is not None:
            c = global_clipnorm
            if isinstance(c, bool) or not isinstance(c, (int, float)) or not math.isfinite(c) or c <= 0:
                raise ValueError(f"global_clipnorm must be a finite number > 0 (got {c!r})")
        self._clip = None if global_clipnorm is None else float(global_clipnorm)
        self._skip_nonfinite = bool(skip_nonfinite)
        if not self.clip_active:
            self.gn = self.gn_partials = None
        elif self.gn is None:
            if self.on_gpu:
                dev = self.params.device
                self.gn = torch.zeros(8, dtype=torch.float32, device=dev)
                self.gn[1] = 1.0
                self.gn_partials = torch.zeros(-(-self.n // self.gn_chunk), dtype=torch.float32, device=dev)
            else:
                self.gn = [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
        self._dirty = True

    @property
    def clip_active(self) -> bool:
        return self._clip is not None or self._skip_nonfinite

    @property
    def global_clipnorm(self):
        return self._clip

    @property
    def skip_nonfinite(self) -> bool:
        return self._skip_nonfinite

    def clip_stats(self):
        """{"norm", "scale"} of the most recent step (the norm before clipping) and the counts
        {"clipped", "skipped"} since the last `reset_clip_counters()`; one device-to-host copy.
        None while neither clipping nor the skip is on."""
        if self.gn is None:
            return None
        if self.on_gpu:
            torch.cuda.synchronize(self.params.device)   # (the step may have run on a replica's own stream)
        gn = self.gn.cpu().tolist() if self.on_gpu else self.gn
        return {"norm": gn[0], "scale": gn[1], "clipped": int(gn[5]), "skipped": int(gn[6])}

    def reset_clip_counters(self):
        if self.gn is not None:
            if self.on_gpu:
                self.gn[5:7].zero_()
            else:
                self.gn[5] = self.gn[6] = 0.0

    def sync_hparams(self):
        """Write host-side lr / step count / schedule (and the clip threshold and skip switch) into
        the device buffers (never inside a capture)."""
        if self.hs is not None and self._dirty:
            wu, tot, end = self._sched or (0, 0, 0.0)
            self.hs.copy_(torch.tensor([float(self._iterations), self._lr, 0.0, 0.0, float(wu), float(tot), end, 0.0]),
                          non_blocking=False)
            if self.gn is not None:
                self.gn[3:5].copy_(torch.tensor([self._clip or 0.0, float(self._skip_nonfinite)]), non_blocking=False)
            self._dirty = False

    def _device_step(self, adam: bool, b1=0.0, b2=0.0):
        from ..ops.native import native
        if not torch.cuda.is_current_stream_capturing():
            self.sync_hparams()
        if self._sched is None:
            native.opt_hparams(self.hs, b1, b2, adam)
        else:
            native.opt_hparams_sched(self.hs, b1, b2, adam)
        if self.gn is not None:
            native.grad_norm(self.grads[: self.n], self.gscale, self.gn_chunk, self.gn_partials, self.gn)

    def _host_clip(self):
        """CPU form of the norm pass: (skip, gradient scale including the clip scale).  The norm
        is taken in float64; the scale formula and the counters are the device's."""
        if self.gn is None:
            return False, self.gscale
        gn = self.gn
        gn[3], gn[4] = self._clip or 0.0, float(self._skip_nonfinite)
        g = self.grads[: self.n].double() * self.gscale
        norm = float((g * g).sum().sqrt())
        scale = gn[3] / norm if gn[3] > 0 and norm > gn[3] else 1.0
        skip = bool(gn[4]) and not math.isfinite(norm)
        gn[0], gn[1], gn[2] = norm, scale, float(skip)
        gn[5] += scale < 1.0 and not skip
        gn[6] += skip
        return skip, self.gscale * scale

    def state_tensors(self):
        return {}


class Adam(FlatOptimizer):
    def __init__(self, engine, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7):
        super().__init__(engine, lr)
        self.b1, self.b2, self.eps = beta1, beta2, eps
        self.m = torch.zeros_like(self.params)
        self.v = torch.zeros_like(self.params)

    def step(self):
        if self.on_gpu:
            from ..ops.native import native
            self._device_step(True, self.b1, self.b2)
            self._iterations += 1
            native.adam(self.params, self.grads, self.m, self.v, 0.0, self.b1, self.b2, self.eps, self.gscale, self.hs,
                        self.gn)
        else:
            self._iterations += 1
            skip, gs = self._host_clip()
            if skip:
                return
            t = self._iterations
            lr_t = self.lr_at(t) * math.sqrt(1 - self.b2 ** t) / (1 - self.b1 ** t)
            g = self.grads * gs
            self.m.mul_(self.b1).add_(g, alpha=1 - self.b1)
            self.v.mul_(self.b2).addcmul_(g, g, value=1 - self.b2)
            self.params.sub_(lr_t * self.m / (self.v.sqrt() + self.eps))

    def state_tensors(self):
        return {"m": self.m, "v": self.v}


class SGD(FlatOptimizer):
    def __init__(self, engine, lr=0.1, momentum=0.9, nesterov=False, weight_decay=0.0):
        super().__init__(engine, lr)
        self.mu, self.nesterov, self.wd = momentum, nesterov, weight_decay
        self.mom = torch.zeros_like(self.params)

    def step(self):
        if self.on_gpu:
            from ..ops.native import native
            self._device_step(False)
            self._iterations += 1
            native.sgd(self.params, self.grads, self.mom, 0.0, self.mu, self.wd, self.nesterov, self.gscale, self.hs,
                       self.gn)
        else:
            self._iterations += 1
            skip, gs = self._host_clip()
            if skip:
                return
            lr = self.lr_at(self._iterations)
            g = self.grads * gs + self.wd * self.params
            self.mom.mul_(self.mu).sub_(lr * g)
            if self.nesterov:
                self.params.add_(self.mu * self.mom - lr * g)
            else:
                self.params.add_(self.mom)

    def state_tensors(self):
        return {"momentum": self.mom}


LARS_CHUNK = 16384       # floats per block of the norm / update passes (kLarsDefaultChunk)


def lars_table(segments, chunk: int = LARS_CHUNK) -> torch.Tensor:
    """Host segment table, int32 [nseg][4] = {offset, size, adapt, chunk0}, from (offset, size,
    adapt) triples in ascending order.  chunk0 is the running count of ceil(size / chunk): block
    chunk0 + c of both passes owns chunk c of the segment, so the table and the chunk size fix
    the reduction order."""
    rows, c0 = [], 0
    for off, size, adapt in segments:
        rows.append([int(off), int(size), int(bool(adapt)), c0])
        c0 += -(-int(size) // chunk)
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 4)


def lars_chunks(table: torch.Tensor, chunk: int) -> int:
    return int(sum(-(-int(size) // chunk) for size in table[:, 1].tolist()))


def lars_segments(L):
    """[(offset, size, adapt, layer name or None)] over the trainable prefix of a ParamLayout:
    every `kernel` entry is one adapted segment (53 conv kernels + the dense kernel), runs of
    per-channel entries (biases, BN gamma / beta) merge into non-adapted segments.  The
    alignment padding after the last entry belongs to no segment."""
    segs = []
    ents = sorted((e for e in L.entries.values() if e.trainable), key=lambda e: e.offset)
    for e in ents:
        if e.kind == "kernel":
            segs.append((e.offset, e.size, 1, e.layer))
        elif segs and not segs[-1][2] and segs[-1][0] + segs[-1][1] == e.offset:
            segs[-1] = (segs[-1][0], segs[-1][1] + e.size, 0, None)
        else:
            segs.append((e.offset, e.size, 0, None))
    return segs


class LARS(FlatOptimizer):
    """Layer-wise adaptive rate scaling.  For a kernel w with gradient g (gs the gradient scale):
        ratio = eta |w| / (|gs g| + wd |w| + eps)   (1 when either norm is 0)
        v <- mu v + lr ratio (gs g + wd w);   w <- w - v
    Biases and BN parameters take ratio 1 and no weight decay.  On the GPU the norms are a
    segmented reduction in a fixed order (bit-identical on every replica and every run), and
    lr, the step count and the trust ratios stay on the device, so the step captures into a
    HIP graph."""

    def __init__(self, engine, lr=0.1, momentum=0.9, weight_decay=0.0, eta=1e-3, eps=0.0, nesterov=False,
                 chunk=None):
        if nesterov:
            raise ValueError("LARS has no Nesterov form here: use --optimizer sgd --nesterov, or drop --nesterov")
        super().__init__(engine, lr)
        self.mu, self.wd, self.eta, self.eps = momentum, weight_decay, eta, eps
        self.nesterov = False
        self.mom = torch.zeros_like(self.params)
        self.chunk = int(chunk or LARS_CHUNK)
        self.segments = lars_segments(engine.L)
        self.table_host = lars_table([s[:3] for s in self.segments], self.chunk)
        dev = self.params.device
        self.ratios = torch.ones(len(self.segments), dtype=torch.float32, device=dev)
        if self.on_gpu:
            self.table = self.table_host.to(dev)
            self.partials = torch.zeros(2 * lars_chunks(self.table_host, self.chunk), dtype=torch.float32, device=dev)

    def step(self):
        if self.on_gpu:
            from ..ops.native import native
            self._device_step(False)
            self._iterations += 1
            native.lars(self.params, self.grads, self.mom, self.table, self.table_host, self.chunk, self.partials,
                        self.ratios, 0.0, self.mu, self.wd, self.eta, self.eps, self.gscale, self.hs, self.gn)
        else:
            self._iterations += 1
            skip, gs = self._host_clip()
            if skip:
                return
            lr = self.lr_at(self._iterations)
            for i, (off, size, adapt, _) in enumerate(self.segments):
                w = self.params[off:off + size]
                g = self.grads[off:off + size] * gs
                v = self.mom[off:off + size]
                ratio, wd = 1.0, 0.0
                if adapt:
                    wd = self.wd
                    wn, gn = float((w * w).sum().sqrt()), float((g * g).sum().sqrt())
                    if wn > 0 and gn > 0:
                        ratio = self.eta * wn / (gn + wd * wn + self.eps)
                self.ratios[i] = ratio
                v.mul_(self.mu).add_(g + wd * w, alpha=lr * ratio)
                w.sub_(v)

    def state_tensors(self):
        return {"momentum": self.mom}

    def trust_ratios(self):
        """{layer name: trust ratio of the most recent step} for the adapted (kernel) segments."""
        r = self.ratios.detach().cpu().tolist()
        return {name: r[i] for i, (_, _, adapt, name) in enumerate(self.segments) if adapt}


def make_optimizer(name: str, engine, lr: float, **kw) -> FlatOptimizer:
    opt = _make_optimizer(name, engine, lr, **kw)
    if kw.get("global_clipnorm") is not None or kw.get("skip_nonfinite"):
        opt.set_grad_clip(kw.get("global_clipnorm"), bool(kw.get("skip_nonfinite")))
    return opt


def _make_optimizer(name: str, engine, lr: float, **kw) -> FlatOptimizer:
    if name == "lars":
        return LARS(engine, lr, kw.get("momentum", 0.9), kw.get("weight_decay", 0.0), kw.get("lars_eta", 1e-3),
                    kw.get("lars_eps", 0.0), kw.get("nesterov", False))
    if name == "adam":
        return Adam(engine, lr, kw.get("beta1", 0.9), kw.get("beta2", 0.999), kw.get("eps", 1e-7))
    if name == "sgd":
        return SGD(engine, lr, kw.get("momentum", 0.9), kw.get("nesterov", False), kw.get("weight_decay", 0.0))
    raise ValueError(f"unknown optimizer {name!r}")
