"""Mixup (Zhang et al.) and CutMix (Yun et al.) draws, as the per-image table the stem and
loss-head kernels read (csrc/kernels/kernels.h, `StemParams::mix`).

A table is int32 [B][8]; row b = (partner, y0, x0, y1, x1, w_pix bits, w_lab bits, 0):
image b's pixel becomes w*A_b + (1 - w)*A_partner with w = 0 inside the half-open box and
w_pix outside, and its target w_lab*T(y_b) + (1 - w_lab)*T(y_partner).  The tables are built on
the host (numpy) and uploaded by the caller (parallel/strategies.py `Augment.mix`).

Draws are per batch, as in both papers: one permutation, one lambda ~ Beta(alpha, alpha) and, for
CutMix, one box for the whole batch."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np

COLS = 8


def _bits(w: float) -> int:
    return int(np.array(w, dtype=np.float32).view(np.int32))


def identity_table(B: int) -> np.ndarray:
    """partner = b, empty box, both weights 1: the kernels then give the unmixed step bit for bit."""
    t = np.zeros((B, COLS), dtype=np.int32)
    t[:, 0] = np.arange(B)
    t[:, 5] = t[:, 6] = _bits(1.0)
    return t


def mixup_table(partner, lam: float) -> np.ndarray:
    """Empty box, w_pix = w_lab = lambda."""
    t = identity_table(len(partner))
    t[:, 0] = partner
    t[:, 5] = t[:, 6] = _bits(lam)
    return t


def cutmix_box(Hc: int, Wc: int, lam: float, cy: int, cx: int) -> Tuple[int, int, int, int, float]:
    """The box of sides int(Hc*sqrt(1 - lam)) x int(Wc*sqrt(1 - lam)) centred on (cy, cx), clipped
    to the image, and w_lab = 1 - (clipped area)/(Hc*Wc)."""
    r = math.sqrt(max(0.0, 1.0 - lam))
    h, w = int(Hc * r), int(Wc * r)
    y0, x0 = cy - h // 2, cx - w // 2
    y1, x1 = y0 + h, x0 + w
    y0, y1 = min(max(y0, 0), Hc), min(max(y1, 0), Hc)
    x0, x1 = min(max(x0, 0), Wc), min(max(x1, 0), Wc)
    return y0, x0, y1, x1, 1.0 - ((y1 - y0) * (x1 - x0)) / float(Hc * Wc)


def cutmix_table(partner, box: Tuple[int, int, int, int], w_lab: float) -> np.ndarray:
    """w_pix = 1 (outside the box the image is its own), the partner's pixels inside the box."""
    t = identity_table(len(partner))
    t[:, 0] = partner
    t[:, 1:5] = np.asarray(box, dtype=np.int32)
    t[:, 6] = _bits(w_lab)
    return t


class MixSampler:
    """The per-batch draws of one replica.  Its generator is derived from the replica's seed but
    separate from the flip / crop generators, so enabling mixing changes none of their draws."""

    def __init__(self, mixup: float, cutmix: float, prob: float, Hc: int, Wc: int, seed: int):
        self.mixup, self.cutmix, self.prob = float(mixup), float(cutmix), float(prob)
        self.Hc, self.Wc = int(Hc), int(Wc)
        self.rng = np.random.default_rng([int(seed), 0x6D6978])

    @property
    def enabled(self) -> bool:
        return self.mixup > 0 or self.cutmix > 0

    def draw(self, B: int) -> Optional[np.ndarray]:
        """The table of the next batch of B images, or None when this batch is not mixed."""
        if not self.enabled:
            return None
        r = self.rng
        if not r.random() < self.prob:
            return None
        partner = r.permutation(B)
        cut = self.cutmix > 0 and (self.mixup <= 0 or r.random() < 0.5)
        if not cut:
            return mixup_table(partner, float(r.beta(self.mixup, self.mixup)))
        lam = float(r.beta(self.cutmix, self.cutmix))
        cy, cx = int(r.integers(0, self.Hc)), int(r.integers(0, self.Wc))
        y0, x0, y1, x1, w_lab = cutmix_box(self.Hc, self.Wc, lam, cy, cx)
        return cutmix_table(partner, (y0, x0, y1, x1), w_lab)
