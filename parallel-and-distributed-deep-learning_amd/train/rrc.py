"""Random-resized-crop draws (the Inception / torchvision RandomResizedCrop algorithm), as the
per-image box table the stem kernels read (csrc/kernels/kernels.h, `StemParams::rrc`).

A table is int32 [B][4]; row b = (y0, x0, h, w), a box of the H x W source image in whole pixels
that the stem kernel resizes to the crop size.  Per image: an area fraction uniform in `scale` and
a log-uniform aspect ratio w / h in `ratio` give w = round(sqrt(area * r)), h = round(sqrt(area / r));
the first of 10 tries that fits the image is placed uniformly, and an image with none takes the
centred largest box within the ratio bounds.  Tables are built on the host (numpy) and uploaded by
the caller (parallel/strategies.py `Augment.rrc`)."""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np

COLS = 4
TRIES = 10


def full_table(B: int, H: int, W: int) -> np.ndarray:
    """Every box the whole source image (a plain resize; at H x W = the crop size, the identity)."""
    t = np.zeros((B, COLS), dtype=np.int32)
    t[:, 2], t[:, 3] = H, W
    return t


def fallback_box(H: int, W: int, ratio: Tuple[float, float]) -> Tuple[int, int, int, int]:
    """The centred largest box whose aspect ratio is within the bounds."""
    r = W / H
    if r < ratio[0]:
        w, h = W, min(H, int(round(W / ratio[0])))
    elif r > ratio[1]:
        h, w = H, min(W, int(round(H * ratio[1])))
    else:
        h, w = H, W
    return (H - h) // 2, (W - w) // 2, h, w


class RrcSampler:
    """The per-batch draws of one replica.  Its generator is derived from the replica's seed but
    separate from the flip / crop / mix generators, so enabling it changes none of their draws."""

    def __init__(self, enabled: bool, scale: Tuple[float, float], ratio: Tuple[float, float], H: int, W: int, seed: int):
        self.enabled = bool(enabled)
        self.scale = (float(scale[0]), float(scale[1]))
        self.ratio = (float(ratio[0]), float(ratio[1]))
        self.H, self.W = int(H), int(W)
        self.rng = np.random.default_rng([int(seed), 0x727263])

    def draw(self, B: int) -> np.ndarray:
        """The table of the next batch of B images."""
        H, W, r = self.H, self.W, self.rng
        area = H * W * r.uniform(self.scale[0], self.scale[1], (B, TRIES))
        asp = np.exp(r.uniform(math.log(self.ratio[0]), math.log(self.ratio[1]), (B, TRIES)))
        u = r.random((B, 2))
        w = np.rint(np.sqrt(area * asp)).astype(np.int64)
        h = np.rint(np.sqrt(area / asp)).astype(np.int64)
        fits = (w > 0) & (w <= W) & (h > 0) & (h <= H)
        first = fits.argmax(1)                      # the first try that fits (0 when none does)
        rows = np.arange(B)
        t = np.empty((B, COLS), dtype=np.int64)
        t[:, 2], t[:, 3] = h[rows, first], w[rows, first]
        none = ~fits.any(1)
        t[none, 2:] = fallback_box(H, W, self.ratio)[2:]
        t[:, 0] = np.minimum((u[:, 0] * (H - t[:, 2] + 1)).astype(np.int64), H - t[:, 2])
        t[:, 1] = np.minimum((u[:, 1] * (W - t[:, 3] + 1)).astype(np.int64), W - t[:, 3])
        t[none, :2] = fallback_box(H, W, self.ratio)[:2]
        return t.astype(np.int32)
