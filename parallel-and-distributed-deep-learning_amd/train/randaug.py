"""RandAugment draws, as the widened per-image table the stem kernels read (csrc/kernels/kernels.h,
`StemParams::rrc`, "RandAugment rows"; csrc/kernels/stem_aug.hip).

A table is int32 [B][16]: columns 0..3 the image's box (train/rrc.py, or the batch's crop window),
4..9 the Q16 inverse affine map a b c / d e f, 10 the colour chain's op codes (4 bits each) and the
has_geo flag (bit 16), 11..14 the ops' fp32 parameters, 15 the grey mean the kernel fills in.

Per image N ops are drawn uniformly from OPS with a random sign, at magnitude M of the 31 bins of
the torchvision tables: shear <= 0.3, translate <= 150/331 of the crop, rotate <= 30 degrees,
brightness / color / contrast factors 1 +- 0.9 M/30, posterize to 8 - round(4 M/30) bits, solarize
at 255 (1 - M/30).  The geometric ops of an image are composed, in the order drawn, into one
matrix, so the source is sampled once (an intermediate picture's fill and rounding do not exist);
contrast takes the grey mean of the source box.  An op that changes nothing at its magnitude
(factor 1, 8 bits, threshold 255, a zero warp) is left out, so M = 0 gives identity rows."""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np

COLS = 16
ONE = 1 << 16
OPS = ("identity", "shear_x", "shear_y", "translate_x", "translate_y", "rotate",
       "brightness", "color", "contrast", "posterize", "solarize")
# the kernel's colour op codes (kernels.h)
CODE = {"brightness": 1, "color": 2, "contrast": 3, "solarize": 4, "posterize": 5}
HAS_GEO = 1 << 16


def widen(boxes: np.ndarray) -> np.ndarray:
    """A [B][4] box table as [B][16] identity rows (no map, no chain): the same pictures bit for bit."""
    t = np.zeros((boxes.shape[0], COLS), dtype=np.int32)
    t[:, :4] = boxes
    t[:, 4] = t[:, 8] = ONE
    return t


def crop_boxes(B: int, off: Tuple[int, int], crop: int) -> np.ndarray:
    """The boxes of a batch without --rrc: the batch's crop window, whole pixels (bitwise stem mode 2)."""
    return np.tile(np.array([off[0], off[1], crop, crop], dtype=np.int32), (B, 1))


def build_table(boxes: np.ndarray, op: np.ndarray, sign: np.ndarray, M: int, crop: int) -> np.ndarray:
    """The table of ops `op` [B][N] (indices into OPS) with signs `sign` [B][N] (+-1) at magnitude M."""
    B, N = op.shape
    m = M / 30.0
    t = widen(boxes)
    s = sign.astype(np.float64)
    # inverse maps in doubled centre-relative coordinates (a translation by t pixels is 2 t)
    A = np.tile(np.eye(3), (B, N, 1, 1))
    th = np.where(op == 5, s * math.radians(30.0 * m), 0.0)
    A[:, :, 0, 0] = A[:, :, 1, 1] = np.cos(th)
    A[:, :, 0, 1] = np.sin(th) + np.where(op == 1, s * 0.3 * m, 0.0)
    A[:, :, 1, 0] = -np.sin(th) + np.where(op == 2, s * 0.3 * m, 0.0)
    shift = 2.0 * s * (150.0 / 331.0) * crop * m
    A[:, :, 0, 2] = np.where(op == 3, shift, 0.0)
    A[:, :, 1, 2] = np.where(op == 4, shift, 0.0)
    total = A[:, 0]
    for k in range(1, N):            # the first op's inverse is applied last
        total = total @ A[:, k]
    q = np.rint(total[:, :2, :] * ONE).astype(np.int64).reshape(B, 6)
    t[:, 4:10] = q
    geo = (q != np.array([ONE, 0, 0, 0, ONE, 0])).any(1)
    # the colour chain: the image's colour ops in the order drawn, no-ops left out
    factor = 1.0 + s * 0.9 * m
    bits = 8 - int(round(4.0 * m))
    par = np.zeros((B, N), dtype=np.float32)
    code = np.zeros((B, N), dtype=np.int64)
    for name, c in CODE.items():
        sel = op == OPS.index(name)
        code[sel] = c
        if name == "posterize":
            par[sel] = float(256 - (1 << (8 - bits)))
            code[sel & (bits >= 8)] = 0
        elif name == "solarize":
            par[sel] = 255.0 * (1.0 - m)
            code[sel & (m <= 0)] = 0
        else:
            par[sel] = factor[sel]
            code[sel & (factor == 1.0)] = 0
    slot = np.cumsum(code > 0, axis=1) - 1
    words = np.where(geo, HAS_GEO, 0).astype(np.int64)
    pars = np.zeros((B, 4), dtype=np.float32)
    for k in range(N):
        on = code[:, k] > 0
        words[on] |= code[on, k] << (4 * slot[on, k])
        pars[on, slot[on, k]] = par[on, k]
    t[:, 10] = words
    t[:, 11:15] = pars.view(np.int32)
    return t


class RandAugSampler:
    """The per-batch draws of one replica.  Like RrcSampler its generator is derived from the
    replica's seed but is its own, so enabling it changes no flip, crop, box or mix draw."""

    def __init__(self, randaugment, crop: int, seed: int):
        self.enabled = randaugment is not None
        self.N, self.M = (int(randaugment[0]), int(randaugment[1])) if self.enabled else (0, 0)
        self.crop = int(crop)
        self.rng = np.random.default_rng([int(seed), 0x72616E64])

    def draw(self, boxes: np.ndarray) -> np.ndarray:
        """The [B][16] table of the next batch, given its [B][4] boxes."""
        B = boxes.shape[0]
        op = self.rng.integers(0, len(OPS), (B, self.N))
        sign = self.rng.integers(0, 2, (B, self.N)) * 2 - 1
        return build_table(boxes, op, sign, self.M, self.crop)
