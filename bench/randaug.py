"""RandAugment in the stem: what the per-image affine warp and colour chain cost the preprocess kernel.

    python bench/randaug.py [--batches 256 2560] [--out profiles/randaug_stem.txt]

The method of bench/rrc.py (device events around back-to-back launches after a warm-up, three windows
per case, their median, the windows printed).  Per batch and source size (256 -> 224 and 384 -> 224,
uint8 in, bf16 out), with and without a mixup table, on boxes drawn by train/rrc.py with the default
ranges: the tile form and the per-pixel form of stem_aug.hip on the [B][16] table train/randaug.py
draws at N = 2, M = 9 (the grey-mean launch included: it is part of every call), and the band form of
stem_rrc.hip on the same boxes (the yardstick: no warp, no chain).  The three cases are alternated and
the round is run twice, so the file shows the run-to-run spread next to the differences."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import pddl  # noqa: E402,F401
from mix import windows  # noqa: E402
from pddl.ops.native import require_native  # noqa: E402
from pddl.train.mix import mixup_table  # noqa: E402
from pddl.train.randaug import RandAugSampler  # noqa: E402
from pddl.train.rrc import RrcSampler  # noqa: E402

CROP = 224


def kernel_rows(batches, sources, emit):
    N = require_native()
    N.allow_knob_changes(True)       # (the per-pixel form is the same launch under set_variant("stem", 0))
    dev = torch.device("cuda", 0)
    hs = (CROP + 6) // 2
    for B in batches:
        mix = torch.from_numpy(mixup_table(np.random.default_rng(B).permutation(B), 0.7)).to(dev)
        x2 = torch.empty(B, hs, hs, 16, dtype=torch.bfloat16, device=dev)
        for S in sources:
            g = torch.Generator(device=dev).manual_seed(S)
            img = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device=dev, generator=g)
            flip = torch.randint(0, 2, (B,), dtype=torch.uint8, device=dev, generator=g)
            boxes = RrcSampler(True, (0.08, 1.0), (3 / 4, 4 / 3), S, S, 0).draw(B)
            wide = torch.from_numpy(RandAugSampler((2, 9), CROP, 0).draw(boxes)).to(dev)
            rrc = torch.from_numpy(boxes).to(dev)
            for mixed in (False, True):
                kw = {"mix": mix} if mixed else {}
                cases = [("aug tile", 2, wide), ("aug pixel", 1, wide), ("rrc band", 1, rrc)]
                for rnd in range(2):
                    for name, variant, tab in cases:
                        N.set_variant("stem", variant)
                        fn = (lambda: N.stem_s2d(img, flip, 0, CROP, CROP, 0, 0, x2, None, **kw, rrc=tab))
                        med, w = windows(fn, 100 if B > 1000 else 400)
                        form, _ = N.stem_last_launch()
                        N.set_variant("stem", 1)
                        emit({"case": f"stem_s2d {S}->{CROP} {name} mix={'mixup' if mixed else 'none'}", "batch": B,
                              "round": rnd, "form": form, "us": round(med, 2), "windows_us": [round(x, 2) for x in w]})
            del img
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 2560])
    ap.add_argument("--sources", type=int, nargs="+", default=[256, 384])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    text = []

    def emit(x):
        ln = x if isinstance(x, str) else json.dumps(x)
        text.append(ln)
        print(ln, flush=True)
    emit(f"# bench/randaug.py on {torch.cuda.get_device_name(0)}; N = 2, M = 9, boxes of the default --rrc ranges")
    kernel_rows(a.batches, a.sources, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
