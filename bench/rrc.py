"""Random-resized-crop: what the per-image resampling costs the stem preprocess kernel and a whole
training step.

    python bench/rrc.py [--batches 256 2560] [--out profiles/rrc.txt]

The method of bench/mix.py (device events around back-to-back launches after a warm-up, three
windows per case, their median, the windows printed).  Per batch and source size (224 -> 224 and
256 -> 224, uint8 in, bf16 out), with and without a mixup table: the unaugmented stem_s2d launch
(the row form: identity, or RandomCrop at one offset), the band form of mode 3 on boxes drawn by
train/rrc.py with the default ranges, and its per-pixel twin.  GB/s counts the bytes a launch must
move: the boxes' pixels (the partner's too under a table) and the s2d image written; next to the
6.29 TB/s measured HBM peak.  Then one batch-256 HipEngine step with and without a box table.

    python bench/rrc.py --antialias [--out profiles/rrc_antialias.txt]

The rows of --antialias instead: 512 -> 224 and 384 -> 224 with boxes drawn from the whole source, the
band and the per-pixel antialias forms and mode 3 (no antialias) on the same input, with and without
a mixup table; then a batch-256 step at 448 -> 224 with and without the flag."""
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
from mix import HBM_PEAK, windows  # noqa: E402
from pddl.ops.native import require_native  # noqa: E402
from pddl.train.mix import mixup_table  # noqa: E402
from pddl.train.rrc import RrcSampler  # noqa: E402

CROP = 224


def kernel_rows(batches, emit):
    N = require_native()
    N.allow_knob_changes(True)       # (the per-pixel twin is the same launch under set_variant("stem", 0))
    dev = torch.device("cuda", 0)
    hs = (CROP + 6) // 2
    for B in batches:
        mix = torch.from_numpy(mixup_table(np.random.default_rng(B).permutation(B), 0.7)).to(dev)
        x2 = torch.empty(B, hs, hs, 16, dtype=torch.bfloat16, device=dev)
        for S in (224, 256):
            g = torch.Generator(device=dev).manual_seed(S)
            img = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device=dev, generator=g)
            flip = torch.randint(0, 2, (B,), dtype=torch.uint8, device=dev, generator=g)
            t = RrcSampler(True, (0.08, 1.0), (3 / 4, 4 / 3), S, S, 0).draw(B)
            rrc = torch.from_numpy(t).to(dev)
            area = int((t[:, 2].astype(np.int64) * t[:, 3]).sum())
            mode, off = (0, (0, 0)) if S == CROP else (2, (7, 13))
            for mixed in (False, True):
                kw = {"mix": mix} if mixed else {}
                sides = 2 if mixed else 1
                plain = B * CROP * CROP * 3 * sides + x2.numel() * 2
                boxed = area * 3 * sides + x2.numel() * 2
                cases = [("rows (no rrc)", 1, {}, plain), ("rrc band", 1, {"rrc": rrc}, boxed), ("rrc pixel", 0, {"rrc": rrc}, boxed)]
                for name, variant, rk, nbytes in cases:
                    N.set_variant("stem", variant)
                    fn = (lambda: N.stem_s2d(img, flip, mode, CROP, CROP, off[0], off[1], x2, None, **kw, **rk))
                    med, w = windows(fn, 100 if B > 1000 else 400)
                    form, band = N.stem_last_launch()
                    N.set_variant("stem", 1)
                    emit({"case": f"stem_s2d {S}->{CROP} {name} mix={'mixup' if mixed else 'none'}", "batch": B, "form": form,
                          "band": band, "us": round(med, 2), "windows_us": [round(x, 2) for x in w],
                          "GBps": round(nbytes / med / 1e3, 1), "of_peak": round(nbytes / (med * 1e-6) / HBM_PEAK, 3)})
            del img
            torch.cuda.empty_cache()


def antialias_rows(batches, emit):
    N = require_native()
    N.allow_knob_changes(True)
    dev = torch.device("cuda", 0)
    hs = (CROP + 6) // 2
    for B in batches:
        mix = torch.from_numpy(mixup_table(np.random.default_rng(B).permutation(B), 0.7)).to(dev)
        x2 = torch.empty(B, hs, hs, 16, dtype=torch.bfloat16, device=dev)
        for S in (512, 384):
            g = torch.Generator(device=dev).manual_seed(S)
            img = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device=dev, generator=g)
            flip = torch.randint(0, 2, (B,), dtype=torch.uint8, device=dev, generator=g)
            t = RrcSampler(True, (0.08, 1.0), (3 / 4, 4 / 3), S, S, 0).draw(B)
            rrc = torch.from_numpy(t).to(dev)
            area = int((t[:, 2].astype(np.int64) * t[:, 3]).sum())
            for mixed in (False, True):
                kw = {"mix": mix} if mixed else {}
                nbytes = area * 3 * (2 if mixed else 1) + x2.numel() * 2     # every box pixel once, the image written
                for name, variant, aa in (("antialias band", 1, True), ("antialias pixel", 0, True), ("mode 3 band", 1, False)):
                    N.set_variant("stem", variant)
                    fn = (lambda: N.stem_s2d(img, flip, 0, CROP, CROP, 0, 0, x2, None, **kw, rrc=rrc, antialias=aa))
                    med, w = windows(fn, 20 if variant == 0 else 100 if B > 1000 else 400)
                    form, band = N.stem_last_launch()
                    N.set_variant("stem", 1)
                    emit({"case": f"stem_s2d {S}->{CROP} {name} mix={'mixup' if mixed else 'none'}", "batch": B, "form": form,
                          "band": band, "us": round(med, 2), "windows_us": [round(x, 2) for x in w],
                          "GBps": round(nbytes / med / 1e3, 1), "of_peak": round(nbytes / (med * 1e-6) / HBM_PEAK, 3)})
            del img
            torch.cuda.empty_cache()


def step_rows(emit, S=256, antialias=(False,)):
    """One batch-256 HipEngine training step (forward, backward, Adam, re-prep), eager, 256 -> 224:
    RandomCrop at one offset against a box table, alternated."""
    from pddl.models.engine import HipEngine
    from pddl.models.resnet50 import ParamLayout
    from pddl.train.optim import make_optimizer
    B = 256
    dev = torch.device("cuda", 0)
    img = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device=dev)
    lab = torch.randint(0, 1000, (B,), device=dev)
    flip = torch.randint(0, 2, (B,), dtype=torch.uint8, device=dev)
    rrc = torch.from_numpy(RrcSampler(True, (0.08, 1.0), (3 / 4, 4 / 3), S, S, 1).draw(B)).to(dev)
    engines = {}            # one engine per antialias value, alternated between the cases
    for aa in antialias:
        engines[aa] = eng = HipEngine(ParamLayout(), B, crop=CROP, image_size=S, antialias=aa)
        eng.init(seed=0)
        engines[aa] = (eng, make_optimizer("adam", eng, lr=1e-3))
    cases = [("none", False, {"crop_offset": (7, 13)})] if len(antialias) == 1 else []
    for kind, aa, kw in (cases + [("rrc" + (" antialias" if aa else ""), aa, {"rrc": rrc}) for aa in antialias]) * 2:
        eng, opt = engines[aa]

        def step():
            eng.forward_backward(img, lab, 1.0 / B, flip=flip, **kw)
            opt.step()
            eng.after_update()
        med, w = windows(step, 20)
        emit({"case": f"HipEngine step {S}->{CROP} rrc={kind}", "batch": B, "us": round(med, 1),
              "windows_us": [round(x, 1) for x in w], "img_per_s": round(B / med * 1e6)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 2560])
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--antialias", action="store_true", help="the antialias rows (large sources) instead")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    text = []

    def emit(x):
        ln = x if isinstance(x, str) else json.dumps(x)
        text.append(ln)
        print(ln, flush=True)
    emit(f"# bench/rrc.py on {torch.cuda.get_device_name(0)}; HBM peak taken as {HBM_PEAK / 1e12:.2f} TB/s")
    if a.antialias:
        antialias_rows(a.batches, emit)
    else:
        kernel_rows(a.batches, emit)
    if not a.no_step:
        step_rows(emit, *((448, (False, True)) if a.antialias else ()))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
