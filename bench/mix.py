"""Mixup / CutMix: what the table costs the stem preprocess kernels, the two training heads and a
whole training step, and whether the unmixed kernels kept their speed.

    python bench/mix.py [--batches 256 2560] [--out profiles/mixup.txt]
    python bench/mix.py --ab DIR        # + the unmixed kernels of the build in DIR against this build

Device events around back-to-back launches after a warm-up, three such windows per case, their
median (the method of bench/loss_head.py); the windows' spread is printed, since it is what a
difference has to exceed.  Per case: microseconds and GB/s against the bytes the kernel must move
(the mixed stem reads 2 B Hc Wc 3 and writes B Hs Ws 32; a head reads its logits once and writes
its dlogits), next to the 6.29 TB/s measured HBM peak.  uint8 input, crop 224 from 224 (identity)
and from 244 (crop), the bf16 row form and the fp32 form; then one batch-256 HipEngine step with
and without a mixup table.

--ab DIR: child processes, alternately loading the extensions of DIR (PDDL_NATIVE_DIR: a build of
the parent commit) and this tree's, time the UNMIXED stem_s2d and softmax_xent launches; both
builds' medians per round and the run-to-run spread are reported."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import pddl  # noqa: E402,F401
from pddl.ops.native import require_native  # noqa: E402

HBM_PEAK = 6.29e12
CROP = 224


def timeit(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000 / iters


def windows(fn, iters):
    w = [timeit(fn, iters) for _ in range(3)]
    return statistics.median(w), w


def _table(B, kind, dev):
    from pddl.train.mix import cutmix_box, cutmix_table, identity_table, mixup_table
    import numpy as np
    p = np.random.default_rng(B).permutation(B)
    if kind == "mixup":
        t = mixup_table(p, 0.7)
    elif kind == "cutmix":
        y0, x0, y1, x1, w = cutmix_box(CROP, CROP, 0.6, 100, 120)
        t = cutmix_table(p, (y0, x0, y1, x1), w)
    else:
        t = identity_table(B)
    return torch.from_numpy(t).to(dev)


def stem_cases(N, B, dev, kinds):
    """(name, launch, bytes) of the stem kernels at batch B."""
    hs = (CROP + 6) // 2
    out = []
    for S in (224, 244):
        g = torch.Generator(device=dev).manual_seed(S)
        img = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device=dev, generator=g)
        flip = torch.randint(0, 2, (B,), dtype=torch.uint8, device=dev, generator=g)
        mode, off = (0, (0, 0)) if S == CROP else (2, (7, 13))
        for dtype, form in ((torch.bfloat16, "bf16 rows"), (torch.float32, "fp32")):
            x2 = torch.empty(B, hs, hs, 16, dtype=dtype, device=dev)
            wr = x2.numel() * x2.element_size()
            for kind in kinds:
                kw = {} if kind == "none" else {"mix": _table(B, kind, dev)}
                rd = B * CROP * CROP * 3 * (1 if kind == "none" else 2)
                out.append((f"stem_s2d {form} {S}->{CROP} mix={kind}",
                            (lambda img=img, flip=flip, mode=mode, off=off, x2=x2, kw=kw:
                             N.stem_s2d(img, flip, mode, CROP, CROP, off[0], off[1], x2, None, **kw)), rd + wr))
    return out


def head_cases(N, B, dev, kinds):
    g = torch.Generator(device=dev).manual_seed(B)
    logits = torch.randn(B, 1000, device=dev, generator=g) * 3
    lab = torch.randint(0, 1000, (B,), device=dev, generator=g)
    dl16 = torch.empty(B, 1024, dtype=torch.bfloat16, device=dev)
    dl32 = torch.empty(B, 1000, device=dev)
    st = torch.zeros(2, device=dev)
    out = []
    for name, dl in (("softmax_xent", dl16), ("softmax_xent_f32", dl32)):
        fn = getattr(N, name)
        for kind in kinds:
            kw = {} if kind == "none" else {"mix": _table(B, kind, dev)}
            nbytes = logits.numel() * 4 + dl.numel() * dl.element_size()
            out.append((f"{name} mix={kind}",
                        (lambda fn=fn, dl=dl, kw=kw: fn(logits, lab, 1000, 1.0 / B, dl, st[0:1], st[1:2], **kw)), nbytes))
    return out


def iters_for(name, B):
    if name.startswith("stem"):
        return 100 if B > 1000 else 400
    return 2000


def run_kernels(batches, kinds, emit):
    N = require_native()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows = []
    for B in batches:
        for make in (stem_cases, head_cases):
            for name, fn, nbytes in make(N, B, dev, kinds):
                med, w = windows(fn, iters_for(name, B))
                row = {"case": name, "batch": B, "us": round(med, 2), "windows_us": [round(x, 2) for x in w],
                       "GBps": round(nbytes / med / 1e3, 1), "of_peak": round(nbytes / (med * 1e-6) / HBM_PEAK, 3)}
                rows.append(row)
                emit(row)
            torch.cuda.empty_cache()
    return rows


def run_step(emit):
    """One batch-256 HipEngine training step (forward, backward, Adam, re-prep), eager, with and
    without a mixup table (lambda 0.2 of the own image: every pixel blended)."""
    from pddl.models.engine import HipEngine
    from pddl.models.resnet50 import ParamLayout
    from pddl.train.mix import mixup_table
    from pddl.train.optim import make_optimizer
    import numpy as np
    B = 256
    dev = torch.device("cuda", 0)
    eng = HipEngine(ParamLayout(), B, crop=CROP, image_size=CROP)
    eng.init(seed=0)
    opt = make_optimizer("adam", eng, lr=1e-3)
    img = torch.randint(0, 256, (B, CROP, CROP, 3), dtype=torch.uint8, device=dev)
    lab = torch.randint(0, 1000, (B,), device=dev)
    flip = torch.randint(0, 2, (B,), dtype=torch.uint8, device=dev)
    tab = torch.from_numpy(mixup_table(np.random.default_rng(1).permutation(B), 0.2)).to(dev)
    rows = []
    for kind, kw in (("none", {}), ("mixup", {"mix": tab}), ("none", {}), ("mixup", {"mix": tab})):
        def step():
            eng.forward_backward(img, lab, 1.0 / B, flip=flip, **kw)
            opt.step()
            eng.after_update()
        med, w = windows(step, 20)
        row = {"case": f"HipEngine step mix={kind}", "batch": B, "us": round(med, 1),
               "windows_us": [round(x, 1) for x in w], "img_per_s": round(B / med * 1e6)}
        rows.append(row)
        emit(row)
    return rows


def run_ab(parent_dir, batches, rounds, emit):
    """Alternate child processes on the two builds; each times the unmixed kernels only."""
    res = {"parent": [], "new": []}
    for r in range(rounds):
        for which in ("parent", "new"):
            env = dict(os.environ)
            env.pop("PDDL_NATIVE_DIR", None)
            if which == "parent":
                env["PDDL_NATIVE_DIR"] = os.path.abspath(parent_dir)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--batches"] + [str(b) for b in batches]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"{which} child failed:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            rows = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
            res[which].append({(x["case"], x["batch"]): x for x in rows})
    lines = [f"unmixed kernels, the parent commit's build against this build, {rounds} alternating rounds "
             "(median us of 3 windows per round)"]
    ok = True
    for key in res["new"][0]:
        pa = [r[key]["us"] for r in res["parent"]]
        ne = [r[key]["us"] for r in res["new"]]
        allw = [w for r in res["parent"] for w in r[key]["windows_us"]]
        spread = max(allw) - min(allw)
        # inside: not above the parent's slowest window, or no further from the parent's median than
        # the parent's own windows lie apart (times are kept to 0.01 us)
        d = statistics.median(ne) - statistics.median(pa)
        inside = statistics.median(ne) <= max(allw) + 1e-9 or d <= max(spread, 0.01) + 1e-9
        ok = ok and inside
        lines.append(f"  {key[0]:<42} b{key[1]:<5} parent {pa}  new {ne}  parent windows {min(allw):.2f}..{max(allw):.2f} "
                     f"(spread {spread:.2f})  new - parent medians {d:+.2f}  {'inside' if inside else 'OUTSIDE'} the spread")
    lines.append("all unmixed kernels inside the parent's run-to-run spread" if ok
                 else "SOME unmixed kernel is slower than the parent's run-to-run spread")
    for ln in lines:
        emit(ln)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 2560])
    ap.add_argument("--ab", default=None, help="directory with the parent commit's extensions")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:      # unmixed kernels only, no mix argument: runs on a build from before the option
        run_kernels(a.batches, ("none",), lambda row: print(json.dumps(row), flush=True))
        return
    text = []

    def emit(x):
        ln = x if isinstance(x, str) else json.dumps(x)
        text.append(ln)
        print(ln, flush=True)
    emit(f"# bench/mix.py on {torch.cuda.get_device_name(0)}; HBM peak taken as {HBM_PEAK / 1e12:.2f} TB/s")
    emit("# GBps / of_peak of a stem row with a table count the bytes of a fully mixed batch (2 B Hc Wc 3 read), not the "
         "bytes moved: the identity and CutMix tables skip most partner loads, so their figures overstate the traffic")
    run_kernels(a.batches, ("none", "identity", "mixup", "cutmix"), emit)
    if not a.no_step:
        run_step(emit)
    if a.ab:
        run_ab(a.ab, a.batches, a.rounds, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
