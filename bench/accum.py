"""Gradient accumulation (--accum-steps): the three modes of the streaming kernel on the full
parameter buffer, and a batch-256 training step at K = 1 against K = 4, per image.

Kernel: store (acc = g), add (acc += g), fold (g += acc) over ParamLayout().total floats, µs per
call and GB/s of the bytes the mode requests (store: 1 read + 1 write, add / fold: 2 reads +
1 write).  Timed twice: "hot" re-runs one buffer pair (2 x 102 MB stay in the 256 MB memory-side
cache), "cold" rotates through enough pairs that every call streams from HBM, as it does inside
a training step, where a whole forward + backward runs between two calls.

Step: SingleStrategy.train_step on synthetic images (eager launches, the bench preset's Adam),
interleaved repeats of K = 1 and K = 4; a K = 4 run makes a quarter of the updates and one
accumulation pass per micro-step.

    python bench/accum.py [--iters 50] [--repeats 5] [--steps 40] [--batch 256] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import pddl  # noqa: E402,F401
from pddl.models.resnet50 import ParamLayout  # noqa: E402
from pddl.ops.native import require_native  # noqa: E402

MODES = (("store", 0, 2), ("add", 1, 3), ("fold", 2, 3))   # name, mode, floats moved per element


def timeit(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000 / iters


def kernel_bench(a, res):
    N = require_native()
    n = ParamLayout().total
    res["n"] = n
    pairs = [(torch.zeros(n, device="cuda"), torch.full((n,), 1e-30, device="cuda")) for _ in range(a.pairs)]
    for name, mode, moved in MODES:
        for kind, use in (("hot", pairs[:1]), ("cold", pairs)):
            it = [0]

            def call():
                acc, g = use[it[0] % len(use)]
                it[0] += 1
                N.grad_accum(acc, g, mode)

            us = statistics.median(timeit(call, a.iters) for _ in range(a.repeats))
            res[f"{name}_{kind}_us"] = round(us, 1)
            res[f"{name}_{kind}_GBps"] = round(moved * 4 * n / us / 1e3)
    del pairs
    torch.cuda.empty_cache()


def step_bench(a, res):
    from pddl.config import make_config
    from pddl.parallel.strategies import make_strategy
    from pddl.train.trainer import Trainer
    B = a.batch
    g = torch.Generator(device="cuda").manual_seed(0)
    img = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, device="cuda", generator=g)
    lab = torch.randint(0, 1000, (B,), device="cuda", generator=g)
    sts = {}
    for K in (1, 4):
        cfg = make_config("bench", strategy="single", batch_size=B, crop=224, device="cuda", graphs=False,
                          accum_steps=K, lr=1e-6)
        sts[K] = make_strategy(cfg)
        Trainer(cfg, sts[K])
    steps = a.steps - a.steps % 4

    def run(K):
        st = sts[K]
        return timeit(lambda: st.train_step(img, lab), steps) / B     # µs per image

    for K in (1, 4):
        run(K)                                                         # warm-up: lazy tables, code objects
    t = {1: [], 4: []}
    for _ in range(a.repeats):
        for K in (1, 4):
            t[K].append(run(K))
    for K in (1, 4):
        res[f"k{K}_us_per_image"] = round(statistics.median(t[K]), 3)
        res[f"k{K}_us_per_image_all"] = [round(x, 3) for x in t[K]]
        res[f"k{K}_img_per_s"] = round(1e6 / statistics.median(t[K]), 1)
    res["step_batch"] = B
    res["k4_over_k1"] = round(res["k4_us_per_image"] / res["k1_us_per_image"], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=6, help="buffer pairs the cold timing rotates through")
    ap.add_argument("--steps", type=int, default=40, help="training steps per timed window (rounded down to a multiple of 4)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-step", action="store_true", help="kernel timings only")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = {}
    kernel_bench(a, res)
    if not a.no_step:
        step_bench(a, res)
    print(json.dumps(res), flush=True)
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
