"""The three loss-head kernels alone, with and without label smoothing: softmax_xent (bf16
dlogits), softmax_xent_f32 and eval_metrics on [B][1000] fp32 logits, in microseconds per launch.

    python bench/loss_head.py [--batches 32 256 1024 2560] [--smoothing 0 0.1] [--json out.json]

The method of bench/eval.py: device events around 2000 back-to-back launches, three such windows,
their median; the three windows are printed too, since their spread is what a difference between
two builds has to exceed.  eps = 0 is called without the argument, so the same script times a
build from before the option existed (--smoothing 0).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import pddl  # noqa: E402,F401
from pddl.ops.native import require_native  # noqa: E402

ITERS = 2000


def timeit(fn, iters=ITERS):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 256, 1024, 2560])
    ap.add_argument("--smoothing", type=float, nargs="+", default=[0.0, 0.1])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    N = require_native()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows = []
    for B in a.batches:
        g = torch.Generator(device=dev).manual_seed(B)
        logits = torch.randn(B, 1000, device=dev, generator=g) * 3
        lab = torch.randint(0, 1000, (B,), device=dev, generator=g)
        dl16 = torch.empty(B, 1024, dtype=torch.bfloat16, device=dev)
        dl32 = torch.empty(B, 1000, device=dev)
        out = torch.zeros(3, device=dev)
        for eps in a.smoothing:
            kw = {"smoothing": eps} if eps else {}
            calls = {
                "softmax_xent": lambda: N.softmax_xent(logits, lab, 1000, 1.0 / B, dl16, out[0:1], out[1:2], **kw),
                "softmax_xent_f32": lambda: N.softmax_xent_f32(logits, lab, 1000, 1.0 / B, dl32, out[0:1], out[1:2],
                                                               **kw),
                "eval_metrics": lambda: N.eval_metrics(logits, lab, 1000, 5, out, **kw),
            }
            for name, fn in calls.items():
                w = [timeit(fn) for _ in range(3)]
                row = {"kernel": name, "batch": B, "smoothing": eps, "us": round(statistics.median(w), 2),
                       "windows_us": [round(x, 2) for x in w]}
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
