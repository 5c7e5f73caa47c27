"""Inference throughput: images/s of engine.evaluate_topk (forward + the eval_metrics head), and
the head alone -- eval_metrics against softmax_xent (which also writes the [B][1024] bf16
dlogits an evaluation discards) at the same B, in microseconds.

    python bench/eval.py [--batch 256] [--precision bf16|fp32] [--bn-mode frozen|train] [--crop 224] [--json out.json]
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


def timeit(fn, iters=20):
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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--precision", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--bn-mode", choices=["frozen", "train"], default="frozen", dest="bn_mode")
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from pddl.config import make_config
    from pddl.parallel.strategies import build_engine
    N = require_native()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B = a.batch
    cfg = make_config("bench", batch_size=B, crop=a.crop, image_size=a.crop, precision=a.precision, bn_mode=a.bn_mode)
    eng = build_engine(cfg, dev, B, graphed=False)
    eng.init(seed=0)
    img = torch.randint(0, 256, (B, a.crop, a.crop, 3), dtype=torch.uint8, device=dev)
    lab = torch.randint(0, 1000, (B,), device=dev)
    row = {"batch": B, "precision": a.precision, "bn_mode": a.bn_mode, "crop": a.crop}
    us = statistics.median(timeit(lambda: eng.evaluate_topk(img, lab), a.iters) for _ in range(3))
    row["evaluate_topk_ms"] = round(us / 1e3, 3)
    row["evaluate_topk_img_per_s"] = round(B / us * 1e6, 1)
    us = statistics.median(timeit(lambda: eng.evaluate(img, lab), a.iters) for _ in range(3))
    row["evaluate_ms"] = round(us / 1e3, 3)
    row["evaluate_img_per_s"] = round(B / us * 1e6, 1)
    # the head alone (back-to-back launches: the launch rate bounds both from below)
    logits = torch.randn(B, 1000, device=dev) * 3
    dl = torch.empty(B, 1024, dtype=torch.bfloat16, device=dev)
    out = torch.zeros(3, device=dev)
    row["eval_metrics_us"] = round(statistics.median(
        timeit(lambda: N.eval_metrics(logits, lab, 1000, 5, out), 2000) for _ in range(3)), 2)
    row["softmax_xent_us"] = round(statistics.median(
        timeit(lambda: N.softmax_xent(logits, lab, 1000, 0.0, dl, out[0:1], out[1:2]), 2000) for _ in range(3)), 2)
    print(json.dumps(row), flush=True)
    if a.json:
        json.dump(row, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
