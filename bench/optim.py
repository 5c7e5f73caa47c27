"""Fused optimizer steps over the flat parameter buffer (ParamLayout().n_trainable floats): adam,
sgd and lars as the training step launches them (the one-thread hparams kernel + the update;
lars: + the norm pass), µs per step and achieved GB/s.  adam and lars move the same bytes
(adam: p, g, m, v read, p, m, v written; lars: p, g read, then p, g, v read and p, v written).
With --clip C every optimizer is also timed with global-norm clipping at C (`*_clip_us`: the norm
pass + the update reading the device scale) and the norm pass alone (`grad_norm_us`, GB/s over
the 4 n bytes it reads).

    python bench/optim.py [--iters 50] [--chunk 16384] [--clip 1.0] [--json out.json]
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
from pddl.train.optim import LARS, make_optimizer  # noqa: E402

FLOATS_MOVED = {"adam": 7, "sgd": 5, "lars": 7}   # per parameter, reads + writes


class FlatEngine:
    def __init__(self, L, dev):
        self.L = L
        self.params = torch.randn(L.total, device=dev) * 0.05
        self.grads = torch.randn(L.n_trainable, device=dev) * 1e-2


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=None, help="lars: floats per block (default: the kernel's)")
    ap.add_argument("--clip", type=float, default=None, help="also time every optimizer with --global-clipnorm C")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    L = ParamLayout()
    eng = FlatEngine(L, "cuda")
    n = L.n_trainable
    res = {"n": n}
    for name in ("adam", "sgd", "lars"):
        # a tiny rate: hundreds of timed steps must not blow the parameters up
        if name == "lars":
            opt = LARS(eng, lr=1e-6, momentum=0.9, weight_decay=5e-5, chunk=a.chunk)
            res["lars_chunk"] = opt.chunk
        else:
            opt = make_optimizer(name, eng, lr=1e-6)
        runs = sorted(timeit(opt.step, a.iters) for _ in range(a.repeats))
        us = statistics.median(runs)
        res[f"{name}_us"] = round(us, 1)
        res[f"{name}_us_range"] = [round(runs[0], 1), round(runs[-1], 1)]
        res[f"{name}_GBps"] = round(FLOATS_MOVED[name] * 4 * n / us / 1e3)
        if a.clip is not None:
            opt.set_grad_clip(a.clip)
            runs = sorted(timeit(opt.step, a.iters) for _ in range(a.repeats))
            res[f"{name}_clip_us"] = round(statistics.median(runs), 1)
            res[f"{name}_clip_us_range"] = [round(runs[0], 1), round(runs[-1], 1)]
            res[f"{name}_clip_extra_us"] = round(res[f"{name}_clip_us"] - res[f"{name}_us"], 1)
            st = opt.clip_stats()
            res[f"{name}_clip_scale"] = round(st["scale"], 6)
            if name == "adam":     # the norm pass alone: grad_sqsum_kernel + the one-block fold
                from pddl.ops.native import require_native
                nat = require_native()
                fn = lambda: nat.grad_norm(eng.grads, 1.0, opt.gn_chunk, opt.gn_partials, opt.gn)  # noqa: E731
                runs = sorted(timeit(fn, a.iters) for _ in range(a.repeats))
                us = statistics.median(runs)
                res["clip"], res["grad_norm"], res["grad_norm_chunk"] = a.clip, round(st["norm"], 4), opt.gn_chunk
                res["grad_norm_us"] = round(us, 1)
                res["grad_norm_us_range"] = [round(runs[0], 1), round(runs[-1], 1)]
                res["grad_norm_GBps"] = round(4 * n / us / 1e3)
        del opt
    res["lars_over_adam"] = round(res["lars_us"] / res["adam_us"], 3)
    print(json.dumps(res), flush=True)
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
