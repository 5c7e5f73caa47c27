"""LAMB (`make_optimizer("adam", ..., layer_adapt=True)`) on the GPU: the two-pass segmented kernel
against float64, skip / clip, bitwise reproducibility, graph capture and the engine-level step.
The float64 references take the hyper-parameters rounded to fp32 first (see test_gpu_lars.py)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS, WD, GS, CHUNK, PAD = 1e-3, 0.9, 0.999, 1e-6, 0.01, 0.5, 1024, 60
# the boundary segments of test_gpu_lars.py; PAD sentinel floats follow them and belong to no segment
SIZES = [(4, 1), (252, 1), (1024, 1), (1028, 1), (3 * 1024, 1), (65 * 1024 + 12, 1), (1000, 0)]


def N():
    from pddl.ops.native import require_native
    return require_native()


def f32(x):
    return float(np.float32(x))


def _segments(sizes):
    offs = np.cumsum([0] + [s for s, _ in sizes]).tolist()
    return [(o, s, a) for o, (s, a) in zip(offs, sizes)], offs[-1]


def _inputs(n, seed):
    """p, g ~ N(0, 1), m ~ 0.5 N(0, 1), v = (0.5 N(0, 1))^2 + 1e-2, so |m / c1| < 32 over sqrt(v / c2) > 3.1 at
    t = 1 and |m| < 4 over sqrt(v / c2) > 0.12 at t = 1000: |u| < 32 at both."""
    r = torch.Generator().manual_seed(seed)
    p, g, m, v = (torch.randn(n, generator=r) for _ in range(4))
    return p, g, 0.5 * m, (0.5 * v) ** 2 + 1e-2


def _reference(segs, p, g, m, v, t, gs=GS, wd=WD):
    """float64 LAMB over (offset, size, adapt) segments -> (p, m, v, ratios)."""
    p, g, m, v = (x.double().numpy().copy() for x in (p, g, m, v))
    lr, b1, b2, eps, wd, gs = (f32(x) for x in (LR, B1, B2, EPS, wd, gs))
    ratios = []
    for off, size, adapt in segs:
        sl = slice(off, off + size)
        gg = gs * g[sl]
        m[sl] = b1 * m[sl] + (1 - b1) * gg
        v[sl] = b2 * v[sl] + (1 - b2) * gg * gg
        u = (m[sl] / (1 - b1 ** t)) / (np.sqrt(v[sl] / (1 - b2 ** t)) + eps) + (wd * p[sl] if adapt else 0.0)
        wn, un = math.sqrt((p[sl] ** 2).sum()), math.sqrt((u * u).sum())
        ratios.append(wn / un if adapt and wn > 0 and un > 0 else 1.0)
        p[sl] -= lr * ratios[-1] * u
    return p, m, v, np.array(ratios)


def _run(segs, p, g, m, v, t, hs=False, gn=None, wd=WD, chunk=CHUNK):
    """The two launches on the current stream -> (p, m, v, ratios) device tensors.  With hs the step count and
    the rate come from the device buffer and the launch arguments carry t = 0 and a NaN rate."""
    from pddl.train.optim import lars_chunks, lars_table
    th = lars_table(segs, chunk)
    p, g, m, v = (x.cuda() for x in (p, g, m, v))
    partials = torch.full((2 * lars_chunks(th, chunk),), float("nan"), device="cuda")
    ratios = torch.full((len(segs),), float("nan"), device="cuda")
    hsd = torch.tensor([t, 0.0, LR], device="cuda") if hs else None
    lr, t = (float("nan"), 0) if hs else (LR, t)
    N().lamb(p, g, m, v, th.cuda(), th, chunk, partials, ratios, lr, t, B1, B2, EPS, wd, GS, hsd, gn)
    return p, m, v, ratios


def _check(end, got, ref):
    """m, v to atol 1e-6: |m| < 4 and |v| < 8 here and each is one fma of a rounded product, every rounding at
    most half an ulp of 8 = 2.4e-7.  Ratios to rtol 1e-5: the bound of test_gpu_lars.py for the same tree (sums
    of non-negative terms within ~20 ulp, halved by the root), plus u's own relative error of at most 8 roundings
    = 4.8e-7.  p to atol 1e-6: |p| < 8, so the last fma rounds by at most 2.4e-7; before it, step = lr ratio
    < 4e-3 (ratios are below 4 here) multiplies u's error of 8 x 2^-24 x 32 = 1.5e-5 (6e-8) and the ratio's
    error, in fact below 2e-6 relative, times |u| < 32 (2.6e-7)."""
    for x, x64 in zip(got[:3], ref[:3]):
        assert np.abs(x.cpu().double().numpy()[:end] - x64[:end]).max() <= 1e-6
    assert np.allclose(got[3].cpu().double().numpy(), ref[3], rtol=1e-5, atol=0), (got[3].tolist(), ref[3].tolist())


@pytest.mark.parametrize("hs", [False, True])
@pytest.mark.parametrize("t", [1, 1000])        # the largest bias correction; a steady-state one
def test_kernel_matches_float64_at_every_boundary(t, hs):
    segs, end = _segments(SIZES)
    x0 = _inputs(end + PAD, 7)
    got = _run(segs, *x0, t, hs)
    # (the reference gives the non-adapted segment no decay: lr wd |w| ~ 1e-5 of decay would miss the bound)
    _check(end, got, _reference(segs, *x0, t))
    for x, y in zip(got[:3], (x0[0], x0[2], x0[3])):
        assert torch.equal(x[end:].cpu(), y[end:])                      # the padding is bit-unchanged
    r = got[3].tolist()
    assert r[-1] == 1.0 and all(x != 1.0 and x < 4 for x in r[:-1])


@pytest.mark.parametrize("case,wd", [("zero_w", WD), ("zero_u", 0.0), ("decay_only", WD)])
def test_degenerate_segments(case, wd):
    segs, end = _segments([(2048, 1), (512, 1)])
    p0, g0, m0, v0 = _inputs(end, 3)
    if case == "zero_w":
        p0[:2048] = 0
    else:
        g0[:2048] = 0
        m0[:2048] = 0
    got = _run(segs, p0, g0, m0, v0, 2, wd=wd)
    assert all(torch.isfinite(x).all() for x in got)
    _check(end, got, _reference(segs, p0, g0, m0, v0, 2, wd=wd))
    if case == "decay_only":                                            # u = wd w: ratio 1 / wd
        assert got[3][0].item() == pytest.approx(1 / f32(wd), rel=1e-5)
    else:
        assert got[3][0].item() == 1.0 and (case == "zero_w" or torch.equal(got[0][:2048].cpu(), p0[:2048]))


def test_skip_touches_nothing_and_clip_scales_the_gradient():
    segs, end = _segments(SIZES)
    x0 = _inputs(end, 9)
    got = _run(segs, *x0, 5, gn=torch.tensor([3.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0], device="cuda"))
    for x, y in zip(got[:3], (x0[0], x0[2], x0[3])):
        assert torch.equal(x.cpu(), y)
    assert torch.isnan(got[3]).all()                                    # the NaN fill of _run: never written
    got = _run(segs, *x0, 5, gn=torch.tensor([3.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], device="cuda"))
    x1 = (x0[0], 0.5 * x0[1], x0[2], x0[3])                             # gs * 0.5, exact in fp32
    _check(end, got, _reference(segs, *x1, 5))


def test_bitwise_reproducible_across_runs_and_streams():
    segs, end = _segments([(2359296, 1), (65 * 1024 + 12, 1)])          # conv5-sized: 2304 + 66 partials
    x0 = _inputs(end, 13)
    a, b = _run(segs, *x0, 3), _run(segs, *x0, 3)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        c = _run(segs, *x0, 3)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))


class _FlatEngine:
    """The flat buffers an optimizer needs, with the real layout."""

    def __init__(self, seed):
        from pddl.models.resnet50 import ParamLayout
        self.L = ParamLayout()
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.params = torch.randn(self.L.total, device="cuda", generator=g) * 0.05
        self.grads = torch.randn(self.L.n_trainable, device="cuda", generator=g) * 1e-2


def test_captured_step_replays_like_eager_steps():
    from pddl.train.optim import make_optimizer
    (ea, oa), (eb, ob) = ((e, make_optimizer("adam", e, lr=LR, layer_adapt=True, weight_decay=WD))
                          for e in (_FlatEngine(5), _FlatEngine(5)))
    assert type(oa).__name__ == "LAMB" and len(oa.trust_ratios()) == 54
    for _ in range(4):
        oa.step()
    ob.sync_hparams()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ob.step()
    ob._iterations = 0          # the capture ran no kernels
    for _ in range(4):
        ob.sync_hparams()
        g.replay()
        ob._iterations += 1
    torch.cuda.synchronize()
    for x, y in ((ea.params, eb.params), (oa.m, ob.m), (oa.v, ob.v), (oa.ratios, ob.ratios), (oa.hs, ob.hs)):
        assert torch.equal(x, y)
    end = max(x.offset + x.size for x in ea.L.entries.values() if x.trainable)
    assert ob.hs[0].item() == 4 and ob.m[:end].abs().max() > 0 and (ob.m[end:] == 0).all()   # padding never written


def _strategy(mirrored, monkeypatch):
    from pddl.config import make_config
    from pddl.parallel.strategies import MirroredStrategy, make_strategy
    from pddl.train.trainer import Trainer
    if mirrored:
        monkeypatch.setenv("PDDL_REHEARSE", "1")
    cfg = make_config("bench", strategy="mirrored" if mirrored else "single", batch_size=4, crop=32, image_size=32,
                      optimizer="adam", layer_adapt=True, lr=LR, weight_decay=WD, device="cuda", graphs=False,
                      flip=False, data="synthetic_fixed", seed=0, num_classes=1000)
    st = MirroredStrategy(cfg, devices=[0, 0]) if mirrored else make_strategy(cfg)
    Trainer(cfg, st)
    return st


@pytest.mark.parametrize("replicas", [1, 2])
def test_engine_level_steps(replicas, monkeypatch):
    """Three train_steps through the strategy; two rehearsal replicas on the same data end bit-identical."""
    st = _strategy(replicas == 2, monkeypatch)
    if replicas == 2:
        st.broadcast_state(None)
    pairs = st.mirror.replicas if replicas == 2 else [(st.engine, st.opt)]
    start = pairs[0][0].params.clone()
    g = torch.Generator().manual_seed(99)
    img = torch.randint(0, 256, (4, 32, 32, 3), dtype=torch.uint8, generator=g).cuda().repeat(replicas, 1, 1, 1)
    lab = torch.randint(0, 1000, (4,), generator=g).cuda().repeat(replicas)
    for _ in range(3):
        assert math.isfinite(float(st.train_step(img, lab)[0]))
    torch.cuda.synchronize()
    (e0, o0), (e1, o1) = pairs[0], pairs[-1]
    r = o0.trust_ratios()
    assert type(o0).__name__ == "LAMB" and o0.iterations == 3 and len(r) == 54
    assert all(math.isfinite(x) and x > 0 for x in r.values())
    assert torch.isfinite(e0.params).all() and not torch.equal(e0.params, start)
    for x, y in ((e0.params, e1.params), (o0.m, o1.m), (o0.v, o1.v), (o0.ratios, o1.ratios)):
        assert torch.equal(x, y)
