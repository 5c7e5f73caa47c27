"""LARS on the GPU: the two-pass segmented kernel against float64, bitwise reproducibility, the
device-side learning-rate schedule, graph capture and the engine-level step.

The float64 references take the hyper-parameters rounded to fp32 first: the kernels receive
them as floats, and e.g. 1 - fp32(0.999) differs from 1 - 0.999 by 1.3e-5 relative."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR, MU, WD, ETA, EPS, GS = 0.1, 0.9, 1e-4, 1e-3, 0.0, 0.5
CHUNK = 1024
# (size, adapt): one float4; under one wave of float4s; exactly one chunk; one chunk + one float4;
# three whole chunks; 66 partials (more than a wave's 64 lanes in the fold); a non-adapted segment
SIZES = [(4, 1), (252, 1), (1024, 1), (1028, 1), (3 * 1024, 1), (65 * 1024 + 12, 1), (1000, 0)]
PAD = 60                      # sentinel floats after the last segment: they belong to no segment


def N():
    from pddl.ops.native import require_native
    return require_native()


def f32(x):
    return float(np.float32(x))


def _segments(sizes):
    segs, off = [], 0
    for size, adapt in sizes:
        segs.append((off, size, adapt))
        off += size
    return segs, off


def _inputs(n, seed, mom_scale=0.5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g), torch.randn(n, generator=g), mom_scale * torch.randn(n, generator=g))


def _reference(segs, p, g, v, lr=LR):
    """float64 LARS over (offset, size, adapt) segments -> (p, v, ratios)."""
    p, g, v = p.double().numpy().copy(), g.double().numpy(), v.double().numpy().copy()
    lr, mu, wd0, eta, eps, gs = (f32(x) for x in (lr, MU, WD, ETA, EPS, GS))
    ratios = []
    for off, size, adapt in segs:
        sl = slice(off, off + size)
        w, gg = p[sl], gs * g[sl]
        ratio, wd = 1.0, 0.0
        if adapt:
            wd = wd0
            wn, gn = math.sqrt((w * w).sum()), math.sqrt((gg * gg).sum())
            if wn > 0 and gn > 0:
                ratio = eta * wn / (gn + wd * wn + eps)
        ratios.append(ratio)
        v[sl] = mu * v[sl] + lr * ratio * (gg + wd * w)
        p[sl] = w - v[sl]
    return p, v, np.array(ratios)


def _run(segs, chunk, p, g, v, lr=LR, hs=None):
    """The two launches on the current stream -> (p, v, ratios) device tensors."""
    from pddl.train.optim import lars_chunks, lars_table
    th = lars_table(segs, chunk)
    p, g, v = p.cuda(), g.cuda(), v.cuda()
    partials = torch.full((2 * lars_chunks(th, chunk),), float("nan"), device="cuda")
    ratios = torch.full((len(segs),), float("nan"), device="cuda")
    N().lars(p, g, v, th.cuda(), th, chunk, partials, ratios, lr, MU, WD, ETA, EPS, GS, hs)
    return p, v, ratios


def _check(segs, end, got, ref):
    """Trust ratios to rtol 1e-5: a thread adds at most a few float4s per component before the
    tree combine, so the fp32 sums of non-negative terms are within ~20 ulp (2^-24 each) of exact
    and the square root halves that.  Parameters and momentum to atol 1e-6: |w|, |v| < 8 here, so
    each of the two roundings per element is at most half an ulp of 8 = 4.8e-7 / 2."""
    (p, v, r), (p64, v64, r64) = got, ref
    assert np.allclose(r.cpu().double().numpy(), r64, rtol=1e-5, atol=0), (r.cpu().tolist(), r64.tolist())
    assert np.abs(p.cpu().double().numpy()[:end] - p64[:end]).max() <= 1e-6
    assert np.abs(v.cpu().double().numpy()[:end] - v64[:end]).max() <= 1e-6


def test_kernel_matches_float64_at_every_boundary():
    segs, end = _segments(SIZES)
    p0, g0, v0 = _inputs(end + PAD, 7)
    got = _run(segs, CHUNK, p0, g0, v0)
    torch.cuda.synchronize()
    ref = _reference(segs, p0, g0, v0)
    _check(segs, end, got, ref)
    p, v, r = got
    assert all(x != 1.0 for x in r[:-1].tolist()) and r[-1].item() == 1.0
    # the non-adapted segment is the plain momentum update: no ratio, no decay
    off, size, _ = segs[-1]
    sl = slice(off, off + size)
    vv = f32(MU) * v0[sl].double() + f32(LR) * (f32(GS) * g0[sl].double())
    assert (v[sl].cpu().double() - vv).abs().max() <= 1e-6
    assert (p[sl].cpu().double() - (p0[sl].double() - vv)).abs().max() <= 1e-6
    # the padding is bit-unchanged
    assert torch.equal(p[end:].cpu(), p0[end:]) and torch.equal(v[end:].cpu(), v0[end:])


def test_segment_size_not_a_multiple_of_4_raises():
    p0, g0, v0 = _inputs(64, 1)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        _run([(0, 6, 1)], CHUNK, p0, g0, v0)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        _run([(2, 8, 1)], CHUNK, p0, g0, v0)
    with pytest.raises(RuntimeError, match="inside the buffer"):
        _run([(0, 32, 1), (32, 64, 1)], CHUNK, p0, g0, v0)
    from pddl.train.optim import lars_table
    th = lars_table([(0, 32, 1), (32, 32, 1)], 8)
    with pytest.raises(RuntimeError, match="chunk0"):       # a table built for another chunk size
        N().lars(p0.cuda(), g0.cuda(), v0.cuda(), th.cuda(), th, 16, torch.zeros(64, device="cuda"),
                 torch.zeros(2, device="cuda"), LR, MU, WD, ETA, EPS, GS, None)
    torch.cuda.synchronize()


def test_default_chunk_on_conv5_sized_segment():
    """conv5's 3x3 kernel (2,359,296 floats: 144 partials at the default chunk) plus a 64-float one."""
    from pddl.train.optim import LARS_CHUNK
    assert LARS_CHUNK == N().LARS_DEFAULT_CHUNK
    segs, end = _segments([(2359296, 1), (64, 1)])
    p0, g0, v0 = _inputs(end, 11)
    got = _run(segs, LARS_CHUNK, p0, g0, v0)
    torch.cuda.synchronize()
    _check(segs, end, got, _reference(segs, p0, g0, v0))


def test_bitwise_reproducible_across_runs_and_streams():
    segs, end = _segments([(2359296, 1), (65 * 1024 + 12, 1), (1000, 0)])   # 2304 + 66 partials at chunk 1024
    p0, g0, v0 = _inputs(end, 13)
    a = _run(segs, CHUNK, p0, g0, v0)
    b = _run(segs, CHUNK, p0, g0, v0)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # on another stream, while an unrelated kernel occupies the device
    busy = torch.randn(4096, 4096, device="cuda")
    side, other = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(other):
        for _ in range(8):
            busy = busy @ busy * 1e-3
    with torch.cuda.stream(side):
        c = _run(segs, CHUNK, p0, g0, v0)
    torch.cuda.synchronize()
    for x, y in zip(a, c):
        assert torch.equal(x, y)


def test_zero_gradient_and_zero_weight_segments_take_ratio_one():
    segs, end = _segments([(2048, 1), (1028, 1), (512, 1)])
    p0, g0, v0 = _inputs(end, 3)
    g0[:2048] = 0                      # all-zero gradient
    p0[2048:2048 + 1028] = 0           # all-zero weights
    p, v, r = _run(segs, CHUNK, p0, g0, v0)
    torch.cuda.synchronize()
    assert r[0].item() == 1.0 and r[1].item() == 1.0 and r[2].item() != 1.0
    assert torch.isfinite(p).all() and torch.isfinite(v).all() and torch.isfinite(r).all()
    _check(segs, end, (p, v, r), _reference(segs, p0, g0, v0))


@pytest.mark.parametrize("adam", [False, True])
def test_device_schedule_matches_host_formula(adam):
    from pddl.train.optim import scheduled_lr
    lr, end_lr, wu, tot, b1, b2 = 0.8, 1e-3, 3, 8, 0.9, 0.999
    hs = torch.tensor([0.0, lr, 0.0, 0.0, wu, tot, end_lr, 0.0], device="cuda")
    got = []
    for _ in range(tot + 2):
        N().opt_hparams_sched(hs, b1, b2, adam)
        got.append(hs.cpu().tolist())
    for t, h in enumerate(got, start=1):
        want = scheduled_lr(f32(lr), t, wu, tot, f32(end_lr))
        assert h[0] == t
        assert h[3] == pytest.approx(want, rel=1e-6)
        if adam:
            want *= math.sqrt(1 - f32(b2) ** t) / (1 - f32(b1) ** t)
        assert h[2] == pytest.approx(want, rel=1e-6), t
        assert h[1] == f32(lr) and h[4:7] == [wu, tot, f32(end_lr)]


class _FlatEngine:
    """The flat buffers an optimizer needs, with the real layout."""

    def __init__(self, seed):
        from pddl.models.resnet50 import ParamLayout
        self.L = ParamLayout()
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.params = torch.randn(self.L.total, device="cuda", generator=g) * 0.05
        self.grads = torch.randn(self.L.n_trainable, device="cuda", generator=g) * 1e-2


def _flat_lars(seed=5):
    from pddl.train.optim import make_optimizer
    e = _FlatEngine(seed)
    opt = make_optimizer("lars", e, lr=LR, momentum=MU, weight_decay=WD)
    opt.set_schedule(2, 8, 1e-3)
    return e, opt


def test_captured_step_replays_like_eager_steps():
    from pddl.train.optim import scheduled_lr
    ea, oa = _flat_lars()
    eb, ob = _flat_lars()
    assert torch.equal(ea.params, eb.params)
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
    assert torch.equal(ea.params, eb.params) and torch.equal(oa.mom, ob.mom)
    assert torch.equal(oa.ratios, ob.ratios) and torch.equal(oa.hs, ob.hs)
    assert ob.hs[0].item() == 4 and ob.hs[3].item() == pytest.approx(scheduled_lr(f32(LR), 4, 2, 8, f32(1e-3)), rel=1e-6)
    # a host-side change of the base rate reaches the next replay
    oa.lr = ob.lr = 0.3
    oa.step()
    ob.sync_hparams()
    g.replay()
    ob._iterations += 1
    torch.cuda.synchronize()
    assert ob.hs[3].item() == pytest.approx(scheduled_lr(f32(0.3), 5, 2, 8, f32(1e-3)), rel=1e-6)
    assert torch.equal(ea.params, eb.params) and torch.equal(oa.mom, ob.mom)
    end = max(x.offset + x.size for x in ea.L.entries.values() if x.trainable)
    assert (ob.mom[end:] == 0).all()           # the alignment padding is never written


def _cfg(strategy, **kw):
    from pddl.config import make_config
    return make_config("bench", strategy=strategy, batch_size=4, crop=32, image_size=32, optimizer="lars", lr=0.05,
                       weight_decay=5e-5, device="cuda", graphs=False, flip=False, data="synthetic_fixed", seed=0,
                       num_classes=1000, **kw)


def _batch(n):
    g = torch.Generator().manual_seed(99)
    return (torch.randint(0, 256, (n, 32, 32, 3), dtype=torch.uint8, generator=g).cuda(),
            torch.randint(0, 1000, (n,), generator=g).cuda())


def test_engine_level_single_strategy():
    from pddl.models.engine import HipEngine
    from pddl.parallel.strategies import make_strategy
    from pddl.train.trainer import Trainer
    cfg = _cfg("single")
    st = make_strategy(cfg)
    Trainer(cfg, st)
    assert isinstance(st.engine, HipEngine) and type(st.opt).__name__ == "LARS"
    img, lab = _batch(4)
    start = st.engine.params.clone()
    for _ in range(3):
        s = st.train_step(img, lab)
        assert math.isfinite(float(s[0]))
    r = st.opt.trust_ratios()
    assert len(r) == 54 and all(math.isfinite(x) and x > 0 for x in r.values())
    assert torch.isfinite(st.engine.params).all() and not torch.equal(st.engine.params, start)


def test_two_rehearsal_replicas_end_bit_identical(monkeypatch):
    from pddl.parallel.strategies import MirroredStrategy
    from pddl.train.trainer import Trainer
    monkeypatch.setenv("PDDL_REHEARSE", "1")
    cfg = _cfg("mirrored")
    st = MirroredStrategy(cfg, devices=[0, 0])
    Trainer(cfg, st)
    st.broadcast_state(None)
    img, lab = _batch(4)
    img, lab = torch.cat([img, img]), torch.cat([lab, lab])      # both replicas see the same data
    for _ in range(3):
        s = st.train_step(img, lab)
        assert math.isfinite(float(s[0]))
    torch.cuda.synchronize()
    (e0, o0), (e1, o1) = st.mirror.replicas
    assert o0.iterations == 3
    assert torch.equal(e0.params, e1.params) and torch.equal(o0.mom, o1.mom) and torch.equal(o0.ratios, o1.ratios)
