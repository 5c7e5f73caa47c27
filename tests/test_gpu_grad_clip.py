"""Global-norm gradient clipping and the non-finite skip on the GPU: the fixed-order norm pass
against float64, the three optimizers under clipping, bitwise reproducibility, the skip, graph
capture and the engine-level step (single, two rehearsal replicas, --accum-steps).

gn = {norm, scale, skip, clip, skip_enabled, clipped steps, skipped steps, -}.

Bounds.  Norm and scale to rtol 1e-5 of float64 (the `_check` bound of test_gpu_lars.py, same
argument: a thread adds a few float4s per component before the tree combine; a CPU emulation of
exactly this reduction order at the default chunk on 25.6M gradients ~N(0, 1e-2) with gs = 0.5
is within 1.4e-8 relative).  Parameters and slots to atol 1e-6 + rtol 1e-5 of the float64 update
(the bound of test_gpu_param_pipeline.py's optimizer tests).  The float64 references take the
hyper-parameters rounded to fp32 first, as test_gpu_lars.py does."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR, MU, WD, ETA, EPS, GS = 0.1, 0.9, 1e-4, 1e-3, 0.0, 0.5
B1, B2, AEPS = 0.9, 0.999, 1e-7
CHUNK = 1024
PAD = 60                      # sentinel floats after n
# one float4; under one wave of float4s; exactly one chunk; a chunk + one float4; 66 partials (more
# than one wave in the fold); 258 partials (the fold's lane loop wraps past 256)
NORM_NS = [4, 252, 1024, 1028, 65 * 1024 + 12, 257 * 1024 + 4]
# (size, adapt) segments of the optimizer tests (the SIZES of test_gpu_lars.py): 72 chunks of 1024,
# the last one ragged (248 floats)
SIZES = [(4, 1), (252, 1), (1024, 1), (1028, 1), (3 * 1024, 1), (65 * 1024 + 12, 1), (1000, 0)]
OPT_N = sum(s for s, _ in SIZES)
OPTS = ["adam", "sgd", "sgd_nesterov", "lars"]


def N():
    from pddl.ops.native import require_native
    return require_native()


def f32(x):
    return float(np.float32(x))


def _norm64(g, gs=GS):
    return math.sqrt(float(((f32(gs) * g.double().cpu()) ** 2).sum()))


def _gn(clip=0.0, skip_enabled=0.0, fill=0.0):
    gn = torch.full((8,), fill)
    gn[3], gn[4], gn[5], gn[6] = clip, skip_enabled, 0.0, 0.0
    return gn.cuda()


def _grad_norm(g, n, gn, chunk=CHUNK):
    partials = torch.full((-(-n // chunk) + 3,), float("nan"), device="cuda")
    N().grad_norm(g[:n], GS, chunk, partials, gn)
    return partials


@pytest.mark.parametrize("n", NORM_NS)
def test_norm_at_every_boundary(n):
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n + PAD, generator=gen)
    g[n:] = 1e6                                   # sentinels: they must not enter the sum
    want = _norm64(g[:n])
    g = g.cuda()
    # clip = 0: measure only
    gn = _gn(fill=float("nan"))
    partials = _grad_norm(g, n, gn)
    m = -(-n // CHUNK)
    h = gn.cpu().tolist()
    print(f"n {n}: norm {h[0]!r} float64 {want!r} rel {abs(h[0] - want) / want:.2e}")
    assert torch.isfinite(partials[:m]).all() and torch.isnan(partials[m:]).all()
    assert h[0] == pytest.approx(want, rel=1e-5) and h[1] == 1.0 and h[2] == 0.0 and h[5:7] == [0.0, 0.0]
    # the partials are the chunks' sums
    for b in {0, m - 1}:
        c = g[b * CHUNK:min(n, (b + 1) * CHUNK)].double().cpu() * f32(GS)
        assert partials[b].item() == pytest.approx(float((c * c).sum()), rel=1e-5)
    # clip above the norm: exactly 1, counter unmoved
    gn = _gn(clip=2 * want, fill=float("nan"))
    _grad_norm(g, n, gn)
    h = gn.cpu().tolist()
    assert h[0] == pytest.approx(want, rel=1e-5) and h[1] == 1.0 and h[2] == 0.0 and h[5] == 0.0
    # clip = half the norm
    gn = _gn(clip=want / 2, fill=float("nan"))
    _grad_norm(g, n, gn)
    _grad_norm(g, n, gn)
    h = gn.cpu().tolist()
    print(f"n {n}: scale {h[1]!r}")
    assert h[1] == pytest.approx(0.5, rel=1e-5) and h[1] < 1.0 and h[2] == 0.0
    assert h[3] == f32(want / 2) and h[5] == 2.0 and h[6] == 0.0          # one count per call


def test_default_chunk_on_the_whole_parameter_buffer():
    from pddl.models.resnet50 import ParamLayout
    from pddl.train.optim import GRAD_NORM_CHUNK
    assert GRAD_NORM_CHUNK == N().GRAD_NORM_DEFAULT_CHUNK == 16384
    n = ParamLayout().n_trainable
    gen = torch.Generator(device="cuda").manual_seed(21)
    g = torch.randn(n, device="cuda", generator=gen) * 1e-2
    want = math.sqrt(float(((g.double() * f32(GS)) ** 2).sum()))
    gn = _gn(clip=want / 2, fill=float("nan"))
    _grad_norm(g, n, gn, GRAD_NORM_CHUNK)
    h = gn.cpu().tolist()
    print(f"n {n}: norm {h[0]!r} float64 {want!r} rel {abs(h[0] - want) / want:.2e} scale {h[1]!r}")
    assert h[0] == pytest.approx(want, rel=1e-5) and h[1] == pytest.approx(0.5, rel=1e-5) and h[5] == 1.0


def test_launcher_errors():
    g = torch.zeros(64, device="cuda")
    gn, partials = _gn(), torch.zeros(8, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 4"):
        N().grad_norm(g[:6], GS, 16, partials, gn)
    for chunk in (2, 6):
        with pytest.raises(RuntimeError, match="chunk must be a positive multiple of 4"):
            N().grad_norm(g, GS, chunk, partials, gn)
    with pytest.raises(RuntimeError, match="partials buffer smaller"):
        N().grad_norm(g, GS, 4, partials, gn)                       # 16 chunks, 8 floats
    with pytest.raises(RuntimeError, match="gn"):
        N().grad_norm(g, GS, 16, partials, gn[:4])
    N().grad_norm(g, GS, 8, partials, gn)                           # 8 chunks fit
    torch.cuda.synchronize()
    assert gn.cpu().tolist()[:3] == [0.0, 1.0, 0.0]


# ---- the optimizers under clipping ----------------------------------------------------------

def _segments():
    segs, off = [], 0
    for size, adapt in SIZES:
        segs.append((off, size, adapt))
        off += size
    return segs


@pytest.fixture(scope="module")
def src():
    """Magnitudes of test_gpu_param_pipeline.py's optimizer tests (|p|, |g| ~ 0.5, momentum ~ 0.1,
    Adam v >= 1e-3), host tensors, never written."""
    gen = torch.Generator().manual_seed(27)
    r = lambda s: s * torch.randn(OPT_N + PAD, generator=gen)   # noqa: E731
    d = dict(p=r(0.5), g=r(0.5), mom=r(0.1), m=r(0.05), v=1e-3 + 0.1 * torch.rand(OPT_N + PAD, generator=gen))
    d["norm"] = _norm64(d["g"][:OPT_N])
    return d


class _State:
    """Device copies of the source vectors and the buffers one optimizer's calls need."""

    def __init__(self, name, src, g=None):
        from pddl.train.optim import lars_chunks, lars_table
        self.name = name
        self.p = src["p"].cuda()
        self.g = (src["g"] if g is None else g).cuda()
        self.hs = torch.tensor([0.0, LR, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], device="cuda")
        if name == "adam":
            self.slots = [src["m"].cuda(), src["v"].cuda()]
        else:
            self.slots = [src["mom"].cuda()]
        if name == "lars":
            self.th = lars_table(_segments(), CHUNK)
            self.td = self.th.cuda()
            self.partials = torch.zeros(2 * lars_chunks(self.th, CHUNK), device="cuda")
            self.ratios = torch.full((len(SIZES),), 7.0, device="cuda")
        self.gn_partials = torch.zeros(-(-OPT_N // CHUNK), device="cuda")

    def step(self, gn):
        """hparams kernel, norm pass (when gn is given), update: the calls of FlatOptimizer.step."""
        n, nat = OPT_N, N()
        nat.opt_hparams(self.hs, B1, B2, self.name == "adam")
        if gn is not None:
            nat.grad_norm(self.g[:n], GS, CHUNK, self.gn_partials, gn)
        if self.name == "adam":
            nat.adam(self.p[:n], self.g[:n], self.slots[0][:n], self.slots[1][:n], 0.0, B1, B2, AEPS, GS, self.hs, gn)
        elif self.name == "lars":
            nat.lars(self.p[:n], self.g[:n], self.slots[0][:n], self.td, self.th, CHUNK, self.partials, self.ratios,
                     0.0, MU, WD, ETA, EPS, GS, self.hs, gn)
        else:
            nat.sgd(self.p[:n], self.g[:n], self.slots[0][:n], 0.0, MU, WD, self.name == "sgd_nesterov", GS, self.hs,
                    gn)

    def tensors(self):
        return [self.p, *self.slots, self.hs] + ([self.ratios] if self.name == "lars" else [])


def _reference(name, src, scale, lr_t):
    """The float64 update of the source vectors with the gradient GS * scale * g -> (p, slots, ratios)."""
    n = OPT_N
    p, g = src["p"][:n].double().numpy().copy(), src["g"][:n].double().numpy()
    mu, wd0, eta, eps, gs = (f32(x) for x in (MU, WD, ETA, EPS, GS))
    b1, b2, aeps = f32(B1), f32(B2), f32(AEPS)
    gg = gs * scale * g
    if name == "adam":
        m = b1 * src["m"][:n].double().numpy() + (1 - b1) * gg
        v = b2 * src["v"][:n].double().numpy() + (1 - b2) * gg * gg
        return p - lr_t * m / (np.sqrt(v) + aeps), [m, v], None
    v = src["mom"][:n].double().numpy().copy()
    if name != "lars":
        gr = gg + wd0 * p
        v = mu * v - lr_t * gr
        return p + ((mu * v - lr_t * gr) if name == "sgd_nesterov" else v), [v], None
    ratios = []
    for off, size, adapt in _segments():
        sl = slice(off, off + size)
        w, ge = p[sl], gg[sl]
        ratio, wd = 1.0, 0.0
        if adapt:
            wd = wd0
            wn, gnorm = math.sqrt((w * w).sum()), math.sqrt((ge * ge).sum())
            if wn > 0 and gnorm > 0:
                ratio = eta * wn / (gnorm + wd * wn + eps)
        ratios.append(ratio)
        v[sl] = mu * v[sl] + lr_t * ratio * (ge + wd * w)
        p[sl] = w - v[sl]
    return p, [v], np.array(ratios)


def _close(got, ref):
    err = np.abs(got.double().cpu().numpy() - ref)
    allow = 1e-6 + 1e-5 * np.abs(ref)
    print(f"  worst error / allowance {float((err / allow).max()):.3f}")
    return bool((err <= allow).all())


@pytest.mark.parametrize("name", OPTS)
def test_optimizer_under_clipping_matches_float64(name, src):
    n = OPT_N
    st = _State(name, src)
    gn = _gn(clip=src["norm"] / 2)
    st.step(gn)
    torch.cuda.synchronize()
    h = gn.cpu().tolist()
    assert h[0] == pytest.approx(src["norm"], rel=1e-5) and h[1] == pytest.approx(0.5, rel=1e-5) and h[5] == 1.0
    lr_t = st.hs[2].item()                        # (Adam: the device's bias-corrected rate, an fp32 hyper-parameter)
    assert st.hs[0].item() == 1.0
    p64, s64, r64 = _reference(name, src, (src["norm"] / 2) / src["norm"], lr_t)
    assert _close(st.p[:n], p64)
    for s, r in zip(st.slots, s64):
        assert _close(s[:n], r)
    if r64 is not None:
        assert np.allclose(st.ratios.cpu().double().numpy(), r64, rtol=1e-5, atol=0)
    # past n nothing is written
    assert torch.equal(st.p[n:].cpu(), src["p"][n:])
    for s, key in zip(st.slots, ("m", "v") if name == "adam" else ("mom",)):
        assert torch.equal(s[n:].cpu(), src[key][n:])
    # the clipping is really in there: the unclipped float64 update is elsewhere
    q64, _, _ = _reference(name, src, 1.0, lr_t)
    assert not ((np.abs(st.p[:n].double().cpu().numpy() - q64) <= 1e-6 + 1e-5 * np.abs(q64)).all())


@pytest.mark.parametrize("name", OPTS)
def test_clip_above_the_norm_is_bitwise_the_plain_step(name, src):
    a, b, c = _State(name, src), _State(name, src), _State(name, src)
    gb, gc = _gn(clip=2 * src["norm"], skip_enabled=1.0), _gn(clip=0.0)
    for _ in range(2):
        a.step(None)
        b.step(gb)
        c.step(gc)
    torch.cuda.synchronize()
    for other, gn in ((b, gb), (c, gc)):
        for x, y in zip(a.tensors(), other.tensors()):
            assert torch.equal(x, y)
        assert gn.cpu().tolist()[1:3] == [1.0, 0.0] and gn.cpu().tolist()[5:7] == [0.0, 0.0]


@pytest.mark.parametrize("name", ["adam", "lars"])
def test_bitwise_reproducible_across_runs_and_streams(name, src):
    def run():
        st, gn = _State(name, src), _gn(clip=src["norm"] / 2)
        st.step(gn)
        return st.tensors() + [gn, st.gn_partials]
    a = run()
    b = run()
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
        c = run()
    torch.cuda.synchronize()
    for x, y in zip(a, c):
        assert torch.equal(x, y)


# first element; last element of a full chunk; last element of the ragged final chunk
POSITIONS = [0, CHUNK - 1, OPT_N - 1]


@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_step_is_skipped(bad, pos, src):
    """The injected values are plain data: the norm pass flags them, the update kernels return."""
    assert OPT_N % CHUNK and OPT_N - 1 >= (OPT_N // CHUNK) * CHUNK
    g_bad = src["g"].clone()
    g_bad[pos] = bad
    for name in OPTS:
        st = _State(name, src, g_bad)
        before = [t.clone() for t in st.tensors()]
        gn = _gn(clip=src["norm"] / 2, skip_enabled=1.0)
        st.step(gn)
        torch.cuda.synchronize()
        h = gn.cpu().tolist()
        assert not math.isfinite(h[0]) and h[2] == 1.0 and h[6] == 1.0, (name, h)
        for x, y in zip(st.tensors(), before):
            if x is st.hs:
                assert x[0].item() == y[0].item() + 1            # the step count still advances
            else:
                assert torch.equal(x, y), name                    # p, slots, LARS ratios: bit-unchanged
        # a following finite step updates normally and leaves the skip counter alone
        st.g.copy_(src["g"])
        st.step(gn)
        torch.cuda.synchronize()
        h = gn.cpu().tolist()
        assert h[0] == pytest.approx(src["norm"], rel=1e-5) and h[2] == 0.0 and h[5] == 1.0 and h[6] == 1.0
        assert st.hs[0].item() == 2.0 and not torch.equal(st.p, before[0]) and torch.isfinite(st.p).all()
        if name == "lars":
            assert (st.ratios[:-1] != 7.0).all() and st.ratios[-1].item() == 1.0
    # skip_enabled = 0: the flag stays 0 (and the step is taken)
    st = _State("sgd", src, g_bad)
    gn = _gn(clip=0.0, skip_enabled=0.0)
    st.step(gn)
    torch.cuda.synchronize()
    h = gn.cpu().tolist()
    assert not math.isfinite(h[0]) and h[2] == 0.0 and h[6] == 0.0
    assert not torch.isfinite(st.p[:OPT_N]).all()


# ---- FlatOptimizer: capture ----------------------------------------------------------------

class _FlatEngine:
    """The flat buffers an optimizer needs, with the real layout."""

    def __init__(self, seed):
        from pddl.models.resnet50 import ParamLayout
        self.L = ParamLayout()
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.params = torch.randn(self.L.total, device="cuda", generator=g) * 0.05
        self.grads = torch.randn(self.L.n_trainable, device="cuda", generator=g) * 1e-2


@pytest.mark.parametrize("name", ["adam", "lars"])
def test_captured_step_replays_like_eager_steps(name):
    from pddl.train.optim import make_optimizer

    def make():
        e = _FlatEngine(5)
        n1 = math.sqrt(float((e.grads.double() ** 2).sum()))
        opt = make_optimizer(name, e, lr=LR if name == "lars" else 1e-3, momentum=MU, weight_decay=WD,
                             global_clipnorm=n1 / 2, skip_nonfinite=True)
        return e, opt, n1
    (ea, oa, n1), (eb, ob, _) = make(), make()
    assert torch.equal(ea.params, eb.params) and oa.gn is not None
    assert oa.gn_partials.numel() == -(-ea.L.n_trainable // 16384)     # one float per chunk of the norm pass
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

    def same():
        assert torch.equal(ea.params, eb.params) and torch.equal(oa.hs, ob.hs) and torch.equal(oa.gn, ob.gn)
        for x, y in zip(oa.state_tensors().values(), ob.state_tensors().values()):
            assert torch.equal(x, y)
        if name == "lars":
            assert torch.equal(oa.ratios, ob.ratios)
    same()
    st = ob.clip_stats()
    assert st["norm"] == pytest.approx(n1, rel=1e-5) and st["scale"] == pytest.approx(0.5, rel=1e-5)
    assert st["clipped"] == 4 and st["skipped"] == 0 and ob.hs[0].item() == 4
    # a host-side change of the threshold reaches the next replay
    for o in (oa, ob):
        o.set_grad_clip(n1 / 4, skip_nonfinite=True)
    oa.step()
    ob.sync_hparams()
    g.replay()
    ob._iterations += 1
    torch.cuda.synchronize()
    same()
    assert ob.clip_stats()["scale"] == pytest.approx(0.25, rel=1e-5) and ob.clip_stats()["clipped"] == 5
    ob.reset_clip_counters()
    assert ob.clip_stats()["clipped"] == 0 and ob.clip_stats()["scale"] == pytest.approx(0.25, rel=1e-5)


# ---- engine level ---------------------------------------------------------------------------

def _cfg(strategy, **kw):
    from pddl.config import make_config
    base = dict(strategy=strategy, batch_size=4, crop=32, image_size=32, optimizer="sgd", momentum=0.0, lr=0.05,
                weight_decay=0.0, device="cuda", graphs=False, flip=False, data="synthetic_fixed", seed=0,
                num_classes=1000)
    base.update(kw)
    return make_config("bench", **base)


def _batch(n, seed=99):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (n, 32, 32, 3), dtype=torch.uint8, generator=g).cuda(),
            torch.randint(0, 1000, (n,), generator=g).cuda())


def _single(**kw):
    from pddl.parallel.strategies import make_strategy
    from pddl.train.trainer import Trainer
    cfg = _cfg("single", **kw)
    st = make_strategy(cfg)
    Trainer(cfg, st)
    return st


@pytest.fixture(scope="module")
def twin():
    """The unclipped twin's first step (same seed, same batch; measure only): its gradient norm
    and its parameter change."""
    st = _single(skip_nonfinite=True)
    n = st.engine.L.n_trainable
    start = st.engine.params[:n].clone()
    st.train_step(*_batch(4))
    torch.cuda.synchronize()
    cs = st.opt.clip_stats()
    assert cs["scale"] == 1.0 and cs["clipped"] == 0 and cs["skipped"] == 0
    want = math.sqrt(float((st.engine.grads[:n].double() ** 2).sum()))
    assert cs["norm"] == pytest.approx(want, rel=1e-5)
    return {"norm": cs["norm"], "start": start, "delta": (st.engine.params[:n] - start).double().cpu()}


def test_engine_level_single_strategy(twin):
    from pddl.models.engine import HipEngine
    n1 = twin["norm"]
    assert math.isfinite(n1) and n1 > 0
    st = _single(global_clipnorm=n1 / 2)
    n = st.engine.L.n_trainable
    assert isinstance(st.engine, HipEngine) and type(st.opt).__name__ == "SGD" and st.opt.global_clipnorm == n1 / 2
    assert torch.equal(st.engine.params[:n], twin["start"])
    img, lab = _batch(4)
    st.train_step(img, lab)
    torch.cuda.synchronize()
    cs = st.opt.clip_stats()
    print(f"twin norm {n1!r}, clipped run: {cs}")
    assert cs["scale"] == pytest.approx(0.5, rel=1e-5) and cs["clipped"] == 1 and cs["skipped"] == 0
    got = (st.engine.params[:n] - twin["start"]).double().cpu()
    want = twin["delta"] / 2
    err, allow = (got - want).abs(), 1e-6 + 1e-5 * want.abs()
    print(f"parameter change: worst error / allowance {float((err / allow).max()):.3f}, "
          f"largest change {float(want.abs().max()):.3e}")
    assert float(want.abs().max()) > 1e-5 and bool((err <= allow).all())
    for _ in range(3):
        s = st.train_step(img, lab)
        assert math.isfinite(float(s[0]))
    assert torch.isfinite(st.engine.params).all() and st.opt.iterations == 4


def test_two_rehearsal_replicas_end_bit_identical(monkeypatch, twin):
    """Both replicas see the twin's batch, so the all-reduced mean gradient of step 1 is the twin's;
    a quarter of its norm as the threshold keeps all 3 Adam steps (lr 1e-3) clipping."""
    from pddl.parallel.strategies import MirroredStrategy
    from pddl.train.trainer import Trainer
    monkeypatch.setenv("PDDL_REHEARSE", "1")
    cfg = _cfg("mirrored", optimizer="adam", lr=1e-3, global_clipnorm=twin["norm"] / 4, skip_nonfinite=True)
    st = MirroredStrategy(cfg, devices=[0, 0])
    Trainer(cfg, st)
    st.broadcast_state(None)
    img, lab = _batch(4)
    img, lab = torch.cat([img, img]), torch.cat([lab, lab])
    for _ in range(3):
        s = st.train_step(img, lab)
        assert math.isfinite(float(s[0]))
    torch.cuda.synchronize()
    (e0, o0), (e1, o1) = st.mirror.replicas
    print(o0.clip_stats(), o1.clip_stats())
    assert o0.iterations == 3
    assert torch.equal(e0.params, e1.params) and torch.equal(o0.m, o1.m) and torch.equal(o0.v, o1.v)
    assert torch.equal(o0.gn[:7], o1.gn[:7])
    assert o0.clip_stats()["clipped"] == 3 and o1.clip_stats()["clipped"] == 3 and o0.clip_stats()["skipped"] == 0


def test_accum_steps_reports_the_norm_of_the_folded_mean_gradient(twin):
    st = _single(accum_steps=2, global_clipnorm=twin["norm"] / 2)
    n = st.engine.L.n_trainable
    start = st.engine.params.clone()
    st.train_step(*_batch(4, 7))
    torch.cuda.synchronize()
    assert st.opt.iterations == 0 and torch.equal(st.engine.params, start)
    assert st.opt.clip_stats()["norm"] == 0.0                        # no update yet: the norm pass has not run
    st.train_step(*_batch(4, 8))
    torch.cuda.synchronize()
    assert st.opt.iterations == 1 and not torch.equal(st.engine.params, start)
    want = math.sqrt(float((st.engine.grads[:n].double() ** 2).sum()))
    cs = st.opt.clip_stats()
    print(f"folded mean gradient: norm {cs['norm']!r} float64 {want!r}, scale {cs['scale']!r}")
    assert cs["norm"] == pytest.approx(want, rel=1e-5)
    scale = (twin["norm"] / 2) / want if want > twin["norm"] / 2 else 1.0
    assert cs["scale"] == pytest.approx(scale, rel=1e-5) and cs["clipped"] == int(scale < 1.0)
