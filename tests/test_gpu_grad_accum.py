"""Gradient accumulation on the GPU (--accum-steps): the streaming kernel bit for bit against
torch fp32, the accumulator on the real bucket layout and a side stream, the engine's
accumulated gradient against the one-batch reference, the CLI's step accounting and two
rehearsal replicas."""
import json
import math
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = 7.25            # guard value (no input equals it: inputs are randn, and SENT + SENT != SENT)
GUARD = 8
OFFSETS = [0, 1, 2, 3, 5]
SMALL = [0, 1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025]


def _native():
    from pddl.ops.native import require_native
    return require_native()


def _sweep_lengths():
    # one full sweep of the kernel's grid-stride loop, and just past it, +- 1
    s = _native().grad_accum_sweep(0)
    return [s - 1, s, s + 1, s + 4, s + 5, s + 6]


@pytest.fixture(scope="module")
def pool():
    """Random fp32 source data shared by every kernel case (never written)."""
    n = max(_sweep_lengths()) + 64
    g = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randn(n, device="cuda", generator=g)
    b = torch.randn(n, device="cuda", generator=g)
    return a, b


def _slices(pool, n, off_acc, off_g):
    """acc / g slices of length n at the given float offsets of fresh 16-byte aligned buffers,
    sentinel guards on both sides."""
    a, b = pool
    A = torch.full((off_acc + GUARD + n + GUARD + 4,), SENT, device="cuda")
    G = torch.full((off_g + GUARD + n + GUARD + 4,), SENT, device="cuda")
    assert A.data_ptr() % 16 == 0 and G.data_ptr() % 16 == 0
    # (GUARD is a multiple of 4, so the slice's misalignment is the offset's)
    sa, sg = off_acc + GUARD, off_g + GUARD
    A[sa:sa + n] = a[:n]
    G[sg:sg + n] = b[:n]
    return A, G, sa, sg


def _check(pool, n, off_acc, off_g, mode):
    a, b = pool
    A, G, sa, sg = _slices(pool, n, off_acc, off_g)
    A0, G0 = A.clone(), G.clone()
    _native().grad_accum(A[sa:sa + n], G[sg:sg + n], mode)
    wantA, wantG = A0.clone(), G0.clone()
    if mode == 0:
        wantA[sa:sa + n] = b[:n]
    elif mode == 1:
        wantA[sa:sa + n] = a[:n] + b[:n]
    else:
        wantG[sg:sg + n] = b[:n] + a[:n]
    # whole buffers: the result, both guards and the untouched operand, bit for bit
    assert torch.equal(A.view(torch.int32), wantA.view(torch.int32)), (n, off_acc, off_g, mode)
    assert torch.equal(G.view(torch.int32), wantG.view(torch.int32)), (n, off_acc, off_g, mode)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("off", OFFSETS)
def test_kernel_bitwise_small_lengths(pool, off, mode):
    for n in SMALL:
        _check(pool, n, off, off, mode)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_kernel_bitwise_around_one_grid_sweep(pool, mode):
    for n in _sweep_lengths():
        for off in OFFSETS:
            _check(pool, n, off, off, mode)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_kernel_mismatched_alignment_takes_the_scalar_path(pool, mode):
    for off_acc, off_g in [(0, 1), (1, 0), (2, 5), (3, 2), (1, 3)]:
        for n in SMALL + [4099]:
            _check(pool, n, off_acc, off_g, mode)


def test_kernel_store_copies_bit_patterns():
    """Mode 0 is a copy, not arithmetic: -0.0, denormals, infinities and NaN payloads survive."""
    bits = torch.tensor([0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0x7fc00001, 0xffc12345,
                         0x7f800001, 0x00000000, 0x3f800000, 0x80000001], dtype=torch.int64)
    bits = bits.repeat(97)[:1031]                                 # head + body + tail at every offset
    src = bits.cuda()
    src = (src - (src >= 2 ** 31).to(torch.int64) * 2 ** 32).to(torch.int32)
    for off in OFFSETS:
        n = src.numel()
        G = torch.zeros(off + n + 4, dtype=torch.int32, device="cuda")
        A = torch.full((off + n + 4,), 0x12345678, dtype=torch.int32, device="cuda")
        G[off:off + n] = src
        _native().grad_accum(A.view(torch.float32)[off:off + n], G.view(torch.float32)[off:off + n], 0)
        assert torch.equal(A[off:off + n], src)
        assert (A[:off] == 0x12345678).all() and (A[off + n:] == 0x12345678).all()
    z = torch.full((5,), -0.0, device="cuda")
    out = torch.ones(5, device="cuda")
    _native().grad_accum(out, z, 0)
    assert torch.signbit(out).all() and (out == 0).all()


def test_binding_checks():
    N = _native()
    a, b = torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    with pytest.raises(RuntimeError):
        N.grad_accum(a, b[:7], 0)                                  # lengths differ
    with pytest.raises(RuntimeError):
        N.grad_accum(a, b, 3)                                      # no such mode
    with pytest.raises(RuntimeError):
        N.grad_accum(a[::2], b[::2], 0)                            # not contiguous
    with pytest.raises(RuntimeError):
        N.grad_accum(a.double(), b.double(), 0)                    # not fp32
    with pytest.raises(RuntimeError):
        N.grad_accum(a[:6], a[2:], 1)                              # overlapping slices
    N.grad_accum(a[:0], b[:0], 1)                                  # n = 0: a no-op
    torch.cuda.synchronize()


class _FlatEngine:
    def __init__(self, L, device="cuda"):
        self.L = L
        self.grads = torch.zeros(L.total, dtype=torch.float32, device=device)


def test_accumulator_on_the_real_bucket_layout_and_a_side_stream():
    from pddl.models.resnet50 import ParamLayout
    from pddl.train.accum import GradAccumulator
    L = ParamLayout()
    bks = L.buckets(32)
    assert len(bks) >= 3 and bks[0][0] == 0 and bks[-1][1] == L.n_trainable
    eng = _FlatEngine(L)
    K = 3
    acc = GradAccumulator(eng, K, bks)
    assert acc.acc.shape == eng.grads.shape and acc.acc.device == eng.grads.device
    gen = torch.Generator(device="cuda").manual_seed(17)
    gs = [torch.randn(L.total, device="cuda", generator=gen) for _ in range(K)]
    nt = L.n_trainable
    seen = []
    side = torch.cuda.Stream()
    want = None
    for m in range(K):
        eng.grads.copy_(gs[m])
        want = gs[m].clone() if want is None else want + gs[m]      # ((g1 + g2) + g3)
        last = m == K - 1
        assert acc.last == last
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            cb = acc.wrap(lambda i, m=m: seen.append((m, i, torch.cuda.current_stream() == side)))
            for i in range(len(bks)):                               # backward order: bucket 0 completes first
                cb(i)
        torch.cuda.current_stream().wait_stream(side)
        assert acc.advance() == last
        torch.cuda.synchronize()
        if not last:
            assert torch.equal(acc.acc[:nt], want[:nt]), m
            assert torch.equal(eng.grads, gs[m]), m                 # the gradient itself is untouched
            assert not seen
        else:
            assert torch.equal(eng.grads[:nt], want[:nt])
            assert torch.equal(eng.grads[nt:], gs[m][nt:])          # outside every bucket: untouched
    assert seen == [(K - 1, i, True) for i in range(len(bks))]      # once per bucket, only on micro-step K
    assert acc.micro == 0 and not acc.last


def test_engine_accumulated_gradient_within_the_one_batch_noise_floor():
    """K = 2 micro-batches of 2 images through HipEngine (bucket callbacks on the side stream)
    against the bf16-point TorchEngine on the same 4 images as one batch, with the bound
    tests/test_gpu_engine.py applies to a one-batch gradient: per tensor <= 3 x floor + 0.5 %,
    median <= 1.5 x the floor's median, the floor being the CPU-vs-GPU reference difference."""
    from test_gpu_engine import _engines, _grad_errors
    from pddl.models.reference import TorchEngine
    from pddl.train.accum import GradAccumulator
    torch.manual_seed(0)
    B, crop, image_size, K = 4, 160, 224, 2
    L, he, te = _engines(B, crop, image_size, bf16_points=True)
    assert he.side is not None                                      # the two-stream step: callbacks on the side stream
    tc = TorchEngine(L, B, crop=crop, device="cpu", bf16_points=True, fused_proj=he.fuse_proj)
    tc.params.copy_(te.params.cpu())
    img = torch.randint(0, 256, (B, image_size, image_size, 3), dtype=torch.uint8, device="cuda")
    lab = torch.randint(0, 1000, (B,), device="cuda")
    flip = torch.tensor([1, 0, 0, 1], dtype=torch.uint8, device="cuda")
    off = (7, 3)
    bks = L.buckets(32)
    acc = GradAccumulator(he, K, bks)
    seen, streams = [], []

    def comm(i):
        seen.append(i)
        streams.append(torch.cuda.current_stream() == he.side)

    loss = 0.0
    for m in range(K):
        sl = slice(m * 2, m * 2 + 2)
        s = he.forward_backward(img[sl], lab[sl], 1.0 / B, flip=flip[sl], crop_offset=off, bucket_cb=acc.wrap(comm),
                                buckets=bks).clone()
        acc.advance()
        loss += s[0].item()
        if m == 0:
            assert not seen
    s_t = te.forward_backward(img, lab, 1.0 / B, flip=flip, crop_offset=off)
    tc.forward_backward(img.cpu(), lab.cpu(), 1.0 / B, flip=flip.cpu(), crop_offset=off)
    torch.cuda.synchronize()
    assert seen == list(range(len(bks))) and all(streams)
    assert abs(loss - s_t[0].item()) / s_t[0].item() < 2e-3

    class _Cpu:
        grads = tc.grads.cuda()
    floor = {n: r for r, n in _grad_errors(L, _Cpu, te)}
    errs = _grad_errors(L, he, te)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    m_e, m_f = med([r for r, _ in errs]), med(list(floor.values()))
    print(f"accumulated 2 x 2: engine median {m_e:.4f}, floor median {m_f:.4f}, ratio {m_e / m_f:.3f}, "
          f"worst {errs[0][1]} {errs[0][0]:.4f} (floor {floor[errs[0][1]]:.4f})")
    over = [(n, round(r, 4), round(floor[n], 4)) for r, n in errs if r > 3 * floor[n] + 0.005]
    assert not over, over[:8]
    assert m_e <= 1.5 * m_f, (m_e, m_f)


def test_cli_counts_updates_not_micro_steps(monkeypatch, capsys, tmp_path):
    from pddl import cli
    from pddl.parallel.strategies import SingleStrategy
    from pddl.train.optim import scheduled_lr
    changed, holder = [], {}
    orig = SingleStrategy.train_step

    def step(self, images, labels):
        before = self.engine.params.clone()
        s = orig(self, images, labels)
        torch.cuda.synchronize()
        changed.append(not torch.equal(before, self.engine.params))
        holder["st"] = self
        return s

    monkeypatch.setattr(SingleStrategy, "train_step", step)
    jl = tmp_path / "m.jsonl"
    rc = cli.run("single", ["--device", "cuda", "--data", "synthetic", "--batch-size", "4", "--crop", "160",
                            "--accum-steps", "2", "--steps-per-epoch", "4", "--epochs", "1", "--lr-schedule", "poly",
                            "--lr", "0.01", "--lr-end", "0.002", "--validation-steps", "1", "--no-save",
                            "--metrics-jsonl", str(jl), "--verbose", "2"])
    assert rc == 0
    st = holder["st"]
    assert st.accum is not None and st.accum.k == 2 and st.accum.micro == 0
    assert changed == [False, True, False, True]                    # exactly two updates, on the K-th calls
    assert st.opt.iterations == 2
    assert st.opt.schedule == (0, 2, 0.002)                         # (warm-up, total) in updates: 4 steps / K
    want = scheduled_lr(0.01, 2, 0, 2, 0.002)
    out = capsys.readouterr().out
    assert "accum_steps=2" in out and "effective global batch=8" in out
    assert re.findall(r" - lr: (\S+) - ", out) == [f"{want:.4g}"]
    rec = json.loads(jl.read_text().splitlines()[-1])
    assert rec["lr"] == want and rec["accum_steps"] == 2 and rec["effective_global_batch"] == 8
    assert st.opt.hs[0].item() == 2                                 # the device's own step count
    assert st.opt.hs[3].item() == pytest.approx(want, rel=1e-6)


def test_two_rehearsal_replicas_end_bit_identical(monkeypatch):
    from pddl.config import make_config
    from pddl.parallel.strategies import MirroredStrategy
    from pddl.train.trainer import Trainer
    monkeypatch.setenv("PDDL_REHEARSE", "1")
    cfg = make_config("bench", strategy="mirrored", batch_size=4, crop=32, image_size=32, optimizer="lars", lr=0.05,
                      weight_decay=5e-5, device="cuda", flip=False, data="synthetic_fixed", seed=0, num_classes=1000,
                      accum_steps=2)
    st = MirroredStrategy(cfg, devices=[0, 0])
    Trainer(cfg, st)
    st.broadcast_state(None)
    g = torch.Generator().manual_seed(99)
    (e0, o0), (e1, o1) = st.mirror.replicas
    prev = e0.params.clone()
    changed = []
    for _ in range(4):                                              # two updates of K = 2 micro-steps
        img = torch.randint(0, 256, (4, 32, 32, 3), dtype=torch.uint8, generator=g).cuda()
        lab = torch.randint(0, 1000, (4,), generator=g).cuda()
        s = st.train_step(torch.cat([img, img]), torch.cat([lab, lab]))   # both replicas see the same data
        assert math.isfinite(float(s[0]))
        torch.cuda.synchronize()
        changed.append(not torch.equal(prev, e0.params))
        prev = e0.params.clone()
    assert changed == [False, True, False, True]
    assert o0.iterations == 2 and o1.iterations == 2
    assert torch.equal(e0.params, e1.params) and torch.equal(o0.mom, o1.mom) and torch.equal(o0.ratios, o1.ratios)


def test_overlapped_replica_step_folds_before_the_bucket_all_reduce(monkeypatch):
    """The eager in-process replica step with its bucketed RCCL all-reduce overlapped with backward
    (the multi-replica schedule, forced on one GPU with PDDL_MIRROR segmented=1; K > 1 never replays
    graphs): the wrapped bucket callbacks fold on the engine's side stream before the comm thread's
    all-reduce.  A 1-rank all-reduce is the identity, so the gradient after the K-th micro-step is
    the one the single strategy's whole-buffer path accumulates from the same batches (up to the
    order of the engine's fp32 weight-gradient atomics), and every bucket is reduced once per
    update."""
    from pddl.config import make_config
    from pddl.parallel.strategies import make_strategy
    from pddl.train.trainer import Trainer
    from pddl.utils.envopts import with_opt
    g = torch.Generator().manual_seed(7)
    batches = [(torch.randint(0, 256, (4, 32, 32, 3), dtype=torch.uint8, generator=g).cuda(),
                torch.randint(0, 1000, (4,), generator=g).cuda()) for _ in range(2)]
    grads = {}
    for strategy in ("single", "mirrored"):
        if strategy == "mirrored":
            monkeypatch.setenv("PDDL_MIRROR", with_opt("PDDL_MIRROR", "segmented", "1"))
        cfg = make_config("bench", strategy=strategy, batch_size=4, crop=32, image_size=32, optimizer="sgd", lr=1e-3,
                          device="cuda", flip=False, data="synthetic_fixed", seed=0, accum_steps=2, bucket_mb=4.0)
        st = make_strategy(cfg)
        Trainer(cfg, st)
        issued = st.mirror.comm.watchdog_state()["issued"] if strategy == "mirrored" else 0
        for img, lab in batches:
            st.train_step(img, lab)
        torch.cuda.synchronize()
        assert st.opt.iterations == 1
        grads[strategy] = st.engine.grads[:st.engine.L.n_trainable].clone()
        if strategy == "mirrored":
            assert st.mirror.comm is not None and st.mirror.graphs is None
            nb = len(st.mirror.buckets)
            assert nb >= 3
            assert st.mirror.comm.watchdog_state()["issued"] - issued == nb     # once per update, not per micro-step
    a, b = grads["mirrored"], grads["single"]
    assert b.norm() > 0
    assert ((a - b).norm() / b.norm()).item() < 1e-3
