"""The train-mode BatchNormalization kernels (csrc/kernels/bn.hip), one by one, against fp64.

  bn_apply       every form x relu x bits, at grids where lanes loop (two items in flight, a last
                 single item, lanes that stop an iteration earlier), bf16 and fp32 activations
  bn_bwd_reduce  every C / 8 (powers of two and not), forced and heuristic block caps, tiny and
                 ragged row counts; integer inputs, so the sums are exact whatever the atomics' order
  bn_stats       a three-layer table, training and eval mode, the zero-variance / clamp / count = 1 edges
  bn_bwd_apply   single and dual, in place and not, with and without a bias gradient, at a channel offset
  the chain      reduce -> apply against fp64 autograd of batch_norm(training=True)
  forward stats  the fp32 engine's bn_bwd_reduce(z, z, 0) -> bn_stats at |mean| >> sigma

Outputs start as the sentinel NaN pattern inside sentinel guards; accumulators start nonzero.
Scalars (eps, momentum) reach the reference as the fp32 values the kernels receive.
Elementwise bounds: fp32 |got - ref| <= k U S (S = sum of the |terms|), bf16 adds half a bf16 ulp,
2^(E - 9) with E from frexp(ref), and from frexp(k U S) where ref is exactly 0.

bn_bwd_reduce takes `bn_red_blocks` as a cap: the launcher asks for M / (8 RPI) blocks first
(RPI = 256 / (C / 8) rows per pass), so a short input (M = 3 under a cap of 7) runs as one block.
Blocks with no rows occur where the rows per block round up: C = 2048 at M = 601 (75 blocks of 9
rows, 8 of them empty) and M = 2049 (256 blocks, 28 empty), C = 1000 at M = 601 (one empty);
test_bn_bwd_reduce_exact asserts those counts, and the empty blocks must add exact zeros.

Forward statistics of the fp32 engine (test_forward_statistics_f32: M = 4096, C = 64, fp32 z,
bound (D + 4) U (mean^2 + sigma^2) / sigma^2 with D = 56), worst relative error observed on an MI355X:
  |mean| / sigma = 0    variance 2.12e-7 (0.06 of the bound), 1/sigma 1.21e-7
  |mean| / sigma = 3    variance 2.98e-6 (0.08 of the bound), 1/sigma 1.45e-6
  |mean| / sigma = 30   variance 3.54e-4 (0.11 of the bound), 1/sigma 1.77e-4
The bound holds at 30: the raw-sum form loses what the cancellation predicts and no more.
"""
import math
import struct

import pytest
import torch
import torch.nn.functional as F

from pddl.models.resnet50 import BN_EPS

from kernel_checks import ByteOut as Bits, Out, U, dev, rel64, table

pytestmark = pytest.mark.gpu

EPS = float(torch.tensor(BN_EPS, dtype=torch.float32))        # the values the kernels receive
MOM = float(torch.tensor(0.99, dtype=torch.float32))
ONE_MINUS_MOM = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(0.99, dtype=torch.float32))
DTYPES = [torch.bfloat16, torch.float32]
_STAT_FMT = "<8ifi"      # BnStatLayer: C, sum_off, sq_off, ch, gamma, beta, mm, mv, count, pad


def N():
    from pddl.ops.native import require_native
    return require_native()


@pytest.fixture
def knobs():
    nat = N()
    yield nat
    nat.set_variant("bn_apply_blocks", 0)
    nat.set_variant("bn_red_blocks", 0)


def gen(seed):
    return torch.Generator(device=dev).manual_seed(seed)


def randn(g, *shape, dtype=torch.float32, scale=1.0, shift=0.0):
    return (torch.randn(*shape, device=dev, generator=g) * scale + shift).to(dtype)


def randint(g, lo, hi, *shape, dtype=torch.float32):
    return torch.randint(lo, hi + 1, shape, device=dev, generator=g).to(dtype)


def signed(g, C, lo=0.5):
    """Per-channel factors of either sign, magnitude in [lo, lo + 1)."""
    v = torch.rand(C, device=dev, generator=g) + lo
    return v * (torch.randint(0, 2, (C,), device=dev, generator=g) * 2 - 1).float()


def tol_of(ref, S, dtype, k):
    t = k * U * S
    if dtype == torch.bfloat16:
        # half a bf16 ulp of the exact value, 2^(E - 9); where that value is 0 (every ReLU-clamped
        # element) frexp would allow 2^-9, so there it is half an ulp of the fp32 term, all the
        # rounding can see
        t = t + torch.pow(2.0, (torch.frexp(torch.where(ref == 0, t, ref))[1] - 9).double())
    return t


def check_close(got, ref, S, dtype, k, what):
    err = (got.double() - ref).abs()
    over = err - tol_of(ref, S, dtype, k)
    worst = over.max().item()
    assert worst <= 0.0, f"{what}: {int((over > 0).sum())} elements over the bound, worst by {worst:.3e}"


def pack_bits(y):
    M, C = y.shape
    w = (y.float() > 0).view(M, C // 8, 8).to(torch.int32)
    return (w << torch.arange(8, device=dev, dtype=torch.int32)).sum(-1).to(torch.uint8).reshape(-1)


def loop_rows(C, blocks):
    """Rows such that, with stride = blocks * 256 channel groups, the total is
    4 strides + stride / 2 + 3 C / 8 groups in whole rows: some lanes run two two-item iterations
    and a last single item, others stop one iteration earlier.  When that total is a multiple of
    the stride (every lane would do the same) a row is dropped.  At C = 2048 under one block a row is
    a whole stride, so there the 7 rows give every lane the same three two-item iterations and a
    last single item, and no lane stops earlier.  blocks = 0: the heuristic grid (512 blocks
    below 4M groups), a total between one and two strides."""
    cg = C // 8
    if blocks == 0:
        stride = 512 * 256
        return (stride + stride // 2) // cg + 3
    stride = blocks * 256
    M = (4 * stride + stride // 2 + 3 * cg) // cg
    if (M * cg) % stride == 0 and stride > cg:
        M -= 1
    return M


# ------------------------------------------------------------------------------ bn_apply
@pytest.mark.parametrize("blocks", [1, 3, 0])
@pytest.mark.parametrize("C", [8, 64, 256, 2048])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_bn_apply_forms(knobs, dtype, C, blocks):
    """y = act(z a + b (+ r | + r a2 + b2)) and its ReLU bitmask, every form x relu x bits."""
    nat = knobs
    nat.set_variant("bn_apply_blocks", blocks)
    M = loop_rows(C, blocks)
    g = gen(100 + C + blocks)
    z = randn(g, M, C, dtype=dtype, scale=2.0, shift=0.7)
    r = randn(g, M, C, dtype=dtype)
    a, a2 = signed(g, C), signed(g, C)
    b, b2 = randn(g, C), randn(g, C)
    zd, rd, ad, bd, a2d, b2d = (t.double() for t in (z, r, a, b, a2, b2))
    base, base_s = zd * ad + bd, (zd * ad).abs() + bd.abs()
    forms = {
        "plain": (None, None, None, base, base_s),
        "res": (r, None, None, base + rd, base_s + rd.abs()),
        "proj": (r, a2, b2, base + (rd * a2d + b2d), base_s + (rd * a2d).abs() + b2d.abs()),
    }
    for form, (rr, aa2, bb2, pre, S) in forms.items():
        for relu in (True, False):
            ref = pre.clamp_min(0.0) if relu else pre
            for with_bits in (True, False):
                what = f"bn_apply {form} relu={relu} bits={with_bits} M={M} C={C}"
                y = Out(M * C, dtype)
                bt = Bits(M * C // 8)
                nat.bn_apply(z, a, b, rr, aa2, bb2, relu, y.t.view(M, C), bt.t if with_bits else None)
                y.check(what)
                bt.check(what)
                yv = y.t.view(M, C)
                check_close(yv, ref, S, dtype, 8, what)
                if with_bits:
                    assert torch.equal(bt.t, pack_bits(yv)), f"{what}: bits != packed (stored y > 0)"
                else:
                    assert bool((bt.t == 0xA5).all()), f"{what}: bits written without a bits buffer"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_bn_apply_rejects_c24(dtype):
    z = torch.zeros(4, 24, dtype=dtype, device=dev)
    a = torch.ones(24, device=dev)
    with pytest.raises(RuntimeError, match="bn_apply: C/8 must divide 256"):
        N().bn_apply(z, a, a, None, None, None, True, torch.empty_like(z), None)


# ------------------------------------------------------------------------- bn_bwd_reduce
def red_launch(M, C, cap):
    """The launch shape bn_bwd_reduce takes: (RPI, blocks, rows per block)."""
    rpi = 256 // (C // 8)
    nb = M // (rpi * 8)
    lim = cap if cap > 0 else (512 if M * C > (1 << 27) else 256)
    nb = max(1, min(nb, lim))
    return rpi, nb, (M + nb - 1) // nb


def red_rows(C):
    rpi = 256 // (C // 8)
    rows = {1, 3, max(1, rpi - 1), 2 * rpi + 1, 601}
    if C <= 64:
        rows.add(4999)   # the short rows of a narrow layer reach several blocks only here
    if C == 2048:
        rows.add(2049)   # 256 blocks of 9 rows: the last 28 blocks start past the last row
    return sorted(rows)


def surplus_blocks(M, C, cap):
    """Blocks of the launch whose row range is empty: they must add exact zeros."""
    _, nb, rows_per = red_launch(M, C, cap)
    return sum(1 for b in range(nb) if b * rows_per >= M)


@pytest.mark.parametrize("C", [8, 24, 64, 320, 1000, 2048])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_bn_bwd_reduce_exact(knobs, dtype, C):
    """Small-integer inputs: every partial sum is an integer below 2^24, so sg / sgx (/ sg2 / sgx2)
    must receive exactly the fp64 sums on top of their nonzero starting values."""
    nat = knobs
    g_ = gen(200 + C)
    mean = randint(g_, -2, 2, C)
    mean2 = mean + 1.0 + randint(g_, 0, 1, C)          # differs from mean in every channel
    start = [randint(g_, -9, 9, C) + 0.5 for _ in range(4)]
    zero = torch.zeros(C, device=dev)
    if C == 2048:   # the launches with more blocks than rows' worth of work
        assert surplus_blocks(2049, C, 0) == 28 and surplus_blocks(601, C, 0) == 8
    if C == 1000:
        assert surplus_blocks(601, C, 0) == 1
    for M in red_rows(C):
        g = randint(g_, -3, 3, M, C, dtype=dtype)
        z = randint(g_, -4, 4, M, C, dtype=dtype)
        z2 = randint(g_, -4, 4, M, C, dtype=dtype)
        gd, zd, z2d = g.double(), z.double(), z2.double()
        want_sg, want_sgx = gd.sum(0), (gd * (zd - mean.double())).sum(0)
        want_sgx2 = (gd * (z2d - mean2.double())).sum(0)
        want_s, want_q = zd.sum(0), (zd * zd).sum(0)
        for cap in (1, 3, 7, 0):
            nat.set_variant("bn_red_blocks", cap)
            for mode in ("single", "dual", "fwd_stats"):
                what = f"bn_bwd_reduce {mode} M={M} C={C} cap={cap}"
                o = [Out(C, torch.float32, s) for s in start]
                if mode == "single":
                    nat.bn_bwd_reduce(g, z, None, mean, None, o[0].t, o[1].t, None, None)
                    want = [want_sg, want_sgx, None, None]
                elif mode == "dual":
                    nat.bn_bwd_reduce(g, z, z2, mean, mean2, o[0].t, o[1].t, o[2].t, o[3].t)
                    want = [want_sg, want_sgx, want_sg, want_sgx2]
                else:   # the fp32 engine's forward statistics: g and z the same tensor, zero mean
                    nat.bn_bwd_reduce(z, z, None, zero, None, o[0].t, o[1].t, None, None)
                    want = [want_s, want_q, None, None]
                for k, (oo, w, s) in enumerate(zip(o, want, start)):
                    oo.check(f"{what} [{k}]")
                    inc = oo.t.double() - s.double()
                    if w is None:
                        assert bool((inc == 0).all()), f"{what}: accumulator {k} touched"
                    else:
                        assert torch.equal(inc, w), \
                            f"{what}: accumulator {k} off by up to {(inc - w).abs().max().item()}"


@pytest.mark.parametrize("C,M,cap", [(64, 601, 0), (320, 601, 3), (1000, 257, 7), (2048, 601, 0)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_bn_bwd_reduce_real(knobs, dtype, C, M, cap):
    """Real-valued inputs: the worst-case fp32 bound (D + 2) U sum|term| per channel, D the longest
    addition chain of the launch: ceil(rows per block / RPI) in a lane, RPI folds, one atomic per
    block (the starting value is one more term)."""
    nat = knobs
    nat.set_variant("bn_red_blocks", cap)
    rpi, nb, rows_per = red_launch(M, C, cap)
    D = math.ceil(rows_per / rpi) + rpi + nb
    g_ = gen(300 + C)
    g, z, z2 = randn(g_, M, C, dtype=dtype), randn(g_, M, C, dtype=dtype, scale=2.0, shift=0.7), \
        randn(g_, M, C, dtype=dtype, scale=3.0, shift=-0.4)
    mean, mean2 = randn(g_, C, shift=0.7), randn(g_, C, shift=-0.4)
    start = [randn(g_, C, scale=5.0) for _ in range(4)]
    o = [Out(C, torch.float32, s) for s in start]
    nat.bn_bwd_reduce(g, z, z2, mean, mean2, o[0].t, o[1].t, o[2].t, o[3].t)
    gd = g.double()
    t1, t2 = gd * (z.double() - mean.double()), gd * (z2.double() - mean2.double())
    for k, (oo, terms, s) in enumerate(zip(o, (gd, t1, gd, t2), start)):
        oo.check(f"bn_bwd_reduce real [{k}]")
        err = (oo.t.double() - (s.double() + terms.sum(0))).abs()
        bound = (D + 2) * U * (s.double().abs() + terms.abs().sum(0))
        print(f"bn_bwd_reduce real C={C} M={M} blocks={nb} D={D} [{k}]: worst err / bound "
              f"{(err / bound).max().item():.3f}")
        assert bool((err <= bound).all()), f"accumulator {k}: {(err / bound).max().item():.2f} x the bound"


# ------------------------------------------------------------------------------ bn_stats
def _stats_case(seed=400):
    """Three layers (C = 8 at count 1, C = 64, C = 2048) with their own channel, accumulator and
    parameter offsets; hand-made accumulator rows for the edges."""
    g_ = gen(seed)
    lay, off_p, off_c, off_a = [], 8, 0, 8
    for C, count in ((8, 1.0), (64, 1000.0), (2048, 3136.0)):
        gamma, beta, mm, mv = (off_p + i * (C + 8) for i in range(4))
        off_p += 4 * (C + 8)
        lay.append(dict(C=C, count=count, ch=off_c + 8, s=off_a, q=off_a + C + 8, gamma=gamma, beta=beta, mm=mm,
                        mv=mv))
        off_c += C + 16
        off_a += 2 * (C + 8)
    prm = randn(g_, off_p + 8)
    acc = randn(g_, off_a + 8)
    for l in lay:
        C, n = l["C"], l["count"]
        mu = randn(g_, C, scale=1.5)
        var = torch.rand(C, device=dev, generator=g_) + 0.25
        if n == 1.0:   # one row: S = z, Q = z^2 with z an integer, the variance is exactly 0
            mu, var = randint(g_, -4, 4, C), torch.zeros(C, device=dev)
        acc[l["s"]:l["s"] + C] = (mu.double() * n).float()
        acc[l["q"]:l["q"] + C] = ((var.double() + mu.double() ** 2) * n).float()
        prm[l["mv"]:l["mv"] + C] = torch.rand(C, device=dev, generator=g_) + 0.5
        prm[l["gamma"]:l["gamma"] + C] = signed(g_, C)
    l = lay[1]      # n = 1000
    # channel 0: a constant channel (z = 1.5): var exactly 0, 1/sigma = rsqrt(eps)
    acc[l["s"] + 0], acc[l["q"] + 0] = 1500.0, 2250.0
    # channel 1: Q a hair below n m^2: the clamp applies; its moving variance starts at 0 and must stay 0
    acc[l["s"] + 1] = 1500.0
    acc[l["q"] + 1] = torch.nextafter(torch.tensor(2250.0), torch.tensor(0.0)).item()
    prm[l["mv"] + 1] = 0.0
    tab = table([struct.pack(_STAT_FMT, l["C"], l["s"], l["q"], l["ch"], l["gamma"], l["beta"], l["mm"], l["mv"],
                             l["count"], 0) for l in lay])
    return lay, prm, acc, tab, off_c + 8


def _stats_check(lay, prm0, mu, var, outs, what):
    """mean, 1/sigma, scale, shift of every layer from (mu, var) in fp64, per-term U bounds:
    1/sigma = rsqrtf(fl(var) + eps) carries the rounding of var, of the sum and ~2 U of rsqrtf."""
    mean, inv, scale, shift = outs
    owned = torch.zeros(mean.n, dtype=torch.bool, device=dev)
    for l in lay:
        C, sl = l["C"], slice(l["ch"], l["ch"] + l["C"])
        owned[sl] = True
        m, v = mu[l["name"]], var[l["name"]]
        gam, bet = prm0[l["gamma"]:l["gamma"] + C].double(), prm0[l["beta"]:l["beta"] + C].double()
        is_ = 1.0 / torch.sqrt(v + EPS)
        a = gam * is_
        for name, got, ref, bound in (("mean", mean, m, 2 * U * m.abs()), ("inv", inv, is_, 4 * U * is_),
                                      ("scale", scale, a, 6 * U * a.abs()),
                                      ("shift", shift, bet - m * a, 8 * U * (bet.abs() + (m * a).abs()))):
            err = (got.t[sl].double() - ref).abs()
            assert bool((err <= bound).all()), \
                f"{what} C={C} {name}: {(err / (bound + 1e-300)).max().item():.2f} x the bound"
    for o in outs:
        o.check(what, owned)


def test_bn_stats_training():
    nat = N()
    lay, prm, acc, tab, nch = _stats_case()
    prm0 = prm.clone()
    outs = [Out(nch, torch.float32) for _ in range(4)]
    nat.bn_stats(acc, tab, 3, 2048, True, prm, *(o.t for o in outs), EPS, MOM)
    mu, var, changed = {}, {}, torch.zeros(prm.numel(), dtype=torch.bool, device=dev)
    for i, l in enumerate(lay):
        l["name"] = i
        C, n = l["C"], l["count"]
        S, Q = acc[l["s"]:l["s"] + C].double(), acc[l["q"]:l["q"] + C].double()
        m = S / n
        v = (Q / n - m * m).clamp_min(0.0)
        mu[i], var[i] = m, v
        vu = v * n / (n - 1.0 if n > 1.0 else 1.0)     # Bessel-corrected; count = 1 divides by 1
        for off, new in ((l["mm"], m), (l["mv"], vu)):
            old = prm0[off:off + C].double()
            ref, S_ = old * MOM + ONE_MINUS_MOM * new, (old * MOM).abs() + (ONE_MINUS_MOM * new).abs()
            err = (prm[off:off + C].double() - ref).abs()
            assert bool((err <= 4 * U * S_).all()), \
                f"moving statistic C={C}: {(err / (4 * U * S_ + 1e-300)).max().item():.2f} x the bound"
            changed[off:off + C] = True
    _stats_check(lay, prm0, mu, var, outs, "bn_stats training")
    assert torch.equal(prm.view(torch.int32)[~changed], prm0.view(torch.int32)[~changed]), "params touched"
    l = lay[1]
    rs = 1.0 / math.sqrt(EPS)
    for c in (0, 1):    # zero and clamped variance: 1/sigma = rsqrt(eps)
        assert abs(outs[1].t[l["ch"] + c].item() - rs) <= 4 * U * rs
    assert prm[l["mv"] + 1].item() == 0.0, "a clamped variance moved a zero moving variance"


def test_bn_stats_eval():
    nat = N()
    lay, prm, acc, tab, nch = _stats_case(seed=401)
    prm0 = prm.clone()
    outs = [Out(nch, torch.float32) for _ in range(4)]
    nat.bn_stats(acc, tab, 3, 2048, False, prm, *(o.t for o in outs), EPS, MOM)
    mu, var = {}, {}
    for i, l in enumerate(lay):
        l["name"] = i
        mu[i] = prm0[l["mm"]:l["mm"] + l["C"]].double()
        var[i] = prm0[l["mv"]:l["mv"] + l["C"]].double()
    _stats_check(lay, prm0, mu, var, outs, "bn_stats eval")
    assert torch.equal(prm.view(torch.int32), prm0.view(torch.int32)), "eval-mode bn_stats wrote params"


# -------------------------------------------------------------------------- bn_bwd_apply
def _bwd_apply_ref(g, z, gamma, inv, mean, sg, sgx, M):
    """fp64 (A, B, C), dz and parameter gradients of one layer, with the magnitudes their bounds use."""
    gd, zd = g.double(), z.double()
    gam, is_, mu, s0, s1 = (t.double() for t in (gamma, inv, mean, sg, sgx))
    A = gam * is_
    B = -A * is_ * is_ * s1 / M
    t1, t2 = A * s0 / M, B * mu
    return dict(A=A, B=B, C=-t1 - t2, Cs=t1.abs() + t2.abs(), dgamma=s1 * is_, dbeta=s0,
                dz=A * gd + B * zd + (-t1 - t2), S=(A * gd).abs() + (B * zd).abs() + t1.abs() + t2.abs())


def _bwd_apply_check_layer(R, layer, out, coef, grads, ldc, own_c, own_g, dtype, what):
    """One layer's coef rows, dz and gradients against its reference R; marks what the layer owns
    in coef / grads.  layer = [C, ch, gamma_off, beta_off, bias_off, M]."""
    C, ch, o_gamma, o_beta, o_bias, M = layer
    for k, (name, bnd) in enumerate((("A", 8 * U * R["A"].abs()), ("B", 8 * U * R["B"].abs()),
                                     ("C", 8 * U * R["Cs"]))):     # C's bound includes its cancellation
        sl = slice(k * ldc + ch, k * ldc + ch + C)
        own_c[sl] = True
        err = (coef.t[sl].double() - R[name]).abs()
        assert bool((err <= bnd).all()), f"{what} coef {name}: {(err / (bnd + 1e-300)).max().item():.2f} x the bound"
    check_close(out.t.view(M, C), R["dz"], R["S"], dtype, 16, f"{what} dz")
    dgamma, dbeta = grads.t[o_gamma:o_gamma + C], grads.t[o_beta:o_beta + C]
    own_g[o_gamma:o_gamma + C] = True
    own_g[o_beta:o_beta + C] = True
    assert bool(((dgamma.double() - R["dgamma"]).abs() <= 4 * U * R["dgamma"].abs()).all()), f"{what} dgamma"
    assert torch.equal(dbeta.double(), R["dbeta"]), f"{what} dbeta"
    if o_bias >= 0:
        own_g[o_bias:o_bias + C] = True
        assert bool((grads.t[o_bias:o_bias + C] == 0).all()), f"{what} dbias"


def _bwd_apply_case(nat, dtype, g, z, z2, refs, dual, alias, bias, ch, arrays, offs, ldc):
    """One launch: dz / dz2 separate or over g (alias), bias gradient or bias_off = -1."""
    prm, mean, inv, sg, sgx = arrays
    M, C = g.shape
    what = f"bn_bwd_apply dual={dual} alias={alias} bias={bias} ch={ch} M={M} C={C}"
    gin = Out(M * C, dtype, g)                  # g lives in guards too: it may be an output
    dz = gin if alias == "dz" else Out(M * C, dtype)
    dz2 = None if not dual else (gin if alias == "dz2" else Out(M * C, dtype))
    coef, grads = Out(3 * ldc, torch.float32), Out(prm.numel(), torch.float32)
    l1 = [C, ch, offs[0], offs[1], offs[2] if bias else -1, M]
    l2 = [C, ch + C, offs[3], offs[4], offs[5] if bias else -1, M]
    nat.bn_bwd_apply(gin.t.view(M, C), z, z2 if dual else None, l1, l2 if dual else [], prm, mean, inv, sg, sgx,
                     dz.t.view(M, C), dz2.t.view(M, C) if dual else None, grads.t, coef.t)
    own_c = torch.zeros(3 * ldc, dtype=torch.bool, device=dev)
    own_g = torch.zeros(prm.numel(), dtype=torch.bool, device=dev)
    _bwd_apply_check_layer(refs[0], l1, dz, coef, grads, ldc, own_c, own_g, dtype, what + " layer 1")
    if dual:
        _bwd_apply_check_layer(refs[1], l2, dz2, coef, grads, ldc, own_c, own_g, dtype, what + " layer 2")
    coef.check(what, own_c)
    grads.check(what, own_g)   # bias_off = -1: nothing beyond gamma / beta is written
    for o in {id(x): x for x in (gin, dz, dz2) if x is not None}.values():
        o.check(what)
    if alias == "none":
        iv = torch.int16 if dtype == torch.bfloat16 else torch.int32
        assert torch.equal(gin.t.view(iv), g.reshape(-1).view(iv)), f"{what}: g changed"


@pytest.mark.parametrize("blocks", [1, 3, 0])
@pytest.mark.parametrize("C", [8, 64, 256, 2048])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_bn_bwd_apply_forms(knobs, dtype, C, blocks):
    """coef (A, B, C), dz / dz2 and the parameter gradients: single and dual, separate outputs and
    in place over g, with and without a bias gradient, at channel offsets 0 and 64."""
    nat = knobs
    nat.set_variant("bn_apply_blocks", blocks)
    M = loop_rows(C, blocks)
    g_ = gen(500 + C + blocks)
    g = randn(g_, M, C, dtype=dtype)
    z = randn(g_, M, C, dtype=dtype, scale=2.0, shift=0.7)
    z2 = randn(g_, M, C, dtype=dtype, scale=3.0, shift=-0.4)
    for ch in (0, 64):
        nch = ch + 2 * C + 8                    # per-channel arrays: layer 1 at ch, layer 2 at ch + C
        ldc = nch + 12                          # coef rows wider than the channel count
        mean, sg, sgx = randn(g_, nch), randn(g_, nch, scale=30.0), randn(g_, nch, scale=30.0)
        inv = torch.rand(nch, device=dev, generator=g_) + 0.5
        offs = [8 + i * (C + 8) for i in range(6)]   # gamma1 beta1 bias1 gamma2 beta2 bias2
        prm = randn(g_, 8 + 6 * (C + 8))
        refs = []
        for zz, c0, o_gamma in ((z, ch, offs[0]), (z2, ch + C, offs[3])):
            prm[o_gamma:o_gamma + C] = signed(g_, C)
            sl = slice(c0, c0 + C)
            refs.append(_bwd_apply_ref(g, zz, prm[o_gamma:o_gamma + C], inv[sl], mean[sl], sg[sl], sgx[sl], M))
        for dual in (False, True):
            for alias in (("none", "dz", "dz2") if dual else ("none", "dz")):
                for bias in (True, False):
                    _bwd_apply_case(nat, dtype, g, z, z2, refs, dual, alias, bias, ch, (prm, mean, inv, sg, sgx),
                                    offs, ldc)


# ------------------------------------------------------------------ chain against autograd
# The fp32 chain has no project tolerance: the same formulas evaluated in torch fp32 (on a CPU, the
# inputs of _chain_inputs, _chain_f32_formulas below) against fp64 autograd measured, norm-relative,
# for plain 1500 x 64 | proj 700 x 256 (BN3) | proj (BN0):
#   dz 6.01e-8 | 5.50e-8 | 5.60e-8, dgamma 1.27e-7 | 1.28e-7 | 1.25e-7, dbeta 1.21e-7 | 1.14e-7 | 1.14e-7
# The kernels get 4 x the largest of each, for their different summation order.
CHAIN_F32_MEASURED = {"dz": 6.01e-8, "dgamma": 1.28e-7, "dbeta": 1.21e-7}
CHAIN_TOL = {torch.bfloat16: {"dz": 2e-2, "dgamma": 1e-2, "dbeta": 1e-2},
             torch.float32: {k: 4 * v for k, v in CHAIN_F32_MEASURED.items()}}


def _chain_inputs(M, C, dtype, seed):
    g_ = torch.Generator().manual_seed(seed)   # host generator: the same inputs wherever measured

    def rn(*s, scale=1.0, shift=0.0):
        return (torch.randn(*s, generator=g_) * scale + shift).to(dtype)
    g, z, z0 = rn(M, C), rn(M, C, scale=2.0, shift=0.7), rn(M, C, scale=3.0, shift=-0.4)
    gamma = torch.rand(2 * C, generator=g_) + 0.5
    return g, z, z0, gamma


def _chain_stats(z):
    zd = z.double()
    return zd.mean(0).float(), torch.rsqrt(zd.var(0, unbiased=False) + EPS).float()


def _chain_autograd(g, z, gamma):
    zz = z.double().clone().requires_grad_(True)
    ga = gamma.double().clone().requires_grad_(True)
    be = torch.zeros_like(ga, requires_grad=True)
    F.batch_norm(zz, None, None, ga, be, training=True, eps=EPS).backward(g.double())
    return {"dz": zz.grad, "dgamma": ga.grad, "dbeta": be.grad}


def _chain_f32_formulas(g, z, gamma, mean, inv):
    """What the two kernels compute, in plain torch fp32 (the measurement behind CHAIN_F32_MEASURED)."""
    M = z.shape[0]
    g, z = g.float(), z.float()
    sg, sgx = g.sum(0), (g * (z - mean)).sum(0)
    A = gamma * inv
    B = -A * inv * inv * sgx / M
    return {"dz": A * g + B * z + (-A * sg / M - B * mean), "dgamma": sgx * inv, "dbeta": sg}


@pytest.mark.parametrize("proj", [False, True], ids=["plain", "proj"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_bn_bwd_chain_vs_autograd(dtype, proj):
    nat = N()
    M, C = (700, 256) if proj else (1500, 64)
    g, z, z0, gamma = (t.to(dev) for t in _chain_inputs(M, C, dtype, 7 + proj))
    tol = CHAIN_TOL[dtype]
    mean, inv = torch.zeros(2 * C, device=dev), torch.ones(2 * C, device=dev)
    mean[:C], inv[:C] = _chain_stats(z)
    mean[C:], inv[C:] = _chain_stats(z0)
    sg, sgx = torch.zeros(2 * C, device=dev), torch.zeros(2 * C, device=dev)
    grads, coef = torch.zeros(6 * C, device=dev), torch.zeros(6 * C, device=dev)
    prm = torch.cat([gamma, torch.zeros(4 * C, device=dev)])    # gamma3 | gamma0 | ...
    dz_o, dz0_o = Out(M * C, dtype), Out(M * C, dtype)
    dz, dz0 = dz_o.t.view(M, C), dz0_o.t.view(M, C)
    if proj:
        nat.bn_bwd_reduce(g, z, z0, mean[:C], mean[C:], sg[:C], sgx[:C], sg[C:], sgx[C:])
        nat.bn_bwd_apply(g, z, z0, [C, 0, 0, 2 * C, 4 * C, M], [C, C, C, 3 * C, 5 * C, M], prm, mean, inv, sg, sgx,
                         dz, dz0, grads, coef)
    else:
        nat.bn_bwd_reduce(g, z, None, mean[:C], None, sg[:C], sgx[:C], None, None)
        nat.bn_bwd_apply(g, z, None, [C, 0, 0, 2 * C, 4 * C, M], [], prm, mean, inv, sg, sgx, dz, None, grads, coef)
    dz_o.check("chain dz")
    dz0_o.check("chain dz0", None if proj else torch.zeros(M * C, dtype=torch.bool, device=dev))
    for zi, dzi, off in ((z, dz, 0), (z0, dz0, C)) if proj else ((z, dz, 0),):
        want = _chain_autograd(g, zi, gamma[off:off + C])
        got = {"dz": dzi, "dgamma": grads[off:off + C], "dbeta": grads[2 * C + off:2 * C + off + C]}
        for k in ("dz", "dgamma", "dbeta"):
            e = rel64(got[k], want[k])
            print(f"chain {'proj' if proj else 'plain'} off={off} {k}: {e:.3e} (tolerance {tol[k]:.1e})")
            assert e <= tol[k], f"{k} at offset {off}: {e:.3e} > {tol[k]:.1e}"


# ------------------------------------------------- forward statistics of the fp32 engine
@pytest.mark.parametrize("ratio", [0, 3, 30])
def test_forward_statistics_f32(ratio):
    """The fp32 train-BN engine's batch statistics: bn_bwd_reduce(z, z, mean = 0) accumulates raw
    sum z and sum z^2 in fp32, bn_stats subtracts in double.  Relative error of the variance
    <= (D + 4) U (mean^2 + sigma^2) / sigma^2, of 1/sigma half that (M = 4096, C = 64: 16 blocks
    of 256 rows, RPI = 32, D = 8 + 32 + 16 = 56).  The observed errors are in the module docstring."""
    nat = N()
    M, C = 4096, 64
    rpi, nb, rows_per = red_launch(M, C, 0)
    D = math.ceil(rows_per / rpi) + rpi + nb
    assert D == 56
    g_ = gen(600 + ratio)
    sigma = torch.rand(C, device=dev, generator=g_) + 0.5
    sign = (torch.randint(0, 2, (C,), device=dev, generator=g_) * 2 - 1).float()
    z = torch.randn(M, C, device=dev, generator=g_) * sigma + ratio * sigma * sign
    acc = torch.zeros(2 * C, device=dev)
    nat.bn_bwd_reduce(z, z, None, torch.zeros(C, device=dev), None, acc[:C], acc[C:], None, None)
    prm = torch.zeros(4 * C, device=dev)
    prm[:C] = 1.0
    outs = [Out(C, torch.float32) for _ in range(4)]
    tab = table([struct.pack(_STAT_FMT, C, 0, C, 0, 0, C, 2 * C, 3 * C, float(M), 0)])
    # momentum 0: the moving variance becomes the batch variance times M / (M - 1)
    nat.bn_stats(acc, tab, 1, C, True, prm, *(o.t for o in outs), EPS, 0.0)
    zd = z.double()
    m, v = zd.mean(0), zd.var(0, unbiased=False)
    bound = (D + 4) * U * (m * m + v) / v
    got_v = prm[3 * C:].double() * (M - 1) / M
    e_v = (got_v - v).abs() / v
    is_ = 1.0 / torch.sqrt(v + EPS)
    e_i = (outs[1].t.double() - is_).abs() / is_
    print(f"forward statistics |mean|/sigma={ratio}: variance {(e_v / bound).max().item():.3f}, "
          f"1/sigma {(e_i / (bound / 2)).max().item():.3f} of the bound (worst rel. err {e_v.max().item():.2e}, "
          f"{e_i.max().item():.2e})")
    assert bool((e_v <= bound).all()), f"variance: {(e_v / bound).max().item():.2f} x the bound"
    assert bool((e_i <= bound / 2).all()), f"1/sigma: {(e_i / (bound / 2)).max().item():.2f} x the bound"
