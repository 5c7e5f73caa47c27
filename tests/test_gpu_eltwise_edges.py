"""Edge shapes of the pooling, column-sum and loss kernels (csrc/kernels/f32.hip and the pool /
GAP / colsum / softmax_xent part of csrc/kernels/eltwise.hip) against fp64 / exact references.

  max-pool   non-square and degenerate images, negative inputs (a zero pad tap wins and its
             gradient is dropped), integer inputs with many ties (first tap in scan order), the
             grid-stride wrap of the fp32 kernels, the bf16 per-output forms under a small
             `pool_blocks` (loops, column sums spanning iterations) and the streaming forms
  GAP        HW = 1 and 49, narrow and wide C, gp as a column slice of wider rows (bf16; the
             fp32 kernel takes contiguous gp only), partial column-sum rows given or not
  colsum     every column-group count (ragged passes, idle lanes), ldg > C, rows around the
             per-block row count, the rebalanced grid
  softmax    ncls around the wave width, row strides wider than ncls with +inf pads, ties,
             labels at both ends, logits scaled so the max-subtraction matters

Outputs start as the sentinel NaN pattern (byte outputs as 0xA5) inside guards; accumulators
start nonzero.  Sums of small integers must be exact whatever the order of the atomics.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from kernel_checks import ByteOut, Out, U, dev, pack_bits, pool_bwd_ref, pool_ref, rel64

pytestmark = pytest.mark.gpu

SHAPES = [(2, 12, 9), (1, 13, 14), (3, 1, 5), (2, 2, 1)]     # (B, H, W)
F32_POOL_C = {(2, 12, 9): 4, (1, 13, 14): 12, (3, 1, 5): 64, (2, 2, 1): 8}


def N():
    from pddl.ops.native import require_native
    return require_native()


@pytest.fixture
def pool_blocks():
    nat = N()
    yield lambda v: nat.set_variant("pool_blocks", v)
    nat.set_variant("pool_blocks", 8192)


def gen(seed):
    return torch.Generator(device=dev).manual_seed(seed)


def randint(g, lo, hi, *shape, dtype=torch.float32):
    return torch.randint(lo, hi + 1, shape, device=dev, generator=g).to(dtype)


def osize(n):
    return (n - 1) // 2 + 1


def same_bits(a, b):
    v = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v))


# ------------------------------------------------------------------------------ max-pool
def pad_winner(tap, H, W):
    """Outputs whose winning tap lies in the zero padding."""
    B, Ho, Wo, C = tap.shape
    ho, wo = torch.arange(Ho, device=dev).view(1, Ho, 1, 1), torch.arange(Wo, device=dev).view(1, 1, Wo, 1)
    hi, wi = 2 * ho - 1 + tap // 3, 2 * wo - 1 + tap % 3
    return (hi < 0) | (hi >= H) | (wi < 0) | (wi >= W)


def pool_inputs(g, B, H, W, C, dtype, kind):
    if kind == "ties":      # few distinct integers, many negative: ties everywhere, pad zeros win
        return randint(g, -3, 2, B, H, W, C, dtype=dtype)
    return (torch.randn(B, H, W, C, device=dev, generator=g) - 0.5).to(dtype)


@pytest.mark.parametrize("kind", ["ties", "real"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_maxpool_f32_small(shape, kind):
    nat = N()
    B, H, W = shape
    C = F32_POOL_C[shape]
    Ho, Wo = osize(H), osize(W)
    g = gen(11 + H)
    x = pool_inputs(g, B, H, W, C, torch.float32, kind)
    y, idx = Out(B * Ho * Wo * C, torch.float32), ByteOut(B * Ho * Wo * C)
    nat.maxpool_fwd_f32(x, y.t.view(B, Ho, Wo, C), idx.t.view(B, Ho, Wo, C))
    y.check("maxpool_fwd_f32 y")
    idx.check("maxpool_fwd_f32 idx")
    best, tap = pool_ref(x)
    assert torch.equal(y.t.view(B, Ho, Wo, C).double(), best)
    assert torch.equal(idx.t.view(B, Ho, Wo, C), tap), "tap is not the first maximum in scan order"
    assert bool(pad_winner(tap, H, W).any()), "the case must let a zero pad tap win"
    if kind == "real":      # no ties: F.pad + max_pool2d says the same
        tref = F.max_pool2d(F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2)[:, :, :Ho, :Wo].permute(0, 2, 3, 1)
        assert torch.equal(y.t.view(B, Ho, Wo, C), tref.contiguous())
    gy = randint(g, -3, 3, B, Ho, Wo, C)
    xmask = torch.randn(B, H, W, C, device=dev, generator=g)
    gx = Out(B * H * W * C, torch.float32)
    nat.maxpool_bwd_f32(gy, idx.t.view(B, Ho, Wo, C), xmask, gx.t.view(B, H, W, C))
    gx.check("maxpool_bwd_f32 gx")
    assert torch.equal(gx.t.view(B, H, W, C).double(), pool_bwd_ref(gy, tap, xmask, H, W))
    if kind == "real":      # and autograd of F.pad + max_pool2d drops the pad taps' gradient likewise
        xr = x.clone().requires_grad_(True)
        F.max_pool2d(F.pad(xr.permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2)[:, :, :Ho, :Wo].backward(
            gy.permute(0, 3, 1, 2))
        assert torch.equal(gx.t.view(B, H, W, C), (xr.grad * (xmask > 0)).contiguous())


def test_maxpool_fwd_f32_grid_wrap():
    """1 x 129 x 129 x 4096: 65 * 65 * 1024 items, just past the 16384 x 256 lanes of the grid."""
    nat = N()
    B, H, W, C = 1, 129, 129, 4096
    Ho, Wo = osize(H), osize(W)
    assert Ho * Wo * C // 4 > 16384 * 256
    x = torch.randn(B, H, W, C, device=dev, generator=gen(21)) - 0.5
    y, idx = Out(B * Ho * Wo * C, torch.float32), ByteOut(B * Ho * Wo * C)
    nat.maxpool_fwd_f32(x, y.t.view(B, Ho, Wo, C), idx.t.view(B, Ho, Wo, C))
    y.check("maxpool_fwd_f32 wrap")
    idx.check("maxpool_fwd_f32 wrap idx")
    # torch pads with -inf: a window that touches the padding sees a real zero here
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, padding=1).permute(0, 2, 3, 1)
    ho, wo = torch.arange(Ho, device=dev).view(1, Ho, 1, 1), torch.arange(Wo, device=dev).view(1, 1, Wo, 1)
    border = (ho == 0) | (wo == 0) | (2 * ho + 1 >= H) | (2 * wo + 1 >= W)
    ref = torch.where(border, ref.clamp_min(0.0), ref)
    assert torch.equal(y.t.view(B, Ho, Wo, C), ref)
    assert int(idx.t.max()) <= 8, "an argmax tap was not written"


def test_maxpool_bwd_f32_grid_wrap():
    """1 x 65 x 65 x 4096 inputs: 65 * 65 * 1024 items, past the grid; any tap in 0..8 per output."""
    nat = N()
    B, H, W, C = 1, 65, 65, 4096
    Ho, Wo = osize(H), osize(W)
    assert H * W * C // 4 > 16384 * 256
    g = gen(22)
    gy = randint(g, -3, 3, B, Ho, Wo, C)
    tap = torch.randint(0, 9, (B, Ho, Wo, C), device=dev, generator=g).to(torch.uint8)
    xmask = torch.randn(B, H, W, C, device=dev, generator=g)
    gx = Out(B * H * W * C, torch.float32)
    nat.maxpool_bwd_f32(gy, tap, xmask, gx.t.view(B, H, W, C))
    gx.check("maxpool_bwd_f32 wrap")
    assert torch.equal(gx.t.view(B, H, W, C).double(), pool_bwd_ref(gy, tap, xmask, H, W))


BF16_POOL = [(s, c) for s in SHAPES for c in (8, 32, 512, 64, 128, 256)] + [((2, 23, 17), 8)]


@pytest.mark.parametrize("shape,C", BF16_POOL, ids=str)
def test_maxpool_bf16_forms(pool_blocks, shape, C):
    """The per-output forms (C = 8, 32, 512) under pool_blocks = 2, so that their grid-stride loops
    and per-thread column sums span iterations once an image has more than 512 items (the
    2 x 23 x 17 x 8 case is there for C = 8), and the streaming forms (C = 64, 128, 256)."""
    nat = N()
    pool_blocks(2)
    B, H, W = shape
    Ho, Wo = osize(H), osize(W)
    g = gen(31 + H + C)
    for kind in ("ties", "real"):
        x = pool_inputs(g, B, H, W, C, torch.bfloat16, kind)
        best, tap = pool_ref(x)
        for with_bits in (True, False):
            what = f"maxpool_fwd {shape} C={C} {kind} bits={with_bits}"
            y, idx, bt = Out(B * Ho * Wo * C, torch.bfloat16), ByteOut(B * Ho * Wo * C), ByteOut(B * Ho * Wo * C // 8)
            nat.maxpool_fwd(x, y.t.view(B, Ho, Wo, C), idx.t.view(B, Ho, Wo, C), bt.t if with_bits else None)
            for o in (y, idx, bt):
                o.check(what)
            assert torch.equal(y.t.view(B, Ho, Wo, C).double(), best), what
            assert torch.equal(idx.t.view(B, Ho, Wo, C), tap), f"{what}: tap is not the first maximum in scan order"
            if with_bits:
                assert torch.equal(bt.t, pack_bits(y.t)), f"{what}: bits != packed (y > 0)"
            else:
                assert bool((bt.t == 0xA5).all()), f"{what}: bits written without a bits buffer"
        gy = randint(g, -3, 3, B, Ho, Wo, C, dtype=torch.bfloat16)
        xmask = torch.randn(B, H, W, C, device=dev, generator=g).to(torch.bfloat16)
        rows = nat.maxpool_bwd_partial_rows(B, H, W, C)
        for xm in (xmask, None):
            want = pool_bwd_ref(gy, tap, xm, H, W)
            for with_cs in (True, False):
                what = f"maxpool_bwd {shape} C={C} {kind} xmask={xm is not None} colsum={with_cs}"
                gx, cs = Out(B * H * W * C, torch.bfloat16), Out(rows * C, torch.float32)
                nat.maxpool_bwd(gy, tap, xm, gx.t.view(B, H, W, C), cs.t if with_cs else None)
                gx.check(what)
                assert torch.equal(gx.t.view(B, H, W, C).double(), want), what
                if with_cs:
                    cs.check(what)
                    assert torch.equal(cs.t.view(rows, C).double().sum(0), want.sum((0, 1, 2))), \
                        f"{what}: partial rows do not sum to the column sums"
                else:
                    cs.check(what, torch.zeros(rows * C, dtype=torch.bool, device=dev))


def pool_colsum_chain(B, H, W, C, blocks):
    """Longest addition chain behind one partial column-sum row of maxpool_bwd: up to 4 routed
    gradients per input position, the positions a lane walks, the fold across the wave."""
    cg = C // 8
    fold = int(math.log2(64 // cg))
    if C in (64, 128, 256):     # streaming form: a lane walks (H + 1) / 2 row pairs of 2 x 2 positions
        return 4 + 4 * ((H + 1) // 2) + fold
    total = B * H * W * cg      # per-input-position form: grid-stride iterations of a lane
    grid = min((total + 255) // 256, blocks)
    return 4 + math.ceil(total / (grid * 256)) + fold


@pytest.mark.parametrize("shape,C", [((2, 12, 9), c) for c in (8, 32, 512, 64, 128, 256)] + [((2, 23, 17), 8)], ids=str)
def test_maxpool_bwd_colsum_real(pool_blocks, shape, C):
    """Real-valued gradients: the fused column sums against fp64 with the worst-case fp32 bound
    (D + 2) U sum|term| per channel, D from the launch shape (pool_colsum_chain; the partial rows
    themselves are added in fp64 here), and gx within half a bf16 ulp + 4 U S of the fp64 sum."""
    nat = N()
    pool_blocks(2)
    B, H, W = shape
    Ho, Wo = osize(H), osize(W)
    g = gen(35 + H + C)
    _, tap = pool_ref(pool_inputs(g, B, H, W, C, torch.bfloat16, "ties"))
    gy = (torch.randn(B, Ho, Wo, C, device=dev, generator=g) + 0.3).to(torch.bfloat16)
    xmask = torch.randn(B, H, W, C, device=dev, generator=g).to(torch.bfloat16)
    rows = nat.maxpool_bwd_partial_rows(B, H, W, C)
    D = pool_colsum_chain(B, H, W, C, 2)
    gx, cs = Out(B * H * W * C, torch.bfloat16), Out(rows * C, torch.float32)
    nat.maxpool_bwd(gy, tap, xmask, gx.t.view(B, H, W, C), cs.t)
    gx.check("maxpool_bwd real gx")
    cs.check("maxpool_bwd real colsum")
    want, mag = pool_bwd_ref(gy, tap, xmask, H, W), pool_bwd_ref(gy.abs(), tap, xmask, H, W)
    fp32 = 4 * U * mag
    half_ulp = torch.pow(2.0, (torch.frexp(torch.where(want == 0, fp32, want))[1] - 9).double())
    assert bool(((gx.t.view(B, H, W, C).double() - want).abs() <= half_ulp + fp32).all()), "gx"
    err = (cs.t.view(rows, C).double().sum(0) - want.sum((0, 1, 2))).abs()
    bound = (D + 2) * U * mag.sum((0, 1, 2))
    print(f"maxpool_bwd colsum real {shape} C={C} D={D}: worst err / bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all()), f"column sums {(err / bound).max().item():.2f} x the bound"


# ---------------------------------------------------------------------------------- GAP
GAP_CASES = [(d, hw, c) for d in (torch.float32, torch.bfloat16) for hw in (1, 49) for c in (4, 8, 2048)
             if not (d == torch.bfloat16 and c == 4)]      # the bf16 kernels move 8 channels per lane


@pytest.mark.parametrize("dtype,HW,C", GAP_CASES, ids=str)
def test_gap_edges(pool_blocks, dtype, HW, C):
    """Integer inputs: the forward sum is exact and y = fl(sum * fl(1 / HW)) (then to bf16), each
    backward element is fl(gp * fl(1 / HW)) under the mask; a partial column-sum row adds HW such
    values in a chain, bound (HW + 2) U sum|term|."""
    f32 = dtype == torch.float32
    nat = N()
    B = 3
    H, W = (1, 1) if HW == 1 else (7, 7)
    inv = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(HW), dtype=torch.float32))
    g_ = gen(41 + HW + C)
    for blocks in ((8192,) if f32 else (8192, 2)):     # (the fp32 kernels have a fixed grid cap)
        pool_blocks(blocks)
        x = randint(g_, -4, 4, B, H, W, C, dtype=dtype)
        y = Out(B * C, dtype)
        (nat.gap_fwd_f32 if f32 else nat.gap_fwd)(x, y.t.view(B, C))
        y.check("gap_fwd")
        want = (x.double().sum((1, 2)) * inv).float().to(dtype)
        assert same_bits(y.t.view(B, C), want), f"gap_fwd HW={HW} C={C}"
        ymask = torch.randn(B, H, W, C, device=dev, generator=g_).to(dtype)
        gpv = randint(g_, -3, 3, B, C, dtype=dtype)
        if f32:
            gp = gpv
        else:       # a column slice of wider rows; the rest is never read
            wide = torch.full((B, C + 16), float("inf"), dtype=dtype, device=dev)
            wide[:, 8:8 + C] = gpv
            gp = wide[:, 8:8 + C]
        o = torch.where(ymask.double() > 0, (gpv.double() * inv).float().double().view(B, 1, 1, C), 0.0)
        for with_rows in (True, False):
            what = f"gap_bwd HW={HW} C={C} rows={with_rows} pool_blocks={blocks}"
            gout, cs = Out(B * HW * C, dtype), Out(B * C, torch.float32)
            (nat.gap_bwd_f32 if f32 else nat.gap_bwd)(gp, ymask, gout.t.view(B, H, W, C), cs.t if with_rows else None)
            gout.check(what)
            assert same_bits(gout.t.view(B, H, W, C), o.float().to(dtype)), what
            if with_rows:
                cs.check(what)
                err = (cs.t.view(B, C).double() - o.sum((1, 2))).abs()
                assert bool((err <= (HW + 2) * U * o.abs().sum((1, 2))).all()), f"{what}: partial rows"
            else:
                cs.check(what, torch.zeros(B * C, dtype=torch.bool, device=dev))


# ------------------------------------------------------------------------------- colsum
def _colsum_case(fn, M, C, ldg, dtype, g_, what):
    buf = torch.full((M, ldg), float("inf"), dtype=dtype, device=dev)    # pad columns are never read
    buf[:, :C] = randint(g_, -3, 3, M, C, dtype=dtype)
    start = randint(g_, -9, 9, C) + 0.5
    out = Out(C, torch.float32, start)
    fn(buf, C, out)
    out.check(what)
    inc = out.t.double() - start.double()
    want = buf[:, :C].double().sum(0)
    assert torch.equal(inc, want), f"{what}: off by up to {(inc - want).abs().max().item()}"


@pytest.mark.parametrize("C,ldg", [(8, 8), (40, 40), (320, 320), (1000, 1000), (2048, 2048), (64, 96)])
def test_colsum_bf16_exact(C, ldg):
    nat, g_ = N(), gen(51 + C)
    for M in (1, 511, 513, 3000):
        _colsum_case(lambda b, c, o: nat.colsum(b[:, :c], c, o.t), M, C, ldg, torch.bfloat16, g_,
                     f"colsum M={M} C={C} ldg={ldg}")


def test_colsum_bf16_rebalanced_grid():
    """C = 8 (one column group per block column) with more than 4096 blocks of 512 rows: the
    launcher rebalances the rows per block.  Integer sums stay far below 2^24."""
    M = 512 * 4096 + 513
    _colsum_case(lambda b, c, o: N().colsum(b, c, o.t), M, 8, 8, torch.bfloat16, gen(52), f"colsum M={M} C=8")


@pytest.mark.parametrize("C,ldg", [(4, 4), (100, 100), (1000, 1000), (10, 10), (1001, 1001),
                                   (4, 8), (100, 104), (1000, 1024), (10, 13), (1001, 1004), (100, 102)])
def test_colsum_f32_exact(C, ldg):
    """Vector path (C % 4 == 0 and ldg % 4 == 0: 1, 25 and 250 column groups, C = 1000 ending on a
    ragged 64-group pass) and scalar path (any other C or row stride), ldg == C and ldg > C."""
    nat, g_ = N(), gen(53 + C + ldg)
    for M in (1, 255, 257, 3000):
        _colsum_case(lambda b, c, o: nat.colsum_f32(b, c, o.t), M, C, ldg, torch.float32, g_,
                     f"colsum_f32 M={M} C={C} ldg={ldg}")


def colsum_chain(M, C):
    """Longest addition chain of a bf16 colsum launch: rows of a lane, RL row lanes, row blocks."""
    G = C // 8
    CG = min(G, 32)
    RL, gx, rpb = 256 // CG, (G + CG - 1) // CG, 512
    gy = (M + rpb - 1) // rpb
    if gx * gy > 4096:
        gy = (4096 + gx - 1) // gx
        rpb = (M + gy - 1) // gy
        gy = (M + rpb - 1) // rpb
    return math.ceil(rpb / RL) + RL + gy


def colsum_f32_chain(M, C, ldg):
    """The same for colsum_f32: the scalar path adds a block's rows in one thread."""
    if C % 4 or ldg % 4:
        by = min((M + 255) // 256, 65535)
        return (M + by - 1) // by + by
    CG = min(C // 4, 64)
    RL, blocks = 256 // CG, min((M + 255) // 256, 2048)
    return math.ceil(((M + blocks - 1) // blocks) / RL) + RL + blocks


def _colsum_real(fn, M, C, ldg, dtype, D, seed, what):
    """Real-valued rows: (D + 2) U sum|term| per column, the nonzero starting value one of the terms."""
    g_ = gen(seed)
    buf = torch.full((M, ldg), float("inf"), dtype=dtype, device=dev)
    buf[:, :C] = (torch.randn(M, C, device=dev, generator=g_) * 2 + 0.5).to(dtype)
    start = torch.randn(C, device=dev, generator=g_) * 5
    out = Out(C, torch.float32, start)
    fn(buf, C, out)
    out.check(what)
    v = buf[:, :C].double()
    err = (out.t.double() - (start.double() + v.sum(0))).abs()
    bound = (D + 2) * U * (start.double().abs() + v.abs().sum(0))
    print(f"{what} D={D}: worst err / bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all()), f"{what}: {(err / bound).max().item():.2f} x the bound"


@pytest.mark.parametrize("C,ldg,M", [(1000, 1000, 3000), (64, 96, 513), (8, 8, 3000)])
def test_colsum_bf16_real(C, ldg, M):
    _colsum_real(lambda b, c, o: N().colsum(b[:, :c], c, o.t), M, C, ldg, torch.bfloat16, colsum_chain(M, C),
                 57 + C, f"colsum real M={M} C={C} ldg={ldg}")


@pytest.mark.parametrize("C,ldg,M", [(1000, 1000, 3000), (100, 104, 257), (1001, 1001, 3000), (100, 102, 257)])
def test_colsum_f32_real(C, ldg, M):
    """Vector path (C = 1000; C = 100 in rows of 104) and scalar path (C = 1001; C = 100 in rows of 102)."""
    _colsum_real(lambda b, c, o: N().colsum_f32(b, c, o.t), M, C, ldg, torch.float32, colsum_f32_chain(M, C, ldg),
                 59 + C + ldg, f"colsum_f32 real M={M} C={C} ldg={ldg}")


# --------------------------------------------------------------------------- softmax-xent
# Scale 1 keeps the project's numbers (tests/test_gpu_kernels.py, tests/test_gpu_f32.py): loss 1e-5
# relative, fp32 dlogits 1e-6 norm-relative.  Scale 30 has none: torch's own fp32 cross_entropy
# (on a CPU) against fp64 on the logits of _xent_inputs measured, as the largest over every
# (ncls, B) below: loss 5.65e-8 relative, gradient 4.28e-8 norm-relative, and elementwise 4.68e-6
# of S = (p + onehot) gscale (78.6 U; 33.9 U at scale 1).  The kernels get 8 x that, because
# __expf is the fast form.
# The loss is summed by one fp32 atomic per row, in an order that varies from launch to launch.
# Over 400 launches of every (ncls, B = 5 | 37) case on an MI355X the sums took up to 7 distinct
# values (the total of ~9.5e3 at B = 37 has an ulp of 1.0e-7 of itself) and the worst relative
# error was 3.56e-7 (softmax_xent) and 3.40e-7 (softmax_xent_f32) at scale 30, 0.79 of the
# 4.52e-7 allowed; 3.31e-7 and 2.72e-7 at scale 1.
XENT30_LOSS = 5.65e-8
XENT30_GRAD = 4.28e-8
XENT30_ELEM = 4.68e-6
# The fp32 term of the bf16 dlogits bound at scale 1, in units of U S.  Derived, not measured:
# |x - max| <= 32 feeds exp with an absolute error of up to 32 U, the sum of ncls <= 1000 terms
# over 64 lanes and 6 shuffles adds 22 U, __expf, the division and the two products a few more.
# (Next to it: torch's fp32 gradient measured 33.9 U S there; half a bf16 ulp is 32768 U |ref|.)
XENT1_ELEM = 64 * U
TINY = 2.0 ** -126    # fp32 results below the smallest normal may flush to zero
XENT_TOL = {1: (1e-5, 1e-6, XENT1_ELEM), 30: (8 * XENT30_LOSS, 8 * XENT30_GRAD, 8 * XENT30_ELEM)}
XENT_B = (1, 5, 37)


def _xent_inputs(ncls, B, scale):
    """Host generator: the same logits wherever the tolerances are measured.  Rows 1 and 2 (when
    there) carry an exact tie at the maximum, labelled with its first and its second index."""
    g_ = torch.Generator().manual_seed(1000 * ncls + 10 * B + scale)
    x = torch.randn(B, ncls, generator=g_) * 3 * scale
    lab = torch.randint(0, ncls, (B,), generator=g_)
    lab[0] = 0 if (B > 1 or scale == 1) else ncls - 1
    lab[-1] = ncls - 1 if B > 1 else lab[0]
    if B == 1:      # keep the single row's loss away from zero: its label is not the prediction
        x[0, lab[0]] = x[0].min() - 1.0
    first, second = ncls // 3, ncls - 2
    for row, which in ((1, first), (2, second)):
        if row < B - 1:
            x[row, first] = x[row, second] = x[row].max() + 1.0
            lab[row] = which
    return x, lab


def _xent_ref(x, lab, gscale):
    xd = x.double()
    lse = torch.logsumexp(xd, 1)
    p = torch.softmax(xd, 1)
    onehot = F.one_hot(lab, x.shape[1]).double()
    j = torch.arange(x.shape[1], device=x.device).expand_as(xd)
    pred = torch.where(xd == xd.max(1, keepdim=True).values, j, x.shape[1]).min(1).values
    return (lse - xd.gather(1, lab.view(-1, 1)).view(-1)).sum().item(), (p - onehot) * gscale, \
        (p + onehot) * abs(gscale), int((pred == lab).sum())


@pytest.mark.parametrize("ncls", [10, 64, 65, 1000])
@pytest.mark.parametrize("kernel", ["softmax_xent", "softmax_xent_f32"])
def test_softmax_xent_edges(kernel, ncls):
    nat = N()
    fn = getattr(nat, kernel)
    dtype = torch.bfloat16 if kernel == "softmax_xent" else torch.float32
    for scale in (1, 30):
        tol_loss, tol_grad, tol_elem = XENT_TOL[scale]
        for B in XENT_B:
            x, lab = (t.to(dev) for t in _xent_inputs(ncls, B, scale))
            gscale = float(torch.tensor(1.0 / B, dtype=torch.float32))
            loss, dref, S, ncorrect = _xent_ref(x, lab, gscale)
            for ldl in (ncls, 1024):
                logits = torch.full((B, ldl), float("inf"), device=dev)
                logits[:, :ncls] = x
                before = logits.clone()
                for ldd in (ncls, 1024):
                    what = f"{kernel} ncls={ncls} B={B} scale={scale} ldl={ldl} ldd={ldd}"
                    dl = Out(B * ldd, dtype)
                    ls, cr = Out(1, torch.float32, torch.tensor([3.0])), Out(1, torch.float32, torch.tensor([2.0]))
                    fn(logits, lab, ncls, gscale, dl.t.view(B, ldd), ls.t, cr.t)
                    for o in (dl, ls, cr):
                        o.check(what)
                    assert same_bits(logits, before), f"{what}: logits changed"
                    got = dl.t.view(B, ldd)
                    assert bool((got[:, ncls:] == 0).all()), f"{what}: pad columns of dlogits not zero"
                    assert cr.t.item() - 2.0 == ncorrect, f"{what}: correct {cr.t.item() - 2.0} != {ncorrect}"
                    e_loss = abs((ls.t.item() - 3.0) - loss) / loss
                    err = (got[:, :ncls].double() - dref).abs()
                    if dtype == torch.float32:
                        e_grad = rel64(got[:, :ncls], dref)
                        print(f"{what}: loss {e_loss:.2e} (<= {tol_loss:.1e}), dlogits {e_grad:.2e} (<= {tol_grad:.1e})")
                        assert e_grad <= tol_grad, f"{what}: dlogits {e_grad:.3e} > {tol_grad:.1e}"
                    else:
                        bound = torch.pow(2.0, (torch.frexp(dref)[1] - 9).double()) + tol_elem * S + TINY
                        worst = (err / bound).max().item()
                        print(f"{what}: loss {e_loss:.2e} (<= {tol_loss:.1e}), dlogits {worst:.3f} of the bound")
                        assert worst <= 1.0, f"{what}: dlogits {worst:.2f} x the bound"
                    assert e_loss <= tol_loss, f"{what}: loss {e_loss:.3e} > {tol_loss:.1e}"
