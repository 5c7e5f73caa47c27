"""The hand-written matrix-core kernels of the stem and of stage 2 (csrc/kernels/conv3x3c64.hip,
c3c1.hip, stem.hip, bwd1x1.hip) against plain fp64 references, at the smallest shapes at which
their tiling can go wrong.

  conv3x3c64   forward (with / without bits) and data gradient (partial column sums, idle rows
               zero): H < 4, W = 1, 61 and 62, a partial last row tile, workgroups capped to 1
               and 3 so that one walks several tiles across images and both window buffers;
               W = 63 rejected with nothing written
  ..._wgrad    the same shapes and caps, dw preloaded, ld_dw = 576 and 640 (pad columns untouched)
  c3c1         M around the 64-row tile, residual and the two bits outputs given or not; y1
               against a reference built from the kernel's own (verified) block output
  stem_pool    forward and backward at crops 8, 28, 36 (pool heights 2, 7, 9) x every row-block
               argument, crop 248 (the widest the prefetch covers), crop 252 rejected; ties
               after ReLU exercise the tap scan order, taps into the zero padding the router
  bwd1x1       plain (both channel pairs, M around the tile, padded wd / dw rows), stride-2
               (odd and even sides; `out` owned at the grid pixels only, not pre-zeroed) and
               pre form (downstream outputs against a reference from the kernel's own gx)
  ..._multitile  every form with its workgroups capped (bwd1x1_grid: 1 and 3 workgroups, 8 pairs
               of the (512, 128) form), so that one workgroup walks 2-6 tiles of a few hundred
               rows: both LDS buffers, even and odd parity at the end, a full and a 1-row last
               tile, workgroups that end on different buffers, the prefetched ReLU bits, the
               staging written over the g images under the next tile's DMA, dW summed across
               tiles, the empty last DMA; stride-2 tiles that begin inside an image and span two
  ..._real_grid  plain (both channel pairs) and dual at the production grid, M = 128 W + 37 for W
               workgroups / pairs: every one runs 2-3 tiles at stride W, the last tile 37 rows
  ..._dual     the dual form element by element, M = 1, 65, 300 and the capped shapes: wd2 a
               column slice and dw / dw2 two ranges of one 320-float-row tensor (the rest stays
               sentinel), gx given and gx=None (out / out_s bit-identical, a gx buffer not
               passed untouched), every partial row written, the column-sum rows of waves 4-7 zero

Every bf16 / fp32 output is an `Out` (sentinel NaN inside guards), every bits / argmax output a
`ByteOut`; accumulators start nonzero.  Each case runs twice:

  exact  small sparse integers (activations / gradients in {-1, 0, 1}, weights in {-2..2},
         scales in {0.5, 1, 2}, integer shifts): every product sum is an integer far below 2^24,
         so fp32 accumulation is exact in any order and across any atomics; bf16 outputs must be
         bit-identical to the rounded fp64 reference and fp32 sums equal to it.  Outputs that are
         summed afterwards are integers of magnitude <= 256 (bf16-exact).  The preconditions are
         asserted on the reference alone.
  real   randn inputs, every element within
           2^-8 |ref| + (K + 4) U (|a| (*) |b|) |scale|
         (one bf16 rounding with slack for a double-rounding boundary + fp32 accumulation over
         the reduction length K, `(*)` the same contraction over absolute values); fp32
         accumulators without the first term and K = the number of reduced rows.

ReLU bits equal pack_bits of the kernel's own stored output, byte for byte.  Inputs come from a
host generator, so the references (and the exact-case preconditions) are the same on any device.
"""
import functools
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn.functional as F

from kernel_checks import (BF, F32, ByteOut, Out, U, bn, check, check_bits, check_exact, check_real, dev, gen, ints,
                           nothing, pack_bits, pool_bwd_ref, pool_ref, precond, randn, tern, untouched)

pytestmark = pytest.mark.gpu

KINDS = ["exact", "real"]


def N():
    from pddl.ops.native import require_native
    return require_native()


# --------------------------------------------------------------------------- conv3x3c64
C64_SHAPES = [(1, 1, 1), (2, 3, 62), (3, 5, 7), (2, 9, 61), (5, 4, 16)]      # (N, H, W)


def conv64(x, w):
    """3x3 / pad 1 / stride 1, 64 -> 64, fp64: x [N, H, W, 64], w [64, 576] with k = (r * 3 + s) * 64 + ci."""
    n, h, wd, _ = x.shape
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1))
    wt = w.double().view(64, 9, 64)
    out = torch.zeros(n, h, wd, 64, dtype=torch.float64, device=x.device)
    for r in range(3):
        for s in range(3):
            out += xp[:, r:r + h, s:s + wd] @ wt[:, r * 3 + s].t()
    return out


def wgrad64(x, gy):
    """dW[co][(r * 3 + s) * 64 + ci] = sum over pixels of gy[pixel][co] x[pixel + (r - 1, s - 1)][ci], fp64."""
    n, h, wd, _ = x.shape
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1))
    g2 = gy.double().reshape(-1, 64)
    dw = torch.zeros(64, 9, 64, dtype=torch.float64, device=x.device)
    for r in range(3):
        for s in range(3):
            dw[:, r * 3 + s] = g2.t() @ xp[:, r:r + h, s:s + wd].reshape(-1, 64)
    return dw.view(64, 576)


@functools.lru_cache(maxsize=None)
def c64_case(shape, kind):
    n, h, w = shape
    exact = kind == "exact"
    g = gen(1000 + 64 * h + w + exact)
    if exact:
        x, gy, wt = tern(g, n, h, w, 64), tern(g, n, h, w, 64), ints(g, -2, 2, 64, 576)
    else:
        x, gy, wt = randn(g, n, h, w, 64), randn(g, n, h, w, 64), randn(g, 64, 576, scale=0.05)
    sc, sh = bn(g, 64, exact)
    keep = randn(g, n, h, w, 64)                  # the data gradient's ReLU mask: bits of (keep > 0)
    conv, mag = conv64(x, wt), conv64(x.abs(), wt.abs())
    c = NS(x=x, gy=gy, w=wt, sc=sc, sh=sh, mbits=pack_bits(keep).view(n, h, w, 8))
    c.fwd, c.fwd_mag = torch.relu(conv * sc.double() + sh.double()), mag * sc.double().abs() + sh.double().abs()
    c.dg, c.dg_mag = conv * (keep.double() > 0), mag * (keep.double() > 0)
    c.dw, c.dw_mag = wgrad64(x, gy), wgrad64(x.abs(), gy.abs())
    if exact:
        precond("conv3x3c64", mag, c.dg)
        precond("conv3x3c64_wgrad", c.dw_mag)
    return c


@pytest.fixture
def knob():
    nat, used = N(), []

    def set_(which, v):
        used.append(which)
        nat.set_variant(which, v)
    try:
        yield set_
    finally:
        for which in used:
            nat.set_variant(which, 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("grid", [0, 1, 3])
@pytest.mark.parametrize("shape", C64_SHAPES, ids=str)
def test_conv3x3c64_forward(knob, shape, grid, kind):
    nat, (n, h, w), c = N(), shape, c64_case(shape, kind)
    M = n * h * w
    knob("c64_grid", grid)
    for with_bits in (True, False):
        what = f"conv3x3c64 fwd {shape} grid={grid} {kind} bits={with_bits}"
        out, bt = Out(M * 64, BF), ByteOut(M * 8)
        nat.conv3x3c64(c.x, c.w, 0, out.t.view(n, h, w, 64), scale=c.sc, shift=c.sh,
                       bits=bt.t.view(n, h, w, 8) if with_bits else None)
        out.check(what)
        check(kind, out.t, c.fwd, c.fwd_mag, 576, what)
        if with_bits:
            check_bits(bt, out, what)
        else:
            untouched(bt, what)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("grid", [0, 1, 3])
@pytest.mark.parametrize("shape", C64_SHAPES, ids=str)
def test_conv3x3c64_dgrad(knob, shape, grid, kind):
    """The masked data gradient and its partial column sums: 4 rows per workgroup, summed in fp32
    before the bf16 rounding (so M more additions per channel in the real case), the rows of the
    workgroups the grid leaves out zero."""
    nat, (n, h, w), c = N(), shape, c64_case(shape, kind)
    M = n * h * w
    rows = nat.conv3x3c64_partial_rows(M)
    knob("c64_grid", grid)
    what = f"conv3x3c64 dgrad {shape} grid={grid} {kind}"
    out, part = Out(M * 64, BF), Out(rows * 64, F32)
    nat.conv3x3c64(c.x, c.w, 1, out.t.view(n, h, w, 64), bits=c.mbits, colsum=part.t)
    out.check(what)
    part.check(what + " colsum")
    check(kind, out.t, c.dg, c.dg_mag, 576, what)
    used = min(n * ((h + 3) // 4), grid if grid else rows // 4, rows // 4)
    assert bool((part.t.view(rows, 64)[4 * used:] == 0).all()), f"{what}: rows of idle workgroups not zero"
    check(kind, part.t.view(rows, 64).double().sum(0), c.dg.sum((0, 1, 2)), c.dg_mag.sum((0, 1, 2)), 576 + M + 2,
          what + " colsum", rounded=False)


def test_conv3x3c64_rejects_w63():
    nat = N()
    g = gen(63)
    x, wt = tern(g, 1, 2, 63, 64), ints(g, -2, 2, 64, 576)
    sc, sh = bn(g, 64, True)
    M = 2 * 63
    out, bt, dw = Out(M * 64, BF), ByteOut(M * 8), Out(64 * 576, F32)
    with pytest.raises(RuntimeError, match="62"):
        nat.conv3x3c64(x, wt, 0, out.t.view(1, 2, 63, 64), scale=sc, shift=sh, bits=bt.t.view(1, 2, 63, 8))
    with pytest.raises(RuntimeError, match="62"):
        nat.conv3x3c64_wgrad(x, x, dw.t.view(64, 576))
    torch.cuda.synchronize()
    out.check("conv3x3c64 W=63", nothing(M * 64))
    dw.check("conv3x3c64_wgrad W=63", nothing(64 * 576))
    untouched(bt, "conv3x3c64 W=63")


C64W_CASES = [(s, g_, 576) for s in C64_SHAPES for g_ in (0, 1, 2)] + [((3, 5, 7), 1, 640)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,grid,ld", C64W_CASES, ids=str)
def test_conv3x3c64_wgrad(knob, shape, grid, ld, kind):
    nat, (n, h, w), c = N(), shape, c64_case(shape, kind)
    what = f"conv3x3c64_wgrad {shape} grid={grid} ld_dw={ld} {kind}"
    if ld == 576:
        dw, owned = Out(64 * ld, F32, start=torch.full((64 * ld,), 0.5, device=dev)), None
    else:       # the 64 pad columns of each row are not the kernel's: they stay sentinel
        dw = Out(64 * ld, F32)
        dw.t.view(64, ld)[:, :576] = 0.5
        owned = (torch.arange(64 * ld, device=dev) % ld) < 576
    knob("c64w_grid", grid)
    nat.conv3x3c64_wgrad(c.x, c.gy, dw.t.view(64, ld))
    dw.check(what, owned)
    check(kind, dw.t.view(64, ld)[:, :576], c.dw + 0.5, c.dw_mag + 0.5, n * h * w, what, rounded=False)


# --------------------------------------------------------------------------------- c3c1
@functools.lru_cache(maxsize=None)
def c3c1_case(M, kind):
    exact = kind == "exact"
    g = gen(2000 + 2 * M + exact)
    sc3, sh3 = bn(g, 256, exact)
    sc1, sh1 = bn(g, 64, exact)
    if exact:
        a, w3, w1 = tern(g, M, 64), ints(g, -2, 2, 256, 64), ints(g, -2, 2, 64, 256)
        w3 = (w3.float() * torch.where(sc3 == 0.5, 2.0, 1.0).view(256, 1)).to(BF)    # the block output stays an integer
        res = ints(g, 0, 3, M, 256)
    else:
        a, w3, w1 = torch.relu(randn(g, M, 64)), randn(g, 256, 64, scale=0.05), randn(g, 64, 256, scale=0.05)
        res = torch.relu(randn(g, M, 256))
    acc, mag = a.double() @ w3.double().t(), a.double().abs() @ w3.double().abs().t()
    c = NS(a=a, w3=w3, sc3=sc3, sh3=sh3, w1=w1, sc1=sc1, sh1=sh1, res=res)
    pre, c.mag = acc * sc3.double() + sh3.double(), mag * sc3.double().abs() + sh3.double().abs()
    c.out = {False: torch.relu(pre), True: torch.relu(pre + res.double())}
    c.out_mag = {False: c.mag, True: c.mag + res.double().abs()}
    if exact:
        precond("c3c1", mag, torch.cat([c.out[False], c.out[True]]))
    return c


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_bits", [True, False])
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 200])
def test_c3c1(M, with_res, with_bits, kind):
    nat, c = N(), c3c1_case(M, kind)
    what = f"c3c1 M={M} res={with_res} bits={with_bits} {kind}"
    out, y1, b3, b1 = Out(M * 256, BF), Out(M * 64, BF), ByteOut(M * 32), ByteOut(M * 8)
    nat.c3c1(c.a, c.w3, c.sc3, c.sh3, c.res if with_res else None, out.t.view(M, 256), b3.t if with_bits else None,
             c.w1, c.sc1, c.sh1, y1.t.view(M, 64), b1.t if with_bits else None)
    out.check(what + " out")
    y1.check(what + " y1")
    check(kind, out.t, c.out[with_res], c.out_mag[with_res], 64, what + " out")
    # phase 2 reads the rounded block output: its reference starts from the kernel's own `out`
    o = out.t.view(M, 256).double()
    mag1 = o.abs() @ c.w1.double().abs().t()
    if kind == "exact":
        precond("c3c1 y1", mag1)
    check(kind, y1.t, torch.relu(o @ c.w1.double().t() * c.sc1.double() + c.sh1.double()),
          mag1 * c.sc1.double().abs() + c.sh1.double().abs(), 256, what + " y1")
    if with_bits:
        check_bits(b3, out, what + " bits3")
        check_bits(b1, y1, what + " bits1")
    else:
        untouched(b3, what + " bits3")
        untouched(b1, what + " bits1")


# ------------------------------------------------------------------------- fused stem
def stem_dims(crop):
    hs = (crop + 6) // 2
    return hs, hs - 3, (hs - 3) // 2


def stem_cols(x2):
    """The 4x4 / stride-1 window of the space-to-depth input as GEMM rows, fp64:
    [B, Hs, Ws, 16] -> [B, H1, W1, 256], k = (R * 4 + S) * 16 + c."""
    B, Hs, Ws, _ = x2.shape
    xw = x2.double().unfold(1, 4, 1).unfold(2, 4, 1)            # [B, H1, W1, 16, R, S]
    return xw.permute(0, 1, 2, 4, 5, 3).reshape(B, Hs - 3, Ws - 3, 256)


def at_tap(v, tap):
    """v [B, H1, W1, C] at the window tap of every pool output (0 where the tap is padding)."""
    B, _, _, C = v.shape
    Ho, Wo = tap.shape[1:3]
    vp = F.pad(v, (0, 0, 1, 1, 1, 1))
    ar = lambda n_, *s: torch.arange(n_, device=v.device).view(*s)
    t = tap.long()
    return vp[ar(B, B, 1, 1, 1), 2 * ar(Ho, 1, Ho, 1, 1) + t // 3, 2 * ar(Wo, 1, 1, Wo, 1) + t % 3, ar(C, 1, 1, 1, C)]


@functools.lru_cache(maxsize=None)
def stem_fwd_case(B, crop, kind):
    exact = kind == "exact"
    hs, h1, h2 = stem_dims(crop)
    g = gen(3000 + 4 * crop + 2 * B + exact)
    if exact:
        x2, w = tern(g, B, hs, hs, 16), ints(g, -2, 2, 64, 256)
    else:
        x2, w = randn(g, B, hs, hs, 16), randn(g, 64, 256, scale=0.08)
    sc, sh = bn(g, 64, exact)
    cols = stem_cols(x2)
    mag = cols.abs() @ w.double().abs().t()
    c = NS(x2=x2, w=w, sc=sc, sh=sh)
    c.c1 = torch.relu(cols @ w.double().t() * sc.double() + sh.double())       # fp64, unrounded
    # element bound of a stored conv value: (K + 4) U mag |scale| (+ |shift|) + one bf16 rounding
    c.c1_bound = 2.0 ** -8 * c.c1 + (256 + 4) * U * (mag * sc.double().abs() + sh.double().abs())
    if exact:
        precond("stem_pool_fwd", mag)
        c.best, c.tap = pool_ref(c.c1.to(BF))
    else:
        c.best, c.tap = pool_ref(c.c1)
    return c


STEM_CASES = [(B, crop, rows) for crop in (8, 28, 36) for B in (1, 3) for rows in (0, 1, 2, "all")] + [(1, 248, 0)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,crop,rows", STEM_CASES, ids=str)
def test_stem_pool_fwd(B, crop, rows, kind):
    """exact: the pool of the bf16-rounded conv rows bit for bit, the first maximum in scan order
    (ReLU leaves many tied zeros).  real: with ĉ the kernel's conv values, |ĉ - c| <= b, the
    kernel's tap t holds the largest ĉ, so its stored value is within b_t of c_t and the true
    maximum c_s exceeds c_t by at most b_t + b_s."""
    nat, c = N(), stem_fwd_case(B, crop, kind)
    _, _, h2 = stem_dims(crop)
    rows = h2 if rows == "all" else rows
    n = B * h2 * h2 * 64
    for with_bits in (True, False):
        what = f"stem_pool_fwd B={B} crop={crop} rows={rows} {kind} bits={with_bits}"
        pool, idx, bt = Out(n, BF), ByteOut(n), ByteOut(n // 8)
        nat.stem_pool_fwd(c.x2, c.w, c.sc, c.sh, pool.t.view(B, h2, h2, 64), idx.t.view(B, h2, h2, 64),
                          bt.t.view(B, h2, h2, 8) if with_bits else None, rows)
        pool.check(what)
        idx.check(what + " idx")
        got, tap = pool.t.view(B, h2, h2, 64), idx.t.view(B, h2, h2, 64)
        assert int(tap.max()) <= 8, f"{what}: an argmax tap was not written"
        if kind == "exact":
            check_exact(got, c.best, what)
            assert torch.equal(tap, c.tap), f"{what}: tap is not the first maximum in scan order"
        else:
            c_t, b_t, b_s = at_tap(c.c1, tap), at_tap(c.c1_bound, tap), at_tap(c.c1_bound, c.tap)
            err = (got.double() - c_t).abs()
            assert bool((err <= b_t).all()), \
                f"{what}: pool value {(err / b_t.clamp_min(1e-300)).max().item():.2f} x the bound"
            short = c.best - c_t
            assert bool((short <= b_t + b_s).all()), \
                f"{what}: a tap is {(short / (b_t + b_s).clamp_min(1e-300)).max().item():.2f} x the bound below the maximum"
        if with_bits:
            check_bits(bt, pool, what)
        else:
            untouched(bt, what)


def test_stem_pool_rejects_crop_252():
    nat = N()
    hs, _, h2 = stem_dims(252)
    g = gen(252)
    x2, w = tern(g, 1, hs, hs, 16), ints(g, -2, 2, 64, 256)
    sc, sh = bn(g, 64, True)
    n = h2 * h2 * 64
    pool, idx, bt = Out(n, BF), ByteOut(n), ByteOut(n // 8)
    with pytest.raises(RuntimeError, match="crop"):
        nat.stem_pool_fwd(x2, w, sc, sh, pool.t.view(1, h2, h2, 64), idx.t.view(1, h2, h2, 64), bt.t.view(1, h2, h2, 8), 0)
    dw, cs = Out(64 * 256, F32), Out(nat.stem_pool_bwd_partial_rows(1, h2, 0) * 64, F32)
    with pytest.raises(RuntimeError, match="crop"):
        nat.stem_pool_bwd(x2, tern(g, 1, h2, h2, 64), ints(g, 0, 8, 1, h2, h2, 64, dtype=torch.uint8), dw.t.view(64, 256),
                          cs.t, 0)
    torch.cuda.synchronize()
    pool.check("stem_pool_fwd crop 252", nothing(n))
    dw.check("stem_pool_bwd crop 252", nothing(64 * 256))
    cs.check("stem_pool_bwd crop 252", nothing(cs.n))
    untouched(idx, "stem_pool_fwd crop 252 idx")
    untouched(bt, "stem_pool_fwd crop 252")


@functools.lru_cache(maxsize=None)
def stem_bwd_case(B, crop, kind):
    exact = kind == "exact"
    hs, h1, h2 = stem_dims(crop)
    g = gen(4000 + 4 * crop + 2 * B + exact)
    # taps of a real pool over integers with many negatives: ties, and zero pad taps that win
    _, tap = pool_ref(ints(g, -3, 2, B, h1, h1, 64))
    if exact:
        x2, gpool, dw0 = tern(g, B, hs, hs, 16), ints(g, -3, 3, B, h2, h2, 64), ints(g, -9, 9, 64, 256, dtype=F32) + 0.5
    else:
        x2, gpool, dw0 = randn(g, B, hs, hs, 16), randn(g, B, h2, h2, 64), randn(g, 64, 256, dtype=F32)
    cols = stem_cols(x2).reshape(-1, 256)
    gc1 = pool_bwd_ref(gpool, tap, None, h1, h1)                     # conv1's output gradient, fp64
    gabs = pool_bwd_ref(gpool.abs(), tap, None, h1, h1)
    many = pool_bwd_ref(torch.ones_like(gpool), tap, None, h1, h1) >= 2
    c = NS(x2=x2, gpool=gpool, tap=tap, dw0=dw0, gc1=gc1, gabs=gabs)
    c.dw = dw0.double() + gc1.reshape(-1, 64).t() @ cols
    c.dw_mag = dw0.double().abs() + gabs.reshape(-1, 64).t() @ cols.abs()
    # a conv pixel fed by two to four pool outputs is their fp32 sum rounded to bf16 (as the unfused
    # pair stores it) before the weight-gradient MFMAs: one more rounding of those pixels
    c.dw_round = 2.0 ** -8 * (gabs * many).reshape(-1, 64).t() @ cols.abs()
    if exact:
        precond("stem_pool_bwd", c.dw_mag, gc1)
        assert bool(((tap == 0) | (tap == 3)).any()) and bool((tap == 8).any())
    return c


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,crop,rows", STEM_CASES, ids=str)
def test_stem_pool_bwd(B, crop, rows, kind):
    nat, c = N(), stem_bwd_case(B, crop, kind)
    _, h1, h2 = stem_dims(crop)
    rows = h2 if rows == "all" else rows
    what = f"stem_pool_bwd B={B} crop={crop} rows={rows} {kind}"
    prow = nat.stem_pool_bwd_partial_rows(B, h2, rows)
    dw, cs = Out(64 * 256, F32, start=c.dw0), Out(prow * 64, F32)
    nat.stem_pool_bwd(c.x2, c.gpool, c.tap, dw.t.view(64, 256), cs.t, rows)
    dw.check(what + " dw")
    cs.check(what + " colsum")
    fold = cs.t.view(prow, 64).double().sum(0)
    if kind == "exact":
        check_exact(dw.t, c.dw, what + " dw")
        check_exact(fold, c.gc1.sum((0, 1, 2)), what + " colsum")
    else:
        P = B * h1 * h1
        err, bound = (dw.t.view(64, 256).double() - c.dw).abs(), (P + 4) * U * c.dw_mag + c.dw_round
        print(f"{what}: dw worst err / bound {(err / bound).max().item():.3f}")
        assert bool((err <= bound).all()), f"{what}: dw {(err / bound).max().item():.2f} x the bound"
        # fp32 sums of the routed gradients before their rounding: at most h1 * h1 additions a row
        check_real(fold, c.gc1.sum((0, 1, 2)), c.gabs.sum((0, 1, 2)), h1 * h1, what + " colsum", rounded=False)


# ------------------------------------------------------------------------------- bwd1x1
def b1_inputs(g, M, CO, CI, exact, ld_wd=None):
    ld_wd = ld_wd or CO
    wd = torch.full((CI, ld_wd), float("inf"), dtype=BF, device=dev)          # pad columns are never read
    if exact:
        gy, x, dw0 = tern(g, M, CO), tern(g, M, CI), ints(g, -9, 9, CO, CI, dtype=F32) + 0.5
        wd[:, :CO] = ints(g, -2, 2, CI, CO)
    else:
        gy, x, dw0 = randn(g, M, CO), torch.relu(randn(g, M, CI)), randn(g, CO, CI, dtype=F32)
        wd[:, :CO] = randn(g, CI, CO, scale=0.05)
    return gy, x, wd, dw0, randn(g, M, CI)      # the last: bits of (keep > 0) mask the data gradient


def b1_refs(gy, x, wd, dw0, keep):
    """out = bit * (g . Wd^T), dW = dW0 + g^T . x, each with its contraction over absolute values."""
    CO = gy.shape[-1]
    g2, x2, k2 = gy.double().reshape(-1, CO), x.double().reshape(-1, x.shape[-1]), keep.double().reshape(-1, x.shape[-1]) > 0
    w = wd[:, :CO].double()
    return NS(out=(g2 @ w.t()) * k2, out_mag=(g2.abs() @ w.abs().t()) * k2,
              dw=dw0.double() + g2.t() @ x2, dw_mag=dw0.double().abs() + g2.abs().t() @ x2.abs())


def b1_check_sums(kind, cs, rows, CI, dw, ld_dw, r, M, CO, what):
    """The partial column sums (fp32, taken before the bf16 rounding: M more additions) and dW."""
    fold = cs.t.view(rows, CI).double().sum(0)
    check(kind, fold, r.out.sum(0), r.out_mag.sum(0), CO + M + 2, what + " colsum", rounded=False)
    check(kind, dw.t.view(CO, ld_dw)[:, :CI], r.dw, r.dw_mag, M, what + " dw", rounded=False)


def b1_precond(kernel, r):
    """Exact kind: every sum |a||b| (|dw0| + sum_m |g||x| included) below 2^24, `out` integers of
    magnitude <= 256, and each column's sum_m |out| below 2^24 (the fp32 column sums are exact in
    any order, however many tiles and workgroups they are folded over)."""
    precond(kernel, torch.cat([r.out_mag.reshape(-1), r.dw_mag.reshape(-1), r.out.abs().sum(0)]), r.out)


def b1_dw(CO, CI, dw0, padded):
    """dW preloaded with dw0; padded: rows of CI + 4 floats whose pad is not the kernel's (stays sentinel)."""
    ld_dw = CI + 4 if padded else CI
    dw = Out(CO * ld_dw, F32)
    dw.t.view(CO, ld_dw)[:, :CI] = dw0
    return dw, ld_dw, (torch.arange(CO * ld_dw, device=dev) % ld_dw) < CI


def b1_rows(nat, what, M, CO, CI, want, dual=False):
    """The partial rows the launcher reports; `want`: the rows of the capped / production grid
    (did the geometry under test really run?)."""
    rows = nat.bwd1x1_partial_rows(M, CO, CI, dual)
    if want is not None:
        assert rows == want, f"{what}: {rows} partial rows, {want} expected from the grid under test"
    return rows


def b1_grid(nat, CO, CI, dual=False):
    """(W, M, rows) of the real-grid cases: W the workgroups (pairs) of a large problem, M = 128 W +
    37 rows -- 2 W + 1 tiles, so every workgroup runs 2-3 tiles at stride W."""
    nw = 4 if CO == 256 and not dual else 8
    rows = nat.bwd1x1_partial_rows(1 << 20, CO, CI, dual)
    return rows // nw, 64 * 2 * (rows // nw) + 37, rows


def test_bwd1x1_grid_knob(knob):
    """bwd1x1_grid = 0 leaves the launch geometry as it is (2 workgroups per CU, dual 1, CU / 2
    pairs in multiples of 8, never more workgroups than tiles of the 256 forms); v > 0 caps the
    workgroups, the pairs in multiples of 8 and at least 8; v < 0 is refused."""
    nat = N()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pairs = max(8, cus // 2 // 8 * 8)
    for cap in (0, 1, 3, 8, 20, 1 << 20):
        knob("bwd1x1_grid", cap)
        for M in (1, 64, 65, 477, 64 * 3 * cus + 1):
            T = (M + 63) // 64
            assert nat.bwd1x1_partial_rows(M, 256, 64) == min(T, 2 * cus, cap or T) * 4, (cap, M)
            assert nat.bwd1x1_partial_rows(M, 256, 64, True) == min(T, cus, cap or T) * 8, (cap, M)
            assert nat.bwd1x1_partial_rows(M, 512, 128) == (min(pairs, max(8, cap // 8 * 8)) if cap else pairs) * 8, (cap, M)
    knob("bwd1x1_grid", 3)
    with pytest.raises(RuntimeError, match="bwd1x1_grid"):
        nat.set_variant("bwd1x1_grid", -1)
    assert nat.bwd1x1_partial_rows(1 << 20, 256, 64) == 3 * 4       # (the refused value changed nothing)


def b1_plain(nat, CO, CI, M, padded, kind, want_rows=None):
    exact = kind == "exact"
    ld_wd = CO + 8 if padded else CO
    what = f"bwd1x1 ({CO},{CI}) M={M} padded={padded} rows={want_rows} {kind}"
    gy, x, wd, dw0, keep = b1_inputs(gen(5000 + CO + 2 * M + exact), M, CO, CI, exact, ld_wd)
    r = b1_refs(gy, x, wd, dw0, keep)
    if exact:
        b1_precond("bwd1x1", r)
    rows = b1_rows(nat, what, M, CO, CI, want_rows)
    out, cs = Out(M * CI, BF), Out(rows * CI, F32)
    dw, ld_dw, dw_owned = b1_dw(CO, CI, dw0, padded)
    nat.bwd1x1(gy, x, wd, pack_bits(keep).view(M, CI // 8), out.t.view(M, CI), cs.t, dw.t.view(CO, ld_dw))
    out.check(what + " out")
    cs.check(what + " colsum")
    dw.check(what + " dw", dw_owned)
    check(kind, out.t, r.out, r.out_mag, CO, what + " out")
    b1_check_sums(kind, cs, rows, CI, dw, ld_dw, r, M, CO, what)


B1_CASES = [(co, ci, M, False) for co, ci in ((256, 64), (512, 128)) for M in (1, 63, 64, 65, 257)] + \
           [(256, 64, 65, True), (512, 128, 65, True)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("CO,CI,M,padded", B1_CASES, ids=str)
def test_bwd1x1_plain(CO, CI, M, padded, kind):
    b1_plain(N(), CO, CI, M, padded, kind)


# (CO, CI, cap, M, padded): one workgroup over 6 / 4 / 4 tiles (a 13-row, a full and a 1-row last tile);
# 8 tiles over 3 workgroups (3, 3, 2: they end on different buffers); 20 and 16 tiles over 8 pairs
# (3, 3, 3, 3, 2, 2, 2, 2 and 2 each, both halves of every pair)
B1_MULTI = [(256, 64, 1, 333, True), (256, 64, 1, 256, False), (256, 64, 1, 193, False), (256, 64, 3, 477, False),
            (512, 128, 8, 1221, True), (512, 128, 8, 1024, False)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("CO,CI,cap,M,padded", B1_MULTI, ids=str)
def test_bwd1x1_plain_multitile(knob, CO, CI, cap, M, padded, kind):
    """The persistent tile loop: with the workgroups capped one of them walks several tiles, so the
    two stage buffers alternate, the ReLU bits of the next tile are prefetched and rotated, the
    dgrad staging overwrites the g images under the next tile's DMA and dW is summed over tiles."""
    knob("bwd1x1_grid", cap)
    b1_plain(N(), CO, CI, M, padded, kind, want_rows=cap * 4 if CO == 256 else 8 * 8)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("CO,CI", [(256, 64), (512, 128)])
def test_bwd1x1_plain_real_grid(CO, CI, kind):
    """The production grid (knob at 0) with 2-3 tiles per workgroup (pair) at stride W."""
    nat = N()
    _, M, rows = b1_grid(nat, CO, CI)
    b1_plain(nat, CO, CI, M, False, kind, want_rows=rows)


def b1_stride2(nat, CO, CI, B, Hf, Wf, kind, padded=False, want_rows=None):
    """The gradient lives on the stride-2 grid; `out` is full resolution, starts as sentinels and
    must be written at the grid pixels only; `out2` is the compact copy."""
    exact = kind == "exact"
    Hc, Wc = (Hf + 1) // 2, (Wf + 1) // 2
    M = B * Hc * Wc
    what = f"bwd1x1 stride-2 ({CO},{CI}) B={B} {Hf}x{Wf} padded={padded} rows={want_rows} {kind}"
    g = gen(6000 + CO + 16 * Hf + B + exact)
    gy, _, wd, dw0, _ = b1_inputs(g, M, CO, CI, exact)
    gy = gy.view(B, Hc, Wc, CO)
    x = tern(g, B, Hf, Wf, CI) if exact else torch.relu(randn(g, B, Hf, Wf, CI))
    keep = randn(g, B, Hf, Wf, CI)
    r = b1_refs(gy, x[:, ::2, ::2], wd, dw0, keep[:, ::2, ::2])
    if exact:
        b1_precond("bwd1x1 stride-2", r)
    rows = b1_rows(nat, what, M, CO, CI, want_rows)
    out, out2, cs = Out(B * Hf * Wf * CI, BF), Out(M * CI, BF), Out(rows * CI, F32)
    dw, ld_dw, dw_owned = b1_dw(CO, CI, dw0, padded)
    nat.bwd1x1(gy, x, wd, pack_bits(keep).view(B, Hf, Wf, CI // 8), out.t.view(B, Hf, Wf, CI), cs.t,
               dw.t.view(CO, ld_dw), out2.t.view(B, Hc, Wc, CI))
    on_grid = torch.zeros(B, Hf, Wf, CI, dtype=torch.bool, device=dev)
    on_grid[:, ::2, ::2] = True
    out.check(what + " out", on_grid.reshape(-1))
    out2.check(what + " out2")
    cs.check(what + " colsum")
    dw.check(what + " dw", dw_owned)
    check(kind, out.t.view(B, Hf, Wf, CI)[:, ::2, ::2].contiguous(), r.out, r.out_mag, CO, what + " out")
    check(kind, out2.t, r.out, r.out_mag, CO, what + " out2")
    b1_check_sums(kind, cs, rows, CI, dw, ld_dw, r, M, CO, what)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,Hf,Wf", [(1, 7, 5), (2, 13, 11), (1, 6, 8), (2, 12, 10)], ids=str)
@pytest.mark.parametrize("CO,CI", [(256, 64), (512, 128)])
def test_bwd1x1_stride2(CO, CI, B, Hf, Wf, kind):
    b1_stride2(N(), CO, CI, B, Hf, Wf, kind)


# (CO, CI, cap, B, Hf, Wf, padded): 121-pixel images (M = 363: 6 tiles, each but the first beginning inside
# an image, two spanning two) over 1 and 3 workgroups; 132-pixel images (M = 660: 11 tiles, four spanning
# two images) over 8 pairs, three of which run 2 tiles and five 1
B1_S2_MULTI = [(256, 64, 1, 3, 21, 21, False), (256, 64, 3, 3, 21, 21, True), (512, 128, 8, 5, 23, 21, True)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("CO,CI,cap,B,Hf,Wf,padded", B1_S2_MULTI, ids=str)
def test_bwd1x1_stride2_multitile(knob, CO, CI, cap, B, Hf, Wf, padded, kind):
    """From the second tile on the x descriptor is rebased at the tile's first image (n_first) and
    the next tile's bits are prefetched through the compact-to-full row map."""
    knob("bwd1x1_grid", cap)
    b1_stride2(N(), CO, CI, B, Hf, Wf, kind, padded, want_rows=cap * 4 if CO == 256 else 8 * 8)


def b1_pre(nat, M, kind, padded=False, want_rows=None):
    """gx = bit(gmask) * (g1 . w1d^T + g) with its column sums against fp64; then the plain
    form's outputs against a reference that starts from the kernel's own (rounded) gx."""
    exact = kind == "exact"
    what = f"bwd1x1 pre M={M} padded={padded} rows={want_rows} {kind}"
    g = gen(7000 + 2 * M + exact)
    if exact:
        g1, w1d, add = tern(g, M, 64, p=0.125), ints(g, -1, 1, 256, 64), ints(g, -2, 2, M, 256)
    else:
        g1, w1d, add = randn(g, M, 64), randn(g, 256, 64, scale=0.05), randn(g, M, 256)
    ox = randn(g, M, 256)
    _, x, wd, dw0, keep = b1_inputs(g, M, 256, 64, exact)
    if exact:
        wd = (wd.float() * (torch.rand(64, 256, generator=g) < 0.125).to(dev)).to(BF)   # keeps |out| <= 256
    on = ox.double() > 0
    gx_ref = (g1.double() @ w1d.double().t() + add.double()) * on
    gx_mag = (g1.double().abs() @ w1d.double().abs().t() + add.double().abs()) * on
    if exact:
        precond("bwd1x1 pre gx", torch.cat([gx_mag.reshape(-1), gx_ref.abs().sum(0)]), gx_ref)
    rows = b1_rows(nat, what, M, 256, 64, want_rows)
    gx, csx = Out(M * 256, BF), Out(rows * 256, F32)
    out, cs = Out(M * 64, BF), Out(rows * 64, F32)
    dw, ld_dw, dw_owned = b1_dw(256, 64, dw0, padded)
    nat.bwd1x1(add, x, wd, pack_bits(keep).view(M, 8), out.t.view(M, 64), cs.t, dw.t.view(256, ld_dw),
               g1=g1, w1d=w1d, gmask=pack_bits(ox).view(M, 32), gx=gx.t.view(M, 256), colsum_gx=csx.t)
    for o, name in ((gx, "gx"), (csx, "colsum_gx"), (out, "out"), (cs, "colsum")):
        o.check(f"{what} {name}")
    dw.check(what + " dw", dw_owned)
    check(kind, gx.t, gx_ref, gx_mag, 64, what + " gx")
    fold = csx.t.view(rows, 256).double().sum(0)
    check(kind, fold, gx_ref.sum(0), gx_mag.sum(0), 64 + M + 2, what + " colsum_gx", rounded=False)
    r = b1_refs(gx.t.view(M, 256), x, wd, dw0, keep)
    if exact:
        b1_precond("bwd1x1 pre", r)
    check(kind, out.t, r.out, r.out_mag, 256, what + " out")
    b1_check_sums(kind, cs, rows, 64, dw, ld_dw, r, M, 256, what)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [1, 65, 300])
def test_bwd1x1_pre(M, kind):
    b1_pre(N(), M, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,padded", [(333, False), (477, True)], ids=str)
@pytest.mark.parametrize("cap", [1, 3])
def test_bwd1x1_pre_multitile(knob, cap, M, padded, kind):
    """g is overwritten in place in both stage buffers, gx stored from every tile and its column
    sums carried in registers across the workgroup's tiles."""
    knob("bwd1x1_grid", cap)
    b1_pre(N(), M, kind, padded, want_rows=cap * 4)


# (M, cap): less than a tile, a 1-row second tile, a ragged 5th; 6 and 8 tiles over 1 and 3 workgroups;
# "grid": the production grid with 2-3 tiles per workgroup
B1_DUAL = [(1, 0), (65, 0), (300, 0), (333, 1), (477, 1), (333, 3), (477, 3), ("grid", 0)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,cap", B1_DUAL, ids=str)
def test_bwd1x1_dual(knob, M, cap, kind):
    """The dual form as the engine launches it (wd2 a column slice with 320-element rows, dw and dw2
    two 64-column ranges of one [256][320] tensor), once with gx and once without.  gx and its
    column sums against fp64; out / out_s / dw / dw2 / column sums against fp64 from the fp64 g
    (exact: g is an integer of magnitude <= 256, so the bf16 tile holds it exactly) or from the
    kernel's own stored gx (real: the tile is that bf16 g).  Without gx: out and out_s bit-identical
    (each tile's GEMMs run in a fixed order; the gx branch only stores), the sums and weight
    gradients within the same bounds, a gx buffer that is not passed untouched."""
    nat = N()
    exact = kind == "exact"
    W, Mg, full = b1_grid(nat, 256, 64, True)
    if M == "grid":
        M, want = Mg, full
    else:
        want = (cap if cap else min((M + 63) // 64, W)) * 8
    what = f"bwd1x1 dual M={M} cap={cap} {kind}"
    knob("bwd1x1_grid", cap)
    rows = b1_rows(nat, what, M, 256, 64, want, dual=True)
    g = gen(8000 + 2 * M + exact)
    wd_all = torch.full((64, 320), float("inf"), dtype=BF, device=dev)      # columns 0-63 are never read
    if exact:
        g1, w1d, add = tern(g, M, 64, p=0.125), ints(g, -1, 1, 256, 64), ints(g, -2, 2, M, 256)
        x2, w2, dw20 = tern(g, M, 64), ints(g, -2, 2, 64, 256), ints(g, -9, 9, 256, 64, dtype=F32) + 0.5
    else:
        g1, w1d, add = randn(g, M, 64), randn(g, 256, 64, scale=0.05), randn(g, M, 256)
        x2, w2, dw20 = torch.relu(randn(g, M, 64)), randn(g, 64, 256, scale=0.05), randn(g, 256, 64, dtype=F32)
    ox = randn(g, M, 256)
    _, x, wd, dw0, keep = b1_inputs(g, M, 256, 64, exact)
    if exact:       # sparse weights keep |out|, |out_s| <= 256
        wd = (wd.float() * (torch.rand(64, 256, generator=g) < 0.125).to(dev)).to(BF)
        w2 = (w2.float() * (torch.rand(64, 256, generator=g) < 0.125).to(dev)).to(BF)
    wd_all[:, 64:] = w2
    wd2 = wd_all[:, 64:]
    on = ox.double() > 0
    gx_ref = (g1.double() @ w1d.double().t() + add.double()) * on
    gx_mag = (g1.double().abs() @ w1d.double().abs().t() + add.double().abs()) * on
    if exact:
        precond("bwd1x1 dual gx", torch.cat([gx_mag.reshape(-1), gx_ref.abs().sum(0)]), gx_ref)
    bits, gmask = pack_bits(keep).view(M, 8), pack_bits(ox).view(M, 32)
    dw_owned = (torch.arange(256 * 320, device=dev) % 320) < 128

    def launch(gx):
        o = NS(out=Out(M * 64, BF), out_s=Out(M * 64, BF), cs=Out(rows * 64, F32), csx=Out(rows * 256, F32),
               dwa=Out(256 * 320, F32))
        dwa = o.dwa.t.view(256, 320)
        dwa[:, :64], dwa[:, 64:128] = dw0, dw20
        nat.bwd1x1(add, x, wd, bits, o.out.t.view(M, 64), o.cs.t, dwa[:, :64], g1=g1, w1d=w1d, gmask=gmask, gx=gx,
                   colsum_gx=o.csx.t, x2=x2, wd2=wd2, out_s=o.out_s.t.view(M, 64), dw2=dwa[:, 64:128])
        return o

    gx = Out(M * 256, BF)
    a = launch(gx.t.view(M, 256))
    gx.check(what + " gx")
    check(kind, gx.t, gx_ref, gx_mag, 64, what + " gx")
    gsrc = gx_ref if exact else gx.t.view(M, 256)
    r = b1_refs(gsrc, x, wd, dw0, keep)
    r2 = b1_refs(gsrc, x2, wd2, dw20, torch.ones(M, 64, device=dev))         # the shortcut half: no mask
    if exact:
        b1_precond("bwd1x1 dual", r)
        b1_precond("bwd1x1 dual shortcut", r2)
    gx_none = Out(M * 256, BF)
    b = launch(None)
    gx_none.check(what + " gx not passed", nothing(M * 256))
    for o, tag in ((a, what + " with gx"), (b, what + " gx=None")):
        for t, name in ((o.out, "out"), (o.out_s, "out_s"), (o.cs, "colsum"), (o.csx, "colsum_gx")):
            t.check(f"{tag} {name}")      # (every reported partial row written: no sentinel left)
        o.dwa.check(tag + " dw / dw2", dw_owned)
        fold = o.csx.t.view(rows, 256).double().sum(0)
        check(kind, fold, gx_ref.sum(0), gx_mag.sum(0), 64 + M + 2, tag + " colsum_gx", rounded=False)
        check(kind, o.out.t, r.out, r.out_mag, 256, tag + " out")
        check(kind, o.out_s.t, r2.out, r2.out_mag, 256, tag + " out_s")
        b1_check_sums(kind, o.cs, rows, 64, o.dwa, 320, r, M, 256, tag)
        check(kind, o.dwa.t.view(256, 320)[:, 64:128], r2.dw, r2.dw_mag, M, tag + " dw2", rounded=False)
        assert bool((o.cs.t.view(rows // 8, 8, 64)[:, 4:] == 0).all()), \
            f"{tag}: column-sum rows of waves 4-7 (the shortcut half) not zero"
    assert torch.equal(a.out.t.view(torch.int16), b.out.t.view(torch.int16)), f"{what}: out differs without gx"
    assert torch.equal(a.out_s.t.view(torch.int16), b.out_s.t.view(torch.int16)), f"{what}: out_s differs without gx"

