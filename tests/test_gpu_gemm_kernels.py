"""The implicit-GEMM and weight-gradient kernels (csrc/kernels/igemm.hip, wgrad.hip) against plain
fp64 references, at the smallest shapes that reach each kernel, gather mode, epilogue and edge.

  igemm_kernel      256x64 and 128x128 tiles, one and two LDS stages, direct / halo / dual gathers,
                    the window form, every epilogue mode (forward: residual, bits, split second
                    output, stride-2 residual, batch statistics; data gradient: bf16 mask, bits,
                    add, column sums, the three stride-2 scatters, fused BN-backward sums; the fp32
                    head), the epilogue-operand prefetch, split-K slices
  igemm8_kernel     forced at small grids (knob igemm8 + 16): M around the 256-row tile, K loops
                    shorter than, equal to and longer than the prefetch depth, the three gathers
  igemm_pk_kernel   every (KT, NB) instantiation with the workgroup count capped to 1 and 3
                    (igemm_pk_grid), so that one workgroup walks several tiles and the ring crosses
                    tile boundaries at M = 677; a partial column tile; the dual-source form
  igemm_splitk_reduce_kernel   forced and heuristic slice counts, uneven slices, a workspace of
                    exactly igemm_splitk_floats inside guards, one float short -> unsplit
  wgrad_kernel / wgrad8_kernel   both widths, fast and gather, one and two stages, m splits,
                    dw preloaded with 0.5 and wider than K, g wider than Cout

Every case asserts through igemm_last_launch() / wgrad_last_tiling() that the kernel it is meant
for really ran.  Every bf16 / fp32 output is an `Out` (sentinel NaN inside guards), every bits
output a `ByteOut`; row strides are larger than the rows, and the pad must stay sentinel.  Each case
runs twice (kernel_checks.py):

  exact  activations and gradients in {-1, 0, 1}, weights in {-2..2}, scales in {0.5, 1, 2},
         integer shifts, residual in {0..3}: fp32 accumulation is exact in any order, bf16 outputs
         must be bit-identical to the rounded fp64 reference and fp32 sums equal to it.
  real   randn inputs, every element within 2^-8 |ref| + (K + 4 + slices) U mag (slices: the
         split-K slice count, 0 unsplit); fp32 sums over `rows` rows within (K + rows + 2 + 4) U mag
         without the rounding term.  Sums defined on the STORED bf16 values (batch statistics, the
         BN-backward sums) are compared with the same sums of the kernel's own stored output:
         rows + 2 additions, and two more roundings per term for g * (z - mean).
"""
import zlib
from types import SimpleNamespace as NS

import pytest
import torch

from kernel_checks import (BF, F32, PRECOND, ByteOut, Out, bn, check, dev, gather, gen, guards_only, ints, pack_bits,
                           precond, randn, tern, untouched)

pytestmark = pytest.mark.gpu

KINDS = ["exact", "real"]
PAD = 8          # extra elements of every padded row (bf16 rows stay 16-byte aligned)
DEFAULTS = {"igemm": 0, "igemm_pf": 1, "igemm8": 2, "igemm8_min_n": 512, "igemm8_min_tiles": 128, "igemm_n64": 1,
            "igemm_splitk": 1, "igemm_pk": 2, "igemm_pk_all": 0, "igemm_pk_dual": 2, "igemm_pk_grid": 0,
            "wgrad8": 2, "wgrad1": 1}
DIRECT, HALO, DUAL = "direct", "halo", "dual"


def N():
    from pddl.ops.native import require_native
    return require_native()


@pytest.fixture
def knob():
    """Sets kernel knobs and puts every one it touched back to its default afterwards.  Every test
    here starts from the per-tile kernels: ring off, split-K off, no epilogue prefetch."""
    nat, used = N(), []

    def set_(which, v):
        used.append(which)
        nat.set_variant(which, v)
    try:
        set_("igemm_pk", 0)
        set_("igemm_splitk", 0)
        set_("igemm_pf", 0)
        yield set_
    finally:
        nat.splitk_use(None)
        for which in used:
            nat.set_variant(which, DEFAULTS[which])


@pytest.fixture(scope="module", autouse=True)
def _report_preconditions():
    """After the module: the largest exact-case magnitudes per kernel family (shown with -s)."""
    yield
    for k, (m, r) in sorted(PRECOND.items()):
        print(f"PRECOND {k}: largest sum |a||b| {m:.0f}, largest summed |ref| {r:.0f}")


# ---------------------------------------------------------------------------- references
def gathered(a1, a2, geom):
    """A of one or two sources; the second at its own H2 x W2 and stride2 = ceil(H2 / Ho) (1x1)."""
    H, W, R, S, stride, pad, Ho, Wo = geom
    A = gather(a1, H, W, R, S, stride, pad, Ho, Wo)
    if a2 is not None:
        H2, W2 = a2.shape[1], a2.shape[2]
        if (H2, W2) == (H, W):
            A2 = gather(a2, H, W, R, S, stride, pad, Ho, Wo)
        else:
            A2 = gather(a2, H2, W2, 1, 1, (H2 + Ho - 1) // Ho, 0, Ho, Wo)
        A = torch.cat([A, A2], 1)
    return A


def gemm_ref(a1, a2, geom, B):
    """acc = A @ B[:, :K].T and the same contraction over absolute values, fp64."""
    A = gathered(a1, a2, geom)
    Bk = B[:, :A.shape[1]].double()
    return A @ Bk.t(), A.abs() @ Bk.abs().t()


def wgrad_ref(x, geom, g, K):
    """dW = g.T @ A (the first K columns of A) and its absolute-value contraction, fp64."""
    A = gathered(x, None, geom)[:, :K]
    g2 = g.double().reshape(A.shape[0], -1)
    return g2.t() @ A, g2.abs().t() @ A.abs()


# ------------------------------------------------------------------------------- buffers
def strided(t, fill=float("inf")):
    """t [rows, n] inside rows of n + PAD elements; the pad (`fill`) is not the kernel's to read."""
    rows, n = t.shape
    buf = torch.full((rows, n + PAD), fill, dtype=t.dtype, device=dev)
    buf[:, :n] = t
    return buf[:, :n]


class Rows:
    """A guarded output of `rows` rows of n elements at row stride n + PAD; the pad stays sentinel."""

    def __init__(self, rows, n, dtype, start=None):
        self.ld = n + PAD
        self.o = Out(rows * self.ld, dtype)
        self.v = self.o.t.view(rows, self.ld)[:, :n]
        self.cols = (torch.arange(rows * self.ld, device=dev) % self.ld) < n
        if start is not None:
            self.v.copy_(start)

    def check(self, what, rows_owned=None):
        owned = self.cols if rows_owned is None else self.cols & rows_owned.repeat_interleave(self.ld)
        self.o.check(what, owned)


class ByteRows:
    def __init__(self, rows, n):
        self.ld = n + PAD
        self.o = ByteOut(rows * self.ld)
        self.v = self.o.t.view(rows, self.ld)[:, :n]

    def check_packed(self, stored, what):
        """The bytes equal pack_bits of the stored output; the pad bytes are untouched."""
        self.o.check(what)
        full = self.o.t.view(-1, self.ld)
        assert bool((full[:, self.v.shape[1]:] == 0xA5).all()), f"{what}: bits pad written"
        want = pack_bits(stored.contiguous()).view(stored.shape[0], -1)
        assert torch.equal(self.v, want), f"{what}: bits != packed (stored output > 0)"


def launched(nat, expect, what):
    got = nat.igemm_last_launch()
    assert len(got) == len(expect), f"{what}: launched {got}, meant {expect}"
    for g_, e in zip(got, expect):
        for k, v in e.items():
            assert g_[k] == v, f"{what}: launched {got}, meant {expect}"


# ----------------------------------------------------------------------- the shared runner
def spec(**kw):
    """One igemm problem.  a2: None, ("same", C2) or (H2, W2, C2).  ws: None, "exact" or "short"."""
    d = dict(N=1, H=1, W=1, C=64, R=1, S=1, stride=1, pad=0, Nn=128, mode="fwd", a2=None, relu=1, res=False,
             bits=False, mask=False, add=False, colsum=False, n_split=0, relu2=0, up2=0, Hf=0, Wf=0, stats=False,
             bnz=False, ws=None, slices=0)
    assert not set(kw) - set(d), set(kw) - set(d)
    d.update(kw)
    return NS(**d)


def rows1x1(M, **kw):
    """M GEMM rows as M images of one pixel (1x1 / direct)."""
    return spec(N=M, **kw)


def name(c):
    base = vars(spec())
    return ",".join(f"{k}={v}" for k, v in vars(c).items() if base[k] != v) or "plain"


def run_igemm(nat, c, kind, expect, family):
    exact = kind == "exact"
    what = f"{family} [{name(c)}] {kind}"
    g = gen(zlib.crc32(name(c).encode()) * 2 + exact)
    Ho, Wo = (c.H + 2 * c.pad - c.R) // c.stride + 1, (c.W + 2 * c.pad - c.S) // c.stride + 1
    geom = (c.H, c.W, c.R, c.S, c.stride, c.pad, Ho, Wo)
    M, Nn = c.N * Ho * Wo, c.Nn
    act = (lambda *s: tern(g, *s)) if exact else (lambda *s: randn(g, *s))
    a1 = act(c.N, c.H, c.W, c.C)
    a2 = None
    if c.a2 is not None:
        a2 = act(c.N, c.H, c.W, c.a2[1]) if c.a2[0] == "same" else act(c.N, *c.a2)
    K = c.R * c.S * (c.C + (a2.shape[-1] if a2 is not None else 0))
    B = strided(ints(g, -2, 2, Nn, K) if exact else randn(g, Nn, K, scale=0.05))
    acc, mag = gemm_ref(a1, a2, geom, B)
    assert acc.shape == (M, Nn)
    if exact:
        precond(family, mag)
    KB = K + c.slices                       # the bound's reduction length: (KB + 4) U mag
    ws = None
    if c.ws:
        floats = nat.igemm_splitk_floats(M, Nn, K)
        assert floats > 0, f"{what}: the plan does not split"
        ws = Out(floats - (c.ws == "short"), F32)
        nat.splitk_use(ws.t)
    mode = {"fwd": 0, "dgrad": 1, "f32": 2}[c.mode]
    kw = dict(relu=c.relu, up2=c.up2, Hf=c.Hf, Wf=c.Wf)
    rows = nat.igemm_partial_rows(M, Nn, K, c.bnz)
    part = Out(rows * Nn, F32) if c.colsum else None
    stats = Out(rows * 2 * Nn, F32) if (c.stats or c.bnz) else None
    call = lambda out, **more: nat.igemm(a1, a2, c.H, c.W, c.R, c.S, c.stride, c.pad, Ho, Wo, B, mode, out=out,
                                         colsum=part.t if part else None, stats=stats.t if stats else None,
                                         **kw, **more)

    if c.mode in ("fwd", "f32"):
        sc, sh = bn(g, Nn, exact)
        if c.stats and exact:
            sc = torch.ones_like(sc)
        pre, pmag = acc * sc.double() + sh.double(), mag * sc.double().abs() + sh.double().abs()
        if c.mode == "f32":
            out = Rows(M, Nn, F32)
            call(out.v, scale=sc, shift=sh)
            launched(nat, expect, what)
            out.check(what)
            check(kind, out.v.contiguous(), pre, pmag, KB, what, rounded=False)
            if ws:
                guards_only(ws, what + " workspace")
            return
        res = None
        if c.res:
            rrows = c.N * c.Hf * c.Wf if c.up2 else M
            res = strided(ints(g, 0, 3, rrows, Nn) if exact else torch.relu(randn(g, rrows, Nn)))
            r64 = res.double()
            if c.up2:       # the residual of the Hf x Wf grid at [n, 2 i, 2 j]
                assert ((c.Hf + 1) // 2, (c.Wf + 1) // 2) == (Ho, Wo)
                r64 = r64.view(c.N, c.Hf, c.Wf, Nn)[:, ::2, ::2].reshape(M, Nn)
                res = res.unflatten(0, (c.N, c.Hf, c.Wf))
            pre, pmag = pre + r64, pmag + r64.abs()
        seg0 = c.n_split if c.n_split else Nn
        out, bt = Rows(M, seg0, BF), ByteRows(M, seg0 // 8)
        out2 = Rows(M, Nn - seg0, BF) if c.n_split else None
        call(out.v, scale=sc, shift=sh, res=res, bits_out=bt.v if c.bits else None,
             out2=out2.v if out2 else None, relu2=c.relu2, n_split=c.n_split)
        launched(nat, expect, what)
        out.check(what + " out")
        act_ = lambda v, on: torch.relu(v) if on else v
        check(kind, out.v.contiguous(), act_(pre[:, :seg0], c.relu), pmag[:, :seg0], KB, what + " out")
        if out2:
            out2.check(what + " out2")
            check(kind, out2.v.contiguous(), act_(pre[:, seg0:], c.relu2), pmag[:, seg0:], KB, what + " out2")
        if c.bits:
            bt.check_packed(out.v, what)
        else:
            untouched(bt.o, what)
        if c.stats:          # sums of exactly the stored values, both segments
            stats.check(what + " stats")
            v = out.v.double() if not out2 else torch.cat([out.v.double(), out2.v.double()], 1)
            if exact:
                assert float((v * v).sum(0).max()) < 2 ** 24, f"{what}: test bug, sum v^2"
                precond(family + " stats", (v * v).sum(0), v)
            fold = stats.t.view(rows, 2, Nn).double().sum(0)
            check(kind, fold[0], v.sum(0), v.abs().sum(0), M - 2, what + " stats sum", rounded=False)
            check(kind, fold[1], (v * v).sum(0), (v * v).sum(0), M - 2, what + " stats sum of squares", rounded=False)
        if ws:
            guards_only(ws, what + " workspace")
        return

    # ---- data gradient
    full = (c.N, c.Hf, c.Wf) if c.up2 else None
    rfull = c.N * c.Hf * c.Wf if c.up2 else M
    if c.up2:
        assert ((c.Hf + 1) // 2, (c.Wf + 1) // 2) == (Ho, Wo)
    mrows = M if c.up2 == 3 else rfull                    # (up2 3: the mask lives on the compact grid)
    keep = randn(g, mrows, Nn)
    on = keep.double() > 0
    mask = None
    if c.mask:
        mask = strided(keep)
    elif c.bits:
        mask = strided(pack_bits(keep).view(mrows, Nn // 8), fill=0xFF)
    else:
        on = torch.ones_like(on)
    add = add64 = None
    if c.add:
        add = strided(ints(g, -2, 2, rfull, Nn) if exact else randn(g, rfull, Nn))
        add64 = add.double()
    out = Rows(rfull, Nn, BF)
    out2 = Rows(M, Nn, BF) if (c.up2 >= 2) else None
    z = mean = None
    if c.bnz:
        z = strided(ints(g, -3, 3, M, Nn) if exact else randn(g, M, Nn))
        mean = ints(g, -2, 2, Nn, dtype=F32) if exact else randn(g, Nn, scale=0.5, dtype=F32)
    shape4 = lambda t: t.unflatten(0, full) if (full and t is not None and t.shape[0] == rfull) else t
    call(shape4(out.v), mask=shape4(mask), add=shape4(add), out2=out2.v if out2 else None, bn_z=z, bn_mean=mean)
    launched(nat, expect, what)
    grid = None
    if not c.up2:
        ref, rmag = acc, mag
        if c.add:
            ref, rmag = ref + add64, rmag + add64.abs()
        ref, rmag = ref * on, rmag * on
        written, wmag = ref, rmag
    else:
        grid = torch.zeros(c.N, c.Hf, c.Wf, dtype=torch.bool, device=dev)
        grid[:, ::2, ::2] = True
        grid = grid.reshape(-1)
        if c.up2 == 1:          # all four positions of every compact pixel: the whole fine grid
            ref = torch.zeros(rfull, Nn, dtype=torch.float64, device=dev)
            rmag = torch.zeros_like(ref)
            ref[grid], rmag[grid] = acc, mag
            if c.add:
                ref, rmag = ref + add64, rmag + add64.abs()
            ref, rmag = ref * on, rmag * on
            written, wmag, grid = ref, rmag, None
        else:                   # the grid positions only
            ref, rmag = acc, mag
            if c.add:
                ref, rmag = ref + add64[grid], rmag + add64[grid].abs()
            on_g = on if c.up2 == 3 else on[grid]
            ref, rmag = ref * on_g, rmag * on_g
            written, wmag = ref, rmag
    out.check(what + " out", grid)
    got = out.v if grid is None else out.v[grid]
    check(kind, got.contiguous(), ref, rmag, KB, what + " out")
    if out2:
        out2.check(what + " out2")
        check(kind, out2.v.contiguous(), ref, rmag, KB, what + " out2")
    if c.colsum:             # of the unrounded masked values of every position written
        part.check(what + " colsum")
        if exact:
            precond(family + " colsum", wmag.sum(0))
        check(kind, part.t.view(rows, Nn).double().sum(0), written.sum(0), wmag.sum(0), KB + written.shape[0] + 2,
              what + " colsum", rounded=False)
    if c.bnz:                # (sum g, sum g (z - mean)) of the stored gradient
        stats.check(what + " bn sums")
        gq, dz = out.v.double(), z.double() - mean.double()
        if exact:
            assert float((gq * dz).abs().sum(0).max()) < 2 ** 24 and float((gq * gq).sum(0).max()) < 2 ** 24
            precond(family + " bnz", (gq * dz).abs().sum(0), gq)
        fold = stats.t.view(rows, 2, Nn).double().sum(0)
        check(kind, fold[0], gq.sum(0), gq.abs().sum(0), M - 2, what + " sum g", rounded=False)
        check(kind, fold[1], (gq * dz).sum(0), (gq * dz).abs().sum(0), M, what + " sum g (z - mean)", rounded=False)
    if ws:
        guards_only(ws, what + " workspace")


def tile(kernel, stages=1, gather=DIRECT, pf=0, bnz=0, slices=1):
    return dict(kernel=kernel, stages=stages, gather=gather, pf=pf, bnz=bnz, slices=slices)


T128, T64 = "tile128x128", "tile256x64"


def ids(cases):
    return [name(c[0]) if isinstance(c, tuple) else name(c) for c in cases]


# ------------------------------------------------------------------- per-tile igemm_kernel
HALO3 = dict(R=3, S=3, pad=1)
PLAIN = [
    # 128x128 (Nn = 128, 136, 256 below the 8-phase width): M = 1, a tail, several tiles
    (rows1x1(1, Nn=128, C=64), T128, DIRECT),
    (rows1x1(129, Nn=136, C=192), T128, DIRECT),
    (rows1x1(300, Nn=256, C=128), T128, DIRECT),
    # 3x3 / pad 1 at stride 1 and 2 on a 5 x 7 image: tiles span images, M = 105 and 36
    (spec(N=3, H=5, W=7, C=64, Nn=128, **HALO3), T128, HALO),
    (spec(N=3, H=5, W=7, C=64, Nn=128, stride=2, **HALO3), T128, HALO),
    # the window form: 4 taps x 16 channels are one contiguous k-tile
    (spec(N=3, H=6, W=6, C=16, R=4, S=4, Nn=128), T128, DIRECT),
    (spec(N=3, H=6, W=6, C=16, R=4, S=4, Nn=64), T64, DIRECT),
] + [
    # 256x64: Nn = 8, 64, and 192 (three column tiles by the igemm_n64 rule) x M around the tile
    (rows1x1(M, Nn=Nn, C=64), T64, DIRECT) for Nn in (8, 64, 192) for M in (1, 255, 257, 600)
] + [
    (spec(N=n, H=h, W=w, C=64, Nn=Nn, **HALO3), T64, HALO)
    for Nn in (8, 64, 192) for n, h, w in ((1, 1, 1), (17, 3, 5), (257, 1, 1), (40, 3, 5))
]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("stages", [1, 2])
@pytest.mark.parametrize("case", PLAIN, ids=ids(PLAIN))
def test_igemm_tiles(knob, case, stages, kind):
    c, kernel, gat = case
    knob("igemm", 0 if stages == 1 else 2)
    run_igemm(N(), c, kind, [tile(kernel, stages, gat)], "igemm_kernel")


DUALS = [
    # the data gradient's K concatenation (same geometry), masked
    (spec(N=5, H=3, W=9, C=64, a2=("same", 128), Nn=128, mode="dgrad", mask=True), T128),
    (spec(N=5, H=3, W=9, C=64, a2=("same", 128), Nn=64, mode="dgrad", mask=True), T64),
    # the projection forward: the second source at its own 5 x 5 grid, stride 2 onto 3 x 3
    (spec(N=15, H=3, W=3, C=64, a2=(5, 5, 128), Nn=128, bits=True), T128),
    (spec(N=15, H=3, W=3, C=64, a2=(5, 5, 128), Nn=192, bits=True), T64),
    (spec(N=15, H=3, W=3, C=128, a2=(6, 5, 64), Nn=136), T128),
]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("stages", [1, 2])
@pytest.mark.parametrize("case", DUALS, ids=ids(DUALS))
def test_igemm_dual_source(knob, case, stages, kind):
    c, kernel = case
    knob("igemm", 0 if stages == 1 else 2)
    knob("igemm_pk_dual", 0)
    run_igemm(N(), c, kind, [tile(kernel, stages, DUAL)], "igemm_kernel dual")


def both_widths(**kw):
    """One 128-wide (Nn = 136) and one 64-wide (Nn = 192) problem of M = 300 rows: an M tail in both."""
    return [(rows1x1(300, Nn=136, C=128, **kw), T128), (rows1x1(300, Nn=192, C=128, **kw), T64)]


def both_widths_up2(**kw):
    """Compact 3 x 3 grids of 15 images (M = 135) under fine grids of odd and even sides."""
    return [(spec(N=15, H=3, W=3, C=64, Nn=Nn, Hf=Hf, Wf=Wf, **kw), k)
            for Nn, k in ((136, T128), (192, T64)) for Hf, Wf in ((5, 6), (6, 5))]


EPILOGUES = (
    both_widths(relu=0) + both_widths(res=True) + both_widths(res=True, bits=True) +
    # columns >= 64 of Nn = 320 go to the second output; 256x64 by the igemm_n64 rule, 128x128 without it
    [(rows1x1(300, Nn=320, C=128, n_split=64, bits=True, relu2=0), T64),
     (rows1x1(300, Nn=320, C=128, n_split=64, bits=True, relu2=1, relu=0), "n64=0")] +
    both_widths_up2(res=True, up2=1, bits=True) +
    both_widths(mode="dgrad", mask=True) + both_widths(mode="dgrad", bits=True) +
    both_widths(mode="dgrad", add=True, bits=True, colsum=True) +
    both_widths_up2(mode="dgrad", up2=1, add=True, mask=True, colsum=True) +
    both_widths_up2(mode="dgrad", up2=2, add=True, bits=True, colsum=True) +
    both_widths_up2(mode="dgrad", up2=3, mask=True, colsum=True) +
    both_widths_up2(mode="dgrad", up2=3, add=True, bits=True) +
    [(rows1x1(M, Nn=1000, C=2048, mode="f32"), T128) for M in (1, 6, 130)]
)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", EPILOGUES, ids=ids(EPILOGUES))
def test_igemm_epilogues(knob, case, kind):
    c, kernel = case
    if kernel == "n64=0":
        knob("igemm_n64", 0)
        kernel = T128
    run_igemm(N(), c, kind, [tile(kernel)], "igemm_kernel epilogue")


PF_CASES = [(c, k, pf, stages) for pf in (0, 1, 2) for stages in (1, 2)
            for c, k in both_widths(res=True, bits=True) + both_widths(mode="dgrad", add=True, bits=True, colsum=True)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", PF_CASES, ids=[f"pf{c[2]}-s{c[3]}-{name(c[0])}" for c in PF_CASES])
def test_igemm_epilogue_prefetch(knob, case, kind):
    """PF instantiations: the forward residual whenever the knob is on; the data gradient's add
    on two-stage tiles, or on every tile with igemm_pf = 2."""
    c, kernel, pf, stages = case
    knob("igemm_pf", pf)
    knob("igemm", 0 if stages == 1 else 2)
    on = pf and (c.mode == "fwd" or stages == 2 or pf == 2)
    run_igemm(N(), c, kind, [tile(kernel, stages, pf=1 if on else 0)], "igemm_kernel PF")


BN_SUMS = both_widths(stats=True, relu=0) + both_widths(stats=True, res=True) + \
    both_widths(mode="dgrad", bnz=True, add=True, bits=True) + \
    [(spec(N=3, H=5, W=7, C=64, Nn=Nn, mode="dgrad", bnz=True, mask=True, **HALO3), k) for Nn, k in ((128, T128), (64, T64))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", BN_SUMS, ids=ids(BN_SUMS))
def test_igemm_bn_sums(knob, case, kind):
    c, kernel = case
    gat = HALO if c.R == 3 else DIRECT
    run_igemm(N(), c, kind, [tile(kernel, 1, gat, bnz=1 if c.bnz else 0)], "igemm_kernel BN sums")


# ------------------------------------------------------------------------ igemm8_kernel
FWD8 = dict(res=True, bits=True)
DG8 = dict(mode="dgrad", add=True, bits=True, colsum=True)
EIGHT = (
    # M around the 256-row tile; KT = 4: the K loop is shorter than the prefetch depth
    [(rows1x1(M, Nn=256, C=256, **FWD8), DIRECT) for M in (1, 255, 256, 257, 700)] +
    # KT = 5, 6 and 18 (equal to the lead and longer), two column tiles
    [(rows1x1(257, Nn=512, C=C, **FWD8), DIRECT) for C in (320, 384, 1152)] +
    [(rows1x1(700, Nn=512, C=256, **DG8), DIRECT), (rows1x1(255, Nn=256, C=320, **DG8), DIRECT)] +
    # 3x3 / pad 1, K = 1152: M = 280 spans images
    [(spec(N=8, H=5, W=7, C=128, Nn=256, **HALO3, **DG8), HALO), (spec(N=8, H=5, W=7, C=128, Nn=256, **HALO3, **FWD8), HALO)] +
    # dual source, K = 128 + 256, with the stride-2 scatter (odd and even fine grids); M = 261
    [(spec(N=29, H=3, W=3, C=128, a2=("same", 256), Nn=256, mode="dgrad", up2=1, Hf=Hf, Wf=Wf, mask=True, colsum=True), DUAL)
     for Hf, Wf in ((5, 6), (6, 5))] +
    [(spec(N=29, H=3, W=3, C=128, a2=(5, 5, 256), Nn=256, bits=True), DUAL)]
)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("stagger", [1, 2])
@pytest.mark.parametrize("case", EIGHT, ids=ids(EIGHT))
def test_igemm8(knob, case, stagger, kind):
    """The 8-phase kernel at grids of 1 to 6 workgroups (knob + 16: whatever the grid)."""
    c, gat = case
    knob("igemm8", 16 + stagger)
    knob("igemm8_min_n", 256)
    knob("igemm_pk_dual", 0)
    run_igemm(N(), c, kind, [dict(kernel="igemm8_stagger" if stagger == 2 else "igemm8", gather=gat, slices=1)],
              "igemm8_kernel")


# ---------------------------------------------------------------------- igemm_pk_kernel
RING_FWD = dict(res=True, bits=True)
RING_DG = dict(mode="dgrad", add=True, bits=True, colsum=True)
M_RING = 128 * 5 + 37
RING = (
    # every instantiation, two column tiles x six row tiles, the last one partial
    [(rows1x1(M_RING, Nn=256, C=64 * kt, **m), nb, grid)
     for kt, nb in ((1, 2), (2, 2), (4, 2), (8, 2), (2, 3), (2, 4)) for grid in (0, 1, 3) for m in (RING_FWD, RING_DG)] +
    [(rows1x1(M, Nn=256, C=128, **m), 2, grid) for M in (1, 128) for grid in (0, 1) for m in (RING_FWD, RING_DG)] +
    # a 32-column last column tile that still plans the 128x128 form
    [(rows1x1(M_RING, Nn=160, C=128, **m), 2, grid) for grid in (0, 3) for m in (RING_FWD, RING_DG)] +
    # a stride-2 forward: 7 x 5 images onto 4 x 3
    [(spec(N=11, H=7, W=5, stride=2, C=128, Nn=256, **RING_FWD), 2, grid) for grid in (1, 3)] +
    # the other epilogue modes
    [(rows1x1(M_RING, Nn=256, C=128, **m), 2, 3)
     for m in (dict(), dict(res=True), dict(bits=True, relu=0), dict(mode="dgrad", add=True),
               dict(mode="dgrad", bits=True), dict(mode="dgrad", bits=True, colsum=True),
               dict(mode="dgrad", add=True, colsum=True), dict(mode="dgrad", add=True, bits=True))]
)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", RING, ids=[f"nb{c[1]}-g{c[2]}-{name(c[0])}" for c in RING])
def test_igemm_ring(knob, case, kind):
    """The persistent ring kernel; with the workgroup cap one workgroup owns up to 12 tiles, so
    the ring crosses tile boundaries (and a row-tile change) with NB - 1 steps in flight."""
    c, nb, grid = case
    nat = N()
    knob("igemm_pk", nb)
    knob("igemm_pk_all", 1)
    knob("igemm_pk_grid", grid)
    Ho, Wo = (c.H - 1) // c.stride + 1, (c.W - 1) // c.stride + 1
    tiles = ((c.N * Ho * Wo + 127) // 128) * ((c.Nn + 127) // 128)
    assert tiles <= 64                      # (below any device's workgroup count: the cap alone decides)
    run_igemm(nat, c, kind, [dict(kernel="ring", kt=c.C // 64, nb=nb, gather=DIRECT, slices=1,
                                  grid=min(tiles, grid) if grid else tiles)], "igemm_pk_kernel")


RING_DUAL = [(spec(N=17, H=3, W=3, C=f, a2=(5, 5, cin), Nn=4 * f, bits=True), grid)
             for f, cin in ((64, 64), (128, 256), (256, 512), (512, 1024)) for grid in (1,)] + \
            [(spec(N=17, H=3, W=3, C=64, a2=(5, 5, 64), Nn=256, bits=False), 0),
             (spec(N=17, H=3, W=3, C=128, a2=(6, 5, 256), Nn=512, bits=True), 3)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", RING_DUAL, ids=[f"g{c[1]}-{name(c[0])}" for c in RING_DUAL])
def test_igemm_ring_dual(knob, case, kind):
    """The dual-source ring (KT = 2, 6, 12, 24): the second source at 5 x 5 / stride 2 under a
    3 x 3 output; M = 153 is two row tiles, all of them walked by one workgroup."""
    c, grid = case
    knob("igemm_pk", 2)
    knob("igemm_pk_dual", 24)
    knob("igemm_pk_grid", grid)
    tiles = 2 * ((c.Nn + 127) // 128)
    run_igemm(N(), c, kind, [dict(kernel="ring_dual", kt=(c.C + c.a2[2]) // 64, nb=2, gather=DUAL,
                                  grid=min(tiles, grid) if grid else tiles)], "igemm_pk_kernel dual")


# --------------------------------------------------------------------------- split-K
SK_FWD = dict(res=True, bits=True)
SK_DG = dict(mode="dgrad", add=True, mask=True, colsum=True)
SPLITK = (
    # (problem, knob, slices): KT equal to the slice count, and KT = 7 in 3 uneven slices
    [(rows1x1(300, Nn=Nn, C=C, **m), ks, min(ks, C // 64))
     for Nn in (136, 64) for C, ks in ((128, 2), (448, 3), (512, 8), (192, 8)) for m in (SK_FWD, SK_DG)] +
    # 3x3 / pad 1, KT = 9
    [(spec(N=3, H=5, W=7, C=64, Nn=Nn, **HALO3, **m), ks, ks)
     for Nn in (136, 64) for ks, m in ((3, SK_DG), (2, SK_FWD), (8, SK_FWD))] +
    # the fp32 head, forced and by the heuristic (8 column tiles, KT = 32)
    [(rows1x1(6, Nn=1000, C=2048, mode="f32"), 3, 3), (rows1x1(6, Nn=1000, C=2048, mode="f32"), 1, None),
     (rows1x1(300, Nn=136, C=512, **SK_FWD), 1, None), (rows1x1(300, Nn=64, C=1024, **SK_DG), 1, None)]
)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("stages", [1, 2])
@pytest.mark.parametrize("case", SPLITK, ids=[f"ks{c[1]}-{name(c[0])}" for c in SPLITK])
def test_igemm_splitk(knob, case, stages, kind):
    """Slices into a workspace of exactly igemm_splitk_floats (inside guards), then the combine
    with the fused epilogue.  Knob 1 is the heuristic: its slice count comes from the plan."""
    c, ks, slices = case
    nat = N()
    knob("igemm_splitk", ks)
    knob("igemm", 0 if stages == 1 else 2)
    K = c.R * c.S * c.C
    Ho, Wo = (c.H + 2 * c.pad - c.R) // c.stride + 1, (c.W + 2 * c.pad - c.S) // c.stride + 1
    cfg, _, planned = nat.igemm_plan(c.N * Ho * Wo, c.Nn, K)
    if slices is None:
        slices = planned
        assert slices > 1, "the heuristic does not split this problem"
    assert planned == slices
    kernel = T64 if cfg == 0 else T128
    assert kernel == (T64 if c.Nn in (64, 192) else T128)
    c = spec(**{**vars(c), "ws": "exact", "slices": slices})
    gat = HALO if c.R == 3 else DIRECT
    run_igemm(nat, c, kind, [tile(kernel, stages, gat, slices=slices),
                             dict(kernel="combine256x64" if cfg == 0 else "combine128x128", slices=slices)],
              "igemm split-K")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Nn", [136, 64])
def test_igemm_splitk_short_workspace_runs_unsplit(knob, Nn, kind):
    """A workspace one float short: the same tile runs unsplit and gives the unsplit result."""
    knob("igemm_splitk", 3)
    c = rows1x1(300, Nn=Nn, C=448, ws="short", **SK_DG)
    run_igemm(N(), c, kind, [tile(T64 if Nn == 64 else T128)], "igemm split-K, short workspace")


# ------------------------------------------------------------------------------- wgrad
def run_wgrad(nat, kind, what, n, h, w, C, R, stride, pad, Cout, tiling, splits=0, co_split=0, K=None):
    """dw [Cout][K] += g.T @ A: dw preloaded with 0.5 in rows of K + PAD, g in rows of Cout + PAD
    (with co_split: two gradients, rows >= co_split of dw from the second)."""
    exact = kind == "exact"
    g_ = gen(zlib.crc32(what.encode()) * 2 + exact)
    Ho, Wo = (h + 2 * pad - R) // stride + 1, (w + 2 * pad - R) // stride + 1
    M = n * Ho * Wo
    K = K or R * R * C
    x = tern(g_, n, h, w, C) if exact else randn(g_, n, h, w, C)
    gy = tern(g_, M, Cout) if exact else randn(g_, M, Cout)
    ref, mag = wgrad_ref(x, (h, w, R, R, stride, pad, Ho, Wo), gy, K)
    if exact:
        precond("wgrad", mag)
    dw = Rows(Cout, K, F32, start=torch.full((Cout, K), 0.5, device=dev))
    full = dw.o.t.view(Cout, dw.ld)                                      # dw [Cout][>= K] at row stride K + PAD
    if co_split:
        g1, g2 = strided(gy[:, :co_split].contiguous(), fill=7.0), strided(gy[:, co_split:].contiguous(), fill=7.0)
        nat.wgrad(x, h, w, R, R, stride, pad, Ho, Wo, g1, g2, co_split, full, K, splits)
    else:
        nat.wgrad(x, h, w, R, R, stride, pad, Ho, Wo, strided(gy, fill=7.0), None, 0, full, K, splits)
    assert nat.wgrad_last_tiling() == tiling, f"{what}: tiling {nat.wgrad_last_tiling()}, meant {tiling}"
    dw.check(what)
    # M products a sum, and at most 4 partial sums added by atomics onto the preloaded value
    check(kind, dw.v.contiguous(), ref + 0.5, mag + 0.5, M + 4, what, rounded=False)


# (n, h, w) of M = 1, 63, 64, 65 and 200 output pixels (stride 1)
WG_M = [(1, 1, 1), (7, 3, 3), (1, 8, 8), (5, 1, 13), (8, 5, 5)]
WGRAD = (
    # 128-wide tile: fast (1x1, K = 64 and 192) and gather (3x3 / pad 1, K = 576)
    [(n, h, w, C, 1, 1, 0, Cout, 128) for n, h, w in WG_M for C, Cout in ((64, 72), (192, 128), (64, 136))] +
    [(n, h, w, 64, 3, 1, 1, Cout, 128) for n, h, w in WG_M for Cout in (72, 128, 136)] +
    # 64-wide tile
    [(n, h, w, 64, R, 1, R // 2, Cout, 64) for n, h, w in WG_M[1:4] for R in (1, 3) for Cout in (8, 64)] +
    # 3x3 / stride 2 on an odd image
    [(3, 7, 5, 64, 3, 2, 1, 72, 128), (3, 7, 5, 64, 3, 2, 1, 64, 64)]
)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("stages", [1, 2])
@pytest.mark.parametrize("case", WGRAD, ids=str)
def test_wgrad_tiles(knob, case, stages, kind):
    n, h, w, C, R, stride, pad, Cout, tiling = case
    knob("wgrad8", 0)
    knob("wgrad1", 2 if stages == 1 else 0)
    run_wgrad(N(), kind, f"wgrad_kernel {case} stages={stages} {kind}", n, h, w, C, R, stride, pad, Cout, tiling)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("stages", [1, 2])
@pytest.mark.parametrize("splits", [1, 3, 0])
@pytest.mark.parametrize("Cout,tiling", [(136, 128), (64, 64)])
def test_wgrad_splits(knob, Cout, tiling, splits, stages, kind):
    """The m-reduction split across workgroups (atomics onto the preloaded dw): M = 200."""
    knob("wgrad8", 0)
    knob("wgrad1", 2 if stages == 1 else 0)
    for R in (1, 3):
        run_wgrad(N(), kind, f"wgrad_kernel splits={splits} Cout={Cout} R={R} stages={stages} {kind}", 8, 5, 5, 64, R, 1,
                  R // 2, Cout, tiling, splits=splits)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("stages", [1, 2])
def test_wgrad_window_and_second_gradient(knob, stages, kind):
    """The window form (4 taps x 16 channels, K = 256) and g2 / co_split (two launches: rows
    >= 64 of dw from the second gradient on the 128-wide tile)."""
    nat = N()
    knob("wgrad8", 0)
    knob("wgrad1", 2 if stages == 1 else 0)
    what = f"wgrad_kernel window stages={stages} {kind}"
    exact = kind == "exact"
    g_ = gen(77 + exact)
    x = tern(g_, 3, 6, 6, 16) if exact else randn(g_, 3, 6, 6, 16)
    gy = tern(g_, 27, 64) if exact else randn(g_, 27, 64)
    ref, mag = wgrad_ref(x, (6, 6, 4, 4, 1, 0, 3, 3), gy, 256)
    if exact:
        precond("wgrad", mag)
    dw = Rows(64, 256, F32, start=torch.full((64, 256), 0.5, device=dev))
    nat.wgrad(x, 6, 6, 4, 4, 1, 0, 3, 3, strided(gy, fill=7.0), None, 0, dw.o.t.view(64, dw.ld), 256, 0)
    assert nat.wgrad_last_tiling() == 64
    dw.check(what)
    check(kind, dw.v.contiguous(), ref + 0.5, mag + 0.5, 27 + 4, what, rounded=False)
    for R in (1, 3):
        run_wgrad(nat, kind, f"wgrad_kernel g2 R={R} stages={stages} {kind}", 5, 1, 13, 64, R, 1, R // 2, 64 + 136, 128,
                  co_split=64)


# (n, h, w): 1, 2, 3 and 4 m-tiles of 64 rows plus a partial one
WG8_M = [(9, 3, 3), (29, 1, 5), (11, 1, 19), (13, 3, 7)]
WGRAD8 = (
    # fast: K = 256, 320, 1152 x Cout = 128, 120 (one co half) and 256
    [(n, h, w, C, 1, 1, 0, Cout) for (n, h, w), C in zip(WG8_M, (256, 320, 1152, 256)) for Cout in (128, 120, 256)] +
    # gather: 3x3 / pad 1 (K = 1152), and a strided 1x1 (one tap, K = 256 and 320)
    [(n, h, w, 128, 3, 1, 1, Cout) for n, h, w in WG8_M[1:3] for Cout in (120, 256)] +
    [(5, 7, 5, C, 1, 2, 0, Cout) for C in (256, 320) for Cout in (128, 256)] +
    [(3, 7, 5, 128, 3, 2, 1, 256)]
)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("stagger", [1, 2])
@pytest.mark.parametrize("case", WGRAD8, ids=str)
def test_wgrad8(knob, case, stagger, kind):
    n, h, w, C, R, stride, pad, Cout = case
    knob("wgrad8", 16 + stagger)
    run_wgrad(N(), kind, f"wgrad8_kernel {case} stagger={stagger} {kind}", n, h, w, C, R, stride, pad, Cout,
              1128 if Cout <= 128 else 1256)
