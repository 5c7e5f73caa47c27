"""The fp32 matrix-core kernels of the reference-precision path (csrc/kernels/conv_f32.hip) against
plain fp64 references, at the smallest shapes that reach each kernel, epilogue and edge.

  conv_f32_kernel<VEC> / scalar   64 x 64 tiles: rows and columns around the tile, K % 16 != 0, K < 16,
                    the scalar gather (C = 3, 10), the scalar epilogue of a ragged last column group
  conv_f32_big_kernel<64 / 128>   128 x BN LDS-DMA tiles: K loops of 1, 2, 3 and 4 steps of the 3-stage
                    pipeline, a second 64-row half that is empty or holds one row, tiles that span
                    images and borders, the 4x4 window, the launcher's fallbacks to 64 x 64
  conv_f32_splitk_kernel<64 / 128>   2, 3, 5 and 8 slices (even, odd, uneven, beginning inside a
                    tap), a workspace of exactly the planned floats inside guards, one float short and
                    none at all -> unsplit
  wgrad_f32_kernel<VEC> / scalar, wgrad_f32_big_kernel   dw preloaded with 0.5, one-step reductions,
                    ragged gradient columns, K tails, m-splits that begin inside an image

Every case asserts through conv_f32_last_launch() that the kernel, slice count and weight-gradient
split it is meant for really ran.  Every output is an `Out` (sentinel NaN inside guards): y (with the
stride-2 scatter: the off-grid positions must stay sentinel), the partial column sums at exactly
ceil(M / 64) * Cout floats, dw at exactly Cout * K, the workspace at exactly the plan's floats.  Each
case runs twice (kernel_checks.py):

  exact  activations and gradients in {-1, 0, 1}, weights in {-2..2}, scales in {0.5, 1, 2}, integer
         shifts and bias, residual in {0..3}, add in {-2..2}: every sum is exact in fp32 in any
         order, and the outputs, the folded column sums and dw must EQUAL the fp64 reference.
  real   randn activations, 0.05 randn weights: |got - ref| <= (L + 4) U mag per element, U = 2^-24,
         mag the same contraction over absolute values carried through the epilogue.  The fp32 MFMA
         is an fmaf chain with one rounding per term, each further term one more rounding:
         L = K + slices for a convolution (slices 1 unsplit), K + rows + 2 for a column sum folded
         over `rows` rows, M + splits for a weight gradient.

The ReLU mask of the data gradients holds positive and negative values and both zeros (mask > 0).
"""
import zlib
from types import SimpleNamespace as NS

import pytest
import torch

from kernel_checks import (F32, PRECOND, Out, bn, check, dev, gather, gen, guards_only, ints, is_sent, precond, randn,
                           tern)

pytestmark = pytest.mark.gpu

KINDS = ["exact", "real"]
DEFAULTS = {"conv_f32": 1, "conv_f32_splitk": 4, "conv_f32_sk_elig": 1, "wgrad_f32_wpc64": 16, "wgrad_f32_wpc128": 3}
SEEN = {}        # asserted kernel -> slice counts / splits seen (printed after the module)


def N():
    from pddl.ops.native import require_native
    return require_native()


@pytest.fixture
def knob():
    """Sets kernel knobs and puts every one it touched back to its default afterwards, and the
    thread's split-K workspace back to none.  Every test here starts with split-K off."""
    nat, used = N(), []

    def set_(which, v):
        used.append(which)
        nat.set_variant(which, v)
    try:
        nat.splitk_use(None)
        set_("conv_f32_splitk", 0)
        yield set_
    finally:
        nat.splitk_use(None)
        for which in used:
            nat.set_variant(which, DEFAULTS[which])


@pytest.fixture(scope="module", autouse=True)
def _report():
    """After the module (shown with -s): the largest exact-case magnitudes per kernel family and
    the kernels, slice counts and splits that were asserted."""
    yield
    for k, (m, r) in sorted(PRECOND.items()):
        print(f"PRECOND {k}: largest sum |a||b| {m:.0f}, largest summed |ref| {r:.0f}")
    for k, v in sorted(SEEN.items()):
        print(f"ASSERTED {k}: slices / splits {sorted(v)}")


# ----------------------------------------------------------------------------- the problems
def spec(**kw):
    """One fp32 conv problem.  epi: "plain" / "fwd" / "dgrad".  ws: None, "exact" or "short"."""
    d = dict(N=1, H=1, W=1, C=64, R=1, S=1, stride=1, pad=0, Cout=64, epi="fwd", bias=False, res=False, relu=0,
             add=False, mask=False, colsum=False, up2=0, Hf=0, Wf=0, ws=None)
    assert not set(kw) - set(d), set(kw) - set(d)
    d.update(kw)
    return NS(**d)


def rows1x1(M, **kw):
    """M GEMM rows as M images of one pixel."""
    return spec(N=M, **kw)


def also(c, **kw):
    return spec(**{**vars(c), **kw})


def name(c):
    base = vars(spec())
    return ",".join(f"{k}={v}" for k, v in vars(c).items() if base[k] != v) or "default"


def out_hw(c):
    return (c.H + 2 * c.pad - c.R) // c.stride + 1, (c.W + 2 * c.pad - c.S) // c.stride + 1


FWD = dict(epi="fwd", res=True, relu=1)
DG = dict(epi="dgrad", add=True, mask=True, colsum=True)
HALO3 = dict(R=3, S=3, pad=1)
T64, T64S, B64, B128 = "tile64", "tile64_scalar", "big64", "big128"


def kernels_of(c, big64_knob=1):
    """(knob conv_f32, kernel) of every kernel that accepts the problem: the 64 x 64 kernel with
    float4 gathers for C % 4 == 0, else the scalar one; the LDS-DMA tiles for C % 16 == 0 and at
    most 32 taps."""
    out = [(0, T64 if c.C % 4 == 0 else T64S)]
    if c.C % 16 == 0 and c.R * c.S <= 32:
        out += [(big64_knob, B64), (2, B128)]
    return out


def cross(cases, big64_knob=1):
    return [(c, v, k) for c in cases for v, k in kernels_of(c, big64_knob)]


def ids(cases):
    return [f"{c[2]}-{name(c[0])}" for c in cases]


def launched(nat, expect, what):
    got = nat.conv_f32_last_launch()
    assert len(got) == len(expect), f"{what}: launched {got}, meant {expect}"
    for g_, e in zip(got, expect):
        for k, v in e.items():
            assert g_[k] == v, f"{what}: launched {got}, meant {expect}"
    for e in expect:
        SEEN.setdefault(e["kernel"], set()).add(e.get("slices", 1))


def relu_mask(g, *shape):
    """A ReLU mask as the engines keep it (the activation itself): positive values, negative values,
    and zeros of both signs -- only `> 0` lets the gradient through."""
    m = torch.randn(shape, generator=g)
    z = torch.rand(shape, generator=g)
    m = torch.where(z < 0.25, torch.zeros(()), m)
    m = torch.where(z < 0.08, -torch.zeros(()), m)
    return m.to(dev)


# --------------------------------------------------------------------- the shared conv runner
def run_conv(nat, c, kind, expect, family):
    exact = kind == "exact"
    what = f"{family} [{name(c)}] {kind}"
    g = gen(zlib.crc32(name(c).encode()) * 2 + exact)
    Ho, Wo = out_hw(c)
    M, K, Cout = c.N * Ho * Wo, c.R * c.S * c.C, c.Cout
    x = tern(g, c.N, c.H, c.W, c.C).float() if exact else randn(g, c.N, c.H, c.W, c.C, dtype=F32)
    w = ints(g, -2, 2, Cout, K, dtype=F32) if exact else randn(g, Cout, K, scale=0.05, dtype=F32)
    A = gather(x, c.H, c.W, c.R, c.S, c.stride, c.pad, Ho, Wo)
    acc, mag = A @ w.double().t(), A.abs() @ w.double().abs().t()
    assert acc.shape == (M, Cout)
    if exact:
        precond(family, mag)
    L = K + expect[0]["slices"]                     # the bound's reduction length: (L + 4) U mag
    ws = None
    if c.ws:
        BN, tiles, slices, floats = nat.conv_f32_splitk_plan(M, Cout, K, c.C, c.R * c.S)
        assert floats > 0 and floats == tiles * slices * 128 * BN, f"{what}: the plan does not split"
        ws = Out(floats - (c.ws == "short"), F32)
        nat.splitk_use(ws.t)
    if c.up2:
        assert c.epi == "dgrad" and c.Hf >= 2 * Ho - 1 and c.Wf >= 2 * Wo - 1
    oshape = (c.N, c.Hf, c.Wf, Cout) if c.up2 else (c.N, Ho, Wo, Cout)
    rfull = oshape[0] * oshape[1] * oshape[2]
    y = Out(rfull * Cout, F32)
    y4 = y.t.view(oshape)
    prows = (M + 63) // 64
    part = Out(prows * Cout, F32) if c.colsum else None
    conv = (x, c.R, c.S, c.stride, c.pad)
    owned = None

    if c.epi == "plain":
        b = None
        if c.bias:
            b = ints(g, -3, 3, Cout, dtype=F32) if exact else randn(g, Cout, scale=0.1, dtype=F32)
        nat.conv_f32(*conv, w, b, y4)
        ref, rmag = acc, mag
        if c.bias:
            ref, rmag = ref + b.double(), rmag + b.double().abs()
    elif c.epi == "fwd":
        sc, sh = bn(g, Cout, exact)
        ref, rmag = acc * sc.double() + sh.double(), mag * sc.double().abs() + sh.double().abs()
        res = None
        if c.res:
            res = ints(g, 0, 3, M, Cout, dtype=F32) if exact else randn(g, M, Cout, dtype=F32)
            ref, rmag = ref + res.double(), rmag + res.double().abs()
            res = res.view(oshape)
        nat.conv_f32_epi(*conv, Ho, Wo, w, 1, scale=sc, shift=sh, res=res, relu=c.relu, y=y4)
        if c.relu:
            ref = torch.relu(ref)
    else:
        add = keep = None
        ref, rmag = acc, mag
        if c.add:                       # (with up2 the compact tensor, indexed by the GEMM row)
            add = ints(g, -2, 2, M, Cout, dtype=F32) if exact else randn(g, M, Cout, dtype=F32)
            ref, rmag = ref + add.double(), rmag + add.double().abs()
            add = add.view(c.N, Ho, Wo, Cout)
        grid = None
        if c.up2:
            grid = torch.zeros(c.N, c.Hf, c.Wf, dtype=torch.bool, device=dev)
            grid[:, :2 * Ho - 1:2, :2 * Wo - 1:2] = True
            grid = grid.reshape(-1)
            assert int(grid.sum()) == M
            owned = grid.repeat_interleave(Cout)
        if c.mask:                      # (full resolution: indexed by the output row)
            keep = relu_mask(g, rfull, Cout)
            on = (keep.double() > 0) if grid is None else (keep.double() > 0)[grid]
            ref, rmag = ref * on, rmag * on
            keep = keep.view(oshape)
        nat.conv_f32_epi(*conv, Ho, Wo, w, 2, add=add, mask=keep, up2=c.up2, y=y4, colsum=part.t if part else None)
    launched(nat, expect, what)
    y.check(what + " y", owned)
    got = y.t.view(rfull, Cout)
    check(kind, (got if owned is None else got[grid]).contiguous(), ref, rmag, L, what + " y", rounded=False)
    if c.colsum:
        part.check(what + " colsum")
        if exact:
            precond(family + " colsum", rmag.sum(0))
        check(kind, part.t.view(prows, Cout).double().sum(0), ref.sum(0), rmag.sum(0), K + M + 2, what + " colsum",
              rounded=False)
    if ws is not None:
        guards_only(ws, what + " workspace")
        if expect[0]["slices"] == 1:
            assert bool(is_sent(ws.t).all()), f"{what}: an unsplit launch wrote the workspace"
        else:
            assert not bool(is_sent(ws.t).all()), f"{what}: the slices never reached the workspace"


def conv_case(knob, case, kind, family):
    c, v, kernel = case
    Ho, Wo = out_hw(c)
    M = c.N * Ho * Wo
    bm, bn_ = (64, 64) if kernel in (T64, T64S) else (128, 64 if kernel == B64 else 128)
    knob("conv_f32", v)
    run_conv(N(), c, kind, [dict(kernel=kernel, slices=1, grid=-(-M // bm) * -(-c.Cout // bn_), m_per_split=0)], family)


# ------------------------------------------------------------------------- rows and columns
ROWS = cross([rows1x1(M, **DG) for M in (1, 63, 64, 65, 127, 128, 129, 300)] +
             [rows1x1(M, **FWD) for M in (1, 65, 129, 300)], big64_knob=3)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ROWS, ids=ids(ROWS))
def test_conv_rows_around_the_tiles(knob, case, kind):
    """M around the 64- and 128-row tiles (C = 64, Cout = 64).  With column sums, M = 64 and 65 pin
    the empty and the one-row second half of a 128-row tile: the partial buffer has exactly
    ceil(M / 64) rows, so a row written for an empty half lands in its guard."""
    conv_case(knob, case, kind, "conv rows")


COLS = cross([rows1x1(65, C=32, Cout=co, **m) for co in (1, 4, 10, 100, 136, 200) for m in (FWD, DG)])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", COLS, ids=ids(COLS))
def test_conv_column_edges(knob, case, kind):
    """Cout below, at and across the column tiles; Cout % 4 != 0 takes the scalar epilogue for the
    last column group, and rows of 1 and 10 floats are not 16-byte aligned."""
    conv_case(knob, case, kind, "conv columns")


KLOOP = cross([rows1x1(129, C=C, Cout=72, **m) for C in (16, 32, 48, 64) for m in (FWD, DG)], big64_knob=3)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", KLOOP, ids=ids(KLOOP))
def test_conv_k_loop_lengths(knob, case, kind):
    """KT = 1, 2, 3 and 4 steps of the 3-stage LDS-DMA pipeline (its prologue issues one or two
    steps, its wait counts assume one in flight), and one to four steps of the two-buffer kernel."""
    conv_case(knob, case, kind, "conv K loop")


KTAILS = cross([rows1x1(65, C=C, Cout=72, **m) for C in (20, 40, 3, 10) for m in (FWD, DG)])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", KTAILS, ids=ids(KTAILS))
def test_conv_k_tails(knob, case, kind):
    """K % 16 != 0 with float4 gathers (C = 20, 40), and the scalar gather at K < 16 (C = 3, 10)."""
    c, v, kernel = case
    assert kernel == (T64 if c.C in (20, 40) else T64S)
    conv_case(knob, case, kind, "conv K tail")


GEOMS = [dict(N=3, H=5, W=7, C=64, **HALO3), dict(N=3, H=5, W=7, C=64, stride=2, **HALO3),
         dict(N=3, H=5, W=7, C=64, stride=2)]
SPANS = cross([spec(Cout=72, **geo, **m) for geo in GEOMS for m in (FWD, DG)])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", SPANS, ids=ids(SPANS))
def test_conv_tiles_span_images_and_borders(knob, case, kind):
    """3x3 / pad 1 at stride 1 (M = 105) and stride 2 (3 x 4, M = 36), and 1x1 / stride 2 (M = 36),
    on 5 x 7 images: every tile holds several images and every border."""
    c = case[0]
    assert c.N * out_hw(c)[0] * out_hw(c)[1] == (105 if c.stride == 1 else 36)
    conv_case(knob, case, kind, "conv geometry")


STEM = cross([spec(N=2, H=9, W=11, C=3, R=7, S=7, stride=2, pad=3, Cout=64, **m) for m in (FWD, DG)] +
             [spec(N=3, H=6, W=6, C=16, R=4, S=4, Cout=64, **m) for m in (FWD, DG)])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", STEM, ids=ids(STEM))
def test_conv_stem_forms(knob, case, kind):
    """7x7 / 2 / 3 on 3 channels (K = 147: the scalar gather only) and the 4x4 window on 16
    channels (K = 256, M = 27: every 16-float step is one tap)."""
    c, v, kernel = case
    assert kernel == T64S if c.C == 3 else c.R * c.S * c.C == 256
    conv_case(knob, case, kind, "conv stem")


FALLBACK = [(spec(N=1, H=7, W=7, C=16, R=6, S=6, Cout=64, **FWD), 1, T64),
            (spec(N=1, H=7, W=7, C=16, R=6, S=6, Cout=64, **DG), 2, T64),
            (rows1x1(65, C=20, Cout=72, **FWD), 2, T64), (rows1x1(65, C=20, Cout=72, **DG), 1, T64),
            (rows1x1(65, C=10, Cout=72, **FWD), 2, T64S)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", FALLBACK, ids=[f"knob{c[1]}-{name(c[0])}" for c in FALLBACK])
def test_conv_dispatch_fallbacks(knob, case, kind):
    """36 taps do not fit the tap bitmask and C % 16 != 0 cannot feed 16-float steps: the 64 x 64
    kernels run even when the knob asks for the LDS-DMA tiles."""
    conv_case(knob, case, kind, "conv fallback")


# -------------------------------------------------------------------------------- epilogues
def subsets(*keys):
    return [{k: True for i, k in enumerate(keys) if bits >> i & 1} for bits in range(1 << len(keys))]


EPIS = ([dict(epi="plain", bias=b) for b in (False, True)] +
        [dict(epi="fwd", res=r, relu=a) for r in (False, True) for a in (0, 1)] +
        [dict(epi="dgrad", **s) for s in subsets("add", "mask", "colsum")])
EPILOGUES = (cross([spec(N=3, H=5, W=7, C=64, Cout=100, **HALO3, **m) for m in EPIS]) +
             [(c, v, k) for c, v, k in cross([rows1x1(129, C=64, Cout=100, **m) for m in EPIS])
              if k != T64 and not (c.epi == "dgrad" and 0 < c.add + c.mask + c.colsum < 3)] +
             cross([rows1x1(65, C=32, Cout=10, **m) for m in EPIS]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", EPILOGUES, ids=ids(EPILOGUES))
def test_conv_epilogues(knob, case, kind):
    """PLAIN with and without bias, FWD with and without residual and ReLU, DGRAD with every subset
    of {add, mask, colsum}.  Cout = 100 is 25 whole column groups (the 16-byte path alone); Cout = 10
    ends on a ragged group, which takes the scalar path of every epilogue."""
    conv_case(knob, case, kind, "conv epilogue")


SCATTER = cross([spec(N=3, H=3, W=4, C=64, Cout=co, epi="dgrad", up2=1, Hf=Hf, Wf=Wf, add=True, mask=True, colsum=cs)
                 for Hf, Wf in ((5, 7), (6, 8)) for co, cs in ((100, True), (100, False), (10, True))] +
                [spec(N=3, H=3, W=4, C=64, Cout=100, epi="dgrad", up2=1, Hf=6, Wf=7)])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", SCATTER, ids=ids(SCATTER))
def test_conv_stride2_scatter(knob, case, kind):
    """GEMM row (n, i, j) of a 3 x 4 grid goes to (n, 2 i, 2 j) of the odd 5 x 7 grid, of the even
    6 x 8 one and of 6 x 7; the off-grid positions stay sentinel, `add` is compact, `mask` is full."""
    conv_case(knob, case, kind, "conv scatter")


# ---------------------------------------------------------------------------------- split-K
WINDOW = dict(N=3, H=6, W=6, C=16, R=4, S=4)
SPLITS = [
    # (problem, slices by design: min(8, K / 16 / 8) on any device of 18 or more CUs)
    (spec(Cout=64, **WINDOW), 2),                        # K = 256: the second slice begins at tap 8
    (rows1x1(129, C=400, Cout=100), 3),                  # K = 400: slices of 8, 8 and 9 steps
    (rows1x1(65, C=640, Cout=136), 5),                   # K = 640
    (spec(N=3, H=5, W=7, C=128, Cout=100, **HALO3), 8),  # K = 1152: 9 steps each, slice 1 begins inside tap 1
    (rows1x1(300, C=640, Cout=136), 5),                  # 3 x 3 and 3 x 2 tiles
]
SPLITK = [(also(c, **m), s, v, k) for c, s in SPLITS for m in (FWD, DG) for v, k in ((1, B64), (2, B128))] + \
         [(also(SPLITS[3][0], up2=1, Hf=10, Wf=13, **DG), 8, v, k) for v, k in ((1, B64), (2, B128))]


def run_splitk(knob, c, slices, v, kernel, kind, family, ws="exact", sk=4):
    nat = N()
    knob("conv_f32", v)
    knob("conv_f32_splitk", sk)
    Ho, Wo = out_hw(c)
    M, K = c.N * Ho * Wo, c.R * c.S * c.C
    BN = 64 if kernel == B64 else 128
    tiles = -(-M // 128) * -(-c.Cout // BN)
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    assert tiles <= 9 and cus >= 18, "the designed slice counts need 4 * CUs / tiles >= 8"
    plan = nat.conv_f32_splitk_plan(M, c.Cout, K, c.C, c.R * c.S)
    want = slices if sk else 1
    assert plan == (BN, tiles, want, tiles * want * 128 * BN if want > 1 else 0), f"plan {plan}, designed {want} slices"
    if ws == "exact" and sk:
        expect = [dict(kernel=kernel, slices=slices, grid=tiles * slices, m_per_split=0),
                  dict(kernel="combine64" if BN == 64 else "combine128", slices=slices, grid=2 * tiles, m_per_split=0)]
    else:
        expect = [dict(kernel=kernel, slices=1, grid=tiles, m_per_split=0)]
    run_conv(nat, also(c, ws=ws if sk else None), kind, expect, family)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", SPLITK, ids=[f"{c[3]}-ks{c[1]}-{name(c[0])}" for c in SPLITK])
def test_conv_splitk(knob, case, kind):
    """Slices into a workspace of exactly the planned floats (inside guards), then the combine with
    the fused epilogue of each 64-row half."""
    c, slices, v, kernel = case
    run_splitk(knob, c, slices, v, kernel, kind, "conv split-K")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("v,kernel", [(1, B64), (2, B128)])
@pytest.mark.parametrize("ws", ["short", None])
@pytest.mark.parametrize("epi", ["fwd", "dgrad"])
def test_conv_splitk_short_or_no_workspace_runs_unsplit(knob, epi, ws, v, kernel, kind):
    """A workspace one float short of the plan, or none: the same tile runs unsplit, gives the
    unsplit result and leaves the workspace alone."""
    c = also(SPLITS[1][0], **(FWD if epi == "fwd" else DG))
    run_splitk(knob, c, 3, v, kernel, kind, "conv split-K, unsplit", ws=ws)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("v,kernel", [(1, B64), (2, B128)])
def test_conv_splitk_off_runs_unsplit(knob, v, kernel, kind):
    run_splitk(knob, also(SPLITS[1][0], **DG), 3, v, kernel, kind, "conv split-K off", sk=0)


# -------------------------------------------------------------------------- weight gradients
W64, W64S, W128 = "wgrad64", "wgrad64_scalar", "wgrad128"


def wg(n, h, w, C, Cout, R=1, stride=1, pad=0):
    return NS(n=n, h=h, w=w, C=C, Cout=Cout, R=R, stride=stride, pad=pad)


def wname(c):
    return f"{c.n}x{c.h}x{c.w}x{c.C}-{c.R}x{c.R}s{c.stride}p{c.pad}-Cout{c.Cout}"


def run_wgrad(nat, c, kind, kernel, m_per_split=None, grid=None):
    """dw [Cout][K] += g.T @ A, dw preloaded with 0.5 at exactly Cout * K floats inside guards."""
    exact = kind == "exact"
    what = f"{kernel} [{wname(c)}] {kind}"
    g_ = gen(zlib.crc32(wname(c).encode()) * 2 + exact)
    Ho, Wo = (c.h + 2 * c.pad - c.R) // c.stride + 1, (c.w + 2 * c.pad - c.R) // c.stride + 1
    M, K = c.n * Ho * Wo, c.R * c.R * c.C
    x = tern(g_, c.n, c.h, c.w, c.C).float() if exact else randn(g_, c.n, c.h, c.w, c.C, dtype=F32)
    gy = tern(g_, M, c.Cout).float() if exact else randn(g_, M, c.Cout, dtype=F32)
    A = gather(x, c.h, c.w, c.R, c.R, c.stride, c.pad, Ho, Wo)
    ref, mag = gy.double().t() @ A, gy.double().abs().t() @ A.abs()
    if exact:
        precond("wgrad_f32", mag)
    dw = Out(c.Cout * K, F32, start=torch.full((c.Cout, K), 0.5, device=dev))
    nat.wgrad_f32(x, c.R, c.R, c.stride, c.pad, gy.view(c.n, Ho, Wo, c.Cout), dw.t.view(c.Cout, K))
    got = nat.conv_f32_last_launch()
    assert len(got) == 1 and got[0]["kernel"] == kernel and got[0]["slices"] == 1, f"{what}: launched {got}"
    mps = got[0]["m_per_split"]
    assert mps > 0 and mps % 16 == 0 and (m_per_split is None or mps == m_per_split), f"{what}: launched {got}"
    splits = -(-M // mps)
    side = 128 if kernel == W128 else 64
    assert got[0]["grid"] == -(-c.Cout // side) * -(-K // side) * splits, f"{what}: launched {got}"
    assert grid is None or got[0]["grid"] == grid, f"{what}: launched {got}"
    SEEN.setdefault(kernel, set()).add(splits)
    dw.check(what)
    # M products a sum, and one partial sum per split added by atomics onto the preloaded value
    check(kind, dw.t, ref + 0.5, mag + 0.5, M + splits, what, rounded=False)


WG64 = (
    # one-step and two-step reductions: M = 1, 15, 16, 17; K = 4 and Cout = 1, and one full tile
    [(wg(M, 1, 1, C, Cout), W64) for M in (1, 15, 16, 17) for C, Cout in ((4, 1), (64, 64))] +
    # Cout tails: 10 takes the ragged gradient loader (rows of 10 floats), 100 and 136 two row tiles
    [(wg(3, 5, 7, 64, Cout), W64) for Cout in (10, 100, 136)] +
    # K tails: the stem (scalar gather, K = 147), K = 40, K = 576 = 9 column tiles
    [(wg(2, 9, 11, 3, 64, R=7, stride=2, pad=3), W64S), (wg(3, 5, 7, 40, 64), W64),
     (wg(3, 5, 7, 64, 64, R=3, pad=1), W64)] +
    # strided: 1x1 / 2 / 0 and 3x3 / 2 / 1 on 5 x 7
    [(wg(3, 5, 7, 64, 64, stride=2), W64), (wg(3, 5, 7, 64, 64, R=3, stride=2, pad=1), W64)]
)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", WG64, ids=[f"{k}-{wname(c)}" for c, k in WG64])
def test_wgrad64(knob, case, kind):
    c, kernel = case
    knob("conv_f32", 0)
    run_wgrad(N(), c, kind, kernel)


@pytest.mark.parametrize("kind", KINDS)
def test_wgrad64_two_splits_begin_inside_an_image(knob, kind):
    """M = 300 rows of 10 x 10 images in two splits of 160 and 140: the second begins inside image 1
    and ends on a 12-row step."""
    knob("conv_f32", 0)
    run_wgrad(N(), wg(3, 10, 10, 64, 64), kind, W64, m_per_split=160, grid=2)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("v", [1, 2])
def test_wgrad64_where_the_wide_tiles_do_not_apply(knob, v, kind):
    """Cout = 64 keeps the 64 x 64 kernel by default; Cout % 4 != 0 keeps it even when forced."""
    knob("conv_f32", v)
    run_wgrad(N(), wg(3, 5, 7, 64, 64 if v == 1 else 10), kind, W64)


WG128 = [
    (wg(4, 1, 1, 256, 136), 1, None),                 # M = 4: one step, a Cout tail (the Dense shape in miniature)
    (wg(3, 14, 14, 128, 128), 1, 304),                # M = 588: splits of 304 and 284 rows, n_first = 1
    (wg(3, 14, 14, 16, 128, R=3, pad=1), 2, 304),     # K = 144: a 16-column second k-tile
    (wg(3, 5, 7, 64, 8), 2, None),                    # Cout = 8, K = 64: most of the tile empty
    (wg(3, 6, 6, 16, 128, R=4), 1, None),             # the 4x4 window, K = 256
    (wg(3, 6, 6, 16, 64, R=4), 2, None),
]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", WG128, ids=[f"knob{v}-{wname(c)}" for c, v, _ in WG128])
def test_wgrad128(knob, case, kind):
    """The 128 x 128 LDS-DMA weight gradient where the launcher takes it (knob 1: both sides at
    least 128 wide) and forced where it does not (knob 2)."""
    c, v, mps = case
    knob("conv_f32", v)
    run_wgrad(N(), c, kind, W128, m_per_split=mps, grid=None if mps is None else 2 * -(-c.R * c.R * c.C // 128))
