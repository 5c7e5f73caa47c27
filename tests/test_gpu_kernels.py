"""Numerics of every native HIP kernel against a plain PyTorch fp32 reference of the same op.

All tests run on the MI355X through the in-tree `_pddl_native` extension (no fallback).
bf16 inputs are generated once and the fp32 reference consumes the SAME rounded values,
so tolerances only cover fp32-accumulation order and the final bf16 rounding.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

dev = "cuda"


def N():
    from pddl.ops.native import require_native
    return require_native()


@pytest.fixture(autouse=True)
def _unsplit_by_default(request):
    """Kernel-equivalence tests compare tilings that must share one k order: split-K (on by
    default for small-M problems when the calling thread has a workspace current, e.g. after an
    engine ran) is switched off here and exercised explicitly by the split-K tests."""
    if "splitk" in request.node.name:
        yield
        return
    N().set_variant("igemm_splitk", 0)
    yield
    N().set_variant("igemm_splitk", 1)


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, device=dev) * scale).to(torch.bfloat16)


def conv_ref(x, w, stride, pad):
    # x NHWC, w OHWI -> NHWC fp32
    y = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1)


CONV_CASES = [
    # N, H, C, Cout, R, stride, pad
    (2, 14, 64, 64, 1, 1, 0),
    (3, 9, 64, 128, 3, 1, 1),
    (2, 14, 256, 512, 1, 2, 0),
    (2, 7, 128, 136, 3, 1, 1),
    (1, 15, 64, 256, 1, 2, 0),
    (2, 10, 192, 64, 1, 1, 0),
    (4, 8, 512, 64, 3, 1, 1),
]


@pytest.mark.parametrize("case", CONV_CASES)
@pytest.mark.parametrize("with_res", [False, True])
def test_igemm_forward(case, with_res):
    torch.manual_seed(0)
    n, h, c, co, r, st, pad = case
    x = rnd(n, h, h, c)
    w = rnd(co, r, r, c, scale=0.05)
    ho = (h + 2 * pad - r) // st + 1
    scale = torch.rand(co, device=dev) + 0.5
    shift = torch.randn(co, device=dev)
    res = rnd(n, ho, ho, co) if with_res else None
    out = torch.empty(n, ho, ho, co, dtype=torch.bfloat16, device=dev)
    N().igemm(x, None, h, h, r, r, st, pad, ho, ho, w.view(co, -1), 0, scale, shift, res, None, None, out, 1,
              None, 0, 0, 0, 0, 0, None, None)
    ref = conv_ref(x, w, st, pad) * scale + shift
    if with_res:
        ref = ref + res.float()
    ref = ref.relu()
    assert rel(out, ref) < 1e-2


def test_kernel_knobs_freeze_after_first_launch():
    """Tile knobs are process-global launch configuration: once a kernel has launched, set_variant
    raises unless tuning mode is on (tests / micro-benchmarks call allow_knob_changes(True)), so
    replica threads of one process can never see the launch plan change between their steps."""
    x = rnd(1, 4, 4, 64)
    w = rnd(64, 64)
    out = torch.empty(1, 4, 4, 64, dtype=torch.bfloat16, device=dev)
    ones, zeros = torch.ones(64, device=dev), torch.zeros(64, device=dev)
    N().igemm(x, None, 4, 4, 1, 1, 1, 0, 4, 4, w, 0, ones, zeros, None, None, None, out, 0, None, 0, 0, 0, 0, 0,
              None, None)
    N().allow_knob_changes(False)
    try:
        assert N().knobs_frozen()
        with pytest.raises(RuntimeError, match="read-only"):
            N().set_variant("igemm_pk", 0)
    finally:
        N().allow_knob_changes(True)
    assert not N().knobs_frozen()
    N().set_variant("igemm_pk", 2)   # (the default, restored in tuning mode)


def test_igemm_split_outputs_and_f32():
    torch.manual_seed(1)
    n, h, c, f = 2, 8, 64, 64
    x = rnd(n, h, h, c)
    w = rnd(5 * f, 1, 1, c, scale=0.1)
    scale = torch.rand(5 * f, device=dev) + 0.5
    shift = torch.randn(5 * f, device=dev)
    y1 = torch.empty(n, 4, 4, f, dtype=torch.bfloat16, device=dev)
    sc = torch.empty(n, 4, 4, 4 * f, dtype=torch.bfloat16, device=dev)
    N().igemm(x, None, h, h, 1, 1, 2, 0, 4, 4, w.view(5 * f, c), 0, scale, shift, None, None, None, y1, 1,
              sc, 0, f, 0, 0, 0, None, None)
    ref = conv_ref(x, w, 2, 0) * scale + shift
    assert rel(y1, ref[..., :f].relu()) < 1e-2
    assert rel(sc, ref[..., f:]) < 1e-2
    # fp32 dense epilogue
    a = rnd(6, 2048)
    wd = rnd(1000, 2048, scale=0.02)
    bias = torch.randn(1000, device=dev)
    ones = torch.ones(1000, device=dev)
    out = torch.empty(6, 1000, device=dev)
    N().igemm(a.view(6, 1, 1, 2048), None, 1, 1, 1, 1, 1, 0, 1, 1, wd, 2, ones, bias, None, None, None, out, 0,
              None, 0, 0, 0, 0, 0, None, None)
    ref = a.float() @ wd.float().t() + bias
    assert rel(out, ref) < 1e-3


def _fold(part, rows, C):
    import struct
    cs = torch.zeros(C, device=dev)
    tab = torch.frombuffer(bytearray(struct.pack("<q4i", 0, rows, C, 0, 0)), dtype=torch.uint8).clone().to(dev)
    N().colsum_reduce(part, tab, 1, cs)
    return cs


def dgrad_weights(w, a):
    # W'[c][r'][s'][co] = a[co] * W[co][R-1-r'][S-1-s'][c]
    wt = (w.float() * a.view(-1, 1, 1, 1)).flip(1).flip(2).permute(3, 1, 2, 0).contiguous()
    return wt.to(torch.bfloat16)


@pytest.mark.parametrize("case", [(2, 9, 64, 128, 3, 1, 1), (2, 14, 64, 256, 1, 1, 0), (2, 14, 256, 128, 1, 2, 0),
                                  (1, 15, 128, 64, 1, 2, 0)])
def test_igemm_dgrad(case):
    torch.manual_seed(2)
    n, h, cin, co, r, st, pad = case
    ho = (h + 2 * pad - r) // st + 1
    g = rnd(n, ho, ho, co)
    w = rnd(co, r, r, cin, scale=0.05)
    a = torch.rand(co, device=dev) + 0.5
    add = rnd(n, h, h, cin)
    mask = rnd(n, h, h, cin)
    out = torch.empty(n, h, h, cin, dtype=torch.bfloat16, device=dev)
    wt = dgrad_weights(w, a)
    pd = r - 1 - pad
    rows = N().igemm_partial_rows(n * ho * ho, cin, r * r * co)
    part = torch.full((rows * cin,), float("nan"), device=dev)
    N().igemm(g, None, ho, ho, r, r, 1, pd, ho, ho, wt.view(cin, -1), 1, None, None, None, mask, add, out, 0,
              None, 0, 0, 1 if st == 2 else 0, h, h, part, None)
    gs = (g.float() * a).permute(0, 3, 1, 2)
    ref = torch.nn.grad.conv2d_input((n, cin, h, h), w.float().permute(0, 3, 1, 2), gs, stride=st, padding=pad)
    ref = (ref.permute(0, 2, 3, 1) + add.float()) * (mask.float() > 0)
    assert rel(out, ref) < 1e-2
    cs = _fold(part, rows, cin)
    assert rel(cs, ref.sum((0, 1, 2))) < 1e-2


KNOB_DEFAULTS = {"igemm_pk": 2, "igemm_pf": 1}


@pytest.mark.parametrize("knob,big", [("igemm8", 1), ("igemm8", 2), ("igemm", 2), ("igemm_pf", 2)])
@pytest.mark.parametrize("kind", ["fwd3x3", "fwd1x1res", "dgrad_up2_dual", "fwd1x1resid", "dgrad1x1add"])
def test_igemm_big_tile_matches(kind, knob, big):
    """The 8-phase 256x256 kernel (igemm8 1, with the wave-row stagger 2), the forced 2-stage
    pipeline (igemm 2) and the epilogue-operand prefetch on single-stage dgrads (igemm_pf 2)
    compute the same result (same k order) as the default 4-wave 128x128 tile, including the
    fused epilogues and the per-wave column-sum rows.  These problems have 1-3 tiles of 256x256, so
    the 8-phase kernel is forced (knob + 16: whatever the grid) where the problem is one it takes
    (Nn a multiple of 256, K >= 256); igemm_last_launch() tells that it ran."""
    torch.manual_seed(12)
    n, h, ho = 3, 14, 7
    if kind == "fwd3x3":
        x = rnd(n, h, h, 128)
        w = rnd(256, 9 * 128, scale=0.05)
        sc, sh = torch.rand(256, device=dev) + 0.5, torch.randn(256, device=dev)
    elif kind == "fwd1x1res":
        x = rnd(n, h, h, 256)
        w = rnd(320, 256, scale=0.05)
        sc, sh = torch.rand(320, device=dev) + 0.5, torch.randn(320, device=dev)
    elif kind == "fwd1x1resid":      # short-K 1x1 with a residual (the early-prefetch path)
        x = rnd(n, h, h, 128)
        w = rnd(512, 128, scale=0.05)
        sc, sh = torch.rand(512, device=dev) + 0.5, torch.randn(512, device=dev)
        res = rnd(n, h, h, 512)
    elif kind == "dgrad1x1add":      # short-K 1x1 dgrad: residual-gradient add + ReLU bits + column sums
        g = rnd(n, h, h, 64)
        wt = rnd(256, 64, scale=0.05)
        addv = rnd(n, h, h, 256)
        bits = pack_bits(rnd(n, h, h, 256))
    else:
        g1, g0 = rnd(n, ho, ho, 128), rnd(n, ho, ho, 512)
        wt = rnd(256, 640, scale=0.05)
        mask = rnd(n, h, h, 256)
    outs = []
    N().set_variant("igemm8_min_tiles", 1)
    N().set_variant("igemm8_min_n", 256)       # (tiny problems: let the 8-phase kernel take them)
    N().set_variant("igemm8", 0)                 # baseline: the 128x128 tile
    default = KNOB_DEFAULTS.get(knob, 0)
    for kv in (0, big + 16 if knob == "igemm8" else big):
        N().set_variant(knob, kv)
        try:
            if kind == "fwd3x3":
                y = torch.empty(n, h, h, 256, dtype=torch.bfloat16, device=dev)
                N().igemm(x, None, h, h, 3, 3, 1, 1, h, h, w, 0, sc, sh, None, None, None, y, 1, None, 0, 0, 0, 0, 0,
                          None, None)
                outs.append(y.float())
            elif kind == "fwd1x1resid":
                y = torch.empty(n, h, h, 512, dtype=torch.bfloat16, device=dev)
                bo = torch.zeros(n, h, h, 64, dtype=torch.uint8, device=dev)
                N().igemm(x, None, h, h, 1, 1, 1, 0, h, h, w, 0, sc, sh, res, None, None, y, 1, None, 0, 0, 0, 0, 0,
                          None, bo)
                outs.append(torch.cat([y.float().flatten(), bo.float().flatten()]))
            elif kind == "dgrad1x1add":
                out = torch.empty(n, h, h, 256, dtype=torch.bfloat16, device=dev)
                rows = N().igemm_partial_rows(n * h * h, 256, 64)
                part = torch.full((rows * 256,), float("nan"), device=dev)
                N().igemm(g, None, h, h, 1, 1, 1, 0, h, h, wt, 1, None, None, None, bits, addv, out, 0, None, 0, 0,
                          0, 0, 0, part, None)
                outs.append(torch.cat([out.float().flatten(), _fold(part, rows, 256)]))
            elif kind == "fwd1x1res":
                y1 = torch.empty(n, h, h, 64, dtype=torch.bfloat16, device=dev)
                y2 = torch.empty(n, h, h, 256, dtype=torch.bfloat16, device=dev)
                bits = torch.zeros(n, h, h, 8, dtype=torch.uint8, device=dev)
                N().igemm(x, None, h, h, 1, 1, 1, 0, h, h, w, 0, sc, sh, None, None, None, y1, 1, y2, 0, 64, 0, 0, 0,
                          None, bits)
                outs.append(torch.cat([y1.float().flatten(), y2.float().flatten(), bits.float().flatten()]))
            else:
                out = torch.empty(n, h, h, 256, dtype=torch.bfloat16, device=dev)
                rows = N().igemm_partial_rows(n * ho * ho, 256, 640)
                part = torch.full((rows * 256,), float("nan"), device=dev)
                N().igemm(g1, g0, ho, ho, 1, 1, 1, 0, ho, ho, wt, 1, None, None, None, mask, None, out, 0, None, 0, 0,
                          1, h, h, part, None)
                outs.append(torch.cat([out.float().flatten(), _fold(part, rows, 256)]))
            ran = [l["kernel"] for l in N().igemm_last_launch()]
            if knob == "igemm8" and kv and kind in ("fwd3x3", "dgrad_up2_dual"):
                assert ran == ["igemm8_stagger" if big == 2 else "igemm8"], ran
            else:
                assert "igemm8" not in ran and "igemm8_stagger" not in ran, ran
        finally:
            N().set_variant(knob, default)
    N().set_variant("igemm8_min_tiles", 128)
    N().set_variant("igemm8_min_n", 512)
    N().set_variant("igemm8", 2)
    assert rel(outs[1], outs[0]) < 1e-5


@pytest.mark.parametrize("stagger", [1, 2])
def test_igemm8_round_split_dgrad_colsum(stagger):
    """A problem whose 256x256 tiles leave a partial last round (300 tiles on 256 CUs) runs the
    full rounds on the 8-phase kernel and the M-tail on the 128x128 tile (two launches, one
    partial-row table): output and fused column sums equal the single-kernel result."""
    torch.manual_seed(23)
    n, h, cin, co = 3, 160, 256, 256            # M = 76800 rows = 300 x 256
    g = rnd(n, h, h, co)
    wt = rnd(cin, co, scale=0.05)
    add, mask = rnd(n, h, h, cin), rnd(n, h, h, cin)
    outs = []
    N().set_variant("igemm8_min_n", 256)
    for kv in (0, stagger):
        N().set_variant("igemm8", kv)
        try:
            out = torch.empty(n, h, h, cin, dtype=torch.bfloat16, device=dev)
            rows = N().igemm_partial_rows(n * h * h, cin, co)
            part = torch.full((rows * cin,), float("nan"), device=dev)
            N().igemm(g, None, h, h, 1, 1, 1, 0, h, h, wt, 1, None, None, None, mask, add, out, 0, None, 0, 0, 0, 0, 0,
                      part, None)
            outs.append((out.float(), _fold(part, rows, cin), rows))
        finally:
            N().set_variant("igemm8", 2)
    N().set_variant("igemm8_min_n", 512)
    (o0, c0, r0), (o1, c1, r1) = outs
    assert r0 == r1 == 1200          # (both tilings keep 4 partial rows per 256 GEMM rows)
    assert rel(o1, o0) < 1e-5 and rel(c1, c0) < 1e-4


@pytest.mark.parametrize("stagger", [1, 2])
@pytest.mark.parametrize("case", [
    # N, H, C, Cout, R, stride, pad   (conv4 / conv5 3x3, a strided 1x1 with tile overhang, long-K 1x1)
    (4, 14, 256, 256, 3, 1, 1),
    (5, 7, 512, 512, 3, 1, 1),
    (3, 15, 512, 1280, 1, 2, 0),
    (2, 9, 2048, 512, 1, 1, 0),
])
def test_igemm8_forward_vs_fp32(case, stagger):
    """8-phase kernel against the fp32 conv reference on ResNet-50 stage-4/5 shapes (K up to
    4608 = 72 K-tiles through the counted-vmcnt pipeline; M tails).  The grids are 1-15 tiles, so
    the kernel is forced (knob + 16) and igemm_last_launch() tells that it ran.  (Widths that are
    not a multiple of 256 never plan this kernel: the long-K 1x1 has Nn = 512.)"""
    torch.manual_seed(21)
    n, h, c, co, r, st, pad = case
    x = rnd(n, h, h, c)
    w = rnd(co, r, r, c, scale=0.03)
    ho = (h + 2 * pad - r) // st + 1
    scale = torch.rand(co, device=dev) + 0.5
    shift = torch.randn(co, device=dev)
    res = rnd(n, ho, ho, co)
    out = torch.empty(n, ho, ho, co, dtype=torch.bfloat16, device=dev)
    N().set_variant("igemm8_min_tiles", 1)
    N().set_variant("igemm8_min_n", 256)
    N().set_variant("igemm8", 16 + stagger)
    try:
        for _ in range(3):       # repeated launches: a pipeline race would show up as a changing result
            N().igemm(x, None, h, h, r, r, st, pad, ho, ho, w.view(co, -1), 0, scale, shift, res, None, None, out, 1,
                      None, 0, 0, 0, 0, 0, None, None)
            ran = [l["kernel"] for l in N().igemm_last_launch()]
            assert ran == ["igemm8_stagger" if stagger == 2 else "igemm8"], ran
            ref = (conv_ref(x, w, st, pad) * scale + shift + res.float()).relu()
            assert rel(out, ref) < 1e-2
    finally:
        N().set_variant("igemm8", 2)
        N().set_variant("igemm8_min_tiles", 128)
        N().set_variant("igemm8_min_n", 512)


def test_igemm_dgrad_dual_source():
    torch.manual_seed(3)
    n, h, cin, f = 2, 14, 256, 128
    ho = 7
    g1 = rnd(n, ho, ho, f)
    g0 = rnd(n, ho, ho, 4 * f)
    w1 = rnd(f, 1, 1, cin, scale=0.05)
    w0 = rnd(4 * f, 1, 1, cin, scale=0.05)
    a1 = torch.rand(f, device=dev) + 0.5
    a0 = torch.rand(4 * f, device=dev) + 0.5
    wt = torch.cat([dgrad_weights(w1, a1).view(cin, f), dgrad_weights(w0, a0).view(cin, 4 * f)], 1).contiguous()
    mask = rnd(n, h, h, cin)
    out = torch.empty(n, h, h, cin, dtype=torch.bfloat16, device=dev)
    N().igemm(g1, g0, ho, ho, 1, 1, 1, 0, ho, ho, wt, 1, None, None, None, mask, None, out, 0, None, 0, 0, 1, h, h,
              None, None)
    r1 = torch.nn.grad.conv2d_input((n, cin, h, h), w1.float().permute(0, 3, 1, 2),
                                    (g1.float() * a1).permute(0, 3, 1, 2), stride=2)
    r0 = torch.nn.grad.conv2d_input((n, cin, h, h), w0.float().permute(0, 3, 1, 2),
                                    (g0.float() * a0).permute(0, 3, 1, 2), stride=2)
    ref = (r1 + r0).permute(0, 2, 3, 1) * (mask.float() > 0)
    assert rel(out, ref) < 1e-2


@pytest.mark.parametrize("shape", [(64, 64, 1, 11), (128, 256, 2, 9), (256, 512, 2, 7), (512, 1024, 2, 5)])
@pytest.mark.parametrize("ring", [0, 24])
def test_igemm_dual_source_forward(shape, ring):
    """The projection block's fused conv3 + shortcut forward (two A sources along K, the shortcut
    at its own geometry and stride) against fp32: on the persistent ring (igemm_pk_kernel DUAL,
    K / 64 = 2, 6, 12, 24) and on the per-tile kernels; odd spatial sizes give partial row tiles,
    the ReLU bits are checked against the output's signs."""
    torch.manual_seed(23)
    f, cin, st, ho = shape
    n, h = 3, (ho - 1) * st + 1 + (st - 1)
    y2 = rnd(n, ho, ho, f)
    x = rnd(n, h, h, cin)
    w3 = rnd(4 * f, 1, 1, f, scale=0.05)
    w0 = rnd(4 * f, 1, 1, cin, scale=0.05)
    wcat = torch.cat([w3.view(4 * f, f), w0.view(4 * f, cin)], 1).contiguous()
    sc, sh = torch.rand(4 * f, device=dev) + 0.5, torch.randn(4 * f, device=dev)
    out = torch.empty(n, ho, ho, 4 * f, dtype=torch.bfloat16, device=dev)
    bits = torch.empty(n, ho, ho, f // 2, dtype=torch.uint8, device=dev)
    N().set_variant("igemm_pk_dual", ring)
    try:
        N().igemm(y2, x, ho, ho, 1, 1, 1, 0, ho, ho, wcat, 0, sc, sh, None, None, None, out, 1, None, 0, 0, 0, 0, 0,
                  None, bits)
        torch.cuda.synchronize()
    finally:
        N().set_variant("igemm_pk_dual", 2)
    ref = ((conv_ref(y2, w3, 1, 0) + conv_ref(x, w0, st, 0)) * sc + sh).relu()
    assert rel(out, ref) < 1e-2
    assert torch.equal(bits, pack_bits(out))


def pack_bits(x):
    """Reference ReLU bitmask: bit e of byte [..., c // 8] is (x[..., 8 * (c // 8) + e] > 0)."""
    b = (x.float() > 0).to(torch.int32).view(*x.shape[:-1], x.shape[-1] // 8, 8)
    return (b << torch.arange(8, device=x.device, dtype=torch.int32)).sum(-1).to(torch.uint8)


def test_bitmask_forward_and_dgrad():
    torch.manual_seed(9)
    n, h, c, f = 2, 8, 64, 64
    x = rnd(n, h, h, c)
    w = rnd(5 * f, 1, 1, c, scale=0.1)
    scale = torch.rand(5 * f, device=dev) + 0.5
    shift = torch.randn(5 * f, device=dev)
    y1 = torch.empty(n, h, h, f, dtype=torch.bfloat16, device=dev)
    sc = torch.empty(n, h, h, 4 * f, dtype=torch.bfloat16, device=dev)
    bits = torch.full((n, h, h, f // 8), 0xAA, dtype=torch.uint8, device=dev)
    N().igemm(x, None, h, h, 1, 1, 1, 0, h, h, w.view(5 * f, c), 0, scale, shift, None, None, None, y1, 1,
              sc, 0, f, 0, 0, 0, None, bits)
    assert torch.equal(bits, pack_bits(y1))
    # a dgrad masked by the bits equals the same dgrad masked by the bf16 tensor
    g = rnd(n, h, h, 4 * f)
    wt = rnd(f, 4 * f, scale=0.05)
    o1 = torch.empty(n, h, h, f, dtype=torch.bfloat16, device=dev)
    o2 = torch.empty_like(o1)
    for m, o in ((y1, o1), (bits, o2)):
        N().igemm(g, None, h, h, 1, 1, 1, 0, h, h, wt, 1, None, None, None, m, None, o, 0, None, 0, 0, 0, 0, 0,
                  None, None)
    assert torch.equal(o1, o2)
    # maxpool forward bits
    xp = torch.relu(torch.randn(n, 12, 12, c, device=dev)).to(torch.bfloat16)
    yp = torch.empty(n, 6, 6, c, dtype=torch.bfloat16, device=dev)
    idx = torch.empty(n, 6, 6, c, dtype=torch.uint8, device=dev)
    pb = torch.empty(n, 6, 6, c // 8, dtype=torch.uint8, device=dev)
    N().maxpool_fwd(xp, yp, idx, pb)
    assert torch.equal(pb, pack_bits(yp))


@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("aligned", [True, False])
def test_bits_out_packed_and_unaligned(ring, aligned):
    """The forward epilogues' ReLU-bit side output (one byte per lane) equals the bf16 output's
    signs and writes nothing outside the mask, at an aligned and an odd byte offset, on the
    per-tile kernel (with an M tail and a split second output) and on the ring kernel (residual
    forward, K = 128).  (A packed 4-byte store of four lanes' bytes measured slower and was
    removed, profiles/r4_bits_pkdual.txt.)"""
    torch.manual_seed(19)
    n, h = 3, 37                                   # M = 4107 rows: a partial last row tile
    K, Nn = (128, 256) if ring else (64, 320)
    x = rnd(n, h, h, K)
    w = rnd(Nn, K, scale=0.1)
    sc, sh = torch.rand(Nn, device=dev) + 0.5, torch.randn(Nn, device=dev)
    f = 64 if not ring else Nn                     # (per-tile: y1 = first 64 columns, the rest to out2)
    nb = n * h * h * f // 8
    raw = torch.full((nb + 4,), 0x5A, dtype=torch.uint8, device=dev)
    bits = (raw[:nb] if aligned else raw[1:nb + 1]).view(n, h, h, f // 8)
    y = torch.empty(n, h, h, f, dtype=torch.bfloat16, device=dev)
    if ring:
        res = rnd(n, h, h, Nn)
        N().igemm(x, None, h, h, 1, 1, 1, 0, h, h, w, 0, sc, sh, res, None, None, y, 1, None, 0, 0, 0, 0, 0, None,
                  bits)
    else:
        y2 = torch.empty(n, h, h, Nn - f, dtype=torch.bfloat16, device=dev)
        N().igemm(x, None, h, h, 1, 1, 1, 0, h, h, w, 0, sc, sh, None, None, None, y, 1, y2, 0, f, 0, 0, 0, None,
                  bits)
    torch.cuda.synchronize()
    assert torch.equal(bits, pack_bits(y))
    # nothing outside the mask was written
    if aligned:
        assert torch.equal(raw[nb:], torch.full((4,), 0x5A, dtype=torch.uint8, device=dev))
    else:
        assert raw[0].item() == 0x5A and torch.equal(raw[nb + 1:], torch.full((3,), 0x5A, dtype=torch.uint8, device=dev))


WG_CASES = [
    (2, 14, 64, 256, 1, 1, 0),
    (3, 9, 64, 64, 3, 1, 1),
    (2, 14, 256, 512, 1, 2, 0),
    (2, 7, 128, 128, 3, 1, 1),
    (4, 28, 64, 64, 1, 1, 0),
]


@pytest.mark.parametrize("case", WG_CASES)
def test_wgrad(case):
    torch.manual_seed(4)
    n, h, cin, co, r, st, pad = case
    ho = (h + 2 * pad - r) // st + 1
    x = rnd(n, h, h, cin)
    g = rnd(n, ho, ho, co)
    dw = torch.zeros(co, r * r * cin, device=dev)
    N().wgrad(x, h, h, r, r, st, pad, ho, ho, g, None, 0, dw, r * r * cin, 0)
    ref = torch.nn.grad.conv2d_weight(x.float().permute(0, 3, 1, 2), (co, cin, r, r),
                                      g.float().permute(0, 3, 1, 2), stride=st, padding=pad)
    ref = ref.permute(0, 2, 3, 1).reshape(co, -1)
    assert rel(dw, ref) < 5e-3


@pytest.mark.parametrize("case", WG_CASES)
def test_wgrad_single_stage_matches_double(case):
    """The single-LDS-stage 128-wide wgrad (knob wgrad1=2; the default 1 picks it for all but
    the long-reduction 1x1 / stem layers) equals the 2-stage one (wgrad1=0)."""
    torch.manual_seed(6)
    n, h, cin, co, r, st, pad = case
    ho = (h + 2 * pad - r) // st + 1
    x = rnd(n, h, h, cin)
    g = rnd(n, ho, ho, co)
    outs = []
    try:
        for kv in (0, 2):
            N().set_variant("wgrad1", kv)
            dw = torch.zeros(co, r * r * cin, device=dev)
            N().wgrad(x, h, h, r, r, st, pad, ho, ho, g, None, 0, dw, r * r * cin, 0)
            outs.append(dw)
    finally:
        N().set_variant("wgrad1", 1)
    assert rel(outs[1], outs[0]) < 1e-5


def test_wgrad_dual_and_padded_k():
    torch.manual_seed(5)
    # dual gradient source (conv1 + conv0 of a projection block)
    n, h, cin, f = 2, 8, 128, 64
    x = rnd(n, h, h, cin)
    g1 = rnd(n, h, h, f)
    g0 = rnd(n, h, h, 4 * f)
    dw = torch.zeros(5 * f, cin, device=dev)
    N().wgrad(x, h, h, 1, 1, 1, 0, h, h, g1, g0, f, dw, cin, 0)
    ref = torch.cat([g1, g0], -1).float().reshape(-1, 5 * f).t() @ x.float().reshape(-1, cin)
    assert rel(dw, ref) < 5e-3
    # stem-style: rows of 192, only the first 147 columns, Cout 64; dense-style Cout 1000
    a = rnd(3, 5, 5, 192)
    g = rnd(3, 5, 5, 64)
    dw = torch.zeros(64, 147, device=dev)
    N().wgrad(a, 5, 5, 1, 1, 1, 0, 5, 5, g, None, 0, dw, 147, 0)
    ref = g.float().reshape(-1, 64).t() @ a.float().reshape(-1, 192)[:, :147]
    assert rel(dw, ref) < 5e-3
    p = rnd(16, 2048)
    dl = torch.zeros(16, 1024, dtype=torch.bfloat16, device=dev)
    dl[:, :1000] = rnd(16, 1000)
    dw = torch.zeros(1000, 2048, device=dev)
    N().wgrad(p.view(16, 1, 1, 2048), 1, 1, 1, 1, 1, 0, 1, 1, dl, None, 0, dw, 2048, 0)
    ref = dl[:, :1000].float().t() @ p.float()
    assert rel(dw, ref) < 5e-3


@pytest.mark.parametrize("stagger", [1, 2])
@pytest.mark.parametrize("case", [
    (4, 14, 1024, 256, 1, 1, 0),     # 1x1 s1 (direct rows), K = 1024
    (8, 14, 256, 256, 3, 1, 1),      # 3x3 pad 1: arithmetic im2col gather, 9 taps
    (4, 14, 256, 256, 3, 2, 1),      # 3x3 s2 (v1.5 downsampling conv2)
    (4, 14, 512, 1024, 1, 2, 0),     # 1x1 s2 projection: gather path with one tap
    (3, 11, 264, 320, 1, 1, 0),      # M, Cout and K tails of the 256x256 tile
    (32, 14, 256, 512, 1, 1, 0),     # several m splits per tile
])
def test_wgrad8_vs_fp32(case, stagger):
    """8-phase 256x256 weight-gradient kernel against the fp32 reference and the 128-wide
    kernel, repeated (a staging race would show up as a changing result).  These grids are
    smaller than the launcher's fill threshold, so the kernel is forced (knob +16)."""
    torch.manual_seed(31)
    n, h, cin, co, r, st, pad = case
    ho = (h + 2 * pad - r) // st + 1
    x = rnd(n, h, h, cin)
    g = rnd(n, ho, ho, co)
    ref = torch.nn.grad.conv2d_weight(x.float().permute(0, 3, 1, 2), (co, cin, r, r),
                                      g.float().permute(0, 3, 1, 2), stride=st, padding=pad)
    ref = ref.permute(0, 2, 3, 1).reshape(co, -1)
    outs = []
    try:
        for kv in (0, 16 + stagger, 16 + stagger, 16 + stagger):
            N().set_variant("wgrad8", kv)
            dw = torch.zeros(co, r * r * cin, device=dev)
            N().wgrad(x, h, h, r, r, st, pad, ho, ho, g, None, 0, dw, r * r * cin, 0)
            assert rel(dw, ref) < 5e-3
            outs.append(dw)
    finally:
        N().set_variant("wgrad8", 1)
    for o in outs[1:]:
        assert rel(o, outs[0]) < 1e-4
    assert rel(outs[2], outs[1]) < 1e-5


BIG_CASES = [
    # N, H, C, Cout, R, stride, pad: each input is larger than the 31-bit buffer range
    (5400, 56, 64, 64, 3, 1, 1),      # 3x3 halo gather: igemm AM_HALO, wgrad rowinfo gather
    (1400, 56, 256, 256, 1, 1, 0),    # 1x1 rows: igemm direct, wgrad8 direct
    (21500, 14, 256, 256, 3, 1, 1),   # 3x3 on wgrad8's stepped gather
]


@pytest.mark.parametrize("case", BIG_CASES)
def test_operands_beyond_2gib(case):
    """Activations larger than 2 GiB (b2048 training: the stage-1 tensors are 3.3 GB) go through
    the per-tile / per-split rebased buffer descriptors.  Only the first and last 3 images are
    non-zero, so an offset that wraps or starts from the wrong image shows up as wrong values
    there or as non-zeros in between (forward), or as a wrong weight gradient."""
    torch.manual_seed(7)
    n, h, c, co, r, st, pad = case
    ho = (h + 2 * pad - r) // st + 1
    assert n * h * h * c * 2 > 2 ** 31
    x = torch.zeros(n, h, h, c, dtype=torch.bfloat16, device=dev)
    g = torch.zeros(n, ho, ho, co, dtype=torch.bfloat16, device=dev)
    ends = [slice(0, 3), slice(n - 3, n)]
    for s in ends:
        x[s] = rnd(3, h, h, c)
        g[s] = rnd(3, ho, ho, co)
    w = rnd(co, r, r, c, scale=0.05)
    ones, zero = torch.ones(co, device=dev), torch.zeros(co, device=dev)
    out = torch.empty(n, ho, ho, co, dtype=torch.bfloat16, device=dev)
    N().igemm(x, None, h, h, r, r, st, pad, ho, ho, w.view(co, -1), 0, ones, zero, None, None, None, out, 0,
              None, 0, 0, 0, 0, 0, None, None)
    for s in ends:
        assert rel(out[s], conv_ref(x[s], w, st, pad)) < 1e-2
    assert out[3:n - 3].count_nonzero().item() == 0
    del out
    dw = torch.zeros(co, r * r * c, device=dev)
    N().wgrad(x, h, h, r, r, st, pad, ho, ho, g, None, 0, dw, r * r * c, 0)
    ref = sum(torch.nn.grad.conv2d_weight(x[s].float().permute(0, 3, 1, 2), (co, c, r, r),
                                          g[s].float().permute(0, 3, 1, 2), stride=st, padding=pad) for s in ends)
    assert rel(dw, ref.permute(0, 2, 3, 1).reshape(co, -1)) < 5e-3


@pytest.mark.parametrize("h,c", [(12, 64), (13, 64), (35, 64), (13, 128), (18, 256), (12, 32), (13, 8)])
def test_maxpool_and_gap(h, c):
    """Max pool (pad 1, 3x3/s2; the row-streaming kernels for C = 64 / 128 / 256, the per-output
    and per-pixel ones otherwise) against PyTorch, including odd sizes and partial column bands,
    then GAP."""
    torch.manual_seed(6)
    _maxpool_gap(h, c)


def _maxpool_gap(h, c):
    n = 2
    x = torch.relu(torch.randn(n, h, h, c, device=dev)).to(torch.bfloat16)
    ho = (h + 2 - 3) // 2 + 1
    y = torch.empty(n, ho, ho, c, dtype=torch.bfloat16, device=dev)
    idx = torch.empty(n, ho, ho, c, dtype=torch.uint8, device=dev)
    N().maxpool_fwd(x, y, idx, None)
    xr = x.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
    yr = F.max_pool2d(F.pad(xr, (1, 1, 1, 1)), 3, 2)
    assert torch.equal(y.float(), yr.permute(0, 2, 3, 1).detach())
    gy = rnd(n, ho, ho, c)
    yr.backward(gy.float().permute(0, 3, 1, 2))
    gx = torch.empty_like(x)
    rows = N().maxpool_bwd_partial_rows(n, h, h, c)
    part = torch.full((rows * c,), float("nan"), device=dev)
    N().maxpool_bwd(gy, idx, x, gx, part)
    ref = xr.grad.permute(0, 2, 3, 1) * (x.float() > 0)
    assert rel(gx, ref) < 1e-2
    assert rel(_fold(part, rows, c), ref.sum((0, 1, 2))) < 1e-2
    # GAP
    z = torch.relu(torch.randn(n, 7, 7, 256, device=dev)).to(torch.bfloat16)
    p = torch.empty(n, 256, dtype=torch.bfloat16, device=dev)
    N().gap_fwd(z, p)
    assert rel(p, z.float().mean((1, 2))) < 1e-2
    gp = rnd(n, 256)
    gz = torch.empty_like(z)
    part = torch.full((n * 256,), float("nan"), device=dev)
    N().gap_bwd(gp, z, gz, part)
    ref = (gp.float() / 49).view(n, 1, 1, 256) * (z.float() > 0)
    assert rel(gz, ref) < 1e-2
    assert rel(_fold(part, n, 256), ref.sum((0, 1, 2))) < 1e-2


def test_colsum_softmax_xent():
    torch.manual_seed(7)
    g = rnd(1000, 64)
    out = torch.zeros(64, device=dev)
    N().colsum(g, 64, out)
    assert rel(out, g.float().sum(0)) < 1e-4
    g = rnd(3000, 2048)
    out = torch.zeros(2048, device=dev)
    N().colsum(g, 2048, out)
    assert rel(out, g.float().sum(0)) < 1e-4
    B = 37
    logits = torch.randn(B, 1000, device=dev) * 3
    lab = torch.randint(0, 1000, (B,), device=dev)
    dl = torch.empty(B, 1024, dtype=torch.bfloat16, device=dev)
    ls = torch.zeros(1, device=dev)
    cr = torch.zeros(1, device=dev)
    N().softmax_xent(logits, lab, 1000, 1.0 / B, dl, ls, cr)
    lr = logits.clone().requires_grad_(True)
    loss = F.cross_entropy(lr, lab, reduction="sum")
    (loss / B).backward()
    assert abs(ls.item() - loss.item()) / loss.item() < 1e-5
    assert cr.item() == (logits.argmax(1) == lab).sum().item()
    assert rel(dl[:, :1000], lr.grad) < 1e-2
    assert dl[:, 1000:].float().abs().max().item() == 0


def test_optimizers():
    torch.manual_seed(8)
    n = 4096
    p = torch.randn(n, device=dev)
    g = torch.randn(n, device=dev)
    m = torch.randn(n, device=dev).abs() * 0.1
    v = torch.rand(n, device=dev) * 0.1
    pr, mr, vr = p.clone(), m.clone(), v.clone()
    lr, b1, b2, eps, t = 1e-3, 0.9, 0.999, 1e-7, 3
    lr_t = lr * (1 - b2 ** t) ** 0.5 / (1 - b1 ** t)
    N().adam(p, g, m, v, lr_t, b1, b2, eps, 1.0, None)
    mr = b1 * mr + (1 - b1) * g
    vr = b2 * vr + (1 - b2) * g * g
    pr = pr - lr_t * mr / (vr.sqrt() + eps)
    assert torch.allclose(p, pr, atol=1e-6) and torch.allclose(m, mr, atol=1e-6) and torch.allclose(v, vr, atol=1e-6)
    mom = torch.randn(n, device=dev)
    p2, mo2 = p.clone(), mom.clone()
    N().sgd(p, g, mom, 0.1, 0.9, 0.0, False, 1.0, None)
    mo2 = 0.9 * mo2 - 0.1 * g
    assert torch.allclose(mom, mo2, atol=1e-6) and torch.allclose(p, p2 + mo2, atol=1e-6)


def test_device_hparams_adam_steps():
    """hs = {t, lr, lr_t} advanced on the device reproduces the host bias-corrected steps."""
    torch.manual_seed(10)
    n = 1024
    p, g = torch.randn(n, device=dev), torch.randn(n, device=dev)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    pr, mr, vr = p.clone(), m.clone(), v.clone()
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-7
    hs = torch.tensor([0.0, lr, 0.0, 0.0], device=dev)
    for t in range(1, 6):
        N().opt_hparams(hs, b1, b2, True)
        N().adam(p, g, m, v, 0.0, b1, b2, eps, 1.0, hs)
        lr_t = lr * (1 - b2 ** t) ** 0.5 / (1 - b1 ** t)
        mr = b1 * mr + (1 - b1) * g
        vr = b2 * vr + (1 - b2) * g * g
        pr = pr - lr_t * mr / (vr.sqrt() + eps)
    assert hs[0].item() == 5.0
    assert torch.allclose(p, pr, atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("S,crop,oy,ox", [(32, 32, 0, 0), (35, 24, 3, 5), (224, 224, 0, 0), (250, 244, 2, 1)])
def test_stem_s2d_row_form_matches_pixel_form(S, crop, oy, ox):
    """Row-staged stem (knob stem=1, default for uint8 identity / crop) is bitwise equal to the
    per-pixel form, with flips, odd source widths and unaligned crop offsets."""
    torch.manual_seed(10)
    B = 3
    img = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device=dev)
    flip = torch.tensor([0, 1, 1], dtype=torch.uint8, device=dev)
    hs = (crop + 6) // 2
    m = 0 if crop == S else 2
    outs = []
    try:
        for v in (0, 1):
            N().set_variant("stem", v)
            x2 = torch.full((B, hs, hs, 16), float("nan"), dtype=torch.bfloat16, device=dev)
            N().stem_s2d(img, flip, m, crop, crop, oy, ox, x2, None)
            outs.append(x2)
    finally:
        N().set_variant("stem", 1)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("mode", ["identity", "resize", "crop"])
def test_stem_s2d_conv_and_wgrad(mode):
    """Preprocess + space-to-depth + 4x4 window igemm == Keras stem conv (7x7/s2 after
    ZeroPadding2D(3)); s2d wgrad folded back == conv2d_weight."""
    from pddl.models.reference import preprocess
    torch.manual_seed(9)
    B, S = 2, 32
    img = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device=dev)
    flip = torch.tensor([0, 1], dtype=torch.uint8, device=dev)
    crop = {"identity": 32, "resize": 40, "crop": 24}[mode]
    m = {"identity": 0, "resize": 1, "crop": 2}[mode]
    oy, ox = (3, 5) if mode == "crop" else (0, 0)
    hs = (crop + 6) // 2
    ho = crop // 2
    x2 = torch.empty(B, hs, hs, 16, dtype=torch.bfloat16, device=dev)
    N().stem_s2d(img, flip, m, crop, crop, oy, ox, x2, None)
    if mode == "crop":   # the device-offset form (graph replays) gives the same image
        x2d = torch.empty_like(x2)
        N().stem_s2d(img, flip, m, crop, crop, 0, 0, x2d, torch.tensor([oy, ox], dtype=torch.int32, device=dev))
        assert torch.equal(x2d, x2)
    x = preprocess(img, crop, True, flip, (oy, ox))                 # NCHW fp32
    ref_x2 = F.pixel_unshuffle(F.pad(x, (3, 3, 3, 3)), 2)           # [B, 3*4, hs, hs]  (c, dy, dx)
    got = x2.float().view(B, hs, hs, 2, 2, 4)[..., :3].permute(0, 5, 3, 4, 1, 2).reshape(B, 12, hs, hs)
    assert rel(got, ref_x2) < 5e-3
    # conv through the window GEMM with weights in the s2d layout
    w = torch.randn(64, 7, 7, 3, device=dev) * 0.05
    w2 = torch.zeros(64, 4, 4, 2, 2, 4, device=dev)
    for r in range(7):
        for s_ in range(7):
            w2[:, r // 2, s_ // 2, r % 2, s_ % 2, :3] = w[:, r, s_, :]
    w2 = w2.view(64, 256).to(torch.bfloat16)
    ones, zeros = torch.ones(64, device=dev), torch.zeros(64, device=dev)
    y = torch.empty(B, ho, ho, 64, dtype=torch.bfloat16, device=dev)
    N().igemm(x2, None, hs, hs, 4, 4, 1, 0, ho, ho, w2, 0, ones, zeros, None, None, None, y, 0, None, 0, 0, 0, 0, 0,
              None, None)
    xb = x2.float().view(B, hs, hs, 2, 2, 4)[..., :3].permute(0, 5, 1, 3, 2, 4).reshape(B, 3, 2 * hs, 2 * hs)
    wq = w2.float().view(64, 4, 4, 2, 2, 4)[..., :3]
    wq = wq.permute(0, 5, 1, 3, 2, 4).reshape(64, 3, 8, 8)[:, :, :7, :7]
    ref = F.conv2d(xb, wq, stride=2).permute(0, 2, 3, 1)
    assert rel(y, ref) < 1e-2
    g = rnd(B, ho, ho, 64)
    dw2 = torch.zeros(64, 256, device=dev)
    N().wgrad(x2, hs, hs, 4, 4, 1, 0, ho, ho, g, None, 0, dw2, 256, 0)
    dw = torch.zeros(64, 147, device=dev)
    N().stem_wgrad_fold(dw2, dw, 64)
    refw = torch.nn.grad.conv2d_weight(xb, (64, 3, 7, 7), g.float().permute(0, 3, 1, 2), stride=2)
    assert rel(dw.view(64, 7, 7, 3), refw.permute(0, 2, 3, 1)) < 5e-3


def test_synth_kernel_matches_cpu_reference():
    """Device synthetic ImageNet == the torch int64 reference (same pixels for the same ids)."""
    import numpy as np
    from pddl.data.datasets import SyntheticImageNet
    ds = SyntheticImageNet(1000, image_size=16, seed=3)
    idx = np.array([0, 5, 999, 123, 77], dtype=np.int64)
    ic, lc = ds.fetch(idx, "cpu")
    ig, lg = ds.fetch(idx, "cuda")
    assert torch.equal(ic, ig.cpu()) and torch.equal(lc, lg.cpu())


@pytest.mark.parametrize("rows,C,pad,off", [(1, 4, 0, 0), (31, 128, 0, 0), (33, 640, 0, 0), (1000, 4096, 0, 0),
                                            (50000, 512, 0, 0), (7, 6, 0, 0), (300, 64, 128, 64), (4097, 1028, 0, 4)])
def test_colsum_reduce_layers(rows, C, pad, off):
    """colsum_reduce (float4 row-lane fold, scalar fallback for unaligned ranges, strided column
    ranges, several layers per launch) against an fp32 torch column sum."""
    import struct
    torch.manual_seed(5)
    ld = pad if pad > 0 else C
    part = torch.randn(off + rows * ld + 3, device=dev)
    out = torch.zeros(2 * C + 5, device=dev)
    tab = torch.frombuffer(bytearray(struct.pack("<q4i", off, rows, C, 0, pad) +
                                     struct.pack("<q4i", off, rows, C, C + 5, pad)), dtype=torch.uint8).to(dev)
    N().colsum_reduce(part, tab, 2, out)
    ref = part[off:off + rows * ld].view(rows, ld)[:, :C].double().sum(0).float()
    assert rel(out[:C], ref) < 1e-5
    assert rel(out[C + 5:], ref) < 1e-5
    assert torch.all(out[C:C + 5] == 0)


@pytest.mark.parametrize("hc,cin,co", [(7, 256, 128), (4, 512, 256), (8, 128, 64)])
def test_dgrad_up2_grid_only_scatter(hc, cin, co):
    """Stride-2 scatter dgrad with up2 = 2 writes only the grid positions (and the compact
    copy): into a pre-zeroed tensor it equals the zero-filling up2 = 1 scatter bitwise, the
    off-grid positions are never touched, and the fused column sums are the same."""
    torch.manual_seed(21)
    n, H = 3, 2 * hc
    g1 = rnd(n, hc, hc, co)
    wt = rnd(cin, co, scale=0.05)
    mask = torch.randint(0, 256, (n, H, H, cin // 8), dtype=torch.uint8, device=dev)
    rows = N().igemm_partial_rows(n * hc * hc, cin, co)
    res = []
    for up2, fill in ((1, 7.0), (2, 7.0)):
        full = torch.full((n, H, H, cin), fill, dtype=torch.bfloat16, device=dev)
        comp = torch.empty(n, hc, hc, cin, dtype=torch.bfloat16, device=dev)
        part = torch.zeros(rows * cin, device=dev)
        N().igemm(g1, None, hc, hc, 1, 1, 1, 0, hc, hc, wt, 1, None, None, None, mask, None, full, 0, comp, 0, 0,
                  up2, H, H, part, None)
        res.append((full, comp, _fold(part, rows, cin)))
    (f1, c1, s1), (f2, c2, s2) = res
    assert torch.equal(c1, c2) and torch.equal(s1, s2)
    assert torch.equal(f1[:, ::2, ::2], f2[:, ::2, ::2]) and torch.equal(f1[:, ::2, ::2], c1)
    off = torch.ones(H, H, dtype=torch.bool, device=dev)
    off[::2, ::2] = False
    assert torch.all(f1[:, off] == 0)          # up2 = 1 zero-fills
    assert torch.all(f2[:, off] == 7.0)        # up2 = 2 leaves them alone


@pytest.mark.parametrize("hc,cin,co", [(7, 256, 128), (4, 512, 256), (8, 128, 64)])
def test_dgrad_up2_compact_mask(hc, cin, co):
    """up2 = 3: the grid-only scatter of up2 = 2 with the ReLU bitmask stored on the compact grid
    (a block input kept only at its stride-2 positions) -- bitwise the up2 = 2 result with the
    full-resolution mask whose grid positions hold the same bits."""
    torch.manual_seed(22)
    n, H = 3, 2 * hc
    g1 = rnd(n, hc, hc, co)
    wt = rnd(cin, co, scale=0.05)
    mask = torch.randint(0, 256, (n, H, H, cin // 8), dtype=torch.uint8, device=dev)
    mc = mask[:, ::2, ::2].contiguous()
    rows = N().igemm_partial_rows(n * hc * hc, cin, co)
    res = []
    for up2, m in ((2, mask), (3, mc)):
        full = torch.zeros((n, H, H, cin), dtype=torch.bfloat16, device=dev)
        comp = torch.empty(n, hc, hc, cin, dtype=torch.bfloat16, device=dev)
        part = torch.zeros(rows * cin, device=dev)
        N().igemm(g1, None, hc, hc, 1, 1, 1, 0, hc, hc, wt, 1, None, None, None, m, None, full, 0, comp, 0, 0,
                  up2, H, H, part, None)
        res.append((full, comp, _fold(part, rows, cin)))
    (f2, c2, s2), (f3, c3, s3) = res
    assert torch.equal(f2, f3) and torch.equal(c2, c3) and torch.equal(s2, s3)


@pytest.mark.parametrize("ho,c,co", [(56, 64, 256), (28, 128, 512), (14, 256, 1024), (7, 512, 2048)])
def test_igemm_forward_stride2_residual(ho, c, co):
    """Forward with up2 != 0: a stride-2 1x1 conv whose residual is the full-resolution tensor read
    at the output rows' grid positions (conv3 of a block feeding a downsampling block, stored
    compact) -- bitwise the full-resolution conv3 + residual + ReLU at the even rows / columns,
    ReLU bits included."""
    torch.manual_seed(23)
    n = 2
    hq = (ho + 1) // 2
    y2 = rnd(n, ho, ho, c)
    w = rnd(co, c, scale=0.05)
    res = rnd(n, ho, ho, co)
    sc, sh = torch.rand(co, device=dev) + 0.5, torch.randn(co, device=dev) * 0.1
    full = torch.empty(n, ho, ho, co, dtype=torch.bfloat16, device=dev)
    bfull = torch.empty(n, ho, ho, co // 8, dtype=torch.uint8, device=dev)
    N().igemm(y2, None, ho, ho, 1, 1, 1, 0, ho, ho, w, 0, sc, sh, res, None, None, full, 1, None, 0, 0, 0, 0, 0,
              None, bfull)
    comp = torch.empty(n, hq, hq, co, dtype=torch.bfloat16, device=dev)
    bcomp = torch.empty(n, hq, hq, co // 8, dtype=torch.uint8, device=dev)
    N().igemm(y2, None, ho, ho, 1, 1, 2, 0, hq, hq, w, 0, sc, sh, res, None, None, comp, 1, None, 0, 0, 1, ho, ho,
              None, bcomp)
    torch.cuda.synchronize()
    ref = full[:, ::2, ::2]
    assert (comp.float() - ref.float()).abs().max().item() <= 1e-2 * ref.float().abs().max().item()
    assert rel(comp, ref) < 1e-3
    # (the ReLU bits agree except where a different tile config's fp32 order flips a value at 0)
    diff = torch.bitwise_xor(bcomp, bfull[:, ::2, ::2].contiguous())
    flipped = sum(((diff >> k) & 1).sum().item() for k in range(8))
    assert flipped <= 1e-4 * comp.numel()


SPLITK_CASES = [
    # kind, N, H, Cin, Cout, R, pad   (stage-5 3x3 at a small batch, a long-K 1x1, odd widths)
    ("fwd", 2, 7, 512, 512, 3, 1),
    ("fwd", 3, 5, 1024, 256, 1, 0),
    ("fwd", 1, 7, 256, 136, 3, 1),
    ("dgrad", 2, 7, 512, 512, 3, 1),
    ("dgrad", 2, 7, 256, 2048, 1, 0),
]


@pytest.mark.parametrize("ks", [0, 3, 8])
@pytest.mark.parametrize("case", SPLITK_CASES)
def test_igemm_splitk_matches_unsplit_and_fp32(case, ks):
    """Split-K (K slices -> fp32 partial tiles in the workspace -> combine kernel running the
    unchanged fused epilogue) against the unsplit kernel and the fp32 reference: forward with
    BN affine + residual + ReLU + bitmask, dgrad with residual-gradient add + ReLU mask + fused
    column sums.  ks 0 = the heuristic (these problems have 1-16 tiles: it splits them).  Three
    launches in a row give identical bits (the combine sums the slices in a fixed order)."""
    torch.manual_seed(31)
    kind, n, h, cin, co, r, pad = case
    M = n * h * h
    nat = N()
    results = []
    for knob in (0, ks if ks else 1):
        nat.set_variant("igemm_splitk", knob)
        try:
            if kind == "fwd":
                K = r * r * cin
                if knob:
                    ws = torch.empty(nat.igemm_splitk_floats(M, co, K), device=dev)
                    nat.splitk_use(ws)
                    assert nat.igemm_plan(M, co, K)[2] > 1
                if not results:
                    x = rnd(n, h, h, cin)
                    w = rnd(co, r, r, cin, scale=0.03)
                    sc, sh = torch.rand(co, device=dev) + 0.5, torch.randn(co, device=dev)
                    res = rnd(n, h, h, co)
                outs = []
                for _ in range(3 if knob else 1):
                    out = torch.empty(n, h, h, co, dtype=torch.bfloat16, device=dev)
                    bits = torch.zeros(n, h, h, (co + 7) // 8, dtype=torch.uint8, device=dev)
                    nat.igemm(x, None, h, h, r, r, 1, pad, h, h, w.view(co, -1), 0, sc, sh, res, None, None, out, 1,
                              None, 0, 0, 0, 0, 0, None, bits)
                    outs.append(out.clone())
                for o in outs[1:]:
                    assert torch.equal(o, outs[0])
                results.append((out.float(), bits.clone(), None))
                ref = (conv_ref(x, w, 1, pad) * sc + sh + res.float()).relu()
            else:
                K = r * r * co
                if knob:
                    ws = torch.empty(nat.igemm_splitk_floats(M, cin, K), device=dev)
                    nat.splitk_use(ws)
                    assert nat.igemm_plan(M, cin, K)[2] > 1
                if not results:
                    g = rnd(n, h, h, co)
                    w = rnd(co, r, r, cin, scale=0.03)
                    a = torch.rand(co, device=dev) + 0.5
                    add, mask = rnd(n, h, h, cin), rnd(n, h, h, cin)
                    wt = dgrad_weights(w, a)
                out = torch.empty(n, h, h, cin, dtype=torch.bfloat16, device=dev)
                rows = nat.igemm_partial_rows(M, cin, K)
                part = torch.full((rows * cin,), float("nan"), device=dev)
                nat.igemm(g, None, h, h, r, r, 1, r - 1 - pad, h, h, wt.view(cin, -1), 1, None, None, None, mask, add,
                          out, 0, None, 0, 0, 0, 0, 0, part, None)
                results.append((out.float(), None, _fold(part, rows, cin)))
                gs = (g.float() * a).permute(0, 3, 1, 2)
                ref = torch.nn.grad.conv2d_input((n, cin, h, h), w.float().permute(0, 3, 1, 2), gs, stride=1,
                                                 padding=pad)
                ref = (ref.permute(0, 2, 3, 1) + add.float()) * (mask.float() > 0)
        finally:
            nat.set_variant("igemm_splitk", 1)
            nat.splitk_use(None)
    (o0, b0, c0), (o1, b1, c1) = results
    assert rel(o1, ref) < 1e-2 and rel(o0, ref) < 1e-2
    assert rel(o1, o0) < 5e-3                       # same math, fp32 partial sums in another order
    if b0 is not None:
        assert (b0 != b1).float().mean().item() < 1e-3   # ReLU bits agree except at exact-zero ties
    if c0 is not None:
        assert rel(c1, c0) < 1e-3


def test_igemm_splitk_dense_head_f32():
    """The fp32 Dense head at a small batch (M = batch rows, 8 tiles of 1000 columns, K = 2048)
    is split by the heuristic; the combine runs the fp32 epilogue."""
    torch.manual_seed(5)
    nat = N()
    a = rnd(32, 2048)
    wd = rnd(1000, 2048, scale=0.02)
    bias = torch.randn(1000, device=dev)
    ones = torch.ones(1000, device=dev)
    assert nat.igemm_plan(32, 1000, 2048)[2] > 1
    ws = torch.empty(nat.igemm_splitk_floats(32, 1000, 2048), device=dev)
    nat.splitk_use(ws)
    out = torch.empty(32, 1000, device=dev)
    try:
        nat.igemm(a.view(32, 1, 1, 2048), None, 1, 1, 1, 1, 1, 0, 1, 1, wd, 2, ones, bias, None, None, None, out, 0,
                  None, 0, 0, 0, 0, 0, None, None)
    finally:
        nat.splitk_use(None)
    ref = a.float() @ wd.float().t() + bias
    assert rel(out, ref) < 1e-3


@pytest.mark.parametrize("nb", [2, 3, 4])
@pytest.mark.parametrize("case", ["fwd_res_k64", "fwd_res_k256_s2", "fwd_nores_k128", "fwd_res_k512",
                                  "dgrad_add_k64", "dgrad_bits_k256", "dgrad_add_k128_nn288"])
def test_igemm_pk_matches(case, nb):
    """The persistent ring kernel (igemm_pk) computes exactly what the per-tile kernel does on
    the short-K 1x1 layers: forward with residual + ReLU-bit output, dgrad with residual-gradient
    add + ReLU bits + fused column sums; several tiles per workgroup (the ring crosses tile
    boundaries), an M tail (rows % 128 != 0), a partial column tile (Nn = 288 = 2 x 128 + 32: a
    width that plans the 128x128 form, which the ring needs; Nn = 320 goes to the 256x64 tile by
    the igemm_n64 rule) and stride 2.  igemm_last_launch() tells which kernel each run took."""
    torch.manual_seed(31)
    n, h = 32, 55                                  # M = 96800 rows: 757 row tiles, ~3-9 tiles per workgroup
    K = int(case.split("_k")[1].split("_")[0])
    Nn = 288 if "nn288" in case else 256
    st = 2 if case.endswith("_s2") else 1
    hi = h * st
    if case.startswith("fwd"):
        x = rnd(n, hi, hi, K)
        w = rnd(Nn, K, scale=0.05)
        sc, sh = torch.rand(Nn, device=dev) + 0.5, torch.randn(Nn, device=dev)
        res = rnd(n, h, h, Nn) if "nores" not in case else None
    else:
        g = rnd(n, h, h, K)
        wt = rnd(Nn, K, scale=0.05)
        addv = rnd(n, h, h, Nn) if "add" in case else None
        bits = pack_bits(rnd(n, h, h, Nn))
    outs = []
    N().set_variant("igemm_pk_all", 1)
    for kv in (0, nb):
        N().set_variant("igemm_pk", kv)
        try:
            if case.startswith("fwd"):
                y = torch.empty(n, h, h, Nn, dtype=torch.bfloat16, device=dev)
                bo = torch.zeros(n, h, h, Nn // 8, dtype=torch.uint8, device=dev)
                N().igemm(x, None, hi, hi, 1, 1, st, 0, h, h, w, 0, sc, sh, res, None, None, y, 1, None, 0, 0, 0, 0, 0,
                          None, bo)
                outs.append(torch.cat([y.float().flatten(), bo.float().flatten()]))
            else:
                out = torch.empty(n, h, h, Nn, dtype=torch.bfloat16, device=dev)
                rows = N().igemm_partial_rows(n * h * h, Nn, K)
                part = torch.full((rows * Nn,), float("nan"), device=dev)
                N().igemm(g, None, h, h, 1, 1, 1, 0, h, h, wt, 1, None, None, None, bits, addv, out, 0, None, 0, 0,
                          0, 0, 0, part, None)
                outs.append(torch.cat([out.float().flatten(), _fold(part, rows, Nn)]))
            torch.cuda.synchronize()
            ran = [(l["kernel"], l["kt"], l["nb"]) for l in N().igemm_last_launch()]
            assert ran == ([("ring", K // 64, nb)] if kv else [("tile128x128", 0, 0)]), ran
        finally:
            N().set_variant("igemm_pk", 2)
    N().set_variant("igemm_pk_all", 0)
    assert rel(outs[1], outs[0]) < 1e-5


@pytest.mark.parametrize("co,ci,M", [(256, 64, 64 * 5 + 13), (256, 64, 64 * 1100 + 29), (512, 128, 64 * 3 + 7),
                                     (512, 128, 64 * 700 + 45)])
def test_bwd1x1_fused(co, ci, M):
    """Fused 1x1 backward (bwd1x1.hip: one read of the output gradient feeds the data gradient
    with its ReLU bits and column sums AND the weight gradient) vs fp32 references:
    out = bits(x) * (g . Wd^T), dw += g^T . x, sum of the partial column-sum rows = out.sum(0).
    Stage-2 shape (256 <- 64) and stage-3 shape (512 <- 128, run as XCD-paired workgroups, one
    per 64-column half); the larger sizes give every workgroup several tiles and a ragged last
    tile, the small ones leave most workgroups without a tile."""
    torch.manual_seed(11)
    g = rnd(M, co)
    x = torch.relu(rnd(M, ci))
    wd = rnd(ci, co, scale=0.05)
    nb = ci // 8
    bits = ((x > 0).view(M, nb, 8).to(torch.int32) << torch.arange(8, device=dev, dtype=torch.int32)).sum(-1)
    bits = bits.to(torch.uint8).contiguous()
    out = torch.full((M, ci), float("nan"), device=dev, dtype=torch.bfloat16)
    rows = N().bwd1x1_partial_rows(M, co, ci)
    colsum = torch.full((rows * ci,), float("nan"), device=dev)
    dw0 = torch.randn(co, ci, device=dev)
    dw = dw0.clone()
    N().bwd1x1(g, x, wd, bits, out, colsum, dw)
    torch.cuda.synchronize()
    ref = (g.float() @ wd.float().t()) * (x > 0)
    assert rel(out, ref) < 1e-2
    assert rel(colsum.view(rows, ci).sum(0), ref.sum(0)) < 1e-3
    assert rel(dw - dw0, g.float().t() @ x.float()) < 1e-3


@pytest.mark.parametrize("M", [64 * 1000 + 37, 3 * 56 * 56, 200])
def test_bwd1x1_pre_form_matches_two_launches(M):
    """bwd1x1 pre form: the next block's conv1 data gradient computed per tile in front of the fused
    conv3 backward -- g = bit(gmask) * (g1 . w1d^T + shortcut gradient), written to gx with its
    column sums -- against the igemm dgrad launch followed by the plain bwd1x1 launch."""
    torch.manual_seed(13)
    g1 = rnd(M, 64)
    w1d = rnd(256, 64, scale=0.05)
    add = rnd(M, 256)
    ox = rnd(M, 256)
    gmask = pack_bits(ox)
    x = torch.relu(rnd(M, 64))
    wd = rnd(64, 256, scale=0.05)
    bits = pack_bits(x)
    rows = N().bwd1x1_partial_rows(M, 256, 64)
    # pre form
    gx = torch.full((M, 256), float("nan"), device=dev, dtype=torch.bfloat16)
    csx = torch.full((rows * 256,), float("nan"), device=dev)
    out = torch.full((M, 64), float("nan"), device=dev, dtype=torch.bfloat16)
    cs = torch.full((rows * 64,), float("nan"), device=dev)
    dw = torch.zeros(256, 64, device=dev)
    N().bwd1x1(add, x, wd, bits, out, cs, dw, g1=g1, w1d=w1d, gmask=gmask, gx=gx, colsum_gx=csx)
    # two launches
    gx_r = torch.empty(M, 256, device=dev, dtype=torch.bfloat16)
    prow = N().igemm_partial_rows(M, 256, 64)
    csx_r = torch.full((prow * 256,), float("nan"), device=dev)
    N().igemm(g1.view(1, 1, M, 64), None, 1, M, 1, 1, 1, 0, 1, M, w1d, 1, None, None, None, gmask.view(1, 1, M, 32),
              add.view(1, 1, M, 256), gx_r.view(1, 1, M, 256), 0, None, 0, 0, 0, 0, 0, csx_r, None)
    out_r = torch.empty(M, 64, device=dev, dtype=torch.bfloat16)
    cs_r = torch.full((rows * 64,), float("nan"), device=dev)
    dw_r = torch.zeros(256, 64, device=dev)
    N().bwd1x1(gx_r, x, wd, bits, out_r, cs_r, dw_r)
    torch.cuda.synchronize()
    ref_gx = (g1.float() @ w1d.float().t() + add.float()) * (ox.float() > 0)
    assert rel(gx, ref_gx) < 1e-2
    assert rel(gx, gx_r) < 2e-3
    assert rel(csx.view(rows, 256).sum(0), ref_gx.sum(0)) < 1e-3
    assert rel(out, out_r) < 5e-3
    assert rel(cs.view(rows, 64).sum(0), cs_r.view(rows, 64).sum(0)) < 5e-3
    assert rel(dw, dw_r) < 5e-3


@pytest.mark.parametrize("co,ci,B,H", [(256, 64, 3, 56), (512, 128, 5, 28), (256, 64, 2, 7)])
def test_bwd1x1_fused_stride2(co, ci, B, H):
    """Stride-2 form of the fused 1x1 backward (a block feeding a downsampling block): the output
    gradient exists only on the stride-2 grid (compact [B, Hc, Wc, co]); x and its ReLU bits are
    full resolution; the data gradient goes to the grid pixels of a pre-zeroed full-resolution
    tensor plus a compact copy, the weight gradient reads x at the grid pixels.  Odd H = 7
    checks the ceil grid (Hc = 4)."""
    torch.manual_seed(12)
    Hc = (H + 1) // 2
    g = rnd(B, Hc, Hc, co)
    x = torch.relu(rnd(B, H, H, ci))
    wd = rnd(ci, co, scale=0.05)
    nb = ci // 8
    bits = ((x > 0).view(B, H, H, nb, 8).to(torch.int32) << torch.arange(8, device=dev, dtype=torch.int32)).sum(-1)
    bits = bits.to(torch.uint8).contiguous()
    out = torch.zeros(B, H, H, ci, device=dev, dtype=torch.bfloat16)
    out2 = torch.full((B, Hc, Hc, ci), float("nan"), device=dev, dtype=torch.bfloat16)
    M = B * Hc * Hc
    rows = N().bwd1x1_partial_rows(M, co, ci)
    colsum = torch.full((rows * ci,), float("nan"), device=dev)
    dw = torch.zeros(co, ci, device=dev)
    N().bwd1x1(g, x, wd, bits, out, colsum, dw, out2)
    torch.cuda.synchronize()
    xs = x[:, ::2, ::2, :]
    refc = (g.float() @ wd.float().t()) * (xs > 0)
    ref = torch.zeros(B, H, H, ci, device=dev)
    ref[:, ::2, ::2, :] = refc
    assert rel(out, ref) < 1e-2 and rel(out2, refc) < 1e-2
    assert rel(colsum.view(rows, ci).sum(0), refc.sum((0, 1, 2))) < 1e-3
    assert rel(dw, g.float().reshape(-1, co).t() @ xs.float().reshape(-1, ci)) < 1e-3


@pytest.mark.parametrize("B,crop,rows", [(2, 224, 0), (3, 244, 0), (2, 160, 1), (2, 96, 3), (1, 224, 56), (2, 244, 7)])
def test_stem_pool_fused_matches_unfused(B, crop, rows):
    """The fused stem (stem.hip: conv1 + BN + ReLU + max-pool, conv1's output only in LDS) equals
    the unfused pair (igemm window GEMM -> bf16 conv1 output -> maxpool_fwd) bit for bit: pool
    output, argmax taps and ReLU bits, for whole-image and row-block workgroups (the block's
    first conv row recomputed) and the ragged 122-wide rows of crop 244."""
    torch.manual_seed(crop + rows)
    hs = (crop + 6) // 2
    h1, h2 = hs - 3, (hs - 3) // 2
    x2 = torch.rand(B, hs, hs, 16, device=dev).to(torch.bfloat16)
    w2 = (torch.randn(64, 256, device=dev) * 0.08).to(torch.bfloat16)
    scale = 0.5 + torch.rand(64, device=dev)
    shift = 0.2 * torch.randn(64, device=dev)
    c1 = torch.empty(B, h1, h1, 64, dtype=torch.bfloat16, device=dev)
    N().igemm(x2, None, hs, hs, 4, 4, 1, 0, h1, h1, w2, 0, scale, shift, None, None, None, c1, 1, None, 0, 0, 0, 0, 0,
              None, None)
    pool_r = torch.empty(B, h2, h2, 64, dtype=torch.bfloat16, device=dev)
    idx_r = torch.empty(B, h2, h2, 64, dtype=torch.uint8, device=dev)
    bits_r = torch.empty(B, h2, h2, 8, dtype=torch.uint8, device=dev)
    N().maxpool_fwd(c1, pool_r, idx_r, bits_r)
    pool = torch.full_like(pool_r, 7.0)
    idx = torch.full_like(idx_r, 99)
    bits = torch.full_like(bits_r, 0x5a)
    N().stem_pool_fwd(x2, w2, scale, shift, pool, idx, bits, rows)
    torch.cuda.synchronize()
    assert (pool.view(torch.int16) != pool_r.view(torch.int16)).sum().item() == 0, (pool.float() - pool_r.float()).abs().max()
    assert torch.equal(idx, idx_r)
    assert torch.equal(bits, bits_r)
    # evaluation form (no bits)
    pool2 = torch.empty_like(pool_r)
    N().stem_pool_fwd(x2, w2, scale, shift, pool2, idx, None, rows)
    assert torch.equal(pool2.view(torch.int16), pool_r.view(torch.int16))


@pytest.mark.parametrize("B,crop,rows", [(2, 224, 0), (3, 244, 0), (2, 160, 1), (2, 96, 5), (1, 224, 56)])
def test_stem_pool_bwd_fused_matches_unfused(B, crop, rows):
    """Fused stem backward (stem.hip: max-pool backward routed into LDS + conv1 weight gradient
    from transposed LDS reads + the stem's column sums) against the unfused pair (maxpool_bwd ->
    bf16 conv1 gradient -> wgrad) and an fp32 reference of the routed gradient's weight gradient."""
    torch.manual_seed(crop + rows + 1)
    hs = (crop + 6) // 2
    h1, h2 = hs - 3, (hs - 3) // 2
    x2 = torch.rand(B, hs, hs, 16, device=dev).to(torch.bfloat16)
    # forward taps from a real pool so the routing is exercised with valid argmax codes
    c1 = torch.relu(torch.randn(B, h1, h1, 64, device=dev)).to(torch.bfloat16)
    pool = torch.empty(B, h2, h2, 64, dtype=torch.bfloat16, device=dev)
    idx = torch.empty(B, h2, h2, 64, dtype=torch.uint8, device=dev)
    N().maxpool_fwd(c1, pool, idx, None)
    gpool = rnd(B, h2, h2, 64)
    gc1 = torch.empty(B, h1, h1, 64, dtype=torch.bfloat16, device=dev)
    prow = N().maxpool_bwd_partial_rows(B, h1, h1, 64)
    cs_r = torch.zeros(prow, 64, device=dev)
    N().maxpool_bwd(gpool, idx, None, gc1, cs_r)
    dw_r = torch.zeros(64, 256, device=dev)
    N().wgrad(x2, hs, hs, 4, 4, 1, 0, h1, h1, gc1, None, 0, dw_r, 256, 0)
    dw = torch.zeros(64, 256, device=dev)
    cs = torch.zeros(N().stem_pool_bwd_partial_rows(B, h2, rows), 64, device=dev)
    N().stem_pool_bwd(x2, gpool, idx, dw, cs, rows)
    torch.cuda.synchronize()
    # fp32 reference: window GEMM of the (bf16) routed gradient
    xw = x2.float().unfold(1, 4, 1).unfold(2, 4, 1)              # [B, h1, h1, 16, 4(R), 4(S)]
    xw = xw.permute(0, 1, 2, 4, 5, 3).reshape(B * h1 * h1, 256)   # k = (R*4 + S)*16 + c
    ref = gc1.float().reshape(-1, 64).t() @ xw
    assert rel(dw, ref) < 1e-5, rel(dw, ref)
    assert rel(dw, dw_r) < 1e-5
    assert torch.allclose(cs.sum(0), cs_r.sum(0), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("n,h,grid", [(24, 56, 0), (6, 56, 4), (50, 13, 3), (3, 17, 0), (4, 61, 0)])
@pytest.mark.parametrize("mode", [0, 1])
def test_conv3x3c64_row_tiles_match_reference(mode, n, h, grid):
    """The 64-channel 3x3 conv kernel (conv3x3c64.hip: 8-wave row tiles, channel halves),
    forward (BN + ReLU + bits) and data gradient (ReLU-bit mask + column sums), against the fp32
    PyTorch conv of the same bf16 operands and against the generic implicit GEMM (same k order).
    `grid` caps the workgroup count so each workgroup streams many tiles (window
    double-buffering, tile tails, a partial last row tile, W = 61 up to the 62-pixel limit)."""
    _c64_case(mode, n, h, grid)


def _c64_case(mode, n, h, grid):
    torch.manual_seed(40 + mode)
    x = rnd(n, h, h, 64)
    w = rnd(64, 576, scale=0.05)
    wr = w.float().view(64, 3, 3, 64).permute(0, 3, 1, 2)
    conv = F.conv2d(x.float().permute(0, 3, 1, 2), wr, padding=1).permute(0, 2, 3, 1)
    out = torch.empty_like(x)
    ref_ig = torch.empty_like(x)
    M = n * h * h
    N().set_variant("c64_grid", grid)
    try:
        if mode == 0:
            sc, sh = torch.rand(64, device=dev) + 0.5, torch.randn(64, device=dev) * 0.1
            bits = torch.zeros(n, h, h, 8, dtype=torch.uint8, device=dev)
            N().conv3x3c64(x, w, 0, out, scale=sc, shift=sh, bits=bits)
            ref = torch.relu(conv * sc + sh)
            bits_ig = torch.zeros_like(bits)
            N().igemm(x, None, h, h, 3, 3, 1, 1, h, h, w, 0, sc, sh, None, None, None, ref_ig, 1, None, 0, 0, 0, 0,
                      0, None, bits_ig)
            assert torch.equal(bits, bits_ig) or (bits != bits_ig).float().mean().item() < 1e-4
        else:
            mask = rnd(n, h, h, 64)
            mbits = pack_bits(mask)
            rows = N().conv3x3c64_partial_rows(M)
            part = torch.full((rows * 64,), float("nan"), device=dev)
            N().conv3x3c64(x, w, 1, out, bits=mbits, colsum=part)
            ref = conv * (mask.float() > 0)
            assert rel(_fold(part, rows, 64), ref.sum((0, 1, 2))) < 1e-3
            N().igemm(x, None, h, h, 3, 3, 1, 1, h, h, w, 1, None, None, None, mbits, None, ref_ig, 0, None, 0, 0,
                      0, 0, 0, None, None)
    finally:
        N().set_variant("c64_grid", 0)
    assert rel(out, ref) < 1e-2
    d = (out.float() - ref_ig.float()).abs().max().item()
    print(f"conv3x3c64 mode {mode}: max |ring - igemm| = {d}")
    assert rel(out, ref_ig) < 2e-3


def test_conv3x3c64_kernels_capture_in_a_hip_graph():
    """The 64-channel 3x3 kernels inside a HIP-graph capture (the Mirrored strategy captures its
    first step): the data gradient with column sums on the full 256-workgroup grid once added a
    zero-byte memset node, which the capture rejects as an invalid argument.  Forward, data
    gradient and weight gradient are captured, replayed, and match eager runs bitwise."""
    torch.manual_seed(44)
    n, h = 24, 56                                  # N * 14 row tiles >= #CUs: the full grid
    x = rnd(n, h, h, 64)
    w = rnd(64, 576, scale=0.05)
    sc, sh = torch.rand(64, device=dev) + 0.5, torch.randn(64, device=dev) * 0.1
    mbits = pack_bits(rnd(n, h, h, 64))
    rows = N().conv3x3c64_partial_rows(n * h * h)
    outs = [dict(y=torch.empty_like(x), bits=torch.zeros(n, h, h, 8, dtype=torch.uint8, device=dev),
                 g=torch.empty_like(x), part=torch.zeros(rows * 64, device=dev),
                 dw=torch.zeros(64, 576, device=dev)) for _ in range(2)]

    def run(o):
        N().conv3x3c64(x, w, 0, o["y"], scale=sc, shift=sh, bits=o["bits"])
        N().conv3x3c64(x, w, 1, o["g"], bits=mbits, colsum=o["part"])
        o["dw"].zero_()
        N().conv3x3c64_wgrad(x, x, o["dw"])

    run(outs[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            run(outs[1])
    g.replay()
    torch.cuda.synchronize()
    for k in ("y", "bits", "g", "part"):
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert rel(outs[1]["dw"], outs[0]["dw"]) < 1e-5   # (fp32 atomics: order may differ)


@pytest.mark.parametrize("n,h,grid", [(24, 56, 0), (5, 56, 3), (7, 13, 2), (3, 61, 0)])
def test_conv3x3c64_wgrad_matches_reference(n, h, grid):
    """Row-tile weight gradient of the 64 -> 64 3x3 conv (conv3x3c64.hip, 8 waves) against the fp32 PyTorch weight gradient of the same bf16
    operands and against the generic wgrad kernel; accumulates into dw (atomics) like the
    engine's zeroed gradient buffer."""
    torch.manual_seed(44)
    x = rnd(n, h, h, 64)
    g = rnd(n, h, h, 64)
    ref = torch.nn.grad.conv2d_weight(x.float().permute(0, 3, 1, 2), (64, 64, 3, 3), g.float().permute(0, 3, 1, 2),
                                      padding=1).permute(0, 2, 3, 1).reshape(64, 576)
    dw = torch.full((64, 576), 0.5, device=dev)
    N().set_variant("c64w_grid", grid)
    try:
        N().conv3x3c64_wgrad(x, g, dw)
    finally:
        N().set_variant("c64w_grid", 0)
    assert rel(dw - 0.5, ref) < 1e-3
    dw2 = torch.zeros(64, 576, device=dev)
    N().wgrad(x, h, h, 3, 3, 1, 1, h, h, g, None, 0, dw2, 576, 0)
    assert rel(dw - 0.5, dw2) < 1e-3


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("m", [4096, 3 * 56 * 56 + 17])
def test_c3c1_boundary_fusion_matches_two_launches(with_res, m):
    """conv3 of a 64-channel block (+ residual) and the next block's conv1 in one launch (c3c1.hip)
    against the two igemm launches: block output, its ReLU bits, the next conv1 output and its
    bits; rows not a multiple of the 64-row tile."""
    torch.manual_seed(50 + with_res)
    a = torch.relu(rnd(m, 64)).to(torch.bfloat16)
    w3 = rnd(256, 64, scale=0.05)
    sc3, sh3 = torch.rand(256, device=dev) + 0.5, torch.randn(256, device=dev) * 0.1
    res = torch.relu(rnd(m, 256)).to(torch.bfloat16) if with_res else None
    w1 = rnd(64, 256, scale=0.05)
    sc1, sh1 = torch.rand(64, device=dev) + 0.5, torch.randn(64, device=dev) * 0.1
    out = torch.empty(m, 256, dtype=torch.bfloat16, device=dev)
    y1 = torch.empty(m, 64, dtype=torch.bfloat16, device=dev)
    b3 = torch.zeros(m, 32, dtype=torch.uint8, device=dev)
    b1 = torch.zeros(m, 8, dtype=torch.uint8, device=dev)
    N().c3c1(a, w3, sc3, sh3, res, out, b3, w1, sc1, sh1, y1, b1)
    # two launches: igemm forward with the 1x1 geometry (M rows as a 1 x M image)
    out_r = torch.empty_like(out)
    y1_r = torch.empty_like(y1)
    b3_r, b1_r = torch.zeros_like(b3), torch.zeros_like(b1)
    av = a.view(1, 1, m, 64)
    N().igemm(av, None, 1, m, 1, 1, 1, 0, 1, m, w3, 0, sc3, sh3,
              res.view(1, 1, m, 256) if res is not None else None, None, None, out_r.view(1, 1, m, 256), 1, None, 0,
              0, 0, 0, 0, None, b3_r.view(1, 1, m, 32))
    N().igemm(out_r.view(1, 1, m, 256), None, 1, m, 1, 1, 1, 0, 1, m, w1, 0, sc1, sh1, None, None, None,
              y1_r.view(1, 1, m, 64), 1, None, 0, 0, 0, 0, 0, None, b1_r.view(1, 1, m, 8))
    torch.cuda.synchronize()
    ref = torch.relu(a.float() @ w3.float().t() * sc3 + sh3 + (res.float() if with_res else 0.0))
    assert rel(out, ref) < 1e-2
    assert rel(out, out_r) < 2e-3
    assert (b3 != b3_r).float().mean().item() < 1e-3
    assert rel(y1, y1_r) < 5e-3
    assert (b1 != b1_r).float().mean().item() < 1e-3


def test_wgrad_finalize_matches_reference():
    """wgrad_finalize (one wave per row, 16-byte vectors where rows are aligned, scalar rows
    otherwise) against fp32 PyTorch: dW[co] *= a[co] and dgamma_raw[co] = <W[co], dW_raw[co]>,
    over a table mixing an unaligned stem-like layer (k = 147), a short row (k = 64), a long
    3x3 row (k = 4608), a layer without scale (ch_off -1) and one without dgamma (dg_off -1)."""
    import struct
    torch.manual_seed(9)
    nat = N()
    layers = [(256, 64, 64, 64), (40, 4608, 320, 320), (96, 576, -1, 360), (72, 100, 456, -1), (64, 147, 0, 0)]
    off, rows = 4, []                    # (aligned rows first; the k = 147 rows end unaligned)
    for cout, k, ch, dg in layers:
        rows.append((off, cout, k, ch, dg))
        off += cout * k
    params = torch.randn(off, device=dev)
    grads = torch.randn(off, device=dev)
    scale = torch.rand(600, device=dev) + 0.5
    dgr = torch.full((600,), float("nan"), device=dev)
    table = torch.tensor(list(b"".join(struct.pack("<5i", *r) for r in rows)), dtype=torch.uint8, device=dev)
    g0 = grads.clone()
    nat.wgrad_finalize(params, grads, table, len(rows), scale, dgr, max(c for c, *_ in layers))
    torch.cuda.synchronize()
    for o, cout, k, ch, dg in rows:
        w = params[o:o + cout * k].view(cout, k)
        d = g0[o:o + cout * k].view(cout, k)
        a = scale[ch:ch + cout, None] if ch >= 0 else 1.0
        assert rel(grads[o:o + cout * k].view(cout, k), d * a) < 1e-6
        if dg >= 0:
            assert rel(dgr[dg:dg + cout], (w * d).sum(1)) < 1e-5
    assert torch.equal(grads[:4], g0[:4])                 # nothing outside the table is touched
    assert torch.isnan(dgr[456:528]).all()                # (dg_off -1: no dgamma written)
