"""The 64-channel (stage-2) boundary kernels (csrc/kernels/c3c1.hip) against the launches they replace,
on the same operands, bit for bit: `out`, `y1` and both ReLU bit planes.

  plain  (c3c1_kernel, one tile per workgroup: the c3c1_grid cap does not apply) conv3 64 -> 256
         (+ residual) + ReLU, then the next conv1 256 -> 64 + ReLU: against the igemm conv3 with the
         residual and the igemm conv1 reading its output
  dual   (c3c1_s2_kernel: persistent grid, two LDS stages) conv2_block1's conv3 + shortcut as one
         K = 64 + 64 GEMM (second source: the block input, the engine's "fuse:" weight [256][128],
         no residual): against the dual-source igemm and the igemm conv1

Two fills.  `ints`: small integers everywhere (scales 1 or 0.5, integer shifts), so every fp32 sum is
exact whatever its order, about a tenth of the pre-activations are exactly 0 and close to half are
negative: the bit planes carry both values and a difference can only be a wrong element.  `real`:
randn operands, where bit identity also needs the kernel's k order and epilogue arithmetic to be
the igemm's.

Rows (MT = 64, the tile height): 40 (one partial tile); MT; 7 MT + 17 with c3c1_grid = 3 (three
workgroups walk 3 + 3 + 2 tiles through both LDS stages, the last tile 17 rows); 2 MT with
c3c1_grid = 0 (fewer tiles than workgroups); MT * CUs + 1 at the production grid (the first
workgroup takes a second tile of one row).  Rows after M stay untouched; the binding rejects a
residual or another width together with `a2`; and the engine at B = 8, 224 with c3c1_proj=1 against
c3c1_proj=0 stores the same forward activations bit for bit.
"""
import functools
from types import SimpleNamespace as NS

import pytest
import torch

from pddl.utils.envopts import with_opt

pytestmark = pytest.mark.gpu

dev = "cuda"
BF = torch.bfloat16
MT = 64                  # rows per tile (c3c1.hip C2_MT)
KINDS = ["ints", "real"]


def N():
    from pddl.ops.native import require_native
    return require_native()


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# (rows, c3c1_grid or None: leave the knob alone)
ROWS = [(40, None), (MT, None), (7 * MT + 17, 3), (2 * MT, 0)]


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(BF).to(dev)


def _randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(dev)


@functools.lru_cache(maxsize=None)
def case(M, kind):
    """Operands of both forms (the plain form uses w3 = wf[:, :64] made contiguous) and the outputs of
    the launches they replace, computed once per (M, kind) and left unchanged."""
    nat = N()
    g = torch.Generator().manual_seed(9100 + 2 * M + (kind == "ints"))
    if kind == "ints":
        a, x2 = _ints(g, -1, 2, M, 64), _ints(g, -1, 2, M, 64)
        wf, w1 = _ints(g, -1, 1, 256, 128), _ints(g, -1, 1, 64, 256)
        res = _ints(g, -3, 3, M, 256)
        sc3 = torch.where(torch.rand(256, generator=g) < 0.5, 0.5, 1.0).to(dev)
        sh3 = torch.randint(-3, 4, (256,), generator=g).float().to(dev)
        sc1 = torch.where(torch.rand(64, generator=g) < 0.5, 0.5, 1.0).to(dev)
        sh1 = torch.randint(-3, 4, (64,), generator=g).float().to(dev)
    else:
        a, x2 = torch.relu(_randn(g, M, 64)), torch.relu(_randn(g, M, 64))
        wf, w1 = _randn(g, 256, 128, scale=0.05), _randn(g, 64, 256, scale=0.05)
        res = _randn(g, M, 256, scale=0.3)
        sc3, sh3 = (torch.rand(256, generator=g) + 0.5).to(dev), (torch.randn(256, generator=g) * 0.1).to(dev)
        sc1, sh1 = (torch.rand(64, generator=g) + 0.5).to(dev), (torch.randn(64, generator=g) * 0.1).to(dev)
    c = NS(a=a, x2=x2, wf=wf, w3=wf[:, :64].contiguous(), w1=w1, res=res, sc3=sc3, sh3=sh3, sc1=sc1, sh1=sh1, ref={})
    v = lambda t, ch: t.view(1, 1, M, ch)
    nat.set_variant("igemm_splitk", 0)     # (one k order, as in test_gpu_kernels.py)
    try:
        for form in ("plain", "res", "dual"):
            out, y1 = torch.empty(M, 256, dtype=BF, device=dev), torch.empty(M, 64, dtype=BF, device=dev)
            b3, b1 = torch.zeros(M, 32, dtype=torch.uint8, device=dev), torch.zeros(M, 8, dtype=torch.uint8, device=dev)
            nat.igemm(v(a, 64), v(x2, 64) if form == "dual" else None, 1, M, 1, 1, 1, 0, 1, M,
                      wf if form == "dual" else c.w3, 0, sc3, sh3, v(res, 256) if form == "res" else None, None, None,
                      v(out, 256), 1, None, 0, 0, 0, 0, 0, None, v(b3, 32))
            nat.igemm(v(out, 256), None, 1, M, 1, 1, 1, 0, 1, M, w1, 0, sc1, sh1, None, None, None, v(y1, 64), 1,
                      None, 0, 0, 0, 0, 0, None, v(b1, 8))
            c.ref[form] = (out, y1, b3, b1)
        torch.cuda.synchronize()
    finally:
        nat.set_variant("igemm_splitk", 1)
    # the fill does what the docstring says (the pre-activation: conv3's, before the ReLU)
    pre = (a.double() @ c.w3.double().t()) * sc3.double() + sh3.double() + res.double()
    if kind == "ints" and M >= MT:
        assert (pre == 0).double().mean().item() > 0.02 and (pre < 0).double().mean().item() > 0.2, "test bug: fill"
    for form in c.ref:
        cut = (c.ref[form][0] == 0).double().mean().item()
        assert M < MT or 0.1 < cut < 0.9, f"test bug: {form} {cut:.2f} of the block output cut"
    return c


def run(M, form, with_bits, kind, cap, what, guard=0):
    """One launch of the kernel under test into fresh buffers (with `guard` sentinel rows after M),
    compared bit for bit with the reference launches."""
    nat, c = N(), case(M, kind)
    SENT = 0x5A
    out = torch.full(((M + guard) * 256,), -7.0, dtype=BF, device=dev)
    y1 = torch.full(((M + guard) * 64,), -7.0, dtype=BF, device=dev)
    b3 = torch.full(((M + guard) * 32,), SENT, dtype=torch.uint8, device=dev)
    b1 = torch.full(((M + guard) * 8,), SENT, dtype=torch.uint8, device=dev)
    if cap is not None:
        nat.set_variant("c3c1_grid", cap)
    try:
        nat.c3c1(c.a, c.wf if form == "dual" else c.w3, c.sc3, c.sh3, c.res if form == "res" else None,
                 out[:M * 256].view(M, 256), b3[:M * 32] if with_bits else None, c.w1, c.sc1, c.sh1,
                 y1[:M * 64].view(M, 64), b1[:M * 8] if with_bits else None, c.x2 if form == "dual" else None)
        torch.cuda.synchronize()
    finally:
        if cap is not None:
            nat.set_variant("c3c1_grid", 0)
    out_r, y1_r, b3_r, b1_r = c.ref[form]
    i16 = lambda t: t.contiguous().view(torch.int16)
    d_out = (i16(out[:M * 256].view(M, 256)) != i16(out_r)).sum().item()
    d_y1 = (i16(y1[:M * 64].view(M, 64)) != i16(y1_r)).sum().item()
    print(f"{what}: out {d_out} of {M * 256} elements differ, y1 {d_y1} of {M * 64}")
    assert d_out == 0, f"{what}: out differs from the igemm launch in {d_out} elements"
    assert d_y1 == 0, f"{what}: y1 differs from the igemm launches in {d_y1} elements"
    if with_bits:
        assert torch.equal(b3[:M * 32].view(M, 32), b3_r), f"{what}: bits3"
        assert torch.equal(b1[:M * 8].view(M, 8), b1_r), f"{what}: bits1"
        if kind == "ints":
            assert 0 < (b3_r == 0).sum().item() and (b3_r != 0).any(), "test bug: one-valued bit plane"
    else:
        assert bool((b3 == SENT).all()) and bool((b1 == SENT).all()), f"{what}: bits written without a bits operand"
    if guard:
        assert bool((out[M * 256:] == -7.0).all()) and bool((y1[M * 64:] == -7.0).all()), f"{what}: rows after M written"
        assert bool((b3[M * 32:] == SENT).all()) and bool((b1[M * 8:] == SENT).all()), f"{what}: bits after M written"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_bits", [True, False])
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("M,cap", ROWS)
def test_plain_matches_igemm_launches(M, cap, with_res, with_bits, kind):
    run(M, "res" if with_res else "plain", with_bits, kind, cap, f"c3c1_s2 plain M={M} grid={cap} res={with_res} {kind}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_bits", [True, False])
@pytest.mark.parametrize("M,cap", ROWS)
def test_dual_matches_igemm_launches(M, cap, with_bits, kind):
    run(M, "dual", with_bits, kind, cap, f"c3c1_s2 dual M={M} grid={cap} {kind}")


@pytest.mark.parametrize("form", ["res", "dual"])
def test_production_grid(form):
    """One workgroup per CU, one tile each, and a last tile of one row for the first workgroup."""
    M = MT * cus() + 1
    run(M, form, True, "real", None, f"c3c1_s2 {form} production grid M={M}")


@pytest.mark.parametrize("form", ["res", "dual"])
@pytest.mark.parametrize("M", [70, 3 * MT])
def test_rows_after_m_untouched(M, form):
    run(M, form, True, "ints", None, f"c3c1_s2 {form} fence M={M}", guard=8)


def test_binding_rejects_misuse_of_a2():
    nat, c = N(), case(40, "ints")
    M = 40
    out, y1 = torch.zeros(M, 256, dtype=BF, device=dev), torch.zeros(M, 64, dtype=BF, device=dev)
    with pytest.raises(RuntimeError, match="c3c1"):      # a residual with the dual form
        nat.c3c1(c.a, c.wf, c.sc3, c.sh3, c.res, out, None, c.w1, c.sc1, c.sh1, y1, None, c.x2)
    with pytest.raises(RuntimeError, match="c3c1"):      # the plain weight with a2
        nat.c3c1(c.a, c.w3, c.sc3, c.sh3, None, out, None, c.w1, c.sc1, c.sh1, y1, None, c.x2)
    with pytest.raises(RuntimeError, match="c3c1"):      # the fused weight without a2
        nat.c3c1(c.a, c.wf, c.sc3, c.sh3, None, out, None, c.w1, c.sc1, c.sh1, y1, None)
    with pytest.raises(RuntimeError, match="c3c1"):      # a2 of another size
        nat.c3c1(c.a, c.wf, c.sc3, c.sh3, None, out, None, c.w1, c.sc1, c.sh1, y1, None, c.x2[:M - 1])
    a128 = torch.zeros(M, 128, dtype=BF, device=dev)
    s = torch.zeros(512, device=dev)
    with pytest.raises(RuntimeError, match="c3c1"):      # the 128-channel form has no dual source
        nat.c3c1(a128, torch.zeros(512, 192, dtype=BF, device=dev), s, s, None, torch.zeros(M, 512, dtype=BF, device=dev),
                 None, torch.zeros(128, 512, dtype=BF, device=dev), s, s, torch.zeros(M, 128, dtype=BF, device=dev), None, c.x2)


def _step(monkeypatch, on, B=8):
    from pddl.models.engine import HipEngine
    from pddl.models.resnet50 import ParamLayout
    monkeypatch.setenv("PDDL_ENGINE", with_opt("PDDL_ENGINE", "c3c1_proj", on))
    he = HipEngine(ParamLayout(), B, crop=224, image_size=224)
    assert he.c3c1_proj == (on == "1") and he.c3c1_proj_min_m <= B * 56 * 56
    b1, b2 = he.L.blocks[0], he.L.blocks[1]
    assert he._c3c1_ok(b1, b2, B * 56 * 56) == (on == "1")
    he.init(seed=7)
    img = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    lab = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(2)).cuda()
    st = he.forward_backward(img, lab, 1.0 / B)
    torch.cuda.synchronize()
    return he, st[0].item() / B, he.grads.clone()


def test_projection_boundary_in_engine(monkeypatch):
    """B = 8 at 224 (25,088 stage-2 rows, above the default gate): c3c1_proj=1 against c3c1_proj=0, same
    seed.  The logits and every activation and bit plane the forward stores are bit-identical (the
    loss to the order of its B-term atomic sum, which the off path does not reproduce either); the
    gradients differ by no more than the order of the weight-gradient atomics allows, measured here
    as c3c1_proj=0 against itself.  Both differences are norms of two independent draws of that one
    noise over 25 M elements, which concentrate far tighter than a factor of 2: the bound is twice the
    measured spread, and exactly 0 when the backward reproduces itself."""
    h0, l0, g0 = _step(monkeypatch, "0")
    h0b, l0b, g0b = _step(monkeypatch, "0")
    h1, l1, g1 = _step(monkeypatch, "1")
    # the loss: its input (the logits, below) is bit-identical; the loss head sums the B per-image
    # terms with fp32 atomics, so c3c1_proj=0 against itself already differs in the last bit
    # (6.898004531860352 against 6.898004055023193 measured).  Two orders of a sum of B positive
    # fp32 terms differ by at most 2 (B - 1) 2^-24 of the sum.
    print(f"loss: on {l1!r} off {l0!r} off again {l0b!r}")
    assert abs(l1 - l0) <= 2 * (8 - 1) * 2.0 ** -24 * abs(l0), f"loss {l1!r} against {l0!r}"
    for name in h0.acts:
        for k, t in h0.acts[name].items():
            assert torch.equal(t.view(torch.int16), h1.acts[name][k].view(torch.int16)), f"{name} {k}"
        for k, t in h0.bits[name].items():
            assert torch.equal(t, h1.bits[name][k]), f"{name} bits {k}"
    assert torch.equal(h0.logits, h1.logits)
    spread = ((g0b - g0).norm() / g0.norm()).item()
    diff = ((g1 - g0).norm() / g0.norm()).item()
    print(f"c3c1_proj 1 vs 0: grad rel {diff:.3e}; 0 vs 0: {spread:.3e}")
    assert diff <= 2 * spread
