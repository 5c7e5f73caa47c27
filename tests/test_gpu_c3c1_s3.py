"""The 128-channel (stage-3) form of the boundary kernel (csrc/kernels/c3c1.hip: conv3 128 -> 512
+ residual + ReLU and the next block's conv1 512 -> 128 + ReLU in one persistent launch) against
plain fp64 references, with the inputs, the two kinds and the bounds of test_gpu_fused_kernels.py:

  exact  small sparse integers, bf16 outputs bit-identical to the rounded fp64 reference; the
         shifts are integers in -3..3 and the residual in 0..3, so a large share of the
         pre-activations is exactly zero or one step to either side of it
  real   randn inputs with a signed residual, so the pre-activations straddle zero; every element
         within 2^-8 |ref| + (K + 4) U (|a| (*) |b|) |scale|

M brackets the 32-row tile (and 64); the capped runs (c3c1_grid 1 and 3) make one workgroup walk
two to six tiles through both LDS stages, ending on either; the production-grid run gives every
workgroup (one per CU) two tiles and the first two a third, the last tile 5 rows.  The kernel is also
held to the two igemm launches it replaces, to rows after M left alone, and to the engine with
PDDL_ENGINE c3c1=1 (stage 2 only).
"""
import functools
from types import SimpleNamespace as NS

import pytest
import torch

from kernel_checks import (BF, ByteOut, Out, bn, check, check_bits, dev, gen, ints, is_sent, precond, randn, sent, tern,
                           untouched)
from pddl.utils.envopts import with_opt

pytestmark = pytest.mark.gpu

KINDS = ["exact", "real"]
F_, C_ = 128, 512
TILE = 32                # rows per tile (c3c1.hip C3_MT)


def N():
    from pddl.ops.native import require_native
    return require_native()


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


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def case(M, kind):
    """c3c1_case of test_gpu_fused_kernels.py at F = 128 (real: the residual keeps its sign)."""
    exact = kind == "exact"
    g = gen(7000 + 2 * M + exact)
    sc3, sh3 = bn(g, C_, exact)
    sc1, sh1 = bn(g, F_, exact)
    if exact:
        a, w3, w1 = tern(g, M, F_), ints(g, -2, 2, C_, F_), ints(g, -2, 2, F_, C_)
        w3 = (w3.float() * torch.where(sc3 == 0.5, 2.0, 1.0).view(C_, 1)).to(BF)    # the block output stays an integer
        res = ints(g, 0, 3, M, C_)
    else:
        a, w3, w1 = torch.relu(randn(g, M, F_)), randn(g, C_, F_, scale=0.05), randn(g, F_, C_, scale=0.05)
        res = randn(g, M, C_, scale=0.3)
    acc, mag = a.double() @ w3.double().t(), a.double().abs() @ w3.double().abs().t()
    c = NS(a=a, w3=w3, sc3=sc3, sh3=sh3, w1=w1, sc1=sc1, sh1=sh1, res=res)
    pre, c.mag = acc * sc3.double() + sh3.double(), mag * sc3.double().abs() + sh3.double().abs()
    c.out = {False: torch.relu(pre), True: torch.relu(pre + res.double())}
    c.out_mag = {False: c.mag, True: c.mag + res.double().abs()}
    # the ReLU is exercised on both sides: a fair share of the block output is cut and a fair share kept
    for r in (False, True):
        cut = float((c.out[r] == 0).double().mean())
        assert M < 32 or 0.1 < cut < 0.9, f"test bug: {cut:.2f} of the pre-activations below zero"
    if exact:
        precond("c3c1_s3", mag, torch.cat([c.out[False], c.out[True]]))
    return c


def run_and_check(M, with_res, with_bits, kind, what):
    nat, c = N(), case(M, kind)
    out, y1, b3, b1 = Out(M * C_, BF), Out(M * F_, BF), ByteOut(M * C_ // 8), ByteOut(M * F_ // 8)
    nat.c3c1(c.a, c.w3, c.sc3, c.sh3, c.res if with_res else None, out.t.view(M, C_), b3.t if with_bits else None,
             c.w1, c.sc1, c.sh1, y1.t.view(M, F_), b1.t if with_bits else None)
    out.check(what + " out")
    y1.check(what + " y1")
    check(kind, out.t, c.out[with_res], c.out_mag[with_res], F_, what + " out")
    # phase 2 reads the rounded block output: its reference starts from the kernel's own `out`
    o = out.t.view(M, C_).double()
    mag1 = o.abs() @ c.w1.double().abs().t()
    if kind == "exact":
        precond("c3c1_s3 y1", mag1)
    check(kind, y1.t, torch.relu(o @ c.w1.double().t() * c.sc1.double() + c.sh1.double()),
          mag1 * c.sc1.double().abs() + c.sh1.double().abs(), C_, what + " y1")
    if with_bits:
        check_bits(b3, out, what + " bits3")
        check_bits(b1, y1, what + " bits1")
    else:
        untouched(b3, what + " bits3")
        untouched(b1, what + " bits1")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_bits", [True, False])
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("M", [1, 31, 32, 33, 63, 64, 65, 129])
def test_c3c1_s3(M, with_res, with_bits, kind):
    run_and_check(M, with_res, with_bits, kind, f"c3c1_s3 M={M} res={with_res} bits={with_bits} {kind}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("cap,M", [(1, 5 * TILE + 7), (1, 2 * TILE), (3, 8 * TILE + 1), (3, 6 * TILE)])
def test_c3c1_s3_capped_grid(knob, cap, M, with_res, kind):
    """One and three workgroups: 6 / 2 tiles in one, 3 + 3 + 3 (the last 1 row) / 2 + 2 + 2."""
    knob("c3c1_grid", cap)
    run_and_check(M, with_res, True, kind, f"c3c1_s3 grid={cap} M={M} res={with_res} {kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_c3c1_s3_real_grid(kind):
    """The production grid (one workgroup per CU): 2 grid + 2 tiles, so every workgroup takes two,
    the first two a third, and the last tile has 5 rows."""
    grid = cus()
    M = (2 * grid + 1) * TILE + 5
    tiles = -(-M // TILE)
    assert grid == min(tiles, cus()) and tiles == 2 * grid + 2 and M % TILE == 5
    run_and_check(M, True, True, kind, f"c3c1_s3 real grid {grid} M={M} {kind}")


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, device=dev) * scale).to(torch.bfloat16)


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("m", [4096, 3 * 28 * 28 + 17])
def test_c3c1_s3_matches_two_launches(with_res, m):
    """The fused launch against the two igemm launches it replaces (the bounds of
    test_gpu_kernels.py::test_c3c1_boundary_fusion_matches_two_launches)."""
    nat = N()
    torch.manual_seed(60 + with_res)
    a = torch.relu(rnd(m, F_)).to(torch.bfloat16)
    w3 = rnd(C_, F_, scale=0.05)
    sc3, sh3 = torch.rand(C_, device=dev) + 0.5, torch.randn(C_, device=dev) * 0.1
    res = torch.relu(rnd(m, C_)).to(torch.bfloat16) if with_res else None
    w1 = rnd(F_, C_, scale=0.05)
    sc1, sh1 = torch.rand(F_, device=dev) + 0.5, torch.randn(F_, device=dev) * 0.1
    out = torch.empty(m, C_, dtype=torch.bfloat16, device=dev)
    y1 = torch.empty(m, F_, dtype=torch.bfloat16, device=dev)
    b3 = torch.zeros(m, C_ // 8, dtype=torch.uint8, device=dev)
    b1 = torch.zeros(m, F_ // 8, dtype=torch.uint8, device=dev)
    nat.c3c1(a, w3, sc3, sh3, res, out, b3, w1, sc1, sh1, y1, b1)
    out_r, y1_r = torch.empty_like(out), torch.empty_like(y1)
    b3_r, b1_r = torch.zeros_like(b3), torch.zeros_like(b1)
    nat.set_variant("igemm_splitk", 0)     # (one k order, as in test_gpu_kernels.py)
    try:
        nat.igemm(a.view(1, 1, m, F_), None, 1, m, 1, 1, 1, 0, 1, m, w3, 0, sc3, sh3,
                  res.view(1, 1, m, C_) if res is not None else None, None, None, out_r.view(1, 1, m, C_), 1, None, 0,
                  0, 0, 0, 0, None, b3_r.view(1, 1, m, C_ // 8))
        nat.igemm(out_r.view(1, 1, m, C_), None, 1, m, 1, 1, 1, 0, 1, m, w1, 0, sc1, sh1, None, None, None,
                  y1_r.view(1, 1, m, F_), 1, None, 0, 0, 0, 0, 0, None, b1_r.view(1, 1, m, F_ // 8))
        torch.cuda.synchronize()
    finally:
        nat.set_variant("igemm_splitk", 1)
    ref = torch.relu(a.float() @ w3.float().t() * sc3 + sh3 + (res.float() if with_res else 0.0))
    fig = (rel(out, ref), rel(out, out_r), (b3 != b3_r).float().mean().item(), rel(y1, y1_r),
           (b1 != b1_r).float().mean().item())
    print("c3c1_s3 vs two launches m=%d res=%s: out/ref %.2e out %.2e bits3 %.2e y1 %.2e bits1 %.2e" % ((m, with_res) + fig))
    assert fig[0] < 1e-2
    assert fig[1] < 2e-3
    assert fig[2] < 1e-3
    assert fig[3] < 5e-3
    assert fig[4] < 1e-3


@pytest.mark.parametrize("M", [70, 3 * TILE])
def test_c3c1_s3_fence(M):
    """Rows after M are not the kernel's: `out`, `y1` and both bits planes are the first M rows of
    buffers with 8 more rows of sentinel, which stay as they were (M = 70: inside the last tile)."""
    nat, c = N(), case(M, "real")
    G = 8
    out, y1 = sent((M + G) * C_, BF), sent((M + G) * F_, BF)
    b3 = torch.full(((M + G) * C_ // 8,), 0xA5, dtype=torch.uint8, device=dev)
    b1 = torch.full(((M + G) * F_ // 8,), 0xA5, dtype=torch.uint8, device=dev)
    nat.c3c1(c.a, c.w3, c.sc3, c.sh3, c.res, out[:M * C_].view(M, C_), b3[:M * C_ // 8], c.w1, c.sc1, c.sh1,
             y1[:M * F_].view(M, F_), b1[:M * F_ // 8])
    torch.cuda.synchronize()
    assert not bool(is_sent(out[:M * C_]).any()) and not bool(is_sent(y1[:M * F_]).any())
    assert bool(is_sent(out[M * C_:]).all()), "out: rows after M written"
    assert bool(is_sent(y1[M * F_:]).all()), "y1: rows after M written"
    assert bool((b3[M * C_ // 8:] == 0xA5).all()) and bool((b1[M * F_ // 8:] == 0xA5).all()), "bits: rows after M written"


def test_c3c1_s3_rejects_other_widths():
    nat = N()
    a = torch.zeros(4, 256, dtype=BF, device=dev)
    w3, w1 = torch.zeros(1024, 256, dtype=BF, device=dev), torch.zeros(256, 1024, dtype=BF, device=dev)
    s = torch.zeros(1024, device=dev)
    with pytest.raises(RuntimeError, match="c3c1"):
        nat.c3c1(a, w3, s, s, None, torch.zeros(4, 1024, dtype=BF, device=dev), None, w1, s, s,
                 torch.zeros(4, 256, dtype=BF, device=dev), None)
    c = case(33, "exact")                     # F = 128 operands with stage-2 weights
    with pytest.raises(RuntimeError, match="w3"):
        nat.c3c1(c.a, torch.zeros(256, 64, dtype=BF, device=dev), c.sc3, c.sh3, None,
                 torch.zeros(33, C_, dtype=BF, device=dev), None, c.w1, c.sc1, c.sh1,
                 torch.zeros(33, F_, dtype=BF, device=dev), None)


def test_c3c1_s3_in_engine(monkeypatch):
    """The engine at B = 8, 224 with the stage-3 boundaries fused (PDDL_ENGINE c3c1=2, the default)
    against stage 2 only (c3c1=1): same loss, flat gradients to fp32 order (the bounds of
    test_gpu_engine.py::test_c3c1_boundary_fusion_in_engine)."""
    from pddl.models.engine import HipEngine
    from pddl.models.resnet50 import ParamLayout
    L = ParamLayout()
    B = 8
    got = []
    for on in ("2", "1"):
        monkeypatch.setenv("PDDL_ENGINE", with_opt("PDDL_ENGINE", "c3c1", on))
        he = HipEngine(L, B, crop=224, image_size=224)
        assert he.c3c1 == int(on)
        nfused = sum(he._c3c1_ok(b, nb) for b, nb in zip(L.blocks, L.blocks[1:]))
        assert nfused == (3 if on == "2" else 1)
        he.init(seed=7)
        img = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
        lab = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(2)).cuda()
        st = he.forward_backward(img, lab, 1.0 / B)
        torch.cuda.synchronize()
        got.append((st[0].item() / B, he.grads.clone()))
    (l2, g2), (l1, g1) = got
    print(f"c3c1=2 vs 1: loss rel {abs(l2 - l1) / abs(l1):.2e}, grad rel {((g2 - g1).norm() / g1.norm()).item():.3e}")
    assert abs(l2 - l1) < 1e-4 * abs(l1)
    assert ((g2 - g1).norm() / g1.norm()).item() < 3e-2
