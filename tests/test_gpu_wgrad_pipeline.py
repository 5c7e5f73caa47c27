"""The software-pipelined fragment reads of the 8-phase weight-gradient kernel (wgrad8_kernel).

Each phase of the kernel issues the NEXT phase's transposed LDS reads under its own MFMAs, so
the first phase of a split (fragments read by the prologue), the last one (nothing left to
prefetch) and the hand-over between two m-tiles are the places where a wrong register set, a
missed wait or a half restaged too early would show.  The shapes are the smallest that reach
each of them.  Reference: torch.nn.grad.conv2d_weight in fp32 on the same bf16-rounded inputs.

Routing: these grids are below the launcher's fill threshold, so the kernel is forced with the
knob's +16 bit, and `wgrad_last_tiling()` is asserted to report the kernel that ran (1256 / 1128 for
the 8-phase kernel's 256- and 128-wide co tiles, 128 for the knob-0 comparison run).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

dev = "cuda"


def N():
    from pddl.ops.native import require_native
    return require_native()


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def rnd(*shape):
    return torch.randn(*shape, device=dev).to(torch.bfloat16)


_inputs = {}


def problem(case):
    """Inputs and the fp32 reference of one geometry, computed once and shared (read-only)."""
    if case not in _inputs:
        torch.manual_seed(53)
        n, h, cin, co, r, st, pad = case
        ho = (h + 2 * pad - r) // st + 1
        x = rnd(n, h, h, cin)
        g = rnd(n, ho, ho, co)
        ref = torch.nn.grad.conv2d_weight(x.float().permute(0, 3, 1, 2), (co, cin, r, r),
                                          g.float().permute(0, 3, 1, 2), stride=st, padding=pad)
        _inputs[case] = (x, g, ref.permute(0, 2, 3, 1).reshape(co, -1).contiguous(), ho)
    return _inputs[case]


def run(case, knob):
    n, h, cin, co, r, st, pad = case
    x, g, _, ho = problem(case)
    nat = N()
    nat.set_variant("wgrad8", knob)
    dw = torch.zeros(co, r * r * cin, device=dev)
    nat.wgrad(x, h, h, r, r, st, pad, ho, ho, g, None, 0, dw, r * r * cin, 0)
    return dw, nat.wgrad_last_tiling()


def check(case, stagger):
    ref = problem(case)[2]
    nat = N()
    try:
        base, tiling = run(case, 0)
        assert tiling == 128
        outs = []
        for _ in range(3):
            dw, tiling = run(case, 16 + stagger)
            assert tiling == (1128 if case[3] <= 128 else 1256)
            outs.append(dw)
    finally:
        nat.set_variant("wgrad8", 2)   # (the default)
    e_ref = [rel(o, ref) for o in outs]
    e_base = [rel(o, base) for o in outs]
    e_rep = rel(outs[2], outs[1])
    print(f"{case} stagger={stagger}: vs fp32 {e_ref}, vs 128-wide {e_base}, repeat {e_rep}")
    assert rel(base, ref) < 5e-3
    assert max(e_ref) < 5e-3
    assert max(e_base) < 1e-4
    assert e_rep < 1e-5   # (a staging or WAR race shows up as a changing result)


# N, H, C, Cout, R, stride, pad
PIPELINE_CASES = [
    (1, 8, 256, 256, 1, 1, 0),      # one split of exactly 1 m-tile: prologue reads, no hand-over
    (2, 8, 256, 256, 1, 1, 0),      # 2 m-tiles: one hand-over, both X register-set parities
    (3, 7, 256, 256, 1, 1, 0),      # 3 m-tiles, M = 147: partial last m-tile
    (4, 7, 512, 512, 3, 1, 1),      # conv5 3x3: a 256-wide K tile is half a tap, 18 % padding reads
]


@pytest.mark.parametrize("stagger", [1, 2])
@pytest.mark.parametrize("case", PIPELINE_CASES)
def test_wgrad8_pipeline_edges(case, stagger):
    check(case, stagger)


# The 128 (co) x 256 (k) form for Cout <= 128: three halves per m-tile in a ring of three buffers,
# two phases per m-tile.
NARROW_CASES = [
    (2, 28, 128, 128, 3, 1, 1),     # stage-3 3x3: K = 1152 = 4.5 K-tiles (K tail), 25 m-tiles
    (2, 28, 128, 128, 3, 2, 1),     # the stride-2 one (M = 392: 6.1 m-tiles)
    (2, 14, 128, 120, 3, 1, 1),     # co tail
    (1, 8, 256, 128, 1, 1, 0),      # exactly 1 m-tile (only the prologue stages)
    (2, 8, 256, 128, 1, 1, 0),      # 2 m-tiles (the ring is never refilled)
    (3, 7, 256, 128, 1, 1, 0),      # 3 m-tiles, partial last one: first refill of buffer 2
    (4, 8, 256, 128, 1, 1, 0),      # 4 m-tiles: the ring wraps to buffer 0
]


@pytest.mark.parametrize("stagger", [1, 2])
@pytest.mark.parametrize("case", NARROW_CASES)
def test_wgrad8_narrow_tile(case, stagger):
    check(case, stagger)


def test_wgrad8_pipeline_several_splits():
    """Several m splits per tile (atomics from more than one block per output tile), with the
    stagger value the launcher uses by default."""
    check((32, 14, 256, 512, 1, 1, 0), 2)
