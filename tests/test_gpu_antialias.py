"""stem_s2d `antialias=True` (csrc/kernels/stem_aa.hip) against the definition in csrc/kernels/kernels.h
(`ref64` of test_antialias_cpu.py is its fp64 form).  Every launch goes into a sentinel-guarded output and asserts
the form and band height that ran.  The bound: all terms are non-negative, so every rounding is relative to the
value.  uint8 input: the exact horizontal sum is divided (1), the vertical chain rounds per tap (T_y), then the
division and the scaling; fp32 input adds the T_x fma of the horizontal chain.  An unshrunk axis counts its 2 taps:
its lerp weight k / 2N is exact at the crops used with such boxes (16, 32), and on filtered rows those boxes are 2x
up (weights 1/4, 3/4), so the rounded difference is at most 3 roundings of the result.  With T = T_y + T_x:
|got - ref| <= (T + 4) 2^-24 ref, plus half a bf16 ulp for a bf16 output; a blend adds 3 (1 - w, product, fma)."""
import functools

import numpy as np
import pytest
import torch

from kernel_checks import BF, F32, Out, U, bits, dev
from pddl.ops.native import require_native as N
from test_antialias_cpu import ref64
from test_gpu_rrc import s2d

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
same = lambda a, b: torch.equal(bits(a.contiguous()), bits(b.contiguous()))      # noqa: E731
# (name, source, crop, a box per image): image 1 of each is flipped
CASES = [
    ("3.3x_2.3x_corner", 80, 24, [(0, 0, 80, 80), (3, 7, 55, 55), (25, 25, 55, 55)]),     # x0 = 7: shift 3 * 7 % 4 = 1
    ("exactly_2x", 48, 24, [(0, 0, 48, 48), (0, 5, 48, 36)]),
    ("one_axis_and_1px", 96, 32, [(5, 9, 16, 75), (5, 3, 90, 1), (2, 50, 1, 40)]),       # x only; w = 1; h = 1
    ("whole_2.3x", 37, 16, [(0, 0, 37, 37), (20, 17, 17, 20), (28, 1, 8, 36)]),
]
AUTO = 8     # the band height chosen at every kernel-test shape here (the launcher's cap: their spans fit LDS)


@functools.lru_cache(None)
def inputs(k):
    name, S, crop, rows = CASES[k]
    img = torch.randint(0, 256, (len(rows), S, S, 3), generator=torch.Generator().manual_seed(S)).to(torch.uint8)
    flip = (torch.arange(len(rows)) % 3 == 1).to(torch.uint8)
    raw, T = ref64(img.numpy(), rows, flip.tolist(), crop)
    return img.to(dev), flip.to(dev), torch.from_numpy(raw).to(dev), torch.from_numpy(T).to(dev)


def run(img, flip, crop, dtype, rrc, mix=None, form="aa_band", variant=1, band=0, antialias=True):
    B, hs = img.shape[0], (crop + 6) // 2
    rrc = rrc if torch.is_tensor(rrc) else torch.tensor(rrc, dtype=torch.int32, device=dev)
    out = Out(B * hs * hs * 16, dtype)
    try:
        N().set_variant("stem", variant)
        N().set_variant("stem_rrc_band", band)
        N().stem_s2d(img, flip, 0, crop, crop, 0, 0, out.t, None, mix, rrc, antialias=antialias)
        ran = N().stem_last_launch()
    finally:
        N().set_variant("stem", 1)
        N().set_variant("stem_rrc_band", 0)
    out.check(f"stem {form}")
    assert ran == (form, 0 if "pixel" in form else band or AUTO), f"{ran} ran, not the {form} form at band {band or AUTO}"
    return out.t.view(B, hs, hs, 16)


def check(got, raw, T, extra, what, rounded):
    ref = s2d(raw * float(np.float32(1) / np.float32(255)))
    bound = (s2d(T.expand_as(raw)) + 4 + extra) * U * ref
    if rounded:       # half a bf16 ulp of the value that is rounded
        bound = bound + torch.where(ref > 0, 2.0 ** (torch.floor(torch.log2((ref + bound).clamp_min(1e-30))) - 8), 0.0)
    err = (got.double() - ref).abs()
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} over, worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}"


@DTYPES
@pytest.mark.parametrize("k", range(len(CASES)), ids=[c[0] for c in CASES])
def test_both_forms_against_fp64_and_each_other(k, dtype):
    (name, S, crop, rows), (img, flip, raw, T) = CASES[k], inputs(k)
    want = run(img, flip, crop, dtype, rows)
    check(want, raw, T, 0, f"antialias {name}", dtype == BF)
    assert same(run(img, flip, crop, dtype, rows, band=1), want), "(crop + 6) / 2 bands with overlapping spans"
    assert same(run(img, flip, crop, dtype, rows, form="aa_pixel", variant=0), want), "the per-pixel form"
    check(run(img.float(), flip, crop, dtype, rows, form="aa_pixel"), raw, T, 0, f"antialias {name} fp32 input", dtype == BF)


@DTYPES
def test_constant_image_is_exact_for_any_box(dtype):
    S, crop, vals = 96, 16, torch.tensor([[255, 1, 128], [37, 200, 0], [90, 254, 3]], dtype=torch.uint8)
    img = vals.view(3, 1, 1, 3).expand(3, S, S, 3).contiguous().to(dev)
    flip, rows = torch.tensor([0, 1, 0], dtype=torch.uint8, device=dev), [(0, 0, 96, 96), (11, 23, 85, 41), (90, 1, 6, 95)]
    pic = (vals.float() * (np.float32(1) / np.float32(255))).view(3, 1, 1, 3).expand(3, crop, crop, 3).to(dev)
    for kw in ({}, {"band": 1}, {"form": "aa_pixel", "variant": 0}):
        assert same(run(img, flip, crop, dtype, rows, **kw), s2d(pic).to(dtype)), kw


@DTYPES
def test_unshrunk_boxes_are_the_flag_off_picture_bitwise(dtype):
    S, crop, rows = 37, 24, [(5, 7, 1, 1), (10, 0, 1, 20), (0, 12, 24, 1), (13, 13, 24, 24), (0, 0, 24, 24), (3, 2, 17, 23)]
    img = torch.randint(0, 256, (len(rows), S, S, 3), generator=torch.Generator().manual_seed(3)).to(torch.uint8).to(dev)
    flip = (torch.arange(len(rows), device=dev) % 3 == 1).to(torch.uint8)
    off = run(img, flip, crop, dtype, rows, form="band", antialias=False)
    assert same(run(img, flip, crop, dtype, rows), off)
    assert same(run(img, flip, crop, dtype, rows, form="aa_pixel", variant=0), off)


@DTYPES
def test_mix_table_selects_and_blends_antialiased_images(dtype):
    (name, S, crop, rows), (img, flip, raw, T) = CASES[0], inputs(0)
    B, partner, mbox = len(rows), torch.tensor([1, 2, 0], device=dev), [(0, 0, 0, 0), (3, 2, 14, 9), (-4, -3, crop + 9, 11)]
    inside = torch.zeros(B, crop, crop, 1, dtype=torch.bool, device=dev)
    for b, (y0, x0, y1, x1) in enumerate(mbox):
        inside[b, max(y0, 0):y1, max(x0, 0):x1] = True
    plain = run(img, flip, crop, dtype, rows)
    for weights in ((1.0, 0.0, 1.0), (0.5, 0.3, 0.9), None):
        tab = torch.zeros(B, 8, dtype=torch.int32)      # (partner, y0, x0, y1, x1, w_pix bits, w_lab bits, 0)
        w = torch.tensor(weights or (1.0, 1.0, 1.0), dtype=torch.float32)
        tab[:, 0], tab[:, 5], tab[:, 6] = (partner.cpu() if weights else torch.arange(B)), w.view(torch.int32), 0x3F800000
        tab[:, 1:5] = torch.tensor(mbox if weights else [(0, 0, 0, 0)] * B)
        got = run(img, flip, crop, dtype, rows, mix=tab.to(dev))
        assert same(got, run(img, flip, crop, dtype, rows, mix=tab.to(dev), form="aa_pixel", variant=0))
        wpix = torch.where(inside, 0.0, w.double().to(dev).view(B, 1, 1, 1))
        if weights is None:
            assert same(got, plain), "the identity table"
        elif weights[1] == 0.0:
            assert same(got, torch.where(s2d(wpix.expand(-1, -1, -1, 3)) == 0, plain[partner], plain)) and not same(got, plain)
        else:
            check(got, wpix * raw + (1 - wpix) * raw[partner], torch.maximum(T, T[partner]), 3, "antialias blend", dtype == BF)


@pytest.mark.parametrize("which", ["bf16-frozen", "bf16-train", "fp32-frozen", "fp32-train", "captured"])
def test_engines_evaluation_and_a_captured_step_use_the_antialias_kernel(which):
    from pddl.models import engine as e16, engine_f32 as e32
    from pddl.models.resnet50 import ParamLayout
    from pddl.train.graph import GraphedTrainStep
    from pddl.train.optim import make_optimizer
    cap = which == "captured"
    make = {"bf16-frozen": e16.make_hip_engine, "bf16-train": lambda *a, **k: e16.make_hip_engine(*a, bn_mode="train", **k),
            "fp32-frozen": e32.HipF32Engine, "fp32-train": e32.HipF32EngineBNTrain, "captured": e16.make_hip_engine}[which]
    B, g = 32 if cap else 4, torch.Generator().manual_seed(9)
    eng = make(ParamLayout(), B, crop=224, image_size=256, antialias=True, **({"graphed": True} if cap else {}))
    eng.init(seed=3)
    full = torch.tensor([[0, 0, 256, 256]] * B, dtype=torch.int32, device=dev)
    rrc = [full, full + torch.tensor([7, 3, -10, -130], dtype=torch.int32, device=dev)]     # the second: shrunk in y only
    img = torch.randint(0, 256, (B, 256, 256, 3), dtype=torch.uint8, generator=g).to(dev)
    lab, flip = torch.randint(0, 1000, (B,), generator=g).to(dev), (torch.arange(B, device=dev) % 3 == 1).to(torch.uint8)
    step = lambda tab: eng.forward_backward(img, lab, 1.0 / B, flip=flip, rrc=tab)      # noqa: E731
    if cap:     # (the first call runs eagerly and captures)
        gs = GraphedTrainStep(eng, make_optimizer("sgd", eng, lr=1e-3), B, (256, 256), 1.0 / B, rrc=True)
        step = lambda tab: gs(img, lab, flip, (0, 0), None, tab)      # noqa: E731
    seen = []
    for tab in (rrc[0], rrc[1], rrc[0]) if cap else (rrc[0], None):
        step(tab) if tab is not None else eng.evaluate(img, lab)
        torch.cuda.synchronize()
        assert (not cap or gs.graph is not None) and N().stem_last_launch() == ("aa_band", 5)   # (the tallest band at 256 px)
        x2 = (eng.stem_x2 if hasattr(eng, "stem_x2") else eng.x2)[:B]            # (the fp32 engines call it x2)
        seen.append(torch.full_like(x2, float("nan")))
        N().stem_s2d(img, flip if tab is not None else None, 0, 224, 224, 0, 0, seen[-1], None, None,
                     tab if tab is not None else full, antialias=True)
        assert same(x2, seen[-1]), f"{which}: the stem image is not stem_s2d(rrc=table, antialias=True)"
    assert not same(seen[0], seen[1])
