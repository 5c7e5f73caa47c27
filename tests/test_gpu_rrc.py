"""Random-resized-crop in the stem preprocess kernels (stem_s2d mode 3, csrc/kernels/stem_rrc.hip)
against the definition in csrc/kernels/kernels.h (`StemParams::rrc`; `ref64` below is its fp64 form).
Every launch goes into a sentinel-guarded output and asserts the kernel form that ran."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kernel_checks import BF, F32, Out, bits, check_real, dev
from pddl.ops.native import require_native as N

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
same = lambda a, b: torch.equal(bits(a.contiguous()), bits(b.contiguous()))      # noqa: E731


def inputs(B, S, step=1):
    g = torch.Generator().manual_seed(7 * B + S)
    img = torch.randint(0, 256 // step, (B, S, S, 3), generator=g).mul(step).to(torch.uint8).to(dev)
    return img, (torch.arange(B, device=dev) % 3 == 1).to(torch.uint8)       # flips 0 1 0 0 1 ...


def run(img, flip, crop, dtype, rrc=None, mix=None, form="band", mode=0, off=(0, 0), variant=1, band=0):
    B, hs = img.shape[0], (crop + 6) // 2
    rrc = rrc if rrc is None or torch.is_tensor(rrc) else torch.tensor(rrc, dtype=torch.int32, device=dev)
    out = Out(B * hs * hs * 16, dtype)
    try:
        N().set_variant("stem", variant)
        N().set_variant("stem_rrc_band", band)
        N().stem_s2d(img, flip, mode, crop, crop, off[0], off[1], out.t, None, mix, rrc)
        ran = N().stem_last_launch()
    finally:
        N().set_variant("stem", 1)
        N().set_variant("stem_rrc_band", 0)
    out.check(f"stem {form}")
    assert ran[0] == form, f"the {ran[0]} form ran, not the {form} form"
    return out.t.view(B, hs, hs, 16), ran[1]


def s2d(a):      # [B, Hc, Wc, 3] -> the zero-padded space-to-depth layout [B, hs, ws, 16]
    B, hs, ws = a.shape[0], (a.shape[1] + 6) // 2, (a.shape[2] + 6) // 2
    return F.pad(a, (0, 1, 3, 3, 3, 3)).view(B, hs, 2, ws, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(B, hs, ws, 16)


def ref64(img, flip, crop, rows):
    """The definition in fp64 for in-range boxes: (raw 0..255 values [B, crop, crop, 3], the largest tap of each)."""
    S, o, den = img.shape[1], torch.arange(crop, device=dev), 2 * crop
    out, mag = [], []
    for b, (y0, x0, h, w) in enumerate(rows):
        assert 0 <= y0 and 1 <= h and y0 + h <= S and 0 <= x0 and 1 <= w and x0 + w <= S, "test bug: box outside"
        ny, nx = (2 * o + 1) * h - crop, (2 * (crop - 1 - o if flip[b] else o) + 1) * w - crop
        ty, tx = ny // den, nx // den                                     # (floor division)
        fy, fx = ((ny - ty * den).double() / den).view(-1, 1, 1), ((nx - tx * den).double() / den).view(1, -1, 1)
        ya, yb, xa, xb = y0 + ty.clamp(0, h - 1), y0 + (ty + 1).clamp(0, h - 1), x0 + tx.clamp(0, w - 1), x0 + (tx + 1).clamp(0, w - 1)
        src = img[b].double()
        A, Bq, C, D = src[ya][:, xa], src[ya][:, xb], src[yb][:, xa], src[yb][:, xb]
        top, bot = A + (Bq - A) * fx, C + (D - C) * fx
        out.append(top + (bot - top) * fy)
        mag.append(torch.stack([A, Bq, C, D]).amax(0))
    return torch.stack(out), torch.stack(mag)


# (name, source, crop, boxes, clamped boxes): 1 x 1, h = 1, w = 1, at the bottom-right corner, the whole source, overhanging
OVER = (-3, -4, 60, 20)
CASES = [
    ("s37c24", 37, 24, [(5, 7, 1, 1), (10, 0, 1, 20), (0, 12, 30, 1), (20, 17, 17, 20), (0, 0, 37, 37), OVER], {OVER: (0, 0, 37, 20)}),
    ("s37c40", 37, 40, [(17, 3, 3, 3), (0, 0, 37, 37)], {}),       # every source row reused by many output rows
    ("s37c256", 37, 256, [(2, 3, 30, 25), (6, 0, 31, 37)], {}),     # Ws = 131 > 128
]
# fp32 roundings of one value: fx, b - a, fma (top; bot alike, the two enter a convex combination: 3),
# bot - top, fy, fma, the constant 1/255, the scaling: K = 8, each at most U x the largest tap (check_real
# adds 4 U and, for bf16, 2^-8 |ref|).  Blended: both sides and the blend's 1 - w, two products and sum.
K_RRC, K_BLEND = 8, 16


@DTYPES
@pytest.mark.parametrize("S,crop", [(37, 24), (32, 32)])
def test_unscaled_boxes_are_the_crop_and_identity_modes_bitwise(S, crop, dtype):
    img, flip = inputs(5, S)
    m, old = S - crop, "rows" if dtype == BF else "pixel"
    offs = [(0, 0), (m, m), (m // 2, 0), (0, m), (m // 3, m // 2)]
    got, _ = run(img, flip, crop, dtype, [(oy, ox, crop, crop) for oy, ox in offs])
    for b, off in enumerate(offs):
        assert same(got[b], run(img, flip, crop, dtype, form=old, mode=2, off=off)[0][b]), f"image {b}: not mode 2 at {off}"
    assert m or same(got, run(img, flip, crop, dtype, form=old)[0]), "the identity box is not mode 0"


@DTYPES
def test_exact_interpolation_at_2x(dtype):
    # weights 1/4, 1/2, 3/4 on multiples of 16: every raw value an integer; then one fp32 multiply, one rounding
    crop, (img, flip) = 24, inputs(4, 50, step=16)
    rows = [(1, 2, h, w) for h in (crop // 2, 2 * crop) for w in (crop // 2, 2 * crop)]
    raw = ref64(img, flip, crop, rows)[0]
    assert bool((raw == raw.round()).all()) and bool((raw != raw[:, :1, :1]).any())
    want = s2d(torch.from_numpy(raw.cpu().numpy().astype(np.float32) * (np.float32(1) / np.float32(255))).to(dev)).to(dtype)
    got = run(img, flip, crop, dtype, rows)[0]
    assert same(got, want), f"{int((got != want).sum())} elements differ"


@DTYPES
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_real_inputs_against_fp64_and_band_form_equals_pixel_form(case, dtype):
    name, S, crop, rows, clamped = case
    img, flip = inputs(len(rows), S)
    raw, mag = ref64(img, flip, crop, [clamped.get(r, r) for r in rows])
    want, band = run(img, flip, crop, dtype, rows)
    assert name != "s37c24" or ((crop + 6) // 2) % band != 0, "test bug: the last band should be a partial one"
    check_real(want, s2d(raw / 255.0), s2d(mag / 255.0), K_RRC, f"rrc {name}", rounded=dtype == BF)
    assert same(run(img, flip, crop, dtype, rows, form="pixel", variant=0)[0], want)
    for band in (1, 3):                        # one s2d row per workgroup, three
        got, ran = run(img, flip, crop, dtype, rows, band=band)
        assert ran == band and same(got, want), f"{name}, band height {ran}"
    assert same(run(img.float(), flip, crop, dtype, rows, form="pixel")[0], want), "fp32 input"


@DTYPES
def test_mix_table_selects_and_blends_resampled_images(dtype):
    # weights 0 / 1: bit for bit a selection between the own and the partner's unmixed outputs; else fp64
    name, S, crop, rows, clamped = CASES[0]
    B, rrc, (img, flip) = len(rows), rows, inputs(len(rows), S)
    partner = torch.tensor([1, 0, 4, 5, 2, 3], device=dev)
    mbox = [(0, 0, 0, 0), (0, 0, crop, crop), (3, 2, 4, 3), (crop - 5, crop - 7, crop, crop), (-4, -3, crop + 9, 11), (6, 0, 13, crop)]
    inside = torch.zeros(B, crop, crop, 1, dtype=torch.bool, device=dev)
    for b, (y0, x0, y1, x1) in enumerate(mbox):
        inside[b, max(y0, 0):y1, max(x0, 0):x1] = True
    plain = run(img, flip, crop, dtype, rrc)[0]
    for weights in ((1.0, 0.0), (0.5, 0.3, 0.9)):
        w = torch.tensor([weights[b % len(weights)] for b in range(B)], dtype=torch.float32)
        tab = torch.zeros(B, 8, dtype=torch.int32)      # (partner, y0, x0, y1, x1, w_pix bits, w_lab bits, 0)
        tab[:, 0], tab[:, 1:5], tab[:, 5], tab[:, 6] = partner.cpu(), torch.tensor(mbox), w.view(torch.int32), 0x3F800000
        got = run(img, flip, crop, dtype, rrc, mix=tab.to(dev))[0]
        assert same(got, run(img, flip, crop, dtype, rrc, mix=tab.to(dev), form="pixel", variant=0)[0])
        wpix = torch.where(inside, 0.0, w.double().to(dev).view(B, 1, 1, 1))
        if len(weights) == 2:
            assert same(got, torch.where(s2d(wpix.expand(-1, -1, -1, 3)) == 0, plain[partner], plain)) and not same(got, plain)
        else:
            raw, mag = ref64(img, flip, crop, [clamped.get(r, r) for r in rows])
            ref = wpix * raw + (1 - wpix) * raw[partner]
            check_real(got, s2d(ref / 255.0), s2d(torch.maximum(mag, mag[partner]) / 255.0), K_BLEND, "rrc blend", rounded=dtype == BF)


def engine(which, B, **kw):
    from pddl.models import engine as e16, engine_f32 as e32
    from pddl.models.resnet50 import ParamLayout
    make = {"bf16-frozen": e16.make_hip_engine, "bf16-train": lambda *a, **k: e16.make_hip_engine(*a, bn_mode="train", **k),
            "fp32-frozen": e32.HipF32Engine, "fp32-train": e32.HipF32EngineBNTrain}[which]
    eng = make(ParamLayout(), B, crop=224, image_size=224, **kw)
    eng.init(seed=3)
    g = torch.Generator().manual_seed(B)
    hw = torch.randint(60, 225, (2, B, 2), generator=g)
    rrc = torch.cat([(torch.rand(2, B, 2, generator=g) * (225 - hw)).long(), hw], 2).to(torch.int32).to(dev)   # two tables
    img = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, generator=g).to(dev)
    return eng, img, torch.randint(0, 1000, (B,), generator=g).to(dev), (torch.arange(B, device=dev) % 3 == 1).to(torch.uint8), rrc


@pytest.mark.parametrize("which", ["bf16-frozen", "bf16-train", "fp32-frozen", "fp32-train", "captured"])
def test_engines_and_a_captured_step_hand_the_boxes_to_the_stem(which):
    # the stem image is bitwise the direct launch with the step's (or the replay's) table; rrc=None is today's image
    cap = which == "captured"
    eng, img, lab, flip, rrc = engine("bf16-frozen" if cap else which, 32 if cap else 4, **({"graphed": True} if cap else {}))
    B, step = img.shape[0], lambda tab: eng.forward_backward(img, lab, 1.0 / img.shape[0], flip=flip, rrc=tab)
    if cap:
        from pddl.train.graph import GraphedTrainStep
        from pddl.train.optim import make_optimizer
        gs = GraphedTrainStep(eng, make_optimizer("sgd", eng, lr=1e-3), B, (224, 224), 1.0 / B, rrc=True)
        step = lambda tab: gs(img, lab, flip, (0, 0), None, tab)      # noqa: E731 (the first call runs eagerly and captures)
    seen = []
    for tab in (rrc[0], rrc[1], rrc[0]) if cap else (rrc[0], None):
        step(tab)
        torch.cuda.synchronize()
        assert (not cap or gs.graph is not None) and N().stem_last_launch()[0] == ("band" if tab is not None else "rows" if which.startswith("bf16") else "pixel")
        x2 = (eng.stem_x2 if hasattr(eng, "stem_x2") else eng.x2)[:B]            # (the fp32 engines call it x2)
        seen.append(torch.full_like(x2, float("nan")))
        N().stem_s2d(img, flip, 0, 224, 224, 0, 0, seen[-1], None, None, tab)
        assert same(x2, seen[-1]), f"{which}: the stem image is not stem_s2d(rrc={'table' if tab is not None else None})"
    assert not same(seen[0], seen[1])
