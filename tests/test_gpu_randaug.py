"""RandAugment rows in the stem preprocess kernels (stem_s2d with a [B][16] table, csrc/kernels/stem_aug.hip)
against the definition in csrc/kernels/kernels.h (`StemParams::rrc`, "RandAugment rows"; `ref64` below is
its fp64 form).  Every launch goes into a sentinel-guarded output and asserts the kernel form that ran."""
import math
import struct

import numpy as np
import pytest
import torch

from kernel_checks import BF, F32, Out, check_real, dev
from pddl.ops.native import require_native as N
from test_gpu_rrc import CASES, K_RRC, inputs, s2d, same

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
FORMS = pytest.mark.parametrize("form", ["aug_tile", "aug_pixel"])
ONE, F255 = 1 << 16, np.float32(1) / np.float32(255)
BOXES, CLAMPED = CASES[0][3], CASES[0][4]        # s37c24: 1 x 1, h = 1, w = 1, corner, whole source, overhanging
LUMA = [float(np.float32(c)) for c in (0.299, 0.587, 0.114)]
# fp32 roundings of one value.  Geometry: the weights are exact, so K_RRC less its two weight roundings.
# Colour (raw values integers): color: 3 (grey) + v - g + fma + 1/255 + scaling = 7, contrast: 2 (mean) + 4 = 6,
# brightness 3, each at most U x (1 + |k|) x 255.  Mixed (exact sides): 2 x (1/255, scaling) + 1 - w, product, fma.
K_GEO, K_COLOR, K_MIX = K_RRC - 2, 7, 7


def table(rows, mats=None, ops=None):
    """[B][16]: boxes, float matrices (a b tx / d e ty, shifts in pixels; None: no map), chains [(code, par)..]."""
    t = torch.zeros(len(rows), 16, dtype=torch.int32)
    t[:, :4], t[:, 4], t[:, 8] = torch.tensor(rows), ONE, ONE
    for b, m in enumerate(mats or []):
        t[b, 4:10] = torch.tensor([round(v * ONE * (2 if k % 3 == 2 else 1)) for k, v in enumerate(m)])
        t[b, 10] = ONE
    for b, chain in enumerate(ops or []):
        for k, (code, par) in enumerate(chain):
            t[b, 10] |= code << (4 * k)
            t[b, 11 + k] = struct.unpack("i", struct.pack("f", par))[0]
    return t.to(dev)


def run(img, flip, crop, dtype, tab, form="aug_tile", mix=None):
    B, hs = img.shape[0], (crop + 6) // 2
    out = Out(B * hs * hs * 16, dtype)
    try:
        N().set_variant("stem", {"aug_tile": 2, "band": 1}.get(form, 0))     # (the per-pixel form is the default)
        N().stem_s2d(img, flip, 0, crop, crop, 0, 0, out.t, None, mix, tab)
        ran = N().stem_last_launch()[0]
    finally:
        N().set_variant("stem", 1)
    out.check(f"stem {form}")
    assert ran == form, f"the {ran} form ran, not the {form} form"
    return out.t.view(B, hs, hs, 16)


def mean_of(img, b, box):
    y0, x0, h, w = box
    p = img[b, y0:y0 + h, x0:x0 + w].long()
    return int(((19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 32768) >> 16).sum()), h * w


def chain64(x, chain, mean):
    """The colour chain in fp64: (values, the magnitude that carries the roundings)."""
    mag = torch.full_like(x, 255.0)
    for code, a in chain:
        a = struct.unpack("f", struct.pack("f", a))[0]
        g = mean if code == 3 else (LUMA[0] * x[..., 0] + LUMA[1] * x[..., 1] + LUMA[2] * x[..., 2]).unsqueeze(-1)
        x = {1: a * x, 2: g + a * (x - g), 3: g + a * (x - g), 4: torch.where(x >= a, 255.0 - x, x),
             5: (x.long() & int(a)).double()}[code].clamp(0, 255)
        mag = mag * (1 + abs(a)) if code < 4 else mag
    return x, mag


def ref64(img, flip, crop, tab, rows):
    """The definition in fp64 for has_geo rows over in-range boxes: (raw values [B, crop, crop, 3], largest tap)."""
    o, NQ = torch.arange(crop, device=dev), crop << 16
    u, v, out, mag = (2 * o + 1 - crop).view(1, -1), (2 * o + 1 - crop).view(-1, 1), [], []
    for b, (r, (y0, x0, h, w)) in enumerate(zip(tab.tolist(), rows)):
        assert r[10] >> 16 == 1, "test bug: a row without a map"
        U, V = r[4] * u + r[5] * v + r[6], r[7] * u + r[8] * v + r[9]
        U = -U if flip[b] else U
        fill = ((U.abs() >= NQ) | (V.abs() >= NQ)).unsqueeze(-1)

        def taps(P, n):
            X8 = torch.div((P.clamp(1 - NQ, NQ - 1) + NQ) * n, crop << 9, rounding_mode="floor") - 128
            return (X8 >> 8).clamp(0, n - 1), ((X8 >> 8) + 1).clamp(0, n - 1), ((X8 & 255).double() / 256).unsqueeze(-1)
        (ya, yb, fy), (xa, xb, fx) = taps(V, h), taps(U, w)
        src = img[b, y0:y0 + h, x0:x0 + w].double()
        A, Bq, C, D = src[ya, xa], src[ya, xb], src[yb, xa], src[yb, xb]
        top, bot = A + (Bq - A) * fx, C + (D - C) * fx
        out.append(torch.where(fill, 128.0, top + (bot - top) * fy))
        mag.append(torch.where(fill, 128.0, torch.stack([A, Bq, C, D]).amax(0)))
    return torch.stack(out), torch.stack(mag)


def permuted(img, flip, crop, rows, mats):
    """Integer matrices and whole-pixel shifts over crop-sized boxes, by index arithmetic: raw fp32 values."""
    o, out = torch.arange(crop, device=dev), []
    u, v = (2 * o + 1 - crop).view(1, -1), (2 * o + 1 - crop).view(-1, 1)
    for k, ((y0, x0, _, _), (a, b, c, d, e, f)) in enumerate(zip(rows, mats)):
        X, Y = a * u + b * v + 2 * c, d * u + e * v + 2 * f
        x, y = ((-X if flip[k] else X) + crop - 1) // 2, (Y + crop - 1) // 2
        ok = ((x >= 0) & (x < crop) & (y >= 0) & (y < crop)).unsqueeze(-1)
        out.append(torch.where(ok, img[k, (y0 + y).clamp(0, crop + y0 - 1), (x0 + x).clamp(0, crop + x0 - 1)].float(), 128.0))
    return torch.stack(out)


R30 = (math.cos(math.pi / 6), math.sin(math.pi / 6), 0, -math.sin(math.pi / 6), math.cos(math.pi / 6), 0)
SHEAR, SHIFT = (1, 0.3, 0, 0, 1, 0), (1, 0, 3.25, 0, 1, -1.5)
PRODUCT = tuple((np.array([R30[:3], R30[3:], (0, 0, 1)]) @ np.array([SHEAR[:3], SHEAR[3:], (0, 0, 1)])
                 @ np.array([SHIFT[:3], SHIFT[3:], (0, 0, 1)]))[:2].reshape(-1))
EXACT = [(0, 1, 0, -1, 0, 0), (0, -1, 0, 1, 0, 0), (-1, 0, 0, 0, -1, 0), (1, 0, 5, 0, 1, -3), (1, 0, 0, 0, 1, 0)]


@DTYPES
@FORMS
def test_identity_rows_are_the_four_column_result_bitwise(form, dtype):
    img, flip = inputs(len(BOXES), 37)
    old = run(img, flip, 24, dtype, torch.tensor(BOXES, dtype=torch.int32, device=dev), "band" if form == "aug_tile" else "pixel")
    assert same(run(img, flip, 24, dtype, table(BOXES), form), old)


@DTYPES
@FORMS
def test_quarter_turns_and_whole_pixel_shifts_permute_the_source_and_fill(form, dtype):
    img, flip = inputs(len(EXACT), 37)
    rows = [(5 + k, 7 - k, 24, 24) for k in range(len(EXACT))]
    raw = permuted(img, flip, 24, rows, EXACT)
    assert int((raw[3] == 128.0).sum()) >= 3 * 5 * 24, "test bug: the shifted picture has no fill"
    want = s2d(raw * float(F255)).to(dtype)
    got = run(img, flip, 24, dtype, table(rows, EXACT), form)
    assert same(got, want), f"{int((got != want).sum())} elements differ"


@DTYPES
@pytest.mark.parametrize("S", [37, 300])      # 300: the block's 300-row rectangle is over the LDS budget, global taps
@pytest.mark.parametrize("mat", [R30, SHEAR, SHIFT, PRODUCT], ids=["rotate", "shear", "shift", "product"])
def test_real_maps_against_fp64_and_tile_form_equals_pixel_form(mat, S, dtype):
    boxes = BOXES if S == 37 else [(0, 0, 300, 300), (20, 17, 280, 283), (5, 7, 1, 1)]
    rows = [CLAMPED.get(r, r) for r in boxes]
    (img, flip), tab = inputs(len(boxes), S), table(boxes, [mat] * len(boxes))
    raw, mag = ref64(img, flip, 24, tab, rows)
    got = run(img, flip, 24, dtype, tab)
    check_real(got, s2d(raw / 255.0), s2d(mag / 255.0), K_GEO, f"aug s{S}", rounded=dtype == BF)
    assert same(run(img, flip, 24, dtype, tab, "aug_pixel"), got)


@DTYPES
@FORMS
@pytest.mark.parametrize("chain", [[(4, 100.0)], [(5, 224.0)], [(1, 1.45)], [(2, 0.4)], [(2, 1.7)], [(3, 1.6)], [(3, 0.3), (4, 128.0), (1, 0.8), (5, 192.0)]],
                         ids=["solarize", "posterize", "brightness", "color-", "color+", "contrast", "chain"])
def test_colour_ops_on_an_unscaled_box(chain, form, dtype):
    (img, flip), box = inputs(2, 37), (5, 7, 24, 24)
    tab = table([box] * 2, None, [chain] * 2)
    got = run(img, flip, 24, dtype, tab, form)
    raw = torch.stack([img[b, 5:29, 7:31].flip(1) if flip[b] else img[b, 5:29, 7:31] for b in range(2)]).double()
    sums = [mean_of(img, b, box) for b in range(2)]
    mean = torch.tensor([s / n for s, n in sums], dtype=torch.float64, device=dev).view(2, 1, 1, 1)
    ref, mag = chain64(raw, chain, mean)
    if all(code >= 4 for code, _ in chain):
        assert same(got, s2d(ref.float() * float(F255)).to(dtype)), "an integer op is not exact"
    elif len(chain) == 1:                          # (the long chain mixes discontinuous ops with rounded ones: forms only)
        check_real(got, s2d(ref / 255.0), s2d(mag / 255.0), K_COLOR, f"aug {chain}", rounded=dtype == BF)
    assert same(got, run(img, flip, 24, dtype, tab, "aug_pixel"))
    want15 = [np.float32(s) / np.float32(n) if any(c == 3 for c, _ in chain) else np.float32(0) for s, n in sums]
    assert tab[:, 15].cpu().view(torch.float32).tolist() == [float(m) for m in want15], "column 15 is not the grey mean"


@DTYPES
@FORMS
def test_mix_table_resamples_the_partner_with_its_own_row(form, dtype):
    (img, flip), rows = inputs(2, 37), [(5, 7, 24, 24), (9, 2, 24, 24)]
    mats, chains = [EXACT[0], EXACT[3]], [[(4, 100.0)], [(5, 224.0)]]
    tab, mix = table(rows, mats, chains), torch.zeros(2, 8, dtype=torch.int32)
    w = torch.tensor([0.3, 0.75])
    mix[:, 0], mix[:, 1:5], mix[:, 5], mix[:, 6] = torch.tensor([1, 0]), torch.tensor([(3, 2, 14, 19), (0, 0, 0, 0)]), w.view(torch.int32), 0x3F800000
    got = run(img, flip, 24, dtype, tab, form, mix=mix.to(dev))
    raw = torch.stack([chain64(permuted(img, flip, 24, rows, mats)[b].double(), chains[b], None)[0] for b in range(2)])
    wpix = w.double().to(dev).view(2, 1, 1, 1).expand(2, 24, 24, 1).clone()
    wpix[0, 3:14, 2:19] = 0.0
    ref = wpix * raw + (1 - wpix) * raw.flip(0)
    check_real(got, s2d(ref / 255.0), s2d(torch.full_like(ref, 1.0)), K_MIX, "aug mix", rounded=dtype == BF)
    real = table(rows, [R30, PRODUCT], [[(3, 1.6)], [(2, 0.4)]])       # rounded sides: the two forms agree bit for bit
    assert same(run(img, flip, 24, dtype, real, form, mix=mix.to(dev)), run(img, flip, 24, dtype, real, "aug_pixel", mix=mix.to(dev)))


@pytest.mark.parametrize("cap", [False, True], ids=["eager", "captured"])
def test_engine_and_captured_step_hand_the_widened_table_to_the_stem(cap):
    from pddl.models.engine import make_hip_engine
    from pddl.models.resnet50 import ParamLayout
    B = 32 if cap else 4
    eng = make_hip_engine(ParamLayout(), B, crop=224, image_size=224, **({"graphed": True} if cap else {}))
    eng.init(seed=3)
    g = torch.Generator().manual_seed(B)
    img = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, generator=g).to(dev)
    lab, flip = torch.randint(0, 1000, (B,), generator=g).to(dev), (torch.arange(B, device=dev) % 3 == 1).to(torch.uint8)
    tabs = [table([(3 + b, 5, 180, 180 + b) for b in range(B)], [m] * B, [c] * B)
            for m, c in ((R30, [(3, 1.6)]), (PRODUCT, [(1, 1.45), (5, 224.0)]))]
    step = lambda tab: eng.forward_backward(img, lab, 1.0 / B, flip=flip, rrc=tab)      # noqa: E731
    if cap:
        from pddl.train.graph import GraphedTrainStep
        from pddl.train.optim import make_optimizer
        gs = GraphedTrainStep(eng, make_optimizer("sgd", eng, lr=1e-3), B, (224, 224), 1.0 / B, rrc=16)
        step = lambda tab: gs(img, lab, flip, (0, 0), None, tab)      # noqa: E731 (the first call runs eagerly and captures)
    seen = []
    for tab in (tabs[0], tabs[1], tabs[0]) if cap else tabs:
        step(tab)
        torch.cuda.synchronize()
        assert (not cap or gs.graph is not None) and N().stem_last_launch()[0] == "aug_pixel"
        seen.append(torch.full_like(eng.stem_x2[:B], float("nan")))
        N().stem_s2d(img, flip, 0, 224, 224, 0, 0, seen[-1], None, None, tab)
        assert same(eng.stem_x2[:B], seen[-1]), "the stem image is not stem_s2d(rrc=the widened table)"
    assert not same(seen[0], seen[1]) and (not cap or same(seen[0], seen[2]))
