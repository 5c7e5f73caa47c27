"""Mixup / CutMix on the GPU: the MIX forms of the stem preprocess kernels (exact where every weight
is 0 or 1, against fp64 where they blend), the identity table against the unmixed kernels bit for
bit, the MIX forms of the two training heads against fp64, the four HIP engines' wiring of `mix=`,
and a captured whole step replayed with two tables.

A table row is (partner, y0, x0, y1, x1, w_pix bits, w_lab bits, 0): the pixel becomes
w*A_b + (1 - w)*A_partner with w = 0 inside the half-open box and w_pix outside (A: what the
unmixed kernel gives, each image with its own flip), the target w_lab*T(y_b) + (1 - w_lab)*T(y_p)
with T(y) = (1 - eps) onehot(y) + eps / K, and `correct` counts the argmax against y_b when
w_lab >= 0.5 and against y_p otherwise."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kernel_checks import Out, U, dev, rel64
from test_gpu_eltwise_edges import XENT1_ELEM, XENT_B, _xent_inputs, same_bits
from test_gpu_label_smoothing import ATOMIC_SPREAD, _batch, _check_dlogits, _hip_engine, _padded, _spread_dense_bias

pytestmark = pytest.mark.gpu

# --------------------------------------------------------------------------------- bounds
# The heads follow the rule of tests/test_gpu_eltwise_edges.py and test_gpu_label_smoothing.py: a
# kernel gets 8 x what torch's own fp32 soft-target cross_entropy loses against fp64 on the same
# inputs, and never less than the project's floors: loss 1e-5 relative, fp32 dlogits 1e-6
# norm-relative, 64 U S elementwise (S = (p + t) |gscale|), plus half a bf16 ulp of the reference
# for bf16 dlogits.  The torch floor, on a CPU, as the largest over every (ncls, B) of the grid:
#
#     for eps in (0.0, 0.1):
#         for scale in (1, 30):
#             for ncls in (10, 64, 65, 1000):
#                 for B in (1, 5, 37):
#                     x, lab, tab = head_case(ncls, B, scale, "cpu"); gs = float(torch.tensor(1 / B, dtype=torch.float32))
#                     yp, _, _, wl = rows(tab, B)
#                     def run(x):
#                         T = F.one_hot(lab, ncls).to(x.dtype) * (1 - eps) + eps / ncls
#                         w = wl.to(x.dtype)[:, None]
#                         x = x.clone().requires_grad_(True)
#                         l = F.cross_entropy(x, w * T + (1 - w) * T[yp], reduction="sum")
#                         (l * gs).backward()
#                         return l.item(), x.grad
#                     (l32, g32), (l64, g64) = run(x), run(x.double())
#                     S = mixed_ref(x, lab, gs, eps, tab)[2]
#                     # abs(l32 - l64) / l64 | (g32 - g64).norm() / g64.norm() | ((g32 - g64).abs() / (S + TINY)).max()
#
#     eps  scale  loss rel.  gradient norm-rel.  elementwise / S
#     0.0    1    8.68e-8    1.09e-7             2.02e-6 (33.9 U)
#     0.0   30    5.65e-8    4.10e-8             5.63e-6 (94.5 U)
#     0.1    1    1.74e-7    2.82e-7             1.61e-6 (27.0 U)
#     0.1   30    9.56e-8    6.23e-7             1.40e-6 (23.5 U)
#
# (the smallest mean loss per row of the grid is 2.87, so the relative loss error is well defined)
#
# The kernels' worst errors on an MI355X over the same grid (every ldl, ldd), one run:
#
#     eps  scale  loss rel. (xent / xent_f32)  f32 gradient norm-rel.  f32 elementwise / its bound
#     0.0    1    2.15e-7 / 1.50e-7            6.90e-8                 0.123
#     0.0   30    1.67e-7 / 2.13e-7            4.17e-8                 0.433
#     0.1    1    2.19e-7 / 2.39e-7            7.11e-8                 0.045
#     0.1   30    2.32e-7 / 1.65e-7            5.46e-8                 0.039
#
# i.e. at most 0.024 of the loss bound and 0.07 of the gradient bound; the bf16 dlogits reached
# 0.996 of theirs, which is the half bf16 ulp of the reference that rounding to bf16 costs by
# itself.  (The loss is an fp32 atomic sum in no fixed order on an accumulator preloaded with 3.0.)
FLOOR = {(0.0, 1): (8.68e-8, 1.09e-7, 2.02e-6), (0.0, 30): (5.65e-8, 4.10e-8, 5.63e-6),
         (0.1, 1): (1.74e-7, 2.82e-7, 1.61e-6), (0.1, 30): (9.56e-8, 6.23e-7, 1.40e-6)}
NCLS = (10, 64, 65, 1000)      # 65 crosses the wave width
SCALES = (1, 30)
EPS = (0.0, 0.1)


def tol(eps, scale):
    """(loss relative, fp32 dlogits norm-relative, elementwise in units of S)"""
    f = FLOOR[(eps, scale)]
    return max(1e-5, 8 * f[0]), max(1e-6, 8 * f[1]), max(XENT1_ELEM, 8 * f[2])


def N():
    from pddl.ops.native import require_native
    return require_native()


def table(rows_, device=dev):
    """rows of (partner, y0, x0, y1, x1, w_pix, w_lab) -> int32 [B][8]."""
    t = np.zeros((len(rows_), 8), dtype=np.int32)
    for i, r in enumerate(rows_):
        t[i, :5] = r[:5]
        t[i, 5:7] = np.array(r[5:7], dtype=np.float32).view(np.int32)
    return torch.from_numpy(t).to(device)


def identity(B, device=dev):
    return table([(b, 0, 0, 0, 0, 1.0, 1.0) for b in range(B)], device)


def rows(tab, B):
    """(partner, box, w_pix, w_lab) of the first B rows, the weights as the fp32 values the kernels read."""
    t = tab[:B]
    w = t[:, 5:7].contiguous().view(torch.float32)
    return t[:, 0].long().clamp(0, B - 1), t[:, 1:5].long(), w[:, 0], w[:, 1]


# ===================================================================================== stem
# (name, B, S, crop, mode, (oy, ox), input dtype, output dtype); mode 0 identity, 1 bilinear, 2 crop
STEM_CASES = [
    ("rows-crop", 5, 37, 24, 2, (3, 5), torch.uint8, torch.bfloat16),      # odd source width: every row its own alignment
    ("rows-identity", 5, 32, 32, 0, (0, 0), torch.uint8, torch.bfloat16),
    ("rows-wide", 2, 256, 256, 0, (0, 0), torch.uint8, torch.bfloat16),    # Ws = 131 > 128: the column loop runs twice
    ("pixel-bilinear", 5, 32, 40, 1, (0, 0), torch.float32, torch.bfloat16),
    ("f32-crop", 5, 37, 24, 2, (3, 5), torch.uint8, torch.float32),
    ("f32-bilinear", 5, 32, 40, 1, (0, 0), torch.uint8, torch.float32),
]
STEM_IDS = [c[0] for c in STEM_CASES]


@functools.lru_cache(maxsize=None)
def _stem_input(B, S, in_dtype):
    g = torch.Generator().manual_seed(100 * B + S)
    img = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=g).to(dev)
    # an unflipped image with a flipped partner and the reverse (partners below)
    flip = torch.tensor([0, 1, 0, 1, 1][:B], dtype=torch.uint8, device=dev)
    return (img if in_dtype == torch.uint8 else img.float()), flip


def _partners(B):
    return [0, 2, 1, 4, 3][:B] if B == 5 else [1, 0]


def _boxes(B, Hc, Wc, shift=0):
    """Empty, the whole image, 1 x 1 at (0, 0), one touching the bottom-right corner, one
    overhanging the image on every side but the right (to be clamped); `shift` rotates them."""
    b = [(0, 0, 0, 0), (0, 0, Hc, Wc), (0, 0, 1, 1), (Hc - 5, Wc - 7, Hc, Wc), (-4, -3, Hc + 9, 11)]
    b = b[shift:] + b[:shift]
    return b[:B] if B == 5 else [b[4], b[3]]


def _stem_tables(B, Hc, Wc, weights):
    """Two tables over the same partners: the boxes, and the boxes rotated by two rows."""
    out = []
    for k, shift in enumerate((0, 2)):
        bx = _boxes(B, Hc, Wc, shift)
        out.append(table([(p,) + bx[i] + (weights[(i + k) % len(weights)], 1.0) for i, p in enumerate(_partners(B))]))
    return out


def _run_stem(case, mix, crop_dev=False, variant=None):
    """One launch into a sentinel-filled output with a spare image behind the batch; returns the
    [B, hs, hs, 16] result after checking that rows >= B and the guards are untouched."""
    name, B, S, crop, mode, (oy, ox), in_dtype, out_dtype = case
    img, flip = _stem_input(B, S, in_dtype)
    hs = (crop + 6) // 2
    n = B * hs * hs * 16
    out = Out(n + hs * hs * 16, out_dtype)
    cd = torch.tensor([oy, ox], dtype=torch.int32, device=dev) if crop_dev else None
    try:
        if variant is not None:
            N().set_variant("stem", variant)
        N().stem_s2d(img, flip, mode, crop, crop, 0 if crop_dev else oy, 0 if crop_dev else ox, out.t, cd, mix)
    finally:
        if variant is not None:
            N().set_variant("stem", 1)
    owned = torch.zeros(out.n, dtype=torch.bool, device=dev)
    owned[:n] = True
    out.check(f"stem {name}", owned)
    return out.t[:n].view(B, hs, hs, 16)


def _s2d_mask(m):
    """[B, Hc, Wc] bool -> the s2d layout [B, hs, hs, 16] (False in the padding ring)."""
    B, Hc, Wc = m.shape
    hs, ws = (Hc + 6) // 2, (Wc + 6) // 2
    p = F.pad(m, (3, 3, 3, 3))
    return p.view(B, hs, 2, ws, 2).permute(0, 1, 3, 2, 4).reshape(B, hs, ws, 4, 1).expand(B, hs, ws, 4, 4).reshape(B, hs, ws, 16)


def _inside(tab, B, Hc, Wc):
    _, box, _, _ = rows(tab, B)
    ys = torch.arange(Hc, device=dev).view(1, Hc, 1)
    xs = torch.arange(Wc, device=dev).view(1, 1, Wc)
    return ((ys >= box[:, 0].view(B, 1, 1)) & (ys < box[:, 2].view(B, 1, 1)) &
            (xs >= box[:, 1].view(B, 1, 1)) & (xs < box[:, 3].view(B, 1, 1)))


def _check_padding(x2, what):
    B, hs, ws, _ = x2.shape
    v = x2.view(B, hs, ws, 4, 4)
    assert bool((v[..., 3] == 0).all()), f"{what}: channel 3 not zero"
    img = v.view(B, hs, ws, 2, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * hs, 2 * ws, 4)
    ring = torch.ones(2 * hs, 2 * ws, dtype=torch.bool, device=dev)
    ring[3:-3, 3:-3] = False
    assert bool((img[:, ring] == 0).all()), f"{what}: padding ring not zero"


@pytest.mark.parametrize("case", STEM_CASES, ids=STEM_IDS)
def test_stem_exact_with_weights_0_and_1(case):
    """Every weight 0 or 1: the result is, bit for bit, a selection between the unmixed outputs of
    the image and of its partner."""
    name, B, S, crop = case[:4]
    plain = _run_stem(case, None)
    for k, tab in enumerate(_stem_tables(B, crop, crop, (1.0, 0.0, 1.0))):
        what = f"stem {name} table {k}"
        got = _run_stem(case, tab)
        partner, _, w_pix, _ = rows(tab, B)
        take = _s2d_mask(_inside(tab, B, crop, crop)) | (w_pix == 0).view(B, 1, 1, 1)
        want = torch.where(take, plain[partner], plain)
        assert same_bits(got, want), f"{what}: {int((got != want).sum())} elements differ from the selection"
        assert not same_bits(got, plain), f"{what}: nothing was mixed"
        _check_padding(got, what)


@pytest.mark.parametrize("case", STEM_CASES, ids=STEM_IDS)
def test_stem_blend_against_fp64(case):
    """Weights 0.5, 0.3, 0.9 against fp64 w a + (1 - w) b.  a, b: the uint8 values over 255 for the
    identity / crop modes; for the bilinear mode the unmixed fp32 kernel's own values (its resize
    is pinned by the existing tests; the bound below counts the roundings of the blend, which is
    what this test is about).
    fp32 output: 8 x 2^-24 x max(a, b) -- six fp32 roundings (the constant 1/255, two scalings,
    1 - w, two products, the sum), with margin for contraction.  bf16 output: that plus
    2^-8 |ref| (one round-to-nearest and the boundary flip the fp32 error can cause)."""
    name, B, S, crop, mode, (oy, ox), in_dtype, out_dtype = case
    img, flip = _stem_input(B, S, in_dtype)
    if mode == 1:
        f32case = (name, B, S, crop, mode, (oy, ox), in_dtype, torch.float32)
        A = _run_stem(f32case, None).double()
    else:
        a = img[:, oy:oy + crop, ox:ox + crop].double() / 255.0               # [B, Hc, Wc, 3]
        a = torch.where(flip.bool().view(B, 1, 1, 1), a.flip(2), a)
        a = F.pad(a, (0, 1, 3, 3, 3, 3))                                       # channel 3 and the ring: zero
        hs = (crop + 6) // 2
        A = a.view(B, hs, 2, hs, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(B, hs, hs, 16)
    for k, tab in enumerate(_stem_tables(B, crop, crop, (0.5, 0.3, 0.9))):
        what = f"stem {name} blend table {k}"
        got = _run_stem(case, tab)
        partner, _, w_pix, _ = rows(tab, B)
        w = torch.where(_s2d_mask(_inside(tab, B, crop, crop)), 0.0, w_pix.double().view(B, 1, 1, 1))
        ref = w * A + (1.0 - w) * A[partner]
        bound = 8 * U * torch.maximum(A, A[partner])
        if out_dtype == torch.bfloat16:
            bound = bound + 2.0 ** -8 * ref.abs()
        err = (got.double() - ref).abs()
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print(f"{what}: worst err / bound {worst:.3f}")
        assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements over the bound ({worst:.2f} x)"
        _check_padding(got, what)


@pytest.mark.parametrize("case", STEM_CASES, ids=STEM_IDS)
def test_stem_identity_table_is_the_unmixed_kernel(case):
    B = case[1]
    assert same_bits(_run_stem(case, identity(B)), _run_stem(case, None))
    # a longer table (a graph's static buffer) serves a shorter batch
    assert same_bits(_run_stem(case, identity(B + 3)), _run_stem(case, None))


@pytest.mark.parametrize("case", [c for c in STEM_CASES if c[0].startswith("rows")], ids=lambda c: c[0])
def test_stem_row_form_equals_pixel_form_with_a_table(case):
    name, B, S, crop = case[:4]
    for weights in ((1.0, 0.0, 1.0), (0.5, 0.3, 0.9)):
        for tab in _stem_tables(B, crop, crop, weights):
            assert same_bits(_run_stem(case, tab, variant=1), _run_stem(case, tab, variant=0)), f"stem {name} {weights}"


def test_stem_device_crop_offset_equals_host_offset_with_a_table():
    for case in (STEM_CASES[0], STEM_CASES[4]):
        for tab in _stem_tables(case[1], case[3], case[3], (0.5, 0.0, 1.0)):
            assert same_bits(_run_stem(case, tab, crop_dev=True), _run_stem(case, tab))


def test_bad_tables_are_rejected_or_clamped():
    case = STEM_CASES[0]
    B, crop = case[1], case[3]
    plain = _run_stem(case, None)
    # partners and boxes far outside their ranges: a wrong picture, every read in range
    wild = table([(-7, -100, -100, 10 ** 6, 10 ** 6, 1.0, 1.0), (10 ** 6, 0, 0, 0, 0, 0.0, 1.0)] +
                 [(b, 2 ** 30, 2 ** 30, -2 ** 30, -2 ** 30, 1.0, 1.0) for b in range(2, B)])
    got = _run_stem(case, wild)
    assert same_bits(got[0], plain[0]) and same_bits(got[1], plain[B - 1]) and same_bits(got[2:], plain[2:])
    x, lab, gscale = _head_inputs(10, 5, 1)[:3]
    dl, st = torch.zeros(5, 64, dtype=torch.bfloat16, device=dev), torch.zeros(2, device=dev)
    for bad in (identity(5).float(), identity(5).cpu(), identity(4), identity(5)[:, :7], identity(8)[::2]):
        with pytest.raises(RuntimeError, match="mix"):
            N().stem_s2d(*_stem_input(B, case[2], case[6]), 2, crop, crop, 0, 0, torch.empty_like(plain), None, bad)
        with pytest.raises(RuntimeError, match="mix"):
            N().softmax_xent(x, lab, 10, gscale, dl, st[0:1], st[1:2], 0.0, bad)
    assert not bool(dl.any()) and not bool(st.any())


# ==================================================================================== heads
def head_case(ncls, B, scale, device=dev):
    """The logits of the existing head tests (ties at the maximum in rows 1 and 2) with a table over
    them: w_lab 0.5 (a tie: the own label counts), 1, 0.3, 0 in turn; row 2 mixes with row 1, whose
    label is the argmax; the last row mixes with itself; row 3 has a partner of its own label."""
    x, lab = _xent_inputs(ncls, B, scale)
    lab = lab.clone()
    partner = [(b + 1) % B for b in range(B)]
    if B > 3:
        partner[2] = 1
        lab[3] = lab[4]
    partner[B - 1] = B - 1
    w = (0.5, 1.0, 0.3, 0.0)
    tab = table([(partner[b], 0, 0, 0, 0, 1.0, w[b % 4]) for b in range(B)], device)
    return x.to(device), lab.to(device), tab


@functools.lru_cache(maxsize=None)
def _head_inputs(ncls, B, scale):
    x, lab, tab = head_case(ncls, B, scale)
    return x, lab, float(torch.tensor(1.0 / B, dtype=torch.float32)), tab


def mixed_ref(x, lab, gscale, eps, tab):
    """fp64: loss sum, gradient, S = (p + t) |gscale|, the count of `correct`."""
    B, K = x.shape
    xd = x.double()
    partner, _, _, wl = rows(tab, B)
    T = F.one_hot(lab, K).double() * (1.0 - eps) + eps / K
    w = wl.double().view(B, 1)
    t = w * T + (1.0 - w) * T[partner]
    p = torch.softmax(xd, 1)
    loss = (torch.logsumexp(xd, 1) - (t * xd).sum(1)).sum().item()
    j = torch.arange(K, device=x.device).expand_as(xd)
    pred = torch.where(xd == xd.max(1, keepdim=True).values, j, K).min(1).values
    counted = torch.where(wl >= 0.5, lab, lab[partner])
    return loss, (p - t) * gscale, (p + t) * abs(gscale), int((pred == counted).sum())


@functools.lru_cache(maxsize=None)
def _head_ref(ncls, B, scale, eps):
    x, lab, gscale, tab = _head_inputs(ncls, B, scale)
    return mixed_ref(x, lab, gscale, eps, tab)


WORST = {}


@pytest.mark.parametrize("ncls", NCLS)
@pytest.mark.parametrize("kernel", ["softmax_xent", "softmax_xent_f32"])
def test_mixed_training_heads_against_fp64(kernel, ncls):
    fn = getattr(N(), kernel)
    dtype = torch.bfloat16 if kernel == "softmax_xent" else torch.float32
    for scale in SCALES:
        for B in XENT_B:
            x, lab, gscale, tab = _head_inputs(ncls, B, scale)
            for ldl in (ncls, 1024):
                logits = _padded(x, ldl)
                before = logits.clone()
                for eps in EPS:
                    tol_loss, tol_grad, tol_elem = tol(eps, scale)
                    loss, dref, S, hits = _head_ref(ncls, B, scale, eps)
                    for ldd in (ncls, 1024):
                        what = f"{kernel} mix eps={eps} ncls={ncls} B={B} scale={scale} ldl={ldl} ldd={ldd}"
                        dl = Out(B * ldd, dtype)
                        ls, cr = Out(1, torch.float32, torch.tensor([3.0])), Out(1, torch.float32, torch.tensor([2.0]))
                        fn(logits, lab, ncls, gscale, dl.t.view(B, ldd), ls.t, cr.t, eps, tab)
                        for o in (dl, ls, cr):
                            o.check(what)
                        assert same_bits(logits, before), f"{what}: logits changed"
                        got = dl.t.view(B, ldd)
                        assert bool((got[:, ncls:] == 0).all()), f"{what}: pad columns of dlogits not zero"
                        assert cr.t.item() - 2.0 == hits, f"{what}: correct {cr.t.item() - 2.0} != {hits}"
                        e_loss = abs((ls.t.item() - 3.0) - loss) / loss
                        print(f"{what}: loss {e_loss:.2e} (<= {tol_loss:.1e})")
                        e_elem = _check_dlogits(what, got[:, :ncls], dref, S, dtype, tol_grad, tol_elem)
                        assert e_loss <= tol_loss, f"{what}: loss {e_loss:.3e} > {tol_loss:.1e}"
                        k = (kernel, eps, scale)
                        e_g = rel64(got[:, :ncls], dref) if dtype == torch.float32 else 0.0
                        old = WORST.get(k, (0.0, 0.0, 0.0))
                        WORST[k] = (max(old[0], e_loss), max(old[1], e_g), max(old[2], e_elem))
    for (kn, eps, scale), w in sorted(WORST.items()):
        if kn == kernel:
            print(f"worst {kn} eps={eps} scale={scale}: loss {w[0]:.2e} gradient {w[1]:.2e} "
                  f"elementwise {w[2]:.3f} of its bound")


@pytest.mark.parametrize("kernel", ["softmax_xent", "softmax_xent_f32"])
def test_identity_table_head_is_the_unmixed_head(kernel):
    """dlogits bit for bit, equal hit counts, and the loss sums (one fp32 atomic per row in no fixed
    order; the mixed form also adds a row's three terms in another order) within the documented
    spread of that sum."""
    fn = getattr(N(), kernel)
    dtype = torch.bfloat16 if kernel == "softmax_xent" else torch.float32
    for ncls, B, scale, ldd in ((1000, 37, 1, 1024), (1000, 37, 30, 1000), (65, 5, 30, 128), (10, 1, 1, 10)):
        x, lab, gscale, _ = _head_inputs(ncls, B, scale)
        for eps in EPS:
            res = []
            for tab in (None, identity(B), identity(B + 3)):
                dl, st = torch.full((B, ldd), 7.0, dtype=dtype, device=dev), torch.zeros(2, device=dev)
                fn(x, lab, ncls, gscale, dl, st[0:1], st[1:2], eps, tab)
                res.append((dl, st))
            for dl, st in res[1:]:
                what = f"{kernel} identity eps={eps} ncls={ncls} B={B} scale={scale}"
                assert same_bits(dl, res[0][0]), f"{what}: dlogits differ"
                assert st[1].item() == res[0][1][1].item(), f"{what}: correct differs"
                d = abs(st[0].item() - res[0][1][0].item()) / res[0][1][0].item()
                print(f"{what}: loss sums differ by {d:.2e}")
                assert d <= ATOMIC_SPREAD


# ================================================================================== engines
ENG_EPS = 0.1
ENG_B = 4


def _eng_table(B, crop=224):
    """A mixup row, a CutMix row, a row mixed with itself at w_lab 0.5, an identity row."""
    return table([(1, 0, 0, 0, 0, 0.3, 0.3), (2, 40, 60, 150, 224, 1.0, 1.0 - (110 * 164) / float(crop * crop)),
                  (2, 0, 0, 0, 0, 0.5, 0.5), (3, 0, 0, 0, 0, 1.0, 1.0)][:B])


@pytest.mark.parametrize("which", ["bf16-frozen", "bf16-train", "fp32-frozen", "fp32-train"])
def test_engine_hands_the_table_to_stem_and_head(which):
    """forward_backward(mix=table) of each HIP engine: its stem image is the direct stem_s2d launch
    with that table bit for bit, and loss, accuracy count and dlogits are the fp64 mixed head of the
    engine's own logits, to the eps = 0.1 / scale 1 bounds of the head test.  mix=None is the call
    without the argument."""
    B, K = ENG_B, 1000
    eng = _hip_engine(which, B, label_smoothing=ENG_EPS)
    eng.init(seed=3)
    _spread_dense_bias(eng)
    img, lab = _batch(B)
    flip = torch.tensor([0, 1, 1, 0], dtype=torch.uint8, device=dev)
    tab = _eng_table(B)
    gscale = 1.0 / B
    tol_loss, tol_grad, tol_elem = tol(ENG_EPS, 1)
    stats = eng.forward_backward(img, lab, gscale, flip=flip, mix=tab).clone()
    torch.cuda.synchronize()
    stem = (lambda: (eng.stem_x2 if hasattr(eng, "stem_x2") else eng.x2)[:B])    # (the fp32 engines call it x2)
    x2 = stem()
    want = torch.full_like(x2, float("nan"))
    N().stem_s2d(img, flip, 0, 224, 224, 0, 0, want, None, tab)
    assert same_bits(x2, want), f"{which}: the engine's stem image is not stem_s2d(mix=table)"
    logits = eng.logits[:B, :K]
    loss, dref, S, hits = mixed_ref(logits, lab, gscale, ENG_EPS, tab)
    plain = mixed_ref(logits, lab, gscale, ENG_EPS, identity(B))[0]
    e = abs(stats[0].item() - loss) / loss
    print(f"{which}: loss {stats[0].item():.6f} fp64 {loss:.6f} (rel {e:.2e}); unmixed target {plain:.6f}; "
          f"correct {stats[1].item()} fp64 {hits}")
    assert e <= tol_loss and abs(plain - loss) / loss > 100 * tol_loss
    assert stats[1].item() == hits
    dtype = torch.bfloat16 if which.startswith("bf16") else torch.float32
    _check_dlogits(f"{which} mixed head gradient", eng.dlogits[:B, :K], dref, S, dtype, tol_grad, tol_elem)
    assert bool((eng.dlogits[:B, K:] == 0).all())
    # mix=None and no argument: the same launches, so the same stem image and, of the same logits,
    # the same head outputs.  (The logits are compared, not assumed: the train-mode BN engines sum
    # their batch statistics in no fixed order, so two runs of one call already differ there; each
    # run is then held to the unmixed fp64 head of its own logits.)
    runs = []
    for kw in ({}, {"mix": None}):
        s = eng.forward_backward(img, lab, gscale, flip=flip, **kw).clone()
        torch.cuda.synchronize()
        runs.append((stem().clone(), eng.logits[:B].clone(), eng.dlogits[:B].clone(), s))
    assert same_bits(runs[0][0], runs[1][0])
    N().stem_s2d(img, flip, 0, 224, 224, 0, 0, want, None)
    assert same_bits(runs[0][0], want)
    same_logits = same_bits(runs[0][1], runs[1][1])
    print(f"{which}: logits of two unmixed runs bitwise equal: {same_logits}")
    assert same_logits or which.endswith("train"), f"{which}: a frozen-BN forward is the same bits every run"
    if same_logits:
        assert same_bits(runs[0][2], runs[1][2]) and runs[0][3][1].item() == runs[1][3][1].item()
    for _, lg, dlg, s in runs:
        loss, dref, S, hits = mixed_ref(lg[:, :K], lab, gscale, ENG_EPS, identity(B))
        assert abs(s[0].item() - loss) <= tol_loss * loss and s[1].item() == hits
        _check_dlogits(f"{which} unmixed head gradient", dlg[:, :K], dref, S, dtype, tol_grad, tol_elem)


def test_hip_engine_matches_torch_engine_with_mixup():
    """HipEngine against TorchEngine with a mixup table (every row blended, each with its own weight): the bounds of
    test_gpu_engine.test_engine_matches_reference (loss 3 %, per tensor 15 %, cosine > 0.99)."""
    from pddl.models.reference import TorchEngine
    B = ENG_B
    he = _hip_engine("bf16-frozen", B, label_smoothing=ENG_EPS)
    he.init(seed=3)
    _spread_dense_bias(he)
    te = TorchEngine(he.L, B, crop=224, device="cuda", fused_proj=he.fuse_proj, label_smoothing=ENG_EPS)
    te.params.copy_(he.params)
    img, lab = _batch(B)
    flip = torch.tensor([0, 1, 1, 0], dtype=torch.uint8, device="cuda")
    tab = table([(p, 0, 0, 0, 0, w, w) for p, w in ((2, 0.35), (3, 0.6), (1, 0.2), (0, 0.8))])
    s_h = he.forward_backward(img, lab, 1.0 / B, flip=flip, mix=tab).clone()
    s_t = te.forward_backward(img, lab, 1.0 / B, flip=flip, mix=tab)
    torch.cuda.synchronize()
    assert abs(s_h[0].item() - s_t[0].item()) / s_t[0].item() < 0.03
    bad = []
    for e in he.L.entries.values():
        if not e.trainable:
            continue
        a = he.grads[e.offset:e.offset + e.size].float()
        b = te.grads[e.offset:e.offset + e.size].float()
        r = ((a - b).norm() / (b.norm() + 1e-20)).item()
        if r > 0.15:
            bad.append((e.name, r))
    assert not bad, bad[:10]
    assert F.cosine_similarity(he.grads, te.grads, dim=0).item() > 0.99
    # and the table matters at this bound
    te0 = TorchEngine(he.L, B, crop=224, device="cuda", fused_proj=he.fuse_proj, label_smoothing=ENG_EPS)
    te0.params.copy_(he.params)
    s_0 = te0.forward_backward(img, lab, 1.0 / B, flip=flip)
    assert abs(s_0[0].item() - s_t[0].item()) > 1e-3 * s_t[0].item()


# ============================================================================ captured step
CAP_B = 32          # the batch and crop of tests/test_gpu_capture.py


def test_captured_step_reads_the_table_of_each_replay():
    """One whole-step graph of HipEngine, captured with the static table; replayed with a CutMix
    table, then with the identity table.  Each replay equals the eager step with that table from
    the parameters the replay started from (stats 1e-3, gradients 2e-3: the bounds of
    tests/test_gpu_capture.py), the identity replay equals the eager step without a table, and after
    each replay the stem image is the direct stem_s2d launch with that table, and loss and dlogits
    are the fp64 mixed head of the replayed logits.  (The loss alone could not tell the tables apart:
    with one weight for the whole batch, the label terms of a permutation sum to the same.)"""
    from pddl.train.graph import GraphedTrainStep
    from pddl.train.mix import cutmix_table
    from pddl.train.optim import make_optimizer
    from test_gpu_label_smoothing import _cap_inputs
    B = CAP_B
    eng = _hip_engine("bf16-frozen", B, graphed=True, label_smoothing=ENG_EPS)
    eng.init(seed=13)
    bias = _spread_dense_bias(eng)
    opt = make_optimizer("sgd", eng, lr=1e-3)
    img, lab, flip = _cap_inputs(bias)
    g = torch.Generator().manual_seed(5)
    cut = torch.from_numpy(cutmix_table(torch.randperm(B, generator=g).numpy(), (30, 50, 190, 224),
                                        1.0 - (160 * 174) / (224.0 * 224.0))).to(dev)
    gs = GraphedTrainStep(eng, opt, B, (224, 224), 1.0 / B, mix=True)
    gs(img[0], lab[0], flip[0], (0, 0), cut)
    torch.cuda.synchronize()
    assert gs.graph is not None
    # the two replays back to back, as in training (each is a whole step: the update is inside)
    replays = []
    for name, tab in (("cutmix", cut), ("identity", identity(B))):
        start = eng.params.clone()
        l_r = gs(img[1], lab[1], flip[1], (0, 0), tab)[0].item() / B
        g_r = eng.grads.clone()
        torch.cuda.synchronize()
        assert not torch.equal(eng.params, start)
        want, dref, S, _ = mixed_ref(eng.logits[:B, :1000], lab[1], 1.0 / B, ENG_EPS, tab)
        _check_dlogits(f"{name} replay", eng.dlogits[:B, :1000], dref, S, torch.bfloat16, *tol(ENG_EPS, 1)[1:])
        x2 = torch.full_like(eng.stem_x2[:B], float("nan"))
        N().stem_s2d(img[1], flip[1], 0, 224, 224, 0, 0, x2, None, tab)
        assert same_bits(eng.stem_x2[:B], x2), f"{name} replay: the stem did not read this table"
        replays.append((name, start, l_r, g_r, want / B, x2))
    assert not same_bits(replays[0][5], replays[1][5])
    # then each batch again as a whole eager step from the parameters its replay started from
    for (name, start, l_r, g_r, want, _), eager_kw in zip(replays, ({"mix": cut}, {})):
        eng.params.copy_(start)
        eng.after_update()
        l_e = eng.forward_backward(img[1], lab[1], 1.0 / B, flip=flip[1], **eager_kw)[0].item() / B
        g_e = eng.grads.clone()
        opt.step()
        eng.after_update()
        torch.cuda.synchronize()
        r_g = ((g_r - g_e).norm() / g_e.norm()).item()
        print(f"{name}: replay loss {l_r:.6f} eager {l_e:.6f} fp64 of the replay's logits {want:.6f}; "
              f"gradients differ by {r_g:.2e}")
        assert abs(l_r - l_e) <= 1e-3 * abs(l_e) and r_g < 2e-3
        assert abs(l_r - want) <= tol(ENG_EPS, 1)[0] * want
