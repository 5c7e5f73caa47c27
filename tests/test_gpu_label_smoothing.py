"""Label smoothing on the GPU: the three loss-head kernels (softmax_xent, softmax_xent_f32,
eval_metrics) with `smoothing` against fp64, eps = 0 against today's kernels bit for bit, the four
HIP engines' wiring of `label_smoothing`, and a captured whole step.

The target is t_j = (1 - eps) * [j == y] + eps / K, the loss logsumexp(z) - sum_j t_j z_j and the
gradient (softmax - t) * gscale (Keras CategoricalCrossentropy(label_smoothing=eps))."""
import functools

import pytest
import torch
import torch.nn.functional as F

from kernel_checks import Out, U, dev, rel64
from test_gpu_eltwise_edges import TINY, XENT1_ELEM, XENT_B, _xent_inputs, _xent_ref, same_bits

pytestmark = pytest.mark.gpu

# --------------------------------------------------------------------------------- bounds
# The rule of tests/test_gpu_eltwise_edges.py: a kernel gets 8 x what torch's own fp32
# cross_entropy loses against fp64 on the same inputs (__expf is the fast form), and never less than
# the project's scale-1 numbers: loss 1e-5 relative, fp32 dlogits 1e-6 norm-relative, 64 U S
# elementwise (S = (p + t) |gscale|).  The torch floor, on a CPU, as the largest over every
# (ncls, B) of the grid below:
#
#     for eps in (0.1, 1.0):
#         for scale in (1, 30):
#             for ncls in (10, 64, 65, 1000):
#                 for B in (1, 5, 37):
#                     x, lab = _xent_inputs(ncls, B, scale); gs = float(torch.tensor(1 / B, dtype=torch.float32))
#                     def run(x):
#                         x = x.clone().requires_grad_(True)
#                         l = F.cross_entropy(x, lab, reduction="sum", label_smoothing=eps)
#                         (l * gs).backward()
#                         return l.item(), x.grad
#                     (l32, g32), (l64, g64) = run(x), run(x.double())
#                     t = torch.full((B, ncls), eps / ncls, dtype=torch.float64); t[torch.arange(B), lab] += 1 - eps
#                     S = (torch.softmax(x.double(), 1) + t) * gs
#                     # abs(l32 - l64) / l64 | (g32 - g64).norm() / g64.norm() | ((g32 - g64).abs() / S).max()
#
#     eps  scale  loss rel.  gradient norm-rel.  elementwise / S
#     0.1    1    1.74e-7    2.82e-7             1.25e-6 (21.0 U)
#     0.1   30    1.23e-7    3.81e-7             8.81e-7 (14.8 U)
#     1.0    1    1.29e-7    8.37e-7             8.82e-7 (14.8 U)
#     1.0   30    1.15e-7    7.71e-7             7.70e-7 (12.9 U)
#
# (the smallest mean loss per row of the grid is 3.85, so the relative loss error is well defined)
#
# The kernels' worst errors on an MI355X over the same grid (every ldl, ldd), one run:
#
#     eps  scale  loss rel. (xent / xent_f32 / eval_metrics)  f32 gradient norm-rel.  f32 elementwise / S
#     0.1    1    2.45e-7 / 2.45e-7 / 1.67e-7                 6.84e-8                 9.6 U
#     0.1   30    1.61e-7 / 1.61e-7 / 1.61e-7                 5.50e-8                 7.3 U
#     1.0    1    2.09e-7 / 1.57e-7 / 9.78e-8                 1.05e-7                 7.5 U
#     1.0   30    1.56e-7 / 1.56e-7 / 1.15e-7                 7.87e-8                 5.0 U
#
# i.e. at most 0.025 of the loss bound, 0.05 of the gradient bound and 0.064 of the elementwise
# bound; the bf16 dlogits reached 0.998 of theirs, which is the half bf16 ulp of the reference
# that rounding to bf16 costs by itself.  (The loss is an fp32 atomic sum in no fixed order, on top
# of an accumulator preloaded with 3.0: its error is the sum's, not the per-row formula's.)  With
# and without `smoothing=0.0`, eval_metrics' loss sums differed by at most 1.45e-7 relative.
FLOOR = {(0.1, 1): (1.74e-7, 2.82e-7, 1.25e-6), (0.1, 30): (1.23e-7, 3.81e-7, 8.81e-7),
         (1.0, 1): (1.29e-7, 8.37e-7, 8.82e-7), (1.0, 30): (1.15e-7, 7.71e-7, 7.70e-7)}
NCLS = (10, 64, 65, 1000)      # 65 crosses the wave width
SCALES = (1, 30)
EPS = (0.1, 1.0)               # 1.0: the label has no weight of its own -- the one-hot term is really scaled
# The loss is one fp32 atomic per row in no fixed order: tests/test_gpu_eltwise_edges.py documents
# the spread of that sum as 4.52e-7 relative (8 x 5.65e-8)
ATOMIC_SPREAD = 4.52e-7


def tol(eps, scale):
    """(loss relative, fp32 dlogits norm-relative, elementwise in units of S)"""
    f = FLOOR[(eps, scale)]
    return max(1e-5, 8 * f[0]), max(1e-6, 8 * f[1]), max(XENT1_ELEM, 8 * f[2])


def N():
    from pddl.ops.native import require_native
    return require_native()


@functools.lru_cache(maxsize=None)
def _inputs(ncls, B, scale):
    x, lab = (t.to(dev) for t in _xent_inputs(ncls, B, scale))
    return x, lab, float(torch.tensor(1.0 / B, dtype=torch.float32))


def smoothed_ref(x, lab, gscale, eps):
    """fp64: loss sum, gradient, S = (p + t) |gscale|."""
    xd = x.double()
    t = torch.full_like(xd, eps / x.shape[1])
    t[torch.arange(x.shape[0], device=x.device), lab] += 1.0 - eps
    p = torch.softmax(xd, 1)
    loss = (torch.logsumexp(xd, 1) - (t * xd).sum(1)).sum().item()
    return loss, (p - t) * gscale, (p + t) * abs(gscale)


@functools.lru_cache(maxsize=None)
def _ref(ncls, B, scale, eps):
    """The shared, read-only fp64 reference of one case: (loss, gradient, S, top-1 hits, top-5 hits)."""
    x, lab, gscale = _inputs(ncls, B, scale)
    vl = x.gather(1, lab[:, None])
    idx = torch.arange(ncls, device=x.device)[None, :]
    rank = ((x > vl) | ((x == vl) & (idx < lab[:, None]))).sum(1)
    top1, top5 = int((rank == 0).sum()), int((rank < 5).sum())
    assert top1 == _xent_ref(x, lab, gscale)[3]     # the eps = 0 count of the existing test
    return smoothed_ref(x, lab, gscale, eps) + (top1, top5)


def _padded(x, ldl):
    logits = torch.full((x.shape[0], ldl), float("inf"), device=dev)
    logits[:, :x.shape[1]] = x
    return logits


def _check_dlogits(what, got, dref, S, dtype, tol_grad, tol_elem):
    """Elementwise against tol_elem S (+ half a bf16 ulp of the reference for bf16), and the fp32
    norm-relative error.  Returns the worst elementwise error over its bound."""
    err = (got.double() - dref).abs()
    bound = tol_elem * S + TINY
    if dtype == torch.bfloat16:
        bound = bound + torch.pow(2.0, (torch.frexp(dref)[1] - 9).double())
    worst = (err / bound).max().item()
    in_S = (err / (S + TINY)).max().item()
    msg = f"{what}: dlogits {worst:.3f} of the elementwise bound ({in_S / U:.1f} U S)"
    if dtype == torch.float32:
        e_grad = rel64(got, dref)
        msg += f", norm-relative {e_grad:.2e} (<= {tol_grad:.2e})"
    print(msg)
    assert worst <= 1.0, f"{what}: dlogits {worst:.2f} x the elementwise bound"
    if dtype == torch.float32:
        assert e_grad <= tol_grad, f"{what}: dlogits {e_grad:.3e} > {tol_grad:.2e}"
    return worst


# --------------------------------------------------------------------- 1. kernel edges
@pytest.mark.parametrize("ncls", NCLS)
@pytest.mark.parametrize("kernel", ["softmax_xent", "softmax_xent_f32"])
def test_smoothed_training_heads_edges(kernel, ncls):
    fn = getattr(N(), kernel)
    dtype = torch.bfloat16 if kernel == "softmax_xent" else torch.float32
    for scale in SCALES:
        for B in XENT_B:
            x, lab, gscale = _inputs(ncls, B, scale)
            for ldl in (ncls, 1024):
                logits = _padded(x, ldl)
                before = logits.clone()
                for eps in EPS:
                    tol_loss, tol_grad, tol_elem = tol(eps, scale)
                    loss, dref, S, top1, _ = _ref(ncls, B, scale, eps)
                    for ldd in (ncls, 1024):
                        what = f"{kernel} eps={eps} ncls={ncls} B={B} scale={scale} ldl={ldl} ldd={ldd}"
                        dl = Out(B * ldd, dtype)
                        ls, cr = Out(1, torch.float32, torch.tensor([3.0])), Out(1, torch.float32, torch.tensor([2.0]))
                        fn(logits, lab, ncls, gscale, dl.t.view(B, ldd), ls.t, cr.t, eps)
                        for o in (dl, ls, cr):
                            o.check(what)
                        assert same_bits(logits, before), f"{what}: logits changed"
                        got = dl.t.view(B, ldd)
                        assert bool((got[:, ncls:] == 0).all()), f"{what}: pad columns of dlogits not zero"
                        assert cr.t.item() - 2.0 == top1, f"{what}: correct {cr.t.item() - 2.0} != {top1}"
                        e_loss = abs((ls.t.item() - 3.0) - loss) / loss
                        print(f"{what}: loss {e_loss:.2e} (<= {tol_loss:.1e})")
                        _check_dlogits(what, got[:, :ncls], dref, S, dtype, tol_grad, tol_elem)
                        assert e_loss <= tol_loss, f"{what}: loss {e_loss:.3e} > {tol_loss:.1e}"


@pytest.mark.parametrize("ncls", NCLS)
def test_smoothed_eval_metrics_edges(ncls):
    nat = N()
    for scale in SCALES:
        for B in XENT_B:
            x, lab, _ = _inputs(ncls, B, scale)
            for ldl in (ncls, 1024):
                logits = _padded(x, ldl)
                before = logits.clone()
                plain = Out(3, torch.float32, torch.tensor([3.0, 2.0, 1.0]))
                nat.eval_metrics(logits, lab, ncls, 5, plain.t)
                for eps in EPS:
                    what = f"eval_metrics eps={eps} ncls={ncls} B={B} scale={scale} ldl={ldl}"
                    loss, _, _, top1, top5 = _ref(ncls, B, scale, eps)
                    out = Out(3, torch.float32, torch.tensor([3.0, 2.0, 1.0]))
                    nat.eval_metrics(logits, lab, ncls, 5, out.t, eps)
                    out.check(what)
                    assert same_bits(logits, before), f"{what}: logits changed"
                    got = out.t.tolist()
                    assert (got[1] - 2.0, got[2] - 1.0) == (top1, top5), f"{what}: hits {got[1:]} != {(top1, top5)}"
                    assert got[1:] == plain.t.tolist()[1:], f"{what}: hits differ from the eps = 0 hits"
                    e_loss = abs((got[0] - 3.0) - loss) / loss
                    print(f"{what}: loss {e_loss:.2e} (<= {tol(eps, scale)[0]:.1e})")
                    assert e_loss <= tol(eps, scale)[0], f"{what}: loss {e_loss:.3e}"


def test_smoothing_outside_0_1_is_rejected():
    nat = N()
    x, lab, gscale = _inputs(10, 5, 1)
    dl = torch.zeros(5, 64, dtype=torch.bfloat16, device=dev)
    dl32, out = torch.zeros(5, 10, device=dev), torch.zeros(3, device=dev)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match="smoothing"):
            nat.softmax_xent(x, lab, 10, gscale, dl, out[0:1], out[1:2], bad)
        with pytest.raises(RuntimeError, match="smoothing"):
            nat.softmax_xent_f32(x, lab, 10, gscale, dl32, out[0:1], out[1:2], smoothing=bad)
        with pytest.raises(RuntimeError, match="smoothing"):
            nat.eval_metrics(x, lab, 10, 5, out, smoothing=bad)
    assert not bool(out.any()) and not bool(dl.any()) and not bool(dl32.any())


# ------------------------------------------------------------- 2. eps = 0 is today's kernel
@pytest.mark.parametrize("kernel", ["softmax_xent", "softmax_xent_f32"])
def test_eps0_training_head_is_bit_identical(kernel):
    """dlogits of the 7-argument call and of smoothing=0.0 (positional and by keyword) are the same
    bits; the hit counts are equal and the loss sums (fp32 atomics in no fixed order) within the
    loss bound."""
    fn = getattr(N(), kernel)
    dtype = torch.bfloat16 if kernel == "softmax_xent" else torch.float32
    for ncls, B, scale, ldd in ((1000, 37, 1, 1024), (1000, 37, 30, 1000), (65, 5, 30, 128), (10, 1, 1, 10)):
        x, lab, gscale = _inputs(ncls, B, scale)
        res = []
        for extra, kw in (((), {}), ((0.0,), {}), ((), {"smoothing": 0.0})):
            dl, st = torch.full((B, ldd), 7.0, dtype=dtype, device=dev), torch.zeros(2, device=dev)
            fn(x, lab, ncls, gscale, dl, st[0:1], st[1:2], *extra, **kw)
            res.append((dl, st))
        for dl, st in res[1:]:
            assert same_bits(dl, res[0][0]), f"{kernel} ncls={ncls} B={B} scale={scale}: dlogits differ at eps = 0"
            assert st[1].item() == res[0][1][1].item()
            assert abs(st[0].item() - res[0][1][0].item()) <= 1e-5 * res[0][1][0].item()


def test_eps0_eval_metrics_is_unchanged():
    """Equal counts with and without the argument; the loss sums (fp32 atomics in no fixed order)
    within the documented spread of that sum.  (B = 1 has one addend: equal bits.)"""
    nat = N()
    for ncls, B, scale in ((1000, 37, 1), (65, 5, 1), (1000, 5, 30), (10, 1, 30)):
        x, lab, _ = _inputs(ncls, B, scale)
        a, b, c = (torch.zeros(3, device=dev) for _ in range(3))
        nat.eval_metrics(x, lab, ncls, 5, a)
        nat.eval_metrics(x, lab, ncls, 5, b, 0.0)
        nat.eval_metrics(x, lab, ncls, 5, c, smoothing=0.0)
        for o in (b, c):
            assert o[1:].tolist() == a[1:].tolist()
            d = abs(o[0].item() - a[0].item()) / a[0].item()
            print(f"eval_metrics eps=0 ncls={ncls} B={B} scale={scale}: loss sums differ by {d:.2e}")
            assert d <= ATOMIC_SPREAD and (B > 1 or d == 0.0)


# ----------------------------------------------------------------- 3. head consistency
@pytest.mark.parametrize("eps", EPS)
def test_eval_and_training_heads_agree(eps):
    """eval_metrics(eps) and softmax_xent(eps, gscale = 0) sum the same loss (to the loss bound of
    test 1), and gscale = 0 leaves all-zero dlogits."""
    nat = N()
    for ncls, B, scale in ((1000, 37, 1), (1000, 37, 30), (65, 5, 30), (10, 1, 1)):
        x, lab, _ = _inputs(ncls, B, scale)
        ev = torch.zeros(3, device=dev)
        nat.eval_metrics(x, lab, ncls, 5, ev, eps)
        for kernel, dtype in (("softmax_xent", torch.bfloat16), ("softmax_xent_f32", torch.float32)):
            dl, st = torch.full((B, 1024), 7.0, dtype=dtype, device=dev), torch.zeros(2, device=dev)
            getattr(nat, kernel)(x, lab, ncls, 0.0, dl, st[0:1], st[1:2], eps)
            assert bool((dl == 0).all()), f"{kernel}: gscale = 0 left non-zero dlogits"
            d = abs(st[0].item() - ev[0].item()) / ev[0].item()
            print(f"{kernel} vs eval_metrics eps={eps} ncls={ncls} B={B} scale={scale}: loss sums differ by {d:.2e}")
            assert d <= tol(eps, scale)[0] and st[1].item() == ev[1].item()


# -------------------------------------------------------------------- 4. engine wiring
ENG_EPS = 0.1
ENG_B = 4


def _hip_engine(which, B, crop=224, **kw):
    from pddl.models.engine import make_hip_engine
    from pddl.models.engine_f32 import HipF32Engine, HipF32EngineBNTrain
    from pddl.models.resnet50 import ParamLayout
    L = ParamLayout()
    if which.startswith("bf16"):
        eng = make_hip_engine(L, B, bn_mode=which.split("-")[1], crop=crop, image_size=224, **kw)
    else:
        cls = HipF32Engine if which == "fp32-frozen" else HipF32EngineBNTrain
        eng = cls(L, B, crop=crop, image_size=224, **kw)
    return eng


def _spread_dense_bias(eng, seed=17):
    """Dense bias 3 randn: the logits spread, so the smoothing term is far above rounding."""
    off = eng.L.off("dense", "bias")
    g = torch.Generator().manual_seed(seed)
    bias = 3 * torch.randn(1000, generator=g)
    eng.params[off:off + 1000] = bias.to(eng.params.device)
    eng.after_update()
    return bias


def _batch(B, seed=23):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, generator=g).cuda()
    return img, torch.randint(0, 1000, (B,), generator=g).cuda()


@pytest.mark.parametrize("which", ["bf16-frozen", "bf16-train", "fp32-frozen", "fp32-train"])
def test_engine_hands_label_smoothing_to_its_heads(which):
    """forward_backward, evaluate and evaluate_topk of each HIP engine against the fp64 smoothed
    loss and gradient of the engine's own logits, to the eps = 0.1 / scale 1 bounds of test 1.  (An
    engine that drops the option misses every gradient entry by eps / K gscale, ~10 % of a typical
    one, against 0.4 % for half a bf16 ulp.)"""
    B, K = ENG_B, 1000
    eng = _hip_engine(which, B, label_smoothing=ENG_EPS)
    assert eng.label_smoothing == ENG_EPS
    eng.init(seed=3)
    _spread_dense_bias(eng)
    img, lab = _batch(B)
    tol_loss, tol_grad, tol_elem = tol(ENG_EPS, 1)
    gscale = 1.0 / B
    stats = eng.forward_backward(img, lab, gscale).clone()
    torch.cuda.synchronize()
    logits = eng.logits[:B, :K]
    loss, dref, S = smoothed_ref(logits, lab, gscale, ENG_EPS)
    plain = smoothed_ref(logits, lab, gscale, 0.0)[0]
    e = abs(stats[0].item() - loss) / loss
    print(f"{which}: forward_backward loss {stats[0].item():.6f} fp64 {loss:.6f} (rel {e:.2e}); plain CE {plain:.6f}")
    assert e <= tol_loss and abs(plain - loss) / loss > 100 * tol_loss
    dtype = torch.bfloat16 if which.startswith("bf16") else torch.float32
    assert eng.dlogits.dtype == dtype
    _check_dlogits(f"{which} head gradient", eng.dlogits[:B, :K], dref, S, dtype, tol_grad, tol_elem)
    assert bool((eng.dlogits[:B, K:] == 0).all())
    # evaluate (the training head with gscale = 0) and evaluate_topk (eval_metrics): the smoothed
    # loss of the eval-mode logits
    for name in ("evaluate", "evaluate_topk"):
        out = getattr(eng, name)(img, lab).clone()
        torch.cuda.synchronize()
        want = smoothed_ref(eng.logits[:B, :K], lab, 0.0, ENG_EPS)[0]
        e = abs(out[0].item() - want) / want
        print(f"{which}: {name} loss {out[0].item():.6f} fp64 {want:.6f} (rel {e:.2e})")
        assert e <= tol_loss, f"{which} {name}: loss {e:.3e} > {tol_loss:.1e}"


def test_hip_engine_matches_torch_engine_with_label_smoothing():
    """HipEngine against TorchEngine(label_smoothing=0.1): the bounds of
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
    s_h = he.forward_backward(img, lab, 1.0 / B, flip=flip).clone()
    s_t = te.forward_backward(img, lab, 1.0 / B, flip=flip)
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
    # and the option matters at this bound: the dense-bias gradient is the batch sum of the head
    # gradient, whose label-free part moves by eps / K per class
    te0 = TorchEngine(he.L, B, crop=224, device="cuda", fused_proj=he.fuse_proj)
    te0.params.copy_(he.params)
    s_0 = te0.forward_backward(img, lab, 1.0 / B, flip=flip)
    assert abs(s_0[0].item() - s_t[0].item()) > 1e-3 * s_t[0].item()


# -------------------------------------------------------------------- 5. captured step
CAP_B = 32          # the batch and crop of tests/test_gpu_capture.py


def _cap_inputs(bias):
    """Two batches, labelled with the 32 classes of the smallest Dense bias: the label's logit lies
    ~2 sigma = 6 below the row mean, so eps = 0.1 lowers the loss by ~0.6 of ~17, far above the
    1e-3 to which a replay and an eager step agree."""
    g = torch.Generator().manual_seed(21)
    img = torch.randint(0, 256, (2, CAP_B, 224, 224, 3), dtype=torch.uint8, generator=g).cuda()
    low = bias.argsort()[:CAP_B]
    lab = torch.stack([low, low.flip(0)]).cuda()
    flip = torch.randint(0, 2, (2, CAP_B), dtype=torch.uint8, generator=g).cuda()
    return img, lab, flip


def _cap_engine(eps):
    """graphed=True: the engine of a whole-step graph, on one stream."""
    from pddl.train.optim import make_optimizer
    eng = _hip_engine("bf16-frozen", CAP_B, graphed=True, label_smoothing=eps)
    eng.init(seed=13)
    bias = _spread_dense_bias(eng)
    assert eng.side is None
    return eng, make_optimizer("sgd", eng, lr=1e-3), bias


def _replayed_step(eps):
    """One eager step (then the capture) and one replay of a whole-step graph; then the replayed
    batch again as an eager step FROM THE PARAMETERS THE REPLAY STARTED FROM.  (Two trajectories
    that each apply their own update cannot be held to 2e-3: an fp32 parameter difference of
    1e-8 from the weight gradients' atomic order flips bf16 roundings downstream and moved the
    next gradient by up to 1.5e-3 here.)  Returns the replay's and the eager step's
    (loss, gradient), and the fp64 smoothed and plain losses of the replay's logits."""
    from pddl.train.graph import GraphedTrainStep
    B = CAP_B
    eng, opt, bias = _cap_engine(eps)
    img, lab, flip = _cap_inputs(bias)
    gs = GraphedTrainStep(eng, opt, B, (224, 224), 1.0 / B)
    gs(img[0], lab[0], flip[0], (0, 0))
    torch.cuda.synchronize()
    assert gs.graph is not None
    start = eng.params.clone()
    replay = (gs(img[1], lab[1], flip[1], (0, 0))[0].item() / B, eng.grads.clone())
    torch.cuda.synchronize()
    assert opt.iterations == 2 and not torch.equal(eng.params, start)     # the graph holds the update too
    of_logits = [smoothed_ref(eng.logits[:B, :1000], lab[1], 1.0 / B, e)[0] / B for e in (eps, 0.0)]
    eng.params.copy_(start)
    eng.after_update()
    eager = (eng.forward_backward(img[1], lab[1], 1.0 / B, flip=flip[1])[0].item() / B, eng.grads.clone())
    torch.cuda.synchronize()
    return replay, eager, of_logits


def test_captured_step_keeps_label_smoothing():
    """A whole-step graph of HipEngine at eps = 0.1 replays its eager step (stats 1e-3, gradients
    2e-3: the bounds of tests/test_gpu_capture.py), its replayed loss is the smoothed loss of the
    replayed logits, and differs from the eps = 0 graph's."""
    (l_r, g_r), (l_e, g_e), (want, plain) = _replayed_step(ENG_EPS)
    r_g = ((g_r - g_e).norm() / g_e.norm()).item()
    print(f"eps {ENG_EPS}: replay loss {l_r:.6f} eager {l_e:.6f}, gradients differ by {r_g:.2e}; "
          f"fp64 of the replay's logits: smoothed {want:.6f} plain {plain:.6f}")
    assert abs(l_r - l_e) <= 1e-3 * abs(l_e) and r_g < 2e-3
    assert abs(l_r - want) <= tol(ENG_EPS, 1)[0] * want
    (l_0, _), (l_0e, _), (want0, _) = _replayed_step(0.0)
    print(f"eps 0: replay loss {l_0:.6f} eager {l_0e:.6f}")
    assert abs(l_0 - l_0e) <= 1e-3 * abs(l_0e) and abs(l_0 - want0) <= 1e-5 * want0
    # (the two graphs' weights differ by one SGD step of rate 1e-3 on the eps / K part of the gradient)
    assert abs(l_r - l_0) > 10 * 1e-3 * l_0, (l_r, l_0)
