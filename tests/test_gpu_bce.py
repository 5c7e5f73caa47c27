"""The sigmoid binary cross-entropy heads on the GPU (sigmoid_bce, sigmoid_bce_f32, eval_metrics(bce=True)) against
fp64 -- F.binary_cross_entropy_with_logits in double on the explicit target matrix, mean over the classes, and the
closed-form gradient (sigmoid - t) gscale / K -- then the four HIP engines' wiring of loss="bce" and a captured step.

Bounds, by the rule of tests/test_gpu_label_smoothing.py: max(the project's lower limits -- loss 1e-5 relative, fp32
dlogits 1e-6 norm-relative, 64 U S elementwise with S = (sigmoid + t) |gscale| / K --, 8 x what the definition loses
in plain fp32 torch on a CPU against fp64), the largest over the grid below (every ncls, B, eps, thresh, mix):

    scale  loss rel.  gradient norm-rel.  elementwise / S     smallest mean loss per row
      1    1.33e-7    1.09e-7             2.11e-7 (3.5 U)     1.13
     30    1.55e-7    5.80e-8             2.33e-7 (3.9 U)     17.8

The kernels' worst errors on an MI355X over the same grid (every ldl, ldd), one run:

    scale  loss rel. (bce / bce_f32 / eval_metrics)  f32 gradient norm-rel.  f32 elementwise / S
      1    3.14e-7 / 3.14e-7 / 3.14e-7                 1.07e-7                 4.4 U
     30    1.37e-7 / 1.37e-7 / 1.01e-7                 5.33e-8                 3.7 U

i.e. at most 0.03 of the loss bound, 0.11 of the gradient bound and 0.07 of the elementwise bound; the bf16 dlogits
reached 0.9986 of theirs, the half bf16 ulp of the reference that rounding to bf16 costs by itself.  (The loss is an
fp32 atomic sum in no fixed order on top of an accumulator preloaded with 3.0.)
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from kernel_checks import Out, dev, rel64
from test_gpu_eltwise_edges import XENT1_ELEM, _xent_inputs, same_bits
from test_gpu_label_smoothing import CAP_B, N, _batch, _check_dlogits, _hip_engine, _padded, _spread_dense_bias
from test_gpu_mix import _eng_table, identity, table

pytestmark = pytest.mark.gpu
FLOOR = {1: (1.33e-7, 1.09e-7, 2.11e-7), 30: (1.55e-7, 5.80e-8, 2.33e-7)}
NCLS = (7, 8, 9, 512, 513, 1000)   # either side of a lane's 8 columns, one full wave iteration, one past it, production
GRID = [(B, scale, eps, thr, mixed) for B in (1, 5) for scale in (1, 30) for eps in (0.0, 0.1) for thr in (None, 0.2)
        for mixed in (False, True)]
KERNELS = {"sigmoid_bce": torch.bfloat16, "sigmoid_bce_f32": torch.float32}


def tol(scale):
    """(loss relative, fp32 dlogits norm-relative, elementwise in units of S)"""
    f = FLOOR[scale]
    return max(1e-5, 8 * f[0]), max(1e-6, 8 * f[1]), max(XENT1_ELEM, 8 * f[2])


def mix_tab(B, device=dev):
    """Label weights 0.3, 0.5, 0.3 (its own partner: the same label twice), 1 and 0.7."""
    return table([(p, 0, 0, 0, 0, 1.0, w) for p, w in ((1, 0.3), (2, 0.5), (2, 0.3), (3, 1.0), (0, 0.7))][:B] if B > 1
                 else [(0, 0, 0, 0, 0, 1.0, 0.3)], device)


def bce_ref(x, lab, gscale, eps, thr, tab):
    """fp64: loss sum, gradient, S, the count of `correct`."""
    B, K = x.shape
    xd, counted = x.double(), lab
    t = F.one_hot(lab, K).double() * (1.0 - eps) + eps / K
    if tab is not None:
        p, w = tab[:B, 0].long(), tab[:B, 6].contiguous().view(torch.float32).double()
        t, counted = w[:, None] * t + (1.0 - w[:, None]) * t[p], torch.where(w >= 0.5, lab, lab[p])
    if thr is not None:
        t = (t > thr).double()
    loss = F.binary_cross_entropy_with_logits(xd, t, reduction="none").mean(1).sum().item()
    j = torch.arange(K, device=x.device).expand_as(xd)
    pred = torch.where(xd == xd.max(1, keepdim=True).values, j, K).min(1).values
    sig = torch.sigmoid(xd)
    return loss, (sig - t) * gscale / K, (sig + t) * abs(gscale) / K, int((pred == counted).sum())


@functools.lru_cache(maxsize=None)
def case(ncls, B, scale, eps, thr, mixed):
    """The shared, read-only inputs and fp64 reference of one case."""
    x, lab = (t.to(dev) for t in _xent_inputs(ncls, B, scale))
    gscale, tab = float(torch.tensor(1.0 / B, dtype=torch.float32)), mix_tab(B) if mixed else None
    return (x, lab, gscale, tab) + bce_ref(x, lab, gscale, eps, thr, tab)


def _thr(thr):
    return {} if thr is None else {"thresh": thr}


@pytest.mark.parametrize("ncls", NCLS)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_training_heads_against_fp64(kernel, ncls):
    fn, dtype = getattr(N(), kernel), KERNELS[kernel]
    ldd_pad = (ncls // 64 + 1) * 64
    for B, scale, eps, thr, mixed in GRID:
        x, lab, gscale, tab, loss, dref, S, hits = case(ncls, B, scale, eps, thr, mixed)
        tol_loss, tol_grad, tol_elem = tol(scale)
        for ldd in (ldd_pad,) + ((ncls,) if dtype == torch.float32 else ()):
            bits = []
            for ldl in (ldd_pad, ncls + 3):     # pad columns of +inf: a stray read shows in the loss
                what = f"{kernel} ncls={ncls} B={B} scale={scale} eps={eps} thr={thr} mix={mixed} ldl={ldl} ldd={ldd}"
                dl = Out(B * ldd, dtype)
                ls, cr = Out(1, torch.float32, torch.tensor([3.0])), Out(1, torch.float32, torch.tensor([2.0]))
                fn(_padded(x, ldl), lab, ncls, gscale, dl.t.view(B, ldd), ls.t, cr.t, eps, tab, **_thr(thr))
                for o in (dl, ls, cr):
                    o.check(what)
                got = dl.t.view(B, ldd)
                assert bool((got[:, ncls:] == 0).all()), f"{what}: pad columns of dlogits not zero"
                assert cr.t.item() - 2.0 == hits, f"{what}: correct {cr.t.item() - 2.0} != {hits}"
                e_loss = abs((ls.t.item() - 3.0) - loss) / loss
                print(f"{what}: loss {e_loss:.2e} (<= {tol_loss:.1e})")
                _check_dlogits(what, got[:, :ncls], dref, S, dtype, tol_grad, tol_elem)
                assert e_loss <= tol_loss, f"{what}: loss {e_loss:.3e} > {tol_loss:.1e}"
                bits.append(got.clone())
            if not mixed:       # the identity table (longer than the batch) is the unmixed call, bit for bit
                fn(_padded(x, ldd_pad), lab, ncls, gscale, got, ls.t, cr.t, eps, identity(B + 3), **_thr(thr))
                bits.append(got)
            assert all(same_bits(bits[0], o) for o in bits[1:]), f"{what}: dlogits differ between aligned / misaligned logits / the identity table"


@pytest.mark.parametrize("ncls", NCLS)
def test_eval_metrics_bce_against_fp64_and_the_training_head(ncls):
    nat = N()
    for B, scale, eps, thr, mixed in GRID:
        if mixed:
            continue
        x, lab, _, _, loss, _, _, _ = case(ncls, B, scale, eps, thr, False)
        for ldl in ((ncls // 64 + 1) * 64, ncls + 3):
            what = f"eval_metrics bce ncls={ncls} B={B} scale={scale} eps={eps} thr={thr} ldl={ldl}"
            logits = _padded(x, ldl)
            plain, out = (Out(3, torch.float32, torch.tensor([3.0, 2.0, 1.0])) for _ in range(2))
            nat.eval_metrics(logits, lab, ncls, 5, plain.t, eps)
            nat.eval_metrics(logits, lab, ncls, 5, out.t, eps, bce=True, **_thr(thr))
            out.check(what)
            assert out.t.tolist()[1:] == plain.t.tolist()[1:], f"{what}: hits differ from the softmax form's"
            dl, st = torch.empty(B, 1024, dtype=torch.bfloat16, device=dev), torch.zeros(2, device=dev)
            nat.sigmoid_bce(logits, lab, ncls, 0.0, dl, st[0:1], st[1:2], eps, None, **_thr(thr))
            e_loss, e_head = abs((out.t[0].item() - 3.0) - loss) / loss, abs((out.t[0].item() - 3.0) - st[0].item()) / loss
            print(f"{what}: loss {e_loss:.2e}, against the training head {e_head:.2e} (<= {tol(scale)[0]:.1e})")
            assert max(e_loss, e_head) <= tol(scale)[0] and st[1].item() == out.t[1].item() - 2.0, what


def test_bad_threshold_is_rejected():
    nat, (x, lab, gscale) = N(), case(9, 5, 1, 0.0, None, False)[:3]
    dl, dl32, out = torch.zeros(5, 64, dtype=torch.bfloat16, device=dev), torch.zeros(5, 9, device=dev), torch.zeros(3, device=dev)
    for bad in (1.0, 1.5, float("nan")):
        for call in (lambda: nat.sigmoid_bce(x, lab, 9, gscale, dl, out[0:1], out[1:2], thresh=bad),
                     lambda: nat.sigmoid_bce_f32(x, lab, 9, gscale, dl32, out[0:1], out[1:2], thresh=bad),
                     lambda: nat.eval_metrics(x, lab, 9, 5, out, bce=True, thresh=bad)):
            with pytest.raises(RuntimeError, match="thresh"):
                call()
    assert not bool(out.any()) and not bool(dl.any()) and not bool(dl32.any())


# ------------------------------------------------------------------------------ engines
ENG = dict(loss="bce", label_smoothing=0.1, bce_threshold=0.2)


@pytest.mark.parametrize("which", ["bf16-frozen", "bf16-train", "fp32-frozen", "fp32-train"])
def test_engine_runs_the_bce_heads(which):
    """forward_backward (with a mix table), evaluate and evaluate_topk of each HIP engine against the fp64 definition on
    the engine's own logits, to the scale-1 bounds; HipEngine also against TorchEngine, to the bounds of
    test_gpu_label_smoothing's parity test (loss 3 %, per tensor 15 %, cosine > 0.99)."""
    B, K = 4, 1000
    eng = _hip_engine(which, B, **ENG)
    eng.init(seed=3)
    _spread_dense_bias(eng)
    (img, lab), tab, gscale, flip = _batch(B), _eng_table(B), 1.0 / B, torch.tensor([0, 1, 1, 0], dtype=torch.uint8, device=dev)
    tol_loss, tol_grad, tol_elem = tol(1)
    stats = eng.forward_backward(img, lab, gscale, flip=flip, mix=tab).clone()
    loss, dref, S, hits = bce_ref(eng.logits[:B, :K], lab, gscale, 0.1, 0.2, tab)
    print(f"{which}: loss {stats[0].item():.6f} fp64 {loss:.6f}, correct {stats[1].item()} ({hits})")
    assert abs(stats[0].item() - loss) <= tol_loss * loss and stats[1].item() == hits
    dtype = torch.bfloat16 if which.startswith("bf16") else torch.float32
    _check_dlogits(f"{which} bce head gradient", eng.dlogits[:B, :K], dref, S, dtype, tol_grad, tol_elem)
    assert bool((eng.dlogits[:B, K:] == 0).all())
    if which == "bf16-frozen":
        from pddl.models.reference import TorchEngine
        te = TorchEngine(eng.L, B, crop=224, device="cuda", fused_proj=eng.fuse_proj, **ENG)
        te.params.copy_(eng.params)
        s_t = te.forward_backward(img, lab, gscale, flip=flip, mix=tab)
        assert abs(stats[0].item() - s_t[0].item()) / s_t[0].item() < 0.03
        bad = [(e.name, r) for e in eng.L.entries.values() if e.trainable for r in
               [rel64(eng.grads[e.offset:e.offset + e.size], te.grads[e.offset:e.offset + e.size].double())] if r > 0.15]
        assert not bad and F.cosine_similarity(eng.grads, te.grads, dim=0).item() > 0.99, bad[:10]
    for name in ("evaluate", "evaluate_topk"):
        out = getattr(eng, name)(img, lab).clone()
        want = bce_ref(eng.logits[:B, :K], lab, 0.0, 0.1, 0.2, None)[0]
        assert abs(out[0].item() - want) <= tol_loss * want, f"{which} {name}: {out[0].item()} for {want}"


def test_captured_step_keeps_the_bce_head():
    """A whole-step graph of HipEngine(loss="bce"): the replayed loss is the eager step's from the same parameters
    (1e-3, the bound of tests/test_gpu_capture.py) and the fp64 BCE of the replay's logits."""
    from pddl.train.graph import GraphedTrainStep
    from pddl.train.optim import make_optimizer
    B = CAP_B
    eng = _hip_engine("bf16-frozen", B, graphed=True, **ENG)
    eng.init(seed=13)
    _spread_dense_bias(eng)
    g = torch.Generator().manual_seed(21)
    img = torch.randint(0, 256, (2, B, 224, 224, 3), dtype=torch.uint8, generator=g).cuda()
    lab, flip = torch.randint(0, 1000, (2, B), generator=g).cuda(), torch.zeros(B, dtype=torch.uint8, device=dev)
    gs = GraphedTrainStep(eng, make_optimizer("sgd", eng, lr=1e-3), B, (224, 224), 1.0 / B)
    gs(img[0], lab[0], flip, (0, 0))
    torch.cuda.synchronize()
    assert gs.graph is not None
    start = eng.params.clone()
    l_r = gs(img[1], lab[1], flip, (0, 0))[0].item()
    want = bce_ref(eng.logits[:B, :1000], lab[1], 1.0 / B, 0.1, 0.2, None)[0]
    eng.params.copy_(start)
    eng.after_update()
    l_e = eng.forward_backward(img[1], lab[1], 1.0 / B, flip=flip)[0].item()
    print(f"replay loss {l_r:.6f} eager {l_e:.6f} fp64 of the replay's logits {want:.6f}")
    assert abs(l_r - l_e) <= 1e-3 * abs(l_e) and abs(l_r - want) <= tol(1)[0] * want
