"""Evaluation on the GPU: the eval_metrics head kernel against torch and against softmax_xent,
`evaluate_topk` of the HIP engines against `evaluate`, and the per-replica fan-out of the
in-process replica strategies (two replicas sharing the GPU in a rehearsal, eager steps) through
`eval_step`, `Trainer.fit`'s validation and `Trainer.evaluate`.

Shapes: 64-pixel images, 8 per replica (tests/test_gpu_multirank.py)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B, S = 8, 64
dev = "cuda"


def N():
    from pddl.ops.native import require_native
    return require_native()


def _ref(logits, labels, k):
    """[loss sum, top-1 hits, top-k hits] in torch: rank = #{j : l[j] > l[label] or (l[j] == l[label] and j < label)}."""
    vl = logits.gather(1, labels[:, None])
    idx = torch.arange(logits.shape[1], device=logits.device)[None, :]
    rank = ((logits > vl) | ((logits == vl) & (idx < labels[:, None]))).sum(1)
    return F.cross_entropy(logits, labels, reduction="sum").item(), (rank == 0).sum().item(), (rank < k).sum().item()


def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("nb,ncls,ldl,k", [(37, 1000, 1024, 5), (1, 1000, 1024, 5), (37, 1000, 1000, 5),
                                           (37, 10, 10, 5), (37, 3, 3, 5), (37, 3, 8, 1)])
def test_eval_metrics_kernel(nb, ncls, ldl, k):
    """Loss sum within rel 1e-5 of F.cross_entropy (the bound of test_colsum_softmax_xent for the same
    sum), both counts exactly the rank reference's; +inf in the pad columns of a row (ldl > ncls)
    reaches no output; loss and top-1 agree with softmax_xent on the same logits; a second launch
    into the same `out` doubles it (the kernel accumulates)."""
    torch.manual_seed(7)
    buf = torch.full((nb, ldl), float("inf"), device=dev)
    buf[:, :ncls] = torch.randn(nb, ncls, device=dev) * 3
    lab = torch.randint(0, ncls, (nb,), device=dev)
    out = torch.zeros(3, device=dev)
    N().eval_metrics(buf, lab, ncls, k, out)
    got = out.tolist()
    loss, top1, topk = _ref(buf[:, :ncls], lab, k)
    print(f"eval_metrics {got} reference {(loss, top1, topk)} loss rel {_rel(got[0], loss):.2e}")
    assert got[1] == top1 and got[2] == topk
    assert _rel(got[0], loss) < 1e-5
    if k >= ncls:
        assert got[2] == nb
    ldd = (ncls + 63) // 64 * 64
    dl = torch.empty(nb, ldd, dtype=torch.bfloat16, device=dev)
    ls, cr = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    N().softmax_xent(buf, lab, ncls, 1.0 / nb, dl, ls, cr)
    print(f"softmax_xent loss {ls.item()} correct {cr.item()} loss rel {_rel(got[0], ls.item()):.2e}")
    assert got[1] == cr.item() and _rel(got[0], ls.item()) < 1e-5
    N().eval_metrics(buf, lab, ncls, k, out)
    twice = out.tolist()
    assert twice[1] == 2 * got[1] and twice[2] == 2 * got[2] and _rel(twice[0], 2 * got[0]) < 1e-6


def test_eval_metrics_kernel_ties():
    """The hand-built tie rows of tests/test_eval_cpu.py: equal logits are ordered by index."""
    from test_eval_cpu import tie_rows
    logits, labels, want = tie_rows()
    logits, labels = logits.to(dev), labels.to(dev)
    for i, (t1, t5) in enumerate(want):
        out = torch.zeros(3, device=dev)
        N().eval_metrics(logits[i:i + 1], labels[i:i + 1], 10, 5, out)
        assert out.tolist()[1:] == [t1, t5], (i, out)
        assert _rel(out[0].item(), F.cross_entropy(logits[i:i + 1], labels[i:i + 1]).item()) < 1e-5
    out = torch.zeros(3, device=dev)
    N().eval_metrics(logits, labels, 10, 10, out)        # k >= ncls: always a hit
    assert out.tolist()[1:] == [1, 4]
    ls, cr = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    N().softmax_xent(logits, labels, 10, 1.0, torch.empty(4, 64, dtype=torch.bfloat16, device=dev), ls, cr)
    assert cr.item() == 1
    for bad in ((logits, labels, 10, 0, out), (logits[:, :8], labels, 10, 5, out)):   # k < 1; row shorter than ncls
        with pytest.raises(RuntimeError):
            N().eval_metrics(*bad)


def _data(n=2 * B):
    g = torch.Generator().manual_seed(1234)
    img = torch.randint(0, 256, (n, S, S, 3), dtype=torch.uint8, generator=g)
    lab = torch.randint(0, 1000, (n,), generator=g)
    return img.to(dev), lab.to(dev)


@pytest.mark.parametrize("kind", ["bf16", "f32", "bf16-bn"])
def test_engine_evaluate_topk_matches_evaluate(kind):
    from pddl.models.engine import HipEngine
    from pddl.models.engine_bn import HipEngineBNTrain
    from pddl.models.engine_f32 import HipF32Engine
    from pddl.models.resnet50 import ParamLayout
    from pddl.train.optim import make_optimizer
    L = ParamLayout()
    if kind == "bf16-bn":
        eng = HipEngineBNTrain(L, B, bn_mode="train", crop=S, image_size=S)
    else:
        eng = {"bf16": HipEngine, "f32": HipF32Engine}[kind](L, B, crop=S, image_size=S)
    eng.init(seed=0)
    img, lab = _data(B)
    if kind == "bf16-bn":       # one training step first: the moving statistics and the weights have moved
        opt = make_optimizer("adam", eng, lr=1e-3)
        eng.forward_backward(img, lab, 1.0 / B)
        opt.step()
        eng.after_update()
    ws = eng.ws.clone()
    t = eng.evaluate_topk(img, lab).clone()
    assert torch.equal(eng.ws, ws)            # the per-step workspace (the 2-float stats in it) is untouched
    e = eng.evaluate(img, lab).clone()
    print(kind, "evaluate_topk", t.tolist(), "evaluate", e.tolist())
    assert t.shape == (3,) and e.shape == (2,)
    assert t[1].item() == e[1].item() and _rel(t[0].item(), e[0].item()) < 1e-5
    assert t[2].item() >= t[1].item() and torch.isfinite(t).all()
    assert eng.evaluate_topk(img, lab, k=1000)[2].item() == B


def _cfg(strategy, batch):
    from pddl.config import make_config
    return make_config("bench", strategy=strategy, batch_size=batch, crop=S, image_size=S, optimizer="adam", lr=1e-4,
                       device="cuda", graphs=False, flip=False, data="synthetic_fixed", seed=0, bucket_mb=4.0,
                       num_classes=1000)


def _spy(engines):
    """Records (replica index, B) of every evaluate / evaluate_topk call on these engines."""
    calls = []
    for i, eng in enumerate(engines):
        for name in ("evaluate", "evaluate_topk"):
            if not hasattr(eng, name):
                continue

            def spy(images, labels, *a, _orig=getattr(eng, name), _i=i, **k):
                calls.append((_i, images.shape[0]))
                return _orig(images, labels, *a, **k)
            setattr(eng, name, spy)
    return calls


def _direct(engines, img, lab, cuts):
    tot = 0
    for eng, (s, e) in zip(engines, cuts):
        tot = tot + eng.evaluate_topk(img[s:e], lab[s:e]).clone()
    return tot


def _same(got, ref, tol=1e-6):
    assert got[1].item() == ref[1].item() and got[2].item() == ref[2].item(), (got, ref)
    assert _rel(got[0].item(), ref[0].item()) < tol, (got, ref)


from test_eval_cpu import one_process_job  # noqa: E402,F401  (fixture)


@pytest.fixture
def rehearse(monkeypatch):
    monkeypatch.setenv("PDDL_REHEARSE", "1")


def test_two_mirrored_replicas_eval_step(rehearse):
    """eval_step of two Mirrored replicas (sharing the GPU) = the sum of each replica engine's own
    evaluate_topk on its half (same engine, batch and kernel plan: counts exact, loss rel 1e-6);
    within 5e-3 of one engine of capacity 16 on all 16 images (another GEMM tile plan: the bound
    tests/test_gpu_multirank.py uses for the same 2-replicas-vs-1 loss); evaluation between eager
    training steps sees the updated weights; a 13-image batch splits 7 / 6."""
    from pddl.parallel.strategies import MirroredStrategy, make_strategy
    from pddl.train.trainer import Trainer
    cfg = _cfg("mirrored", B)
    st = MirroredStrategy(cfg, devices=[0, 0])
    Trainer(cfg, st)
    st.broadcast_state(None)
    engines = [e for e, _ in st.mirror.replicas]
    img, lab = _data()
    halves = [(0, B), (B, 2 * B)]
    ref = _direct(engines, img, lab, halves)
    calls = _spy(engines)
    got = st.eval_step(img, lab, top5=True)
    torch.cuda.synchronize()
    assert sorted(calls) == [(0, B), (1, B)], calls          # each replica scored its own 8 images
    assert got.shape == (3,) and got.device == engines[0].params.device
    _same(got, ref)
    got2 = st.eval_step(img, lab)
    assert got2.shape == (2,)
    _same(torch.cat([got2, got[2:]]), ref)
    cfg1 = _cfg("single", 2 * B)
    st1 = make_strategy(cfg1)
    Trainer(cfg1, st1)
    one = st1.eval_step(img, lab, top5=True)
    print("2 replicas", got.tolist(), "1 replica of 16", one.tolist())
    assert _rel(got[0].item(), one[0].item()) < 5e-3
    # evaluation interleaved with training steps
    st.train_step(img, lab)
    e1 = st.eval_step(img, lab, top5=True)
    st.train_step(img, lab)
    e2 = st.eval_step(img, lab, top5=True)
    torch.cuda.synchronize()
    assert e1[0].item() != e2[0].item() and e1[0].item() != got[0].item()      # the weights moved
    _same(e2, _direct(engines, img, lab, halves))
    # 13 images: shares 7 and 6
    del calls[:]
    e13 = st.eval_step(img[:13], lab[:13], top5=True)
    assert sorted(calls) == [(0, 7), (1, 6)], calls
    _same(e13, _direct(engines, img, lab, [(0, 7), (7, 13)]))


def _fit_and_evaluate(cfg, st):
    from pddl.train.trainer import Trainer
    tr = Trainer(cfg, st)
    calls = _spy([e for e, _ in st.mirror.replicas])
    h = tr.fit(1, [], steps_per_epoch=2, validation_steps=2).history
    assert sorted(calls) == [(0, B), (0, B), (1, B), (1, B)], calls
    for k in ("val_loss", "val_accuracy"):
        assert len(h[k]) == 1 and h[k][0] == h[k][0] and abs(h[k][0]) != float("inf"), (k, h[k])
    assert h["val_loss"][0] > 0
    m = tr.evaluate(steps=2)
    assert m["images"] == 4 * B and m["top5_accuracy"] >= m["accuracy"]
    assert _rel(m["loss"], h["val_loss"][0]) < 1e-5 and m["accuracy"] == h["val_accuracy"][0]


def test_fit_validates_on_two_mirrored_replicas(rehearse):
    """Trainer.fit through the end-of-epoch validation on two replicas: each replica gets its 8 of
    the 16-image validation batch (one engine of capacity 8 cannot take the 16)."""
    from pddl.parallel.strategies import MirroredStrategy
    cfg = _cfg("mirrored", B)
    _fit_and_evaluate(cfg, MirroredStrategy(cfg, devices=[0, 0]))


def test_fit_validates_on_two_multiworker_local_replicas(rehearse, one_process_job, monkeypatch):
    """The same through one MultiWorker process driving two local replicas (PDDL_LOCAL_GPUS=2)."""
    from pddl.parallel.strategies import MultiWorkerStrategy
    monkeypatch.setenv("PDDL_LOCAL_GPUS", "2")
    cfg = _cfg("multiworker", B)
    st = MultiWorkerStrategy(cfg)
    st._local_devices = lambda info: [0, 0]      # (both replicas on GPU 0, whatever the machine has)
    _fit_and_evaluate(cfg, st)
