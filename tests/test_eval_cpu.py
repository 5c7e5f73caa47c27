"""Evaluation as a first-class path, on the CPU: the per-replica fan-out of the in-process replica
strategies (every replica scores its own share, within its engine's capacity), the uneven split
and chunking of `_LocalReplicas.evaluate`, the rank definition behind top-1 / top-k
(`TorchEngine.evaluate_topk`, the oracle of the eval_metrics kernel), `Trainer.evaluate`,
`--evaluate`, and the HIP engines' `evaluate_topk` schedule bound to the built extension."""
import json
import os
import re

import pytest
import torch

S = 64


def _cfg(strategy, **kw):
    from pddl.config import make_config
    # (plain SGD: one step moves the weights in proportion to the gradient, so the 2-replica and
    # the 1-replica run differ by the gradients' summation order only; Adam's first step is
    # lr * sign(g) and turns a reassociated ~0 gradient into a 2 * lr difference)
    base = dict(strategy=strategy, device="cpu", image_size=S, crop=S, data="synthetic_fixed", flip=False,
                optimizer="sgd", momentum=0.0, lr=1e-3, seed=3, train_images=8, val_images=8, verbose=0, save=False)
    base.update(kw)
    return make_config("bench", **base)


def _spy(monkeypatch):
    """Records (id(engine), B) of every TorchEngine.evaluate / evaluate_topk call and holds each to
    the engine's capacity."""
    from pddl.models.reference import TorchEngine
    calls = []
    for name in ("evaluate", "evaluate_topk"):
        orig = getattr(TorchEngine, name, None)
        if orig is None:
            continue

        def spy(self, images, labels, *a, _orig=orig, **k):
            B = images.shape[0]
            calls.append((id(self), B))
            assert B <= self.batch, f"replica got {B} images, capacity {self.batch}"
            return _orig(self, images, labels, *a, **k)
        monkeypatch.setattr(TorchEngine, name, spy)
    return calls


def _fit(cfg, st, **kw):
    from pddl.train.trainer import Trainer
    tr = Trainer(cfg, st)
    return tr, tr.fit(1, [], validation=True, **kw)


def test_mirrored_validation_fans_out_within_capacity(monkeypatch):
    """Two Mirrored CPU replicas of batch 2: each validation step hands every replica its 2 images
    (the engine's capacity), and val_loss / val_accuracy equal one replica at batch 4 on the same
    images (fp32 torch, only the summation order differs: rel 1e-5)."""
    from pddl.parallel.strategies import MirroredStrategy, SingleStrategy
    monkeypatch.setenv("PDDL_CPU_REPLICAS", "2")
    calls = _spy(monkeypatch)
    cfg = _cfg("mirrored", batch_size=2)
    st = MirroredStrategy(cfg)
    _, hist = _fit(cfg, st, steps_per_epoch=1, validation_steps=2)
    ids = [id(e) for e, _ in st.mirror.replicas]
    assert calls == [(ids[0], 2), (ids[1], 2)] * 2, calls
    cfg1 = _cfg("single", batch_size=4)
    _, ref = _fit(cfg1, SingleStrategy(cfg1), steps_per_epoch=1, validation_steps=2)
    for k in ("val_loss", "val_accuracy"):
        print(k, hist.history[k][0], ref.history[k][0])
        assert hist.history[k][0] == pytest.approx(ref.history[k][0], rel=1e-5)
    assert sorted(hist.history) == sorted(ref.history) == ["accuracy", "loss", "lr", "val_accuracy", "val_loss"]


@pytest.fixture
def one_process_job():
    """A job of one process, whatever launcher variables the environment holds; the variables the
    strategy exports for torch.distributed (RANK, WORLD_SIZE, ...) do not outlive the test."""
    saved = dict(os.environ)
    for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "OMPI_COMM_WORLD_RANK", "SLURM_PROCID"):
        os.environ.pop(v, None)
    yield
    os.environ.clear()
    os.environ.update(saved)


def test_multiworker_local_replicas_validation_within_capacity(one_process_job, monkeypatch):
    """One MultiWorker process driving 2 local CPU replicas, validation batch 3 per replica: every
    replica scores at most 3 images per validation step."""
    from pddl.parallel.strategies import MultiWorkerStrategy
    monkeypatch.setenv("PDDL_LOCAL_GPUS", "2")
    calls = _spy(monkeypatch)
    cfg = _cfg("multiworker", batch_size=2, val_batch_size=3, val_images=12)
    st = MultiWorkerStrategy(cfg)
    _, hist = _fit(cfg, st, steps_per_epoch=1, validation_steps=2)
    ids = [id(e) for e, _ in st.mirror.replicas]
    assert calls == [(ids[0], 3), (ids[1], 3)] * 2, calls
    assert all(torch.isfinite(torch.tensor(hist.history[k][0])) for k in ("val_loss", "val_accuracy"))


@pytest.fixture(scope="module")
def replicas2():
    """Two CPU replicas of capacity 2 with one set of weights, and 9 images scored one by one."""
    from pddl.parallel.strategies import _LocalReplicas
    lr = _LocalReplicas(_cfg("mirrored", batch_size=2), ["cpu", "cpu"])
    lr.broadcast()
    g = torch.Generator().manual_seed(7)
    img = torch.randint(0, 256, (9, S, S, 3), dtype=torch.uint8, generator=g)
    lab = torch.randint(0, 1000, (9,), generator=g)
    eng = lr.replicas[0][0]
    each = torch.stack([eng.evaluate_topk(img[i:i + 1], lab[i:i + 1]) for i in range(9)]).double()
    return lr, img, lab, each


@pytest.mark.parametrize("n,want", [(5, [(0, 2), (0, 1), (1, 2)]),    # shares 3 and 2, capacity 2
                                    (1, [(0, 1)]),                     # replica 1 has no share: skipped
                                    (9, [(0, 2), (0, 2), (0, 1), (1, 2), (1, 2)]),
                                    (4, [(0, 2), (1, 2)])])
def test_local_replicas_evaluate_split_and_chunks(replicas2, monkeypatch, n, want):
    """Shares differ by at most one image, none is dropped, a share above the capacity goes in
    chunks, and the result is the sum of the per-image results."""
    lr, img, lab, each = replicas2
    calls = _spy(monkeypatch)
    ids = [id(e) for e, _ in lr.replicas]
    got = lr.evaluate(img[:n], lab[:n], top5=True)
    assert [(ids.index(i), b) for i, b in calls] == want
    ref = each[:n].sum(0)
    assert got.shape == (3,) and got[1].item() == ref[1].item() and got[2].item() == ref[2].item()
    assert got[0].item() == pytest.approx(ref[0].item(), rel=1e-5)
    got2 = lr.evaluate(img[:n], lab[:n])
    assert got2.shape == (2,) and got2[1].item() == ref[1].item()
    assert got2[0].item() == pytest.approx(ref[0].item(), rel=1e-5)


def tie_rows():
    """Hand-built logits [4][10], labels, and the expected (top-1 hits, top-5 hits) per row:
    an all-equal row with label 0 / 4 / 5 (rank = label: equal logits are ordered by index), and
    a row whose label ties with five lower-index columns (rank 5)."""
    logits = torch.zeros(4, 10)
    logits[3] = torch.tensor([1., 1., 1., 1., 1., -2., -2., 1., 0.5, -1.])
    labels = torch.tensor([0, 4, 5, 7])
    return logits, labels, [(1, 1), (0, 1), (0, 0), (0, 0)]


def test_torch_engine_evaluate_topk_rank_semantics(monkeypatch):
    import torch.nn.functional as F
    from pddl.models.reference import TorchEngine
    from pddl.models.resnet50 import ParamLayout
    eng = TorchEngine(ParamLayout(10), 4, crop=32, num_classes=10)
    eng.init(seed=0)
    logits, labels, want = tie_rows()
    img = torch.zeros(4, 32, 32, 3, dtype=torch.uint8)
    for i, (t1, t5) in enumerate(want):
        monkeypatch.setattr(eng.model, "logits", lambda p, x, training=True, i=i: logits[i:i + 1])
        out = eng.evaluate_topk(img[:1], labels[i:i + 1])
        assert out.tolist()[1:] == [t1, t5], (i, out)
        assert out[0].item() == pytest.approx(F.cross_entropy(logits[i:i + 1], labels[i:i + 1]).item(), rel=1e-6)
    monkeypatch.setattr(eng.model, "logits", lambda p, x, training=True: logits)
    out = eng.evaluate_topk(img, labels)
    assert out.tolist()[1:] == [1, 2]
    assert eng.evaluate(img, labels).tolist() == out[:2].tolist()      # rank 0 is evaluate's first argmax
    assert eng.evaluate_topk(img, labels, k=10).tolist()[1:] == [1, 4]   # k >= ncls: always a hit
    assert eng.evaluate_topk(img, labels, k=11).tolist()[1:] == [1, 4]
    assert eng.evaluate_topk(img, labels, k=1).tolist()[1:] == [1, 1]


def test_trainer_evaluate_scores_the_ragged_last_batch(monkeypatch):
    """5 validation images on two replicas of batch 2 (batches of 4 and 1): all 5 are scored, and
    the result equals one replica's."""
    from pddl.parallel.strategies import MirroredStrategy, SingleStrategy
    from pddl.train.trainer import Trainer
    monkeypatch.setenv("PDDL_CPU_REPLICAS", "2")
    cfg = _cfg("mirrored", batch_size=2, val_images=5, data="synthetic")
    m = Trainer(cfg, MirroredStrategy(cfg)).evaluate()
    cfg1 = _cfg("single", batch_size=4, val_images=5, data="synthetic")
    r = Trainer(cfg1, SingleStrategy(cfg1)).evaluate()
    assert list(m) == ["loss", "accuracy", "top5_accuracy", "images"] and m["images"] == r["images"] == 5
    for k in ("loss", "accuracy", "top5_accuracy"):
        assert m[k] == pytest.approx(r[k], rel=1e-5)
    assert m["top5_accuracy"] >= m["accuracy"]
    assert list(Trainer(cfg1, SingleStrategy(cfg1)).evaluate(steps=1, top5=False)) == ["loss", "accuracy", "images"]


def test_cli_evaluate(tmp_path, monkeypatch, capsys):
    """--evaluate scores a saved model: the printed metrics are Trainer.evaluate()'s of the trainer
    that saved it, the parameters stay bit-identical, no checkpoint is written; PS refuses."""
    from pddl import cli
    from pddl.parallel.strategies import SingleStrategy
    from pddl.train.trainer import Trainer
    monkeypatch.chdir(tmp_path)
    cfg = _cfg("single", batch_size=2, image_size=32, crop=32, data="synthetic", train_images=4, num_classes=1000)
    tr = Trainer(cfg, SingleStrategy(cfg))
    tr.fit(1, [], validation=False, steps_per_epoch=2)
    path = str(tmp_path / "model.h5")
    tr.save(path)
    want = tr.evaluate(steps=3)
    seen = {}
    orig = Trainer.evaluate

    def spy(self, *a, **k):
        seen["trainer"], seen["before"] = self, self.strategy.engine.params.clone()
        return orig(self, *a, **k)
    monkeypatch.setattr(Trainer, "evaluate", spy)
    capsys.readouterr()
    jl = str(tmp_path / "m.jsonl")
    rc = cli.run("single", ["--device", "cpu", "--evaluate", "--weights", path, "--data", "synthetic", "--image-size",
                            "32", "--crop", "32", "--batch-size", "2", "--seed", "3", "--validation-steps", "3",
                            "--metrics-jsonl", jl])
    assert rc == 0
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("evaluate - ")]
    assert len(line) == 1, line
    m = re.match(r"evaluate - loss: (\S+) - accuracy: (\S+) - top5_accuracy: (\S+) - (\d+) images - (\S+) img/s$", line[0])
    assert m, line[0]
    assert [m.group(1), m.group(2), m.group(3)] == [f"{want[k]:.4f}" for k in ("loss", "accuracy", "top5_accuracy")]
    assert int(m.group(4)) == want["images"] == 6
    rec = [json.loads(ln) for ln in open(jl)]
    assert len(rec) == 1 and rec[0]["images"] == 6
    for k in ("loss", "accuracy", "top5_accuracy"):
        assert rec[0][k] == pytest.approx(want[k], rel=1e-6)
    after = seen["trainer"].strategy.engine.params
    assert torch.equal(after, seen["before"]) and torch.equal(after, tr.strategy.engine.params)
    assert sorted(os.listdir(tmp_path)) == ["m.jsonl", "model.h5"]          # nothing saved
    assert cli.run("ps", ["--device", "cpu", "--evaluate", "--weights", path]) == 2
    assert "--evaluate is not supported for --strategy ps" in capsys.readouterr().err


@pytest.mark.parametrize("eng", ["bf16", "bf16-bn", "f32", "f32-bn"])
def test_evaluate_topk_schedule_binds(eng, monkeypatch):
    """evaluate_topk of each HIP engine on CPU tensors against the recording stand-in of the
    native module (tests/test_engine_schedule_cpu.py): every call, eval_metrics among them, binds
    to the signature the built extension publishes."""
    from test_engine_schedule_cpu import ENGINES, Recorder, check_call
    from pddl.models import engine, engine_bn, engine_f32
    from pddl.models.resnet50 import ParamLayout
    from pddl.ops.native import require_native
    ext = require_native()
    rec = Recorder(ext)
    for mod in (engine, engine_bn, engine_f32):
        monkeypatch.setattr(mod, "require_native", lambda: rec, raising=False)
    monkeypatch.setenv("PDDL_ENGINE", "")
    cls, conv = ENGINES[eng]
    B = 2
    e = cls(ParamLayout(), B, crop=S, image_size=S, device="cpu")
    e.init(seed=0)
    ws = e.ws.data_ptr(), e.ws.numel()
    rec.calls.clear()
    out = e.evaluate_topk(torch.zeros(B, S, S, 3, dtype=torch.uint8), torch.zeros(B, dtype=torch.int64), k=5)
    assert out is e.eval_stats and out.shape == (3,)
    assert not (ws[0] <= out.data_ptr() < ws[0] + 4 * ws[1])       # its own buffer, outside the workspace
    names = [n for n, _, _ in rec.calls]
    assert conv in names and names.count("eval_metrics") == 1 and names[-1] == "eval_metrics", names[-3:]
    assert "softmax_xent" not in names and "softmax_xent_f32" not in names
    for call in rec.calls:
        check_call(ext, *call)
    _, args, kwargs = rec.calls[-1]
    assert not kwargs and args[0].shape[0] == B and args[2] == 1000 and args[3] == 5 and args[4] is e.eval_stats
