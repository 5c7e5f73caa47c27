"""LARS and the per-step learning-rate schedule on CPU: the torch-op form of the update against
an independent float64 formula, the schedule formula, the callback list, the CLI, checkpoints,
the parameter-server rejection and replica equality."""
import json
import re

import numpy as np
import pytest
import torch

LR, MU, WD, ETA, EPS, GS = 0.05, 0.9, 5e-5, 1e-3, 0.0, 0.5


def _engine(seed=3):
    from pddl.models.reference import TorchEngine
    from pddl.models.resnet50 import ParamLayout
    e = TorchEngine(ParamLayout(), 1, crop=32)
    e.init(seed=seed)
    return e


def _lars(e, **kw):
    from pddl.train.optim import make_optimizer
    args = dict(lr=LR, momentum=MU, weight_decay=WD, lars_eta=ETA, lars_eps=EPS)
    args.update(kw)
    opt = make_optimizer("lars", e, **args)
    opt.gscale = GS
    return opt


def _tail_end(L):
    return max(e.offset + e.size for e in L.entries.values() if e.trainable)


def _ref_step(L, p, v, g, lr):
    """One LARS step in float64, entry by entry: kernels are adapted, everything else is plain
    momentum with no decay."""
    ratios = {}
    for e in L.entries.values():
        if not e.trainable:
            continue
        sl = slice(e.offset, e.offset + e.size)
        w, gg = p[sl], GS * g[sl]
        ratio, wd = 1.0, 0.0
        if e.kind == "kernel":
            wd = WD
            wn, gn = np.sqrt((w * w).sum()), np.sqrt((gg * gg).sum())
            if wn > 0 and gn > 0:
                ratio = ETA * wn / (gn + wd * wn + EPS)
            ratios[e.layer] = ratio
        v[sl] = MU * v[sl] + lr * ratio * (gg + wd * w)
        p[sl] = w - v[sl]
    return ratios


def test_lars_matches_float64_per_entry():
    e = _engine()
    L, n = e.L, e.L.n_trainable
    end = _tail_end(L)
    assert end < n, "the layout has alignment padding after the last trainable entry"
    opt = _lars(e)
    assert type(opt).__name__ == "LARS" and len(opt.trust_ratios()) == 54
    e.params[end:n] = 7.0                      # sentinel in the padding: no segment owns it
    p64 = e.params[:n].double().numpy().copy()
    v64 = np.zeros(n)
    p0 = e.params[:n].clone()
    gen = torch.Generator().manual_seed(17)
    for step in range(3):
        e.grads[:n] = torch.randn(n, generator=gen) * 1e-2
        g = e.grads[:n].clone()
        opt.step()
        ratios = _ref_step(L, p64, v64, g.double().numpy(), LR)
        if step == 0:
            for ent in L.entries.values():
                if ent.trainable and ent.kind != "kernel":
                    sl = slice(ent.offset, ent.offset + ent.size)
                    assert torch.equal(e.params[sl], p0[sl] - LR * (GS * g[sl])), ent.name   # no decay, no ratio
        got = opt.trust_ratios()
        for name, r in ratios.items():
            assert got[name] == pytest.approx(r, rel=1e-5), name
    assert opt.iterations == 3
    assert np.abs(e.params[:end].double().numpy() - p64[:end]).max() <= 1e-6
    assert np.abs(opt.mom[:end].double().numpy() - v64[:end]).max() <= 1e-6
    assert (e.params[end:n] == 7.0).all() and (opt.mom[end:n] == 0).all()     # padding never written


def test_lars_zero_gradient_and_zero_weight_take_ratio_one():
    e = _engine()
    L, n = e.L, e.L.n_trainable
    opt = _lars(e)
    e.grads[:n] = torch.randn(n, generator=torch.Generator().manual_seed(1)) * 1e-2
    zg, zw = L.entry("conv2_block1_1_conv", "kernel"), L.entry("conv3_block1_2_conv", "kernel")
    e.grads[zg.offset:zg.offset + zg.size] = 0
    e.params[zw.offset:zw.offset + zw.size] = 0
    opt.step()
    r = opt.trust_ratios()
    assert r["conv2_block1_1_conv"] == 1.0 and r["conv3_block1_2_conv"] == 1.0
    assert r["dense"] != 1.0
    assert torch.isfinite(e.params[:n]).all() and torch.isfinite(opt.mom).all()
    assert all(np.isfinite(x) and x > 0 for x in r.values())


def test_lars_rejects_nesterov_and_unknown_names():
    from pddl.train.optim import make_optimizer
    e = _engine()
    with pytest.raises(ValueError, match="Nesterov"):
        make_optimizer("lars", e, lr=0.1, nesterov=True)
    with pytest.raises(ValueError):
        make_optimizer("lamb", e, lr=0.1)


def test_schedule_formula_on_the_host():
    from pddl.train.optim import scheduled_lr
    lr, end, wu, tot = 0.8, 1e-4, 5, 25
    f = lambda t: scheduled_lr(lr, t, wu, tot, end)   # noqa: E731
    assert f(1) == pytest.approx(lr / 5)
    assert f(wu) == pytest.approx(lr)
    assert f(wu + 1) == pytest.approx(end + (lr - end) * (19 / 20) ** 2)
    assert f(tot) == end and f(tot + 1) == end and f(10 * tot) == end
    assert f(tot - 1) == pytest.approx(end + (lr - end) * (1 / 20) ** 2)
    assert scheduled_lr(lr, 1, 0, 10, end) == pytest.approx(end + (lr - end) * 0.81)    # no warm-up
    assert all(f(t) > f(t + 1) for t in range(wu, tot))                              # decays monotonically


def test_schedule_drives_every_cpu_optimizer():
    """set_schedule on the base class: SGD and Adam follow it too (LARS is checked end to end)."""
    import math
    from pddl.train.optim import make_optimizer, scheduled_lr
    for name in ("sgd", "adam"):
        e = _engine()
        n = e.L.n_trainable
        opt = make_optimizer(name, e, lr=0.1, momentum=0.0)
        opt.set_schedule(2, 4, 0.01)
        with pytest.raises(ValueError):
            opt.set_schedule(4, 4, 0.01)
        for t in range(1, 6):
            e.grads[:n] = 1.0
            before = e.params[:8].clone()
            opt.step()
            s = scheduled_lr(0.1, t, 2, 4, 0.01)
            if name == "adam":   # constant gradient 1: m = 1 - b1^t, v = 1 - b2^t, so the bias correction cancels
                s *= math.sqrt(1 - 0.999 ** t) / (math.sqrt(1 - 0.999 ** t) + 1e-7)
            assert torch.allclose(before - e.params[:8], torch.full((8,), s), rtol=1e-4, atol=1e-7), (name, t)
        assert opt.current_lr == 0.01


def test_poly_schedule_drops_the_lr_callbacks():
    from pddl.config import make_config
    from pddl.parallel.strategies import make_strategy
    from pddl.train.trainer import default_callbacks
    for lr_schedule, present in (("poly", False), ("plateau", True)):
        cfg = make_config("horovod", device="cpu", lr_schedule=lr_schedule)
        assert cfg.warmup_epochs == 3
        names = [type(c).__name__ for c in default_callbacks(cfg, make_strategy(cfg))]
        assert ("ReduceLROnPlateau" in names) == present
        assert ("LearningRateWarmupCallback" in names) == present
        assert "EarlyStopping" in names


def test_cli_lars_poly_end_to_end(capsys, tmp_path):
    from pddl import cli
    from pddl.train.optim import scheduled_lr
    jl = tmp_path / "m.jsonl"
    rc = cli.run("single", ["--device", "cpu", "--optimizer", "lars", "--weight-decay", "5e-5", "--lr-schedule", "poly",
                            "--warmup-epochs", "1", "--lr", "0.05", "--lr-end", "0.002", "--batch-size", "2",
                            "--crop", "32", "--image-size", "32", "--validation-steps", "1", "--no-save",
                            "--metrics-jsonl", str(jl), "--verbose", "2", "--epochs", "2", "--max-steps", "2"])
    assert rc == 0
    out = capsys.readouterr().out
    assert "optimizer=lars" in out
    lrs = re.findall(r" - lr: (\S+) - ", out)
    # 2 steps per epoch: warm-up ends at step 2, the schedule at step 4; each line shows its last step's rate
    want = [scheduled_lr(0.05, t, 2, 4, 0.002) for t in (2, 4)]
    assert lrs == [f"{w:.4g}" for w in want] == ["0.05", "0.002"]
    recs = [json.loads(x) for x in jl.read_text().splitlines()]
    assert [r["lr"] for r in recs] == want
    assert all(np.isfinite(r["loss"]) for r in recs)


def test_lars_checkpoint_round_trip(tmp_path):
    from pddl.config import make_config
    from pddl.utils.checkpoint import h5, load_checkpoint, save_keras_h5
    e = _engine()
    n = e.L.n_trainable
    opt = _lars(e)
    gen = torch.Generator().manual_seed(2)
    for _ in range(2):
        e.grads[:n] = torch.randn(n, generator=gen) * 1e-2
        opt.step()
    path = str(tmp_path / "lars.h5")
    save_keras_h5(path, e, opt, make_config("single", device="cpu"))
    tc = json.loads(h5().read_attr(path, "", "training_config"))
    assert tc["optimizer_config"]["class_name"] == "LARS"
    assert tc["optimizer_config"]["config"] == {"name": "LARS", "learning_rate": LR, "momentum": MU,
                                                "weight_decay": WD, "eta": ETA, "epsilon": EPS}
    names = h5().read_attr(path, "optimizer_weights", "weight_names")
    assert names[0] == "LARS/iter:0" and "LARS/dense/kernel/momentum:0" in names
    e2 = _engine(seed=9)
    opt2 = _lars(e2)
    load_checkpoint(path, e2, opt2)
    assert opt2.iterations == 2
    for ent in e.L.entries.values():
        sl = slice(ent.offset, ent.offset + ent.size)
        assert torch.equal(e2.params[sl], e.params[sl]), ent.name
        if ent.trainable:
            assert torch.equal(opt2.mom[sl], opt.mom[sl]), ent.name
    assert opt.mom.abs().max() > 0


def test_ps_rejects_lars(capsys):
    from pddl import cli
    assert cli.run("ps", ["--device", "cpu", "--optimizer", "lars"]) == 2
    assert "--optimizer lars is not supported for --strategy ps" in capsys.readouterr().err


def test_cpu_mirrored_replicas_stay_identical_with_lars(monkeypatch):
    from pddl.config import make_config
    from pddl.parallel.strategies import make_strategy
    from pddl.train.trainer import Trainer
    monkeypatch.setenv("PDDL_CPU_REPLICAS", "2")
    cfg = make_config("mirrored", device="cpu", data="synthetic", image_size=32, crop=32, flip=False, epochs=1,
                      max_steps=2, verbose=0, save=False, train_images=64, val_images=8, seed=5, lr=0.05,
                      batch_size=2, optimizer="lars", weight_decay=5e-5, lr_schedule="poly", warmup_epochs=0)
    st = make_strategy(cfg)
    tr = Trainer(cfg, st)
    start = st.mirror.replicas[0][0].params.clone()
    tr.fit(1, [], validation=False)
    (e0, o0), (e1, o1) = st.mirror.replicas
    assert type(o0).__name__ == "LARS" and o0.iterations == 2 and o0.schedule == (0, 2, cfg.lr_end)
    assert torch.equal(e0.params, e1.params) and torch.equal(o0.mom, o1.mom)
    assert not torch.equal(e0.params, start)
