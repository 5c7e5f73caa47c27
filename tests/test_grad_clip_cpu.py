"""Global-norm gradient clipping and the non-finite skip on the CPU (--global-clipnorm,
--skip-nonfinite): the torch-op branches of the three optimizers against hand-written float64
formulas, the unclipped step bitwise against the optimizer without the option, the skip, the
configuration checks, the CLI, the epoch logs and replica equality.

scale = clip / norm when norm > clip else 1 (Keras: clip / max(norm, clip)), norm the L2 norm of
gscale * g over the whole trainable buffer; weight decay is added after the clipped gradient."""
import json
import math

import numpy as np
import pytest
import torch

LR, MU, WD, GS = 0.05, 0.9, 5e-5, 0.5
B1, B2, EPS = 0.9, 0.999, 1e-7


class _FlatEngine:
    """The flat buffers an optimizer needs, with the real layout."""

    def __init__(self, seed):
        from pddl.models.resnet50 import ParamLayout
        self.L = ParamLayout()
        g = torch.Generator().manual_seed(seed)
        self.params = torch.randn(self.L.total, generator=g) * 0.05
        self.grads = torch.randn(self.L.n_trainable, generator=g) * 1e-2


def _opt(name, e, **kw):
    from pddl.train.optim import make_optimizer
    opt = make_optimizer(name, e, lr=LR, momentum=MU, weight_decay=WD, beta1=B1, beta2=B2, eps=EPS, **kw)
    opt.gscale = GS
    return opt


def _norm64(g):
    return math.sqrt(float(((GS * g.double()) ** 2).sum()))


def _ref(name, L, p, slots, g, scale, t, nesterov=False):
    """One float64 step of `name` on numpy arrays, the gradient being GS * scale * g."""
    gg = GS * scale * g
    if name == "adam":
        m, v = slots
        lr_t = LR * math.sqrt(1 - B2 ** t) / (1 - B1 ** t)
        m[:] = B1 * m + (1 - B1) * gg
        v[:] = B2 * v + (1 - B2) * gg * gg
        p -= lr_t * m / (np.sqrt(v) + EPS)
    elif name == "sgd":
        (v,) = slots
        gr = gg + WD * p
        v[:] = MU * v - LR * gr
        p += (MU * v - LR * gr) if nesterov else v
    else:
        (v,) = slots
        for e in L.entries.values():
            if not e.trainable:
                continue
            sl = slice(e.offset, e.offset + e.size)
            w, ge = p[sl], gg[sl]
            ratio, wd = 1.0, 0.0
            if e.kind == "kernel":
                wd = WD
                wn, gn = np.sqrt((w * w).sum()), np.sqrt((ge * ge).sum())
                if wn > 0 and gn > 0:
                    ratio = 1e-3 * wn / (gn + wd * wn)
            v[sl] = MU * v[sl] + LR * ratio * (ge + wd * w)
            p[sl] = w - v[sl]


def _slots(opt):
    return list(opt.state_tensors().values())


def _end(L):
    return max(e.offset + e.size for e in L.entries.values() if e.trainable)


@pytest.mark.parametrize("name,nesterov", [("adam", False), ("sgd", False), ("sgd", True), ("lars", False)])
def test_cpu_branch_matches_float64(name, nesterov):
    """Two steps: the first clipped to half its norm, the second under a threshold above its norm."""
    e = _FlatEngine(3)
    n, end = e.L.n_trainable, _end(e.L)
    e.grads[end:] = 0                      # (the padding carries no gradient; LARS owns no segment there)
    kw = dict(nesterov=True) if nesterov else {}
    n1 = _norm64(e.grads)
    opt = _opt(name, e, global_clipnorm=n1 / 2, **kw)
    assert opt.clip_active and opt.global_clipnorm == n1 / 2 and not opt.skip_nonfinite
    p64 = e.params[:n].double().numpy().copy()
    s64 = [np.zeros(n) for _ in _slots(opt)]
    for t, clip in ((1, n1 / 2), (2, 4 * n1)):
        opt.set_grad_clip(clip)
        g = e.grads.clone()
        opt.step()
        st = opt.clip_stats()
        scale = clip / n1 if n1 > clip else 1.0
        assert st["norm"] == pytest.approx(n1, rel=1e-9) and st["scale"] == pytest.approx(scale, rel=1e-9)
        assert st["clipped"] == 1 and st["skipped"] == 0
        _ref(name, e.L, p64, s64, g.double().numpy(), scale, t, nesterov)
        got = e.params[:n].double().numpy()
        assert np.allclose(got[:end], p64[:end], rtol=1e-5, atol=1e-6), np.abs(got[:end] - p64[:end]).max()
        for s, r in zip(_slots(opt), s64):
            assert np.allclose(s.double().numpy()[:end], r[:end], rtol=1e-5, atol=1e-6)
    assert opt.iterations == 2
    opt.reset_clip_counters()
    assert opt.clip_stats()["clipped"] == 0


@pytest.mark.parametrize("name", ["adam", "sgd", "lars"])
def test_unclipped_step_is_bitwise_the_plain_step(name):
    a, b, c = _FlatEngine(5), _FlatEngine(5), _FlatEngine(5)
    oa = _opt(name, a)
    ob = _opt(name, b, global_clipnorm=10 * _norm64(b.grads))
    oc = _opt(name, c, skip_nonfinite=True)       # measure only
    assert oa.gn is None and oa.gn_partials is None and oa.clip_stats() is None and not oa.clip_active
    for _ in range(2):
        oa.step(), ob.step(), oc.step()
    for o, e in ((ob, b), (oc, c)):
        assert torch.equal(a.params, e.params)
        for x, y in zip(_slots(oa), _slots(o)):
            assert torch.equal(x, y)
        st = o.clip_stats()
        assert st["scale"] == 1.0 and st["clipped"] == 0 and st["norm"] == pytest.approx(_norm64(e.grads), rel=1e-9)
    # turning both off drops the buffers again
    ob.set_grad_clip()
    assert ob.gn is None and not ob.clip_active


@pytest.mark.parametrize("name", ["adam", "sgd", "lars"])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_skip_leaves_state_untouched_and_counts_the_step(name, bad):
    e = _FlatEngine(7)
    opt = _opt(name, e, global_clipnorm=1.0, skip_nonfinite=True)
    opt.step()
    p0, s0 = e.params.clone(), [s.clone() for s in _slots(opt)]
    r0 = opt.ratios.clone() if name == "lars" else None
    good = e.grads.clone()
    e.grads[12345] = bad
    opt.step()
    st = opt.clip_stats()
    assert opt.iterations == 2 and st["skipped"] == 1 and not math.isfinite(st["norm"])
    assert torch.equal(e.params, p0) and all(torch.equal(x, y) for x, y in zip(_slots(opt), s0))
    if r0 is not None:
        assert torch.equal(opt.ratios, r0)
    e.grads.copy_(good)
    opt.step()
    st = opt.clip_stats()
    assert opt.iterations == 3 and st["skipped"] == 1 and math.isfinite(st["norm"])
    assert not torch.equal(e.params, p0) and torch.isfinite(e.params).all()
    # without the switch the step is taken (and poisons the parameters, as before)
    e2 = _FlatEngine(7)
    o2 = _opt(name, e2, global_clipnorm=1.0)
    e2.grads[12345] = bad
    o2.step()
    assert o2.clip_stats()["skipped"] == 0 and not torch.isfinite(e2.params).all()


def _cfg(preset, **kw):
    from pddl.config import make_config
    base = dict(device="cpu", data="synthetic", image_size=32, crop=32, flip=False, epochs=1, verbose=0, save=False,
                train_images=64, val_images=8, seed=5)
    base.update(kw)
    return make_config(preset, **base)


def test_check_clip_and_cli(capsys):
    from pddl import cli
    from pddl.config import check_clip, config_from_args
    from pddl.parallel import parameter_server
    from pddl.parallel.strategies import make_strategy
    from pddl.train.optim import make_optimizer
    check_clip(_cfg("single"))
    check_clip(_cfg("single", global_clipnorm=1.5, skip_nonfinite=True))
    check_clip(_cfg("ps"))
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), True):
        with pytest.raises(ValueError, match="--global-clipnorm"):
            check_clip(_cfg("single").replace(global_clipnorm=bad))
        with pytest.raises(ValueError, match="global_clipnorm"):
            make_optimizer("sgd", _FlatEngine(1), lr=LR, global_clipnorm=bad)
    with pytest.raises(ValueError, match="--global-clipnorm"):
        make_strategy(_cfg("single", batch_size=2).replace(global_clipnorm=-2.0))
    for kw in (dict(global_clipnorm=1.0), dict(skip_nonfinite=True)):
        with pytest.raises(ValueError, match="no process holds a whole gradient"):
            check_clip(_cfg("ps", **kw))
        with pytest.raises(ValueError, match="--strategy ps"):
            parameter_server.run_ps_job(_cfg("ps", **kw))
    # the flags
    cfg = config_from_args("horovod", ["--device", "cpu", "--global-clipnorm", "2.5", "--skip-nonfinite"])
    assert cfg.global_clipnorm == 2.5 and cfg.skip_nonfinite is True
    cfg = config_from_args("horovod", ["--device", "cpu"])
    assert cfg.global_clipnorm is None and cfg.skip_nonfinite is False
    for argv in (["--global-clipnorm", "0"], ["--global-clipnorm", "-3"], ["--global-clipnorm", "nan"]):
        assert cli.run("single", ["--device", "cpu"] + argv) == 2
        err = capsys.readouterr().err
        assert "--global-clipnorm" in err and len(err.strip().splitlines()) == 1
    for argv in (["--global-clipnorm", "1"], ["--skip-nonfinite"]):
        assert cli.run("ps", ["--device", "cpu"] + argv) == 2
        err = capsys.readouterr().err
        assert "--strategy ps" in err and "whole gradient" in err and len(err.strip().splitlines()) == 1


def test_fit_logs_and_banner(tmp_path, capsys):
    """Two CPU steps of the single-GPU script: with the flags the banner shows them and the
    epoch's JSONL record carries grad_norm / clipped_steps / skipped_steps; without, none."""
    from pddl import cli
    common = ["--device", "cpu", "--batch-size", "2", "--crop", "32", "--image-size", "32", "--validation-steps", "1",
              "--no-save", "--verbose", "0", "--max-steps", "2", "--epochs", "1", "--optimizer", "sgd"]
    keys = {"grad_norm", "clipped_steps", "skipped_steps"}
    jl = tmp_path / "on.jsonl"
    flags = ["--global-clipnorm", "1e-3", "--skip-nonfinite"]
    assert cli.run("single", common + flags + ["--metrics-jsonl", str(jl)]) == 0
    out = capsys.readouterr().out
    assert "global_clipnorm=0.001" in out and "skip_nonfinite=True" in out
    (rec,) = [json.loads(x) for x in jl.read_text().splitlines()]
    assert keys <= set(rec)
    assert rec["grad_norm"] > 1e-3 and math.isfinite(rec["grad_norm"])     # (a fresh ResNet's gradient is far above)
    assert rec["clipped_steps"] == 2 and rec["skipped_steps"] == 0
    jl = tmp_path / "off.jsonl"
    assert cli.run("single", common + ["--metrics-jsonl", str(jl)]) == 0
    out = capsys.readouterr().out
    assert "global_clipnorm=None" in out and "skip_nonfinite=False" in out
    (rec,) = [json.loads(x) for x in jl.read_text().splitlines()]
    assert not keys & set(rec)


def test_two_cpu_mirrored_replicas_end_equal(monkeypatch):
    from pddl.parallel.strategies import make_strategy
    from pddl.train.trainer import Trainer
    monkeypatch.setenv("PDDL_CPU_REPLICAS", "2")
    cfg = _cfg("mirrored", max_steps=2, batch_size=2, optimizer="adam", lr=1e-3, global_clipnorm=1e-3,
               skip_nonfinite=True)
    st = make_strategy(cfg)
    tr = Trainer(cfg, st)
    start = st.mirror.replicas[0][0].params.clone()
    hist = tr.fit(1, [], validation=False)
    (e0, o0), (e1, o1) = st.mirror.replicas
    assert o0.iterations == 2 and o0.global_clipnorm == 1e-3 and o1.skip_nonfinite
    assert torch.equal(e0.params, e1.params) and torch.equal(o0.m, o1.m) and torch.equal(o0.v, o1.v)
    assert o0.clip_stats() == o1.clip_stats() and o0.clip_stats()["clipped"] == 2
    assert not torch.equal(e0.params, start)
    assert hist.history["clipped_steps"] == [2] and hist.history["skipped_steps"] == [0]
