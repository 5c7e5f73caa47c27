"""LAMB (`--optimizer adam --layer-adapt`) on CPU: the torch-op form of the update against an independent
float64 loop, the unchanged default Adam, the CLI rejections and the checkpoint round trip."""
import math

import numpy as np
import pytest
import torch

LR, B1, B2, EPS, WD, GS = 1e-3, 0.9, 0.999, 1e-6, 0.01, 0.5


def _engine(seed=3):
    from pddl.models.reference import TorchEngine
    from pddl.models.resnet50 import ParamLayout
    e = TorchEngine(ParamLayout(), 1, crop=32)
    e.init(seed=seed)
    return e


def _opt(e, layer_adapt=True, wd=WD):
    from pddl.train.optim import make_optimizer
    opt = make_optimizer("adam", e, lr=LR, beta1=B1, beta2=B2, eps=EPS, weight_decay=wd, layer_adapt=layer_adapt)
    opt.gscale = GS
    return opt


def _steps(e, opt, k, seed):
    """k optimizer steps on seeded gradients -> the gradients, in float64."""
    gen, n, gs = torch.Generator().manual_seed(seed), e.L.n_trainable, []
    for _ in range(k):
        e.grads[:n] = torch.randn(n, generator=gen) * 1e-2
        gs.append(e.grads[:n].double().numpy().copy())
        opt.step()
    return gs


def test_lamb_matches_float64_per_segment():
    """Three steps on the real layout.  p, m, v to atol 1e-6 (all below 8: a few fp32 roundings of half an ulp
    each per step); ratios to rtol 1e-5 (the bound of test_lars_cpu.py for the same fp32 sums)."""
    from pddl.train.optim import lars_segments
    e = _engine()
    n = e.L.n_trainable
    segs = lars_segments(e.L)
    end = segs[-1][0] + segs[-1][1]
    e.params[end:n] = 7.0                      # sentinel in the padding: no segment owns it
    p, m, v = e.params[:n].double().numpy().copy(), np.zeros(n), np.zeros(n)
    opt = _opt(e)
    assert type(opt).__name__ == "LAMB" and len(opt.trust_ratios()) == 54 and end < n
    for t, g in enumerate(_steps(e, opt, 3, 17), start=1):
        ratios = []
        for off, size, adapt, _ in segs:
            sl = slice(off, off + size)
            gg = GS * g[sl]
            m[sl] = B1 * m[sl] + (1 - B1) * gg
            v[sl] = B2 * v[sl] + (1 - B2) * gg * gg
            u = (m[sl] / (1 - B1 ** t)) / (np.sqrt(v[sl] / (1 - B2 ** t)) + EPS) + (WD * p[sl] if adapt else 0.0)
            ratios.append(math.sqrt((p[sl] ** 2).sum() / (u * u).sum()) if adapt else 1.0)
            p[sl] -= LR * ratios[-1] * u
    assert opt.iterations == 3
    for x, x64 in ((e.params, p), (opt.m, m), (opt.v, v)):
        assert np.abs(x[:end].double().numpy() - x64[:end]).max() <= 1e-6
    assert np.allclose(opt.ratios.double().numpy(), ratios, rtol=1e-5, atol=0)
    assert all((r == 1.0) == (not s[2]) for r, s in zip(opt.ratios.tolist(), segs))
    assert (e.params[end:n] == 7.0).all() and (opt.m[end:n] == 0).all() and (opt.v[end:n] == 0).all()


def test_default_adam_is_unchanged_and_ignores_weight_decay():
    (ea, oa), (eb, ob) = ((e, _opt(e, layer_adapt=False, wd=wd)) for e, wd in ((_engine(), 0.0), (_engine(), WD)))
    assert type(oa).__name__ == type(ob).__name__ == "Adam"
    p0 = ea.params[:ea.L.n_trainable].double().numpy().copy()
    (g,) = _steps(ea, oa, 1, 4)
    _steps(eb, ob, 1, 4)
    assert torch.equal(ea.params, eb.params)
    gg = GS * g                                # one epsilon-hat step from zero slots
    want = p0 - LR * math.sqrt(1 - B2) / (1 - B1) * ((1 - B1) * gg) / (np.sqrt((1 - B2) * gg * gg) + EPS)
    assert np.abs(ea.params[:len(p0)].double().numpy() - want).max() <= 1e-6


@pytest.mark.parametrize("preset,argv,msg", [("single", ["--optimizer", "sgd"], "--layer-adapt needs --optimizer adam"),
                                             ("ps", [], "--layer-adapt is not supported for --strategy ps")])
def test_cli_rejects_layer_adapt(preset, argv, msg, capsys):
    from pddl import cli
    from pddl.config import config_from_args
    argv = ["--device", "cpu", "--layer-adapt", "--epochs", "1", "--max-steps", "1", "--no-save"] + argv
    assert config_from_args(preset, argv).layer_adapt is True      # (an unknown flag would be ignored and the job run)
    assert cli.run(preset, argv) == 2
    assert msg in capsys.readouterr().err


def test_lamb_checkpoint_resume_round_trip(tmp_path):
    import json
    from pddl.config import make_config
    from pddl.parallel.strategies import make_strategy
    from pddl.train.trainer import Trainer
    from pddl.utils.checkpoint import h5, save_keras_h5
    e = _engine()
    opt = _opt(e)
    _steps(e, opt, 2, 2)
    path = str(tmp_path / "lamb.h5")
    cfg = make_config("single", device="cpu", optimizer="adam", layer_adapt=True, crop=32, image_size=32, batch_size=1)
    save_keras_h5(path, e, opt, cfg)
    oc = json.loads(h5().read_attr(path, "", "training_config"))["optimizer_config"]
    assert oc == {"class_name": "LAMB", "config": {"name": "LAMB", "learning_rate": LR, "beta_1": B1, "beta_2": B2,
                                                   "epsilon": EPS, "weight_decay": WD}}
    names = h5().read_attr(path, "optimizer_weights", "weight_names")
    assert names[0] == "LAMB/iter:0" and "LAMB/dense/kernel/m:0" in names and "LAMB/dense/kernel/v:0" in names
    st = make_strategy(cfg.replace(resume=path))
    Trainer(cfg, st)
    end = max(x.offset + x.size for x in e.L.entries.values() if x.trainable)
    assert type(st.opt).__name__ == "LAMB" and st.opt.iterations == 2 and opt.v.abs().max() > 0
    assert torch.equal(st.opt.m[:end], opt.m[:end]) and torch.equal(st.opt.v[:end], opt.v[:end])
    assert torch.equal(st.engine.params[:end], e.params[:end])
