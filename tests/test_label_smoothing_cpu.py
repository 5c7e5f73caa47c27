"""Label smoothing on the CPU (--label-smoothing): TorchEngine against a hand-written fp64 target
formula, and the option's way from the command line to the engine, the banner and the JSONL log.

The target is t_j = (1 - eps) * [j == y] + eps / K and the loss logsumexp(z) - sum_j t_j z_j
(Keras CategoricalCrossentropy(label_smoothing=eps))."""
import json

import pytest
import torch

SEED = 11


def _cfg(preset, **kw):
    from pddl.config import make_config
    base = dict(device="cpu", data="synthetic", image_size=32, crop=32, flip=False, epochs=1, verbose=0, save=False,
                train_images=64, val_images=8, seed=SEED)
    base.update(kw)
    return make_config(preset, **base)


def _engine(cap, **kw):
    from pddl.models.reference import TorchEngine
    from pddl.models.resnet50 import ParamLayout
    e = TorchEngine(ParamLayout(), cap, crop=32, **kw)
    e.init(seed=SEED)
    # spread the logits, so that the smoothing term is far above rounding
    off = e.L.off("dense", "bias")
    g = torch.Generator().manual_seed(SEED)
    e.params[off:off + 1000] = 3 * torch.randn(1000, generator=g)
    return e


def _batch(B):
    g = torch.Generator().manual_seed(SEED + 1)
    return (torch.randint(0, 256, (B, 32, 32, 3), dtype=torch.uint8, generator=g),
            torch.randint(0, 1000, (B,), generator=g))


def _smoothed_loss_sum(logits, lab, eps):
    """sum over the batch of logsumexp(z) - sum_j t_j z_j, in the dtype of `logits`."""
    K = logits.shape[1]
    t = torch.full_like(logits, eps / K)
    t[torch.arange(len(lab)), lab] += 1.0 - eps
    return (torch.logsumexp(logits, 1) - (t * logits).sum(1)).sum()


@pytest.mark.parametrize("eps", [0.1, 1.0])
def test_torch_engine_matches_fp64_target_formula(eps):
    """Loss and flat gradient of TorchEngine(label_smoothing=eps) equal the fp64 formula pushed
    through autograd (from the engine's own fp32 logits on), to 1e-5."""
    from pddl.models.reference import preprocess
    B = 4
    img, lab = _batch(B)
    e = _engine(B, label_smoothing=eps)
    assert e.label_smoothing == eps
    stats = e.forward_backward(img, lab, 1.0 / B)
    # the same forward with the loss written out in fp64
    p = e.params[: e.L.n_trainable].clone().requires_grad_(True)
    e.model.stats = e.params
    e.model.bind(p)
    logits = e.model.logits(p, preprocess(img, 32, True, None, (0, 0)), training=True)
    loss = _smoothed_loss_sum(logits.double(), lab, eps)
    (loss / B).backward()
    rel = abs(stats[0].item() - loss.item()) / loss.item()
    gerr = ((e.grads.double() - p.grad.double()).norm() / p.grad.double().norm()).item()
    print(f"eps {eps}: loss {stats[0].item():.6f} fp64 {loss.item():.6f} rel {rel:.2e}; gradient rel {gerr:.2e}")
    assert rel < 1e-5 and gerr < 1e-5
    # and the option is really in there: the plain cross-entropy of these logits is elsewhere
    plain = _smoothed_loss_sum(logits.detach().double(), lab, 0.0).item()
    assert abs(plain - loss.item()) / loss.item() > 1e-3
    # evaluate / evaluate_topk report the smoothed loss of the eval-mode logits
    with torch.no_grad():
        ev = e.model.logits(e.params, preprocess(img, 32, False), training=False)
    want = _smoothed_loss_sum(ev.double(), lab, eps).item()
    assert abs(e.evaluate(img, lab)[0].item() - want) / want < 1e-5
    assert abs(e.evaluate_topk(img, lab)[0].item() - want) / want < 1e-5


def test_torch_engine_eps0_is_the_default():
    B = 4
    img, lab = _batch(B)
    a, b = _engine(B), _engine(B, label_smoothing=0.0)
    assert a.label_smoothing == 0.0
    sa, sb = a.forward_backward(img, lab, 1.0 / B), b.forward_backward(img, lab, 1.0 / B)
    assert torch.equal(sa, sb) and torch.equal(a.grads, b.grads)
    assert torch.equal(a.evaluate_topk(img, lab), b.evaluate_topk(img, lab))
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="label_smoothing"):
            _engine(B, label_smoothing=bad)


def test_config_and_cli(capsys, monkeypatch):
    from pddl import cli
    from pddl.config import config_from_args
    from pddl.parallel.strategies import build_engine, make_strategy
    assert config_from_args("single", ["--label-smoothing", "0.1"]).label_smoothing == 0.1
    assert config_from_args("single", []).label_smoothing == 0.0
    for preset in ("single", "mirrored", "multiworker", "horovod", "ps"):
        cfg = config_from_args(preset, ["--device", "cpu", "--label-smoothing", "0.25", "--crop", "32"])
        assert cfg.label_smoothing == 0.25
        assert build_engine(cfg, torch.device("cpu"), 2).label_smoothing == 0.25
    assert build_engine(_cfg("single"), torch.device("cpu"), 2).label_smoothing == 0.0
    # outside [0, 1]: a configuration error before anything is built; the entry scripts exit 2
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="--label-smoothing"):
            make_strategy(_cfg("single", batch_size=2, label_smoothing=bad))
        for preset in ("single", "horovod", "ps"):
            assert cli.run(preset, ["--device", "cpu", "--label-smoothing", str(bad)]) == 2
            err = capsys.readouterr().err
            assert "--label-smoothing" in err and len(err.strip().splitlines()) == 1
    from pddl.parallel import parameter_server
    with pytest.raises(ValueError, match="--label-smoothing"):
        parameter_server.run_ps_job(_cfg("ps", label_smoothing=1.5))
    # the PS preset takes the flag: cli.run hands the job a configuration that carries it
    got = []
    monkeypatch.setattr(parameter_server, "run_ps_job", lambda cfg: got.append(cfg) or 0)
    assert cli.run("ps", ["--device", "cpu", "--label-smoothing", "0.1"]) == 0
    assert [c.label_smoothing for c in got] == [0.1]
    for edge in ("0", "1"):
        assert cli.run("ps", ["--device", "cpu", "--label-smoothing", edge]) == 0


def test_banner_and_jsonl_record(tmp_path, capsys):
    """Two CPU steps of the single-GPU script: the banner and the per-epoch record carry the
    value, the --evaluate record too, and the losses are those of the smoothed target."""
    from pddl import cli
    common = ["--device", "cpu", "--batch-size", "2", "--crop", "32", "--image-size", "32", "--validation-steps", "1",
              "--no-save", "--verbose", "0", "--max-steps", "2", "--epochs", "1"]
    recs = {}
    for eps in ("0.1", "0"):
        jl = tmp_path / f"m{eps}.jsonl"
        flag = ["--label-smoothing", eps] if eps != "0" else []
        assert cli.run("single", common + ["--metrics-jsonl", str(jl)] + flag) == 0
        out = capsys.readouterr().out
        assert f"label_smoothing={eps}" in out
        recs[eps] = [json.loads(x) for x in jl.read_text().splitlines()]
        assert len(recs[eps]) == 1 and recs[eps][0]["label_smoothing"] == float(eps)
    # same seed, same data: the first run's losses are the smoothed ones
    assert recs["0.1"][0]["loss"] != recs["0"][0]["loss"]
    assert recs["0.1"][0]["val_loss"] != recs["0"][0]["val_loss"]
    jl = tmp_path / "e.jsonl"
    assert cli.run("single", common + ["--evaluate", "--label-smoothing", "0.1", "--metrics-jsonl", str(jl)]) == 0
    rec = json.loads(jl.read_text().splitlines()[-1])
    assert rec["evaluate"] is True and rec["label_smoothing"] == 0.1
