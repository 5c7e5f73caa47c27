"""Mixup / CutMix on the CPU (--mixup, --cutmix, --mix-prob): the draws of `Augment.mix` and the
table they make, TorchEngine against a hand-mixed batch with a soft-target cross-entropy, and the
options' way from the command line to the banner, the JSONL record and the CPU strategies.

A table row is (partner, y0, x0, y1, x1, w_pix bits, w_lab bits, 0): the pixel becomes
w*A_b + (1 - w)*A_partner (w = 0 inside the box, w_pix outside) and the target
w_lab*T(y_b) + (1 - w_lab)*T(y_partner)."""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pddl.utils.envopts import with_opt

SEED = 23


def _cfg(preset, **kw):
    from pddl.config import make_config
    base = dict(device="cpu", data="synthetic", image_size=32, crop=32, flip=False, epochs=1, verbose=0, save=False,
                train_images=64, val_images=8, seed=SEED)
    base.update(kw)
    return make_config(preset, **base)


def _aug(**kw):
    from pddl.parallel.strategies import Augment
    return Augment(_cfg("single", **kw), torch.device("cpu"), SEED)


def _f(col):
    """A float column of a table (stored as its bits)."""
    return col.contiguous().view(torch.float32) if isinstance(col, torch.Tensor) else col.view(np.float32)


# ------------------------------------------------------------------------------ Augment
def test_flip_and_crop_draws_do_not_depend_on_mixing():
    kw = dict(flip=True, image_size=40, crop=32)
    plain, mixed = _aug(**kw), _aug(mixup=0.2, cutmix=1.0, mix_prob=0.5, **kw)
    assert plain.mix(6) is None and not plain.mixing and mixed.mixing
    for _ in range(8):
        (fa, oa), (fb, ob) = plain(6), mixed(6)
        mixed.mix(6)
        assert torch.equal(fa, fb) and oa == ob


def test_cutmix_box_geometry():
    from pddl.train.mix import cutmix_box, cutmix_table, identity_table
    Hc, Wc = 32, 24
    # lambda = 0.75: sides int(32 * 0.5) = 16 and int(24 * 0.5) = 12 around the centre, unclipped
    assert cutmix_box(Hc, Wc, 0.75, 16, 12) == (8, 6, 24, 18, 1.0 - (16 * 12) / (Hc * Wc))
    # clipped at the top-left corner: rows -8..8 -> 0..8, columns -6..6 -> 0..6
    y0, x0, y1, x1, w = cutmix_box(Hc, Wc, 0.75, 0, 0)
    assert (y0, x0, y1, x1) == (0, 0, 8, 6) and w == 1.0 - 48 / (Hc * Wc)
    # clipped at the bottom-right
    y0, x0, y1, x1, w = cutmix_box(Hc, Wc, 0.75, 31, 23)
    assert (y0, x0, y1, x1) == (23, 17, 32, 24) and w == 1.0 - (9 * 7) / (Hc * Wc)
    # lambda = 0: the whole image, the label is the partner's; lambda = 1: a zero-size box
    assert cutmix_box(Hc, Wc, 0.0, 16, 12) == (0, 0, 32, 24, 0.0)
    y0, x0, y1, x1, w = cutmix_box(Hc, Wc, 1.0, 5, 7)
    assert (y1 - y0, x1 - x0, w) == (0, 0, 1.0)
    t = cutmix_table(np.array([1, 0]), (8, 6, 24, 18), 0.75)
    assert t.dtype == np.int32 and t.shape == (2, 8)
    assert t[:, 0].tolist() == [1, 0] and t[0, 1:5].tolist() == [8, 6, 24, 18] and (t[:, 7] == 0).all()
    assert _f(t[:, 5]).tolist() == [1.0, 1.0] and _f(t[:, 6]).tolist() == [0.75, 0.75]
    i = identity_table(3)
    assert i[:, 0].tolist() == [0, 1, 2] and (i[:, 1:5] == 0).all() and (_f(i[:, 5:7]) == 1.0).all()


def test_mixup_and_cutmix_tables_from_augment():
    B = 16
    a = _aug(mixup=0.4)
    for _ in range(4):
        t = a.mix(B)
        assert t.dtype == torch.int32 and tuple(t.shape) == (B, 8)
        assert sorted(t[:, 0].tolist()) == list(range(B))            # partner is a permutation
        assert (t[:, 1:5] == 0).all() and (t[:, 7] == 0).all()        # empty box
        w_pix, w_lab = _f(t[:, 5]), _f(t[:, 6])
        assert torch.equal(w_pix, w_lab) and (w_pix == w_pix[0]).all() and 0.0 <= w_pix[0] <= 1.0
    c = _aug(cutmix=1.0)
    areas = set()
    for _ in range(8):
        t = c.mix(B)
        assert sorted(t[:, 0].tolist()) == list(range(B))
        y0, x0, y1, x1 = t[0, 1:5].tolist()
        assert (t[:, 1:5] == t[0, 1:5]).all()                         # one box per batch
        assert 0 <= y0 <= y1 <= 32 and 0 <= x0 <= x1 <= 32
        assert (_f(t[:, 5]) == 1.0).all()
        want = np.float32(1.0 - (y1 - y0) * (x1 - x0) / (32.0 * 32.0))
        assert (_f(t[:, 6]) == float(want)).all()
        areas.add((y1 - y0) * (x1 - x0))
    assert len(areas) > 1
    # both on: each mixed batch is one of the two kinds
    b = _aug(mixup=0.4, cutmix=1.0)
    kinds = set()
    for _ in range(24):
        t = b.mix(B)
        cut = bool((_f(t[:, 5]) == 1.0).all()) and not bool((t[:, 1:5] == 0).all())
        up = bool((t[:, 1:5] == 0).all()) and torch.equal(_f(t[:, 5]), _f(t[:, 6]))
        assert cut != up or bool((_f(t[:, 6]) == 1.0).all())
        kinds.add("cut" if cut else "up")
    assert kinds == {"cut", "up"}


def test_mix_prob_and_determinism():
    from pddl.train.mix import identity_table
    B = 8
    off = _aug(mixup=0.4, mix_prob=0.0)
    for _ in range(4):
        assert off.mix(B) is None                                     # eager: the unmixed step
        assert torch.equal(off.mix(B, graphed=True), torch.from_numpy(identity_table(B)))
    half = _aug(mixup=0.4, mix_prob=0.5)
    got = [half.mix(B) is None for _ in range(64)]
    assert 8 < sum(got) < 56
    # the same seed draws the same tables, another seed others
    from pddl.parallel.strategies import Augment
    cfg = _cfg("single", mixup=0.4, cutmix=1.0)
    a, b, c = (Augment(cfg, torch.device("cpu"), s) for s in (SEED, SEED, SEED + 1))
    ta, tb, tc = ([x.mix(B) for _ in range(6)] for x in (a, b, c))
    assert all(torch.equal(x, y) for x, y in zip(ta, tb))
    assert not all(torch.equal(x, y) for x, y in zip(ta, tc))


# ------------------------------------------------------------------------------ TorchEngine
def _engine(cap, **kw):
    from pddl.models.reference import TorchEngine
    from pddl.models.resnet50 import ParamLayout
    e = TorchEngine(ParamLayout(), cap, crop=32, **kw)
    e.init(seed=SEED)
    off = e.L.off("dense", "bias")
    g = torch.Generator().manual_seed(SEED)
    e.params[off:off + 1000] = 3 * torch.randn(1000, generator=g)
    return e


def _batch(B, S=32):
    g = torch.Generator().manual_seed(SEED + 1)
    return (torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=g),
            torch.randint(0, 1000, (B,), generator=g))


def _table(rows):
    """rows of (partner, y0, x0, y1, x1, w_pix, w_lab) -> int32 [B][8]."""
    t = np.zeros((len(rows), 8), dtype=np.int32)
    for i, r in enumerate(rows):
        t[i, :5] = r[:5]
        t[i, 5:7] = np.array(r[5:7], dtype=np.float32).view(np.int32)
    return torch.from_numpy(t)


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_torch_engine_matches_hand_mixed_batch(eps):
    """A mixup row, a CutMix row, a row mixed with itself and an identity row: loss, accuracy count
    and flat gradient equal soft-target F.cross_entropy on the batch mixed by hand (slices and
    scalar weights), pushed through the same model."""
    B = 4
    img, lab = _batch(B)
    flip = torch.tensor([0, 1, 0, 1], dtype=torch.uint8)
    rows = [(1, 0, 0, 0, 0, 0.3, 0.3), (2, 4, 6, 20, 30, 1.0, 1.0 - (16 * 24) / 1024.0),
            (2, 0, 0, 0, 0, 0.5, 0.5), (3, 0, 0, 0, 0, 1.0, 1.0)]
    mix = _table(rows)
    e = _engine(B, label_smoothing=eps)
    stats = e.forward_backward(img, lab, 1.0 / B, flip=flip, mix=mix)
    grads = e.grads.clone()
    # by hand
    from pddl.models.reference import preprocess
    x = preprocess(img, 32, True, flip, (0, 0))
    hand = x.clone()
    hand[0] = 0.3 * x[0] + (1.0 - 0.3) * x[1]
    hand[1, :, 4:20, 6:30] = x[2, :, 4:20, 6:30]
    T = F.one_hot(lab, 1000).float() * (1.0 - eps) + eps / 1000
    tgt = T.clone()
    tgt[0] = 0.3 * T[0] + (1.0 - 0.3) * T[1]
    w1 = float(np.float32(rows[1][6]))
    tgt[1] = w1 * T[1] + (1.0 - w1) * T[2]
    assert torch.equal(preprocess(img, 32, True, flip, (0, 0), mix), hand)
    p = e.params[: e.L.n_trainable].clone().requires_grad_(True)
    e.model.stats = e.params
    e.model.bind(p)
    logits = e.model.logits(p, hand, training=True)
    logits.retain_grad()
    loss = F.cross_entropy(logits, tgt, reduction="sum")
    (loss / B).backward()
    assert torch.equal(stats[0], loss.detach()) and torch.equal(grads, p.grad)
    # dlogits = (softmax - t) / B
    want = (torch.softmax(logits.detach().double(), 1) - tgt.double()) / B
    assert (logits.grad.double() - want).abs().max().item() < 1e-6
    counted = torch.stack([lab[1], lab[1], lab[2], lab[3]])     # w_lab 0.3 -> partner; 0.5 ties to the own label
    assert stats[1].item() == (logits.argmax(1) == counted).sum().item()
    # mixing is really in there
    plain = _engine(B, label_smoothing=eps).forward_backward(img, lab, 1.0 / B, flip=flip)
    assert abs(plain[0].item() - stats[0].item()) > 1e-3


def test_identity_table_is_the_unmixed_step():
    from pddl.train.mix import identity_table
    B = 4
    img, lab = _batch(B)
    flip = torch.tensor([1, 0, 0, 1], dtype=torch.uint8)
    a, b, c = _engine(B, label_smoothing=0.1), _engine(B, label_smoothing=0.1), _engine(B, label_smoothing=0.1)
    sa = a.forward_backward(img, lab, 1.0 / B, flip=flip)
    sb = b.forward_backward(img, lab, 1.0 / B, flip=flip, mix=None)
    sc = c.forward_backward(img, lab, 1.0 / B, flip=flip, mix=torch.from_numpy(identity_table(B)))
    assert torch.equal(sa, sb) and torch.equal(a.grads, b.grads)
    assert torch.equal(sa, sc) and torch.equal(a.grads, c.grads)


def test_bad_table_is_clamped():
    """Partner and box outside their ranges are clamped (the kernels' rule), never an error."""
    from pddl.models.reference import preprocess
    B = 2
    img, _ = _batch(B)
    x = preprocess(img, 32, True)
    got = preprocess(img, 32, True, None, (0, 0), _table([(7, -5, -5, 99, 99, 1.0, 1.0), (-3, 30, 30, 40, 40, 1.0, 1.0)]))
    assert torch.equal(got[0], x[1])
    want = x[1].clone()
    want[:, 30:, 30:] = x[0][:, 30:, 30:]
    assert torch.equal(got[1], want)


# ------------------------------------------------------------------------------ configuration
def test_flags_and_errors(capsys):
    from pddl import cli
    from pddl.config import check_mix, config_from_args
    cfg = config_from_args("single", ["--mixup", "0.2", "--cutmix", "1.0", "--mix-prob", "0.5"])
    assert (cfg.mixup, cfg.cutmix, cfg.mix_prob) == (0.2, 1.0, 0.5)
    cfg = config_from_args("single", [])
    assert (cfg.mixup, cfg.cutmix, cfg.mix_prob) == (0.0, 0.0, 1.0)
    for flag, bad in (("--mixup", "-0.1"), ("--cutmix", "nan"), ("--mix-prob", "1.5"), ("--mix-prob", "-0.5"),
                      ("--mixup", "nan"), ("--cutmix", "-1")):
        for preset in ("single", "horovod", "ps"):
            assert cli.run(preset, ["--device", "cpu", flag, bad]) == 2
            err = capsys.readouterr().err
            assert flag in err and len(err.strip().splitlines()) == 1
    from pddl.parallel import parameter_server
    from pddl.parallel.strategies import make_strategy
    with pytest.raises(ValueError, match="--mixup"):
        make_strategy(_cfg("single", batch_size=2, mixup=-1.0))
    with pytest.raises(ValueError, match="--mix-prob"):
        parameter_server.run_ps_job(_cfg("ps", mixup=0.2, mix_prob=2.0))
    check_mix(_cfg("single", mixup=0.0, cutmix=0.0, mix_prob=0.0))


def test_banner_summary_and_jsonl_record(tmp_path, capsys):
    from pddl import cli
    common = ["--device", "cpu", "--batch-size", "4", "--crop", "32", "--image-size", "32", "--validation-steps", "1",
              "--no-save", "--verbose", "1", "--max-steps", "2", "--epochs", "1"]
    recs = {}
    for name, flags in (("mix", ["--mixup", "0.2", "--cutmix", "1", "--mix-prob", "1"]), ("plain", [])):
        jl = tmp_path / f"{name}.jsonl"
        assert cli.run("single", common + ["--metrics-jsonl", str(jl)] + flags) == 0
        out = capsys.readouterr().out
        if flags:
            assert "mixup=0.2, cutmix=1, mix_prob=1" in out and "batch_mix (MixUp / CutMix, p=1)" in out
        else:
            assert "mixup=0, cutmix=0, mix_prob=1" in out and "batch_mix" not in out
        recs[name] = [json.loads(x) for x in jl.read_text().splitlines()]
    r = recs["mix"][0]
    assert (r["mixup"], r["cutmix"], r["mix_prob"]) == (0.2, 1.0, 1.0) and math.isfinite(r["loss"])
    assert (recs["plain"][0]["mixup"], recs["plain"][0]["cutmix"]) == (0.0, 0.0)
    # same seed, same data: the training loss is the mixed one, validation never mixes
    assert r["loss"] != recs["plain"][0]["loss"]


def test_two_cpu_mirrored_replicas_mix(monkeypatch):
    from pddl.parallel.strategies import make_strategy
    from pddl.train.trainer import Trainer
    monkeypatch.setenv("PDDL_CPU_REPLICAS", "2")
    cfg = _cfg("mirrored", max_steps=2, batch_size=4, mixup=0.2, cutmix=1.0)
    st = make_strategy(cfg)
    tr = Trainer(cfg, st)
    seen = []
    for r, (eng, _) in enumerate(st.mirror.replicas):
        fb = eng.forward_backward
        eng.forward_backward = (lambda *a, _fb=fb, _r=r, **k: (seen.append((_r, k.get("mix"))), _fb(*a, **k))[1])
    hist = tr.fit(1, [], validation=False)
    assert math.isfinite(hist.history["loss"][0])
    assert len(seen) == 4 and all(m is not None and tuple(m.shape) == (4, 8) for _, m in seen)
    # each replica mixes within its own batch, with its own draws
    assert all(sorted(m[:, 0].tolist()) == [0, 1, 2, 3] for _, m in seen)
    r0 = [m for r, m in seen if r == 0]
    r1 = [m for r, m in seen if r == 1]
    assert not all(torch.equal(a, b) for a, b in zip(r0, r1))
    (e0, _), (e1, _) = st.mirror.replicas
    assert torch.equal(e0.params, e1.params)


def test_native_cpu_ps_job_mixes(monkeypatch):
    from pddl.parallel.parameter_server import run_ps_job
    monkeypatch.setenv("PDDL_PS", with_opt("PDDL_PS", "impl", "native"))
    monkeypatch.setenv("PDDL_PS", with_opt("PDDL_PS", "heartbeat", "600"))
    cfg = _cfg("ps", steps_per_epoch=2, validation_steps=1, batch_size=4, epochs=1, mixup=0.2, cutmix=1.0)
    res = run_ps_job(cfg, num_ps=1, num_workers=1, return_results=True)
    wk = [r for r in res if r[0] == "worker"]
    ps = [r for r in res if r[0] == "ps"]
    assert len(wk) == 1 and wk[0][2] == 2 and ps[0][2] == 2
    assert math.isfinite(wk[0][3][0]["loss"])
