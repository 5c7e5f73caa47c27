"""Random-resized-crop on the CPU (--rrc): the draws of `Augment.rrc` (a row is y0, x0, h, w), TorchEngine
against a batch resampled by hand, and the options' way from the command line to banner and JSONL record."""
import json

import numpy as np
import torch

SEED = 23


def test_boxes_follow_the_inception_draw_and_leave_the_other_draws_alone():
    from pddl.config import make_config
    from pddl.parallel.strategies import Augment
    from pddl.train.rrc import RrcSampler, fallback_box
    _aug = lambda seed=SEED, **kw: Augment(make_config("single", device="cpu", image_size=40, crop=32, flip=True, mixup=0.2,  # noqa: E731
                                                        cutmix=1.0, **kw), torch.device("cpu"), seed)
    H, W, scale, ratio = 40, 56, (0.08, 1.0), (3 / 4, 4 / 3)
    s = RrcSampler(True, scale, ratio, H, W, SEED)
    t = np.concatenate([s.draw(64) for _ in range(8)])
    assert t.dtype == np.int32 and t.shape == (512, 4)
    y0, x0, h, w = t.astype(np.int64).T
    assert (t[:, :2] >= 0).all() and (t[:, 2:] >= 1).all() and (y0 + h <= H).all() and (x0 + w <= W).all()
    # h and w are rounded to whole pixels, so the drawn (real) sides lie within half a pixel of them
    fb = (t == np.array(fallback_box(H, W, ratio))).all(1)
    ok = (((w - .5) * (h - .5) <= scale[1] * H * W) & ((w + .5) * (h + .5) >= scale[0] * H * W) &
          ((w - .5) / (h + .5) <= ratio[1]) & ((w + .5) / (h - .5) >= ratio[0]))
    assert (ok | fb).all() and len(set(map(tuple, t))) > 400 and y0.min() == 0 and (y0 + h).max() == H
    # no try can fit: every box is the centred fallback, itself within the ratio bounds
    tall = RrcSampler(True, (0.9, 1.0), (3.0, 4.0), 40, 20, SEED).draw(5)
    assert (tall == np.array([16, 0, 7, 20])).all() and fallback_box(20, 80, (0.5, 2.0)) == (0, 20, 20, 40)
    # the same seed draws the same tables, another seed others; flip and mix draws do not change
    plain, boxed, again = _aug(), _aug(rrc=True), _aug(rrc=True)
    assert plain.rrc(6) is None
    for _ in range(8):
        (fa, oa), (fb, ob) = plain(6), boxed(6)
        ta, tb = boxed.rrc(6), again.rrc(6)
        assert torch.equal(fa, fb) and torch.equal(plain.mix(6), boxed.mix(6))
        assert ob == (0, 0) and 0 <= min(oa) and max(oa) <= 8           # --rrc: no RandomCrop offset
        assert ta.dtype == torch.int32 and tuple(ta.shape) == (6, 4) and torch.equal(ta, tb)
    assert not torch.equal(_aug(SEED + 1, rrc=True).rrc(6), _aug(rrc=True).rrc(6))


def test_torch_engine_matches_hand_resampled_batch():
    """A 16 x 16 box to 32 x 32 (2x up), the whole image, a 1 x 1 box, a flipped 2x-up box; then the step equals
    the plain step on that batch (pixels multiples of 16: the resampled batch is whole numbers, so exists as uint8)."""
    from pddl.models.reference import TorchEngine, preprocess
    from pddl.models.resnet50 import ParamLayout
    g = torch.Generator().manual_seed(SEED)
    img, lab = (torch.randint(0, 16, (4, 32, 32, 3), generator=g) * 16).to(torch.uint8), torch.randint(0, 1000, (4,), generator=g)
    flip = torch.tensor([0, 0, 0, 1], dtype=torch.uint8)
    rrc = torch.tensor([[8, 4, 16, 16], [0, 0, 32, 32], [5, 9, 1, 1], [8, 4, 16, 16]], dtype=torch.int32)
    x = preprocess(img, 32, True, flip, (0, 0), None, rrc)
    f = img.float() * (1.0 / 255.0)
    up = f[0, 8:24, 4:20]                                              # 2x up: taps k-1, k at 1/4 and 3/4
    pad = torch.cat([up[:1], up, up[-1:]], 0)
    rows = torch.stack([0.25 * pad[:-2] + 0.75 * pad[1:-1], 0.75 * pad[1:-1] + 0.25 * pad[2:]], 1).reshape(32, 16, 3)
    pad = torch.cat([rows[:, :1], rows, rows[:, -1:]], 1)
    want0 = torch.stack([0.25 * pad[:, :-2] + 0.75 * pad[:, 1:-1], 0.75 * pad[:, 1:-1] + 0.25 * pad[:, 2:]], 2).reshape(32, 32, 3)
    assert torch.allclose(x[0].permute(1, 2, 0), want0, atol=1e-6)
    assert torch.equal(x[1], f[1].permute(2, 0, 1)) and torch.equal(x[2], f[2, 5, 9].view(3, 1, 1).expand(3, 32, 32))
    assert torch.equal(x[3], preprocess(img[3:], 32, True, None, (0, 0), None, rrc[3:])[0].flip(-1))
    e, plain = (TorchEngine(ParamLayout(), 4, crop=32) for _ in range(2))
    for eng in (e, plain):      # (Dense bias 3 randn: the logits spread, so loss and gradient are far above rounding)
        eng.init(seed=SEED)
        off = eng.L.off("dense", "bias")
        eng.params[off:off + 1000] = 3 * torch.randn(1000, generator=torch.Generator().manual_seed(SEED))
    s = e.forward_backward(img, lab, 0.25, flip=flip, rrc=rrc)
    hand = (x * 255.0).round().permute(0, 2, 3, 1).contiguous()
    assert torch.equal(preprocess(hand.to(torch.uint8), 32, True), x)
    s0 = plain.forward_backward(hand.to(torch.uint8), lab, 0.25)
    assert abs(s[0].item() - s0[0].item()) <= 1e-5 * abs(s0[0].item())
    assert ((e.grads - plain.grads).norm() / plain.grads.norm()).item() < 1e-4


def test_flags_banner_record_and_errors(tmp_path, capsys):
    from pddl import cli
    from pddl.config import config_from_args
    cfg = config_from_args("single", ["--rrc", "--rrc-scale", "0.25", "1", "--rrc-ratio", "0.5", "2"])
    assert cfg.rrc is True and tuple(cfg.rrc_scale) == (0.25, 1.0) and tuple(cfg.rrc_ratio) == (0.5, 2.0)
    for flag, bad in (("--rrc-scale", ("0.5", "0.25")), ("--rrc-scale", ("0", "1")), ("--rrc-scale", ("0.5", "1.5")),
                      ("--rrc-ratio", ("2", "1")), ("--rrc-ratio", ("-1", "1")), ("--rrc-ratio", ("nan", "1"))):
        for preset in ("single", "horovod", "ps"):
            assert cli.run(preset, ["--device", "cpu", "--rrc", flag, *bad]) == 2
            assert flag in (err := capsys.readouterr().err) and len(err.strip().splitlines()) == 1
    common = ["--device", "cpu", "--batch-size", "4", "--crop", "32", "--image-size", "40", "--validation-steps", "1",
              "--no-save", "--verbose", "1", "--max-steps", "2", "--epochs", "1"]
    recs = {}
    for name, flags in (("rrc", ["--rrc", "--rrc-scale", "0.25", "1"]), ("plain", [])):
        jl = tmp_path / f"{name}.jsonl"
        assert cli.run("single", common + ["--metrics-jsonl", str(jl)] + flags) == 0
        out = capsys.readouterr().out
        assert f"rrc={bool(flags)}, rrc_scale={'0.25' if flags else '0.08'}-1, rrc_ratio=0.75-1.33333" in out
        assert ("RandomResizedCrop 32x32" in out) == bool(flags)
        recs[name] = json.loads(jl.read_text().splitlines()[0])
    r = recs["rrc"]
    assert (r["rrc"], r["rrc_scale"], r["rrc_ratio"]) == (True, [0.25, 1.0], [3 / 4, 4 / 3]) and np.isfinite(r["loss"])
    assert recs["plain"]["rrc"] is False and r["loss"] != recs["plain"]["loss"]
