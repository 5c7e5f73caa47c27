"""RandAugment on the CPU (--randaugment N M): the draws of train/randaug.py (a row is the box, the Q16 map, the
colour chain), `aug_resample` on maps whose picture is a permutation of the source, and the option's way from the
command line through a two-step Trainer run."""
import json

import numpy as np
import pytest
import torch

SEED, ONE = 23, 1 << 16


def _aug(seed=SEED, **kw):
    from pddl.config import make_config
    from pddl.parallel.strategies import Augment
    return Augment(make_config("single", device="cpu", image_size=40, crop=32, flip=True, mixup=0.2, cutmix=1.0, **kw),
                   torch.device("cpu"), seed)


def test_magnitude_zero_draws_identity_rows():
    from pddl.train.randaug import RandAugSampler, crop_boxes, widen
    boxes = crop_boxes(64, (3, 5), 32)
    t = RandAugSampler((4, 0), 32, SEED).draw(boxes)
    assert t.dtype == np.int32 and t.shape == (64, 16) and (t == widen(boxes)).all() and (t[:, 10] == 0).all()


@pytest.mark.parametrize("sign", [1, -1])
def test_every_parameter_is_within_its_range(sign):
    from pddl.train.randaug import OPS, build_table, crop_boxes
    op = np.arange(len(OPS)).reshape(-1, 1)
    for M in (9, 30):
        m, t = M / 30, build_table(crop_boxes(len(OPS), (0, 0), 224), op, np.full_like(op, sign), M, 224)
        q, par = t[:, 4:10].astype(np.int64), t[:, 11].copy().view(np.float32)
        ident = np.array([ONE, 0, 0, 0, ONE, 0])
        want = {n: ident.copy() for n in OPS}
        want["shear_x"][1] = want["shear_y"][3] = round(sign * 0.3 * m * ONE)
        want["translate_x"][2] = want["translate_y"][5] = round(sign * 2 * 150 / 331 * 224 * m * ONE)
        c, s = np.cos(np.radians(30 * m)), sign * np.sin(np.radians(30 * m))
        want["rotate"] = np.rint(np.array([c, s, 0, -s, c, 0]) * ONE).astype(np.int64)
        for k, n in enumerate(OPS):
            assert (q[k] == want[n]).all() and (t[k, 10] >> 16) == (0 < k < 6), n
        assert np.abs(q[:, [0, 1, 3, 4]]).max() <= ONE and np.abs(q[:, [2, 5]]).max() <= 2 * 150 / 331 * 224 * ONE + 1
        f = np.float32(1 + sign * 0.9 * m)
        bits = 8 - round(4 * m)
        assert (t[6:, 10] == [1, 2, 3, 5, 4]).all() and (par[6:9] == f).all() and 0.1 <= f <= 1.9 + 1e-6
        assert par[9] == 256 - (1 << (8 - bits)) and 4 <= bits <= 8 and par[10] == np.float32(255 * (1 - m)) and (t[:6, 10] & 0xFFFF == 0).all()


def test_sampler_leaves_the_other_draws_alone_and_widens_the_table():
    plain, aug, both, again = _aug(rrc=True), _aug(randaugment=(2, 9)), _aug(rrc=True, randaugment=(2, 9)), _aug(randaugment=(2, 9))
    assert (plain.table_cols, aug.table_cols, both.table_cols, _aug().table_cols) == (4, 16, 16, 0)
    for _ in range(4):
        (fa, _), (fb, ob), (fc, _), _ = plain(6), aug(6), both(6), again(6)
        ta, tb, tc = plain.rrc(6), aug.rrc(6), both.rrc(6)
        assert torch.equal(fa, fb) and torch.equal(fa, fc) and torch.equal(plain.mix(6), both.mix(6))
        assert tuple(tb.shape) == (6, 16) and torch.equal(tc[:, :4], ta) and torch.equal(tb, again.rrc(6))
        assert tb[:, :4].tolist() == [[ob[0], ob[1], 32, 32]] * 6 and torch.equal(tb[:, 4:], tc[:, 4:])
    assert bool((tb[:, 10] != 0).any())


def test_aug_resample_permutes_the_source_on_quarter_turns_and_whole_pixel_shifts():
    from pddl.models.reference import aug_resample, rrc_resample
    mats = [(0, 1, 0, -1, 0, 0), (0, -1, 0, 1, 0, 0), (-1, 0, 0, 0, -1, 0), (1, 0, 5, 0, 1, -3)]
    img = torch.randint(0, 256, (4, 37, 37, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(SEED))
    t = torch.zeros(4, 16, dtype=torch.int32)
    t[:, :4] = torch.tensor([5, 7, 24, 24])
    t[:, 4:10], t[:, 10] = torch.tensor(mats) * torch.tensor([ONE, ONE, 2 * ONE] * 2), ONE
    flip = torch.tensor([0, 1, 0, 1], dtype=torch.uint8)
    x = aug_resample(img, t, 24, 24, flip).permute(0, 2, 3, 1)
    f = img[:, 5:29, 7:31].float() * (1.0 / 255.0)
    fl = lambda a: a.flip(1)                                                    # noqa: E731 (the flip comes first)
    assert torch.equal(x[0], f[0].transpose(0, 1).flip(1)) and torch.equal(x[1], fl(f[1]).transpose(0, 1).flip(0))
    assert torch.equal(x[2], f[2].flip(0).flip(1))
    want = torch.full((24, 24, 3), 128.0 / 255.0)
    want[3:, :19] = fl(f[3])[:21, 5:]
    assert torch.equal(x[3], want)
    t[:, 10] = 0                                                                # no map: the box picture
    assert torch.equal(aug_resample(img, t, 24, 24, flip), rrc_resample(img, t[:, :4], 24, 24, flip))


def test_flag_parsing_errors_and_a_two_step_run(tmp_path, capsys):
    from pddl import cli
    from pddl.config import check_randaug, config_from_args, make_config
    assert tuple(config_from_args("single", ["--randaugment", "2", "9"]).randaugment) == (2, 9)
    for bad in ((0, 9), (5, 9), (2, -1), (2, 31), (2.0, 9)):
        with pytest.raises(ValueError, match="--randaugment"):
            check_randaug(make_config("single", randaugment=bad))
    assert cli.run("single", ["--device", "cpu", "--randaugment", "2", "9", "--antialias"]) == 2
    assert "--antialias" in capsys.readouterr().err
    common = ["--device", "cpu", "--batch-size", "4", "--crop", "32", "--image-size", "40", "--validation-steps", "1",
              "--no-save", "--verbose", "1", "--max-steps", "2", "--epochs", "1"]
    loss = {}
    for name, flags in (("aug", ["--randaugment", "2", "9"]), ("plain", [])):
        jl = tmp_path / f"{name}.jsonl"
        assert cli.run("single", common + ["--metrics-jsonl", str(jl)] + flags) == 0
        assert f"randaugment={'(2, 9)' if flags else None}" in capsys.readouterr().out
        loss[name] = json.loads(jl.read_text().splitlines()[0])["loss"]
    assert np.isfinite(loss["aug"]) and loss["aug"] != loss["plain"]
