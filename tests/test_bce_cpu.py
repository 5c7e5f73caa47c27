"""--loss bce on the CPU: TorchEngine's head against a hand-written fp64 evaluation of the definition in
csrc/kernels/kernels.h, check_loss's rejections through the CLI, the flag's way to the banner and the records, and the
four HIP engines' schedules under loss="bce" against the bindings' signatures."""
import json
import math

import pytest
import torch

from test_engine_schedule_cpu import ENGINES, Recorder, check_call


def table(rows):
    """rows of (partner, w_lab) -> the int32 [B][8] mix table."""
    t = torch.zeros(len(rows), 8, dtype=torch.int32)
    for b, (p, w) in enumerate(rows):
        t[b, 0] = p
        t[b, 5:7] = torch.tensor([1.0, w]).view(torch.int32)
    return t


def hand64(z, lab, rows, eps, thr):
    """Plain Python doubles: (loss sum, correct, d loss / d logits)."""
    B, K = len(z), len(z[0])
    T = [[(1 - eps) * (j == lab[b]) + eps / K for j in range(K)] for b in range(B)]
    loss, correct, grad = 0.0, 0, []
    for b, (p, w) in enumerate(rows):
        t = [w * T[b][j] + (1 - w) * T[p][j] for j in range(K)]
        t = [float(v > thr) for v in t] if thr is not None else t
        loss += sum(max(v, 0) - tj * v + math.log1p(math.exp(-abs(v))) for v, tj in zip(z[b], t)) / K
        correct += z[b].index(max(z[b])) == (lab[b] if w >= 0.5 else lab[p])
        grad.append([(1 / (1 + math.exp(-v)) - tj) / K for v, tj in zip(z[b], t)])
    return loss, correct, grad


@pytest.mark.parametrize("thr", [None, 0.2])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("mixed", [False, True])
def test_torch_engine_head_against_fp64(mixed, eps, thr):
    """7 fp32 operations per element and a sum of K non-negative terms: (K + 8) U on loss and gradient, the
    gradient in units of (sigmoid + t) / K."""
    from pddl.models.reference import bce_targets, sigmoid_bce_sum
    B, K, U = 4, 11, 2.0 ** -24
    g = torch.Generator().manual_seed(3)
    z = (torch.randn(B, K, generator=g) * 6).requires_grad_(True)
    lab = torch.tensor([3, 0, 10, 3])
    rows = [(1, 0.3), (2, 0.5), (3, 1.0), (0, 0.7)] if mixed else [(b, 1.0) for b in range(B)]   # rows 3 and 0 share a label
    rows = [(p, float(torch.tensor(w, dtype=torch.float32))) for p, w in rows]
    target, counted = bce_targets(lab, table(rows) if mixed else None, K, eps, thr)
    loss = sigmoid_bce_sum(z, target)
    loss.backward()
    want, correct, grad = hand64(z.detach().double().tolist(), lab.tolist(), rows, eps, thr)
    assert abs(loss.item() - want) <= (K + 8) * U * want and int((z.argmax(1) == counted).sum()) == correct
    S = (torch.sigmoid(z.detach().double()) + target.double()) / K
    assert bool(((z.grad.double() - torch.tensor(grad)).abs() <= (K + 8) * U * S).all())


@pytest.mark.parametrize("flags", [["--loss", "hinge"], ["--loss", "bce", "--bce-target-threshold", "1.0"],
                                   ["--loss", "bce", "--bce-target-threshold", "-0.1"], ["--bce-target-threshold", "0.2"]])
def test_check_loss_rejections_exit_2(flags, capsys):
    """(The run is bounded, so a build that does not know the flags trains two tiny steps and returns 0.)"""
    from pddl import cli
    bounded = ["--device", "cpu", "--batch-size", "2", "--crop", "32", "--image-size", "40", "--validation-steps", "1",
               "--no-save", "--max-steps", "2", "--epochs", "1"]
    assert cli.run("single", bounded + flags) == 2 and "--" in capsys.readouterr().err


def test_flag_config_banner_and_records(tmp_path, capsys):
    from pddl import cli
    common = ["--device", "cpu", "--batch-size", "4", "--crop", "32", "--image-size", "40", "--validation-steps", "1",
              "--no-save", "--verbose", "1", "--max-steps", "2", "--epochs", "1", "--mixup", "0.2", "--label-smoothing", "0.1"]
    recs = {}
    for name, flags in (("bce", ["--loss", "bce", "--bce-target-threshold", "0.2"]), ("plain", [])):
        jl = tmp_path / f"{name}.jsonl"
        assert cli.run("single", common + ["--metrics-jsonl", str(jl)] + flags) == 0
        assert ("loss=bce, bce_threshold=0.2" if flags else "loss=crossentropy, bce_threshold=None") in capsys.readouterr().out
        recs[name] = json.loads(jl.read_text().splitlines()[0])
    assert (recs["bce"]["loss_head"], recs["bce"]["bce_threshold"]) == ("bce", 0.2)
    assert (recs["plain"]["loss_head"], recs["plain"]["bce_threshold"]) == ("crossentropy", None)
    assert recs["bce"]["loss"] < 0.5 * recs["plain"]["loss"]       # a mean over 1000 classes against log(1000)


@pytest.mark.parametrize("eng", list(ENGINES))
def test_schedule_binds_under_bce(eng, monkeypatch):
    from pddl.models import engine, engine_bn, engine_f32
    from pddl.models.resnet50 import ParamLayout
    from pddl.ops.native import require_native
    ext = require_native()
    rec = Recorder(ext)
    for mod in (engine, engine_bn, engine_f32):
        monkeypatch.setattr(mod, "require_native", lambda: rec, raising=False)
    e = ENGINES[eng][0](ParamLayout(), 2, crop=64, image_size=64, device="cpu", loss="bce", bce_threshold=0.2)
    e.init(seed=0)
    images, labels = torch.zeros(2, 64, 64, 3, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
    e.forward_backward(images, labels, 0.5)
    e.evaluate(images, labels)
    e.evaluate_topk(images, labels)
    for call in rec.calls:
        check_call(ext, *call)
    heads = [(n, kw) for n, _, kw in rec.calls if n.startswith(("sigmoid_bce", "softmax_xent", "eval_metrics"))]
    assert [n.startswith("sigmoid_bce") for n, _ in heads] == [True, True, False] and heads[2][0] == "eval_metrics"
    assert heads[0][1]["thresh"] == 0.2 and heads[2][1] == {"bce": True, "thresh": 0.2}
