"""The forward's boundary launches under PDDL_ENGINE c3c1 = 2 (the default), 1 and 0, recorded on the
CPU (see test_engine_schedule_cpu): 2 fuses conv3 + the next conv1 at the plain stride-1
boundaries of stage 2 (one, 64 wide) and stage 3 (two, 128 wide), and the two stage-3 blocks whose
conv1 ran inside the launch get no conv1 igemm of their own; 1 is stage 2 only; the train-BN engine
never takes the path."""
import pytest
import torch

from pddl.models import engine, engine_bn, engine_f32
from pddl.models.resnet50 import ParamLayout
from pddl.ops.native import require_native
from test_engine_schedule_cpu import Recorder, check_call, signature


def _record(cls, spec, monkeypatch):
    ext = require_native()
    rec = Recorder(ext)
    for mod in (engine, engine_bn, engine_f32):
        monkeypatch.setattr(mod, "require_native", lambda: rec, raising=False)
    monkeypatch.setenv("PDDL_ENGINE", spec)
    B, size = 2, 64
    e = cls(ParamLayout(), B, crop=size, image_size=size, device="cpu")
    e.init(seed=0)
    e.forward_backward(torch.zeros(B, size, size, 3, dtype=torch.uint8), torch.zeros(B, dtype=torch.int64), 1.0 / B)
    for call in rec.calls:
        check_call(ext, *call)      # every recorded call binds to the published signature
    return e, [(name, signature(getattr(ext, name)).bind(*args, **kwargs).arguments) for name, args, kwargs in rec.calls]


def _c3c1(calls):
    return [a for name, a in calls if name == "c3c1"]


def _conv1_igemms(e, calls, block):
    """Forward igemm launches that write `block`'s conv1 output."""
    y1 = e.acts[block]["y1"]
    return [a for name, a in calls if name == "igemm" and a["out"].data_ptr() == y1.data_ptr()]


@pytest.mark.parametrize("spec", ["", "c3c1=2"])
def test_stage3_boundaries_fused(monkeypatch, spec):
    e, calls = _record(engine.HipEngine, spec, monkeypatch)
    assert e.c3c1 == 2
    cc = _c3c1(calls)
    assert sorted(a["a"].shape[-1] for a in cc) == [64, 128, 128]
    for a in cc:
        f = a["a"].shape[-1]
        M = a["a"].numel() // f
        assert tuple(a["w3"].shape) == (4 * f, f) and tuple(a["w1"].shape) == (f, 4 * f)
        assert a["res"] is not None and a["res"].numel() == M * 4 * f
        assert a["out"].numel() == M * 4 * f and a["y1"].numel() == M * f
        assert a["bits3"].numel() == M * f // 2 and a["bits1"].numel() == M * f // 8
    wide = [a for a in cc if a["a"].shape[-1] == 128]
    blocks = {b.name: b for b in e.L.blocks}
    assert {a["y1"].data_ptr() for a in wide} == {e.acts[n]["y1"].data_ptr() for n in ("conv3_block3", "conv3_block4")}
    assert {a["out"].data_ptr() for a in wide} == {e.acts[n]["out"].data_ptr() for n in ("conv3_block2", "conv3_block3")}
    assert blocks["conv3_block3"].filters == 128
    for name in ("conv3_block3", "conv3_block4", "conv2_block3"):
        assert not _conv1_igemms(e, calls, name), name
    for name in ("conv3_block1", "conv3_block2", "conv4_block1", "conv4_block2"):
        assert len(_conv1_igemms(e, calls, name)) == 1, name


def test_stage2_only(monkeypatch):
    e, calls = _record(engine.HipEngine, "c3c1=1", monkeypatch)
    assert e.c3c1 == 1
    cc = _c3c1(calls)
    assert len(cc) == 1 and cc[0]["a"].shape[-1] == 64
    for name in ("conv3_block3", "conv3_block4"):
        assert len(_conv1_igemms(e, calls, name)) == 1, name


def test_off(monkeypatch):
    e, calls = _record(engine.HipEngine, "c3c1=0", monkeypatch)
    assert e.c3c1 == 0 and not _c3c1(calls)
    for name in ("conv2_block3", "conv3_block3", "conv3_block4"):
        assert len(_conv1_igemms(e, calls, name)) == 1, name


def test_train_bn_engine_never_takes_it(monkeypatch):
    e, calls = _record(engine_bn.HipEngineBNTrain, "c3c1=2", monkeypatch)
    assert e.c3c1 == 0 and not _c3c1(calls)
