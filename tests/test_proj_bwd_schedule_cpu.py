"""The launch schedule of conv2_block1's backward with PDDL_ENGINE proj_bwd on and off, recorded on
the CPU (see test_engine_schedule_cpu): on, one bwd1x1 launch carries the shortcut conv's
operands and no 64-wide weight gradient takes a second gradient; off, the three launches of
before; the train-BN engine never takes the path."""
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
        check_call(ext, *call)
    return e, [(name, signature(getattr(ext, name)).bind(*args, **kwargs).arguments) for name, args, kwargs in rec.calls]


def _dual(calls):
    return [a for name, a in calls if name == "bwd1x1" and a.get("x2") is not None]


def _split_wgrads_k64(calls):
    return [a for name, a in calls if name == "wgrad" and a.get("g2") is not None and a["K"] == 64]


def test_proj_bwd_on(monkeypatch):
    e, calls = _record(engine.HipEngine, "proj_bwd=1,proj_bwd_min_m=1", monkeypatch)
    assert e.proj_bwd
    dual = _dual(calls)
    assert len(dual) == 1
    a = dual[0]
    assert a.get("gx") is None and a["g1"] is not None and a["colsum_gx"] is not None
    M = a["g"].shape[0] * a["g"].shape[1] * a["g"].shape[2]
    assert a["x2"].shape[-1] == 64 and a["x2"].numel() == M * 64 and a["out_s"].numel() == M * 64
    assert tuple(a["wd2"].shape) == (64, 256) and a["wd2"].stride(0) == 320
    assert tuple(a["dw2"].shape) == (256, 64) and tuple(a["dw"].shape) == (256, 64)
    assert not _split_wgrads_k64(calls)


def test_proj_bwd_default_is_on_from_its_row_threshold(monkeypatch):
    """On by default, from proj_bwd_min_m GEMM rows up (b64 at 224; here 2 x 16 x 16 rows)."""
    e, calls = _record(engine.HipEngine, "", monkeypatch)
    s2 = e._s2_fed()
    assert e.proj_bwd and not _dual(calls) and len(_split_wgrads_k64(calls)) == 1
    assert e.proj_bwd_min_m == 64 * 56 * 56
    assert not e._proj_bwd(0, s2, 2) and e._proj_bwd(0, s2, e.proj_bwd_min_m // (16 * 16))
    assert not e._proj_bwd(0, s2, e.proj_bwd_min_m // (16 * 16) - 1) and not e._proj_bwd(1, s2, 10 ** 6)
    e, calls = _record(engine.HipEngine, "proj_bwd_min_m=1", monkeypatch)
    assert len(_dual(calls)) == 1 and not _split_wgrads_k64(calls)


@pytest.mark.parametrize("spec", ["proj_bwd=0,proj_bwd_min_m=1", "proj_bwd_min_m=1,c1pre=0", "proj_bwd_min_m=1,fuse_bwd=0"])
def test_proj_bwd_off(monkeypatch, spec):
    """The key off, or the pre form the path needs off: the launches of before."""
    e, calls = _record(engine.HipEngine, spec, monkeypatch)
    assert e.proj_bwd == ("proj_bwd=0" not in spec)
    assert not _dual(calls)
    assert len(_split_wgrads_k64(calls)) == 1


def test_train_bn_engine_never_takes_it(monkeypatch):
    e, calls = _record(engine_bn.HipEngineBNTrain, "proj_bwd=1,proj_bwd_min_m=1", monkeypatch)
    assert not e.proj_bwd and not _dual(calls)
