"""The forward's launches at the conv2_block1 -> 2 boundary (PDDL_ENGINE c3c1_proj, c3c1_proj_min_m),
recorded on the CPU (see test_engine_schedule_cpu, test_c3c1_s3_schedule_cpu): with the row gate
lowered to the 512 stage-2 rows of the B = 2, 64-pixel engine, conv2_block1's dual-source conv3 +
shortcut GEMM and conv2_block2's conv1 become one c3c1 call with the pool output as `a2`; at the
default gate the call list is the one without the path, and c3c1_proj=0, c3c1=0 and fuse_proj=0 each
switch it off."""
import pytest
import torch

from pddl.models import engine, engine_bn
from test_c3c1_s3_schedule_cpu import _c3c1, _conv1_igemms, _record


def _ptr(v):
    return v.data_ptr() if isinstance(v, torch.Tensor) else v


def _flat(calls):
    """A call list as comparable values: tensors by address, shape and dtype."""
    return [(name, {k: (_ptr(v), tuple(v.shape), v.dtype) if isinstance(v, torch.Tensor) else v for k, v in a.items()})
            for name, a in calls]


def _dual_conv3(e, calls, block):
    """Dual-source (x2 given) forward igemm launches that write `block`'s output."""
    out = e.acts[block]["out"]
    return [a for name, a in calls
            if name == "igemm" and a["out"].data_ptr() == out.data_ptr() and a.get("a2") is not None]


def test_projection_boundary_fused(monkeypatch):
    e, calls = _record(engine.HipEngine, "c3c1_proj_min_m=1", monkeypatch)
    assert e.c3c1 == 2 and e.c3c1_proj and e.c3c1_proj_min_m == 1
    cc = _c3c1(calls)
    assert len(cc) == 4
    new = [a for a in cc if a.get("a2") is not None]
    assert len(new) == 1
    a = new[0]
    M = a["a"].numel() // 64
    assert M == 512 and a["a"].shape[-1] == 64
    assert a["a"].data_ptr() == e.acts["conv2_block1"]["y2"].data_ptr()
    assert a["a2"].data_ptr() == e.pool.data_ptr() and a["a2"].numel() == M * 64
    assert tuple(a["w3"].shape) == (256, 128) and tuple(a["w1"].shape) == (64, 256)
    assert a["res"] is None
    assert a["out"].data_ptr() == e.acts["conv2_block1"]["out"].data_ptr() and a["out"].numel() == M * 256
    assert a["y1"].data_ptr() == e.acts["conv2_block2"]["y1"].data_ptr() and a["y1"].numel() == M * 64
    k = e.ch["fuse:conv2_block1"]
    assert a["scale3"].data_ptr() == e.scale[k:].data_ptr() and a["shift3"].data_ptr() == e.shift[k:].data_ptr()
    assert a["bits3"].numel() == M * 32 and a["bits1"].numel() == M * 8
    assert not _conv1_igemms(e, calls, "conv2_block2")
    assert not _dual_conv3(e, calls, "conv2_block1")
    # the rest of the boundaries are as before
    assert len(_conv1_igemms(e, calls, "conv2_block1")) == 1
    assert sorted(x["a"].shape[-1] for x in cc if x.get("a2") is None) == [64, 128, 128]


def _default_calls(monkeypatch):
    e, calls = _record(engine.HipEngine, "c3c1_proj=0", monkeypatch)
    assert not e.c3c1_proj
    return e, calls


def test_default_gate_keeps_the_separate_launches(monkeypatch):
    e, calls = _record(engine.HipEngine, "", monkeypatch)
    assert e.c3c1_proj and e.c3c1_proj_min_m >= 16384
    assert len(_c3c1(calls)) == 3 and all(a.get("a2") is None for a in _c3c1(calls))
    assert len(_dual_conv3(e, calls, "conv2_block1")) == 1 and len(_conv1_igemms(e, calls, "conv2_block2")) == 1
    names = [n for n, _ in calls]
    e0, calls0 = _default_calls(monkeypatch)
    assert names == [n for n, _ in calls0]
    # same launches on the same operands (two engines: compare shapes, dtypes and scalars)
    strip = lambda cs: [(n, {k: v[1:] if isinstance(v, tuple) else v for k, v in a.items()}) for n, a in _flat(cs)]
    assert strip(calls) == strip(calls0)


@pytest.mark.parametrize("spec", ["c3c1_proj=0", "c3c1=0", "fuse_proj=0"])
def test_switched_off(monkeypatch, spec):
    e, calls = _record(engine.HipEngine, spec + ",c3c1_proj_min_m=1", monkeypatch)
    assert not e.c3c1_proj
    assert all(a.get("a2") is None for a in _c3c1(calls))
    assert len(_conv1_igemms(e, calls, "conv2_block2")) == 1
    if spec != "fuse_proj=0":
        assert len(_dual_conv3(e, calls, "conv2_block1")) == 1


def test_train_bn_engine_never_takes_it(monkeypatch):
    e, calls = _record(engine_bn.HipEngineBNTrain, "c3c1_proj_min_m=1", monkeypatch)
    assert e.c3c1 == 0 and not e.c3c1_proj and not _c3c1(calls)
