"""The four HIP engines' launch schedules, checked on the CPU against the bindings' signatures.

Every engine runs init / forward_backward / after_update / evaluate on CPU tensors against a
stand-in for the native module that records each call instead of launching it.  Every
recorded call must then bind to the signature the built extension publishes in its
docstring, with a tensor wherever the binding takes a tensor and a number wherever it takes
a number -- so a misplaced or misspelt argument in a rarely taken fusion branch fails here
and not first on the GPU.  No launch counts and no digests: the schedule itself may change.
"""
import inspect
import re

import pytest
import torch

from pddl.models import engine, engine_bn, engine_f32
from pddl.models.resnet50 import ParamLayout
from pddl.ops.native import require_native


class Recorder:
    """Stand-in for the native module: forwards the table-size / epilogue-mode constants and the
    host-only *_partial_rows functions, answers splitk_default_floats itself, and only records
    every other call (nothing launches, on a GPU machine either)."""

    def __init__(self, ext):
        self._ext = ext
        self.calls = []

    def __getattr__(self, name):
        real = getattr(self._ext, name)   # (a binding the extension does not have: AttributeError)
        if name.endswith("_BYTES") or name.startswith("EPI_"):
            assert isinstance(real, int)
            return real
        if name.endswith("_partial_rows"):
            return real
        if name == "splitk_default_floats":
            return lambda device: 4096
        return lambda *args, **kwargs: self.calls.append((name, args, kwargs))


def _split_top(s, sep=","):
    """Split at the separators outside brackets."""
    parts, depth, cur = [], 0, ""
    for ch in s:
        depth += ch in "[("
        depth -= ch in "])"
        if ch == sep and depth == 0:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
    return parts + [cur] if cur.strip() else parts


def signature(fn) -> inspect.Signature:
    """The signature in the first line of a pybind11 docstring, annotations kept as text.  (A
    binding may default an argument in the middle of its list: not a valid Python `def`, but
    Signature.bind handles it.)"""
    m = re.match(r"\w+\((.*)\) -> ", fn.__doc__.splitlines()[0])
    params = []
    for item in _split_top(m.group(1)):
        name, _, ann = item.partition(":")
        ann, eq, default = ann.partition(" = ")
        params.append(inspect.Parameter(name.strip(), inspect.Parameter.POSITIONAL_OR_KEYWORD,
                                        annotation=ann.strip(),
                                        default=default.strip() if eq else inspect.Parameter.empty))
    return inspect.Signature(params, __validate_parameters__=False)


def check_call(ext, name, args, kwargs):
    """(name, args, kwargs) binds to ext.name's signature with values of the annotated kinds."""
    sig = signature(getattr(ext, name))
    try:
        bound = sig.bind(*args, **kwargs)
    except TypeError as e:
        raise AssertionError(f"{name}: {e}") from None
    for pname, v in bound.arguments.items():
        ann = sig.parameters[pname].annotation
        kinds = [a.strip() for a in ann.split("|")]
        what = f"{name}({pname}: {ann}) got {type(v).__name__}"
        if kinds[0] == "torch.Tensor":
            assert isinstance(v, torch.Tensor) or (v is None and "None" in kinds), what
        elif kinds[0] in ("typing.SupportsInt", "typing.SupportsFloat", "int", "float", "bool"):
            assert isinstance(v, (int, float)) and not isinstance(v, torch.Tensor), what
            if kinds[0] in ("typing.SupportsInt", "int"):
                assert isinstance(v, int), what


def test_signature_parser():
    ext = require_native()
    sig = signature(ext.igemm)
    assert list(sig.parameters)[:3] == ["a1", "a2", "H"] and len(sig.parameters) == 30
    assert sig.parameters["a2"].annotation == "torch.Tensor | None" and sig.parameters["a2"].default == "None"
    assert sig.parameters["H"].default is inspect.Parameter.empty
    t = torch.zeros(1)
    ok = ("wgrad", (t, 1, 1, 1, 1, 1, 0, 1, 1, t), dict(dw=t, K=1))
    check_call(ext, *ok)
    for bad in (("wgrad", (t, 1, 1, 1, 1, 1, 0, 1, 1, t), dict(dw=t)),            # K missing
                ("wgrad", (t, 1, 1, 1, 1, 1, 0, 1, 1, t), dict(dw=t, K=1, k=3)),   # unknown keyword
                ("wgrad", (t, 1, 1, 1, 1, 1, 0, 1, 1, t, 0, None, t, 1, 0), {}),  # g2 / co_split swapped
                ("wgrad", (t, 1, 1, 1, 1, 1, 0, 1, 1, t), dict(dw=None, K=1)),     # a required tensor
                ("wgrad", (t, 1, 1, 1, 1, 1, 0, 1, 1, t), dict(dw=t, K=t))):       # a tensor for a number
        with pytest.raises(AssertionError):
            check_call(ext, *bad)


ENGINES = {
    "bf16": (engine.HipEngine, "igemm"),
    "bf16-bn": (engine_bn.HipEngineBNTrain, "igemm"),
    "f32": (engine_f32.HipF32Engine, "conv_f32_epi"),
    "f32-bn": (engine_f32.HipF32EngineBNTrain, "conv_f32_epi"),
}
# (PDDL_ENGINE, crop of the 64-pixel image); crop 56: stem modes 2 (training) and 1 (evaluation)
CONFIGS = {
    "default": ("", 64),
    "unfused": ("fuse_proj=0,fuse_bwd=0,fuse_stem=0,c64=0,c3c1=0,c1pre=0,s2c=0,bitmask=0", 64),
    "c64": ("c64_min_m=1", 64),
    "fuse_bwd2": ("fuse_bwd=2", 64),
    "no_bwd_s2": ("fuse_bwd_s2=0", 64),
    "crop56": ("", 56),
}


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("eng", list(ENGINES))
def test_schedule_binds(eng, cfg, monkeypatch):
    ext = require_native()
    rec = Recorder(ext)
    for mod in (engine, engine_bn, engine_f32):
        monkeypatch.setattr(mod, "require_native", lambda: rec, raising=False)
    spec, crop = CONFIGS[cfg]
    monkeypatch.setenv("PDDL_ENGINE", spec)
    cls, conv = ENGINES[eng]
    B, size = 2, 64
    L = ParamLayout()
    e = cls(L, B, crop=crop, image_size=size, device="cpu")
    e.init(seed=0)
    images = torch.zeros(B, size, size, 3, dtype=torch.uint8)
    labels = torch.zeros(B, dtype=torch.int64)
    buckets = L.buckets(32)
    fired = []
    e.forward_backward(images, labels, 1.0 / B, bucket_cb=fired.append, buckets=buckets)
    e.after_update()
    e.evaluate(images, labels)
    assert fired == list(range(len(buckets)))
    assert sum(name == conv for name, _, _ in rec.calls) > 0, "the stand-in was bypassed"
    for call in rec.calls:
        check_call(ext, *call)
