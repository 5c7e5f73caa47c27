"""The two-stream hazard protocol of the HIP engines (models/side_stream.py) on the CPU: the
mixin on a bare host object, with fake streams and events that log every record / wait / launch
together with the stream it happened on.  A mistake in this protocol is a silent race on the GPU,
so the tests assert the exact log."""
import contextlib

import pytest
import torch

from pddl.models.side_stream import SideStream

NAMES = ("_init_side", "_side_begin_step", "_event", "_side_run", "_before_write", "_join_side", "_bucket_ready",
         "begin_defer", "take_deferred", "end_defer")


class Host(SideStream):
    device = torch.device("cuda")
    defer_side = True


class FakeStream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_event(self, ev):
        self.log.append(("wait", self.name, ev.i))


class World:
    """torch.cuda's streams and events, replaced: one log, a current stream, numbered events."""

    def __init__(self, mp):
        self.log, self.n_events = [], 0
        self.main = self.cur = FakeStream("main", self.log)
        world = self

        class FakeEvent:
            def __init__(self):
                self.i = world.n_events
                world.n_events += 1

            def record(self, stream):
                world.log.append(("record", self.i, stream.name))

        @contextlib.contextmanager
        def stream(s):
            prev, world.cur = world.cur, s
            try:
                yield
            finally:
                world.cur = prev

        mp.setattr(torch.cuda, "Event", FakeEvent)
        mp.setattr(torch.cuda, "Stream", lambda dev: FakeStream("side", self.log))
        mp.setattr(torch.cuda, "current_stream", lambda dev=None: world.cur)
        mp.setattr(torch.cuda, "stream", stream)

    def fn(self, *args):
        self.log.append(("launch", self.cur.name, args))

    def cb(self, i):
        self.log.append(("bucket", self.cur.name, i))

    def take(self):
        out = list(self.log)
        del self.log[:]
        return out


@pytest.fixture
def world(monkeypatch):
    return World(monkeypatch)


def _host(two_stream=True):
    h = Host()
    h._init_side(h.device, two_stream)
    return h


def test_init_side(world):
    h = _host()
    assert h.side.name == "side" and h._defer is None
    assert (h._evpool, h._evi, h._pending, h._last_side) == ([], 0, {}, None)
    assert _host(False).side is None
    cpu = Host()
    cpu._init_side(torch.device("cpu"), True)      # (no side stream off the GPU)
    assert cpu.side is None and cpu._defer is None
    assert world.take() == []


def test_two_steps_reuse_the_event_pool(world):
    h = _host()
    step = [("record", 0, "main"), ("wait", "side", 0), ("launch", "side", (1, "x")), ("record", 1, "side"),
            ("record", 2, "main"), ("wait", "side", 2), ("launch", "side", (2,)), ("record", 3, "side")]
    for _ in range(2):
        h._side_begin_step()
        h._side_run(world.fn, 1, "x", reads=("a",))
        h._side_run(world.fn, 2, reads=("b", "c"))
        assert world.take() == step
        assert h._evi == 4 and len(h._evpool) == 4 and world.n_events == 4
        assert {k: e.i for k, e in h._pending.items()} == {"a": 1, "b": 3, "c": 3}
        assert h._last_side.i == 3
    h._side_begin_step()
    assert (h._pending, h._last_side, h._evi) == ({}, None, 0) and len(h._evpool) == 4


def test_before_write_waits_once_per_pending_key(world):
    h = _host()
    h._side_begin_step()
    h._side_run(world.fn, reads=("a", ("g", 1)))
    h._side_run(world.fn, reads=("b",))
    h._side_run(world.fn)                            # (reads nothing: nothing to wait for later)
    h._side_run(world.fn, reads=("a",))              # the LAST reader of "a" is what a write waits for
    world.take()
    h._before_write("unknown")
    assert world.take() == []
    h._before_write("a", ("g", 1), "unknown")
    assert world.take() == [("wait", "main", 7), ("wait", "main", 1)]
    h._before_write("a", ("g", 1))
    assert world.take() == []
    assert list(h._pending) == ["b"]
    with torch.cuda.stream(FakeStream("other", world.log)):      # the wait lands on the CURRENT stream
        h._before_write("b")
    assert world.take() == [("wait", "other", 3)]
    assert h._pending == {} and world.n_events == 8


def test_join_side_is_idempotent(world):
    h = _host()
    h._side_begin_step()
    h._join_side()                                   # nothing ran on the side stream yet
    assert world.take() == []
    h._side_run(world.fn, reads=("a",))
    h._side_run(world.fn, reads=("b",))
    world.take()
    h._join_side()
    assert world.take() == [("wait", "main", 3)]
    assert h._pending == {} and h._last_side is None
    h._join_side()
    h._before_write("a", "b")
    assert world.take() == []
    h._side_run(world.fn, reads=("a",))              # the pool goes on where the step left it
    assert world.take() == [("record", 4, "main"), ("wait", "side", 4), ("launch", "side", ()), ("record", 5, "side")]


def test_one_stream_runs_inline(world):
    h = _host(False)
    h._side_begin_step()
    h._side_run(world.fn, 7, reads=("a",))
    h._before_write("a")
    h._bucket_ready(world.cb, 0)
    h._join_side()
    assert world.take() == [("launch", "main", (7,)), ("bucket", "main", 0)]
    assert world.n_events == 0 and h._pending == {} and h._last_side is None and h._evpool == []


def test_deferred_mode_queues(world):
    h = _host()
    h._side_begin_step()
    h._side_run(world.fn, 0, reads=("a",))
    world.take()
    h.begin_defer()
    assert h._defer == []
    h._side_run(world.fn, 1, reads=("a",))
    h._side_run(world.fn, 2)
    h._before_write("a")                             # pass-through: the pending reader is NOT waited for
    h._bucket_ready(world.cb, 3)                     # pass-through: the callback on the calling stream
    assert world.take() == [("bucket", "main", 3)]
    assert list(h._pending) == ["a"] and world.n_events == 2
    q = h.take_deferred()
    assert q == [(world.fn, (1,)), (world.fn, (2,))] and h._defer == []
    h._side_run(world.fn, 4)
    with pytest.raises(AssertionError, match="deferred side work left uncaptured"):
        h.end_defer()
    assert h._defer is None                          # (back to launching either way)
    h.begin_defer()
    h._side_run(world.fn, 5)
    assert h.take_deferred() == [(world.fn, (5,))]
    h.end_defer()
    assert h._defer is None and world.take() == []
    h._side_run(world.fn, 6)                         # launching again
    assert world.take() == [("record", 2, "main"), ("wait", "side", 2), ("launch", "side", (6,)), ("record", 3, "side")]


def test_begin_defer_needs_a_side_stream_and_defer_side(world):
    with pytest.raises(AssertionError):
        _host(False).begin_defer()
    h = _host()
    h.defer_side = False
    with pytest.raises(AssertionError):
        h.begin_defer()


def test_bucket_ready_runs_the_callback_on_the_side_stream(world):
    h = _host()
    h._side_begin_step()
    h._side_run(world.fn, reads=("a",))
    world.take()
    h._bucket_ready(world.cb, 0)
    assert world.take() == [("record", 2, "main"), ("wait", "side", 2), ("bucket", "side", 0), ("record", 3, "side")]
    assert h._last_side.i == 3 and list(h._pending) == ["a"]     # the compute stream did not block
    h._join_side()                                   # the step's join covers the callback's work
    assert world.take() == [("wait", "main", 3)]


def test_bucket_ready_joins_first_when_the_callback_needs_it(world):
    h = _host()
    h._side_begin_step()
    h._side_run(world.fn, reads=("a",))
    world.take()

    def cb(i):
        world.cb(i)
    cb.needs_join = True
    h._bucket_ready(cb, 1)
    assert world.take() == [("wait", "main", 1), ("bucket", "main", 1)]
    assert h._pending == {} and h._last_side is None and world.n_events == 2


def test_engines_resolve_to_the_mixin():
    from pddl.models.engine import HipEngine
    from pddl.models.engine_bn import HipEngineBNTrain
    from pddl.models.engine_f32 import HipF32Engine, HipF32EngineBNTrain
    for cls in (HipEngine, HipEngineBNTrain, HipF32Engine, HipF32EngineBNTrain):
        assert issubclass(cls, SideStream)
        for name in NAMES:
            assert getattr(cls, name) is SideStream.__dict__[name], (cls.__name__, name)
