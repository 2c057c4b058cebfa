"""hawq_amd.runner without a device: the order of library calls of graph capture / replay / destruction and of the event
timer.  ``hawq_amd._lib.call`` is a recorder, the stream a stub with a ``cuda_stream`` handle."""
import types

import pytest
import torch


class Recorder:
    """stands for ``_lib.call``: logs (name, args), hands out event / graph handles, scripts the elapsed times"""

    def __init__(self):
        self.calls, self.handles, self.ms, self.engines = [], 0, [], []

    def __call__(self, name, *args):
        self.calls.append((name, args))
        if name in ("hawq_event_create", "hawq_graph_end"):
            self.handles += 1
            args[-1]._obj.value = 0x1000 + self.handles
        if name == "hawq_event_elapsed_ms":
            args[-1]._obj.value = self.ms.pop(0) if self.ms else 1.0

    def names(self, prefix=""):
        return [n for n, _ in self.calls if n.startswith(prefix)]

    def values(self, name):
        """the handle each `name` call was given (first argument, or the one it wrote for a create)"""
        return [(a[0]._obj if name == "hawq_event_create" else a[0]).value for n, a in self.calls if n == name]


@pytest.fixture
def rec(monkeypatch):
    from hawq_amd import _lib
    r = Recorder()
    monkeypatch.setattr(_lib, "call", r)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: r.calls.append(("synchronize", ())))
    yield r
    for eng in r.engines:   # no fake handle may reach the real library when an engine is collected later
        eng._graph = eng._graph_u8 = None


def _engine(rec, use_graph=True, fail_at=None):
    from hawq_amd import _lib
    from hawq_amd.runner import GraphRunner

    class Engine(GraphRunner):
        def __init__(self):
            self.use_graph, self.dev, self.stream = use_graph, "dev", types.SimpleNamespace(cuda_stream=0x51)
            self.passes, self.resets = 0, 0

        def _launch_chain(self, u8):
            self.passes += 1
            _lib.call("op_a", int(u8), self.stream.cuda_stream)
            if self.passes == fail_at:
                raise RuntimeError("launch failed")
            _lib.call("op_b", int(u8), self.stream.cuda_stream)

        def _on_graph_dropped(self):
            self.resets += 1

    rec.engines.append(Engine())
    return rec.engines[-1]


def test_first_run_captures_and_later_runs_replay(rec):
    eng = _engine(rec)
    eng.run_resident()
    assert rec.names() == ["op_a", "op_b", "synchronize", "hawq_graph_begin", "op_a", "op_b", "hawq_graph_end", "hawq_graph_launch"]
    assert all(a[-1] == 0x51 or n == "hawq_graph_end" for n, a in rec.calls if n != "synchronize")
    g = eng._graph.value
    assert rec.calls[-1] == ("hawq_graph_launch", (eng._graph, 0x51)) and eng._graph_u8 is None
    del rec.calls[:]
    eng.run_resident()
    assert rec.names() == ["hawq_graph_launch"] and eng._graph.value == g


def test_u8_captures_a_second_graph_and_leaves_the_first_alone(rec):
    eng = _engine(rec)
    eng.run_resident()
    first = eng._graph
    del rec.calls[:]
    eng.run_resident(u8=True)
    assert rec.names() == ["op_a", "op_b", "synchronize", "hawq_graph_begin", "op_a", "op_b", "hawq_graph_end", "hawq_graph_launch"]
    assert [a[0] for n, a in rec.calls if n in ("op_a", "op_b")] == [1, 1, 1, 1]
    assert eng._graph is first and eng._graph_u8.value != first.value
    assert rec.calls[-1][1][0] is eng._graph_u8
    del rec.calls[:]
    eng.run_resident()
    eng.run_resident(u8=True)
    assert [(n, a[0].value) for n, a in rec.calls] == [("hawq_graph_launch", first.value), ("hawq_graph_launch", eng._graph_u8.value)]


def test_capture_is_ended_when_a_launch_raises_inside_it(rec):
    eng = _engine(rec, fail_at=2)   # the warm-up pass succeeds, the captured pass fails
    with pytest.raises(RuntimeError, match="launch failed"):
        eng.run_resident()
    assert rec.names() == ["op_a", "op_b", "synchronize", "hawq_graph_begin", "op_a", "hawq_graph_end"]
    assert eng._graph is None   # nothing half-captured is kept or replayed


def test_drop_graph_destroys_each_live_graph_once_and_resets_the_engine(rec):
    eng = _engine(rec)
    eng.run_resident()
    eng.run_resident(u8=True)
    live = sorted((eng._graph.value, eng._graph_u8.value))
    del rec.calls[:]
    eng._drop_graph()
    assert sorted(rec.values("hawq_graph_destroy")) == live and rec.names() == ["hawq_graph_destroy"] * 2
    assert eng._graph is None and eng._graph_u8 is None and eng.resets == 1
    eng._drop_graph()
    assert rec.names() == ["hawq_graph_destroy"] * 2   # nothing is destroyed twice
    eng = _engine(rec)
    eng.run_resident()   # only the fp32 graph is live
    del rec.calls[:]
    eng._drop_graph()
    assert rec.names() == ["hawq_graph_destroy"]


def test_without_graph_every_run_launches_directly(rec):
    eng = _engine(rec, use_graph=False)
    eng.run_resident()
    eng.run_resident(u8=True)
    eng._drop_graph()
    assert rec.names() == ["op_a", "op_b"] * 2 and not rec.names("hawq_graph_")
    assert eng._graph is None and eng._graph_u8 is None


def test_an_engine_needs_no_constructor(rec):
    from hawq_amd.runner import GraphRunner
    eng = GraphRunner.__new__(GraphRunner)
    eng._drop_graph()
    assert not rec.calls and not eng.subs and eng._lut_key is None


@pytest.mark.parametrize("warm,reps", [(1, 3), (2, 5), (0, 1)])
def test_event_timer_launches_warm_plus_reps_between_create_and_destroy(rec, warm, reps):
    from hawq_amd.runner import EventTimer
    rec.ms = [7.5]
    with EventTimer(0x51) as timer:
        assert timer.elapsed_ms(lambda: rec("launch"), reps, warm) == 7.5
    assert rec.names() == (["hawq_event_create"] * 2 + ["launch"] * warm + ["hawq_event_record"] + ["launch"] * reps
                           + ["hawq_event_record", "hawq_event_elapsed_ms"] + ["hawq_event_destroy"] * 2)
    created = rec.values("hawq_event_create")
    assert len(set(created)) == 2 and rec.values("hawq_event_destroy") == created
    assert [(a[0].value, a[1]) for n, a in rec.calls if n == "hawq_event_record"] == [(created[0], 0x51), (created[1], 0x51)]
    assert [a[0].value for n, a in rec.calls if n == "hawq_event_elapsed_ms"] == created[:1]


@pytest.mark.parametrize("n", [2, 6])
def test_event_timer_destroys_every_event_when_a_launch_raises(rec, n):
    from hawq_amd.runner import EventTimer

    def launch():
        rec("launch")
        if len(rec.names("launch")) == 3:
            raise RuntimeError("launch failed")

    with pytest.raises(RuntimeError, match="launch failed"):
        with EventTimer(0x51, n) as timer:
            timer.elapsed_ms(launch, 4)
    created = rec.values("hawq_event_create")
    assert len(set(created)) == n and rec.values("hawq_event_destroy") == created
    assert rec.names("launch") == ["launch"] * 3 and not rec.names("hawq_event_elapsed")


def test_two_round_minimum_skips_what_round_one_refused(rec):
    from hawq_amd.runner import EventTimer, two_round_min
    # candidate 2 is refused in round one; round one then times 1, 3 and round two 1, 3 again
    rec.ms = [5.0, 9.0, 6.0, 4.0]
    prepared = []

    def prepare(c):
        prepared.append(c)

        def launch():
            if c == 2:
                raise RuntimeError("refused")
            rec("launch", c)
        return launch

    with EventTimer(0x51) as timer:
        times = two_round_min(timer, [1, 2, 3], prepare, 2)
    assert prepared == [1, 2, 3, 1, 3]
    assert times == {1: 5.0, 3: 4.0}
    assert [a[0] for n, a in rec.calls if n == "launch"] == [1] * 3 + [3] * 3 + [1] * 3 + [3] * 3

    # a refusal in round two only loses that round's sample; entries of a caller's dict are kept and extended
    rec.ms, seen = [3.0, 8.0, 2.0], []

    def flaky(c):
        seen.append(c)
        if seen.count(c) == 2 and c == -4:
            raise RuntimeError("refused")
        return lambda: None

    with EventTimer(0x51) as timer:
        times = two_round_min(timer, [-2, -4], flaky, 1, {7: 1.0})
    assert times == {7: 1.0, -2: 2.0, -4: 8.0}
