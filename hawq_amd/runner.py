"""What the three fused-plan executors (engine.py, engine_mbv2.py, engine_inception.py) share: HIP event timing for the tuners
and the execution scaffolding of a plan - stream hand-over, hipGraph capture / replay / destruction, the fork / join of
concurrent sub-batch chains and the two public entry points.

An engine derives from ``GraphRunner`` and provides its plan (``_build(N, H, W)``: ``x_in``, ``logits``, ``stream``, ``_batch`` and
the launch list; ``_ensure_u8(N, H, W)``: ``x_u8``, ``lut_dev``) and these hooks:
  * ``_launch_chain(u8)``      the launches of ONE chain, in order, on its stream (the leaf of ``_launch_all``);
  * ``_on_graph_dropped()``    what else a rebuild invalidates besides the captured graphs;
  * ``_collect_logits(redo)``  the result of the forward just queued (default: a clone of ``logits``);
  * ``_upload_lut(mean, std)`` fill ``lut_dev`` for ``forward_uint8`` (default: the [3][256] table of ``input_lut``).
Nothing here needs a constructor: the class attributes below are the state of an engine that has not built a plan yet.
"""
from __future__ import annotations

import ctypes as C
import os
from contextlib import contextmanager

import numpy as np
import torch

from . import _lib


def _i32(arr, dev):
    return torch.from_numpy(np.ascontiguousarray(arr, np.int32)).to(dev)


def _act_range(bits, mode):
    if mode == 'symmetric':
        return -(2 ** (bits - 1)), 2 ** (bits - 1) - 1
    return 0, 2 ** bits - 1


def _rng(act):
    """(lo, hi) of a QuantAct's integer range"""
    return _act_range(act.activation_bit, act.quant_mode)


class EventTimer:
    """``n`` HIP events on the stream with handle ``sp``, destroyed on exit - also when a launch in between raises."""

    def __init__(self, sp, n: int = 2):
        self.sp, self.n, self.events = sp, n, []

    def __enter__(self):
        try:
            for _ in range(self.n):
                e = C.c_void_p()
                _lib.call("hawq_event_create", C.byref(e))
                self.events.append(e)
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        while self.events:
            _lib.call("hawq_event_destroy", self.events.pop(0))

    def record(self, i):
        _lib.call("hawq_event_record", self.events[i], self.sp)

    def ms(self, i, j) -> float:
        """milliseconds between events i and j (waits for event j)"""
        out = C.c_float()
        _lib.call("hawq_event_elapsed_ms", self.events[i], self.events[j], C.byref(out))
        return out.value

    def elapsed_ms(self, launch, reps, warm: int = 1) -> float:
        """``warm`` untimed calls of ``launch``, then the milliseconds of ``reps`` calls together"""
        for _ in range(warm):
            launch()
        self.record(0)
        for _ in range(reps):
            launch()
        self.record(1)
        return self.ms(0, 1)

    def median_us(self, launch, reps, warm) -> float:
        """``warm`` untimed calls of ``launch``, then ``reps`` calls timed one by one (``n`` > ``reps`` events): their median, in
        microseconds"""
        for _ in range(warm):
            launch()
        self.record(0)
        for r in range(reps):
            launch()
            self.record(r + 1)
        return sorted(self.ms(r, r + 1) * 1000.0 for r in range(reps))[reps // 2]


def two_round_min(timer, candidates, prepare, reps, times=None):
    """Time every candidate in two rounds and keep each one's minimum (one hiccup must not decide a launch): ``times[c]`` = ms per
    ``reps`` launches, added to ``times`` if given.  ``prepare(c)`` selects candidate c and returns its launch; a candidate for which
    either raises RuntimeError (the library refuses it) gets no entry, and one refused in round one is skipped in round two."""
    times = {} if times is None else times
    refused = set()
    for _ in range(2):
        for c in candidates:
            if c in refused:
                continue
            try:
                ms = timer.elapsed_ms(prepare(c), reps)
            except RuntimeError:
                refused.add(c)
                continue
            times[c] = min(times.get(c, ms), ms)
    return times


class GraphRunner:
    subs = ()             # engines of the concurrent sub-batch chains of this plan, each with a stream of its own
    _graph = _graph_u8 = None
    _lut_key = None       # (mean, std) of the table in lut_dev

    # ------------------------------------------------------------------ hooks
    def _launch_chain(self, u8: bool):
        raise NotImplementedError

    def _on_graph_dropped(self):
        pass

    def _collect_logits(self, redo):
        """``redo(engine)`` repeats the same forward on another engine."""
        return self.logits.clone()

    def _upload_lut(self, mean, std):
        self.lut_dev.copy_(self.input_lut(mean, std).to(self.dev), non_blocking=False)

    # ------------------------------------------------------------------ launches and graphs
    def _launch_all(self, u8: bool = False):
        if not self.subs:
            return self._launch_chain(u8)
        fork = torch.cuda.Event()   # every chain on its own stream, joined back into self.stream
        fork.record(self.stream)
        for sub in self.subs:
            sub.stream.wait_event(fork)
            sub._launch_all(u8)
            join = torch.cuda.Event()
            join.record(sub.stream)
            self.stream.wait_event(join)

    def run_resident(self, u8: bool = False):
        """One forward over ``self.x_in`` (or, ``u8``, over ``self.x_u8``) already resident, on ``self.stream``: a replay of the
        hipGraph of that input form (captured on first use), or - ``use_graph`` False - the launches one by one."""
        if not self.use_graph:
            return self._launch_all(u8)
        attr = "_graph_u8" if u8 else "_graph"
        if getattr(self, attr) is None:
            self._launch_all(u8)   # warm-up outside capture (module loading, first-touch, lazy tuning)
            torch.cuda.synchronize(self.dev)
            _lib.call("hawq_graph_begin", self.stream.cuda_stream)
            g = C.c_void_p()
            try:
                self._launch_all(u8)
            finally:   # a stream must not be left capturing
                _lib.call("hawq_graph_end", self.stream.cuda_stream, C.byref(g))
            setattr(self, attr, g)
        _lib.call("hawq_graph_launch", getattr(self, attr), self.stream.cuda_stream)

    def _drop_graph(self):
        for attr in ("_graph", "_graph_u8"):
            g = getattr(self, attr)
            if g is not None:
                setattr(self, attr, None)
                _lib.call("hawq_graph_destroy", g)
        self._on_graph_dropped()

    def __del__(self):
        try:
            self._drop_graph()
        except Exception:
            pass

    def _time_graph(self, reps: int) -> float:
        """ms per replay of the captured graph (tuning only) on synthetic images ~ N(0, 1), seeded: an all-zero batch
        (HAWQ_TUNE_INPUT=zero) switches fewer bits in every pipe than real data does and replays ~1.5 % faster, which is not the
        regime the plans are chosen for, and uninitialised memory made the choice depend on whatever the allocator handed out."""
        if os.environ.get("HAWQ_TUNE_INPUT", "normal") == "zero":
            self.x_in.zero_()
        else:
            g = torch.Generator(device=self.dev)
            g.manual_seed(0)
            self.x_in.normal_(generator=g)
        with EventTimer(self.stream.cuda_stream) as timer, torch.cuda.stream(self.stream):
            ms = timer.elapsed_ms(self.run_resident, reps, warm=2)
        torch.cuda.synchronize(self.dev)
        return ms / reps

    # ------------------------------------------------------------------ entry points
    @contextmanager
    def _handed_over(self):
        """the body runs on ``self.stream`` after everything queued on the caller's stream, which then waits for it"""
        cur = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            yield
        cur.wait_stream(self.stream)

    def __call__(self, x):
        """fp32 NCHW images on the GPU -> a FRESH fp32 logits tensor."""
        if not x.is_cuda:
            raise RuntimeError(f"{type(self).__name__}: input must be on the MI355X (no CPU path)")
        N, Cc, H, W = x.shape
        if Cc != 3:
            raise ValueError("expected [N,3,H,W] images")
        if self._batch != (N, H, W):
            self._build(N, H, W)
        with self._handed_over():
            self.x_in.copy_(x, non_blocking=True)
            self.run_resident()
            return self._collect_logits(lambda eng: eng(x))

    def _forward_uint8(self, x_u8, mean, std):
        """``forward_uint8`` behind each engine's own argument check"""
        N, H, W, _ = x_u8.shape
        if self._batch != (N, H, W):
            self._build(N, H, W)
        self._ensure_u8(N, H, W)
        key = (tuple(float(v) for v in mean), tuple(float(v) for v in std))
        with self._handed_over():
            if self._lut_key != key:
                self._upload_lut(mean, std)
                self._lut_key = key
            self.x_u8.copy_(x_u8, non_blocking=True)
            self.run_resident(u8=True)
            return self._collect_logits(lambda eng: eng.forward_uint8(x_u8, mean, std))
