"""Host side of the vectorised InceptionV3 pool / requant kernels (hawq_amd/csrc/incep_pool.hip): the entry points exist in the
header, the ctypes table and the library, ``hawq_incep_pool_v_avg3_tile`` reports the tiles the plans run on, and ``hawq_incep_pool_v_ok`` accepts what the engine launches and refuses what the kernels
cannot do.  Nothing here launches a kernel: ``_ok`` never does, and ``hawq_incep_pool_v`` is only called on refused descriptions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUANT, MAX3S2, AVG3, GLOBAL = 0, 1, 2, 3
PRE = (3 << 28, 30, -32768, 32767)
POST8 = (5 << 27, 33, -128, 127)
POST16 = (1 << 30, 31, -20000, 20000)

_BUF = np.zeros(4096 + 16, np.int8)
BASE = (_BUF.ctypes.data + 15) // 16 * 16   # a 16-byte aligned host address: _ok only looks at the pointer values


def _args(C_, in_bits=16, out_bits=8, pre=None, post=POST8, N=2, H=8, W=8, in_pitch=None, in_off=0, ldo=None, c_off=0,
          in_ptr=None, out_ptr=None):
    from hawq_amd import _lib
    a = _lib.IncepPoolArgs()
    a.in_, a.out = (BASE if in_ptr is None else in_ptr), (BASE + 2048 if out_ptr is None else out_ptr)
    a.N, a.H, a.W, a.C, a.in_bits, a.in_pitch, a.in_off = N, H, W, C_, in_bits, (C_ if in_pitch is None else in_pitch), in_off
    a.out_bits, a.ldo, a.c_off = out_bits, (C_ if ldo is None else ldo), c_off
    if pre:
        a.pre, (a.m1, a.ek1, a.lo1, a.hi1) = 1, pre
    if post:
        a.post, (a.m2, a.ek2, a.lo2, a.hi2) = 1, post
    return a


def _ok(a, op):
    from hawq_amd import _lib
    return _lib.load().hawq_incep_pool_v_ok(C.byref(a), op)


def lib_has(name):
    from hawq_amd import _lib
    return hasattr(_lib.load(), name)


def _tile(a):
    from hawq_amd import _lib
    th, tw = C.c_int32(), C.c_int32()
    _lib.call("hawq_incep_pool_v_avg3_tile", C.byref(a), C.byref(th), C.byref(tw))
    return th.value, tw.value


def test_average_pool_tiles_of_the_shipped_plans():
    """(rows, columns) of the average pool's workgroup tile: what 32 KB of LDS hold at 32 channels, evened out over the map, halved
    while the launch has fewer than 512 workgroups; 32 columns on maps wider than 40"""
    avg = lambda n, h, w, c: _args(c, 16, 8, PRE, POST8, N=n, H=h, W=w)
    assert [_tile(avg(128, 35, 35, c)) for c in (192, 256, 288)] == [(9, 35)] * 3      # the batch-128 plan: 630 output lanes
    assert _tile(avg(128, 17, 17, 768)) == (17, 17) and _tile(avg(128, 8, 8, 1280)) == (8, 8)
    assert _tile(avg(1, 35, 35, 288)) == (3, 35) and _tile(avg(1, 17, 17, 768)) == (3, 17) and _tile(avg(1, 8, 8, 2048)) == (4, 8)
    assert _tile(avg(2, 10, 45, 48)) == (3, 32) and _tile(avg(128, 147, 147, 64)) == (13, 32)
    for n, h, w, c in ((128, 35, 35, 288), (1, 299, 299, 16), (4, 40, 40, 32), (2, 3, 1000, 64)):
        th, tw = _tile(avg(n, h, w, c))
        assert 1 <= th <= h and 1 <= tw <= w and (th + 2) * (tw + 2) * 32 * 2 <= 32768   # the staged tile fits the LDS it is given
    bad = avg(2, 5, 4, 64)
    bad.hi1 = 40000
    with pytest.raises(RuntimeError, match="hawq_incep_pool_v_avg3_tile"):
        _tile(bad)


def test_entry_points_are_declared_bound_and_exported():
    from hawq_amd import _lib
    header = open(os.path.join(ROOT, "include", "hawq_mi355.h")).read()
    assert re.search(r"int hawq_incep_pool_v_ok\(const hawq_incep_pool_args \*a, int op\);", header)
    assert re.search(r"int hawq_incep_pool_v\(const hawq_incep_pool_args \*a, int op, void \*stream\);", header)
    assert re.search(r"HAWQ_INCEP_POOL_REQUANT = 0, HAWQ_INCEP_POOL_MAX3S2 = 1, HAWQ_INCEP_POOL_AVG3 = 2, HAWQ_INCEP_POOL_GLOBAL = 3", header)
    assert re.search(r"#define HAWQ_ABI_VERSION 5\b", header)
    assert re.search(r"int hawq_incep_pool_v_avg3_tile\(const hawq_incep_pool_args \*a, int32_t \*th, int32_t \*tw\);", header)
    assert len(_lib.SIGNATURES["hawq_incep_pool_v_avg3_tile"]) == 3 and lib_has("hawq_incep_pool_v_avg3_tile")
    assert len(_lib.SIGNATURES["hawq_incep_pool_v_ok"]) == 2 and len(_lib.SIGNATURES["hawq_incep_pool_v"]) == 3
    lib = _lib.load()
    assert lib.hawq_incep_pool_v_ok is not None and lib.hawq_incep_pool_v is not None
    assert lib.hawq_abi_version() == 5
    assert _lib.INCEP_POOL_OPS == {"hawq_incep_requant": REQUANT, "hawq_incep_maxpool3s2": MAX3S2,
                                   "hawq_incep_avgpool_branch": AVG3, "hawq_incep_global_avgpool": GLOBAL}


# the description kinds of tests/test_gpu_inception_kernels.py::test_pool_kernels_at_every_description_the_engine_launches
KINDS = {
    "requant_16_8": (REQUANT, lambda c: _args(c, 16, 8, None, POST8)),
    "requant_16_16_slice": (REQUANT, lambda c: _args(c, 16, 16, None, POST16, ldo=2 * c + 32, c_off=c + 16)),
    "maxpool_8_8": (MAX3S2, lambda c: _args(c, 8, 8, None, None, H=7, W=5)),
    "maxpool_16_16": (MAX3S2, lambda c: _args(c, 16, 16, None, None, H=7, W=5)),
    "maxpool_16_16_pre_post_slice": (MAX3S2, lambda c: _args(c, 16, 16, PRE, POST16, H=7, W=5, ldo=c + 64, c_off=32)),
    "avgpool_16_8": (AVG3, lambda c: _args(c, 16, 8, PRE, POST8, H=5, W=4)),
    "global_16_8": (GLOBAL, lambda c: _args(c, 16, 8, None, POST8)),
}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_ok_accepts_every_description_kind_the_engine_uses(kind):
    op, make = KINDS[kind]
    for c in (64, 192, 256, 288, 768, 1280, 2048):
        for n in (1, 128):
            a = make(c)
            a.N = n
            assert _ok(a, op) == 1, (kind, c, n)


REFUSED = {
    "unknown_op_4": (4, lambda: _args(64)),
    "unknown_op_negative": (-1, lambda: _args(64)),
    "c_not_multiple_of_16": (REQUANT, lambda: _args(24, in_pitch=32, ldo=32)),
    "in_pitch_not_multiple_of_16": (REQUANT, lambda: _args(16, in_pitch=24)),
    "c_off_not_multiple_of_16": (REQUANT, lambda: _args(16, ldo=32, c_off=8)),
    "in_off_not_multiple_of_16": (REQUANT, lambda: _args(16, in_pitch=32, in_off=8)),
    "misaligned_in": (REQUANT, lambda: _args(64, in_ptr=BASE + 8)),
    "misaligned_out": (AVG3, lambda: _args(64, pre=PRE, out_ptr=BASE + 2048 + 2)),
    "null_in": (REQUANT, lambda: _args(64, in_ptr=0)),
    "out_slice_outside_row": (REQUANT, lambda: _args(64, ldo=96, c_off=48)),
    "in_slice_outside_row": (GLOBAL, lambda: _args(64, in_pitch=96, in_off=48)),
    "narrowing_without_post": (REQUANT, lambda: _args(64, 16, 8, None, None)),
    "post_clamp_outside_store": (REQUANT, lambda: _args(64, 16, 8, None, (5 << 27, 33, -129, 127))),
    "bad_widths": (REQUANT, lambda: _args(64, 32, 8)),
    "maxpool_map_smaller_than_window": (MAX3S2, lambda: _args(64, 16, 16, None, None, H=2, W=5)),
    "maxpool_pre_negative_multiplier": (MAX3S2, lambda: _args(64, 16, 16, (-(3 << 28), 30, -32768, 32767), POST16)),
    "maxpool_pre_small_exponent": (MAX3S2, lambda: _args(64, 16, 16, (3 << 10, 12, -32768, 32767), POST16)),
    "maxpool_pre_with_shift": (MAX3S2, lambda: _args(64, 16, 16, (3 << 28, 30 | 1 << 8, -32768, 32767), POST16)),
    "avgpool_pre_clamp_outside_int16": (AVG3, lambda: _args(64, 16, 8, (3 << 28, 30, -32768, 40000), POST8)),
    "global_sum_outside_int32": (GLOBAL, lambda: _args(64, 16, 8, None, POST8, H=32, W=32)),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refused_descriptions_launch_nothing_and_say_why(case):
    from hawq_amd import _lib
    op, make = REFUSED[case]
    a = make()
    lib = _lib.load()
    assert _ok(a, op) == 0
    rc = lib.hawq_incep_pool_v(C.byref(a), op, None)
    assert rc != 0
    msg = lib.hawq_last_error().decode()
    assert msg.startswith("hawq_incep_pool_v") and len(msg) > len("hawq_incep_pool_v (op 0): ")
    with pytest.raises(RuntimeError, match="hawq_incep_pool_v"):
        _lib.call("hawq_incep_pool_v", C.byref(a), op, None)


def test_the_conditions_are_not_stricter_than_stated():
    """the neighbours of the refusals above that the kernels do support"""
    assert _ok(_args(64, 16, 16, (3 << 28, 16, -32768, 32767), POST16, H=3, W=3), MAX3S2) == 1   # e1 == in_bits
    assert _ok(_args(64, 8, 8, (3 << 28, 8, -128, 127), (1 << 30, 31, -128, 127), H=3, W=4), MAX3S2) == 1
    assert _ok(_args(64, 16, 16, (-5, 3, -9, 9), POST16), REQUANT) == 1      # only the max pool needs a monotone pre
    assert _ok(_args(64, 16, 8, None, POST8, H=25, W=26), GLOBAL) == 1       # 650 pixels of 16 bits fit int32
    assert _ok(_args(64, 16, 8, None, POST8, H=25, W=27), GLOBAL) == 0
    assert _ok(_args(64, 8, 8, None, POST8, H=299, W=299), GLOBAL) == 1
    assert _ok(_args(48, 8, 16, None, None, in_pitch=64, in_off=16, ldo=96, c_off=48), REQUANT) == 1   # widening without post
