"""The fused conv + max pool kernel's host side, no device: what hawq_incep_conv_band_pool_ok (hawq_amd/csrc/incep_band_pool.hip)
accepts and refuses, and what a plan's ``"stem_pool"`` field may hold (hawq_amd/engine_inception.py: check_stem_pool)."""
import ctypes as C
import os

import pytest

from hawq_amd import _lib
from tests.test_incep_band_host import _block

NAMES = ("hawq_incep_conv_band_pool_ok", "hawq_incep_conv_band_pool")
# (pad, H, W, Cin, Cout): q_conv3, q_conv5 and the small shapes of the device test
SHAPES = [(1, 147, 147, 32, 64), (0, 73, 73, 80, 192), (0, 5, 5, 16, 16), (1, 3, 3, 96, 208), (1, 12, 14, 32, 48), (0, 11, 13, 80, 80),
          (1, 12, 14, 64, 96), (0, 41, 5, 16, 32), (1, 3, 70, 48, 16)]


def test_both_names_are_declared_listed_and_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hawq_mi355.h")).read()
    for name in NAMES:
        assert f"int {name}(const hawq_incep_conv_args *a" in header and name in _lib.SIGNATURES and hasattr(_lib.load(), name)


@pytest.mark.parametrize("N", [1, 128])
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("g", SHAPES, ids=str)
def test_the_stem_pairs_and_the_small_shapes_are_accepted(g, bits, N):
    assert _lib.load().hawq_incep_conv_band_pool_ok(C.byref(_block(g, N, (1, bits)))) == 1


@pytest.mark.parametrize("changes", [
    dict(stride=2), dict(KH=1, KW=1), dict(Cin=112), dict(pad_h=1, pad_w=0), dict(epilogue=0, out_bits=32), dict(epilogue=2),
    dict(out_bits=32), dict(H=4), dict(ldo=32),dict(out=0x40002), dict(c_off=8),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_single_field_changes_are_refused_with_a_reason(changes):
    L = _lib.load()   # the block is q_conv2's (pad 0), so H = 4 gives Ho = 2
    assert L.hawq_incep_conv_band_pool_ok(C.byref(_block(**changes))) == 0 and b"band_pool" in L.hawq_last_error()
    assert L.hawq_incep_conv_band_pool(C.byref(_block(**changes)), None) != 0   # refused before any launch


def test_the_plan_check():
    from hawq_amd.engine_inception import check_stem_pool
    from hawq_amd.plan import StalePlan
    cands, ok = [2, 4], lambda c: c == 2
    assert check_stem_pool([2], cands, ok) == [2] and check_stem_pool([4, 2], cands, lambda c: True) == [4, 2]
    assert check_stem_pool(None, cands, ok) == [] and check_stem_pool([], cands, ok) == []
    for bad in ("24", {"convs": [2]}, [2, 2], [1], [True], [2, 4]):   # no list, named twice, no candidate (twice), refused
        with pytest.raises(StalePlan):
            check_stem_pool(bad, cands, ok)
