"""The band kernel's host side, no device: what hawq_incep_conv_band_ok (hawq_amd/csrc/incep_band.hip) accepts and refuses, and what a
plan's ``"stem_band"`` field may hold (hawq_amd/engine_inception.py: check_stem_band)."""
import ctypes as C
import os

import pytest

from hawq_amd import _lib
from hawq_amd.engine_inception import check_stem_band
from hawq_amd.plan import StalePlan

STEM = [(0, 149, 149, 32, 32), (1, 147, 147, 32, 64), (0, 73, 73, 80, 192)]   # (pad, H, W, Cin, Cout) of q_conv2, q_conv3, q_conv5


def _block(g=STEM[0], N=1, form=(1, 8), **changes):
    """a well-formed block on made-up addresses (nothing is dereferenced), with single fields changed"""
    pad, H, W, Cin, Cout = g
    a, lim = _lib.IncepConvArgs(), (127 if form[1] == 8 else 32767)
    a.in_, a.wgt, a.bias, a.out, a.m, a.ek = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad_h, a.pad_w = N, H, W, Cin, Cout, 3, 3, 1, pad, pad
    a.epilogue, a.out_bits, a.relu, a.ldo, a.c_off = form[0], form[1], 1, Cout + 32, 16
    a.q_lo, a.q_hi, a.m2, a.ek2, a.q2_lo, a.q2_hi = -lim - 1, lim, 1 << 30, 31, -lim - 1, lim
    for k, v in changes.items():
        setattr(a, k, v)
    return a


def test_both_names_are_declared_listed_and_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hawq_mi355.h")).read()
    for name in ("hawq_incep_conv_band_ok", "hawq_incep_conv_band"):
        assert f"int {name}(const hawq_incep_conv_args *a" in header and name in _lib.SIGNATURES and hasattr(_lib.load(), name)


@pytest.mark.parametrize("N", [1, 128])
@pytest.mark.parametrize("form", [(1, 8), (1, 16), (2, 16), (0, 32)], ids=str)   # (epilogue, out_bits)
@pytest.mark.parametrize("g", STEM, ids=str)
def test_the_stem_geometries_are_accepted(g, form, N):
    assert _lib.load().hawq_incep_conv_band_ok(C.byref(_block(g, N, form))) == 1


@pytest.mark.parametrize("changes", [
    dict(KH=1, KW=1), dict(KH=5, KW=5), dict(KH=1, KW=3), dict(stride=2), dict(pad_h=2, pad_w=2), dict(pad_h=1, pad_w=0),
    dict(Cin=112), dict(Cin=24), dict(Cout=40), dict(ldo=72), dict(c_off=8), dict(in_=0x10008), dict(wgt=0x20004), dict(out=0x40002),
    dict(out_bits=4), dict(epilogue=0, out_bits=8), dict(m=None), dict(ek=None),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_single_field_changes_are_refused(changes):
    L = _lib.load()
    assert L.hawq_incep_conv_band_ok(C.byref(_block(**changes))) == 0
    assert L.hawq_incep_conv_band(C.byref(_block(**changes)), None) != 0 and L.hawq_last_error()   # refused before any launch


def test_the_plan_check():
    stem, ok = [0, 1, 2, 3, 4], lambda c: c in (1, 2, 4)
    assert check_stem_band([1, 2, 4], stem, ok) == [1, 2, 4] and check_stem_band([4], stem, ok) == [4]
    assert check_stem_band(None, stem, ok) == [] and check_stem_band([], stem, ok) == []
    for bad in ([1, 7], [3], [1, 1], [True], "12", {"convs": [1]}):
        with pytest.raises(StalePlan):
            check_stem_band(bad, stem, ok)
