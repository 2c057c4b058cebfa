"""The fused average pool + 1x1 conv kernel's host side, no device: what hawq_incep_avgpool_conv_ok (hawq_amd/csrc/incep_pool_conv.hip)
accepts and refuses, and what a plan's ``"pool_conv"`` field may hold (hawq_amd/engine_inception.py: check_pool_conv)."""
import ctypes as C
import os

import pytest

from hawq_amd import _lib

NAMES = ("hawq_incep_avgpool_conv_ok", "hawq_incep_avgpool_conv")
# (H = W, C, Cout) of the nine average-pool branches: Inception-A x3, -B x4, -C x2
BRANCHES = [(35, 192, 32), (35, 256, 64), (35, 288, 64)] + [(17, 768, 192)] * 4 + [(8, 1280, 192), (8, 2048, 192)]


def _pair(g=BRANCHES[0], n=1, pool=None, **conv):
    """well-formed blocks on made-up addresses (nothing is dereferenced), with single fields changed; the ignored fields are 0"""
    hw, Cc, Cout = g
    p, c = _lib.IncepPoolArgs(), _lib.IncepConvArgs()
    p.in_, (p.N, p.H, p.W, p.C), (p.in_bits, p.in_pitch, p.in_off, p.out_bits) = 0x10000, (n, hw, hw, Cc), (16, Cc + 32, 16, 8)
    (p.pre, p.m1, p.ek1, p.lo1, p.hi1), (p.post, p.m2, p.ek2, p.lo2, p.hi2) = (1, 1 << 30, 31, -32768, 32767), (1, 1 << 30, 31, -128, 127)
    c.wgt, c.bias, c.out, c.m, c.ek = 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    c.N, c.H, c.W, c.Cin, c.Cout, c.KH, c.KW, c.stride = n, hw, hw, Cc, Cout, 1, 1, 1
    c.epilogue, c.out_bits, c.relu, c.ldo, c.c_off = 2, 16, 1, Cout + 32, 16
    c.q_lo, c.q_hi, c.m2, c.ek2, c.q2_lo, c.q2_hi = -32768, 32767, 1 << 30, 31, -32768, 32767
    for block, changes in ((p, pool or {}), (c, conv)):
        for k, v in changes.items():
            setattr(block, k, v)
    return C.byref(p), C.byref(c)


def test_both_names_are_declared_listed_and_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hawq_mi355.h")).read()
    for name in NAMES:
        assert f"int {name}(const hawq_incep_pool_args *p, const hawq_incep_conv_args *c" in header
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)


@pytest.mark.parametrize("N", [1, 128])
@pytest.mark.parametrize("g", sorted(set(BRANCHES)), ids=str)
def test_the_shipped_branches_are_accepted(g, N):
    assert _lib.load().hawq_incep_avgpool_conv_ok(*_pair(g, N)) == 1


# the clause a case is meant to hit, by a word of its reason -> (pool changes, conv changes)
VIOLATIONS = {
    "1x1": [({}, dict(KH=3, KW=3, pad_h=1, pad_w=1)), ({}, dict(stride=2)), ({}, dict(pad_h=1))],
    "does not read": [({}, dict(N=2)), ({}, dict(H=34)), ({}, dict(Cin=208))],
    "pooled tensor": [(dict(out_bits=16), {})], "pre clamp": [(dict(lo1=-32769), {})], "post clamp": [(dict(hi2=128), {})],
    "in_bits": [(dict(in_bits=32), {})],
    "multiples of 16": [(dict(C=200), dict(Cin=200)), (dict(in_pitch=232), {}), (dict(in_off=8), {}), ({}, dict(Cout=40)),
                        ({}, dict(ldo=72)), ({}, dict(c_off=8))],
    "ldo < c_off": [({}, dict(ldo=32))],
    "aligned": [(dict(in_=0x10008), {}), ({}, dict(wgt=0x20004)), ({}, dict(out=0x40002))],
    "only the REQUANT": [({}, dict(epilogue=0, out_bits=32))], "out_bits must be 8 or 16": [({}, dict(out_bits=32))],
    "192 output channels": [({}, dict(Cout=208, ldo=256))],
    "wider": [(dict(W=111), dict(W=111)), (dict(W=63), dict(W=63, Cout=80, ldo=112))],   # the limits of Cout <= 64 and of Cout > 64
    "workgroups": [(dict(N=1 << 30), dict(N=1 << 30))],
}


@pytest.mark.parametrize("why,pool,conv", [(w, *case) for w, cases in VIOLATIONS.items() for case in cases],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()) or "-" if isinstance(d, dict) else d)
def test_single_contract_violations_are_refused_with_their_reason(why, pool, conv):
    L = _lib.load()
    assert L.hawq_incep_avgpool_conv_ok(*_pair(pool=pool, **conv)) == 0 and why.encode() in L.hawq_last_error()
    assert L.hawq_incep_avgpool_conv(*_pair(pool=pool, **conv), None) != 0   # refused before any launch


@pytest.mark.parametrize("W,Cout", [(110, 64), (62, 192)])
def test_the_widest_maps_are_accepted(W, Cout):
    assert _lib.load().hawq_incep_avgpool_conv_ok(*_pair(pool=dict(W=W), W=W, Cout=Cout, ldo=Cout + 32)) == 1


def test_the_plan_check():
    from hawq_amd.engine_inception import check_pool_conv
    from hawq_amd.plan import StalePlan
    cands, ok = [9, 16], lambda c: c == 9
    assert check_pool_conv([9], cands, ok) == [9] and check_pool_conv([16, 9], cands, lambda c: True) == [16, 9]
    assert check_pool_conv(None, cands, ok) == [] and check_pool_conv([], cands, ok) == []
    for bad in ("9", {"convs": [9]}, [9, 9], [1], [True], [9, 16]):   # no list, named twice, no candidate (twice), refused
        with pytest.raises(StalePlan):
            check_pool_conv(bad, cands, ok)
