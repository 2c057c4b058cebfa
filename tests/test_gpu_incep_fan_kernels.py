"""The fan-out conv launch (hawq_amd/csrc/incep_fan.hip, hawq_incep_conv_group_fan) against the existing entry points on the same
inputs: hawq_incep_conv_tiled gives every member's primary output, and hawq_incep_requant on that output with the fan's table gives
every fan output (both are pinned to the CPU oracle by the Inception kernel and network tests).  Every byte of every output is
compared - the written slices, the channels around them (rows are wider than the slices and pre-filled) and the guard bands of
tests/guard.py.  The shapes are the smallest at which the kernel can still go wrong; each case runs on every tile that takes it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.guard import dev, guard_arena, out_buf  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

RAW, RQ, RQ2 = 0, 1, 2
SENTINEL = -77
# fan tables (m, ek, lo, hi), in the order a member's fan uses them.  On the outputs these cases make, each does what its name says
# through hawq_incep_requant alone, and the test asserts that before it compares anything.
TIES = (1 << 30, 32, 2, 20)                 # y / 4: an exact tie wherever y = 2 mod 4; a narrow clamp that saturates at both ends
SATURATE = (1 << 30, 29, 3, 100)            # 2 y: most of an int8 store's range is beyond hi, zeros are below lo
FOUR_BIT = (1 << 30, 33, 0, 15)             # y / 8 into the 4-bit range 0 .. 15
SHIFTED = (3 << 28, (2 << 8) | 34, -128, 127)   # the pre-shifted form: ((y << 2) * 0.75) / 16
SIGNED = (1 << 30, 32, -8, 7)               # for the relu = 0 member: saturates at a negative lo
TABLES = (TIES, SATURATE, FOUR_BIT, SHIFTED)


def _m(N, H, W, Cin, Cout, KH=1, KW=1, ph=0, pw=0, stride=1, epilogue=RQ, bits=8, n=0, relu=1, tables=TABLES, out=None, ldo=None,
       c_off=16, to=None, fan_ldo=None, fan_off=32):
    """a member: geometry, epilogue, its slice c_off .. c_off + Cout of rows of `ldo` elements (`out`: a name shared by the slices of
    one buffer), and `n` fan outputs with `tables`[:n] into slice fan_off .. of rows of `fan_ldo` int8 (`to`: the consumers' names)"""
    return dict(g=(N, H, W, Cin, Cout, KH, KW, ph, pw, stride), epilogue=epilogue, bits=bits, n=n, relu=relu, tables=tables[:n], out=out,
                ldo=Cout + 32 if ldo is None else ldo, c_off=c_off, to=to, fan_ldo=Cout + 48 if fan_ldo is None else fan_ldo, fan_off=fan_off)


# pixels: 25 (one partial block), 243 (two blocks of 128 with a ragged tail, one partial block of 256), 338 (two blocks of 256);
# Cout 16 / 48 / 80 (one 64-channel block plus a remainder; 80 is the smallest tile 1 takes); Cin 16 / 48: K no multiple of 64
CASES = {
    "rq_n0": [_m(1, 5, 5, 16, 16, n=0)],
    "rq2_n0": [_m(1, 5, 5, 16, 16, epilogue=RQ2, bits=16, n=0)],
    "rq_n1_25px": [_m(1, 5, 5, 16, 16, n=1)],
    "rq2_n3_243px": [_m(3, 9, 9, 48, 48, epilogue=RQ2, bits=16, n=3)],
    "rq2_n4_338px_c80": [_m(2, 13, 13, 16, 80, epilogue=RQ2, bits=16, n=4)],
    "rq_n4_3x3s2": [_m(3, 9, 9, 48, 80, 3, 3, 0, 0, 2, n=4)],
    "rq2_n1_1x7": [_m(2, 13, 13, 16, 48, 1, 7, 0, 3, epilogue=RQ2, bits=16, n=1)],
    "rq_n3_3x3_k576": [_m(3, 9, 9, 64, 48, 3, 3, 1, 1, n=3)],
    "rq2_n4_3x3_k576_c80": [_m(2, 13, 13, 64, 80, 3, 3, 1, 1, epilogue=RQ2, bits=16, n=4)],
    "rq_n3_signed": [_m(3, 9, 9, 48, 48, n=3, relu=0, tables=(SIGNED, SATURATE, SHIFTED))],
    # a level of a unit: an int8 conv of its own (no fan) and two slices of the concat buffer, whose producers write their channels of
    # the consumers X, Y (both) and Z (the second only); channels 0 .. 16, 64 .. 80 and 160 .. 192 of every row stay as they were
    "three_members": [_m(3, 9, 9, 48, 48, n=0),
                      _m(3, 9, 9, 48, 48, epilogue=RQ2, bits=16, n=2, out="cat", ldo=192, c_off=16, to=("X", "Y"), fan_ldo=192, fan_off=16),
                      _m(3, 9, 9, 16, 80, 1, 7, 0, 3, epilogue=RQ2, bits=16, n=3, out="cat", ldo=192, c_off=80, to=("X", "Y", "Z"),
                         fan_ldo=192, fan_off=80)],
}


def _lib():
    from hawq_amd import _lib
    return _lib


def _block(mb):
    a = _lib().IncepConvArgs()
    a.in_, a.wgt, a.bias, a.out, a.m, a.ek = 16, 16, 16, 16, 16, 16
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.pad_h, a.pad_w, a.stride = mb["g"]
    a.epilogue, a.relu, a.out_bits, a.ldo, a.c_off = mb["epilogue"], mb["relu"], mb["bits"], mb["ldo"], mb["c_off"]
    lim = (1 << (mb["bits"] - 1)) - 1
    a.q_lo, a.q_hi, a.q2_lo, a.q2_hi = (0 if mb["relu"] else -lim - 1), lim, -(lim + 1) // 2, lim // 2
    a.m2, a.ek2 = 5 << 27, 31   # the second requant: ratio 5 / 16
    return a


def _accepting_tiles(members):
    """host-only (no device): the tile ids every member accepts - the fabricated pointers are never dereferenced"""
    L = _lib().load()
    return [t for t in range(1, L.hawq_incep_conv_num_tiles() + 1) if all(L.hawq_incep_conv_tile_ok(C.byref(_block(m)), t) for m in members)]


PARAMS = [pytest.param(name, t, id=f"{name}-tile{t}") for name, ms in CASES.items() for t in _accepting_tiles(ms)]


def test_the_cases_reach_every_tile_and_every_fan_size():
    by_case = {name: [p.values[1] for p in PARAMS if p.values[0] == name] for name in CASES}
    assert all(3 in ts and 2 in ts for ts in by_case.values())
    assert by_case["rq_n3_3x3_k576"] == [2, 3, 4] and by_case["rq2_n4_3x3_k576_c80"] == [1, 2, 3, 4]
    assert by_case["rq2_n4_338px_c80"] == by_case["rq_n4_3x3s2"] == [1, 2, 3]
    for ep in (RQ, RQ2):
        assert {m["n"] for ms in CASES.values() for m in ms if m["epilogue"] == ep} >= {0, 1, 3, 4}
    assert [m["n"] for m in CASES["three_members"]] == [0, 2, 3]
    for ms in CASES.values():
        for m in ms:
            assert m["c_off"] > 0 and m["ldo"] > m["c_off"] + m["g"][4] and m["fan_off"] > 0 and m["fan_ldo"] > m["fan_off"] + m["g"][4]


def _dyadic(v, m, ek):
    """round_half_even(((v << k) * m) / 2^e) in exact integers, and where the ties were"""
    e, k = ek & 0xff, ek >> 8
    t = (v.astype(np.int64) << k) * np.int64(m)
    half = np.int64(1) << (e - 1)
    q, tie = (t + half) >> e, ((t + half) & ((np.int64(1) << e) - 1)) == 0
    return np.where(tie, q & ~np.int64(1), q), tie


def _out_hw(g):
    N, H, W, Cin, Cout, KH, KW, ph, pw, stride = g
    return (H + 2 * ph - KH) // stride + 1, (W + 2 * pw - KW) // stride + 1


@functools.lru_cache(maxsize=None)
def _operands(name):
    """per member (x, w, b, m, ek) on the host, made once per case and never changed"""
    from hawq_amd.quant_utils import requant_table
    gen = torch.Generator().manual_seed(7 + sum(map(ord, name)))
    ops = []
    for mb in CASES[name]:
        N, H, W, Cin, Cout, KH, KW = mb["g"][:7]
        x = torch.randint(-128, 128, (N, H, W, Cin), generator=gen, dtype=torch.int8)
        w = torch.randint(-128, 128, (Cout, KH, KW, Cin), generator=gen, dtype=torch.int8)
        b = torch.randint(-2 ** 20, 2 ** 20, (Cout,), generator=gen, dtype=torch.int32)
        s_w = torch.rand(Cout, generator=gen) * 1e-3 + 1e-4
        # acc + bias is about sqrt(K 74^4 + 2^40 / 3): an output scale that spreads it over the store, some of it into the clamp
        s_out = torch.tensor([0.02 * 6e-4 * (KH * KW * Cin * 5476. ** 2 + 2. ** 40 / 3) ** 0.5 * 2.5 / 2 ** (mb["bits"] - 1)])
        m, ek = requant_table(torch.tensor([0.02]), s_w, s_out, lift=False)
        ops.append((x.numpy(), w.numpy(), b.numpy(), np.asarray(m, np.int32), np.asarray(ek, np.int32)))
    return ops


class _Side:
    """the device buffers of one side (the fan launch, or the oracle): inputs, sentinel-filled primary outputs and fan outputs"""

    def __init__(self, name):
        self.members, self.prim, self.cons, self.args, self.keep = CASES[name], {}, {}, [], []
        for i, (mb, (x, w, b, m, ek)) in enumerate(zip(self.members, _operands(name))):
            Ho, Wo = _out_hw(mb["g"])
            P = mb["g"][0] * Ho * Wo
            key = mb["out"] or f"out{i}"
            if key not in self.prim:
                self.prim[key] = out_buf(P * mb["ldo"], torch.int8 if mb["bits"] == 8 else torch.int16, SENTINEL, key)
            for j in range(mb["n"]):
                ck = mb["to"][j] if mb["to"] else f"fan{i}.{j}"
                if ck not in self.cons:
                    self.cons[ck] = out_buf(P * mb["fan_ldo"], torch.int8, SENTINEL, ck)
            t = [dev(v) for v in (x, w, b, m, ek)]
            a = _block(mb)
            a.in_, a.wgt, a.bias, a.m, a.ek = (v.data_ptr() for v in t)
            a.out = self.prim[key].data_ptr()
            self.keep += t
            self.args.append(a)

    def consumer(self, i, j):
        mb = self.members[i]
        return self.cons[mb["to"][j] if mb["to"] else f"fan{i}.{j}"]

    def group(self):
        g = _lib().IncepGroupArgs()
        g.n = len(self.args)
        for i, a in enumerate(self.args):
            g.conv[i] = a
        fans = (_lib().IncepFan * len(self.args))()
        for i, mb in enumerate(self.members):
            fans[i].n = mb["n"]
            for j, (m, ek, lo, hi) in enumerate(mb["tables"]):
                f = fans[i].to[j]
                f.out, f.m, f.ek, f.lo, f.hi, f.ldo, f.c_off = self.consumer(i, j).data_ptr(), m, ek, lo, hi, mb["fan_ldo"], mb["fan_off"]
        return g, fans

    def requants(self):
        """the oracle's fan outputs: hawq_incep_requant from every member's slice of its primary output, per table"""
        out = []
        for i, (mb, a) in enumerate(zip(self.members, self.args)):
            Ho, Wo = _out_hw(mb["g"])
            for j, (m, ek, lo, hi) in enumerate(mb["tables"]):
                p = _lib().IncepPoolArgs()
                p.in_, p.out, p.N, p.H, p.W, p.C = a.out, self.consumer(i, j).data_ptr(), mb["g"][0], Ho, Wo, mb["g"][4]
                p.in_bits, p.in_pitch, p.in_off, p.out_bits, p.ldo, p.c_off = mb["bits"], mb["ldo"], mb["c_off"], 8, mb["fan_ldo"], mb["fan_off"]
                p.post, p.m2, p.ek2, p.lo2, p.hi2 = 1, m, ek, lo, hi
                out.append(p)
        return out


def _check_tables_bite(side):
    """the oracle's own outputs show ties and saturation at both ends, per member with a fan"""
    for i, mb in enumerate(side.members):
        if not mb["n"]:
            continue
        Ho, Wo = _out_hw(mb["g"])
        rows = side.prim[mb["out"] or f"out{i}"].cpu().numpy().reshape(-1, mb["ldo"])
        y = rows[:, mb["c_off"]:mb["c_off"] + mb["g"][4]].astype(np.int64)
        assert len(np.unique(y)) > 8 and (mb["relu"] or (y < 0).any())
        for j, (m, ek, lo, hi) in enumerate(mb["tables"]):
            want, tie = _dyadic(y, m, ek)
            got = side.consumer(i, j).cpu().numpy().reshape(-1, mb["fan_ldo"])[:, mb["fan_off"]:mb["fan_off"] + mb["g"][4]]
            assert np.array_equal(got, np.clip(want, lo, hi)), (i, j)   # hawq_incep_requant is the rule the fan restates
            if j == 0:   # TIES / SIGNED: exact ties inside the clamp, and both clamps used by values beyond them
                assert (tie & (want > lo) & (want < hi)).any() and (want < lo).any() and (want > hi).any(), (i, j)
            if (m, ek, lo, hi) == SATURATE:
                assert (want < lo).any() and (want > hi).any()
            if (m, ek, lo, hi) == FOUR_BIT:
                assert got.min() == 0 and got.max() == 15 and (want > 15).any()


@pytest.mark.parametrize("name,tile", PARAMS)
def test_fan_launch_equals_the_tiled_conv_and_the_requant_launches(guard_arena, name, tile):
    L = _lib().load()
    s = torch.cuda.current_stream().cuda_stream
    fan, ref = _Side(name), _Side(name)
    g, fans = fan.group()
    assert L.hawq_incep_conv_group_fan_ok(C.byref(g), fans, tile) == 1
    assert L.hawq_incep_conv_group_fan(C.byref(g), fans, tile, s) == 0, L.hawq_last_error()
    for a in ref.args:
        assert L.hawq_incep_conv_tiled(C.byref(a), tile, s) == 0, L.hawq_last_error()
    for p in ref.requants():
        assert L.hawq_incep_requant(C.byref(p), s) == 0, L.hawq_last_error()
    torch.cuda.synchronize()
    _check_tables_bite(ref)
    for key in ref.prim:   # whole buffers: the slices and the channels around them, which still hold what they were filled with
        assert torch.equal(fan.prim[key], ref.prim[key]), f"primary output {key} differs from hawq_incep_conv_tiled's"
    assert sorted(fan.cons) == sorted(ref.cons)
    for key in ref.cons:
        assert torch.equal(fan.cons[key], ref.cons[key]), f"fan output {key} differs from hawq_incep_requant's"
    written = {key: np.zeros(t.numel(), bool) for key, t in {**ref.prim, **ref.cons}.items()}
    for i, mb in enumerate(ref.members):
        written[mb["out"] or f"out{i}"].reshape(-1, mb["ldo"])[:, mb["c_off"]:mb["c_off"] + mb["g"][4]] = True
        for j in range(mb["n"]):
            key = mb["to"][j] if mb["to"] else f"fan{i}.{j}"
            written[key].reshape(-1, mb["fan_ldo"])[:, mb["fan_off"]:mb["fan_off"] + mb["g"][4]] = True
    for key, t in {**fan.prim, **fan.cons}.items():
        assert not written[key].all() and (t.cpu().numpy()[~written[key]] == SENTINEL).all(), key
    guard_arena.check()


def test_a_refused_description_is_an_error_and_writes_nothing(guard_arena):
    L = _lib().load()
    s = torch.cuda.current_stream().cuda_stream
    side = _Side("three_members")
    g, fans = side.group()
    assert L.hawq_incep_conv_group_fan_ok(C.byref(g), fans, 3) == 1
    fans[2].to[1].c_off = 32   # consumer Y: 32 .. 112 meets the second member's 16 .. 64
    for tile in (2, 3):
        assert L.hawq_incep_conv_group_fan_ok(C.byref(g), fans, tile) == 0
        assert L.hawq_incep_conv_group_fan(C.byref(g), fans, tile, s) != 0
        assert b"two fan outputs overlap" in L.hawq_last_error()
    fans[2].to[1].c_off = 80
    fans[1].to[0].hi = 128
    assert L.hawq_incep_conv_group_fan(C.byref(g), fans, 3, s) != 0 and b"clamp bounds" in L.hawq_last_error()
    fans[1].to[0].hi = 20
    assert L.hawq_incep_conv_group_fan(C.byref(g), fans, 0, s) != 0 and L.hawq_incep_conv_group_fan(C.byref(g), fans, 5, s) != 0
    fans[0].n = 5
    assert L.hawq_incep_conv_group_fan(C.byref(g), fans, 3, s) != 0
    torch.cuda.synchronize()
    for key, t in {**side.prim, **side.cons}.items():
        assert (t == SENTINEL).all(), key
    guard_arena.check()
