"""What the nibble InceptionV3 plan decides without a device: the storage policy (hawq_amd.engine_inception.nibble_storage) on hand-made
producer / consumer tables, and the refusals of hawq_incep_conv_nib_ok, which is host arithmetic on the argument block."""
import ctypes as C

import pytest

from hawq_amd import _lib
from hawq_amd.engine_inception import InceptionEngine, PlanNotApplicable, nibble_storage

R, U4, S8 = "requant", (0, 15), (-128, 127)
# (table of (lo, hi, producer, consumers), conv_ok, tensors stored hawq4)
TABLES = {
    # requant -> t0 -> conv0 -> t1 -> conv1: the whole branch
    "chain": ([(*U4, R, [0]), (0, 7, ("conv", 0), [1])], [True, True], {0, 1}),
    # conv1 is not a nibble conv: t1 stays int8, conv0 still reads nibbles
    "consumer_falls_back": ([(*U4, R, [0]), (0, 7, ("conv", 0), [1])], [True, False], {0}),
    # conv0 falls back: t0 is int8, so conv0 cannot write nibbles and t1 is int8 although conv1 would take them
    "producer_falls_back": ([(*U4, R, [0]), (0, 7, ("conv", 0), [1])], [False, True], set()),
    # one of two consumers (the 1x3 / 3x1 pair) falls back: the tensor does
    "any_consumer": ([(*U4, R, [0]), (0, 7, ("conv", 0), [1, 2])], [True, True, False], {0}),
    # a pool's output, signed values, 8-bit values, a tensor nobody reads
    "pool_producer": ([(*U4, None, [0])], [True], set()),
    "signed": ([(-8, 7, R, [0])], [True], set()),
    "eight_bit": ([(0, 255, R, [0])], [True], set()),
    "no_consumer": ([(*U4, R, [])], [], set()),
}


@pytest.mark.parametrize("name", list(TABLES))
def test_storage_policy(name):
    table, conv_ok, want = TABLES[name]
    assert nibble_storage(table, conv_ok) == want


def test_nibble_does_not_compose_with_grouped_or_fan_out():
    for kw in ({"grouped": True}, {"fan_out": True}):
        with pytest.raises(PlanNotApplicable, match="grouped or fan_out"):
            InceptionEngine(None, nibble=True, **kw)


def _block(**kw):
    a = _lib.IncepConvArgs()
    a.in_, a.wgt, a.bias, a.out, a.m, a.ek = (0x1000,) * 6   # never dereferenced
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride = 1, 8, 8, 1024, 128, 1, 1, 1
    a.epilogue, a.out_bits, a.ldo, a.q_hi, a.q2_hi = _lib.INCEP_REQUANT, 4, 128, 15, 15
    for k, v in kw.items():
        setattr(a, k, v)
    return a


# the largest K = KH KW Cin with 16 * 15 * 8 * K <= 2^31 - 1, in the multiples of 16 a 1x1 and a 7x7 window reach
K_LAST, K_LAST_7x7 = 1118480, 49 * 22816
REFUSED = [dict(in_=0x1008), dict(wgt=0x1004), dict(out=0x1008), dict(ldo=136), dict(c_off=8, ldo=144), dict(epilogue=_lib.INCEP_RAW),
           dict(q_hi=16), dict(q_lo=-1), dict(epilogue=_lib.INCEP_REQUANT2, q2_hi=16), dict(out_bits=12), dict(Cin=24), dict(KH=8),
           dict(Cin=K_LAST + 16), dict(KH=7, KW=7, pad_h=3, pad_w=3, Cin=22816 + 16), dict(m=None), dict(in_=None)]


def test_nib_ok_refusals_and_the_last_shape_every_tile_accepts():
    lib = _lib.load()
    tiles = range(1, lib.hawq_incep_conv_nib_num_tiles() + 1)
    ok = lambda a, t: lib.hawq_incep_conv_nib_ok(C.byref(a), t)   # noqa: E731
    assert all(ok(_block(), t) for t in tiles) and not ok(_block(), 0) and not ok(_block(), len(tiles) + 1)
    for kw in REFUSED:
        assert not any(ok(_block(**kw), t) for t in tiles), kw
    for last in (dict(Cin=K_LAST), dict(KH=7, KW=7, pad_h=3, pad_w=3, Cin=22816), dict(epilogue=_lib.INCEP_RAW, out_bits=32),
                 dict(out_bits=8, q_lo=-128, q_hi=127), dict(out_bits=16, q_lo=-32768, q_hi=32767),
                 dict(N=2 ** 15 - 1, H=2048, W=2048)):
        assert all(ok(_block(**last), t) for t in tiles), last
    assert K_LAST * 1920 <= 2 ** 31 - 1 < (K_LAST + 16) * 1920 and K_LAST_7x7 * 1920 <= 2 ** 31 - 1 < 49 * (22816 + 16) * 1920
    # each tile's own bound: tile 1 is for more than 64 output channels, the K-split tile for K >= 512
    assert [ok(_block(Cout=64, ldo=64), t) for t in tiles] == [0, 1, 1] and [ok(_block(Cout=80, ldo=80), t) for t in tiles] == [1, 1, 1]
    assert [ok(_block(Cin=496), t) for t in tiles] == [1, 1, 0] and [ok(_block(Cin=512), t) for t in tiles] == [1, 1, 1]
    assert not ok(_block(N=2 ** 15, H=2048, W=2048), 2)   # 2^37 pixels: 2^31 blocks of 64


# ---- the int32 bound, restated in tests/test_gpu_incep_nib_bound.py from the kernel's comment and not read from the library
def test_the_bound_is_the_pinned_one():
    from tests.test_gpu_incep_nib_bound import PINNED, WINDOWS, k_accepted, last_cin
    assert PINNED == {"1x1": (1118480, 1118480, 1118496), "7x7": (22816, 1117984, 22832)}
    for win, (last, K, first) in PINNED.items():
        KH, KW = WINDOWS[win][:2]
        assert last == last_cin(KH, KW) and K == KH * KW * last and first == last + 16
        assert k_accepted(KH, KW, last) and not k_accepted(KH, KW, first)
        assert 1920 * K <= 2 ** 31 - 1 < 1920 * KH * KW * first


def test_nib_ok_agrees_with_the_restated_bound_on_every_tile():
    from tests.test_gpu_incep_nib_bound import PINNED, shape
    from tests.test_gpu_incep_nib_kernels import RAW, _block as block
    lib = _lib.load()
    tiles = range(1, lib.hawq_incep_conv_nib_num_tiles() + 1)
    for win, (last, K, first) in PINNED.items():
        for cout, at_last in ((16, [0, 1, 1]), (80, [1, 1, 1])):   # tile 1 is for more than 64 channels; K >= 512: tile 3 takes it
            for cin, want in ((last, at_last), (first, [0, 0, 0])):
                g, N = shape(win, cin, cout)
                a = block(g, (0x1000,) * 6, RAW, 32, N=N)
                assert [lib.hawq_incep_conv_nib_ok(C.byref(a), t) for t in tiles] == want, (win, cout, cin)
        assert K >= 512


def test_group_nib_ok_applies_the_bound_to_hawq4_members_only():
    from tests.test_gpu_incep_group_nib_kernels import A, group
    from tests.test_gpu_incep_nib_bound import PINNED, shape
    from tests.test_gpu_incep_nib_kernels import RAW, _block as block
    lib = _lib.load()
    ok = lambda blocks, mask, tile: lib.hawq_incep_conv_group_nib_ok(C.byref(group(blocks)), mask, tile)   # noqa: E731
    # made-up addresses far apart: the first refused 1x1 input is 6.7 MB as int8
    small = block(A, (0x10000000, 0x100000, 0x200000, 0x20000000, 0x300000, 0x300000), RAW, 32)
    for win, (last, _, first) in PINNED.items():
        member = lambda cin: block(shape(win, cin, 16)[0], (0x30000000, 0x100000, 0x200000, 0x40000000, 0x300000, 0x300000), RAW, 32,   # noqa: E731
                                   N=shape(win, cin, 16)[1])
        for tile in (1, 2):
            assert ok([small, member(last)], 0b10, tile) and ok([small, member(last)], 0b11, tile)
            assert not ok([small, member(first)], 0b10, tile) and not ok([small, member(first)], 0b11, tile)
            assert ok([small, member(first)], 0b00, tile) and ok([small, member(first)], 0b01, tile)   # the same geometry as int8
