"""Host-side contract of the grouped InceptionV3 conv launch (hawq_incep_conv_group_ok, include/hawq_mi355.h), of the level schedule
(hawq_amd/engine_inception.py: unit_convs / conv_levels) and of the ``"groups"`` field of a conv tile plan (make_plan / check_groups).
Host-only functions on fabricated pointers, called through ctypes, and pure Python: no GPU needed."""
import ctypes as C
import json
import os
import re

import pytest

from hawq_amd import _lib
from hawq_amd.engine import StalePlan
from hawq_amd.engine_inception import InceptionEngine, check_groups, conv_levels, launch_digest, make_plan, unit_convs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("hawq_incep_conv_group_ok", "hawq_incep_conv_group")
R, RQ, RQ2 = _lib.INCEP_RAW, _lib.INCEP_REQUANT, _lib.INCEP_REQUANT2


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


class Fab:
    """fabricated, never dereferenced buffers: every ``buf()`` is `room` bytes away from the one before"""

    def __init__(self, room=1 << 28):
        self.room, self.next = room, 1 << 20

    def buf(self):
        self.next += self.room
        return self.next


def member(fab, H, W, cin, cout, kh=1, kw=1, ph=0, pw=0, stride=1, n=2, epilogue=RQ, out_bits=8, out=None, ldo=None, c_off=0, in_=None):
    a = _lib.IncepConvArgs()
    a.in_, a.wgt, a.bias, a.m, a.ek = (fab.buf() if in_ is None else in_), fab.buf(), fab.buf(), fab.buf(), fab.buf()
    a.out = fab.buf() if out is None else out
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad_h, a.pad_w = n, H, W, cin, cout, kh, kw, stride, ph, pw
    a.epilogue, a.relu, a.out_bits, a.ldo, a.c_off = epilogue, 1, out_bits, (cout if ldo is None else ldo), c_off
    lim = 127 if out_bits == 8 else 32767
    a.q_lo, a.q_hi, a.q2_lo, a.q2_hi = 0, lim, -lim, lim
    return a


def group(members):
    g = _lib.IncepGroupArgs()
    g.n = len(members)
    for i, a in enumerate(members[:_lib.INCEP_GROUP_MAX]):
        g.conv[i] = a
    return g


def ok(lib, members, tile):
    return lib.hawq_incep_conv_group_ok(C.byref(group(members)), tile)


def concat(fab, ldo, slices, H, W, cin, **kw):
    """1x1 REQUANT2 members writing the channel slices (c_off, cout) of one int16 buffer of pitch `ldo`"""
    out = fab.buf()
    return [member(fab, H, W, cin, co, epilogue=RQ2, out_bits=16, out=out, ldo=ldo, c_off=off, **kw) for off, co in slices]


def levels_1(fab):
    """level 1 of each unit type, as the plan builds it: the 1x1 branch and the pool branch's conv write slices of the unit's int16
    buffer, the first convs of the sequences write int8 buffers of their own"""
    a = concat(fab, 256, [(0, 64), (224, 32)], 35, 35, 192)
    b = concat(fab, 768, [(0, 192), (576, 192)], 17, 17, 768)
    c = concat(fab, 2048, [(0, 320), (1856, 192)], 8, 8, 1280)
    return {
        "A": [a[0], member(fab, 35, 35, 192, 48), member(fab, 35, 35, 192, 64), a[1]],
        "B": [b[0], member(fab, 17, 17, 768, 128), member(fab, 17, 17, 768, 128), b[1]],
        "C": [c[0], member(fab, 8, 8, 1280, 384), member(fab, 8, 8, 1280, 448), c[1]],
        "RA": [member(fab, 35, 35, 288, 384, 3, 3, stride=2, epilogue=RQ2, out_bits=16, ldo=768), member(fab, 35, 35, 288, 64)],
        "RB": [member(fab, 17, 17, 768, 192), member(fab, 17, 17, 768, 192)],
    }


def test_entry_points_are_declared_and_the_abi_is_unchanged(lib):
    header = open(os.path.join(ROOT, "include", "hawq_mi355.h")).read()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert "#define HAWQ_INCEP_GROUP_MAX 8" in header and _lib.INCEP_GROUP_MAX == 8
    assert lib.hawq_abi_version() == 5
    assert lib.hawq_incep_conv_num_tiles() == 4


def test_struct_size():
    assert C.sizeof(_lib.IncepGroupArgs) == 8 + 8 * C.sizeof(_lib.IncepConvArgs)
    assert _lib.IncepGroupArgs.conv.offset == 8


def test_accepts_level_1_of_every_unit_type_on_every_tile_its_members_accept(lib):
    for kind, ms in levels_1(Fab()).items():
        assert len(ms) == (4 if kind in "ABC" else 2)
        each = [t for t in range(1, 5) if all(lib.hawq_incep_conv_tile_ok(C.byref(a), t) for a in ms)]
        assert 3 in each, kind
        for t in range(1, 5):
            assert ok(lib, ms, t) == (1 if t in each else 0), (kind, t)
    # the 8 x 8 units' level 2: the 1x3 / 3x1 pair into the halves of its inner concat buffer and the other branch's 3x3
    fab = Fab()
    inner, x = fab.buf(), fab.buf()
    ms = [member(fab, 8, 8, 384, 384, 1, 3, 0, 1, epilogue=RQ2, out_bits=16, out=inner, ldo=768, c_off=0, in_=x),
          member(fab, 8, 8, 384, 384, 3, 1, 1, 0, epilogue=RQ2, out_bits=16, out=inner, ldo=768, c_off=384, in_=x),
          member(fab, 8, 8, 448, 384, 3, 3, 1, 1)]
    assert [ok(lib, ms, t) for t in range(1, 5)] == [1, 1, 1, 1]


def test_accepts_one_member_and_eight(lib):
    fab = Fab()
    ms = [member(fab, 5, 5, 16, 16) for _ in range(8)]
    assert ok(lib, ms[:1], 3) == 1 and ok(lib, ms, 3) == 1 and ok(lib, ms, 2) == 1
    g = group(ms[:3])   # blocks beyond n are ignored, whatever they hold
    g.conv[5].Cin = -7
    assert lib.hawq_incep_conv_group_ok(C.byref(g), 3) == 1


def test_refuses_no_member(lib):
    assert ok(lib, [], 3) == 0
    assert lib.hawq_incep_conv_group_ok(None, 3) == 0


def test_refuses_nine_members(lib):
    fab = Fab()
    g = group([member(fab, 5, 5, 16, 16) for _ in range(8)])
    assert lib.hawq_incep_conv_group_ok(C.byref(g), 3) == 1
    g.n = 9
    assert lib.hawq_incep_conv_group_ok(C.byref(g), 3) == 0
    g.n = -1
    assert lib.hawq_incep_conv_group_ok(C.byref(g), 3) == 0


def test_refuses_tiles_0_and_5(lib):
    ms = levels_1(Fab())["B"]
    assert ok(lib, ms, 3) == 1
    assert ok(lib, ms, 0) == 0 and ok(lib, ms, 5) == 0 and ok(lib, ms, -1) == 0


def test_refuses_tile_1_with_a_64_channel_member(lib):
    fab = Fab()
    ms = [member(fab, 35, 35, 192, 96), member(fab, 35, 35, 192, 64)]
    assert ok(lib, ms[:1], 1) == 1 and ok(lib, ms, 3) == 1
    assert ok(lib, ms, 1) == 0


def test_refuses_tile_4_with_a_short_k_member(lib):
    fab = Fab()
    ms = [member(fab, 8, 8, 512, 64), member(fab, 8, 8, 496, 64)]
    assert ok(lib, ms[:1], 4) == 1 and ok(lib, ms, 3) == 1
    assert ok(lib, ms, 4) == 0


def test_refuses_a_misaligned_slice(lib):
    fab = Fab()
    ms = concat(fab, 96, [(0, 32), (40, 48)], 8, 8, 64)
    assert [ok(lib, ms, t) for t in range(1, 5)] == [0, 0, 0, 0]
    assert ok(lib, concat(fab, 96, [(0, 32), (48, 48)], 8, 8, 64), 3) == 1


def test_refuses_overlapping_slices_of_one_buffer(lib):
    fab = Fab()
    assert ok(lib, concat(fab, 192, [(0, 64), (64, 96), (160, 32)], 8, 8, 64), 3) == 1
    assert ok(lib, concat(fab, 192, [(0, 64), (48, 96), (160, 32)], 8, 8, 64), 3) == 0
    assert ok(lib, concat(fab, 192, [(160, 32), (0, 64), (64, 112)], 8, 8, 64), 3) == 0
    assert ok(lib, concat(fab, 192, [(0, 64), (0, 64)], 8, 8, 64), 3) == 0


def test_refuses_overlapping_extents_of_two_buffers(lib):
    fab = Fab()
    n_bytes = 2 * 8 * 8 * 64   # an int8 output of N = 2, 8 x 8, 64 channels
    out = fab.buf()
    for shift, want in ((n_bytes, 1), (n_bytes - 16, 0), (16, 0), (-n_bytes + 16, 0), (-n_bytes, 1)):
        ms = [member(fab, 8, 8, 64, 64, out=out), member(fab, 8, 8, 64, 64, out=out + shift)]
        assert ok(lib, ms, 3) == want, shift
    # one buffer seen through two pitches is not a pair of slices
    ms = [member(fab, 8, 8, 64, 32, out=out, ldo=64, c_off=0), member(fab, 8, 8, 64, 32, out=out, ldo=128, c_off=32)]
    assert ok(lib, ms, 3) == 0


def test_refuses_a_member_that_reads_another_members_output(lib):
    fab = Fab()
    first = member(fab, 8, 8, 64, 64)
    assert ok(lib, [first, member(fab, 8, 8, 64, 64)], 3) == 1
    assert ok(lib, [first, member(fab, 8, 8, 64, 64, in_=first.out)], 3) == 0
    assert ok(lib, [member(fab, 8, 8, 64, 64, in_=first.out), first], 3) == 0
    assert ok(lib, [first, member(fab, 8, 8, 64, 64, in_=first.out + 2 * 8 * 8 * 64 - 16)], 3) == 0
    assert ok(lib, [first, member(fab, 8, 8, 64, 64, in_=first.out + 2 * 8 * 8 * 64)], 3) == 1


def test_refuses_two_to_the_31_workgroups(lib):
    fab = Fab(room=1 << 48)
    ms = [member(fab, 35, 35, 192, 192, n=1 << 24) for _ in range(8)]   # each: 1225 * 2^17 pixel blocks x 3 channel blocks
    assert all(lib.hawq_incep_conv_tile_ok(C.byref(a), 3) for a in ms)
    per = -(-(35 * 35 << 24) // 128) * 3
    assert 4 * per < 1 << 31 <= 8 * per
    assert ok(lib, ms[:4], 3) == 1 and ok(lib, ms, 3) == 0


# ---------------------------------------------------------------------- the level schedule
@pytest.fixture(scope="module", params=["uniform8", "uniform4"])
def model(request):
    from hawq_amd.api import build_quantized_resnet
    return build_quantized_resnet("inceptionv3", request.param, seed=0)


# level sizes per unit, in network order (the issue's table): 35^2 units, 35 -> 17, 17^2 units, 17 -> 8, 8^2 units
LEVEL_SIZES = [[4, 2, 1]] * 3 + [[2, 1, 1]] + [[4, 2, 2, 1, 1]] * 4 + [[2, 2, 1, 1]] + [[4, 3, 2]] * 2


def test_conv_levels_of_the_network(model):
    sizes = [[len(lv) for lv in conv_levels(u)] for _, u in model.units()]
    assert sizes == LEVEL_SIZES
    flat = [n for s in sizes for n in s]
    assert sum(1 for n in flat if n >= 2) == 27 and sum(n for n in flat if n >= 2) == 74 and flat.count(1) == 15
    assert sum(flat) + 5 + 1 == 95   # with the stem's convs and the classifier: the 95 conv launches of the plan


def test_every_conv_is_in_exactly_one_level_and_levels_respect_branch_order(model):
    from hawq_amd.q_inceptionv3 import Q_InceptConv
    for _, u in model.units():
        convs, levels = unit_convs(u), conv_levels(u)
        assert sorted(i for lv in levels for i in lv) == list(range(len(convs)))
        assert {id(ic) for ic, _, _ in convs} == {id(m) for m in u.modules() if isinstance(m, Q_InceptConv)} and len(convs) == len(
            {id(ic) for ic, _, _ in convs})
        for d, lv in enumerate(levels, 1):
            assert lv == sorted(lv)
            assert all(convs[i][2] == d for i in lv)
        for bi, br in enumerate(u.branches.children()):
            mine = [(ic, d) for ic, b, d in convs if b == bi]
            seq = list(br.q_conv_list) if hasattr(br, "q_conv_list") else ([br.q_conv] if hasattr(br, "q_conv") else [])
            assert [ic for ic, _ in mine[:len(seq)]] == seq and [d for _, d in mine[:len(seq)]] == list(range(1, len(seq) + 1))
            if hasattr(br, "q_conv1x3"):   # the pair shares the level after the branch's last sequential conv
                assert mine[len(seq):] == [(br.q_conv1x3, len(seq) + 1), (br.q_conv3x1, len(seq) + 1)]
            else:
                assert len(mine) == len(seq)


def test_the_option_needs_no_device(model):
    assert InceptionEngine(model, grouped=1).grouped is True and InceptionEngine(model).grouped is False
    assert InceptionEngine(model, grouped=True, tune=True, fast_pools=True, fused_stem=True).group_launches == []


# ---------------------------------------------------------------------- plans
KEYS = [(8, 8, 1280, 320, 1, 1, 1, 0, 0, 2, 16, 2048, 0), (8, 8, 1280, 384, 1, 1, 1, 0, 0, 1, 8, 384, 0),
        (8, 8, 384, 384, 1, 3, 1, 0, 1, 2, 16, 768, 0), (8, 8, 384, 384, 3, 1, 1, 1, 0, 2, 16, 768, 384),
        (8, 8, 1280, 448, 1, 1, 1, 0, 0, 1, 8, 448, 0), (8, 8, 448, 384, 3, 3, 1, 1, 1, 1, 8, 384, 0)]
LEVELS = [[0, 1, 4], [2, 3, 5]]
GROUPS = [{"convs": [4, 1, 0], "tile": 3, "us": {"3": 20.5, "4": 31.25, "singles": 44.0}},
          {"convs": [5, 2, 3], "tile": 4, "us": {"4": 18.0, "singles": 30.125}}]


def _plan(groups=GROUPS):
    return make_plan((1, 299, 299), KEYS, 4, [3, 3, 4, 4, 3, 4], [{0: 9.0 + i, 3: 8.0, 4: 8.5} for i in range(6)], groups)


def test_groups_survive_json_and_replay():
    plan = _plan()
    again = json.loads(json.dumps(plan))
    assert again == plan and again["groups"] == GROUPS
    seen = []
    got = check_groups(again["groups"], len(KEYS), LEVELS, lambda convs, tile: seen.append((tuple(convs), tile)) or True)
    assert got == [([4, 1, 0], 3), ([5, 2, 3], 4)] and seen == [((4, 1, 0), 3), ((5, 2, 3), 4)]
    assert check_groups([GROUPS[1]], len(KEYS), LEVELS, lambda c, t: True) == [([5, 2, 3], 4)]


def test_a_plan_without_groups_is_accepted_and_keeps_its_form():
    plain = make_plan((1, 299, 299), KEYS, 4, [3, 3, 4, 4, 3, 4], [{} for _ in KEYS])
    assert "groups" not in plain
    assert check_groups(plain.get("groups"), len(KEYS), LEVELS, lambda c, t: False) == []
    assert make_plan((1, 299, 299), KEYS, 4, [3, 3, 4, 4, 3, 4], [{} for _ in KEYS], [])["groups"] == []
    assert check_groups([], len(KEYS), LEVELS, lambda c, t: False) == []


def test_the_launch_digest_of_a_grouped_plan_is_the_ungrouped_one():
    with_groups, without = _plan(), _plan(None)
    assert with_groups["launches"] == without["launches"] == launch_digest(KEYS)
    assert {k: v for k, v in with_groups.items() if k != "groups"} == without


@pytest.mark.parametrize("groups,why", [
    ([{"convs": [0, 1, 6], "tile": 3}], "no conv launch 6"),
    ([{"convs": [0, 1, -1], "tile": 3}], "no conv launch -1"),
    ([{"convs": [0, 1, "4"], "tile": 3}], "no conv launch '4'"),
    ([{"convs": [0, 1, 4, 4], "tile": 3}], "named twice"),
    ([{"convs": [0, 1, 4], "tile": 3}, {"convs": [4, 1, 0], "tile": 3}], "named twice"),
    ([{"convs": [0, 1], "tile": 3}], "not one level"),
    ([{"convs": [0, 1, 4, 5], "tile": 3}], "not one level"),
    ([{"convs": [0, 1, 2], "tile": 3}], "not one level"),
    ([{"convs": [], "tile": 3}], "not one level"),
    ([{"convs": [0, 1, 4], "tile": 2}], "tile 2 is refused"),
    ([{"convs": [0, 1, 4], "tile": "3"}], "refused"),
    ([{"convs": [0, 1, 4]}], "not a list of conv groups"),
    ([[0, 1, 4]], "not a list of conv groups"),
    (7, "not a list of conv groups"),
])
def test_stale_groups_are_refused(groups, why):
    with pytest.raises(StalePlan, match=why):
        check_groups(groups, len(KEYS), LEVELS, lambda convs, tile: tile != 2)
