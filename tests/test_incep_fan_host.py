"""Host-side contract of the fan-out conv launch (hawq_incep_conv_group_fan_ok, include/hawq_mi355.h), of the boundary function over the
launch records (hawq_amd/engine_inception.py: fan_boundaries) and of the ``"fan_out"`` field of a conv tile plan (make_plan /
check_fan_out).  Host-only functions on fabricated pointers, called through ctypes, and pure Python: no GPU needed."""
import ctypes as C
import json
import os
import re

import pytest

from hawq_amd import _lib
from hawq_amd.engine import StalePlan
from hawq_amd.engine_inception import InceptionEngine, Launch, check_fan_out, fan_boundaries, fan_key, make_plan
from tests.test_incep_group_host import KEYS, Fab, concat, group, levels_1, member

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, RQ, RQ2 = _lib.INCEP_RAW, _lib.INCEP_REQUANT, _lib.INCEP_REQUANT2
TABLE = dict(m=5 << 27, ek=31, lo=-128, hi=127)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def fans(*per_member):
    """an array of hawq_incep_fan: per member a list of dicts with the fields of hawq_incep_fan_out (TABLE where not given)"""
    arr = (_lib.IncepFan * max(len(per_member), 1))()
    for i, outs in enumerate(per_member):
        arr[i].n = len(outs)
        for j, o in enumerate(outs[:_lib.INCEP_FAN_MAX]):
            for k, v in {**TABLE, **o}.items():
                setattr(arr[i].to[j], k, v)
    return arr


def ok(lib, members, fan, tile=3):
    return lib.hawq_incep_conv_group_fan_ok(C.byref(group(members)), fan, tile)


def why(lib, members, fan, tile=3):
    """the reason the launch itself gives for refusing (it checks before it touches the device, so none is needed)"""
    assert ok(lib, members, fan, tile) == 0
    assert lib.hawq_incep_conv_group_fan(C.byref(group(members)), fan, tile, None) != 0
    return lib.hawq_last_error().decode()


def consumer(fab, n, ldo):
    """n consumer buffers (int8 rows of ldo channels) as fan outputs into channel slice c_off"""
    outs = [fab.buf() for _ in range(n)]
    return lambda c_off, **kw: [dict(out=o, ldo=ldo, c_off=c_off, **kw) for o in outs]


def test_entry_points_are_declared_and_the_abi_is_unchanged(lib):
    header = open(os.path.join(ROOT, "include", "hawq_mi355.h")).read()
    for name in ("hawq_incep_conv_group_fan_ok", "hawq_incep_conv_group_fan"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert "#define HAWQ_INCEP_FAN_MAX 4" in header and _lib.INCEP_FAN_MAX == 4
    assert lib.hawq_abi_version() == 5


def test_structs_match_the_header_layout(tmp_path):
    import subprocess
    structs = {"hawq_incep_fan_out": _lib.IncepFanOut, "hawq_incep_fan": _lib.IncepFan}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "hawq_mi355.h")}"', 'int main(void) {']
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ['return 0; }']))
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    assert C.sizeof(_lib.IncepFanOut) == 32 and C.sizeof(_lib.IncepFan) == 136
    # the whole argument list of the kernel: the group, its grid map (4 x 8 int32) and eight fans
    assert C.sizeof(_lib.IncepGroupArgs) + 128 + 8 * C.sizeof(_lib.IncepFan) == 2312 <= 4096


def test_accepts_groups_of_one_and_three_with_fans_of_0_2_and_4(lib):
    fab = Fab()
    one = concat(fab, 256, [(64, 64)], 35, 35, 192)
    to = consumer(fab, 4, 256)
    for n in (0, 1, 2, 3, 4):
        for t in (2, 3):
            assert ok(lib, one, fans(to(64)[:n]), t) == 1, (n, t)
    assert ok(lib, [member(fab, 35, 35, 192, 64)], fans(to(64)[:3])) == 1   # an int8 REQUANT member
    a, b = concat(fab, 768, [(0, 192), (576, 192)], 17, 17, 768)
    three = [a, member(fab, 17, 17, 768, 128), b]
    f = fans(to(0)[:2], [], [dict(o, ldo=768) for o in consumer(fab, 4, 768)(576)])
    assert [ok(lib, three, f, t) for t in range(1, 5)] == [1, 1, 1, 1]
    # slices of shared consumer buffers: both members write every consumer, in their own channels
    shared = consumer(fab, 3, 768)
    assert ok(lib, three, fans(shared(0), [], shared(576))) == 1
    assert ok(lib, three, fans(shared(0), [], shared(192))) == 1   # touching, not overlapping


def test_with_no_fan_it_agrees_with_the_grouped_launch(lib):
    for kind, ms in levels_1(Fab()).items():
        for t in range(0, 6):
            assert ok(lib, ms, fans(*[[] for _ in ms]), t) == lib.hawq_incep_conv_group_ok(C.byref(group(ms)), t), (kind, t)
    fab = Fab()
    bad = concat(fab, 192, [(0, 64), (48, 96)], 8, 8, 64)
    assert ok(lib, bad, fans([], [])) == 0 and "hawq_incep_conv_group_ok" in why(lib, bad, fans([], []))
    assert lib.hawq_incep_conv_group_fan_ok(None, fans([]), 3) == 0
    assert lib.hawq_incep_conv_group_fan_ok(C.byref(group(bad[:1])), None, 3) == 0


def test_refusals_name_their_reason(lib):
    fab = Fab()
    ms = concat(fab, 256, [(64, 64)], 35, 35, 192)
    to = consumer(fab, 5, 256)
    good = to(64)
    assert ok(lib, ms, fans(good[:4])) == 1
    f = fans(good[:4])
    f[0].n = 5
    assert "0 .. 4 fan outputs" in why(lib, ms, f)
    f[0].n = -1
    assert "0 .. 4 fan outputs" in why(lib, ms, f)
    raw = [member(fab, 8, 8, 64, 64, epilogue=R, out_bits=32)]
    assert ok(lib, raw, fans([])) == 1
    assert "RAW member" in why(lib, raw, fans([dict(out=fab.buf(), ldo=64, c_off=0)]))
    assert "clamp bounds" in why(lib, ms, fans([dict(good[0], hi=128)]))
    assert "clamp bounds" in why(lib, ms, fans([dict(good[0], lo=-129)]))
    assert "clamp bounds" in why(lib, ms, fans([dict(good[0], lo=8, hi=7)]))
    assert ok(lib, ms, fans([dict(good[0], lo=7, hi=7)])) == 1
    for ek in (0, 63, 16 << 8 | 31, -1):
        assert "dyadic form" in why(lib, ms, fans([dict(good[0], ek=ek)])), ek
    assert ok(lib, ms, fans([dict(good[0], ek=62)])) == 1 and ok(lib, ms, fans([dict(good[0], ek=15 << 8 | 1)])) == 1
    assert "dyadic form" in why(lib, ms, fans([dict(good[0], m=-1)]))
    assert "16-byte" in why(lib, ms, fans([dict(good[0], out=good[0]["out"] + 8)]))
    assert "16-byte" in why(lib, ms, fans([dict(good[0], ldo=264)]))
    assert "16-byte" in why(lib, ms, fans([dict(good[0], c_off=72)]))
    assert "16-byte" in why(lib, ms, fans([dict(good[0], c_off=-16)]))
    assert "null fan output" in why(lib, ms, fans([dict(good[0], out=None)]))
    assert "ldo < c_off + Cout" in why(lib, ms, fans([dict(good[0], c_off=208)]))
    assert ok(lib, ms, fans([dict(good[0], c_off=192)])) == 1
    for tile in (0, 5, -1):
        assert "no such tile" in why(lib, ms, fans(good[:1]), tile)
    assert "tile 3 refuses the launch (member 0, fan output 2)" in why(lib, ms, fans(good[:2] + [dict(good[2], hi=128)]))


def test_refuses_overlapping_buffers(lib):
    fab = Fab()
    a, b = concat(fab, 768, [(0, 192), (576, 192)], 17, 17, 768)
    to = consumer(fab, 2, 768)
    assert ok(lib, [a, b], fans(to(0), to(576))) == 1
    # a fan output over a member's input (its own, and the other member's)
    assert "member's input" in why(lib, [a, b], fans([dict(out=a.in_, ldo=768, c_off=0)], []))
    assert "member's input" in why(lib, [a, b], fans([dict(out=b.in_ + 2 * 17 * 17 * 768 - 16, ldo=768, c_off=0)], []))
    assert ok(lib, [a, b], fans([dict(out=b.in_ + 2 * 17 * 17 * 768, ldo=768, c_off=0)], [])) == 1
    # over a member's primary output: byte extents for the int16 concat buffer, channel intervals inside one int8 buffer
    assert "primary output" in why(lib, [a, b], fans([dict(out=a.out, ldo=768, c_off=0)], []))
    assert "primary output" in why(lib, [a, b], fans([], [dict(out=a.out + 1024, ldo=768, c_off=0)]))
    x = fab.buf()
    p8 = [member(fab, 8, 8, 64, 32, out=x, ldo=128, c_off=0), member(fab, 8, 8, 64, 32, out=x, ldo=128, c_off=64)]
    assert ok(lib, p8, fans([dict(out=x, ldo=128, c_off=32)], [dict(out=x, ldo=128, c_off=96)])) == 1
    assert "primary output" in why(lib, p8, fans([dict(out=x, ldo=128, c_off=48)], []))
    assert "primary output" in why(lib, p8, fans([dict(out=x, ldo=64, c_off=32)], []))   # another pitch: byte extents
    # over another fan output, in the same buffer (channel intervals) ...
    assert "two fan outputs overlap" in why(lib, [a, b], fans(to(0), to(176)))
    assert "two fan outputs overlap" in why(lib, [a, b], fans(to(0), to(0)))
    assert "two fan outputs overlap" in why(lib, [a, b], fans(to(0)[:1] * 2, []))   # one member, the same target twice
    assert ok(lib, [a, b], fans(to(0), to(192))) == 1
    # ... and in different buffers (byte extents)
    o = to(0)[0]["out"]
    n_bytes = (2 * 17 * 17 - 1) * 768 + 192
    for shift, want in ((n_bytes, 1), (n_bytes - 16, 0), (16, 0), (-n_bytes + 16, 0), (-n_bytes, 1)):
        f = fans([dict(out=o, ldo=768, c_off=0)], [dict(out=o + shift, ldo=768, c_off=0)])
        assert ok(lib, [a, b], f) == want, shift
        assert want or "two fan outputs overlap" in why(lib, [a, b], f)


# ---------------------------------------------------------------------- the boundary function, on hand-written records
POST = (3 << 28, 30, -127, 127)


def _conv(fab, place, level, ref, out, ldo, c_off, cout, epilogue=RQ2, out_bits=16):
    a = member(fab, 17, 17, 64, cout, epilogue=epilogue, out_bits=out_bits, out=out, ldo=ldo, c_off=c_off)
    return Launch("hawq_incep_conv", (a,), "conv", ref, place, level)


def _pool(name, place, level, src, pitch, out, ldo, c_off, c, in_bits=16, out_bits=16, post=None):
    a = _lib.IncepPoolArgs()
    a.in_, a.out, a.N, a.H, a.W, a.C = src, out, 2, 17, 17, c
    a.in_bits, a.in_pitch, a.in_off, a.out_bits, a.ldo, a.c_off = in_bits, pitch, 0, out_bits, ldo, c_off
    if post:
        a.post, (a.m2, a.ek2, a.lo2, a.hi2) = 1, post
    return Launch(name, (a,), "pool", _lib.INCEP_POOL_OPS[name], place, level)


def _entry(place, src, pitch, outs, tables=None):
    return [_pool("hawq_incep_requant", place, 0, src, pitch, o, pitch, 0, pitch, out_bits=8, post=(tables or [POST] * len(outs))[i])
            for i, o in enumerate(outs)]


def test_boundary_of_a_unit_fed_only_by_convs():
    fab = Fab()
    stem, cat, outs = fab.buf(), fab.buf(), [fab.buf(), fab.buf(), fab.buf()]
    tables = [(3 << 28, 30, -127, 127), (5 << 27, 31, 0, 15), (1 << 30, 32, -8, 7)]
    recs = [_pool("hawq_incep_maxpool3s2", "stem", 0, fab.buf(), 192, stem, 192, 0, 192)]
    recs += _entry(0, stem, 192, [fab.buf()])
    recs += [_conv(fab, 0, 1, 0, cat, 256, 0, 64), _conv(fab, 0, 1, 1, fab.buf(), 48, 0, 48, RQ, 8), _conv(fab, 0, 2, 2, cat, 256, 64, 96),
             _conv(fab, 0, 1, 3, cat, 256, 160, 96)]
    recs += _entry(1, cat, 256, outs, tables)
    recs += [_conv(fab, 1, 1, 4, fab.buf(), 256, 0, 64)]
    b0, b1 = fan_boundaries(recs)
    assert (b0["unit"], b0["requants"], b0["candidate"], b0["producers"]) == (0, [1], False, {})   # fed only by a pool
    assert b0["slices"] == [(0, 192, None)] and b0["residual"] == [(0, 192)]
    assert (b1["unit"], b1["requants"], b1["candidate"], b1["residual"]) == (1, [6, 7, 8], True, [])
    assert b1["slices"] == [(0, 64, 2), (64, 96, 4), (160, 96, 5)]
    assert sorted(b1["producers"]) == [2, 4, 5]
    for i, (c_off, cout) in ((2, (0, 64)), (4, (64, 96)), (5, (160, 96))):
        assert b1["producers"][i] == [(outs[j], 256, tables[j], c_off, cout) for j in range(3)]


def test_boundary_with_a_pool_slice_and_with_two_adjacent_ones():
    fab = Fab()
    prev, cat, outs = fab.buf(), fab.buf(), [fab.buf(), fab.buf()]
    recs = [_conv(fab, 3, 1, 0, cat, 768, 0, 384), _conv(fab, 3, 3, 1, cat, 768, 384, 96),
            _pool("hawq_incep_maxpool3s2", 3, 0, prev, 288, cat, 768, 480, 288)]
    recs += _entry(4, cat, 768, outs)
    (b3, b4) = fan_boundaries(recs)
    assert b3["requants"] == [] and not b3["candidate"]
    assert b4["candidate"] and b4["slices"] == [(0, 384, 0), (384, 96, 1), (480, 288, None)]
    assert b4["residual"] == [(480, 288)]   # exactly the pool's slice
    assert b4["producers"] == {0: [(o, 768, POST, 0, 384) for o in outs], 1: [(o, 768, POST, 384, 96) for o in outs]}
    # an 8 x 8 unit: a conv, two inner-concat requants next to each other, a conv
    fab = Fab()
    cat, inner = fab.buf(), [fab.buf(), fab.buf()]
    recs = [_conv(fab, 9, 1, 0, cat, 2048, 0, 320), _conv(fab, 9, 2, 1, inner[0], 768, 0, 384), _conv(fab, 9, 2, 2, inner[0], 768, 384, 384),
            _pool("hawq_incep_requant", 9, 2, inner[0], 768, cat, 2048, 320, 768, post=POST),
            _pool("hawq_incep_requant", 9, 3, inner[1], 768, cat, 2048, 1088, 768, post=POST),
            _conv(fab, 9, 1, 3, cat, 2048, 1856, 192)]
    recs += _entry(10, cat, 2048, [fab.buf()])
    b10 = fan_boundaries(recs)[-1]
    assert b10["unit"] == 10 and b10["candidate"] and sorted(b10["producers"]) == [0, 5]
    assert b10["slices"] == [(0, 320, 0), (320, 768, None), (1088, 768, None), (1856, 192, 5)]
    assert b10["residual"] == [(320, 1536)]   # the two requants' slices, merged
    # two separate non-conv ranges stay two
    recs = [_pool("hawq_incep_maxpool3s2", 1, 0, fab.buf(), 64, cat, 256, 0, 64), _conv(fab, 1, 1, 0, cat, 256, 64, 64),
            _pool("hawq_incep_maxpool3s2", 1, 0, fab.buf(), 128, cat, 256, 128, 128)] + _entry(2, cat, 256, [fab.buf()])
    assert fan_boundaries(recs)[-1]["residual"] == [(0, 64), (128, 128)]


def test_a_boundary_whose_entry_requants_are_not_plain_is_no_candidate():
    fab = Fab()
    cat = fab.buf()
    for change in ("pre", "in_off", "out_bits"):
        recs = [_conv(fab, 0, 1, 0, cat, 64, 0, 64)] + _entry(1, cat, 64, [fab.buf()])
        assert fan_boundaries(recs)[-1]["candidate"]
        setattr(recs[-1].args[0], change, 16)
        b = fan_boundaries(recs)[-1]
        assert not b["candidate"] and b["producers"] == {}, change
    # a REQUANT (not REQUANT2) conv, or a conv into another buffer, produces nothing
    recs = [_conv(fab, 0, 1, 0, cat, 64, 0, 64, RQ), _conv(fab, 0, 1, 1, fab.buf(), 64, 0, 64)] + _entry(1, cat, 64, [fab.buf()])
    assert not fan_boundaries(recs)[-1]["candidate"]


def test_the_option_needs_no_device():
    from hawq_amd.api import build_quantized_resnet
    model = build_quantized_resnet("inceptionv3", "uniform8", seed=0)
    assert InceptionEngine(model, fan_out=1).fan_out is True and InceptionEngine(model).fan_out is False
    eng = InceptionEngine(model, fan_out=True, grouped=True, tune=True, fast_pools=True, fused_stem=True)
    assert eng.fan_launches == [] and eng.fan_candidates == [] and eng.residual_requants == []
    with pytest.raises(TypeError):
        InceptionEngine(model, fan=True)


# ---------------------------------------------------------------------- plans
FAN = [{"unit": 1, "tiles": {"0,3,5": 3, "8": 2}, "us": {"plain": 40.5, "fan": 33.25, "0,3,5@3": 20.0, "8@2": 9.5}},
       {"unit": 4, "tiles": {"30": 1}, "us": {}}]
CANDS = {1: ["0,3,5", "8"], 2: ["11"], 4: ["30"]}


def _plan(fan=FAN):
    return make_plan((1, 299, 299), KEYS, 4, [3, 3, 4, 4, 3, 4], [{} for _ in KEYS], None, fan)


def test_fan_key():
    assert fan_key([0, 3, 5]) == "0,3,5" and fan_key((8,)) == "8"


def test_fan_out_survives_json_and_replay():
    plan = _plan()
    again = json.loads(json.dumps(plan))
    assert again == plan and again["fan_out"] == FAN and "groups" not in plan
    seen = []
    got = check_fan_out(again["fan_out"], CANDS, lambda u, k, t: seen.append((u, k, t)) or True)
    assert got == [(1, {"0,3,5": 3, "8": 2}), (4, {"30": 1})] and sorted(seen) == [(1, "0,3,5", 3), (1, "8", 2), (4, "30", 1)]
    assert check_fan_out([], CANDS, lambda u, k, t: False) == []
    assert _plan([])["fan_out"] == []


def test_a_plan_without_the_field_keeps_its_form_and_its_digest():
    with_fan, without = _plan(), _plan(None)
    assert "fan_out" not in without and {k: v for k, v in with_fan.items() if k != "fan_out"} == without
    assert make_plan((1, 299, 299), KEYS, 4, [3, 3, 4, 4, 3, 4], [{} for _ in KEYS]) == without


@pytest.mark.parametrize("entries,why", [
    ([{"unit": 3, "tiles": {"30": 1}}], "not a candidate"),
    ([{"unit": "1", "tiles": {"30": 1}}], "not a candidate"),
    ([{"unit": True, "tiles": {"30": 1}}], "not a candidate"),
    ([{"unit": 4, "tiles": {"30": 1}}, {"unit": 4, "tiles": {"30": 1}}], "named twice"),
    ([{"unit": 1, "tiles": {"0,3,5": 3}}], "are not its producers"),
    ([{"unit": 1, "tiles": {"0,3,5": 3, "8": 2, "9": 2}}], "are not its producers"),
    ([{"unit": 4, "tiles": {"31": 1}}], "are not its producers"),
    ([{"unit": 4, "tiles": {"30": 4}}], "tile 4 is refused"),
    ([{"unit": 4, "tiles": {"30": "1"}}], "refused"),
    ([{"unit": 4, "tiles": {"30": True}}], "refused"),
    ([{"unit": 4}], "not a list of fan-out boundaries"),
    ([{"tiles": {"30": 1}}], "not a list of fan-out boundaries"),
    ([{"unit": 4, "tiles": 3}], "not a list of fan-out boundaries"),
    ([[4, 1]], "not a list of fan-out boundaries"),
    (7, "not a list of fan-out boundaries"),
])
def test_stale_fan_out_entries_are_refused(entries, why):
    with pytest.raises(StalePlan, match=why):
        check_fan_out(entries, CANDS, lambda u, k, t: t != 4)
