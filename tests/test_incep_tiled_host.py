"""Host-side contract of the LDS-tiled InceptionV3 conv entry points (hawq_incep_conv_num_tiles / hawq_incep_conv_tile_ok) and of the
conv tile plans of hawq_amd/engine_inception.py (launch_digest / make_plan / check_plan).  Host-only functions, called through
ctypes, and pure Python: no GPU needed."""
import ctypes as C
import json
import os
import re

import pytest

from hawq_amd import _lib
from hawq_amd.engine import StalePlan
from hawq_amd.engine_inception import check_plan, launch_digest, make_plan

# (KH, KW, pad_h, pad_w, stride, H, W, Cin, Cout): every conv geometry of the network (tests/test_gpu_inception_kernels.py)
GEOMETRIES = [
    (3, 3, 0, 0, 2, 299, 299, 16, 32), (3, 3, 0, 0, 1, 149, 149, 32, 32), (3, 3, 1, 1, 1, 147, 147, 32, 64),
    (1, 1, 0, 0, 1, 73, 73, 64, 80), (3, 3, 0, 0, 1, 73, 73, 80, 192), (1, 1, 0, 0, 1, 35, 35, 192, 48),
    (5, 5, 2, 2, 1, 35, 35, 48, 64), (3, 3, 1, 1, 1, 35, 35, 64, 96), (3, 3, 1, 1, 1, 35, 35, 96, 96),
    (3, 3, 0, 0, 2, 35, 35, 288, 384), (3, 3, 0, 0, 2, 35, 35, 96, 96), (1, 7, 0, 3, 1, 17, 17, 128, 128),
    (7, 1, 3, 0, 1, 17, 17, 160, 192), (3, 3, 0, 0, 2, 17, 17, 192, 320), (1, 1, 0, 0, 1, 8, 8, 1280, 448),
    (3, 3, 1, 1, 1, 8, 8, 448, 384), (1, 3, 0, 1, 1, 8, 8, 384, 384), (3, 1, 1, 0, 1, 8, 8, 384, 384),
]
ENTRY_POINTS = ("hawq_incep_conv_num_tiles", "hawq_incep_conv_tile_ok", "hawq_incep_conv_tiled")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def args(g, n=2, epilogue=_lib.INCEP_REQUANT, out_bits=8, **kw):
    KH, KW, ph, pw, stride, H, W, Cin, Cout = g
    a = _lib.IncepConvArgs()
    a.in_, a.wgt, a.bias, a.out, a.m, a.ek = 16, 16, 16, 16, 16, 16   # never dereferenced by the host-only query
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad_h, a.pad_w = n, H, W, Cin, Cout, KH, KW, stride, ph, pw
    a.epilogue, a.relu, a.out_bits, a.ldo, a.c_off = epilogue, 1, out_bits, Cout, 0
    lim = 127 if out_bits == 8 else 32767
    a.q_lo, a.q_hi, a.q2_lo, a.q2_hi = 0, lim, -lim, lim
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def ok(lib, a, tile):
    return lib.hawq_incep_conv_tile_ok(C.byref(a), tile)


def test_entry_points_are_declared_and_the_abi_is_unchanged(lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hawq_mi355.h")).read()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert lib.hawq_abi_version() == 5
    assert lib.hawq_incep_conv_num_tiles() >= 3


def test_the_workgroup_body_and_the_tile_table_are_written_once():
    """the tiled, the grouped and the fan-out kernels share one workgroup body (incep_tile_body.h, included as text by each), one tile
    table with one dispatch over it and one layout of a group's grid (incep_tile.h): each is written once across the five files"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hawq_amd", "csrc")
    kernels = ("incep_tiled.hip", "incep_group.hip", "incep_fan.hip")
    text = {name: open(os.path.join(csrc, name)).read() for name in ("incep_tile.h", "incep_tile_body.h") + kernels}

    def where(what):
        return {name: len(re.findall(what, t)) for name, t in text.items() if re.search(what, t)}
    for what in (r"__builtin_amdgcn_mfma_i32_32x32x32_i8", r"constexpr int NT ="):
        assert where(what) == {"incep_tile_body.h": 1}, what
    assert where(r'#include "incep_tile_body\.h"') == dict.fromkeys(kernels, 1)
    for what in (r"\bkTiles\[[^\]]*\] =", r"enum \{ NUM_TILES\b", r"struct TileShape\b", r"switch \(tile\)", r"128, 128, 2, 2, 1>", r"256, 64, 4, 1, 1>",
                 r"128, 64, 2, 2, 1>", r"64, 32, 1, 1, 2>", r"struct GroupMap\b", r"struct Span\b", r"bid >= mp\.end\[j\]", r"= INT32_MAX"):
        assert where(what) == {"incep_tile.h": 1}, what
    # the loop over a member's fan outputs is the fan kernel's own: its requant and its store
    for what in (r"#pragma unroll 1\n", r"dyadic_rne\(q\[4 \* e \+ u\], f\.m, f\.ek\), f\.lo, f\.hi\)", r"f\.out \+ \(size_t\)p \* f\.ldo \+ f\.c_off \+ cb"):
        assert where(what) == {"incep_fan.hip": 1}, what


def test_tile_0_takes_every_geometry_of_the_network(lib):
    for g in GEOMETRIES:
        for epi, bits in ((_lib.INCEP_RAW, 32), (_lib.INCEP_REQUANT, 8), (_lib.INCEP_REQUANT, 16), (_lib.INCEP_REQUANT2, 16)):
            assert ok(lib, args(g, epilogue=epi, out_bits=bits), 0) == 1, g
        assert ok(lib, args(g, n=128, ldo=g[8] + 160, c_off=96), 0) == 1


def test_refuses_unknown_tile_ids(lib):
    T = lib.hawq_incep_conv_num_tiles()
    for g in GEOMETRIES:
        assert ok(lib, args(g), -1) == 0 and ok(lib, args(g), T + 1) == 0 and ok(lib, args(g), 1000) == 0


@pytest.mark.parametrize("change", [
    dict(in_=None), dict(wgt=None), dict(bias=None), dict(out=None), dict(m=None), dict(Cin=24), dict(Cout=40), dict(N=0),
    dict(KH=8), dict(KW=0), dict(stride=3), dict(pad_h=2), dict(pad_w=-1), dict(ldo=32), dict(c_off=-16), dict(epilogue=3),
    dict(out_bits=4), dict(q_hi=128), dict(q_lo=5, q_hi=4), dict(H=1, W=1, pad_h=0, pad_w=0)])
def test_refuses_what_hawq_incep_conv_refuses(lib, change):
    """every tile id, tile 0 included, answers 0 for an argument block that the base entry point rejects"""
    g = (3, 3, 1, 1, 1, 35, 35, 64, 96)
    T = lib.hawq_incep_conv_num_tiles()
    assert ok(lib, args(g), 0) == 1
    a = args(g, **change)
    for tile in range(T + 1):
        assert ok(lib, a, tile) == 0, (change, tile)
    a = args(g, epilogue=_lib.INCEP_REQUANT2, out_bits=8, q2_hi=200)
    assert ok(lib, a, 0) == 0


def test_coverage_of_the_network_geometries(lib):
    T = lib.hawq_incep_conv_num_tiles()
    table = {(gi, t): ok(lib, args(g), t) for gi, g in enumerate(GEOMETRIES) for t in range(1, T + 1)}
    assert set(table.values()) <= {0, 1}
    for gi, g in enumerate(GEOMETRIES):
        assert any(table[gi, t] for t in range(1, T + 1)), f"no tiled kernel takes {g}"
    for t in range(1, T + 1):
        assert any(table[gi, t] for gi in range(len(GEOMETRIES))), f"tile {t} takes no geometry of the network"
    refused = sum(1 for v in table.values() if not v)
    assert 3 * refused <= len(GEOMETRIES) * T, f"{refused} of {len(GEOMETRIES) * T} (geometry, tile) pairs refused"
    # the answer does not depend on the batch, the epilogue or the concat slice (as long as that is 16-channel aligned)
    for gi, g in enumerate(GEOMETRIES):
        for t in range(1, T + 1):
            assert ok(lib, args(g, n=128, epilogue=_lib.INCEP_REQUANT2, out_bits=16, ldo=g[8] + 32, c_off=16), t) == table[gi, t]
            assert ok(lib, args(g, n=1, epilogue=_lib.INCEP_RAW, out_bits=32), t) == table[gi, t]


def test_tiled_kernels_need_16_byte_rows(lib):
    """ids > 0 store whole 16-byte runs: a slice or pitch that is not a multiple of 16 channels is left to tile 0"""
    g = (1, 7, 0, 3, 1, 17, 17, 128, 128)
    T = lib.hawq_incep_conv_num_tiles()
    for change in (dict(ldo=136), dict(ldo=144, c_off=8), dict(out=24), dict(in_=8), dict(wgt=4)):
        a = args(g, **change)
        assert ok(lib, a, 0) == 1
        assert not any(ok(lib, a, t) for t in range(1, T + 1)), change


# ---------------------------------------------------------------------- plans
def _keys():
    # launch_key layout: H, W, Cin, Cout, KH, KW, stride, pad_h, pad_w, epilogue, out_bits, ldo, c_off
    return [(H, W, Cin, Cout, KH, KW, s, ph, pw, 1 + (i % 2), 8 if i % 2 == 0 else 16, Cout + 32 * (i % 2), 16 * (i % 2))
            for i, (KH, KW, ph, pw, s, H, W, Cin, Cout) in enumerate(GEOMETRIES)]


def _plan(T=4):
    keys = _keys()
    tiles = [i % (T + 1) for i in range(len(keys))]
    us = [{0: 10.0 + i, tiles[i]: 5.25 + i} for i in range(len(keys))]
    return keys, tiles, make_plan((2, 299, 299), keys, T, tiles, us)


def test_launch_digest_is_stable_and_sees_every_field():
    keys = _keys()
    d = launch_digest(keys)
    assert d == launch_digest([list(k) for k in keys]) == launch_digest(tuple(keys)) and re.fullmatch(r"[0-9a-f]{64}", d)
    # a recorded value: the digest may not change between builds, or every recorded plan goes stale
    assert launch_digest([(8, 8, 384, 384, 1, 3, 1, 0, 1, 2, 16, 768, 0)]) == "4e77953b4eccfb5bbf2683f10c1801c7787986c43c46fdac4428d8ecaf8256d5"
    for i in range(len(keys)):
        for f in range(len(keys[i])):
            other = [list(k) for k in keys]
            other[i][f] += 1
            assert launch_digest(other) != d
    assert launch_digest(keys[::-1]) != d and launch_digest(keys[:-1]) != d


def test_plan_survives_json_and_replays():
    keys, tiles, plan = _plan()
    again = json.loads(json.dumps(plan))
    assert again == plan
    assert again["tiles"] == tiles and again["batch"] == [2, 299, 299] and again["num_tiles"] == 4
    assert again["launches"] == launch_digest(keys) and again["us"][3] == {"0": 13.0, "3": 8.25}
    seen = []
    assert check_plan(again, (2, 299, 299), keys, 4, lambda i, t: seen.append((i, t)) or True) == tiles
    assert seen == list(enumerate(tiles))


def test_stale_plans_are_refused():
    keys, tiles, plan = _plan()
    yes = lambda i, t: True   # noqa: E731
    with pytest.raises(StalePlan, match="batch shape"):
        check_plan(plan, (3, 299, 299), keys, 4, yes)
    with pytest.raises(StalePlan, match="batch shape"):
        check_plan(plan, (2, 224, 224), keys, 4, yes)
    with pytest.raises(StalePlan, match="conv tiles"):
        check_plan(plan, (2, 299, 299), keys, 5, yes)
    changed = [list(k) for k in keys]
    changed[7][3] += 16
    with pytest.raises(StalePlan, match="launch list"):
        check_plan(plan, (2, 299, 299), changed, 4, yes)
    with pytest.raises(StalePlan, match="launch list"):
        check_plan(plan, (2, 299, 299), keys[:-1], 4, yes)
    with pytest.raises(StalePlan, match="tile 2"):
        check_plan(plan, (2, 299, 299), keys, 4, lambda i, t: not (i == 2 and t == 2))
    for bad in (5, -1, "1", 1.0, None):
        p = dict(plan, tiles=[bad] + tiles[1:])
        with pytest.raises(StalePlan, match="refused"):
            check_plan(p, (2, 299, 299), keys, 4, yes)
    with pytest.raises(StalePlan):
        check_plan({"tiles": tiles}, (2, 299, 299), keys, 4, yes)
    assert issubclass(StalePlan, ValueError)
