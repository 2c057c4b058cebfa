"""Host side of the variant table of the expand conv alone (fused_wp.hip, reduce.wgt == NULL) through the library's host-only queries:
the numbering is append-only (the first variants are the ones recorded plans already name, in their order), every slice split divides
C3 / 64, the count does not move with out_sub / res_sub, and every "@solo" entry of profiles/plans.json carries the count the library
reports for its shape.  No GPU."""
import ctypes as C
import json
import os
import re

import pytest

from hawq_amd import _lib
from tests.conv_choice_cases import RES16, conv, with_fast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (pixels per workgroup, slice split) of the variants that existed before the table grew, in their order
FIRST = {64: [(128, 1)], 128: [(128, 1)], 256: [(128, 1), (128, 2), (128, 4)], 512: [(128, 1), (128, 2), (128, 4), (128, 8)]}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _solo(c, c3, n=64, hw=14, **fields):
    er = _lib.ExpandReduceArgs()
    full = conv(n, hw, c, c3, 1, 1, **with_fast(dict(dict(RES16, res_out=None), **fields), 1))
    C.memmove(C.byref(er.expand), C.byref(full), C.sizeof(full))
    return er


def _shapes(lib, er):
    out = []
    for v in range(1, lib.hawq_conv_expand_reduce_variants(C.byref(er)) + 1):
        px, ys = C.c_int32(-1), C.c_int32(-1)
        assert lib.hawq_conv_expand_reduce_variant_shape(C.byref(er), v, C.byref(px), C.byref(ys)) == 0, v
        out.append((px.value, ys.value))
    return out


@pytest.mark.parametrize("c", sorted(FIRST))
def test_first_variants_are_the_recorded_ones_and_splits_divide(lib, c):
    er = _solo(c, 4 * c)
    shapes = _shapes(lib, er)
    assert shapes[:len(FIRST[c])] == FIRST[c]
    assert len(set(shapes)) == len(shapes)
    assert all(px in (64, 128) and (4 * c // 64) % ys == 0 for px, ys in shapes)
    # variant 0 is the default (variant 1); an id behind the last and a null argument are refused and leave the outputs alone
    px, ys = C.c_int32(-1), C.c_int32(-1)
    assert lib.hawq_conv_expand_reduce_variant_shape(C.byref(er), 0, C.byref(px), C.byref(ys)) == 0 and (px.value, ys.value) == shapes[0]
    px, ys = C.c_int32(-1), C.c_int32(-1)
    assert lib.hawq_conv_expand_reduce_variant_shape(C.byref(er), len(shapes) + 1, C.byref(px), C.byref(ys)) != 0
    assert (px.value, ys.value) == (-1, -1)
    assert lib.hawq_conv_expand_reduce_variant_shape(None, 1, C.byref(px), C.byref(ys)) != 0


@pytest.mark.parametrize("c", sorted(FIRST))
def test_a_split_that_does_not_divide_drops_that_variant_alone(lib, c):
    full = _shapes(lib, _solo(c, 4 * c))
    for nsl in (1, 2, 3, 5, 6, 12, 24, 4 * c // 64):
        got = _shapes(lib, _solo(c, 64 * nsl))
        assert got == [(px, ys) for px, ys in full if nsl % ys == 0], nsl   # the others keep their order


@pytest.mark.parametrize("c", sorted(FIRST))
def test_counts_do_not_move_with_out_sub_or_res_sub(lib, c):
    plain = _shapes(lib, _solo(c, 4 * c, hw=14))
    assert _shapes(lib, _solo(c, 4 * c, hw=14, out_sub=2)) == plain
    assert _shapes(lib, _solo(c, 4 * c, hw=7, stride2=2, H2=14, W2=14)) == plain
    assert _shapes(lib, _solo(c, 4 * c, hw=14, out_bits=4, q_hi=15)) == plain   # hawq4 block input


def test_pair_variants_and_other_families_have_no_shape_entry_of_their_own(lib):
    """A pair's wave-private variants report split 1; the variants of the other two pair kernels report nothing."""
    from tests.conv_choice_cases import REQUANT
    for c in (64, 128, 256):
        er = _solo(c, 4 * c, hw=14, res_out=16)
        red = conv(64, 14, 4 * c, c, 1, 1, **with_fast(REQUANT, 1))
        C.memmove(C.byref(er.reduce), C.byref(red), C.sizeof(red))
        n = lib.hawq_conv_expand_reduce_variants(C.byref(er))
        assert n >= 2
        got = []
        for v in range(1, n + 1):
            px, ys = C.c_int32(-1), C.c_int32(-1)
            rc = lib.hawq_conv_expand_reduce_variant_shape(C.byref(er), v, C.byref(px), C.byref(ys))
            got.append(None if rc else (px.value, ys.value))
        wp = [g for g in got if g is not None]
        assert wp and all(ys == 1 and px in (128, 256) for px, ys in wp) and None in got


def test_recorded_plans_carry_the_library_counts(lib):
    with open(os.path.join(ROOT, "profiles", "plans.json")) as f:
        plans = json.load(f)
    seen = 0
    for key, plan in sorted(plans.items()):
        names = plan.get("pair_launches") or []
        for k, name in enumerate(names):
            if not name.endswith("@solo"):
                continue
            c = 64 << (int(re.match(r"stage(\d+)\.", name)[1]) - 1)   # bottleneck ResNets: the expand conv of stage s reads 64 * 2^(s-1) channels
            count = lib.hawq_conv_expand_reduce_variants(C.byref(_solo(c, 4 * c)))
            assert plan["pair_variant_counts"][k] == count, (key, name)
            chains = [plan] + list(plan.get("per_chain") or [])
            for ch in chains:
                if ch.get("fused_variants"):
                    assert 0 <= int(ch["fused_variants"].split(".")[k]) <= count, (key, name)
            seen += 1
    assert seen >= 12
