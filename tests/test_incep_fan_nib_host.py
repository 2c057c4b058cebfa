"""Host side of the mixed-form fan-out launch: hawq_incep_conv_group_nib_fan_ok on made-up addresses (nothing is dereferenced), the
boundary function on a nibble plan's entry requants, and the engine option's preconditions.  No GPU."""
import ctypes as C

import pytest

from hawq_amd import _lib
from hawq_amd.engine_inception import InceptionEngine, PlanNotApplicable, fan_boundaries
from tests.test_gpu_incep_fan_nib_kernels import check_refusals, describe
from tests.test_incep_fan_host import POST, Fab, _conv, _entry, _pool

_ADDR = {}


def _addr(i, what):
    """made-up addresses, 16-byte aligned and far apart, one per operand and buffer"""
    return _ADDR.setdefault((i, what), 0x10000000 * (len(_ADDR) + 1))


@pytest.mark.parametrize("tile", [1, 2])
def test_ok_takes_the_three_member_level(tile):
    g, mask, fans, fan_mask = describe("level", _addr)
    assert (g.n, mask, [f.n for f in fans], fan_mask) == (3, 0b010, [0, 4, 1], 0x150)
    assert _lib.load().hawq_incep_conv_group_nib_fan_ok(C.byref(g), mask, fans, fan_mask, tile) == 1


def test_ok_refuses_and_names_the_reason():
    g, mask, fans, fan_mask = describe("level", _addr)
    check_refusals(g, mask, fans, fan_mask, _addr(None, "X"), None)


def test_boundary_targets_carry_the_form_and_buffer_the_nibble_plan_issues():
    fab = Fab()
    cat, prev, outs, nib_out = fab.buf(), fab.buf(), [fab.buf(), fab.buf()], fab.buf()
    recs = [_conv(fab, 3, 1, 0, cat, 768, 0, 384), _conv(fab, 3, 3, 1, cat, 768, 384, 96),
            _pool("hawq_incep_maxpool3s2", 3, 0, prev, 288, cat, 768, 480, 288)] + _entry(4, cat, 768, outs)
    plain = fan_boundaries(recs)[-1]
    assert plain["forms"] == [8, 8] and plain["producers"][0] == [(o, 768, POST, 0, 384) for o in outs]
    # the plan issues the second entry requant hawq4, into a buffer of its own, clamped to the nibble range
    a = _lib.IncepPoolArgs.from_buffer_copy(recs[-1].args[0])
    a.out, a.out_bits, a.lo2, a.hi2 = nib_out, 4, 0, 15
    b = fan_boundaries(recs, {recs[-1]: a})[-1]
    assert b["candidate"] and b["forms"] == [8, 4] and b["residual"] == plain["residual"] == [(480, 288)]
    nib_post = POST[:2] + (0, 15)
    assert b["producers"] == {0: [(outs[0], 768, POST, 0, 384), (nib_out, 768, nib_post, 0, 384)],
                              1: [(outs[0], 768, POST, 384, 96), (nib_out, 768, nib_post, 384, 96)]}
    assert fan_boundaries(recs, {})[-1] == plain   # an all-int8 list: unchanged
    a.out_bits = 16   # an issued block that is neither int8 nor hawq4 makes the boundary no candidate
    assert not fan_boundaries(recs, {recs[-1]: a})[-1]["candidate"]


def test_the_option_needs_nibble_and_fan_out_still_does_not_compose():
    with pytest.raises(PlanNotApplicable, match="nibble_fan"):
        InceptionEngine(None, nibble_fan=True)
    with pytest.raises(PlanNotApplicable, match="fan_out"):
        InceptionEngine(None, nibble=True, fan_out=True)
