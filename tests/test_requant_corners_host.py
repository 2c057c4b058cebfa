"""The corner list of tests/requant_corners.py, the Python restatements of the requant forms and the host-side refusals,
without a device.  The conditions on the list are conditions: the GPU file relies on them."""
import ctypes as C

import numpy as np
import pytest

from tests import requant_corners as R

PAIRS = R.pairs()
EXACT = [R.rne(v, t.m, t.e, t.k) for t, v in PAIRS]


# ------------------------------------------------------------------------------------------------ the list
def test_the_list_is_the_product_the_module_documents():
    assert len(R.TABLES) == len(R.MS) * len(R.ES) * len(R.KS) == 225
    assert {(t.m, t.e, t.k) for t in R.TABLES} == {(m, e, k) for m in R.MS for e in R.ES for k in R.KS}
    for t in R.TABLES:
        assert t.vbits == 31 - t.k and t.lim == 2 ** t.vbits - 1 and t.ek == t.e | t.k << 8
        base = {0, 1, -1, 2, -2, 3, -3, t.lim, -t.lim, t.lim - 1, 1 - t.lim, t.lim // 2, -(t.lim // 2)}
        assert {v for v in base if abs(v) <= t.lim} <= set(t.values)
    assert 0 < sum(t.provably_fast for t in R.TABLES) < len(R.TABLES)
    assert len(R.SCALAR_TABLES) == 24
    assert {R.ids0_form(ek) for _, ek in R.SCALAR_TABLES} == {True, False} and {ek >> 8 == 0 for _, ek in R.SCALAR_TABLES} == {True, False}


def test_every_pair_is_inside_the_contract():
    for t, v in PAIRS:
        assert 0 <= t.m < 2 ** 31 and 33 <= t.e <= 62 and t.k >= 0
        assert abs(v << t.k) <= 2 ** 31 - 1
    assert all(-2 ** 31 <= q < 2 ** 31 for q in EXACT)


def test_every_tie_point_of_the_rule_is_listed_and_is_a_tie():
    n = 0
    for t in R.TABLES:
        sh = t.e - 1 - t.k - R.tz(t.m) if t.m else -1
        if t.m and 0 <= sh < t.vbits:
            for u in R.TIE_U:
                if abs(u << sh) <= t.lim:
                    assert (u << sh) in t.values and R.is_tie(u << sh, t.m, t.e, t.k)
                    n += 1
        if t.e == 62:   # the product stays below 2^62: no tie inside the contract
            assert not any(R.is_tie(v, t.m, t.e, t.k) for v in t.values)
    assert n >= 100


def test_ties_of_both_signs_at_the_smallest_and_the_largest_shift():
    ties = [(t, v) for t, v in PAIRS if R.is_tie(v, t.m, t.e, t.k)]
    assert any(v > 0 for _, v in ties) and any(v < 0 for _, v in ties)
    for s in (1, 29):
        assert any(t.e - 32 == s and v > 0 for t, v in ties) and any(t.e - 32 == s and v < 0 for t, v in ties)
    # half-up and half-even differ on the odd side only: both parities of the quotient occur
    assert {R.rne(v, t.m, t.e, t.k) & 1 for t, v in ties} == {0}
    assert {(((v << t.k) * t.m) >> t.e) & 1 for t, v in ties} == {0, 1}
    # a proof that calls a table tie-free is never contradicted by the list
    assert not any(t.provably_fast for t, _ in ties)


def test_tie_free_tables_at_the_ends_of_shift_and_pre_shift():
    fast = [t for t in R.TABLES if t.provably_fast and t.m]
    for s in (1, 30):
        for k in (0, 30):
            assert any(t.e - 32 == s and t.k == k for t in fast), (s, k)


def test_results_land_on_both_sides_of_every_clamp_edge_and_far_outside():
    got = set(EXACT)
    for lo, hi in R.CLAMPS:
        for edge in (lo - 1, lo, hi, hi + 1):
            assert edge in got, (lo, hi, edge)
    assert max(EXACT) >= 2 ** 28 and min(EXACT) <= -2 ** 28


def test_centres_cover_every_value_inside_the_contract():
    for t in R.TABLES:
        offs = (-1, 0, 1) if t.lim < 128 else tuple(range(-128, 128))
        cs = R.centres(t, offs)
        reach = {c + o for c in cs for o in offs}
        assert set(t.values) <= reach and max(abs(v) for v in reach) <= t.lim
    for t in R.TABLES:   # post-ReLU inputs: the non-negative half
        if t.lim >= 128:
            assert max(abs(c + o) for c in R.centres(t, tuple(range(0, 128))) for o in (0, 127)) <= t.lim


def test_the_launch_plan_holds_every_pair_and_nothing_outside_a_contract():
    for tables in (R.TABLES, tuple(t for t in R.TABLES if t.provably_fast), tuple(t for t in R.TABLES if t.k == 0)):
        launches = R.plan(tables)
        assert R.coverage(launches, tables) == {(i, v) for i, t in enumerate(tables) for v in t.values}
        for L in launches:
            R.check_contract(L.V, L.m, L.ek)
            assert L.V.shape == (128, 256)
    relu = R.plan(R.TABLES, relu_inputs=True)
    assert R.coverage(relu, R.TABLES) == {(i, v) for i, t in enumerate(R.TABLES) for v in t.values}   # (the bias carries the sign)
    assert {L.kind for L in R.plan(R.TABLES)} == {'int8', 'tiny'} and {L.kind for L in relu} == {'relu', 'tiny_relu'}
    with pytest.raises(AssertionError):
        R.check_contract(np.array([[2 ** 16]]), [3], [34 | 15 << 8])


def test_the_array_form_of_the_reference_equals_the_python_integers():
    t, v = zip(*PAIRS)
    got = R.np_rne(np.array(v), np.array([x.m for x in t]), np.array([x.e for x in t]), np.array([x.k for x in t]))
    assert got.tolist() == EXACT


# ------------------------------------------------------------------------------------------------ the restatements
def test_restatements_equal_exact_round_half_even():
    n_nt = n_k0 = n_s0 = 0
    for (t, v), want in zip(PAIRS, EXACT):
        c = R.dynt_prepare(t.m, t.ek)
        assert R.dyadic_rne(v, t.m, t.ek) == want, (t, v)
        assert R.dyadic_tie(v, c) == want, (t, v)
        if t.provably_fast:
            assert R.dyadic_nt(v, c) == want and R.dyadic_nt_k(v, c, False) == want, (t, v)
            n_nt += 1
            if t.k == 0:
                assert R.dyadic_nt_k(v, c, True) == want
                n_k0 += 1
            if R.ids0_form(t.ek):
                assert R.dyadic_s0(v, t.m, t.ek) == want, (t, v)
                n_s0 += 1
    assert n_nt > 1000 and n_k0 > 100 and n_s0 > 50


MUTATIONS = {
    "no tie correction": lambda v, c: R.dyadic_tie(v, c, tie_fix=False),
    "& 15 for & 31": lambda v, c: R.dyadic_tie(v, c, mask=15),
    "no pre-shift": lambda v, c: R.dyadic_tie(v, c, preshift=False),
    "no rounding constant": lambda v, c: R.dyadic_tie(v, R.dynt_prepare(c.m, (c.s + 32) | c.k << 8, rounding=False)),
    "logical shift": lambda v, c: R.dyadic_tie(v, c, arith=False),
    "tie test without the high-word bits": lambda v, c: R.dyadic_tie(v, c, tie_hi_bits=False),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_each_mutation_is_caught_by_the_list(name):
    f = MUTATIONS[name]
    wrong = sum(f(v, R.dynt_prepare(t.m, t.ek)) != want for (t, v), want in zip(PAIRS, EXACT))
    assert wrong >= 1, name
    if name in ("& 15 for & 31", "no pre-shift", "no rounding constant", "logical shift"):   # also on the tie-free form
        wrong_nt = 0
        for (t, v), want in zip(PAIRS, EXACT):
            if t.provably_fast:
                c = R.dynt_prepare(t.m, t.ek, rounding=name != "no rounding constant")
                wrong_nt += R.dyadic_nt(v, c, mask=15 if name.startswith("&") else 31, preshift=name != "no pre-shift", arith=name != "logical shift") != want
        assert wrong_nt >= 1, name


# ------------------------------------------------------------------------------------------------ pack_ctab
def test_pack_ctab_constant_is_exact_at_the_ends_of_the_bias_range():
    from hawq_amd.packing import pack_ctab
    near = 0
    for t in R.TABLES:
        for bias in (t.lim - 127, 127 - t.lim):
            if abs(bias) > t.lim:
                continue   # (k = 30: the whole range is {-1, 0, 1})
            row = pack_ctab([bias], [t.m], [t.ek])[0]
            cc = (bias << t.k) * t.m + (1 << (t.e - 1))
            assert int(row[0]) == t.m and int(row[1]) == (t.e - 32) | t.k << 8
            assert (int(row[3]) << 32) | (int(row[2]) & 0xFFFFFFFF) == cc, (t, bias)
            assert tuple(int(x) for x in row) == R.ctab_constant(bias, t.m, t.ek)
            near += cc >= 2 ** 62 + 2 ** 60
            for off in (-127, -1, 0, 127):   # the epilogue's use of the row on a raw accumulator (|bias + off| <= lim)
                assert R.dyadic_ctab(off, row, True) == R.rne(bias + off, t.m, t.e, t.k)
                if t.provably_fast:
                    assert R.dyadic_ctab(off, row, False) == R.rne(bias + off, t.m, t.e, t.k)
    assert near >= 1   # a fused constant near 1.5 * 2^62 is among them


def test_pack_ctab_refuses_operands_it_would_wrap_on():
    from hawq_amd.packing import pack_ctab
    pack_ctab([2 ** 31 - 1], [2 ** 31 - 1], [62])
    pack_ctab([-(2 ** 16 - 1)], [2 ** 31 - 1], [62 | 15 << 8])
    for bias, m, ek in (([2 ** 31], [1], [33]), ([-(2 ** 31)], [1], [33]), ([2 ** 16], [3], [34 | 15 << 8]), ([2], [1], [33 | 30 << 8]),
                        ([1], [1], [33 | 31 << 8]), ([0], [1], [33 | 40 << 8]), ([2 ** 40], [2 ** 30], [47]),
                        ([1], [2 ** 31], [33]), ([1], [-1], [33]), ([0, 2 ** 31], [1, 1], [33, 33])):
        with pytest.raises(ValueError):
            pack_ctab(bias, m, ek)


# ------------------------------------------------------------------------------------------------ refusals
# Tables outside the contract in a per-call field are refused on the host, before anything is launched: the blocks below point at
# host memory and are otherwise launches the entry point takes (asserted through its own applicability query where it has one), so
# the refusal is about the table, and the message says so.
GOOD = (1 << 30, 34)
BAD_SCALARS = [(1 << 30, 32), (1 << 30, 63), (1 << 30, 33 | 31 << 8), (-1, 34), (-(1 << 30), 40)]


@pytest.fixture(scope="module")
def lib():
    from hawq_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def host_mem():
    buf = np.zeros(1 << 16, np.uint8)
    return buf, buf.ctypes.data


def _residual_block(lib, p, cin=64, cout=256):
    """a single-branch fast RESIDUAL 1x1 conv on uint16 residuals"""
    a = lib.ConvArgs()
    a.in_, a.wgt, a.bias, a.m, a.e, a.ctab, a.flags, a.res_in, a.res_out, a.out_q = (p,) * 10
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad, a.in_bits, a.w_bits = 1, 4, 4, cin, cout, 1, 1, 1, 0, 8, 8
    a.epilogue, a.fast_tables, a.res_in_bits, a.res_out_bits, a.out_bits, a.q_lo, a.q_hi = lib.EPI_RESIDUAL, 1, 16, 16, 8, 0, 127
    (a.m_id_scalar, a.e_id_scalar), (a.mq, a.eq) = GOOD, GOOD
    return a


def _set(a, field, m, ek):
    if field == "q":
        a.mq, a.eq = m, ek
    else:
        a.m_id_scalar, a.e_id_scalar = m, ek


def _last(lib):
    return lib.load().hawq_last_error().decode()


@pytest.mark.parametrize("field", ["q", "id"])
@pytest.mark.parametrize("bad", BAD_SCALARS)
def test_conv2d_and_splitk_refuse_scalar_tables_outside_the_contract(lib, host_mem, bad, field):
    p = host_mem[1]
    for fast in (1, 5):
        a = _residual_block(lib, p, 128, 256)
        a.fast_tables = fast
        assert lib.load().hawq_conv2d_splitk_ok(C.byref(a), 2) == 1, _last(lib)   # (the plan of the launch itself is fine)
        _set(a, field, *bad)
        assert lib.load().hawq_conv2d(C.byref(a), None) != 0
        assert ("eq" if field == "q" else "e_id_scalar") in _last(lib), _last(lib)
        assert lib.load().hawq_conv2d_splitk(C.byref(a), 2, p, p, None) != 0
        assert ("eq" if field == "q" else "e_id_scalar") in _last(lib), _last(lib)


@pytest.mark.parametrize("field", ["q", "id"])
@pytest.mark.parametrize("bad", BAD_SCALARS)
def test_expand_reduce_refuses_scalar_tables_outside_the_contract(lib, host_mem, bad, field):
    p = host_mem[1]
    seen = 0
    for cin, cout in ((64, 256), (128, 512), (256, 1024)):
        b = lib.ExpandReduceArgs()
        b.expand = _residual_block(lib, p, cin, cout)
        r = lib.ConvArgs()
        r.in_, r.wgt, r.bias, r.m, r.e, r.ctab, r.out_q = (p,) * 7
        r.N, r.H, r.W, r.Cin, r.Cout, r.KH, r.KW, r.stride, r.pad, r.in_bits, r.w_bits = 1, 4, 4, cout, cin, 1, 1, 1, 0, 8, 8
        r.epilogue, r.relu, r.fast_tables, r.out_bits, r.q_lo, r.q_hi = lib.EPI_REQUANT, 1, 1, 8, 0, 127
        b.reduce = r
        n = lib.load().hawq_conv_expand_reduce_variants(C.byref(b))
        assert n >= 3   # the pair as such is taken, by all three kernel families
        _set(b.expand, field, *bad)
        for tile in range(0, n + 1):
            b.tile = tile
            assert lib.load().hawq_conv_expand_reduce(C.byref(b), None) != 0, (cin, tile)
            assert "scalar tables outside the fast contract" in _last(lib), (cin, tile, _last(lib))
            seen += 1
    assert seen >= 12


@pytest.mark.parametrize("field", ["q", "id"])
@pytest.mark.parametrize("bad", BAD_SCALARS)
def test_linear_bottleneck_refuses_scalar_tables_outside_the_contract(lib, host_mem, bad, field):
    p = host_mem[1]
    b = lib.BottleneckArgs()
    e, q = b.expand, b.project
    e.in_, e.wgt, e.ctab = p, p, p
    e.N, e.H, e.W, e.Cin, e.Cout, e.KH, e.KW, e.stride, e.pad, e.in_bits, e.w_bits = 1, 16, 16, 64, 384, 1, 1, 1, 0, 8, 8
    e.epilogue, e.relu, e.q_lo, e.q_hi, e.out_bits, e.fast_tables = lib.EPI_REQUANT, 1, 0, 127, 8, 1
    b.dw_wgt9c, b.dw_ctab, b.dw_stride, b.dw_q_lo, b.dw_q_hi, b.dw_fast_tables, b.c_mid, b.tile = p, p, 1, 0, 127, 1, 384, 0
    q.wgt, q.ctab, q.res_in, q.res_out, q.out_q = (p,) * 5
    q.N, q.H, q.W, q.Cin, q.Cout, q.KH, q.KW, q.stride, q.pad, q.in_bits, q.w_bits = 1, 16, 16, 384, 64, 1, 1, 1, 0, 8, 8
    q.epilogue, q.res_no_relu, q.fast_tables, q.res_in_bits, q.res_out_bits, q.out_bits, q.q_lo, q.q_hi = lib.EPI_RESIDUAL, 1, 1, 32, 32, 8, -128, 127
    (q.m_id_scalar, q.e_id_scalar), (q.mq, q.eq) = GOOD, GOOD
    assert lib.load().hawq_linear_bottleneck_ok(C.byref(b)) == 1
    _set(q, field, *bad)
    assert lib.load().hawq_linear_bottleneck_ok(C.byref(b)) == 0
    assert lib.load().hawq_linear_bottleneck(C.byref(b), None) != 0
    assert ("(mq, eq)" if field == "q" else "scalar table") in _last(lib), _last(lib)
