"""The kernels' requant epilogues at the corners of the dyadic table contract (tests/requant_corners.py).

Method: driven accumulators.  A 1x1 conv with 0/1 diagonal weights W[c][c mod Cin] = 1 on one 16 x 16 image whose 256 pixels
carry the offsets -128 .. 127 (or -1 .. 1 for tables whose whole range is that small) has acc[p][c] = bias[c] + offset[p]: the bias
centres channel c on a chosen value of its table and the pixels walk across it.  Every comparison is np.array_equal against exact
round-half-even in integers (requant_corners.np_rne, itself checked against Python integers on the host) plus the clamp; there is
no tolerance.  Before every upload a host-side assert proves that no driven value lies outside its table's contract."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import tests.test_gpu_kernels as K
import tests.test_gpu_splitk as SK
from tests import requant_corners as R
from tests.guard import dev, guard_arena, out_buf  # noqa: F401  (guard_arena: fixture)
from tests.test_gpu_kernels import lib  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guard_arena")]

COUT, CIN, HW = 128, 64, 16
NPIX = HW * HW

# fast_tables value -> the tables of the list whose contract admits that form (include/hawq_mi355.h at fast_tables):
# 0 exact general path and 5 exact-tie mode take every table; 1 needs the tie-freedom proof; bit 1 (3, 7) and bit 3 (9, 13) promise k == 0
FORMS = {
    0: lambda t: True, 5: lambda t: True, 1: lambda t: t.provably_fast,
    3: lambda t: t.provably_fast and t.k == 0, 7: lambda t: t.k == 0,
    9: lambda t: t.provably_fast and t.k == 0, 13: lambda t: t.k == 0,
}


@functools.lru_cache(maxsize=None)
def form_plan(fast, cout=COUT):
    tables = tuple(t for t in R.TABLES if FORMS[fast](t))
    launches = R.plan(tables, cout)
    # every admitted pair of the list is in some launch of this form
    want = {(i, v) for i, t in enumerate(tables) for v in t.values}
    assert R.coverage(launches, tables) == want and len(want) >= 400
    return tables, launches


def generic_tiles(lib):
    return list(range(0, lib.load().hawq_conv2d_num_tiles() - lib.load().hawq_conv2d_num_band_tiles() + 1))


def image(off, cin=CIN):
    """[1][cin][16][16]: every input column carries the same 256 offsets"""
    return np.broadcast_to(np.asarray(off, np.int64).reshape(1, 1, HW, HW), (1, cin, HW, HW)).copy()


def diagonal(cout=COUT, cin=CIN, k=1):
    """W[c][c mod cin] = 1 on the centre tap"""
    w = np.zeros((cout, cin, k, k), np.int64)
    w[np.arange(cout), np.arange(cout) % cin, k // 2, k // 2] = 1
    return w


NP_OF = {torch.int8: np.int8, torch.uint8: np.uint8, torch.int16: np.int16, torch.uint16: np.uint16, torch.int32: np.int32}


def put(t, a):
    """overwrite a device tensor with host values (converted on the host: same dtype on both sides of the copy)"""
    t.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(NP_OF[t.dtype]))).reshape(t.shape))


def stale(t):
    """fill an output with a byte pattern no expectation consists of"""
    t.view(torch.uint8).fill_(0x3C)


def i32(a):
    return np.asarray(a, np.int64).astype(np.int32)


class Driven:
    """One hawq_conv2d argument block on the driven conv (1x1, or 3x3 / pad 1 with only the centre tap set); `load` moves a launch of
    the plan into its device tables.  layout: "nhwc", or what a special-purpose kernel family reads - "band2" (planar input + wgt_band)
    and "k128" (wgt_k128)."""

    def __init__(self, lib, cin=CIN, cout=COUT, k=1, layout="nhwc"):
        from hawq_amd.packing import pack_conv_weight, pack_ctab, pack_w1x1_k128, pack_w3x3_band
        self.lib, self.pack_ctab, self.cout = lib, pack_ctab, cout
        wt = diagonal(cout, cin, k)
        self.a, self.keep = K.conv_args(lib, image(R.OFFSETS["int8"], cin), wt, np.zeros(cout, np.int64), 1, k // 2, 8, 8)
        self.x = {kind: dev(K.pack_act(image(off, cin), 8)) for kind, off in R.OFFSETS.items()}
        self.xp = {kind: dev(K.to_planar(K.pack_act(image(off, cin), 8))) for kind, off in R.OFFSETS.items()}
        self.planar_in = layout == "band2"
        if layout == "band2":
            self.keep['wb'] = dev(pack_w3x3_band(pack_conv_weight(wt, 8), cout, cin))
            self.a.wgt_band = self.keep['wb'].data_ptr()
        if layout == "k128":
            self.keep['wk'] = dev(pack_w1x1_k128(pack_conv_weight(wt, 8), cout, cin))
            self.a.wgt_k128 = self.keep['wk'].data_ptr()
        self.m, self.e, self.ctab = (dev(np.zeros(cout, np.int32)), dev(np.full(cout, 33, np.int32)), dev(np.zeros((cout, 4), np.int32)))
        self.a.m, self.a.e, self.a.ctab = self.m.data_ptr(), self.e.data_ptr(), self.ctab.data_ptr()

    def load(self, L):
        R.check_contract(L.V, L.m, L.ek)   # nothing outside a table's contract is uploaded
        assert len(L.bias) == self.cout
        put(self.keep['b'], i32(L.bias)), put(self.m, i32(L.m)), put(self.e, i32(L.ek))
        put(self.ctab, self.pack_ctab(L.bias, L.m, L.ek))
        self.set_input(L.kind, self.planar_in)

    def set_input(self, kind, planar):
        self.a.in_, self.a.in_planar = (self.xp if planar else self.x)[kind].data_ptr(), int(planar)

    def run(self, tile):
        self.a.tile = tile
        self.lib.call("hawq_conv2d", C.byref(self.a), K.stream())

    def try_run(self, tile):
        """False when the tile refuses this launch (a special-purpose kernel that is not built for it)"""
        self.a.tile = tile
        return self.lib.load().hawq_conv2d(C.byref(self.a), K.stream()) == 0


def cp(t, bits=8, c=COUT, planar=False):
    """device q tensor -> [C][256] int64"""
    got = K.from_planar(t, (1, HW, HW, c), bits) if planar else K.unpack_q(t, (1, HW, HW, c), bits)
    return got.reshape(c, NPIX)


def carrier(t, c=COUT):
    return t.cpu().numpy().astype(np.int64).reshape(NPIX, c).T


def requant(V, L):
    return R.np_rne(V, L.m[:, None], (L.ek & 0xff)[:, None], (L.ek >> 8)[:, None])


def scalar(v, m, ek):
    return R.np_rne(v, m, ek & 0xff, ek >> 8)


# ================================================================================== 1. hawq_conv2d, every generic tile
@pytest.mark.parametrize("out_bits,relu", [(8, 0), (8, 1), (4, 0), (4, 1)])
@pytest.mark.parametrize("fast", sorted(FORMS))
def test_conv2d_requant_at_the_corners(lib, fast, out_bits, relu):
    """REQUANT on every generic tile: the exact path (0), the tie form (5, 7, 13) on every table they admit, the two-instruction
    form (1, 3, 9) on the provably tie-free ones; int8 and hawq4 outputs, with and without ReLU, NHWC and (fast forms) planar."""
    tables, launches = form_plan(fast)
    d = Driven(lib)
    a = d.a
    lo, hi = (-128, 127) if out_bits == 8 else (0, 15)
    out = out_buf(NPIX * COUT * out_bits // 8, torch.uint8, 0)
    a.epilogue, a.relu, a.fast_tables = lib.EPI_REQUANT, relu, fast
    a.out_q, a.out_bits, a.q_lo, a.q_hi = out.data_ptr(), out_bits, lo, hi
    edges = set()
    for L in launches:
        d.load(L)
        ref = np.clip(requant(np.maximum(L.V, 0), L) if relu else L.Q, lo, hi)
        edges |= {x for x in (lo - 1, lo, hi, hi + 1) if (L.Q == x).any()}
        for tile in generic_tiles(lib):
            for planar in ((0, 1) if fast else (0,)):
                a.out_planar = planar
                stale(out)
                d.run(tile)
                got = cp(out, out_bits, planar=bool(planar))
                bad = np.argwhere(got != ref)
                assert bad.size == 0, (fast, tile, planar, [(tables[L.tidx[c]][:3], int(L.V[c, p]), int(got[c, p]), int(ref[c, p])) for c, p in bad[:5]])
    assert edges == {lo - 1, lo, hi, hi + 1}   # results exactly on both sides of both clamp edges were on the device


@pytest.mark.parametrize("res_bits", [16, 32])
@pytest.mark.parametrize("fast", [0, 5, 1])
def test_conv2d_residual_per_channel_corners(lib, fast, res_bits):
    """Single-branch RESIDUAL: per-channel tables at the corners, mid-range scalar tables.  res_out is compared exactly where the sum
    fits the carrier; above 65535 the uint16 carrier holds 65535 and the overflow flag is set."""
    from hawq_amd.quant_utils import tables_are_fast
    tables, launches = form_plan(fast)
    m1, e1, mq, eq = 0x5A5A5A5B, 34, 0x5A5A5A5B, 40   # odd m: provably tie-free for 17-bit residuals / 31-bit sums
    assert tables_are_fast([m1], [e1], 17) and tables_are_fast([mq], [eq], 31)
    rng = np.random.default_rng(16)
    res = rng.integers(0, 60000, (NPIX, COUT)).astype(np.int64)
    res[::7] = 0
    idq = scalar(res, m1, e1).T
    d = Driven(lib)
    a = d.a
    keep = dict(res=dev(res.astype(np.uint16 if res_bits == 16 else np.int32)))
    flags = out_buf(1, torch.int32, 0)
    out_res = out_buf(NPIX * COUT, torch.uint16 if res_bits == 16 else torch.int32, 0)
    out_q = out_buf(NPIX * COUT, torch.uint8, 0)
    a.epilogue, a.fast_tables, a.flags = lib.EPI_RESIDUAL, fast, flags.data_ptr()
    a.res_in, a.res_in_bits, a.m_id_scalar, a.e_id_scalar = keep['res'].data_ptr(), res_bits, m1, e1
    a.res_out, a.res_out_bits = out_res.data_ptr(), res_bits
    a.out_q, a.out_bits, a.q_lo, a.q_hi, a.mq, a.eq = out_q.data_ptr(), 8, 0, 127, mq, eq
    overflowed = 0
    for L in launches:
        d.load(L)
        o = np.maximum(L.Q + idq, 0)
        assert o.max() < 2 ** 31   # (mq, eq) has no pre-shift: its contract is the int32 range
        ref_q = np.clip(scalar(o, mq, eq), 0, 127)
        for tile in generic_tiles(lib):
            flags.zero_(), stale(out_res), stale(out_q)
            d.run(tile)
            got = carrier(out_res)
            if res_bits == 16:
                assert np.array_equal(got[o <= 65535], o[o <= 65535]) and (got[o > 65535] == 65535).all(), (fast, tile)
                assert bool(flags.item() & 1) == bool((o > 65535).any()), (fast, tile)
            else:
                assert np.array_equal(got, o), (fast, tile)
            assert np.array_equal(cp(out_q), ref_q), (fast, tile)
        overflowed += int((o > 65535).any())
    assert 0 < overflowed < len(launches) or res_bits == 32 or overflowed   # the flag was seen set (and, where a launch stays below, clear)


@pytest.mark.parametrize("fast", [0, 5, 1])
def test_conv2d_residual_dual_branch_corners(lib, fast):
    """Dual-branch RESIDUAL: in2 / wgt2 / ctab_id driven like the main branch, both per-channel tables at corners at once (launch i of the
    plan on the main branch, its neighbour on the identity conv)."""
    tables, launches = form_plan(fast)
    mq, eq = 0x5A5A5A5B, 40
    d = Driven(lib)
    a = d.a
    b2, m_id, e_id, ctab_id = dev(np.zeros(COUT, np.int32)), dev(np.zeros(COUT, np.int32)), dev(np.zeros(COUT, np.int32)), dev(np.zeros((COUT, 4), np.int32))
    flags = out_buf(1, torch.int32, 0)
    out_res = out_buf(NPIX * COUT, torch.uint16, 0)
    out_q = out_buf(NPIX * COUT, torch.uint8, 0)
    a.wgt2, a.bias2, a.m_id, a.e_id, a.ctab_id = d.keep['w'].data_ptr(), b2.data_ptr(), m_id.data_ptr(), e_id.data_ptr(), ctab_id.data_ptr()
    a.H2, a.W2, a.Cin2, a.stride2, a.in2_bits, a.w2_bits = HW, HW, CIN, 1, 8, 8
    a.epilogue, a.fast_tables, a.flags = lib.EPI_RESIDUAL, fast, flags.data_ptr()
    a.res_out, a.res_out_bits = out_res.data_ptr(), 16
    a.out_q, a.out_bits, a.q_lo, a.q_hi, a.mq, a.eq = out_q.data_ptr(), 8, 0, 127, mq, eq
    for i, L in enumerate(launches):
        same = [j for j, x in enumerate(launches) if x.kind == L.kind]
        L2 = launches[same[(same.index(i) + 1) % len(same)]]
        d.load(L)
        R.check_contract(L2.V, L2.m, L2.ek)
        put(b2, i32(L2.bias)), put(m_id, i32(L2.m)), put(e_id, i32(L2.ek)), put(ctab_id, d.pack_ctab(L2.bias, L2.m, L2.ek))
        a.in2 = d.x[L2.kind].data_ptr()
        o = np.maximum(L.Q + L2.Q, 0)
        ref_q = np.clip(scalar(o, mq, eq), 0, 127)
        for tile in generic_tiles(lib):
            flags.zero_(), stale(out_res), stale(out_q)
            d.run(tile)
            got = carrier(out_res)
            assert np.array_equal(got[o <= 65535], o[o <= 65535]) and (got[o > 65535] == 65535).all(), (fast, tile)
            assert bool(flags.item() & 1) == bool((o > 65535).any()), (fast, tile)
            assert np.array_equal(cp(out_q), ref_q), (fast, tile)


def scalar_values(m, ek, vmax, signed):
    """the list's rule for one scalar table, inside what the carrier holds"""
    e, k = ek & 0xff, ek >> 8
    lim = min((1 << (31 - k)) - 1, vmax)
    vals = {v for v in R._values(m, e, k, 31 - k, (1 << (31 - k)) - 1)} | {lim, lim - 1, lim // 2, -lim, 1 - lim, -(lim // 2)}
    return sorted(v for v in vals if abs(v) <= lim and (signed or v >= 0))


@pytest.mark.parametrize("res_bits", [16, 32])
@pytest.mark.parametrize("which", ["id", "q"])
def test_conv2d_residual_scalar_corners(lib, which, res_bits):
    """Each scalar corner for (m_id_scalar, e_id_scalar) and for (mq, eq), the per-channel table mid-range.  The residual is data: it holds
    the list's values for the scalar table.  For (mq, eq) the identity table is the exact ratio 1 + 2^-30 (b == r for r < 2^28, provably tie-free there) and the
    main branch contributes 0, so the QuantAct sees the residual itself."""
    from hawq_amd.quant_utils import tables_are_fast
    d = Driven(lib)
    a = d.a
    mid = R.Table(0x5A5A5A5B, 40, 0, 40, 31, 2 ** 31 - 1, True, (0,))
    L = R.plan((mid,), COUT)[0]
    d.load(L)
    one = ((1 << 30) + 1, 33 | 3 << 8)
    vmax = 65535 if res_bits == 16 else 2 ** 28 - 1
    res_t = dev(np.zeros((NPIX, COUT), np.uint16 if res_bits == 16 else np.int32))
    flags = out_buf(1, torch.int32, 0)
    out_res = out_buf(NPIX * COUT, torch.uint16 if res_bits == 16 else torch.int32, 0)
    out_q = out_buf(NPIX * COUT, torch.uint8, 0)
    a.epilogue, a.flags = lib.EPI_RESIDUAL, flags.data_ptr()
    a.res_in, a.res_in_bits, a.res_out, a.res_out_bits = res_t.data_ptr(), res_bits, out_res.data_ptr(), res_bits
    a.out_q, a.out_bits, a.q_lo, a.q_hi = out_q.data_ptr(), 8, 0, 127
    rng = np.random.default_rng(5)
    ran = {0: 0, 1: 0, 5: 0}
    for m, ek in R.SCALAR_TABLES:
        vals = scalar_values(m, ek, vmax, signed=False)
        res = rng.integers(0, min(vmax, (1 << (31 - (ek >> 8))) - 1) + 1, (NPIX, COUT)).astype(np.int64)
        res.reshape(-1)[:len(vals) * 37:37] = vals   # the listed values, spread over pixels and channels
        assert np.abs(res << (ek >> 8)).max() <= 2 ** 31 - 1 and set(vals) <= set(res.reshape(-1).tolist())
        put(res_t, res)
        if which == "id":
            (a.m_id_scalar, a.e_id_scalar), (a.mq, a.eq) = (m, ek), (0x5A5A5A5B, 40)
            o = np.maximum(L.Q + scalar(res, m, ek).T, 0)
        else:
            (a.m_id_scalar, a.e_id_scalar), (a.mq, a.eq) = one, (m, ek)
            assert np.array_equal(scalar(res, *one), res)
            o = np.maximum(L.Q + res.T, 0)
            assert np.abs(o << (ek >> 8)).max() <= 2 ** 31 - 1   # L.Q is 0 or -1 around zero: (-1 + r) stays inside
        ref_q = np.clip(scalar(o, int(a.mq), int(a.eq)), 0, 127)
        vb = int(o.max()).bit_length() if which == "q" else int(res.max()).bit_length()
        proved = tables_are_fast([m], [ek], max(vb, 1)) and (which == "id" or tables_are_fast([one[0]], [one[1]], 28))
        for fast in (0, 5) + ((1,) if proved else ()):
            a.fast_tables = fast
            for tile in generic_tiles(lib):
                flags.zero_(), stale(out_res), stale(out_q)
                d.run(tile)
                got = carrier(out_res)
                if res_bits == 16:
                    assert np.array_equal(got[o <= 65535], o[o <= 65535]) and (got[o > 65535] == 65535).all(), (m, ek, fast, tile)
                    assert bool(flags.item() & 1) == bool((o > 65535).any()), (m, ek, fast, tile)
                else:
                    assert np.array_equal(got, o), (m, ek, fast, tile)
                assert np.array_equal(cp(out_q), ref_q), (m, ek, fast, tile)
            ran[fast] += 1
    assert ran[0] == ran[5] == len(R.SCALAR_TABLES) and ran[1] >= 4


@pytest.mark.parametrize("clamp16", [0, 1])
@pytest.mark.parametrize("fast", [0, 1, 5])
def test_conv2d_signed_direct_epilogue_corners(lib, fast, clamp16):
    """MobileNetV2's closing epilogue (res_no_relu = 1, int32 carrier): negative values and negative exact ties reach the stored sum, and
    with res_clamp16 the results land on and beyond +-32768.  Without the clamp an identity is added (a signed int32 residual)."""
    from hawq_amd.quant_utils import tables_are_fast
    tables, launches = form_plan(fast)
    m1, e1, mq, eq = 0x5A5A5A5B, 34, 0x5A5A5A5B, 40
    assert tables_are_fast([m1], [e1], 17) and tables_are_fast([mq], [eq], 31)
    rng = np.random.default_rng(3)
    res = rng.integers(-60000, 60000, (NPIX, COUT)).astype(np.int64)
    d = Driven(lib)
    a = d.a
    keep = dict(res=dev(res.astype(np.int32)))
    out_res = out_buf(NPIX * COUT, torch.int32, 0)
    out_q = out_buf(NPIX * COUT, torch.uint8, 0)
    a.epilogue, a.fast_tables, a.res_no_relu, a.res_clamp16 = lib.EPI_RESIDUAL, fast, 1, clamp16
    if not clamp16:
        a.res_in, a.res_in_bits, a.m_id_scalar, a.e_id_scalar = keep['res'].data_ptr(), 32, m1, e1
    a.res_out, a.res_out_bits = out_res.data_ptr(), 32
    a.out_q, a.out_bits, a.q_lo, a.q_hi, a.mq, a.eq = out_q.data_ptr(), 8, -128, 127, mq, eq
    seen, neg_ties = set(), 0
    for L in launches:
        d.load(L)
        o = np.clip(L.Q, -32768, 32767) if clamp16 else L.Q + scalar(res, m1, e1).T
        seen |= {x for x in (-32769, -32768, 32767, 32768) if (L.Q == x).any()}
        e_, k_ = (L.ek & 0xff)[:, None], (L.ek >> 8)[:, None]
        neg_ties += int((((L.V << k_) * L.m[:, None]) & ((np.int64(1) << e_) - 1) == (np.int64(1) << (e_ - 1)))[L.V < 0].sum())
        ref_q = np.clip(scalar(o, mq, eq), -128, 127)
        for tile in generic_tiles(lib):
            stale(out_res), stale(out_q)
            d.run(tile)
            assert np.array_equal(carrier(out_res), o), (fast, clamp16, tile)
            assert np.array_equal(cp(out_q), ref_q), (fast, clamp16, tile)
    assert seen == {-32769, -32768, 32767, 32768}
    assert neg_ties >= (10 if fast != 1 else 0)


# ================================================================ 2. / 6. the special-purpose tiles and the split-K form
MID_ID, MID_Q = (0x5A5A5A5B, 34), (0x5A5A5A5B, 40)   # odd m: provably tie-free for 17-bit residuals / 31-bit sums, no pre-shift


def sweep(lib, d, fast, tiles, run, planar_out=(0, 1)):
    """Every launch of the form's plan through `run(tile)` with the REQUANT epilogue (both ReLU settings) and with the single-branch
    RESIDUAL epilogue on uint16 residuals (per-channel corners, mid-range scalar tables).  A tile that refuses the layer is skipped as a
    whole; returns the tiles that ran, per epilogue."""
    from hawq_amd.quant_utils import tables_are_fast
    assert tables_are_fast([MID_ID[0]], [MID_ID[1]], 17) and tables_are_fast([MID_Q[0]], [MID_Q[1]], 31)
    cout, a = d.cout, d.a
    tables, launches = form_plan(fast, cout)
    res = np.random.default_rng(cout).integers(0, 60000, (NPIX, cout)).astype(np.int64)
    res[::5] = 0
    idq = scalar(res, *MID_ID).T
    res_t = dev(res.astype(np.uint16))
    flags = out_buf(1, torch.int32, 0)
    out_res, out_q = out_buf(NPIX * cout, torch.uint16, 0), out_buf(NPIX * cout, torch.uint8, 0)
    a.fast_tables, a.out_q, a.out_bits, a.flags = fast, out_q.data_ptr(), 8, flags.data_ptr()
    (a.m_id_scalar, a.e_id_scalar), (a.mq, a.eq) = MID_ID, MID_Q

    def requant_form(relu, outp):
        a.epilogue, a.relu, a.out_planar, a.q_lo, a.q_hi = lib.EPI_REQUANT, relu, outp, -128, 127
        a.res_in, a.res_out = None, None

    def residual_form(outp):
        a.epilogue, a.relu, a.out_planar, a.q_lo, a.q_hi = lib.EPI_RESIDUAL, 0, outp, 0, 127
        a.res_in, a.res_in_bits, a.res_out, a.res_out_bits = res_t.data_ptr(), 16, out_res.data_ptr(), 16

    d.load(launches[0])
    requant_form(1, 0)
    took_q = [t for t in tiles if run(t)]
    residual_form(0)
    took_r = [t for t in took_q if run(t)]
    for L in launches:
        d.load(L)
        o = np.maximum(L.Q + idq, 0)
        ref_q = np.clip(scalar(o, *MID_Q), 0, 127)
        for tile in took_q:
            for relu in (0, 1):
                ref = np.clip(requant(np.maximum(L.V, 0), L) if relu else L.Q, -128, 127)
                for outp in planar_out:
                    requant_form(relu, outp)
                    stale(out_q)
                    assert run(tile), (tile, relu, outp)
                    assert np.array_equal(cp(out_q, 8, cout, bool(outp)), ref), (fast, tile, relu, outp)
        for tile in took_r:
            for outp in planar_out:
                residual_form(outp)
                flags.zero_(), stale(out_res), stale(out_q)
                assert run(tile), (tile, outp)
                got = carrier(out_res, cout)
                assert np.array_equal(got[o <= 65535], o[o <= 65535]) and (got[o > 65535] == 65535).all(), (fast, tile, outp)
                assert bool(flags.item() & 1) == bool((o > 65535).any()), (fast, tile, outp)
                assert np.array_equal(cp(out_q, 8, cout, bool(outp)), ref_q), (fast, tile, outp)
    return took_q, took_r


@pytest.mark.parametrize("fast", [1, 5])
@pytest.mark.parametrize("family", ["band", "band2", "gemm2"])
def test_special_purpose_tiles_at_the_corners(lib, family, fast):
    """The 3x3 band tiles and the weight-stationary kernel (Cin = 64), the band_v2 tiles (Cin = 128, planar input, wgt_band) and the
    streaming 1x1 tiles (Cin = 128, wgt_k128): REQUANT and single-branch RESIDUAL in the tie-free and the exact-tie instantiation.
    Cout = 64 and 128, so that every tile id of the family meets a layer it is built for."""
    import tests.test_gpu_band2 as B2
    import tests.test_gpu_gemm2 as G2
    ntiles, nband = lib.load().hawq_conv2d_num_tiles(), lib.load().hawq_conv2d_num_band_tiles()
    ids, cin, k, layout = {"band": (list(range(ntiles - nband + 1, ntiles - nband + 1 + len(K.BAND_GEOM))), 64, 3, "nhwc"),
                           "band2": (B2._ids(lib), 128, 3, "band2"), "gemm2": (G2._ids(lib), 128, 1, "k128")}[family]
    ran_q, ran_r = set(), set()
    for cout in (64, 128):
        d = Driven(lib, cin, cout, k, layout)
        q, r = sweep(lib, d, fast, ids, d.try_run)
        ran_q |= set(q)
        ran_r |= set(r)
    assert ran_q == set(ids) and ran_r == set(ids), (ids, ran_q, ran_r)


@pytest.mark.parametrize("fast", [1, 5, 0])
def test_splitk_plumbs_the_tables_through(lib, fast):
    """hawq_conv2d_splitk, two K slices: it shares the epilogues, this checks its own parameter plumbing in each table mode."""
    d = Driven(lib, 128, COUT)
    d.a.epilogue, d.a.out_q, d.a.out_bits = lib.EPI_REQUANT, d.m.data_ptr(), 8   # (any non-null pointer: the workspace query reads the geometry only)
    ws = SK.workspace(lib, d.a, 2)

    def run(tile):
        SK.splitk(lib, d.a, 2, ws)
        return True

    q, r = sweep(lib, d, fast, [0], run, planar_out=(0,))
    assert q == [0] and r == [0]
    assert int(ws[1].abs().sum()) == 0   # every arrival counter back at zero


# ================================================================================== 5. the depthwise kernels
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("form", ["generic", 1, 5])
def test_depthwise_requant_at_the_corners(lib, form, stride):
    """hawq_depthwise3x3_requant (exact form: both ReLU settings, signed clamp) and hawq_depthwise3x3_requant_fast (fast_tables 1 on the
    provably tie-free tables, 5 on all): C = 64, centre-tap weights, a 16 x 16 output map (stride 2 reads every other pixel of a
    32 x 32 input whose sampled pixels carry the offsets)."""
    from hawq_amd.packing import pack_ctab
    c = 64
    tables, launches = form_plan(0 if form == "generic" else form, c)
    hin = HW * stride
    x = {}
    for kind, off in R.OFFSETS.items():
        full = np.full((1, hin, hin, c), 77, np.int8)   # pixels the stride skips meet zero weights
        full[0, ::stride, ::stride, :] = off.reshape(HW, HW, 1)
        x[kind] = dev(np.concatenate([full.reshape(-1), np.zeros(64, np.int8)]))
    w9 = np.zeros((9, c), np.int8)
    w9[4] = 1
    w9, bias, m, e, ctab = dev(w9), dev(np.zeros(c, np.int32)), dev(np.zeros(c, np.int32)), dev(np.zeros(c, np.int32)), dev(np.zeros((c, 4), np.int32))
    out = out_buf(NPIX * c, torch.int8, 0)
    for L in launches:
        R.check_contract(L.V, L.m, L.ek)
        put(bias, i32(L.bias)), put(m, i32(L.m)), put(e, i32(L.ek)), put(ctab, pack_ctab(L.bias, L.m, L.ek))
        for relu in ((0, 1) if form == "generic" else (1,)):
            lo, hi = ((-128, 127) if not relu else (-100, 100)) if form == "generic" else (0, 127)
            ref = np.clip(requant(np.maximum(L.V, 0), L) if relu else L.Q, lo, hi)
            stale(out)
            if form == "generic":
                lib.call("hawq_depthwise3x3_requant", x[L.kind].data_ptr(), w9.data_ptr(), bias.data_ptr(), m.data_ptr(), e.data_ptr(), 1, hin, hin, c, c,
                         stride, relu, lo, hi, out.data_ptr(), None, K.stream())
            else:
                lib.call("hawq_depthwise3x3_requant_fast", x[L.kind].data_ptr(), w9.data_ptr(), ctab.data_ptr(), form, 1, hin, hin, c, c, stride, lo, hi,
                         out.data_ptr(), K.stream())
            got = out.cpu().numpy().astype(np.int64).reshape(NPIX, c).T
            assert np.array_equal(got, ref), (form, stride, relu)


# ================================================================================== 3. hawq_conv_expand_reduce
UNIT = ((1 << 30) + 1, 33 | 3 << 8)   # the ratio 1 + 2^-30: rne(v * ratio) == v for |v| < 2^28, provably tie-free there; an ids0_form table


def mid_table(c, m=0x5A5A5A5B, ek=40):
    return np.full(c, m, np.int64), np.full(c, ek, np.int64)


class Pair:
    """The fused expand (RESIDUAL) + reduce (REQUANT) launch on c = 64 -> c3 = 256 -> 64 channels, F._case's layout, with 0/1 diagonal
    weights in both convs: acc3[p][j] = b3[j] + x[p][j mod c] and acc1[p][i] = b1[i] + q[p][i]."""

    def __init__(self, lib, c=64, c3=256):
        from hawq_amd.packing import pack_conv_weight, pack_ctab
        self.lib, self.c, self.c3, self.pack_ctab = lib, c, c3, pack_ctab
        w1 = np.zeros((c, c3, 1, 1), np.int64)
        w1[np.arange(c), np.arange(c), 0, 0] = 1
        self.x = {kind: dev(K.pack_act(image(R.OFFSETS[kind], c), 8)) for kind in ("relu", "tiny_relu")}
        self.x["zero"] = dev(np.zeros(NPIX * c, np.uint8))
        self.t = dict(w3=dev(pack_conv_weight(diagonal(c3, c), 8)), w1=dev(pack_conv_weight(w1, 8)),
                      b3=dev(np.zeros(c3, np.int32)), m3=dev(np.zeros(c3, np.int32)), e3=dev(np.zeros(c3, np.int32)), ctab3=dev(np.zeros((c3, 4), np.int32)),
                      b1=dev(np.zeros(c, np.int32)), m1=dev(np.zeros(c, np.int32)), e1=dev(np.zeros(c, np.int32)), ctab1=dev(np.zeros((c, 4), np.int32)),
                      res=dev(np.zeros((NPIX, c3), np.uint16)), flags=out_buf(1, torch.int32, 0),
                      res_out=out_buf(NPIX * c3, torch.uint16, 0), y=out_buf(NPIX * c, torch.uint8, 0))
        t = self.t
        self.args = a = lib.ExpandReduceArgs()
        ex, rd = a.expand, a.reduce
        ex.wgt, ex.bias, ex.m, ex.e, ex.ctab, ex.flags = (t[k].data_ptr() for k in ("w3", "b3", "m3", "e3", "ctab3", "flags"))
        ex.N, ex.H, ex.W, ex.Cin, ex.Cout, ex.KH, ex.KW, ex.stride, ex.pad, ex.in_bits, ex.w_bits = 1, HW, HW, c, c3, 1, 1, 1, 0, 8, 8
        ex.epilogue, ex.res_in, ex.res_in_bits, ex.res_out, ex.res_out_bits = lib.EPI_RESIDUAL, t['res'].data_ptr(), 16, t['res_out'].data_ptr(), 16
        ex.out_bits, ex.q_lo, ex.q_hi = 8, 0, 127
        rd.wgt, rd.bias, rd.m, rd.e, rd.ctab, rd.out_q = (t[k].data_ptr() for k in ("w1", "b1", "m1", "e1", "ctab1", "y"))
        rd.N, rd.H, rd.W, rd.Cin, rd.Cout, rd.KH, rd.KW, rd.stride, rd.pad, rd.in_bits, rd.w_bits = 1, HW, HW, c3, c, 1, 1, 1, 0, 8, 8
        rd.epilogue, rd.out_bits = lib.EPI_REQUANT, 8

    def check(self, kind, exp, res, ident, nextq, red, relu, clamp, fast, what):
        """Upload (bias, m, ek) of both convs, the residual and the scalar tables; run every variant, NHWC and planar; compare res_out,
        the flag and the reduce conv's output with the exact chain.  Returns the QK0 predicate of the launch."""
        a, t, c, c3 = self.args, self.t, self.c, self.c3
        ex, rd = a.expand, a.reduce
        off = R.OFFSETS[kind] if kind != "zero" else np.zeros(NPIX, np.int64)
        (b3, m3, ek3), (b1, m1, ek1) = exp, red
        V3 = b3[:, None] + off[None, :]
        R.check_contract(V3, m3, ek3), R.check_contract(res.T, [ident[0]], [ident[1]])
        o = np.maximum(R.np_rne(V3, m3[:, None], (ek3 & 0xff)[:, None], (ek3 >> 8)[:, None]) + scalar(res, *ident).T, 0)
        R.check_contract(o, [nextq[0]], [nextq[1]])
        q = np.clip(scalar(o, *nextq), 0, 127)
        V1 = b1[:, None] + q[:c]
        R.check_contract(V1, m1, ek1)
        y = np.clip(R.np_rne(np.maximum(V1, 0) if relu else V1, m1[:, None], (ek1 & 0xff)[:, None], (ek1 >> 8)[:, None]), *clamp)
        for name, v in (("b3", b3), ("m3", m3), ("e3", ek3), ("b1", b1), ("m1", m1), ("e1", ek1), ("res", res)):
            put(t[name], i32(v) if name != "res" else v)
        put(t['ctab3'], self.pack_ctab(b3, m3, ek3)), put(t['ctab1'], self.pack_ctab(b1, m1, ek1))
        ex.in_ = self.x[kind].data_ptr()
        (ex.m_id_scalar, ex.e_id_scalar), (ex.mq, ex.eq) = ident, nextq
        ex.fast_tables = rd.fast_tables = fast
        rd.relu, rd.q_lo, rd.q_hi = relu, clamp[0], clamp[1]
        nvar = self.lib.load().hawq_conv_expand_reduce_variants(C.byref(a))
        assert nvar >= 3
        for tile in range(0, nvar + 1):
            for planar in (0, 1):
                a.tile, rd.out_planar = tile, planar
                t['flags'].zero_(), stale(t['res_out']), stale(t['y'])
                self.lib.call("hawq_conv_expand_reduce", C.byref(a), K.stream())
                got = carrier(t['res_out'], c3)
                assert np.array_equal(got[o <= 65535], o[o <= 65535]) and (got[o > 65535] == 65535).all(), (what, fast, tile, planar)
                assert bool(t['flags'].item() & 1) == bool((o > 65535).any()), (what, fast, tile, planar)
                assert np.array_equal(cp(t['y'], 8, c, bool(planar)), y), (what, fast, tile, planar)
        return (nextq[1] >> 8) == 0 and R.ids0_form(ident[1])   # fused_er2.hip / fused_wp.hip: the QK0 instantiations


@pytest.mark.parametrize("fast", [1, 5, 9, 13])
def test_expand_reduce_expand_tables_at_the_corners(lib, fast):
    """The expand conv's per-channel tables at the corners (fast_tables 1, 5 and with bit 3 on the k = 0 subset), mid-range scalar and
    reduce tables; the identity table in and out of ids0_form and (mq, eq) with and without a pre-shift, so that both the SC0 / QK0
    instantiations and the others run."""
    pair = Pair(lib)
    tables = tuple(t for t in R.TABLES if FORMS[fast](t))
    launches = R.plan(tables, pair.c3, relu_inputs=True)
    assert R.coverage(launches, tables) == {(i, v) for i, t in enumerate(tables) for v in t.values}
    res = np.random.default_rng(33).integers(0, 30000, (NPIX, pair.c3)).astype(np.int64)
    res[::3] = 0
    red = (np.arange(pair.c, dtype=np.int64) * 3 - 40,) + mid_table(pair.c, ek=33)
    qk0 = set()
    # (0x5A5A5A5B, 33 | 1 << 8): ratio 0.35 in ids0_form; MID_ID: ratio 0.09, not; (0x5A5A5A5B, 41 | 1 << 8): (mq, eq) with a pre-shift (o < 2^30)
    combos = ((MID_ID, MID_Q), ((0x5A5A5A5B, 33 | 1 << 8), MID_Q), ((0x5A5A5A5B, 33 | 1 << 8), (0x5A5A5A5B, 41 | 1 << 8)))
    for i, L in enumerate(launches):
        for ident, nextq in (combos if i == 0 else combos[i % 3:i % 3 + 1]):   # the first launch under all three, the others in turn
            qk0.add(pair.check(L.kind, (L.bias, L.m, L.ek), res, ident, nextq, red, 1, (-128, 127), fast, ("expand", i)))
    assert qk0 == {True, False}


@pytest.mark.parametrize("fast", [1, 5, 9, 13])
def test_expand_reduce_reduce_tables_at_the_corners(lib, fast):
    """The reduce conv's per-channel tables at the corners, centred by its bias on the q values the expand side produces: the expand
    conv contributes 0 (m = 0), the residual carries the offsets 0 .. 127 through unit identity and QuantAct tables, so q[p][i] is the
    offset of pixel p.  Both ReLU settings of the reduce conv, int8 and (0, 15) clamps."""
    pair = Pair(lib)
    tables = tuple(t for t in R.TABLES if FORMS[fast](t))
    launches = R.plan(tables, pair.c, relu_inputs=True)
    assert R.coverage(launches, tables) == {(i, v) for i, t in enumerate(tables) for v in t.values}
    zero = (np.zeros(pair.c3, np.int64), np.zeros(pair.c3, np.int64), np.full(pair.c3, 33, np.int64))
    for i, L in enumerate(launches):
        res = np.broadcast_to(L.off.reshape(NPIX, 1), (NPIX, pair.c3)).copy()
        relu, clamp = ((1, (-128, 127)), (0, (-128, 127)), (1, (0, 15)))[i % 3]
        pair.check("zero", zero, res, UNIT, UNIT, (L.bias, L.m, L.ek), relu, clamp, fast, ("reduce", i))


@pytest.mark.parametrize("which", ["id", "q"])
def test_expand_reduce_scalar_corners(lib, which):
    """Every scalar corner for the identity table and for (mq, eq), per-channel tables mid-range: fast_tables 5 always, 1 where the
    proof covers the scalar table for the values it meets.  Both values of the QK0 predicate occur."""
    from hawq_amd.quant_utils import tables_are_fast
    pair = Pair(lib)
    c, c3 = pair.c, pair.c3
    exp = (np.arange(c3, dtype=np.int64) % 7,) + mid_table(c3)           # a = rne(small * 0.0014) = 0
    red = (np.arange(c, dtype=np.int64) * 3 - 40,) + mid_table(c, ek=33)
    rng = np.random.default_rng(9)
    qk0, proved_n = set(), 0
    for m, ek in R.SCALAR_TABLES:
        lim = min(65535, (1 << (31 - (ek >> 8))) - 1)
        vals = scalar_values(m, ek, 65535, signed=False)
        res = rng.integers(0, lim + 1, (NPIX, c3)).astype(np.int64)
        res.reshape(-1)[:len(vals) * 41:41] = vals
        ident, nextq = ((m, ek), MID_Q) if which == "id" else (UNIT, (m, ek))
        proved = tables_are_fast([m], [ek], 16)
        proved_n += int(proved)
        for fast in (5, 1) if proved else (5,):
            qk0.add(pair.check("relu", exp, res, ident, nextq, red, 1, (-128, 127), fast, (which, m, ek)))
    assert qk0 == {True, False} and proved_n >= 4


# ================================================================================== 4. hawq_linear_bottleneck
def unit_table(c):
    return (np.zeros(c, np.int64),) + mid_table(c, *UNIT)   # bias 0, ratio 1 + 2^-30: the layer passes small integers through


class Unit:
    """One linear-bottleneck launch (MB's setup) with 0/1 diagonal 1x1 weights and centre-tap depthwise weights on a 16 x 16 output
    map: hidden channel j sees b1[j] + x[p][j mod cin], the depthwise conv b2[j] + h1[p][j], output channel i b3[i] + h2[p][i].
    Stride 2 reads every other pixel of a 32 x 32 input whose sampled pixels carry the offsets."""

    def __init__(self, lib, widths, stride, identity):
        from hawq_amd.packing import pack_conv_weight, pack_ctab
        cin, ip, hid, cout, op = widths
        self.lib, self.pack_ctab, self.widths, self.identity = lib, pack_ctab, widths, identity
        cin_p, hid_p, cout_p = (-(-v // 64) * 64 for v in (cin, hid, cout))
        self.hid_p, self.cout_p = hid_p, cout_p
        hin = HW * stride
        self.x = {}
        for kind in ("relu", "tiny_relu"):
            full = np.full((hin, hin, ip), 55, np.int8)   # pixels the stride skips never reach an output (centre tap only)
            full[::stride, ::stride, :] = R.OFFSETS[kind].reshape(HW, HW, 1)
            self.x[kind] = dev(np.concatenate([full.reshape(-1), np.zeros(64, np.int8)]))
        w1 = np.zeros((hid, cin, 1, 1), np.int64)
        w1[np.arange(hid), np.arange(hid) % cin, 0, 0] = 1
        w3 = np.zeros((cout, hid, 1, 1), np.int64)
        w3[np.arange(cout), np.arange(cout), 0, 0] = 1
        w9 = np.zeros((9, hid_p), np.int8)
        w9[4, :hid] = 1
        self.t = t = dict(w1=dev(pack_conv_weight(w1, 8, cin_p, hid_p)), w9=dev(w9), w3=dev(pack_conv_weight(w3, 8, hid_p, cout_p)),
                          ct1=dev(np.zeros((hid_p, 4), np.int32)), ct2=dev(np.zeros((hid_p, 4), np.int32)), ct3=dev(np.zeros((cout_p, 4), np.int32)),
                          res=dev(np.zeros(NPIX * op + 64, np.int32)), out16=out_buf(NPIX * op, torch.int32, 0), out_q=out_buf(NPIX * op, torch.int8, 0))
        self.b = b = lib.BottleneckArgs()
        e, q = b.expand, b.project
        e.wgt, e.ctab = t['w1'].data_ptr(), t['ct1'].data_ptr()
        e.N, e.H, e.W, e.Cin, e.Cout, e.KH, e.KW, e.stride, e.pad, e.in_bits, e.w_bits = 1, hin, hin, cin_p, hid_p, 1, 1, 1, 0, 8, 8
        e.in_pitch = ip if ip != cin_p else 0
        e.epilogue, e.relu, e.q_lo, e.q_hi, e.out_bits = lib.EPI_REQUANT, 1, 0, 127, 8
        b.dw_wgt9c, b.dw_ctab, b.dw_stride, b.dw_q_lo, b.dw_q_hi, b.c_mid = t['w9'].data_ptr(), t['ct2'].data_ptr(), stride, 0, 127, hid
        q.wgt, q.ctab = t['w3'].data_ptr(), t['ct3'].data_ptr()
        q.N, q.H, q.W, q.Cin, q.Cout, q.KH, q.KW, q.stride, q.pad, q.in_bits, q.w_bits = 1, HW, HW, hid_p, cout_p, 1, 1, 1, 0, 8, 8
        q.out_pitch = op if op != cout_p else 0
        q.epilogue, q.res_no_relu, q.res_clamp16 = lib.EPI_RESIDUAL, 1, int(not identity)
        q.res_out, q.res_out_bits, q.out_q, q.out_bits, q.q_lo, q.q_hi = t['out16'].data_ptr(), 32, t['out_q'].data_ptr(), 8, -128, 127
        if identity:
            q.res_in, q.res_in_bits = t['res'].data_ptr(), 32

    def check(self, kind, t1, t2, t3, res, ident, nextq, fast, what, tiles=(0, 1, 2, 3, 4)):
        cin, ip, hid, cout, op = self.widths
        b, t = self.b, self.t
        off = R.OFFSETS[kind]

        def layer(V, tab):
            R.check_contract(V, tab[1], tab[2])
            return R.np_rne(V, tab[1][:, None], (tab[2] & 0xff)[:, None], (tab[2] >> 8)[:, None])

        h1 = np.clip(layer(t1[0][:, None] + off[None, :], t1), 0, 127)
        h2 = np.clip(layer(t2[0][:, None] + h1, t2), 0, 127)
        v = layer(t3[0][:, None] + h2[:cout], t3)
        if self.identity:
            R.check_contract(res.T, [ident[0]], [ident[1]])
            v = v + scalar(res, *ident).T
            full = np.zeros((NPIX, op), np.int64)
            full[:, :cout] = res
            put(t['res'][:NPIX * op], full)
            b.project.m_id_scalar, b.project.e_id_scalar = ident
        else:
            v = np.clip(v, -32768, 32767)
        R.check_contract(v, [nextq[0]], [nextq[1]])
        ref_q = np.clip(scalar(v, *nextq), -128, 127)
        for name, tab, cp_ in (("ct1", t1, self.hid_p), ("ct2", t2, self.hid_p), ("ct3", t3, self.cout_p)):
            pad = lambda a, fill=0: np.concatenate([np.asarray(a, np.int64), np.full(cp_ - len(a), fill, np.int64)])
            put(t[name], self.pack_ctab(pad(tab[0]), pad(tab[1]), pad(tab[2], 33)))
        b.expand.in_ = self.x[kind].data_ptr()
        b.project.mq, b.project.eq = nextq
        b.expand.fast_tables = b.dw_fast_tables = b.project.fast_tables = fast
        for tile in tiles:
            b.tile = tile
            assert self.lib.load().hawq_linear_bottleneck_ok(C.byref(b)) == 1, (what, tile, self.lib.load().hawq_last_error().decode())
            stale(t['out16']), stale(t['out_q'])
            self.lib.call("hawq_linear_bottleneck", C.byref(b), K.stream())
            got = t['out16'].cpu().numpy().astype(np.int64).reshape(NPIX, op)[:, :cout].T
            assert np.array_equal(got, v), (what, fast, tile)
            gq = t['out_q'].cpu().numpy().astype(np.int64).reshape(NPIX, op)[:, :cout].T
            assert np.array_equal(gq, ref_q), (what, fast, tile)
        return v


UNITS = {"wide": (64, 64, 384, 64, 64), "narrow": (32, 32, 32, 16, 16)}


@pytest.mark.parametrize("fast", [1, 5])
@pytest.mark.parametrize("stride,identity", [(1, True), (2, False)])
@pytest.mark.parametrize("layer", ["expand", "depthwise", "project"])
@pytest.mark.parametrize("unit", sorted(UNITS))
def test_linear_bottleneck_tables_at_the_corners(lib, unit, layer, stride, identity, fast):
    """Tiles 0 to 4 on a 64 -> 384 -> 64 unit and on a narrow (32, 32, 32, 16, 16) one, stride 1 with identity and stride 2 without:
    the corners on the expand, depthwise and project tables in turn, the other two passing their integers through.  On the project
    side negative values and negative exact ties reach the stored int32 sum."""
    cin, ip, hid, cout, op = widths = UNITS[unit]
    u = Unit(lib, widths, stride, identity)
    n = cout if layer == "project" else hid
    tables = tuple(t for t in R.TABLES if FORMS[fast](t))
    launches = R.plan(tables, n, relu_inputs=True)
    assert R.coverage(launches, tables) == {(i, v) for i, t in enumerate(tables) for v in t.values}
    res = np.random.default_rng(hid).integers(-30000, 30000, (NPIX, cout)).astype(np.int64)
    neg_ties = 0
    for i, L in enumerate(launches):
        corner = (L.bias, L.m, L.ek)
        t1, t2, t3 = (corner if layer == "expand" else unit_table(hid), corner if layer == "depthwise" else unit_table(hid),
                      corner if layer == "project" else unit_table(cout))
        u.check(L.kind, t1, t2, t3, res, MID_ID, MID_Q, fast, (unit, layer, i), tiles=(0, 1, 2, 3, 4) if i % 4 == 0 else (i % 5,))
        e_, k_ = (L.ek & 0xff)[:, None], (L.ek >> 8)[:, None]
        neg_ties += int((((L.V << k_) * L.m[:, None]) & ((np.int64(1) << e_) - 1) == (np.int64(1) << (e_ - 1)))[L.V < 0].sum())
    assert layer != "project" or fast == 1 or neg_ties >= 10


@pytest.mark.parametrize("which", ["id", "q"])
@pytest.mark.parametrize("unit", sorted(UNITS))
def test_linear_bottleneck_scalar_corners(lib, unit, which):
    """Every scalar corner for the identity table and for the next QuantAct (stride 1, identity): the residual is signed int32 data
    holding the list's values; for (mq, eq) it reaches the QuantAct through a unit identity table while the convs contribute 0."""
    from hawq_amd.quant_utils import tables_are_fast
    cin, ip, hid, cout, op = widths = UNITS[unit]
    u = Unit(lib, widths, 1, True)
    zero3 = (np.zeros(cout, np.int64), np.zeros(cout, np.int64), np.full(cout, 33, np.int64))
    rng = np.random.default_rng(cout)
    proved_n = 0
    for j, (m, ek) in enumerate(R.SCALAR_TABLES):
        lim = min(2 ** 28 - 1, (1 << (31 - (ek >> 8))) - 1)
        vals = scalar_values(m, ek, 2 ** 28 - 1, signed=True)
        res = rng.integers(-lim, lim + 1, (NPIX, cout)).astype(np.int64)
        res.reshape(-1)[:len(vals) * 29:29] = vals
        assert set(vals) <= set(res.reshape(-1).tolist())
        ident, nextq = ((m, ek), MID_Q) if which == "id" else (UNIT, (m, ek))
        proved = tables_are_fast([m], [ek], lim.bit_length())
        proved_n += int(proved)
        for fast in (5, 1) if proved else (5,):
            u.check("relu", unit_table(hid), unit_table(hid), zero3, res, ident, nextq, fast, (unit, which, m, ek), tiles=(0, 1 + j % 4))
    assert proved_n >= 4


# ================================================================================== 7. the fused stems
def stem_image(off, hin, step):
    """fp32 [1][3][hin][hin] whose channel-0 pixels (step * Y, step * X) hold the offsets and every other pixel -128: with a single-tap
    weight the conv output at the sampled pixels is the offset, and the 3x3 / 2 max-pool (where there is one) picks it"""
    x = np.full((1, 3, hin, hin), -128, np.float32)
    x[0, 0, ::step, ::step] = off.reshape(HW, HW)
    return x


def scalar_plan(m, ek, vmax, c):
    """launches of unit per-channel tables whose biases walk the pixels' offsets 0 .. 127 across the list's values for one scalar table"""
    e, k = ek & 0xff, ek >> 8
    lim = min((1 << (31 - k)) - 1, vmax)
    t = R.Table(m, e, k, ek, 31 - k, lim, False, tuple(scalar_values(m, ek, vmax, signed=False)))
    cs = R.centres(t, (0, 127))
    out = []
    for at in range(0, len(cs), c):
        part = cs[at:at + c]
        out.append(np.array(part + [part[0]] * (c - len(part)), np.int64))
    assert set(t.values) <= {int(b) + o for bias in out for b in bias for o in range(128)}
    return out


@pytest.mark.parametrize("out_bits", [8, 4])
@pytest.mark.parametrize("fast", [0, 1])
def test_stem_fused_per_channel_corners(lib, fast, out_bits):
    """hawq_stem_fused: per-channel corners through the bias with a single-tap weight; the expectation takes the pooled maximum of the
    raw accumulators before the requant, as the kernel's header says."""
    from hawq_amd.packing import pack_stem_weight
    tables, launches = form_plan(fast, 64)
    wt = np.zeros((64, 3, 7, 7), np.int64)
    wt[:, 0, 3, 3] = 1
    x = {kind: dev(stem_image(R.OFFSETS[kind], 64, 4)) for kind in ("int8", "tiny")}
    wd, bd, md, ed = dev(pack_stem_weight(wt)), dev(np.zeros(64, np.int32)), dev(np.zeros(64, np.int32)), dev(np.zeros(64, np.int32))
    res, qo = out_buf(NPIX * 64, torch.uint16, 0), out_buf(NPIX * 64 * out_bits // 8, torch.uint8, 0)
    lo, hi = (-128, 127) if out_bits == 8 else (0, 15)
    mq, eq = 0x5A5A5A5B, 37   # ratio 0.011 on values up to 32767; odd m, provably tie-free for 16-bit values
    for L in launches:
        R.check_contract(L.V, L.m, L.ek)
        put(bd, i32(L.bias)), put(md, i32(L.m)), put(ed, i32(L.ek))
        v = np.maximum(np.clip(L.Q, -32768, 32767), 0)
        stale(res), stale(qo)
        lib.call("hawq_stem_fused", x[L.kind].data_ptr(), 1, 3, 64, 64, 1.0, -128, 127, wd.data_ptr(), bd.data_ptr(), md.data_ptr(), ed.data_ptr(),
                 -32768, 32767, res.data_ptr(), qo.data_ptr(), out_bits, mq, eq, lo, hi, fast, K.stream())
        assert np.array_equal(carrier(res, 64), v), fast
        assert np.array_equal(cp(qo, out_bits, 64), np.clip(scalar(v, mq, eq), lo, hi)), fast


@pytest.mark.parametrize("fast", [0, 1])
def test_stem_fused_scalar_corners(lib, fast):
    """(mq, eq) at every scalar corner: unit per-channel tables make the 16-bit activation the bias plus the pixel's offset."""
    from hawq_amd.packing import pack_stem_weight
    from hawq_amd.quant_utils import tables_are_fast
    wt = np.zeros((64, 3, 7, 7), np.int64)
    wt[:, 0, 3, 3] = 1
    x = dev(stem_image(R.OFFSETS["relu"], 64, 4))
    _, um, uek = unit_table(64)
    wd, bd, md, ed = dev(pack_stem_weight(wt)), dev(np.zeros(64, np.int32)), dev(i32(um)), dev(i32(uek))
    res, qo = out_buf(NPIX * 64, torch.uint16, 0), out_buf(NPIX * 64, torch.uint8, 0)
    ran = 0
    for m, ek in R.SCALAR_TABLES:
        if fast and not tables_are_fast([m], [ek], 15):
            continue
        for bias in scalar_plan(m, ek, 32767, 64):
            V = bias[:, None] + R.OFFSETS["relu"][None, :]
            R.check_contract(V, um, uek), R.check_contract(V, [m], [ek])
            assert V.min() >= 0 and V.max() <= 32767
            put(bd, i32(bias))
            stale(res), stale(qo)
            lib.call("hawq_stem_fused", x.data_ptr(), 1, 3, 64, 64, 1.0, -128, 127, wd.data_ptr(), bd.data_ptr(), md.data_ptr(), ed.data_ptr(),
                     -32768, 32767, res.data_ptr(), qo.data_ptr(), 8, m, ek, -128, 127, fast, K.stream())
            assert np.array_equal(carrier(res, 64), V), (m, ek)
            assert np.array_equal(cp(qo, 8, 64), np.clip(scalar(V, m, ek), -128, 127)), (m, ek)
        ran += 1
    assert ran >= (len(R.SCALAR_TABLES) if not fast else 4)


def stem3x3_args(lib, wd, ctab, out16, out_q, fast):
    a = lib.ConvArgs()
    a.wgt, a.ctab = wd.data_ptr(), ctab.data_ptr()
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad, a.in_bits, a.w_bits = 1, HW, HW, 64, 64, 1, 1, 1, 0, 8, 8
    a.epilogue, a.res_no_relu, a.res_clamp16, a.fast_tables, a.out_pitch = lib.EPI_RESIDUAL, 0, 1, fast, 32
    a.res_out, a.res_out_bits, a.out_q, a.out_bits, a.q_lo, a.q_hi = out16.data_ptr(), 32, out_q.data_ptr(), 8, 0, 127
    return a


def stem3x3_setup(lib):
    from hawq_amd.packing import pack_conv_weight
    wrow = np.zeros((32, 27, 1, 1), np.int64)
    wrow[:, (1 * 3 + 1) * 3 + 0] = 1   # the centre tap of channel 0 in (kh, kw, c) order
    return dev(pack_conv_weight(wrow, 8, 64, 64)), dev(np.zeros((64, 4), np.int32)), out_buf(NPIX * 32, torch.int32, 0), out_buf(NPIX * 32, torch.int8, 0)


def pad64(a, fill=0):
    return np.concatenate([np.asarray(a, np.int64), np.full(64 - len(a), fill, np.int64)])


@pytest.mark.parametrize("fast", [1, 5])
def test_stem3x3s2_per_channel_corners(lib, fast):
    """hawq_stem3x3s2: 32 real channels, per-channel corners through the fused constants, ReLU and the 16-bit clamp behind them."""
    from hawq_amd.packing import pack_ctab
    tables, launches = form_plan(fast, 32)
    wd, ctab, out16, out_q = stem3x3_setup(lib)
    x = {kind: dev(stem_image(R.OFFSETS[kind], 32, 2)) for kind in ("int8", "tiny")}
    a = stem3x3_args(lib, wd, ctab, out16, out_q, fast)
    a.mq, a.eq = 0x5A5A5A5B, 37
    for L in launches:
        R.check_contract(L.V, L.m, L.ek)
        put(ctab, pack_ctab(pad64(L.bias), pad64(L.m), pad64(L.ek, 33)))
        v = np.clip(np.maximum(L.Q, 0), -32768, 32767)
        xp = x[L.kind].data_ptr()
        assert lib.load().hawq_stem3x3s2_ok(xp, None, None, 32, 32, C.byref(a)) == 1
        stale(out16), stale(out_q)
        lib.call("hawq_stem3x3s2", xp, None, None, 32, 32, 1.0, -128, 127, C.byref(a), K.stream())
        assert np.array_equal(carrier(out16, 32), v), fast
        assert np.array_equal(carrier(out_q, 32), np.clip(scalar(v, int(a.mq), int(a.eq)), 0, 127)), fast


def test_stem3x3s2_scalar_corners(lib):
    from hawq_amd.packing import pack_ctab
    from hawq_amd.quant_utils import tables_are_fast
    wd, ctab, out16, out_q = stem3x3_setup(lib)
    x = dev(stem_image(R.OFFSETS["relu"], 32, 2))
    _, um, uek = unit_table(32)
    proved_n = 0
    for m, ek in R.SCALAR_TABLES:
        proved = bool(tables_are_fast([m], [ek], 15))
        proved_n += proved
        for fast in (5, 1) if proved else (5,):
            a = stem3x3_args(lib, wd, ctab, out16, out_q, fast)
            a.mq, a.eq = m, ek
            for bias in scalar_plan(m, ek, 32767, 32):
                V = bias[:, None] + R.OFFSETS["relu"][None, :]
                R.check_contract(V, um, uek), R.check_contract(V, [m], [ek])
                put(ctab, pack_ctab(pad64(bias), pad64(um), pad64(uek, 33)))
                stale(out16), stale(out_q)
                lib.call("hawq_stem3x3s2", x.data_ptr(), None, None, 32, 32, 1.0, -128, 127, C.byref(a), K.stream())
                assert np.array_equal(carrier(out16, 32), V), (m, ek, fast)
                assert np.array_equal(carrier(out_q, 32), np.clip(scalar(V, m, ek), 0, 127)), (m, ek, fast)
    assert proved_n >= 4


# ================================================================================== 8. the InceptionV3 entries (dyadic_rne everywhere)
class Incep:
    """the driven 1x1 conv as a hawq_incep_conv argument block: int8 NHWC input, [Cout][1][1][Cin] diagonal weights"""

    def __init__(self, lib, cout=COUT, cin=CIN):
        self.lib, self.cout = lib, cout
        self.x = {kind: dev(np.ascontiguousarray(image(R.OFFSETS[kind], cin).transpose(0, 2, 3, 1)).astype(np.int8)) for kind in ("int8", "tiny")}
        self.w = dev(diagonal(cout, cin).reshape(cout, cin).astype(np.int8))

    def member(self, out, out_bits):
        t = dict(b=dev(np.zeros(self.cout, np.int32)), m=dev(np.zeros(self.cout, np.int32)), ek=dev(np.zeros(self.cout, np.int32)))
        a = self.lib.IncepConvArgs()
        a.wgt, a.bias, a.m, a.ek, a.out = self.w.data_ptr(), t['b'].data_ptr(), t['m'].data_ptr(), t['ek'].data_ptr(), out.data_ptr()
        a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride = 1, HW, HW, CIN, self.cout, 1, 1, 1
        a.out_bits, a.ldo = out_bits, self.cout
        return a, t

    def load(self, a, t, L):
        R.check_contract(L.V, L.m, L.ek)
        put(t['b'], i32(L.bias)), put(t['m'], i32(L.m)), put(t['ek'], i32(L.ek))
        a.in_ = self.x[L.kind].data_ptr()


INCEP_FORMS = [(lambda lib: lib.INCEP_REQUANT, 16, 0, (-32768, 32767)), (lambda lib: lib.INCEP_REQUANT, 8, 1, (-128, 127)),
               (lambda lib: lib.INCEP_REQUANT2, 16, 0, (-32768, 32767)), (lambda lib: lib.INCEP_REQUANT2, 8, 1, (-100, 127))]


def incep_expect(L, relu, clamp, second):
    q = np.clip(requant(np.maximum(L.V, 0), L) if relu else L.Q, *clamp)
    if second is not None:
        (m2, ek2), clamp2 = second
        R.check_contract(q, [m2], [ek2])
        q = np.clip(scalar(q, m2, ek2), *clamp2)
    return q


@pytest.mark.parametrize("form", range(len(INCEP_FORMS)))
def test_incep_conv_and_every_tile_at_the_corners(lib, form):
    """hawq_incep_conv and hawq_incep_conv_tiled on every tile id hawq_incep_conv_tile_ok accepts: every table of the list, int16 and
    int8 outputs, and REQUANT2's second table walking through the scalar corners."""
    epi, out_bits, relu, clamp = INCEP_FORMS[form]
    epi = epi(lib)
    tables, launches = form_plan(0)
    inc = Incep(lib)
    out = out_buf(NPIX * COUT, torch.int16 if out_bits == 16 else torch.int8, 0)
    a, t = inc.member(out, out_bits)
    a.epilogue, a.relu, a.q_lo, a.q_hi = epi, relu, clamp[0], clamp[1]
    ntiles = lib.load().hawq_incep_conv_num_tiles()
    ran = set()
    for i, L in enumerate(launches):
        inc.load(a, t, L)
        second = None
        if epi == lib.INCEP_REQUANT2:
            second = (R.SCALAR_TABLES[(i * 5 + form) % len(R.SCALAR_TABLES)], (-128, 127) if out_bits == 8 else (-32768, 32767))
            (a.m2, a.ek2), (a.q2_lo, a.q2_hi) = second
        want = incep_expect(L, relu, clamp, second)
        for tile in range(0, ntiles + 1):
            if not lib.load().hawq_incep_conv_tile_ok(C.byref(a), tile):
                continue
            stale(out)
            if tile == 0:
                lib.call("hawq_incep_conv", C.byref(a), K.stream())
            else:
                lib.call("hawq_incep_conv_tiled", C.byref(a), tile, K.stream())
            assert np.array_equal(carrier(out), want), (form, i, tile)
            ran.add(tile)
    assert 0 in ran and len(ran) >= 3


@pytest.mark.parametrize("with_fan", [False, True])
def test_incep_group_and_fan_at_the_corners(lib, with_fan):
    """hawq_incep_conv_group (two members, neighbouring launches of the plan) and hawq_incep_conv_group_fan (each member with two int8
    fan outputs whose tables walk through the scalar corners; k <= 15)."""
    tables, launches = form_plan(0)
    inc = Incep(lib)
    outs = [out_buf(NPIX * COUT, torch.int16, 0), out_buf(NPIX * COUT, torch.int8, 0)]
    fouts = [[out_buf(NPIX * COUT, torch.int8, 0) for _ in range(2)] for _ in range(2)]
    members = [inc.member(outs[0], 16), inc.member(outs[1], 8)]
    forms = [(0, (-32768, 32767)), (1, (-128, 127))]
    g = lib.IncepGroupArgs()
    g.n = 2
    fans = (lib.IncepFan * 2)()
    ntiles = lib.load().hawq_incep_conv_num_tiles()
    ran = set()
    for i, L in enumerate(launches):
        pair = (L, launches[(i + 1) % len(launches)])
        want, fwant = [], [[], []]
        for k_, ((a, t), Lk, (relu, clamp)) in enumerate(zip(members, pair, forms)):
            inc.load(a, t, Lk)
            a.epilogue, a.relu, a.q_lo, a.q_hi = lib.INCEP_REQUANT, relu, clamp[0], clamp[1]
            g.conv[k_] = a
            want.append(incep_expect(Lk, relu, clamp, None))
            fans[k_].n = 2 if with_fan else 0
            for j in range(2):
                m, ek = R.SCALAR_TABLES[(i * 4 + k_ * 2 + j) % len(R.SCALAR_TABLES)]
                assert (ek >> 8) <= 15
                R.check_contract(want[k_], [m], [ek])
                f = fans[k_].to[j]
                f.out, f.m, f.ek, f.lo, f.hi, f.ldo, f.c_off = fouts[k_][j].data_ptr(), m, ek, (-128, 0)[j], 127, COUT, 0
                fwant[k_].append(np.clip(scalar(want[k_], m, ek), f.lo, f.hi))
        for tile in range(1, ntiles + 1):
            ok = (lib.load().hawq_incep_conv_group_fan_ok(C.byref(g), fans, tile) if with_fan else lib.load().hawq_incep_conv_group_ok(C.byref(g), tile))
            if not ok:
                continue
            for o in outs + fouts[0] + fouts[1]:
                stale(o)
            if with_fan:
                lib.call("hawq_incep_conv_group_fan", C.byref(g), fans, tile, K.stream())
            else:
                lib.call("hawq_incep_conv_group", C.byref(g), tile, K.stream())
            for k_ in range(2):
                assert np.array_equal(carrier(outs[k_]), want[k_]), (i, tile, k_)
                for j in range(2 if with_fan else 0):
                    assert np.array_equal(carrier(fouts[k_][j]), fwant[k_][j]), (i, tile, k_, j)
            ran.add(tile)
    assert len(ran) >= 2


@pytest.mark.parametrize("side", ["pre", "post"])
def test_incep_pool_v_requant_at_the_scalar_corners(lib, side):
    """The requant op of hawq_incep_pool_v (and hawq_incep_requant, whose bytes it reproduces) with the corner tables its own _ok
    function admits on either side: int16 data holding the list's values for the table."""
    c = 64
    x = dev(np.zeros((NPIX, c), np.int16))
    out = [out_buf(NPIX * c, torch.int16, 0), out_buf(NPIX * c, torch.int16, 0)]
    rng = np.random.default_rng(8)
    took = 0
    for m, ek in R.SCALAR_TABLES:
        lim = min(32767, (1 << (31 - (ek >> 8))) - 1)
        vals = scalar_values(m, ek, 32767, signed=True)
        v = rng.integers(-lim, lim + 1, (NPIX, c)).astype(np.int64)
        v.reshape(-1)[:len(vals) * 23:23] = vals
        R.check_contract(v, [m], [ek])
        put(x, v)
        a = lib.IncepPoolArgs()
        a.in_, a.N, a.H, a.W, a.C, a.in_bits, a.in_pitch, a.out_bits, a.ldo = x.data_ptr(), 1, HW, HW, c, 16, c, 16, c
        if side == "pre":
            a.pre, a.m1, a.ek1, a.lo1, a.hi1 = 1, m, ek, -32768, 32767
        else:
            a.post, a.m2, a.ek2, a.lo2, a.hi2 = 1, m, ek, -32768, 32767
        a.out = out[0].data_ptr()
        if not lib.load().hawq_incep_pool_v_ok(C.byref(a), lib.INCEP_POOL_OPS["hawq_incep_requant"]):
            assert (ek >> 8) != 0, (m, ek)   # every table without a pre-shift is admitted
            continue
        want = np.clip(scalar(v, m, ek), -32768, 32767)
        stale(out[0]), stale(out[1])
        lib.call("hawq_incep_pool_v", C.byref(a), lib.INCEP_POOL_OPS["hawq_incep_requant"], K.stream())
        a.out = out[1].data_ptr()
        lib.call("hawq_incep_requant", C.byref(a), K.stream())
        for o in out:
            assert np.array_equal(o.cpu().numpy().astype(np.int64).reshape(NPIX, c), want), (side, m, ek)
        took += 1
    assert took >= 16
