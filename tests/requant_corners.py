"""The corners of the dyadic table contract: one case list, one exact reference, and Python restatements of the
requant forms of hawq_amd/csrc/common.h with their 32 / 64-bit wrap-around written out.

A table is (m, e, k): q = round_half_even(((v << k) * m) / 2^e) with 0 <= m < 2^31, e in [33, 62] (so the fast forms'
shift s = e - 32 lies in [1, 30] and survives the kernels' ``& 31``), pre-shift k >= 0 and |v << k| < 2^31.  The list
is the product of the extreme and a few middle values of each field; the values per table are the ends of the
admitted range, zero's neighbours, every exact rounding tie the table has near u * 2^sh for small odd u, and a value
that lands on each clamp edge where the table reaches it.

``rne`` (Python integers) is the only expectation the tests use for the requant itself.  This is a plain module:
tests/test_requant_corners_host.py checks the list and the restatements without a device,
tests/test_gpu_requant_corners.py drives the kernels' accumulators onto the same pairs.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from hawq_amd.quant_utils import tables_are_fast

MS = (0, 1, 3, 1 << 30, 3 << 29, 5 << 27, (1 << 30) + 1, 0x5A5A5A5B, (1 << 31) - 1)
ES = (33, 34, 47, 61, 62)
KS = (0, 1, 7, 15, 30)
TIE_U = (1, -1, 3, -3, 5, -5)

# scalar tables for the per-call fields (mq, eq) and (m_id_scalar, e_id_scalar): in and out of ids0_form (e = 33, k >= 1),
# with and without a pre-shift
SCALAR_MS = (1, 1 << 30, (1 << 30) + 1, (1 << 31) - 1)
SCALAR_EKS = ((33, 0), (33, 1), (33, 15), (34, 0), (61, 0), (62, 0))

CLAMPS = ((-128, 127), (0, 127), (0, 15), (-32768, 32767))

EDGE_RESULTS = tuple(sorted({x for lo, hi in CLAMPS for x in (lo - 1, lo, hi, hi + 1)}))

Table = namedtuple("Table", "m e k ek vbits lim provably_fast values")


def tz(m: int) -> int:
    return (m & -m).bit_length() - 1


# ---------------------------------------------------------------------------------------------- the exact reference
def rne(v: int, m: int, e: int, k: int) -> int:
    """round-half-even of ((v << k) * m) / 2^e in Python integers."""
    p = (int(v) << k) * int(m)
    q, r, half = p >> e, p & ((1 << e) - 1), 1 << (e - 1)
    if r > half or (r == half and (q & 1)):
        q += 1
    return q


def is_tie(v: int, m: int, e: int, k: int) -> bool:
    return ((int(v) << k) * int(m)) & ((1 << e) - 1) == 1 << (e - 1)


def clamp(q: int, lo: int, hi: int) -> int:
    return lo if q < lo else (hi if q > hi else q)


# ---------------------------------------------------------------------------------------------- the case list
def _values(m, e, k, vbits, lim):
    vals = {0}
    for a in (1, 2, 3, lim, lim - 1, lim // 2):
        vals.update((a, -a))
    if m:
        sh = e - 1 - k - tz(m)
        if 0 <= sh < vbits:   # (v << k) * m = u * odd(m) * 2^(e-1): every odd u is an exact tie
            for u in TIE_U:
                vals.update((u << sh) + d for d in (-1, 0, 1))
    # beyond the rule above: where the table reaches them, one value whose exact result lands on each edge of the clamps the
    # kernels use and on its outer neighbour (q_lo - 1, q_lo, q_hi, q_hi + 1), so that v_med3 and the saturating packs see both
    # sides of every edge
    if m:
        for r in EDGE_RESULTS:
            v0 = ((r << e) // m) >> k
            hit = [v for v in (v0 - 1, v0, v0 + 1, v0 + 2) if abs(v) <= lim and rne(v, m, e, k) == r]
            vals.update(hit[:1])
    return tuple(sorted(v for v in vals if abs(v) <= lim))


def _tables():
    out = []
    for m in MS:
        for e in ES:
            for k in KS:
                vbits = 31 - k
                lim = (1 << vbits) - 1
                ek = e | k << 8
                out.append(Table(m, e, k, ek, vbits, lim, bool(tables_are_fast([m], [ek], vbits)), _values(m, e, k, vbits, lim)))
    return tuple(out)


TABLES = _tables()
SCALAR_TABLES = tuple((m, e | k << 8) for m in SCALAR_MS for e, k in SCALAR_EKS)


def pairs(tables=TABLES):
    """every (table, value) of the list"""
    return [(t, v) for t in tables for v in t.values]


def ids0_form(ek: int) -> bool:
    """common.h ids0_form: the scalar identity table lifted to (e = 33, k >= 1)"""
    return (ek & 0xff) == 33 and (ek >> 8) >= 1


# ---------------------------------------------------------------------------------------------- wrap-around
def i32(x: int) -> int:
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def i64(x: int) -> int:
    x &= 0xFFFFFFFFFFFFFFFF
    return x - (1 << 64) if x >> 63 else x


# ---------------------------------------------------------------------------------------------- common.h, restated
def dyadic_rne(v, m, ek):
    """common.h dyadic_rne, with its (int32_t) truncation"""
    e, k = ek & 0xff, ek >> 8
    t = i64(i32(v << k) * m + (1 << (e - 1)))
    f = t >> e
    if t & ((1 << e) - 1) == 0:
        f &= ~1
    return i32(f)


DyNt = namedtuple("DyNt", "m s k add")


def dynt_prepare(m, ek, rounding=True):
    s, k = (ek & 0xff) - 32, ek >> 8
    return DyNt(m, s, k, (((1 << (s - 1)) & 0xFFFFFFFF) << 32) if rounding else 0)


def _shift(hi, s, mask, arith):
    s &= mask                      # the kernels take s from a table word with `& 31`; the hardware ignores the upper bits
    return hi >> s if arith else i32((hi & 0xFFFFFFFF) >> s)


def dyadic_nt(v, c, mask=31, preshift=True, arith=True):
    """common.h dyadic_nt: hi32((v << k) * m + 2^(e-1)) >> s.  The keyword arguments are the mutations the host test plants."""
    t = i64(i32(v << c.k if preshift else v) * c.m + c.add)
    return _shift(i32(t >> 32), c.s, mask, arith)


def dyadic_nt_k(v, c, k0):
    """common.h dyadic_nt_k<K0>: K0 skips the pre-shift (the host guarantees k == 0)"""
    t = i64(i32(v if k0 else v << c.k) * c.m + c.add)
    return i32(t >> 32) >> (c.s & 31)


def dyadic_tie(v, c, mask=31, preshift=True, arith=True, tie_fix=True, tie_hi_bits=True):
    """common.h dyadic_tie: half-up, then one less when an exact tie rounded to an odd result"""
    t = i64(i32(v << c.k if preshift else v) * c.m + c.add)
    hi = i32(t >> 32)
    q = _shift(hi, c.s, mask, arith)
    tie = (t & 0xFFFFFFFF) == 0 and (not tie_hi_bits or (hi & ((1 << (c.s & mask)) - 1)) == 0)
    return q - ((q & 1) if tie and tie_fix else 0)


def dyadic_s0(v, m, ek):
    """common.h dys0_prepare + dyadic_s0: ((v << (k - 1)) * m + 2^31) >> 32 for ids0_form tables"""
    assert ids0_form(ek)
    return i32(i64(i32(v << ((ek >> 8) - 1)) * m + (1 << 31)) >> 32)


def ctab_constant(bias, m, ek):
    """pack_ctab's arithmetic: the words {m, (e - 32) | k << 8, lo32(Cc), hi32(Cc)}, Cc = (bias << k) * m + 2^(e-1) in 64 bits"""
    e, k = ek & 0xff, ek >> 8
    cc = i64((bias << k) * m + (1 << (e - 1)))
    return m, (e - 32) | k << 8, i32(cc), i32(cc >> 32)


def dyadic_ctab(acc, row, tie):
    """the fast epilogues' use of a ctab row on a raw accumulator: hi32((acc << k) * m + Cc) >> s, optionally tie-aware"""
    m, sk, lo, hi = (int(x) for x in row)
    c = DyNt(m, sk & 31, sk >> 8, i64(((hi & 0xFFFFFFFF) << 32) | (lo & 0xFFFFFFFF)))
    return dyadic_tie(acc, c) if tie else dyadic_nt(acc, c)


# ---------------------------------------------------------------------------------------------- driven accumulators
def centres(t: Table, offsets):
    """Biases that put every listed value of the table on some pixel of a channel whose accumulator is bias + offset, while
    every offset of that channel stays inside the table's contract (|bias + offset| <= lim).  Greedy cover from below."""
    lo, hi = min(offsets), max(offsets)
    assert t.lim + lo >= -t.lim - hi, "the offsets do not fit this table at all"
    out, covered = [], None
    for v in t.values:
        if covered is not None and v <= covered:
            continue
        c = min(max(v - lo, -t.lim - lo), t.lim - hi)   # v sits on the lowest offset unless that breaks the contract
        assert c + lo >= -t.lim and c + hi <= t.lim and c + lo <= v <= c + hi
        out.append(c)
        covered = c + hi
    return out


def np_rne(v, m, e, k):
    """rne on int64 arrays: inside the contract the product stays below 2^62, so int64 holds every intermediate.  The host test
    checks it against the Python-integer ``rne`` on every pair of the list."""
    v, m, e, k = (np.asarray(a, np.int64) for a in (v, m, e, k))
    assert (np.abs(v << k) < (1 << 31)).all() and ((m >= 0) & (m < (1 << 31))).all() and ((e >= 1) & (e <= 62)).all()
    p = (v << k) * m
    one = np.int64(1)
    q, r, half = p >> e, p & ((one << e) - 1), one << (e - 1)
    return q + ((r > half) | ((r == half) & ((q & 1) == 1)))


OFFSETS = {   # what the 256 pixels of a 16 x 16 map add to a channel's bias
    "int8": np.arange(256, dtype=np.int64) - 128,        # int8 activations: every offset -128 .. 127 once
    "relu": np.arange(256, dtype=np.int64) % 128,        # post-ReLU activations
    "tiny": np.arange(256, dtype=np.int64) % 3 - 1,      # for tables whose whole range is {-1, 0, 1} (k = 30)
    "tiny_relu": np.arange(256, dtype=np.int64) % 2,
}

Launch = namedtuple("Launch", "kind off tidx bias m ek V Q")   # per channel: table index, bias, m, e | k << 8; V, Q: [C][256] values and exact results


def check_contract(V, m, ek):
    """the host-side assert before every upload: no (table, value) of a launch lies outside the table's contract"""
    m, ek = np.asarray(m, np.int64).reshape(-1, 1), np.asarray(ek, np.int64).reshape(-1, 1)
    e, k = ek & 0xff, ek >> 8
    assert ((m >= 0) & (m < (1 << 31)) & (e >= 33) & (e <= 62) & (k >= 0) & (k <= 30)).all()
    assert (np.abs(np.asarray(V, np.int64)) <= ((np.int64(1) << (31 - k)) - 1)).all(), "a driven value violates |v << k| < 2^31"


def plan(tables, cout=128, relu_inputs=False):
    """Lay the list onto launches of `cout` channels: one (table, bias) per channel, tables of a tiny range apart from the others
    (they need other input columns).  Returns the launches; ``coverage`` says which pairs of the list they hold."""
    out = []
    for tiny in (False, True):
        kind = ("tiny" if tiny else "int8") if not relu_inputs else ("tiny_relu" if tiny else "relu")
        off = OFFSETS[kind]
        slots = [(i, c) for i, t in enumerate(tables) if (t.lim < 128) == tiny for c in centres(t, (int(off.min()), int(off.max())))]
        for at in range(0, len(slots), cout):
            part = slots[at:at + cout]
            part += [part[0]] * (cout - len(part))
            tidx = np.array([i for i, _ in part])
            bias = np.array([c for _, c in part], np.int64)
            m = np.array([tables[i].m for i in tidx], np.int64)
            ek = np.array([tables[i].ek for i in tidx], np.int64)
            V = bias[:, None] + off[None, :]
            check_contract(V, m, ek)
            out.append(Launch(kind, off, tidx, bias, m, ek, V, np_rne(V, m[:, None], (ek & 0xff)[:, None], (ek >> 8)[:, None])))
    return out


def coverage(launches, tables, keep=lambda v: True):
    """the (table index, value) pairs of the list that occur in these launches"""
    got = set()
    for L in launches:
        for c, i in enumerate(L.tidx):
            row = set(L.V[c].tolist())
            got.update((int(i), v) for v in tables[i].values if v in row and keep(v))
    return got
