"""The mixed-form grouped launch with a fan-out epilogue (hawq_amd/csrc/incep_fan_nib.hip, hawq_incep_conv_group_nib_fan) against a
plain int64 convolution and the exact dyadic requant on the CPU: members of either operand form with int8 and hawq4 fan outputs, on
both tiles.  Whole buffers are compared - the written slices and the channels around them, which keep their fill - inside the guard
bands of tests/guard.py.  The shapes are the smallest at which the kernel can still go wrong."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.guard import dev, guard_arena, out_buf  # noqa: F401  (the fixture)
from tests.test_gpu_incep_fan_kernels import _dyadic   # round_half_even in exact integers, and where the ties were
from tests.test_gpu_incep_nib_kernels import REQUANT as RQ, REQUANT2 as RQ2, _block, _lib

pytestmark = pytest.mark.gpu

# fan tables (m, ek, lo, hi) on primary outputs of 0 .. a few hundred (`_reference` spreads them so and asserts what each is for)
TIES = (1 << 30, 32, 2, 13)                 # y / 4: an exact tie wherever y = 2 mod 4, inside a narrow clamp that saturates at both ends
SATURATE = (1 << 30, 29, 3, 100)            # 2 y: zeros are below lo, most values beyond hi (int8 outputs only)
FOUR_BIT = (1 << 30, 33, 0, 15)             # y / 8 into 0 .. 15
SHIFTED = (3 << 28, (2 << 8) | 34, 0, 15)   # the pre-shifted form: ((y << 2) * 0.75) / 16, into 0 .. 15
FILL = {4: 7, 8: 77, 16: 77}                # per element; a hawq4 byte is filled with 0x77


def _m(nib, N, g, epilogue, bits, fans=(), out=None, ldo=None, c_off=16):
    """a member: operand form, batch, (KH, KW, pad_h, pad_w, stride, H, W, Cin, Cout), epilogue and store width, its slice of the rows
    `out` (a name; default a buffer of its own), and its fans (table, hawq4?, consumer name or None, ldo or None, c_off)"""
    return dict(nib=nib, N=N, g=g, epilogue=epilogue, bits=bits, out=out, ldo=g[8] + 32 if ldo is None else ldo, c_off=c_off,
                fans=[(t, h4, to, g[8] + 48 if fl is None else fl, off) for t, h4, to, fl, off in fans])


def _own(*fans):
    return [(t, h4, None, None, 32) for t, h4 in fans]


# pixels: 25 = 1 x 5 x 5 (one partial block) and 243 = 3 x 9 x 9 (two 128-pixel blocks and a ragged tail)
CASES = {
    "nib_c16_int8fan": [_m(1, 1, (1, 1, 0, 0, 1, 5, 5, 16, 16), RQ, 8, _own((TIES, 0)))],
    "i8_c16_nibfan": [_m(0, 1, (1, 1, 0, 0, 1, 5, 5, 16, 16), RQ, 8, _own((FOUR_BIT, 1)))],
    "i8_c48_n4": [_m(0, 3, (1, 1, 0, 0, 1, 9, 9, 48, 48), RQ2, 16, _own((TIES, 1), (SATURATE, 0), (FOUR_BIT, 1), (SHIFTED, 0)))],
    "nib_3x3_k432_c80_n4": [_m(1, 3, (3, 3, 1, 1, 1, 9, 9, 48, 80), RQ2, 16, _own((TIES, 0), (FOUR_BIT, 1), (SHIFTED, 1), (SATURATE, 0)))],
    "nib_c144": [_m(1, 1, (1, 1, 0, 0, 1, 5, 5, 16, 144), RQ2, 16, _own((TIES, 1)))],   # past one 128-channel block: tile 1
    # a level of a unit: a conv of its own without a fan, and two slices of the 16-bit concat buffer whose hawq4 fan slices are
    # byte-neighbours in the consumer X (channels 16 .. 63 and 64 .. 143 of 160); 0 .. 15 and 144 .. 159 of every row keep their fill
    "level": [_m(0, 3, (1, 1, 0, 0, 1, 9, 9, 16, 16), RQ, 8),
              _m(1, 3, (1, 1, 0, 0, 1, 9, 9, 48, 48), RQ2, 16, [(TIES, 1, "X", 160, 16), (SATURATE, 0, "Y", 160, 16), (FOUR_BIT, 1, None, None, 32),
                                                              (SHIFTED, 0, None, None, 32)], out="cat", ldo=160, c_off=16),
              _m(0, 3, (1, 1, 0, 0, 1, 9, 9, 16, 80), RQ2, 16, [(SHIFTED, 1, "X", 160, 64)], out="cat", ldo=160, c_off=64)],
}
PARAMS = [(name, t) for name in CASES for t in (1, 2) if name != "nib_c144" or t == 1]


def _pixels(mb):
    KH, KW, ph, pw, s, H, W = mb["g"][:7]
    return mb["N"] * ((H + 2 * ph - KH) // s + 1) * ((W + 2 * pw - KW) // s + 1)


def _keys(name):
    """(primary buffer, [fan buffer]) names per member"""
    return [(mb["out"] or f"out{i}", [to or f"fan{i}.{j}" for j, (_, _, to, _, _) in enumerate(mb["fans"])]) for i, mb in enumerate(CASES[name])]


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Per member its operands (x, w, b, m, e) and, per buffer, (bits, expected [P][ldo] int64 with the fill around the slices): the
    conv in int64, requants by `_dyadic`.  Asserts that every fan table does on these outputs what it is for."""
    ops, bufs = [], {}
    for i, (mb, (pkey, fkeys)) in enumerate(zip(CASES[name], _keys(name))):
        KH, KW, ph, pw, s, H, W, Cin, Cout = mb["g"]
        N, P = mb["N"], _pixels(mb)
        rng = np.random.default_rng(11 + i + sum(map(ord, name)))
        x = rng.integers(0, 16, (N, H, W, Cin)) if mb["nib"] else rng.integers(-128, 128, (N, H, W, Cin))
        w = rng.integers(-8, 8, (Cout, KH, KW, Cin)) if mb["nib"] else rng.integers(-128, 128, (Cout, KH, KW, Cin))
        Ho, Wo = (H + 2 * ph - KH) // s + 1, (W + 2 * pw - KW) // s + 1
        xp = np.zeros((N, H + 2 * ph, W + 2 * pw, Cin), np.int64)
        xp[:, ph:ph + H, pw:pw + W] = x
        ref = np.zeros((N, Ho, Wo, Cout), np.int64)
        for kh in range(KH):
            for kw in range(KW):
                ref += xp[:, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s] @ w[:, kh, kw].T.astype(np.int64)
        b = rng.integers(-300, 300, Cout) - np.rint(ref.mean(axis=(0, 1, 2))).astype(np.int64)   # centred: the ReLU cuts about half
        ref = (ref + b).reshape(P, Cout)
        # per-channel ratios that spread the sums over 0 .. 2^spread: the primary output ends near 0 .. 600 (REQUANT2: times 5/8), or
        # in an 8-bit store's upper clamp
        spread = 11 if mb["epilogue"] == RQ2 else 9
        m = rng.integers(1 << 29, 1 << 30, Cout).astype(np.int32)
        e = np.full(Cout, 30 + max(int(np.abs(ref).max()).bit_length() - spread, 1), np.int32)
        a = _block(mb["g"], (0,) * 6, **_forms(mb))
        y = np.clip(np.stack([_dyadic(np.maximum(ref[:, c], 0), m[c], int(e[c]))[0] for c in range(Cout)], -1), a.q_lo, a.q_hi)
        if mb["epilogue"] == RQ2:
            y = np.clip(_dyadic(y, a.m2, a.ek2)[0], a.q2_lo, a.q2_hi)
        assert len(np.unique(y)) > 8
        ops.append((x, w, b.astype(np.int32), m, e))
        for key, bits, ldo, off, val in [(pkey, mb["bits"], mb["ldo"], mb["c_off"], y)] + [
                (k, 4 if h4 else 8, fl, fo, _fan_want(y, t, h4)) for k, (t, h4, _, fl, fo) in zip(fkeys, mb["fans"])]:
            have = bufs.setdefault(key, (bits, np.full((P, ldo), FILL[bits], np.int64)))
            assert have[0] == bits and have[1].shape == (P, ldo) and (have[1][:, off:off + Cout] == FILL[bits]).all()
            have[1][:, off:off + Cout] = val
    for _, exp in bufs.values():
        exp.setflags(write=False)
    return ops, bufs


def _fan_want(y, table, h4):
    """what a fan output makes of the primary output `y`, after asserting that its table bites on it"""
    m, ek, lo, hi = table
    q, tie = _dyadic(y, m, ek)
    want = np.clip(q, lo, hi)
    if table == TIES:
        assert (tie & (q > lo) & (q < hi)).any() and (q < lo).any() and (q > hi).any()
    elif table == SATURATE:
        assert not h4 and (q < lo).any() and (q > hi).any()
    else:   # the 0 .. 15 range, both ends reached, the upper one by saturation
        assert want.min() == 0 and want.max() == 15 and (q > 15).any() and (table != SHIFTED or ek >> 8)
    return want


def _forms(mb):
    lim = (1 << (mb["bits"] - 1)) - 1
    return dict(epilogue=mb["epilogue"], out_bits=mb["bits"], ldo=mb["ldo"], c_off=mb["c_off"], q=(0, lim), relu=1, N=mb["N"],
                **(dict(m2=5 << 28, ek2=31, q2=(0, lim // 2)) if mb["epilogue"] == RQ2 else {}))   # 5 / 8, ties of its own


def describe(name, addr):
    """(group, mask, fans, fan_mask) of case `name` on the addresses ``addr(i, what)`` (what: "x", "w", "b", "m", "ek" of member i)
    and ``addr(None, buffer name)``"""
    members = CASES[name]
    g, fans, mask, fan_mask = _lib().IncepGroupArgs(), (_lib().IncepFan * len(members))(), 0, 0
    g.n = len(members)
    for i, (mb, (pkey, fkeys)) in enumerate(zip(members, _keys(name))):
        ptrs = (addr(i, "x"), addr(i, "w"), addr(i, "b"), addr(None, pkey), addr(i, "m"), addr(i, "ek"))
        g.conv[i] = _block(mb["g"], ptrs, **_forms(mb))
        mask |= mb["nib"] << i
        fans[i].n = len(mb["fans"])
        for j, (k, ((m, ek, lo, hi), h4, _, fl, fo)) in enumerate(zip(fkeys, mb["fans"])):
            f = fans[i].to[j]
            f.out, f.m, f.ek, f.lo, f.hi, f.ldo, f.c_off = addr(None, k), m, ek, lo, hi, fl, fo
            fan_mask |= h4 << (4 * i + j)
    return g, mask, fans, fan_mask


def _device(name):
    """the case on the device: operands uploaded, every output buffer filled; (description, {buffer name: tensor})"""
    from hawq_amd.packing import pack_conv_weight, pack_hawq4
    ops, bufs = _reference(name)
    t = {}
    for i, (mb, (x, w, b, m, e)) in enumerate(zip(CASES[name], ops)):
        t[i, "x"] = dev(pack_hawq4(x) if mb["nib"] else x.astype(np.int8), f"x{i}")
        t[i, "w"] = dev(pack_conv_weight(w.transpose(0, 3, 1, 2), 4 if mb["nib"] else 8), f"w{i}")
        t[i, "b"], t[i, "m"], t[i, "ek"] = dev(b, f"b{i}"), dev(m, f"m{i}"), dev(e, f"ek{i}")
    dt = {4: torch.uint8, 8: torch.int8, 16: torch.int16}
    for key, (bits, exp) in bufs.items():
        t[None, key] = out_buf(exp.size // (2 if bits == 4 else 1), dt[bits], 0x77 if bits == 4 else 77, key)
    return describe(name, lambda i, what: t[i, what].data_ptr()), {k[1]: v for k, v in t.items() if k[0] is None}


def _unchanged(name, outs):
    return all((t == (0x77 if _reference(name)[1][k][0] == 4 else 77)).all() for k, t in outs.items())


@pytest.mark.parametrize("name,tile", PARAMS, ids=[f"{n}-tile{t}" for n, t in PARAMS])
def test_fan_launch_equals_int64_conv_and_requants(guard_arena, name, tile):   # noqa: F811
    from hawq_amd.packing import unpack_hawq4
    L = _lib().load()
    (g, mask, fans, fan_mask), outs = _device(name)
    assert L.hawq_incep_conv_group_nib_fan_ok(C.byref(g), mask, fans, fan_mask, tile) == 1
    assert L.hawq_incep_conv_group_nib_fan(C.byref(g), mask, fans, fan_mask, tile, torch.cuda.current_stream().cuda_stream) == 0, L.hawq_last_error()
    torch.cuda.synchronize()
    for key, (bits, exp) in _reference(name)[1].items():
        got = outs[key].cpu().numpy().reshape(exp.shape[0], -1)
        got = unpack_hawq4(got) if bits == 4 else got
        assert np.array_equal(got.astype(np.int64), exp), f"{key} ({bits} bits) differs from the reference"


def check_refusals(g, mask, fans, fan_mask, x_ptr, stream):
    """Walks the "level" description through its refusals; each is refused by `_ok` and by the launch, which names its reason: a
    hawq4 fan with hi = 16; a fan_mask bit beyond fan[i].n (member 2 has one output) and beyond n; member 2's slice of X from an
    origin 16 bytes = 32 nibbles on - another buffer by the rules, clear of member 1's slice by channels but not by the bytes its
    half-byte extents cover; and tile 3.  The description is as it was afterwards."""
    L = _lib().load()
    for change, fm, tile, why in (((fans[1].to[0], "hi", 16), fan_mask, 2, b"clamp bounds outside a nibble"),
                                  (None, fan_mask | 1 << (4 * 2 + 1), 2, b"fan_mask names a fan output that does not exist"),
                                  (None, fan_mask | 1 << (4 * 3), 2, b"fan_mask names a fan output that does not exist"),
                                  ((fans[2].to[0], "out", x_ptr + 16), fan_mask, 2, b"two fan outputs overlap"),
                                  (None, fan_mask, 3, b"no such tile")):
        old = change and getattr(*change[:2])
        if change:
            setattr(*change)
        assert L.hawq_incep_conv_group_nib_fan_ok(C.byref(g), mask, fans, fm, tile) == 0, why
        assert L.hawq_incep_conv_group_nib_fan(C.byref(g), mask, fans, fm, tile, stream) != 0 and why in L.hawq_last_error(), why
        if change:
            setattr(*change[:2], old)
    assert L.hawq_incep_conv_group_nib_fan_ok(C.byref(g), mask, fans, fan_mask, 2) == 1   # the refusals above are not the case's


def test_a_refused_description_is_an_error_and_writes_nothing(guard_arena):   # noqa: F811
    (g, mask, fans, fan_mask), outs = _device("level")
    check_refusals(g, mask, fans, fan_mask, outs["X"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _unchanged("level", outs)
