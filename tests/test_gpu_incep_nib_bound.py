"""The nibble-packed InceptionV3 conv (hawq_amd/csrc/incep_nib.hip) at the bound its int32 accumulator rests on.  The kernel feeds weights
as 16 w and shifts the sum right by 4, so a launch is accepted iff 16 * 15 * 8 * K <= 2^31 - 1 with K = KH KW Cin (|w| <= 8, a <= 15).
The rule is restated here from that comment, not read from the library; the last accepted Cin of a 1x1 and of a 7x7 window runs on
every tile with operands that drive channel 0 of a full-window pixel to -120 K, and the first refused Cin launches nothing.
tests/test_incep_nib_host.py holds the host half."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.guard import dev, guard_arena, out_buf  # noqa: F401  (the fixture)
from tests.test_gpu_incep_nib_kernels import NT, RAW, REQUANT, _block, _lib

pytestmark = pytest.mark.gpu

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


def k_accepted(KH, KW, Cin):
    """incep_nib.hip: 16 (weights as nibble << 4) * 15 * 8 * K <= 2^31 - 1"""
    return 16 * 15 * 8 * KH * KW * Cin <= INT32_MAX


def last_cin(KH, KW):
    """the largest multiple of 16 the rule accepts for this window"""
    return INT32_MAX // (16 * 15 * 8) // (KH * KW) // 16 * 16


# window -> (KH, KW, pad_h, pad_w, N, H, W), stride 1.  1x1: 6 pixels, one ragged pixel block and rows beyond P in every tile;
# 7x7 / pad 3 on a 7 x 7 map: the centre pixel sees all 49 taps, every other pixel some padding
WINDOWS = {"1x1": (1, 1, 0, 0, 2, 1, 3), "7x7": (7, 7, 3, 3, 1, 7, 7)}
# window -> (last accepted Cin, its K, first refused Cin): a change to the bound has to be made here too
PINNED = {"1x1": (1118480, 1118480, 1118496), "7x7": (22816, 1117984, 22832)}
COUT_MAX = 80   # tile 1 wants more than 64 channels; tiles 2 and 3 run on the first 16 rows of the same weights
LDO_EXTRA, C_OFF = 48, 32


def shape(win, cin, cout):
    """(the geometry tuple of test_gpu_incep_nib_kernels._block, N)"""
    KH, KW, ph, pw, N, H, W = WINDOWS[win]
    return (KH, KW, ph, pw, 1, H, W, cin, cout), N


# (window, tile, Cout)
RUNS = [(win, tile, COUT_MAX if tile == 1 else 16) for win in WINDOWS for tile in range(1, NT + 1)]


@functools.lru_cache(maxsize=None)
def bound_case(win):
    """x [N][H][W][Cin] int8, the hawq4 weights of COUT_MAX rows (bytes), bias and the int64 conv + bias [N][H][W][COUT_MAX] at the
    last accepted Cin.  Weight row 0 is all -8, row 1 all 7, row 2 alternates -8 and 7 along K; pixel 0 (1x1) or the whole map (7x7)
    is 15 everywhere; the rest is random in the full ranges."""
    from hawq_amd.packing import pack_hawq4
    KH, KW, ph, pw, N, H, W = WINDOWS[win]
    cin = last_cin(KH, KW)
    rng = np.random.default_rng(cin)
    x = rng.integers(0, 16, (N, H, W, cin), dtype=np.int8)
    if win == "1x1":
        x[0, 0, 0] = 15
    else:
        x[:] = 15
    w = rng.integers(-8, 8, (COUT_MAX, KH, KW, cin), dtype=np.int8)
    w[0], w[1] = -8, 7
    w[2].reshape(-1)[0::2], w[2].reshape(-1)[1::2] = -8, 7
    b = rng.integers(-(1 << 20), 1 << 20, COUT_MAX).astype(np.int64)
    b[0], b[1] = 0, 1 << 27
    xp = np.zeros((N, H + 2 * ph, W + 2 * pw, cin), np.int64)
    xp[:, ph:ph + H, pw:pw + W] = x
    ref = np.zeros((N, H, W, COUT_MAX), np.int64)
    step = 1 << 16   # K in pieces: an int64 copy of all the weights at once would be 0.7 GB
    for kh in range(KH):
        for kw in range(KW):
            for c0 in range(0, cin, step):
                ref += xp[:, kh:kh + H, kw:kw + W, c0:c0 + step] @ w[:, kh, kw, c0:c0 + step].T.astype(np.int64)
    ref += b
    wp = np.concatenate([pack_hawq4(w[c]).reshape(-1) for c in range(COUT_MAX)])
    x, b = np.ascontiguousarray(x), b.astype(np.int32)
    for a in (x, wp, b, ref):
        a.setflags(write=False)
    return x, wp, b, ref


@pytest.mark.parametrize("epilogue,out_bits", [(RAW, 32), (REQUANT, 16)], ids=["raw", "requant16"])
@pytest.mark.parametrize("win,tile,cout", RUNS, ids=[f"{w}-t{t}-c{c}" for w, t, c in RUNS])
def test_the_last_accepted_k_sums_exactly(guard_arena, win, tile, cout, epilogue, out_bits):   # noqa: F811
    from hawq_amd.packing import pack_hawq4
    from tests.requant_corners import np_rne
    L = _lib().load()
    cin, K, _ = PINNED[win]
    g, N = shape(win, cin, cout)
    assert cin == last_cin(g[0], g[1]) and K == g[0] * g[1] * cin and k_accepted(g[0], g[1], cin)
    x, wp, b, ref = bound_case(win)
    ref, b = ref[..., :cout], b[:cout]
    # the inputs reach the bound: channel 0 of a full-window pixel is -120 K, and sixteen times that is what the accumulator holds
    full = (0, 0, 0) if win == "1x1" else (0, 3, 3)
    assert ref[full][0] == -120 * K and INT32_MIN <= 16 * ref[full][0] == {"1x1": INT32_MIN + 2048, "7x7": -2146529280}[win]
    assert ref[full][1] == 105 * K + (1 << 27) <= INT32_MAX
    ldo = cout + LDO_EXTRA
    P = ref[..., 0].size
    m, ek = np.full(cout, 1 << 30, np.int32), np.full(cout, 30 + 12, np.int32)   # ratio 2^-12: -120 K lands on the int16 floor, signed
    lo, hi = (-32768, 32767) if epilogue == REQUANT else (0, 0)
    out = out_buf(P * ldo, torch.int32 if out_bits == 32 else torch.int16, 77, "out")
    xd, wd = dev(pack_hawq4(x), "x"), dev(wp[:cout * K // 2].copy(), "w")   # (copies: the shared case is read-only)
    bd, md, ed = dev(b.copy(), "bias"), dev(m, "m"), dev(ek, "ek")
    a = _block(g, (xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), md.data_ptr(), ed.data_ptr()), epilogue, out_bits,
               ldo, C_OFF, (lo, hi), relu=0, N=N)
    assert L.hawq_incep_conv_nib_ok(C.byref(a), tile)
    assert L.hawq_incep_conv_nib(C.byref(a), tile, torch.cuda.current_stream().cuda_stream) == 0, L.hawq_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(P, ldo).astype(np.int64)
    want = ref.reshape(P, cout)
    if epilogue == REQUANT:
        want = np.clip(np_rne(want, 1 << 30, 42, 0), lo, hi)
        assert want.min() == np_rne(-120 * K, 1 << 30, 42, 0) < 0 < want.max()   # the sign survives, unclamped
    assert np.array_equal(got[:, C_OFF:C_OFF + cout], want)
    assert (np.delete(got, np.s_[C_OFF:C_OFF + cout], axis=-1) == 77).all()


@pytest.mark.parametrize("win", sorted(WINDOWS))
def test_the_first_refused_k_is_an_error_and_writes_nothing(guard_arena, win):   # noqa: F811
    L = _lib().load()
    _, _, cin = PINNED[win]
    assert cin == last_cin(*WINDOWS[win][:2]) + 16 and not k_accepted(*WINDOWS[win][:2], cin)
    p = dev(np.zeros(64, np.int32), "operands").data_ptr()   # nothing may be read: one small buffer stands for every operand
    for tile, cout in ((1, COUT_MAX), (2, 16), (3, 16)):
        g, N = shape(win, cin, cout)
        out = out_buf(N * g[5] * g[6] * cout, torch.int32, 77, "out")
        a = _block(g, (p, p, p, out.data_ptr(), p, p), RAW, 32, N=N)
        assert L.hawq_incep_conv_nib(C.byref(a), tile, torch.cuda.current_stream().cuda_stream) != 0
        assert b"K too long" in L.hawq_last_error(), L.hawq_last_error()
        torch.cuda.synchronize()
        assert (out == 77).all()
