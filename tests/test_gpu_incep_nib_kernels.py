"""The nibble-packed InceptionV3 conv (hawq_amd/csrc/incep_nib.hip, hawq_incep_conv_nib) against a plain int64 convolution and the
exact dyadic requant: every tile id on the smallest shapes that reach each mechanism of the kernel, every epilogue and store width,
in a channel slice of a wider row, in guard-banded buffers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.guard import dev, guard_arena, out_buf  # noqa: F401  (the fixture)
from tests.test_gpu_incep_tiled_kernels import _dyadic   # round_half_even(v m / 2^e) in exact integers

pytestmark = pytest.mark.gpu
RAW, REQUANT, REQUANT2 = 0, 1, 2

# (KH, KW, pad_h, pad_w, stride, H, W, Cin, Cout), N = 2: H W is no multiple of a tile's pixels, so a tile straddles the two images
CASES = [
    (1, 1, 0, 0, 1, 5, 7, 16, 16),      # Cin 16: half an MFMA K block, one unit of eight in the step; Cout below every tile
    (1, 1, 0, 0, 1, 5, 7, 48, 80),      # an odd unit count (3); Cout no multiple of 64 or 128
    (1, 1, 0, 0, 1, 9, 9, 128, 64),     # exactly one full LDS row per step
    (1, 7, 0, 3, 1, 6, 9, 48, 32),      # units of a 16-byte slot in different taps, one of them in the padding
    (7, 1, 3, 0, 1, 9, 6, 80, 48),
    (3, 3, 0, 0, 2, 9, 9, 80, 144),     # stride 2, no padding, odd map; two channel blocks of tile 1, K = 720 (tile 3's split)
    (5, 5, 2, 2, 1, 7, 5, 48, 16),      # K = 1200: ten steps, both stages reused
]
EPILOGUES = [(RAW, 32), (REQUANT, 4), (REQUANT, 8), (REQUANT, 16), (REQUANT2, 4), (REQUANT2, 8), (REQUANT2, 16)]
_gid = lambda g: "k{}x{}_p{}{}_s{}_{}x{}_c{}-{}".format(*g)   # noqa: E731


def _lib():
    from hawq_amd import _lib
    return _lib


def _block(g, ptrs, epilogue=RAW, out_bits=32, ldo=None, c_off=0, q=(0, 0), m2=0, ek2=0, q2=(0, 0), relu=0, N=2):
    KH, KW, ph, pw, stride, H, W, Cin, Cout = g
    a = _lib().IncepConvArgs()
    a.in_, a.wgt, a.bias, a.out, a.m, a.ek = ptrs
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad_h, a.pad_w = N, H, W, Cin, Cout, KH, KW, stride, ph, pw
    a.epilogue, a.relu, a.out_bits, a.ldo, a.c_off = epilogue, relu, out_bits, (Cout if ldo is None else ldo), c_off
    a.q_lo, a.q_hi, a.m2, a.ek2, a.q2_lo, a.q2_hi = q[0], q[1], m2, ek2, q2[0], q2[1]
    return a


FAKE = (0x1000,) * 6   # host arithmetic only: nothing is dereferenced
NT = _lib().load().hawq_incep_conv_nib_num_tiles()
PAIRS = [(g, t) for g in CASES for t in range(1, NT + 1) if _lib().load().hawq_incep_conv_nib_ok(C.byref(_block(g, FAKE)), t)]


@functools.lru_cache(maxsize=None)
def _case(g):
    """operands with the corners of both ranges planted, and the int64 convolution + bias, [N][Ho][Wo][Cout]"""
    KH, KW, ph, pw, s, H, W, Cin, Cout = g
    rng = np.random.default_rng(sum(g))
    x = rng.integers(0, 16, (2, H, W, Cin))
    w = rng.integers(-8, 8, (Cout, KH, KW, Cin))
    x.reshape(-1)[::5], x.reshape(-1)[1::7] = 15, 0      # a sign-extended activation nibble would read 15 as -1,
    w.reshape(-1)[::3], w.reshape(-1)[1::4] = -8, 7      # a zero-extended weight nibble -8 as 8
    Ho, Wo = (H + 2 * ph - KH) // s + 1, (W + 2 * pw - KW) // s + 1
    xp = np.zeros((2, H + 2 * ph, W + 2 * pw, Cin), np.int64)
    xp[:, ph:ph + H, pw:pw + W] = x
    ref = np.zeros((2, Ho, Wo, Cout), np.int64)
    for kh in range(KH):
        for kw in range(KW):
            ref += xp[:, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s] @ w[:, kh, kw].T.astype(np.int64)
    # unsigned activations and many -8s make every sum negative: the bias centres each channel, so that both signs are met
    b = rng.integers(-300, 300, Cout) - np.rint(ref.mean(axis=(0, 1, 2))).astype(np.int64)
    ref = ref + b
    for a in (x, w, b, ref):
        a.setflags(write=False)
    return x, w, b, ref


@pytest.mark.parametrize("epilogue,out_bits", EPILOGUES)
@pytest.mark.parametrize("g,tile", PAIRS, ids=[f"{_gid(g)}-t{t}" for g, t in PAIRS])
def test_nibble_conv_equals_int64_conv_and_requant(guard_arena, g, tile, epilogue, out_bits):   # noqa: F811
    from hawq_amd.packing import pack_conv_weight, pack_hawq4, unpack_hawq4
    L = _lib().load()
    x, w, b, ref = _case(g)
    Cout, (N, Ho, Wo, _) = g[8], ref.shape
    ldo, c_off, hi = Cout + 48, 32, {4: 15, 8: 127, 16: 32767, 32: 0}[out_bits]
    lo = 0 if out_bits == 4 else -hi - 1
    rng = np.random.default_rng(Cout)
    # per-channel ratios that spread |ref| over the store's range, with exact ties on channel 0 (ratio 1/2: every odd value)
    m = rng.integers(1 << 29, 1 << 30, Cout).astype(np.int32)
    e = np.full(Cout, 30 + max(int(np.abs(ref).max()).bit_length() - out_bits, 1), np.int32)   # the largest sums pass the upper clamp
    m[0], e[0] = 1 << 30, 31
    m2, e2, q2 = (5 << 27, 31, (lo // 2, hi // 2)) if epilogue == REQUANT2 else (0, 0, (0, 0))   # 5/16, ties of its own
    dt = {4: torch.uint8, 8: torch.int8, 16: torch.int16, 32: torch.int32}[out_bits]
    sentinel, relu = (0x77 if out_bits == 4 else 77), int(out_bits != 8)   # 0x77: two nibbles of 7
    out = out_buf(N * Ho * Wo * ldo // (2 if out_bits == 4 else 1), dt, sentinel, "out")
    xd = dev(pack_hawq4(x), "x")
    wd = dev(pack_conv_weight(w.transpose(0, 3, 1, 2), 4), "w")
    bd, md, ed = dev(b.astype(np.int32), "bias"), dev(m, "m"), dev(e, "ek")
    a = _block(g, (xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), md.data_ptr(), ed.data_ptr()), epilogue, out_bits,
               ldo, c_off, (lo, hi), m2, e2, q2, relu=relu)
    assert L.hawq_incep_conv_nib(C.byref(a), tile, torch.cuda.current_stream().cuda_stream) == 0, L.hawq_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(N, Ho, Wo, -1)
    got = unpack_hawq4(got) if out_bits == 4 else got.astype(np.int64)
    want = ref
    if epilogue != RAW:
        v = np.maximum(ref, 0) if relu else ref
        want = np.clip(np.stack([_dyadic(v[..., c], m[c], int(e[c])) for c in range(Cout)], -1), lo, hi)
        if epilogue == REQUANT2:
            want = np.clip(_dyadic(want, m2, e2), *q2)
        assert (np.abs(v[..., 0]) % 2 == 1).any() and len(np.unique(want)) >= 4   # no degenerate inputs: ties, several levels
    assert np.array_equal(got[..., c_off:c_off + Cout], want)
    assert (np.delete(got, np.s_[c_off:c_off + Cout], axis=-1) == (7 if out_bits == 4 else sentinel)).all()


def test_a_refused_block_is_an_error_and_writes_nothing(guard_arena):   # noqa: F811
    L = _lib().load()
    g = CASES[2]
    out = out_buf(2 * 81 * 64, torch.int8, 77, "out")
    d = dev(np.zeros(2 * 81 * 64, np.int32), "operands")   # large enough to stand for every operand
    p = d.data_ptr()
    bad = _block(g, (p, p, p, out.data_ptr(), p, p), REQUANT, 4, q=(0, 16))   # 16 does not fit a nibble
    for a, tile in ((bad, 2), (_block(g, (p, p, p, out.data_ptr(), p, p)), 1), (_block(g, (p, p, p, out.data_ptr(), p, p)), NT + 1)):
        assert L.hawq_incep_conv_nib(C.byref(a), tile, torch.cuda.current_stream().cuda_stream) != 0 and L.hawq_last_error()
    torch.cuda.synchronize()
    assert (out == 77).all()
