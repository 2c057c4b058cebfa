"""The LDS-band 3x3 conv kernel (hawq_amd/csrc/incep_band.hip, hawq_incep_conv_band) against the float64 conv and integer host maths."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_incep_tiled_kernels import _args, _dyadic, _operands, _out_shape, _reference

pytestmark = pytest.mark.gpu

# (pad, H, W, Cin, Cout), 3x3 / stride 1, the smallest shapes that expose one failure each: a 1 x 1 map (only the centre tap in bounds);
# one output pixel, the widest Cin, Cout no multiple of 64; P = 429 with a ragged Cout block and every border class; 45 K units (the
# odd half-step tail); longer than any band in one direction by a non-multiple with one output row / column in the other; Cin = 64;
# then q_conv2, q_conv3, q_conv5.  N = 3 on the small ones, so that bands cross image boundaries.
SHAPES = [(1, 1, 1, 16, 16), (0, 3, 3, 96, 208), (1, 11, 13, 32, 48), (0, 11, 13, 80, 80), (1, 2, 150, 48, 16), (0, 150, 3, 16, 32),
          (1, 12, 14, 64, 96), (0, 149, 149, 32, 32), (1, 147, 147, 32, 64), (0, 73, 73, 80, 192)]
_sid = lambda s: "p{}_{}x{}_c{}-{}".format(*s)   # noqa: E731
_cache = {}


def _case(s):
    """geometry, batch, device operands and the float64 conv of shape `s`: computed once, shared, never changed"""
    if s not in _cache:
        g, N = (3, 3, s[0], s[0], 1, *s[1:]), (1 if s in SHAPES[-3:] else 3)
        x, w, b = _operands(g, N, seed=sum(s))
        b[0], b[1] = 1, 2   # the tie channels keep both signs and parities under a ReLU
        _cache[s] = (g, N, x.cuda(), w.cuda(), b.cuda(), _reference(x, w, b, g).numpy())
    return _cache[s]


def _launch(a):
    from hawq_amd import _lib
    rc = _lib.load().hawq_incep_conv_band(C.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("s", SHAPES, ids=_sid)
def test_raw_equals_the_float64_conv_inside_sentinel_rows(s):
    g, N, xd, wd, bd, ref = _case(s)
    Cout, rows = s[4], int(np.prod(ref.shape[:3]))
    buf = torch.full(((rows + 2) * Cout,), -5, dtype=torch.int32, device="cuda")   # one sentinel row in front and one behind
    assert _launch(_args(xd, wd, bd, g, buf[Cout:])) == 0
    got = buf.cpu().numpy().reshape(rows + 2, Cout)
    assert np.array_equal(got[1:-1].reshape(ref.shape), ref) and (got[0] == -5).all() and (got[-1] == -5).all()


@pytest.mark.parametrize("s", SHAPES, ids=_sid)
@pytest.mark.parametrize("epilogue,out_bits,relu", [(1, 8, 1), (1, 16, 1), (2, 16, 1), (2, 16, 0)])
def test_requant_epilogues_match_host_maths_and_leave_neighbour_channels_alone(epilogue, out_bits, relu, s):
    from hawq_amd.quant_utils import requant_table
    g, N, xd, wd, bd, ref = _case(s)
    Cout = s[4]
    s_w = torch.rand(Cout, generator=torch.Generator().manual_seed(9)) * 1e-3 + 1e-4
    s_out = torch.tensor([float(np.abs(ref).max()) * 0.02 * 1.1e-3 / (2 ** (out_bits - 1))])
    m, ek = requant_table(torch.tensor([0.02]), s_w, s_out, lift=False)
    (m[0], ek[0]), (m[1], ek[1]) = (1 << 30, 31), (3 << 28, 30)   # ratios 1/2 and 3/4: exact ties at odd v and at v = 2 mod 4
    lo, hi = -(1 << (out_bits - 1)), (1 << (out_bits - 1)) - 1
    m2, ek2, q2 = *((5 << 27, 31) if epilogue == 2 else (0, 0)), (lo // 2, hi // 2)
    ldo, c_off, sentinel = Cout + 32, 16, -77
    out = torch.full((int(np.prod(ref.shape[:3])) * ldo,), sentinel, dtype=torch.int8 if out_bits == 8 else torch.int16, device="cuda")
    md, ekd = torch.from_numpy(m).cuda(), torch.from_numpy(ek).cuda()
    a = _args(xd, wd, bd, g, out, epilogue=epilogue, ldo=ldo, c_off=c_off, out_bits=out_bits, m=md, ek=ekd, relu=relu, q=(lo, hi),
              m2=m2, ek2=ek2, q2=q2)
    assert _launch(a) == 0
    got = out.cpu().numpy().reshape(*ref.shape[:3], ldo)
    v = np.maximum(ref, 0) if relu else ref
    want = np.clip(np.stack([_dyadic(v[..., c], m[c], int(ek[c]) & 0xff) for c in range(Cout)], -1), lo, hi)
    if epilogue == 2:
        want = np.clip(_dyadic(want, m2, ek2), *q2)
    assert np.array_equal(got[..., c_off:c_off + Cout], want)
    assert (got[..., :c_off] == sentinel).all() and (got[..., c_off + Cout:] == sentinel).all()


def test_a_refused_block_is_an_error_and_writes_nothing():
    from hawq_amd import _lib
    g = (3, 3, 1, 1, 2, 12, 14, 32, 32)   # stride 2
    xd, wd, bd = (t.cuda() for t in _operands(g, 2, seed=1))
    out = torch.full((int(np.prod(_out_shape(g, 2))),), -9, dtype=torch.int32, device="cuda")
    a = _args(xd, wd, bd, g, out)
    assert _lib.load().hawq_incep_conv_band_ok(C.byref(a)) == 0 and _launch(a) != 0 and _lib.load().hawq_last_error()
    assert (out == -9).all()
