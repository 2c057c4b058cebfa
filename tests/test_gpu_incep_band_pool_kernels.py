"""The fused 3x3 conv + 3x3 / stride 2 max pool kernel (hawq_amd/csrc/incep_band_pool.hip, hawq_incep_conv_band_pool) against the
float64 conv, the host's integer requant and a numpy max."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_incep_tiled_kernels import _args, _dyadic, _operands, _reference

pytestmark = pytest.mark.gpu

# (pad, H, W, Cin, Cout): one pooled pixel; one pooled pixel with all nine taps at the border, the widest Cin, a ragged channel
# block; even Ho and Wo (the last conv row and column belong to no window); 45 K units (the odd half-step tail); Cin = 64; one
# pooled column over five steps of 8 conv rows (Ho = 39: 19 pooled rows, the last step holds 3); one pooled row over 34 pooled
# columns = five 7-column strips, the last with 6; then q_conv3 + q_pool1 and q_conv5 + q_pool2.  N = 3 on the small ones, so that
# the walk crosses image boundaries.
SHAPES = [(0, 5, 5, 16, 16), (1, 3, 3, 96, 208), (1, 12, 14, 32, 48), (0, 11, 13, 80, 80), (1, 12, 14, 64, 96), (0, 41, 5, 16, 32),
          (1, 3, 70, 48, 16), (1, 147, 147, 32, 64), (0, 73, 73, 80, 192)]
_cache = {}


def _case(s):
    """geometry, device operands and the float64 conv of shape `s`: computed once, shared, never changed"""
    if s not in _cache:
        g = (3, 3, s[0], s[0], 1, *s[1:])
        x, w, b = _operands(g, 1 if s in SHAPES[-2:] else 3, seed=sum(s))
        b[0], b[1] = 1, 2   # the tie channels keep both signs and parities under a ReLU
        _cache[s] = (g, x.cuda(), w.cuda(), b.cuda(), _reference(x, w, b, g).numpy())
    return _cache[s]


def _launch(a):
    from hawq_amd import _lib
    rc = _lib.load().hawq_incep_conv_band_pool(C.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("s", SHAPES, ids=lambda s: "p{}_{}x{}_c{}-{}".format(*s))
@pytest.mark.parametrize("out_bits,relu", [(8, 1), (16, 1), (16, 0)])
def test_equals_conv_requant_max_and_leaves_everything_else_alone(out_bits, relu, s):
    from hawq_amd.quant_utils import requant_table
    g, xd, wd, bd, ref = _case(s)
    Cout = s[4]
    s_w = torch.rand(Cout, generator=torch.Generator().manual_seed(9)) * 1e-3 + 1e-4
    s_out = torch.tensor([float(np.abs(ref).max()) * 0.02 * 1.1e-3 / (2 ** (out_bits - 1))])
    m, ek = requant_table(torch.tensor([0.02]), s_w, s_out, lift=False)
    (m[0], ek[0]), (m[1], ek[1]) = (1 << 30, 31), (3 << 28, 30)   # ratios 1/2 and 3/4: exact ties at odd v and at v = 2 mod 4
    lo, hi = -(1 << (out_bits - 1)), (1 << (out_bits - 1)) - 1
    v = np.maximum(ref, 0) if relu else ref
    q = np.clip(np.stack([_dyadic(v[..., c], m[c], int(ek[c]) & 0xff) for c in range(Cout)], -1), lo, hi)
    Hp, Wp = (q.shape[1] - 3) // 2 + 1, (q.shape[2] - 3) // 2 + 1
    want = np.max([q[:, dy:dy + 2 * Hp:2, dx:dx + 2 * Wp:2] for dy in range(3) for dx in range(3)], 0)
    ldo, c_off, sentinel, rows = Cout + 32, 16, -77, q.shape[0] * Hp * Wp
    buf = torch.full(((rows + 2) * ldo,), sentinel, dtype=torch.int8 if out_bits == 8 else torch.int16, device="cuda")
    a = _args(xd, wd, bd, g, buf[ldo:], epilogue=1, ldo=ldo, c_off=c_off, out_bits=out_bits, m=torch.from_numpy(m).cuda(),
              ek=torch.from_numpy(ek).cuda(), relu=relu, q=(lo, hi))   # one sentinel row in front of the tensor and one behind
    assert _launch(a) == 0
    got = buf.cpu().numpy().reshape(rows + 2, ldo)
    assert np.array_equal(got[1:-1, c_off:c_off + Cout].reshape(want.shape), want)
    got[1:-1, c_off:c_off + Cout] = sentinel
    assert (got == sentinel).all()


def test_a_refused_block_is_an_error_and_writes_nothing():
    from hawq_amd import _lib
    g = (3, 3, 1, 1, 2, 12, 14, 32, 32)   # stride 2
    xd, wd, bd = (t.cuda() for t in _operands(g, 2, seed=1))
    out = torch.full((2 * 6 * 7 * 32,), -9, dtype=torch.int8, device="cuda")
    t = torch.ones(32, dtype=torch.int32, device="cuda")
    a = _args(xd, wd, bd, g, out, epilogue=1, out_bits=8, m=t, ek=t * 31, q=(-128, 127))
    assert _lib.load().hawq_incep_conv_band_pool_ok(C.byref(a)) == 0 and _launch(a) != 0 and _lib.load().hawq_last_error()
    assert (out == -9).all()
