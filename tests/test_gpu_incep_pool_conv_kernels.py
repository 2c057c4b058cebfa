"""The fused 3x3 average pool + 1x1 conv kernel (hawq_amd/csrc/incep_pool_conv.hip, hawq_incep_avgpool_conv) against a plain int64
numpy computation and, over the whole buffer, against hawq_incep_avgpool_branch + hawq_incep_conv on the same inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_incep_tiled_kernels import _args, _dyadic, _operands

pytestmark = pytest.mark.gpu

# (N, H, W, C, Cout).  The kernel walks C in chunks of 64 and owns bands of full rows, which it halves while the launch has fewer than
# 256 workgroups: at N = 3 every band below is two rows (one where the map is one).  1 x 1 (one tap in the map) and 3 x 3 (every
# window touches the padding); 8 x 8 in four bands of 16 pixels, C = one chunk + 16; 17 x 17 on both configurations (Cout <= 64 and
# the limit 192) in bands of 34 pixels, a ragged second pixel tile and a one-row last band, three chunks with a 16-channel tail;
# one-row bands of the widest maps either configuration takes (110 and 62 columns).  Then the launches that fill the chip and keep
# their bands: 128 images of 9 x 36 (five rows, then four: 180 pixels), 256 of 7 x 35 (245 pixels: all eight pixel tiles and four
# pool items of the wide configuration), 96 of 17 x 17 with Cout 80 (rows 6, 6, 5: 102 pixels, the second pool item and second
# tile row of the deep configuration) and 256 of 8 x 8 (a whole image in two pixel tiles).
SHAPES = [(3, 1, 1, 16, 16), (3, 3, 3, 48, 32), (3, 8, 8, 80, 80), (3, 17, 17, 144, 192), (3, 17, 17, 48, 64), (3, 2, 110, 16, 32),
          (3, 2, 62, 16, 80), (128, 9, 36, 16, 32), (256, 7, 35, 16, 32), (96, 17, 17, 16, 80), (256, 8, 8, 16, 80)]
FORMS = [(1, 8, 1), (2, 16, 1), (2, 16, 0)]   # (epilogue, out_bits, relu)
PRE, POST = (3 << 28, 31, -120, 120), (1 << 30, 31, -100, 100)   # ratios 3/8 (the clamp binds) and 1/2 (a tie at every odd value)
_cache = {}


def _case(s):
    """device operands, pool block fields and the exact int64 accumulators of shape `s`: computed once, shared, never changed"""
    if s not in _cache:
        N, H, W, Cc, Cout = s
        pitch, off = Cc + 32, 16
        x = torch.randint(-600, 600, (N, H, W, pitch), generator=torch.Generator().manual_seed(sum(s)), dtype=torch.int16)
        _, w, b = _operands((1, 1, 0, 0, 1, H, W, Cc, Cout), 1, seed=sum(s))
        b[0], b[1] = 1, 2   # the tie channels keep both signs and parities under a ReLU
        v = np.clip(_dyadic(x.numpy()[..., off:off + Cc].astype(np.int64), PRE[0], PRE[1]), PRE[2], PRE[3])
        vp = np.pad(v, ((0, 0), (1, 1), (1, 1), (0, 0)))
        t = 100 * sum(vp[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)) + 9
        pooled = np.clip(_dyadic(np.sign(t) * (np.abs(t) // 900), POST[0], POST[1]), POST[2], POST[3])   # truncation toward zero
        acc = pooled.reshape(-1, Cc) @ w.numpy().reshape(Cout, Cc).astype(np.int64).T + b.numpy().astype(np.int64)
        _cache[s] = (x.cuda(), w.cuda(), b.cuda(), pitch, off, acc)
    return _cache[s]


def _pool_block(x, s, pitch, off, out=None):
    from hawq_amd import _lib
    p = _lib.IncepPoolArgs()
    p.in_, p.out = x.data_ptr(), (out.data_ptr() if out is not None else None)
    p.N, p.H, p.W, p.C, p.in_bits, p.in_pitch, p.in_off, p.out_bits, p.ldo = *s[:4], 16, pitch, off, 8, s[3]
    (p.pre, p.m1, p.ek1, p.lo1, p.hi1), (p.post, p.m2, p.ek2, p.lo2, p.hi2) = (1, *PRE), (1, *POST)
    return p


def _call(name, *args):
    from hawq_amd import _lib
    rc = getattr(_lib.load(), name)(*args, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("s", SHAPES, ids=lambda s: "n{}_{}x{}_c{}-{}".format(*s))
@pytest.mark.parametrize("epilogue,out_bits,relu", FORMS)
def test_equals_pool_then_conv_and_leaves_everything_else_alone(epilogue, out_bits, relu, s):
    from hawq_amd.quant_utils import requant_table
    xd, wd, bd, pitch, off, acc = _case(s)
    N, H, W, Cc, Cout = s
    s_w = torch.rand(Cout, generator=torch.Generator().manual_seed(9)) * 1e-3 + 1e-4
    s_out = torch.tensor([float(np.abs(acc).max()) * 0.02 * 1.1e-3 / (2 ** (out_bits - 1))])
    m, ek = requant_table(torch.tensor([0.02]), s_w, s_out, lift=False)
    (m[0], ek[0]), (m[1], ek[1]) = (1 << 30, 31), (3 << 28, 30)   # ratios 1/2 and 3/4: exact ties at odd v and at v = 2 mod 4
    lo, hi = -(1 << (out_bits - 1)), (1 << (out_bits - 1)) - 1
    m2, ek2, q2 = ((5 << 27, 31, (lo // 2, hi // 2)) if epilogue == 2 else (0, 0, (0, 0)))
    v = np.maximum(acc, 0) if relu else acc
    want = np.clip(np.stack([_dyadic(v[:, c], m[c], int(ek[c]) & 0xff) for c in range(Cout)], -1), lo, hi)
    if epilogue == 2:
        want = np.clip(_dyadic(want, m2, ek2), *q2)
    ldo, c_off, sentinel, rows = Cout + 32, 16, -77, N * H * W
    dt = torch.int8 if out_bits == 8 else torch.int16
    bufs = [torch.full(((rows + 2) * ldo,), sentinel, dtype=dt, device="cuda") for _ in range(2)]
    dense = torch.zeros(rows * Cc, dtype=torch.int8, device="cuda")   # the pooled tensor of the two-launch form
    g, md, ekd = (1, 1, 0, 0, 1), torch.from_numpy(m).cuda(), torch.from_numpy(ek).cuda()
    blocks = [_args(dense.view(N, H, W, Cc), wd, bd, g, buf[ldo:], epilogue=epilogue, ldo=ldo, c_off=c_off, out_bits=out_bits, m=md,
                    ek=ekd, relu=relu, q=(lo, hi), m2=m2, ek2=ek2, q2=q2) for buf in bufs]   # a sentinel row in front and one behind
    blocks[0].in_ = None   # the fused launch ignores it
    assert _call("hawq_incep_avgpool_conv", C.byref(_pool_block(xd, s, pitch, off)), C.byref(blocks[0])) == 0
    assert _call("hawq_incep_avgpool_branch", C.byref(_pool_block(xd, s, pitch, off, dense))) == 0
    assert _call("hawq_incep_conv", C.byref(blocks[1])) == 0
    assert torch.equal(bufs[0], bufs[1]), "differs from hawq_incep_avgpool_branch + hawq_incep_conv"
    got = bufs[0].cpu().numpy().reshape(rows + 2, ldo)
    assert np.array_equal(got[1:-1, c_off:c_off + Cout], want)
    got[1:-1, c_off:c_off + Cout] = sentinel
    assert (got == sentinel).all()


def test_a_refused_pair_is_an_error_and_writes_nothing():
    from hawq_amd import _lib
    s = (2, 8, 8, 16, 208)   # Cout above the kernel's limit
    x = torch.zeros(2, 8, 8, 48, dtype=torch.int16, device="cuda")
    _, w, b = (t.cuda() for t in _operands((1, 1, 0, 0, 1, 8, 8, 16, 208), 1, seed=1))
    out = torch.full((2 * 8 * 8 * 208,), -9, dtype=torch.int8, device="cuda")
    t = torch.ones(208, dtype=torch.int32, device="cuda")
    c = _args(x[..., :16], w, b, (1, 1, 0, 0, 1), out, epilogue=1, out_bits=8, m=t, ek=t * 31, q=(-128, 127))
    p = _pool_block(x, s, 48, 16)
    assert _lib.load().hawq_incep_avgpool_conv_ok(C.byref(p), C.byref(c)) == 0
    assert _call("hawq_incep_avgpool_conv", C.byref(p), C.byref(c)) != 0 and _lib.load().hawq_last_error()
    assert (out == -9).all()
