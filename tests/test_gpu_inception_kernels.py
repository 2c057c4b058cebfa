"""InceptionV3 kernels (hawq_amd/csrc/inception.hip) against exact host computations."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (KH, KW, pad_h, pad_w, stride, H, W, Cin, Cout): every conv geometry of the network (Cin 3 of the stem padded to 16)
GEOMETRIES = [
    (3, 3, 0, 0, 2, 299, 299, 16, 32), (3, 3, 0, 0, 1, 149, 149, 32, 32), (3, 3, 1, 1, 1, 147, 147, 32, 64),
    (1, 1, 0, 0, 1, 73, 73, 64, 80), (3, 3, 0, 0, 1, 73, 73, 80, 192), (1, 1, 0, 0, 1, 35, 35, 192, 48),
    (5, 5, 2, 2, 1, 35, 35, 48, 64), (3, 3, 1, 1, 1, 35, 35, 64, 96), (3, 3, 1, 1, 1, 35, 35, 96, 96),
    (3, 3, 0, 0, 2, 35, 35, 288, 384), (3, 3, 0, 0, 2, 35, 35, 96, 96), (1, 7, 0, 3, 1, 17, 17, 128, 128),
    (7, 1, 3, 0, 1, 17, 17, 160, 192), (3, 3, 0, 0, 2, 17, 17, 192, 320), (1, 1, 0, 0, 1, 8, 8, 1280, 448),
    (3, 3, 1, 1, 1, 8, 8, 448, 384), (1, 3, 0, 1, 1, 8, 8, 384, 384), (3, 1, 1, 0, 1, 8, 8, 384, 384),
]


def _lib():
    from hawq_amd import _lib
    return _lib


def _launch(x, w, b, KH, KW, ph, pw, stride, epilogue=0, out=None, ldo=None, c_off=0, out_bits=32, m=None, ek=None, relu=0,
            q=(0, 0), m2=0, ek2=0, q2=(0, 0)):
    L = _lib()
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = (H + 2 * ph - KH) // stride + 1, (W + 2 * pw - KW) // stride + 1
    if out is None:
        out = torch.empty(N * Ho * Wo * Cout, dtype=torch.int32, device="cuda")
        ldo = Cout
    a = L.IncepConvArgs()
    a.in_, a.wgt, a.bias, a.out = x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr()
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW = N, H, W, Cin, Cout, KH, KW
    a.stride, a.pad_h, a.pad_w, a.epilogue, a.relu = stride, ph, pw, epilogue, relu
    a.m, a.ek = (m.data_ptr() if m is not None else None), (ek.data_ptr() if ek is not None else None)
    a.q_lo, a.q_hi, a.m2, a.ek2, a.q2_lo, a.q2_hi = q[0], q[1], m2, ek2, q2[0], q2[1]
    a.out_bits, a.ldo, a.c_off = out_bits, ldo, c_off
    L.call("hawq_incep_conv", a, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out, (N, Ho, Wo)


def _reference(x, w, b, ph, pw, stride):
    """float64 conv on the CPU: exact for these integer operands (|sum| << 2^53)."""
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double(), b.double(), stride,
                                   (ph, pw))
    return y.permute(0, 2, 3, 1).round().long()


def _operands(g, N, seed):
    KH, KW, ph, pw, stride, H, W, Cin, Cout = g
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-128, 128, (N, H, W, Cin), generator=gen, dtype=torch.int8)
    w = torch.randint(-128, 128, (Cout, KH, KW, Cin), generator=gen, dtype=torch.int8)
    b = torch.randint(-2 ** 20, 2 ** 20, (Cout,), generator=gen, dtype=torch.int32)
    return x, w, b


@pytest.mark.parametrize("g", GEOMETRIES, ids=lambda g: "k{}x{}_p{}{}_s{}_{}x{}_c{}-{}".format(*g))
def test_raw_conv_equals_float64_conv(g):
    KH, KW, ph, pw, stride, H, W, Cin, Cout = g
    N = 1 if H * W * Cin > 1 << 20 else 2
    x, w, b = _operands(g, N, seed=H + Cin + KH * 7 + KW)
    out, (N, Ho, Wo) = _launch(x.cuda(), w.cuda(), b.cuda(), KH, KW, ph, pw, stride)
    ref = _reference(x, w, b, ph, pw, stride)
    assert ref.shape == (N, Ho, Wo, Cout)
    assert torch.equal(out.cpu().long().view(N, Ho, Wo, Cout), ref)


def _dyadic(v, m, e):
    """round_half_even(v * m / 2^e) in exact integers (the rounding of fixedpoint_fn's requant, quant_utils.py:404-408)."""
    v, m = v.astype(np.int64), np.broadcast_to(np.asarray(m, np.int64), v.shape)
    t = v * m
    half = np.int64(1) << (e - 1)
    q = (t + half) >> e
    tie = ((t + half) & ((np.int64(1) << e) - 1)) == 0
    return np.where(tie, q & ~np.int64(1), q)


@pytest.mark.parametrize("epilogue,out_bits,relu", [(1, 8, 1), (1, 16, 1), (2, 16, 1), (2, 16, 0)])
def test_requant_epilogues_match_host_maths_and_leave_neighbour_channels_alone(epilogue, out_bits, relu):
    from hawq_amd.quant_utils import requant_table
    g = (1, 7, 0, 3, 1, 17, 17, 64, 48)
    KH, KW, ph, pw, stride, H, W, Cin, Cout = g
    x, w, b = _operands(g, 2, seed=5)
    ref = _reference(x, w, b, ph, pw, stride).numpy()
    gen = torch.Generator().manual_seed(9)
    s_a = torch.tensor([0.02])
    s_w = torch.rand(Cout, generator=gen) * 1e-3 + 1e-4
    s_out = torch.tensor([float(np.abs(ref).max()) * 0.02 * 1.1e-3 / (2 ** (out_bits - 1))])
    m, ek = requant_table(s_a, s_w, s_out, lift=False)
    m[0], ek[0] = 1 << 30, 31   # ratio 1/2: every odd value is an exact tie
    m[1], ek[1] = 3 << 28, 30   # ratio 3/4: ties at v = 2 mod 4
    lo, hi = (-(1 << (out_bits - 1)), (1 << (out_bits - 1)) - 1)
    m2, ek2 = (5 << 27, 31) if epilogue == 2 else (0, 0)   # second requant ratio 5/16 with ties of its own
    q2 = (lo // 2, hi // 2)
    ldo, c_off = Cout + 32, 16
    dt = torch.int8 if out_bits == 8 else torch.int16
    sentinel = -77
    Ho, Wo = H, W
    out = torch.full((2 * Ho * Wo * ldo,), sentinel, dtype=dt, device="cuda")
    _launch(x.cuda(), w.cuda(), b.cuda(), KH, KW, ph, pw, stride, epilogue=epilogue, out=out, ldo=ldo, c_off=c_off,
            out_bits=out_bits, m=torch.from_numpy(m).cuda(), ek=torch.from_numpy(ek).cuda(), relu=relu, q=(lo, hi), m2=m2,
            ek2=ek2, q2=q2)
    got = out.cpu().numpy().reshape(2, Ho, Wo, ldo)
    v = np.maximum(ref, 0) if relu else ref
    e = (ek & 0xff).astype(np.int64)
    want = np.clip(np.stack([_dyadic(v[..., c], m[c], e[c]) for c in range(Cout)], -1), lo, hi)
    if epilogue == 2:
        want = np.clip(_dyadic(want, m2, ek2), *q2)
    assert np.array_equal(got[..., c_off:c_off + Cout], want)
    assert (got[..., :c_off] == sentinel).all() and (got[..., c_off + Cout:] == sentinel).all()
    assert (np.abs(v[..., 0]) % 2 == 1).any()   # the tie channel did see ties


def test_raw_conv_writes_only_its_concat_slice():
    g = (3, 1, 1, 0, 1, 8, 8, 384, 384)
    KH, KW, ph, pw, stride, H, W, Cin, Cout = g
    x, w, b = _operands(g, 2, seed=3)
    ldo, c_off = 3 * Cout + 16, Cout + 16
    out = torch.full((2 * H * W * ldo,), -5, dtype=torch.int32, device="cuda")
    _launch(x.cuda(), w.cuda(), b.cuda(), KH, KW, ph, pw, stride, out=out, ldo=ldo, c_off=c_off)
    got = out.cpu().view(2, H, W, ldo)
    assert torch.equal(got[..., c_off:c_off + Cout].long(), _reference(x, w, b, ph, pw, stride))
    assert (got[..., :c_off] == -5).all() and (got[..., c_off + Cout:] == -5).all()


@pytest.mark.parametrize("shape", [(2, 48, 35, 35), (1, 16, 17, 17), (2, 8, 8, 8)])
def test_avgpool3x3_equals_brute_force(shape):
    """16-bit integers (times a scale), sums of both signs: rint(x / s), 3x3 window with zero padding, trunc(sum / 9 + 0.01)."""
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(C)
    xi = torch.randint(-32768, 32768, shape, generator=gen).float()
    xi[0, 0] = 32767.0
    xi[-1, -1] = -32768.0
    s = 0.0123
    x = (xi * s).float()
    xd = x.cuda()
    y = torch.empty_like(xd)
    _lib().call("hawq_avgpool3x3_f32", xd.data_ptr(), y.data_ptr(), N * C, H, W, s, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    q = torch.round(x / torch.tensor(s, dtype=torch.float32)).long()   # x_int = round(x / s) on the CPU, IEEE binary32
    pad = torch.nn.functional.pad(q, (1, 1, 1, 1))
    ssum = sum(pad[:, :, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))
    num = 100 * ssum + 9
    p = torch.where(num >= 0, num // 900, -((-num) // 900))
    want = (p.float() * torch.tensor(s, dtype=torch.float32))
    assert torch.equal(y.cpu(), want)


def _pool_call(name, x, out, N, H, W, C, in_bits, ldo, c_off, out_bits, pre=None, post=None, in_pitch=None, in_off=0):
    L = _lib()
    a = L.IncepPoolArgs()
    a.in_, a.out = x.data_ptr(), out.data_ptr()
    a.N, a.H, a.W, a.C, a.in_bits, a.in_pitch, a.in_off = N, H, W, C, in_bits, (C if in_pitch is None else in_pitch), in_off
    a.out_bits, a.ldo, a.c_off = out_bits, ldo, c_off
    if pre:
        a.pre, (a.m1, a.ek1, a.lo1, a.hi1) = 1, pre
    if post:
        a.post, (a.m2, a.ek2, a.lo2, a.hi2) = 1, post
    L.call(name, a, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _rq(v, t):
    m, ek, lo, hi = t
    return np.clip(_dyadic(v, m, ek & 0xff), lo, hi)


def _trunc_avg(s, d):
    num = 100 * s + d
    return np.where(num >= 0, num // (100 * d), -((-num) // (100 * d)))


POOL_NAMES = {"requant": "hawq_incep_requant", "maxpool": "hawq_incep_maxpool3s2", "avgpool": "hawq_incep_avgpool_branch",
              "global": "hawq_incep_global_avgpool"}
PRE = (3 << 28, 30, -32768, 32767)                 # ratio 3/4, ties at 2 mod 4
POST8 = (5 << 27, 33, -128, 127)                   # ratio 5/64 to 8 bits
POST16 = (1 << 30, 31, -20000, 20000)              # ratio 1/2, every odd value a tie


def _check_pool(op, N, H, W, C, in_bits, out_bits, pre_t, post_t, ldo, c_off, in_pitch=None, in_off=0, seed=0):
    """one pool / requant launch against brute-force host maths: NHWC integers of `in_bits` in rows of `in_pitch` channels, of which
    the kernel reads [in_off, in_off + C); optional requant before (per element) and after; stored into the channel slice
    [c_off, c_off + C) of rows `ldo` wide, whose other channels must keep their sentinel"""
    in_pitch = C if in_pitch is None else in_pitch
    lim = 1 << (in_bits - 1)
    gen = np.random.default_rng(seed)
    xf = gen.integers(-lim, lim, (N, H, W, in_pitch)).astype(np.int16 if in_bits == 16 else np.int8)
    xf[0, 0, 0, in_off], xf[-1, -1, -1, in_off + C - 1] = lim - 1, -lim
    v = xf[..., in_off:in_off + C].astype(np.int64)
    if pre_t:
        v = _rq(v, pre_t)
    if op == "requant":
        r = v
    elif op == "maxpool":
        Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        r = np.max(np.stack([v[:, dy:dy + 2 * Ho - 1:2, dx:dx + 2 * Wo - 1:2] for dy in range(3) for dx in range(3)]), 0)
    elif op == "avgpool":
        p = np.pad(v, ((0, 0), (1, 1), (1, 1), (0, 0)))
        r = _trunc_avg(sum(p[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)), 9)
    else:
        r = _trunc_avg(v.sum((1, 2), keepdims=True), H * W)
    want = _rq(r, post_t) if post_t else r
    dt = torch.int8 if out_bits == 8 else torch.int16
    out = torch.full((N * want.shape[1] * want.shape[2] * ldo,), -3, dtype=dt, device="cuda")
    xd = torch.from_numpy(xf).cuda()
    _pool_call(POOL_NAMES[op], xd, out, N, H, W, C, in_bits, ldo, c_off, out_bits, pre=pre_t, post=post_t, in_pitch=in_pitch,
               in_off=in_off)
    got = out.cpu().numpy().reshape(N, want.shape[1], want.shape[2], ldo)
    assert np.array_equal(got[..., c_off:c_off + C], want)
    assert (got[..., :c_off] == -3).all() and (got[..., c_off + C:] == -3).all()
    assert np.abs(want).max() > 3   # the slice does not pass for sentinels
    return want


@pytest.mark.parametrize("op", ["requant", "maxpool", "avgpool", "global"])
def test_pool_kernels_match_brute_force_and_write_only_their_slice(op):
    """The fused plan's pool / requant launches: int16 NHWC in, optional requant before (per element) and after, stored into a
    channel slice of a wider row whose other channels keep their sentinel."""
    N, H, C = 2, {"requant": 9, "maxpool": 17, "avgpool": 17, "global": 8}[op], 48
    out_bits, pre_t, post_t = {"requant": (8, None, POST8), "maxpool": (16, PRE, POST16), "avgpool": (8, PRE, POST8),
                               "global": (8, None, POST8)}[op]
    _check_pool(op, N, H, H, C, 16, out_bits, pre_t, post_t, ldo=C + 48, c_off=32, seed=len(op))


def _engine_pool_descriptions():
    """(op, in_bits, out_bits, pre, post, C, in_pitch, ldo, c_off) of every pool / requant launch a built InceptionEngine issues,
    for both shipped schedules"""
    from hawq_amd import _lib as L
    from hawq_amd.api import build_quantized_resnet
    from hawq_amd.engine_inception import InceptionEngine
    from hawq_amd.quant_modules import QuantAct, freeze_model
    by_name = {v: k for k, v in POOL_NAMES.items()}
    out = []
    for scheme in ("uniform8", "uniform4"):
        model = build_quantized_resnet("inceptionv3", scheme, seed=0).cuda()
        for m in model.modules():
            if isinstance(m, QuantAct):
                m.x_min.fill_(-1.0 if m.quant_mode == "symmetric" else 0.0), m.x_max.fill_(1.0)
                m.compute_scale()
        freeze_model(model)
        eng = InceptionEngine(model)
        eng._build(1, 299, 299)   # the plan only: nothing is launched
        args = [a for a in eng._keep if isinstance(a, L.IncepPoolArgs)]
        names = [n for n in eng.op_names if n in by_name]
        assert len(args) == len(names) == eng.n_launches - 95 - 3   # all but the convs, the two input launches and the logits'
        out += [(by_name[n], a.in_bits, a.out_bits, bool(a.pre), bool(a.post), a.C, a.in_pitch, a.ldo, a.c_off)
                for n, a in zip(names, args)]
    return out


def test_pool_kernels_at_every_description_the_engine_launches():
    """Every distinct (op, widths, requants present, channel count, row pitches, slice offset) among the pool / requant launches of
    a built InceptionEngine - `_pool` is used five ways - at a small H != W map against the brute-force host maths."""
    descs = _engine_pool_descriptions()
    distinct = sorted(set(descs))
    kinds = {d[:5] for d in distinct}
    assert kinds == {("requant", 16, 8, False, True),    # a conv branch's q_input_act
                     ("maxpool", 8, 8, False, False),    # the stem's first max pool
                     ("maxpool", 16, 16, False, False),  # the stem's second
                     ("maxpool", 16, 16, True, True),    # a reduction unit's max-pool branch, into its slice
                     ("avgpool", 16, 8, True, True),     # an average-pool branch
                     ("requant", 16, 16, False, True),   # Inception-C's inner concat into the unit's slice
                     ("global", 16, 8, False, True)}, kinds
    assert {288, 768, 1280, 2048} <= {d[5] for d in distinct}
    assert any(d[0] == "maxpool" and d[8] > 0 for d in distinct) and any(d[:3] == ("requant", 16, 16) and d[8] > 0 for d in distinct)
    for i, (op, in_bits, out_bits, pre, post, C, in_pitch, ldo, c_off) in enumerate(distinct):
        assert in_pitch == C   # the engine never reads a slice: in_off > 0 is covered by the edge cases below
        H, W = {"requant": (5, 4), "maxpool": (7, 5), "avgpool": (5, 4), "global": (8, 8)}[op]
        post_t = (POST8 if out_bits == 8 else POST16) if post else None
        _check_pool(op, 2, H, W, C, in_bits, out_bits, PRE if pre else None, post_t, ldo=ldo, c_off=c_off, seed=100 + i)
    print(f"{len(descs)} pool launches, {len(distinct)} distinct descriptions")


@pytest.mark.parametrize("case", ["in_slice_requant", "in_slice_maxpool", "in_slice_avgpool", "in_slice_global", "in8_avgpool",
                                  "in8_requant_to_16", "in8_global", "maxpool_3x3_map", "maxpool_3x4_map", "grid_stride_twice"])
def test_pool_kernel_edges(case):
    """What the kernel supports and no plan exercises: an input channel slice (in_off > 0, in_pitch > C), 8-bit input with requants,
    H != W, a map of exactly the max pool's window, and more elements than the 8192 x 256 grid covers in one pass."""
    if case.startswith("in_slice_"):
        op = case[len("in_slice_"):]
        out_bits, pre_t, post_t = {"requant": (8, None, POST8), "maxpool": (16, PRE, POST16), "avgpool": (8, PRE, POST8),
                                   "global": (8, None, POST8)}[op]
        _check_pool(op, 2, 9, 7, 48, 16, out_bits, pre_t, post_t, ldo=96, c_off=32, in_pitch=112, in_off=48, seed=1)
    elif case == "in8_avgpool":
        _check_pool("avgpool", 2, 6, 9, 80, 8, 8, (3 << 28, 30, -128, 127), (1 << 30, 31, -128, 127), ldo=80, c_off=0, seed=2)
    elif case == "in8_requant_to_16":
        _check_pool("requant", 3, 5, 3, 32, 8, 16, None, (5 << 28, 28, -32768, 32767), ldo=64, c_off=16, in_pitch=48, in_off=16, seed=3)
    elif case == "in8_global":
        _check_pool("global", 2, 8, 5, 64, 8, 8, None, (1 << 30, 29, -128, 127), ldo=64, c_off=0, seed=4)
    elif case == "maxpool_3x3_map":
        want = _check_pool("maxpool", 2, 3, 3, 96, 16, 16, PRE, POST16, ldo=128, c_off=16, seed=5)
        assert want.shape == (2, 1, 1, 96)
    elif case == "maxpool_3x4_map":
        want = _check_pool("maxpool", 2, 3, 4, 64, 8, 8, None, None, ldo=64, c_off=0, seed=6)
        assert want.shape == (2, 1, 1, 64)
    else:
        N, H, W, C = 2, 24, 23, 2048
        assert N * H * W * C > 8192 * 256
        _check_pool("requant", N, H, W, C, 16, 8, None, POST8, ldo=C + 16, c_off=16, seed=7)
