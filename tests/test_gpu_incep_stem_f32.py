"""InceptionV3's fused fp32 stem on the GPU: hawq_incep_stem_f32 against exact host maths and against the three launches it replaces
(hawq_fakequant_f32 + hawq_f32_nchw_to_q_nhwc + hawq_incep_conv), byte for byte over whole sentinel-filled buffers, and
InceptionEngine(fused_stem=True) against the default engine and the live reference's fixtures.  No tolerance anywhere."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.guard import dev, out_buf
from tests.test_gpu_inception_network import _load_reference_state

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
# one output pixel; even sizes (the last input row and column are never read); P = 3 * 4 * 5 = 60, no multiple of 32; a strip that
# ends past the image (Ho = 17 = 4 * 4 + 1) beside P = 544 in more than one workgroup; the real row length (149 = 4 * 32 + 21 pixels)
SHAPES = [(1, 3, 3), (2, 4, 6), (3, 9, 11), (2, 35, 34), (1, 299, 299)]
CHANNELS = [(32, 32, 0), (16, 16, 0), (48, 64, 16)]   # (Cout, ldo, c_off); 48 = a full and a half 32-channel block


def _lib():
    from hawq_amd import _lib
    return _lib


# ------------------------------------------------------------------ host maths
def _dyadic(v, m, ek):
    """round_half_even(((v << k) * m) / 2^e), ek = e | k << 8, in exact integers - the host's integer requant as
    tests/test_gpu_incep_tiled_kernels.py restates it (fixedpoint_fn's rounding, quant_utils.py:404-408), with the table's pre-shift"""
    v = v.astype(np.int64)
    m, ek = np.broadcast_to(np.asarray(m, np.int64), v.shape), np.broadcast_to(np.asarray(ek, np.int64), v.shape)
    e, k = ek & 0xff, ek >> 8
    t = (v << k) * m
    half = np.int64(1) << (e - 1)
    q = (t + half) >> e
    tie = ((t + half) & ((np.int64(1) << e) - 1)) == 0
    return np.where(tie, q & ~np.int64(1), q)


def _quantise(x, inv, lo, hi):
    """the input QuantAct in binary32: float32 multiply, round half to even, clip"""
    with np.errstate(over="ignore"):
        r = np.rint(np.float32(inv) * x.astype(np.float32))
    assert r.dtype == np.float32
    return np.clip(r, np.float32(lo), np.float32(hi)).astype(np.int64)


def _conv27(q, w):
    """int64 3x3 / stride 2 / pad 0 conv of the 27 taps: q [N][3][H][W], w [Cout][3][3][3] -> [N][Ho][Wo][Cout]"""
    N, _, Hh, Ww = q.shape
    Ho, Wo = (Hh - 3) // 2 + 1, (Ww - 3) // 2 + 1
    acc = np.zeros((N, Ho, Wo, w.shape[0]), np.int64)
    for c in range(3):
        for kh in range(3):
            for kw in range(3):
                win = q[:, c, kh:kh + 2 * Ho - 1:2, kw:kw + 2 * Wo - 1:2]
                acc += win[..., None] * w[:, c, kh, kw].astype(np.int64)
    return acc


@functools.lru_cache(maxsize=None)
def _operands(shape, cout):
    """images, weights, bias and tables of a (shape, Cout) case, with the accumulators (host maths) - computed once, shared by the
    clamp / ReLU cases, never modified.  Channels 0 and 1 carry exact requant ties: m = 2^30 with e = 31 + 1 as (e = 32, k = 1) and as
    (e = 31, k = 0), both the ratio 1/2, where every odd accumulator is a tie; their weights are small so that the ties survive the clamp."""
    N, Hh, Ww = shape
    g = torch.Generator().manual_seed(1000 * N + 10 * Hh + Ww + cout)
    inv, in_lo, in_hi = 37.25, -128, 127
    x = torch.randn((N, 3, Hh, Ww), generator=g, dtype=torch.float32).numpy()
    flat = x.reshape(-1)
    # -0.0, values beyond both clamp bounds (finite, overflowing inv * x, infinite), the bounds themselves and their half-way points
    plant = np.array([-0.0, 0.0, 1e6, -1e6, 3e38, -3e38, np.inf, -np.inf, 127 / inv, -128 / inv, 127.5 / inv, -128.5 / inv, 4.0, -4.0],
                     np.float32)
    pos = np.arange(plant.size) * max(1, flat.size // plant.size - 1) % flat.size
    flat[pos] = plant
    w = torch.randint(-128, 128, (cout, 3, 3, 3), generator=g, dtype=torch.int8).numpy()
    w[:2] = torch.randint(-2, 3, (2, 3, 3, 3), generator=g, dtype=torch.int8).numpy()
    b = torch.randint(-2 ** 16, 2 ** 16, (cout,), generator=g, dtype=torch.int32).numpy()
    b[0], b[1] = 1, 2
    m = torch.randint(2 ** 29, 2 ** 31 - 1, (cout,), generator=g, dtype=torch.int64).numpy().astype(np.int32)
    ek = (33 + np.arange(cout) % 13).astype(np.int32)   # e across 33 .. 45
    m[0], ek[0] = 1 << 30, 32 | (1 << 8)
    m[1], ek[1] = 1 << 30, 31
    q = _quantise(x, inv, in_lo, in_hi)
    assert q.min() == in_lo and q.max() == in_hi
    acc = _conv27(q, w)
    for a in (x, w, b, m, ek, acc):
        a.setflags(write=False)
    return x, inv, in_lo, in_hi, w, b, m, ek, acc


def _expected(acc, b, m, ek, relu, qrange):
    v = acc + b.astype(np.int64)
    if relu:
        v = np.maximum(v, 0)
    return v, np.clip(_dyadic(v, m, ek), *qrange)


# ------------------------------------------------------------------ device plumbing
def _conv1_args(N, Hh, Ww, cin, wgt, bias, m, ek, out, cout, ldo, c_off, relu, qrange, in_=None):
    a = _lib().IncepConvArgs()
    a.in_, a.wgt, a.bias, a.out, a.m, a.ek = in_, wgt.data_ptr(), bias.data_ptr(), out.data_ptr(), m.data_ptr(), ek.data_ptr()
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad_h, a.pad_w = N, Hh, Ww, cin, cout, 3, 3, 2, 0, 0
    a.epilogue, a.relu, a.q_lo, a.q_hi, a.out_bits, a.ldo, a.c_off = _lib().INCEP_REQUANT, relu, qrange[0], qrange[1], 8, ldo, c_off
    return a


def _run_both(x, inv, in_lo, in_hi, w, b, m, ek, cout, ldo, c_off, relu, qrange):
    """(bytes of hawq_incep_stem_f32, bytes of the three launches it replaces), each a whole sentinel-filled [P][ldo] buffer"""
    from hawq_amd.engine_inception import pack_stem_u8_weights
    lib = _lib()
    N, _, Hh, Ww = x.shape
    Ho, Wo = (Hh - 3) // 2 + 1, (Ww - 3) // 2 + 1
    s = torch.cuda.current_stream().cuda_stream
    # (buffers come from the guard arena when the calling test has made one current: tests/test_gpu_contract_edges.py)
    xd = dev(x.copy())
    bd, md, ekd = (dev(t.copy()) for t in (b, m, ek))
    # the fused launch
    wt = dev(pack_stem_u8_weights(w, cout))
    out = out_buf(N * Ho * Wo * ldo, torch.int8, SENTINEL)
    a = _conv1_args(N, Hh, Ww, 3, wt, bd, md, ekd, out, cout, ldo, c_off, relu, qrange)
    assert lib.load().hawq_incep_stem_f32_ok(xd.data_ptr(), inv, in_lo, in_hi, C.byref(a)) == 1
    lib.call("hawq_incep_stem_f32", xd.data_ptr(), inv, in_lo, in_hi, C.byref(a), s)
    # the default plan's three launches: fake-quantise, NCHW -> NHWC int8 padded to 16 channels, hawq_incep_conv at K = 9 x 16
    xq = out_buf(tuple(xd.shape), torch.float32, None)
    x0 = out_buf(N * Hh * Ww * 16, torch.int8, SENTINEL)
    w16 = np.zeros((cout, 3, 3, 16), np.int8)
    w16[..., :3] = w.transpose(0, 2, 3, 1)
    w16d = dev(w16)
    base = out_buf(out.numel(), torch.int8, SENTINEL)
    a3 = _conv1_args(N, Hh, Ww, 16, w16d, bd, md, ekd, base, cout, ldo, c_off, relu, qrange, in_=x0.data_ptr())
    lib.call("hawq_fakequant_f32", xd.data_ptr(), xq.data_ptr(), xd.numel(), inv, 1.0, in_lo, in_hi, s)
    lib.call("hawq_f32_nchw_to_q_nhwc", xq.data_ptr(), x0.data_ptr(), N, 3, Hh, Ww, 16, 8, 1.0, s)
    lib.call("hawq_incep_conv", C.byref(a3), s)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(N, Ho, Wo, ldo), base.cpu().numpy().reshape(N, Ho, Wo, ldo)


def _check(got, base, want, cout, c_off):
    print("bytes differing from the three launches:", int((got != base).sum()), "of", got.size,
          "| from host maths:", int((got[..., c_off:c_off + cout].astype(np.int64) != want).sum()), "of", want.size)
    assert np.array_equal(got[..., c_off:c_off + cout].astype(np.int64), want), "differs from host maths"
    assert np.array_equal(got, base), "differs from fakequant + nchw_to_q + hawq_incep_conv"
    rest = np.ones(got.shape[-1], bool)
    rest[c_off:c_off + cout] = False
    assert (got[..., rest] == SENTINEL).all(), "bytes outside the channel slice changed"


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "{}x{}x{}".format(*s))
@pytest.mark.parametrize("channels", CHANNELS, ids=lambda c: "c{}_ldo{}_off{}".format(*c))
@pytest.mark.parametrize("relu", [0, 1], ids=["linear", "relu"])
@pytest.mark.parametrize("qrange", [(-128, 127), (0, 15)], ids=["int8", "uint4"])
def test_stem_f32_equals_host_maths_and_the_three_launches(shape, channels, relu, qrange):
    cout, ldo, c_off = channels
    x, inv, in_lo, in_hi, w, b, m, ek, acc = _operands(shape, cout)
    v, want = _expected(acc, b, m, ek, relu, qrange)
    got, base = _run_both(x, inv, in_lo, in_hi, w, b, m, ek, cout, ldo, c_off, relu, qrange)
    _check(got, base, want, cout, c_off)
    if np.prod(shape) > 9:   # (more than one output pixel) the cases test what they claim
        assert len(np.unique(want)) > 4
    if np.prod(shape) > 1000:   # hundreds of pixels: channels 0 and 1 did meet exact ties, and not only clamped ones
        odd = (np.abs(v[..., :2]) % 2 == 1)
        assert odd.any(), "no exact requant tie"
        if qrange == (-128, 127):
            assert (odd & (np.abs(v[..., :2]) < 250)).any(), "every tie was clamped away"


def test_stem_f32_rounds_half_to_even_and_clamps_the_input():
    """inv_scale = 32 on values (k + 0.5) / 32: every product is exactly half-way, so rintf must round to the even neighbour; the input
    clamp (-100, 90) is asymmetric and cuts both ends of k = -140 .. 139."""
    N, Hh, Ww, cout = 2, 35, 34, 32
    k = (np.arange(N * 3 * Hh * Ww, dtype=np.int64) * 7) % 280 - 140
    x = ((k.astype(np.float32) + np.float32(0.5)) / np.float32(32)).reshape(N, 3, Hh, Ww)
    assert np.array_equal(x.reshape(-1).astype(np.float64) * 32, k + 0.5)   # exact in binary32
    q = _quantise(x, 32.0, -100, 90)
    assert np.array_equal(q.reshape(-1), np.clip(np.where(k % 2 == 0, k, k + 1), -100, 90))
    _, _, _, _, w, b, m, ek, _ = _operands((N, Hh, Ww), cout)
    v, want = _expected(_conv27(q, w), b, m, ek, 1, (-128, 127))
    got, base = _run_both(x, 32.0, -100, 90, w, b, m, ek, cout, cout, 0, 1, (-128, 127))
    _check(got, base, want, cout, 0)


def test_stem_f32_refused_description_sets_the_error_and_writes_nothing():
    lib = _lib()
    x, inv, in_lo, in_hi, w, b, m, ek, _ = _operands((2, 4, 6), 32)
    xd = torch.from_numpy(x.copy()).cuda()
    t = [torch.from_numpy(v.copy()).cuda() for v in (np.zeros((32, 32), np.int8), b, m, ek)]
    out = torch.full((2 * 1 * 2 * 32,), SENTINEL, dtype=torch.int8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for change in ({"Cin": 16}, {"stride": 1}, {"epilogue": 2}, {"c_off": 16}, {"inv": float("nan")}, {"in_hi": 128}):
        a = _conv1_args(2, 4, 6, 3, t[0], t[1], t[2], t[3], out, 32, 32, 0, 1, (-128, 127))
        args = {"inv": inv, "in_lo": in_lo, "in_hi": in_hi}
        for name, value in change.items():
            if name in args:
                args[name] = value
            else:
                setattr(a, name, value)
        assert lib.load().hawq_incep_stem_f32_ok(xd.data_ptr(), args["inv"], args["in_lo"], args["in_hi"], C.byref(a)) == 0, change
        with pytest.raises(RuntimeError, match="hawq_incep_stem_f32"):
            lib.call("hawq_incep_stem_f32", xd.data_ptr(), args["inv"], args["in_lo"], args["in_hi"], C.byref(a), s)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------ 2. the network: the reference's frozen state
@functools.lru_cache(maxsize=None)
def _reference_model(scheme):
    from hawq_amd.api import build_quantized_resnet
    fx = H.load(f"net_inceptionv3_{scheme}_b2.npz")
    q = build_quantized_resnet("inceptionv3", scheme, seed=0).cuda()
    _load_reference_state(q, fx)
    q.invalidate_engine()
    return q, fx


def _images(b, seed=0):
    from hawq_amd.skeleton import synthetic_images
    return synthetic_images(b, seed=seed, size=299)


def _engine(model, **kw):
    from hawq_amd.engine_inception import InceptionEngine
    return InceptionEngine(model, **kw)


def _units(eng, model):
    return {n: eng.unit_output(n) for n, _ in model.units()}


def _assert_fused_launch_list(eng):
    names = eng.op_names
    assert eng.n_launches == len(names) == 145
    assert names[0] == "hawq_incep_stem_f32" and names.count("hawq_incep_stem_f32") == 1
    assert "hawq_fakequant_f32" not in names and "hawq_f32_nchw_to_q_nhwc" not in names


@pytest.mark.parametrize("scheme", ["uniform8", "uniform4"])
def test_fused_stem_plan_matches_the_default_plan_and_the_golden(scheme):
    model, fx = _reference_model(scheme)
    x = _images(2)
    assert H.sha(x.numpy()) == str(fx["input_sha"])
    base, fused = _engine(model), model.engine(fused_stem=True)
    assert model.engine() is fused and fused.fused_stem
    with torch.no_grad():
        y0, y1 = base(x.cuda()), model(x.cuda())
        assert torch.equal(fused(x.cuda()), y1)   # replay of the captured graph
    assert model._engine is fused and fused._graph is not None
    _assert_fused_launch_list(fused)
    assert base.n_launches == 147 and base.op_names[:2] == ["hawq_fakequant_f32", "hawq_f32_nchw_to_q_nhwc"]
    assert fused.conv_launches == base.conv_launches and len(fused.conv_launches) == 95
    u0, u1 = _units(base, model), _units(fused, model)
    for i, n in enumerate(fx["unit_names"]):
        assert np.array_equal(u1[str(n)], u0[str(n)]), n
        assert np.array_equal(H.digest(u1[str(n)]), fx["unit_digest"][i]), n
    assert torch.equal(y1, y0)
    assert np.array_equal(y1.cpu().numpy(), fx["logits"])
    model.invalidate_engine()
    assert model.engine().fused_stem is False


@pytest.mark.parametrize("batch", [1, 3])
def test_fused_stem_on_unseen_images_graph_and_eager(batch):
    model, _ = _reference_model("uniform8")
    x = torch.randn((batch, 3, 299, 299), generator=torch.Generator().manual_seed(40 + batch)).cuda()
    base, fused, eager = _engine(model), _engine(model, fused_stem=True), _engine(model, fused_stem=True, use_graph=False)
    with torch.no_grad():
        y0, y1, y2 = base(x), fused(x), eager(x)
        assert torch.equal(fused(x), y1)
    assert fused._graph is not None and eager._graph is None
    _assert_fused_launch_list(fused)
    _assert_fused_launch_list(eager)
    u0, u1, u2 = _units(base, model), _units(fused, model), _units(eager, model)
    for n in u0:
        assert np.array_equal(u1[n], u0[n]) and np.array_equal(u2[n], u0[n]), n
    assert torch.equal(y1, y0) and torch.equal(y2, y0) and y0.abs().max() > 0


def test_fused_stem_composes_with_fast_pools_tune_and_plans():
    model, _ = _reference_model("uniform8")
    x = _images(2, seed=5).cuda()
    with torch.no_grad():
        y0 = _engine(model)(x)
        pools = _engine(model, fused_stem=True, fast_pools=True)
        assert torch.equal(pools(x), y0)
        _assert_fused_launch_list(pools)
        assert "hawq_incep_pool_v" in pools.op_names
        # tuned with the fused stem: conv1 is neither timed nor re-issued, its entry records tile 0
        tuned_f = _engine(model, fused_stem=True, tune=True, fast_pools=True)
        assert torch.equal(tuned_f(x), y0)
        _assert_fused_launch_list(tuned_f)
        assert tuned_f.op_names.count("hawq_incep_conv_tiled") == 94 and "hawq_incep_conv" not in tuned_f.op_names
        assert tuned_f.conv_tiles[0] == 0 and tuned_f.conv_us[0] == {} and all(0 in us for us in tuned_f.conv_us[1:])
        # tuned without it
        tuned_d = _engine(model, tune=True)
        assert torch.equal(tuned_d(x), y0)
        assert 0 in tuned_d.conv_us[0]
        from hawq_amd.engine_inception import _TUNE_REPS, _TUNE_WARMUP
        per = _TUNE_WARMUP + _TUNE_REPS
        assert tuned_f.n_timing_launches == per * sum(len(us) for us in tuned_f.conv_us) > 0
        assert tuned_d.n_timing_launches == per * sum(len(us) for us in tuned_d.conv_us)
        assert len(tuned_d.conv_us[0]) >= 1 and tuned_f.conv_launches == tuned_d.conv_launches
        # plans cross over in both directions, through JSON, and time nothing
        plan_d, plan_f = json.loads(json.dumps(tuned_d.export_plan())), json.loads(json.dumps(tuned_f.export_plan()))
        assert plan_d["launches"] == plan_f["launches"] and plan_f["tiles"][0] == 0
        T = _lib().load().hawq_incep_conv_num_tiles()
        plan_d["tiles"][0] = T   # whatever id conv1 carries is ignored by a fused-stem plan, as the uint8 plan ignores it
        a = _engine(model, fused_stem=True, plan=plan_d)
        b = _engine(model, plan=plan_f)
        assert torch.equal(a(x), y0) and torch.equal(b(x), y0)
        assert a.n_timing_launches == 0 and b.n_timing_launches == 0
        assert a.conv_tiles == plan_d["tiles"] and b.conv_tiles == plan_f["tiles"]
        _assert_fused_launch_list(a)
        assert b.n_launches == 147 and b.op_names[2] == "hawq_incep_conv_tiled"
        assert a.export_plan()["tiles"] == plan_d["tiles"]


def test_forward_uint8_and_alternation_on_a_fused_stem_engine():
    model, _ = _reference_model("uniform8")
    u8 = torch.randint(0, 256, (2, 299, 299, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).cuda()
    x = _images(2, seed=9).cuda()
    base, fused = _engine(model), _engine(model, fused_stem=True)
    with torch.no_grad():
        y8 = base.forward_uint8(u8)
        y32 = base(x)
        a = fused(x)
        b = fused.forward_uint8(u8)
        plan = (fused.x_in.data_ptr(), fused.x_u8.data_ptr(), fused._graph.value, fused._graph_u8.value)
        c = fused(x)
        d = fused.forward_uint8(u8)
        e = fused(x)
    assert plan == (fused.x_in.data_ptr(), fused.x_u8.data_ptr(), fused._graph.value, fused._graph_u8.value)   # no rebuild
    assert torch.equal(b, y8) and torch.equal(d, y8)
    assert torch.equal(a, y32) and torch.equal(c, y32) and torch.equal(e, y32)
    names8 = [op.args[0] for op in fused._ops_u8]
    assert fused.n_launches_u8 == 145 and names8[0] == "hawq_incep_stem_u8" and "hawq_incep_stem_f32" not in names8
    assert fused._ops_u8[1:] == fused._ops[1:]
    assert names8 == [op.args[0] for op in base._ops_u8]


def test_fused_stem_refuses_a_16_bit_input_quantact():
    from hawq_amd.api import build_quantized_resnet, calibrate
    from hawq_amd.engine_inception import PlanNotApplicable
    model = build_quantized_resnet("inceptionv3", "uniform8", seed=1).cuda()
    x = _images(1).cuda()
    calibrate(model, x)
    ia = model.features.q_init_block.q_input_activ
    ia.activation_bit = 16
    with torch.no_grad():
        with pytest.raises(PlanNotApplicable, match="fused_stem: the input QuantAct"):
            _engine(model, fused_stem=True)(x)
        y = _engine(model)(x)   # the default plan still takes the model
    assert y.shape == (1, 1000) and bool(torch.isfinite(y).all())
