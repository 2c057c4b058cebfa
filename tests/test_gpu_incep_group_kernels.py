"""The grouped InceptionV3 conv launch (hawq_amd/csrc/incep_group.hip, hawq_incep_conv_group) against its members launched one by one
through hawq_incep_conv_tiled with the same tile, byte for byte over whole sentinel-filled output buffers, and against exact host
computations (float64 conv + the dyadic requant in integers).  The cases are the smallest shapes at which the mapping workgroup ->
member -> (pixel block, channel block) can go wrong; each runs on every tile all its members accept."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RAW, RQ, RQ2 = 0, 1, 2
SENTINEL = -77


def _m(KH, KW, ph, pw, stride, H, W, Cin, Cout, epilogue=RQ, out_bits=8, out=None, ldo=None, c_off=0, x=None):
    """a member: geometry, epilogue, the output buffer it writes (`out`: a name shared by the slices of one buffer) and the input it
    reads (`x`: a name shared by members that read one tensor)"""
    return dict(g=(KH, KW, ph, pw, stride, H, W, Cin, Cout), epilogue=epilogue, out_bits=32 if epilogue == RAW else out_bits, out=out,
                ldo=Cout if ldo is None else ldo, c_off=c_off, x=x)


# name -> (members, indices of the members that are also checked against the host computation)
CASES = {
    # P = 16 N and 81 N: neither a multiple of a pixel tile, and the first member ends mid-way through the grid
    "mixed_pixels": ([_m(3, 3, 0, 0, 2, 9, 9, 48, 80), _m(1, 1, 0, 0, 1, 9, 9, 48, 16)], (0, 1)),
    # 64-channel tiles: 1, 2, 3, 4 channel blocks per member; 128-channel tiles would be 1, 1, 2, 2 (refused here: Cout 16)
    "mixed_channel_blocks": ([_m(1, 1, 0, 0, 1, 8, 8, 32, co) for co in (16, 80, 144, 208)], (3,)),
    # P = 289 N crosses pixel tiles inside an image; K = 1120
    "level_17": ([_m(1, 7, 0, 3, 1, 17, 17, 160, 160), _m(7, 1, 3, 0, 1, 17, 17, 160, 192)], (1,)),
    # slices 0 .. 64 and 160 .. 192 of one int16 buffer (64 .. 160 stay sentinel), an int8 buffer, a RAW int32 buffer
    "concat_level": ([_m(1, 1, 0, 0, 1, 8, 8, 64, 64, RQ2, 16, "cat", 192, 0), _m(1, 1, 0, 0, 1, 8, 8, 64, 48),
                      _m(1, 1, 0, 0, 1, 8, 8, 64, 96, RAW), _m(1, 1, 0, 0, 1, 8, 8, 64, 32, RQ2, 16, "cat", 192, 160)], (2, 3)),
    # the 8 x 8 units' second level: K >= 512 everywhere, so the K-split tile takes it and reduces inside a group
    "pair_8": ([_m(1, 3, 0, 1, 1, 8, 8, 384, 384, RQ2, 16, "inner", 768, 0, "x"), _m(3, 1, 1, 0, 1, 8, 8, 384, 384, RQ2, 16, "inner", 768, 384, "x"),
                _m(3, 3, 1, 1, 1, 8, 8, 448, 384)], (1,)),
    "one_member": ([_m(1, 1, 0, 0, 1, 5, 5, 16, 16)], (0,)),
    "eight_members": ([_m(1, 1, 0, 0, 1, 5, 5, 16, 16) for _ in range(8)], (7,)),
}


def _lib():
    from hawq_amd import _lib
    return _lib


def _accepting_tiles(members):
    """host-only (no device): the tile ids every member accepts - the fabricated pointers are never dereferenced"""
    L, tiles = _lib().load(), []
    for t in range(1, L.hawq_incep_conv_num_tiles() + 1):
        for m in members:
            a = _lib().IncepConvArgs()
            a.in_, a.wgt, a.bias, a.out, a.m, a.ek = 16, 16, 16, 16, 16, 16
            KH, KW, ph, pw, stride, H, W, Cin, Cout = m["g"]
            a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad_h, a.pad_w = 1, H, W, Cin, Cout, KH, KW, stride, ph, pw
            a.epilogue, a.out_bits, a.ldo, a.c_off, a.q_hi, a.q2_hi = m["epilogue"], m["out_bits"], m["ldo"], m["c_off"], 127, 127
            if not L.hawq_incep_conv_tile_ok(C.byref(a), t):
                break
        else:
            tiles.append(t)
    return tiles


PARAMS = [pytest.param(name, t, id=f"{name}-tile{t}") for name, (ms, _) in CASES.items() for t in _accepting_tiles(ms)]


def test_the_cases_reach_every_tile():
    by_case = {name: [p.values[1] for p in PARAMS if p.values[0] == name] for name in CASES}
    assert all(3 in ts and len(ts) >= 2 for ts in by_case.values())
    assert by_case["level_17"] == [1, 2, 3, 4] and by_case["pair_8"] == [1, 2, 3, 4]
    assert by_case["mixed_pixels"] == by_case["mixed_channel_blocks"] == by_case["concat_level"] == [2, 3]


def _dyadic(v, m, e):
    """round_half_even(v * m / 2^e) in exact integers (the rounding of fixedpoint_fn's requant, quant_utils.py:404-408)."""
    v, m = v.astype(np.int64), np.broadcast_to(np.asarray(m, np.int64), v.shape)
    t = v * m
    half = np.int64(1) << (e - 1)
    q = (t + half) >> e
    tie = ((t + half) & ((np.int64(1) << e) - 1)) == 0
    return np.where(tie, q & ~np.int64(1), q)


def _out_hw(g):
    KH, KW, ph, pw, stride, H, W = g[:7]
    return (H + 2 * ph - KH) // stride + 1, (W + 2 * pw - KW) // stride + 1


@functools.lru_cache(maxsize=None)
def _operands(name, N):
    """per member (x, w, b, m, ek, clamp, m2, ek2, clamp2) on the host, made once per (case, N) and never changed"""
    from hawq_amd.quant_utils import requant_table
    members, _ = CASES[name]
    gen = torch.Generator().manual_seed(1000 * N + len(name) + sum(sum(m["g"]) for m in members))
    xs, ops = {}, []
    for i, mb in enumerate(members):
        KH, KW, ph, pw, stride, H, W, Cin, Cout = mb["g"]
        key = mb["x"] or f"x{i}"
        if key not in xs:
            xs[key] = torch.randint(-128, 128, (N, H, W, Cin), generator=gen, dtype=torch.int8)
        w = torch.randint(-128, 128, (Cout, KH, KW, Cin), generator=gen, dtype=torch.int8)
        b = torch.randint(-2 ** 20, 2 ** 20, (Cout,), generator=gen, dtype=torch.int32)
        bits = mb["out_bits"] if mb["epilogue"] != RAW else 8
        s_w = torch.rand(Cout, generator=gen) * 1e-3 + 1e-4
        # acc + bias is about sqrt(K 74^4 + 2^40 / 3): an output scale that spreads it over the store, some of it into the clamp
        s_out = torch.tensor([0.02 * 6e-4 * (KH * KW * Cin * 5476. ** 2 + 2. ** 40 / 3) ** 0.5 * 2.5 / 2 ** (bits - 1)])
        m, ek = requant_table(torch.tensor([0.02]), s_w, s_out, lift=False)
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        ops.append((xs[key], w, b, m, ek, (lo, hi), 5 << 27, 31, (lo // 2, hi // 2)))   # second requant: ratio 5/16, with ties
    return ops


def _buffers(name, N):
    """sentinel-filled output buffers of a case, by name (the slices of one buffer share a name)"""
    members, _ = CASES[name]
    bufs = {}
    for i, mb in enumerate(members):
        key = mb["out"] or f"out{i}"
        Ho, Wo = _out_hw(mb["g"])
        dt = {8: torch.int8, 16: torch.int16, 32: torch.int32}[mb["out_bits"]]
        if key not in bufs:
            bufs[key] = torch.full((N * Ho * Wo * mb["ldo"],), SENTINEL, dtype=dt, device="cuda")
    return bufs


def _args(name, N, dev, bufs):
    members, _ = CASES[name]
    out = []
    for i, (mb, (x, w, b, m, ek, q, m2, ek2, q2)) in enumerate(zip(members, dev)):
        KH, KW, ph, pw, stride, H, W, Cin, Cout = mb["g"]
        a = _lib().IncepConvArgs()
        a.in_, a.wgt, a.bias, a.m, a.ek = x.data_ptr(), w.data_ptr(), b.data_ptr(), m.data_ptr(), ek.data_ptr()
        a.out = bufs[mb["out"] or f"out{i}"].data_ptr()
        a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad_h, a.pad_w = N, H, W, Cin, Cout, KH, KW, stride, ph, pw
        a.epilogue, a.relu, a.out_bits, a.ldo, a.c_off = mb["epilogue"], 1, mb["out_bits"], mb["ldo"], mb["c_off"]
        if mb["epilogue"] != RAW:
            a.q_lo, a.q_hi = q
        if mb["epilogue"] == RQ2:
            a.m2, a.ek2, (a.q2_lo, a.q2_hi) = m2, ek2, q2
        out.append(a)
    return out


def _group(args):
    g = _lib().IncepGroupArgs()
    g.n = len(args)
    for i, a in enumerate(args):
        g.conv[i] = a
    return g


def _to_device(ops):
    seen = {}
    dev = []
    for x, w, b, m, ek, q, m2, ek2, q2 in ops:
        if id(x) not in seen:
            seen[id(x)] = x.cuda()
        dev.append((seen[id(x)], w.cuda(), b.cuda(), torch.from_numpy(m).cuda(), torch.from_numpy(ek).cuda(), q, m2, ek2, q2))
    return dev


def _host(mb, op):
    """what the member writes into its channel slice: int64 [N, Ho, Wo, Cout]"""
    x, w, b, m, ek, (lo, hi), m2, ek2, (lo2, hi2) = op
    g = mb["g"]
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double(), b.double(), g[4], (g[2], g[3]))
    v = y.permute(0, 2, 3, 1).round().long().numpy()   # exact: |sum| << 2^53
    if mb["epilogue"] == RAW:
        return v
    v, e = np.maximum(v, 0), (ek & 0xff).astype(np.int64)
    want = np.clip(np.stack([_dyadic(v[..., c], m[c], e[c]) for c in range(g[8])], -1), lo, hi)
    if mb["epilogue"] == RQ2:
        want = np.clip(_dyadic(want, m2, ek2), lo2, hi2)
    return want


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("name,tile", PARAMS)
def test_group_equals_its_members_one_by_one_and_the_host(name, tile, N):
    L = _lib().load()
    members, checked = CASES[name]
    ops = _operands(name, N)
    dev = _to_device(ops)
    s = torch.cuda.current_stream().cuda_stream
    grouped, single = _buffers(name, N), _buffers(name, N)
    g = _group(_args(name, N, dev, grouped))
    assert L.hawq_incep_conv_group_ok(C.byref(g), tile) == 1
    assert L.hawq_incep_conv_group(C.byref(g), tile, s) == 0, L.hawq_last_error()
    for a in _args(name, N, dev, single):
        assert L.hawq_incep_conv_tiled(C.byref(a), tile, s) == 0, L.hawq_last_error()
    torch.cuda.synchronize()
    for key in grouped:
        assert torch.equal(grouped[key], single[key]), f"buffer {key} differs from the single launches'"
    written = {key: np.zeros(t.numel(), bool) for key, t in grouped.items()}
    for i, mb in enumerate(members):
        key = mb["out"] or f"out{i}"
        Ho, Wo = _out_hw(mb["g"])
        sl = slice(mb["c_off"], mb["c_off"] + mb["g"][8])
        written[key].reshape(N, Ho, Wo, mb["ldo"])[..., sl] = True
        if i in checked:
            got = grouped[key].cpu().numpy().reshape(N, Ho, Wo, mb["ldo"])[..., sl]
            want = _host(mb, ops[i])
            assert np.array_equal(got, want), f"member {i} differs from the host computation"
            assert len(np.unique(want)) > 8   # not all clamped away
    for key, t in grouped.items():   # channels no member owns keep their sentinel
        assert (t.cpu().numpy()[~written[key]] == SENTINEL).all(), key


def test_a_refused_group_is_an_error_and_writes_nothing():
    L = _lib().load()
    name, N = "concat_level", 1
    dev = _to_device(_operands(name, N))
    bufs = _buffers(name, N)
    args = _args(name, N, dev, bufs)
    args[3].c_off = 48   # 48 .. 80 meets member 0's 0 .. 64
    g = _group(args)
    s = torch.cuda.current_stream().cuda_stream
    for tile in (2, 3):
        assert L.hawq_incep_conv_group_ok(C.byref(g), tile) == 0
        assert L.hawq_incep_conv_group(C.byref(g), tile, s) != 0
        assert b"overlapping" in L.hawq_last_error()
    g.n = 0
    assert L.hawq_incep_conv_group(C.byref(g), 3, s) != 0
    g.n = 4
    assert L.hawq_incep_conv_group(C.byref(g), 0, s) != 0 and L.hawq_incep_conv_group(C.byref(g), 5, s) != 0
    torch.cuda.synchronize()
    for key, t in bufs.items():
        assert (t == SENTINEL).all(), key
