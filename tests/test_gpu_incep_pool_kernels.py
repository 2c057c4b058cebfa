"""The vectorised pool / requant kernels (hawq_amd/csrc/incep_pool.hip, ``hawq_incep_pool_v``) against the entry points they stand
for (hawq_amd/csrc/inception.hip) and against brute-force host maths: the same input into two sentinel-filled outputs, both equal to
numpy inside the slice, equal to each other over the whole buffer.

Shapes follow the kernels' own work split: a lane owns 16 channels; REQUANT is flat (256 lanes per block); MAX3S2 cuts an output row
of Wo * C / 16 lanes into blocks of 64 .. 256; AVG3 works on tiles of whole rows (W <= 40, else 32 columns) x TH rows x 32 channels, where TH is what
32 KB of LDS hold, halved while the launch has fewer than 512 workgroups - so it depends on N and C: the small cases get tiles of 1 to
6 rows (one pass of the 256 threads over the outputs), the ``avgpool_tall_*`` cases have enough workgroups to keep the tiles of the
batch-128 plan (9 x 35 and 17 x 17 pixels x 2 groups = 630 and 578 output lanes, three passes).  AVG3_TILES pins the tile of every
average-pool case to what ``hawq_incep_pool_v_avg3_tile`` reports.  GLOBAL works on 64-channel chunks with 64 pixel lanes."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OLD = {"requant": "hawq_incep_requant", "maxpool": "hawq_incep_maxpool3s2", "avgpool": "hawq_incep_avgpool_branch",
       "global": "hawq_incep_global_avgpool"}
OPS = {"requant": 0, "maxpool": 1, "avgpool": 2, "global": 3}
PRE = (3 << 28, 30, -32768, 32767)                 # ratio 3/4, ties at 2 mod 4
POST8 = (5 << 27, 33, -128, 127)                   # ratio 5/64 to 8 bits
POST16 = (1 << 30, 31, -20000, 20000)              # ratio 1/2, every odd value a tie
SENTINEL = -3


def _dyadic(v, m, e):
    """round_half_even(v * m / 2^e) in exact integers"""
    t = v.astype(np.int64) * np.int64(m)
    half = np.int64(1) << (e - 1)
    q = (t + half) >> e
    tie = ((t + half) & ((np.int64(1) << e) - 1)) == 0
    return np.where(tie, q & ~np.int64(1), q)


def _rq(v, t):
    m, ek, lo, hi = t
    return np.clip(_dyadic(v, m, ek & 0xff), lo, hi)


def _trunc_avg(s, d):
    num = 100 * s + d
    return np.where(num >= 0, num // (100 * d), -((-num) // (100 * d)))


def _brute_force(op, v, pre_t, post_t):
    N, H, W, _ = v.shape
    if pre_t:
        v = _rq(v, pre_t)
    if op == "requant":
        r = v
    elif op == "maxpool":
        Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        r = np.max(np.stack([v[:, dy:dy + 2 * Ho - 1:2, dx:dx + 2 * Wo - 1:2] for dy in range(3) for dx in range(3)]), 0)
    elif op == "avgpool":
        p = np.pad(v, ((0, 0), (1, 1), (1, 1), (0, 0)))
        s = sum(p[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))
        r = _trunc_avg(s, 9)
    else:
        r = _trunc_avg(v.sum((1, 2), keepdims=True), H * W)
    return _rq(r, post_t) if post_t else r


def _check(op, N, H, W, Cc, in_bits, out_bits, pre_t, post_t, ldo=None, c_off=0, in_pitch=None, in_off=0, seed=0, negative=False,
           tile=None):
    from hawq_amd import _lib as L
    in_pitch, ldo = (Cc if in_pitch is None else in_pitch), (Cc if ldo is None else ldo)
    lim = 1 << (in_bits - 1)
    gen = np.random.default_rng(seed)
    xf = gen.integers(-lim, (-lim // 8 if negative else lim), (N, H, W, in_pitch)).astype(np.int16 if in_bits == 16 else np.int8)
    xf[0, 0, 0, in_off], xf[-1, -1, -1, in_off + Cc - 1] = lim - 1, -lim
    v = xf[..., in_off:in_off + Cc].astype(np.int64)
    if negative and op in ("avgpool", "global"):   # the trunc-toward-zero rule sees negative sums that are no multiple of the divisor
        pv = _rq(v, pre_t) if pre_t else v
        s = pv.sum((1, 2)) if op == "global" else pv[:, :2, :2].sum((1, 2))
        assert (s < 0).sum() > s.size // 2 and (s % (H * W if op == "global" else 9) != 0).any()
    want = _brute_force(op, v, pre_t, post_t)
    Ho, Wo = want.shape[1:3]
    xd = torch.from_numpy(xf).cuda()
    dt = torch.int8 if out_bits == 8 else torch.int16
    outs = [torch.full((N * Ho * Wo * ldo,), SENTINEL, dtype=dt, device="cuda") for _ in range(2)]
    sp = torch.cuda.current_stream().cuda_stream
    for new, out in enumerate(outs):
        a = L.IncepPoolArgs()
        a.in_, a.out = xd.data_ptr(), out.data_ptr()
        a.N, a.H, a.W, a.C, a.in_bits, a.in_pitch, a.in_off = N, H, W, Cc, in_bits, in_pitch, in_off
        a.out_bits, a.ldo, a.c_off = out_bits, ldo, c_off
        if pre_t:
            a.pre, (a.m1, a.ek1, a.lo1, a.hi1) = 1, pre_t
        if post_t:
            a.post, (a.m2, a.ek2, a.lo2, a.hi2) = 1, post_t
        if new:
            assert L.load().hawq_incep_pool_v_ok(C.byref(a), OPS[op]) == 1
            if tile is not None:   # the case runs the tile it was written for
                th, tw = C.c_int32(), C.c_int32()
                L.call("hawq_incep_pool_v_avg3_tile", C.byref(a), C.byref(th), C.byref(tw))
                assert (th.value, tw.value) == tile
            L.call("hawq_incep_pool_v", C.byref(a), OPS[op], sp)
        else:
            L.call(OLD[op], C.byref(a), sp)
    torch.cuda.synchronize()
    for out in outs:
        got = out.cpu().numpy().reshape(N, Ho, Wo, ldo)
        assert np.array_equal(got[..., c_off:c_off + Cc], want)
        assert (got[..., :c_off] == SENTINEL).all() and (got[..., c_off + Cc:] == SENTINEL).all()
    assert torch.equal(outs[0], outs[1])            # the whole buffer: nothing outside the slice was touched
    assert np.abs(want).max() > abs(SENTINEL)       # the slice does not pass for sentinels
    return want


_KIND = {"requant": (8, None, POST8), "maxpool": (16, PRE, POST16), "avgpool": (8, PRE, POST8), "global": (8, None, POST8)}


@pytest.mark.parametrize("op", ["requant", "maxpool", "avgpool", "global"])
@pytest.mark.parametrize("hw", [(5, 4), (7, 5)], ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("channels", [16, 48])
def test_small_odd_maps(op, hw, channels):
    out_bits, pre_t, post_t = _KIND[op]
    _check(op, 2, hw[0], hw[1], channels, 16, out_bits, pre_t, post_t, seed=hw[0] + channels)


@pytest.mark.parametrize("op", ["requant", "maxpool", "avgpool", "global"])
def test_slices_on_both_sides(op):
    """in_off > 0 with in_pitch > C, c_off > 0 with ldo > c_off + C"""
    out_bits, pre_t, post_t = _KIND[op]
    _check(op, 2, 9, 7, 48, 16, out_bits, pre_t, post_t, ldo=96, c_off=32, in_pitch=112, in_off=48, seed=1)


@pytest.mark.parametrize("op", ["avgpool", "global"])
@pytest.mark.parametrize("in_bits", [16, 8])
def test_negative_sums_truncate_toward_zero(op, in_bits):
    lim = 1 << (in_bits - 1)
    pre_t = (3 << 28, 30, -lim, lim - 1) if op == "avgpool" else None
    post_t = (1 << 30, 31, -128, 127) if in_bits == 8 else POST8
    _check(op, 2, 6, 5, 32, in_bits, 8, pre_t, post_t, seed=2, negative=True)


CASES = {
    # more than one block / tile / chunk, none of them full
    "requant_many_blocks": ("requant", 2, 11, 9, 80, 16, 8, None, POST8, dict(ldo=96, c_off=16)),
    "requant_16_16_slice": ("requant", 2, 5, 4, 768, 16, 16, None, POST16, dict(ldo=2048, c_off=1280)),
    "maxpool_row_of_five_blocks": ("maxpool", 2, 7, 13, 768, 16, 16, PRE, POST16, dict(ldo=768 + 32, c_off=16)),
    "maxpool_wide_map": ("maxpool", 2, 9, 181, 48, 16, 16, PRE, POST16, {}),      # 90 x 3 lanes: five blocks of 64
    "maxpool_one_block_of_256": ("maxpool", 2, 5, 33, 256, 16, 16, PRE, POST16, {}),
    "maxpool_one_block_of_128": ("maxpool", 2, 5, 17, 256, 16, 16, PRE, POST16, {}),
    "maxpool_3x3_map": ("maxpool", 2, 3, 3, 96, 16, 16, PRE, POST16, dict(ldo=128, c_off=16)),
    "maxpool_3x4_map": ("maxpool", 2, 3, 4, 64, 8, 8, None, None, {}),
    "maxpool_plain_16": ("maxpool", 2, 7, 5, 192, 16, 16, None, None, {}),
    "avgpool_tiles_in_both_dimensions": ("avgpool", 2, 10, 45, 48, 16, 8, PRE, POST8, dict(ldo=64, c_off=16)),
    "avgpool_two_column_tiles_exactly": ("avgpool", 2, 4, 64, 16, 16, 8, PRE, POST8, {}),
    "avgpool_tiles_of_five_rows": ("avgpool", 2, 20, 5, 2048, 16, 8, PRE, POST8, {}),      # 512 workgroups after two halvings
    "avgpool_whole_map_tiles": ("avgpool", 8, 6, 3, 2048, 16, 8, PRE, POST8, {}),          # 512 workgroups at once: no halving
    # tiles of the batch-128 plan: more than 256 output lanes per workgroup (three passes of the output loop), tap rows up to 18
    "avgpool_tall_9x35_tile": ("avgpool", 16, 9, 35, 1040, 16, 8, PRE, POST8, {}),         # 528 workgroups; last chunk 16 channels
    "avgpool_tall_35x35_map_in_four_tiles": ("avgpool", 4, 35, 35, 1024, 16, 8, PRE, POST8, dict(ldo=1056, c_off=16)),
    "avgpool_tall_17x17_whole_map": ("avgpool", 8, 17, 17, 2048, 16, 8, PRE, POST8, {}),
    "avgpool_one_pixel_map": ("avgpool", 2, 1, 1, 32, 16, 8, PRE, POST8, {}),
    "avgpool_to_16": ("avgpool", 2, 5, 4, 32, 16, 16, PRE, POST16, {}),
    "global_8x8": ("global", 2, 8, 8, 80, 16, 8, None, POST8, dict(ldo=96, c_off=16)),
    "global_non_square": ("global", 2, 9, 8, 192, 16, 8, None, POST8, {}),
    "global_single_image": ("global", 1, 8, 8, 2048, 16, 8, None, POST8, {}),
    "global_with_pre": ("global", 2, 8, 5, 64, 16, 16, PRE, POST16, {}),
    # 8-bit input
    "in8_avgpool": ("avgpool", 2, 6, 9, 80, 8, 8, (3 << 28, 30, -128, 127), (1 << 30, 31, -128, 127), {}),
    "in8_requant_to_16": ("requant", 3, 5, 3, 32, 8, 16, None, (5 << 28, 28, -32768, 32767), dict(ldo=64, c_off=16, in_pitch=48, in_off=16)),
    "in8_requant_widening_without_post": ("requant", 2, 5, 3, 32, 8, 16, None, None, {}),
    "in8_global": ("global", 2, 8, 5, 64, 8, 8, None, (1 << 30, 29, -128, 127), {}),
    "in8_maxpool_with_requants": ("maxpool", 2, 7, 5, 48, 8, 8, (3 << 28, 30, -128, 127), (1 << 30, 31, -128, 127), {}),
}


# (TH, TW) of every average-pool case above, as hawq_incep_pool_v_avg3_tile must report it
AVG3_TILES = {
    "avgpool_tiles_in_both_dimensions": (3, 32), "avgpool_two_column_tiles_exactly": (4, 32), "avgpool_tiles_of_five_rows": (5, 5),
    "avgpool_whole_map_tiles": (6, 3), "avgpool_tall_9x35_tile": (9, 35), "avgpool_tall_35x35_map_in_four_tiles": (9, 35),
    "avgpool_tall_17x17_whole_map": (17, 17), "avgpool_one_pixel_map": (1, 1), "avgpool_to_16": (3, 4), "in8_avgpool": (3, 9),
}


def test_the_tall_tile_cases_loop_over_their_outputs():
    """what the tall cases are for: more output lanes per workgroup (TH TW 16-channel group pairs) than its 256 threads, and more
    staged pixels than that too; and every average-pool case has a pinned tile"""
    assert {c for c, v in CASES.items() if v[0] == "avgpool"} == set(AVG3_TILES)
    tall = {c: t for c, t in AVG3_TILES.items() if c.startswith("avgpool_tall_")}
    assert len(tall) == 3 and all(th * tw * 2 > 2 * 256 and th > 8 for th, tw in tall.values())
    assert all(th * tw * 2 <= 256 for c, (th, tw) in AVG3_TILES.items() if c not in tall)


@pytest.mark.parametrize("case", sorted(CASES))
def test_edges(case):
    op, N, H, W, Cc, in_bits, out_bits, pre_t, post_t, kw = CASES[case]
    want = _check(op, N, H, W, Cc, in_bits, out_bits, pre_t, post_t, seed=len(case), tile=AVG3_TILES.get(case), **kw)
    if case in ("maxpool_3x3_map", "maxpool_3x4_map"):
        assert want.shape[1:3] == (1, 1)


def _pools(eng):
    """(op index, argument block, op id) of every pool / requant launch, read from the engine's launch records"""
    return [(eng._at[r], r.args[0], r.ref) for r in eng._launches if r.kind == "pool"]


def test_every_pool_launch_of_the_shipped_networks_is_taken_and_equal():
    """An engine with fast_pools=True for both schedules: every one of its pool / requant launches goes to hawq_incep_pool_v (none
    stays silently on the old kernel), and every distinct description among them, at a small H != W map, equals brute force."""
    from hawq_amd.api import build_quantized_resnet
    from hawq_amd.engine_inception import InceptionEngine
    from hawq_amd.quant_modules import QuantAct, freeze_model
    names = {v: k for k, v in OPS.items()}
    descs = set()
    for scheme in ("uniform8", "uniform4"):
        model = build_quantized_resnet("inceptionv3", scheme, seed=0).cuda()
        for m in model.modules():
            if isinstance(m, QuantAct):
                m.x_min.fill_(-1.0 if m.quant_mode == "symmetric" else 0.0), m.x_max.fill_(1.0)
                m.compute_scale()
        freeze_model(model)
        eng = InceptionEngine(model, fast_pools=True)
        eng._build(1, 299, 299)   # the plan only: nothing is launched
        assert len(eng.pool_launches) == 49 == eng.n_launches - 95 - 3
        assert all(n == "hawq_incep_pool_v" for n, _ in eng.pool_launches), eng.pool_launches
        for (idx, a, op), (_, op2) in zip(_pools(eng), eng.pool_launches):
            assert op == op2 and eng._ops[idx].args[2] == op
            assert a.in_pitch == a.C and a.in_off == 0
            descs.add((names[op], a.in_bits, a.out_bits, bool(a.pre), bool(a.post), a.C, a.ldo, a.c_off))
    assert {d[0] for d in descs} == set(OPS) and {288, 768, 1280, 2048} <= {d[5] for d in descs}
    for i, (op, in_bits, out_bits, pre, post, Cc, ldo, c_off) in enumerate(sorted(descs)):
        H, W = {"requant": (5, 4), "maxpool": (7, 5), "avgpool": (5, 4), "global": (8, 7)}[op]
        post_t = (POST8 if out_bits == 8 else POST16) if post else None
        _check(op, 2, H, W, Cc, in_bits, out_bits, PRE if pre else None, post_t, ldo=ldo, c_off=c_off, seed=100 + i)
