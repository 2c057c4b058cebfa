"""The fused stem (`hawq_stem_fused`, `hawq_stem_fused_u8`) computes every conv pixel once per workgroup: a workgroup
stores T = 28 pooled columns x R = 8 pooled rows (two wave groups of 4 rows), the third window column of a pooled pixel
comes from the neighbouring lane and the third window row is carried from one pooled row to the next.  These tests sit
on the seams of that tiling.  Reference: the CPU oracle chain quantize -> conv 7x7/2 -> max-pool(3,2,1) -> dyadic
requant; every comparison is exact equality on both outputs."""
import numpy as np
import pytest
import torch

from tests.guard import guard_arena, out_buf  # noqa: F401  (guard_arena: fixture)
from tests.test_gpu_kernels import dev, lib, odyadic, orc, rand_tables, stream, unpack_q  # noqa: F401  (lib, orc: fixtures)

f32 = np.float32
T, R = 28, 8                                   # pooled columns / rows a workgroup stores
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SCALE = f32(0.0213)
INV = f32(1) / SCALE


def pooled(size):
    return ((size - 1) // 2) // 2 + 1         # conv 7/2 pad 3, then pool 3/2 pad 1


def images(xu8):
    """uint8 NHWC -> the normalised fp32 NCHW tensor, with the float32 operations of `input_quant_lut`."""
    u = torch.from_numpy(xu8).to(torch.float32).div(255)
    v = (u - torch.tensor(MEAN, dtype=torch.float32)) / torch.tensor(STD, dtype=torch.float32)
    return np.ascontiguousarray(v.permute(0, 3, 1, 2).numpy())


def reference(orc, xu8, wt, b, m, e, mq, eq):
    acc = orc.maxpool(orc.conv2d(orc.quantize_f32(images(xu8), SCALE, 8), wt, b, 2, 3), 3, 2, 1)
    r16 = np.maximum(odyadic(orc, acc, m, e, (-32768, 32767)), 0)
    return acc, r16, {8: odyadic(orc, r16, mq, eq, (-128, 127)), 4: odyadic(orc, r16, mq, eq, (0, 15))}


def run_variants(lib, xu8, wt, b, m, e, mq, eq, r16, q_ref, fasts):
    """all of: fp32 / uint8 entry x fast_tables x out_bits 8 / 4 x (both outputs, out_q alone, res_out alone)"""
    from hawq_amd.packing import pack_stem_weight
    from hawq_amd.quant_utils import input_quant_lut
    n, hh, ww, cin = xu8.shape
    hp, wp = r16.shape[2:]
    xd, ud = dev(images(xu8)), dev(xu8)
    lut = dev(input_quant_lut(float(INV), MEAN, STD).numpy())
    wd, bd, md, ed = dev(pack_stem_weight(wt)), dev(b.astype(np.int32)), dev(m), dev(e)
    tail = lambda res, qo, bits, lo, hi, fast: (wd.data_ptr(), bd.data_ptr(), md.data_ptr(), ed.data_ptr(), -32768, 32767,
                                                res.data_ptr() if res is not None else 0, qo.data_ptr() if qo is not None else 0,
                                                bits, int(mq[0]), int(eq[0]), lo, hi, fast, stream())
    for entry in ("f32", "u8"):
        for fast in fasts:
            for bits, (lo, hi) in ((8, (-128, 127)), (4, (0, 15))):
                for want_res, want_q in ((1, 1), (0, 1), (1, 0)):
                    res = out_buf(r16.size, torch.uint16, 0xABCD) if want_res else None
                    qo = out_buf(r16.size * bits // 8, torch.uint8, 0x5A) if want_q else None
                    if entry == "f32":
                        lib.call("hawq_stem_fused", xd.data_ptr(), n, cin, hh, ww, float(INV), -128, 127, *tail(res, qo, bits, lo, hi, fast))
                    else:
                        lib.call("hawq_stem_fused_u8", ud.data_ptr(), lut.data_ptr(), n, cin, hh, ww, *tail(res, qo, bits, lo, hi, fast))
                    tag = (entry, fast, bits, want_res, want_q)
                    if want_res:
                        got = res.cpu().numpy().astype(np.int64).reshape(n, hp, wp, 64).transpose(0, 3, 1, 2)
                        assert np.array_equal(got, r16), tag
                    if want_q:
                        assert np.array_equal(unpack_q(qo, (n, hp, wp, 64), bits), q_ref[bits]), tag


def random_case(orc, shape):
    from hawq_amd.quant_utils import requant_table, tables_are_fast
    n, hh, ww = shape
    rng = np.random.default_rng(1000 * hh + ww)
    xu8 = rng.integers(0, 256, (n, hh, ww, 3)).astype(np.uint8)
    wt = rng.integers(-127, 128, (64, 3, 7, 7)).astype(np.int64)
    b = rng.integers(-30000, 30000, 64).astype(np.int64)
    m, e = rand_tables(rng, 64, 2e-3, 4e-2)
    mq, eq = requant_table(torch.tensor([0.0041 * 0.7]), torch.ones(1), torch.tensor([0.7]))
    acc, r16, q_ref = reference(orc, xu8, wt, b, m, e, mq, eq)
    assert acc.shape[2:] == (pooled(hh), pooled(ww))
    can_fast = tables_are_fast(m, e, int(np.abs(acc).max()).bit_length() + 1) and tables_are_fast(mq, eq, 17)
    return xu8, wt, b, m, e, mq, eq, r16, q_ref, (0, 1) if can_fast else (0,)


# pooled columns T - 1, T, T + 1 (even and odd conv width), 2 T + 1; pooled rows R, R + 1 (even and odd conv height); odd batch
SEAMS = [(3, 4 * R, 4 * (T - 1)), (3, 4 * R + 4, 4 * T), (3, 4 * R, 4 * (T + 1)), (3, 4 * R + 2, 4 * T + 2), (3, 4 * R + 4, 4 * (2 * T + 1))]
# smallest and odd maps: one pooled row, odd Hc / Wc
SMALL = [(1, 7, 7), (1, 9, 46), (2, 46, 38), (1, 35, 51)]


def test_seam_shapes_are_what_they_claim():
    assert [(pooled(h), pooled(w)) for _, h, w in SEAMS] == [(R, T - 1), (R + 1, T), (R, T + 1), (R + 1, T + 1), (R + 1, 2 * T + 1)]
    assert ((4 * R + 2 - 1) // 2 + 1) % 2 == 1 and ((4 * T + 2 - 1) // 2 + 1) % 2 == 1      # the fourth has odd Hc and Wc
    assert [(pooled(h), pooled(w)) for _, h, w in SMALL] == [(2, 2), (3, 12), (12, 10), (9, 13)]


@pytest.mark.gpu
@pytest.mark.usefixtures("guard_arena")
@pytest.mark.parametrize("shape", SEAMS + SMALL)
def test_stem_tile_seams_and_small_maps(lib, orc, shape):
    xu8, wt, b, m, e, mq, eq, r16, q_ref, fasts = random_case(orc, shape)
    assert fasts == (0, 1), "these tables were chosen to satisfy the fast contract"
    run_variants(lib, xu8, wt, b, m, e, mq, eq, r16, q_ref, fasts)


# ---- directed neighbour ownership: one bright pixel per image, centre-tap weights, zero bias
DH, DW = 4 * R + 4, 4 * (T + 1)               # Hc 18, Wc 58, pooled 9 x 29: column seam 27|28, row seams 3|4 (waves) and 7|8 (workgroups)
D_ROWS = [0, 1, 6, 7, 8, 9, 14, 15, 16, 17]   # conv rows at the image border and on both sides of the row seams
D_COLS = [0, 1, 53, 54, 55, 56, 57]           # conv columns at the image border and on both sides of the column seam
_directed = {}


def directed_case(orc):
    if not _directed:
        from hawq_amd.quant_utils import requant_table, tables_are_fast
        pos = [(cy, cx) for cy in D_ROWS for cx in D_COLS]
        xu8 = np.zeros((len(pos), DH, DW, 3), np.uint8)          # u = 0: strongly negative after Normalize
        for i, (cy, cx) in enumerate(pos):
            xu8[i, 2 * cy, 2 * cx, 0] = 255                      # the centre tap of conv pixel (cy, cx)
        wt = np.zeros((64, 3, 7, 7), np.int64)
        wt[:, 0, 3, 3] = 1 + np.arange(64) % 127
        b = np.zeros(64, np.int64)
        m, e = rand_tables(np.random.default_rng(5), 64, 0.2, 0.9)
        mq, eq = requant_table(torch.tensor([0.0041 * 0.7]), torch.ones(1), torch.tensor([0.7]))
        conv = orc.conv2d(orc.quantize_f32(images(xu8), SCALE, 8), wt, b, 2, 3)
        ref = reference(orc, xu8, wt, b, m, e, mq, eq)
        can_fast = tables_are_fast(m, e, int(np.abs(ref[0]).max()).bit_length() + 1) and tables_are_fast(mq, eq, 17)
        _directed.update(pos=pos, xu8=xu8, wt=wt, b=b, m=m, e=e, mq=mq, eq=eq, conv=conv, ref=ref, fasts=(0, 1) if can_fast else (0,))
    return _directed


def test_directed_cases_put_the_maximum_on_neighbour_owned_positions(orc):
    """CPU only: the sweep is worth something only if, on each side of each seam, some image's pooled maximum comes from the
    window position another lane (third column) or the carried row (third row) supplies."""
    d = directed_case(orc)
    conv, acc = d["conv"], d["ref"][0]
    bright = conv[:, 0].max()
    assert bright > 0 and (np.sort(conv[:, 0].reshape(len(d["pos"]), -1), axis=1)[:, -2] < 0).all()   # one positive conv pixel per image
    for i, (cy, cx) in enumerate(d["pos"]):                      # exactly the pooled pixels whose window holds (cy, cx) carry it
        hit = np.zeros(acc.shape[2:], bool)
        hit[np.ix_([py for py in range(hit.shape[0]) if abs(2 * py - cy) <= 1], [px for px in range(hit.shape[1]) if abs(2 * px - cx) <= 1])] = True
        assert np.array_equal(acc[i, 0] == bright, hit), (cy, cx)
    third_col = {px for (cy, cx) in d["pos"] for px in [(cx - 1) // 2] if cx % 2 == 1 and px < pooled(DW)}   # cx = 2 px + 1
    third_row = {py for (cy, cx) in d["pos"] for py in [(cy - 1) // 2] if cy % 2 == 1 and py < pooled(DH)}
    assert {T - 1, T} <= third_col                               # last stored lane (fed by the halo lane) and first lane of the next tile
    assert {3, 4, R - 1, R} <= third_row                         # both sides of the wave seam and of the workgroup seam


@pytest.mark.gpu
@pytest.mark.usefixtures("guard_arena")
def test_stem_directed_neighbour_ownership(lib, orc):
    d = directed_case(orc)
    acc, r16, q_ref = d["ref"]
    assert (r16[:, 0] > 0).sum() == (acc[:, 0] == d["conv"][:, 0].max()).sum()   # the bright value survives the requant, nothing else does
    run_variants(lib, d["xu8"], d["wt"], d["b"], d["m"], d["e"], d["mq"], d["eq"], r16, q_ref, d["fasts"])
