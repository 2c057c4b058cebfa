"""The shape corners of the check contract: for every launcher whose check (``*_applies``, ``*_ok``, ``*_refusal``) computes a
capacity, one Python restatement of that rule, written from the comments and headers of hawq_amd/csrc, and the case list that
follows from it - for a rule in one variable both ends of every maximal accepted run and the first refused neighbour on each side.

Nothing here calls the library: tests/test_contract_edges_host.py holds the restatements against the built library's queries
(no device), tests/test_gpu_contract_edges.py launches the accepted ends and asks the refused neighbours for their error.

Rules restated
  band_v1 / band_persist  a workgroup of bm consecutive pixels keeps their image rows, one row more when the tile starts inside a
                          row, and a halo row above and below, each with a zero column left and right, in one LDS stage whose last
                          four pixels are the zeros:  (ceil(bm / W) + 3) * (W + 2) <= band_px - 4
  band_v2                 pixels m0 - W - 1 .. m0 + bm + W with the start rounded down to eight: bm + 2 W + 9 <= band_px - 4
  band_v2, out_sub = s    the source pixels between the windows of a tile's first and last output; every tile of the launch must fit
  band_persist            float-reciprocal pixel division: N H W < 2^23
  incep_stem_f32          column chunks of 159 outputs (2 * 159 + 1 <= 320 input columns per tile row)
  hawq_linear_bottleneck  more than 96 channels in or out: output maps of at most 8 x 8 pixels
  global average pool     bound * H W <= (2^31 - 1 - H W) / 100, bound = 2^(in_bits - 1) or max(hi1, -lo1) + 1 with a pre requant
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

WIDTHS = range(1, 97)   # the widths the host test asks every band tile about

# ---------------------------------------------------------------------------------------------- band_v1 / band_persist
# the 3x3 band tiles in tile-id order: band_v1's B0 .. B5, then the weight-stationary kernel at 1 / 2 workgroups per CU
BandTile = namedtuple("BandTile", "name bm bn band_px one_slice persist")
BAND_TILES = (BandTile("B0", 256, 64, 512, True, False), BandTile("B1", 256, 128, 512, False, False),
              BandTile("B2", 128, 128, 256, False, False), BandTile("B3", 256, 128, 384, False, False),
              BandTile("B4", 128, 128, 256, False, False), BandTile("B5", 128, 64, 256, False, False),
              BandTile("WS1", 256, 64, 512, True, True), BandTile("WS2", 256, 64, 512, True, True))


def band_used(bm, w):
    """band pixels a tile of bm pixels needs on a map w wide (rows it touches + the unaligned start + two halo rows, w + 2 each)"""
    return (-(-bm // w) + 3) * (w + 2)


def band_fits(bm, band_px, w):
    return band_used(bm, w) <= band_px - 4


def band_takes(t: BandTile, w, cin, cout, bits=8):
    """REQUANT to 8 bits or 16-bit RESIDUAL with fast tables, dense rows - does band tile `t` take the layer?"""
    slices = cin // 64 if bits == 8 else cin // 128
    if t.persist:
        return bits == 8 and cin == 64 and cout == 64 and band_fits(t.bm, t.band_px, w)
    return (cout % t.bn == 0 and (bits == 8 or cin % 128 == 0) and (slices == 1 or not t.one_slice) and band_fits(t.bm, t.band_px, w))


def band_takers(w, cin, cout, bits=8):
    """indices into BAND_TILES"""
    return [i for i, t in enumerate(BAND_TILES) if band_takes(t, w, cin, cout, bits)]


def runs(accepts, values=WIDTHS):
    """maximal runs [(first, last), ..] of consecutive values with accepts(v)"""
    out = []
    for v in values:
        if accepts(v):
            if out and out[-1][1] == v - 1:
                out[-1][1] = v
            else:
                out.append([v, v])
    return [tuple(r) for r in out]


def run_ends(rs):
    return sorted({v for r in rs for v in r})


def first_refused(rs, lowest=1):
    """the neighbours of every run that no run holds"""
    held = {v for a, b in rs for v in range(a, b + 1)}
    return sorted({v for a, b in rs for v in (a - 1, b + 1) if v >= lowest and v not in held})


# the runs as the issue's table pins them: a change of a tile's LDS geometry shows up here
BAND_RUNS = {"B0": [(3, 61), (64, 70)], "B1": [(3, 61), (64, 70)], "WS1": [(3, 61), (64, 70)], "WS2": [(3, 61), (64, 70)],
             "B2": [(3, 29), (32, 34)], "B4": [(3, 29), (32, 34)], "B5": [(3, 29), (32, 34)],
             "B3": [(6, 27), (29, 29), (32, 32)]}
# the first refused neighbours of those runs, and the widths 1 and 2 (both side taps outside the image) for every geometry
BAND_REFUSED = {"B0": [1, 2, 62, 63, 71], "B2": [1, 2, 30, 31, 35], "B3": [1, 2, 5, 28, 30, 31, 33]}
BAND_WIDTHS = sorted({v for rs in BAND_RUNS.values() for v in run_ends(rs)})             # every width at which some tile's run ends
BAND_REFUSED_WIDTHS = sorted({v for vs in BAND_REFUSED.values() for v in vs})


def band_runs(t: BandTile):
    return runs(lambda w: band_fits(t.bm, t.band_px, w))


def band_slack(t: BandTile, w):
    return t.band_px - 4 - band_used(t.bm, w)


# ---------------------------------------------------------------------------------------------- band_v2
Band2Tile = namedtuple("Band2Tile", "name bm band_px sub_bm sub_band_px")
BAND2_TILES = (Band2Tile("V128", 128, 256, 128, 768), Band2Tile("V256", 256, 384, 64, 512))
BAND2_RUNS = [(1, 57)]


def band2_used(bm, w):
    return bm + 2 * w + 2 + 7


def band2_fits(t: Band2Tile, w):
    return band2_used(t.bm, w) <= t.band_px - 4


def sub_grid(n, s=2):
    return (n - 1) // s + 1


def band2_sub_worst(n, h, w, bm, s=2):
    """the longest band any pixel tile of the strided launch needs: from the top-left tap of its first output's window, rounded down
    to eight pixels, to the bottom-right tap of its last output's window, on the source map [n][h][w]"""
    ho, wo = sub_grid(h, s), sub_grid(w, s)
    m_out = n * ho * wo

    def src(m):
        i, r = divmod(m, ho * wo)
        y, x = divmod(r, wo)
        return (i * h + s * y) * w + s * x
    worst = 0
    for m0 in range(0, m_out, bm):
        first = (src(m0) - w - 1) & ~7
        last = src(min(m0 + bm, m_out) - 1) + w + 1
        worst = max(worst, last - first + 1)
    return worst


def band2_sub_fits(t: Band2Tile, n, h, w, s=2):
    return band2_sub_worst(n, h, w, t.sub_bm, s) <= t.sub_band_px - 4


SUB_N, SUB_H, SUB_SEARCH = 2, 9, range(1, 513)   # the strided twins' widest source width is looked for on a [2][9][W] map
SUB_WIDEST = {"V128": 128, "V256": 128}          # pinned: 65 output columns would put a further source row into a tile's band


def band2_sub_widest(t: Band2Tile, n=SUB_N, h=SUB_H):
    return max(w for w in SUB_SEARCH if band2_sub_fits(t, n, h, w))


# ---------------------------------------------------------------------------------------------- band_persist's pixel count
PERSIST_PIXELS = 1 << 23   # floor(m / d) from a float reciprocal is corrected for 0 <= m < 2^23


def fdiv_f32(m, d):
    """band_persist's fdiv in numpy binary32 (the library builds without fast-math and without contraction, so these are the
    same operations): truncate m * (1 / d), then the two corrections"""
    m = np.asarray(m, np.int64)
    r = np.float32(1.0) / np.float32(d)
    g = (m.astype(np.float32) * r).astype(np.int64)
    g = g - (g * d > m)
    g = g + ((g + 1) * d <= m)
    return g


# ---------------------------------------------------------------------------------------------- shapes that reach the seams
def seam_height(w, n=2, bms=(128, 256)):
    """The smallest H >= 3 at which an [n][H][w] launch has, for every pixel tile size of `bms`, at least two full tiles and a ragged
    one, and a tile that straddles the boundary between two images."""
    for h in range(3, 2048):
        if all(tile_facts(n, h, w, bm) for bm in bms):
            return h
    raise ValueError(f"no height reaches the seams at width {w} for tiles of {bms} pixels")


def band_seam_height(w):
    """seam_height for the pixel tiles of the band tiles that take a map `w` wide (a 64-wide map of two images is a multiple of 128
    pixels at every height, and only 256-pixel tiles take it)"""
    return seam_height(w, bms=tuple(sorted({t.bm for t in BAND_TILES if band_fits(t.bm, t.band_px, w)})))


def tile_facts(n, h, w, bm):
    m = n * h * w
    return m // bm >= 2 and m % bm != 0 and n >= 2 and (h * w) % bm != 0


# ---------------------------------------------------------------------------------------------- incep_stem_f32
STEM_CW = (320 - 1) // 2   # output columns per workgroup: 2 CW + 1 input columns in five 64-lane loads


def stem_chunks(w):
    """(output columns, column chunks, width of the last chunk)"""
    wo = (w - 3) // 2 + 1
    n = -(-wo // STEM_CW)
    return wo, n, wo - (n - 1) * STEM_CW


# (N, H, W) -> (chunks, last chunk): one full chunk; 159 + 1; 159 + 2; two full chunks; two full chunks + 1
STEM_SHAPES = {(1, 11, 319): (1, 159), (2, 9, 321): (2, 1), (1, 9, 323): (2, 2), (1, 9, 637): (2, 159), (1, 9, 639): (3, 1)}

# ---------------------------------------------------------------------------------------------- wide linear-bottleneck units
LB_WIDE_MAX = 8   # output rows and columns of a unit with more than 96 channels in or out


def lb_wide_takes(h, w, stride):
    return (h - 1) // stride + 1 <= LB_WIDE_MAX and (w - 1) // stride + 1 <= LB_WIDE_MAX


# cin, in_pitch, hidden, cout, out_pitch, stride, identity, (n, h, w), small hidden-side weights: the rows of
# tests/test_gpu_mbv2_kernels.py::UNITS that end on an 8 x 8 map
LB_WIDE_UNITS = [(160, 160, 960, 160, 160, 1, True, (2, 8, 8), False),
                 (160, 160, 960, 320, 320, 1, False, (1, 8, 8), False),
                 (96, 96, 576, 160, 160, 2, False, (2, 15, 16), False),
                 (96, 96, 576, 160, 160, 2, False, (1, 16, 16), False)]
# (cin = in_pitch, cout = out_pitch, stride, (h, w)) the check refuses: one row or one column more than 8 x 8
LB_WIDE_REFUSED = [(160, 160, 1, (9, 8)), (160, 160, 1, (8, 9)), (160, 320, 1, (9, 8)), (160, 320, 1, (8, 9)), (96, 160, 2, (17, 16)), (96, 160, 2, (16, 17))]

def bottleneck_args(cin, cout, stride, nhw, ptr=16):
    """A hawq_bottleneck_args block the check takes up to its geometry rules (six times expanded hidden width, the 16-bit clamp, no
    identity); cin / cout are the stored pitches.  Pointers are dummies unless the caller sets real ones."""
    from hawq_amd import _lib
    n, h, w = nhw
    pad64 = lambda c: (c + 63) // 64 * 64   # noqa: E731
    b = _lib.BottleneckArgs()
    e, q = b.expand, b.project
    hid = 6 * cin
    e.in_, e.wgt, e.ctab, q.wgt, q.ctab, b.dw_wgt9c, b.dw_ctab = (ptr,) * 7
    e.N, e.H, e.W, e.Cin, e.Cout, e.KH, e.KW, e.stride, e.pad, e.in_bits, e.w_bits = n, h, w, pad64(cin), pad64(hid), 1, 1, 1, 0, 8, 8
    e.in_pitch = cin if cin != pad64(cin) else 0
    e.epilogue, e.relu, e.q_lo, e.q_hi, e.out_bits, e.fast_tables = _lib.EPI_REQUANT, 1, 0, 127, 8, 1
    b.dw_stride, b.dw_q_lo, b.dw_q_hi, b.dw_fast_tables, b.c_mid, b.tile = stride, 0, 100, 1, hid, 0
    q.N, q.H, q.W = n, (h - 1) // stride + 1, (w - 1) // stride + 1
    q.Cin, q.Cout, q.KH, q.KW, q.stride, q.pad, q.in_bits, q.w_bits = pad64(hid), pad64(cout), 1, 1, 1, 0, 8, 8
    q.out_pitch = cout if cout != pad64(cout) else 0
    q.epilogue, q.res_no_relu, q.res_clamp16, q.fast_tables = _lib.EPI_RESIDUAL, 1, 1, 1
    q.res_out, q.res_out_bits, q.out_q, q.out_bits, q.q_lo, q.q_hi, q.mq, q.eq = ptr, 32, ptr, 8, -128, 127, 3, 34
    return b


# ---------------------------------------------------------------------------------------------- global average pool
INT32_MAX = (1 << 31) - 1


def pool_bound(in_bits, pre_clamp=None):
    """bound of a summand: 2^(in_bits - 1), or max(hi1, -lo1) + 1 behind a pre requant"""
    if pre_clamp is None:
        return 1 << (in_bits - 1)
    lo, hi = pre_clamp
    return max(hi, -lo) + 1


def pool_global_takes(hw, in_bits, pre_clamp=None):
    """100 * sum + H W fits int32 for every input the summand bound admits"""
    return hw < (1 << 31) and pool_bound(in_bits, pre_clamp) * hw <= (INT32_MAX - hw) // 100


def pool_global_max_hw(in_bits, pre_clamp=None):
    lo, hi = 1, 1 << 31
    while hi - lo > 1:   # the rule is monotone in H W
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pool_global_takes(mid, in_bits, pre_clamp) else (lo, mid)
    return lo


def pool_shape(hw, max_w=1024):
    """(H, W) with H * W == hw, H >= 2 and the largest W <= max_w that divides it"""
    w = max(d for d in range(1, min(max_w, hw - 1) + 1) if hw % d == 0)
    return hw // w, w


POOL_PRE = (3 << 28, 30, -2048, 2047)   # ratio 3/4 and a clamp that every 16-bit extreme reaches: summand bound 2049
# name -> (in_bits, pre table or None, largest H W the check takes), pinned: 16 bits is the issue's 5 x 131
POOL_BOUNDS = {"int16": (16, None, 655), "int8": (8, None, 167759), "pre_clamp": (16, POOL_PRE, 10480)}


def trunc_avg(s, hw):
    """the pool's average in Python integers: (100 s + hw) / (100 hw), truncated toward zero as C divides"""
    num, den = 100 * int(s) + hw, 100 * hw
    return num // den if num >= 0 else -((-num) // den)
