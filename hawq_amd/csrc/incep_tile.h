// What the three files of the LDS-tiled InceptionV3 conv share (incep_tiled.hip: one conv per launch, incep_group.hip: up to eight
// on one grid, incep_fan.hip: the grouped launch with a fan-out epilogue):
//   the tile table and the one place that names each tile's template constants (for_tile)
//   the workgroup body, in incep_tile_body.h
//   the grouped launches' grid: GroupMap, the workgroup's member (group_member), the host's layout of it (group_grid)
//
// The body is shared as text: each kernel file includes incep_tile_body.h inside its own function template, so every translation
// unit compiles the token stream it would compile with the body written out, and no kernel's code depends on the sharing.  As one
// `__forceinline__` function template with a callable for the fan, called from all three kernels, it is the same source but not the
// same code for incep_tiled_kernel: 104 / 104 / 70 / 85 VGPRs for tiles 1 - 4 with the argument block by reference and 104 / 104 /
// 76 / 91 by value, against 102 / 102 / 74 / 90 with the body in the kernel - same occupancy, no scratch, another instruction stream
// (DESIGN.md 10).
#pragma once
#include "common.h"

extern "C" int hawq_incep_conv_tile_ok(const hawq_incep_conv_args *a, int tile);

namespace {

// tile ids 1 .. NUM_TILES (id 0 is hawq_incep_conv's kernel, 64 px x 64 ch, inception.hip): BM pixels x BN channels per workgroup
//   1  128 px x 128 ch, 4 waves of 64 x 64   the 147^2 .. 35^2 maps with 96 and more output channels
//   2  256 px x  64 ch, 4 waves of 64 x 64   the large maps with 32 .. 64 output channels (and 80 / 192 in two passes)
//   3  128 px x  64 ch, 4 waves of 64 x 32   the 17^2 maps
//   4   64 px x  32 ch, 2 waves of 64 x 32 that split K: the 8 x 8 maps at batch 1 - 16 (one image = one pixel tile, twice the
//      workgroups of a 64-channel tile)
enum { NUM_TILES = 4 };
struct TileShape {
    int bm, bn;
};
constexpr TileShape kTiles[NUM_TILES + 1] = {{64, 64}, {128, 128}, {256, 64}, {128, 64}, {64, 32}};

// the template constants of tile ID: WPX x WCH waves tile the BM x BN block, each with (BM / WPX / 32) x (BN / WCH / 32) MFMA tiles;
// KS = 2: two such wave sets split every K step between them (32 bytes each) and add their accumulators through LDS at the end
template <int ID, int BM_, int BN_, int WPX_, int WCH_, int KS_>
struct Tile {
    static_assert(ID >= 1 && ID <= NUM_TILES && kTiles[ID].bm == BM_ && kTiles[ID].bn == BN_, "kTiles and the dispatch name one shape");
    static constexpr int BM = BM_, BN = BN_, WPX = WPX_, WCH = WCH_, KS = KS_, NT = 64 * WPX_ * WCH_ * KS_;
};

// f(Tile<...>()) for tile id `tile` in 1 .. NUM_TILES
template <class F>
void for_tile(int tile, F &&f) {
    switch (tile) {
        case 1: f(Tile<1, 128, 128, 2, 2, 1>()); break;
        case 2: f(Tile<2, 256, 64, 4, 1, 1>()); break;
        case 3: f(Tile<3, 128, 64, 2, 2, 1>()); break;
        default: f(Tile<4, 64, 32, 1, 1, 2>()); break;
    }
}

// ---- the grid of a grouped launch --------------------------------------------------------
// Member i owns ceil(P_i / BM) * ceil(Cout_i / BN) consecutive workgroups of a 1-D grid, pixel blocks fastest.
// What the host works out per member and passes by value: end = workgroups of members 0 .. i (INT32_MAX beyond n), npb = pixel
// blocks, Ho x Wo = output map
struct GroupMap {
    int32_t end[HAWQ_INCEP_GROUP_MAX], npb[HAWQ_INCEP_GROUP_MAX], Ho[HAWQ_INCEP_GROUP_MAX], Wo[HAWQ_INCEP_GROUP_MAX];
};

// workgroup `bid`: its member mi, and its index inside the member (pixel block local % npb, channel block local / npb).
// `mp` by value and `local`, `npb` named in front of the return: spelled otherwise (a reference; the expressions inside the return's
// braces) the kernels' scalar code for the selection comes out in another order than with these lines inside the kernels.
struct GroupMember {
    int mi, local, npb;
};
__device__ __forceinline__ GroupMember group_member(const GroupMap mp, const int bid) {
    int mi = 0, first = 0;   // the member and its first workgroup
#pragma unroll
    for (int j = 0; j < HAWQ_INCEP_GROUP_MAX - 1; ++j) {
        if (bid >= mp.end[j]) mi = j + 1, first = mp.end[j];
    }
    const int local = bid - first, npb = mp.npb[mi];
    return {mi, local, npb};
}

struct Span {
    uintptr_t lo, hi;   // bytes [lo, hi)
};
bool meet(const Span &x, const Span &y) { return x.lo < y.hi && y.lo < x.hi; }

// the host's view of the grid: per member its output pixels and the bytes it reads (in) and writes (out)
struct GroupGrid {
    GroupMap mp;
    long long total, P[HAWQ_INCEP_GROUP_MAX];
    Span in[HAWQ_INCEP_GROUP_MAX], out[HAWQ_INCEP_GROUP_MAX];
};

// lays the members of `g` (n in 1 .. 8) out on a grid of tile `tile` (1 .. NUM_TILES); a reason and the member `who` where that
// cannot be done (NULL: `gg` is filled).  No pointer is dereferenced.
const char *group_grid(const hawq_incep_group_args *g, int tile, GroupGrid *gg, int *who) {
    const int bm = kTiles[tile].bm, bn = kTiles[tile].bn;
    GroupMap *mp = &gg->mp;
    Span *in = gg->in, *out = gg->out;
    long long wgs = 0;
    for (int i = 0; i < g->n; ++i) {
        const hawq_incep_conv_args *a = &g->conv[i];
        *who = i;
        if (!hawq_incep_conv_tile_ok(a, tile)) return "the tile refuses this member (hawq_incep_conv_tile_ok)";
        const int Ho = (a->H + 2 * a->pad_h - a->KH) / a->stride + 1, Wo = (a->W + 2 * a->pad_w - a->KW) / a->stride + 1;
        const long long P = (long long)a->N * Ho * Wo, npb = (P + bm - 1) / bm;   // npb < 2^31 (hawq_incep_conv_tile_ok)
        wgs += npb * ((a->Cout + bn - 1) / bn);
        if (wgs >= (1ll << 31)) return "too many workgroups";
        mp->end[i] = (int32_t)wgs, mp->npb[i] = (int32_t)npb, mp->Ho[i] = Ho, mp->Wo[i] = Wo;
        const size_t es = a->epilogue == HAWQ_INCEP_RAW ? 4 : (size_t)a->out_bits / 8;
        gg->P[i] = P;
        in[i].lo = (uintptr_t)a->in, in[i].hi = in[i].lo + (size_t)a->N * a->H * a->W * a->Cin;
        out[i].lo = (uintptr_t)a->out + (size_t)a->c_off * es;
        out[i].hi = (uintptr_t)a->out + ((size_t)(P - 1) * a->ldo + a->c_off + a->Cout) * es;
    }
    for (int i = g->n; i < HAWQ_INCEP_GROUP_MAX; ++i) mp->end[i] = INT32_MAX, mp->npb[i] = 1, mp->Ho[i] = mp->Wo[i] = 0;
    gg->total = wgs;
    return nullptr;
}

}  // namespace
