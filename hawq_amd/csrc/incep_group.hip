// Grouped launch of the LDS-tiled InceptionV3 convs (grouped-GEMM style): one 1-D grid whose workgroups are dealt out to up to
// HAWQ_INCEP_GROUP_MAX independent convs - the sibling convs at one depth of an Inception unit's branches.
//   hawq_incep_conv_group_ok   host arithmetic only: is this a group tile `tile` can run in one launch
//   hawq_incep_conv_group      the launch: writes, byte for byte, what hawq_incep_conv_tiled(&g->conv[i], tile, s), i = 0 .. n - 1, write
// Members keep their own argument blocks (shape, window, stride, epilogue, tables, buffers, output slice); only the grid is shared.
// Member i owns ceil(P_i / BM) * ceil(Cout_i / BN) consecutive workgroups, pixel blocks fastest as in the 2-D grid of the single
// launch.  A workgroup finds its member by comparing its index with the (at most 8) running totals the host passes by value, takes
// (pixel block, channel block) from its index inside the member, and runs the tiled kernel's body on the member's argument block.
// Everything it reads for that is wave-uniform: the totals and the argument blocks are kernel arguments, the member index is a
// function of the workgroup id, so the descriptor arrives through scalar loads from the kernarg segment (no copy in scratch:
// DESIGN.md 10).  The grid (GroupMap, group_member, group_grid) is in incep_tile.h, which incep_fan.hip shares.
#include "incep_tile.h"

namespace {

// The tiled kernel's workgroup body (incep_tile_body.h, the text incep_tiled_kernel includes) on one member: the same staging,
// lds_off swizzle, MFMA order and epilogue, so a workgroup writes the bytes the single launch's workgroup writes.
// `a`: the member (wave-uniform), Ho x Wo its output map; the workgroup computes pixels pblock .. pblock + BM - 1 and channels
// cblock .. cblock + BN - 1 in the two LDS stages `lds`.
template <int BM, int BN, int WPX, int WCH, int KS>
__device__ __forceinline__ void incep_tiled_body(const hawq_incep_conv_args &a, const int Ho, const int Wo, const long long pblock,
                                                 const int cblock, char *lds) {
#define INCEP_TILE_BLOCK
#define INCEP_TILE_STORED(p, cb, q)
#include "incep_tile_body.h"
#undef INCEP_TILE_BLOCK
#undef INCEP_TILE_STORED
}

template <int BM, int BN, int WPX, int WCH, int KS>
__global__ __launch_bounds__(64 * WPX * WCH * KS) void incep_group_kernel(hawq_incep_group_args g, GroupMap mp) {
    const GroupMember m = group_member(mp, blockIdx.x);
    __shared__ __attribute__((aligned(16))) char lds[2 * (BM + BN) * 64];
    incep_tiled_body<BM, BN, WPX, WCH, KS>(g.conv[m.mi], mp.Ho[m.mi], mp.Wo[m.mi], (long long)(m.local % m.npb) * BM, (m.local / m.npb) * BN, lds);
}

// why tile `tile` does not run group `g` in one launch (NULL: it does, and `gg` describes the grid).  No pointer is dereferenced.
const char *group_refusal(const hawq_incep_group_args *g, int tile, GroupGrid *gg, int *who) {
    *who = -1;
    if (!g) return "null group";
    if (g->n < 1 || g->n > HAWQ_INCEP_GROUP_MAX) return "a group has 1 .. 8 members";
    if (tile < 1 || tile > NUM_TILES) return "no such tile (a group runs on one of the ids 1 .. 4)";
    if (const char *why = group_grid(g, tile, gg, who)) return why;
    const Span *in = gg->in, *out = gg->out;
    for (int i = 0; i < g->n; ++i) {
        const hawq_incep_conv_args *a = &g->conv[i];
        *who = i;
        for (int j = 0; j < g->n; ++j) {
            const hawq_incep_conv_args *b = &g->conv[j];
            if (meet(in[i], out[j])) return "a member reads what a member of the group writes";
            if (j <= i) continue;
            const bool rows = a->out == b->out && a->ldo == b->ldo && a->out_bits == b->out_bits &&
                              (a->epilogue == HAWQ_INCEP_RAW) == (b->epilogue == HAWQ_INCEP_RAW);   // slices of one concat buffer
            if (rows ? (a->c_off < b->c_off + b->Cout && b->c_off < a->c_off + a->Cout) : meet(out[i], out[j]))
                return "two members write overlapping outputs";
        }
    }
    *who = -1;
    return nullptr;
}

template <class T>
void launch(const hawq_incep_group_args *g, const GroupGrid &gg, hipStream_t stream) {
    hipLaunchKernelGGL((incep_group_kernel<T::BM, T::BN, T::WPX, T::WCH, T::KS>), dim3((unsigned)gg.total), dim3(T::NT), 0, stream, *g, gg.mp);
}

}  // namespace

extern "C" int hawq_incep_conv_group_ok(const hawq_incep_group_args *g, int tile) {
    GroupGrid gg;
    int who;
    return group_refusal(g, tile, &gg, &who) == nullptr;
}

extern "C" int hawq_incep_conv_group(const hawq_incep_group_args *g, int tile, void *stream) {
    GroupGrid gg;
    int who;
    const char *why = group_refusal(g, tile, &gg, &who);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_group: tile %d refuses the group (member %d): %s", tile, who, why);
    for_tile(tile, [&](auto t) { launch<decltype(t)>(g, gg, (hipStream_t)stream); });
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
