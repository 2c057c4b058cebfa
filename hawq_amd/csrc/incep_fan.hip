// Grouped launch of the LDS-tiled InceptionV3 convs with a fan-out epilogue: next to its own output every member may store the
// int8 branch inputs of the NEXT unit, which the plan otherwise makes with one hawq_incep_requant launch per branch from the 16-bit
// concat buffer this epilogue has just written.
//   hawq_incep_conv_group_fan_ok   host arithmetic only: does tile `tile` run this group with these fans in one launch
//   hawq_incep_conv_group_fan      the launch: member i writes, byte for byte, what hawq_incep_conv_tiled(&g->conv[i], tile, s) writes,
//                                  and for j < fan[i].n   to[j].out[p * ldo + c_off + co] = (int8) clamp(dyadic_rne(y; m, ek), lo, hi)
//                                  of the element y it stored (after its last clamp) at pixel p, channel co
// Grid and member selection are incep_group.hip's (incep_tile.h: GroupMap, group_member, group_grid): one 1-D grid, running totals by
// value, the member a function of the workgroup id.  The workgroup body is the tiled kernel's (incep_tile_body.h) with fan_store below
// as its hook.
// The fan descriptors travel as kernel arguments next to the conv blocks: 1096 (group) + 128 (map) + 1088 (8 fans of 136 bytes) =
// 2312 bytes of the 4096 a launch may carry; member and fan index are wave-uniform, so they arrive through scalar loads.
// A lane holds 16 consecutive channels of one pixel when the epilogue ends (q[16]); a fan output is 16 dyadic_rne + clamp on them,
// four pack4_i8 and one 16-byte store.  Vector stores only.
#include "incep_tile.h"

extern "C" int hawq_incep_conv_group_ok(const hawq_incep_group_args *g, int tile);

namespace {

// the body's hook (INCEP_TILE_STORED): a lane has stored channels cb .. cb + 15 of pixel p; `fn`: the member's fan (wave-uniform)
__device__ __forceinline__ void fan_store(const hawq_incep_fan &fn, const long long p, const int cb, const int (&q)[16]) {
    // the fan: q[r] is what the member stored; each consumer takes it at its own scale, as int8, into its own row
#pragma unroll 1
    for (int t = 0; t < fn.n; ++t) {
        const hawq_incep_fan_out &f = fn.to[t];
        v4i d;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int s[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] = clampi(dyadic_rne(q[4 * e + u], f.m, f.ek), f.lo, f.hi);
            d[e] = (int)pack4_i8(s[0], s[1], s[2], s[3]);
        }
        *reinterpret_cast<v4i *>((int8_t *)f.out + (size_t)p * f.ldo + f.c_off + cb) = d;   // 16-byte aligned (fan_refusal)
    }
}

// the tiled kernel's workgroup body as incep_group.hip runs it (incep_tiled_body), with the member's fan `fn` for the hook
template <int BM, int BN, int WPX, int WCH, int KS>
__device__ __forceinline__ void incep_fan_body(const hawq_incep_conv_args &a, const hawq_incep_fan &fn, const int Ho, const int Wo,
                                               const long long pblock, const int cblock, char *lds) {
#define INCEP_TILE_BLOCK
#define INCEP_TILE_STORED(p, cb, q) fan_store(fn, p, cb, q)
#include "incep_tile_body.h"
#undef INCEP_TILE_BLOCK
#undef INCEP_TILE_STORED
}

struct FanSet {
    hawq_incep_fan fan[HAWQ_INCEP_GROUP_MAX];
};

// The occupancy floor is the group kernel's (3 waves per SIMD for the two large tiles, 4 for the others).  Without it the scheduler
// spreads the fan loop's 16 independent requants over 50 more VGPRs than the K loop needs and the kernel loses a wave per SIMD; with
// it the accumulators stay in VGPRs (no AGPR copy) and every instantiation fits: 122 / 156 / 80 / 85 registers, no scratch.
template <int BM, int BN, int WPX, int WCH, int KS>
__global__ __launch_bounds__(64 * WPX * WCH * KS) __attribute__((amdgpu_waves_per_eu(BM * BN >= 128 * 128 ? 3 : 4))) void incep_fan_kernel(hawq_incep_group_args g, GroupMap mp, FanSet fs) {
    const GroupMember m = group_member(mp, blockIdx.x);
    __shared__ __attribute__((aligned(16))) char lds[2 * (BM + BN) * 64];
    incep_fan_body<BM, BN, WPX, WCH, KS>(g.conv[m.mi], fs.fan[m.mi], mp.Ho[m.mi], mp.Wo[m.mi], (long long)(m.local % m.npb) * BM,
                                         (m.local / m.npb) * BN, lds);
}

// why tile `tile` does not run group `g` with the fans `fan` in one launch (NULL: it does, and `gg` describes the grid).
// No pointer is dereferenced.  `who`: the member, `which`: its fan output (-1: none in particular).
const char *fan_refusal(const hawq_incep_group_args *g, const hawq_incep_fan *fan, int tile, GroupGrid *gg, int *who, int *which) {
    *who = *which = -1;
    if (!g || !fan) return "null group or fan list";
    if (tile < 1 || tile > NUM_TILES) return "no such tile (a group runs on one of the ids 1 .. 4)";
    if (!hawq_incep_conv_group_ok(g, tile)) return "the grouped launch refuses the group (hawq_incep_conv_group_ok)";
    (void)group_grid(g, tile, gg, who);   // the grid hawq_incep_conv_group launches: its checks have just passed
    const Span *in = gg->in, *out = gg->out;
    Span fo[HAWQ_INCEP_GROUP_MAX][HAWQ_INCEP_FAN_MAX];
    for (int i = 0; i < g->n; ++i) {
        const hawq_incep_conv_args *a = &g->conv[i];
        const long long P = gg->P[i];
        *who = i;
        if (fan[i].n < 0 || fan[i].n > HAWQ_INCEP_FAN_MAX) return "a member has 0 .. 4 fan outputs";
        if (fan[i].n > 0 && a->epilogue == HAWQ_INCEP_RAW) return "a RAW member has no fan (the fan takes a requantised output)";
        for (int j = 0; j < fan[i].n; ++j) {
            const hawq_incep_fan_out *f = &fan[i].to[j];
            *which = j;
            if (!f->out) return "null fan output";
            if (!(f->lo >= -128 && f->lo <= f->hi && f->hi <= 127)) return "fan clamp bounds outside int8 (-128 <= lo <= hi <= 127)";
            if (f->m < 0 || f->ek < 0 || (f->ek & 0xff) < 1 || (f->ek & 0xff) > 62 || (f->ek >> 8) > 15)
                return "fan table outside the dyadic form (m >= 0, 1 <= e <= 62, k <= 15)";
            if (((uintptr_t)f->out & 15) || f->ldo % 16 || f->c_off % 16 || f->c_off < 0)
                return "a fan output is stored in 16-byte runs: out 16-byte aligned, ldo and c_off multiples of 16";
            if (f->ldo < f->c_off + a->Cout) return "fan ldo < c_off + Cout";
            fo[i][j].lo = (uintptr_t)f->out + (size_t)f->c_off;
            fo[i][j].hi = (uintptr_t)f->out + (size_t)(P - 1) * f->ldo + f->c_off + a->Cout;
        }
        *which = -1;
    }
    // independence, by group_refusal's two rules: channel intervals for slices of one buffer (same base, pitch, element width),
    // byte extents otherwise
    for (int i = 0; i < g->n; ++i) {
        const hawq_incep_conv_args *a = &g->conv[i];
        for (int j = 0; j < fan[i].n; ++j) {
            const hawq_incep_fan_out *f = &fan[i].to[j];
            *who = i, *which = j;
            for (int k = 0; k < g->n; ++k) {
                const hawq_incep_conv_args *b = &g->conv[k];
                if (meet(fo[i][j], in[k])) return "a fan output overlaps a member's input";
                const bool rows = f->out == b->out && f->ldo == b->ldo && b->epilogue != HAWQ_INCEP_RAW && b->out_bits == 8;
                if (rows ? (f->c_off < b->c_off + b->Cout && b->c_off < f->c_off + a->Cout) : meet(fo[i][j], out[k]))
                    return "a fan output overlaps a member's primary output";
                for (int l = 0; l < fan[k].n; ++l) {
                    if (k < i || (k == i && l <= j)) continue;
                    const hawq_incep_fan_out *h = &fan[k].to[l];
                    const bool same = f->out == h->out && f->ldo == h->ldo;
                    if (same ? (f->c_off < h->c_off + b->Cout && h->c_off < f->c_off + a->Cout) : meet(fo[i][j], fo[k][l]))
                        return "two fan outputs overlap";
                }
            }
        }
    }
    *who = *which = -1;
    return nullptr;
}

template <class T>
void launch(const hawq_incep_group_args *g, const GroupGrid &gg, const FanSet &fs, hipStream_t stream) {
    static_assert(sizeof(hawq_incep_group_args) + sizeof(GroupMap) + sizeof(FanSet) <= 4096, "kernel arguments");
    hipLaunchKernelGGL((incep_fan_kernel<T::BM, T::BN, T::WPX, T::WCH, T::KS>), dim3((unsigned)gg.total), dim3(T::NT), 0, stream, *g, gg.mp, fs);
}

}  // namespace

extern "C" int hawq_incep_conv_group_fan_ok(const hawq_incep_group_args *g, const hawq_incep_fan *fan, int tile) {
    GroupGrid gg;
    int who, which;
    return fan_refusal(g, fan, tile, &gg, &who, &which) == nullptr;
}

extern "C" int hawq_incep_conv_group_fan(const hawq_incep_group_args *g, const hawq_incep_fan *fan, int tile, void *stream) {
    GroupGrid gg;
    int who, which;
    const char *why = fan_refusal(g, fan, tile, &gg, &who, &which);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_group_fan: tile %d refuses the launch (member %d, fan output %d): %s", tile, who, which, why);
    FanSet fs;
    for (int i = 0; i < HAWQ_INCEP_GROUP_MAX; ++i) {
        fs.fan[i] = fan[i < g->n ? i : 0];
        if (i >= g->n) fs.fan[i].n = 0;
    }
    for_tile(tile, [&](auto t) { launch<decltype(t)>(g, gg, fs, (hipStream_t)stream); });
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
