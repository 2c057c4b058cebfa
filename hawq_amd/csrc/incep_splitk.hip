// Cross-workgroup split-K form of the grouped InceptionV3 conv launch (incep_group.hip) for launches with few output tiles: batch 1 - 16,
// where a level of an 8 x 8 or 17 x 17 unit puts 6 - 21 workgroups on the chip and lasts as long as one workgroup's whole K loop.
//   hawq_incep_conv_group_splitk_ok          host arithmetic only: does the launch take this group with these slice counts
//   hawq_incep_conv_group_splitk_workspace   bytes of the slab and of the counters
//   hawq_incep_conv_group_splitk             the launch: writes, byte for byte, what hawq_incep_conv_group(g, 3, stream) writes
// Same argument block, same independence rules (incep_tile.h: group_grid, group_dependence), tile 3's shape: 128 px x 64 ch, 4 waves of
// 64 px x 32 ch.  Integer partial sums are exact in any order (mod 2^32 included), so the bytes do not depend on the slice counts or
// on which workgroup arrives last.
//
// Grid.  Member i has tiles_i = ceil(P_i / 128) * ceil(Cout_i / 64) output tiles and its own slice count S_i; it owns tiles_i * S_i
// consecutive workgroups of a 1-D grid, slice-major (workgroup `local` of the member: slice local / tiles_i of tile local % tiles_i),
// so the slices of one tile lie tiles_i workgroups apart and spread over the chip.  The host passes the running totals by value
// (GroupMap, as the grouped launch does) together with tiles_i, S_i, q_i and the member's first slab and counter (SliceMap).
//
// K slicing.  K is walked in the tiled body's 64-byte steps (four 16-channel units of the flattened [KH][KW][Cin] axis per row):
// steps_i = ceil(KH KW (Cin / 16) / 4), q_i = ceil(steps_i / S_i), slice z walks steps z q_i .. min((z + 1) q_i, steps_i) - 1.  A slice
// may start in the middle of a tap: each staging thread derives (kh, kw, c16) of its first unit with one division and then advances as
// the tiled body does.  Padding taps and units beyond K are zeros, as there.
//
// K loop (this file's own; the tiled body's loop is two stages with one global round trip and one barrier per step).  Slices are
// short - 1 - 8 steps - so the round trip, not the MFMAs, is what a slice lasts.  Here a workgroup moves CH = 4 steps at a time: it
// issues all 12 16-byte loads of a chunk (2 pixel rows + 1 weight row per thread and step) before it waits for any of them, writes
// them to four LDS stages (48 KiB, the swizzle of lds_off), passes ONE barrier and runs the chunk's 16 MFMAs per wave.  A slice of up
// to four steps is one round trip and one barrier.  A longer walk (an unsplit member runs its whole K loop here) issues the next
// chunk's loads in front of the MFMAs, holds them in registers (48 VGPRs) and writes them after a second barrier: one round trip per
// four steps, hidden under four steps of MFMAs.
//
// Partials and arrival (conv_splitk.hip's protocol; placement independent, nothing spins, any residency of the grid is fine):
//   every thread: its share of the 128 x 64 int32 partial tile -> the slice's slab, in MFMA register order, 16-byte stores; agent-scope
//   release fence; workgroup barrier; thread 0: relaxed agent-scope fetch_add on the tile's counter, "last" to the others through LDS;
//   the last arriver: agent-scope acquire fence, counter back to 0, adds the other slices' slabs to the partial it still holds in
//   registers and runs the epilogue - the tiled body's statements (RAW, REQUANT, REQUANT2; out_bits 8, 16, 32; ldo / c_off; 16-byte
//   stores).
// A member with S_i = 1 goes from its K loop straight to the epilogue and touches neither slab nor counter.
// Workspace: slab [sum over S_i > 1 of tiles_i * S_i][4 waves][2 MFMA tiles][4 register quads][64 lanes][4] int32, tile-major inside a
// member (a tile's S_i slabs are contiguous); one int32 counter per tile of such a member, zero before the first launch and left zero
// by every launch.
// SliceMap, the host's slice layout and, as text, the arrival protocol are in incep_splitk.h and incep_splitk_arrive.h: the mixed-form
// split launch (incep_group_nib_splitk.hip) runs the same ones.
#include "incep_splitk.h"

namespace {

using SKT = Tile<3, 128, 64, 2, 2, 1>;
constexpr int BM = SKT::BM, BN = SKT::BN, WPX = SKT::WPX, WCH = SKT::WCH, NT = SKT::NT;
constexpr int RSTEP = NT / 4, APT = BM / RSTEP, BPT = BN / RSTEP, RPT = APT + BPT;
constexpr int WM = BM / WPX / 32, WN = BN / WCH / 32;
constexpr int STAGE = (BM + BN) * 64;   // bytes of one K step of both operand tiles
constexpr int CH = 4;                   // K steps per chunk: loads in flight together, LDS stages
constexpr int SLAB = BM * BN;           // int32 partial sums per slab
static_assert(WM == 2 && WN == 1 && APT == 2 && BPT == 1, "the 128 x 64 tile: 4 waves of 64 px x 32 ch");

__global__ __launch_bounds__(NT) void incep_splitk_kernel(hawq_incep_group_args g, GroupMap mp, SliceMap sm, int32_t *slab, int32_t *counters) {
    __shared__ __attribute__((aligned(16))) char lds[CH * STAGE];
    __shared__ int last;
    const GroupMember gm = group_member(mp, blockIdx.x);
    const hawq_incep_conv_args &a = g.conv[gm.mi];
    const int Ho = mp.Ho[gm.mi], Wo = mp.Wo[gm.mi];
    const int tiles = sm.tiles[gm.mi], S = sm.S[gm.mi];
    const int z = gm.local / tiles, tile = gm.local % tiles;   // slice-major
    const long long pblock = (long long)(tile % gm.npb) * BM;
    const int cblock = (tile / gm.npb) * BN;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int wpx = wave % WPX, wch = wave / WPX;
    const int slot = tid & 3, r0 = tid >> 2;
    const long long P = (long long)a.N * Ho * Wo;
    const int C16 = a.Cin >> 4, K16 = a.KH * a.KW * C16, steps = (K16 + 3) >> 2;
    const int s0 = z * sm.q[gm.mi], s1 = min(s0 + sm.q[gm.mi], steps);   // this slice's steps
    const int8_t *in = (const int8_t *)a.in, *wgt = (const int8_t *)a.wgt;

    // the rows this thread stages
    const int8_t *abase[APT];
    int iy0[APT], ix0[APT];
#pragma unroll
    for (int i = 0; i < APT; ++i) {
        const long long p = pblock + r0 + i * RSTEP;
        abase[i] = in, iy0[i] = -(1 << 20), ix0[i] = 0;   // a row beyond P: every tap fails the bounds test below
        if (p < P) {
            const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
            abase[i] = in + (size_t)(p / ((long long)Wo * Ho)) * a.H * a.W * a.Cin;
            iy0[i] = oy * a.stride - a.pad_h, ix0[i] = ox * a.stride - a.pad_w;
        }
    }
    const int co = cblock + (r0 & ~31) + cperm(r0 & 31);
    const bool wv = co < a.Cout;
    const int8_t *wrow = wgt + (wv ? (size_t)co * K16 * 16 : 0);
    // this thread's k16 unit of the step to load next: the slice's first step may lie anywhere on the [KH][KW][Cin / 16] axis
    int k16 = 4 * s0 + slot, c16 = k16 % C16, kw = (k16 / C16) % a.KW, kh = (k16 / C16) / a.KW;

    v4i rg[CH][RPT];
    bool ok[CH][RPT];
    const v4i zero = {0, 0, 0, 0};
    // the first n steps of a chunk: unconditional loads (a refused element reads the first bytes of its operand, and becomes zeros on
    // its way to LDS), none of them waited for before the last is issued
    auto load = [&](int n) {
#pragma unroll
        for (int t = 0; t < CH; ++t) {
            if (t >= n) break;
            const bool kv = k16 < K16;
#pragma unroll
            for (int i = 0; i < APT; ++i) {
                const int iy = iy0[i] + kh, ix = ix0[i] + kw;
                ok[t][i] = kv && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                const size_t off = ok[t][i] ? ((size_t)iy * a.W + ix) * a.Cin + c16 * 16 : 0;
                rg[t][i] = *reinterpret_cast<const v4i *>((ok[t][i] ? abase[i] : in) + off);
            }
            ok[t][APT] = kv && wv;
            rg[t][APT] = *reinterpret_cast<const v4i *>(wrow + (ok[t][APT] ? (size_t)k16 * 16 : 0));
            k16 += 4, c16 += 4;
            while (c16 >= C16) {
                c16 -= C16;
                if (++kw == a.KW) kw = 0, ++kh;
            }
        }
    };
    auto write = [&](int n) {
#pragma unroll
        for (int t = 0; t < CH; ++t) {
            if (t >= n) break;
#pragma unroll
            for (int i = 0; i < RPT; ++i) *reinterpret_cast<v4i *>(lds + t * STAGE + lds_off(r0 + i * RSTEP, slot)) = ok[t][i] ? rg[t][i] : zero;
        }
    };

    v16i acc[WM];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0;

    auto compute = [&](int n) {
#pragma unroll
        for (int t = 0; t < CH; ++t) {
            if (t >= n) break;
            const char *s = lds + t * STAGE;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {   // the 32-byte halves of the step
                v4i af[WM];
#pragma unroll
                for (int i = 0; i < WM; ++i) af[i] = *reinterpret_cast<const v4i *>(s + lds_off(wpx * 32 * WM + 32 * i + l31, 2 * kk + h));
                const v4i bf = *reinterpret_cast<const v4i *>(s + lds_off(BM + wch * 32 + l31, 2 * kk + h));
#pragma unroll
                for (int i = 0; i < WM; ++i) acc[i] = __builtin_amdgcn_mfma_i32_32x32x32_i8(bf, af[i], acc[i], 0, 0, 0);
            }
        }
    };

    int n = min(CH, s1 - s0), left = s1 - s0 - n;
    load(n);
    for (;;) {
        write(n);
        __syncthreads();
        const int staged = n;
        n = min(CH, left), left -= n;
        if (n > 0) load(n);   // in flight under the MFMAs of the staged chunk
        compute(staged);
        if (n <= 0) break;
        __syncthreads();   // every wave has read the stages the next chunk overwrites
    }

#include "incep_splitk_arrive.h"

    // the tiled body's epilogue: acc[i][r] = channel cblock + 32 wch + 16 h + r of pixel pblock + 32 (wpx WM + i) + l31
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        const long long p = pblock + 32 * (wpx * WM + i) + l31;
        const int cb = cblock + 32 * wch + 16 * h;
        if (p >= P || cb >= a.Cout) continue;   // Cout % 16 == 0: the 16 channels of a lane half are all valid or all not
        const size_t row = (size_t)p * a.ldo + a.c_off + cb;   // a multiple of 16 elements (hawq_incep_conv_tile_ok)
        int q[16];
        if (a.epilogue == HAWQ_INCEP_RAW) {
#pragma unroll
            for (int r = 0; r < 16; ++r) q[r] = acc[i][r] + a.bias[cb + r];
            v4i *o = reinterpret_cast<v4i *>((int32_t *)a.out + row);
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = v4i{q[4 * r], q[4 * r + 1], q[4 * r + 2], q[4 * r + 3]};
            continue;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = cb + r;
            int v = acc[i][r] + a.bias[c];
            if (a.relu) v = max(v, 0);
            q[r] = clampi(dyadic_rne(v, a.m[c], a.ek[c]), a.q_lo, a.q_hi);
            if (a.epilogue == HAWQ_INCEP_REQUANT2) q[r] = clampi(dyadic_rne(q[r], a.m2, a.ek2), a.q2_lo, a.q2_hi);
        }
        if (a.out_bits == 16) {
            v4i *o = reinterpret_cast<v4i *>((int16_t *)a.out + row);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                v4i d;
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = (q[8 * r + 2 * e] & 0xffff) | (int)((unsigned)q[8 * r + 2 * e + 1] << 16);
                o[r] = d;
            }
        } else {
            v4i d;
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = (int)pack4_i8(q[4 * e], q[4 * e + 1], q[4 * e + 2], q[4 * e + 3]);
            *reinterpret_cast<v4i *>((int8_t *)a.out + row) = d;
        }
    }
}

// why the launch does not take group `g` with slice counts `slices` (NULL: it does, and `sg` describes it); `who`: the member, or -1.
// No pointer of an argument block is dereferenced.
const char *split_refusal(const hawq_incep_group_args *g, int tile, const int32_t *slices, SplitGrid *sg, int *who) {
    *who = -1;
    if (!g) return "null group";
    if (g->n < 1 || g->n > HAWQ_INCEP_GROUP_MAX) return "a group has 1 .. 8 members";
    if (tile != 3) return "only tile 3 (128 px x 64 ch) has a split-K form";
    if (!slices) return "null slice counts";
    if (const char *why = group_grid(g, tile, &sg->gg, who)) return why;
    if (const char *why = group_dependence(g, &sg->gg, who)) return why;
    if (const char *why = split_layout(g, 0u, slices, sg, who)) return why;
    if (!sg->slabs) return "no member has more than one slice (that launch is hawq_incep_conv_group)";
    return nullptr;
}

}  // namespace

extern "C" int hawq_incep_conv_group_splitk_ok(const hawq_incep_group_args *g, int tile, const int32_t *slices) {
    SplitGrid sg;
    int who;
    return split_refusal(g, tile, slices, &sg, &who) == nullptr;
}

extern "C" int hawq_incep_conv_group_splitk_workspace(const hawq_incep_group_args *g, int tile, const int32_t *slices, int64_t *slab_bytes,
                                                      int64_t *counter_bytes) {
    SplitGrid sg;
    int who;
    const char *why = split_refusal(g, tile, slices, &sg, &who);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_group_splitk_workspace: tile %d refuses the group (member %d): %s", tile, who, why);
    if (slab_bytes) *slab_bytes = sg.slabs * SLAB * 4;
    if (counter_bytes) *counter_bytes = sg.counters * 4;
    return 0;
}

extern "C" int hawq_incep_conv_group_splitk(const hawq_incep_group_args *g, int tile, const int32_t *slices, void *slab, int32_t *counters,
                                            void *stream) {
    SplitGrid sg;
    int who;
    const char *why = split_refusal(g, tile, slices, &sg, &who);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_group_splitk: tile %d refuses the group (member %d): %s", tile, who, why);
    HAWQ_REQUIRE(slab && !((uintptr_t)slab & 15) && counters, "hawq_incep_conv_group_splitk: slab (16-byte aligned) and counters must be non-null");
    hipLaunchKernelGGL(incep_splitk_kernel, dim3((unsigned)sg.total), dim3(NT), 0, (hipStream_t)stream, *g, sg.gg.mp, sg.sm, (int32_t *)slab, counters);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
