// Cross-workgroup split-K form of the mixed-form grouped InceptionV3 conv launch (incep_group_nib.hip) for launches with few output
// tiles: the levels of a nibble plan's 8 x 8 and 17 x 17 units at batch 1 - 16, which put 6 - 21 workgroups on the chip.
//   hawq_incep_conv_group_nib_splitk_ok          host arithmetic only: does the launch take this group, mask and slice counts
//   hawq_incep_conv_group_nib_splitk_workspace   bytes of the slab and of the counters
//   hawq_incep_conv_group_nib_splitk             the launch: writes, byte for byte, what hawq_incep_conv_group_nib(g, mask, 2, stream) writes
// Bit i of `mask`: member i's in and wgt are hawq4.  Only mixed-group tile 2 (128 px x 64 ch, 4 waves of 64 px x 32 ch) has this form.
//
// Grid, slices, partials, arrival and workspace are incep_splitk.hip's (incep_splitk.h, and incep_splitk_arrive.h as text): member i
// owns tiles_i * S_i consecutive workgroups, slice-major; GroupMap, SliceMap and the mask travel by value, so the choice between the two
// K loops below is a scalar branch on (mask >> member) & 1, as in incep_group_nib_kernel.
//
// K steps depend on the member's form.  A step is one 64-byte row per pixel and per output channel in LDS: four 16-byte units of 16
// int8 channels (steps = ceil(KH KW (Cin / 16) / 4)), or eight 8-byte units of 16 nibble channels (steps = ceil(KH KW (Cin / 16) / 8)).
// q = ceil(steps / S), slice z walks steps z q .. min((z + 1) q, steps) - 1, and may begin in the middle of a tap: a staging thread
// derives (kh, kw, c16) of its first unit from k16 = 4 s0 + slot or 8 s0 + unit with one division and then advances as its family's
// single-launch body does.  Padding taps, rows beyond P or Cout and units beyond K are zeros.
//
// K loops.  Both move CH = 4 steps at a time: all loads of a chunk are issued before any is waited for, written to four LDS stages
// (48 KiB: both forms stage (128 + 64) * 64 bytes a step, and a workgroup runs one of them), one barrier, the chunk's MFMAs; a longer
// walk holds the next chunk in registers under those MFMAs and writes it after a second barrier.
//   int8:  a thread owns 16-byte slot tid & 3 of rows tid >> 2 (+ 64): 2 pixel rows + 1 weight row, 12 loads of 16 bytes a chunk;
//          2 x 2 MFMAs (32x32x32 i8) a step and wave - incep_splitk_kernel's loop.
//   hawq4: a thread owns 8-byte unit tid & 7 of rows tid >> 3 (+ 32 ..): 4 pixel rows + 2 weight rows, 24 loads of 8 bytes a chunk, the
//          same 48 registers, placed at lds_off(row, unit >> 1) + 8 (unit & 1) as in incep_nib_body.h; a lane reads 16-byte slots and
//          widens the two units of each (widen_act, widen_wgt): 4 x 2 MFMAs a step and wave.  Which loads of a chunk are real is one
//          bit each of a 24-bit register, not 24 flags.
//
// Partials are the raw int32 accumulators.  A hawq4 member's are 16 x the true sums (its weights sit in the high nibbles); the >> 4 of
// the nibble epilogue is applied once, to the complete sum, never per slice: the parent shifts the sum as it stands mod 2^32, and
// shifted partials add up to something else where that sum wraps.  Sums mod 2^32 commute, so the bytes written do not depend on the
// slice counts or on which workgroup arrives last.
//
// Epilogue: the parents' statements with the one difference between them - (acc >> 4) against acc - as a shift count that is 4 or 0:
// bias, RAW or relu / dyadic requant / second requant, then 32-, 16- or 8-bit stores at `row`, or (hawq4 members only: the host
// refuses out_bits 4 on an int8 member) pack8_u4 stores at byte row >> 1.  No fan-out hook.
#include "incep_group_nib.h"
#include "incep_splitk.h"

namespace {

using SKT = Tile<kGn[2].i8, 128, 64, 2, 2, 1>;
constexpr int BM = SKT::BM, BN = SKT::BN, WPX = SKT::WPX, WCH = SKT::WCH, NT = SKT::NT;
constexpr int WM = BM / WPX / 32, WN = BN / WCH / 32;
constexpr int STAGE = (BM + BN) * 64;   // bytes of one K step of both operand tiles, in either form
constexpr int CH = 4;                   // K steps per chunk: loads in flight together, LDS stages
constexpr int SLAB = BM * BN;           // int32 partial sums per slab
static_assert(WM == 2 && WN == 1 && NT == 256, "the 128 x 64 tile: 4 waves of 64 px x 32 ch");

// steps s0 .. s1 - 1 of an int8 member's K loop into acc: incep_splitk_kernel's chunked loop
__device__ __forceinline__ void i8_slice(const hawq_incep_conv_args &a, const int Ho, const int Wo, const long long pblock, const int cblock,
                                         const int s0, const int s1, char *lds, v16i (&acc)[WM]) {
    constexpr int RSTEP = NT / 4, APT = BM / RSTEP, BPT = BN / RSTEP, RPT = APT + BPT;
    static_assert(APT == 2 && BPT == 1, "2 pixel rows + 1 weight row per thread");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int wpx = wave % WPX, wch = wave / WPX;
    const int slot = tid & 3, r0 = tid >> 2;
    const long long P = (long long)a.N * Ho * Wo;
    const int C16 = a.Cin >> 4, K16 = a.KH * a.KW * C16;
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
}

// steps s0 .. s1 - 1 of a hawq4 member's K loop into acc (16 x the sums): the same scheme on nibble rows
__device__ __forceinline__ void nib_slice(const hawq_incep_conv_args &a, const int Ho, const int Wo, const long long pblock, const int cblock,
                                          const int s0, const int s1, char *lds, v16i (&acc)[WM]) {
    constexpr int RSTEP = NT / 8, APT = BM / RSTEP, BPT = BN / RSTEP, RPT = APT + BPT;
    static_assert(APT == 4 && BPT == 2 && CH * RPT <= 32, "4 pixel rows + 2 weight rows per thread; one validity bit per load of a chunk");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int wpx = wave % WPX, wch = wave / WPX;
    const int unit = tid & 7, r0 = tid >> 3;
    const long long P = (long long)a.N * Ho * Wo;
    const int C16 = a.Cin >> 4, K16 = a.KH * a.KW * C16;
    const size_t pix_bytes = (size_t)a.Cin >> 1;
    const char *in = (const char *)a.in, *wgt = (const char *)a.wgt;

    // the rows this thread stages
    const char *abase[APT];
    int iy0[APT], ix0[APT];
#pragma unroll
    for (int i = 0; i < APT; ++i) {
        const long long p = pblock + r0 + i * RSTEP;
        abase[i] = in, iy0[i] = -(1 << 20), ix0[i] = 0;   // a row beyond P: every tap fails the bounds test below
        if (p < P) {
            const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
            abase[i] = in + (size_t)(p / ((long long)Wo * Ho)) * a.H * a.W * pix_bytes;
            iy0[i] = oy * a.stride - a.pad_h, ix0[i] = ox * a.stride - a.pad_w;
        }
    }
    const char *wrow[BPT];
    bool wv[BPT];
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
        const int q = r0 + j * RSTEP, co = cblock + (q & ~31) + cperm(q & 31);
        wv[j] = co < a.Cout;
        wrow[j] = wgt + (wv[j] ? (size_t)co * K16 * 8 : 0);
    }
    // this thread's unit of the step to load next: the slice's first step may lie anywhere on the [KH][KW][Cin / 16] axis
    int k16 = 8 * s0 + unit, c16 = k16 % C16, kw = (k16 / C16) % a.KW, kh = (k16 / C16) / a.KW;

    v2i rg[CH][RPT];
    unsigned okm = 0;   // bit t * RPT + i: load i of step t of the chunk in rg is real
    const v2i zero = {0, 0};
    // the first n steps of a chunk: unconditional loads (a refused unit reads the first 8 bytes of its operand, and becomes zeros on its
    // way to LDS), none of them waited for before the last is issued
    auto load = [&](int n) {
        okm = 0;
#pragma unroll
        for (int t = 0; t < CH; ++t) {
            if (t >= n) break;
            const bool kv = k16 < K16;
#pragma unroll
            for (int i = 0; i < APT; ++i) {
                const int iy = iy0[i] + kh, ix = ix0[i] + kw;
                const bool v = kv && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                const size_t off = v ? ((size_t)iy * a.W + ix) * pix_bytes + c16 * 8 : 0;
                rg[t][i] = *reinterpret_cast<const v2i *>((v ? abase[i] : in) + off);
                okm |= (unsigned)v << (t * RPT + i);
            }
#pragma unroll
            for (int j = 0; j < BPT; ++j) {
                const bool v = kv && wv[j];
                rg[t][APT + j] = *reinterpret_cast<const v2i *>(wrow[j] + (v ? (size_t)k16 * 8 : 0));
                okm |= (unsigned)v << (t * RPT + APT + j);
            }
            k16 += 8, c16 += 8;
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
            for (int i = 0; i < RPT; ++i)
                *reinterpret_cast<v2i *>(lds + t * STAGE + lds_off(r0 + i * RSTEP, unit >> 1) + 8 * (unit & 1)) = (okm >> (t * RPT + i)) & 1 ? rg[t][i] : zero;
        }
    };
    auto compute = [&](int n) {
#pragma unroll
        for (int t = 0; t < CH; ++t) {
            if (t >= n) break;
            const char *s = lds + t * STAGE;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {   // the 32-byte halves of the row
                v4i af[WM];
#pragma unroll
                for (int i = 0; i < WM; ++i) af[i] = *reinterpret_cast<const v4i *>(s + lds_off(wpx * 32 * WM + 32 * i + l31, 2 * kk + h));
                const v4i bf = *reinterpret_cast<const v4i *>(s + lds_off(BM + wch * 32 + l31, 2 * kk + h));
#pragma unroll
                for (int u = 0; u < 2; ++u) {   // the even unit of every lane's slot, then the odd one
                    const v4i wb = widen_wgt(bf[2 * u], bf[2 * u + 1]);
#pragma unroll
                    for (int i = 0; i < WM; ++i) acc[i] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wb, widen_act(af[i][2 * u], af[i][2 * u + 1]), acc[i], 0, 0, 0);
                }
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
}

__global__ __launch_bounds__(NT) void incep_group_nib_splitk_kernel(hawq_incep_group_args g, GroupMap mp, SliceMap sm, unsigned mask, int32_t *slab,
                                                                    int32_t *counters) {
    __shared__ __attribute__((aligned(16))) char lds[CH * STAGE];
    __shared__ int last;
    const GroupMember gm = group_member(mp, blockIdx.x);
    const hawq_incep_conv_args &a = g.conv[gm.mi];
    const int Ho = mp.Ho[gm.mi], Wo = mp.Wo[gm.mi];
    const int tiles = sm.tiles[gm.mi], S = sm.S[gm.mi];
    const int z = gm.local / tiles, tile = gm.local % tiles;   // slice-major
    const long long pblock = (long long)(tile % gm.npb) * BM;
    const int cblock = (tile / gm.npb) * BN;
    const bool nib = (mask >> gm.mi) & 1;   // a function of the workgroup id and the kernel arguments: scalar

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int wpx = wave % WPX, wch = wave / WPX;
    const long long P = (long long)a.N * Ho * Wo;
    const int K16 = a.KH * a.KW * (a.Cin >> 4), steps = nib ? (K16 + 7) >> 3 : (K16 + 3) >> 2;
    const int s0 = z * sm.q[gm.mi], s1 = min(s0 + sm.q[gm.mi], steps);   // this slice's steps

    v16i acc[WM];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0;

    if (nib) nib_slice(a, Ho, Wo, pblock, cblock, s0, s1, lds, acc);
    else i8_slice(a, Ho, Wo, pblock, cblock, s0, s1, lds, acc);

#include "incep_splitk_arrive.h"

    // acc[i][r] = (16 x, hawq4) channel cblock + 32 wch + 16 h + r of pixel pblock + 32 (wpx WM + i) + l31, all slices added
    const int sh = nib ? 4 : 0;   // a hawq4 sum is an exact multiple of 16
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        const long long p = pblock + 32 * (wpx * WM + i) + l31;
        const int cb = cblock + 32 * wch + 16 * h;
        if (p >= P || cb >= a.Cout) continue;   // Cout % 16 == 0: the 16 channels of a lane half are all valid or all not
        const size_t row = (size_t)p * a.ldo + a.c_off + cb;   // a multiple of 16 elements (the members' _ok)
        int q[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) q[r] = (acc[i][r] >> sh) + a.bias[cb + r];
        if (a.epilogue == HAWQ_INCEP_RAW) {
            v4i *o = reinterpret_cast<v4i *>((int32_t *)a.out + row);
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = v4i{q[4 * r], q[4 * r + 1], q[4 * r + 2], q[4 * r + 3]};
            continue;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = cb + r;
            if (a.relu) q[r] = max(q[r], 0);
            q[r] = clampi(dyadic_rne(q[r], a.m[c], a.ek[c]), a.q_lo, a.q_hi);
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
        } else if (a.out_bits == 4) {   // hawq4: 16 channels = two dwords at byte row / 2
            *reinterpret_cast<v2i *>((char *)a.out + (row >> 1)) = v2i{(int)pack8_u4(q), (int)pack8_u4(q + 8)};
        } else {
            v4i d;
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = (int)pack4_i8(q[4 * e], q[4 * e + 1], q[4 * e + 2], q[4 * e + 3]);
            *reinterpret_cast<v4i *>((int8_t *)a.out + row) = d;
        }
    }
}

// why the launch does not take group `g` with the forms `mask` and the slice counts `slices` (NULL: it does, and `sg` describes it);
// `who`: the member, or -1.  gn_refusal's reasons, then split_layout's.  No pointer of an argument block is dereferenced.
const char *gn_split_refusal(const hawq_incep_group_args *g, unsigned mask, int tile, const int32_t *slices, SplitGrid *sg, int *who) {
    *who = -1;
    if (tile != 2 && tile >= 1 && tile <= NUM_GN_TILES) return "only tile 2 (128 px x 64 ch) has a split-K form";
    if (const char *why = gn_refusal(g, mask, tile, &sg->gg, who)) return why;
    if (!slices) return "null slice counts";
    if (const char *why = split_layout(g, mask, slices, sg, who)) return why;
    if (!sg->slabs) return "no member has more than one slice (that launch is hawq_incep_conv_group_nib)";
    return nullptr;
}

}  // namespace

extern "C" int hawq_incep_conv_group_nib_splitk_ok(const hawq_incep_group_args *g, uint32_t mask, int tile, const int32_t *slices) {
    SplitGrid sg;
    int who;
    return gn_split_refusal(g, mask, tile, slices, &sg, &who) == nullptr;
}

extern "C" int hawq_incep_conv_group_nib_splitk_workspace(const hawq_incep_group_args *g, uint32_t mask, int tile, const int32_t *slices,
                                                          int64_t *slab_bytes, int64_t *counter_bytes) {
    SplitGrid sg;
    int who;
    const char *why = gn_split_refusal(g, mask, tile, slices, &sg, &who);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_group_nib_splitk_workspace: tile %d refuses the group (member %d, mask 0x%x): %s", tile, who, (unsigned)mask, why);
    if (slab_bytes) *slab_bytes = sg.slabs * SLAB * 4;
    if (counter_bytes) *counter_bytes = sg.counters * 4;
    return 0;
}

extern "C" int hawq_incep_conv_group_nib_splitk(const hawq_incep_group_args *g, uint32_t mask, int tile, const int32_t *slices, void *slab,
                                                int32_t *counters, void *stream) {
    SplitGrid sg;
    int who;
    const char *why = gn_split_refusal(g, mask, tile, slices, &sg, &who);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_group_nib_splitk: tile %d refuses the group (member %d, mask 0x%x): %s", tile, who, (unsigned)mask, why);
    HAWQ_REQUIRE(slab && !((uintptr_t)slab & 15) && counters, "hawq_incep_conv_group_nib_splitk: slab (16-byte aligned) and counters must be non-null");
    static_assert(sizeof(hawq_incep_group_args) + sizeof(GroupMap) + sizeof(SliceMap) + sizeof(unsigned) + 2 * sizeof(void *) <= 4096, "kernel arguments");
    hipLaunchKernelGGL(incep_group_nib_splitk_kernel, dim3((unsigned)sg.total), dim3(NT), 0, (hipStream_t)stream, *g, sg.gg.mp, sg.sm, (unsigned)mask,
                       (int32_t *)slab, counters);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
