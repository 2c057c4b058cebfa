// Grouped launch of the LDS-tiled InceptionV3 convs with a fan-out epilogue: next to its own output every member may store the
// int8 branch inputs of the NEXT unit, which the plan otherwise makes with one hawq_incep_requant launch per branch from the 16-bit
// concat buffer this epilogue has just written.
//   hawq_incep_conv_group_fan_ok   host arithmetic only: does tile `tile` run this group with these fans in one launch
//   hawq_incep_conv_group_fan      the launch: member i writes, byte for byte, what hawq_incep_conv_tiled(&g->conv[i], tile, s) writes,
//                                  and for j < fan[i].n   to[j].out[p * ldo + c_off + co] = (int8) clamp(dyadic_rne(y; m, ek), lo, hi)
//                                  of the element y it stored (after its last clamp) at pixel p, channel co
// Grid and member selection are incep_group.hip's: one 1-D grid, running totals by value, the member a function of the workgroup id.
// The fan descriptors travel as kernel arguments next to the conv blocks: 1096 (group) + 128 (map) + 1088 (8 fans of 136 bytes) =
// 2312 bytes of the 4096 a launch may carry; member and fan index are wave-uniform, so they arrive through scalar loads.
// A lane holds 16 consecutive channels of one pixel when the epilogue ends (q[16]); a fan output is 16 dyadic_rne + clamp on them,
// four pack4_i8 and one 16-byte store.  Vector stores only.
#include "common.h"

extern "C" int hawq_incep_conv_group_ok(const hawq_incep_group_args *g, int tile);

namespace {

// incep_tiled_kernel's workgroup body as incep_group.hip carries it (incep_tiled_body), line for line, with two changes: the extra
// argument `fn` (the member's fan, wave-uniform) and the loop over its outputs at the end of the epilogue
// (tests/test_incep_fan_host.py compares the texts).  A copy for the reason given there: the existing instantiations keep their code.
template <int BM, int BN, int WPX, int WCH, int KS>
__device__ __forceinline__ void incep_fan_body(const hawq_incep_conv_args &a, const hawq_incep_fan &fn, const int Ho, const int Wo,
                                               const long long pblock, const int cblock, char *lds) {
    constexpr int NT = 64 * WPX * WCH * KS, RSTEP = NT / 4;
    constexpr int WM = BM / WPX / 32, WN = BN / WCH / 32;
    constexpr int APT = BM / RSTEP, BPT = BN / RSTEP, RPT = APT + BPT;
    constexpr int STAGE = (BM + BN) * 64;
    static_assert(BM % RSTEP == 0 && BN % RSTEP == 0 && BM % (32 * WPX) == 0 && BN % (32 * WCH) == 0, "tile shape");
    static_assert(WM * WN > 1, "a wave owns more than one MFMA tile");
    static_assert(KS == 1 || (KS == 2 && WM * WN * 16 * 64 * 4 * WPX * WCH <= 2 * STAGE), "K-split reduction must fit the stages");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int wk = wave / (WPX * WCH), wr = wave % (WPX * WCH), wpx = wr % WPX, wch = wr / WPX;
    const int slot = tid & 3, r0 = tid >> 2;
    const long long P = (long long)a.N * Ho * Wo;
    const int C16 = a.Cin >> 4, K16 = a.KH * a.KW * C16, steps = (K16 + 3) >> 2;
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
    const int8_t *wrow[BPT];
    bool wv[BPT];
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
        const int q = r0 + j * RSTEP, co = cblock + (q & ~31) + cperm(q & 31);
        wv[j] = co < a.Cout;
        wrow[j] = wgt + (wv[j] ? (size_t)co * K16 * 16 : 0);
    }
    // this thread's k16 unit of the step to load next
    int k16 = slot, c16 = k16 % C16, kw = (k16 / C16) % a.KW, kh = (k16 / C16) / a.KW;

    v4i rg[RPT];
    bool ok[RPT];
    const v4i zero = {0, 0, 0, 0};
    // loads are unconditional (a refused element reads the first bytes of its operand) and zeroed when they are written to LDS:
    // no branch around a load, so all RPT of them are in flight together
    auto load = [&]() {
        const bool kv = k16 < K16;
#pragma unroll
        for (int i = 0; i < APT; ++i) {
            const int iy = iy0[i] + kh, ix = ix0[i] + kw;
            ok[i] = kv && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            const size_t off = ok[i] ? ((size_t)iy * a.W + ix) * a.Cin + c16 * 16 : 0;
            rg[i] = *reinterpret_cast<const v4i *>((ok[i] ? abase[i] : in) + off);
        }
#pragma unroll
        for (int j = 0; j < BPT; ++j) {
            ok[APT + j] = kv && wv[j];
            rg[APT + j] = *reinterpret_cast<const v4i *>(wrow[j] + (ok[APT + j] ? (size_t)k16 * 16 : 0));
        }
        k16 += 4, c16 += 4;
        while (c16 >= C16) {
            c16 -= C16;
            if (++kw == a.KW) kw = 0, ++kh;
        }
    };
    auto write = [&](int stage) {
        char *s = lds + stage * STAGE;
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            *reinterpret_cast<v4i *>(s + lds_off(r0 + i * RSTEP, slot)) = ok[i] ? rg[i] : zero;
        }
    };

    v16i acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

    auto compute = [&](int stage) {
        const char *s = lds + stage * STAGE;
#pragma unroll
        for (int t = 0; t < 2 / KS; ++t) {
            const int kk = KS == 2 ? wk : t;   // the 32-byte half of the step
            v4i af[WM], bf[WN];
#pragma unroll
            for (int i = 0; i < WM; ++i)
                af[i] = *reinterpret_cast<const v4i *>(s + lds_off(wpx * 32 * WM + 32 * i + l31, 2 * kk + h));
#pragma unroll
            for (int j = 0; j < WN; ++j)
                bf[j] = *reinterpret_cast<const v4i *>(s + lds_off(BM + wch * 32 * WN + 32 * j + l31, 2 * kk + h));
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(bf[j], af[i], acc[i][j], 0, 0, 0);
        }
    };

    load();
    write(0);
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const bool more = s + 1 < steps;
        if (more) load();          // in flight under the MFMAs of step s
        compute(s & 1);
        if (more) write((s + 1) & 1);   // the other stage: last read in step s - 1, before the barrier that ended it
        __syncthreads();
    }

    if (KS == 2) {   // every wave is past the last barrier: the stages are free
        int *red = reinterpret_cast<int *>(lds);
        if (wk == 1) {
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) red[(((i * WN + j) * 16 + r) * (WPX * WCH) + wr) * 64 + lane] = acc[i][j][r];
        }
        __syncthreads();
        if (wk == 1) return;
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] += red[(((i * WN + j) * 16 + r) * (WPX * WCH) + wr) * 64 + lane];
    }

    // acc[i][j][r] = channel cblock + 32 (wch WN + j) + 16 h + r of pixel pblock + 32 (wpx WM + i) + l31
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        const long long p = pblock + 32 * (wpx * WM + i) + l31;
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int cb = cblock + 32 * (wch * WN + j) + 16 * h;
            if (p >= P || cb >= a.Cout) continue;   // Cout % 16 == 0: the 16 channels of a lane half are all valid or all not
            const size_t row = (size_t)p * a.ldo + a.c_off + cb;   // a multiple of 16 elements (hawq_incep_conv_tile_ok)
            int q[16];
            if (a.epilogue == HAWQ_INCEP_RAW) {
#pragma unroll
                for (int r = 0; r < 16; ++r) q[r] = acc[i][j][r] + a.bias[cb + r];
                v4i *o = reinterpret_cast<v4i *>((int32_t *)a.out + row);
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = v4i{q[4 * r], q[4 * r + 1], q[4 * r + 2], q[4 * r + 3]};
                continue;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cb + r;
                int v = acc[i][j][r] + a.bias[co];
                if (a.relu) v = max(v, 0);
                q[r] = clampi(dyadic_rne(v, a.m[co], a.ek[co]), a.q_lo, a.q_hi);
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
    }
}

// the tiles of hawq_incep_conv_tiled: ids 1 .. NUM_TILES, BM pixels x BN channels (incep_tiled.hip)
enum { NUM_TILES = 4 };
struct TileShape {
    int bm, bn;
};
const TileShape kTiles[NUM_TILES + 1] = {{64, 64}, {128, 128}, {256, 64}, {128, 64}, {64, 32}};

// per member, as in incep_group.hip: end = workgroups of members 0 .. i (INT32_MAX beyond n), npb = pixel blocks, Ho x Wo = output map
struct GroupMap {
    int32_t end[HAWQ_INCEP_GROUP_MAX], npb[HAWQ_INCEP_GROUP_MAX], Ho[HAWQ_INCEP_GROUP_MAX], Wo[HAWQ_INCEP_GROUP_MAX];
};
struct FanSet {
    hawq_incep_fan fan[HAWQ_INCEP_GROUP_MAX];
};

// The occupancy floor is the group kernel's (3 waves per SIMD for the two large tiles, 4 for the others).  Without it the scheduler
// spreads the fan loop's 16 independent requants over 50 more VGPRs than the K loop needs and the kernel loses a wave per SIMD; with
// it the accumulators stay in VGPRs (no AGPR copy) and every instantiation fits: 122 / 156 / 80 / 85 registers, no scratch.
template <int BM, int BN, int WPX, int WCH, int KS>
__global__ __launch_bounds__(64 * WPX * WCH * KS) __attribute__((amdgpu_waves_per_eu(BM * BN >= 128 * 128 ? 3 : 4))) void incep_fan_kernel(hawq_incep_group_args g, GroupMap mp, FanSet fs) {
    const int bid = blockIdx.x;
    int mi = 0, first = 0;   // the member and its first workgroup
#pragma unroll
    for (int j = 0; j < HAWQ_INCEP_GROUP_MAX - 1; ++j) {
        if (bid >= mp.end[j]) mi = j + 1, first = mp.end[j];
    }
    const int local = bid - first, npb = mp.npb[mi];
    __shared__ __attribute__((aligned(16))) char lds[2 * (BM + BN) * 64];
    incep_fan_body<BM, BN, WPX, WCH, KS>(g.conv[mi], fs.fan[mi], mp.Ho[mi], mp.Wo[mi], (long long)(local % npb) * BM, (local / npb) * BN,
                                         lds);
}

struct Span {
    uintptr_t lo, hi;   // bytes [lo, hi)
};
bool meet(const Span &x, const Span &y) { return x.lo < y.hi && y.lo < x.hi; }

// why tile `tile` does not run group `g` with the fans `fan` in one launch (NULL: it does, and `mp` / `total` describe the grid).
// No pointer is dereferenced.  `who`: the member, `which`: its fan output (-1: none in particular).
const char *fan_refusal(const hawq_incep_group_args *g, const hawq_incep_fan *fan, int tile, GroupMap *mp, long long *total, int *who,
                        int *which) {
    *who = *which = -1;
    if (!g || !fan) return "null group or fan list";
    if (tile < 1 || tile > NUM_TILES) return "no such tile (a group runs on one of the ids 1 .. 4)";
    if (!hawq_incep_conv_group_ok(g, tile)) return "the grouped launch refuses the group (hawq_incep_conv_group_ok)";
    const int bm = kTiles[tile].bm, bn = kTiles[tile].bn;
    Span in[HAWQ_INCEP_GROUP_MAX], out[HAWQ_INCEP_GROUP_MAX], fo[HAWQ_INCEP_GROUP_MAX][HAWQ_INCEP_FAN_MAX];
    long long wgs = 0;
    for (int i = 0; i < g->n; ++i) {   // the grid, as hawq_incep_conv_group lays it out (its checks passed above)
        const hawq_incep_conv_args *a = &g->conv[i];
        const int Ho = (a->H + 2 * a->pad_h - a->KH) / a->stride + 1, Wo = (a->W + 2 * a->pad_w - a->KW) / a->stride + 1;
        const long long P = (long long)a->N * Ho * Wo, npb = (P + bm - 1) / bm;
        wgs += npb * ((a->Cout + bn - 1) / bn);
        mp->end[i] = (int32_t)wgs, mp->npb[i] = (int32_t)npb, mp->Ho[i] = Ho, mp->Wo[i] = Wo;
        const size_t es = a->epilogue == HAWQ_INCEP_RAW ? 4 : (size_t)a->out_bits / 8;
        in[i].lo = (uintptr_t)a->in, in[i].hi = in[i].lo + (size_t)a->N * a->H * a->W * a->Cin;
        out[i].lo = (uintptr_t)a->out + (size_t)a->c_off * es;
        out[i].hi = (uintptr_t)a->out + ((size_t)(P - 1) * a->ldo + a->c_off + a->Cout) * es;
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
    for (int i = g->n; i < HAWQ_INCEP_GROUP_MAX; ++i) mp->end[i] = INT32_MAX, mp->npb[i] = 1, mp->Ho[i] = mp->Wo[i] = 0;
    *total = wgs;
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

template <int BM, int BN, int WPX, int WCH, int KS>
void launch(const hawq_incep_group_args *g, const GroupMap &mp, const FanSet &fs, long long total, hipStream_t stream) {
    static_assert(sizeof(hawq_incep_group_args) + sizeof(GroupMap) + sizeof(FanSet) <= 4096, "kernel arguments");
    hipLaunchKernelGGL((incep_fan_kernel<BM, BN, WPX, WCH, KS>), dim3((unsigned)total), dim3(64 * WPX * WCH * KS), 0, stream, *g, mp, fs);
}

}  // namespace

extern "C" int hawq_incep_conv_group_fan_ok(const hawq_incep_group_args *g, const hawq_incep_fan *fan, int tile) {
    GroupMap mp;
    long long total;
    int who, which;
    return fan_refusal(g, fan, tile, &mp, &total, &who, &which) == nullptr;
}

extern "C" int hawq_incep_conv_group_fan(const hawq_incep_group_args *g, const hawq_incep_fan *fan, int tile, void *stream) {
    GroupMap mp;
    long long total = 0;
    int who, which;
    const char *why = fan_refusal(g, fan, tile, &mp, &total, &who, &which);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_group_fan: tile %d refuses the launch (member %d, fan output %d): %s", tile, who, which, why);
    FanSet fs;
    for (int i = 0; i < HAWQ_INCEP_GROUP_MAX; ++i) {
        fs.fan[i] = fan[i < g->n ? i : 0];
        if (i >= g->n) fs.fan[i].n = 0;
    }
    hipStream_t s = (hipStream_t)stream;
    switch (tile) {   // the instantiations of hawq_incep_conv_tiled
        case 1: launch<128, 128, 2, 2, 1>(g, mp, fs, total, s); break;
        case 2: launch<256, 64, 4, 1, 1>(g, mp, fs, total, s); break;
        case 3: launch<128, 64, 2, 2, 1>(g, mp, fs, total, s); break;
        default: launch<64, 32, 1, 1, 2>(g, mp, fs, total, s); break;
    }
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
