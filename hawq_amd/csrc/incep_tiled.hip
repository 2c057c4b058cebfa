// LDS-tiled variants of the InceptionV3 rectangular conv (inception.hip: hawq_incep_conv), same argument block, same arithmetic:
//   hawq_incep_conv_num_tiles   T: tile ids 1 .. T are the kernels below, id 0 is hawq_incep_conv's kernel
//   hawq_incep_conv_tile_ok     host arithmetic only: does that tile take this launch
//   hawq_incep_conv_tiled       the launch
// The sums are integers, so every tile computes exactly what tile 0 computes; the epilogue is tile 0's, statement for statement.
//
// K is the window taps times Cin, walked in units of 16 channels ("k16" = one 16-byte run of a weight row / of an input pixel): weight
// rows [KH][KW][Cin] are contiguous in that order, so k16 unit u of a row is at byte 16 u, and for the activations u = tap * Cin/16 + c16
// names the tap (kh, kw) and the channel run.  A K step is four units = 64 bytes per row: one tap x 64 channels when Cin % 64 == 0, and
// parts of neighbouring taps otherwise (Cin = 32: two taps per step; Cin = 48, 80: runs of both) - no MFMA column is spent on padding
// except in the last step of a K that is not a multiple of 64.  Units beyond K and taps outside the image are zeros.
//
// Per step a workgroup stages BM pixel rows and BN weight rows of 64 bytes into one of two LDS stages: thread t owns unit (t & 3) of
// rows (t >> 2) + i * NT/4, loads 16 bytes per row to registers while the MFMAs of the previous step run, and writes them with
// ds_write_b128 afterwards (one barrier per step).  Register staging, not LDS-DMA: a tap that falls into the padding must become
// zeros, and the DMA can only copy.  Rows are 64 bytes with the 16-byte slot XOR-swizzled by (row >> 2) & 3 (common.h lds_off): the
// ds_read_b128 fragment reads of 32 consecutive rows are conflict-free in each of the instruction's four 16-lane groups.
// Weight rows are staged in cperm order (LDS row q of a 32-row group holds channel cperm(q)), so lane half h ends up with the 16
// consecutive channels 16 h .. 16 h + 15 of one pixel, as in tile 0 - and stores them as whole 16-byte runs.
#include "common.h"

extern "C" int hawq_incep_conv(const hawq_incep_conv_args *a, void *stream);

namespace {

// BM pixels x BN channels per workgroup; WPX x WCH waves tile it, each with (BM / WPX / 32) x (BN / WCH / 32) MFMA tiles;
// KS = 2: two such wave sets split every K step between them (32 bytes each) and add their accumulators through LDS at the end.
template <int BM, int BN, int WPX, int WCH, int KS>
__global__ __launch_bounds__(64 * WPX * WCH * KS) void incep_tiled_kernel(hawq_incep_conv_args a, int Ho, int Wo) {
    constexpr int NT = 64 * WPX * WCH * KS, RSTEP = NT / 4;
    constexpr int WM = BM / WPX / 32, WN = BN / WCH / 32;
    constexpr int APT = BM / RSTEP, BPT = BN / RSTEP, RPT = APT + BPT;
    constexpr int STAGE = (BM + BN) * 64;
    static_assert(BM % RSTEP == 0 && BN % RSTEP == 0 && BM % (32 * WPX) == 0 && BN % (32 * WCH) == 0, "tile shape");
    static_assert(WM * WN > 1, "a wave owns more than one MFMA tile");
    static_assert(KS == 1 || (KS == 2 && WM * WN * 16 * 64 * 4 * WPX * WCH <= 2 * STAGE), "K-split reduction must fit the stages");
    __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int wk = wave / (WPX * WCH), wr = wave % (WPX * WCH), wpx = wr % WPX, wch = wr / WPX;
    const int slot = tid & 3, r0 = tid >> 2;
    const long long P = (long long)a.N * Ho * Wo;
    const long long pblock = (long long)blockIdx.x * BM;
    const int cblock = blockIdx.y * BN;
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
        }
    }
}

// tile ids 1 .. NUM_TILES
//   1  128 px x 128 ch, 4 waves of 64 x 64   the 147^2 .. 35^2 maps with 96 and more output channels
//   2  256 px x  64 ch, 4 waves of 64 x 64   the large maps with 32 .. 64 output channels (and 80 / 192 in two passes)
//   3  128 px x  64 ch, 4 waves of 64 x 32   the 17^2 maps
//   4   64 px x  32 ch, 2 waves of 64 x 32 that split K: the 8 x 8 maps at batch 1 - 16 (one image = one pixel tile, twice the
//      workgroups of a 64-channel tile)
enum { NUM_TILES = 4 };
struct TileShape {
    int bm, bn;
};
const TileShape kTiles[NUM_TILES + 1] = {{64, 64}, {128, 128}, {256, 64}, {128, 64}, {64, 32}};

struct Geo {
    int Ho, Wo;
    long long P;
};

// hawq_incep_conv's own argument checks, as a reason (NULL: the launch is well formed).  No pointer is dereferenced.
const char *refusal(const hawq_incep_conv_args *a, Geo *g) {
    if (!a || !a->in || !a->wgt || !a->bias || !a->out) return "null pointer";
    if (!(a->N > 0 && a->H > 0 && a->W > 0 && a->Cin > 0 && a->Cout > 0 && a->Cin % 16 == 0 && a->Cout % 16 == 0))
        return "bad shape (channels must be multiples of 16)";
    if (!(a->KH >= 1 && a->KH <= 7 && a->KW >= 1 && a->KW <= 7 && (a->stride == 1 || a->stride == 2))) return "window or stride not supported";
    if (!(a->pad_h >= 0 && a->pad_w >= 0 && 2 * a->pad_h < a->KH + 1 && 2 * a->pad_w < a->KW + 1)) return "padding too large for the window";
    g->Ho = (a->H + 2 * a->pad_h - a->KH) / a->stride + 1, g->Wo = (a->W + 2 * a->pad_w - a->KW) / a->stride + 1;
    if (!(g->Ho > 0 && g->Wo > 0)) return "empty output";
    if (!(a->c_off >= 0 && a->ldo >= a->c_off + a->Cout)) return "ldo < c_off + Cout";
    if (a->epilogue == HAWQ_INCEP_REQUANT || a->epilogue == HAWQ_INCEP_REQUANT2) {
        if (!a->m || !a->ek) return "requant tables missing";
        if (a->out_bits != 8 && a->out_bits != 16) return "out_bits must be 8 or 16";
        const int lim = a->out_bits == 16 ? 32767 : 127;
        if (!(a->q_lo >= -lim - 1 && a->q_hi <= lim && a->q_lo <= a->q_hi &&
              (a->epilogue != HAWQ_INCEP_REQUANT2 || (a->q2_lo >= -lim - 1 && a->q2_hi <= lim && a->q2_lo <= a->q2_hi))))
            return "clamp bounds outside the store";
    } else if (a->epilogue != HAWQ_INCEP_RAW) {
        return "unknown epilogue";
    }
    g->P = (long long)a->N * g->Ho * g->Wo;
    if ((g->P + 63) / 64 >= (1ll << 31)) return "too many output pixels";
    return nullptr;
}

// why tile `tile` (1 .. NUM_TILES) does not take a well-formed launch (NULL: it does)
const char *tile_refusal(const hawq_incep_conv_args *a, int tile) {
    if (a->ldo % 16 || a->c_off % 16 || ((uintptr_t)a->out & 15) || ((uintptr_t)a->in & 15) || ((uintptr_t)a->wgt & 15))
        return "the tiled kernels store 16-byte runs: out, in, wgt 16-byte aligned, ldo and c_off multiples of 16";
    if (tile == 1 && a->Cout <= 64) return "the 128-channel tile is for more than 64 output channels";
    if (tile == 4 && a->KH * a->KW * a->Cin < 512) return "the K-split tile is for K >= 512";
    return nullptr;
}

template <int BM, int BN, int WPX, int WCH, int KS>
void launch(const hawq_incep_conv_args *a, const Geo &g, hipStream_t stream) {
    dim3 grid((unsigned)((g.P + BM - 1) / BM), (unsigned)((a->Cout + BN - 1) / BN));
    hipLaunchKernelGGL((incep_tiled_kernel<BM, BN, WPX, WCH, KS>), grid, dim3(64 * WPX * WCH * KS), 0, stream, *a, g.Ho, g.Wo);
}

}  // namespace

extern "C" int hawq_incep_conv_num_tiles(void) { return NUM_TILES; }

extern "C" int hawq_incep_conv_tile_ok(const hawq_incep_conv_args *a, int tile) {
    Geo g;
    if (tile < 0 || tile > NUM_TILES || refusal(a, &g)) return 0;
    return tile == 0 || !tile_refusal(a, tile);
}

extern "C" int hawq_incep_conv_tiled(const hawq_incep_conv_args *a, int tile, void *stream) {
    if (tile == 0) return hawq_incep_conv(a, stream);
    HAWQ_REQUIRE(tile > 0 && tile <= NUM_TILES, "hawq_incep_conv_tiled: no tile %d (ids 0 .. %d)", tile, NUM_TILES);
    Geo g;
    const char *why = refusal(a, &g);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_tiled: %s", why);
    why = tile_refusal(a, tile);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_tiled: tile %d (%d px x %d ch) refuses the launch: %s", tile, kTiles[tile].bm, kTiles[tile].bn, why);
    hipStream_t s = (hipStream_t)stream;
    switch (tile) {
        case 1: launch<128, 128, 2, 2, 1>(a, g, s); break;
        case 2: launch<256, 64, 4, 1, 1>(a, g, s); break;
        case 3: launch<128, 64, 2, 2, 1>(a, g, s); break;
        default: launch<64, 32, 1, 1, 2>(a, g, s); break;
    }
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
