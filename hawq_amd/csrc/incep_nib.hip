// Nibble-packed InceptionV3 conv: the launches of hawq_incep_conv (inception.hip) on hawq4 operands, same argument block, same integers.
//   hawq_incep_conv_nib_num_tiles   T: tile ids 1 .. T are the kernels below (there is no id 0)
//   hawq_incep_conv_nib_ok          host arithmetic only: does that tile take this launch
//   hawq_incep_conv_nib             the launch
// in:  unsigned 4-bit activations, hawq4 NHWC rows (Cin / 2 bytes per pixel);  wgt: signed 4-bit, hawq4 [Cout][KH][KW][Cin].
// hawq4 (include/hawq_mi355.h): byte k of an 8-channel dword = c_k | c_{k+4} << 4, so `d & 0x0f0f0f0f` is channels 0 - 3 as int8x4 and
// `(d >> 4) & 0x0f0f0f0f` channels 4 - 7.
//
// Both operands stay packed from HBM through LDS into the fragment registers and become int8x4 MFMA operands only there.
//
// K is the window taps times Cin, walked in units of 16 channels = 8 bytes (two dwords): unit u = tap * Cin/16 + c16 of a pixel, and
// byte 8 u of a weight row.  An LDS row is 64 bytes = 8 units = 128 K values, and that is the K step: the stage of a tile has the
// bytes it has in the int8 kernels ((BM + BN) * 64, two stages, at most 32 KiB), but each barrier now closes four MFMA K blocks per
// fragment pair instead of two.  A thread stages unit (t & 7) of rows (t >> 3) + i * NT/8 with 8-byte loads into registers while the
// previous step's MFMAs run and writes them with ds_write_b64 afterwards; the unit, not the 16-byte slot, is what it owns, because
// with an odd Cin/16 (16, 48, 80 ...) the two units of a slot lie in different taps - one of them may be padding - and a unit is
// the largest run that is always one tap.  Units beyond K (an odd unit count: the last MFMA is half empty) and taps outside the
// image are staged as zero bytes, which widen to exact zeros on both sides.
//
// Fragment reads are ds_read_b128: lane (l31, h) reads the 16-byte slot 2 t + h of row l31 (t = 0, 1), that is units 4 t + 2 h and
// 4 t + 2 h + 1, and issues two MFMAs from it - the first on the even unit of every lane, the second on the odd one.  An MFMA K block
// is therefore units {4 t, 4 t + 2} and then {4 t + 1, 4 t + 3}: K is summed, both operands use the same lane map, so the order of K
// inside a step is free, and a 16-byte read per lane keeps the bank pattern of 64-byte rows with the slot XOR-swizzled by
// (row >> 2) & 3 (common.h lds_off) conflict-free, as in the int8 kernels; an 8-byte read per MFMA would take twice the LDS
// instructions.  The staging writes of 8 lanes fill one 64-byte row, 32 lanes four rows = all 64 banks once.
//
// Widening (VALU per dword: 3 on either side).  Activations zero-extend: d & M, (d >> 4) & M.  Weights are fed as nibble << 4, the
// int8 value 16 w with the nibble's sign bit as the byte's: (d << 4) & ~M, d & ~M.  The accumulator is then exactly 16 times the
// int8-container sum and is shifted right by 4 in front of the bias.  16 * 15 * 8 * K < 2^31 is proved on the host from the shape
// alone (hawq_incep_conv_nib_ok: K = KH KW Cin <= 1118481; |w| <= 8, a <= 15), so no layer needs its weights read.  A true sign
// extension costs two more instructions per dword (xor 8, subtract 8 per byte).  A fragment is widened once per unit and used by
// every MFMA of its row or column of the wave tile: 12 (WM + WN) instructions per 2 WM WN MFMAs, 6 per MFMA on a 64 x 64 wave tile
// and 9 on a 64 x 32 one, against the 16 passes of a 32x32x32 MFMA.
//
// Weight rows are staged in cperm order (LDS row q of a 32-row group holds channel cperm(q)), so lane half h ends up with the 16
// consecutive channels 16 h .. 16 h + 15 of one pixel - one 8-byte store of hawq4, 16 bytes of int8, 32 of int16, 64 of int32.
#include "common.h"

namespace {

// tile ids 1 .. NUM_NIB_TILES: BM pixels x BN channels per workgroup, 256 threads each
//   1  128 px x 128 ch, 4 waves of 64 x 64                    the 147^2 .. 35^2 maps with 96 and more output channels
//   2  128 px x  64 ch, 4 waves of 64 x 32                    32 .. 64 output channels, and the 17^2 maps (289 px = 2.3 tiles an image)
//   3   64 px x  64 ch, 2 x 2 waves of 32 x 64 that split K   the 8^2 maps (one image = one pixel tile) at batch 1 - 16
enum { NUM_NIB_TILES = 3 };
struct NibShape {
    int bm, bn;
};
constexpr NibShape kNib[NUM_NIB_TILES + 1] = {{0, 0}, {128, 128}, {128, 64}, {64, 64}};
// 16 (weights as nibble << 4) * 15 * 8 * K <= 2^31 - 1
constexpr long long NIB_K_MAX = ((1ll << 31) - 1) / (16 * 15 * 8);

constexpr int NIB_LO = 0x0f0f0f0f, NIB_HI = (int)0xf0f0f0f0u;
// one unit (dwords d0, d1 = channels 0 - 7, 8 - 15) -> the 16 int8 of an MFMA operand, in channel order
__device__ __forceinline__ v4i widen_act(int d0, int d1) {
    return v4i{d0 & NIB_LO, (int)((unsigned)d0 >> 4) & NIB_LO, d1 & NIB_LO, (int)((unsigned)d1 >> 4) & NIB_LO};
}
// 16 w per byte
__device__ __forceinline__ v4i widen_wgt(int d0, int d1) { return v4i{(d0 << 4) & NIB_HI, d0 & NIB_HI, (d1 << 4) & NIB_HI, d1 & NIB_HI}; }

template <int BM, int BN, int WPX, int WCH, int KS>
__global__ __launch_bounds__(64 * WPX * WCH * KS) void incep_nib_kernel(hawq_incep_conv_args a, int Ho, int Wo) {
    constexpr int NT = 64 * WPX * WCH * KS, RSTEP = NT / 8;
    constexpr int WM = BM / WPX / 32, WN = BN / WCH / 32;
    constexpr int APT = BM / RSTEP, BPT = BN / RSTEP, RPT = APT + BPT;
    constexpr int STAGE = (BM + BN) * 64;
    static_assert(BM % RSTEP == 0 && BN % RSTEP == 0 && BM % (32 * WPX) == 0 && BN % (32 * WCH) == 0, "tile shape");
    static_assert(KS == 1 || (KS == 2 && WM * WN * 16 * 64 * 4 * WPX * WCH <= 2 * STAGE), "K-split reduction must fit the stages");
    __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int wk = wave / (WPX * WCH), wr = wave % (WPX * WCH), wpx = wr % WPX, wch = wr / WPX;
    const int unit = tid & 7, r0 = tid >> 3;
    const long long P = (long long)a.N * Ho * Wo, pblock = (long long)blockIdx.x * BM;
    const int cblock = blockIdx.y * BN;
    const int C16 = a.Cin >> 4, K16 = a.KH * a.KW * C16, steps = (K16 + 7) >> 3;
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
    // this thread's unit of the step to load next
    int k16 = unit, c16 = k16 % C16, kw = (k16 / C16) % a.KW, kh = (k16 / C16) / a.KW;

    v2i rg[RPT];
    bool ok[RPT];
    const v2i zero = {0, 0};
    // loads are unconditional (a refused unit reads the first 8 bytes of its operand) and zeroed when they are written to LDS
    auto load = [&]() {
        const bool kv = k16 < K16;
#pragma unroll
        for (int i = 0; i < APT; ++i) {
            const int iy = iy0[i] + kh, ix = ix0[i] + kw;
            ok[i] = kv && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            const size_t off = ok[i] ? ((size_t)iy * a.W + ix) * pix_bytes + c16 * 8 : 0;
            rg[i] = *reinterpret_cast<const v2i *>((ok[i] ? abase[i] : in) + off);
        }
#pragma unroll
        for (int j = 0; j < BPT; ++j) {
            ok[APT + j] = kv && wv[j];
            rg[APT + j] = *reinterpret_cast<const v2i *>(wrow[j] + (ok[APT + j] ? (size_t)k16 * 8 : 0));
        }
        k16 += 8, c16 += 8;
        while (c16 >= C16) {
            c16 -= C16;
            if (++kw == a.KW) kw = 0, ++kh;
        }
    };
    auto write = [&](int stage) {
        char *s = lds + stage * STAGE;
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            *reinterpret_cast<v2i *>(s + lds_off(r0 + i * RSTEP, unit >> 1) + 8 * (unit & 1)) = ok[i] ? rg[i] : zero;
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
            const int tt = KS == 2 ? wk : t;   // the 32-byte half of the row
            v4i af[WM], bf[WN];
#pragma unroll
            for (int i = 0; i < WM; ++i)
                af[i] = *reinterpret_cast<const v4i *>(s + lds_off(wpx * 32 * WM + 32 * i + l31, 2 * tt + h));
#pragma unroll
            for (int j = 0; j < WN; ++j)
                bf[j] = *reinterpret_cast<const v4i *>(s + lds_off(BM + wch * 32 * WN + 32 * j + l31, 2 * tt + h));
#pragma unroll
            for (int u = 0; u < 2; ++u) {   // the even unit of every lane's slot, then the odd one
                v4i wa[WM], wb[WN];
#pragma unroll
                for (int i = 0; i < WM; ++i) wa[i] = widen_act(af[i][2 * u], af[i][2 * u + 1]);
#pragma unroll
                for (int j = 0; j < WN; ++j) wb[j] = widen_wgt(bf[j][2 * u], bf[j][2 * u + 1]);
#pragma unroll
                for (int i = 0; i < WM; ++i)
#pragma unroll
                    for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wb[j], wa[i], acc[i][j], 0, 0, 0);
            }
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

    // acc[i][j][r] = 16 x channel cblock + 32 (wch WN + j) + 16 h + r of pixel pblock + 32 (wpx WM + i) + l31
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        const long long p = pblock + 32 * (wpx * WM + i) + l31;
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int cb = cblock + 32 * (wch * WN + j) + 16 * h;
            if (p >= P || cb >= a.Cout) continue;   // Cout % 16 == 0: the 16 channels of a lane half are all valid or all not
            const size_t row = (size_t)p * a.ldo + a.c_off + cb;   // a multiple of 16 elements (hawq_incep_conv_nib_ok)
            int q[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) q[r] = (acc[i][j][r] >> 4) + a.bias[cb + r];   // the sum is an exact multiple of 16
            if (a.epilogue == HAWQ_INCEP_RAW) {
                v4i *o = reinterpret_cast<v4i *>((int32_t *)a.out + row);
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = v4i{q[4 * r], q[4 * r + 1], q[4 * r + 2], q[4 * r + 3]};
                continue;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cb + r;
                if (a.relu) q[r] = max(q[r], 0);
                q[r] = clampi(dyadic_rne(q[r], a.m[co], a.ek[co]), a.q_lo, a.q_hi);
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
            } else if (a.out_bits == 8) {
                v4i d;
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = (int)pack4_i8(q[4 * e], q[4 * e + 1], q[4 * e + 2], q[4 * e + 3]);
                *reinterpret_cast<v4i *>((int8_t *)a.out + row) = d;
            } else {   // hawq4: 16 channels = two dwords at byte row / 2
                *reinterpret_cast<v2i *>((char *)a.out + (row >> 1)) = v2i{(int)pack8_u4(q), (int)pack8_u4(q + 8)};
            }
        }
    }
}

struct Geo {
    int Ho, Wo;
    long long P;
};

// why no nibble tile takes this block (NULL: it is well formed).  No pointer is dereferenced.
const char *refusal(const hawq_incep_conv_args *a, Geo *g) {
    if (!a || !a->in || !a->wgt || !a->bias || !a->out) return "null pointer";
    if (!(a->N > 0 && a->H > 0 && a->W > 0 && a->Cin > 0 && a->Cout > 0 && a->Cin % 16 == 0 && a->Cout % 16 == 0))
        return "bad shape (channels must be multiples of 16)";
    if (!(a->KH >= 1 && a->KH <= 7 && a->KW >= 1 && a->KW <= 7 && (a->stride == 1 || a->stride == 2))) return "window or stride not supported";
    if (!(a->pad_h >= 0 && a->pad_w >= 0 && 2 * a->pad_h < a->KH + 1 && 2 * a->pad_w < a->KW + 1)) return "padding too large for the window";
    g->Ho = (a->H + 2 * a->pad_h - a->KH) / a->stride + 1, g->Wo = (a->W + 2 * a->pad_w - a->KW) / a->stride + 1;
    if (!(g->Ho > 0 && g->Wo > 0)) return "empty output";
    if (!(a->c_off >= 0 && a->ldo >= a->c_off + a->Cout)) return "ldo < c_off + Cout";
    if ((long long)a->KH * a->KW * a->Cin > NIB_K_MAX) return "K too long: 16 * 15 * 8 * KH KW Cin must fit int32 (weights are fed as 16 w)";
    if (a->epilogue == HAWQ_INCEP_REQUANT || a->epilogue == HAWQ_INCEP_REQUANT2) {
        if (!a->m || !a->ek) return "requant tables missing";
        if (a->out_bits != 4 && a->out_bits != 8 && a->out_bits != 16) return "out_bits must be 4, 8 or 16";
        const int lo = a->out_bits == 4 ? 0 : a->out_bits == 8 ? -128 : -32768, hi = a->out_bits == 4 ? 15 : a->out_bits == 8 ? 127 : 32767;
        if (!(a->q_lo >= lo && a->q_hi <= hi && a->q_lo <= a->q_hi &&
              (a->epilogue != HAWQ_INCEP_REQUANT2 || (a->q2_lo >= lo && a->q2_hi <= hi && a->q2_lo <= a->q2_hi))))
            return "clamp bounds outside the store (out_bits 4 holds 0 .. 15)";
    } else if (a->epilogue != HAWQ_INCEP_RAW) {
        return "unknown epilogue";
    } else if (a->out_bits == 4) {
        return "a RAW epilogue stores int32: out_bits 4 needs REQUANT or REQUANT2";
    }
    if (a->ldo % 16 || a->c_off % 16 || ((uintptr_t)a->out & 15) || ((uintptr_t)a->in & 15) || ((uintptr_t)a->wgt & 15))
        return "out, in, wgt must be 16-byte aligned, ldo and c_off multiples of 16";
    g->P = (long long)a->N * g->Ho * g->Wo;
    if ((g->P + 63) / 64 >= (1ll << 31) || a->Cout / 64 > 65534) return "too many output pixels or channels for the grid";
    return nullptr;
}

// why tile `tile` (1 .. NUM_NIB_TILES) does not take a well-formed launch (NULL: it does)
const char *tile_refusal(const hawq_incep_conv_args *a, int tile) {
    if (tile == 1 && a->Cout <= 64) return "the 128-channel tile is for more than 64 output channels";
    if (tile == 3 && a->KH * a->KW * a->Cin < 512) return "the K-split tile is for K >= 512";
    return nullptr;
}

template <int BM, int BN, int WPX, int WCH, int KS>
void launch(const hawq_incep_conv_args *a, const Geo &g, hipStream_t stream) {
    dim3 grid((unsigned)((g.P + BM - 1) / BM), (unsigned)((a->Cout + BN - 1) / BN));
    hipLaunchKernelGGL((incep_nib_kernel<BM, BN, WPX, WCH, KS>), grid, dim3(64 * WPX * WCH * KS), 0, stream, *a, g.Ho, g.Wo);
}

}  // namespace

extern "C" int hawq_incep_conv_nib_num_tiles(void) { return NUM_NIB_TILES; }

extern "C" int hawq_incep_conv_nib_ok(const hawq_incep_conv_args *a, int tile) {
    Geo g;
    return tile >= 1 && tile <= NUM_NIB_TILES && !refusal(a, &g) && !tile_refusal(a, tile);
}

extern "C" int hawq_incep_conv_nib(const hawq_incep_conv_args *a, int tile, void *stream) {
    HAWQ_REQUIRE(tile >= 1 && tile <= NUM_NIB_TILES, "hawq_incep_conv_nib: no tile %d (ids 1 .. %d)", tile, NUM_NIB_TILES);
    Geo g;
    const char *why = refusal(a, &g);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_nib: %s", why);
    why = tile_refusal(a, tile);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_nib: tile %d (%d px x %d ch) refuses the launch: %s", tile, kNib[tile].bm, kNib[tile].bn, why);
    hipStream_t s = (hipStream_t)stream;
    if (tile == 1) launch<128, 128, 2, 2, 1>(a, g, s);
    else if (tile == 2) launch<128, 64, 2, 2, 1>(a, g, s);
    else launch<64, 64, 2, 1, 2>(a, g, s);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
