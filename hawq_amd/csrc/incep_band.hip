// LDS-band 3x3 / stride 1 conv for narrow inputs (Cin <= 96): the stem convs of InceptionV3 (hawq_incep_conv_band), on
// hawq_incep_conv's argument block and with its arithmetic - the bytes written are hawq_incep_conv's.
//
// The tiled kernels (incep_tiled.hip) gather every 16-channel unit of every tap from global memory and pass a barrier per 64 bytes
// of K.  Here a workgroup (4 waves) owns a BAND of one image: R output rows x 32 output columns, and
//   * stages the band's input halo, (R + 2) x 34 pixels of Cin bytes, in LDS once (16-byte loads; positions outside the map are
//     zeros, which is the padding), so the nine taps are LDS address offsets: no gather, no barrier inside the K loop;
//   * keeps the weights of its BN output channels in LDS for every band it walks ([Cout][3][3][Cin] rows as they are, rows in cperm
//     order so that a lane half ends up with 16 consecutive channels);
//   * walks bands blockIdx.x, + gridDim.x, ...: the next band's halo is loaded to registers in front of the MFMAs of the current
//     one and written to LDS behind them (two barriers per band).
// Wave w computes output rows w * WM .. + WM - 1 of the band (one 32-pixel MFMA tile per row) times WN 32-channel tiles, K walked in
// 16-channel units u = tap * Cin/16 + c16, two per v_mfma_i32_32x32x32_i8 (lane half h takes unit 2 s + h).  Cin/16 is a template
// constant, so every fragment address is the lane's base plus a compile-time offset; with an odd Cin/16 the two units of a step can
// lie in different taps (the offset is then a select between two constants) and the last step has one unit only: lane half 1 reads
// that unit again against zero weights.  Rows i and i + 1 of a wave read the same input rows at taps kh and kh - 1: the same
// address expressions, one LDS read.
// LDS rows are padded to an odd number of 16-byte units where that fits (pixel stride Cin + 16 for Cin = 32, 64; weight row 9 Cin
// + 16 for an even unit count): the 16 lanes of a ds_read_b128 group then hit 16 distinct bank quads.  At most 64 KB per workgroup.
#include "common.h"

extern "C" int hawq_incep_conv_tile_ok(const hawq_incep_conv_args *a, int tile);

namespace {

constexpr int CW = 32, BC = CW + 2;   // output columns of a band, and the input columns under them
constexpr int MAX_WGS = 1024;         // workgroups of a launch, all channel blocks together: bands beyond that are walked

// per Cin / 16: output channels per workgroup, output rows per band, padding bytes of a pixel in LDS
struct BandShape {
    int bn, r, pad;
};
constexpr BandShape kBand[7] = {{0, 0, 0}, {64, 8, 0}, {64, 8, 16}, {64, 8, 0}, {64, 8, 16}, {64, 4, 0}, {32, 8, 0}};

template <int C16, int BN, int R, int PAD>
__global__ __launch_bounds__(256) void incep_band_kernel(hawq_incep_conv_args a, int Ho, int Wo, int nrb, int ncb, int nbands) {
    constexpr int U = 9 * C16, S = (U + 1) / 2, CIN = 16 * C16, PS = CIN + PAD, WROW = (U | 1) * 16;
    constexpr int WM = R / 4, WN = BN / 32, NQ = (R + 2) * BC * C16, NCH = (NQ + 255) / 256;
    static_assert(BN * WROW + (R + 2) * BC * PS <= 65536, "two workgroups share a CU's LDS");
    static_assert(WM * WN > 1, "a wave owns more than one MFMA tile");
    __shared__ __attribute__((aligned(16))) char wl[BN * WROW];            // weight row q: channel cblock + (q & ~31) + cperm(q & 31)
    __shared__ __attribute__((aligned(16))) char bl[(R + 2) * BC * PS];    // the halo: [row][column] pixels of PS bytes

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int cblock = blockIdx.y * BN;
    const int8_t *in = (const int8_t *)a.in, *wgt = (const int8_t *)a.wgt;
    const v4i zero = {0, 0, 0, 0};

    for (int j = tid; j < BN * U; j += 256) {
        const int q = j / U, u = j - q * U, co = cblock + (q & ~31) + cperm(q & 31);
        v4i w = zero;
        if (co < a.Cout) w = *reinterpret_cast<const v4i *>(wgt + ((size_t)co * U + u) * 16);
        *reinterpret_cast<v4i *>(wl + q * WROW + u * 16) = w;
    }

    // chunk q = tid + 256 k of a halo: 16 channels c of pixel (row, col); loads are unconditional (a refused chunk reads the first
    // bytes of the input) and zeroed when they are written to LDS, as in the tiled kernels
    v4i rg[NCH];
    unsigned okm = 0;
    auto load = [&](int band) {
        const int cb = band % ncb, t2 = band / ncb, rb = t2 % nrb, n = t2 / nrb;
        const int iy0 = rb * R - a.pad_h, ix0 = cb * CW - a.pad_w;
        const int8_t *img = in + (size_t)n * a.H * a.W * CIN;
        okm = 0;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int q = tid + 256 * k, c = q % C16, pos = q / C16, col = pos % BC, row = pos / BC;
            const int iy = iy0 + row, ix = ix0 + col;
            const bool ok = q < NQ && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            const size_t off = ok ? ((size_t)iy * a.W + ix) * CIN + c * 16 : 0;
            rg[k] = *reinterpret_cast<const v4i *>((ok ? img : in) + off);
            okm |= (unsigned)ok << k;
        }
    };
    auto write = [&]() {
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int q = tid + 256 * k, c = q % C16, pos = q / C16;
            if (q < NQ) *reinterpret_cast<v4i *>(bl + pos * PS + c * 16) = ((okm >> k) & 1) ? rg[k] : zero;
        }
    };

    // byte offset of K unit u in the halo, from the pixel under tap (0, 0)
    auto aoff = [](int u) {
        const int tap = u / C16, c = u % C16;
        return ((tap / 3) * BC + tap % 3) * PS + c * 16;
    };
    const char *abase = bl + ((wave * WM) * BC + l31) * PS + (C16 % 2 == 0 ? 16 * h : 0);
    const char *bbase = wl + l31 * WROW;

    int band = blockIdx.x;   // the grid holds no more workgroups than bands
    load(band);
    write();
    for (;;) {
        __syncthreads();   // the halo (and, the first time, the weights) is in LDS
        const int next = band + gridDim.x;
        const bool more = next < nbands;
        if (more) load(next);   // in flight under the MFMAs

        v16i acc[WM][WN];
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int u0 = 2 * s, u1 = 2 * s + 1 < U ? 2 * s + 1 : u0;   // the odd tail: unit u0 again, against zero weights
            const int ao = C16 % 2 == 0 ? aoff(u0) : (h ? aoff(u1) : aoff(u0));
            const int bo = (h ? u1 : u0) * 16;
            v4i af[WM], bf[WN];
#pragma unroll
            for (int i = 0; i < WM; ++i) af[i] = *reinterpret_cast<const v4i *>(abase + i * BC * PS + ao);
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                bf[j] = *reinterpret_cast<const v4i *>(bbase + 32 * j * WROW + bo);
                if (2 * s + 1 >= U && h) bf[j] = zero;
            }
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(bf[j], af[i], acc[i][j], 0, 0, 0);
        }
        __syncthreads();   // every wave has read this band's halo
        if (more) write();

        // acc[i][j][r] = channel cblock + 32 j + 16 h + r of pixel (row wave WM + i, column l31) of the band; hawq_incep_conv's
        // epilogue, statement for statement
        const int cb = band % ncb, t2 = band / ncb, rb = t2 % nrb, n = t2 / nrb;
        const int ox = cb * CW + l31;
#pragma unroll
        for (int i = 0; i < WM; ++i) {
            const int oy = rb * R + wave * WM + i;
            const long long p = ((long long)n * Ho + oy) * Wo + ox;
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                const int cbk = cblock + 32 * j + 16 * h;
                if (oy >= Ho || ox >= Wo || cbk >= a.Cout) continue;   // Cout % 16 == 0: a lane half's 16 channels are valid or not
                const size_t row = (size_t)p * a.ldo + a.c_off + cbk;   // a multiple of 16 elements (hawq_incep_conv_band_ok)
                int q[16];
                if (a.epilogue == HAWQ_INCEP_RAW) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) q[r] = acc[i][j][r] + a.bias[cbk + r];
                    v4i *o = reinterpret_cast<v4i *>((int32_t *)a.out + row);
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = v4i{q[4 * r], q[4 * r + 1], q[4 * r + 2], q[4 * r + 3]};
                    continue;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = cbk + r;
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
        if (!more) break;
        band = next;
    }
}

// why the band kernel does not take a launch (NULL: it does).  No pointer is dereferenced.
const char *band_refusal(const hawq_incep_conv_args *a) {
    if (!hawq_incep_conv_tile_ok(a, 0)) return "hawq_incep_conv refuses the launch";
    if (a->KH != 3 || a->KW != 3 || a->stride != 1) return "only 3x3 windows at stride 1";
    if (a->pad_h != a->pad_w || a->pad_h > 1) return "padding must be 0 or 1, the same in both directions";
    if (a->Cin > 96) return "Cin must be at most 96";
    if (a->ldo % 16 || a->c_off % 16 || ((uintptr_t)a->out & 15) || ((uintptr_t)a->in & 15) || ((uintptr_t)a->wgt & 15))
        return "16-byte runs: out, in, wgt 16-byte aligned, ldo and c_off multiples of 16";
    if (a->epilogue == HAWQ_INCEP_RAW && a->out_bits != 32) return "a RAW epilogue stores 32 bits";
    return nullptr;
}

template <int C16>
void launch(const hawq_incep_conv_args *a, hipStream_t stream) {
    constexpr BandShape s = kBand[C16];
    const int Ho = a->H + 2 * a->pad_h - 2, Wo = a->W + 2 * a->pad_w - 2;
    const int nrb = (Ho + s.r - 1) / s.r, ncb = (Wo + CW - 1) / CW;
    const long long nbands = (long long)a->N * nrb * ncb;   // <= the output pixels, which hawq_incep_conv bounds below 2^37 ...
    const int gy = (a->Cout + s.bn - 1) / s.bn, cap = MAX_WGS / gy > 0 ? MAX_WGS / gy : 1;
    dim3 grid((unsigned)(nbands < cap ? nbands : cap), (unsigned)gy);
    hipLaunchKernelGGL((incep_band_kernel<C16, s.bn, s.r, s.pad>), grid, dim3(256), 0, stream, *a, Ho, Wo, nrb, ncb, (int)nbands);
}

// ... and the kernel counts bands in an int
bool bands_fit(const hawq_incep_conv_args *a) {
    const int r = kBand[a->Cin >> 4].r;
    const long long Ho = a->H + 2 * a->pad_h - 2, Wo = a->W + 2 * a->pad_w - 2;
    return a->N * ((Ho + r - 1) / r) * ((Wo + CW - 1) / CW) < (1ll << 31) - MAX_WGS;
}

}  // namespace

extern "C" int hawq_incep_conv_band_ok(const hawq_incep_conv_args *a) {
    const char *why = band_refusal(a);
    if (!why && !bands_fit(a)) why = "too many bands";
    if (why) hawq_set_error("hawq_incep_conv_band: %s", why);
    return why ? 0 : 1;
}

extern "C" int hawq_incep_conv_band(const hawq_incep_conv_args *a, void *stream) {
    const char *why = band_refusal(a);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_band: %s", why);
    HAWQ_REQUIRE(bands_fit(a), "hawq_incep_conv_band: too many bands");
    switch (a->Cin >> 4) {
        case 1: launch<1>(a, (hipStream_t)stream); break;
        case 2: launch<2>(a, (hipStream_t)stream); break;
        case 3: launch<3>(a, (hipStream_t)stream); break;
        case 4: launch<4>(a, (hipStream_t)stream); break;
        case 5: launch<5>(a, (hipStream_t)stream); break;
        default: launch<6>(a, (hipStream_t)stream); break;
    }
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
