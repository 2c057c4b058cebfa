// Stem, pooling and small tail kernels of the integer ResNet pipeline (gfx950).
//   hawq_quantize_input      quant_modules.py:271-274 / quant_utils.py:73-97, 237-258
//   hawq_stem_conv7          quant_modules.py:489-494 + q_resnet.py:117-122 (conv, QuantAct16, ReLU)
//   hawq_maxpool3s2_requant  q_resnet.py:93,119 (+ first unit's QuantAct, q_resnet.py:234/239)
//   hawq_requant_residual    quant_modules.py:288-293 (S_w == 1)
//   hawq_avgpool_requant     quant_modules.py:596-600, quant_utils.py:334-337, q_resnet.py:129-131
#include <stdlib.h>

#include "common.h"

namespace {

// ------------------------------------------------------------------ input quantiser
// One thread per output pixel: reads 3 planes (coalesced along W), writes one dword (c0,c1,c2,0).
__global__ __launch_bounds__(256) void quantize_input_kernel(const float *__restrict__ x, int8_t *__restrict__ out,
                                                             int N, int C, int H, int W, int out_h, int out_w,
                                                             int pad_top, int pad_left, float inv_scale, int lo,
                                                             int hi) {
    const long long total = (long long)N * H * W;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int w = (int)(i % W);
        const long long r = i / W;
        const int hh = (int)(r % H);
        const int n = (int)(r / H);
        int q[4] = {0, 0, 0, 0};
        for (int c = 0; c < C; ++c) {
            const float v = x[((long long)(n * C + c) * H + hh) * W + w];
            const float t = __fmul_rn(inv_scale, v);  // `1. / scale * input` : one binary32 rounding
            float rr = rintf(t);                      // round-half-even == torch.round
            rr = fminf(fmaxf(rr, (float)lo), (float)hi);
            q[c] = (int)rr;
        }
        reinterpret_cast<uint32_t *>(out)[((long long)n * out_h + hh + pad_top) * out_w + w + pad_left] =
            pack4_i8(q[0], q[1], q[2], q[3]);
    }
}

// ------------------------------------------------------------------ stem 7x7/2 conv
__device__ __forceinline__ int cperm(int i) { return (((i >> 2) & 1) << 4) + (i & 3) + ((i >> 3) << 2); }

// Each wave keeps the whole 64x(7x32 B) weight matrix in registers (14 x v4i) and walks pixel
// tiles of 64 pixels; the B operand (7 rows x 32 contiguous bytes of the padded NHWC4 image per
// output pixel) is loaded straight from global/L1 - every input byte is reused ~12x by
// neighbouring pixels and rows, all of it cache hits.
__global__ __launch_bounds__(256) void stem_conv7_kernel(const int8_t *__restrict__ in, const int8_t *__restrict__ wgt,
                                                         const int32_t *__restrict__ bias,
                                                         const int32_t *__restrict__ m, const int32_t *__restrict__ e,
                                                         int N, int Hp, int Wp, int Ho, int Wo, int q_lo, int q_hi,
                                                         uint16_t *__restrict__ out16, int32_t *__restrict__ out_acc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    v4i wf[2][7];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int kh = 0; kh < 7; ++kh)
            wf[c][kh] = *reinterpret_cast<const v4i *>(wgt + ((c * 32 + cperm(l31)) * 7 + kh) * 32 + h * 16);
    const int M = N * Ho * Wo;
    const int ntiles = (M + 63) / 64;
    for (int tile = blockIdx.x * 4 + wave; tile < ntiles; tile += gridDim.x * 4) {
        v16i acc[2][2];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[c][p][r] = 0;
        const int8_t *src[2];
        int pix[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            pix[p] = tile * 64 + p * 32 + l31;
            const int mm = pix[p] < M ? pix[p] : M - 1;
            const int n = mm / (Ho * Wo);
            const int r = mm - n * (Ho * Wo);
            const int oy = r / Wo, ox = r - oy * Wo;
            src[p] = in + (((long long)n * Hp + 2 * oy) * Wp + 2 * ox) * 4 + h * 16;
        }
#pragma unroll
        for (int kh = 0; kh < 7; ++kh) {
            v4i af[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int *s = reinterpret_cast<const int *>(src[p] + (long long)kh * Wp * 4);  // 8-B aligned
                v2i a = *reinterpret_cast<const v2i *>(s), b = *reinterpret_cast<const v2i *>(s + 2);
                af[p].x = a.x, af[p].y = a.y, af[p].z = b.x, af[p].w = b.y;
            }
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int p = 0; p < 2; ++p)
                    acc[c][p] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[c][kh], af[p], acc[c][p], 0, 0, 0);
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int ch = c * 32 + h * 16;
            int bb[16], mm[16], ee[16];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v4i t0 = reinterpret_cast<const v4i *>(bias + ch)[i];
                v4i t1 = reinterpret_cast<const v4i *>(m + ch)[i];
                v4i t2 = reinterpret_cast<const v4i *>(e + ch)[i];
                bb[4 * i] = t0.x, bb[4 * i + 1] = t0.y, bb[4 * i + 2] = t0.z, bb[4 * i + 3] = t0.w;
                mm[4 * i] = t1.x, mm[4 * i + 1] = t1.y, mm[4 * i + 2] = t1.z, mm[4 * i + 3] = t1.w;
                ee[4 * i] = t2.x, ee[4 * i + 1] = t2.y, ee[4 * i + 2] = t2.z, ee[4 * i + 3] = t2.w;
            }
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                if (pix[p] >= M) continue;
                const size_t elem = (size_t)pix[p] * 64 + ch;
                int v[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] = acc[c][p][r] + bb[r];
                if (out_acc) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        v4i w = {v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]};
                        reinterpret_cast<v4i *>(out_acc + elem)[i] = w;
                    }
                }
                if (out16) {
                    int w[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        // QuantAct 16-bit (clamp) then ReLU; both monotone, so they commute with max-pool
                        const int a = max(clampi(dyadic_rne(v[2 * i], mm[2 * i], ee[2 * i]), q_lo, q_hi), 0);
                        const int b = max(clampi(dyadic_rne(v[2 * i + 1], mm[2 * i + 1], ee[2 * i + 1]), q_lo, q_hi), 0);
                        w[i] = min(a, 65535) | (min(b, 65535) << 16);
                    }
                    v4i *dst = reinterpret_cast<v4i *>(out16 + elem);
                    v4i a = {w[0], w[1], w[2], w[3]}, b = {w[4], w[5], w[6], w[7]};
                    dst[0] = a;
                    dst[1] = b;
                }
            }
        }
    }
}


// ------------------------------------------------------------------ fused stem
// input quantiser + 7x7/2 conv + bias + 3x3/2 max-pool + QuantAct16 + ReLU + first unit's QuantAct in
// ONE kernel (q_resnet.py:115-122 + 234/239).  The 16-bit conv output at 112x112 (205 MB per 128-image
// batch) never exists in memory, and every conv pixel is computed exactly once per workgroup.
//
// A workgroup owns a strip of SF_R = 8 pooled rows x SF_T = 28 pooled columns of ONE image.  The input
// patch it needs (39 rows x 120 pixels) is quantised straight into an int8 NHWC4 LDS patch.  Wave w takes
// the 32-channel half w & 1 of the four pooled rows 4 (w >> 1) ... + 3 and keeps that half's weights (7
// fragments) in registers throughout.  Its 32 pixel lanes hold CONSECUTIVE pooled columns px0 + lane, and it
// walks down the 9 conv rows 2 py - 1 ... of its pooled rows.  Per conv row two MFMA tiles are computed:
// T0 = conv column 2 px - 1 and T1 = conv column 2 px of the lane's pooled pixel.  The third window column,
// 2 px + 1, is T0 of lane + 1, so
//     rowmax = max(T0, T0 of lane + 1, T1)
// costs one DPP-shifted v_max per accumulator register, and the pooled pixel is the max of three consecutive
// row maxima; an odd conv row (2 py + 1) closes pooled row py and opens py + 1, so it is computed once and
// carried.  The max is taken on the raw accumulators, because the per-channel requantisation is monotone
// (m > 0) and the bias is constant.  Lanes 28-31 are halo lanes: lane 28 feeds lane 27's third column, none of
// them stores (the next workgroup owns those columns); 28 tiles ImageNet's 56 pooled columns without waste.
// Per 32 channels and pooled row that is 28 MFMAs (+ 14 per wave for the opening row) where the window walk of
// the first version took 63.
//
// Max-pool padding is -inf: a conv row outside the conv map is skipped (wave-uniform), and of the conv columns
// only T0 can be outside for a lane whose result is used (2 px <= Wc - 1 for every px < Wp) - one select per
// accumulator register, on border strips only.
//
// LDS patch: pixel PAIRS (8 bytes) are de-interleaved into two planes, E = even pairs, O = odd pairs, each
// [39][30] pairs.  A lane's B fragment (16 bytes = pairs 2 j + dx, 2 j + dx + 1 with j = lane + k-half) is
// {E[j], O[j]} for T0 and {O[j], E[j + 1]} for T1: three ds_read_b64 per weight row serve both tiles, every
// one of them 32 lanes x 8 contiguous bytes (no bank conflict, no alignment replay) from a single copy of the
// patch - the first version needed a second, 8-byte-shifted copy and three stores per group for that.
// Halo lanes read up to 32 bytes past a row (into the next row / the pad): harmless, never stored.
//
// Resources (hipcc -O3, gfx950): 104 VGPRs with uint8 input, 120 with fp32 input, no scratch; 20 560 / 19 792 bytes of LDS per
// workgroup; N x ceil(Hp / 8) x ceil(Wp / 28) workgroups (1792 at 128 ImageNet images).  Registers allow 4 workgroups per CU
// (LDS would allow 7), so fill, MFMA and epilogue phases of different workgroups still overlap, four deep where the window walk
// ran six deep at 80 VGPRs: both accumulator tiles, the open pooled row and 7 weight fragments are live in the MFMA part.  The
// weight fragments are re-read per conv row (L1-resident) so that they do not also live through the epilogue.
constexpr int SF_T = 28;                        // pooled columns a workgroup stores
constexpr int SF_R = 8;                         // pooled rows per workgroup (two wave pairs x 4)
constexpr int SF_ROWS = 4 * SF_R + 7;           // input rows of the patch (39)
constexpr int SF_SLOTS = SF_T + 2;              // pixel pairs per row and plane (30: 120 pixels)
constexpr int SF_ROWB = SF_SLOTS * 8;           // bytes per row of one plane
constexpr int SF_PLANE = SF_ROWS * SF_ROWB;     // bytes per plane (9360: no multiple of 512, > 2040 - the E and O reads of a fragment stay separate ds_read_b64)
constexpr int SF_NG = SF_ROWS * SF_SLOTS;       // groups of 4 pixels (one pair for each plane)
constexpr int SF_GPT = (SF_NG + 255) / 256;     // groups per thread (5)

// lane i <- lane i + 1 (wave_shl:1; lane 63 keeps its own value).  Lane 31 receives lane 32's - a halo lane.
__device__ __forceinline__ int sf_lane_up(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x130, 0xf, 0xf, false); }

// U8: the image arrives as uint8 NHWC [N][H][W][Cin] (what an image decoder produces) together with a [3][256] int8
// table lut[c][u] = QuantAct(normalise_c(u / 255)) built on the host with the reference's own float operations
// (hawq_amd.engine.input_lut): the input quantiser becomes a table look-up - exact, and the input read shrinks 4x.
template <bool U8>
__global__ __launch_bounds__(256, 4) void stem_fused_kernel(
    const float *__restrict__ x, const uint8_t *__restrict__ xu8, const int8_t *__restrict__ lut,
    int N, int Cin, int H, int W, float inv_scale, int in_lo, int in_hi,
    const int8_t *__restrict__ wgt, const int32_t *__restrict__ bias, const int32_t *__restrict__ m,
    const int32_t *__restrict__ e, int a_lo, int a_hi, int Hc, int Wc, int Hp, int Wp,
    uint16_t *__restrict__ res_out, void *__restrict__ out_q, int out_bits, int mq, int eq, int q_lo, int q_hi,
    int fast, int dbg) {
    __shared__ __attribute__((aligned(16))) char patch[2 * SF_PLANE + 48];
    // fast contract: per-channel fused requant constants {m, (e - 32) | k << 8, lo32(C), hi32(C)}, C = (bias << k) * m + 2^(e-1) - the form
    // of hawq_amd.packing.pack_ctab, built here from (bias, m, e) by the first 64 threads while the others already fetch the patch.  The
    // epilogue then reads ONE 16-byte LDS entry per output instead of three global table words, and a requant is shift + v_mad_i64_i32 +
    // shift
    __shared__ __attribute__((aligned(16))) int ctab_s[64 * 4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (fast && t < 64) {
        const int mm = m[t], ek = e[t], ee = ek & 0xff, kk = ek >> 8;
        const long long cc = ((long long)bias[t] << kk) * (long long)mm + (1ll << (ee - 1));
        const v4i ent = {mm, (ee - 32) | (kk << 8), (int)(unsigned)cc, (int)(cc >> 32)};
        *reinterpret_cast<v4i *>(ctab_s + 4 * t) = ent;
    }
    const int l31 = lane & 31, h = lane >> 5;
    const int bw = (Wp + SF_T - 1) / SF_T, bh = (Hp + SF_R - 1) / SF_R;
    int b = blockIdx.x;
    const int bx = b % bw;
    b /= bw;
    const int by = b % bh;
    const int n = b / bh;
    const int py0 = by * SF_R, px0 = bx * SF_T;

    // ---- fill: group g = 4 pixels (one pair for each plane) at patch row g / 30; input pixel (4 py0 - 5 + row, 4 px0 - 5 + 4 slot).
    // All global loads of a batch of groups are issued before any is consumed (the fill is latency-bound otherwise); coordinates are
    // clamped into the image so every load is legal, out-of-image pixels are zeroed by mask (the conv's zero padding).
    auto group_geom = [&](int k, int &gaddr, unsigned &gmask, int &iy, int &ix) {
        const int g = t + 256 * k;
        const int gg = g < SF_NG ? g : SF_NG - 1;
        const int r = gg / SF_SLOTS, s = gg - r * SF_SLOTS;
        iy = 4 * py0 - 5 + r, ix = 4 * px0 - 5 + 4 * s;
        const bool rowok = g < SF_NG && (unsigned)iy < (unsigned)H && !HAWQ_DBG_BIT(dbg, 16);
        gaddr = r * SF_ROWB + s * 8;
        gmask = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (rowok && (unsigned)(ix + j) < (unsigned)W) gmask |= 1u << j;
    };
    auto store_group = [&](int gaddr, const int (&w)[4]) {
        *reinterpret_cast<v2i *>(patch + gaddr) = v2i{w[0], w[1]};
        *reinterpret_cast<v2i *>(patch + SF_PLANE + gaddr) = v2i{w[2], w[3]};
    };
    if constexpr (U8) {
        // ---- uint8 input: table look-up straight into the LDS patch
        __shared__ int8_t lut_s[3 * 256];
        for (int i = t; i < 3 * 256 / 4; i += 256) reinterpret_cast<int *>(lut_s)[i] = reinterpret_cast<const int *>(lut)[i];
        __syncthreads();
        unsigned raw[SF_GPT][3];   // the group's 12 bytes (4 pixels x 3 channels), little-endian
        unsigned gmask[SF_GPT];
        int gaddr[SF_GPT];
#pragma unroll
        for (int k = 0; k < SF_GPT; ++k) {
            int iy, ix;
            group_geom(k, gaddr[k], gmask[k], iy, ix);
            const int yy = min(max(iy, 0), H - 1);
            const size_t rowoff = ((size_t)n * H + yy) * W * Cin;
            if (Cin == 3 && ix >= 0 && ix + 5 < W) {
                // 4 aligned dwords cover the 12 bytes at any misalignment (and stay inside the row: ix + 5 < W)
                const size_t b0 = rowoff + (size_t)ix * 3;
                const unsigned *q4 = reinterpret_cast<const unsigned *>(xu8 + (b0 & ~(size_t)3));
                const unsigned d0 = q4[0], d1 = q4[1], d2 = q4[2], d3 = q4[3];
                const unsigned sh = (unsigned)(b0 & 3);
                raw[k][0] = __builtin_amdgcn_alignbyte(d1, d0, sh);
                raw[k][1] = __builtin_amdgcn_alignbyte(d2, d1, sh);
                raw[k][2] = __builtin_amdgcn_alignbyte(d3, d2, sh);
            } else {  // image borders / fewer channels: byte loads with clamped coordinates
                unsigned char bb[12];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint8_t *px = xu8 + rowoff + (size_t)min(max(ix + j, 0), W - 1) * Cin;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) bb[3 * j + ch] = ch < Cin ? px[ch] : 0;
                }
#pragma unroll
                for (int d = 0; d < 3; ++d)
                    raw[k][d] = (unsigned)bb[4 * d] | ((unsigned)bb[4 * d + 1] << 8) | ((unsigned)bb[4 * d + 2] << 16) | ((unsigned)bb[4 * d + 3] << 24);
            }
        }
#pragma unroll
        for (int k = 0; k < SF_GPT; ++k) {
            if (t + 256 * k >= SF_NG) continue;
            int w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = (gmask[k] >> j) & 1;
                auto byte_at = [&](int i) { return (raw[k][i >> 2] >> (8 * (i & 3))) & 0xffu; };
                w[j] = ok ? (int)pack4_i8(lut_s[byte_at(3 * j)], Cin > 1 ? lut_s[256 + byte_at(3 * j + 1)] : 0,
                                          Cin > 2 ? lut_s[512 + byte_at(3 * j + 2)] : 0, 0)
                          : 0;
            }
            store_group(gaddr[k], w);
        }
    } else {
        // ---- fp32 input: q = clamp(rint(fl(1/S) * x))  (quant_utils.py:73-97), in two batches of groups (3 + 2) so that the
        // loads in flight (3 float4 per group) stay inside the register budget of the MFMA phase
        const size_t plane = (size_t)H * W;
        auto quant1 = [&](float v) {
            v = rintf(__fmul_rn(inv_scale, v));
            return (int)fminf(fmaxf(v, (float)in_lo), (float)in_hi);
        };
        constexpr int GB = 3;
#pragma unroll
        for (int kb = 0; kb < SF_GPT; kb += GB) {
            float4 v[GB][3];
            int gaddr[GB];
            unsigned gmask[GB];  // bit j: pixel j of the group is inside the image
#pragma unroll
            for (int k = 0; k < GB; ++k) {
                if (kb + k >= SF_GPT) continue;
                int iy, ix;
                group_geom(kb + k, gaddr[k], gmask[k], iy, ix);
                const int yy = min(max(iy, 0), H - 1);
                const float *src = x + ((size_t)n * Cin) * plane + (size_t)yy * W;
                const bool interior = ix >= 0 && ix + 3 < W;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    if (ch < Cin) {
                        if (interior) {
                            v[k][ch] = *reinterpret_cast<const float4 *>(src + ch * plane + ix);
                        } else {
                            const float *s1 = src + ch * plane;
                            v[k][ch].x = s1[min(max(ix, 0), W - 1)], v[k][ch].y = s1[min(max(ix + 1, 0), W - 1)];
                            v[k][ch].z = s1[min(max(ix + 2, 0), W - 1)], v[k][ch].w = s1[min(max(ix + 3, 0), W - 1)];
                        }
                    } else {
                        v[k][ch] = make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < GB; ++k) {
                if (kb + k >= SF_GPT || t + 256 * (kb + k) >= SF_NG) continue;
                const float px4[4][3] = {{v[k][0].x, v[k][1].x, v[k][2].x}, {v[k][0].y, v[k][1].y, v[k][2].y},
                                         {v[k][0].z, v[k][1].z, v[k][2].z}, {v[k][0].w, v[k][1].w, v[k][2].w}};
                int w[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool ok = (gmask[k] >> j) & 1;
                    w[j] = ok ? (int)pack4_i8(quant1(px4[j][0]), Cin > 1 ? quant1(px4[j][1]) : 0, Cin > 2 ? quant1(px4[j][2]) : 0, 0) : 0;
                }
                store_group(gaddr[k], w);
            }
        }
    }
    __syncthreads();

    // ---- conv rows -> row maxima -> pooled rows, all in registers
    const int c = wave & 1;                        // 32-channel half of this wave
    const int pyw = py0 + 4 * (wave >> 1);         // its first pooled row
    const int px = px0 + l31;
    const bool store_lane = l31 < SF_T && px < Wp;
    // T0 (conv column 2 px - 1) outside the conv map: the left image border, and - odd Wc only - the column right of the last pooled pixel
    const bool t0_in = (unsigned)(2 * px - 1) < (unsigned)Wc;
    const bool border = px0 == 0 || 2 * (px0 + SF_T) - 1 >= Wc;   // wave-uniform: some lane that matters needs the select
    const int8_t *wlane = wgt + ((c * 32 + cperm(l31)) * 7) * 32 + h * 16;
    const char *rb = patch + (16 * (wave >> 1)) * SF_ROWB + 8 * (l31 + h);   // pair j = lane + k-half of the wave's first patch row
    const int ch = c * 32 + h * 16;
    const int NEG = (int)0x80000000;
    int run[16];   // max of the conv rows seen so far of the pooled row that is open
#pragma unroll
    for (int r = 0; r < 16; ++r) run[r] = NEG;
#pragma unroll 1   // one copy of the row body and of the epilogue; conv row k = 0 ... 8 is cy = 2 pyw - 1 + k, patch rows 2 k ... 2 k + 6
    for (int k = 0; k <= 8; ++k, rb += 2 * SF_ROWB) {
        const int cy = 2 * pyw - 1 + k;
        if (cy > Hc) break;
        int rm[16];
        if ((unsigned)cy < (unsigned)Hc && !(HAWQ_DBG_BIT(dbg, 32) && k > 0)) {
            v4i wf[7];   // re-read per conv row (14 KB in all, L1-resident): 28 registers that need not live through the epilogue
#pragma unroll
            for (int kh = 0; kh < 7; ++kh) wf[kh] = *reinterpret_cast<const v4i *>(wlane + kh * 32);
            v16i t0, t1;
#pragma unroll
            for (int r = 0; r < 16; ++r) t0[r] = 0, t1[r] = 0;
#pragma unroll
            for (int kh = 0; kh < 7; ++kh) {
                const char *p = rb + kh * SF_ROWB;
                const v2i e0 = *reinterpret_cast<const v2i *>(p), o0 = *reinterpret_cast<const v2i *>(p + SF_PLANE),
                          e1 = *reinterpret_cast<const v2i *>(p + 8);
                const v4i a0 = {e0.x, e0.y, o0.x, o0.y}, a1 = {o0.x, o0.y, e1.x, e1.y};
                t0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[kh], a0, t0, 0, 0, 0);
                t1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[kh], a1, t1, 0, 0, 0);
            }
            if (border) {
#pragma unroll
                for (int r = 0; r < 16; ++r) t0[r] = t0_in ? t0[r] : NEG;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) rm[r] = max(max(t0[r], sf_lane_up(t0[r])), t1[r]);
        } else {   // max-pool padding: -inf
#pragma unroll
            for (int r = 0; r < 16; ++r) rm[r] = NEG;
        }
        if (k & 1) {   // conv row 2 py: the middle row of the open pooled row
#pragma unroll
            for (int r = 0; r < 16; ++r) run[r] = max(run[r], rm[r]);
            continue;
        }
        int best[16];   // conv row 2 py + 1 closes pooled row py = pyw + k / 2 - 1 and opens the next one
#pragma unroll
        for (int r = 0; r < 16; ++r) best[r] = max(run[r], rm[r]), run[r] = rm[r];
        const int py = pyw + (k >> 1) - 1;
        if (k == 0 || py >= Hp || HAWQ_DBG_BIT(dbg, 64)) continue;   // wave-uniform
        const size_t opix = ((size_t)n * Hp + py) * Wp + px;
        int r16[16], qa[16];
        if (fast) {  // host-proved tie-free tables (hawq_amd.quant_utils.tables_are_fast): fused constants from LDS, 3-instruction requants
            const DyNt dq = dynt_prepare(mq, eq);
            const int lo0 = max(a_lo, 0);   // QuantAct16's clamp and the ReLU behind it in one v_med3 (a_hi >= 0)
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const v4i t4 = *reinterpret_cast<const v4i *>(ctab_s + 4 * (ch + j));
                DyNt d;
                d.m = t4.x, d.s = t4.y & 31, d.k = t4.y >> 8;
                d.add = (long long)(((unsigned long long)(unsigned)t4.w << 32) | (unsigned)t4.z);
                const int v = med3i(dyadic_nt(best[j], d), lo0, a_hi);
                r16[j] = v;
                qa[j] = med3i(dyadic_nt(v, dq), q_lo, q_hi);
            }
        } else {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const v4i b4 = *reinterpret_cast<const v4i *>(bias + ch + 4 * g), m4 = *reinterpret_cast<const v4i *>(m + ch + 4 * g),
                          e4 = *reinterpret_cast<const v4i *>(e + ch + 4 * g);
                const int bb[4] = {b4.x, b4.y, b4.z, b4.w}, mm[4] = {m4.x, m4.y, m4.z, m4.w}, ee[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int v = max(clampi(dyadic_rne(best[4 * g + j] + bb[j], mm[j], ee[j]), a_lo, a_hi), 0);
                    r16[4 * g + j] = v;
                    qa[4 * g + j] = clampi(dyadic_rne(v, mq, eq), q_lo, q_hi);
                }
            }
        }
        if (res_out && store_lane) {
            v4i lo, hi;
            lo.x = r16[0] | (r16[1] << 16), lo.y = r16[2] | (r16[3] << 16), lo.z = r16[4] | (r16[5] << 16), lo.w = r16[6] | (r16[7] << 16);
            hi.x = r16[8] | (r16[9] << 16), hi.y = r16[10] | (r16[11] << 16), hi.z = r16[12] | (r16[13] << 16), hi.w = r16[14] | (r16[15] << 16);
            v4i *dst = reinterpret_cast<v4i *>(res_out + opix * 64 + ch);
            dst[0] = lo;
            dst[1] = hi;
        }
        if (out_q && store_lane) {
            if (out_bits == 8) {
                v4i w = {(int)pack4_i8(qa[0], qa[1], qa[2], qa[3]), (int)pack4_i8(qa[4], qa[5], qa[6], qa[7]),
                         (int)pack4_i8(qa[8], qa[9], qa[10], qa[11]), (int)pack4_i8(qa[12], qa[13], qa[14], qa[15])};
                *reinterpret_cast<v4i *>((int8_t *)out_q + opix * 64 + ch) = w;
            } else {
                v2i w = {(int)pack8_u4(&qa[0]), (int)pack8_u4(&qa[8])};
                *reinterpret_cast<v2i *>((uint8_t *)out_q + ((opix * 64 + ch) >> 1)) = w;
            }
        }
    }
}

// ------------------------------------------------------------------ 3x3/2 max-pool (+ QuantAct)
// thread = 8 channels of one output pixel (16 B of uint16)
__global__ __launch_bounds__(256) void maxpool_requant_kernel(const uint16_t *__restrict__ in, int N, int H, int W,
                                                              int C, int Ho, int Wo, uint16_t *__restrict__ res_out,
                                                              void *__restrict__ out_q, int out_bits, int mq, int eq,
                                                              int q_lo, int q_hi) {
    const int cg = C >> 3;
    const long long total = (long long)N * Ho * Wo * cg;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int g = (int)(i % cg);
        long long r = i / cg;
        const int ox = (int)(r % Wo);
        r /= Wo;
        const int oy = (int)(r % Ho);
        const int n = (int)(r / Ho);
        int best[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) best[k] = 0;  // inputs are >= 0 (post-ReLU) and the window is never empty
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * oy - 1 + ky;
            if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = 2 * ox - 1 + kx;
                if ((unsigned)ix >= (unsigned)W) continue;
                const v4i v = *reinterpret_cast<const v4i *>(in + (((long long)n * H + iy) * W + ix) * C + g * 8);
                const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    best[2 * k] = max(best[2 * k], w[k] & 0xffff);
                    best[2 * k + 1] = max(best[2 * k + 1], (int)((unsigned)w[k] >> 16));
                }
            }
        }
        const long long elem = (((long long)n * Ho + oy) * Wo + ox) * C + g * 8;
        if (res_out) {
            v4i o;
            o.x = best[0] | (best[1] << 16);
            o.y = best[2] | (best[3] << 16);
            o.z = best[4] | (best[5] << 16);
            o.w = best[6] | (best[7] << 16);
            *reinterpret_cast<v4i *>(res_out + elem) = o;
        }
        if (out_q) {
            int q[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) q[k] = clampi(dyadic_rne(best[k], mq, eq), q_lo, q_hi);
            if (out_bits == 8) {
                v2i o;
                o.x = (int)pack4_i8(q[0], q[1], q[2], q[3]);
                o.y = (int)pack4_i8(q[4], q[5], q[6], q[7]);
                *reinterpret_cast<v2i *>((int8_t *)out_q + elem) = o;
            } else {
                *reinterpret_cast<uint32_t *>((uint8_t *)out_q + (elem >> 1)) = pack8_u4(q);
            }
        }
    }
}

// ------------------------------------------------------------------ stand-alone block-input QuantAct
__global__ __launch_bounds__(256) void requant_residual_kernel(const void *__restrict__ in, int in_bits, long long n8,
                                                               void *__restrict__ out_q, int out_bits, int mq, int eq,
                                                               int q_lo, int q_hi) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        int v[8];
        if (in_bits == 16) {
            const v4i t = reinterpret_cast<const v4i *>(in)[i];
            const int w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[2 * k] = w[k] & 0xffff;
                v[2 * k + 1] = (int)((unsigned)w[k] >> 16);
            }
        } else {
            const v4i a = reinterpret_cast<const v4i *>(in)[2 * i], b = reinterpret_cast<const v4i *>(in)[2 * i + 1];
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
        }
        int q[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = clampi(dyadic_rne(v[k], mq, eq), q_lo, q_hi);
        if (out_bits == 8) {
            v2i o;
            o.x = (int)pack4_i8(q[0], q[1], q[2], q[3]);
            o.y = (int)pack4_i8(q[4], q[5], q[6], q[7]);
            reinterpret_cast<v2i *>(out_q)[i] = o;
        } else {
            reinterpret_cast<uint32_t *>(out_q)[i] = pack8_u4(q);
        }
    }
}

// ------------------------------------------------------------------ global average pool + QuantAct
// trunc(sum/HW + 0.01) in exact rationals (== floor(sum/HW) for sum >= 0), then the next QuantAct's table
__device__ __forceinline__ void avgpool_finish(long long s, int HW, int i, int8_t *out, int32_t *pooled, int mq, int eq,
                                               int q_lo, int q_hi) {
    const long long p = (100 * s + HW) / (100ll * HW);
    if (pooled) pooled[i] = (int32_t)p;
    out[i] = (int8_t)clampi(dyadic_rne((int32_t)p, mq, eq), q_lo, q_hi);
}

// general form: thread = one (n, c), strided over HW (int32 residuals, odd channel counts)
__global__ __launch_bounds__(256) void avgpool_requant_kernel(const void *__restrict__ in, int in_bits, int N, int HW,
                                                              int C, int8_t *__restrict__ out,
                                                              int32_t *__restrict__ pooled, int mq, int eq, int q_lo,
                                                              int q_hi) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N * C) return;
    const int n = i / C, c = i - n * C;
    long long s = 0;
    for (int k = 0; k < HW; ++k) {
        const size_t idx = ((size_t)n * HW + k) * C + c;
        s += in_bits == 16 ? (long long)((const uint16_t *)in)[idx] : (long long)((const int32_t *)in)[idx];
    }
    avgpool_finish(s, HW, i, out, pooled, mq, eq, q_lo, q_hi);
}

// uint16 residuals, C % 256 == 0: workgroup = (image, 256 channels); lane group g = t / 32 takes pixels g, g+8, ...
// with 16-byte loads (8 channels per lane: a wave instruction reads two full 512-byte pixel rows), partial sums
// meet in LDS.  HW * 65535 < 2^31 is checked by the launcher.
__global__ __launch_bounds__(256) void avgpool_requant_u16_kernel(const uint16_t *__restrict__ in, int HW, int C,
                                                                  int8_t *__restrict__ out, int32_t *__restrict__ pooled,
                                                                  int mq, int eq, int q_lo, int q_hi) {
    __shared__ int part[8][256];
    const int t = threadIdx.x, cg = t & 31, g = t >> 5;
    const int n = blockIdx.x / (C >> 8), c0 = (blockIdx.x % (C >> 8)) << 8;
    int s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint16_t *base = in + (size_t)n * HW * C + c0 + cg * 8;
    for (int k = g; k < HW; k += 8) {
        const uint4 v = *reinterpret_cast<const uint4 *>(base + (size_t)k * C);
        s[0] += v.x & 0xffff, s[1] += v.x >> 16, s[2] += v.y & 0xffff, s[3] += v.y >> 16;
        s[4] += v.z & 0xffff, s[5] += v.z >> 16, s[6] += v.w & 0xffff, s[7] += v.w >> 16;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) part[g][cg * 8 + j] = s[j];
    __syncthreads();
    long long tot = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) tot += part[j][t];
    avgpool_finish(tot, HW, n * C + c0 + t, out, pooled, mq, eq, q_lo, q_hi);
}

inline int grid_for(long long work_items) {
    long long g = (work_items + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace

extern "C" int hawq_quantize_input(const float *x, int8_t *out, int32_t N, int32_t C, int32_t H, int32_t W,
                                   int32_t out_h, int32_t out_w, int32_t pad_top, int32_t pad_left, float inv_scale,
                                   int32_t lo, int32_t hi, void *stream) {
    HAWQ_REQUIRE(x && out, "hawq_quantize_input: null pointer");
    HAWQ_REQUIRE(C >= 1 && C <= 4, "hawq_quantize_input: C=%d must be 1..4", C);
    HAWQ_REQUIRE(N > 0 && H > 0 && W > 0 && out_h >= H + pad_top && out_w >= W + pad_left,
                 "hawq_quantize_input: bad geometry");
    hipLaunchKernelGGL(quantize_input_kernel, dim3(grid_for((long long)N * H * W)), dim3(256), 0, (hipStream_t)stream,
                       x, out, N, C, H, W, out_h, out_w, pad_top, pad_left, inv_scale, lo, hi);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int hawq_stem_conv7(const int8_t *in, const int8_t *wgt, const int32_t *bias, const int32_t *m,
                               const int32_t *e, int32_t N, int32_t Hp, int32_t Wp, int32_t Ho, int32_t Wo,
                               int32_t q_lo, int32_t q_hi, uint16_t *out16, int32_t *out_acc, void *stream) {
    HAWQ_REQUIRE(in && wgt && bias, "hawq_stem_conv7: null pointer");
    HAWQ_REQUIRE(out16 || out_acc, "hawq_stem_conv7: no output requested");
    HAWQ_REQUIRE(!out16 || (m && e), "hawq_stem_conv7: out16 needs m/e tables");
    HAWQ_REQUIRE(Hp >= 2 * (Ho - 1) + 7 && Wp >= 2 * (Wo - 1) + 8 && (Wp % 2) == 0,
                 "hawq_stem_conv7: padded input %dx%d too small for output %dx%d", Hp, Wp, Ho, Wo);
    const long long M = (long long)N * Ho * Wo;
    HAWQ_REQUIRE(M > 0 && M < (1ll << 30), "hawq_stem_conv7: bad size");
    const long long tiles = (M + 63) / 64;
    long long grid = (tiles + 3) / 4;
    if (grid > 2048) grid = 2048;
    if (!m) m = bias, e = bias;  // never dereferenced for out16 == NULL, keeps loads in-bounds
    hipLaunchKernelGGL(stem_conv7_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, in, wgt, bias, m, e, N,
                       Hp, Wp, Ho, Wo, q_lo, q_hi, out16, out_acc);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int hawq_maxpool3s2_requant(const uint16_t *in, int32_t N, int32_t H, int32_t W, int32_t C,
                                       uint16_t *res_out, void *out_q, int32_t out_bits, int32_t mq, int32_t eq,
                                       int32_t q_lo, int32_t q_hi, void *stream) {
    HAWQ_REQUIRE(in && (res_out || out_q), "hawq_maxpool3s2_requant: null pointer");
    HAWQ_REQUIRE(C > 0 && C % 8 == 0, "hawq_maxpool3s2_requant: C must be a multiple of 8");
    HAWQ_REQUIRE(!out_q || out_bits == 8 || out_bits == 4, "hawq_maxpool3s2_requant: out_bits 4/8");
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    hipLaunchKernelGGL(maxpool_requant_kernel, dim3(grid_for((long long)N * Ho * Wo * (C / 8))), dim3(256), 0,
                       (hipStream_t)stream, in, N, H, W, C, Ho, Wo, res_out, out_q, out_bits, mq, eq, q_lo, q_hi);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int hawq_requant_residual(const void *in, int32_t in_bits, int64_t n, void *out_q, int32_t out_bits,
                                     int32_t mq, int32_t eq, int32_t q_lo, int32_t q_hi, void *stream) {
    HAWQ_REQUIRE(in && out_q, "hawq_requant_residual: null pointer");
    HAWQ_REQUIRE(n > 0 && n % 8 == 0, "hawq_requant_residual: n must be a positive multiple of 8");
    HAWQ_REQUIRE((in_bits == 16 || in_bits == 32) && (out_bits == 8 || out_bits == 4),
                 "hawq_requant_residual: in_bits 16/32, out_bits 4/8");
    hipLaunchKernelGGL(requant_residual_kernel, dim3(grid_for(n / 8)), dim3(256), 0, (hipStream_t)stream, in, in_bits,
                       (long long)(n / 8), out_q, out_bits, mq, eq, q_lo, q_hi);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int hawq_avgpool_requant(const void *in, int32_t in_bits, int32_t N, int32_t HW, int32_t C, int8_t *out,
                                    int32_t *pooled_out, int32_t mq, int32_t eq, int32_t q_lo, int32_t q_hi,
                                    void *stream) {
    HAWQ_REQUIRE(in && out, "hawq_avgpool_requant: null pointer");
    HAWQ_REQUIRE(in_bits == 16 || in_bits == 32, "hawq_avgpool_requant: in_bits 16/32");
    HAWQ_REQUIRE(N > 0 && HW > 0 && C > 0, "hawq_avgpool_requant: bad geometry");
    if (in_bits == 16 && C % 256 == 0 && HW <= 32768 && (reinterpret_cast<size_t>(in) & 15) == 0)
        hipLaunchKernelGGL(avgpool_requant_u16_kernel, dim3(N * (C / 256)), dim3(256), 0, (hipStream_t)stream,
                           (const uint16_t *)in, HW, C, out, pooled_out, mq, eq, q_lo, q_hi);
    else
        hipLaunchKernelGGL(avgpool_requant_kernel, dim3((N * C + 255) / 256), dim3(256), 0, (hipStream_t)stream, in,
                           in_bits, N, HW, C, out, pooled_out, mq, eq, q_lo, q_hi);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}

namespace {
int stem_fused_launch(const float *x, const uint8_t *xu8, const int8_t *lut, int32_t N, int32_t C, int32_t H, int32_t W,
                      float inv_scale, int32_t in_lo, int32_t in_hi, const int8_t *wgt, const int32_t *bias, const int32_t *m,
                      const int32_t *e, int32_t a_lo, int32_t a_hi, uint16_t *res_out, void *out_q, int32_t out_bits,
                      int32_t mq, int32_t eq, int32_t q_lo, int32_t q_hi, int32_t fast_tables, void *stream) {
    HAWQ_REQUIRE((x || (xu8 && lut)) && wgt && bias && m && e, "hawq_stem_fused: null pointer");
    HAWQ_REQUIRE(!fast_tables || ((eq & 0xff) >= 33 && (eq & 0xff) <= 62), "hawq_stem_fused: fast_tables needs eq in [33,62]");
    HAWQ_REQUIRE(res_out || out_q, "hawq_stem_fused: no output requested");
    HAWQ_REQUIRE(C >= 1 && C <= 3 && N > 0 && H >= 7 && W >= 7, "hawq_stem_fused: bad geometry (C <= 3)");
    HAWQ_REQUIRE(!out_q || out_bits == 8 || out_bits == 4, "hawq_stem_fused: out_bits 4/8");
    HAWQ_REQUIRE(a_lo >= -32768 && a_hi <= 65535 && a_hi >= 0, "hawq_stem_fused: 16-bit activation range expected");
    HAWQ_REQUIRE(!lut || (reinterpret_cast<size_t>(lut) & 3) == 0, "hawq_stem_fused_u8: lut must be 4-byte aligned");
    const int Hc = (H + 6 - 7) / 2 + 1, Wc = (W + 6 - 7) / 2 + 1;    // conv 7x7 / 2, pad 3
    const int Hp = (Hc + 2 - 3) / 2 + 1, Wp = (Wc + 2 - 3) / 2 + 1;  // max-pool 3x3 / 2, pad 1
    const long long blocks = (long long)((Wp + SF_T - 1) / SF_T) * ((Hp + SF_R - 1) / SF_R) * N;
    HAWQ_REQUIRE(blocks < (1ll << 31), "hawq_stem_fused: problem too large");
    const int dbg = HAWQ_DBG_ENV();
    if (xu8)
        hipLaunchKernelGGL(stem_fused_kernel<true>, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, x, xu8, lut, N, C, H,
                           W, inv_scale, in_lo, in_hi, wgt, bias, m, e, a_lo, a_hi, Hc, Wc, Hp, Wp, res_out, out_q, out_bits,
                           mq, eq, q_lo, q_hi, fast_tables, dbg);
    else
        hipLaunchKernelGGL(stem_fused_kernel<false>, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, x, xu8, lut, N, C, H,
                           W, inv_scale, in_lo, in_hi, wgt, bias, m, e, a_lo, a_hi, Hc, Wc, Hp, Wp, res_out, out_q, out_bits,
                           mq, eq, q_lo, q_hi, fast_tables, dbg);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
}  // namespace

extern "C" int hawq_stem_fused(const float *x, int32_t N, int32_t C, int32_t H, int32_t W, float inv_scale, int32_t in_lo,
                               int32_t in_hi, const int8_t *wgt, const int32_t *bias, const int32_t *m, const int32_t *e,
                               int32_t a_lo, int32_t a_hi, uint16_t *res_out, void *out_q, int32_t out_bits, int32_t mq,
                               int32_t eq, int32_t q_lo, int32_t q_hi, int32_t fast_tables, void *stream) {
    HAWQ_REQUIRE(x, "hawq_stem_fused: null pointer");
    return stem_fused_launch(x, nullptr, nullptr, N, C, H, W, inv_scale, in_lo, in_hi, wgt, bias, m, e, a_lo, a_hi, res_out,
                             out_q, out_bits, mq, eq, q_lo, q_hi, fast_tables, stream);
}

extern "C" int hawq_stem_fused_u8(const uint8_t *x, const int8_t *lut, int32_t N, int32_t C, int32_t H, int32_t W,
                                  const int8_t *wgt, const int32_t *bias, const int32_t *m, const int32_t *e, int32_t a_lo,
                                  int32_t a_hi, uint16_t *res_out, void *out_q, int32_t out_bits, int32_t mq, int32_t eq,
                                  int32_t q_lo, int32_t q_hi, int32_t fast_tables, void *stream) {
    HAWQ_REQUIRE(x && lut, "hawq_stem_fused_u8: null pointer");
    return stem_fused_launch(nullptr, x, lut, N, C, H, W, 0.f, -128, 127, wgt, bias, m, e, a_lo, a_hi, res_out, out_q, out_bits,
                             mq, eq, q_lo, q_hi, fast_tables, stream);
}
