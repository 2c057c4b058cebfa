// Implicit-GEMM integer convolution for gfx950 (MI355X) with fused HAWQ epilogues.
//
// GEMM view: D[Cout][M] = W[Cout][K] * X[K][M],  M = N*Ho*Wo output pixels,
// K = KH*KW*Cin.  Weights are the MFMA "A" operand (rows = output channels), pixels the "B"
// operand (cols), so that after v_mfma_i32_32x32x32_i8 every lane owns ONE pixel and, thanks
// to a row permutation applied when the weight fragment is read from LDS, 16 CONSECUTIVE
// output channels of it: the epilogue then stores 16 int8 (one dwordx4) / 16 uint16 (two
// dwordx4) per lane straight into the NHWC output.
//
// K is walked in chunks of 64 input channels of one filter tap.  Each chunk of both operands is
// fetched global->registers (16 B per thread per row, im2col addressing with zero fill for
// padding), unpacked to int8 if the tensor is 4-bit (hawq4 nibble format), and written to a
// double-buffered, XOR-swizzled LDS tile [rows][64 B]; fragments are read back with
// conflict-free ds_read_b128.  All MACs are exact int32.
//
// Reference arithmetic replaced: quant_modules.py:489-494 (conv), q_resnet.py:242-258 (ReLU,
// residual add), quant_utils.py:390-456 (fixedpoint_fn case 0 / case 1).
//
// This header is the device code the conv translation units share (conv_igemm.hip, band_v1.hip, conv_splitk.hip):
// ConvP, Cfg, the pipelines, both epilogues and conv_kernel.  conv_dispatch.hip fills ConvP and instantiates nothing.
#pragma once
#include <stdio.h>
#include <stdlib.h>

#include "common.h"

// kernel arguments of every kernel built from this header; filled by conv_check (conv_dispatch.h)
struct ConvP {
    const uint8_t *in, *wgt;
    const int32_t *bias;
    int N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo, M;
    int in_bits, w_bits;
    const uint8_t *in2, *wgt2;
    const int32_t *bias2;
    int H2, W2, Cin2, stride2, in2_bits, w2_bits;
    int relu;
    const int32_t *m, *e, *m_id, *e_id;
    int m_id_s, e_id_s;
    const void *res_in;
    int res_in_bits;
    void *res_out;
    int res_out_bits;
    void *out_q;
    int out_bits, q_lo, q_hi, mq, eq;
    int32_t *out_acc;
    float *out_f32;
    const float *fscale;
    int ldo, n_valid;
    int32_t *flags;
    const int32_t *ctab, *ctab_id;
    int k0;   // fast path requant mode (dyadic_mode): 0 tie-free, 1 tie-free + every pre-shift 0, 2 exact tie handling
    int ck0;  // every PER-CHANNEL pre-shift (ctab, ctab_id) is zero (fast_tables bit 3): epilogue_fast<..., CK0 = true>
    int res_no_relu, res_clamp16;   // exact general RESIDUAL epilogue: no ReLU after the sum / clamp to the int16 range (hawq_conv_args)
    int ring_bytes;  // LDS bytes of the operand ring actually allocated (fewer stages when the K loop is shorter than the ring)
    int in_planar, out_planar;  // activation layout of in / out_q: 0 = NHWC rows, 1 = channel-group planes (hawq_mi355.h)
    int gfast;                  // general (direct) RESIDUAL epilogue with the fast contract's arithmetic: 32-bit / signed residuals whose tables the host has proved
    int in_pitch, out_pitch;    // bytes per pixel row of `in` / channels per pixel row of out_q, res_out, res_in (hawq_conv_args, ABI 4; always > 0 here)
    int res_sub;                // hawq_conv_args.out_sub = s >= 2 (else 0): the launch is a 1x1 conv of stride s (Ho, Wo, M are the subsampled grid's) and
                                // res_in, a tensor of the H x W source map, is read at pixel (n, s oy, s ox) of it; or res_sub (hawq_res_sub) = s: `in` is
                                // dense over the launch's own grid and res_in alone lives on the res_H x res_W map, read at (n, s oy, s ox)
    int res_H, res_W;           // the map res_in lives on (H x W unless res_sub says otherwise: then H2 x W2)
    int dbg;  // HAWQ_DBG ablation bits (timing experiments only): 1 = skip operand loads, 2 = skip MFMAs
    long long *dbgbuf;  // HAWQ_DBG & 128: per-phase cycle sums of workgroup 0 / wave 0 (band kernel)
};

namespace {

template <int BM_, int BN_, int WM_, int WN_, int NS_, int KSUB_ = 1, int MINB_ = 2, int KG_ = 1>
struct Cfg {
    static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_;
    static constexpr int MINB = MINB_;       // waves per SIMD the register allocation must allow (launch_bounds)
    static constexpr int NS = NS_;           // LDS ring stages of the asynchronous (global_load_lds) pipeline
    static constexpr int KSUB = KSUB_;       // 64-channel sub-chunks per ring stage (one barrier per stage)
    // KG > 1: intra-workgroup split-K.  KG groups of WM x WN waves each own the sub-chunks sub % KG == group of every ring
    // stage - they issue their LDS-DMA and run their MFMAs - and the partial accumulators are summed through LDS before
    // the epilogue.  For the long-K, few-pixel layers (reduce convs of stages 3-4, FC): the K loop of a tile is bound by
    // the per-wave LDS-DMA rate, so KG x the issuing waves per tile shortens it almost KG-fold.
    static constexpr int KG = KG_;
    static constexpr int NWG = WM_ * WN_;    // waves per K group
    static constexpr int NW = NWG * KG;      // waves per workgroup
    static constexpr int NT = NW * 64;       // threads per workgroup
    static constexpr int NTG = NWG * 64;     // threads per K group
    static constexpr int RPP = NTG / 4;      // operand rows staged per pass of a K group (4 lanes x 16 B per 64-B row)
    static constexpr int PT = BM / WM / 32;  // pixel MFMA tiles per wave
    static constexpr int CT = BN / WN / 32;  // channel MFMA tiles per wave
    static constexpr int AL = BM / RPP;      // 16-B A loads per thread per sub-chunk
    static constexpr int WL = BN / RPP;
    static constexpr int STAGE_BYTES = KSUB * (BM + BN) * 64;
    static constexpr int LDS_BYTES = NS * STAGE_BYTES;  // the register-staged path uses the first two stages
    static_assert(NW == 4 || NW == 8 || NW == 16, "4, 8 or 16 waves per workgroup");
    static_assert(BM % RPP == 0 && BN % RPP == 0, "tile rows must fill whole staging passes");
    static_assert(KSUB % KG == 0 && (KG == 1 || BM * BN * 4 <= LDS_BYTES), "split-K: sub-chunks per group, partial sums staged on the ring");
};

// 8 bytes of hawq4 (16 channels) -> 16 int8.  Unsigned: zero-extended.  Signed weights come
// out as value*16 (nibble moved to the top of its byte); the accumulator is shifted back by 4
// after the K loop, which is exact.
template <bool SIGNED16>
__device__ __forceinline__ v4i unpack16(unsigned x0, unsigned x1) {
    v4i r;
    if (SIGNED16) {
        r.x = (int)((x0 << 4) & 0xF0F0F0F0u);
        r.y = (int)(x0 & 0xF0F0F0F0u);
        r.z = (int)((x1 << 4) & 0xF0F0F0F0u);
        r.w = (int)(x1 & 0xF0F0F0F0u);
    } else {
        r.x = (int)(x0 & 0x0F0F0F0Fu);
        r.y = (int)((x0 >> 4) & 0x0F0F0F0Fu);
        r.z = (int)(x1 & 0x0F0F0F0Fu);
        r.w = (int)((x1 >> 4) & 0x0F0F0F0Fu);
    }
    return r;
}

template <int BITS>
__device__ __forceinline__ v4i load_chunk16(const uint8_t *p, bool valid) {
    v4i z = {0, 0, 0, 0};
    if (!valid) return z;
    if (BITS == 8) return *reinterpret_cast<const v4i *>(p);
    v2i t = *reinterpret_cast<const v2i *>(p);
    z.x = t.x;
    z.y = t.y;
    return z;
}

// One GEMM segment: acc[ct][pt] += W_tile * X_tile over all taps and input channels.
template <class C, int A_BITS, int W_BITS>
__device__ __forceinline__ void gemm_segment(v16i (&acc)[C::CT][C::PT], const uint8_t *__restrict__ in,
                                             const uint8_t *__restrict__ wgt, int H, int W, int Cin, int KH,
                                             int KW, int stride, int pad, int Ho, int Wo, int M, int Cout,
                                             int m0, int c0, char *smem, int apitch) {
    // apitch: bytes from one pixel row of `in` to the next (Cin * A_BITS / 8 when dense)
    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int wave_m = wave % C::WM, wave_c = wave / C::WM;
    const int lrow = t >> 2, lslot = t & 3;
    constexpr int ABYTES = A_BITS == 8 ? 16 : 8;  // bytes per 16 channels in global memory
    constexpr int WBYTES = W_BITS == 8 ? 16 : 8;

    // per-thread im2col row bookkeeping
    int pix_base[C::AL], iy0[C::AL], ix0[C::AL];
    bool mval[C::AL];
#pragma unroll
    for (int i = 0; i < C::AL; ++i) {
        const int m = m0 + lrow + C::RPP * i;
        mval[i] = m < M;
        const int mm = mval[i] ? m : 0;
        const int n = mm / (Ho * Wo);
        const int r = mm - n * (Ho * Wo);
        const int oy = r / Wo, ox = r - oy * Wo;
        iy0[i] = oy * stride - pad;
        ix0[i] = ox * stride - pad;
        pix_base[i] = (n * H + iy0[i]) * W + ix0[i];
    }
    const int taps = KH * KW;
    const int cchunks = Cin >> 6;
    const int nk = taps * cchunks;
    const size_t wrow_bytes = (size_t)taps * Cin * W_BITS / 8;

    char *ldsA = smem;                 // [2][BM][64]
    char *ldsW = smem + 2 * C::BM * 64;  // [2][BN][64]

    v4i ra[C::AL], rw[C::WL];
    int kh = 0, kw = 0, cc = 0;  // coordinates of the chunk being LOADED

    auto load_regs = [&]() {
#pragma unroll
        for (int i = 0; i < C::AL; ++i) {
            const int iy = iy0[i] + kh, ix = ix0[i] + kw;
            const bool v = mval[i] && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
            const size_t off = (size_t)(pix_base[i] + kh * W + kw) * apitch + (size_t)(cc << 6) * A_BITS / 8 + lslot * ABYTES;
            ra[i] = load_chunk16<A_BITS>(in + (v ? off : 0), v);
        }
#pragma unroll
        for (int j = 0; j < C::WL; ++j) {
            const int c = c0 + lrow + C::RPP * j;
            const bool v = c < Cout;
            const size_t off = (size_t)c * wrow_bytes + ((size_t)((kh * KW + kw) * Cin + (cc << 6))) * W_BITS / 8 +
                               lslot * WBYTES;
            rw[j] = load_chunk16<W_BITS>(wgt + (v ? off : 0), v);
        }
        if (++cc == cchunks) {
            cc = 0;
            if (++kw == KW) {
                kw = 0;
                ++kh;
            }
        }
    };
    auto store_lds = [&](int buf) {
#pragma unroll
        for (int i = 0; i < C::AL; ++i) {
            v4i v = ra[i];
            if (A_BITS == 4) v = unpack16<false>((unsigned)v.x, (unsigned)v.y);
            *reinterpret_cast<v4i *>(ldsA + buf * C::BM * 64 + lds_off(lrow + C::RPP * i, lslot)) = v;
        }
#pragma unroll
        for (int j = 0; j < C::WL; ++j) {
            v4i v = rw[j];
            if (W_BITS == 4) v = unpack16<true>((unsigned)v.x, (unsigned)v.y);
            *reinterpret_cast<v4i *>(ldsW + buf * C::BN * 64 + lds_off(lrow + C::RPP * j, lslot)) = v;
        }
    };

    const int l31 = lane & 31, h = lane >> 5;
    int arow[C::PT], wrow[C::CT];
#pragma unroll
    for (int p = 0; p < C::PT; ++p) arow[p] = wave_m * (C::PT * 32) + p * 32 + l31;
#pragma unroll
    for (int c = 0; c < C::CT; ++c) wrow[c] = wave_c * (C::CT * 32) + c * 32 + cperm(l31);

    load_regs();
    store_lds(0);
    __syncthreads();
    for (int k = 0; k < nk; ++k) {
        const int buf = k & 1;
        if (k + 1 < nk) load_regs();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int slot = 2 * ks + h;
            v4i wf[C::CT], af[C::PT];
#pragma unroll
            for (int c = 0; c < C::CT; ++c)
                wf[c] = *reinterpret_cast<const v4i *>(ldsW + buf * C::BN * 64 + lds_off(wrow[c], slot));
#pragma unroll
            for (int p = 0; p < C::PT; ++p)
                af[p] = *reinterpret_cast<const v4i *>(ldsA + buf * C::BM * 64 + lds_off(arow[p], slot));
#pragma unroll
            for (int c = 0; c < C::CT; ++c)
#pragma unroll
                for (int p = 0; p < C::PT; ++p)
                    acc[c][p] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[c], af[p], acc[c][p], 0, 0, 0);
        }
        if (k + 1 < nk) store_lds(buf ^ 1);
        __syncthreads();
    }
    if (W_BITS == 4) {
#pragma unroll
        for (int c = 0; c < C::CT; ++c)
#pragma unroll
            for (int p = 0; p < C::PT; ++p)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[c][p][r] >>= 4;
    }
}

// ------------------------------------------------------------------------------------------
// Asynchronous int8 x int8 pipeline: both operand tiles of every K chunk are streamed
// global -> LDS with global_load_lds (no VGPR staging, no ds_write) into an NS-stage ring, NS-1
// chunks ahead of the MFMAs.  One s_barrier per chunk: [wait chunk k landed] [barrier: everyone is
// also done reading the stage chunk k+NS-1 will overwrite] [issue chunk k+NS-1] [MFMA chunk k].
// The LDS image is lane-linear (16 rows x 64 B per wave instruction), so the XOR swizzle that keeps
// the fragment reads conflict-free is applied to the per-lane SOURCE address; padding taps and
// rows beyond M read a 16-byte zero page.  With a second branch (identity conv) its chunks simply
// continue the same chunk sequence and accumulate into acc2, so its loads overlap the first
// branch's MFMAs.
__device__ __attribute__((aligned(16))) const int g_zero16[4] = {0, 0, 0, 0};


// NIB: both operands are hawq4 nibble-packed.  A ring-stage row still holds 64 BYTES (= 128 channels), the
// packed bytes travel through LDS untouched and every fragment (8 B = 16 channels per lane) is unpacked to
// int8 in registers right before its MFMA (activations zero-extended, weights as value*16 with the
// accumulators shifted back by 4 at the end - exact).  Needs Cin % 128 == 0 (launcher-checked).
// RANGE (cross-workgroup split-K, conv_splitk.hip): only ring stages [kb, ke) of the chunk sequence run; a range lies inside one
// branch.  PLANAR: the first branch reads channel-group planes [Cin / 16][N*H*W][16 B] (in_planar) instead of NHWC rows.
template <class C, bool DUAL, bool NIB, bool RANGE = false, bool PLANAR = false>
__device__ __forceinline__ void gemm_pipeline(v16i (&acc)[C::CT][C::PT], v16i (&acc2)[DUAL ? C::CT : 1][DUAL ? C::PT : 1],
                                              const ConvP &p, int m0, int c0, char *smem, int kb = 0, int ke = 0) {
    constexpr int CSH = NIB ? 7 : 6;  // log2(channels per 64-byte chunk)
    constexpr int NS = C::NS, L = C::AL + C::WL, STAGE = C::STAGE_BYTES;
    static_assert((NS - 2) * L * C::KSUB / C::KG <= 60, "vmcnt range");
    const int t = threadIdx.x;
    const int lane = t & 63, wave = (t >> 6) % C::NWG, kg = (t >> 6) / C::NWG;   // wave inside its K group, K group
    const int wave_m = wave % C::WM, wave_c = wave / C::WM;
    const int tg = t % C::NTG;                                                    // thread inside its K group
    const int lrow = tg >> 2, lslot = tg & 3;
    const char *zero = reinterpret_cast<const char *>(g_zero16);

    // im2col bookkeeping of this thread's rows (first branch) and of the second branch's 1x1/stride-s2 rows
    int pix_base[C::AL], iy0[C::AL], ix0[C::AL], pix2[DUAL ? C::AL : 1];
    bool mval[C::AL];
    int asw[C::AL];  // source slot (16-B unit) after the swizzle
#pragma unroll
    for (int i = 0; i < C::AL; ++i) {
        const int row = lrow + C::RPP * i;
        const int m = m0 + row;
        mval[i] = m < p.M;
        const int mm = mval[i] ? m : 0;
        const int n = mm / (p.Ho * p.Wo);
        const int r = mm - n * (p.Ho * p.Wo);
        const int oy = r / p.Wo, ox = r - oy * p.Wo;
        iy0[i] = oy * p.stride - p.pad;
        ix0[i] = ox * p.stride - p.pad;
        pix_base[i] = (n * p.H + iy0[i]) * p.W + ix0[i];
        if (DUAL) pix2[DUAL ? i : 0] = (n * p.H2 + oy * p.stride2) * p.W2 + ox * p.stride2;
        asw[i] = (lslot ^ ((row >> 2) & 3)) << 4;
    }
    int wsw[C::WL];
#pragma unroll
    for (int j = 0; j < C::WL; ++j) wsw[j] = (lslot ^ (((lrow + C::RPP * j) >> 2) & 3)) << 4;

    const int taps = p.KH * p.KW, cch1 = p.Cin >> CSH;
    const int nk1 = taps * cch1, nk2 = DUAL ? (p.Cin2 >> CSH) : 0, nk = nk1 + nk2;
    const int rowb1 = NIB ? p.Cin >> 1 : p.Cin, rowb2 = DUAL ? (NIB ? p.Cin2 >> 1 : p.Cin2) : 0;  // bytes per pixel / tap row
    const size_t wrow1 = (size_t)taps * rowb1, wrow2 = (size_t)rowb2;

    constexpr int KSUB = C::KSUB, SUBB = (C::BM + C::BN) * 64;  // bytes of one 64-channel sub-chunk (A rows, then W rows)
    int kh = 0, kw = 0, cc = 0, jissue = 0, istage = 0;  // coordinates of the next sub-chunk to ISSUE
    if constexpr (RANGE) {
        jissue = kb * KSUB;
        if (jissue < nk1) {
            const int tap = jissue / cch1;
            cc = jissue - tap * cch1, kh = tap / p.KW, kw = tap - (tap / p.KW) * p.KW;
        }
    }
    const size_t plane = PLANAR ? (size_t)p.N * p.H * p.W * 16 : 0;   // bytes of one 16-channel plane
    auto issue_sub = [&](int sub) {
        char *sa = smem + istage * STAGE + sub * SUBB + wave * 1024;  // + i * RPP * 64: RPP rows x 64 B per pass
        char *sw = sa + C::BM * 64;
        const bool mine = C::KG == 1 || (sub % C::KG) == kg;           // split-K: the sub-chunk's own group loads it
        if (!mine) {
            if (!DUAL || jissue < nk1) {
                if (++cc == cch1) {
                    cc = 0;
                    if (++kw == p.KW) {
                        kw = 0;
                        ++kh;
                    }
                }
            }
            ++jissue;
            return;
        }
        if (!DUAL || jissue < nk1) {
            const int tap_off = kh * p.W + kw;
#pragma unroll
            for (int i = 0; i < C::AL; ++i) {
                const int iy = iy0[i] + kh, ix = ix0[i] + kw;
                const bool v = mval[i] && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
                const char *src = !v ? zero
                                  : PLANAR ? (const char *)p.in + (size_t)((cc << 2) + (asw[i] >> 4)) * plane + (size_t)(pix_base[i] + tap_off) * 16
                                           : (const char *)p.in + (size_t)(pix_base[i] + tap_off) * p.in_pitch + (cc << 6) + asw[i];
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                                 (__attribute__((address_space(3))) void *)(sa + i * (C::RPP * 64)), 16, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < C::WL; ++j) {
                const char *src = (const char *)p.wgt + (size_t)(c0 + lrow + C::RPP * j) * wrow1 +
                                  (size_t)((kh * p.KW + kw) * rowb1 + (cc << 6)) + wsw[j];
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                                 (__attribute__((address_space(3))) void *)(sw + j * (C::RPP * 64)), 16, 0, 0);
            }
            if (++cc == cch1) {
                cc = 0;
                if (++kw == p.KW) {
                    kw = 0;
                    ++kh;
                }
            }
        } else {
            const int c2 = jissue - nk1;
#pragma unroll
            for (int i = 0; i < C::AL; ++i) {
                const char *src = mval[i] ? (const char *)p.in2 + (size_t)pix2[DUAL ? i : 0] * rowb2 + (c2 << 6) + asw[i] : zero;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                                 (__attribute__((address_space(3))) void *)(sa + i * (C::RPP * 64)), 16, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < C::WL; ++j) {
                const char *src = (const char *)p.wgt2 + (size_t)(c0 + lrow + C::RPP * j) * wrow2 + (size_t)(c2 << 6) + wsw[j];
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                                 (__attribute__((address_space(3))) void *)(sw + j * (C::RPP * 64)), 16, 0, 0);
            }
        }
        ++jissue;
    };
    auto issue = [&]() {  // one ring stage = KSUB consecutive sub-chunks (nk1 and nk2 are multiples of KSUB)
#pragma unroll
        for (int sub = 0; sub < KSUB; ++sub) issue_sub(sub);
        if (++istage == NS) istage = 0;
    };

    const int l31 = lane & 31, h = lane >> 5;
    int arow[C::PT], wrow[C::CT];
#pragma unroll
    for (int q = 0; q < C::PT; ++q) arow[q] = wave_m * (C::PT * 32) + q * 32 + l31;
#pragma unroll
    for (int c = 0; c < C::CT; ++c) wrow[c] = wave_c * (C::CT * 32) + c * 32 + cperm(l31);

    auto compute = [&](auto &a, int stage) {
        // fragments of K-step s+1 are fetched from LDS while the MFMAs of K-step s run
        v4i wf[2][C::CT], af[2][C::PT];
        constexpr int SPS = NIB ? 4 : 2;  // MFMA K-steps per 64-byte sub-chunk
        auto fetch = [&](int s, int buf) {
            const char *ldsA = smem + stage * STAGE + (s / SPS) * SUBB, *ldsW = ldsA + C::BM * 64;
            if constexpr (NIB) {
                const int slot = s % SPS;  // 16 packed bytes = 32 channels; lane-half h takes 8 of them
#pragma unroll
                for (int c = 0; c < C::CT; ++c) {
                    const v2i t2 = *reinterpret_cast<const v2i *>(ldsW + lds_off(wrow[c], slot) + h * 8);
                    wf[buf][c] = unpack16<true>((unsigned)t2.x, (unsigned)t2.y);
                }
#pragma unroll
                for (int q = 0; q < C::PT; ++q) {
                    const v2i t2 = *reinterpret_cast<const v2i *>(ldsA + lds_off(arow[q], slot) + h * 8);
                    af[buf][q] = unpack16<false>((unsigned)t2.x, (unsigned)t2.y);
                }
                return;
            }
            const int slot = 2 * (s & 1) + h;
#pragma unroll
            for (int c = 0; c < C::CT; ++c) wf[buf][c] = *reinterpret_cast<const v4i *>(ldsW + lds_off(wrow[c], slot));
#pragma unroll
            for (int q = 0; q < C::PT; ++q) af[buf][q] = *reinterpret_cast<const v4i *>(ldsA + lds_off(arow[q], slot));
        };
        // the K-steps this wave owns: all of the stage, or (split-K) those of the sub-chunks sub % KG == kg
        constexpr int NOWN = SPS * KSUB / C::KG;
        auto step_of = [&](int o) { return C::KG == 1 ? o : ((o / SPS) * C::KG + kg) * SPS + (o % SPS); };
        fetch(step_of(0), 0);
#pragma unroll
        for (int o = 0; o < NOWN; ++o) {
            if (o + 1 < NOWN) fetch(step_of(o + 1), (o + 1) & 1);
#pragma unroll
            for (int c = 0; c < C::CT; ++c)
#pragma unroll
                for (int q = 0; q < C::PT; ++q)
                    a[c][q] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[o & 1][c], af[o & 1][q], a[c][q], 0, 0, 0);
        }
    };

    const int ns1 = nk1 / KSUB, nst = RANGE ? ke : nk / KSUB;  // ring stages of the first branch / end of the stages run
    const int kfirst = RANGE ? kb : 0;
#pragma unroll
    for (int j = 0; j < NS - 1; ++j)
        if (kfirst + j < nst) issue();
    int cstage = 0;
    constexpr int LS = L * KSUB / C::KG;  // loads per thread per stage
    auto step = [&](auto &a, int k) {
        // stage k must have landed: at most min(NS-2, stages issued after k) stages may stay in flight
        const int after = min(NS - 2, nst - 1 - k);
        if (after >= NS - 2) {
            wait_vmcnt<(NS - 2) * LS>();  // steady state
        } else {  // tail: fewer stages behind stage k, wait for exactly those to remain
            switch (after) {
                case 5: wait_vmcnt<(NS > 6 ? 5 : 0) * LS>(); break;
                case 4: wait_vmcnt<(NS > 5 ? 4 : 0) * LS>(); break;
                case 3: wait_vmcnt<(NS > 4 ? 3 : 0) * LS>(); break;
                case 2: wait_vmcnt<(NS > 3 ? 2 : 0) * LS>(); break;
                case 1: wait_vmcnt<(NS > 2 ? 1 : 0) * LS>(); break;
                default: wait_vmcnt<0>(); break;
            }
        }
        __builtin_amdgcn_s_barrier();
        if (jissue < (RANGE ? nst * KSUB : nk) && !HAWQ_DBG_BIT(p.dbg, 1)) issue();
        if (!HAWQ_DBG_BIT(p.dbg, 2)) compute(a, cstage);
        if (++cstage == NS) cstage = 0;
    };
    for (int k = kfirst; k < (RANGE ? min(ns1, nst) : ns1); ++k) step(acc, k);
    if constexpr (DUAL)
        for (int k = RANGE ? max(ns1, kfirst) : ns1; k < nst; ++k) step(acc2, k);
    if constexpr (NIB) {  // weights were unpacked as value*16
#pragma unroll
        for (int c = 0; c < C::CT; ++c)
#pragma unroll
            for (int q = 0; q < C::PT; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    acc[c][q][r] >>= 4;
                    if constexpr (DUAL) acc2[DUAL ? c : 0][DUAL ? q : 0][r] >>= 4;
                }
    }
    __syncthreads();  // all MFMA fragment reads done: the ring may be reused by the epilogue
}

// BITS: 0 = decide at run time (generic kernels), else (a_bits << 4) | w_bits.
template <class C, int BITS>
__device__ __forceinline__ void run_segment(v16i (&acc)[C::CT][C::PT], const uint8_t *in, const uint8_t *wgt,
                                            int a_bits, int w_bits, int H, int W, int Cin, int KH, int KW,
                                            int stride, int pad, int Ho, int Wo, int M, int Cout, int m0, int c0,
                                            char *smem, int apitch) {
    if (BITS == 0x88 || (BITS == 0 && a_bits == 8 && w_bits == 8))
        gemm_segment<C, 8, 8>(acc, in, wgt, H, W, Cin, KH, KW, stride, pad, Ho, Wo, M, Cout, m0, c0, smem, apitch);
    else if (BITS == 0x44 || (BITS == 0 && a_bits == 4 && w_bits == 4))
        gemm_segment<C, 4, 4>(acc, in, wgt, H, W, Cin, KH, KW, stride, pad, Ho, Wo, M, Cout, m0, c0, smem, apitch);
    else if (BITS == 0x84 || (BITS == 0 && a_bits == 8 && w_bits == 4))
        gemm_segment<C, 8, 4>(acc, in, wgt, H, W, Cin, KH, KW, stride, pad, Ho, Wo, M, Cout, m0, c0, smem, apitch);
    else
        gemm_segment<C, 4, 8>(acc, in, wgt, H, W, Cin, KH, KW, stride, pad, Ho, Wo, M, Cout, m0, c0, smem, apitch);
}

__device__ __forceinline__ v4i ld4(const int32_t *p) { return *reinterpret_cast<const v4i *>(p); }

// pixel row of res_in that output pixel `pix` (< M) adds: its own, or with out_sub / res_sub its source pixel on the res_H x res_W map
__device__ __forceinline__ size_t res_row(const ConvP &p, int pix) {
    if (p.res_sub > 1) {
        const int hw = p.Ho * p.Wo, n = pix / hw, r = pix - n * hw, oy = r / p.Wo, ox = r - oy * p.Wo;
        return ((size_t)n * p.res_H + (size_t)oy * p.res_sub) * p.res_W + (size_t)ox * p.res_sub;
    }
    return (size_t)pix;
}


// =============================================================== exact general epilogue (BITS == 0)
// Direct per-lane global accesses, dyadic_rne everywhere: any e in [1,62], any pre-shift, ties
// handled, 16- or 32-bit residuals, run-time operand widths.  Slow but always right.
template <class C, int EPI, bool DUAL>
__device__ __forceinline__ void epilogue_generic(const ConvP &p, v16i (&acc)[C::CT][C::PT],
                                                 v16i (&acc2)[DUAL ? C::CT : 1][DUAL ? C::PT : 1], int m0, int c0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wave_m = wave % C::WM, wave_c = wave / C::WM;
    const int l31 = lane & 31, h = lane >> 5;
    size_t rrow[C::PT];   // pixel row of res_in per pixel tile (out_sub: the source pixel), worked out once, outside the unrolled epilogue
#pragma unroll
    for (int q = 0; q < C::PT; ++q) {
        const int pix = m0 + wave_m * (C::PT * 32) + q * 32 + l31;
        rrow[q] = (EPI == HAWQ_EPI_RESIDUAL && !DUAL) ? res_row(p, pix < p.M ? pix : 0) : (size_t)pix;
    }
#pragma unroll
    for (int c = 0; c < C::CT; ++c) {
        const int ch = c0 + wave_c * (C::CT * 32) + c * 32 + h * 16;
#pragma unroll
        for (int q = 0; q < C::PT; ++q) {
            const int pix = m0 + wave_m * (C::PT * 32) + q * 32 + l31;
            if (pix >= p.M) continue;
            // RAW / DEQUANT address the dense [M][Cout] / [M][ldo] tensors; REQUANT / RESIDUAL rows are out_pitch channels apart (ABI 4)
            constexpr bool PITCHED = EPI == HAWQ_EPI_REQUANT || EPI == HAWQ_EPI_RESIDUAL;
            const int opitch = PITCHED ? p.out_pitch : p.Cout;
            const size_t elem = (size_t)pix * opitch + ch;
            const size_t relem = rrow[q] * opitch + ch;   // (res_in rows: out_sub)
            bool ovf = false;
            int qw[4] = {0, 0, 0, 0};   // int8 output: the lane's 16 channels leave as ONE 16-byte store after the loop
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (PITCHED && ch + 4 * g >= opitch) continue;   // beyond the stored row: nothing to compute, nothing to write
                const v4i b4 = ld4(p.bias + ch + 4 * g);
                const int bb[4] = {b4.x, b4.y, b4.z, b4.w};
                int v[4], qv[4] = {0, 0, 0, 0}, o[4] = {0, 0, 0, 0};
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = acc[c][q][4 * g + j] + bb[j];
                if constexpr (EPI == HAWQ_EPI_RAW) {
                    v4i w = {v[0], v[1], v[2], v[3]};
                    reinterpret_cast<v4i *>(p.out_acc + elem)[g] = w;
                } else if constexpr (EPI == HAWQ_EPI_DEQUANT) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (ch + 4 * g + j < p.n_valid)
                            p.out_f32[(size_t)pix * p.ldo + ch + 4 * g + j] = (float)v[j] * p.fscale[ch + 4 * g + j];
                } else if (p.n_valid > 0 && ch + 4 * g >= p.n_valid) {
                    // padding channels (caller's promise: zero weights / bias / tables, zero identity): zeros without the arithmetic.
                    // Narrow layers padded to the 64-channel tile (MobileNetV2's 16 / 24 / 32-channel projections) spend most of
                    // this exact epilogue's 64-bit requants on them otherwise.
                    if (EPI == HAWQ_EPI_RESIDUAL && p.res_out) {
                        if (p.res_out_bits == 16) reinterpret_cast<v2i *>((uint16_t *)p.res_out + elem)[g] = v2i{0, 0};
                        else reinterpret_cast<v4i *>((int32_t *)p.res_out + elem)[g] = v4i{0, 0, 0, 0};
                    }
                    if ((EPI == HAWQ_EPI_REQUANT || p.out_q) && p.out_bits == 4 && !(g & 1)) reinterpret_cast<uint32_t *>((uint8_t *)p.out_q + (elem >> 1) + (g >> 1) * 4)[0] = 0u;
                } else if (EPI == HAWQ_EPI_RESIDUAL && !DUAL && p.gfast) {
                    // Fast-contract arithmetic on the direct epilogue (round 4): 32-bit / signed residual tensors (MobileNetV2's carriers)
                    // keep this epilogue's per-lane accesses, but every table has been lifted and bounded by the host, so a requant is
                    // shift + v_mad_i64_i32 + shift against the fused constants of `ctab` (bias folded in) instead of dyadic_rne's
                    // ~15 instructions; p.k0 == 2 keeps the exact round-half-even correction where a tie could not be excluded.
                    const bool tie = p.k0 == 2;
                    const DyNt dids = dynt_prepare(p.m_id_s, p.e_id_s), dq = dynt_prepare(p.mq, p.eq);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const v4i t4 = ld4(p.ctab + (size_t)(ch + 4 * g + j) * 4);
                        DyNt dm;
                        dm.m = t4.x, dm.s = t4.y & 31, dm.k = t4.y >> 8;
                        dm.add = (long long)(((unsigned long long)(unsigned)t4.w << 32) | (unsigned)t4.z);
                        const int av = acc[c][q][4 * g + j];
                        int ov = tie ? dyadic_tie(av, dm) : dyadic_nt(av, dm);
                        if (p.res_in) {
                            const int r = p.res_in_bits == 16 ? (int)((const uint16_t *)p.res_in)[relem + 4 * g + j]
                                                              : ((const int32_t *)p.res_in)[relem + 4 * g + j];
                            ov += tie ? dyadic_tie(r, dids) : dyadic_nt(r, dids);
                        }
                        if (!p.res_no_relu) ov = max(ov, 0);
                        if (p.res_clamp16) ov = clampi(ov, -32768, 32767);
                        o[j] = ov;
                        qv[j] = clampi(tie ? dyadic_tie(ov, dq) : dyadic_nt(ov, dq), p.q_lo, p.q_hi);
                        ovf |= ov > 65535;
                    }
                    if (p.res_out) {
                        if (p.res_out_bits == 16) {
                            v2i w = {min(o[0], 65535) | (min(o[1], 65535) << 16), min(o[2], 65535) | (min(o[3], 65535) << 16)};
                            reinterpret_cast<v2i *>((uint16_t *)p.res_out + elem)[g] = w;
                        } else {
                            v4i w = {o[0], o[1], o[2], o[3]};
                            reinterpret_cast<v4i *>((int32_t *)p.res_out + elem)[g] = w;
                        }
                    }
                    if (p.out_q) {
                        if (p.out_bits == 8) {
                            qw[g] = (int)pack4_i8(qv[0], qv[1], qv[2], qv[3]);
                        } else {
                            uint8_t *dst = (uint8_t *)p.out_q + (elem >> 1) + (g >> 1) * 4;
#pragma unroll
                            for (int j = 0; j < 4; ++j) dst[j] = (g & 1) ? (uint8_t)((dst[j] & 0x0f) | (qv[j] << 4)) : (uint8_t)(qv[j] & 0x0f);
                        }
                    }
                } else {
                    const v4i m4 = ld4(p.m + ch + 4 * g), e4 = ld4(p.e + ch + 4 * g);
                    const int mm[4] = {m4.x, m4.y, m4.z, m4.w}, ee[4] = {e4.x, e4.y, e4.z, e4.w};
                    if constexpr (EPI == HAWQ_EPI_REQUANT) {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            qv[j] = clampi(dyadic_rne(p.relu ? max(v[j], 0) : v[j], mm[j], ee[j]), p.q_lo, p.q_hi);
                    } else {
                        int idv[4];
                        if constexpr (DUAL) {
                            const v4i b2 = ld4(p.bias2 + ch + 4 * g), mi = ld4(p.m_id + ch + 4 * g),
                                      ei = ld4(p.e_id + ch + 4 * g);
                            const int bb2[4] = {b2.x, b2.y, b2.z, b2.w}, m1[4] = {mi.x, mi.y, mi.z, mi.w},
                                      e1[4] = {ei.x, ei.y, ei.z, ei.w};
#pragma unroll
                            for (int j = 0; j < 4; ++j) idv[j] = dyadic_rne(acc2[DUAL ? c : 0][DUAL ? q : 0][4 * g + j] + bb2[j], m1[j], e1[j]);
                        } else if (p.res_in) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const int r = p.res_in_bits == 16 ? (int)((const uint16_t *)p.res_in)[relem + 4 * g + j]
                                                                  : ((const int32_t *)p.res_in)[relem + 4 * g + j];
                                idv[j] = dyadic_rne(r, p.m_id_s, p.e_id_s);
                            }
                        } else {   // no identity branch (MobileNetV2 units that change shape): fixedpoint_fn case 0
#pragma unroll
                            for (int j = 0; j < 4; ++j) idv[j] = 0;
                        }
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            o[j] = dyadic_rne(v[j], mm[j], ee[j]) + idv[j];          // no clamp with an identity: quant_utils.py:456
                            if (!p.res_no_relu) o[j] = max(o[j], 0);
                            if (p.res_clamp16) o[j] = clampi(o[j], -32768, 32767);   // case 0 clamps to its 16-bit range (quant_utils.py:409-413)
                            qv[j] = clampi(dyadic_rne(o[j], p.mq, p.eq), p.q_lo, p.q_hi);
                            ovf |= o[j] > 65535;
                        }
                        if (p.res_out) {
                            if (p.res_out_bits == 16) {
                                v2i w = {min(o[0], 65535) | (min(o[1], 65535) << 16), min(o[2], 65535) | (min(o[3], 65535) << 16)};
                                reinterpret_cast<v2i *>((uint16_t *)p.res_out + elem)[g] = w;
                            } else {
                                v4i w = {o[0], o[1], o[2], o[3]};
                                reinterpret_cast<v4i *>((int32_t *)p.res_out + elem)[g] = w;
                            }
                        }
                    }
                    if (EPI == HAWQ_EPI_REQUANT || p.out_q) {
                        if (p.out_bits == 8) {
                            qw[g] = (int)pack4_i8(qv[0], qv[1], qv[2], qv[3]);
                        } else {  // hawq4: byte k of an 8-channel group = c_k | c_{k+4} << 4
                            uint8_t *dst = (uint8_t *)p.out_q + (elem >> 1) + (g >> 1) * 4;
                            if (g & 1) {
#pragma unroll
                                for (int j = 0; j < 4; ++j) dst[j] = (uint8_t)((dst[j] & 0x0f) | (qv[j] << 4));
                            } else {
#pragma unroll
                                for (int j = 0; j < 4; ++j) dst[j] = (uint8_t)(qv[j] & 0x0f);
                            }
                        }
                    }
                }
            }
            if constexpr (PITCHED) {
                // (rows are multiples of 16 channels and ch is one: the lane's 16 bytes are either entirely inside the row or not at all)
                if ((EPI == HAWQ_EPI_REQUANT || p.out_q) && p.out_bits == 8 && ch < opitch)
                    *reinterpret_cast<v4i *>((char *)p.out_q + elem) = v4i{qw[0], qw[1], qw[2], qw[3]};
            }
            if (EPI == HAWQ_EPI_RESIDUAL && ovf && p.res_out && p.res_out_bits == 16) atomicOr(p.flags, 1);
        }
    }
}

// =============================================================== fast epilogue (BITS != 0)
// Host-proved tables (see dyadic_nt), uint16 residuals, everything staged through LDS so that
// each global access of the residual / output tensors is a full-line coalesced 16 B-per-lane access:
//   res tile [BM][BN] uint16 behind the operand staging buffers (filled asynchronously with
//   global_load_lds before the K loop, overwritten in place with the new residual),
//   q tile   [BM][BN] int8 positions, aliased onto the staging buffers (free after the K loop).
// 16-B chunks are XOR-swizzled by the pixel row so that both the per-lane (one pixel, 16 channels)
// and the row-contiguous access patterns are bank-conflict free.
template <class C>
struct Stage {
    static constexpr int RCPR = C::BN / 8;   // 16-B chunks per residual-tile row (uint16)
    static constexpr int QCPR = C::BN / 16;  // 16-B chunks per q-tile row
    __device__ static __forceinline__ int rsw(int row) { return row & (RCPR - 1); }
    __device__ static __forceinline__ int qsw(int row) {
        return QCPR >= 8 ? (row & (QCPR - 1)) : ((row >> 1) & (QCPR - 1));
    }
};

template <class C>
__device__ __forceinline__ void prefetch_residual(const ConvP &p, int m0, int c0, char *res_tile) {
    using S = Stage<C>;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < (C::BM * S::RCPR + C::NT - 1) / C::NT; ++i) {
        const int base = (i * C::NW + wave) * 64;
        if (base >= C::BM * S::RCPR) break;   // (16-wave workgroups on a 64-pixel tile: half of the waves have no piece)
        const int idx = base + lane;
        const int row = idx / S::RCPR, j = idx % S::RCPR;
        const size_t grow = res_row(p, (m0 + row < p.M) ? m0 + row : m0);
        const char *src = (const char *)p.res_in + (grow * p.Cout + c0) * 2 + ((j ^ S::rsw(row)) << 4);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)(res_tile + base * 16), 16, 0, 0);
    }
}

// MODE: see dyadic_mode (0 = tie-free tables, 2 = exact tie handling for every table; 1 = tie-free and shift-free is
// implemented but not instantiated: as a run-time variant it cost registers (spills in the 64x64 dual kernels) for
// a gain inside the measurement noise)
// CK0: the per-channel tables carry no pre-shift: the table word is the shift amount itself (3 VALU instructions per requantised
// accumulator fewer).  NOT instantiated: a wave-uniform branch between the two forms in every fast kernel measured neutral in the
// forward (same-plan A/B 93.08 vs 93.04 k img/s, profiles/r03_valu_trims.md) - these epilogues are not VALU-bound; the fused
// expand -> reduce kernels (fused_er.hip / fused_wp.hip), which are, have their own all-k-zero instantiations
template <class C, int EPI, bool DUAL, int MODE = 0, bool CK0 = false>
__device__ __forceinline__ void epilogue_fast(const ConvP &p, v16i (&acc)[C::CT][C::PT],
                                              v16i (&acc2)[DUAL ? C::CT : 1][DUAL ? C::PT : 1], int m0, int c0,
                                              char *q_tile, char *res_tile, const char *ctab_lds,
                                              const bool active = true) {
    // active == false: a wave that owns no accumulators (band-kernel producer); it only helps with the stores
    using S = Stage<C>;
    constexpr bool RES = EPI == HAWQ_EPI_RESIDUAL;
    constexpr bool K0 = MODE == 1 || CK0;                      // per-channel tables
    constexpr int MODE_C = (CK0 && MODE == 0) ? 1 : MODE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wave_m = wave % C::WM, wave_c = (wave / C::WM) % C::WN;
    const int l31 = lane & 31, h = lane >> 5;
    const int lrow0 = wave_m * (C::PT * 32) + l31;  // tile-local pixel row of pixel tile 0
    DyNt dids = dynt_prepare(p.m_id_s, p.e_id_s), dq = dynt_prepare(p.mq, p.eq);
    asm volatile("" : "+s"(dids.add), "+s"(dq.add));   // opaque rounding constants: one v_mad_i64_i32 instead of v_mul_hi_i32 + v_add (see fused_er.hip)
    const int qhi2 = (p.q_hi & 0xffff) | (p.q_hi << 16);   // RESIDUAL: q >= 0, clamped from above as packed int16 pairs
    unsigned oor = 0;               // OR of all residual outputs: bits >= 16 set <=> uint16 overflow
    unsigned rowmask[C::PT];
#pragma unroll
    for (int q = 0; q < C::PT; ++q) rowmask[q] = (m0 + lrow0 + q * 32 < p.M) ? 0xffffffffu : 0u;
    if (active)
#pragma unroll
    for (int c = 0; c < C::CT; ++c) {
        const int lch = wave_c * (C::CT * 32) + c * 32 + h * 16;  // tile-local first channel of this lane
        // Two accumulator sets (DUAL) leave no room to keep every pixel tile's packed outputs live: walk the pixel tiles one at a
        // time there (the channel constants are re-read from LDS).  The same holds for the RESIDUAL epilogue of a kernel that must fit
        // 4 waves per SIMD (<= 128 registers: the 16-wave band kernels, the 3x3 + residual launches of ResNet18/34): with both pixel
        // tiles live it held 2 x (8 residual + 8 packed residual + 4 packed q) registers beside 64 accumulators and spilled 88-160
        // of them (round 4: found by the scratch check of tests/test_host_logic.py).
        constexpr int WPS = (C::NT / 256 > C::MINB) ? C::NT / 256 : C::MINB;   // waves per SIMD the kernel is built for
        constexpr int QPASS = (DUAL || (RES && WPS >= 4)) ? C::PT : 1, QPER = C::PT / QPASS;
#pragma unroll
        for (int qp = 0; qp < QPASS; ++qp) {
        v4i rin[C::PT][2];             // old residual values of this pass's pixel tiles (32 bytes per lane and tile)
        if constexpr (RES && !DUAL) {
#pragma unroll
            for (int qq = 0; qq < QPER; ++qq) {
                const int q = qp * QPER + qq;
                const int row = lrow0 + q * 32;
                const char *base = res_tile + row * (S::RCPR * 16);
                rin[q][0] = *reinterpret_cast<const v4i *>(base + (((lch >> 3) ^ S::rsw(row)) << 4));
                rin[q][1] = *reinterpret_cast<const v4i *>(base + ((((lch >> 3) + 1) ^ S::rsw(row)) << 4));
            }
        }
        int qpack[QPER][4];            // 16 x int8, or 2 dwords of hawq4 in [0..1]
        int rpack[QPER][RES ? 8 : 1];  // 16 x uint16
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            // fused constants {m, s, C} with C = bias*m + 2^(e-1): (acc+bias)*m + 2^(e-1) == acc*m + C
            DyNt dm[4], di[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const v4i t = *reinterpret_cast<const v4i *>(ctab_lds + (lch + 4 * g + j) * 16);
                dm[j].m = t.x, dm[j].s = K0 ? t.y : (t.y & 31), dm[j].k = K0 ? 0 : (t.y >> 8);
                dm[j].add = (long long)(((unsigned long long)(unsigned)t.w << 32) | (unsigned)t.z);
                if constexpr (DUAL) {
                    const v4i u = *reinterpret_cast<const v4i *>(ctab_lds + C::BN * 16 + (lch + 4 * g + j) * 16);
                    di[j].m = u.x, di[j].s = K0 ? u.y : (u.y & 31), di[j].k = K0 ? 0 : (u.y >> 8);
                    di[j].add = (long long)(((unsigned long long)(unsigned)u.w << 32) | (unsigned)u.z);
                } else {
                    di[j] = dids;
                }
            }
#pragma unroll
            for (int qq = 0; qq < QPER; ++qq) {
                const int q = qp * QPER + qq;
                int qv[4];
                if constexpr (!RES) {
                    // ReLU commutes with the (monotone, 0 -> 0) requantisation: it is folded into q_lo
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        qv[j] = med3i(dyadic_mode<MODE_C>(acc[c][q][4 * g + j], dm[j]), p.q_lo, p.q_hi);
                } else {
                    int idin[4], o[4];
                    if constexpr (DUAL) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) idin[j] = acc2[DUAL ? c : 0][DUAL ? q : 0][4 * g + j];
                    } else {
                        const unsigned w0 = (unsigned)rin[q][g >> 1][(g & 1) * 2], w1 = (unsigned)rin[q][g >> 1][(g & 1) * 2 + 1];
                        idin[0] = (int)(w0 & 0xffffu), idin[1] = (int)(w0 >> 16);
                        idin[2] = (int)(w1 & 0xffffu), idin[3] = (int)(w1 >> 16);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int a = dyadic_mode<MODE_C>(acc[c][q][4 * g + j], dm[j]);
                        const int b = DUAL ? dyadic_mode<MODE_C>(idin[j], di[j]) : dyadic_mode<MODE == 2 ? 2 : 0>(idin[j], di[j]);
                        o[j] = max(a + b, 0);  // no clamp: quant_utils.py:456
                        qv[j] = dyadic_mode<MODE>(o[j], dq);  // o >= 0 and m >= 0: q >= 0 >= q_lo; the upper clamp runs on the packed pairs
                    }
                    // rows beyond M hold bias-only garbage: they never reach memory and must not raise the flag
                    oor |= ((unsigned)(o[0] | o[1]) | (unsigned)(o[2] | o[3])) & rowmask[q];
                    rpack[qq][RES ? 2 * g : 0] = pack2_u16_sat(o[0], o[1]);
                    rpack[qq][RES ? 2 * g + 1 : 0] = pack2_u16_sat(o[2], o[3]);
                }
                const int w = RES ? pack4_min(qv[0], qv[1], qv[2], qv[3], qhi2) : pack4_fast(qv[0], qv[1], qv[2], qv[3]);
                if (p.out_bits == 8) {
                    qpack[qq][g] = w;
                } else if (g & 1) {  // hawq4: low nibbles = channels 0-3 of the 8-group, high = 4-7
                    qpack[qq][g >> 1] |= w << 4;
                } else {
                    qpack[qq][g >> 1] = w;
                }
            }
        }
#pragma unroll
        for (int qq = 0; qq < QPER; ++qq) {
            const int q = qp * QPER + qq;
            const int row = lrow0 + q * 32;
            if constexpr (RES) {
                char *base = res_tile + row * (S::RCPR * 16);
                v4i a = {rpack[qq][0], rpack[qq][1], rpack[qq][2], rpack[qq][3]};
                v4i b = {rpack[qq][4], rpack[qq][5], rpack[qq][6], rpack[qq][7]};
                *reinterpret_cast<v4i *>(base + (((lch >> 3) ^ S::rsw(row)) << 4)) = a;
                *reinterpret_cast<v4i *>(base + ((((lch >> 3) + 1) ^ S::rsw(row)) << 4)) = b;
            }
            char *qb = q_tile + row * (S::QCPR * 16) + (((lch >> 4) ^ S::qsw(row)) << 4);
            if (p.out_bits == 8) {
                v4i w = {qpack[qq][0], qpack[qq][1], qpack[qq][2], qpack[qq][3]};
                *reinterpret_cast<v4i *>(qb) = w;
            } else {
                v2i w = {qpack[qq][0], qpack[qq][1]};
                *reinterpret_cast<v2i *>(qb) = w;
            }
        }
        }  // qp
    }
    if (RES && (oor >> 16) != 0 && p.res_out && !HAWQ_DBG_BIT(p.dbg, ~0)) atomicOr(p.flags, 1);
    if (HAWQ_DBG_BIT(p.dbg, 8)) return;  // rows beyond M never reach memory but may flag: harmless
    __syncthreads();
    const int t = threadIdx.x;
    if constexpr (RES) {
        if (p.res_out) {
#pragma unroll
            for (int i = 0; i < (C::BM * S::RCPR + C::NT - 1) / C::NT; ++i) {
                const int idx = t + C::NT * i;
                const int row = idx / S::RCPR, j = idx % S::RCPR;
                if (idx < C::BM * S::RCPR && m0 + row < p.M) {
                    char *dst = (char *)p.res_out + ((size_t)(m0 + row) * p.Cout + c0) * 2 + ((j ^ S::rsw(row)) << 4);
                    *reinterpret_cast<v4i *>(dst) = *reinterpret_cast<const v4i *>(res_tile + idx * 16);
                }
            }
        }
    }
    if ((!RES || p.out_q) && p.out_planar) {
        // channel-group planes [C / G][M][16 B] (G = 16 int8 / 32 hawq4 channels): what the 3x3 band kernel's LDS-DMA
        // fill wants - 64 consecutive pixels of one plane are one contiguous KiB (tools/ubench/ingest_shape.hip:
        // 16-byte segments a pixel row apart reach 16 GB/s per CU, contiguous ones 57-87).  Pixel index fastest
        // across lanes: 16-B stores of consecutive pixels are contiguous in a plane.
        if (p.out_bits == 8) {
#pragma unroll
            for (int i = 0; i < (C::BM * S::QCPR + C::NT - 1) / C::NT; ++i) {
                const int idx = t + C::NT * i;
                const int ch = idx / C::BM, row = idx % C::BM;
                if (idx < C::BM * S::QCPR && m0 + row < p.M) {
                    char *dst = (char *)p.out_q + ((size_t)((c0 >> 4) + ch) * p.M + (m0 + row)) * 16;
                    *reinterpret_cast<v4i *>(dst) = *reinterpret_cast<const v4i *>(q_tile + (row * S::QCPR + (ch ^ S::qsw(row))) * 16);
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < (C::BM * (S::QCPR / 2) + C::NT - 1) / C::NT; ++i) {
                const int idx = t + C::NT * i;
                const int u = idx / C::BM, row = idx % C::BM;
                if (idx < C::BM * (S::QCPR / 2) && m0 + row < p.M) {
                    const v2i a = *reinterpret_cast<const v2i *>(q_tile + (row * S::QCPR + ((2 * u) ^ S::qsw(row))) * 16);
                    const v2i b = *reinterpret_cast<const v2i *>(q_tile + (row * S::QCPR + ((2 * u + 1) ^ S::qsw(row))) * 16);
                    const v4i w = {a.x, a.y, b.x, b.y};
                    char *dst = (char *)p.out_q + ((size_t)((c0 >> 5) + u) * p.M + (m0 + row)) * 16;
                    *reinterpret_cast<v4i *>(dst) = w;
                }
            }
        }
    } else if (!RES || p.out_q) {
#pragma unroll
        for (int i = 0; i < (C::BM * S::QCPR + C::NT - 1) / C::NT; ++i) {
            const int idx = t + C::NT * i;
            const int row = idx / S::QCPR, j = idx % S::QCPR;
            const int cofs = c0 + ((j ^ S::qsw(row)) << 4);   // first channel of this 16-channel piece
            if (idx < C::BM * S::QCPR && m0 + row < p.M && cofs < p.out_pitch) {   // (out_pitch < Cout: the row ends before the tile does, ABI 4)
                const size_t e0 = (size_t)(m0 + row) * p.out_pitch + cofs;
                if (p.out_bits == 8)
                    *reinterpret_cast<v4i *>((char *)p.out_q + e0) = *reinterpret_cast<const v4i *>(q_tile + idx * 16);
                else
                    *reinterpret_cast<v2i *>((char *)p.out_q + (e0 >> 1)) = *reinterpret_cast<const v2i *>(q_tile + idx * 16);
            }
        }
    }
}

// TIE: the launch's tables are not provably tie-free -> every requant of the fast epilogue applies the exact
// round-half-even correction (dyadic_tie).  A separate instantiation, not a run-time branch: the correction costs
// registers, and register allocation is per kernel (as a branch it pushed the 64x64 dual kernels into 44 spills).
template <class C, int EPI, bool DUAL, int BITS, int BITS2, bool TIE = false>
__global__ __launch_bounds__(C::NT, C::MINB) void conv_kernel(const ConvP p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const bool prof = HAWQ_DBG_BIT(p.dbg, 128) && p.dbgbuf;  // HAWQ_DBG=128: cycle stamps of one wave (tools/convprobe.py)
    const long long t_entry = prof ? (long long)__builtin_readcyclecounter() : 0;
    // XCD-aware tile order: consecutive workgroup ids land on different XCDs (id % 8), so give
    // each XCD a contiguous run of pixel tiles that share the same weight tile in its L2.
    const int tiles_m = (p.M + C::BM - 1) / C::BM;
    const int tiles_c = p.Cout / C::BN;
    const int nwg = tiles_m * tiles_c;
    int wg = blockIdx.x;
    {
        const int q = nwg >> 3, r = nwg & 7, xcd = wg & 7, idx = wg >> 3;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int tc = wg % tiles_c, tm = wg / tiles_c;  // channel tiles of one pixel tile are adjacent
    const int m0 = tm * C::BM, c0 = tc * C::BN;
    constexpr bool FAST = BITS != 0 && (EPI == HAWQ_EPI_REQUANT || EPI == HAWQ_EPI_RESIDUAL);
    char *res_tile = smem + p.ring_bytes;
    char *ctab_lds = res_tile + (EPI == HAWQ_EPI_RESIDUAL ? C::BM * C::BN * 2 : 0);  // [BN][16 B] (+ second branch)
    if constexpr (FAST) {
        // the per-channel requant constants of this tile go to LDS asynchronously, off the epilogue's critical path
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        if (wave < C::BN / 64)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(p.ctab + (size_t)(c0 + wave * 64 + lane) * 4),
                                             (__attribute__((address_space(3))) void *)(ctab_lds + wave * 1024), 16, 0, 0);
        if constexpr (DUAL) {
            if (wave >= C::NW / 2 && wave - C::NW / 2 < C::BN / 64)
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void *)(p.ctab_id + (size_t)(c0 + (wave - C::NW / 2) * 64 + lane) * 4),
                    (__attribute__((address_space(3))) void *)(ctab_lds + C::BN * 16 + (wave - C::NW / 2) * 1024), 16, 0, 0);
        }
    }
    if constexpr (FAST && EPI == HAWQ_EPI_RESIDUAL && !DUAL) prefetch_residual<C>(p, m0, c0, res_tile);

    v16i acc[C::CT][C::PT];
#pragma unroll
    for (int c = 0; c < C::CT; ++c)
#pragma unroll
        for (int q = 0; q < C::PT; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][q][r] = 0;
    v16i acc2[DUAL ? C::CT : 1][DUAL ? C::PT : 1];
    if constexpr (DUAL) {
#pragma unroll
        for (int c = 0; c < C::CT; ++c)
#pragma unroll
            for (int q = 0; q < C::PT; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc2[c][q][r] = 0;
    }
    const long long t_begin = prof ? (long long)__builtin_readcyclecounter() : 0;
    constexpr bool ASYNC8 = BITS == 0x88 && (!DUAL || BITS2 == 0x88);
    constexpr bool ASYNC4 = BITS == 0x44 && (!DUAL || BITS2 == 0x44);
    if constexpr (ASYNC8) {
        gemm_pipeline<C, DUAL, false>(acc, acc2, p, m0, c0, smem);
    } else if (ASYNC4 && (p.Cin & 127) == 0 && (!DUAL || (p.Cin2 & 127) == 0) &&
               ((p.KH * p.KW * (p.Cin >> 7)) % C::KSUB) == 0 && (!DUAL || ((p.Cin2 >> 7) % C::KSUB) == 0)) {
        if constexpr (ASYNC4) gemm_pipeline<C, DUAL, true>(acc, acc2, p, m0, c0, smem);
    } else {
        run_segment<C, BITS>(acc, p.in, p.wgt, p.in_bits, p.w_bits, p.H, p.W, p.Cin, p.KH, p.KW, p.stride, p.pad,
                             p.Ho, p.Wo, p.M, p.Cout, m0, c0, smem, p.in_pitch);
        if constexpr (DUAL)
            run_segment<C, BITS2>(acc2, p.in2, p.wgt2, p.in2_bits, p.w2_bits, p.H2, p.W2, p.Cin2, 1, 1, p.stride2,
                                  0, p.Ho, p.Wo, p.M, p.Cout, m0, c0, smem, p.Cin2 * p.in2_bits / 8);
    }
    if (HAWQ_DBG_BIT(p.dbg, 4)) return;
    const long long t_loop_end = prof ? (long long)__builtin_readcyclecounter() : 0;
    const int kgrp = (threadIdx.x >> 6) / C::NWG;
    if constexpr (C::KG > 1) {
        // split-K: groups 1 .. KG-1 hand their partial accumulators to group 0 through the (now free) ring, one group per
        // round; [wave][tile][register][lane] dwords: conflict-free, every lane finds its own registers
        int *dump = reinterpret_cast<int *>(smem);
        const int slot0 = (((threadIdx.x >> 6) % C::NWG) * (C::CT * C::PT)) * 16 * 64 + (threadIdx.x & 63);
        for (int g = 1; g < C::KG; ++g) {
            if (kgrp == g) {
#pragma unroll
                for (int c = 0; c < C::CT; ++c)
#pragma unroll
                    for (int q = 0; q < C::PT; ++q)
#pragma unroll
                        for (int r = 0; r < 16; ++r) dump[slot0 + ((c * C::PT + q) * 16 + r) * 64] = acc[c][q][r];
            }
            __syncthreads();
            if (kgrp == 0) {
#pragma unroll
                for (int c = 0; c < C::CT; ++c)
#pragma unroll
                    for (int q = 0; q < C::PT; ++q)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[c][q][r] += dump[slot0 + ((c * C::PT + q) * 16 + r) * 64];
            }
            __syncthreads();
            if constexpr (DUAL) {
                if (kgrp == g) {
#pragma unroll
                    for (int c = 0; c < C::CT; ++c)
#pragma unroll
                        for (int q = 0; q < C::PT; ++q)
#pragma unroll
                            for (int r = 0; r < 16; ++r) dump[slot0 + ((c * C::PT + q) * 16 + r) * 64] = acc2[DUAL ? c : 0][DUAL ? q : 0][r];
                }
                __syncthreads();
                if (kgrp == 0) {
#pragma unroll
                    for (int c = 0; c < C::CT; ++c)
#pragma unroll
                        for (int q = 0; q < C::PT; ++q)
#pragma unroll
                            for (int r = 0; r < 16; ++r) acc2[DUAL ? c : 0][DUAL ? q : 0][r] += dump[slot0 + ((c * C::PT + q) * 16 + r) * 64];
                }
                __syncthreads();
            }
        }
    }
    if constexpr (FAST) {
        epilogue_fast<C, EPI, DUAL, TIE ? 2 : 0>(p, acc, acc2, m0, c0, smem, res_tile, ctab_lds, kgrp == 0);
    } else {
        if (C::KG > 1 && kgrp != 0) return;   // the direct epilogue has no barriers: the other groups are done
        epilogue_generic<C, EPI, DUAL>(p, acc, acc2, m0, c0);
    }
    if (prof && blockIdx.x == 8 && threadIdx.x == 0) {
        p.dbgbuf[0] = t_begin - t_entry, p.dbgbuf[1] = t_loop_end - t_begin;
        p.dbgbuf[2] = (long long)__builtin_readcyclecounter() - t_loop_end, p.dbgbuf[3] = 0;
    }
}

}  // namespace
