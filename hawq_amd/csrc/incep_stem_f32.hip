// InceptionV3's input QuantAct + Conv2d_1a_3x3 from fp32 NCHW images in ONE launch (hawq_incep_stem_f32).
//
// Reference path: Q_InceptInitBlock (q_inceptionv3.py of the reference): the input QuantAct (quant_modules.py:271-274,
// quant_utils.py:73-97), then q_conv1 = 3x3 / stride 2 / pad 0, 3 -> 32 channels, with ReLU and its q_activ.  The default fp32 plan
// runs that as three launches (hawq_fakequant_f32, hawq_f32_nchw_to_q_nhwc with the 3 channels padded to 16, hawq_incep_conv at
// K = 9 x 16); this kernel writes the same bytes.  It is the fp32 twin of incep_stem_u8_kernel (incep_stem.hip): same K order
// k = (kh * 3 + kw) * 3 + c, same [Cout][32] weight rows, same lane map (weights give the MFMA rows in cperm order, lane l31 = one
// output pixel, lane half h supplies K bytes 16 h .. 16 h + 15 and ends up owning channels 16 h .. 16 h + 15), same epilogue.
//
// What differs is where the K bytes come from.  Three fp32 planes gathered per output pixel would read, and quantise, every input
// value 2.25 times, so a workgroup owns a strip of one image - STEM_R output rows x up to STEM_CW output columns - and
//   1. loads the strip's 2 R + 1 input rows of the three planes with coalesced dword loads (lane = column; rows of 299 floats are not
//      16-byte aligned, so nothing wider), quantises each value once, q = clamp(rint(inv_scale * x), in_lo, in_hi), and stores the
//      pixel's three int8 values as ONE dword (c0, c1, c2, 0) into an LDS tile [2 R + 1][STEM_ICW] (ds_write_b32, conflict-free);
//   2. after one barrier its four waves walk the strip's 32-pixel groups: a lane reads the 3 pixels (8-byte aligned: ds_read_b64 +
//      ds_read_b32) of two window rows, squeezes each row's 3 x 4 bytes to the 9 contiguous bytes of the NHWC uint8 layout with
//      shifts, and assembles its 16 K bytes: h = 0, row 0 bytes 0..8 + row 1 bytes 0..6; h = 1, row 1 bytes 7..8 + row 2 bytes
//      0..8 + five zeros (k = 27 .. 31, whose weights are zero too).  One v_mfma_i32_32x32x32_i8 per group.
// The weight fragment and the lane half's 16 (bias, m, ek) stay in registers over the groups.  Rows and columns past the image are
// loaded from clamped addresses (no branch around a load), groups past the strip's pixels compute pixel npix - 1 again and store
// nothing, so every lane reaches the MFMA.
#include <math.h>

#include "common.h"

namespace {

constexpr int STEM_R = 4;                     // output rows per workgroup
constexpr int STEM_ROWS = 2 * STEM_R + 1;     // input rows of the tile
constexpr int STEM_ICW = 320;                 // input columns of the tile: five 64-lane loads per row
constexpr int STEM_CW = (STEM_ICW - 1) / 2;   // output columns per workgroup (2 CW + 1 <= ICW)
constexpr int STEM_UNR = 4;                   // row pieces a wave has in flight (3 loads each)

__global__ __launch_bounds__(256) void incep_stem_f32_kernel(const float *__restrict__ x, float inv_scale, float in_lo, float in_hi,
                                                            hawq_incep_conv_args a, int Ho, int Wo, int nstrips, int nchunks) {
    __shared__ __attribute__((aligned(16))) int tile[STEM_ROWS * STEM_ICW];   // (c0, c1, c2, 0) per input pixel
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int cbase = blockIdx.y * 32;
    int b = blockIdx.x;
    const int chunk = b % nchunks;
    b /= nchunks;
    const int strip = b % nstrips, n = b / nstrips;
    const int oy0 = strip * STEM_R, ox0 = chunk * STEM_CW;
    const int rows_out = min(STEM_R, Ho - oy0), cw = min(STEM_CW, Wo - ox0);

    // weight fragment and the lane half's tables (every lane of a half reads the same addresses)
    const int co_row = cbase + cperm(l31);
    const v4i zero = {0, 0, 0, 0};
    const v4i wf = co_row < a.Cout ? *reinterpret_cast<const v4i *>((const int8_t *)a.wgt + (size_t)co_row * 32 + 16 * h) : zero;
    const int c16 = cbase + 16 * h;
    const bool cv = c16 < a.Cout;   // Cout % 16 == 0: the 16 channels of a lane half are all valid or all not
    int tb[16], tm[16], te[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        tb[r] = cv ? a.bias[c16 + r] : 0;
        tm[r] = cv ? a.m[c16 + r] : 0;
        te[r] = cv ? a.ek[c16 + r] : 33;
    }

    // ---- 1. input rows -> quantised LDS tile
    {
        const int iy0 = 2 * oy0, ix0 = 2 * ox0;
        const int nblk = (2 * cw + 1 + 63) >> 6;               // 64-column pieces per row, <= 5
        const int npieces = (2 * rows_out + 1) * nblk;         // <= 45
        const size_t plane = (size_t)a.H * a.W;
        const float *img = x + (size_t)n * 3 * plane;
        for (int u0 = wave; u0 < npieces; u0 += 4 * STEM_UNR) {
            float v[STEM_UNR][3];
            int dst[STEM_UNR];
#pragma unroll
            for (int j = 0; j < STEM_UNR; ++j) {   // a piece past the last one repeats it: same values to the same place
                const int u = min(u0 + 4 * j, npieces - 1);
                const int r = u / nblk, col = (u - r * nblk) * 64 + lane;
                const size_t src = (size_t)min(iy0 + r, a.H - 1) * a.W + min(ix0 + col, a.W - 1);
                dst[j] = r * STEM_ICW + col;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[j][c] = img[c * plane + src];
            }
#pragma unroll
            for (int j = 0; j < STEM_UNR; ++j) {
                int q[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) q[c] = (int)fminf(fmaxf(rintf(__fmul_rn(inv_scale, v[j][c])), in_lo), in_hi);
                tile[dst[j]] = (int)pack4_i8(q[0], q[1], q[2], 0);
            }
        }
    }
    __syncthreads();

    // ---- 2. 32-pixel groups of the strip
    const int npix = rows_out * cw, ngroups = (npix + 31) >> 5;
    for (int g = wave; g < ngroups; g += 4) {   // wave-uniform: every lane reaches the MFMA
        const int qi = g * 32 + l31;
        const bool pv = qi < npix;
        const int qc = pv ? qi : npix - 1;
        const int r = qc / cw, xx = qc - r * cw;
        // window rows: A = row 0 (h = 0) or row 2 (h = 1), B = row 1
        const int offA = (2 * r + 2 * h) * STEM_ICW + 2 * xx, offB = (2 * r + 1) * STEM_ICW + 2 * xx;
        const v2i A01 = *reinterpret_cast<const v2i *>(tile + offA), B01 = *reinterpret_cast<const v2i *>(tile + offB);
        const unsigned A0 = (unsigned)A01.x, A1 = (unsigned)A01.y, A2 = (unsigned)tile[offA + 2];
        const unsigned B0 = (unsigned)B01.x, B1 = (unsigned)B01.y, B2 = (unsigned)tile[offB + 2];
        // 3 x (c0, c1, c2, 0) -> 9 contiguous bytes in ca0, ca1, ca2 (byte 3 of every tile dword is zero)
        const unsigned ca0 = A0 | (A1 << 24), ca1 = (A1 >> 8) | (A2 << 16), ca2 = A2 >> 16;
        const unsigned cb0 = B0 | (B1 << 24), cb1 = (B1 >> 8) | (B2 << 16), cb2 = B2 >> 16;
        v4i af;
        af[0] = (int)(h ? (cb1 >> 24) | (cb2 << 8) | (ca0 << 16) : ca0);
        af[1] = (int)(h ? (ca0 >> 16) | (ca1 << 16) : ca1);
        af[2] = (int)(h ? (ca1 >> 16) | (ca2 << 16) : ca2 | (cb0 << 8));
        af[3] = (int)(h ? 0u : (cb0 >> 24) | (cb1 << 8));
        v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf, af, acc, 0, 0, 0);
        // acc[r] = output channel c16 + r of the pixel (common.h: cperm); hawq_incep_conv's REQUANT epilogue
        if (pv && cv) {
            int o[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                int v = acc[k] + tb[k], ek = te[k];
                asm volatile("" : "+v"(ek));   // only (bias, m, ek) stay resident: what dyadic_rne derives from ek is cheaper than its registers
                if (a.relu) v = max(v, 0);
                o[k] = clampi(dyadic_rne(v, tm[k], ek), a.q_lo, a.q_hi);
            }
            v4i ov;
#pragma unroll
            for (int j = 0; j < 4; ++j) ov[j] = (int)pack4_i8(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
            const size_t p = ((size_t)n * Ho + oy0 + r) * Wo + ox0 + xx;
            *reinterpret_cast<v4i *>((int8_t *)a.out + p * a.ldo + a.c_off + c16) = ov;
        }
    }
}

const char *stem_f32_refusal(const float *x, float inv_scale, int32_t in_lo, int32_t in_hi, const hawq_incep_conv_args *c) {
    if (!c) return "null conv description";
    if (!x) return "null image pointer";
    if (!(inv_scale > 0.f) || !isfinite(inv_scale)) return "inv_scale must be finite and positive";
    if (in_lo < -128 || in_hi > 127 || in_lo > in_hi) return "input clamp bounds outside int8";
    if (c->in) return "`in` must be NULL (the kernel reads the fp32 images)";
    if (!c->wgt || !c->bias || !c->out) return "null weight, bias or output pointer";
    if (!c->m || !c->ek) return "requant tables missing";
    if (c->N <= 0 || c->H < 3 || c->W < 3) return "images must be at least 3 x 3";
    if (c->Cin != 3 || c->KH != 3 || c->KW != 3 || c->stride != 2 || c->pad_h != 0 || c->pad_w != 0)
        return "conv must be 3 channels in, 3x3 / stride 2 / pad 0";
    if (c->Cout <= 0 || c->Cout % 16 != 0) return "Cout must be a positive multiple of 16";
    if (c->epilogue != HAWQ_INCEP_REQUANT || c->out_bits != 8) return "only the REQUANT epilogue with an int8 store";
    if (c->q_lo < -128 || c->q_hi > 127 || c->q_lo > c->q_hi) return "clamp bounds outside the int8 store";
    if (c->c_off < 0 || c->c_off % 16 != 0 || c->ldo % 16 != 0 || c->ldo < c->c_off + c->Cout)
        return "ldo and c_off must be multiples of 16 with ldo >= c_off + Cout";
    if ((reinterpret_cast<size_t>(c->out) & 15) || (reinterpret_cast<size_t>(c->wgt) & 15) || (reinterpret_cast<size_t>(x) & 3))
        return "out and wgt must be 16-byte aligned, x 4-byte aligned";
    const long long P = (long long)c->N * ((c->H - 3) / 2 + 1) * ((c->W - 3) / 2 + 1);
    if (P > 0x7fffffffll - 64) return "too many output pixels";
    return nullptr;
}

}  // namespace

extern "C" int hawq_incep_stem_f32_ok(const float *x, float inv_scale, int32_t in_lo, int32_t in_hi, const hawq_incep_conv_args *conv) {
    return stem_f32_refusal(x, inv_scale, in_lo, in_hi, conv) == nullptr ? 1 : 0;
}

extern "C" int hawq_incep_stem_f32(const float *x, float inv_scale, int32_t in_lo, int32_t in_hi, const hawq_incep_conv_args *conv,
                                   void *stream) {
    const char *why = stem_f32_refusal(x, inv_scale, in_lo, in_hi, conv);
    HAWQ_REQUIRE(!why, "hawq_incep_stem_f32: %s", why);
    const int Ho = (conv->H - 3) / 2 + 1, Wo = (conv->W - 3) / 2 + 1;
    const int nstrips = (Ho + STEM_R - 1) / STEM_R, nchunks = (Wo + STEM_CW - 1) / STEM_CW;
    // one workgroup per (image, strip, column chunk): no more of them than output pixels, which the refusal bounds
    dim3 grid((unsigned)((long long)conv->N * nstrips * nchunks), (unsigned)((conv->Cout + 31) / 32));
    hipLaunchKernelGGL(incep_stem_f32_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, inv_scale, (float)in_lo, (float)in_hi, *conv,
                       Ho, Wo, nstrips, nchunks);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
