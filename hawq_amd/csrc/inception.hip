// InceptionV3 kernels (utils/models/q_inceptionv3.py of the reference):
//   hawq_incep_conv       rectangular implicit-GEMM conv (1x1 .. 7x7, 1x7 / 7x1 / 1x3 / 3x1, own pad_h / pad_w, stride 1 / 2)
//                         with the RAW / REQUANT / REQUANT2 epilogues and a channel-offset store into a concat buffer
//   hawq_avgpool3x3_f32   QuantAveragePool2d(3, 1, padding=1) of the average-pool branches (quant_modules.py:557-602)
// The ResNet kernels assume square windows with one padding value and channels padded to 64; InceptionV3 has 1x7 / 7x1 windows,
// 80 / 48 / 320 / 448 channels and odd maps (149, 147, 73, 71, 35, 17, 8), so these are kernels of their own with plain global
// operand loads: every channel count of the network is a multiple of 16, which is all the loads below need.
#include "common.h"

namespace {

// One workgroup = 4 waves = 64 output pixels x 64 output channels; wave w owns pixels 32 (w & 1) .. +31 and channels
// 32 (w >> 1) .. +31 of that tile.  MFMA v_mfma_i32_32x32x32_i8: the weight operand gives the rows (channels, read in cperm
// order so that lane half h owns channels 16 h .. 16 h + 15 of the wave's 32), the activations give the columns (lane l31 = one
// pixel).  K walks the window taps and, per tap, Cin in steps of 32 (16 bytes per lane half); a half step beyond Cin
// (Cin % 32 == 16) and every tap that falls into the padding contribute zeros.
__global__ __launch_bounds__(256) void incep_conv_kernel(hawq_incep_conv_args a, int Ho, int Wo) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    const long long P = (long long)a.N * Ho * Wo;
    const long long pbase = (long long)blockIdx.x * 64 + 32 * (wave & 1);
    const int cbase = blockIdx.y * 64 + 32 * (wave >> 1);
    if (pbase >= P || cbase >= a.Cout) return;   // no barrier below: a wave with nothing to store leaves at once
    const long long p = pbase + l31;
    const bool pv = p < P;
    int n = 0, oy = 0, ox = 0;
    if (pv) {
        ox = (int)(p % Wo);
        oy = (int)((p / Wo) % Ho);
        n = (int)(p / ((long long)Wo * Ho));
    }
    const int co_row = cbase + cperm(l31);
    const bool wv = co_row < a.Cout;
    const int8_t *in = (const int8_t *)a.in;
    const int8_t *wgt = (const int8_t *)a.wgt + (size_t)(wv ? co_row : 0) * a.KH * a.KW * a.Cin;
    v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const v4i zero = {0, 0, 0, 0};
    for (int kh = 0; kh < a.KH; ++kh) {
        const int iy = oy * a.stride - a.pad_h + kh;
        for (int kw = 0; kw < a.KW; ++kw) {
            const int ix = ox * a.stride - a.pad_w + kw;
            const bool inb = pv && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const int8_t *ip = in + (((size_t)n * a.H + (inb ? iy : 0)) * a.W + (inb ? ix : 0)) * a.Cin;
            const int8_t *wp = wgt + (size_t)(kh * a.KW + kw) * a.Cin;
            for (int c0 = 0; c0 < a.Cin; c0 += 32) {
                const int c = c0 + 16 * h;
                const bool cv = c < a.Cin;
                const v4i af = (inb && cv) ? *reinterpret_cast<const v4i *>(ip + c) : zero;
                const v4i wf = (wv && cv) ? *reinterpret_cast<const v4i *>(wp + c) : zero;
                acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf, af, acc, 0, 0, 0);
            }
        }
    }
    // acc[r] = output channel cbase + 16 h + r of pixel p (common.h: cperm)
    const int c16 = cbase + 16 * h;
    if (!pv || c16 >= a.Cout) return;   // Cout % 16 == 0: the 16 channels of a lane half are all valid or all not
    const size_t row = (size_t)p * a.ldo + a.c_off + c16;
    if (a.epilogue == HAWQ_INCEP_RAW) {
        int32_t *o = (int32_t *)a.out + row;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = acc[r] + a.bias[c16 + r];
        return;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = c16 + r;
        int v = acc[r] + a.bias[co];
        if (a.relu) v = max(v, 0);
        int q = clampi(dyadic_rne(v, a.m[co], a.ek[co]), a.q_lo, a.q_hi);
        if (a.epilogue == HAWQ_INCEP_REQUANT2) q = clampi(dyadic_rne(q, a.m2, a.ek2), a.q2_lo, a.q2_hi);
        if (a.out_bits == 16)
            ((int16_t *)a.out)[row + r] = (int16_t)q;
        else
            ((int8_t *)a.out)[row + r] = (int8_t)q;
    }
}

__global__ __launch_bounds__(256) void avgpool3x3_f32_kernel(const float *__restrict__ x, float *__restrict__ y, long long total,
                                                            int H, int W, float scale) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ox = (int)(i % W), oy = (int)((i / W) % H);
        const float *plane = x + (i / ((long long)W * H)) * (long long)H * W;
        long long s = 0;
        for (int dy = -1; dy <= 1; ++dy) {
            const int iy = oy + dy;
            if (iy < 0 || iy >= H) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const int ix = ox + dx;
                if (ix < 0 || ix >= W) continue;
                s += (long long)rintf(__fdiv_rn(plane[(long long)iy * W + ix], scale));
            }
        }
        // trunc(s / 9 + 0.01) (quant_utils.py:324-337) as an exact rational: C division truncates toward zero, like trunc, for
        // negative sums too; equal to the reference's float32 evaluation for every sum of nine 16-bit values (tests/test_inception_host.py)
        const long long p = (100 * s + 9) / 900;
        y[i] = __fmul_rn((float)p, scale);
    }
}

enum { POOL_NONE = 0, POOL_MAX3S2 = 1, POOL_AVG3 = 2, POOL_GLOBAL = 3 };

__device__ __forceinline__ int pool_load(const hawq_incep_pool_args &a, long long pix, int c) {
    const long long i = pix * a.in_pitch + a.in_off + c;
    int v = a.in_bits == 16 ? (int)((const int16_t *)a.in)[i] : (int)((const int8_t *)a.in)[i];
    if (a.pre) v = clampi(dyadic_rne(v, a.m1, a.ek1), a.lo1, a.hi1);
    return v;
}

// one thread per output element (channel fastest: neighbouring threads read neighbouring bytes of a row)
template <int OP>
__global__ __launch_bounds__(256) void incep_pool_kernel(hawq_incep_pool_args a, int Ho, int Wo) {
    const long long total = (long long)a.N * Ho * Wo * a.C;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % a.C);
        const long long op = i / a.C;
        const int ox = (int)(op % Wo), oy = (int)((op / Wo) % Ho), n = (int)(op / ((long long)Wo * Ho));
        const long long img = (long long)n * a.H * a.W;
        int v;
        if (OP == POOL_NONE) {
            v = pool_load(a, op, c);
        } else if (OP == POOL_MAX3S2) {
            v = -2147483647 - 1;
            for (int dy = 0; dy < 3; ++dy)
                for (int dx = 0; dx < 3; ++dx) v = max(v, pool_load(a, img + (long long)(2 * oy + dy) * a.W + 2 * ox + dx, c));
        } else if (OP == POOL_AVG3) {
            long long s = 0;
            for (int dy = -1; dy <= 1; ++dy) {
                const int iy = oy + dy;
                if (iy < 0 || iy >= a.H) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    const int ix = ox + dx;
                    if (ix >= 0 && ix < a.W) s += pool_load(a, img + (long long)iy * a.W + ix, c);
                }
            }
            v = (int)((100 * s + 9) / 900);
        } else {
            const long long hw = (long long)a.H * a.W;
            long long s = 0;
            for (long long k = 0; k < hw; ++k) s += pool_load(a, img + k, c);
            v = (int)((100 * s + hw) / (100 * hw));
        }
        if (a.post) v = clampi(dyadic_rne(v, a.m2, a.ek2), a.lo2, a.hi2);
        const long long o = op * a.ldo + a.c_off + c;
        if (a.out_bits == 16)
            ((int16_t *)a.out)[o] = (int16_t)v;
        else
            ((int8_t *)a.out)[o] = (int8_t)v;
    }
}

inline int grid_for(long long work_items) {
    long long g = (work_items + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace

extern "C" int hawq_incep_conv(const hawq_incep_conv_args *a, void *stream) {
    HAWQ_REQUIRE(a && a->in && a->wgt && a->bias && a->out, "hawq_incep_conv: null pointer");
    HAWQ_REQUIRE(a->N > 0 && a->H > 0 && a->W > 0 && a->Cin > 0 && a->Cout > 0 && a->Cin % 16 == 0 && a->Cout % 16 == 0,
                 "hawq_incep_conv: bad shape (N=%d H=%d W=%d Cin=%d Cout=%d; channels must be multiples of 16)", a->N, a->H,
                 a->W, a->Cin, a->Cout);
    HAWQ_REQUIRE(a->KH >= 1 && a->KH <= 7 && a->KW >= 1 && a->KW <= 7 && (a->stride == 1 || a->stride == 2),
                 "hawq_incep_conv: window %dx%d / stride %d not supported", a->KH, a->KW, a->stride);
    HAWQ_REQUIRE(a->pad_h >= 0 && a->pad_w >= 0 && 2 * a->pad_h < a->KH + 1 && 2 * a->pad_w < a->KW + 1,
                 "hawq_incep_conv: padding (%d, %d) too large for a %dx%d window", a->pad_h, a->pad_w, a->KH, a->KW);
    const int Ho = (a->H + 2 * a->pad_h - a->KH) / a->stride + 1, Wo = (a->W + 2 * a->pad_w - a->KW) / a->stride + 1;
    HAWQ_REQUIRE(Ho > 0 && Wo > 0, "hawq_incep_conv: empty output");
    HAWQ_REQUIRE(a->c_off >= 0 && a->ldo >= a->c_off + a->Cout, "hawq_incep_conv: ldo %d < c_off %d + Cout %d", a->ldo, a->c_off,
                 a->Cout);
    HAWQ_REQUIRE(a->epilogue == HAWQ_INCEP_RAW || a->epilogue == HAWQ_INCEP_REQUANT || a->epilogue == HAWQ_INCEP_REQUANT2,
                 "hawq_incep_conv: unknown epilogue %d", a->epilogue);
    if (a->epilogue != HAWQ_INCEP_RAW) {
        HAWQ_REQUIRE(a->m && a->ek, "hawq_incep_conv: requant tables missing");
        HAWQ_REQUIRE(a->out_bits == 8 || a->out_bits == 16, "hawq_incep_conv: out_bits must be 8 or 16");
        const int lim = a->out_bits == 16 ? 32767 : 127;
        HAWQ_REQUIRE(a->q_lo >= -lim - 1 && a->q_hi <= lim && a->q_lo <= a->q_hi &&
                         (a->epilogue != HAWQ_INCEP_REQUANT2 || (a->q2_lo >= -lim - 1 && a->q2_hi <= lim && a->q2_lo <= a->q2_hi)),
                     "hawq_incep_conv: clamp bounds outside the %d-bit store", a->out_bits);
    }
    const long long P = (long long)a->N * Ho * Wo;
    HAWQ_REQUIRE((P + 63) / 64 < (1ll << 31), "hawq_incep_conv: too many output pixels");
    dim3 grid((unsigned)((P + 63) / 64), (unsigned)((a->Cout + 63) / 64));
    hipLaunchKernelGGL(incep_conv_kernel, grid, dim3(256), 0, (hipStream_t)stream, *a, Ho, Wo);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int hawq_avgpool3x3_f32(const float *x, float *y, int32_t NC, int32_t H, int32_t W, float scale, void *stream) {
    HAWQ_REQUIRE(x && y && NC > 0 && H > 0 && W > 0, "hawq_avgpool3x3_f32: bad arguments");
    const long long total = (long long)NC * H * W;
    hipLaunchKernelGGL(avgpool3x3_f32_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, y, total, H, W, scale);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}

namespace {
template <int OP>
int incep_pool_launch(const hawq_incep_pool_args *a, void *stream, const char *who) {
    HAWQ_REQUIRE(a && a->in && a->out, "%s: null pointer", who);
    HAWQ_REQUIRE(a->N > 0 && a->H > 0 && a->W > 0 && a->C > 0 && (a->in_bits == 8 || a->in_bits == 16) &&
                     (a->out_bits == 8 || a->out_bits == 16),
                 "%s: bad shape or widths", who);
    HAWQ_REQUIRE(a->in_off >= 0 && a->in_pitch >= a->in_off + a->C && a->c_off >= 0 && a->ldo >= a->c_off + a->C,
                 "%s: channel slice outside its rows", who);
    const int lim = a->out_bits == 16 ? 32767 : 127;
    HAWQ_REQUIRE(!a->post || (a->lo2 >= -lim - 1 && a->hi2 <= lim && a->lo2 <= a->hi2), "%s: post clamp outside the store", who);
    HAWQ_REQUIRE(!a->pre || a->lo1 <= a->hi1, "%s: bad pre clamp", who);
    HAWQ_REQUIRE(a->post || a->out_bits >= a->in_bits, "%s: a narrowing store needs a post requant", who);
    int Ho = a->H, Wo = a->W;
    if (OP == POOL_MAX3S2) {
        HAWQ_REQUIRE(a->H >= 3 && a->W >= 3, "%s: map smaller than the window", who);
        Ho = (a->H - 3) / 2 + 1, Wo = (a->W - 3) / 2 + 1;
    } else if (OP == POOL_GLOBAL) {
        Ho = Wo = 1;
    }
    const long long total = (long long)a->N * Ho * Wo * a->C;
    hipLaunchKernelGGL(incep_pool_kernel<OP>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, *a, Ho, Wo);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
}  // namespace

extern "C" int hawq_incep_requant(const hawq_incep_pool_args *a, void *stream) {
    return incep_pool_launch<POOL_NONE>(a, stream, "hawq_incep_requant");
}
extern "C" int hawq_incep_maxpool3s2(const hawq_incep_pool_args *a, void *stream) {
    return incep_pool_launch<POOL_MAX3S2>(a, stream, "hawq_incep_maxpool3s2");
}
extern "C" int hawq_incep_avgpool_branch(const hawq_incep_pool_args *a, void *stream) {
    return incep_pool_launch<POOL_AVG3>(a, stream, "hawq_incep_avgpool_branch");
}
extern "C" int hawq_incep_global_avgpool(const hawq_incep_pool_args *a, void *stream) {
    return incep_pool_launch<POOL_GLOBAL>(a, stream, "hawq_incep_global_avgpool");
}
