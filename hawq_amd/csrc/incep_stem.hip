// InceptionV3's input QuantAct + Conv2d_1a_3x3 from uint8 images in ONE launch (hawq_incep_stem_u8).
//
// Reference path: Q_InceptInitBlock (q_inceptionv3.py of the reference) on the tensor that torchvision's ToTensor + Normalize
// (quant_train.py:432-440) make of a decoded image: the input QuantAct (quant_modules.py:271-274), then q_conv1 = 3x3 / stride 2 /
// pad 0, 3 -> 32 channels, with ReLU and its q_activ.  The fp32 plan runs that as three launches (fake-quantise, NCHW -> NHWC int8
// with the 3 channels padded to 16, hawq_incep_conv at K = 9 x 16); here the ToTensor + Normalize + QuantAct step is a table look-up
// per byte, and K = 27 fits one v_mfma_i32_32x32x32_i8.
//
// Lane map as in incep_conv_kernel (inception.hip): the weight operand gives the rows (channels in cperm order, so lane half h ends up
// owning channels 16 h .. 16 h + 15 of the wave's 32), the activations the columns (lane l31 = one output pixel), and lane half h
// supplies K bytes 16 h .. 16 h + 15 with k = (kh * 3 + kw) * 3 + c = 9 kh + j.  For a pixel, window row kh is the 9 contiguous NHWC
// bytes x[n][2 oy + kh][2 ox][0 .. 8], so the K bytes of a lane half are: h = 0, row 0 bytes 0..8 + row 1 bytes 0..6; h = 1, row 1
// bytes 7..8 + row 2 bytes 0..8 + five zeros (k = 27 .. 31, whose weights are zero too).
// A workgroup stages the table (768 B) and its 32 channels' (bias, m, ek) in LDS once, a wave loads its weight fragment once, then
// walks 32-pixel groups; each lane half stores its 16 channels of one pixel as one 16-byte store.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void incep_stem_u8_kernel(const uint8_t *__restrict__ x, const int8_t *__restrict__ lut,
                                                           hawq_incep_conv_args a, int Ho, int Wo, int P) {
    __shared__ int lut_s[192];   // int8 [3][256]
    __shared__ int tab_s[3][32];  // bias, m, ek of the workgroup's 32 channels
    const int t = threadIdx.x;
    const int cbase = blockIdx.y * 32;
    if (t < 192) lut_s[t] = reinterpret_cast<const int *>(lut)[t];
    if (t >= 192 && t < 224) {
        const int co = cbase + t - 192;
        const bool ok = co < a.Cout;
        tab_s[0][t - 192] = ok ? a.bias[co] : 0;
        tab_s[1][t - 192] = ok ? a.m[co] : 0;
        tab_s[2][t - 192] = ok ? a.ek[co] : 33;
    }
    __syncthreads();
    const int8_t *lt = reinterpret_cast<const int8_t *>(lut_s);
    const int lane = t & 63, wave = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int co_row = cbase + cperm(l31);
    const v4i zero = {0, 0, 0, 0};
    const v4i wf = co_row < a.Cout ? *reinterpret_cast<const v4i *>((const int8_t *)a.wgt + (size_t)co_row * 32 + 16 * h) : zero;
    const int c16 = cbase + 16 * h;
    const bool cv = c16 < a.Cout;   // Cout % 16 == 0: the 16 channels of a lane half are all valid or all not
    const size_t rs = (size_t)a.W * 3;   // bytes per image row
    const int ngroups = (P + 31) >> 5;
    // the group index is wave-uniform: every lane reaches the MFMA (pixels past P read pixel P - 1 and store nothing)
    for (int g = blockIdx.x * 4 + wave; g < ngroups; g += gridDim.x * 4) {
        const int p = g * 32 + l31;
        const bool pv = p < P;
        const int pc = pv ? p : P - 1;
        const int ox = pc % Wo, nr = pc / Wo, oy = nr % Ho, n = nr / Ho;
        const uint8_t *org = x + (((size_t)n * a.H + 2 * oy) * a.W + 2 * ox) * 3;
        int u[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {   // issue every load before the first look-up
            const int k0 = i, k1 = 16 + i < 27 ? 16 + i : 0;
            const size_t off = h ? (size_t)(k1 / 9) * rs + k1 % 9 : (size_t)(k0 / 9) * rs + k0 % 9;
            u[i] = org[off];
        }
        int q[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = h ? (16 + i) % 3 : i % 3;
            const int v = lt[c * 256 + u[i]];
            q[i] = (h && 16 + i >= 27) ? 0 : v;
        }
        v4i af;
#pragma unroll
        for (int j = 0; j < 4; ++j) af[j] = (int)pack4_i8(q[4 * j], q[4 * j + 1], q[4 * j + 2], q[4 * j + 3]);
        v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf, af, acc, 0, 0, 0);
        // acc[r] = output channel c16 + r of pixel p (common.h: cperm); hawq_incep_conv's REQUANT epilogue
        if (pv && cv) {
            int o[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int v = acc[r] + tab_s[0][16 * h + r];
                if (a.relu) v = max(v, 0);
                o[r] = clampi(dyadic_rne(v, tab_s[1][16 * h + r], tab_s[2][16 * h + r]), a.q_lo, a.q_hi);
            }
            v4i ov;
#pragma unroll
            for (int j = 0; j < 4; ++j) ov[j] = (int)pack4_i8(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
            *reinterpret_cast<v4i *>((int8_t *)a.out + (size_t)p * a.ldo + a.c_off + c16) = ov;
        }
    }
}

const char *stem_u8_refusal(const uint8_t *x, const int8_t *lut, const hawq_incep_conv_args *c) {
    if (!c) return "null conv description";
    if (!x) return "null image pointer";
    if (!lut) return "uint8 images need the look-up table";
    if (c->in) return "`in` must be NULL (the kernel reads the uint8 images)";
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
    if ((reinterpret_cast<size_t>(c->out) & 15) || (reinterpret_cast<size_t>(c->wgt) & 15) || (reinterpret_cast<size_t>(lut) & 3))
        return "out and wgt must be 16-byte aligned, lut 4-byte aligned";
    const long long P = (long long)c->N * ((c->H - 3) / 2 + 1) * ((c->W - 3) / 2 + 1);
    if (P > 0x7fffffffll - 64) return "too many output pixels";
    return nullptr;
}

}  // namespace

extern "C" int hawq_incep_stem_u8_ok(const uint8_t *x, const int8_t *lut, const hawq_incep_conv_args *conv) {
    return stem_u8_refusal(x, lut, conv) == nullptr ? 1 : 0;
}

extern "C" int hawq_incep_stem_u8(const uint8_t *x, const int8_t *lut, const hawq_incep_conv_args *conv, void *stream) {
    const char *why = stem_u8_refusal(x, lut, conv);
    HAWQ_REQUIRE(!why, "hawq_incep_stem_u8: %s", why);
    const int Ho = (conv->H - 3) / 2 + 1, Wo = (conv->W - 3) / 2 + 1;
    const int P = conv->N * Ho * Wo;
    // four 32-pixel groups per workgroup and round; at most 2048 workgroups per channel block (8 per CU), each wave then walks on
    const int groups = (P + 31) / 32, wgs = (groups + 3) / 4;
    dim3 grid((unsigned)(wgs < 2048 ? wgs : 2048), (unsigned)((conv->Cout + 31) / 32));
    hipLaunchKernelGGL(incep_stem_u8_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, lut, *conv, Ho, Wo, P);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
