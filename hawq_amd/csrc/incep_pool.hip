// Vectorised pool / requant kernels of the InceptionV3 plan: hawq_incep_pool_v issues, for one hawq_incep_pool_args block, the same
// bytes as the op's entry point of inception.hip (hawq_incep_requant / _maxpool3s2 / _avgpool_branch / _global_avgpool), which stay
// the default path and the comparison baseline.  What differs from incep_pool_kernel there:
//   * a lane owns 16 consecutive channels of a pixel and moves them with 16-byte global loads and stores (C, the row pitches and the
//     slice offsets are multiples of 16, so every such group is 16-byte aligned and all valid or all not);
//   * coordinates come from the block index plus one 32-bit division per lane, and the average rules divide in int32
//     ((100 s + 9) / 900 with |s| <= 9 * 2^15; the global pool's 100 s + HW is bounded by pool_v_refusal before anything is launched);
//   * MAX3S2 takes the max over the raw inputs and applies `pre` once: pre is monotone non-decreasing when m1 >= 0, k = 0 and
//     e1 >= in_bits (|x m1| / 2^e1 < 2^(in_bits - 1) 2^31 / 2^in_bits = 2^30: the (int32_t) of dyadic_rne cannot wrap; round-half-even
//     and the clamp are monotone), so max_i pre(x_i) == pre(max_i x_i) exactly;
//   * AVG3 stages the pre-requantised tile plus its one-pixel halo in LDS as int16 (zeros in the padding), so every input element is
//     requantised once per tile that sees it instead of once per window, and the nine taps of an output are LDS reads;
//   * GLOBAL splits the H x W pixels of an image over the lanes of a workgroup and reduces the partial sums through LDS.
// The requant itself is dyadic_rne + clampi of common.h, unchanged: these tables are per tensor and may hold exact ties.
#include "common.h"

namespace {

struct Rq {
    int on, m, ek, lo, hi;
};
__device__ __forceinline__ int rq(int v, const Rq &r) { return r.on ? clampi(dyadic_rne(v, r.m, r.ek), r.lo, r.hi) : v; }

// 16 consecutive channels starting at element `e` of an int8 / int16 buffer <-> 16 ints (16-byte accesses only)
template <int BITS>
__device__ __forceinline__ void load16(const void *base, long long e, int *v) {
    if (BITS == 16) {
        const v4i *p = reinterpret_cast<const v4i *>((const int16_t *)base + e);
        const v4i a = p[0], b = p[1];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = (int16_t)a[i], v[2 * i + 1] = a[i] >> 16;
            v[8 + 2 * i] = (int16_t)b[i], v[8 + 2 * i + 1] = b[i] >> 16;
        }
    } else {
        const v4i a = *reinterpret_cast<const v4i *>((const int8_t *)base + e);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[4 * i] = (int8_t)a[i], v[4 * i + 1] = (int8_t)(a[i] >> 8);
            v[4 * i + 2] = (int8_t)(a[i] >> 16), v[4 * i + 3] = a[i] >> 24;
        }
    }
}
__device__ __forceinline__ v4i pack8_i16(const int *v) {
    v4i r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (v[2 * i] & 0xffff) | (int)((unsigned)v[2 * i + 1] << 16);
    return r;
}
// the low BITS of every value, as the (int16_t) / (int8_t) stores of incep_pool_kernel keep them
template <int BITS>
__device__ __forceinline__ void store16(void *base, long long e, const int *v) {
    if (BITS == 16) {
        v4i *p = reinterpret_cast<v4i *>((int16_t *)base + e);
        p[0] = pack8_i16(v), p[1] = pack8_i16(v + 8);
    } else {
        v4i r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = (int)pack4_i8(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
        *reinterpret_cast<v4i *>((int8_t *)base + e) = r;
    }
}
__device__ __forceinline__ Rq rq_pre(const hawq_incep_pool_args &a) { return Rq{a.pre, a.m1, a.ek1, a.lo1, a.hi1}; }
__device__ __forceinline__ Rq rq_post(const hawq_incep_pool_args &a) { return Rq{a.post, a.m2, a.ek2, a.lo2, a.hi2}; }

// REQUANT: one lane per (pixel, 16-channel group), groups fastest
template <int IB, int OB>
__global__ __launch_bounds__(256) void pool_requant_v(hawq_incep_pool_args a, unsigned items) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= items) return;
    const unsigned cg = (unsigned)a.C >> 4, pix = i / cg, g = i - pix * cg;
    const Rq pre = rq_pre(a), post = rq_post(a);
    int v[16];
    load16<IB>(a.in, (long long)pix * a.in_pitch + a.in_off + 16 * g, v);
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = rq(rq(v[k], pre), post);
    store16<OB>(a.out, (long long)pix * a.ldo + a.c_off + 16 * g, v);
}

// MAX3S2: blockIdx.x = output row (n, oy); blockIdx.y, threadIdx.x = (ox, 16-channel group) of that row, groups fastest
template <int IB, int OB>
__global__ __launch_bounds__(256) void pool_max3s2_v(hawq_incep_pool_args a, int Ho, int Wo) {
    const unsigned cg = (unsigned)a.C >> 4, i = blockIdx.y * blockDim.x + threadIdx.x;
    if (i >= (unsigned)Wo * cg) return;
    const unsigned ox = i / cg, g = i - ox * cg;
    const unsigned n = blockIdx.x / (unsigned)Ho, oy = blockIdx.x - n * (unsigned)Ho;
    const long long p0 = ((long long)n * a.H + 2 * oy) * a.W + 2 * ox;
    const Rq pre = rq_pre(a), post = rq_post(a);
    int v[16], t[16];
    load16<IB>(a.in, p0 * a.in_pitch + a.in_off + 16 * g, v);
#pragma unroll
    for (int tap = 1; tap < 9; ++tap) {
        load16<IB>(a.in, (p0 + (long long)(tap / 3) * a.W + tap % 3) * a.in_pitch + a.in_off + 16 * g, t);
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = max(v[k], t[k]);
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = rq(rq(v[k], pre), post);   // pre after the max: monotone (pool_v_refusal)
    store16<OB>(a.out, (((long long)n * Ho + oy) * Wo + ox) * a.ldo + a.c_off + 16 * g, v);
}

// AVG3: blockIdx = (32-channel chunk, tile of TH x TW output pixels, image).  LDS: [(TH + 2) (TW + 2) pixels][cw channels] int16,
// cw = 32, or 16 in the last chunk when C % 32 == 16.
constexpr int AVG_CC = 32, AVG_LDS_BYTES = 32768;
template <int IB, int OB>
__global__ __launch_bounds__(256) void pool_avg3_v(hawq_incep_pool_args a, int TH, int TW, int ntx) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int c0 = blockIdx.x * AVG_CC, sh = (a.C - c0 >= AVG_CC) ? 1 : 0;   // 1 << sh 16-channel groups in this chunk
    const int ty0 = (int)(blockIdx.y / (unsigned)ntx) * TH, tx0 = (int)(blockIdx.y % (unsigned)ntx) * TW;
    const long long img = (long long)blockIdx.z * a.H * a.W;
    const int SW = TW + 2, cw2 = 32 << sh /* bytes per staged pixel */;
    const Rq pre = rq_pre(a), post = rq_post(a);
    const v4i zero = {0, 0, 0, 0};
    for (int j = threadIdx.x; j < ((TH + 2) * SW) << sh; j += 256) {
        const int g = j & sh, pix = j >> sh, ly = (int)((unsigned)pix / (unsigned)SW), lx = pix - ly * SW;
        const int iy = ty0 - 1 + ly, ix = tx0 - 1 + lx;
        v4i *dst = reinterpret_cast<v4i *>(lds + pix * cw2 + 32 * g);
        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
            int v[16];
            load16<IB>(a.in, (img + (long long)iy * a.W + ix) * a.in_pitch + a.in_off + c0 + 16 * g, v);
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = rq(v[k], pre);   // lo1, hi1 inside int16 (pool_v_refusal)
            dst[0] = pack8_i16(v), dst[1] = pack8_i16(v + 8);
        } else {
            dst[0] = zero, dst[1] = zero;
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < (TH * TW) << sh; j += 256) {
        const int g = j & sh, pix = j >> sh, ty = (int)((unsigned)pix / (unsigned)TW), tx = pix - ty * TW;
        const int oy = ty0 + ty, ox = tx0 + tx;
        if (oy >= a.H || ox >= a.W) continue;
        int s[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) s[k] = 0;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const v4i *src = reinterpret_cast<const v4i *>(lds + ((ty + tap / 3) * SW + tx + tap % 3) * cw2 + 32 * g);
            const v4i p = src[0], q = src[1];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                s[2 * k] += (int16_t)p[k], s[2 * k + 1] += p[k] >> 16;
                s[8 + 2 * k] += (int16_t)q[k], s[8 + 2 * k + 1] += q[k] >> 16;
            }
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) s[k] = rq((100 * s[k] + 9) / 900, post);
        store16<OB>(a.out, (img + (long long)oy * a.W + ox) * a.ldo + a.c_off + c0 + 16 * g, s);
    }
}

// GLOBAL: blockIdx = (64-channel chunk, image); lane = (16-channel group g of the chunk, pixel lane pl): 4 groups x 64 pixel lanes.
// Each lane sums the pixels pl, pl + 64, ..; thread c < 64 then adds the 64 partial sums of channel c and finishes it.
constexpr int GL_CC = 64, GL_PL = 64;
template <int IB, int OB>
__global__ __launch_bounds__(256) void pool_global_v(hawq_incep_pool_args a) {
    __shared__ int part[GL_PL][GL_CC];
    __shared__ int res[GL_CC];
    const int c0 = blockIdx.x * GL_CC, g = threadIdx.x & 3, pl = threadIdx.x >> 2, hw = a.H * a.W;
    const bool live = c0 + 16 * g < a.C;
    const long long img = (long long)blockIdx.y * hw;
    const Rq pre = rq_pre(a), post = rq_post(a);
    int s[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) s[k] = 0;
    if (live)
        for (int p = pl; p < hw; p += GL_PL) {
            int v[16];
            load16<IB>(a.in, (img + p) * a.in_pitch + a.in_off + c0 + 16 * g, v);
#pragma unroll
            for (int k = 0; k < 16; ++k) s[k] += rq(v[k], pre);
        }
#pragma unroll
    for (int k = 0; k < 4; ++k) *reinterpret_cast<v4i *>(&part[pl][16 * g + 4 * k]) = v4i{s[4 * k], s[4 * k + 1], s[4 * k + 2], s[4 * k + 3]};
    __syncthreads();
    if (threadIdx.x < GL_CC) {
        int t = 0;
        for (int p = 0; p < GL_PL; ++p) t += part[p][threadIdx.x];
        res[threadIdx.x] = rq((100 * t + hw) / (100 * hw), post);   // |100 t + hw| < 2^31 (pool_v_refusal)
    }
    __syncthreads();
    if (threadIdx.x < 4 && c0 + 16 * (int)threadIdx.x < a.C) {
        int v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = res[16 * threadIdx.x + k];
        store16<OB>(a.out, (long long)blockIdx.y * a.ldo + a.c_off + c0 + 16 * threadIdx.x, v);
    }
}

// AVG3's tile: whole rows of a narrow map (W <= 40), 32 columns otherwise; as many rows as 32 KiB of LDS hold, evened out over the
// map, and halved while the launch has fewer than 512 workgroups (small batches: more, shorter workgroups)
void avg3_tile(const hawq_incep_pool_args *a, int *TH, int *TW) {
    const int tw = a->W <= 40 ? a->W : 32;
    int th = AVG_LDS_BYTES / ((tw + 2) * AVG_CC * 2) - 2;
    if (th > a->H) th = a->H;
    const int nty = (a->H + th - 1) / th;
    th = (a->H + nty - 1) / nty;
    const long long per_row = (long long)a->N * ((a->C + AVG_CC - 1) / AVG_CC) * ((a->W + tw - 1) / tw);
    while (th > 4 && per_row * ((a->H + th - 1) / th) < 512) th = (th + 1) / 2;
    *TH = th, *TW = tw;
}

// why hawq_incep_pool_v does not take this launch (NULL: it does)
const char *pool_v_refusal(const hawq_incep_pool_args *a, int op) {
    if (!a || !a->in || !a->out) return "null pointer";
    if (op != HAWQ_INCEP_POOL_REQUANT && op != HAWQ_INCEP_POOL_MAX3S2 && op != HAWQ_INCEP_POOL_AVG3 && op != HAWQ_INCEP_POOL_GLOBAL)
        return "unknown op";
    if (a->N <= 0 || a->H <= 0 || a->W <= 0 || a->C <= 0 || (a->in_bits != 8 && a->in_bits != 16) ||
        (a->out_bits != 8 && a->out_bits != 16))
        return "bad shape or widths";
    if (a->in_off < 0 || a->in_pitch < (long long)a->in_off + a->C || a->c_off < 0 || a->ldo < (long long)a->c_off + a->C)
        return "channel slice outside its rows";
    if (a->C % 16 || a->in_pitch % 16 || a->in_off % 16 || a->ldo % 16 || a->c_off % 16)
        return "C, in_pitch, in_off, ldo and c_off must be multiples of 16";
    if (((uintptr_t)a->in | (uintptr_t)a->out) & 15) return "in and out must be 16-byte aligned";
    const int lim = a->out_bits == 16 ? 32767 : 127;
    if (a->post && (a->lo2 < -lim - 1 || a->hi2 > lim || a->lo2 > a->hi2)) return "post clamp outside the store";
    if (a->pre && a->lo1 > a->hi1) return "bad pre clamp";
    if (!a->post && a->out_bits < a->in_bits) return "a narrowing store needs a post requant";
    int Wo = a->W;
    if (op == HAWQ_INCEP_POOL_MAX3S2) {
        if (a->H < 3 || a->W < 3) return "map smaller than the window";
        Wo = (a->W - 3) / 2 + 1;
        if (a->pre && (a->m1 < 0 || (a->ek1 >> 8) != 0 || (a->ek1 & 0xff) < a->in_bits || (a->ek1 & 0xff) > 62))
            return "max pool: the pre requant is not provably monotone (needs m1 >= 0, k = 0, e1 >= in_bits)";
    }
    if (op == HAWQ_INCEP_POOL_AVG3 && a->pre && (a->lo1 < -32768 || a->hi1 > 32767))
        return "average pool: pre clamp outside int16";
    if (op == HAWQ_INCEP_POOL_GLOBAL) {
        long long b = 1ll << (a->in_bits - 1);   // bound of a summand
        if (a->pre) b = (a->hi1 > -(long long)a->lo1 ? (long long)a->hi1 : -(long long)a->lo1) + 1;
        const long long hw = (long long)a->H * a->W;
        if (hw >= (1ll << 31) || b * hw > ((1ll << 31) - 1 - hw) / 100) return "global pool: 100 s + H W does not fit int32";
    }
    // block and lane indices are 32-bit (grid.x < 2^31, grid.y and grid.z < 2^16)
    const long long groups = (long long)a->C / 16;
    if ((long long)a->N * a->H * a->W * groups >= (1ll << 31)) return "too many elements for 32-bit lane indices";
    if (op == HAWQ_INCEP_POOL_MAX3S2 && (long long)Wo * groups > 65535ll * 64) return "max pool: output row too long";
    if (op == HAWQ_INCEP_POOL_GLOBAL && a->N > 65535) return "global pool: more than 65535 images";
    if (op == HAWQ_INCEP_POOL_AVG3) {
        int th, tw;
        avg3_tile(a, &th, &tw);
        if (a->N > 65535 || (long long)((a->H + th - 1) / th) * ((a->W + tw - 1) / tw) > 65535)
            return "average pool: more than 65535 images or tiles per image";
    }
    return nullptr;
}

// threads per block of a launch whose rows hold `n` lanes each: 64, 128 or 256, whichever leaves the fewest idle (ties: the larger)
int row_block(long long n) {
    int best = 256;
    long long waste = (n + 255) / 256 * 256 - n;
    for (int b = 128; b >= 64; b >>= 1) {
        const long long w = (n + b - 1) / b * b - n;
        if (w < waste) best = b, waste = w;
    }
    return best;
}

template <int IB, int OB>
void launch(const hawq_incep_pool_args *a, int op, hipStream_t s) {
    const unsigned cg = (unsigned)a->C / 16;
    if (op == HAWQ_INCEP_POOL_REQUANT) {
        const unsigned items = (unsigned)((long long)a->N * a->H * a->W * cg);
        hipLaunchKernelGGL((pool_requant_v<IB, OB>), dim3((items + 255) / 256), dim3(256), 0, s, *a, items);
    } else if (op == HAWQ_INCEP_POOL_MAX3S2) {
        const int Ho = (a->H - 3) / 2 + 1, Wo = (a->W - 3) / 2 + 1;
        const long long row = (long long)Wo * cg;
        const int b = row_block(row);
        hipLaunchKernelGGL((pool_max3s2_v<IB, OB>), dim3((unsigned)a->N * Ho, (unsigned)((row + b - 1) / b)), dim3(b), 0, s, *a, Ho, Wo);
    } else if (op == HAWQ_INCEP_POOL_AVG3) {
        int th, tw;
        avg3_tile(a, &th, &tw);
        const int ntx = (a->W + tw - 1) / tw, nty = (a->H + th - 1) / th;
        const size_t lds = (size_t)(th + 2) * (tw + 2) * AVG_CC * 2;
        hipLaunchKernelGGL((pool_avg3_v<IB, OB>), dim3((a->C + AVG_CC - 1) / AVG_CC, ntx * nty, a->N), dim3(256), lds, s, *a, th, tw, ntx);
    } else {
        hipLaunchKernelGGL((pool_global_v<IB, OB>), dim3((a->C + GL_CC - 1) / GL_CC, a->N), dim3(256), 0, s, *a);
    }
}

}  // namespace

extern "C" int hawq_incep_pool_v_avg3_tile(const hawq_incep_pool_args *a, int32_t *th, int32_t *tw) {
    const char *why = pool_v_refusal(a, HAWQ_INCEP_POOL_AVG3);
    HAWQ_REQUIRE(!why && th && tw, "hawq_incep_pool_v_avg3_tile: %s", why ? why : "null pointer");
    int h, w;
    avg3_tile(a, &h, &w);
    *th = h, *tw = w;
    return 0;
}

extern "C" int hawq_incep_pool_v_ok(const hawq_incep_pool_args *a, int op) { return pool_v_refusal(a, op) == nullptr; }

extern "C" int hawq_incep_pool_v(const hawq_incep_pool_args *a, int op, void *stream) {
    const char *why = pool_v_refusal(a, op);
    HAWQ_REQUIRE(!why, "hawq_incep_pool_v (op %d): %s", op, why);
    hipStream_t s = (hipStream_t)stream;
    if (a->in_bits == 16 && a->out_bits == 16) launch<16, 16>(a, op, s);
    else if (a->in_bits == 16) launch<16, 8>(a, op, s);
    else if (a->out_bits == 16) launch<8, 16>(a, op, s);
    else launch<8, 8>(a, op, s);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
