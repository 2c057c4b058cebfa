// 3x3 / stride 1 conv + 3x3 / stride 2 max pool in one launch (hawq_incep_conv_band_pool): the stem pairs q_conv3 + q_pool1 and
// q_conv5 + q_pool2 of InceptionV3, whose full-resolution tensor only the pool reads.  hawq_incep_conv's argument block; out, ldo and
// c_off describe the POOLED tensor.  The bytes are those of hawq_incep_conv (REQUANT) into a dense tensor followed by
// hawq_incep_maxpool3s2 without tables; the dense tensor never leaves the workgroup.
//
// A workgroup (4 waves) owns a WALK: one image, BN output channels, a strip of SW conv columns (PW = (SW - 1) / 2 pooled columns;
// neighbouring strips recompute the one conv column they share).  It walks the strip downwards in steps of R conv rows:
//   * the step's input halo, (R + 2) x (SW + 2) pixels, goes into LDS once as in incep_band.hip (16-byte loads, zeros for the
//     padding, padded pixel stride); the weights of the BN channels stay in LDS for every walk of the workgroup; the next step's halo
//     (of this walk or the next) is loaded to registers in front of the MFMAs and written to LDS behind them;
//   * a 32-lane MFMA tile covers 32 / SW conv rows of SW columns (SW = 16: two rows), so a 16-column strip fills its tiles;
//   * the requantised values (hawq_incep_conv's REQUANT statements) go, as 16-bit integers, to an LDS tile of R + 2 conv rows used
//     as a ring: conv row y lives in slot y % (R + 2).  Step t computes rows t R .. t R + R - 1 and, after a barrier, pools the rows
//     r = t R / 2 - 1 .. t R / 2 + R / 2 - 2 (conv rows t R - 2 .. t R + R - 2): the two rows a step shares with the one before it
//     are still in the ring, so no conv row of a strip is computed twice.  Walking on to another strip needs no reset: its first
//     step pools r >= 0 only, from rows that step wrote;
//   * in the pool phase a lane owns 16 consecutive channels of a pooled pixel: nine 32-byte LDS reads, packed 16-bit maxima, one
//     16-byte (int8) or two 16-byte (int16) stores.
// Conv rows >= Ho and columns >= Wo of the last step and strip are computed from a zero-filled halo and belong to no window that is
// stored.  Three barriers per step; every loop bound is a kernel argument.
#include "common.h"

extern "C" int hawq_incep_conv_band_ok(const hawq_incep_conv_args *a);

namespace {

constexpr int MAX_WGS = 1024;   // workgroups of a launch, all channel blocks together: walks beyond that are walked in turn

typedef short v8s __attribute__((ext_vector_type(8)));

// per Cin / 16: output channels per workgroup, conv rows per step, conv columns of a strip, padding bytes of a halo pixel and of a
// tile pixel in LDS
struct PoolShape {
    int bn, r, sw, pad, tpad;
};
constexpr PoolShape kPool[7] = {{0, 0, 0, 0, 0},   {64, 8, 32, 0, 16}, {64, 8, 32, 16, 16}, {64, 8, 16, 0, 16},
                                {64, 8, 16, 16, 16}, {64, 8, 16, 0, 0},  {32, 16, 16, 0, 0}};

template <int C16, int BN, int R, int SW, int PAD, int TPAD>
__global__ __launch_bounds__(256) void incep_band_pool_kernel(hawq_incep_conv_args a, int Hp, int Wp, int nstrips, int nsteps,
                                                              int nwalks) {
    constexpr int U = 9 * C16, S = (U + 1) / 2, CIN = 16 * C16, PS = CIN + PAD, WROW = (U | 1) * 16, BC = SW + 2, PW = (SW - 1) / 2;
    constexpr int TR = 32 / SW, WM = R * SW / 128, WN = BN / 32, NQ = (R + 2) * BC * C16, NCH = (NQ + 255) / 256;
    constexpr int RING = R + 2, OPS = 2 * BN + TPAD, CG = BN / 16, ITEMS = (R / 2) * PW * CG;
    static_assert(BN * WROW + (R + 2) * BC * PS + RING * SW * OPS <= 81920, "two workgroups share a CU's LDS");
    static_assert(WM >= 1 && WM * WN > 1 && R % 2 == 0 && 32 % SW == 0, "a wave owns more than one MFMA tile");
    __shared__ __attribute__((aligned(16))) char wl[BN * WROW];            // weight row q: channel cblock + (q & ~31) + cperm(q & 31)
    __shared__ __attribute__((aligned(16))) char bl[(R + 2) * BC * PS];    // the halo: [row][column] pixels of PS bytes
    __shared__ __attribute__((aligned(16))) char tl[RING * SW * OPS];      // the conv tile: [slot][column] pixels of BN int16

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
    // bytes of the input) and zeroed when they are written to LDS, as in incep_band.hip
    v4i rg[NCH];
    unsigned okm = 0;
    auto load = [&](int walk, int t) {
        const int strip = walk % nstrips, n = walk / nstrips;
        const int iy0 = t * R - a.pad_h, ix0 = strip * 2 * PW - a.pad_w;
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
    // MFMA tile i of the wave: conv rows (wave WM + i) TR .. + TR - 1 of the step; lane l31 is pixel (l31 / SW, l31 % SW) of it
    const int lrow = wave * WM * TR + l31 / SW, lcol = l31 % SW;
    const char *abase = bl + (lrow * BC + lcol) * PS + (C16 % 2 == 0 ? 16 * h : 0);
    const char *bbase = wl + l31 * WROW;

    int walk = blockIdx.x, t = 0;   // the grid holds no more workgroups than walks
    load(walk, t);
    write();
    for (;;) {
        __syncthreads();   // the halo (and, the first time, the weights) is in LDS; the pool phase of the step before is over
        int nwalk = walk, nt = t + 1;
        if (nt == nsteps) nwalk = walk + gridDim.x, nt = 0;
        const bool more = nwalk < nwalks;
        if (more) load(nwalk, nt);   // in flight under the MFMAs

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
            for (int i = 0; i < WM; ++i) af[i] = *reinterpret_cast<const v4i *>(abase + i * TR * BC * PS + ao);
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
        __syncthreads();   // every wave has read this step's halo
        if (more) write();

        // acc[i][j][r] = channel cblock + 32 j + 16 h + r of conv pixel (t R + lrow + i TR, column lcol of the strip);
        // hawq_incep_conv's REQUANT epilogue, statement for statement, into the ring
#pragma unroll
        for (int i = 0; i < WM; ++i) {
            const int slot = (t * R + lrow + i * TR) % RING;
            char *px = tl + (slot * SW + lcol) * OPS;
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                const int cl = 32 * j + 16 * h, cbk = cblock + cl;
                if (cbk >= a.Cout) continue;   // Cout % 16 == 0: a lane half's 16 channels are valid or not
                int q[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = cbk + r;
                    int v = acc[i][j][r] + a.bias[co];
                    if (a.relu) v = max(v, 0);
                    q[r] = clampi(dyadic_rne(v, a.m[co], a.ek[co]), a.q_lo, a.q_hi);
                }
                v4i *o = reinterpret_cast<v4i *>(px + 2 * cl);
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    v4i d;
#pragma unroll
                    for (int e = 0; e < 4; ++e) d[e] = (q[8 * r + 2 * e] & 0xffff) | (int)((unsigned)q[8 * r + 2 * e + 1] << 16);
                    o[r] = d;
                }
            }
        }
        __syncthreads();   // the step's conv rows are in the ring

        // pooled rows t R / 2 - 1 .. + R / 2 - 1 of the strip: item = (row, pooled column, 16-channel group)
        const int strip = walk % nstrips, n = walk / nstrips;
        for (int it = tid; it < ITEMS; it += 256) {
            const int cg = it % CG, pcl = (it / CG) % PW, pr = t * (R / 2) - 1 + it / (CG * PW), pc = strip * PW + pcl;
            const int cbk = cblock + 16 * cg;
            if (pr < 0 || pr >= Hp || pc >= Wp || cbk >= a.Cout) continue;
            v8s lo = {-32768, -32768, -32768, -32768, -32768, -32768, -32768, -32768}, hi = lo;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const char *rowp = tl + (((2 * pr + dy) % RING) * SW + 2 * pcl) * OPS + 32 * cg;
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const v8s *p = reinterpret_cast<const v8s *>(rowp + dx * OPS);
                    lo = __builtin_elementwise_max(lo, p[0]);
                    hi = __builtin_elementwise_max(hi, p[1]);
                }
            }
            const size_t row = (((size_t)n * Hp + pr) * Wp + pc) * a.ldo + a.c_off + cbk;   // a multiple of 16 elements (_ok)
            if (a.out_bits == 16) {
                v8s *o = reinterpret_cast<v8s *>((int16_t *)a.out + row);
                o[0] = lo;
                o[1] = hi;
            } else {
                v4i d;
                d[0] = (int)pack4_i8(lo[0], lo[1], lo[2], lo[3]);
                d[1] = (int)pack4_i8(lo[4], lo[5], lo[6], lo[7]);
                d[2] = (int)pack4_i8(hi[0], hi[1], hi[2], hi[3]);
                d[3] = (int)pack4_i8(hi[4], hi[5], hi[6], hi[7]);
                *reinterpret_cast<v4i *>((int8_t *)a.out + row) = d;
            }
        }
        if (!more) break;
        walk = nwalk, t = nt;
    }
}

struct Walks {
    int Hp, Wp, nstrips, nsteps;
    long long nwalks;
};

Walks walks_of(const hawq_incep_conv_args *a) {
    const PoolShape s = kPool[a->Cin >> 4];
    const int Ho = a->H + 2 * a->pad_h - 2, Wo = a->W + 2 * a->pad_w - 2, Hp = (Ho - 3) / 2 + 1, Wp = (Wo - 3) / 2 + 1;
    const int pw = (s.sw - 1) / 2, nstrips = (Wp + pw - 1) / pw;
    const int nsteps = (Hp + 1 + s.r / 2 - 1) / (s.r / 2);   // the last pooled row Hp - 1 is stored by step (Hp + 1) / (R / 2), rounded up
    return {Hp, Wp, nstrips, nsteps, (long long)a->N * nstrips};
}

// why the kernel does not take a launch (NULL: it does).  No pointer is dereferenced.
const char *pool_refusal(const hawq_incep_conv_args *a) {
    if (!a || a->epilogue != HAWQ_INCEP_REQUANT) return "only the REQUANT epilogue";
    if (!hawq_incep_conv_band_ok(a)) return "hawq_incep_conv_band refuses the conv";
    if (a->out_bits != 8 && a->out_bits != 16) return "out_bits must be 8 or 16";
    if (a->H + 2 * a->pad_h - 2 < 3 || a->W + 2 * a->pad_w - 2 < 3) return "the conv output is smaller than the pool window";
    if (walks_of(a).nwalks >= (1ll << 31) - MAX_WGS) return "too many strips";   // the kernel counts walks in an int
    return nullptr;
}

template <int C16>
void launch(const hawq_incep_conv_args *a, hipStream_t stream) {
    constexpr PoolShape s = kPool[C16];
    const Walks w = walks_of(a);
    const int gy = (a->Cout + s.bn - 1) / s.bn, cap = MAX_WGS / gy > 0 ? MAX_WGS / gy : 1;
    dim3 grid((unsigned)(w.nwalks < cap ? w.nwalks : cap), (unsigned)gy);
    hipLaunchKernelGGL((incep_band_pool_kernel<C16, s.bn, s.r, s.sw, s.pad, s.tpad>), grid, dim3(256), 0, stream, *a, w.Hp, w.Wp,
                       w.nstrips, w.nsteps, (int)w.nwalks);
}

}  // namespace

extern "C" int hawq_incep_conv_band_pool_ok(const hawq_incep_conv_args *a) {
    const char *why = pool_refusal(a);
    if (why) hawq_set_error("hawq_incep_conv_band_pool: %s", why);
    return why ? 0 : 1;
}

extern "C" int hawq_incep_conv_band_pool(const hawq_incep_conv_args *a, void *stream) {
    const char *why = pool_refusal(a);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_band_pool: %s", why);
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
