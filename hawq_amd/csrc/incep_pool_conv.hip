// 3x3 / stride 1 / pad 1 average pool + 1x1 conv in one launch (hawq_incep_avgpool_conv): the average-pool branches of the
// Inception-A, -B and -C units, whose pooled int8 tensor only the branch's 1x1 conv reads.  The two unchanged argument blocks of the
// launches it replaces: `p` of hawq_incep_avgpool_branch (p.out, p.ldo, p.c_off ignored) and `c` of hawq_incep_conv (c.in ignored).
// The bytes are those of the pool into a dense int8 tensor followed by the conv (REQUANT / REQUANT2); the tensor never leaves the
// workgroup.
//
// A workgroup (4 waves) owns a BAND of one image - R full-width rows, flattened into up to BM pixels - and ALL output channels, so
// every pooled value is computed once per launch (only the one-row halo at a band seam is requantised twice).  K = C is walked in
// chunks of KC = 64 channels.  Per chunk:
//   * the band's halo, (R + 2) x (W + 2) pixels x 64 channels, goes to LDS as int16 after `pre` (16-byte global loads into
//     registers one chunk ahead, zeros for the padding and for channels >= C), the staging of incep_pool.hip's AVG3;
//   * a lane owns 16 consecutive channels of a pixel: nine 32-byte LDS reads, the int32 sum, (100 s + 9) / 900, `post`, and one
//     16-byte write into the A-operand tile [pixel][64 bytes] (lds_off's swizzle, so the ds_read_b128 fragment reads below are
//     conflict-free) - pool items are spread over all 256 lanes whatever the waves' MFMA tiles are;
//   * the waves (WPX x WCH, each WM x WN MFMA tiles of 32 px x 32 ch, pixel tiles interleaved over WPX so that a short band still
//     feeds every wave) read their A fragments from that tile and their weight fragments straight from global memory
//     ([Cout][C] int8 rows in cperm order, loaded one chunk ahead) into v_mfma_i32_32x32x32_i8.
// Software pipelining inside each wave: iteration k pools chunk k into stage k & 1 of the A tile while the MFMAs of chunk k - 1 read
// stage (k - 1) & 1; the two are interleaved in the instruction stream (one share of the chunk's MFMAs behind every pool item), so
// the matrix pipe runs under the pool's VALU work of the same wave.  Producer / consumer waves were not used: the pool arithmetic is
// the bound (profiles/inception.md), and setting waves aside for a short MFMA job would take lanes away from it.  Two barriers per
// chunk (the halo is single-buffered: 42 KiB at 35 x 35); every loop bound is a kernel argument or a template constant.
#include "common.h"

namespace {

constexpr int KC = 64;          // channels per chunk
constexpr int MAX_COUT = 192;   // 6 channel tiles: 2 x 3 MFMA tiles per wave, 96 accumulator registers
constexpr int FILL_WGS = 256;   // bands shrink while a launch has fewer workgroups than the chip has CUs

// the two configurations: Cout <= 64 (the 35 x 35 maps) and Cout <= 192 (17 x 17, 8 x 8)
struct Config {
    int bm, nt32, wpx, wch, halo;
};
constexpr Config kWide = {256, 2, 4, 1, 336}, kDeep = {128, 6, 2, 2, 192};
// a band holds full rows: one row of W pixels must fit the pixel tile and its three halo rows of W + 2 the halo (wide: 110, deep: 62)
constexpr int max_w(const Config &k) { return k.bm < k.halo / 3 - 2 ? k.bm : k.halo / 3 - 2; }

struct Rq {
    int on, m, ek, lo, hi;
};
__device__ __forceinline__ int rq(int v, const Rq &r) { return r.on ? clampi(dyadic_rne(v, r.m, r.ek), r.lo, r.hi) : v; }

template <int IB, int BM, int NT32, int WPX, int WCH, int HALO>
__global__ __launch_bounds__(256) void incep_pool_conv_kernel(hawq_incep_pool_args p, hawq_incep_conv_args c, int R, int nb) {
    constexpr int WM = BM / 32 / WPX, WN = NT32 / WCH, NPI = BM * 4 / 256, NCH = (HALO * 4 + 255) / 256, LW = IB == 16 ? 2 : 1;
    constexpr int S = 2 * WM, SPI = S / NPI, ASTAGE = BM * KC;
    static_assert(WPX * WCH == 4 && BM % (32 * WPX) == 0 && NT32 % WCH == 0 && S % NPI == 0 && NCH <= 8, "configuration");
    static_assert(HALO * KC * 2 + 2 * ASTAGE <= 81920, "half a CU's LDS: the LDS does not keep a second workgroup off a CU");
    __shared__ __attribute__((aligned(16))) char hl[HALO * KC * 2];   // the halo: [row][column] pixels of 64 int16
    __shared__ __attribute__((aligned(16))) char al[2 * ASTAGE];      // two stages of the A tile: [pixel][64 int8], swizzled

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int wpx = wave % WPX, wch = wave / WPX, g = tid & 3;   // g: this lane's 16-channel group of a chunk, in every item
    const int n = (int)(blockIdx.x / (unsigned)nb), r0 = ((int)blockIdx.x - n * nb) * R;
    const int Rb = min(R, p.H - r0), M = Rb * p.W, HW2 = p.W + 2, HQ = (Rb + 2) * HW2 * 4;   // HQ <= HALO * 4 (bands_of)
    const int C = p.C, nchunks = (C + KC - 1) / KC;
    const Rq pre = {p.pre, p.m1, p.ek1, p.lo1, p.hi1}, post = {p.post, p.m2, p.ek2, p.lo2, p.hi2};
    const v4i zero = {0, 0, 0, 0};

    // halo item q = tid + 256 k: channels 16 g .. + 15 of halo pixel q >> 2 = (hy, hx), map pixel (r0 - 1 + hy, hx - 1); its
    // element offset in `in`, or -1 for the padding and beyond the band's halo
    long long goff[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int hp = (tid + 256 * k) >> 2, hy = hp / HW2, hx = hp - hy * HW2, iy = r0 - 1 + hy, ix = hx - 1;
        const bool in_map = 4 * hp < HQ && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        goff[k] = in_map ? (((long long)n * p.H + iy) * p.W + ix) * p.in_pitch + p.in_off + 16 * g : -1;
    }
    // loads are unconditional (a refused item reads the first bytes of the input) and zeroed when they are written to LDS
    v4i rg[NCH][LW];
    unsigned okm = 0;
    auto load_halo = [&](int c0) {
        okm = 0;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const bool ok = goff[k] >= 0 && c0 + 16 * g < C;
            const long long e = ok ? goff[k] + c0 : 0;
            const v4i *src = IB == 16 ? reinterpret_cast<const v4i *>((const int16_t *)p.in + e)
                                      : reinterpret_cast<const v4i *>((const int8_t *)p.in + e);
#pragma unroll
            for (int w = 0; w < LW; ++w) rg[k][w] = src[w];
            okm |= (unsigned)ok << k;
        }
    };
    auto write_halo = [&]() {
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int q = tid + 256 * k;
            if (q >= HQ) continue;
            int v[16];
            if (IB == 16) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[2 * i] = (int16_t)rg[k][0][i], v[2 * i + 1] = rg[k][0][i] >> 16;
                    v[8 + 2 * i] = (int16_t)rg[k][LW - 1][i], v[8 + 2 * i + 1] = rg[k][LW - 1][i] >> 16;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[4 * i] = (int8_t)rg[k][0][i], v[4 * i + 1] = (int8_t)(rg[k][0][i] >> 8);
                    v[4 * i + 2] = (int8_t)(rg[k][0][i] >> 16), v[4 * i + 3] = rg[k][0][i] >> 24;
                }
            }
            v4i d[2] = {zero, zero};
            if ((okm >> k) & 1) {   // positions outside the map contribute 0 after `pre`
#pragma unroll
                for (int i = 0; i < 16; ++i) v[i] = rq(v[i], pre);   // lo1, hi1 inside int16 (refusal)
#pragma unroll
                for (int i = 0; i < 8; ++i) d[i >> 2][i & 3] = (v[2 * i] & 0xffff) | (int)((unsigned)v[2 * i + 1] << 16);
            }
            v4i *dst = reinterpret_cast<v4i *>(hl + q * 32);
            dst[0] = d[0], dst[1] = d[1];
        }
    };

    // pool item `it`: channels 16 g .. + 15 of band pixel (tid >> 2) + 64 it; its window's first tap in the halo
    int hoff[NPI], aoff[NPI];
    bool pv[NPI];
#pragma unroll
    for (int it = 0; it < NPI; ++it) {
        const int pix = (tid >> 2) + 64 * it, py = pix / p.W, px = pix - py * p.W;
        pv[it] = pix < M;
        hoff[it] = pv[it] ? (py * HW2 + px) * (KC * 2) + 32 * g : 0;
        aoff[it] = lds_off(pix, g);
    }
    auto pool_item = [&](int it, int c0, int stage) {
        v4i d = zero;
        if (pv[it] && c0 + 16 * g < C) {
            int s[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = 0;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const v4i *src = reinterpret_cast<const v4i *>(hl + hoff[it] + ((tap / 3) * HW2 + tap % 3) * (KC * 2));
                const v4i a = src[0], b = src[1];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    s[2 * i] += (int16_t)a[i], s[2 * i + 1] += a[i] >> 16;
                    s[8 + 2 * i] += (int16_t)b[i], s[8 + 2 * i + 1] += b[i] >> 16;
                }
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = rq((100 * s[i] + 9) / 900, post);
#pragma unroll
            for (int i = 0; i < 4; ++i) d[i] = (int)pack4_i8(s[4 * i], s[4 * i + 1], s[4 * i + 2], s[4 * i + 3]);
        }
        *reinterpret_cast<v4i *>(al + stage * ASTAGE + aoff[it]) = d;
    };

    // weight fragments of a chunk: row 32 (wch WN + j) + cperm(l31), bytes c0 + 32 kk + 16 h .. + 15
    const int8_t *wrow[WN];
    bool wv[WN];
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        const int co = 32 * (wch * WN + j) + cperm(l31);
        wv[j] = co < c.Cout;
        wrow[j] = (const int8_t *)c.wgt + (wv[j] ? (size_t)co * C : 0);
    }
    v4i wcur[WN][2], wnext[WN][2];
    auto load_w = [&](int c0) {
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int cc = c0 + 32 * kk + 16 * h;
                const bool ok = wv[j] && cc < C;
                const v4i w = *reinterpret_cast<const v4i *>(wrow[j] + (ok ? cc : 0));
                wnext[j][kk] = ok ? w : zero;
            }
    };

    v16i acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;
    // share `sl` of a chunk's MFMAs: K half kk of pixel tile i WPX + wpx
    auto mfma_share = [&](int sl, int stage) {
        const int kk = sl / WM, i = sl % WM, t = i * WPX + wpx;
        if (32 * t >= M) return;   // wave-uniform: no pixel of this tile is stored
        const v4i af = *reinterpret_cast<const v4i *>(al + stage * ASTAGE + lds_off(32 * t + l31, 2 * kk + h));
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wcur[j][kk], af, acc[i][j], 0, 0, 0);
    };

    load_halo(0);
    write_halo();
    __syncthreads();
    for (int k = 0; k <= nchunks; ++k) {
        load_halo((k + 1) * KC);   // in flight under this iteration's work; beyond C every item is refused
        load_w(k * KC);
#pragma unroll
        for (int it = 0; it < NPI; ++it) {
            if (k < nchunks) pool_item(it, k * KC, k & 1);
            if (k > 0) {
#pragma unroll
                for (int sl = 0; sl < SPI; ++sl) mfma_share(it * SPI + sl, (k - 1) & 1);
            }
        }
        __syncthreads();   // every lane has read chunk k's halo; stage k & 1 of the A tile is complete
        if (k + 1 < nchunks) write_halo();
#pragma unroll
        for (int j = 0; j < WN; ++j) wcur[j][0] = wnext[j][0], wcur[j][1] = wnext[j][1];
        __syncthreads();   // chunk k + 1's halo is in LDS
    }

    // acc[i][j][r] = channel 32 (wch WN + j) + 16 h + r of band pixel 32 (i WPX + wpx) + l31; hawq_incep_conv's REQUANT / REQUANT2
    // epilogue, statement for statement (incep_tile_body.h)
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        const int pix = 32 * (i * WPX + wpx) + l31;
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int cb = 32 * (wch * WN + j) + 16 * h;
            if (pix >= M || cb >= c.Cout) continue;   // Cout % 16 == 0: the 16 channels of a lane half are all valid or all not
            const size_t row = ((size_t)((long long)n * p.H + r0) * p.W + pix) * c.ldo + c.c_off + cb;   // a multiple of 16 elements
            int q[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cb + r;
                int v = acc[i][j][r] + c.bias[co];
                if (c.relu) v = max(v, 0);
                q[r] = clampi(dyadic_rne(v, c.m[co], c.ek[co]), c.q_lo, c.q_hi);
                if (c.epilogue == HAWQ_INCEP_REQUANT2) q[r] = clampi(dyadic_rne(q[r], c.m2, c.ek2), c.q2_lo, c.q2_hi);
            }
            if (c.out_bits == 16) {
                v4i *o = reinterpret_cast<v4i *>((int16_t *)c.out + row);
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
                *reinterpret_cast<v4i *>((int8_t *)c.out + row) = d;
            }
        }
    }
}

// the band of a launch: as many full rows as the configuration's pixel tile and halo hold, evened out over the map, and halved
// while the launch has fewer workgroups than FILL_WGS (small batches: more, shorter workgroups), as avg3_tile does
struct Bands {
    int R, nb;
};
Bands bands_of(const Config &k, int N, int H, int W) {
    int R = k.bm / W;
    if (R > k.halo / (W + 2) - 2) R = k.halo / (W + 2) - 2;
    if (R > H) R = H;
    int nb = (H + R - 1) / R;
    R = (H + nb - 1) / nb;
    while (R > 2 && (long long)N * nb < FILL_WGS) R = (R + 1) / 2, nb = (H + R - 1) / R;
    return {R, nb};
}

// why the kernel does not take a pair (NULL: it does).  No pointer is dereferenced.
const char *refusal(const hawq_incep_pool_args *p, const hawq_incep_conv_args *c) {
    if (!p || !c) return "null argument block";
    if (!p->in || !c->wgt || !c->bias || !c->out || !c->m || !c->ek) return "null pointer";
    if (c->KH != 1 || c->KW != 1 || c->stride != 1 || c->pad_h != 0 || c->pad_w != 0) return "the conv must be 1x1, stride 1, pad 0";
    if (p->N <= 0 || p->H <= 0 || p->W <= 0 || p->C <= 0 || c->Cout <= 0) return "bad shape";
    if (c->N != p->N || c->H != p->H || c->W != p->W || c->Cin != p->C) return "the conv does not read the pool's tensor (N, H, W, Cin)";
    if (p->out_bits != 8) return "the pooled tensor must be int8 (out_bits 8)";
    if (p->in_bits != 8 && p->in_bits != 16) return "in_bits must be 8 or 16";
    if (p->pre && (p->lo1 < -32768 || p->hi1 > 32767 || p->lo1 > p->hi1)) return "pre clamp outside int16";
    if (p->post && (p->lo2 < -128 || p->hi2 > 127 || p->lo2 > p->hi2)) return "post clamp outside int8";
    if (!p->post && !(p->pre ? (p->lo1 >= -128 && p->hi1 <= 127) : p->in_bits == 8)) return "a narrowing pool needs a post requant";
    if (p->C % 16 || p->in_pitch % 16 || p->in_off % 16 || c->Cout % 16 || c->ldo % 16 || c->c_off % 16)
        return "C, in_pitch, in_off, Cout, ldo and c_off must be multiples of 16";
    if (p->in_off < 0 || p->in_pitch < (long long)p->in_off + p->C) return "input channel slice outside its rows";
    if (c->c_off < 0 || c->ldo < (long long)c->c_off + c->Cout) return "ldo < c_off + Cout";
    if (((uintptr_t)p->in | (uintptr_t)c->wgt | (uintptr_t)c->out) & 15) return "in, wgt and out must be 16-byte aligned";
    if (c->epilogue != HAWQ_INCEP_REQUANT && c->epilogue != HAWQ_INCEP_REQUANT2) return "only the REQUANT and REQUANT2 epilogues";
    if (c->out_bits != 8 && c->out_bits != 16) return "out_bits must be 8 or 16";
    const int lim = c->out_bits == 16 ? 32767 : 127;
    if (c->q_lo < -lim - 1 || c->q_hi > lim || c->q_lo > c->q_hi ||
        (c->epilogue == HAWQ_INCEP_REQUANT2 && (c->q2_lo < -lim - 1 || c->q2_hi > lim || c->q2_lo > c->q2_hi)))
        return "clamp bounds outside the store";
    if (c->Cout > MAX_COUT) return "more than 192 output channels";
    const Config &k = c->Cout <= 32 * kWide.nt32 ? kWide : kDeep;
    if (p->W > max_w(k)) return "map wider than a band of full rows holds (110 columns for Cout <= 64, else 62)";
    if ((long long)p->N * bands_of(k, p->N, p->H, p->W).nb >= (1ll << 31)) return "too many workgroups";
    return nullptr;
}

template <int IB>
void launch(const hawq_incep_pool_args *p, const hawq_incep_conv_args *c, hipStream_t s) {
    if (c->Cout <= 32 * kWide.nt32) {
        const Bands b = bands_of(kWide, p->N, p->H, p->W);
        hipLaunchKernelGGL((incep_pool_conv_kernel<IB, kWide.bm, kWide.nt32, kWide.wpx, kWide.wch, kWide.halo>),
                           dim3((unsigned)p->N * b.nb), dim3(256), 0, s, *p, *c, b.R, b.nb);
    } else {
        const Bands b = bands_of(kDeep, p->N, p->H, p->W);
        hipLaunchKernelGGL((incep_pool_conv_kernel<IB, kDeep.bm, kDeep.nt32, kDeep.wpx, kDeep.wch, kDeep.halo>),
                           dim3((unsigned)p->N * b.nb), dim3(256), 0, s, *p, *c, b.R, b.nb);
    }
}

}  // namespace

extern "C" int hawq_incep_avgpool_conv_ok(const hawq_incep_pool_args *p, const hawq_incep_conv_args *c) {
    const char *why = refusal(p, c);
    if (why) hawq_set_error("hawq_incep_avgpool_conv: %s", why);
    return why ? 0 : 1;
}

extern "C" int hawq_incep_avgpool_conv(const hawq_incep_pool_args *p, const hawq_incep_conv_args *c, void *stream) {
    const char *why = refusal(p, c);
    HAWQ_REQUIRE(!why, "hawq_incep_avgpool_conv: %s", why);
    if (p->in_bits == 16) launch<16>(p, c, (hipStream_t)stream);
    else launch<8>(p, c, (hipStream_t)stream);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
