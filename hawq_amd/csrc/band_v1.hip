// 3x3 / stride 1 / pad 1 "band" kernels of rounds 1-3 (family 1 of conv_dispatch.hip), with the epilogues of conv_device.h.
// The generic pipeline re-fetches the activation tile once per filter tap (9x) and synchronises the workgroup
// once per 64-deep K chunk.  Here a workgroup that owns BM consecutive output pixels keeps, per 64-channel
// slice, the whole input BAND those pixels touch (their image rows plus one halo row above and below, each
// row with a zero column left and right) in LDS and reads the nine taps' B fragments from it at shifted
// addresses: activation traffic into LDS drops ~7x, only the weight tiles of the slice are streamed.  One
// pipeline step covers a whole filter ROW (3 taps, K = 192): one barrier per 24 MFMAs per wave.  Band rows are
// GLOBAL rows G = n*Ho + y, so the fill needs no image logic.
//   band ring : BSTAGES x 4 planes x BAND_PX band pixels x 16 B: plane j holds channels 16j..16j+15 of every band
//               pixel.  Consecutive pixels are 16 B apart, so a B-fragment read (16 lanes = 16 mostly consecutive
//               pixels per LDS cycle) is conflict-free WITHOUT a swizzle and every (tap, k-half) address is
//               base + immediate: the inner loop carries no address arithmetic.  The last 4 entries of each
//               plane are zeros: taps whose row lies outside the pixel's image read those.
//   W ring    : WS (3 or 4) stages x (3 taps x BN x 64 B), one stage per (slice, filter row) step, issued WS - 1
//               steps ahead
// Wave specialisation (NPROD > 0).  Measured on gfx950 (tools/ubench/mfma_rate.hip, HAWQ_DBG=128 stamps):
// the matrix pipe serves the OLDEST ready wave of a SIMD first, an LDS-DMA issue blocks its wave for 60-150
// cycles, and hipcc cannot overlap LDS reads with MFMAs once LDS-DMA is in the loop (see lds_read16).  With all
// waves symmetric, a step cost ~3300 cycles for 1536 cycles of MFMA work per SIMD.  So NPROD extra "producer"
// waves own every LDS-DMA issue and every vmcnt wait; the NW "consumer" waves only read fragments (hand
// software-pipelined) and issue MFMAs, and the two kinds meet at the per-step barrier.
#include "conv_dispatch.h"

namespace {

template <int BM_, int BN_, int WM_, int WN_, int BAND_PX_, int BSTAGES_, int MINB_, int NPROD_, int WS_ = 3>
struct BandCfg {
    static constexpr int WS = WS_;                            // W ring stages; W(s + WS - 1) is issued during step s
    static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_, MINB = MINB_, NPROD = NPROD_;
    static constexpr int NW = WM * WN;                        // consumer (MFMA) waves
    static constexpr int NT = (NW + NPROD) * 64;
    static constexpr int ND = NPROD > 0 ? NPROD : NW;         // waves that issue LDS-DMA
    static constexpr int PT = BM / WM / 32, CT = BN / WN / 32;
    static constexpr int BAND_PX = BAND_PX_, BSTAGES = BSTAGES_;  // band pixels per stage (launcher-checked bound)
    static constexpr int PLANE = BAND_PX * 16, BAND_BYTES = 4 * PLANE;
    static constexpr int BPI = BAND_PX / 16 / ND;             // band pieces (1 KiB LDS-DMA instructions) per issuing wave per stage
    static constexpr int RG = BN / 16;                        // 16-row groups of a W tap tile
    static constexpr int RPI = RG / ND, WPI = 3 * RPI;        // W row groups / pieces per issuing wave per step
    static constexpr int WTAP = BN * 64, WSTAGE = 3 * WTAP;
    static constexpr int LDS_BYTES = BSTAGES * BAND_BYTES + WS * WSTAGE;
    static_assert(RG % ND == 0 && (BAND_PX / 16) % ND == 0 && PT >= 1 && CT >= 1 && WS >= 3 && WS <= 5, "tile shape");
    static_assert(BM * BN * 2 <= LDS_BYTES, "epilogue staging aliases the rings");
};

// NIB: both operands hawq4 nibble-packed (Cin % 128 == 0).  A 64-byte slice is then 128 channels, the packed bytes
// travel through LDS untouched and every 16-byte fragment read (32 channels) feeds TWO MFMA K-steps after
// unpacking in registers (activations zero-extended, weights as value*16, accumulators shifted back by 4 - exact);
// both operands pair the same channels with the same K-step, so the channel order inside a slice is irrelevant.
// EPI: REQUANT, or RESIDUAL (single branch, uint16 residuals: the 3x3 second conv of a ResNet18/34 basic block).  The
// residual tile is fetched into the W ring once the K loop has released it (no extra LDS).
template <class C, bool NIB = false, bool TIE = false, int EPI = HAWQ_EPI_REQUANT>
__global__ __launch_bounds__(C::NT, C::MINB) void conv3x3_band_kernel(const ConvP p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const bool prof = HAWQ_DBG_BIT(p.dbg, 128) && p.dbgbuf;
    const long long t_entry = prof ? (long long)__builtin_readcyclecounter() : 0;
    const int tiles_c = p.Cout / C::BN;
    const int nwg = ((p.M + C::BM - 1) / C::BM) * tiles_c;
    int wg = blockIdx.x;
    {
        const int q = nwg >> 3, r = nwg & 7, xcd = wg & 7, idx = wg >> 3;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int tc = wg % tiles_c, tm = wg / tiles_c;
    const int m0 = tm * C::BM, c0 = tc * C::BN;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const bool consumer = wave < C::NW;
    const bool issuer = C::NPROD > 0 ? !consumer : true;
    const int dw = C::NPROD > 0 ? wave - C::NW : wave;       // index among the issuing waves
    char *band = smem, *wring = smem + C::BSTAGES * C::BAND_BYTES, *ctab_lds = smem + C::LDS_BYTES;
    const char *zero = reinterpret_cast<const char *>(g_zero16);

    const int Wo = p.Wo, Wb = Wo + 2;
    const int G0 = m0 / Wo - 1;                 // global row held by band row 0
    const int rowb = NIB ? p.Cin >> 1 : p.Cin;  // bytes per pixel / per filter tap of one output channel
    const int cchunks = rowb >> 6;
    const int nsteps = 3 * cchunks;             // step s = cc * 3 + kh
    const size_t slice_stride = p.in_planar ? (size_t)p.M * 64 : 64;  // bytes from one 64-byte channel slice to the next

    // ------------------------------------------------------------------ LDS-DMA side (issuing waves)
    const char *bsrc[C::BPI];   // band piece j = i * ND + dw fills 64 pixels of plane (j & 3)
    const char *wsrc[C::RPI];   // W row group r * ND + dw (16 rows), source-side swizzled like every operand tile
    if (issuer) {
        const int rows_total = p.N * p.Ho;
#pragma unroll
        for (int i = 0; i < C::BPI; ++i) {
            const int j = i * C::ND + dw;
            const int bpx = (j >> 2) * 64 + lane;
            const int br = bpx / Wb, bc = bpx - br * Wb;
            const int G = G0 + br, x = bc - 1;
            const bool v = (unsigned)G < (unsigned)rows_total && (unsigned)x < (unsigned)Wo && bpx < C::BAND_PX - 4;
            // NHWC: 16 bytes of a pixel row (64 lanes = 64 segments a row apart: slow, see ingest_shape.hip); planar:
            // plane (cc * 4 + (j & 3)) is [M][16 B], the lanes of a band row read consecutive 16-byte units
            bsrc[i] = !v ? nullptr
                      : p.in_planar ? (const char *)p.in + ((size_t)(j & 3) * p.M + (size_t)G * Wo + x) * 16
                                    : (const char *)p.in + ((size_t)G * Wo + x) * rowb + ((j & 3) << 4);
        }
#pragma unroll
        for (int r = 0; r < C::RPI; ++r) {
            const int row = (r * C::ND + dw) * 16 + (lane >> 2);
            wsrc[r] = (const char *)p.wgt + (size_t)(c0 + row) * ((size_t)9 * rowb) + (((lane & 3) ^ ((row >> 2) & 3)) << 4);
        }
    }
    auto issue_band = [&](int cc) {
        char *dst = band + (C::BSTAGES > 1 ? (cc & 1) * C::BAND_BYTES : 0);
#pragma unroll
        for (int i = 0; i < C::BPI; ++i) {
            const int j = i * C::ND + dw;
            const char *src = bsrc[i] ? bsrc[i] + (size_t)cc * slice_stride : zero;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                             (__attribute__((address_space(3))) void *)(dst + (j & 3) * C::PLANE + (j >> 2) * 1024), 16, 0, 0);
        }
    };
    auto issue_w = [&](int s, int cc, int kh) {  // the 3 taps of filter row kh, channel slice cc -> ring stage s % WS
        char *dst = wring + (s % C::WS) * C::WSTAGE + dw * 1024;
        const size_t off = (size_t)(kh * 3) * rowb + (cc << 6);
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
            for (int r = 0; r < C::RPI; ++r)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(wsrc[r] + off + (size_t)kw * rowb),
                                                 (__attribute__((address_space(3))) void *)(dst + kw * C::WTAP + r * (C::ND * 1024)), 16, 0, 0);
    };
    // after barrier #s (which closed step s-1): ring stage (s-1) % WS and band stage (cc+1)&1 are free
    auto issue_step = [&](int s, int cc, int kh) {
        if (C::BSTAGES > 1 && kh == 0 && cc + 1 < cchunks) issue_band(cc + 1);
        const int s2 = s + C::WS - 1;
        if (s2 < nsteps) issue_w(s2, s2 / 3, s2 % 3);
    };
    // Before barrier #(s+1) the issuing waves must have seen W(s+2) land.  With WS == 3 that is the W issued in this
    // very step (everything must have landed).  With WS >= 4 it was issued WS - 3 steps earlier: everything issued in
    // this step and in the WS - 4 steps before it - younger in program order, and LDS-DMA completes in order - may stay
    // in flight (a band prefetch happens in steps with kh == 0 only, so at most one of two consecutive steps has one).
    auto wait_step = [&](int s, int cc, int kh) {
        if (C::WS <= 3) {
            wait_vmcnt<0>();
            return;
        }
        const bool band_now = C::BSTAGES > 1 && kh == 0 && cc + 1 < cchunks;
        const bool w_now = s + C::WS - 1 < nsteps;
        if (C::WS == 4) {
            if (band_now) {
                if (w_now) wait_vmcnt<C::BPI + C::WPI>(); else wait_vmcnt<C::BPI>();
            } else {
                if (w_now) wait_vmcnt<C::WPI>(); else wait_vmcnt<0>();
            }
            return;
        }
        // WS == 5: this step's and the previous step's issues
        const int khp = kh == 0 ? 2 : kh - 1, ccp = kh == 0 ? cc - 1 : cc;
        const bool band_prev = C::BSTAGES > 1 && s >= 1 && khp == 0 && ccp + 1 < cchunks;
        const bool w_prev = s >= 1 && s - 1 + C::WS - 1 < nsteps;
        const int nw = (w_now ? 1 : 0) + (w_prev ? 1 : 0);
        if (band_now || band_prev) {
            if (nw == 2) wait_vmcnt<C::BPI + 2 * C::WPI>(); else if (nw == 1) wait_vmcnt<C::BPI + C::WPI>(); else wait_vmcnt<C::BPI>();
        } else {
            if (nw == 2) wait_vmcnt<2 * C::WPI>(); else if (nw == 1) wait_vmcnt<C::WPI>(); else wait_vmcnt<0>();
        }
    };

    if (issuer) {
        if (dw < C::BN / 64)  // requant constants of this channel tile -> LDS (oldest load: landed before anything else)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(p.ctab + (size_t)(c0 + dw * 64 + lane) * 4),
                                             (__attribute__((address_space(3))) void *)(ctab_lds + dw * 1024), 16, 0, 0);
        issue_band(0);
#pragma unroll
        for (int s = 0; s < C::WS - 1; ++s)
            if (s < nsteps) issue_w(s, s / 3, s % 3);
    }

    // ------------------------------------------------------------------ MFMA side (consumer waves)
    const int wave_m = wave % C::WM, wave_c = (wave / C::WM) % C::WN;
    const int l31 = lane & 31, h = lane >> 5;
    int bp0[C::PT], yy[C::PT];
#pragma unroll
    for (int q = 0; q < C::PT; ++q) {
        const int m = m0 + wave_m * (C::PT * 32) + q * 32 + l31;
        const int G = m / Wo, x = m - G * Wo;
        bp0[q] = (G - G0 - 1) * Wb + x;   // band pixel of tap (kh=0, kw=0)
        yy[q] = G % p.Ho;
    }
    int wofs[C::CT][2];  // A-fragment byte offsets inside a W tap tile (swizzled rows), k-halves 0/1
#pragma unroll
    for (int c = 0; c < C::CT; ++c)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) wofs[c][ks] = lds_off(wave_c * (C::CT * 32) + c * 32 + cperm(l31), 2 * ks + h);

    v16i acc[C::CT][C::PT];
#pragma unroll
    for (int c = 0; c < C::CT; ++c)
#pragma unroll
        for (int q = 0; q < C::PT; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][q][r] = 0;

    const long long t_begin = prof ? (long long)__builtin_readcyclecounter() : 0;
    // Barrier #0: band(0), W(0), W(1) visible.  Barrier #(s+1) closes step s; BEFORE it the issuing waves have
    // seen W(s+2) (and a band prefetch) land, so that the MFMA waves may request the first fragments of step
    // s+1 already at the end of step s and cross the barrier with their LDS reads in flight (the exposed
    // barrier + first-fetch latency was ~500 of ~2000 cycles per step).  Ring stage (s+2)%3 was last read in
    // step s-1, i.e. before barrier #s, after which W(s+2) is issued.
    if (C::NPROD > 0 && !consumer) {
        int cc = 0, kh = 0;
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        for (int s = 0; s < nsteps; ++s) {
            if (!HAWQ_DBG_BIT(p.dbg, 1)) issue_step(s, cc, kh);
            wait_step(s, cc, kh);
            __builtin_amdgcn_s_barrier();
            if (++kh == 3) kh = 0, ++cc;
        }
    } else {
        if (C::NPROD > 0) __builtin_amdgcn_s_setprio(2);  // MFMA waves win issue arbitration against the producers
        const bool early = wave < C::NW / 2;  // waves w and w + NW/2 share a SIMD (only used when NPROD == 0)
        unsigned ap[C::PT], wp[C::CT][2];
        // operand bases of step (s, cc, kh); everything inside the batches is base + compile-time immediate
        auto bases = [&](int s, int cc, int kh) {
            const char *bst = band + (C::BSTAGES > 1 ? (cc & 1) * C::BAND_BYTES : 0) + h * C::PLANE, *wst = wring + (s % C::WS) * C::WSTAGE;
#pragma unroll
            for (int q = 0; q < C::PT; ++q) {
                const bool rowok = (unsigned)(yy[q] + kh - 1) < (unsigned)p.Ho;  // else: another image's row / padding -> zeros
                ap[q] = lds_addr(bst) + (rowok ? bp0[q] + kh * Wb : C::BAND_PX - 4) * 16;
            }
#pragma unroll
            for (int c = 0; c < C::CT; ++c)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) wp[c][ks] = lds_addr(wst) + wofs[c][ks];
        };
        // 6 batches per step (tap kw = b / 2, k-half ks = b % 2) of CT x PT MFMAs, software-pipelined by hand: the
        // fragments of the next batch are requested from LDS before the MFMAs of the current one are issued.
        v4i wf[2][C::CT], af[2][C::PT];
#define BAND_FETCH(B, BUF)                                                                                        \
    if (!HAWQ_DBG_BIT(p.dbg, 4)) {                                                                                           \
        _Pragma("unroll") for (int c = 0; c < C::CT; ++c)                                                         \
            wf[BUF][c] = lds_read16<((B) >> 1) * C::WTAP>(wp[c][(B) & 1]);                                        \
        _Pragma("unroll") for (int q = 0; q < C::PT; ++q)                                                         \
            af[BUF][q] = lds_read16<((B) >> 1) * 16 + ((B) & 1) * (2 * C::PLANE)>(ap[q]);                         \
    }
#define BAND_MMA(B)                                                                                               \
    {                                                                                                             \
        _Pragma("unroll") for (int c = 0; c < C::CT; ++c) pin(wf[(B) & 1][c]);                                    \
        _Pragma("unroll") for (int q = 0; q < C::PT; ++q) pin(af[(B) & 1][q]);                                    \
        if constexpr (NIB) {                                                                                      \
            _Pragma("unroll") for (int hf = 0; hf < 2; ++hf) {                                                    \
                v4i w8[C::CT], a8[C::PT];                                                                         \
                _Pragma("unroll") for (int c = 0; c < C::CT; ++c)                                                 \
                    w8[c] = unpack16<true>((unsigned)wf[(B) & 1][c][2 * hf], (unsigned)wf[(B) & 1][c][2 * hf + 1]); \
                _Pragma("unroll") for (int q = 0; q < C::PT; ++q)                                                 \
                    a8[q] = unpack16<false>((unsigned)af[(B) & 1][q][2 * hf], (unsigned)af[(B) & 1][q][2 * hf + 1]); \
                _Pragma("unroll") for (int c = 0; c < C::CT; ++c)                                                 \
                    _Pragma("unroll") for (int q = 0; q < C::PT; ++q)                                             \
                        acc[c][q] = __builtin_amdgcn_mfma_i32_32x32x32_i8(w8[c], a8[q], acc[c][q], 0, 0, 0);      \
            }                                                                                                     \
        } else {                                                                                                  \
            _Pragma("unroll") for (int c = 0; c < C::CT; ++c)                                                     \
                _Pragma("unroll") for (int q = 0; q < C::PT; ++q)                                                 \
                    acc[c][q] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[(B) & 1][c], af[(B) & 1][q], acc[c][q], 0, 0, 0); \
        }                                                                                                         \
    }
#define BAND_BATCH(B)                                                                                             \
    {                                                                                                             \
        BAND_FETCH((B) + 1, ((B) + 1) & 1)                                                                        \
        wait_lgkm<C::CT + C::PT>();                                                                               \
        BAND_MMA(B)                                                                                               \
    }
        int cc = 0, kh = 0;
        if (C::NPROD == 0) wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        bases(0, 0, 0);
        BAND_FETCH(0, 0)
        for (int s = 0; s < nsteps; ++s) {
            BAND_BATCH(0)
            if (C::NPROD == 0 && early && !HAWQ_DBG_BIT(p.dbg, 1)) issue_step(s, cc, kh);
            BAND_BATCH(1)
            BAND_BATCH(2)
            BAND_BATCH(3)
            if (C::NPROD == 0 && !early && !HAWQ_DBG_BIT(p.dbg, 1)) issue_step(s, cc, kh);
            BAND_BATCH(4)
            if (++kh == 3) kh = 0, ++cc;
            if (s + 1 < nsteps) {  // first fragments of the next step (its operands are visible since the previous barrier)
                bases(s + 1, cc, kh);
                BAND_FETCH(0, 0)
                wait_lgkm<C::CT + C::PT>();
            } else {
                wait_lgkm<0>();
            }
            BAND_MMA(5)
            if (C::NPROD == 0) wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();
        }
#undef BAND_FETCH
#undef BAND_MMA
#undef BAND_BATCH
        if (C::NPROD > 0) __builtin_amdgcn_s_setprio(0);
    }
    const long long t_loop_end = prof ? (long long)__builtin_readcyclecounter() : 0;
    if constexpr (NIB) {  // weights were unpacked as value*16
#pragma unroll
        for (int c = 0; c < C::CT; ++c)
#pragma unroll
            for (int q = 0; q < C::PT; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[c][q][r] >>= 4;
    }
    __syncthreads();
    if constexpr (EPI == HAWQ_EPI_RESIDUAL) {
        using S = Stage<C>;
        static_assert(C::BM * C::BN * 2 <= C::WS * C::WSTAGE && C::BM * C::BN <= C::BSTAGES * C::BAND_BYTES, "epilogue tiles alias the rings");
        constexpr int NWALL = C::NT / 64, PPW = C::BM * S::RCPR / 64 / NWALL;
        static_assert(PPW * NWALL * 64 == C::BM * S::RCPR, "residual tile pieces");
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int base = (i * NWALL + wave) * 64, idx = base + lane;
            const int row = idx / S::RCPR, j = idx % S::RCPR;
            const int grow = (m0 + row < p.M) ? m0 + row : m0;
            const char *src = (const char *)p.res_in + ((size_t)grow * p.Cout + c0) * 2 + ((j ^ S::rsw(row)) << 4);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                             (__attribute__((address_space(3))) void *)(wring + base * 16), 16, 0, 0);
        }
        wait_vmcnt<0>();
        __syncthreads();
    }
    v16i dummy[1][1];
    epilogue_fast<C, EPI, false, TIE ? 2 : 0>(p, acc, dummy, m0, c0, smem, wring, ctab_lds, consumer);
    if (prof && blockIdx.x == 8 && t == 0) {
        p.dbgbuf[0] = t_begin - t_entry, p.dbgbuf[1] = t_loop_end - t_begin;
        p.dbgbuf[2] = (long long)__builtin_readcyclecounter() - t_loop_end, p.dbgbuf[3] = nsteps;
    }
}

using B0 = BandCfg<256, 64, 4, 1, 512, 1, 2, 0>;    // Cin == Cout == 64 (stage 1): 4 waves x (64 px x 64 ch), 2 workgroups per CU
using B1 = BandCfg<256, 128, 4, 2, 512, 2, 1, 8>;   // 8 MFMA waves x (64 px x 64 ch) + 8 producer waves (LDS-DMA ingest scales with the issuing waves)
using B2 = BandCfg<128, 128, 2, 4, 256, 2, 1, 8, 4>;   // 8 MFMA waves x (64 px x 32 ch) + 8 producers: twice the workgroups for 14x14 / 7x7
using B3 = BandCfg<256, 128, 4, 2, 384, 2, 1, 8, 4>;   // B1 with a 384-pixel band (14x14 / 7x7 maps): room for a 4-stage W ring
using B4 = BandCfg<128, 128, 2, 4, 256, 2, 1, 8, 5>;   // B2 with a 5-stage W ring (W issued 4 filter rows ahead)
// round 3: in stages 3-4 a launch has fewer workgroups than the chip has CUs and lasts as long as ONE workgroup (profiles/
// r03_mallprobe.md), so halve the work per workgroup and let two of them share a CU: 128 px x 64 ch, 4 MFMA waves (64 px x 32 ch)
// + 4 producers, 3-stage W ring of 12 KiB stages: 68 KiB.  4x the workgroups of B1 / B3 (392 for the 7x7 layers at batch 128)
using B5 = BandCfg<128, 64, 2, 2, 256, 2, 4, 4, 3>;
constexpr int NUM_BAND_TILES = 6;

typedef void (*KernelFn)(const ConvP);
struct BandInfo { KernelFn fn[2][2][2]; int bm, bn, band_px, bstages, lds, nt; };  // fn[hawq4][exact-tie][residual]
#define BAND_FN(B, N, T) {conv3x3_band_kernel<B, N, T, HAWQ_EPI_REQUANT>, conv3x3_band_kernel<B, N, T, HAWQ_EPI_RESIDUAL>}
#define BAND_ENTRY(B) {{{BAND_FN(B, false, false), BAND_FN(B, false, true)}, {BAND_FN(B, true, false), BAND_FN(B, true, true)}}, B::BM, B::BN, B::BAND_PX, B::BSTAGES, B::LDS_BYTES + B::BN * 16, B::NT}
const BandInfo kBand[NUM_BAND_TILES] = {BAND_ENTRY(B0), BAND_ENTRY(B1), BAND_ENTRY(B2), BAND_ENTRY(B3), BAND_ENTRY(B4), BAND_ENTRY(B5)};

}  // namespace

// tile ids tried, in this order, when the caller leaves the choice open for a layer that needs a band kernel
const int kBandPreference[NUM_BAND_TILES] = {0, 3, 1, 2, 4, 5};

int band_v1_count(void) { return NUM_BAND_TILES; }

// Does band tile `v` take this layer?  (3x3 / stride 1 / pad 1, single branch, fast-contract tables, int8 or hawq4
// operands, REQUANT or 16-bit RESIDUAL epilogue, the band of a pixel tile fits the LDS stage)
bool band_v1_applies(const hawq_conv_args *a, int v) {
    const BandInfo &bi = kBand[v];
    const int wo = a->W, band_rows = (bi.bm + wo - 1) / wo + 1 + 2;
    const bool nib = a->in_bits == 4 && a->w_bits == 4;
    const bool res = a->epilogue == HAWQ_EPI_RESIDUAL;
    const bool epi_ok = (a->epilogue == HAWQ_EPI_REQUANT && a->out_q) ||
                        (res && a->res_in && a->res_in_bits == 16 && (!a->res_out || a->res_out_bits == 16));
    const bool dense = (a->in_pitch == 0 || a->in_pitch == a->Cin * a->in_bits / 8) && (a->out_pitch == 0 || a->out_pitch == a->Cout);
    return a->KH == 3 && a->KW == 3 && a->stride == 1 && a->pad == 1 && a->out_sub < 2 && a->in2 == nullptr && a->fast_tables != 0 && epi_ok && dense &&
           ((a->in_bits == 8 && a->w_bits == 8) || (nib && a->Cin % 128 == 0)) && a->Cout % bi.bn == 0 &&
           band_rows * (wo + 2) <= bi.band_px - 4 && (bi.bstages > 1 || (a->Cin >> (nib ? 7 : 6)) == 1);
}

int band_v1_choose(const hawq_conv_args *, const ConvForm &f, const ConvP &p, ConvChoice &c) {
    const BandInfo &bi = kBand[c.tile];
    c.fn[0] = f.all44 ? 1 : 0, c.fn[1] = p.k0 == 2 ? 1 : 0, c.fn[2] = f.slot == HAWQ_EPI_RESIDUAL ? 1 : 0;
    c.grid = ((p.M + bi.bm - 1) / bi.bm) * (p.Cout / bi.bn), c.block = bi.nt, c.lds = bi.lds;
    return 0;
}

int band_v1_launch(const hawq_conv_args *, const ConvChoice &c, const ConvP &args, void *stream) {
    const BandInfo &bi = kBand[c.tile];
    ConvP p = args;
    p.dbgbuf = conv_dbg_buffer(p.dbg);
    static const bool band_attrs = [] {
        bool good = true;
        for (const BandInfo &b : kBand)
            for (int i = 0; i < 8; ++i)
                good &= hipFuncSetAttribute((const void *)b.fn[i >> 2][(i >> 1) & 1][i & 1], hipFuncAttributeMaxDynamicSharedMemorySize, b.lds) == hipSuccess;
        return good;
    }();
    HAWQ_REQUIRE(band_attrs, "hawq_conv2d: hipFuncSetAttribute failed for the band kernels");
    hipLaunchKernelGGL(bi.fn[c.fn[0]][c.fn[1]][c.fn[2]], dim3(c.grid), dim3(c.block), c.lds, (hipStream_t)stream, p);
    HAWQ_CHECK_HIP(hipGetLastError());
    if (HAWQ_DBG_BIT(p.dbg, 128) && p.dbgbuf) {  // experiment hook: per-phase cycles of one wave (synchronises!)
        long long hbuf[4];
        (void)hipStreamSynchronize((hipStream_t)stream);
        (void)hipMemcpy(hbuf, p.dbgbuf, sizeof(hbuf), hipMemcpyDeviceToHost);
        fprintf(stderr, "[band bm=%d bn=%d M=%d Cin=%d Cout=%d] steps %lld: prologue %lld | K loop %lld | epilogue %lld cycles (wave 0 of workgroup 8, s_memtime)\n",
                bi.bm, bi.bn, p.M, p.Cin, p.Cout, hbuf[3], hbuf[0], hbuf[1], hbuf[2]);
    }
    return 0;
}
