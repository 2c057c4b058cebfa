// Cross-workgroup split-K form of hawq_conv2d for launches with few output tiles (batch 1-16 inference).
//
// At 64 images per chain the late stages already launch 98-392 workgroups; at 1-16 images the stage 3-4 convs launch
// 8-50 (ResNet50 batch 1: the stage-4 3x3 conv, M = 49, K = 4608, runs on 8 workgroups of a 256-CU chip) and every launch
// lasts as long as one workgroup's whole K loop.  Here the grid is (64 px x 64 ch output tiles) x (K slices): each slice
// workgroup runs the asynchronous MFMA pipeline of conv_device.h over its share of the K chunks and writes its int32
// partial tile to a slab with plain vector stores; the workgroup that arrives last at its tile sums the slabs and runs
// the SAME epilogue code as hawq_conv2d (epilogue_fast / epilogue_generic of conv_device.h).  Integer addition is exact
// in any order, so the outputs are bit-identical to hawq_conv2d whatever the slice count or the arrival order.
//
// Arrival protocol (placement independent: a tile's slices may run on different XCDs, each with its own L2):
//   every thread: slab stores -> agent-scope release fence;  workgroup barrier;
//   thread 0: relaxed agent-scope fetch_add on the tile's counter; "last" goes to the other waves through LDS;
//   the last workgroup: agent-scope acquire fence -> reads the slabs -> resets the counter to 0 for the next launch.
// Nothing spins or waits on another workgroup, so any residency of the grid is fine.
//
// Workspace (hawq_conv2d_splitk_workspace): slab [tiles][S + S2][4 waves][4 register quads][64 lanes][4] int32 - each
// slab is one 64 x 64 tile of partial sums in MFMA register order - and one int32 counter per output tile, zero before the
// first launch (every launch leaves them zero).  tiles = ceil(M / 64) * Cout / 64.  The main branch's K chunks (KH * KW *
// Cin / 64) are cut into S equal slices; a second branch (the identity 1x1 conv of a resize unit) is cut into S2 slices of
// its own, of the largest chunk count that divides Cin2 / 64 and does not exceed the main branch's.
#include "conv_dispatch.h"

namespace {

using SK = Cfg<64, 64, 2, 2, 4>;                // 4 waves x (32 px x 32 ch), 4-stage ring, 64-channel chunks
constexpr int SK_TILE = SK::BM * SK::BN;         // int32 partial sums per slab
constexpr int SK_RES = SK::BM * SK::BN * 2;      // uint16 residual tile of the fast RESIDUAL epilogue
constexpr int SK_CTAB = SK::BN * 16 * 2;         // requant constants of both branches
constexpr int SK_LDS = SK::LDS_BYTES + SK_RES + SK_CTAB + 16;   // + the "last arriver" word

struct SplitP {
    int32_t *slab;
    int32_t *counters;
    int tiles_c, ntiles;
    int s1, s2;   // slices of the main / second branch
    int q1, q2;   // ring stages per slice of each branch
    int ns1;      // ring stages of the main branch
};

template <int EPI, bool DUAL, bool FAST, bool TIE, bool PLANAR>
__global__ __launch_bounds__(SK::NT, SK::MINB) void conv_splitk_kernel(const ConvP p, const SplitP s) {
    using C = SK;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tile = blockIdx.x % s.ntiles, z = blockIdx.x / s.ntiles;   // slice-major: a tile's slices spread over the chip
    const int m0 = (tile / s.tiles_c) * C::BM, c0 = (tile % s.tiles_c) * C::BN;
    const int nsl = s.s1 + (DUAL ? s.s2 : 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    v16i acc[C::CT][C::PT], acc2[C::CT][C::PT];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][0][r] = 0;
    const int kb = z < s.s1 ? z * s.q1 : s.ns1 + (z - s.s1) * s.q2;
    const int ke = kb + (z < s.s1 ? s.q1 : s.q2);
    // one accumulator set per slice: a slice never crosses the branch boundary (both arguments are `acc`)
    gemm_pipeline<C, DUAL, false, true, PLANAR>(acc, acc, p, m0, c0, smem, kb, ke);

    const size_t tile_base = (size_t)tile * nsl * SK_TILE;
    int32_t *mine = s.slab + tile_base + (size_t)z * SK_TILE + wave * 1024;
#pragma unroll
    for (int g = 0; g < 4; ++g)
        reinterpret_cast<v4i *>(mine)[g * 64 + lane] = v4i{acc[0][0][4 * g], acc[0][0][4 * g + 1], acc[0][0][4 * g + 2], acc[0][0][4 * g + 3]};
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // this thread's slab stores are visible chip-wide
    __syncthreads();
    int *last = reinterpret_cast<int *>(smem + SK_LDS - 16);
    if (threadIdx.x == 0) {
        const int arrived = __hip_atomic_fetch_add(s.counters + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *last = arrived == nsl - 1;
    }
    __syncthreads();
    if (!*last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // every other slice's stores are visible to this workgroup
    if (threadIdx.x == 0) s.counters[tile] = 0;          // all slices have arrived: nobody touches it again in this launch

#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][0][r] = 0, acc2[0][0][r] = 0;
    const int32_t *base = s.slab + tile_base + wave * 1024;
    for (int j = 0; j < s.s1; ++j) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const v4i v = reinterpret_cast<const v4i *>(base + (size_t)j * SK_TILE)[g * 64 + lane];
            acc[0][0][4 * g] += v.x, acc[0][0][4 * g + 1] += v.y, acc[0][0][4 * g + 2] += v.z, acc[0][0][4 * g + 3] += v.w;
        }
    }
    if constexpr (DUAL) {
        for (int j = s.s1; j < nsl; ++j) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const v4i v = reinterpret_cast<const v4i *>(base + (size_t)j * SK_TILE)[g * 64 + lane];
                acc2[0][0][4 * g] += v.x, acc2[0][0][4 * g + 1] += v.y, acc2[0][0][4 * g + 2] += v.z, acc2[0][0][4 * g + 3] += v.w;
            }
        }
    }

    if constexpr (FAST) {
        char *res_tile = smem + p.ring_bytes;
        char *ctab_lds = res_tile + (EPI == HAWQ_EPI_RESIDUAL ? SK_RES : 0);
        if (wave < C::BN / 64)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(p.ctab + (size_t)(c0 + wave * 64 + lane) * 4),
                                             (__attribute__((address_space(3))) void *)(ctab_lds + wave * 1024), 16, 0, 0);
        if constexpr (DUAL) {
            if (wave >= C::NW / 2 && wave - C::NW / 2 < C::BN / 64)
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void *)(p.ctab_id + (size_t)(c0 + (wave - C::NW / 2) * 64 + lane) * 4),
                    (__attribute__((address_space(3))) void *)(ctab_lds + C::BN * 16 + (wave - C::NW / 2) * 1024), 16, 0, 0);
        }
        if constexpr (EPI == HAWQ_EPI_RESIDUAL && !DUAL) prefetch_residual<C>(p, m0, c0, res_tile);
        wait_vmcnt<0>();
        __syncthreads();
        epilogue_fast<C, EPI, DUAL, TIE ? 2 : 0>(p, acc, acc2, m0, c0, smem, res_tile, ctab_lds);
    } else {
        epilogue_generic<C, EPI, DUAL>(p, acc, acc2, m0, c0);
    }
}

typedef void (*SplitFn)(const ConvP, const SplitP);

struct SplitPlan {
    int s1, s2, q1, q2, ns1, tiles_c, ntiles, M, Ho, Wo;
    long long slab_bytes, counter_bytes;
};

// the staged fast-contract epilogue (epilogue_fast), as opposed to the direct one
bool splitk_fast_epi(const ConvForm &f) { return f.fast && f.needs_tables && !f.wide_res && !f.signed_res; }

// Does the split-K kernel take this launch with `slices` slices of the main branch?  0 = yes (plan filled), else the
// reason goes to hawq_last_error.  Checks the form of the launch (geometry, widths, epilogue, layouts), not its pointers.
int splitk_plan(const hawq_conv_args *a, int slices, SplitPlan &sp) {
    HAWQ_REQUIRE(a != nullptr, "hawq_conv2d_splitk: null args");
    HAWQ_REQUIRE(slices >= 2, "hawq_conv2d_splitk: slices=%d (at least 2)", slices);
    HAWQ_REQUIRE(a->Cin > 0 && a->Cin % 64 == 0 && a->Cout > 0 && a->Cout % 64 == 0, "hawq_conv2d_splitk: Cin / Cout must be positive multiples of 64");
    HAWQ_REQUIRE(a->N > 0 && a->H > 0 && a->W > 0, "hawq_conv2d_splitk: bad geometry");
    HAWQ_REQUIRE(a->in_bits == 8 && a->w_bits == 8, "hawq_conv2d_splitk: int8 operands only (in_bits %d, w_bits %d)", a->in_bits, a->w_bits);
    const bool k1 = a->KH == 1 && a->KW == 1 && a->pad == 0, k3 = a->KH == 3 && a->KW == 3 && a->pad == 1;
    HAWQ_REQUIRE((k1 || k3) && (a->stride == 1 || a->stride == 2), "hawq_conv2d_splitk: 1x1 / pad 0 or 3x3 / pad 1 convs with stride 1 or 2 only");
    HAWQ_REQUIRE(a->n_valid == 0 && (a->in_pitch == 0 || a->in_pitch == a->Cin) && (a->out_pitch == 0 || a->out_pitch == a->Cout),
                 "hawq_conv2d_splitk: n_valid / in_pitch / out_pitch are not supported");
    HAWQ_REQUIRE(a->out_sub < 2, "hawq_conv2d_splitk: out_sub is not supported");
    HAWQ_REQUIRE(hawq_res_sub(*a) < 2, "hawq_conv2d_splitk: res_sub is not supported");
    const int epi = a->epilogue;
    HAWQ_REQUIRE(epi == HAWQ_EPI_RAW || epi == HAWQ_EPI_REQUANT || epi == HAWQ_EPI_RESIDUAL, "hawq_conv2d_splitk: RAW, REQUANT or RESIDUAL epilogue only");
    HAWQ_REQUIRE(epi == HAWQ_EPI_RAW || !a->out_q || a->out_bits == 8, "hawq_conv2d_splitk: out_bits must be 8");
    HAWQ_REQUIRE(epi != HAWQ_EPI_REQUANT || a->out_q, "hawq_conv2d_splitk: REQUANT needs out_q");
    HAWQ_REQUIRE((a->in_planar | a->out_planar | 1) == 1, "hawq_conv2d_splitk: in_planar / out_planar must be 0 or 1");
    const ConvForm f = conv_form(a);
    const bool dual = f.dual, res = epi == HAWQ_EPI_RESIDUAL, fast_epi = splitk_fast_epi(f);
    HAWQ_REQUIRE(!a->in_planar || (!dual && fast_epi), "hawq_conv2d_splitk: in_planar needs a single-branch fast-contract REQUANT / RESIDUAL launch");
    HAWQ_REQUIRE(!a->out_planar || (fast_epi && a->out_q), "hawq_conv2d_splitk: out_planar needs the fast-contract REQUANT / RESIDUAL epilogue");
    sp.Ho = (a->H + 2 * a->pad - a->KH) / a->stride + 1;
    sp.Wo = (a->W + 2 * a->pad - a->KW) / a->stride + 1;
    const long long M = (long long)a->N * sp.Ho * sp.Wo;
    HAWQ_REQUIRE(sp.Ho > 0 && sp.Wo > 0 && M < (1ll << 30) && M * (long long)a->Cout < (1ll << 40), "hawq_conv2d_splitk: bad output size");
    sp.M = (int)M;
    const int nk1 = a->KH * a->KW * (a->Cin >> 6);
    HAWQ_REQUIRE(nk1 % slices == 0, "hawq_conv2d_splitk: %d slices do not divide the %d K chunks", slices, nk1);
    sp.s1 = slices, sp.q1 = nk1 / slices, sp.ns1 = nk1, sp.s2 = 0, sp.q2 = 1;
    if (dual) {
        HAWQ_REQUIRE(res, "hawq_conv2d_splitk: a second branch needs HAWQ_EPI_RESIDUAL");
        HAWQ_REQUIRE(a->in2_bits == 8 && a->w2_bits == 8, "hawq_conv2d_splitk: int8 operands only in the second branch");
        HAWQ_REQUIRE(a->Cin2 > 0 && a->Cin2 % 64 == 0 && a->stride2 > 0 && a->H2 > 0 && a->W2 > 0, "hawq_conv2d_splitk: bad second branch");
        HAWQ_REQUIRE((a->H2 - 1) / a->stride2 + 1 == sp.Ho && (a->W2 - 1) / a->stride2 + 1 == sp.Wo, "hawq_conv2d_splitk: second branch output grid differs");
        const int nk2 = a->Cin2 >> 6;
        int q2 = sp.q1 < nk2 ? sp.q1 : nk2;
        while (nk2 % q2) --q2;
        sp.q2 = q2, sp.s2 = nk2 / q2;
    }
    sp.tiles_c = a->Cout / SK::BN;
    sp.ntiles = ((sp.M + SK::BM - 1) / SK::BM) * sp.tiles_c;
    HAWQ_REQUIRE((long long)sp.ntiles * (sp.s1 + sp.s2) < (1ll << 31), "hawq_conv2d_splitk: grid too large");
    sp.slab_bytes = (long long)sp.ntiles * (sp.s1 + sp.s2) * SK_TILE * 4;
    sp.counter_bytes = (long long)sp.ntiles * 4;
    return 0;
}

#define SK_FN(E, D, F, T, P) conv_splitk_kernel<E, D, F, T, P>
SplitFn pick_kernel(int epi, bool dual, bool fast, bool tie, bool planar) {
    if (epi == HAWQ_EPI_RAW) return SK_FN(HAWQ_EPI_RAW, false, false, false, false);
    if (dual) {
        if (!fast) return SK_FN(HAWQ_EPI_RESIDUAL, true, false, false, false);
        return tie ? SK_FN(HAWQ_EPI_RESIDUAL, true, true, true, false) : SK_FN(HAWQ_EPI_RESIDUAL, true, true, false, false);
    }
    if (epi == HAWQ_EPI_REQUANT) {
        if (!fast) return SK_FN(HAWQ_EPI_REQUANT, false, false, false, false);
        if (planar) return tie ? SK_FN(HAWQ_EPI_REQUANT, false, true, true, true) : SK_FN(HAWQ_EPI_REQUANT, false, true, false, true);
        return tie ? SK_FN(HAWQ_EPI_REQUANT, false, true, true, false) : SK_FN(HAWQ_EPI_REQUANT, false, true, false, false);
    }
    if (!fast) return SK_FN(HAWQ_EPI_RESIDUAL, false, false, false, false);
    if (planar) return tie ? SK_FN(HAWQ_EPI_RESIDUAL, false, true, true, true) : SK_FN(HAWQ_EPI_RESIDUAL, false, true, false, true);
    return tie ? SK_FN(HAWQ_EPI_RESIDUAL, false, true, true, false) : SK_FN(HAWQ_EPI_RESIDUAL, false, true, false, false);
}

}  // namespace

extern "C" int hawq_conv2d_splitk_ok(const hawq_conv_args *a, int32_t slices) {
    SplitPlan sp;
    return splitk_plan(a, slices, sp) == 0 ? 1 : 0;
}

extern "C" int hawq_conv2d_splitk_workspace(const hawq_conv_args *a, int32_t slices, int64_t *slab_bytes, int64_t *counter_bytes) {
    SplitPlan sp;
    const int rc = splitk_plan(a, slices, sp);
    if (rc) return rc;
    if (slab_bytes) *slab_bytes = sp.slab_bytes;
    if (counter_bytes) *counter_bytes = sp.counter_bytes;
    return 0;
}

extern "C" int hawq_conv2d_splitk(const hawq_conv_args *a, int32_t slices, void *slab, int32_t *counters, void *stream) {
    SplitPlan sp;
    const int rc = splitk_plan(a, slices, sp);
    if (rc) return rc;
    HAWQ_REQUIRE(slab && counters, "hawq_conv2d_splitk: slab and counters must be non-null");
    ConvForm f;
    ConvP p;
    if (const int rc = conv_check(a, "hawq_conv2d_splitk", &f, &p)) return rc;   // hawq_conv2d's argument rules and table preparation
    p.ring_bytes = SK::LDS_BYTES;
    p.dbg = 0;
    const SplitFn fn = pick_kernel(a->epilogue, f.dual, splitk_fast_epi(f), p.k0 == 2, a->in_planar != 0);
    SplitP s;
    s.slab = (int32_t *)slab, s.counters = counters;
    s.tiles_c = sp.tiles_c, s.ntiles = sp.ntiles, s.s1 = sp.s1, s.s2 = sp.s2, s.q1 = sp.q1, s.q2 = sp.q2, s.ns1 = sp.ns1;
    hipLaunchKernelGGL(fn, dim3(sp.ntiles * (sp.s1 + sp.s2)), dim3(SK::NT), SK_LDS, (hipStream_t)stream, p, s);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
