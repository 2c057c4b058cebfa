// The general tiles of hawq_conv2d (family 0 of conv_dispatch.hip): conv_kernel of conv_device.h instantiated per tile
// configuration, epilogue and operand-width variant; they take any layer.
#include "conv_dispatch.h"

namespace {

using T0 = Cfg<128, 128, 2, 2, 3>;
using T1 = Cfg<256, 64, 4, 1, 3>;
using T2 = Cfg<64, 64, 2, 2, 4>;
using T3 = Cfg<128, 64, 2, 2, 4>;
// two sub-chunks (K = 128) per ring stage and barrier for the long-K / few-workgroup layers (stages 3-4);
// need an even chunk count, otherwise the launcher falls back to the single-sub-chunk twin
using T4 = Cfg<128, 128, 2, 2, 3, 2>;  // K = 128 per barrier
using T5 = Cfg<64, 64, 2, 2, 4, 2>;
using T6 = Cfg<128, 64, 2, 2, 3, 2>;
// 8-wave workgroups: twice the waves issuing LDS-DMA for the same tile (the DMA rate per wave, not the ring
// depth, bounds the long-K layers when there is at most ~1 workgroup per CU - profiles/r01_ubench_dma_rate.txt)
using T7 = Cfg<128, 128, 2, 4, 3>;
using T8 = Cfg<128, 128, 2, 4, 3, 2>;
using T9 = Cfg<256, 128, 4, 2, 3>;
// shallow rings for the short-K, epilogue-heavy layers (1x1 expand + residual): less LDS per workgroup = more
// workgroups per CU (4 / 5 instead of 3), whose load, epilogue-VALU and store phases then overlap
using T10 = Cfg<64, 64, 2, 2, 3, 1, 6>;
using T11 = Cfg<64, 64, 2, 2, 2, 1, 6>;
using T12 = Cfg<128, 64, 2, 2, 2, 1, 3>;
using T13 = Cfg<128, 128, 2, 4, 2, 1, 2>;
// intra-workgroup split-K (KG groups of waves on alternating 64-channel sub-chunks) for the long-K, few-pixel layers
using T14 = Cfg<64, 64, 2, 2, 3, 2, 4, 2>;     // 8 waves: 2 groups x (2 x 2 waves of 32 x 32), 48 KiB
// (measured, not kept: 16 waves in 4 K groups, and 5-6-stage rings for the same layers - 96-120 KiB of LDS leave one workgroup
// per CU, and these launches live on the overlap BETWEEN workgroups: 15-60 % slower.  Split-K itself ties with the best
// plain tile; it stays as an autotuner choice.)
constexpr int NUM_TILES = 15;

typedef void (*KernelFn)(const ConvP);
// single-branch kernels: epilogue {RAW, REQUANT, RESIDUAL, DEQUANT} x bit variant {run-time, 8/8, 4/4};
// dual-branch (RESIDUAL + identity conv): {run-time, 88/88, 44/44, 88/44, 44/88}
struct TileInfo {
    int BM, BN, lds, ksub, twin, nt, ns, kg;  // twin: tile id to fall back to when KSUB does not divide the chunk count / the layer is not on the asynchronous pipeline
    KernelFn single[4][3];
    KernelFn dual[5];
    KernelFn tie_single[2][2];  // exact-tie instantiations: {REQUANT, RESIDUAL} x {8/8, 4/4}
    KernelFn tie_dual[2];       // {88/88, 44/44}
};
#define SINGLE_ROW(T, E) \
    { conv_kernel<T, E, false, 0, 0>, conv_kernel<T, E, false, 0x88, 0>, conv_kernel<T, E, false, 0x44, 0> }
#define TILE_ENTRY(T, TWIN)                                                                                          \
    {                                                                                                          \
        T::BM, T::BN, T::LDS_BYTES, T::KSUB, TWIN, T::NT, T::NS, T::KG,                                                   \
            {SINGLE_ROW(T, HAWQ_EPI_RAW), SINGLE_ROW(T, HAWQ_EPI_REQUANT), SINGLE_ROW(T, HAWQ_EPI_RESIDUAL),   \
             SINGLE_ROW(T, HAWQ_EPI_DEQUANT)},                                                                 \
        {                                                                                                      \
            conv_kernel<T, HAWQ_EPI_RESIDUAL, true, 0, 0>, conv_kernel<T, HAWQ_EPI_RESIDUAL, true, 0x88, 0x88>, \
                conv_kernel<T, HAWQ_EPI_RESIDUAL, true, 0x44, 0x44>,                                           \
                conv_kernel<T, HAWQ_EPI_RESIDUAL, true, 0x88, 0x44>,                                           \
                conv_kernel<T, HAWQ_EPI_RESIDUAL, true, 0x44, 0x88>                                            \
        },                                                                                                     \
        {{conv_kernel<T, HAWQ_EPI_REQUANT, false, 0x88, 0, true>, conv_kernel<T, HAWQ_EPI_REQUANT, false, 0x44, 0, true>},   \
         {conv_kernel<T, HAWQ_EPI_RESIDUAL, false, 0x88, 0, true>, conv_kernel<T, HAWQ_EPI_RESIDUAL, false, 0x44, 0, true>}}, \
        {conv_kernel<T, HAWQ_EPI_RESIDUAL, true, 0x88, 0x88, true>, conv_kernel<T, HAWQ_EPI_RESIDUAL, true, 0x44, 0x44, true>} \
    }
const TileInfo kTiles[NUM_TILES] = {TILE_ENTRY(T0, 0), TILE_ENTRY(T1, 1), TILE_ENTRY(T2, 2), TILE_ENTRY(T3, 3),
                                    TILE_ENTRY(T4, 0), TILE_ENTRY(T5, 2), TILE_ENTRY(T6, 3),
                                    TILE_ENTRY(T7, 7), TILE_ENTRY(T8, 7), TILE_ENTRY(T9, 9),
                                    TILE_ENTRY(T10, 10), TILE_ENTRY(T11, 11), TILE_ENTRY(T12, 12), TILE_ENTRY(T13, 13),
                                    TILE_ENTRY(T14, 2)};

// kernels whose staged epilogue needs more than the default 64 KiB of dynamic LDS
bool raise_lds_limits() {
    bool ok = true;
    for (const TileInfo &ti : kTiles) {
        const int lds = ti.lds + ti.BM * ti.BN * 2 + ti.BN * 32;
        if (lds <= 64 * 1024) continue;
        for (int v = 0; v < 2; ++v)
            ok &= hipFuncSetAttribute((const void *)ti.tie_single[1][v], hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess &&
                  hipFuncSetAttribute((const void *)ti.tie_dual[v], hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
        for (int v = 1; v < 3; ++v)
            ok &= hipFuncSetAttribute((const void *)ti.single[2][v], hipFuncAttributeMaxDynamicSharedMemorySize, lds) ==
                  hipSuccess;
        for (int v = 1; v < 5; ++v)
            ok &= hipFuncSetAttribute((const void *)ti.dual[v], hipFuncAttributeMaxDynamicSharedMemorySize, lds) ==
                  hipSuccess;
    }
    return ok;
}

enum { TAB_SINGLE, TAB_DUAL, TAB_TIE_SINGLE, TAB_TIE_DUAL };   // ConvChoice.table
KernelFn tile_fn(const TileInfo &ti, const ConvChoice &c) {
    switch (c.table) {
        case TAB_SINGLE: return ti.single[c.fn[0]][c.fn[1]];
        case TAB_DUAL: return ti.dual[c.fn[0]];
        case TAB_TIE_SINGLE: return ti.tie_single[c.fn[0]][c.fn[1]];
        default: return ti.tie_dual[c.fn[0]];
    }
}

}  // namespace

int conv_igemm_count(void) { return NUM_TILES; }
bool conv_igemm_applies(const hawq_conv_args *a, int) { return !a->in_planar; }

int conv_igemm_pick_tile(int M, int Cout, bool dual) {
    // Enough workgroups to fill 256 CUs a few times over, the largest tile that allows it.
    auto nwg = [&](int t) { return ((M + kTiles[t].BM - 1) / kTiles[t].BM) * (Cout / kTiles[t].BN); };
    // two accumulator sets: only the 32-channel-per-wave tiles stay within 256 VGPRs without spilling
    if (dual) return nwg(3) >= 512 ? 3 : 2;
    if (Cout % 128 == 0 && nwg(0) >= 1024) return 0;
    if (nwg(1) >= 1024 && !dual) return 1;
    if (Cout % 128 == 0 && nwg(0) >= 512) return 0;
    if (nwg(3) >= 512) return 3;
    return 2;
}

// c.tile comes in as the tile asked for (or picked) and leaves as the tile that runs: Cout % BN fallback, then the twin rules
int conv_igemm_choose(const hawq_conv_args *a, const ConvForm &f, const ConvP &p, ConvChoice &c) {
    const int nk1 = a->KH * a->KW * (a->Cin >> 6), nk2 = f.dual ? (a->Cin2 >> 6) : 0;   // 64-channel K chunks of the two branches
    // 32-bit residual tensors, the signed forms and the general path use the generic (run-time bit-width, direct epilogue) kernels
    const bool direct = f.wide_res || f.signed_res || (f.needs_tables && !f.fast);
    int tile = c.tile;
    if (p.Cout % kTiles[tile].BN != 0) tile = 2;
    if (kTiles[tile].ksub > 1) {  // K = 128 (or more) per barrier: async pipeline with chunk counts the stage divides
        // (4/4 layers check the divisibility of their 128-channel chunk count inside the kernel and otherwise
        //  run the register-staged loop, which works for any tile without split-K)
        if (f.all88 && ((nk1 % kTiles[tile].ksub) || (nk2 % kTiles[tile].ksub))) tile = kTiles[tile].twin;
        if (kTiles[tile].kg > 1) {   // split-K tiles exist on the asynchronous pipelines only
            const int ks = kTiles[tile].ksub;
            const bool nib_ok = f.all44 && (a->Cin & 127) == 0 && (!f.dual || (a->Cin2 & 127) == 0) &&
                                ((a->KH * a->KW * (a->Cin >> 7)) % ks) == 0 && (!f.dual || ((a->Cin2 >> 7) % ks) == 0);
            if (!(f.all88 || nib_ok) || direct) tile = kTiles[tile].twin;
        }
    }
    const TileInfo &ti = kTiles[tile];
    c.tile = tile;
    c.grid = ((p.M + ti.BM - 1) / ti.BM) * (p.Cout / ti.BN), c.block = ti.nt, c.lds = ti.lds;
    {   // a K loop shorter than the ring needs fewer stages: less LDS = more resident workgroups (the K = 64 expand
        // convs of stage 1 run a single stage).  Only the all-int8 asynchronous pipeline; the register-staged
        // and 4-bit paths keep the full ring.
        const int stages = (nk1 + nk2) / ti.ksub, stage_bytes = ti.lds / ti.ns;
        static const bool full_ring = getenv("HAWQ_FULL_RING") != nullptr;  // A/B switch for measurements
        if (!full_ring && f.all88 && f.needs_tables && !direct && stages >= 1 && stages < ti.ns &&
            stages * stage_bytes >= ti.BM * ti.BN * (ti.kg > 1 ? 4 : 1))  // (the int8 output tile - split-K: the partial sums - is staged on top of the ring)
            c.lds = stages * stage_bytes;
    }
    c.ring_bytes = c.lds;
    auto variant = [&](int ab, int wb) { return direct ? 0 : (ab == 8 && wb == 8 ? 1 : (ab == 4 && wb == 4 ? 2 : 0)); };
    const int v1 = variant(p.in_bits, p.w_bits);
    if (f.dual) {
        const int v2 = variant(p.in2_bits, p.w2_bits);
        c.table = TAB_DUAL, c.fn[0] = (v1 == 0 || v2 == 0) ? 0 : (v1 == v2 ? v1 : (v1 == 1 ? 3 : 4));
        if (p.k0 == 2 && v1 != 0 && v2 != 0) {
            HAWQ_REQUIRE(v1 == v2, "hawq_conv2d: exact-tie mode (fast_tables bit 2) needs equal operand widths in both branches");
            c.table = TAB_TIE_DUAL, c.fn[0] = v1 - 1;
        }
        if (v1 != 0 && v2 != 0) c.lds += ti.BM * ti.BN * 2 + ti.BN * 32;
    } else {
        c.table = TAB_SINGLE, c.fn[0] = f.slot, c.fn[1] = v1;
        if (p.k0 == 2 && v1 != 0 && f.needs_tables) c.table = TAB_TIE_SINGLE, c.fn[0] = f.slot - 1, c.fn[1] = v1 - 1;
        if (v1 != 0 && f.slot == 2) c.lds += ti.BM * ti.BN * 2;
        if (v1 != 0 && f.needs_tables) c.lds += ti.BN * 16;
    }
    return 0;
}

int conv_igemm_launch(const hawq_conv_args *a, const ConvChoice &c, const ConvP &args, void *stream) {
    const TileInfo &ti = kTiles[c.tile];
    ConvP p = args;
    p.dbgbuf = conv_dbg_buffer(p.dbg);
    static const bool attrs_ok = raise_lds_limits();  // once per process; never inside a capture
    HAWQ_REQUIRE(attrs_ok, "hawq_conv2d: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    hipLaunchKernelGGL(tile_fn(ti, c), dim3(c.grid), dim3(c.block), c.lds, (hipStream_t)stream, p);
    HAWQ_CHECK_HIP(hipGetLastError());
    if (HAWQ_DBG_BIT(p.dbg, 128) && p.dbgbuf) {  // experiment hook: per-phase cycles of one wave (synchronises!)
        long long hbuf[4];
        (void)hipStreamSynchronize((hipStream_t)stream);
        (void)hipMemcpy(hbuf, p.dbgbuf, sizeof(hbuf), hipMemcpyDeviceToHost);
        fprintf(stderr, "[conv tile %d (%dx%d, %d thr) M=%d K=%dx%dx%d(+%d) Cout=%d epi=%d] grid %d lds %d: prologue %lld | K loop %lld | epilogue %lld cycles\n",
                c.tile + 1, ti.BM, ti.BN, ti.nt, p.M, a->KH, a->KW, a->Cin, a->in2 ? a->Cin2 : 0, p.Cout, a->epilogue, c.grid, c.lds,
                hbuf[0], hbuf[1], hbuf[2]);
    }
    return 0;
}
