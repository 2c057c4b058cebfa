// LDS-tiled variants of the InceptionV3 rectangular conv (inception.hip: hawq_incep_conv), same argument block, same arithmetic:
//   hawq_incep_conv_num_tiles   T: tile ids 1 .. T are the kernels below, id 0 is hawq_incep_conv's kernel
//   hawq_incep_conv_tile_ok     host arithmetic only: does that tile take this launch
//   hawq_incep_conv_tiled       the launch
// The sums are integers, so every tile computes exactly what tile 0 computes; the epilogue is tile 0's, statement for statement.
//
// K is the window taps times Cin, walked in units of 16 channels ("k16" = one 16-byte run of a weight row / of an input pixel): weight
// rows [KH][KW][Cin] are contiguous in that order, so k16 unit u of a row is at byte 16 u, and for the activations u = tap * Cin/16 + c16
// names the tap (kh, kw) and the channel run.  A K step is four units = 64 bytes per row: one tap x 64 channels when Cin % 64 == 0, and
// parts of neighbouring taps otherwise (Cin = 32: two taps per step; Cin = 48, 80: runs of both) - no MFMA column is spent on padding
// except in the last step of a K that is not a multiple of 64.  Units beyond K and taps outside the image are zeros.
//
// Per step a workgroup stages BM pixel rows and BN weight rows of 64 bytes into one of two LDS stages: thread t owns unit (t & 3) of
// rows (t >> 2) + i * NT/4, loads 16 bytes per row to registers while the MFMAs of the previous step run, and writes them with
// ds_write_b128 afterwards (one barrier per step).  Register staging, not LDS-DMA: a tap that falls into the padding must become
// zeros, and the DMA can only copy.  Rows are 64 bytes with the 16-byte slot XOR-swizzled by (row >> 2) & 3 (common.h lds_off): the
// ds_read_b128 fragment reads of 32 consecutive rows are conflict-free in each of the instruction's four 16-lane groups.
// Weight rows are staged in cperm order (LDS row q of a 32-row group holds channel cperm(q)), so lane half h ends up with the 16
// consecutive channels 16 h .. 16 h + 15 of one pixel, as in tile 0 - and stores them as whole 16-byte runs.
//
// That workgroup body is incep_tile_body.h, shared as text with the grouped launches (incep_group.hip, incep_fan.hip); the tile table
// and the dispatch over it are incep_tile.h's.
#include "incep_tile.h"

extern "C" int hawq_incep_conv(const hawq_incep_conv_args *a, void *stream);

namespace {

// the body on the workgroup's block of a 2-D grid: pixel blocks in x, channel blocks in y
template <int BM, int BN, int WPX, int WCH, int KS>
__global__ __launch_bounds__(64 * WPX * WCH * KS) void incep_tiled_kernel(hawq_incep_conv_args a, int Ho, int Wo) {
    __shared__ __attribute__((aligned(16))) char lds[2 * (BM + BN) * 64];
#define INCEP_TILE_BLOCK                                 \
    const long long pblock = (long long)blockIdx.x * BM; \
    const int cblock = blockIdx.y * BN;
#define INCEP_TILE_STORED(p, cb, q)
#include "incep_tile_body.h"
#undef INCEP_TILE_BLOCK
#undef INCEP_TILE_STORED
}

struct Geo {
    int Ho, Wo;
    long long P;
};

// hawq_incep_conv's own argument checks, as a reason (NULL: the launch is well formed).  No pointer is dereferenced.
const char *refusal(const hawq_incep_conv_args *a, Geo *g) {
    if (!a || !a->in || !a->wgt || !a->bias || !a->out) return "null pointer";
    if (!(a->N > 0 && a->H > 0 && a->W > 0 && a->Cin > 0 && a->Cout > 0 && a->Cin % 16 == 0 && a->Cout % 16 == 0))
        return "bad shape (channels must be multiples of 16)";
    if (!(a->KH >= 1 && a->KH <= 7 && a->KW >= 1 && a->KW <= 7 && (a->stride == 1 || a->stride == 2))) return "window or stride not supported";
    if (!(a->pad_h >= 0 && a->pad_w >= 0 && 2 * a->pad_h < a->KH + 1 && 2 * a->pad_w < a->KW + 1)) return "padding too large for the window";
    g->Ho = (a->H + 2 * a->pad_h - a->KH) / a->stride + 1, g->Wo = (a->W + 2 * a->pad_w - a->KW) / a->stride + 1;
    if (!(g->Ho > 0 && g->Wo > 0)) return "empty output";
    if (!(a->c_off >= 0 && a->ldo >= a->c_off + a->Cout)) return "ldo < c_off + Cout";
    if (a->epilogue == HAWQ_INCEP_REQUANT || a->epilogue == HAWQ_INCEP_REQUANT2) {
        if (!a->m || !a->ek) return "requant tables missing";
        if (a->out_bits != 8 && a->out_bits != 16) return "out_bits must be 8 or 16";
        const int lim = a->out_bits == 16 ? 32767 : 127;
        if (!(a->q_lo >= -lim - 1 && a->q_hi <= lim && a->q_lo <= a->q_hi &&
              (a->epilogue != HAWQ_INCEP_REQUANT2 || (a->q2_lo >= -lim - 1 && a->q2_hi <= lim && a->q2_lo <= a->q2_hi))))
            return "clamp bounds outside the store";
    } else if (a->epilogue != HAWQ_INCEP_RAW) {
        return "unknown epilogue";
    }
    g->P = (long long)a->N * g->Ho * g->Wo;
    if ((g->P + 63) / 64 >= (1ll << 31)) return "too many output pixels";
    return nullptr;
}

// why tile `tile` (1 .. NUM_TILES) does not take a well-formed launch (NULL: it does)
const char *tile_refusal(const hawq_incep_conv_args *a, int tile) {
    if (a->ldo % 16 || a->c_off % 16 || ((uintptr_t)a->out & 15) || ((uintptr_t)a->in & 15) || ((uintptr_t)a->wgt & 15))
        return "the tiled kernels store 16-byte runs: out, in, wgt 16-byte aligned, ldo and c_off multiples of 16";
    if (tile == 1 && a->Cout <= 64) return "the 128-channel tile is for more than 64 output channels";
    if (tile == 4 && a->KH * a->KW * a->Cin < 512) return "the K-split tile is for K >= 512";
    return nullptr;
}

template <class T>
void launch(const hawq_incep_conv_args *a, const Geo &g, hipStream_t stream) {
    dim3 grid((unsigned)((g.P + T::BM - 1) / T::BM), (unsigned)((a->Cout + T::BN - 1) / T::BN));
    hipLaunchKernelGGL((incep_tiled_kernel<T::BM, T::BN, T::WPX, T::WCH, T::KS>), grid, dim3(T::NT), 0, stream, *a, g.Ho, g.Wo);
}

}  // namespace

extern "C" int hawq_incep_conv_num_tiles(void) { return NUM_TILES; }

extern "C" int hawq_incep_conv_tile_ok(const hawq_incep_conv_args *a, int tile) {
    Geo g;
    if (tile < 0 || tile > NUM_TILES || refusal(a, &g)) return 0;
    return tile == 0 || !tile_refusal(a, tile);
}

extern "C" int hawq_incep_conv_tiled(const hawq_incep_conv_args *a, int tile, void *stream) {
    if (tile == 0) return hawq_incep_conv(a, stream);
    HAWQ_REQUIRE(tile > 0 && tile <= NUM_TILES, "hawq_incep_conv_tiled: no tile %d (ids 0 .. %d)", tile, NUM_TILES);
    Geo g;
    const char *why = refusal(a, &g);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_tiled: %s", why);
    why = tile_refusal(a, tile);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_tiled: tile %d (%d px x %d ch) refuses the launch: %s", tile, kTiles[tile].bm, kTiles[tile].bn, why);
    for_tile(tile, [&](auto t) { launch<decltype(t)>(a, g, (hipStream_t)stream); });
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
