// Nibble-packed InceptionV3 conv: the launches of hawq_incep_conv (inception.hip) on hawq4 operands, same argument block, same integers.
//   hawq_incep_conv_nib_num_tiles   T: tile ids 1 .. T are the kernels below (there is no id 0)
//   hawq_incep_conv_nib_ok          host arithmetic only: does that tile take this launch
//   hawq_incep_conv_nib             the launch
// in:  unsigned 4-bit activations, hawq4 NHWC rows (Cin / 2 bytes per pixel);  wgt: signed 4-bit, hawq4 [Cout][KH][KW][Cin].
// hawq4 (include/hawq_mi355.h): byte k of an 8-channel dword = c_k | c_{k+4} << 4, so `d & 0x0f0f0f0f` is channels 0 - 3 as int8x4 and
// `(d >> 4) & 0x0f0f0f0f` channels 4 - 7.
//
// Both operands stay packed from HBM through LDS into the fragment registers and become int8x4 MFMA operands only there.
//
// K is the window taps times Cin, walked in units of 16 channels = 8 bytes (two dwords): unit u = tap * Cin/16 + c16 of a pixel, and
// byte 8 u of a weight row.  An LDS row is 64 bytes = 8 units = 128 K values, and that is the K step: the stage of a tile has the
// bytes it has in the int8 kernels ((BM + BN) * 64, two stages, at most 32 KiB), but each barrier now closes four MFMA K blocks per
// fragment pair instead of two.  A thread stages unit (t & 7) of rows (t >> 3) + i * NT/8 with 8-byte loads into registers while the
// previous step's MFMAs run and writes them with ds_write_b64 afterwards; the unit, not the 16-byte slot, is what it owns, because
// with an odd Cin/16 (16, 48, 80 ...) the two units of a slot lie in different taps - one of them may be padding - and a unit is
// the largest run that is always one tap.  Units beyond K (an odd unit count: the last MFMA is half empty) and taps outside the
// image are staged as zero bytes, which widen to exact zeros on both sides.
//
// Fragment reads are ds_read_b128: lane (l31, h) reads the 16-byte slot 2 t + h of row l31 (t = 0, 1), that is units 4 t + 2 h and
// 4 t + 2 h + 1, and issues two MFMAs from it - the first on the even unit of every lane, the second on the odd one.  An MFMA K block
// is therefore units {4 t, 4 t + 2} and then {4 t + 1, 4 t + 3}: K is summed, both operands use the same lane map, so the order of K
// inside a step is free, and a 16-byte read per lane keeps the bank pattern of 64-byte rows with the slot XOR-swizzled by
// (row >> 2) & 3 (common.h lds_off) conflict-free, as in the int8 kernels; an 8-byte read per MFMA would take twice the LDS
// instructions.  The staging writes of 8 lanes fill one 64-byte row, 32 lanes four rows = all 64 banks once.
//
// Widening (VALU per dword: 3 on either side).  Activations zero-extend: d & M, (d >> 4) & M.  Weights are fed as nibble << 4, the
// int8 value 16 w with the nibble's sign bit as the byte's: (d << 4) & ~M, d & ~M.  The accumulator is then exactly 16 times the
// int8-container sum and is shifted right by 4 in front of the bias.  16 * 15 * 8 * K < 2^31 is proved on the host from the shape
// alone (hawq_incep_conv_nib_ok: K = KH KW Cin <= 1118481; |w| <= 8, a <= 15), so no layer needs its weights read.  A true sign
// extension costs two more instructions per dword (xor 8, subtract 8 per byte).  A fragment is widened once per unit and used by
// every MFMA of its row or column of the wave tile: 12 (WM + WN) instructions per 2 WM WN MFMAs, 6 per MFMA on a 64 x 64 wave tile
// and 9 on a 64 x 32 one, against the 16 passes of a 32x32x32 MFMA.
//
// Weight rows are staged in cperm order (LDS row q of a 32-row group holds channel cperm(q)), so lane half h ends up with the 16
// consecutive channels 16 h .. 16 h + 15 of one pixel - one 8-byte store of hawq4, 16 bytes of int8, 32 of int16, 64 of int32.
#include "incep_nib.h"

namespace {

// tile ids 1 .. NUM_NIB_TILES: BM pixels x BN channels per workgroup, 256 threads each
//   1  128 px x 128 ch, 4 waves of 64 x 64                    the 147^2 .. 35^2 maps with 96 and more output channels
//   2  128 px x  64 ch, 4 waves of 64 x 32                    32 .. 64 output channels, and the 17^2 maps (289 px = 2.3 tiles an image)
//   3   64 px x  64 ch, 2 x 2 waves of 32 x 64 that split K   the 8^2 maps (one image = one pixel tile) at batch 1 - 16
enum { NUM_NIB_TILES = 3 };
struct NibShape {
    int bm, bn;
};
constexpr NibShape kNib[NUM_NIB_TILES + 1] = {{0, 0}, {128, 128}, {128, 64}, {64, 64}};
// 16 (weights as nibble << 4) * 15 * 8 * K <= 2^31 - 1
constexpr long long NIB_K_MAX = ((1ll << 31) - 1) / (16 * 15 * 8);

// the body (incep_nib_body.h, shared as text with incep_group_nib.hip) on the workgroup's block of a 2-D grid: pixel blocks in x,
// channel blocks in y
template <int BM, int BN, int WPX, int WCH, int KS>
__global__ __launch_bounds__(64 * WPX * WCH * KS) void incep_nib_kernel(hawq_incep_conv_args a, int Ho, int Wo) {
    __shared__ __attribute__((aligned(16))) char lds[2 * (BM + BN) * 64];
#define INCEP_NIB_BLOCK                                  \
    const long long pblock = (long long)blockIdx.x * BM; \
    const int cblock = blockIdx.y * BN;
#define INCEP_NIB_STORED(p, cb, q)
#include "incep_nib_body.h"
#undef INCEP_NIB_BLOCK
#undef INCEP_NIB_STORED
}

struct Geo {
    int Ho, Wo;
    long long P;
};

// why no nibble tile takes this block (NULL: it is well formed).  No pointer is dereferenced.
const char *refusal(const hawq_incep_conv_args *a, Geo *g) {
    if (!a || !a->in || !a->wgt || !a->bias || !a->out) return "null pointer";
    if (!(a->N > 0 && a->H > 0 && a->W > 0 && a->Cin > 0 && a->Cout > 0 && a->Cin % 16 == 0 && a->Cout % 16 == 0))
        return "bad shape (channels must be multiples of 16)";
    if (!(a->KH >= 1 && a->KH <= 7 && a->KW >= 1 && a->KW <= 7 && (a->stride == 1 || a->stride == 2))) return "window or stride not supported";
    if (!(a->pad_h >= 0 && a->pad_w >= 0 && 2 * a->pad_h < a->KH + 1 && 2 * a->pad_w < a->KW + 1)) return "padding too large for the window";
    g->Ho = (a->H + 2 * a->pad_h - a->KH) / a->stride + 1, g->Wo = (a->W + 2 * a->pad_w - a->KW) / a->stride + 1;
    if (!(g->Ho > 0 && g->Wo > 0)) return "empty output";
    if (!(a->c_off >= 0 && a->ldo >= a->c_off + a->Cout)) return "ldo < c_off + Cout";
    if ((long long)a->KH * a->KW * a->Cin > NIB_K_MAX) return "K too long: 16 * 15 * 8 * KH KW Cin must fit int32 (weights are fed as 16 w)";
    if (a->epilogue == HAWQ_INCEP_REQUANT || a->epilogue == HAWQ_INCEP_REQUANT2) {
        if (!a->m || !a->ek) return "requant tables missing";
        if (a->out_bits != 4 && a->out_bits != 8 && a->out_bits != 16) return "out_bits must be 4, 8 or 16";
        const int lo = a->out_bits == 4 ? 0 : a->out_bits == 8 ? -128 : -32768, hi = a->out_bits == 4 ? 15 : a->out_bits == 8 ? 127 : 32767;
        if (!(a->q_lo >= lo && a->q_hi <= hi && a->q_lo <= a->q_hi &&
              (a->epilogue != HAWQ_INCEP_REQUANT2 || (a->q2_lo >= lo && a->q2_hi <= hi && a->q2_lo <= a->q2_hi))))
            return "clamp bounds outside the store (out_bits 4 holds 0 .. 15)";
    } else if (a->epilogue != HAWQ_INCEP_RAW) {
        return "unknown epilogue";
    } else if (a->out_bits == 4) {
        return "a RAW epilogue stores int32: out_bits 4 needs REQUANT or REQUANT2";
    }
    if (a->ldo % 16 || a->c_off % 16 || ((uintptr_t)a->out & 15) || ((uintptr_t)a->in & 15) || ((uintptr_t)a->wgt & 15))
        return "out, in, wgt must be 16-byte aligned, ldo and c_off multiples of 16";
    g->P = (long long)a->N * g->Ho * g->Wo;
    if ((g->P + 63) / 64 >= (1ll << 31) || a->Cout / 64 > 65534) return "too many output pixels or channels for the grid";
    return nullptr;
}

// why tile `tile` (1 .. NUM_NIB_TILES) does not take a well-formed launch (NULL: it does)
const char *tile_refusal(const hawq_incep_conv_args *a, int tile) {
    if (tile == 1 && a->Cout <= 64) return "the 128-channel tile is for more than 64 output channels";
    if (tile == 3 && a->KH * a->KW * a->Cin < 512) return "the K-split tile is for K >= 512";
    return nullptr;
}

template <int BM, int BN, int WPX, int WCH, int KS>
void launch(const hawq_incep_conv_args *a, const Geo &g, hipStream_t stream) {
    dim3 grid((unsigned)((g.P + BM - 1) / BM), (unsigned)((a->Cout + BN - 1) / BN));
    hipLaunchKernelGGL((incep_nib_kernel<BM, BN, WPX, WCH, KS>), grid, dim3(64 * WPX * WCH * KS), 0, stream, *a, g.Ho, g.Wo);
}

}  // namespace

extern "C" int hawq_incep_conv_nib_num_tiles(void) { return NUM_NIB_TILES; }

extern "C" int hawq_incep_conv_nib_ok(const hawq_incep_conv_args *a, int tile) {
    Geo g;
    return tile >= 1 && tile <= NUM_NIB_TILES && !refusal(a, &g) && !tile_refusal(a, tile);
}

extern "C" int hawq_incep_conv_nib(const hawq_incep_conv_args *a, int tile, void *stream) {
    HAWQ_REQUIRE(tile >= 1 && tile <= NUM_NIB_TILES, "hawq_incep_conv_nib: no tile %d (ids 1 .. %d)", tile, NUM_NIB_TILES);
    Geo g;
    const char *why = refusal(a, &g);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_nib: %s", why);
    why = tile_refusal(a, tile);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_nib: tile %d (%d px x %d ch) refuses the launch: %s", tile, kNib[tile].bm, kNib[tile].bn, why);
    hipStream_t s = (hipStream_t)stream;
    if (tile == 1) launch<128, 128, 2, 2, 1>(a, g, s);
    else if (tile == 2) launch<128, 64, 2, 2, 1>(a, g, s);
    else launch<64, 64, 2, 1, 2>(a, g, s);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
