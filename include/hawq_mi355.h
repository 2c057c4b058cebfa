/*
 * hawq_mi355.h - C ABI of libhawq_mi355.so: MI355X (gfx950) integer-only kernels for the
 * frozen forward of HAWQ's quantized ResNets.
 *
 * The reference (Zhen-Dong/HAWQ) has no FFI layer: its operator boundary is the Python
 * nn.Module API of utils/quantization_utils/quant_modules.py.  Each entry point below is
 * what a maintainer would bind (ctypes) to replace the arithmetic of
 * one of those modules' frozen forward; the citation on each says which lines it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless named host_*.
 *   - the library never allocates or frees activation memory and keeps no global mutable
 *     state besides a thread-local error string; the device is the pointer's device and
 *     work is enqueued on the hipStream_t passed as `void* stream` (0 = default stream).
 *   - every function returns 0 on success, non-zero on error; hawq_last_error() gives
 *     the message of the calling thread's last failure.
 *   - activations are NHWC.  8-bit tensors are int8; 4-bit tensors are nibble-packed
 *     "hawq4" format: within every group of 8 consecutive channels c0..c7 the 32-bit word is
 *     (c0|c1<<8|c2<<16|c3<<24) | (c4|c5<<8|c6<<16|c7<<24)<<4  (so that two mask ops unpack it
 *     into two int8x4 words in channel order).  16-bit residual tensors are uint16
 *     (post-ReLU values; overflow beyond 65535 sets bit 0 of *flags and saturates) or int32.
 *   - dyadic requantisation tables are (m, ek) pairs, ek = e | k << 8, 0 <= m < 2^31, 1 <= e <= 62:
 *     q = round_half_even(((acc << k) * m) / 2^e)  (quant_utils.py:188-213, 404-408); the
 *     pre-shift k (|acc << k| < 2^31) lets the host lift small e to >= 33 without changing the
 *     rational m * 2^k / 2^e (hawq_amd.quant_utils.requant_table).
 */
#ifndef HAWQ_MI355_H
#define HAWQ_MI355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HAWQ_ABI_VERSION 5

const char *hawq_last_error(void);
int hawq_abi_version(void);
/* number of gfx950 kernels compiled into the library (sanity / "native code loaded" probe) */
int hawq_device_ok(void);

/* ---- epilogue kinds of hawq_conv2d ------------------------------------------------- */
enum {
    HAWQ_EPI_RAW = 0,      /* out_acc[m][c] = acc + bias               (int32 accumulators)  */
    HAWQ_EPI_REQUANT = 1,  /* out_q = clamp(dyadic(relu?(acc+bias)))   conv -> ReLU -> QuantAct */
    HAWQ_EPI_RESIDUAL = 2, /* residual add of two separately requantised branches, ReLU,
                              optional next-unit QuantAct                                     */
    HAWQ_EPI_DEQUANT = 3   /* out_f32[m][c] = float(acc+bias) * fscale[c]   (QuantLinear)     */
};

/*
 * One fused convolution launch.  Replaces, for a frozen model,
 *   QuantBnConv2d.forward   quant_modules.py:489-494   (integer conv + bias)
 *   nn.ReLU                 q_resnet.py:242,246,258
 *   QuantAct.forward/fixedpoint_fn case 0   quant_modules.py:288-293, quant_utils.py:390-413
 *   QuantAct.forward/fixedpoint_fn case 1   quant_modules.py:294-301, quant_utils.py:416-456
 *   (+ the next unit's block-input QuantAct, q_resnet.py:234/239)
 *   QuantLinear.forward     quant_modules.py:125-130   (HAWQ_EPI_DEQUANT, 1x1 "conv" on [B,1,1,K])
 * Implicit GEMM on int8 MFMA; 4-bit operands are unpacked on the way into LDS.
 */
typedef struct hawq_conv_args {
    /* main branch */
    const void *in;       /* [N][H][W][Cin]  int8, or hawq4-packed when in_bits == 4         */
    const void *wgt;      /* [Cout][KH][KW][Cin] int8 / hawq4-packed (see hawq_pack_*)        */
    const int32_t *bias;  /* [Cout] bias_integer                                              */
    int32_t N, H, W, Cin, Cout, KH, KW, stride, pad;
    int32_t in_bits, w_bits; /* 8 or 4 each (any combination)                                  */
    /* optional second branch sharing the output grid: the identity 1x1 conv of a resize unit
       (q_resnet.py:236).  in2 == NULL disables it. */
    const void *in2;
    const void *wgt2;
    const int32_t *bias2;
    int32_t H2, W2, Cin2, stride2, in2_bits, w2_bits;
    /* Without a second branch (in2 == NULL) H2, W2 and stride2 describe the OTHER tensor the RESIDUAL epilogue adds, the stored residual: with
       res_in != NULL and stride2 = s >= 2 ("res_sub"; 0 and 1: res_in is a tensor of this launch's own grid, as always) `in` and out_q are dense
       [N][H][W] tensors and only res_in lives on a larger map, [N][H2][W2][Cout] with (H2 - 1) / s + 1 == H and (W2 - 1) / s + 1 == W, read at pixel
       (n, s y, s x) - the expand conv behind a 3x3 launch that ran with out_sub = s.  Same preconditions as out_sub (1x1 / stride 1 / pad 0, RESIDUAL,
       res_out == NULL, dense NHWC rows), which it excludes.  Taken by the general tiles and by the expand conv alone of hawq_conv_expand_reduce, and
       refused by everything else.  Other epilogues ignore the three.
       Why no field of its own: out_sub is pinned as the LAST field of this block - by the ctypes mirror's layout test and by recorded launch
       lists that hold every field of every block - so three appended fields would have invalidated both; they can follow in a change that
       re-records those.  The hazard of the reuse: single-branch RESIDUAL launches used to ignore these three fields.  A caller who fills a
       dual-branch block and then clears in2 (keeping res_in and a stride2 >= 2) no longer gets the plain launch: it is refused unless
       (H2 - 1) / stride2 + 1 == H and likewise for W, and with such extents res_in is addressed on the H2 x W2 map.  Zero the three fields
       when in2 is cleared. */
    int32_t epilogue; /* HAWQ_EPI_* */
    int32_t relu;     /* apply max(.,0) to acc+bias before requantising (REQUANT only)         */
    /* requant tables of the main branch: per output channel */
    const int32_t *m;
    const int32_t *e;
    /* RESIDUAL: identity branch tables - per channel (second branch) or scalar (passthrough) */
    const int32_t *m_id;
    const int32_t *e_id;
    int32_t m_id_scalar, e_id_scalar;
    const void *res_in;   /* [M][Cout] block input carried as residual (uint16 or int32)      */
    int32_t res_in_bits;  /* 16 or 32                                                          */
    void *res_out;        /* [M][Cout] post-ReLU residual for the next unit, or NULL           */
    int32_t res_out_bits; /* 16 or 32                                                          */
    /* quantised output (REQUANT: this conv's QuantAct; RESIDUAL: next unit's QuantAct) */
    void *out_q;          /* [M][Cout] int8 / hawq4, or NULL                                   */
    int32_t out_bits;     /* 8 or 4                                                            */
    int32_t q_lo, q_hi;   /* clamp range                                                       */
    int32_t mq, eq;       /* RESIDUAL: scalar table of the next QuantAct (S_w == 1)            */
    int32_t *out_acc;     /* RAW: [M][Cout] int32                                              */
    float *out_f32;       /* DEQUANT: [M][ldo] fp32, only channels < n_valid are written       */
    const float *fscale;  /* DEQUANT: [Cout]                                                   */
    int32_t ldo, n_valid; /* n_valid > 0 on the general REQUANT / RESIDUAL path (fast_tables == 0): channels >= n_valid are
                             padding (zero weights, bias, tables and identity) and are written as zeros without arithmetic */
    int32_t *flags;       /* device int32: bit0 = uint16 residual overflow                     */
    int32_t tile;         /* 0 = heuristic; else tile config id (see hawq_conv2d_num_tiles)    */
    const int32_t *ctab;    /* fast path only: [Cout][4] = {m, (e-32)|k<<8, lo32(C), hi32(C)}, C = (bias<<k)*m + 2^(e-1) */
    const int32_t *ctab_id; /* fast path, second branch: same for (bias2, m_id, e_id)                   */
    int32_t fast_tables;  /* caller asserts the "fast contract" for EVERY dyadic table of this call:
                             e in [33,62]; pre-shift k in [0,30] with |value << k| < 2^31; no exact
                             rounding tie is possible for the value ranges involved (the host proves
                             this from the trailing zeros of m - hawq_amd.quant_utils.tables_are_fast).
                             Enables the 2-instruction requant path and the LDS-staged coalesced
                             epilogue (8/8 and 4/4 operand widths, 16-bit residuals); needs ctab
                             (and ctab_id with a second branch).  0 = exact general path (any e in
                             [1,62], any k, ties handled) driven by bias / m / e.
                             Bit 1 (value 3): hint that every pre-shift k of ctab, ctab_id and
                             (mq, eq) is 0 (checked for eq; currently not used to pick a kernel).
                             Bit 2 (value 5): the tie-freedom proof FAILED for some entry; the kernel
                             then applies the exact round-half-even tie correction to every requant
                             of the call (e in [33,62] and |value << k| < 2^31 still required).
                             Bit 3 (value | 8): every PER-CHANNEL pre-shift k of this conv's ctab (and ctab_id) is 0
                             (the scalar tables may still carry one): hawq_conv_expand_reduce then runs the
                             instantiation without the shift / field extraction (3 VALU instructions per output
                             fewer); other entry points ignore the bit.                                          */
    int32_t in_planar;    /* layout of `in`: 0 = NHWC pixel rows [M][Cin*bits/8];  1 = channel-group planes
                             [Cin/G][M][16 B] with G = 16 (int8) / 32 (hawq4) channels per 16-byte unit.  Planes
                             are what the 3x3 band kernels' LDS-DMA fill wants (64 consecutive pixels of one plane
                             are one contiguous KiB); only those kernels read them.                              */
    int32_t out_planar;   /* same for `out_q` (fast-contract REQUANT / RESIDUAL epilogues only)                  */
    /* ABI 3 - RESIDUAL epilogue of networks whose units end WITHOUT an activation (MobileNetV2's linear bottleneck,
       q_mobilenetv2.py:60-93): exact general path only (fast_tables == 0), 32-bit residual tensors.
       res_no_relu: 1 = the requantised sum is stored as is (signed); 0 = ReLU after it (the ResNets, q_resnet.py:258).
       res_clamp16: 1 = clamp the result to [-32768, 32767]: quant_act_int32 WITHOUT an identity branch is fixedpoint_fn case 0,
                    which clamps to its 16-bit range (quant_utils.py:409-413); with an identity (case 1) nothing clamps (:456).
       With res_in == NULL and in2 == NULL there is no identity branch: o = requant(acc + bias).                          */
    int32_t res_no_relu, res_clamp16;
    /* ABI 4 - narrow tensors stored at their own width (MobileNetV2's 16 / 24 / 32 / 96 / 144 / 160-channel tensors,
       q_mobilenetv2.py:36-58: in the reference they are exactly that wide; padding every one of them to the 64-channel tile
       doubled to quadrupled the bytes of the early layers).
       in_pitch:  bytes from one pixel row of `in` to the next; 0 = dense (Cin * in_bits / 8).  A pitch BELOW the dense row lets a
                  tensor of Cin_valid <= in_pitch channels feed a conv whose K (Cin) is padded to 64: the 64-byte chunk reads run on
                  into the following pixel's bytes, where they meet zero weights (integers: garbage x 0 = 0, exact).  Multiple of
                  16, int8 operands, single branch, not planar, not the band kernels; the buffer must be readable 64 bytes past
                  its last row.
       out_pitch: channels per stored pixel row of out_q / res_out / res_in; 0 = Cout.  Channels >= out_pitch are not written
                  at all; on the general path channels in [n_valid, out_pitch) are written as zeros.  Multiple of 16,
                  REQUANT / RESIDUAL epilogues with NHWC rows (fast REQUANT, or the general path), single branch.           */
    int32_t in_pitch, out_pitch;
    /* ABI 5 - the round-5 3x3 kernels (band_v2.hip; 3x3 / stride 1 / pad 1, int8 operands, Cin >= 128, planar input): the SAME weight
       integers as `wgt` (quant_modules.py:462-466: weight_integer of the BN-folded conv), packed by hawq_pack_w3x3_band into the byte
       stream a workgroup consumes - [Cout/64][Cin/64][kh][kw][64 rows][64 B], the 16-byte slots of a row XOR-swizzled - so that every
       LDS-DMA instruction of the weight ring copies one contiguous KiB.  NULL = not provided: those tile ids refuse the layer. */
    const void *wgt_band;
    /* ABI 5 - the round-5 1x1 kernels (gemm_v2.hip; 1x1 / pad 0 convs whose pixel row is a multiple of 128 BYTES - int8 operands with
       Cin % 128 == 0 or, round 6, hawq4 operands (in_bits == w_bits == 4) with Cin % 256 == 0 -, NHWC rows): the weights of
       `wgt` / `wgt2` packed by hawq_pack_w1x1_k128 - [Cout/64][row bytes/128][64 rows][128 B], 16-byte slot s of row r at s ^ ((r >> 1) & 7) -
       so that the K loop walks full 128-byte lines and every weight piece is a contiguous KiB.  NULL = not provided. */
    const void *wgt_k128;
    const void *wgt2_k128;
    /* out_sub = s >= 2 (0 and 1: every pixel, as always): the launch evaluates only the output pixels (n, s y', s x') with y' < Ho' = (Ho - 1) / s + 1
       and x' < Wo' = (Wo - 1) / s + 1 - what a 1x1 / pad 0 / stride s conv (the conv1 and the identity conv of a stage's first unit, q_resnet.py:236-240) reads
       of the block input this launch writes.  `in` and `res_in` stay tensors of the full H x W map and are read at that source pixel; out_q is stored
       densely as [N][Ho'][Wo'][Cout] (int8 or hawq4).  Needs: a 1x1 / stride 1 / pad 0 conv, single branch (in2 == NULL) and res_out == NULL (no dense
       residual is produced; the uint16 overflow flag can only be raised by the pixels that are evaluated).  Taken by hawq_conv2d's general tiles
       (RESIDUAL epilogue, 16- or 32-bit res_in, dense NHWC rows) and by the expand conv alone of hawq_conv_expand_reduce (reduce.wgt == NULL); the special-purpose
       tile ids, hawq_conv2d_splitk and the fused pairs refuse it through their applicability queries.
       Also taken on a 3x3 / stride 1 / pad 1 single-branch launch with the REQUANT or RAW epilogue (the second conv of a stage's last bottleneck, whose
       1x1 successor runs on the subsampled grid): with pad 1 that is exactly the 3x3 / stride s conv on `in`, which stays the full H x W map;
       out_q / out_acc are dense over [N][Ho'][Wo'][Cout].  NHWC rows, out_planar refused; the general tiles take it, every special-purpose 3x3 tile id and
       hawq_conv2d_splitk refuse it through their queries. */
    int32_t out_sub;
} hawq_conv_args;

int hawq_conv2d(const hawq_conv_args *args, void *stream);
/* The tile ids 1 .. hawq_conv2d_num_tiles() are five kernel families in a fixed order, each owning consecutive ids (one table in
 * conv_dispatch.hip; the queries below are read from it): family 0 the general tiles (conv_igemm.hip), which take any layer;
 * 1 the 3x3/stride-1/pad-1 "band" kernels of rounds 1-3 (band_v1.hip); 2 the weight-stationary persistent kernel (band_persist.hip)
 * for Cin == Cout == 64 (int8 in and out; REQUANT - or, round 5, single-branch RESIDUAL on uint16 residuals; NHWC or planar output)
 * with one / two workgroups per CU; 3 (ABI 5) the hawq_conv2d_num_band2_tiles() 3x3 kernels of round 5 (band_v2.hip); 4 the
 * hawq_conv2d_num_gemm2_tiles() streaming 1x1 kernels of round 5 (gemm_v2.hip). */
int hawq_conv2d_num_tiles(void);
/* The LAST hawq_conv2d_num_band_tiles() tile ids - families 1 to 4 - are special-purpose kernels (fast-contract layers only;
 * hawq_conv2d refuses them for any layer they are not built for). */
int hawq_conv2d_num_band_tiles(void);
/* What hawq_conv2d would do with `args`, without doing it: the argument check and the choice of kernel, no launch.  Host only - it
 * never calls the HIP runtime, so it answers on a machine without a GPU (pointers are tested against NULL, never dereferenced).
 * Returns what hawq_conv2d returns for a refused struct, with the same hawq_last_error text.
 *   family, tile, index: the family (above), the 1-based tile id the launch resolves to - after the heuristic, the Cout % BN
 *     fallback and the twin / K-sub rules of the general tiles - and its 0-based position in the family.
 *   fn_table, fn: the slot of the family's function table.  Family 0: fn_table 0 single[epilogue][variant], 1 dual[variant],
 *     2 tie_single[epilogue - 1][variant - 1], 3 tie_dual[variant - 1]; family 1: fn[hawq4][exact-tie][residual]; family 2:
 *     fn[exact-tie][residual]; families 3 and 4: fn_table 0 fn[hawq4][epilogue slot][exact-tie], 1 raw[hawq4]; family 3 with
 *     out_sub: 2 the strided twin's fn[hawq4][exact-tie], 3 its raw[hawq4].  Unused: -1.
 *   grid, block, lds_bytes: the launch; grid is -1 where it depends on the device (family 2 sizes it by the CU count).
 *   stride .. out_pitch: the kernel arguments hawq_conv2d computes rather than copies (effective stride and subsampling, output
 *     grid, folded clamp, defaulted scalar tables, requant mode, pitches); gfast and ring_bytes are 0 outside family 0. */
typedef struct hawq_conv_choice {
    int32_t family, tile, index;
    int32_t fn_table, fn[3];
    int32_t grid, block, lds_bytes;
    int32_t stride, res_sub, Ho, Wo, M, q_lo, mq, eq, m_id_s, e_id_s, k0, ck0, gfast, in_pitch, out_pitch, ring_bytes;
} hawq_conv_choice;
int hawq_conv2d_choice(const hawq_conv_args *args, hawq_conv_choice *out);
/* 1-based id of the preferred band tile that takes this layer as described (geometry, widths, epilogue,
 * fast_tables), 0 if none does: lets a caller decide whether the producer should write planar activations. */
int hawq_conv2d_band_tile(const hawq_conv_args *args);
/* ABI 5: hawq_conv2d_num_band2_tiles() of those ids (the ones in front of the 1x1 kernels) are the round-5 3x3 kernels (band_v2.hip; need args->wgt_band and
 * in_planar == 1; int8 operands with Cin >= 128, or hawq4 operands (in_bits == w_bits == 4) with Cin >= 256; REQUANT, or single-branch RESIDUAL on uint16
 * residuals; int8 / hawq4 output, NHWC or planar).  hawq_conv2d_band2_tile: 1-based id of the first of them that takes the layer as described, else 0.
 * hawq_pack_w3x3_band: [Cout][3][3][Cin] int8 (the layout of `wgt`) -> the stream described at hawq_conv_args.wgt_band, on the host
 * (dst and src are host pointers of Cout * 9 * Cin bytes; Cin = BYTES per tap row - the channel count for int8 weights, half of it for hawq4 -; Cin and Cout multiples of 64). */
int hawq_conv2d_num_band2_tiles(void);
int hawq_conv2d_band2_tile(const hawq_conv_args *args);
/* A 3x3 launch with out_sub = s >= 2 runs the STRIDED TWIN of a round-5 3x3 kernel under the same tile id (128 outputs over a 768-pixel band, 64 outputs over
 * a 512-pixel band): the band of a pixel tile covers the source pixels of its first to its last output, a row and a pixel to either side, and the query refuses
 * every launch in which some tile's band does not fit.  hawq_conv2d_band2_sub_extent: that band for pixel tile `tile` on the `index`-th (0-based) of those
 * kernels, from the function the kernel itself uses - out[0] first band pixel on the source map (line-aligned, may be negative), out[1] band pixels reached,
 * out[2] band pixels an LDS stage holds (a launch fits when out[1] <= out[2] - 4 for every tile), out[3] pixel tiles of the launch, out[4] outputs per tile.
 * Host only. */
int hawq_conv2d_band2_sub_extent(const hawq_conv_args *args, int32_t index, int32_t tile, int32_t *out);
int hawq_pack_w3x3_band(const int8_t *src, int8_t *dst, int32_t Cout, int32_t Cin);
/* ABI 5: the LAST hawq_conv2d_num_gemm2_tiles() tile ids are the round-5 streaming
 * 1x1 kernels (need args->wgt_k128 - and wgt2_k128 with a second branch -, NHWC input, fast_tables; REQUANT, RESIDUAL on uint16
 * residuals, or RESIDUAL with the identity conv as second branch).  hawq_conv2d_gemm2_first(): the 1-based id of the first of them.
 * hawq_pack_w1x1_k128: [Cout][Cin] int8 -> the stream described at hawq_conv_args.wgt_k128 (host pointers; Cin = BYTES per weight row).
 * Round 6 (no change of the argument block): both round-5 kernel families also take
 *   - HAWQ_EPI_RAW (out_acc: int32 accumulators + bias, dense [M][Cout]; no tables needed) - what the parity tests compare with the
 *     oracle's exact sums (quant_modules.py:489-494), and
 *   - the streaming 1x1 kernels take hawq4 operands (both branches of a dual launch must have the same widths) and write int8 or
 *     hawq4 outputs (out_bits 4: q_lo >= 0, q_hi <= 15), NHWC rows or channel-group planes - the reduce convs of the 4-bit schedules
 *     (bit_config.py:806, 1512). */
int hawq_conv2d_num_gemm2_tiles(void);
int hawq_conv2d_gemm2_first(void);
int hawq_pack_w1x1_k128(const int8_t *src, int8_t *dst, int32_t Cout, int32_t Cin);

/* Cross-workgroup split-K form of hawq_conv2d for launches with few output tiles (batch 1-16): the same arguments, the same
 * integers (conv_splitk.hip).  The grid is (64-pixel x 64-channel output tiles) x (K slices); each slice workgroup writes its int32
 * partial tile to `slab`, the last one to arrive at a tile (one int32 arrival counter per tile in `counters`) sums the slabs and
 * runs hawq_conv2d's epilogue.  args->tile is ignored.  Takes: 1x1 / pad 0 or 3x3 / pad 1 convs with stride 1 or 2; int8 operands
 * (both branches) and int8 out_q; HAWQ_EPI_RAW, REQUANT or RESIDUAL (pass-through identity, or the identity 1x1 conv as second
 * branch); NHWC or planar in / out (planar input: single-branch fast-contract launches); any M.  Refuses 4-bit operands or
 * outputs, n_valid / in_pitch / out_pitch, HAWQ_EPI_DEQUANT, and slice counts that do not divide the KH * KW * Cin / 64 K chunks.
 * The second branch's Cin2 / 64 chunks become S2 extra slices of q2 chunks, q2 = the largest divisor of Cin2 / 64 that is
 * <= KH * KW * Cin / 64 / slices.
 *   hawq_conv2d_splitk_ok: 1 = the kernel takes this launch with `slices` slices of the main branch, 0 = it refuses (host only).
 *   hawq_conv2d_splitk_workspace: slab_bytes = tiles * (slices + S2) * 64 * 64 * 4, counter_bytes = tiles * 4 with
 *     tiles = ceil(N * Ho * Wo / 64) * Cout / 64 (host only; non-zero return if the launch is refused).
 *   hawq_conv2d_splitk: `counters` must be zero before the first launch; every launch leaves them zero, so launches on one stream
 *     (and graph replays) may share one workspace.  Launches that may run concurrently need workspaces of their own. */
int hawq_conv2d_splitk_ok(const hawq_conv_args *args, int32_t slices);
int hawq_conv2d_splitk_workspace(const hawq_conv_args *args, int32_t slices, int64_t *slab_bytes, int64_t *counter_bytes);
int hawq_conv2d_splitk(const hawq_conv_args *args, int32_t slices, void *slab, int32_t *counters, void *stream);

/* Fused launch of two consecutive layers of the bottleneck graph (q_resnet.py:231-260): the 1x1 expand conv of unit i
 * with its RESIDUAL epilogue (x + identity -> quant_act_int32 -> ReLU -> quant_act of unit i+1) and the 1x1 reduce
 * conv of unit i+1 with its REQUANT epilogue (ReLU -> quant_act1).  `expand` and `reduce` are filled exactly as for
 * two hawq_conv2d calls, except that expand.out_q and reduce.in are ignored: the 8-bit block input of unit i+1 stays
 * on chip.  Needs: both convs 1x1 / stride 1, int8 operands, fast_tables != 0, uint16 residual in and out (single
 * branch) - or, for expand.Cin == 64, a second branch in2 / wgt2 / ctab_id that is a 1x1 / stride-1 conv over the same pixels with
 * Cin2 == 64 (the first unit of ResNet50's stage 1: its requantised accumulators replace the stored residual) -,
 * reduce.Cin == expand.Cout, reduce.Cout == expand.Cin in {64, 128, 256}; reduce.out_bits 8, or 4 (round 3: the reduce conv's QuantAct
 * is 4-bit and a nibble 3x3 conv follows - the launch packs hawq4 itself, NHWC rows of Cout / 2 bytes or planes [Cout / 32][M][16 B];
 * needs 0 <= q_lo, q_hi <= 15).
 * tile: 0 = default kernel variant for the channel count, 1..hawq_conv_expand_reduce_variants() = a specific one (the variants of
 * fused_er.hip first, then the wave-private ones of fused_wp.hip: same results, different organisation of the launch).
 * reduce.wgt == NULL (round 3): the expand conv ALONE on the wave-private kernel - `expand` exactly as for hawq_conv2d with the
 * RESIDUAL epilogue (single branch, uint16 residual in, 8-bit out_q, res_out optional; expand.Cin in {64, 128, 256, 512}); some
 * variants split the output channels over gridDim.y.  Round 6: expand.out_bits 4 (0 <= q_lo, q_hi <= 15) writes the next unit's block
 * input as hawq4 rows of Cout / 2 bytes - the last expand conv of a stage in a 4-bit schedule, whose successor reads nibbles
 * (bit_config.py:806, 1512).  0 variants = use hawq_conv2d. */
typedef struct hawq_expand_reduce_args {
    hawq_conv_args expand;
    hawq_conv_args reduce;
    int32_t tile;
} hawq_expand_reduce_args;
int hawq_conv_expand_reduce(const hawq_expand_reduce_args *args, void *stream);
/* number of kernel variants that take this pair (0: the pair cannot be fused, launch two hawq_conv2d instead) */
int hawq_conv_expand_reduce_variants(const hawq_expand_reduce_args *args);
/* Host-only: the launch shape of variant `nth` (numbered as `tile`; 0 = the default) when it is a wave-private variant of
 * fused_wp.hip - the pixels one workgroup covers (gridDim.x = ceil(M / pixels)) and the number of workgroups along gridDim.y that
 * share the Cout / 64 output slices of a pixel tile (1 for every pair variant).  Returns 0 and fills both; non-zero, both untouched,
 * for a variant of another kernel family or an id the launch does not have.  For tests, the tuner's log and tools. */
int hawq_conv_expand_reduce_variant_shape(const hawq_expand_reduce_args *args, int32_t nth, int32_t *pixels_per_workgroup, int32_t *slice_split);

/* QuantAct input case (quant_modules.py:271-274; quant_utils.py:73-97, 237-258):
 * q = clamp(rint(inv_scale * x), lo, hi); fp32 NCHW [N][3][H][W] -> int8 NHWC4 with a zero
 * border: out[N][H+2*pad_t..][..][4]; out_h/out_w are the padded extents, (pad_top, pad_left)
 * the offset of pixel (0,0).  The border and channel 3 must have been zeroed once. */
int hawq_quantize_input(const float *x, int8_t *out, int32_t N, int32_t C, int32_t H, int32_t W,
                        int32_t out_h, int32_t out_w, int32_t pad_top, int32_t pad_left,
                        float inv_scale, int32_t lo, int32_t hi, void *stream);

/* Stem: 7x7/2 conv on the padded NHWC4 int8 image + bias, then QuantAct(16b, case 0, clamp)
 * + ReLU fused (requant commutes with the following max-pool because it is monotone):
 * quant_modules.py:489-494 + q_resnet.py:117-122.  wgt is [64][7][8][4] int8 (kw, c zero
 * padded).  out16 [N][Ho][Wo][64] uint16;  out_acc (optional) raw int32. */
int hawq_stem_conv7(const int8_t *in, const int8_t *wgt, const int32_t *bias, const int32_t *m,
                    const int32_t *e, int32_t N, int32_t Hp, int32_t Wp, int32_t Ho, int32_t Wo,
                    int32_t q_lo, int32_t q_hi, uint16_t *out16, int32_t *out_acc, void *stream);

/* Fused stem: QuantAct input case + 7x7/2 conv + bias + MaxPool2d(3,2,1) + QuantAct(16b, clamp) + ReLU
 * + first unit's QuantAct in one launch (q_resnet.py:115-122, 234/239): fp32 NCHW images ->
 * res_out [N][Hp][Wp][64] uint16 and/or out_q int8/hawq4.  The max-pool is taken on the raw accumulators
 * (the per-channel requantisation is monotone), so the 112x112 intermediate never reaches memory.
 * fast_tables: the caller asserts the fast contract for (m, e) and (mq, eq) (see hawq_conv_args). */
int hawq_stem_fused(const float *x, int32_t N, int32_t C, int32_t H, int32_t W, float inv_scale, int32_t in_lo,
                    int32_t in_hi, const int8_t *wgt, const int32_t *bias, const int32_t *m, const int32_t *e,
                    int32_t a_lo, int32_t a_hi, uint16_t *res_out, void *out_q, int32_t out_bits, int32_t mq,
                    int32_t eq, int32_t q_lo, int32_t q_hi, int32_t fast_tables, void *stream);

/* Same kernel fed by uint8 NHWC images [N][H][W][C] (decoder output) and a host-built table
 * lut[c][u] = clamp(rint(fl(1/S) * normalise_c(u / 255))), c < 3, u < 256 (int8, 4-byte aligned): the input
 * QuantAct (quant_modules.py:271-274) of the normalised image becomes a look-up, bit-identical to quantising the
 * fp32 tensor that torchvision's ToTensor + Normalize (quant_train.py:432-440) would have produced.            */
int hawq_stem_fused_u8(const uint8_t *x, const int8_t *lut, int32_t N, int32_t C, int32_t H, int32_t W,
                       const int8_t *wgt, const int32_t *bias, const int32_t *m, const int32_t *e, int32_t a_lo,
                       int32_t a_hi, uint16_t *res_out, void *out_q, int32_t out_bits, int32_t mq, int32_t eq,
                       int32_t q_lo, int32_t q_hi, int32_t fast_tables, void *stream);

/* nn.MaxPool2d(3,2,1) (q_resnet.py:93,119) on the requantised stem output + the first
 * unit's QuantAct: in [N][H][W][C] uint16 -> res_out [N][Ho][Wo][C] uint16 and
 * out_q = clamp(dyadic(res, mq, eq)) int8/hawq4 (either may be NULL). */
int hawq_maxpool3s2_requant(const uint16_t *in, int32_t N, int32_t H, int32_t W, int32_t C,
                            uint16_t *res_out, void *out_q, int32_t out_bits, int32_t mq, int32_t eq,
                            int32_t q_lo, int32_t q_hi, void *stream);

/* Block-input QuantAct on a stored residual (quant_modules.py:288-293 with S_w == 1):
 * in [n] uint16/int32 -> out int8/hawq4.  Used when the producer could not fuse it. */
int hawq_requant_residual(const void *in, int32_t in_bits, int64_t n, void *out_q, int32_t out_bits,
                          int32_t mq, int32_t eq, int32_t q_lo, int32_t q_hi, void *stream);

/* QuantAveragePool2d + quant_act_output (quant_modules.py:596-600, quant_utils.py:334-337,
 * q_resnet.py:129-131): in [N][HW][C] uint16/int32 (>= 0) -> floor(sum/HW) -> dyadic -> clamp
 * -> int8 [N][C].  pooled_out (optional) receives the int32 pooled integers. */
int hawq_avgpool_requant(const void *in, int32_t in_bits, int32_t N, int32_t HW, int32_t C, int8_t *out,
                         int32_t *pooled_out, int32_t mq, int32_t eq, int32_t q_lo, int32_t q_hi,
                         void *stream);

/* QuantLinear on the frozen integer path (quant_modules.py:112-130: F.linear(x_int, weight_integer, bias_integer) * (fc_scaling_factor *
 * prev_act_scaling_factor); the classifier of every Q_ResNet, q_resnet.py:132-134) as its own launch (fc_dequant.hip, round 5):
 *   out_f32[n * ldo + o] = (float)(sum_k q[n][k] * wgt[o][k] + bias[o]) * fscale[o]      for o < n_valid
 * q [N][K] int8, wgt [Nout_p][K] int8 (row-major = the [Cout][1][1][Cin] layout hawq_conv2d takes), bias / fscale [Nout_p].  The same bytes
 * as hawq_conv2d with epilogue DEQUANT on the 1 x 1 map (tests/test_gpu_kernels.py), several times faster for the M = batch, long-K
 * shape.  hawq_fc_dequant_ok: K % 128 == 0 and Nout_p % 32 == 0. */
int hawq_fc_dequant_ok(int32_t N, int32_t K, int32_t Nout_p);
int hawq_fc_dequant(const int8_t *q, const int8_t *wgt, const int32_t *bias, const float *fscale, float *out_f32, int32_t N, int32_t K,
                    int32_t Nout_p, int32_t n_valid, int32_t ldo, void *stream);

/* ---- module-compatible (fp32 tuple convention) adapters ---------------------------------
 * The reference modules exchange fp32 tensors holding integer*scale.  These kernels move
 * between that convention (NCHW fp32) and the integer NHWC tensors the conv kernels use. */

/* x_int = rint(x / S) (quant_modules.py:490, 126): fp32 NCHW [N][C][H][W] -> int8 / hawq4 NHWC
 * with Cpad >= C channels (extra channels zero). */
int hawq_f32_nchw_to_q_nhwc(const float *x, void *out, int32_t N, int32_t C, int32_t H, int32_t W,
                            int32_t Cpad, int32_t bits, float scale, void *stream);
/* y = float(acc) * fscale[c] (quant_modules.py:491-494): int32 NHWC [N][H][W][Cpad] -> fp32 NCHW */
int hawq_acc_nhwc_to_f32_nchw(const int32_t *acc, float *y, int32_t N, int32_t C, int32_t H, int32_t W,
                              int32_t Cpad, const float *fscale, void *stream);
/* QuantAct / fixedpoint_fn on fp32 NCHW tensors (quant_utils.py:363-456).
 * case 0: y = clamp(dyadic(rint(z/S_a/S_w[c]), m[c], e[c])) * S_out
 * case 1: y = (dyadic(rint(ident/S_ida/S_idw[c]), m1, e1) + dyadic(rint((z-ident)/S_a/S_w[c]), m2, e2)) * S_out
 * per_ch = number of entries in sw/m/e (1 or C); per_ch_id likewise for the identity tables. */
int hawq_fixedpoint_f32(const float *z, float *y, int32_t N, int32_t C, int32_t HW, float s_a,
                        const float *s_w, const int32_t *m, const int32_t *e, int32_t per_ch,
                        const float *ident, float s_ida, const float *s_idw, const int32_t *m_id,
                        const int32_t *e_id, int32_t per_ch_id, float s_out, int32_t do_clamp,
                        int32_t q_lo, int32_t q_hi, void *stream);
/* QuantAct input case on fp32 (quant_utils.py:73-97): y = clamp(rint(inv_scale*x)) * scale */
int hawq_fakequant_f32(const float *x, float *y, int64_t n, float inv_scale, float scale, int32_t lo,
                       int32_t hi, void *stream);
/* QuantAveragePool2d on fp32 NCHW (quant_modules.py:596-602): y = trunc(avg(rint(x/S)) + 0.01) * S */
int hawq_avgpool_f32(const float *x, float *y, int32_t NC, int32_t HW, float scale, void *stream);

/* Grouped / depthwise integer conv for the module-compatible path (F.conv2d(..., groups), quant_modules.py:489-494 and
 * 727-736; MobileNetV2's depthwise 3x3): in [N][H][W][Cin] int8, wgt [Cout][KH][KW][Cin/groups] int8, bias [Cout] or NULL
 * -> out_acc [N][Ho][Wo][Cout] int32 (exact). */
int hawq_conv2d_grouped(const int8_t *in, const int8_t *wgt, const int32_t *bias, int32_t N, int32_t H, int32_t W,
                        int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t groups,
                        int32_t *out_acc, void *stream);

/* Depthwise 3x3 / pad 1 conv (groups == Cin == Cout; MobileNetV2's conv2, q_mobilenetv2.py:46-48 through QuantBnConv2d.forward,
 * quant_modules.py:489-494): in [N][H][W][C] int8, wgt9c [3][3][C] int8 (tap-major), bias [C] or NULL -> out_acc
 * [N][Ho][Wo][C] int32 (exact).  C % 4 == 0, stride 1 or 2. */
int hawq_depthwise3x3(const int8_t *in, const int8_t *wgt9c, const int32_t *bias, int32_t N, int32_t H, int32_t W, int32_t C,
                      int32_t stride, int32_t *out_acc, void *stream);

/* The same with the conv's activation + QuantAct fused (conv2 -> ReLU6 -> quant_act2 of a MobileNetV2 unit, q_mobilenetv2.py:70-72;
 * ReLU6 == ReLU + the QuantAct's own clamp: its calibrated range never exceeds 6): out_q[N][Ho][Wo][C] int8 =
 * clamp(dyadic_rne(relu ? max(acc + bias, 0) : acc + bias, m[c], e[c]), q_lo, q_hi) with exact (tie-aware) rounding;
 * out_acc (optional) additionally receives the int32 accumulators.  0 < C_valid < C: channels >= C_valid are padding up to the
 * conv kernels' 64-channel tiles (zero weights / bias / m) - they are written as zeros and cost no loads or MACs (0 = all real). */
int hawq_depthwise3x3_requant(const int8_t *in, const int8_t *wgt9c, const int32_t *bias, const int32_t *m, const int32_t *e,
                              int32_t N, int32_t H, int32_t W, int32_t C, int32_t C_valid, int32_t stride, int32_t relu, int32_t q_lo,
                              int32_t q_hi, int8_t *out_q, int32_t *out_acc, void *stream);

/* The same launch with the fast requant contract (round 4): ctab [C][4] = the fused constants of the layer's requant with the bias folded in
 * (hawq_amd.packing.pack_ctab), fast_tables with the meaning it has in hawq_conv_args: 1, or 5 = exact ties (the host proves the contract, hawq_amd.quant_utils);
 * ReLU is the lower clamp (q_lo >= 0).  3-4 instructions per requant instead of the exact form's ~20. */
int hawq_depthwise3x3_requant_fast(const int8_t *in, const int8_t *wgt9c, const int32_t *ctab, int32_t fast_tables, int32_t N, int32_t H, int32_t W,
                                   int32_t C, int32_t C_valid, int32_t stride, int32_t q_lo, int32_t q_hi, int8_t *out_q, void *stream);

/* One launch per linear-bottleneck unit of MobileNetV2 (Q_LinearBottleneck.forward, q_mobilenetv2.py:59-93; round 4):
 *   block-input int8 -> conv1 1x1 (+ReLU6 + quant_act1) -> conv2 depthwise 3x3 / stride 1|2 / pad 1 (+ReLU6 + quant_act2)
 *   -> conv3 1x1 -> quant_act_int32 (with / without the identity branch) -> the next block-input QuantAct,
 * the expanded ("hidden") tensor never leaves the CU: a workgroup owns an 8 x 16 tile of OUTPUT pixels of one image, recomputes the
 * 1x1 expand conv on the tile's halo window, runs the depthwise taps out of LDS and feeds the projection GEMM from LDS, 32 hidden
 * channels at a time.  Same integers as the three launches (hawq_conv2d REQUANT, hawq_depthwise3x3_requant, hawq_conv2d RESIDUAL).
 *   expand:  as for hawq_conv2d with the REQUANT epilogue and fast_tables != 0 (ctab, q_lo / q_hi, relu = 1); 1x1 / stride 1; Cin is the
 *            K of its packed weights (64 or 128; 192 for the wide units below), in_pitch in {16, 32, 64, 96} (0 = Cin); Cout = the hidden
 *            width padded to 64; out_q is
 *            ignored.  fast_tables bit 3 on BOTH expand and dw_fast_tables (no per-channel pre-shift in ctab / dw_ctab) selects the
 *            instantiation without the shift.
 *   dw_*:    wgt9c [9][expand.Cout] int8 tap-major (zero beyond the real channels); dw_ctab [expand.Cout][4] fused constants of its
 *            requant with the bias folded in (hawq_amd.packing.pack_ctab); dw_fast_tables as hawq_conv_args.fast_tables (1, or 5 = exact
 *            ties); clamp [dw_q_lo >= 0 (ReLU), dw_q_hi <= 127].
 *   project: as for hawq_conv2d with the RESIDUAL epilogue on the direct form: fast_tables != 0 (ctab), res_no_relu = 1, res_clamp16,
 *            res_in (int32, optional identity: then H x W, stride 1, out_pitch == expand's in_pitch), res_out (int32, optional), out_q
 *            int8 (optional), mq / eq / q_lo / q_hi; Cin == expand.Cout; Cout = 64 or 128 packed rows, out_pitch in {16, 32, 64, 96}
 *            (0 = Cout); `in` is ignored.
 *   c_mid:   real hidden channels (channels >= c_mid of every hidden-side table / weight are zero padding).
 *   Wide units: on output maps of at most 8 x 8 pixels the launch also takes in_pitch 160 -> out_pitch 160 or 320 at stride 1 and
 *            in_pitch 96 -> out_pitch 160 at stride 2 (c_mid > 96): 8 x 8 tiles, the projection spread over the waves by output blocks.
 * hawq_linear_bottleneck_ok: 1 when this launch takes the unit as described, else 0 (use the three launches). */
typedef struct hawq_bottleneck_args {
    hawq_conv_args expand;
    hawq_conv_args project;
    const int8_t *dw_wgt9c;
    const int32_t *dw_ctab;
    int32_t dw_stride, dw_q_lo, dw_q_hi, dw_fast_tables;
    int32_t c_mid;
    int32_t tile;   /* 0 = default (channel-planar hidden tensor); 1 = the [pixel][channel] organisation (inputs / outputs up to 64 channels) */
} hawq_bottleneck_args;
int hawq_linear_bottleneck(const hawq_bottleneck_args *args, void *stream);
int hawq_linear_bottleneck_ok(const hawq_bottleneck_args *args);

/* Input QuantAct + im2col for a 3x3 / stride 2 / pad 1 first conv on 3 channels (MobileNetV2's init block, q_mobilenetv2.py:182-186
 * after quant_modules.py:271-274): x fp32 [N][3][H][W] -> out int8 [N][Ho][Wo][64], row = the 27 values
 * clamp(rne(inv_scale * x), q_lo, q_hi) of the output pixel's patch in (kh, kw, c) order (zero outside the image), then 37 zeros.
 * The conv then runs as a 1x1 hawq_conv2d with Cin = 64 on weights laid out in the same (kh, kw, c) order.  C must be 3. */
int hawq_quantize_im2col3x3s2(const float *x, int8_t *out, int32_t N, int32_t C, int32_t H, int32_t W, float inv_scale, int32_t q_lo,
                              int32_t q_hi, void *stream);

/* MobileNetV2's init block as ONE launch (round 4; q_mobilenetv2.py:176-186, 60-65 after quant_modules.py:271-274): the input QuantAct,
 * the 3x3 / stride 2 / pad 1 conv on 3 channels, ReLU6 (as ReLU + clamp), quant_act_int32 and the first unit's block-input QuantAct;
 * neither the patch rows of hawq_quantize_im2col3x3s2 nor anything else intermediate reaches memory.
 *   x / x_u8: exactly one of fp32 NCHW [N][3][H][W] (then inv_scale, in_lo, in_hi describe the input QuantAct) and uint8 NHWC [N][H][W][3]
 *             with lut int8 [3][256] (as hawq_quantize_im2col3x3s2_u8);
 *   conv:     the 1x1 hawq_conv2d launch of the im2col path exactly as it would be issued on the patch rows (N, H = Ho, W = Wo, Cin = Cout = 64,
 *             wgt rows = the 27 taps in (kh, kw, c) order then zeros; RESIDUAL epilogue without identity, fast_tables != 0 with ctab,
 *             res_no_relu / res_clamp16, out_q + mq / eq / q_lo / q_hi, optional int32 res_out, out_pitch 16 or 32); `in` is ignored.
 * hawq_stem3x3s2_ok: 1 when the launch takes this description. */
int hawq_stem3x3s2(const float *x, const uint8_t *x_u8, const int8_t *lut, int32_t H, int32_t W, float inv_scale, int32_t in_lo, int32_t in_hi,
                   const hawq_conv_args *conv, void *stream);
int hawq_stem3x3s2_ok(const float *x, const uint8_t *x_u8, const int8_t *lut, int32_t H, int32_t W, const hawq_conv_args *conv);

/* The same patch rows from uint8 NHWC images [N][H][W][3] (decoder output after resize / crop, quant_train.py:428-440): ToTensor +
 * Normalize + the input QuantAct as one table look-up per channel, lut int8 [3][256] built on the host with the reference
 * pipeline's own float operations (hawq_amd.quant_utils.input_quant_lut) - bit-identical to quantising the normalised fp32 tensor. */
int hawq_quantize_im2col3x3s2_u8(const uint8_t *x, const int8_t *lut, int8_t *out, int32_t N, int32_t C, int32_t H, int32_t W, void *stream);

/* One separable pass of Pillow's 8-bit antialiased resampling (what torchvision's Resize(256) does to the decoded PIL image,
 * quant_train.py:428-440): uint8 HWC in / out, int32 coefficients with 22 fractional bits (hawq_amd/image.py builds them as
 * Resample.c's precompute_coeffs + normalize_coeffs_8bpc do).
 *   horizontal = 1: out[l][o][c], l < lines (input rows line0 + l), o < out_n output columns; in rows are in_w pixels wide
 *   horizontal = 0: out[o][l][c], o < out_n output rows, l < lines columns (in_w == lines, line0 == 0)
 * bounds[2o], bounds[2o+1] = first input index and number of taps of output o; coef[o * ksize + k]. */
int hawq_resample_u8(const uint8_t *in, int32_t in_w, int32_t C, const int32_t *bounds, const int32_t *coef, int32_t ksize,
                     int32_t out_n, int32_t horizontal, int32_t lines, int32_t line0, uint8_t *out, void *stream);

/* Resize + CenterCrop of a whole batch of variable-size images in ONE launch (hawq_amd/csrc/image_batch.hip): both passes above, the
 * 8-bit intermediate kept in LDS, the crop written straight into out uint8 [n_images][crop][crop][3].  Three channels only.
 * One descriptor per image; every *_off is an offset in int32 words into one packed coefficient table `coef`:
 *   hb_off / vb_off: bounds of the crop's output columns / rows, crop x (first input index, taps), absolute input indices;
 *   hc_off / vc_off: their coefficients, crop x kh / crop x kv (22 fractional bits, as hawq_resample_u8).
 * skip_h / skip_v: the resized width / height equals the input's, Pillow skips that pass and the crop window is copied (the
 * offsets and ksize of a skipped pass are not read).  oh, ow: the resized size the crop window (top, left, crop) lies in.
 * A descriptor with h = w = 0 marks an image the launch leaves alone (its band exceeds the LDS budget and the caller resamples it with
 * hawq_resample_u8): it takes no tile and its rows of out are not written. */
typedef struct hawq_image_desc {
    uint64_t base;          /* device address of the image, uint8 [h][w][3], any alignment */
    int32_t h, w, oh, ow;
    int32_t top, left;
    int32_t skip_h, skip_v;
    int32_t hb_off, hc_off, vb_off, vc_off;
    int32_t kh, kv;
} hawq_image_desc;
/* One workgroup: crop rows row0 .. row0 + rows - 1 of image `image`.  It resamples horizontally the crop columns of the input rows
 * y0 .. y1 - 1 those output rows read (from the vertical bounds; top + row0 .. top + row0 + rows - 1 when skip_v) into a uint8 LDS
 * band of (y1 - y0) rows x pitch bytes, pitch = crop * 3 rounded up to a multiple of 4, then runs the vertical pass out of it. */
typedef struct hawq_image_tile {
    int32_t image, row0, rows;
} hawq_image_tile;
/* hawq_image_batch: desc, tiles and coef are device copies of the tables; lds_bytes (dynamic LDS of the launch) >= every tile's band.
 * hawq_image_batch_ok launches nothing and reads the HOST copies of the tables (desc[i].base is not looked at): 1 when every tile's
 * row range lies inside the crop and the tiles of each image cover its crop rows exactly once, every band fits lds_bytes,
 * lds_bytes <= hawq_image_batch_lds_budget, every bounds / coefficient slice lies inside the coef_words words of host_coef, every
 * (first, taps) pair read stays inside its image with taps <= ksize, and the crop window lies inside the resized image (inside the
 * input for a skipped pass); else 0 with the reason in hawq_last_error().  Callers run it on every batch before the upload, so the
 * kernel never sees a table it has not passed.  hawq_image_batch_lds_budget: 65536 bytes - two workgroups share a CU's LDS. */
int hawq_image_batch(const hawq_image_desc *desc, int32_t n_images, const hawq_image_tile *tiles, int32_t n_tiles, const int32_t *coef,
                     uint8_t *out, int32_t crop, int32_t lds_bytes, void *stream);
int hawq_image_batch_ok(const hawq_image_desc *host_desc, int32_t n_images, const hawq_image_tile *host_tiles, int32_t n_tiles,
                        const int32_t *host_coef, int64_t coef_words, int32_t crop, int32_t lds_bytes);
int hawq_image_batch_lds_budget(void);

/* ---- range statistics of the un-frozen QuantAct (calibration / QAT range tracking) -----------------
 * x.data.min(), x.data.max() (quant_modules.py:233-236) of a fp32 tensor -> out2[0], out2[1] (device floats).
 * scratch: >= 8 bytes of device memory owned by the caller for the duration of the call. */
int hawq_minmax_f32(const float *x, int64_t n, float *out2, void *scratch, void *stream);
/* torch.kthvalue(x.view(-1), k).values (negate = 0) or -torch.kthvalue(-x.view(-1), k).values ... i.e. the k-th
 * smallest (1-based) element of x, or of -x returned with the sign of get_percentile_min_max's use
 * (quant_utils.py:38-70: `lower_bound = -torch.kthvalue(-input, k=lower_index).values`): out[0] = negate ? -kth(-x) : kth(x).
 * Exact (radix select on the order-preserving integer image of the floats).  scratch: >= 1040 bytes of device memory. */
int hawq_kthvalue_f32(const float *x, int64_t n, int64_t k, int32_t negate, float *out, void *scratch, void *stream);

/* ---- InceptionV3 (inception.hip) -----------------------------------------------------------
 * Rectangular implicit-GEMM conv on int8 MFMA: KH, KW in 1..7 with their own padding, stride 1 or 2, any H / W.
 * in:   int8 NHWC [N][H][W][Cin], Cin % 16 == 0 (4-bit activations travel in int8 containers)
 * wgt:  int8 [Cout][KH][KW][Cin], Cout % 16 == 0;  bias: int32 [Cout]
 * Output pixel p = (n * Ho + oy) * Wo + ox, channel co goes to out[p * ldo + c_off + co] (ldo >= c_off + Cout), so a branch
 * writes its slice of the unit's concat buffer in place; other channels of the row are never touched.
 *   HAWQ_INCEP_RAW:      int32 acc + bias
 *   HAWQ_INCEP_REQUANT:  q = clamp(dyadic(relu ? max(acc + bias, 0) : acc + bias; m[co], ek[co]), q_lo, q_hi)
 *   HAWQ_INCEP_REQUANT2: then q2 = clamp(dyadic(q; m2, ek2), q2_lo, q2_hi)  (a branch output rescaled to the concat scale)
 * REQUANT* store int8 (out_bits 8) or int16 (out_bits 16).  (m, ek) as in the conv epilogues (common.h dyadic_rne). */
#define HAWQ_INCEP_RAW 0
#define HAWQ_INCEP_REQUANT 1
#define HAWQ_INCEP_REQUANT2 2
typedef struct hawq_incep_conv_args {
    const void *in;
    const void *wgt;
    const int32_t *bias;
    int32_t N, H, W, Cin, Cout, KH, KW, stride, pad_h, pad_w;
    int32_t epilogue, relu;
    const int32_t *m;
    const int32_t *ek;
    int32_t q_lo, q_hi, m2, ek2, q2_lo, q2_hi;
    void *out;
    int32_t out_bits, ldo, c_off, reserved;
} hawq_incep_conv_args;
int hawq_incep_conv(const hawq_incep_conv_args *a, void *stream);
/* LDS-tiled kernels for the same launch (incep_tiled.hip): both operand tiles staged through a two-stage LDS ring (K steps of 64
 * bytes per row, K = taps x Cin walked in 16-channel units), several 32 x 32 MFMA tiles per wave, 16-byte stores.  Same argument
 * block, same integers: every tile id computes, byte for byte, what hawq_incep_conv computes.
 *   hawq_incep_conv_num_tiles: T; tile ids 1 .. T exist (1: 128 px x 128 ch, 2: 256 x 64, 3: 128 x 64, 4: 64 x 32 with the K steps
 *       split between two wave sets), id 0 is hawq_incep_conv's kernel.
 *   hawq_incep_conv_tile_ok:   1 if that tile takes this launch.  Host arithmetic on the argument block only: no pointer is
 *       dereferenced, nothing is launched, no device is needed.  0 for ids outside 0 .. T and for every block hawq_incep_conv
 *       refuses; ids > 0 also need out, in and wgt 16-byte aligned with ldo and c_off multiples of 16, tile 1 Cout > 64 and tile 4
 *       KH * KW * Cin >= 512.
 *   hawq_incep_conv_tiled:     the launch; tile 0 is hawq_incep_conv(a, stream).  A refused tile returns an error (the reason in
 *       hawq_last_error()), launches nothing and writes no byte of out. */
int hawq_incep_conv_num_tiles(void);
int hawq_incep_conv_tile_ok(const hawq_incep_conv_args *a, int tile);
int hawq_incep_conv_tiled(const hawq_incep_conv_args *a, int tile, void *stream);
/* Grouped launch of the tiled kernels (incep_group.hip): up to HAWQ_INCEP_GROUP_MAX independent convs - the sibling convs at one depth
 * of an Inception unit's branches - in ONE launch.  Members keep their own argument blocks and may differ in everything a block holds;
 * only the grid is shared: a 1-D grid in which member i owns ceil(P_i / BM) * ceil(Cout_i / BN) consecutive workgroups of tile `tile`
 * (one id in 1 .. hawq_incep_conv_num_tiles() for the whole group).  Each workgroup runs the tiled kernel's own body on its member.
 *   hawq_incep_conv_group:     writes, byte for byte, what hawq_incep_conv_tiled(&g->conv[i], tile, stream) for i = 0 .. n - 1 write.
 *   hawq_incep_conv_group_ok:  1 if the launch takes this group.  Host arithmetic only: nothing is dereferenced or launched, no device
 *       is needed.  0 for n outside 1 .. 8, a tile outside 1 .. T, a member hawq_incep_conv_tile_ok(member, tile) refuses, 2^31 or more
 *       workgroups in all, and for members that are not independent: two that write intersecting channel intervals
 *       [c_off, c_off + Cout) of one buffer (same out, ldo, element width) or intersecting byte extents of different buffers, or one
 *       whose input bytes intersect any member's output bytes.
 * A refused group makes hawq_incep_conv_group return non-zero (the reason in hawq_last_error()), launch nothing and write no byte.
 * conv[n .. 7] are ignored. */
#define HAWQ_INCEP_GROUP_MAX 8
typedef struct hawq_incep_group_args {
    int32_t n, reserved;
    hawq_incep_conv_args conv[HAWQ_INCEP_GROUP_MAX];
} hawq_incep_group_args;
int hawq_incep_conv_group_ok(const hawq_incep_group_args *g, int tile);
int hawq_incep_conv_group(const hawq_incep_group_args *g, int tile, void *stream);
/* The grouped launch with a fan-out epilogue (incep_fan.hip).  In the InceptionV3 plan every conv branch of a unit starts by
 * requantising the previous unit's whole 16-bit concat buffer to int8 at the branch's scale (hawq_incep_requant, one launch per
 * branch).  The convs that wrote that buffer held those values in registers; here they store the int8 copies themselves.
 *   hawq_incep_conv_group_fan:    member i writes, byte for byte, what hawq_incep_conv_tiled(&g->conv[i], tile, stream) writes.  In
 *       addition, for j < fan[i].n, output pixel p and channel co of member i,
 *           to[j].out[p * ldo + c_off + co] = (int8) clamp(dyadic_rne(y; m, ek), lo, hi)
 *       where y is the element the member stores as its primary output, after its last clamp - what hawq_incep_requant with
 *       post = (m, ek, lo, hi) makes of that element.  Other channels of a fan row are never touched.  A single conv with a fan is a
 *       group of one.  Tile ids 1 .. hawq_incep_conv_num_tiles(); the fan descriptors travel as kernel arguments (2312 bytes in all).
 *   hawq_incep_conv_group_fan_ok: 1 if the launch takes this description.  Host arithmetic only: nothing is dereferenced or launched,
 *       no device is needed.  It needs hawq_incep_conv_group_ok(g, tile); every fan[i].n in 0 .. HAWQ_INCEP_FAN_MAX; no fan on a RAW
 *       member; -128 <= lo <= hi <= 127; m >= 0 and ek = e | k << 8 with 1 <= e <= 62, k <= 15 (common.h dyadic_rne); out 16-byte
 *       aligned, ldo and c_off multiples of 16, ldo >= c_off + Cout of the member; and no fan output that meets a member's input, a
 *       member's primary output or another fan output - channel intervals for slices of one buffer (same out and ldo, int8), byte
 *       extents otherwise.
 * fan points to g->n entries.  A refused call returns non-zero (the reason in hawq_last_error()), launches nothing, writes nothing.
 * Not covered: tile 0, 16-bit fan outputs, fans of the pool kernels. */
#define HAWQ_INCEP_FAN_MAX 4
typedef struct hawq_incep_fan_out {
    void *out;   /* int8 rows of ldo elements */
    int32_t m, ek, lo, hi, ldo, c_off;
} hawq_incep_fan_out;
typedef struct hawq_incep_fan {
    int32_t n, reserved;
    hawq_incep_fan_out to[HAWQ_INCEP_FAN_MAX];
} hawq_incep_fan;
int hawq_incep_conv_group_fan_ok(const hawq_incep_group_args *g, const hawq_incep_fan *fan /* [g->n] */, int tile);
int hawq_incep_conv_group_fan(const hawq_incep_group_args *g, const hawq_incep_fan *fan, int tile, void *stream);
/* InceptionV3's input QuantAct + Conv2d_1a_3x3 from uint8 images in one launch (incep_stem.hip): Q_InceptInitBlock's q_input_activ and
 * q_conv1 (q_inceptionv3.py of the reference) on the tensor that ToTensor + Normalize (quant_train.py:432-440) make of the image, with
 * the QuantAct as a table look-up (quant_modules.py:271-274; lut int8 [3][256] from hawq_amd.quant_utils.input_quant_lut).
 * x:    uint8 NHWC [N][H][W][3], H, W >= 3
 * conv: in = NULL, Cin = 3, KH = KW = 3, stride 2, pad 0, Cout % 16 == 0; wgt int8 [Cout][32] with k = (kh * 3 + kw) * 3 + c for
 *       k < 27 and zeros for k = 27 .. 31 (16-byte aligned); epilogue HAWQ_INCEP_REQUANT with out_bits 8, exactly hawq_incep_conv's;
 *       output pixel p = (n * Ho + oy) * Wo + ox, Ho = (H - 3) / 2 + 1, channel co at out[p * ldo + c_off + co] (out 16-byte
 *       aligned, ldo and c_off multiples of 16); other channels of a row are never touched.
 * hawq_incep_stem_u8_ok: 1 when the launch takes this description. */
int hawq_incep_stem_u8(const uint8_t *x, const int8_t *lut, const hawq_incep_conv_args *conv, void *stream);
int hawq_incep_stem_u8_ok(const uint8_t *x, const int8_t *lut, const hawq_incep_conv_args *conv);
/* The same from fp32 images in one launch (incep_stem_f32.hip): Q_InceptInitBlock's q_input_activ (quant_modules.py:271-274, the
 * input case of quant_utils.py:73-97) and q_conv1 on the fp32 NCHW tensor itself.  It writes, byte for byte, what hawq_fakequant_f32
 * (scale 1.0) + hawq_f32_nchw_to_q_nhwc (Cpad 16, scale 1.0) + hawq_incep_conv write into conv1's output.
 * x:    fp32 NCHW [N][3][H][W], H, W >= 3, 4-byte aligned;  q = (int) fminf(fmaxf(rintf(inv_scale * x), in_lo), in_hi) in binary32
 *       (round half to even; -128 <= in_lo <= in_hi <= 127, inv_scale finite and > 0)
 * conv: exactly hawq_incep_stem_u8's description: in = NULL, Cin = 3, the [Cout][32] weight rows, REQUANT with out_bits 8.
 * A workgroup stages 9 input rows x 320 columns of quantised pixels in LDS (each input value is read and quantised once), then one
 * v_mfma_i32_32x32x32_i8 per 32 pixels x 32 channels.  Other channels of an output row are never touched.
 * hawq_incep_stem_f32_ok: 1 when the launch takes this description (host arithmetic only; nothing is launched or dereferenced). */
int hawq_incep_stem_f32(const float *x, float inv_scale, int32_t in_lo, int32_t in_hi, const hawq_incep_conv_args *conv, void *stream);
int hawq_incep_stem_f32_ok(const float *x, float inv_scale, int32_t in_lo, int32_t in_hi, const hawq_incep_conv_args *conv);
/* Average pool 3x3 / stride 1 / pad 1 of QuantAveragePool2d (count_include_pad: divisor 9 everywhere) on the fp32 (integer *
 * scale) NCHW tensor of the module path: x_int = rint(x / scale), s = sum of the window, p = trunc(s / 9 + 0.01) computed
 * exactly as (100 s + 9) / 900 in C integer division (truncation toward zero), y = p * scale. */
int hawq_avgpool3x3_f32(const float *x, float *y, int32_t NC, int32_t H, int32_t W, float scale, void *stream);

/* Integer NHWC pool / requant launches of the fused InceptionV3 plan (hawq_amd/engine_inception.py).  Every input element
 * first goes through the optional `pre` requant, every output element through the optional `post` requant:
 *   q = clamp(dyadic(v; m, ek), lo, hi)   (per tensor; (m, ek) as in the conv epilogues, k = 0)
 * in:  int8 / int16 (in_bits) [N][H][W] rows of in_pitch elements, channels in_off .. in_off + C - 1
 * out: int8 / int16 (out_bits) rows of ldo elements, channels c_off .. c_off + C - 1; other channels are never touched.
 *   hawq_incep_requant:         elementwise (Ho, Wo = H, W)
 *   hawq_incep_maxpool3s2:      max over 3 x 3 windows, stride 2, no padding
 *   hawq_incep_avgpool_branch:  3 x 3 / stride 1 / pad 1 window sum s (zeros in the padding), p = (100 s + 9) / 900
 *   hawq_incep_global_avgpool:  H x W window (one output pixel per image), p = (100 s + HW) / (100 HW)
 * (the average rules are trunc(s / d + 0.01) of QuantAveragePool2d, C division truncating toward zero) */
typedef struct hawq_incep_pool_args {
    const void *in;
    void *out;
    int32_t N, H, W, C, in_bits, in_pitch, in_off, out_bits, ldo, c_off;
    int32_t pre, m1, ek1, lo1, hi1;
    int32_t post, m2, ek2, lo2, hi2;
} hawq_incep_pool_args;
int hawq_incep_requant(const hawq_incep_pool_args *a, void *stream);
int hawq_incep_maxpool3s2(const hawq_incep_pool_args *a, void *stream);
int hawq_incep_avgpool_branch(const hawq_incep_pool_args *a, void *stream);
int hawq_incep_global_avgpool(const hawq_incep_pool_args *a, void *stream);
/* The same launches on vectorised kernels (hawq_amd/csrc/incep_pool.hip): a lane owns 16 consecutive channels of a pixel and moves
 * them with 16-byte loads and stores; the average pool stages its pre-requantised tile in LDS, the max pool applies `pre` once after
 * the max, the global pool splits the pixels of an image over lanes.  hawq_incep_pool_v writes exactly the bytes the op's entry point
 * above writes for the same argument block.  hawq_incep_pool_v_ok: 1 when hawq_incep_pool_v takes this launch (it launches nothing):
 * C, in_pitch, in_off, ldo and c_off multiples of 16, in / out 16-byte aligned, and per op
 *   MAX3S2 with pre: m1 >= 0, k = 0, e1 >= in_bits (pre is then monotone, so it commutes with the max);
 *   AVG3 with pre:   lo1, hi1 inside int16 (the staged tile is int16);
 *   GLOBAL:          100 * H * W * max|summand| + H * W < 2^31 (int32 average rule).
 * On a refused description hawq_incep_pool_v returns non-zero, sets hawq_last_error() and launches nothing. */
enum { HAWQ_INCEP_POOL_REQUANT = 0, HAWQ_INCEP_POOL_MAX3S2 = 1, HAWQ_INCEP_POOL_AVG3 = 2, HAWQ_INCEP_POOL_GLOBAL = 3 };
int hawq_incep_pool_v_ok(const hawq_incep_pool_args *a, int op);
int hawq_incep_pool_v(const hawq_incep_pool_args *a, int op, void *stream);
/* the workgroup tile (th rows x tw columns of output pixels, x 32 channels) hawq_incep_pool_v uses for this AVG3 description (it
 * depends on the map and, through the workgroup count, on N and C); non-zero with hawq_last_error() on a refused description */
int hawq_incep_pool_v_avg3_tile(const hawq_incep_pool_args *a, int32_t *th, int32_t *tw);

/* ---- hipGraph helpers: capture a sequence of the launches above once, replay per batch */
int hawq_graph_begin(void *stream);
int hawq_graph_end(void *stream, void **graph_exec_out);
int hawq_graph_launch(void *graph_exec, void *stream);
int hawq_graph_destroy(void *graph_exec);

/* ---- timing helper for bench.py: HIP events on the caller's stream ---------------------- */
int hawq_event_create(void **ev);
int hawq_event_record(void *ev, void *stream);
int hawq_event_elapsed_ms(void *ev_start, void *ev_stop, float *ms);
int hawq_event_destroy(void *ev);

/* ---- batched baseline JPEG decode (hawq_amd/csrc/jpeg_decode.hip, hawq_amd/jpeg.py; DESIGN.md "Device JPEG decode") -----------
 * One blob holds everything the kernels read: a header, one descriptor per image, the wave list of the entropy stage, and per image
 * the quantisation tables (64 x uint16, zig-zag order as stored in DQT), the Huffman tables, the entropy-coded bytes and the restart
 * intervals.  Every *_off below is a byte offset into the blob.  Accepted: baseline sequential, 8-bit, one interleaved scan; three
 * components with luma sampling hs x vs in {1x1, 2x1, 2x2} and chroma 1x1, or one component.
 * Output: the bytes of libjpeg-turbo's ISLOW IDCT + fancy upsampling + YCbCr->RGB, tight uint8 [height][width][3] at out_off. */
enum {
    HAWQ_JPEG_OK = 0,
    HAWQ_JPEG_EOF = 1,      /* the interval ran out of bytes */
    HAWQ_JPEG_CODE = 2,     /* a bit pattern that is no code of the table (or a DC category above 15) */
    HAWQ_JPEG_INDEX = 3,    /* an AC run went past coefficient 63 */
    HAWQ_JPEG_MARKER = 4    /* FF xx (xx != 00) inside an interval */
};
typedef struct hawq_jpeg_batch_hdr {   /* at offset 0 of the blob */
    int32_t n_images, n_waves;
    int32_t desc_off, wave_off;        /* hawq_jpeg_desc[n_images], hawq_jpeg_wave[n_waves]; 16-byte aligned */
} hawq_jpeg_batch_hdr;
typedef struct hawq_jpeg_wave {        /* one wave of the entropy stage: one restart interval of one image; image-major, in order */
    int32_t image, interval;
} hawq_jpeg_wave;
/* Canonical Huffman table (JPEG F.2.2.3): codes of length l are mincode[l] .. maxcode[l] (maxcode[l] = -1: none), the value of code c
 * of length l is huffval[valptr[l] + c - mincode[l]].  Index 0 of the three arrays is unused. */
typedef struct hawq_jpeg_huff {
    int32_t mincode[17], maxcode[17], valptr[17];
    uint8_t huffval[256];
    int32_t reserved;
} hawq_jpeg_huff;                      /* 464 bytes */
typedef struct hawq_jpeg_desc {
    int32_t width, height, ncomp;      /* ncomp 1 (Y, written as R = G = B) or 3 (Y, Cb, Cr) */
    int32_t hs, vs;                    /* luma sampling factors; chroma is 1 x 1 */
    int32_t mcus_x, mcus_y;            /* ceil(width / (8 hs)), ceil(height / (8 vs)) */
    int32_t restart;                   /* MCUs per restart interval, 0: the whole scan is one interval */
    int32_t n_intervals;               /* ceil(mcus / restart), 1 without DRI */
    int32_t qt_off[3], dc_off[3], ac_off[3];   /* per component: uint16[64], hawq_jpeg_huff, hawq_jpeg_huff */
    int32_t stream_off, stream_len;    /* the entropy-coded segment */
    int32_t interval_off;              /* int32 [n_intervals][2]: first byte and one past the last, relative to stream_off */
    int32_t scale;                     /* 0 or 1: full size.  2, 4, 8: the reduced decode of libjpeg's DCT-domain scaling (Pillow's
                                          draft mode): stages 2 and 3 produce ceil(width / scale) x ceil(height / scale) pixels from
                                          n x n inverse DCTs, n = 8 / scale per block side (2 n for the chroma of a 2 x 2 image) */
    int64_t coef_block0;               /* first [64] x int16 block of this image in the coefficient slab: component after component,
                                          each mcus_y * v rows of mcus_x * h blocks */
    int64_t plane_off;                 /* first byte of this image's sample planes: component after component, pitch mcus_x * h * n,
                                          n = 8 at full size */
    int64_t out_off;                   /* first byte of the RGB image in out; 16-byte aligned */
} hawq_jpeg_desc;                      /* 112 bytes */
/* hawq_jpeg_batch_ok launches nothing and reads the HOST blob: 1 when the header, every descriptor, table, stream and interval lies
 * inside blob_bytes at its alignment, the geometry is one of the accepted ones and block counts follow from it, every image's range of
 * the slab / planes / out lies inside coef_blocks / plane_bytes / out_bytes behind the previous image's, every interval lies inside its
 * stream, and the wave list names every (image, interval) once in order; else 0 with the reason in hawq_last_error().
 * hawq_jpeg_decode_batch: blob = device copy of host_blob (which it checks again before it launches anything).  Zeroes coef and status
 * on `stream`, then entropy decode (one wave per entry of the wave list) -> coef, dequantise + IDCT -> planes, upsample + colour -> out.
 * status[i]: 0, or the HAWQ_JPEG_* error of one of image i's intervals (which one is not defined): its pixels are not to be used.
 * events: NULL, or four hipEvent_t recorded before stage 1 and behind stages 1, 2 and 3. */
int hawq_jpeg_batch_ok(const void *host_blob, int64_t blob_bytes, int64_t coef_blocks, int64_t plane_bytes, int64_t out_bytes);
int hawq_jpeg_decode_batch(const void *blob, const void *host_blob, int64_t blob_bytes, int16_t *coef, int64_t coef_blocks, uint8_t *planes,
                           int64_t plane_bytes, uint8_t *out, int64_t out_bytes, int32_t *status, void *const *events, void *stream);

/* ---- the same decode with many lanes per long restart interval (jpeg_sync.h) ------------------------------------
 * Intervals of at least min_sync_bytes stream bytes are cut into n_sub = ceil(bytes / sub_bytes) sub-sequences, decoded speculatively by
 * one lane each and synchronised until every lane starts where the lane before it ended; shorter intervals run on the serial wave of
 * hawq_jpeg_decode_batch in the same call.  Same coefficients, same status, same output bytes.
 * The job table lies in the blob at jobs_off (16-byte aligned): one entry per long interval, in the order of the wave list.  Scratch
 * is device memory of scratch_bytes; a job's slice is one hawq_jpeg_sync_job_hdr and n_sub hawq_jpeg_sync_sub. */
enum { HAWQ_JPEG_SYNC_SUB_MIN = 16, HAWQ_JPEG_SYNC_SUB_MAX = 4096 };   /* sub_bytes: a multiple of 4 in this range */
typedef struct hawq_jpeg_sync_job {
    int32_t wave;                      /* index into the wave list */
    int32_t n_sub;                     /* ceil(interval bytes / sub_bytes) */
    int64_t scratch_off;               /* 16-byte aligned; 16 + 32 * n_sub bytes behind the previous job's */
} hawq_jpeg_sync_job;                  /* 16 bytes */
typedef struct hawq_jpeg_sync_job_hdr {/* written by the kernel at scratch_off */
    int32_t rounds;                    /* decode passes until no lane's start changed: 1 (speculation) .. n_sub */
    int32_t decodes;                   /* sub-sequence decodes of all of them */
    int32_t reserved[2];
} hawq_jpeg_sync_job_hdr;              /* 16 bytes */
typedef struct hawq_jpeg_sync_sub {    /* one sub-sequence; a state is (byte relative to the stream, bit | u << 8 | k << 16), byte < 0: none */
    int32_t start_pos, start_uk;       /* the state it last decoded from */
    int32_t end_pos, end_uk;           /* the state behind its last symbol */
    int32_t blocks;                    /* blocks that end in it; after the scan: ordinal of its first block in the interval */
    int32_t dc[3];                     /* sum of its DC differences per component; after the scan: the predictors at its start */
} hawq_jpeg_sync_sub;                  /* 32 bytes */
/* hawq_jpeg_sync_ok launches nothing and reads the HOST blob, which hawq_jpeg_batch_ok has passed: 1 when sub_bytes is a multiple of 4
 * in [HAWQ_JPEG_SYNC_SUB_MIN, HAWQ_JPEG_SYNC_SUB_MAX], min_sync_bytes >= 1, the job table lies inside the blob and names exactly the
 * waves whose interval has at least min_sync_bytes bytes, in order, each with its n_sub and a scratch slice inside scratch_bytes behind
 * the previous job's; else 0 with the reason in hawq_last_error().
 * hawq_jpeg_decode_batch_sync runs both checks again, then works as hawq_jpeg_decode_batch; stage 1 is the serial kernel (which leaves
 * the long intervals out) and one workgroup per job.  events as there: the second one is recorded behind both stage-1 launches. */
int hawq_jpeg_sync_ok(const void *host_blob, int64_t blob_bytes, int32_t sub_bytes, int32_t min_sync_bytes, int64_t jobs_off, int32_t n_jobs,
                      int64_t scratch_bytes);
int hawq_jpeg_decode_batch_sync(const void *blob, const void *host_blob, int64_t blob_bytes, int16_t *coef, int64_t coef_blocks, uint8_t *planes,
                                int64_t plane_bytes, uint8_t *out, int64_t out_bytes, int32_t *status, int32_t sub_bytes, int32_t min_sync_bytes,
                                int64_t jobs_off, int32_t n_jobs, void *scratch, int64_t scratch_bytes, void *const *events, void *stream);

/* ---- progressive JPEGs (SOF2, Huffman; hawq_amd/csrc/jpeg_prog.hip + jpeg_prog.h) --------------------------------
 * The blob begins as the baseline one: hawq_jpeg_batch_hdr, then hawq_jpeg_desc[n_images], whose entropy fields (dc_off, ac_off,
 * stream_off, stream_len, interval_off, restart, n_intervals) are zero; stages 2 and 3 read nothing else.  Behind the batch header, at
 * byte 16, stands a hawq_jpeg_prog_hdr.  The scan table lists the scans of image 0 in file order, then image 1's, ...  The wave list at
 * hawq_jpeg_batch_hdr.wave_off holds hawq_jpeg_prog_wave[n_waves], level after level: the waves of level L are
 * level_start[L - 1] .. level_start[L] - 1 (int32 level_start[n_levels + 1] at level_off), and within a level they name every interval
 * of every scan of that level, in the order of the scan table.
 * level(scan) = 1 + the largest level of the earlier scans of the same image that share a (component, coefficient) with it, 1 without
 * one: the scans of one level write disjoint int16 words, so one launch per level decodes them side by side.
 * An interleaved scan (ncomp = the image's) walks the image's MCUs as the baseline decoder does; a scan of one component walks that
 * component's own grid of ceil(ceil(width * h / hs) / 8) x ceil(ceil(height * v / vs) / 8) blocks in raster order (not the MCU-padded
 * grid of the slab), and its restart interval counts those blocks. */
enum { HAWQ_JPEG_PROG_MAX_SCANS = 64 };   /* per image; no progression has more levels than scans */
typedef struct hawq_jpeg_prog_hdr {    /* at byte 16 of the blob */
    int32_t n_scans, n_levels;
    int32_t scan_off;                  /* hawq_jpeg_scan[n_scans]; 16-byte aligned */
    int32_t level_off;                 /* int32 [n_levels + 1]; 16-byte aligned */
} hawq_jpeg_prog_hdr;
typedef struct hawq_jpeg_prog_wave {   /* one wave of the entropy stage: one restart interval of one scan */
    int32_t scan, interval;
} hawq_jpeg_prog_wave;
typedef struct hawq_jpeg_scan {
    int32_t image;
    int32_t ncomp, comp0;              /* components comp0 .. comp0 + ncomp - 1: one of them, or all (comp0 = 0) */
    int32_t ss, se, ah, al;            /* ss <= se <= 63, se = 0 when ss = 0, ncomp = 1 when ss > 0; al <= 13; ah = 0 or al + 1 */
    int32_t level;
    int32_t dc_off[3];                 /* hawq_jpeg_huff of the scan's i-th component: read when ss = 0 and ah = 0 */
    int32_t ac_off;                    /* hawq_jpeg_huff: read when ss > 0 */
    int32_t restart, n_intervals;      /* MCUs (blocks, in a scan of one component) per restart interval, 0: one interval */
    int32_t interval_off;              /* int32 [n_intervals][2], relative to stream_off */
    int32_t stream_off, stream_len;    /* this scan's entropy-coded segment; 16-byte aligned */
    int32_t reserved[3];
} hawq_jpeg_scan;                      /* 80 bytes */
/* hawq_jpeg_prog_ok launches nothing and reads the HOST blob: 1 when every offset and length lies inside the blob at its alignment, the
 * geometry is accepted, each scan's interval count follows from its grid, every interval lies inside its scan's stream, the Huffman
 * tables a scan reads are canonical, the scans of every image form a legal and COMPLETE progression (per component and coefficient: the
 * first scan has ah = 0, each later one ah = the previous al, DC before AC, al = 0 in the end), every scan's level is exactly the one
 * the rule above gives, the wave lists are as described, and the slab / plane / output slices are disjoint and in bounds; else 0 with
 * the reason in hawq_last_error().
 * hawq_jpeg_decode_batch_prog checks again, zeroes coef and status, launches one entropy grid per level on `stream` and then stages 2
 * and 3 of hawq_jpeg_decode_batch.  status and events as there; the second event is recorded behind the last level. */
int hawq_jpeg_prog_ok(const void *host_blob, int64_t blob_bytes, int64_t coef_blocks, int64_t plane_bytes, int64_t out_bytes);
int hawq_jpeg_decode_batch_prog(const void *blob, const void *host_blob, int64_t blob_bytes, int16_t *coef, int64_t coef_blocks, uint8_t *planes,
                                int64_t plane_bytes, uint8_t *out, int64_t out_bytes, int32_t *status, void *const *events, void *stream);

/* ---- long restart intervals from recorded resume points (hawq_amd/csrc/jpeg_resume.h + jpeg_resume.hip) --------------
 * A resume point is the state in which the serial decoder starts a unit of a restart interval (an MCU; a block in a scan of one
 * component): the unit's index in the interval, the canonical byte and bit of the next unread bit (jpeg_sync.h), the DC predictors and
 * EOBRUN.  Points cut an interval into segments, and a segment is decoded by a wave of its own, as a restart interval with a start bit
 * and a start state.  The blobs are those of hawq_jpeg_decode_batch / _prog with a segment table behind the existing parts: every wave
 * of the wave list has one segment or more, the segments stand in the order of the wave list, and those of one wave partition its units
 * in order. */
typedef struct hawq_jpeg_resume_seg {
    int32_t wave;                      /* index into the wave list: (image, interval), or (scan, interval) in a progressive blob */
    int32_t unit0, n_units;            /* units unit0 .. unit0 + n_units - 1 of the interval, unit0 counted from the interval's first */
    int32_t byte, bit;                 /* the next unread bit: bit 0..7 (0 = first) of the data byte at `byte`, relative to the stream */
    int32_t eobrun;                    /* 0..32767; 0 outside an AC scan */
    int32_t pred[3];                   /* 0 outside a baseline image or a first DC pass, and for components the scan does not have */
    int32_t reserved;
} hawq_jpeg_resume_seg;                /* 40 bytes */
/* hawq_jpeg_resume_record needs no device.  host_blob: a blob hawq_jpeg_batch_ok (progressive = 0) or hawq_jpeg_prog_ok (1) passes.  It
 * runs the serial decoders on the host, a progressive image scan after scan into a slab of its own, and writes the segments of every
 * wave to segs, in the order of the wave list: a new segment begins at the first unit boundary that lies at least `every` (>= 1) stream
 * bytes behind the start of the segment before it, and none begins behind the first decode error of an interval.  *n_segs: how many
 * there are; more than max_segs is an error (n_waves + sum over the intervals of bytes / every is always enough).
 * hawq_jpeg_resume_ok launches nothing and reads the HOST blob, which the checker of its kind has passed: 1 when the table lies inside
 * the blob at a 16-byte aligned offset, every wave has its segments in order, they partition its units in order with at least one unit
 * each, the first one starts at the interval's first byte, bit 0, with a zero state, every later one at a byte inside the interval that
 * is not smaller than its predecessor's, with bit in 0..7 and eobrun in 0..32767, and eobrun / pred are zero where the comments above
 * say so; else 0 with the reason in hawq_last_error().
 * hawq_jpeg_decode_batch_resume / _prog_resume run the checker of the kind and hawq_jpeg_resume_ok again, then work as
 * hawq_jpeg_decode_batch / _prog with one wave per segment in stage 1.  Same coefficients, same status, same output bytes, when the
 * points are those of the blob's streams; with any other table that passes the check every store still goes to a block of the
 * segment's own units. */
int hawq_jpeg_resume_record(const void *host_blob, int64_t blob_bytes, int32_t progressive, int32_t every, hawq_jpeg_resume_seg *segs, int64_t max_segs,
                            int64_t *n_segs);
int hawq_jpeg_resume_ok(const void *host_blob, int64_t blob_bytes, int32_t progressive, int64_t segs_off, int64_t n_segs);
int hawq_jpeg_decode_batch_resume(const void *blob, const void *host_blob, int64_t blob_bytes, int16_t *coef, int64_t coef_blocks, uint8_t *planes,
                                  int64_t plane_bytes, uint8_t *out, int64_t out_bytes, int32_t *status, int64_t segs_off, int64_t n_segs, void *const *events,
                                  void *stream);
int hawq_jpeg_decode_batch_prog_resume(const void *blob, const void *host_blob, int64_t blob_bytes, int16_t *coef, int64_t coef_blocks, uint8_t *planes,
                                       int64_t plane_bytes, uint8_t *out, int64_t out_bytes, int32_t *status, int64_t segs_off, int64_t n_segs,
                                       void *const *events, void *stream);

/* ---- the front end of the baseline decoder on the device (hawq_amd/csrc/jpeg_front.h + jpeg_front.hip) ----------------
 * The raw files of a batch lie in one buffer, file i at table[i].offset (16-byte aligned) with table[i].length bytes.  The scan walks
 * the headers of every file, checks the restart markers of its entropy-coded segment and writes one hawq_jpeg_front_info per file; the
 * fill writes an accepted file's tables, restart intervals and stream into the blob of hawq_jpeg_decode_batch.  A file the walker does
 * not take gets a defer code and nothing else; the caller hands it to hawq_amd.jpeg.parse_jpeg, which accepts or refuses it. */
enum {
    HAWQ_JPEG_FRONT_OK = 0,
    HAWQ_JPEG_FRONT_REFUSED = 1,       /* not a baseline file of the accepted kind, or malformed: parse_jpeg refuses it too */
    HAWQ_JPEG_FRONT_LONG_HEADER = 2,   /* more than HAWQ_JPEG_FRONT_MAX_SEGMENTS marker segments before the scan */
    HAWQ_JPEG_FRONT_TOO_LARGE = 3      /* more than HAWQ_JPEG_FRONT_MAX_BYTES bytes */
};
enum { HAWQ_JPEG_FRONT_MAX_SEGMENTS = 64, HAWQ_JPEG_FRONT_MAX_BYTES = 1 << 30 };
typedef struct hawq_jpeg_front_file {  /* one entry of the file table */
    int64_t offset, length;
} hawq_jpeg_front_file;
typedef struct hawq_jpeg_front_info {
    int32_t defer;                     /* HAWQ_JPEG_FRONT_*; every other field is zero unless it is HAWQ_JPEG_FRONT_OK */
    int32_t width, height, ncomp, hs, vs;
    int32_t restart, n_intervals;
    int32_t tq[3], td[3], ta[3];       /* per component: quantisation, DC and AC table id */
    int32_t qt_at[4];                  /* per quantisation table id: file offset of the 64 bytes in force at the SOS, 0: none */
    int32_t huff_at[4];                /* per DC id 0, 1, AC id 0, 1: file offset of BITS (16 counts, then the values), 0: none */
    int32_t scan_first, scan_end;      /* the entropy-coded segment: first byte, one past the last (where EOI stands) */
    int32_t reserved[5];
} hawq_jpeg_front_info;                /* 128 bytes */
typedef struct hawq_jpeg_front_place { /* where the fill writes one accepted file's share of the blob; every offset 16-byte aligned */
    int32_t file;                      /* index into the file table and the info records */
    int32_t qt_off[3], dc_off[3], ac_off[3];   /* per component: where its table goes, 0: an earlier component has placed it */
    int32_t interval_off, stream_off;
    int32_t reserved[4];
} hawq_jpeg_front_place;               /* 64 bytes */
/* hawq_jpeg_front_scan: files / table / info are device memory, host_table the host copy of table, which is checked before anything is
 * launched: every file 16-byte aligned, inside files_bytes, behind the one before it.  One wave per file on `stream`.
 * hawq_jpeg_front_scan_host: the same walker over host memory; no device.
 * hawq_jpeg_front_fill_ok launches nothing and reads host memory: 1 when every entry of host_place names a file of the table whose info
 * is accepted, every table, the scan and the restart count the info names lie inside that file, and every destination lies inside
 * blob_bytes at a 16-byte aligned offset behind the one before it (per file: per component its quantisation, DC and AC table where
 * placed, then the intervals, then the stream); else 0 with the reason in hawq_last_error().
 * hawq_jpeg_front_fill: info / place are the device copies of host_info / host_place.  It checks again, zeroes blob on `stream` and runs
 * one workgroup per entry: uint16[64] quantisation tables as stored, canonical hawq_jpeg_huff records, int32 [n_intervals][2] from the
 * RSTn markers between scan_first and scan_end, and the bytes of the scan.  Header, descriptors and wave list are the caller's. */
int hawq_jpeg_front_scan(const void *files, int64_t files_bytes, const hawq_jpeg_front_file *table, const hawq_jpeg_front_file *host_table, int32_t n_files,
                         hawq_jpeg_front_info *info, void *stream);
int hawq_jpeg_front_scan_host(const void *host_files, int64_t files_bytes, const hawq_jpeg_front_file *host_table, int32_t n_files, hawq_jpeg_front_info *host_info);
int hawq_jpeg_front_fill_ok(const hawq_jpeg_front_info *host_info, const hawq_jpeg_front_place *host_place, int32_t n, const hawq_jpeg_front_file *host_table,
                            int32_t n_files, int64_t files_bytes, int64_t blob_bytes);
int hawq_jpeg_front_fill(const void *files, int64_t files_bytes, const hawq_jpeg_front_file *table, const hawq_jpeg_front_file *host_table, int32_t n_files,
                         const hawq_jpeg_front_info *info, const hawq_jpeg_front_info *host_info, const hawq_jpeg_front_place *place,
                         const hawq_jpeg_front_place *host_place, int32_t n, void *blob, int64_t blob_bytes, void *stream);

/* ---- the same front end for progressive files (hawq_amd/csrc/jpeg_front_prog.h + jpeg_front.hip) ----------------------
 * hawq_jpeg_front_scan_prog walks a batch as hawq_jpeg_front_scan does and writes for a baseline file exactly the record that one
 * writes.  A file that one refuses is walked again as a progressive Huffman file (SOF2) inside the scope of
 * hawq_amd.jpeg.parse_progressive, baseline until its SOF2 as parse_jpeg(data, progressive=True) takes it.  An accepted progressive
 * file has in its hawq_jpeg_front_info: defer 0, the geometry, tq, qt_at, reserved[0] = HAWQ_JPEG_FRONT_KIND_PROG and reserved[1] = its
 * number of scans (1 .. HAWQ_JPEG_PROG_MAX_SCANS), every other word zero; and one hawq_jpeg_front_scan_rec per scan at
 * scans[file * HAWQ_JPEG_PROG_MAX_SCANS + k], every other record of the file zero.  Bounds of the kernel, beside those above: a
 * progressive file with more than HAWQ_JPEG_FRONT_PROG_MAX_SEGMENTS marker segments in all defers with HAWQ_JPEG_FRONT_LONG_HEADER - 64
 * before the first scan as above, and a DHT and a DRI in front of each of 64 scans behind it. */
enum { HAWQ_JPEG_FRONT_KIND_BASELINE = 0, HAWQ_JPEG_FRONT_KIND_PROG = 1 };
enum { HAWQ_JPEG_FRONT_PROG_MAX_SEGMENTS = 256 };
typedef struct hawq_jpeg_front_scan_rec {
    int32_t ncomp, comp0;              /* components comp0 .. comp0 + ncomp - 1 of the frame */
    int32_t ss, se, ah, al;
    int32_t level;                     /* as hawq_jpeg_scan.level, among the scans of this file */
    int32_t dc_at[3];                  /* file offset of BITS of the DC table in force at the SOS for the scan's i-th component when ss = 0
                                          and ah = 0, else 0 */
    int32_t ac_at;                     /* the same of the AC table when ss > 0, else 0 */
    int32_t restart, n_intervals;      /* in the scan's units, as hawq_jpeg_scan */
    int32_t scan_first, scan_end;      /* the entropy-coded segment: first byte, one past the last (where the next marker stands) */
    int32_t reserved;
} hawq_jpeg_front_scan_rec;            /* 64 bytes */
typedef struct hawq_jpeg_front_scan_place {   /* where the fill writes one scan's share of the progressive blob; offsets 16-byte aligned */
    int32_t file, scan;                /* index into the file table and the info records; the scan's index in that file */
    int32_t qt_off[3];                 /* in the first scan of a file, per component: where its quantisation table goes, 0: nowhere */
    int32_t dc_off[3], ac_off;         /* where the table at dc_at[i] / ac_at goes, 0: nowhere (an earlier scan has placed it, or none) */
    int32_t interval_off, stream_off;
    int32_t reserved[5];
} hawq_jpeg_front_scan_place;          /* 64 bytes */
/* hawq_jpeg_front_scan_prog: as hawq_jpeg_front_scan, with scans = device memory for n_files * HAWQ_JPEG_PROG_MAX_SCANS records, which
 * it zeroes on `stream` first.  One wave per file.  hawq_jpeg_front_scan_prog_host: the same walker over host memory; no device.
 * hawq_jpeg_front_fill_prog_ok launches nothing and reads host memory: 1 when every entry of host_place names a scan of an accepted
 * progressive file, in ascending order, every table it places and the scan's segment lie inside that file, and every destination lies
 * inside blob_bytes at a 16-byte aligned offset behind the one before it (per scan: quantisation tables, DC tables, AC table,
 * intervals, stream); else 0 with the reason in hawq_last_error().
 * hawq_jpeg_front_fill_prog checks again, zeroes blob on `stream` and runs one workgroup per entry, which writes what
 * hawq_jpeg_front_fill writes for a file.  Headers, descriptors, scan table, level list and wave lists are the caller's; the filled
 * blob is one hawq_jpeg_prog_ok must pass before hawq_jpeg_decode_batch_prog reads it. */
int hawq_jpeg_front_scan_prog(const void *files, int64_t files_bytes, const hawq_jpeg_front_file *table, const hawq_jpeg_front_file *host_table,
                              int32_t n_files, hawq_jpeg_front_info *info, hawq_jpeg_front_scan_rec *scans, void *stream);
int hawq_jpeg_front_scan_prog_host(const void *host_files, int64_t files_bytes, const hawq_jpeg_front_file *host_table, int32_t n_files,
                                   hawq_jpeg_front_info *host_info, hawq_jpeg_front_scan_rec *host_scans);
int hawq_jpeg_front_fill_prog_ok(const hawq_jpeg_front_info *host_info, const hawq_jpeg_front_scan_rec *host_scans, const hawq_jpeg_front_scan_place *host_place,
                                 int32_t n, const hawq_jpeg_front_file *host_table, int32_t n_files, int64_t files_bytes, int64_t blob_bytes);
int hawq_jpeg_front_fill_prog(const void *files, int64_t files_bytes, const hawq_jpeg_front_file *table, const hawq_jpeg_front_file *host_table,
                              int32_t n_files, const hawq_jpeg_front_info *info, const hawq_jpeg_front_info *host_info, const hawq_jpeg_front_scan_rec *scans,
                              const hawq_jpeg_front_scan_rec *host_scans, const hawq_jpeg_front_scan_place *place,
                              const hawq_jpeg_front_scan_place *host_place, int32_t n, void *blob, int64_t blob_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HAWQ_MI355_H */
