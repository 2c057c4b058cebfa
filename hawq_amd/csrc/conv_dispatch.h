// What the conv kernel families and the dispatcher of hawq_conv2d (conv_dispatch.hip) agree on.  Host code only.
#pragma once
#include "conv_device.h"

// Every predicate of an accepted launch, derived once by conv_check.
struct ConvForm {
    bool dual;          // second branch (identity conv) present
    bool fast;          // fast_tables != 0
    bool wide_res;      // RESIDUAL with a 32-bit res_in (single branch) or res_out
    bool signed_res;    // single-branch RESIDUAL without ReLU / clamped to int16 / without identity (ABI 3)
    bool all88, all44;  // operand widths of every branch
    bool needs_tables;  // REQUANT or RESIDUAL
    int slot;           // epilogue slot of the function tables: RAW, REQUANT, RESIDUAL, DEQUANT
};

// What conv_choose resolves: everything a launch needs besides the kernel arguments.
struct ConvChoice {
    int family, tile;      // index into kConvFamilies, resolved tile within the family
    int table, fn[3];      // the family's function table and the indices into it (-1: unused)
    int grid, block, lds;  // grid -1: sized by the CU count of the device at launch
    int ring_bytes;        // ConvP.ring_bytes of the plain tiles, else 0
};

// One kernel family: `count` consecutive tile ids.  choose is pure (no HIP call) and may refuse (HAWQ_REQUIRE); launch owns
// the once-per-process attribute static, the launch and the HAWQ_DBG bit-128 print.
struct ConvFamily {
    const char *name, *what;   // what: the words of "tile %d (%s) does not apply to this layer"
    int (*count)(void);
    const int *prefer;         // tiles tried in this order when the caller leaves the choice open for a planar layer; nullptr: never
    bool (*applies)(const hawq_conv_args *a, int v);
    int (*choose)(const hawq_conv_args *a, const ConvForm &f, const ConvP &p, ConvChoice &c);   // c.family, c.tile are set
    int (*launch)(const hawq_conv_args *a, const ConvChoice &c, const ConvP &p, void *stream);
};

#define CONV_FAMILY_DECL(F)                                                                        \
    int F##_count(void);                                                                           \
    bool F##_applies(const hawq_conv_args *a, int v);                                              \
    int F##_choose(const hawq_conv_args *a, const ConvForm &f, const ConvP &p, ConvChoice &c);     \
    int F##_launch(const hawq_conv_args *a, const ConvChoice &c, const ConvP &p, void *stream)
CONV_FAMILY_DECL(conv_igemm);     // conv_igemm.hip: the general tiles
CONV_FAMILY_DECL(band_v1);        // band_v1.hip: 3x3 band kernels
CONV_FAMILY_DECL(band_persist);   // band_persist.hip: weight-stationary 3x3 kernel, 1 / 2 workgroups per CU
CONV_FAMILY_DECL(band_v2);        // band_v2.hip: round-5 3x3 kernels
CONV_FAMILY_DECL(gemm_v2);        // gemm_v2.hip: round-5 streaming 1x1 kernels
extern const int kBandPreference[], kBandV2Preference[];
int conv_igemm_pick_tile(int M, int Cout, bool dual);
long long *conv_dbg_buffer(int dbg);   // ConvP.dbgbuf of a launch: the cycle-stamp buffer if HAWQ_DBG bit 128 is set, else nullptr

ConvForm conv_form(const hawq_conv_args *a);   // reads the struct only: valid for any non-null `a`
// Argument rules of hawq_conv2d and the ConvP fill; `who` prefixes the messages (hawq_conv2d_splitk calls this too).
int conv_check(const hawq_conv_args *a, const char *who, ConvForm *form, ConvP *p);
