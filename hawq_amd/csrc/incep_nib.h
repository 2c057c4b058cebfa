// What the two files of the nibble-packed InceptionV3 conv share (incep_nib.hip: one conv per launch, incep_group_nib.hip: up to eight
// convs of either operand form on one grid): the widening of hawq4 dwords to int8x4 MFMA operands.  The workgroup body is
// incep_nib_body.h, shared as text.
#pragma once
#include "common.h"

extern "C" int hawq_incep_conv_nib_ok(const hawq_incep_conv_args *a, int tile);

namespace {

constexpr int NIB_LO = 0x0f0f0f0f, NIB_HI = (int)0xf0f0f0f0u;
// one unit (dwords d0, d1 = channels 0 - 7, 8 - 15) -> the 16 int8 of an MFMA operand, in channel order
__device__ __forceinline__ v4i widen_act(int d0, int d1) {
    return v4i{d0 & NIB_LO, (int)((unsigned)d0 >> 4) & NIB_LO, d1 & NIB_LO, (int)((unsigned)d1 >> 4) & NIB_LO};
}
// 16 w per byte
__device__ __forceinline__ v4i widen_wgt(int d0, int d1) { return v4i{(d0 << 4) & NIB_HI, d0 & NIB_HI, (d1 << 4) & NIB_HI, d1 & NIB_HI}; }

}  // namespace
