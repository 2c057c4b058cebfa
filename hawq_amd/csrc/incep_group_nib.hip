// Mixed-form grouped launch of the InceptionV3 convs: one 1-D grid whose workgroups are dealt out to up to HAWQ_INCEP_GROUP_MAX
// independent convs, each of which reads either int8 operands (the tiled kernel's, incep_tiled.hip) or hawq4 operands (the nibble
// kernel's, incep_nib.hip) - the sibling convs at one depth of a unit's branches in a plan that keeps some tensors on nibbles.
//   hawq_incep_conv_group_nib_num_tiles   T: tile ids 1 .. T are the kernels below
//   hawq_incep_conv_group_nib_ok          host arithmetic only: is this a group, with this mask, tile `tile` can run in one launch
//   hawq_incep_conv_group_nib             the launch: member i writes, byte for byte, what its single launch on that shape writes
// Grid and member selection are incep_group.hip's (incep_tile.h: GroupMap, group_member, group_grid): running totals by value, pixel
// blocks fastest, members that keep their own argument blocks.  Bit i of `mask`, passed by value beside them, says that member i's
// in and wgt are hawq4.  Member index, mask bit and argument block are functions of the workgroup id and the kernel arguments, so
// the choice between the two bodies is a scalar branch and the descriptor arrives through scalar loads from the kernarg segment.
//
// Why one workgroup shape serves both.  The two families stage the same bytes: BM + BN rows of 64 bytes per stage, two stages,
// rows XOR-swizzled by lds_off, weight rows in cperm order, fragments read as 16-byte slots by lane (l31, h), and the same
// lane-owns-16-channels epilogue.  They differ in what a staging thread owns (a 16-byte slot = 16 int8 channels, four a row, against
// an 8-byte unit = 16 nibble channels, eight a row: 64 and 128 K values per step) and in the widening in front of the MFMA.  So both
// bodies run on the same `lds` array with the same wave layout, and the kernel's LDS is that of either parent: 32 KiB for tile 1,
// 24 KiB for tile 2.  The bodies are the parents' texts (incep_tile_body.h, incep_nib_body.h); neither is called from the other.
//
// Tiles: the shapes both families have with one wave set (KS = 1).  The K-split shapes differ (64 px x 32 ch against 64 x 64) and
// are left out.
#include "incep_group_nib.h"

namespace {

// the tiled kernel's workgroup body on an int8 member, as incep_group.hip runs it
template <int BM, int BN, int WPX, int WCH, int KS>
__device__ __forceinline__ void gn_int8_body(const hawq_incep_conv_args &a, const int Ho, const int Wo, const long long pblock,
                                             const int cblock, char *lds) {
#define INCEP_TILE_BLOCK
#define INCEP_TILE_STORED(p, cb, q)
#include "incep_tile_body.h"
#undef INCEP_TILE_BLOCK
#undef INCEP_TILE_STORED
}

// the nibble kernel's workgroup body on a hawq4 member
template <int BM, int BN, int WPX, int WCH, int KS>
__device__ __forceinline__ void gn_nib_body(const hawq_incep_conv_args &a, const int Ho, const int Wo, const long long pblock,
                                            const int cblock, char *lds) {
#define INCEP_NIB_BLOCK
#define INCEP_NIB_STORED(p, cb, q)
#include "incep_nib_body.h"
#undef INCEP_NIB_BLOCK
#undef INCEP_NIB_STORED
}

// The occupancy floor is the parents': 3 waves per SIMD on tile 1 (64 accumulator registers a lane), 4 on tile 2.  The two bodies
// never run in one workgroup, so the kernel needs the registers of the larger one; the floor keeps the allocator from spending
// more than that on the join of the two.
template <int BM, int BN, int WPX, int WCH>
__global__ __launch_bounds__(64 * WPX * WCH) __attribute__((amdgpu_waves_per_eu(BM * BN >= 128 * 128 ? 3 : 4))) void incep_group_nib_kernel(hawq_incep_group_args g, GroupMap mp, unsigned mask) {
    const GroupMember m = group_member(mp, blockIdx.x);
    __shared__ __attribute__((aligned(16))) char lds[2 * (BM + BN) * 64];
    const long long pblock = (long long)(m.local % m.npb) * BM;
    const int cblock = (m.local / m.npb) * BN;
    if ((mask >> m.mi) & 1) gn_nib_body<BM, BN, WPX, WCH, 1>(g.conv[m.mi], mp.Ho[m.mi], mp.Wo[m.mi], pblock, cblock, lds);
    else gn_int8_body<BM, BN, WPX, WCH, 1>(g.conv[m.mi], mp.Ho[m.mi], mp.Wo[m.mi], pblock, cblock, lds);
}

}  // namespace

extern "C" int hawq_incep_conv_group_nib_num_tiles(void) { return NUM_GN_TILES; }

extern "C" int hawq_incep_conv_group_nib_ok(const hawq_incep_group_args *g, uint32_t mask, int tile) {
    GroupGrid gg;
    int who;
    return gn_refusal(g, mask, tile, &gg, &who) == nullptr;
}

extern "C" int hawq_incep_conv_group_nib(const hawq_incep_group_args *g, uint32_t mask, int tile, void *stream) {
    GroupGrid gg;
    int who;
    const char *why = gn_refusal(g, mask, tile, &gg, &who);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_group_nib: tile %d refuses the group (member %d, mask 0x%x): %s", tile, who, (unsigned)mask, why);
    static_assert(sizeof(hawq_incep_group_args) + sizeof(GroupMap) + sizeof(unsigned) <= 4096, "kernel arguments");
    hipStream_t s = (hipStream_t)stream;
    if (tile == 1) hipLaunchKernelGGL((incep_group_nib_kernel<128, 128, 2, 2>), dim3((unsigned)gg.total), dim3(256), 0, s, *g, gg.mp, (unsigned)mask);
    else hipLaunchKernelGGL((incep_group_nib_kernel<128, 64, 2, 2>), dim3((unsigned)gg.total), dim3(256), 0, s, *g, gg.mp, (unsigned)mask);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
