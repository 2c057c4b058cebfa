// Mixed-form grouped launch of the InceptionV3 convs with a fan-out epilogue: hawq_incep_conv_group_nib (incep_group_nib.hip) whose
// members may store, next to their own output, the branch inputs of the NEXT unit - which a nibble plan otherwise makes with one
// entry requant per branch from the 16-bit concat buffer this epilogue has just written.
//   hawq_incep_conv_group_nib_fan_ok   host arithmetic only: does tile `tile` run this group, with these forms and fans, in one launch
//   hawq_incep_conv_group_nib_fan      the launch: member i writes, byte for byte, what its single launch on that shape writes
//                                      (hawq_incep_conv_nib with bit i of `mask` set, hawq_incep_conv_tiled with it clear), and for
//                                      j < fan[i].n the value s = clamp(dyadic_rne(y; m, ek), lo, hi) of every element y it stored
//                                      (after its last clamp) at pixel p, channel co, into to[j]:
//                                        bit 4 i + j of `fan_mask` clear   int8 rows:   out[p * ldo + c_off + co] = (int8) s
//                                        set                               hawq4 rows:  nibble p * ldo + c_off + co of out, as the
//                                                                          conv's own out_bits 4 store addresses it
// Grid, tiles (ids 1 and 2, 256 threads) and the choice of body are incep_group_nib.hip's; the bodies are the parents' texts
// (incep_tile_body.h, incep_nib_body.h) with fan_store below as the hook of either.  A member of either operand form may carry fan
// outputs of either form.
//
// Kernel arguments: 1096 (group) + 128 (map) + 1088 (8 fans of 136 bytes) + 2 x 4 (masks) = 2320 bytes of the 4096 a launch may
// carry.  Member, mask bit, fan index and form bit are wave-uniform: scalar loads and scalar branches.
//
// The fan epilogue.  A lane holds 16 consecutive channels of one pixel when either body's epilogue ends (q[16]).  The fan outputs
// are walked one at a time (#pragma unroll 1: the 16 requants of one output are all the registers the loop may take next to the
// accumulators still waiting for their own epilogue).  Both forms share the requant AND the byte packing: the 16 results become
// four pack4_i8 dwords d[0 .. 3], which are the int8 row as they stand (one 16-byte store), and since
//     pack8_u4(s) = pack4_i8(s[0 .. 3]) | pack4_i8(s[4 .. 7]) << 4
// the hawq4 row is d[0] | d[1] << 4, d[2] | d[3] << 4 (one 8-byte store).  The form branch is therefore behind the requant loop, two
// OR-shifts and a store long, and scalar.  Vector stores in plain C++ only.
#include "incep_nib.h"
#include "incep_tile.h"

extern "C" int hawq_incep_conv_group_nib_ok(const hawq_incep_group_args *g, uint32_t mask, int tile);

namespace {

// the hook of both bodies: a lane has stored channels cb .. cb + 15 of pixel p (q: what it stored); `fn`: the member's fan, bit t of
// `forms`: output t is hawq4 (both wave-uniform)
__device__ __forceinline__ void fan_store(const hawq_incep_fan &fn, const unsigned forms, const long long p, const int cb,
                                          const int (&q)[16]) {
#pragma unroll 1
    for (int t = 0; t < fn.n; ++t) {
        const hawq_incep_fan_out &f = fn.to[t];
        unsigned d[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int s[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] = clampi(dyadic_rne(q[4 * e + u], f.m, f.ek), f.lo, f.hi);
            d[e] = pack4_i8(s[0], s[1], s[2], s[3]);
        }
        const size_t row = (size_t)p * f.ldo + f.c_off + cb;   // a multiple of 16 elements (fn_refusal)
        if ((forms >> t) & 1) {   // 0 .. 15 a byte: the high nibbles are free
            *reinterpret_cast<v2i *>((char *)f.out + (row >> 1)) = v2i{(int)(d[0] | (d[1] << 4)), (int)(d[2] | (d[3] << 4))};
        } else {
            *reinterpret_cast<v4i *>((int8_t *)f.out + row) = v4i{(int)d[0], (int)d[1], (int)d[2], (int)d[3]};
        }
    }
}

// the tiled kernel's workgroup body on an int8 member, with the member's fan for the hook
template <int BM, int BN, int WPX, int WCH, int KS>
__device__ __forceinline__ void fn_int8_body(const hawq_incep_conv_args &a, const hawq_incep_fan &fn, const unsigned forms, const int Ho,
                                             const int Wo, const long long pblock, const int cblock, char *lds) {
#define INCEP_TILE_BLOCK
#define INCEP_TILE_STORED(p, cb, q) fan_store(fn, forms, p, cb, q)
#include "incep_tile_body.h"
#undef INCEP_TILE_BLOCK
#undef INCEP_TILE_STORED
}

// the nibble kernel's workgroup body on a hawq4 member, with the member's fan for the hook
template <int BM, int BN, int WPX, int WCH, int KS>
__device__ __forceinline__ void fn_nib_body(const hawq_incep_conv_args &a, const hawq_incep_fan &fn, const unsigned forms, const int Ho,
                                            const int Wo, const long long pblock, const int cblock, char *lds) {
#define INCEP_NIB_BLOCK
#define INCEP_NIB_STORED(p, cb, q) fan_store(fn, forms, p, cb, q)
#include "incep_nib_body.h"
#undef INCEP_NIB_BLOCK
#undef INCEP_NIB_STORED
}

struct FanSet {
    hawq_incep_fan fan[HAWQ_INCEP_GROUP_MAX];
};

// The occupancy floor is incep_group_nib_kernel's: 3 waves per SIMD on tile 1, 4 on tile 2.  The kernel needs the registers of the
// larger body plus one fan output's requants; the floor keeps the allocator from spreading the join over more (incep_fan.hip).
template <int BM, int BN, int WPX, int WCH>
__global__ __launch_bounds__(64 * WPX * WCH) __attribute__((amdgpu_waves_per_eu(BM * BN >= 128 * 128 ? 3 : 4))) void incep_fan_nib_kernel(hawq_incep_group_args g, GroupMap mp, FanSet fs, unsigned mask, unsigned fan_mask) {
    const GroupMember m = group_member(mp, blockIdx.x);
    __shared__ __attribute__((aligned(16))) char lds[2 * (BM + BN) * 64];
    const long long pblock = (long long)(m.local % m.npb) * BM;
    const int cblock = (m.local / m.npb) * BN;
    const unsigned forms = (fan_mask >> (HAWQ_INCEP_FAN_MAX * m.mi)) & ((1u << HAWQ_INCEP_FAN_MAX) - 1);
    if ((mask >> m.mi) & 1) fn_nib_body<BM, BN, WPX, WCH, 1>(g.conv[m.mi], fs.fan[m.mi], forms, mp.Ho[m.mi], mp.Wo[m.mi], pblock, cblock, lds);
    else fn_int8_body<BM, BN, WPX, WCH, 1>(g.conv[m.mi], fs.fan[m.mi], forms, mp.Ho[m.mi], mp.Wo[m.mi], pblock, cblock, lds);
}
static_assert(HAWQ_INCEP_FAN_MAX * HAWQ_INCEP_GROUP_MAX <= 32, "fan_mask has one bit per fan output");

// the tile shapes of hawq_incep_conv_group_nib's ids 1 and 2
constexpr int kBm[3] = {0, 128, 128}, kBn[3] = {0, 128, 64};

// what writes in one launch: a member's primary output, or one of its fan outputs as a pseudo-member - the block of a conv that
// reads what its carrier reads and stores the carrier's channels into the fan's rows at the fan's element width
struct Writer {
    hawq_incep_conv_args a;
    Span in, out;
    int who, which;
};

// why tile `tile` does not run group `g` with the forms `mask` and the fans `fan` / `fan_mask` in one launch (NULL: it does, and `gg`
// describes the grid).  No pointer is dereferenced.  `who`: the member, `which`: its fan output (-1: none in particular).
const char *fn_refusal(const hawq_incep_group_args *g, unsigned mask, const hawq_incep_fan *fan, unsigned fan_mask, int tile,
                       GroupGrid *gg, int *who, int *which) {
    *who = *which = -1;
    if (!g || !fan) return "null group or fan list";
    if (tile < 1 || tile > 2) return "no such tile (a mixed group runs on id 1 or 2)";
    if (!hawq_incep_conv_group_nib_ok(g, mask, tile)) return "the mixed-form grouped launch refuses the group (hawq_incep_conv_group_nib_ok)";
    // the grid hawq_incep_conv_group_nib launches: its checks have just passed
    (void)group_grid(g, kBm[tile], kBn[tile], mask, [](int, const hawq_incep_conv_args *) -> const char * { return nullptr; }, gg, who);
    for (int b = 0; b < 32; ++b) {
        const int i = b / HAWQ_INCEP_FAN_MAX, j = b % HAWQ_INCEP_FAN_MAX;
        if (((fan_mask >> b) & 1) && (i >= g->n || j >= fan[i].n)) {
            *who = i, *which = j;
            return "fan_mask names a fan output that does not exist (member >= n or output >= fan[i].n)";
        }
    }
    static_assert(HAWQ_INCEP_GROUP_MAX * (1 + HAWQ_INCEP_FAN_MAX) == 40, "writers");
    Writer w[40];
    int nw = 0;
    for (int i = 0; i < g->n; ++i) {
        const hawq_incep_conv_args *a = &g->conv[i];
        *who = i, *which = -1;
        w[nw++] = Writer{*a, gg->in[i], gg->out[i], i, -1};
        if (fan[i].n < 0 || fan[i].n > HAWQ_INCEP_FAN_MAX) return "a member has 0 .. 4 fan outputs";
        if (fan[i].n > 0 && a->epilogue == HAWQ_INCEP_RAW) return "a RAW member has no fan (the fan takes a requantised output)";
        for (int j = 0; j < fan[i].n; ++j) {
            const hawq_incep_fan_out *f = &fan[i].to[j];
            const bool nib = (fan_mask >> (HAWQ_INCEP_FAN_MAX * i + j)) & 1;
            *which = j;
            if (!f->out) return "null fan output";
            if (nib ? !(f->lo >= 0 && f->lo <= f->hi && f->hi <= 15) : !(f->lo >= -128 && f->lo <= f->hi && f->hi <= 127))
                return nib ? "fan clamp bounds outside a nibble (0 <= lo <= hi <= 15)" : "fan clamp bounds outside int8 (-128 <= lo <= hi <= 127)";
            if (f->m < 0 || f->ek < 0 || (f->ek & 0xff) < 1 || (f->ek & 0xff) > 62 || (f->ek >> 8) > 15)
                return "fan table outside the dyadic form (m >= 0, 1 <= e <= 62, k <= 15)";
            if (((uintptr_t)f->out & 15) || f->ldo % 16 || f->c_off % 16 || f->c_off < 0)
                return "a fan output is stored in runs of 16 elements: out 16-byte aligned, ldo and c_off multiples of 16";
            if (f->ldo < f->c_off + a->Cout) return "fan ldo < c_off + Cout";
            // the pseudo-member: extents in half bytes, as group_grid counts them (an int8 element is two, a hawq4 element one)
            const size_t hb = nib ? 1 : 2;
            Writer &x = w[nw++];
            x = Writer{*a, gg->in[i], Span{}, i, j};
            x.a.out = f->out, x.a.ldo = f->ldo, x.a.c_off = f->c_off, x.a.out_bits = nib ? 4 : 8, x.a.epilogue = HAWQ_INCEP_REQUANT;
            x.out.lo = (uintptr_t)f->out + (size_t)f->c_off * hb / 2;
            x.out.hi = (uintptr_t)f->out + ((size_t)(gg->P[i] - 1) * f->ldo + f->c_off + a->Cout) * hb / 2;
        }
    }
    // independence: every fan output against every member and every other fan output, as a group of two under group_dependence's
    // two rules (the members among themselves have passed them)
    hawq_incep_group_args pair;
    GroupGrid pg;
    pair.n = 2;
    for (int x = 0; x < nw; ++x) {
        if (w[x].which < 0) continue;
        for (int y = 0; y < nw; ++y) {
            if (y == x || (w[y].which >= 0 && y < x)) continue;
            pair.conv[0] = w[x].a, pair.conv[1] = w[y].a;
            pg.in[0] = w[x].in, pg.out[0] = w[x].out, pg.in[1] = w[y].in, pg.out[1] = w[y].out;
            int k;
            if (group_dependence(&pair, &pg, &k)) {
                *who = w[x].who, *which = w[x].which;
                return w[y].which >= 0 ? "two fan outputs overlap" : "a fan output overlaps a member's input or primary output";
            }
        }
    }
    *who = *which = -1;
    return nullptr;
}

}  // namespace

extern "C" int hawq_incep_conv_group_nib_fan_ok(const hawq_incep_group_args *g, uint32_t mask, const hawq_incep_fan *fan,
                                                uint32_t fan_mask, int tile) {
    GroupGrid gg;
    int who, which;
    return fn_refusal(g, mask, fan, fan_mask, tile, &gg, &who, &which) == nullptr;
}

extern "C" int hawq_incep_conv_group_nib_fan(const hawq_incep_group_args *g, uint32_t mask, const hawq_incep_fan *fan,
                                             uint32_t fan_mask, int tile, void *stream) {
    GroupGrid gg;
    int who, which;
    const char *why = fn_refusal(g, mask, fan, fan_mask, tile, &gg, &who, &which);
    HAWQ_REQUIRE(!why, "hawq_incep_conv_group_nib_fan: tile %d refuses the launch (member %d, fan output %d, mask 0x%x, fan_mask 0x%x): %s",
                 tile, who, which, (unsigned)mask, (unsigned)fan_mask, why);
    FanSet fs;
    for (int i = 0; i < HAWQ_INCEP_GROUP_MAX; ++i) {
        fs.fan[i] = fan[i < g->n ? i : 0];
        if (i >= g->n) fs.fan[i].n = 0;
    }
    static_assert(sizeof(hawq_incep_group_args) + sizeof(GroupMap) + sizeof(FanSet) + 2 * sizeof(unsigned) <= 4096, "kernel arguments");
    hipStream_t s = (hipStream_t)stream;
    if (tile == 1) hipLaunchKernelGGL((incep_fan_nib_kernel<128, 128, 2, 2>), dim3((unsigned)gg.total), dim3(256), 0, s, *g, gg.mp, fs, (unsigned)mask, (unsigned)fan_mask);
    else hipLaunchKernelGGL((incep_fan_nib_kernel<128, 64, 2, 2>), dim3((unsigned)gg.total), dim3(256), 0, s, *g, gg.mp, fs, (unsigned)mask, (unsigned)fan_mask);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
