// What the two split-K grouped launches of the InceptionV3 convs share (incep_splitk.hip: int8 members, incep_group_nib_splitk.hip:
// members of either operand form): the slice layout the host passes by value (SliceMap), the host's view of a split launch
// (SplitGrid, split_layout) with the workspace formula, and - as text, in incep_splitk_arrive.h - the arrival protocol.
#pragma once
#include "incep_tile.h"

namespace {

constexpr int MAX_SLICES = 32;

// per member, by value: output tiles, slices, steps per slice, first slab (in slabs) and first counter of the member
struct SliceMap {
    int32_t tiles[HAWQ_INCEP_GROUP_MAX], S[HAWQ_INCEP_GROUP_MAX], q[HAWQ_INCEP_GROUP_MAX], slab0[HAWQ_INCEP_GROUP_MAX],
        cnt0[HAWQ_INCEP_GROUP_MAX];
};

// the host's view of a split launch
struct SplitGrid {
    GroupGrid gg;   // mp.end rewritten to the running totals of tiles_i * S_i
    SliceMap sm;
    long long total, slabs, counters;
};

// Cuts the members of a laid-out group (sg->gg: group_grid's result on 128 px x 64 ch tiles) into slices[i] slices each and rewrites
// the grid; a reason and the member `who` where that cannot be done (NULL: `sg` is filled; sg->slabs == 0: no member is cut).  Bit
// i of `nib`: member i reads hawq4 rows, whose 64-byte K steps hold eight 16-channel units, not four.
const char *split_layout(const hawq_incep_group_args *g, unsigned nib, const int32_t *slices, SplitGrid *sg, int *who) {
    GroupMap *mp = &sg->gg.mp;
    SliceMap *sm = &sg->sm;
    long long wgs = 0, slabs = 0, counters = 0;
    int first = 0;
    for (int i = 0; i < HAWQ_INCEP_GROUP_MAX; ++i) sm->tiles[i] = sm->S[i] = sm->q[i] = 1, sm->slab0[i] = sm->cnt0[i] = 0;
    for (int i = 0; i < g->n; ++i) {
        const hawq_incep_conv_args *a = &g->conv[i];
        *who = i;
        const int S = slices[i], tiles = mp->end[i] - first, per = (nib >> i) & 1 ? 8 : 4;
        first = mp->end[i];
        if (S < 1 || S > MAX_SLICES) return "a member has 1 .. 32 slices";
        const int steps = (a->KH * a->KW * (a->Cin >> 4) + per - 1) / per, q = (steps + S - 1) / S;
        if ((long long)(S - 1) * q >= steps) return "an empty slice: (S - 1) * ceil(steps / S) must stay below the member's K steps";
        if (slabs + (long long)tiles * S >= (1ll << 31) || wgs + (long long)tiles * S >= (1ll << 31)) return "too many workgroups";
        sm->tiles[i] = tiles, sm->S[i] = S, sm->q[i] = q, sm->slab0[i] = (int32_t)slabs, sm->cnt0[i] = (int32_t)counters;
        if (S > 1) slabs += (long long)tiles * S, counters += tiles;
        wgs += (long long)tiles * S;
        mp->end[i] = (int32_t)wgs;
    }
    *who = -1;
    sg->total = wgs, sg->slabs = slabs, sg->counters = counters;
    return nullptr;
}

}  // namespace
