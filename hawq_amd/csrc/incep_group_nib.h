// What the mixed-form grouped launches share (incep_group_nib.hip: the plain launch, incep_group_nib_splitk.hip: its split-K form): the
// table of tile ids both operand families have, and the host's check of a group with a mask (gn_refusal).
#pragma once
#include "incep_nib.h"
#include "incep_tile.h"

namespace {

// tile ids 1 .. NUM_GN_TILES, 256 threads as 2 x 2 waves, with the id of that shape in either family
//   1  128 px x 128 ch, waves of 64 x 64   int8 tile 1, nibble tile 1
//   2  128 px x  64 ch, waves of 64 x 32   int8 tile 3, nibble tile 2
enum { NUM_GN_TILES = 2 };
struct GnTile {
    int bm, bn, i8, nib;
};
constexpr GnTile kGn[NUM_GN_TILES + 1] = {{0, 0, 0, 0}, {128, 128, 1, 1}, {128, 64, 3, 2}};
static_assert(kTiles[kGn[1].i8].bm == 128 && kTiles[kGn[1].i8].bn == 128 && kTiles[kGn[2].i8].bm == 128 && kTiles[kGn[2].i8].bn == 64,
              "the int8 ids name these shapes");

// why tile `tile` does not run group `g` with the forms `mask` in one launch (NULL: it does, and `gg` describes the grid).
// No pointer is dereferenced.
const char *gn_refusal(const hawq_incep_group_args *g, unsigned mask, int tile, GroupGrid *gg, int *who) {
    *who = -1;
    if (!g) return "null group";
    if (g->n < 1 || g->n > HAWQ_INCEP_GROUP_MAX) return "a group has 1 .. 8 members";
    if (mask >> g->n) return "the mask names a member beyond n";
    if (tile < 1 || tile > NUM_GN_TILES) return "no such tile (a mixed group runs on id 1 or 2)";
    const GnTile t = kGn[tile];
    // A member must be a launch its own family's kernel of this wave layout takes: the family's check on its 128 px x 64 ch tile, which
    // asks for a well-formed block, the alignment and (hawq4) the K bound and nothing of its own.  The single launches' tile 1 also
    // turns away Cout <= 64, where half its channel block idles; that is a preference of a launch that may pick its tile per conv, and
    // is not applied here: a group has one tile for all its members, and which one is faster for a level is for the tuner to time.
    auto refuses = [mask](int i, const hawq_incep_conv_args *a) -> const char * {
        if ((mask >> i) & 1) return hawq_incep_conv_nib_ok(a, kGn[2].nib) ? nullptr : "the nibble kernel refuses this member (hawq_incep_conv_nib_ok)";
        if (a->epilogue != HAWQ_INCEP_RAW && a->out_bits == 4) return "out_bits 4 on an int8 member (only a hawq4 member stores nibbles)";
        return hawq_incep_conv_tile_ok(a, kGn[2].i8) ? nullptr : "the tiled int8 kernel refuses this member (hawq_incep_conv_tile_ok)";
    };
    if (const char *why = group_grid(g, t.bm, t.bn, mask, refuses, gg, who)) return why;
    return group_dependence(g, gg, who);
}

}  // namespace
