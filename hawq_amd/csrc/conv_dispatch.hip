// hawq_conv2d in three steps over one table of kernel families.  Host code only.
//   conv_check   the argument rules and the ConvP fill (shared with hawq_conv2d_splitk)
//   conv_choose  family, tile, function-table slot, grid, block, LDS: pure, no HIP call (hawq_conv2d_choice stops here)
//   conv_launch  the family's attribute static, launch and HAWQ_DBG print
#include "conv_dispatch.h"

namespace {

// The tile ids 1 .. hawq_conv2d_num_tiles() in order: each family owns `count` consecutive ids.
enum { FAM_PLAIN, FAM_BAND, FAM_PERSIST, FAM_BAND2, FAM_GEMM2, NUM_FAMILIES };
#define CONV_FAMILY(F, NAME, WHAT, PREFER) {NAME, WHAT, F##_count, PREFER, F##_applies, F##_choose, F##_launch}
const ConvFamily kConvFamilies[NUM_FAMILIES] = {
    CONV_FAMILY(conv_igemm, "plain", nullptr, nullptr),
    CONV_FAMILY(band_v1, "band", "3x3 band kernel", kBandPreference),
    CONV_FAMILY(band_persist, "weight-stationary", "weight-stationary 3x3 kernel", nullptr),
    CONV_FAMILY(band_v2, "band_v2", "round-5 3x3 kernel", kBandV2Preference),
    CONV_FAMILY(gemm_v2, "gemm_v2", "round-5 1x1 kernel", nullptr),
};

// first 1-based tile id of family `fam` (fam == NUM_FAMILIES: one past the last id)
int family_first_id(int fam) {
    int id = 1;
    for (int k = 0; k < fam; ++k) id += kConvFamilies[k].count();
    return id;
}

// 1-based id of the first tile of `fam`, in its order of preference, that takes the layer; 0 if none does
int family_preferred_id(int fam, const hawq_conv_args *a) {
    const ConvFamily &f = kConvFamilies[fam];
    for (int k = 0; f.prefer && k < f.count(); ++k)
        if (f.applies(a, f.prefer[k])) return family_first_id(fam) + f.prefer[k];
    return 0;
}

bool has_shape(const hawq_conv_args *a) { return a && a->W > 0 && a->H > 0 && a->Cin > 0 && a->Cout > 0; }

int conv_choose(const hawq_conv_args *a, const ConvForm &f, const ConvP &p, ConvChoice *c) {
    int id = a->tile > 0 ? a->tile : conv_igemm_pick_tile(p.M, p.Cout, f.dual) + 1;
    if (a->tile == 0 && a->in_planar) {  // only the band kernels read planar activations: first one that takes the layer
        id = 0;
        for (int fam = 0; fam < NUM_FAMILIES && id == 0; ++fam) id = family_preferred_id(fam, a);
        HAWQ_REQUIRE(id > 0, "hawq_conv2d: in_planar input but no 3x3 band kernel takes this layer");
    }
    int fam = 0, v = id - 1;
    while (fam < NUM_FAMILIES && v >= kConvFamilies[fam].count()) v -= kConvFamilies[fam++].count();
    if (fam == FAM_PLAIN || fam == NUM_FAMILIES) {
        HAWQ_REQUIRE(!a->in_planar, "hawq_conv2d: in_planar activations are read by the 3x3 band kernels only (tile %d is not one)", a->tile);
        HAWQ_REQUIRE(fam == FAM_PLAIN, "hawq_conv2d: bad tile id %d", a->tile);
    } else {
        HAWQ_REQUIRE(kConvFamilies[fam].applies(a, v), "hawq_conv2d: tile %d (%s) does not apply to this layer", a->tile, kConvFamilies[fam].what);
    }
    *c = ConvChoice{fam, v, 0, {-1, -1, -1}, 0, 0, 0, 0};
    return kConvFamilies[fam].choose(a, f, p, *c);
}

int conv_launch(const hawq_conv_args *a, const ConvChoice &c, const ConvP &p, void *stream) {
    return kConvFamilies[c.family].launch(a, c, p, stream);
}

}  // namespace

ConvForm conv_form(const hawq_conv_args *a) {
    const bool dual = a->in2 != nullptr, res = a->epilogue == HAWQ_EPI_RESIDUAL;
    ConvForm f;
    f.dual = dual, f.fast = a->fast_tables != 0;
    f.wide_res = res && ((!dual && a->res_in_bits == 32) || (a->res_out && a->res_out_bits == 32));
    // the signed / identity-free RESIDUAL forms (MobileNetV2, ABI 3) live on the direct epilogue like the 32-bit residual tensors do;
    // with fast_tables they run it with the fast contract's arithmetic (ConvP.gfast)
    f.signed_res = res && !dual && (a->res_no_relu || a->res_clamp16 || !a->res_in);
    f.all88 = a->in_bits == 8 && a->w_bits == 8 && (!dual || (a->in2_bits == 8 && a->w2_bits == 8));
    f.all44 = a->in_bits == 4 && a->w_bits == 4 && (!dual || (a->in2_bits == 4 && a->w2_bits == 4));
    f.needs_tables = a->epilogue == HAWQ_EPI_REQUANT || res;
    f.slot = a->epilogue;   // HAWQ_EPI_RAW .. HAWQ_EPI_DEQUANT are 0 .. 3
    return f;
}

#define CHECK(cond, fmt, ...) HAWQ_REQUIRE(cond, "%s: " fmt, who, ##__VA_ARGS__)
int conv_check(const hawq_conv_args *a, const char *who, ConvForm *form, ConvP *pp) {
    CHECK(a != nullptr, "null args");
    const ConvForm f = *form = conv_form(a);
    const int epi = a->epilogue;
    const bool dual = f.dual, fast = f.fast, res = epi == HAWQ_EPI_RESIDUAL;
    const bool direct = !dual && (f.wide_res || f.signed_res);   // runs the direct epilogue (clamps q on both sides), see ConvP.gfast

    CHECK(a->in && a->wgt && a->bias, "in/wgt/bias must be non-null");
    CHECK(a->Cin > 0 && a->Cin % 64 == 0, "Cin=%d must be a positive multiple of 64", a->Cin);
    CHECK(a->Cout > 0 && a->Cout % 64 == 0, "Cout=%d must be a positive multiple of 64", a->Cout);
    CHECK((a->in_bits == 8 || a->in_bits == 4) && (a->w_bits == 8 || a->w_bits == 4), "in_bits/w_bits must be 4 or 8 (got %d/%d)", a->in_bits, a->w_bits);
    CHECK(a->KH > 0 && a->KW > 0 && a->stride > 0 && a->pad >= 0 && a->N > 0 && a->H > 0 && a->W > 0, "bad geometry");
    // out_sub = s >= 2: only the output pixels (n, s y', s x') of a 1x1 / stride 1 / pad 0 launch, stored densely - the 1x1 conv of stride s
    // on `in`, with res_in read at the same source pixels (ConvP.res_sub)
    // - or of a 3x3 / stride 1 / pad 1 REQUANT / RAW launch: the 3x3 conv of stride s (pad 1 keeps pixel (s y', s x') the window's centre).
    // res_sub (stride2 = s >= 2 without a second branch: hawq_res_sub): the same 1x1 launch on a dense small-map `in`, only res_in on the larger H2 x W2 map
    const int sub = a->out_sub >= 2 ? a->out_sub : 1, rsub = hawq_res_sub(*a) ? hawq_res_sub(*a) : 1;
    const bool dense_rows = !a->out_planar && a->in_pitch == 0 && a->out_pitch == 0;
    const bool sub_1x1 = a->KH == 1 && a->KW == 1 && a->stride == 1 && a->pad == 0 && !dual && !a->res_out && res && !a->in_planar && dense_rows;
    const bool sub_3x3 = a->KH == 3 && a->KW == 3 && a->stride == 1 && a->pad == 1 && !dual && (epi == HAWQ_EPI_REQUANT || epi == HAWQ_EPI_RAW) && dense_rows;
    CHECK(sub == 1 || sub_1x1 || sub_3x3,
          "out_sub=%d needs a 1x1 / stride 1 / pad 0 single-branch RESIDUAL launch without res_out, dense NHWC rows", a->out_sub);
    CHECK(rsub == 1 || (sub == 1 && sub_1x1 && (a->H2 - 1) / rsub + 1 == a->H && (a->W2 - 1) / rsub + 1 == a->W),
          "res_sub (stride2 without in2)=%d needs a 1x1 / stride 1 / pad 0 single-branch RESIDUAL launch without res_out and without out_sub, dense NHWC rows, and a "
          "H2 x W2 = %d x %d map whose pixels (s y, s x) are this launch's %d x %d", a->stride2, a->H2, a->W2, a->H, a->W);
    ConvP &p = *pp;
    p = ConvP{};
    p.in = (const uint8_t *)a->in, p.wgt = (const uint8_t *)a->wgt, p.bias = a->bias;
    p.N = a->N, p.H = a->H, p.W = a->W, p.Cin = a->Cin, p.Cout = a->Cout;
    p.KH = a->KH, p.KW = a->KW, p.stride = a->stride * sub, p.pad = a->pad;
    // where res_in is read: at the source pixel of a subsampled 1x1 launch (its own H x W map), or on the larger map of a res_sub launch
    p.res_sub = (sub > 1 && sub_1x1) ? sub : (rsub > 1 ? rsub : 0);
    p.res_H = rsub > 1 ? a->H2 : a->H, p.res_W = rsub > 1 ? a->W2 : a->W;
    CHECK((long long)a->N * p.res_H * p.res_W < (1ll << 30), "problem too large");
    p.Ho = (a->H + 2 * a->pad - a->KH) / p.stride + 1;
    p.Wo = (a->W + 2 * a->pad - a->KW) / p.stride + 1;
    CHECK(p.Ho > 0 && p.Wo > 0, "empty output");
    const long long M = (long long)a->N * p.Ho * p.Wo;
    CHECK(M * (long long)a->Cout < (1ll << 40) && M < (1ll << 30) && (long long)a->N * a->H * a->W < (1ll << 30), "problem too large");
    p.M = (int)M;
    p.in_bits = a->in_bits, p.w_bits = a->w_bits;
    p.in2 = (const uint8_t *)a->in2, p.wgt2 = (const uint8_t *)a->wgt2, p.bias2 = a->bias2;
    p.H2 = a->H2, p.W2 = a->W2, p.Cin2 = a->Cin2, p.stride2 = a->stride2;
    p.in2_bits = a->in2_bits, p.w2_bits = a->w2_bits;
    if (dual) {
        CHECK(res, "second branch needs HAWQ_EPI_RESIDUAL");
        CHECK(a->wgt2 && a->bias2 && a->m_id && a->e_id, "second branch tables missing");
        CHECK(a->Cin2 > 0 && a->Cin2 % 64 == 0, "Cin2 must be a multiple of 64");
        CHECK((a->in2_bits == 8 || a->in2_bits == 4) && (a->w2_bits == 8 || a->w2_bits == 4), "in2_bits/w2_bits must be 4 or 8");
        CHECK((a->H2 - 1) / a->stride2 + 1 == p.Ho && (a->W2 - 1) / a->stride2 + 1 == p.Wo, "second branch output grid differs");
    }
    p.relu = a->relu;
    p.m = a->m, p.e = a->e, p.m_id = a->m_id, p.e_id = a->e_id;
    p.m_id_s = a->m_id_scalar, p.e_id_s = a->e_id_scalar;
    p.res_in = a->res_in, p.res_in_bits = a->res_in_bits;
    p.res_no_relu = a->res_no_relu, p.res_clamp16 = a->res_clamp16;
    p.res_out = a->res_out, p.res_out_bits = a->res_out_bits;
    p.out_q = a->out_q, p.out_bits = a->out_bits, p.q_lo = a->q_lo, p.q_hi = a->q_hi, p.mq = a->mq, p.eq = a->eq;
    p.out_acc = a->out_acc, p.out_f32 = a->out_f32, p.fscale = a->fscale, p.ldo = a->ldo, p.n_valid = a->n_valid;
    {   // ABI 4: pitches of narrow tensors (0 = dense)
        const int dense_in = a->Cin * a->in_bits / 8;
        p.in_pitch = a->in_pitch ? a->in_pitch : dense_in, p.out_pitch = a->out_pitch ? a->out_pitch : a->Cout;
        if (p.in_pitch != dense_in)
            CHECK(a->in_pitch > 0 && a->in_pitch % 16 == 0 && a->in_pitch < dense_in && a->in_bits == 8 && !a->in_planar,
                  "in_pitch=%d needs a multiple of 16 below the dense row (%d bytes), int8 activations, NHWC rows", a->in_pitch, dense_in);
        if (p.out_pitch != a->Cout) {
            CHECK(a->out_pitch > 0 && a->out_pitch % 16 == 0 && a->out_pitch < a->Cout, "out_pitch=%d needs a multiple of 16 below Cout=%d", a->out_pitch, a->Cout);
            CHECK((epi == HAWQ_EPI_REQUANT || res) && !dual && !a->out_planar && (!a->out_q || a->out_bits == 8),
                  "out_pitch exists for single-branch REQUANT / RESIDUAL launches with int8 NHWC outputs");
            // the direct epilogue addresses pitched rows (ConvP.gfast), the fast RESIDUAL tiles are dense
            CHECK(!fast || epi == HAWQ_EPI_REQUANT || direct,
                  "out_pitch with fast_tables needs the REQUANT epilogue or a signed / 32-bit RESIDUAL (the unsigned 16-bit fast RESIDUAL tiles are dense)");
            CHECK(a->n_valid <= a->out_pitch, "n_valid=%d exceeds out_pitch=%d", a->n_valid, a->out_pitch);
        }
    }
    p.flags = a->flags;
    p.ctab = a->ctab, p.ctab_id = a->ctab_id;
    static const int dbg_env = HAWQ_DBG_ENV();
    p.dbg = fast ? dbg_env : 0;  // ablations only touch the fused-plan launches; a launch that stamps cycles attaches ConvP.dbgbuf
    p.k0 = (a->fast_tables & 4) ? 2 : ((a->fast_tables & 2) ? 1 : 0);
    p.ck0 = (a->fast_tables & 8) != 0;
    p.gfast = fast && direct;
    if (fast && f.needs_tables) {
        CHECK(a->ctab && (!dual || a->ctab_id), "fast_tables needs ctab (and ctab_id)");
        if (epi == HAWQ_EPI_REQUANT && a->relu && p.q_lo < 0) p.q_lo = 0;  // ReLU folded into the clamp
        CHECK(!res || !a->out_q || a->q_lo <= 0 || direct, "fast RESIDUAL needs q_lo <= 0");
    }
    auto e_fast = [](int ek) { return (ek & 0xff) >= 33 && (ek & 0xff) <= 62; };
    auto e_any = [](int ek) { return (ek & 0xff) >= 1 && (ek & 0xff) <= 62 && (ek >> 8) >= 0 && (ek >> 8) < 31; };
    if (res && a->out_q) {
        CHECK(a->mq >= 0 && e_any(a->eq), "bad (mq, eq)");
        CHECK(!fast || e_fast(a->eq), "fast_tables needs eq in [33,62]");
        CHECK(!fast || (a->q_hi >= 0 && a->q_hi <= 32767), "fast_tables needs 0 <= q_hi <= 32767 for the next QuantAct");
        CHECK(p.k0 != 1 || (a->eq >> 8) == 0, "fast_tables bit 1 (no pre-shifts) but eq carries one");
    } else {
        p.mq = 0, p.eq = 33;
    }
    if (res && !dual && a->res_in) {
        CHECK(a->m_id_scalar >= 0 && e_any(a->e_id_scalar), "bad (m_id_scalar, e_id_scalar)");
        CHECK(!fast || e_fast(a->e_id_scalar), "fast_tables needs e_id_scalar in [33,62]");
    } else {   // no scalar identity table: another epilogue, the identity conv's per-channel tables, or no identity branch at all (ABI 3)
        p.m_id_s = 0, p.e_id_s = 33;
    }
    switch (epi) {
        case HAWQ_EPI_RAW:
            CHECK(a->out_acc, "RAW needs out_acc");
            break;
        case HAWQ_EPI_REQUANT:
            CHECK(a->out_q && a->m && a->e, "REQUANT needs out_q, m, e");
            CHECK(a->out_bits == 8 || a->out_bits == 4, "out_bits must be 4 or 8");
            break;
        case HAWQ_EPI_RESIDUAL:
            CHECK(a->m && a->e, "RESIDUAL needs m, e");
            CHECK(dual || !a->res_in || a->res_in_bits == 16 || a->res_in_bits == 32, "res_in_bits 16/32");
            CHECK(!(dual && (a->res_no_relu || a->res_clamp16)), "res_no_relu / res_clamp16 exist for single-branch launches");
            CHECK(!fast || !f.signed_res || (a->fast_tables & 2) == 0, "fast_tables bit 1 is not defined for the signed / identity-free RESIDUAL forms");
            CHECK(!a->res_no_relu || !a->res_out || a->res_out_bits == 32, "a residual stored without ReLU is signed: res_out_bits must be 32");
            CHECK(!a->res_out || a->res_out_bits == 32 || (a->res_out_bits == 16 && a->flags), "res_out_bits 16 (with flags) or 32");
            CHECK(!a->out_q || a->out_bits == 8 || a->out_bits == 4, "out_bits must be 4 or 8");
            CHECK(a->res_out || a->out_q, "RESIDUAL needs res_out and/or out_q");
            break;
        case HAWQ_EPI_DEQUANT:
            CHECK(a->out_f32 && a->fscale && a->ldo > 0, "DEQUANT needs out_f32, fscale, ldo");
            break;
        default:
            CHECK(false, "unknown epilogue %d", epi);
    }
    p.in_planar = a->in_planar, p.out_planar = a->out_planar;
    CHECK((a->in_planar | a->out_planar | 1) == 1, "in_planar / out_planar must be 0 or 1");
    CHECK(!a->out_planar || (fast && a->out_q && f.needs_tables && !(res && a->res_out && a->res_out_bits == 32)),
          "out_planar needs the fast-contract REQUANT / RESIDUAL epilogue");
    return 0;
}
#undef CHECK

static_assert(HAWQ_EPI_RAW == 0 && HAWQ_EPI_REQUANT == 1 && HAWQ_EPI_RESIDUAL == 2 && HAWQ_EPI_DEQUANT == 3, "ConvForm.slot is the epilogue id");

long long *conv_dbg_buffer(int dbg) {
    static long long *dbg_dev = nullptr;
    if (HAWQ_DBG_BIT(dbg, 128) && !dbg_dev) (void)hipMalloc(&dbg_dev, 64 * sizeof(long long));
    return HAWQ_DBG_BIT(dbg, 128) ? dbg_dev : nullptr;
}

extern "C" int hawq_conv2d_num_tiles(void) { return family_first_id(NUM_FAMILIES) - 1; }
extern "C" int hawq_conv2d_num_band_tiles(void) { return family_first_id(NUM_FAMILIES) - family_first_id(FAM_BAND); }   // every special-purpose kernel
extern "C" int hawq_conv2d_num_band2_tiles(void) { return kConvFamilies[FAM_BAND2].count(); }
extern "C" int hawq_conv2d_num_gemm2_tiles(void) { return kConvFamilies[FAM_GEMM2].count(); }
extern "C" int hawq_conv2d_gemm2_first(void) { return family_first_id(FAM_GEMM2); }
extern "C" int hawq_conv2d_band_tile(const hawq_conv_args *a) { return has_shape(a) ? family_preferred_id(FAM_BAND, a) : 0; }
extern "C" int hawq_conv2d_band2_tile(const hawq_conv_args *a) { return has_shape(a) ? family_preferred_id(FAM_BAND2, a) : 0; }

extern "C" int hawq_conv2d(const hawq_conv_args *a, void *stream) {
    ConvForm f;
    ConvP p;
    ConvChoice c;
    if (const int rc = conv_check(a, "hawq_conv2d", &f, &p)) return rc;
    if (const int rc = conv_choose(a, f, p, &c)) return rc;
    p.ring_bytes = c.ring_bytes;
    return conv_launch(a, c, p, stream);
}

extern "C" int hawq_conv2d_choice(const hawq_conv_args *a, hawq_conv_choice *out) {
    HAWQ_REQUIRE(out != nullptr, "hawq_conv2d_choice: null out");
    ConvForm f;
    ConvP p;
    ConvChoice c;
    if (const int rc = conv_check(a, "hawq_conv2d", &f, &p)) return rc;
    if (const int rc = conv_choose(a, f, p, &c)) return rc;
    const bool plain = c.family == FAM_PLAIN;   // gfast and ring_bytes are read by the plain tiles' kernels only
    *out = hawq_conv_choice{c.family, family_first_id(c.family) + c.tile, c.tile, c.table, {c.fn[0], c.fn[1], c.fn[2]}, c.grid, c.block, c.lds,
                            p.stride, p.res_sub, p.Ho, p.Wo, p.M, p.q_lo, p.mq, p.eq, p.m_id_s, p.e_id_s, p.k0, p.ck0, plain ? p.gfast : 0,
                            p.in_pitch, p.out_pitch, c.ring_bytes};
    return 0;
}
