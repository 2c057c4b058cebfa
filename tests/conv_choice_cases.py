"""Argument structs for the host-only query hawq_conv2d_choice: one case list for the fixture generator
(tests/golden/make_conv_choices.py) and the test that replays it (tests/test_conv_choice_host.py).

A case is (name, ConvArgs).  Pointers are dummy non-null values: the query tests them against NULL and never dereferences
them.  The list walks the ResNet18 / 50 geometries at the batch sizes on both sides of pick_tile's workgroup thresholds,
MobileNetV2's narrow rows, the FC as DEQUANT, every epilogue form, every operand-width pairing, every fast_tables value the
engines pass, the layout flags, every tile id (29 is one past the last), and one deliberately invalid struct per argument
rule of hawq_conv2d.  This is a plain module; nothing here needs a device.
"""
from __future__ import annotations

from hawq_amd import _lib

PTR = 16
NUM_TILES = 28
BATCHES = (1, 2, 128)
FAST = (0, 1, 3, 5, 9)
WIDTHS = ((8, 8), (4, 4), (4, 8), (8, 4))

# (H = W, Cin, Cout, K, stride): the 1x1, 3x3 and strided convs of ResNet18 / 50 on the 56, 28, 14 and 7 maps
GEOMETRIES = (
    (56, 64, 64, 1, 1), (56, 64, 64, 3, 1), (56, 64, 256, 1, 1), (56, 256, 64, 1, 1), (56, 256, 128, 1, 1), (56, 128, 128, 3, 2),
    (56, 64, 128, 3, 2), (56, 256, 512, 1, 2),
    (28, 128, 128, 3, 1), (28, 128, 512, 1, 1), (28, 512, 128, 1, 1), (28, 512, 256, 1, 1), (28, 256, 256, 3, 2), (28, 128, 256, 3, 2),
    (28, 512, 1024, 1, 2),
    (14, 256, 256, 3, 1), (14, 256, 1024, 1, 1), (14, 1024, 256, 1, 1), (14, 1024, 512, 1, 1), (14, 512, 512, 3, 2), (14, 256, 512, 3, 2),
    (14, 1024, 2048, 1, 2),
    (7, 512, 512, 3, 1), (7, 512, 2048, 1, 1), (7, 2048, 512, 1, 1),
)


def conv(n, hw, cin, cout, k, stride, /, **kw):   # kw: any field of hawq_conv_args, geometry included, set last
    a = _lib.ConvArgs()
    a.in_, a.wgt, a.bias = PTR, PTR, PTR
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad = n, hw, hw, cin, cout, k, k, stride, k // 2
    a.in_bits, a.w_bits = 8, 8
    for key, v in kw.items():
        setattr(a, key, v)
    return a


def with_fast(fields, fast):
    """fast_tables and the constant tables it needs."""
    out = dict(fields, fast_tables=fast)
    if fast:
        out["ctab"] = PTR
        if fields.get("in2"):
            out["ctab_id"] = PTR
    return out


SCALARS = dict(mq=3, eq=34, m_id_scalar=5, e_id_scalar=35)
RAW = dict(epilogue=_lib.EPI_RAW, out_acc=PTR)
REQUANT = dict(epilogue=_lib.EPI_REQUANT, out_q=PTR, out_bits=8, relu=1, q_lo=-128, q_hi=127, m=PTR, e=PTR)
REQUANT4 = dict(REQUANT, out_bits=4, q_lo=0, q_hi=15)
RES16 = dict(epilogue=_lib.EPI_RESIDUAL, m=PTR, e=PTR, out_q=PTR, out_bits=8, q_lo=0, q_hi=127, res_in=PTR, res_in_bits=16,
             res_out=PTR, res_out_bits=16, flags=PTR, **SCALARS)
RESIDUALS = {
    "res16": RES16,
    "res16_out4": dict(RES16, out_bits=4, q_hi=15),
    "res16_last": dict(RES16, out_q=None),                      # no next QuantAct
    "res16_noresout": dict(RES16, res_out=None),
    "res32in": dict(RES16, res_in_bits=32),
    "res32out": dict(RES16, res_out_bits=32, flags=None),
    "res32both": dict(RES16, res_in_bits=32, res_out_bits=32),
    "res_no_relu": dict(RES16, res_in_bits=32, res_out_bits=32, res_no_relu=1, q_lo=-128),
    "res_clamp16": dict(RES16, res_in=None, res_in_bits=0, res_out_bits=32, res_no_relu=1, res_clamp16=1, q_lo=-128),
    "res_noid": dict(RES16, res_in=None, res_in_bits=0, res_out_bits=32),
}
EPILOGUES = dict({"raw": RAW, "requant": REQUANT, "requant4": REQUANT4}, **RESIDUALS)


def identity(hw2, cin2, stride2, bits=(8, 8)):
    """The identity conv of a resize unit as second branch (per-channel identity tables, no stored residual)."""
    return dict(RES16, res_in=None, res_in_bits=0, in2=PTR, wgt2=PTR, bias2=PTR, m_id=PTR, e_id=PTR, H2=hw2, W2=hw2, Cin2=cin2,
                stride2=stride2, in2_bits=bits[0], w2_bits=bits[1])


def dequant(k, n_valid=1000):
    return dict(epilogue=_lib.EPI_DEQUANT, out_f32=PTR, fscale=PTR, ldo=n_valid, n_valid=n_valid)


PACKED = dict(wgt_band=PTR, wgt_k128=PTR, wgt2_k128=PTR)


def build_cases():
    cases = []

    def add(name, n, geo, fields):
        cases.append((f"{len(cases):04d}_{name}", conv(n, *geo, **fields)))

    def geo_name(n, g):
        return f"n{n}_hw{g[0]}_c{g[1]}x{g[2]}_k{g[3]}s{g[4]}"

    # 1. every geometry and batch: the heuristic (tile 0) for the forms the engines launch, general and fast contract
    for g in GEOMETRIES:
        for n in BATCHES:
            for ename, fast in (("requant", 0), ("requant", 1), ("res16", 0), ("res16", 1), ("res32both", 1)):
                add(f"geo_{geo_name(n, g)}_{ename}_f{fast}", n, g, with_fast(EPILOGUES[ename], fast))
    # the identity conv as second branch on the first unit of every stage (ResNet50 conv3 + identity, ResNet18 conv2 + identity)
    duals = (((56, 64, 256, 1, 1), identity(56, 64, 1)), ((28, 128, 512, 1, 1), identity(56, 256, 2)), ((14, 256, 1024, 1, 1), identity(28, 512, 2)),
             ((7, 512, 2048, 1, 1), identity(14, 1024, 2)), ((28, 128, 128, 3, 1), identity(56, 64, 2)), ((7, 512, 512, 3, 1), identity(14, 256, 2)))
    for g, ident in duals:
        for n in BATCHES:
            for fast in FAST:
                add(f"dual_{geo_name(n, g)}_f{fast}", n, g, with_fast(dict(ident, **PACKED), fast))
    # 2. every epilogue form x operand widths x fast_tables on one geometry per kernel size (packed weights offered and not)
    for g in ((28, 128, 128, 3, 1), (14, 1024, 256, 1, 1)):
        for ename, epi in EPILOGUES.items():
            for ab, wb in WIDTHS:
                for fast in FAST:
                    for packed in ({}, PACKED):
                        if (ab != wb and (packed or fast not in (0, 1))) or (packed and fast not in (1, 5)):
                            continue
                        add(f"epi_{geo_name(2, g)}_{ename}_a{ab}w{wb}_f{fast}_p{int(bool(packed))}", 2, g,
                            with_fast(dict(epi, in_bits=ab, w_bits=wb, **packed), fast))
    # widths per branch of a dual launch
    for g, ident_geo in (((14, 256, 1024, 1, 1), (28, 512, 2)), ((28, 128, 128, 3, 1), (56, 128, 2))):
        for ab, wb in WIDTHS:
            for ab2, wb2 in WIDTHS:
                for fast in (0, 1, 5):
                    add(f"dualw_{geo_name(2, g)}_a{ab}w{wb}_a{ab2}w{wb2}_f{fast}", 2, g,
                        with_fast(dict(identity(*ident_geo, bits=(ab2, wb2)), in_bits=ab, w_bits=wb, **PACKED), fast))
    # 3. layout flags: planar in / out with the heuristic and with every band tile, out_sub 2
    planar_geos = ((56, 64, 64, 3, 1), (28, 128, 128, 3, 1), (7, 512, 512, 3, 1), (14, 1024, 256, 1, 1))
    for g in planar_geos:
        for n in BATCHES:
            for ename in ("requant", "requant4", "res16", "raw"):
                for inp, outp in ((1, 0), (0, 1), (1, 1)):
                    for bits in ((8, 8), (4, 4)):
                        for packed in ({}, PACKED):
                            for fast in (0, 1, 5):
                                if n != 2 and ((inp, outp) != (1, 1) or fast != 1 or bits != (8, 8)):
                                    continue
                                if (fast == 0 and packed) or (fast == 5 and (packed or bits != (8, 8))):
                                    continue
                                add(f"planar_{geo_name(n, g)}_{ename}_i{inp}o{outp}_a{bits[0]}_f{fast}_p{int(bool(packed))}", n, g,
                                    with_fast(dict(EPILOGUES[ename], in_planar=inp, out_planar=outp, in_bits=bits[0], w_bits=bits[1], **packed), fast))
    for g in ((56, 64, 256, 1, 1), (28, 128, 512, 1, 1), (14, 256, 1024, 1, 1)):
        for n in BATCHES:
            for ename in ("res16_noresout", "res32in", "requant", "res16"):
                for fast in (0, 1):
                    add(f"sub2_{geo_name(n, g)}_{ename}_f{fast}", n, g, with_fast(dict(EPILOGUES[ename], out_sub=2, res_out=None), fast))
    # 4. MobileNetV2's narrow rows: pitches that are multiples of 16 below the padded 64-channel tile, with n_valid
    for hw, cin, cout, pin, pout, nv in ((56, 64, 64, 16, 0, 0), (56, 64, 64, 32, 0, 0), (56, 128, 64, 96, 32, 24), (28, 192, 64, 144, 32, 32),
                                         (14, 576, 128, 0, 96, 96), (7, 960, 192, 0, 160, 160), (28, 64, 192, 32, 144, 144), (14, 64, 64, 48, 48, 40)):
        for n in (2, 128):
            for ename in ("requant", "res_noid", "res_no_relu", "res16", "res32both"):
                for fast in (0, 1):
                    add(f"narrow_n{n}_hw{hw}_c{cin}x{cout}_p{pin}x{pout}_{ename}_f{fast}", n, (hw, cin, cout, 1, 1),
                        with_fast(dict(EPILOGUES[ename], in_pitch=pin, out_pitch=pout, n_valid=nv), fast))
    # 5. the FC as DEQUANT (1000 classes in 1024 padded channels)
    for k in (512, 2048):
        for n in BATCHES:
            for bits in WIDTHS:
                for tile in (0, 15):
                    add(f"fc_n{n}_k{k}_a{bits[0]}w{bits[1]}_t{tile}", n, (1, k, 1024, 1, 1), dict(dequant(k), in_bits=bits[0], w_bits=bits[1], tile=tile))
    # 6. every tile id (29 is invalid) on layers of every family
    sweeps = [("3x3c64", (56, 64, 64, 3, 1), REQUANT), ("3x3c64res", (56, 64, 64, 3, 1), RES16), ("3x3c128", (28, 128, 128, 3, 1), REQUANT),
              ("3x3c256", (14, 256, 256, 3, 1), RES16), ("3x3raw", (14, 256, 256, 3, 1), RAW),
              ("1x1k1024", (14, 1024, 256, 1, 1), REQUANT), ("1x1raw", (14, 1024, 256, 1, 1), RAW), ("1x1res", (14, 1024, 256, 1, 1), RES16),
              ("1x1dual", (14, 256, 1024, 1, 1), identity(28, 512, 2)), ("3x3s2", (28, 256, 256, 3, 2), REQUANT),
              ("3x3c512", (14, 512, 64, 3, 1), REQUANT)]
    for sname, g, epi in sweeps:
        for tile in range(NUM_TILES + 2):
            for n, bits, fast, inp in ((1, (8, 8), 0, 0), (128, (8, 8), 1, 1), (1, (4, 4), 5, 1), (2, (4, 4), 1, 1), (2, (8, 8), 5, 1)):
                if g[3] == 1:   # the 1x1 kernels read NHWC rows
                    inp = 0
                add(f"tile_{sname}_t{tile}_n{n}_a{bits[0]}_f{fast}_i{inp}", n, g,
                    with_fast(dict(epi, tile=tile, in_planar=inp, in_bits=bits[0], w_bits=bits[1], in2_bits=bits[0], w2_bits=bits[1], **PACKED), fast))
    cases.extend(invalid_cases(len(cases)))
    return cases


# One deliberately invalid struct per argument rule of hawq_conv2d: (fragment of the refusal text, geometry, fields).
G1 = (14, 256, 256, 1, 1)
G3 = (14, 256, 256, 3, 1)
DUAL = identity(28, 128, 2)
INVALID = (
    ("in/wgt/bias must be non-null", G1, dict(REQUANT, bias=None)),
    ("Cin=96 must be a positive multiple of 64", (14, 96, 256, 1, 1), REQUANT),
    ("Cout=100 must be a positive multiple of 64", (14, 256, 100, 1, 1), REQUANT),
    ("in_bits/w_bits must be 4 or 8 (got 2/8)", G1, dict(REQUANT, in_bits=2)),
    ("bad geometry", G1, dict(REQUANT, stride=0)),
    ("out_sub=2 needs a 1x1", G3, with_fast(dict(RES16, out_sub=2, res_out=None), 1)),
    ("empty output", (2, 256, 256, 5, 1), dict(REQUANT, pad=0)),
    ("problem too large", (16384, 64, 64, 1, 1), dict(REQUANT, N=8)),
    ("second branch needs HAWQ_EPI_RESIDUAL", G1, dict(DUAL, epilogue=_lib.EPI_REQUANT)),
    ("second branch tables missing", G1, dict(DUAL, m_id=None)),
    ("Cin2 must be a multiple of 64", G1, dict(DUAL, Cin2=96)),
    ("in2_bits/w2_bits must be 4 or 8", G1, dict(DUAL, w2_bits=16)),
    ("second branch output grid differs", G1, dict(DUAL, stride2=1)),
    ("in_pitch=40 needs a multiple of 16", G1, dict(REQUANT, in_pitch=40)),
    ("out_pitch=40 needs a multiple of 16", G1, dict(REQUANT, out_pitch=40)),
    ("out_pitch exists for single-branch", G1, dict(RAW, out_pitch=32)),
    ("out_pitch with fast_tables needs", G1, with_fast(dict(RES16, out_pitch=32), 1)),
    ("n_valid=48 exceeds out_pitch=32", G1, dict(REQUANT, out_pitch=32, n_valid=48)),
    ("fast_tables needs ctab (and ctab_id)", G1, dict(REQUANT, fast_tables=1)),
    ("fast RESIDUAL needs q_lo <= 0", G1, with_fast(dict(RES16, q_lo=1), 1)),
    ("bad (mq, eq)", G1, dict(RES16, eq=63)),
    ("fast_tables needs eq in [33,62]", G1, with_fast(dict(RES16, eq=20), 1)),
    ("fast_tables needs 0 <= q_hi <= 32767", G1, with_fast(dict(RES16, q_hi=40000), 1)),
    ("fast_tables bit 1 (no pre-shifts) but eq carries one", G1, with_fast(dict(RES16, eq=34 | 1 << 8), 3)),
    ("bad (m_id_scalar, e_id_scalar)", G1, dict(RES16, m_id_scalar=-1)),
    ("fast_tables needs e_id_scalar in [33,62]", G1, with_fast(dict(RES16, e_id_scalar=20), 1)),
    ("RAW needs out_acc", G1, dict(RAW, out_acc=None)),
    ("REQUANT needs out_q, m, e", G1, dict(REQUANT, m=None)),
    ("out_bits must be 4 or 8", G1, dict(REQUANT, out_bits=2)),
    ("RESIDUAL needs m, e", G1, dict(RES16, e=None)),
    ("res_in_bits 16/32", G1, dict(RES16, res_in_bits=8)),
    ("res_no_relu / res_clamp16 exist for single-branch launches", G1, dict(DUAL, res_clamp16=1)),
    ("fast_tables bit 1 is not defined for the signed", G1, with_fast(RESIDUALS["res_noid"], 3)),
    ("a residual stored without ReLU is signed", G1, dict(RES16, res_no_relu=1)),
    ("res_out_bits 16 (with flags) or 32", G1, dict(RES16, flags=None)),
    ("out_bits must be 4 or 8", G1, dict(RES16, out_bits=16)),
    ("RESIDUAL needs res_out and/or out_q", G1, dict(RES16, res_out=None, out_q=None)),
    ("DEQUANT needs out_f32, fscale, ldo", G1, dict(dequant(256), ldo=0)),
    ("unknown epilogue 7", G1, dict(REQUANT, epilogue=7)),
    ("in_planar / out_planar must be 0 or 1", G3, with_fast(dict(REQUANT, in_planar=2), 1)),
    ("out_planar needs the fast-contract", G1, dict(REQUANT, out_planar=1)),
    ("in_planar input but no 3x3 band kernel takes this layer", G1, with_fast(dict(REQUANT, in_planar=1), 1)),
    ("(round-5 1x1 kernel) does not apply", G3, with_fast(dict(REQUANT, tile=28, **PACKED), 1)),
    ("(round-5 3x3 kernel) does not apply", G1, with_fast(dict(REQUANT, tile=24, **PACKED), 1)),
    ("(weight-stationary 3x3 kernel) does not apply", G3, with_fast(dict(REQUANT, tile=22), 1)),
    ("(3x3 band kernel) does not apply", G1, with_fast(dict(REQUANT, tile=16), 1)),
    ("in_planar activations are read by the 3x3 band kernels only (tile 3 is not one)", G3, with_fast(dict(REQUANT, in_planar=1, tile=3), 1)),
    ("bad tile id 29", G1, dict(REQUANT, tile=29)),
    ("exact-tie mode (fast_tables bit 2) needs equal operand widths", G1, with_fast(dict(DUAL, in2_bits=4, w2_bits=4), 5)),
)
REQUIRE_TEXTS = tuple(text for text, _, _ in INVALID) + ("null args",)


def invalid_cases(start):
    return [(f"{start + i:04d}_invalid_{i:02d}", conv(2, *g, **fields)) for i, (_, g, fields) in enumerate(INVALID)]


# hawq_conv2d_splitk_ok / _workspace: the shapes of tests/test_splitk_host.py, taken and refused
def splitk_cases():
    def args(n, h, cin, cout, k, stride, epi, **kw):
        return conv(n, h, cin, cout, k, stride, **dict(epi, **kw))

    stage4 = lambda **kw: args(1, 7, 512, 512, 3, 1, dict(REQUANT, q_lo=0, q_hi=0, m=None, e=None), **kw)   # noqa: E731
    ident = lambda n=1: args(n, 14, 256, 1024, 1, 1, dict(identity(28, 512, 2), m=None, e=None, mq=0, eq=0, m_id_scalar=0, e_id_scalar=0))   # noqa: E731
    shapes = [("stage4_3x3", stage4()), ("stage4_raw", stage4(epilogue=_lib.EPI_RAW, out_acc=PTR)), ("stage4_planar_in", stage4(in_planar=1, fast_tables=1)),
              ("stage4_planar_out", stage4(out_planar=1, fast_tables=1)), ("stage4_planar_general", stage4(in_planar=1)),
              ("strided_3x3", args(1, 14, 512, 512, 3, 2, REQUANT)), ("strided_1x1", args(1, 14, 1024, 512, 1, 2, REQUANT)),
              ("conv3_identity", ident()), ("5x5", args(1, 14, 256, 256, 5, 1, REQUANT)), ("fc_like", args(16, 7, 512, 2048, 1, 1, REQUANT)),
              ("identity_w4", args(1, 14, 256, 1024, 1, 1, identity(28, 512, 2, bits=(4, 8)))),
              ("identity_requant", args(1, 14, 256, 1024, 1, 1, dict(identity(28, 512, 2), epilogue=_lib.EPI_REQUANT)))]
    for field, value in (("in_bits", 4), ("w_bits", 4), ("out_bits", 4), ("n_valid", 500), ("in_pitch", 256), ("out_pitch", 256),
                         ("epilogue", _lib.EPI_DEQUANT), ("out_sub", 2)):
        shapes.append((f"refused_{field}", stage4(**{field: value})))
    return [(f"{name}_s{s}", a, s) for name, a in shapes for s in (1, 2, 4, 5, 8, 16, 32)]
