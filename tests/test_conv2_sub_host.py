"""Host side of the stage-final 3x3 convs on the next stage's grid: hawq_conv2d's check / choose for out_sub on a 3x3 launch and
for "res_sub" (H2 / W2 / stride2 of a single-branch RESIDUAL launch) on the expand conv behind it (hawq_conv2d_choice: no device), the band extents of the strided twins of the round-5 3x3
kernels from the function the kernels themselves use, and the engine's decision helper on every shipped graph.  No GPU."""
import ctypes as C

import pytest

from hawq_amd import _lib
from tests.conv_choice_cases import PACKED, PTR, RAW, REQUANT, REQUANT4, RES16, conv, with_fast

FAM_PLAIN, FAM_BAND2 = 0, 3
# outputs per pixel tile, band pixels per LDS stage, LDS bytes, threads of the strided twins, in tile-id order
TWINS = [(128, 768, 2 * 4 * 768 * 16 + 4 * 12288 + 1024, 384), (64, 512, 2 * 4 * 512 * 16 + 4 * 12288 + 1024, 256)]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _choice(lib, a):
    ch = _lib.ConvChoice()
    rc = lib.hawq_conv2d_choice(C.byref(a), C.byref(ch))
    return rc, ch, lib.hawq_last_error().decode() if rc else ""


def _band2_ids(lib):
    n, nb2, ng2 = lib.hawq_conv2d_num_tiles(), lib.hawq_conv2d_num_band2_tiles(), lib.hawq_conv2d_num_gemm2_tiles()
    return list(range(n - ng2 - nb2 + 1, n - ng2 + 1))


def _sub(n, s=2):
    return (n - 1) // s + 1


@pytest.mark.parametrize("n,hw,c", [(64, 28, 128), (64, 14, 256), (3, 14, 128), (5, 9, 256)])
@pytest.mark.parametrize("epi", [REQUANT, REQUANT4, RAW])
def test_strided_3x3_on_the_twins_of_the_round5_kernels(lib, n, hw, c, epi):
    assert lib.hawq_conv2d_num_tiles() == 28 and len(_band2_ids(lib)) == len(TWINS)   # the ids stay: recorded plans stay readable
    m_out = n * _sub(hw) ** 2
    for tile, (bm, band_px, lds, nt) in zip(_band2_ids(lib), TWINS):
        for bits in (8, 4):
            cin = c if bits == 8 else 2 * c   # (hawq4: a 128-byte pixel row needs 256 channels)
            for fast in (1, 5):
                a = conv(n, hw, cin, 128, 3, 1, **with_fast(dict(epi, out_sub=2, in_planar=1, tile=tile, in_bits=bits, w_bits=bits, **PACKED), fast))
                rc, ch, err = _choice(lib, a)
                assert rc == 0, err
                assert (ch.family, ch.tile, ch.stride, ch.res_sub, ch.Ho, ch.Wo, ch.M) == (FAM_BAND2, tile, 2, 0, _sub(hw), _sub(hw), m_out)
                assert (ch.grid, ch.block, ch.lds_bytes) == (-(-m_out // bm) * 2, nt, lds)
                raw = epi is RAW
                assert ch.fn_table == (3 if raw else 2) and list(ch.fn) == [int(bits == 4), -1 if raw else int(fast == 5), -1]
                # the dense launch of the same struct keeps the table slots it had
                a.out_sub = 0
                rc, ch0, err = _choice(lib, a)
                assert rc == 0 and ch0.fn_table == int(raw) and ch0.stride == 1 and ch0.M == n * hw * hw
    # left to the library (tile 0) a planar strided launch resolves to the first twin that takes it
    a = conv(64, 28, 128, 128, 3, 1, **with_fast(dict(REQUANT, out_sub=2, in_planar=1, **PACKED), 1))
    rc, ch, err = _choice(lib, a)
    assert rc == 0 and ch.tile == _band2_ids(lib)[0] == lib.hawq_conv2d_band2_tile(C.byref(a))


def test_strided_3x3_on_the_general_tiles(lib):
    n_general = lib.hawq_conv2d_num_tiles() - lib.hawq_conv2d_num_band_tiles()
    assert n_general == 15
    for hw, c in ((56, 64), (28, 128), (14, 256)):
        for epi in (REQUANT, REQUANT4, RAW):
            for fast in (0, 1, 5):
                for tile in range(0, n_general + 1):
                    a = conv(64, hw, c, c, 3, 1, **with_fast(dict(epi, out_sub=2, tile=tile), fast))
                    rc, ch, err = _choice(lib, a)
                    assert rc == 0, (tile, err)
                    assert (ch.family, ch.stride, ch.res_sub, ch.Ho, ch.Wo, ch.M) == (FAM_PLAIN, 2, 0, hw // 2, hw // 2, 64 * (hw // 2) ** 2)
                    # exactly the launch of the 3x3 / stride 2 conv on the same map
                    b = conv(64, hw, c, c, 3, 2, **with_fast(dict(epi, tile=tile), fast))
                    rc, chb, err = _choice(lib, b)
                    assert rc == 0 and all(getattr(ch, f) == getattr(chb, f) for f, _ in _lib.ConvChoice._fields_ if f != "fn") and list(ch.fn) == list(chb.fn)


def test_refusal_texts(lib):
    text = "out_sub=2 needs a 1x1 / stride 1 / pad 0 single-branch RESIDUAL launch without res_out, dense NHWC rows"
    fast = lambda f: with_fast(f, 1)   # noqa: E731
    refused = [conv(2, 14, 256, 256, 3, 1, **fast(dict(RES16, out_sub=2, res_out=None))),          # no RESIDUAL form on a 3x3
               conv(2, 14, 256, 256, 3, 1, **fast(dict(REQUANT, out_sub=2, out_planar=1))),
               conv(2, 14, 256, 256, 3, 2, **fast(dict(REQUANT, out_sub=2))),
               conv(2, 14, 256, 256, 3, 1, **fast(dict(REQUANT, out_sub=2, pad=0))),
               conv(2, 14, 256, 256, 5, 1, **fast(dict(REQUANT, out_sub=2))),
               conv(2, 14, 256, 256, 1, 1, **fast(dict(REQUANT, out_sub=2)))]                     # a 1x1 subsamples with RESIDUAL only
    for a in refused:
        rc, _, err = _choice(lib, a)
        assert rc != 0 and err == "hawq_conv2d: " + text, err
    # every special-purpose 3x3 id but the round-5 ones refuses the field through its query
    n, nsp = lib.hawq_conv2d_num_tiles(), lib.hawq_conv2d_num_band_tiles()
    for planar in (0, 1):
        for tile in range(n - nsp + 1, n + 1):
            if tile in _band2_ids(lib):
                continue
            a = conv(64, 56, 64, 64, 3, 1, **fast(dict(REQUANT, out_sub=2, tile=tile, in_planar=planar, **PACKED)))
            rc, _, err = _choice(lib, a)
            assert rc != 0 and "does not apply to this layer" in err, (tile, err)
    a = conv(64, 56, 64, 64, 3, 1, **fast(dict(REQUANT, out_sub=2, **PACKED)))
    assert lib.hawq_conv2d_band_tile(C.byref(a)) == 0 and lib.hawq_conv2d_splitk_ok(C.byref(a), 3) == 0
    a.out_sub = 0
    assert lib.hawq_conv2d_band_tile(C.byref(a)) != 0 and lib.hawq_conv2d_splitk_ok(C.byref(a), 3) == 1
    # a 64-channel int8 row is a single slice: the round-5 kernels refuse it dense and strided (the engine then keeps NHWC rows)
    a = conv(64, 56, 64, 64, 3, 1, **fast(dict(REQUANT, out_sub=2, in_planar=1, **PACKED)))
    assert lib.hawq_conv2d_band2_tile(C.byref(a)) == 0
    rc, _, err = _choice(lib, a)
    assert rc != 0 and "in_planar input but no 3x3 band kernel takes this layer" in err


def test_res_sub_check_and_choice(lib):
    res = dict(RES16, res_out=None)
    a = conv(64, 28, 64, 256, 1, 1, **with_fast(dict(res, stride2=2, H2=56, W2=56), 1))
    rc, ch, err = _choice(lib, a)
    assert rc == 0, err
    assert (ch.family, ch.stride, ch.res_sub, ch.Ho, ch.Wo, ch.M) == (FAM_PLAIN, 1, 2, 28, 28, 64 * 28 * 28)
    # the same grid, tile and function as the out_sub launch on the full map
    b = conv(64, 56, 64, 256, 1, 1, **with_fast(dict(res, out_sub=2), 1))
    rc, chb, err = _choice(lib, b)
    assert rc == 0 and (ch.tile, ch.grid, ch.block, ch.lds_bytes, ch.fn_table, list(ch.fn), ch.M) == \
        (chb.tile, chb.grid, chb.block, chb.lds_bytes, chb.fn_table, list(chb.fn), chb.M)
    assert (chb.stride, chb.res_sub) == (2, 2)
    a.H2 = 55   # (55 - 1) / 2 + 1 == 28 as well: an odd full map
    assert _choice(lib, a)[0] == 0
    for fields in (dict(H2=57), dict(W2=58), dict(out_sub=2), dict(res_out=PTR), dict(stride=2), dict(KH=3, KW=3, pad=1), dict(out_planar=1)):
        bad = conv(64, 28, 64, 256, 1, 1, **with_fast(dict(dict(res, stride2=2, H2=56, W2=56), **fields), 1))
        rc, _, err = _choice(lib, bad)
        assert rc != 0 and ("(stride2 without in2)=2 needs a 1x1" in err or "out_sub=2 needs a 1x1" in err), (fields, err)
    # the three fields keep their old meaning everywhere else: a second branch's geometry, or - no stored residual, another epilogue - nothing
    for fields in (dict(res_in=None, res_in_bits=0, res_out_bits=32), dict(epilogue=_lib.EPI_REQUANT, res_in=None)):
        plain = conv(64, 28, 64, 256, 1, 1, **with_fast(dict(dict(res, stride2=2, H2=56, W2=56), **fields), 1))
        rc, ch, err = _choice(lib, plain)
        assert rc == 0 and ch.res_sub == 0, (fields, err)
    # the streaming 1x1 kernels, split-K
    n = lib.hawq_conv2d_num_tiles()
    for tile in range(lib.hawq_conv2d_gemm2_first(), n + 1):
        g = conv(64, 28, 128, 512, 1, 1, **with_fast(dict(res, tile=tile, **PACKED), 1))
        assert _choice(lib, g)[0] == 0
        g.stride2, g.H2, g.W2 = 2, 56, 56
        rc, _, err = _choice(lib, g)
        assert rc != 0 and "does not apply to this layer" in err
    s = conv(1, 7, 512, 2048, 1, 1, **with_fast(res, 1))
    assert lib.hawq_conv2d_splitk_ok(C.byref(s), 2) == 1
    s.stride2, s.H2, s.W2 = 2, 14, 14
    assert lib.hawq_conv2d_splitk_ok(C.byref(s), 2) == 0 and "res_sub is not supported" in lib.hawq_last_error().decode()


def test_expand_reduce_variant_counts_do_not_move_with_res_sub(lib):
    for c in (64, 128, 256):
        er = _lib.ExpandReduceArgs()
        full = conv(64, 56, c, 4 * c, 1, 1, **with_fast(dict(RES16, res_out=None), 1))
        C.memmove(C.byref(er.expand), C.byref(full), C.sizeof(full))
        n0 = lib.hawq_conv_expand_reduce_variants(C.byref(er))
        assert n0 >= 1
        er.expand.out_sub = 2
        assert lib.hawq_conv_expand_reduce_variants(C.byref(er)) == n0
        er.expand.out_sub, er.expand.H, er.expand.W = 0, 28, 28
        er.expand.stride2, er.expand.H2, er.expand.W2 = 2, 56, 56
        assert lib.hawq_conv_expand_reduce_variants(C.byref(er)) == n0
        er.expand.H2 = 60
        assert lib.hawq_conv_expand_reduce_variants(C.byref(er)) == 0
        # a pair refuses the field on either conv
        er.expand.H2 = 56
        red = conv(64, 28, 4 * c, c, 1, 1, **with_fast(REQUANT, 1))
        C.memmove(C.byref(er.reduce), C.byref(red), C.sizeof(red))
        assert lib.hawq_conv_expand_reduce_variants(C.byref(er)) == 0


# ---------------------------------------------------------------------------------------------- band extents
def _walk(lib, n, h, w, index):
    """(worst band length, band pixels per stage, tiles) over EVERY pixel tile of the strided 3x3 launch on an [n][h][w] map, with
    each tile's band checked against the pixels its outputs' windows touch."""
    a = conv(n, h, 128, 128, 3, 1, **with_fast(dict(REQUANT, out_sub=2, in_planar=1, **PACKED), 1))
    a.W = w
    ext = (C.c_int32 * 5)()
    assert lib.hawq_conv2d_band2_sub_extent(C.byref(a), index, 0, ext) == 0
    tiles, bm, band_px = ext[3], ext[4], ext[2]
    ho, wo = _sub(h), _sub(w)
    m_out = n * ho * wo
    assert tiles == -(-m_out // bm) and (bm, band_px) == TWINS[index][:2]

    def src(m):
        i, r = divmod(m, ho * wo)
        y, x = divmod(r, wo)
        return (i * h + 2 * y) * w + 2 * x
    worst = 0
    for t in range(tiles):
        assert lib.hawq_conv2d_band2_sub_extent(C.byref(a), index, t, ext) == 0
        first, length = ext[0], ext[1]
        lo, hi = src(t * bm), src(min((t + 1) * bm, m_out) - 1)
        assert first % 8 == 0 and lo - w - 1 - 7 <= first <= lo - w - 1       # line-aligned, at most 7 pixels early
        assert first + length - 1 == hi + w + 1                               # ends at the last output's bottom-right tap
        worst = max(worst, length)
    assert lib.hawq_conv2d_band2_sub_extent(C.byref(a), index, tiles, ext) != 0
    return worst, band_px, a


@pytest.mark.parametrize("n,h,w", [(2, 7, 7), (3, 6, 10), (5, 9, 9), (3, 14, 14), (64, 56, 56), (64, 28, 28), (64, 14, 14), (1, 8, 120), (1, 8, 250)])
def test_band_extent_of_every_tile_and_the_query_that_rests_on_it(lib, n, h, w):
    takers = []
    for index, tile in enumerate(_band2_ids(lib)):
        worst, band_px, a = _walk(lib, n, h, w, index)
        a.tile = tile
        rc, ch, err = _choice(lib, a)
        fits = worst <= band_px - 4
        assert (rc == 0) == fits, (index, worst, band_px, err)
        takers.append(fits)
    a.tile = 0
    assert (lib.hawq_conv2d_band2_tile(C.byref(a)) != 0) == any(takers)
    if (h, w) in ((56, 56), (28, 28), (14, 14)):
        assert all(takers)        # the three stage-final maps fit both twins
    if w >= 250:
        assert not any(takers)    # refused, not launched: the engine keeps NHWC rows and a general tile runs


# ---------------------------------------------------------------------------------------------- the engine's decision
def _decisions(arch, monkeypatch=None, **env):
    """{unit name: (s, full map -> small map)} for the units whose 3x3 conv runs on the next stage's grid: IntegerEngine._handover, the
    engine's own decision, asked for every unit of the float skeleton (the unit records carry what _handover reads of the engine's)."""
    from types import SimpleNamespace as NS
    from hawq_amd.engine import IntegerEngine, out_sub_extent
    from hawq_amd.skeleton import build_float_resnet
    net = build_float_resnet(arch)
    named = [(f"{sn}.{un}", u) for sn, stage in net.features.named_children() if sn.startswith("stage")
             for un, u in stage.named_children()]
    geom = lambda blk: NS(kh=blk.conv.kernel_size[0], kw=blk.conv.kernel_size[1], stride=blk.conv.stride[0], pad=blk.conv.padding[0])   # noqa: E731
    units = [dict(name=name, resize=bool(u.resize_identity), convs=[dict(conv=geom(b)) for _, b in u.body.named_children()],
                  ident=geom(u.identity_conv) if u.resize_identity else None) for name, u in named]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = NS(keep_acc=False)
    out, hw = {}, 56
    for ui, u in enumerate(units):
        hw_unit = hw
        for e in u['convs']:
            c = e['conv']
            hw = (hw + 2 * c.pad - c.kh) // c.stride + 1
        sub_out, c2_sub = IntegerEngine._handover(eng, units, ui)
        assert c2_sub in (0, sub_out)
        if c2_sub:
            out[u['name']] = (c2_sub, hw_unit, out_sub_extent(hw_unit, c2_sub))
    return out


def test_which_units_get_the_field(monkeypatch):
    from hawq_amd.skeleton import ARCH
    want = {"resnet50": {"stage1.unit3": (2, 56, 28), "stage2.unit4": (2, 28, 14), "stage3.unit6": (2, 14, 7)},
            "resnet101": {"stage1.unit3": (2, 56, 28), "stage2.unit4": (2, 28, 14), "stage3.unit23": (2, 14, 7)},
            "resnet50b": {}, "resnet18": {}}
    assert set(want) == set(ARCH)
    for arch in ARCH:
        assert _decisions(arch) == want[arch], arch
    # the switches: every 3x3 conv on every pixel again
    assert _decisions("resnet50", monkeypatch, HAWQ_NO_CONV2_SUB="1") == {}
    monkeypatch.delenv("HAWQ_NO_CONV2_SUB")
    assert _decisions("resnet50", monkeypatch, HAWQ_NO_OUT_SUB="1") == {}


def test_decision_helper_corner_cases():
    from hawq_amd.engine import conv2_sub_stride
    bott = [(1, 1, 1, 0), (3, 3, 1, 1), (1, 1, 1, 0)]
    assert conv2_sub_stride(2, bott) == 2 and conv2_sub_stride(3, bott) == 3
    assert conv2_sub_stride(0, bott) == 0 and conv2_sub_stride(1, bott) == 0                 # the next unit reads every pixel
    assert conv2_sub_stride(2, [(3, 3, 1, 1), (3, 3, 1, 1)]) == 0                              # basic block
    assert conv2_sub_stride(2, [(1, 1, 1, 0), (3, 3, 2, 1), (1, 1, 1, 0)]) == 0                # the stride on conv2
    assert conv2_sub_stride(2, [(1, 1, 1, 0), (3, 3, 1, 0), (1, 1, 1, 0)]) == 0                # an unpadded window is not centred on (s y, s x)
    assert conv2_sub_stride(2, [(1, 1, 1, 0), (5, 5, 1, 2), (1, 1, 1, 0)]) == 0
    assert conv2_sub_stride(2, [(1, 1, 1, 0), (3, 3, 1, 1), (3, 3, 1, 1)]) == 0                # the last conv must need one pixel only
    assert conv2_sub_stride(2, [(2, 2, 1, 0), (3, 3, 1, 1), (1, 1, 1, 0)]) == 2                # conv1 keeps every pixel whatever it is
