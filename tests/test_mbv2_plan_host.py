"""The host half of the MobileNetV2 engine's plan (hawq_amd/engine_mbv2.py), no GPU: the switches record, the pure predicates that
choose the form of a unit and of the init block, and what the launch records add up to."""
import pytest

from hawq_amd.engine_mbv2 import Launch, Switches, UnitShape, closing_is_fast, plan_totals, stem_form, unit_launches

ON = {"unfused": "HAWQ_MBV2_UNFUSED", "exact": "HAWQ_MBV2_EXACT", "pad64": "HAWQ_MBV2_PAD64", "no_wide_units": "HAWQ_MBV2_NO_WIDE_UNITS",
      "no_fc2": "HAWQ_NO_FC2"}


def test_switches_from_a_mapping():
    assert Switches.from_env({}) == Switches() == Switches(False, False, False, 0, False, False)
    for field, var in ON.items():
        assert Switches.from_env({var: "1"}) == Switches(**{field: True})
        assert Switches.from_env({var: "0"}) == Switches(**{field: True})   # os.environ.get truthiness: "0" is set
        assert Switches.from_env({var: ""}) == Switches()                   # ... and the empty string is not
    assert [Switches.from_env({"HAWQ_MBV2_UNIT_TILE": v}).unit_tile for v in ("0", "1", "3")] == [0, 1, 3]
    with pytest.raises(ValueError):   # int("") - as before, where the launch was built
        Switches.from_env({"HAWQ_MBV2_UNIT_TILE": ""})
    assert Switches.from_env({"HAWQ_MBV2_TILES": "0", "HAWQ_MBV2_CHAINS": "2", "HAWQ_TILES": "1"}) == Switches()   # not this record's
    assert [Switches(**{f: True}).round3 for f in ("unfused", "exact", "pad64", "no_wide_units", "no_fc2")] == [True, True, True, False, False]
    with pytest.raises(AttributeError):
        Switches().exact = True


# the 17 units of the width-1 network: (true input channels, true output channels, depthwise stride); 24 channels are stored as 32
W1 = [(32, 16, 1), (16, 24, 2), (24, 24, 1), (24, 32, 2), (32, 32, 1), (32, 32, 1), (32, 64, 2), (64, 64, 1), (64, 64, 1), (64, 64, 1),
      (64, 96, 1), (96, 96, 1), (96, 96, 1), (96, 160, 2), (160, 160, 1), (160, 160, 1), (160, 320, 1)]


def _units(size):
    """(UnitShape, input map side) per unit for size x size images, every table proved"""
    side, out = size // 2, []
    for k, (cin, cout, s) in enumerate(W1, start=1):
        u = UnitShape((cin + 15) // 16 * 16, cin * (1 if k == 1 else 6), (cout + 15) // 16 * 16, strides=(1, s, 1), residual=cin == cout and s == 1)
        out.append((u, side))
        side = (side - 1) // s + 1
    return out


def _one(size, sw=Switches(), tapped=False, k=None, **fields):
    """the numbers of the units that run as one launch; `fields` replace those of unit `k`"""
    forms = [unit_launches(sw, tapped, u._replace(**fields) if n == k else u, side, side) for n, (u, side) in enumerate(_units(size), start=1)]
    assert set(forms) <= {1, 3}
    return [n for n, f in enumerate(forms, start=1) if f == 1]


def _one224(k, **fields):
    return _one(224, k=k, **fields)


def test_the_width_1_network_at_224_and_288():
    assert [u.cin_s for u, _ in _units(224)][:5] == [32, 16, 32, 32, 32] and [side for _, side in _units(224)][-4:] == [14, 7, 7, 7]
    assert [u.residual for u, _ in _units(224)] == [k in (3, 5, 6, 8, 9, 10, 12, 13, 15, 16) for k in range(1, 18)]
    assert _one(224) == list(range(1, 17))                      # unit 17 (160 -> 320) is three launches
    assert [side for _, side in _units(288)][-4:] == [18, 9, 9, 9]
    assert _one(288) == list(range(1, 14))                      # 9 x 9 maps: the wide units 14 - 16 too


@pytest.mark.parametrize("field", ["unfused", "exact", "pad64"])
def test_round3_switches_and_tapped_plans_have_no_one_launch_unit(field):
    assert _one(224, Switches(**{field: True})) == []
    assert _one(224, tapped=True) == []


def test_unit_tile_1_and_no_wide_units():
    assert _one(224, Switches(unit_tile=1)) == list(range(1, 11))          # the 96-wide (11 - 13) and the wide units (14 - 16) drop out
    assert _one(224, Switches(unit_tile=2)) == _one(224, Switches(unit_tile=3)) == list(range(1, 17))
    assert _one(224, Switches(no_wide_units=True)) == list(range(1, 14))
    assert _one(224, Switches(no_fc2=True)) == list(range(1, 17))


@pytest.mark.parametrize("k", [1, 3, 9, 14, 16])
def test_what_puts_one_unit_back_on_three_launches(k):
    rest = [n for n in range(1, 17) if n != k]
    for i in range(4):   # one unproved table: conv1's, conv2's, conv3's, the next block-input scalar
        assert _one224(k, proved=tuple(j != i for j in range(4))) == rest
    assert _one224(k, tops=(255, 127)) == rest and _one224(k, tops=(127, 128)) == rest and _one224(k, tops=(127, 15)) == list(range(1, 17))
    residual = _units(224)[k - 1][0].residual
    assert _one224(k, id_proved=False) == (rest if residual else list(range(1, 17)))
    assert _one224(k, depthwise=False) == rest and _one224(k, kernels=(1, 3, 3)) == rest and _one224(k, kernels=((1, 3), 3, 1)) == rest
    assert _one224(k, strides=(2, 1, 1)) == rest and _one224(k, strides=(1, 1, 2)) == rest


def test_wide_units_need_small_output_maps_and_the_known_shapes():
    wide = UnitShape(160, 960, 160, residual=True)
    assert [unit_launches(Switches(), False, wide, h, w) for h, w in ((7, 7), (8, 8), (3, 4), (9, 8), (8, 9))] == [1, 1, 1, 3, 3]
    down = UnitShape(96, 576, 160, strides=(1, 2, 1))
    assert [unit_launches(Switches(), False, down, h, w) for h, w in ((14, 14), (16, 16), (17, 16), (5, 7))] == [1, 1, 3, 1]
    assert unit_launches(Switches(), False, UnitShape(160, 960, 320), 7, 7) == 3
    assert unit_launches(Switches(), False, UnitShape(160, 96, 160), 7, 7) == 3          # (hidden tensors of at most 96 channels: not that tile family)
    assert unit_launches(Switches(), False, UnitShape(96, 576, 160, strides=(1, 1, 1)), 7, 7) == 3
    assert unit_launches(Switches(), False, UnitShape(48, 288, 48), 7, 7) == 3           # a stored width the launch has no tile for


def test_stem_form():
    sw = Switches()
    assert stem_form(sw, False, True, 32, True) == "one" and stem_form(sw, False, True, 16, True) == "one"
    assert [stem_form(sw, False, True, c, True) for c in (48, 64, 8)] == ["im2col"] * 3
    assert stem_form(sw, False, True, 32, False) == "im2col"            # tables unproved
    assert stem_form(sw, True, True, 32, True) == "im2col"              # tapped
    assert stem_form(sw, False, False, 32, True) == stem_form(sw, True, False, 64, False) == "nhwc"   # not a 3x3 / stride 2 conv on 3 channels
    for field in ON:
        want = "im2col" if field in ("unfused", "exact", "pad64") else "one"
        assert stem_form(Switches(**{field: True}), False, True, 32, True) == want, field
        assert stem_form(Switches(**{field: True}), False, False, 32, True) == "nhwc"
    assert stem_form(Switches(unit_tile=1), False, True, 32, True) == "one"


def test_closing_is_fast():
    assert closing_is_fast(Switches(), True, True, True)
    assert not any(closing_is_fast(Switches(), *(j != i for j in range(3))) for i in range(3))
    assert not closing_is_fast(Switches(exact=True), True, True, True)
    assert closing_is_fast(Switches(unfused=True, pad64=True, unit_tile=1, no_wide_units=True, no_fc2=True), True, True, True)


def test_totals_of_a_hand_made_list_of_records():
    assert plan_totals([]) == dict(plan_bytes=0, n_fast=0, n_fused_units=0, n_fast_closing=0)
    records = [Launch("init_block", "hawq_stem3x3s2", (1, None), "stem", 1000, fast="closing"),
               Launch("unit1.conv3", "hawq_linear_bottleneck", (2,), "unit", 200, fast="closing"),
               Launch("unit2.conv1", "hawq_conv2d", (3,), "conv", 30, fast="expand"),
               Launch("unit2.conv2", "hawq_depthwise3x3_requant_fast", (4, 5), "depthwise", 4, geom=(1, 2, 3, 16, 16, 1)),
               Launch("unit2.conv3", "hawq_conv2d", (6,), "conv", 5),                       # an exact closing epilogue
               Launch("unit3.conv1", "hawq_conv2d", (7,), "conv", 6),                       # conv1 on the exact table
               Launch("unit3.conv1", "hawq_conv2d", (8,)),                                  # a RAW tap launch: no bytes, not tuned
               Launch("unit3.conv3", "hawq_linear_bottleneck", (9,), "unit", 7, fast="closing"),
               Launch("final_block", "hawq_conv2d", (10,), "conv", 8, fast="closing"),
               Launch("pool", "hawq_avgpool_requant", (11,)), Launch("output", "hawq_fc_dequant", (12,))]
    assert plan_totals(records) == dict(plan_bytes=1260, n_fast=1, n_fused_units=2, n_fast_closing=4)
    assert [r.kind for r in records].count("other") == 3 and records[0].taps == {} and records[3].geom[3] == 16
