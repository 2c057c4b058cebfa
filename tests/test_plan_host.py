"""hawq_amd/plan.py - the ResNet engine's launch plan as data - on the host: no GPU, no library."""
import json
import os

import pytest

from hawq_amd.plan import ChainChoice, StalePlan, decode, encode, expand_in8_of, from_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "profiles", "plans.json")) as _f:
    PLANS = json.load(_f)
R50, R101 = PLANS["resnet50_uniform8_b32"], PLANS["resnet101_uniform8_b128"]


def _decode(p, chain=0, on=None, **kw):
    """`p` against the build the plan `on` (default: `p` itself) was recorded on - its launch names, inventory and variant counts -
    with `kw` changed"""
    on = p if on is None else on
    a = dict(conv_names=on["conv_launches"], n_pairs=len(on["pair_launches"]), num_tiles=on["num_conv_tiles"],
             variant_counts=on["pair_variant_counts"])
    a.update(kw)
    return decode(p, chain, a["conv_names"], a["n_pairs"], a["num_tiles"], a["variant_counts"])


def _ints(s):
    return [int(v) for v in s.split(".")] if s else []


def test_plans_json_is_what_the_issue_counted():
    assert len(PLANS) == 9 and 0 < sum("per_chain" in p for p in PLANS.values()) < 9   # (both forms are covered below)
    assert all(p["num_conv_tiles"] == 28 for p in PLANS.values())
    assert not any("splitk" in p or "quant_output" in p["conv_launches"] for p in PLANS.values())


@pytest.mark.parametrize("key", sorted(PLANS))
def test_every_recorded_plan_round_trips(key):
    p = PLANS[key]
    choices = [_decode(p, i) for i in range(p["chains"])]
    for i, c in enumerate(choices):
        rec = p["per_chain"][i] if "per_chain" in p else p
        assert c.tiles == _ints(rec["tiles"]) and c.variants == _ints(rec["fused_variants"])
        assert [t for pair in c.split_tiles for t in pair] == _ints(rec["fused_split_tiles"])
        assert len(c.tiles) == len(p["conv_launches"]) and len(c.variants) == len(c.split_tiles) == len(p["pair_launches"])
        assert c.splitk == [0] * (len(c.tiles) + 2 * len(c.variants))
    got = encode(p["batch"], p["chains"], expand_in8_of(p), choices, p["conv_launches"], p["pair_launches"], p["num_conv_tiles"],
                 p["pair_variant_counts"])
    assert got == {k: v for k, v in p.items() if k not in ("git_head", "source")}
    assert json.loads(json.dumps(got)) == got


def test_recorded_plan_is_replayed_per_chain_and_by_launch_name():
    """A chain of a multi-chain engine reads ITS entry of a plan's `per_chain` list, the top-level strings where that entry is empty;
    a chain the plan does not list makes the plan stale; `chains` is never read per chain; nothing given, nothing fixed."""
    plan = {"chains": 2, "tiles": "1.2.3", "fused_variants": "1.0", "fused_split_tiles": "7.8.9.0", "num_conv_tiles": 28,
            "per_chain": [{"tiles": "1.2.3", "fused_variants": "1.0"}, {"chains": 5, "tiles": "4.5.6", "fused_variants": ""}]}
    dec = lambda p, chain: decode(p, chain, ["a", "b", "c"], 2, 28, [3, 1])
    assert dec(plan, 0) == ChainChoice([1, 2, 3], [1, 0], [(7, 8), (9, 0)], [0] * 7)
    assert dec(plan, 1).tiles == [4, 5, 6]
    assert dec(plan, 1).variants == [1, 0] and dec(plan, 1).split_tiles == [(7, 8), (9, 0)]   # empty / absent entries: the top level
    assert dec({k: v for k, v in plan.items() if k != "per_chain"}, 1).tiles == [1, 2, 3]       # no list: every chain reads the top level
    assert plan["chains"] == 2 and "chains" not in ChainChoice._fields
    with pytest.raises(StalePlan, match="lists 2 chains"):
        dec(plan, 2)
    # plan not applicable to this batch shape and no measurement switch set: tune
    assert from_env({}) == {}
    nothing = dec(dict(from_env({}), num_conv_tiles=28), 1)
    assert nothing.tiles is None and nothing.variants is None and not any(nothing.splitk)


def test_each_way_a_plan_goes_stale():
    with pytest.raises(StalePlan, match="another launch list"):    # a superset recorded for a larger network
        _decode(R101, on=R50)
    assert set(R50["conv_launches"]) < set(R101["conv_launches"])
    with pytest.raises(StalePlan, match="another launch list"):
        _decode(dict(R50, conv_launches=R50["conv_launches"][:-1]), on=R50)
    with pytest.raises(StalePlan, match="tile inventory"):
        _decode(R50, num_tiles=R50["num_conv_tiles"] + 1)
    with pytest.raises(StalePlan, match="tile inventory"):
        _decode({k: v for k, v in R50.items() if k != "num_conv_tiles"}, on=R50)
    with pytest.raises(StalePlan, match="numbered differently"):
        _decode(R50, variant_counts=[c + 1 for c in R50["pair_variant_counts"]])
    assert "0" in R50["fused_variants"].split(".")
    no_split = {k: v for k, v in R50.items() if k != "per_chain"}
    with pytest.raises(StalePlan, match="lists no tiles for them"):
        _decode(dict(no_split, fused_split_tiles=""))
    n = len(R50["conv_launches"]) + 2 * len(R50["pair_launches"])
    with pytest.raises(StalePlan, match=f"lists {n - 1} split-K entries, this plan has {n} launches"):
        _decode(dict(R50, splitk=".".join(["0"] * (n - 1))))
    assert _decode(dict(R50, splitk=".".join(["0"] * n))) == _decode(R50)
    with pytest.raises(StalePlan, match="tiles, this plan has"):     # no names recorded: the count still has to fit
        _decode({k: v for k, v in no_split.items() if k != "conv_launches"}, on=R50, conv_names=R50["conv_launches"][:-1])
    assert issubclass(StalePlan, ValueError)


def test_a_launch_no_longer_tuned_is_dropped_by_name():
    for chain in (0, 1):
        rec = dict(R50, conv_launches=R50["conv_launches"] + ["quant_output"], tiles=R50["tiles"] + ".9",
                   per_chain=[dict(pc, tiles=pc["tiles"] + ".9") for pc in R50["per_chain"]])
        assert _decode(rec, chain, on=R50) == _decode(R50, chain)
    # ... and only such a launch: any other extra name is another launch list
    with pytest.raises(StalePlan, match="another launch list"):
        _decode(dict(R50, conv_launches=R50["conv_launches"] + ["stage9.unit1.quant_convbn1"], tiles=R50["tiles"] + ".9"), on=R50)


def test_defaults_of_plans_recorded_before_a_key_existed():
    old = {k: v for k, v in PLANS["resnet50_uniform8_b128"].items() if k not in ("fused_variants", "per_chain", "expand_in8", "splitk")}
    c = _decode(old)
    assert c.variants == [1] * len(old["pair_launches"]) and c.splitk == [0] * (len(old["conv_launches"]) + 2 * len(old["pair_launches"]))
    assert expand_in8_of(old) == "1" and expand_in8_of(R50) == "2" and expand_in8_of({"expand_in8": ""}) == "1"


def test_measurement_switches_decode_like_a_plan():
    n = len(R50["conv_launches"]) + 2 * len(R50["pair_launches"])
    env = {"HAWQ_TILES": R50["tiles"], "HAWQ_ER_TILES": R50["fused_variants"], "HAWQ_ER_SPLIT_TILES": R50["fused_split_tiles"],
           "HAWQ_SPLITK": ".".join(["0"] * n), "HAWQ_CHAINS": "2", "PATH": "/bin"}
    assert set(from_env(env)) == {"tiles", "fused_variants", "fused_split_tiles", "splitk"}
    assert _decode(dict(from_env(env), num_conv_tiles=28), on=R50) == _decode(R50, 0)
    # HAWQ_ER_TILES alone: time the tiles, pin the pairs
    pairs = {k: env[k] for k in ("HAWQ_ER_TILES", "HAWQ_ER_SPLIT_TILES")}
    c = _decode(dict(from_env(pairs), num_conv_tiles=28), on=R50)
    assert c.tiles is None and c.variants == _decode(R50, 0).variants and c.split_tiles == _decode(R50, 0).split_tiles
    assert from_env({"HAWQ_TILES": ""}) == {}


def test_encode_writes_split_k_for_every_chain_once_any_chain_splits():
    c0 = ChainChoice([3, 4], [2], [(5, 6)], [0, 0, 0, 0])
    c1 = c0._replace(splitk=[0, 4, 0, 0])
    got = encode(8, 2, "2", [c0, c1], ["a", "b"], ["p"], 28, [3])
    assert "splitk" not in got and [p["splitk"] for p in got["per_chain"]] == ["0.0.0.0", "0.4.0.0"]
    assert got["per_chain"][0] == {"tiles": "3.4", "fused_variants": "2", "fused_split_tiles": "5.6", "splitk": "0.0.0.0"}
    assert [decode(got, i, ["a", "b"], 1, 28, [3]) for i in (0, 1)] == [c0, c1]
    both = encode(8, 2, "2", [c1, c1], ["a", "b"], ["p"], 28, [3])
    assert both["splitk"] == "0.4.0.0" and "per_chain" not in both
    assert "splitk" not in encode(8, 1, "2", [c0], ["a", "b"], ["p"], 28, [3])
