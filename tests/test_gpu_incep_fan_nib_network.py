"""InceptionV3 uniform4 on nibble-packed operands with fan-out epilogues on its grouped launches (hawq_amd/engine_inception.py:
nibble=True, nibble_fan=True) against the default plan, bit for bit."""
import json

import pytest
import torch

from tests.test_gpu_incep_nib_network import default4, model4  # noqa: F401  (the fixtures: model, seed and batch sizes)

pytestmark = pytest.mark.gpu
FAN_NIB = "hawq_incep_conv_group_nib_fan"


def _check_issued(eng):
    """every entry requant the plan dropped or shortened is accounted for: its boundary is a kept one, whose producers are all
    members of its fan launches and whose residual ranges are exactly the shortened requants"""
    from hawq_amd.engine_inception import fan_boundaries
    bounds = {b["unit"]: b for b in fan_boundaries(eng._launches, eng._nib_pool)}
    kept = [f["unit"] for f in eng.fan_candidates if f["kept"]]
    assert sorted({u for u, _, _ in eng.fan_launches}) == kept and all(bounds[u]["candidate"] for u in kept)
    assert eng.op_names.count(FAN_NIB) == len(eng.fan_launches) == len(eng.nibble_fan_masks)
    for u in kept:
        members = [c for v, convs, _ in eng.fan_launches if v == u for c in convs]
        assert len(members) == len(set(members)) and {eng._launches[i].ref for i in bounds[u]["producers"]} <= set(members)
    want = [(u, i, off, c) for u in kept for i in bounds[u]["requants"] for off, c in bounds[u]["residual"]]
    assert sorted(eng.residual_requants) == sorted(want)
    # launches fewer than without the option, and the forms of the kept boundaries' fan outputs
    return sum(len(bounds[u]["requants"]) for u in kept) - len(want), {f for u in kept for f in bounds[u]["forms"]}


def _unit_on_int8(model, x, unit):
    """a plan (tile 0 everywhere) whose ``"nibble"`` field is the untuned choice without the convs of `unit`: that unit's entry
    requants stay int8, so the fan outputs of the boundary in front of it are int8 ones, carried by hawq4 members"""
    from hawq_amd.engine_inception import InceptionEngine
    from tests.test_gpu_incep_tuned_network import _forced_plan
    probe = InceptionEngine(model, nibble=True, use_graph=False)
    with torch.no_grad():
        probe(x)
    plan = _forced_plan(probe, 0)
    plan["nibble"] = [[c, t] for c, t in sorted(probe.nibble_convs.items()) if probe._convs[c].place != unit]
    assert 0 < len(plan["nibble"]) < len(probe.nibble_convs)
    return json.loads(json.dumps(plan))


# The untuned uniform4 plan stores every entry requant of a candidate boundary hawq4, so its fan outputs are all hawq4; "unit5_int8"
# replays a plan that keeps unit 5 on int8, which puts int8 fan outputs (on hawq4 producers) into the same network.
@pytest.mark.parametrize("kw", [{"nibble_groups": True}, {"nibble_groups": True, "fast_pools": True, "fused_stem": True}, {},
                                {"nibble_groups": True, "plan": 5}],
                         ids=["groups", "groups+fast_pools+fused_stem", "groups_of_one", "unit5_int8"])
def test_nibble_fan_equals_the_default_engine(model4, default4, kw):   # noqa: F811
    from hawq_amd.engine_inception import InceptionEngine
    x, y0, u8, y8, _ = default4
    if "plan" in kw:
        kw = dict(kw, plan=_unit_on_int8(model4, x, kw["plan"]))
    eng = model4.engine(nibble=True, nibble_fan=True, **kw)
    with torch.no_grad():
        y = eng(x)
        assert torch.equal(eng(x), y) and torch.equal(y, y0)
        assert torch.equal(eng.forward_uint8(u8), y8)
    assert eng.n_timing_launches == 0 and eng._graph is not None
    plain = InceptionEngine(model4, nibble=True, **kw)
    with torch.no_grad():
        plain(x)
    saved, forms = _check_issued(eng)
    assert saved > 0 and eng.n_launches == plain.n_launches - saved and FAN_NIB not in plain.op_names
    # a launch with a hawq4 fan output (a fan_mask bit); with a unit on int8, a boundary whose fan outputs are int8 as well
    assert any(eng.nibble_fan_masks) and forms == ({4, 8} if "plan" in kw else {4})
    model4.invalidate_engine()


def test_tuned_nibble_fans_and_their_plan(model4, default4):   # noqa: F811
    from hawq_amd.engine import StalePlan
    from hawq_amd.engine_inception import InceptionEngine
    x, y0, _, _, _ = default4
    kw = dict(nibble=True, nibble_groups=True, nibble_fan=True)
    tuned = InceptionEngine(model4, tune=True, **kw)
    with torch.no_grad():
        assert torch.equal(tuned(x), y0)
    assert tuned.fan_candidates
    for f in tuned.fan_candidates:
        print("boundary", f["unit"], "plain us", round(f["us"]["plain"], 2), "fan us", round(f["us"]["fan"], 2), f["tiles"], "kept", f["kept"])
        assert f["kept"] == (f["us"]["fan"] < f["us"]["plain"])
    _check_issued(tuned)
    plan = json.loads(json.dumps(tuned.export_plan()))
    assert [e["unit"] for e in plan["nibble_fan"]] == [f["unit"] for f in tuned.fan_candidates if f["kept"]]
    replay = InceptionEngine(model4, plan=plan, **kw)
    with torch.no_grad():
        assert torch.equal(replay(x), y0)
    assert replay.n_timing_launches == 0 and replay.op_names == tuned.op_names and replay.export_plan() == plan
    assert replay.fan_launches == tuned.fan_launches and replay.nibble_fan_masks == tuned.nibble_fan_masks
    plain = InceptionEngine(model4, nibble=True, nibble_groups=True, plan=plan)   # an engine without the option ignores the field
    with torch.no_grad():
        assert torch.equal(plain(x), y0)
    assert FAN_NIB not in plain.op_names and plain.fan_launches == [] and "nibble_fan" not in plain.export_plan()
    # stale entries: a unit that is no candidate, a wrong producer set, a refused tile
    f = next(f for f in tuned.fan_candidates)
    entry = {"unit": f["unit"], "tiles": dict(f["tiles"])}
    for stale in ([dict(entry, unit=0)], [{"unit": f["unit"], "tiles": {"0": 2}}], [{"unit": f["unit"], "tiles": {k: 3 for k in entry["tiles"]}}]):
        with pytest.raises(StalePlan), torch.no_grad():
            InceptionEngine(model4, plan=dict(plan, nibble_fan=stale), **kw)(x)
