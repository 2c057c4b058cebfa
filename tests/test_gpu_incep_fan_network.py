"""InceptionV3's fused plan with fan-out conv epilogues (hawq_amd/engine_inception.py: fan_out=True, the ``"fan_out"`` field of a plan)
against the live reference's fixtures and against the default plan, bit for bit; and the launch lists of every engine without the
option against the digests of the lists they issued before the option existed."""
import hashlib
import json

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_gpu_incep_group_network import _forced_groups_plan, _same, _u8
from tests.test_gpu_incep_tuned_network import _forced_plan, _images, _load_reference_state

pytestmark = pytest.mark.gpu

FAN, GROUP, REQUANT, POOL_V = "hawq_incep_conv_group_fan", "hawq_incep_conv_group", "hawq_incep_requant", "hawq_incep_pool_v"
# Per consumer unit: entry requants in the default plan, and residual requants with fan-out (0: every slice of its input is
# conv-produced).  Unit 0 reads the stem's max pool and is no candidate; units 4 and 9 read a max-pool branch's slice (288 of 768 and
# 768 of 1280 channels), unit 10 the two inner-concat requants' (1536 of 2048, adjacent, one range).
ENTRY = [3, 3, 3, 2, 3, 3, 3, 3, 2, 3, 3]
RESIDUAL = {4: (480, 288), 9: (512, 768), 10: (320, 1536)}
# Producer convs per boundary: the convs that write a slice of the previous unit's concat buffer.
PRODUCERS = {1: 4, 2: 4, 3: 4, 4: 2, 5: 4, 6: 4, 7: 4, 8: 4, 9: 2, 10: 2}
N_DEFAULT, N_GROUPED = 128, 81   # 147 - 19 and 100 - 19: the 19 entry requants of units 1, 2, 3, 5, 6, 7, 8


@pytest.fixture(scope="module")
def calibrated():
    from hawq_amd.api import build_quantized_resnet, calibrate
    model = build_quantized_resnet("inceptionv3", "uniform8", seed=1).cuda()
    calibrate(model, _images(2).cuda())
    return model


@pytest.fixture(scope="module")
def default_results(calibrated):
    """logits, unit outputs and uint8 logits of the default engine per (batch, use_graph): computed once, never changed"""
    from hawq_amd.engine_inception import InceptionEngine
    cache = {}

    def get(batch, use_graph):
        if (batch, use_graph) not in cache:
            base = InceptionEngine(calibrated, use_graph=use_graph)
            x = _images(batch, seed=11 + batch).cuda()
            with torch.no_grad():
                y = base(x)
                units = {n: base.unit_output(n) for n, _ in calibrated.units()}
                y8 = base.forward_uint8(_u8(batch))
            assert y.abs().max() > 0 and base.n_launches == 147 and FAN not in base.op_names and base.fan_launches == []
            cache[batch, use_graph] = (x, y, units, y8)
        return cache[batch, use_graph]
    return get


def _check_issued(eng, grouped):
    """what the writer issued is what the boundary function over the records says, and the table of the issue holds"""
    from hawq_amd.engine_inception import fan_boundaries
    bounds = fan_boundaries(eng._launches)
    assert [len(b["requants"]) for b in bounds] == ENTRY and sum(ENTRY) == 31
    assert [b["unit"] for b in bounds if b["candidate"]] == list(range(1, 11))
    assert {b["unit"]: len(b["producers"]) for b in bounds if b["candidate"]} == PRODUCERS
    assert {b["unit"]: b["residual"] for b in bounds if b["residual"] and b["candidate"]} == {k: [v] for k, v in RESIDUAL.items()}
    chosen = {f["unit"] for f in eng.fan_candidates if f["kept"]}
    want_resid = [(b["unit"], i, off, c) for b in bounds if b["unit"] in chosen for i in b["requants"] for off, c in b["residual"]]
    assert sorted(eng.residual_requants) == sorted(want_resid)
    producers = {b["unit"]: sorted(eng._launches[i].ref for i in b["producers"]) for b in bounds}
    for unit in chosen:   # every producer of a chosen boundary is in exactly one fan launch of that boundary
        members = [c for u, convs, _ in eng.fan_launches if u == unit for c in convs]
        assert len(members) == len(set(members)) and set(producers[unit]) <= set(members)
        assert grouped or sorted(members) == producers[unit]
    assert {u for u, _, _ in eng.fan_launches} == chosen
    names = eng.op_names
    assert names.count(FAN) == len(eng.fan_launches)
    return bounds


@pytest.mark.parametrize("scheme", ["uniform8", "uniform4"])
def test_fan_out_plan_matches_reference_golden(scheme):
    from hawq_amd.api import build_quantized_resnet, calibrate
    fx = H.load(f"net_inceptionv3_{scheme}_b2.npz")
    x = _images()
    assert H.sha(x.numpy()) == str(fx["input_sha"])
    model = build_quantized_resnet("inceptionv3", scheme, seed=0).cuda()
    calibrate(model, x.cuda())
    _load_reference_state(model, fx)
    model.invalidate_engine()
    eng = model.engine(fan_out=True)
    assert model.engine() is eng and eng.fan_out
    with torch.no_grad():
        y = model(x.cuda())
    assert model._engine is eng and eng._graph is not None and eng.n_timing_launches == 0
    assert eng.n_launches == N_DEFAULT
    _check_issued(eng, False)
    names = eng.op_names
    assert names.count(FAN) == sum(PRODUCERS.values()) == 34 and names.count("hawq_incep_conv") == 95 - 34
    assert names.count(REQUANT) == 31 - 19 + 4   # the 12 kept entry requants, shortened, and the 8 x 8 units' inner-concat requants
    for i, n in enumerate(fx["unit_names"]):
        assert np.array_equal(H.digest(eng.unit_output(str(n))), fx["unit_digest"][i]), n
    assert np.array_equal(y.cpu().numpy(), fx["logits"])
    model.invalidate_engine()
    assert model.engine().fan_out is False


CONFIGS = {"alone": {}, "fast_pools": {"fast_pools": True}, "fused_stem": {"fused_stem": True}, "grouped": {"grouped": True},
           "tile_plan": {"plan": 3}, "all": {"fast_pools": True, "fused_stem": True, "grouped": True, "plan": 3}}


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("batch", [2, 3])
def test_fan_out_engine_equals_the_default_engine(calibrated, default_results, batch, use_graph, config):
    from hawq_amd.engine_inception import InceptionEngine
    model, kw = calibrated, dict(CONFIGS[config])
    x, y0, units0, y8 = default_results(batch, use_graph)
    if "plan" in kw:   # a tile plan recorded without the option: tile 3 wherever a conv launch takes it
        probe = InceptionEngine(model, use_graph=False)
        with torch.no_grad():
            probe(x)
        plan = _forced_plan(probe, kw["plan"])
        if kw.get("grouped"):   # with its levels as groups on that tile, as a grouped engine records them
            plan["groups"] = _forced_groups_plan(probe, kw["plan"])["groups"]
        kw["plan"] = json.loads(json.dumps(plan))
        assert "fan_out" not in kw["plan"]
    eng = InceptionEngine(model, use_graph=use_graph, fan_out=True, **kw)
    _same(eng, x, y0, units0, model)
    assert eng.n_timing_launches == 0 and (eng._graph is not None) == use_graph
    grouped, stem = bool(kw.get("grouped")), 2 * bool(kw.get("fused_stem"))
    assert eng.n_launches == (N_GROUPED if grouped else N_DEFAULT) - stem
    _check_issued(eng, grouped)
    assert len(eng.fan_candidates) == 10 and all(f["kept"] for f in eng.fan_candidates)
    names = eng.op_names
    if grouped:
        assert len(eng.group_launches) == 27 and names.count(GROUP) + sum(len(c) > 1 for _, c, _ in eng.fan_launches) == 27
    else:
        assert names.count(FAN) == 34 and GROUP not in names
    # unit 0's three entry requants and the four inner-concat requants of the 8 x 8 units are there in either plan
    resid = names.count(POOL_V) if kw.get("fast_pools") else names.count(REQUANT) - 3 - 4
    assert len(eng.residual_requants) == 9 and (resid >= 9 if kw.get("fast_pools") else resid == 9)
    with torch.no_grad():   # the uint8 chain shares the tail
        u8 = _u8(batch)
        y = eng.forward_uint8(u8)
        assert torch.equal(eng.forward_uint8(u8), y)
    assert torch.equal(y, y8) and y8.abs().max() > 0
    assert eng.n_launches_u8 == (N_GROUPED if grouped else N_DEFAULT) - 2
    assert [op.args[0] for op in eng._ops_u8].count(FAN) == names.count(FAN)


def test_tuning_keeps_a_boundary_only_if_fan_out_is_faster_and_the_plan_replays(calibrated, default_results):
    from hawq_amd.engine import StalePlan
    from hawq_amd.engine_inception import InceptionEngine
    model = calibrated
    x, y0, units0, _ = default_results(2, True)
    tuned = InceptionEngine(model, tune=True, fan_out=True, grouped=True, fast_pools=True, fused_stem=True)
    _same(tuned, x, y0, units0, model)
    assert tuned.n_timing_launches > 0 and [f["unit"] for f in tuned.fan_candidates] == list(range(1, 11))
    for f in tuned.fan_candidates:
        us = f["us"]
        print("boundary", f["unit"], "plain us", round(us["plain"], 2), "fan-out us", round(us["fan"], 2), "tiles", f["tiles"], "kept", f["kept"])
        assert f["kept"] == (us["fan"] < us["plain"])
        for key, tile in f["tiles"].items():   # every producer launch on the fastest of the tiles that were timed for it
            timed = {int(k.split("@")[1]): v for k, v in us.items() if k.startswith(key + "@")}
            assert timed and tile == min(timed, key=lambda t: (timed[t], t))
    kept = [f["unit"] for f in tuned.fan_candidates if f["kept"]]
    _check_issued(tuned, True)
    assert sorted({u for u, _, _ in tuned.fan_launches}) == kept
    dropped = sum(ENTRY[u] for u in kept if u not in RESIDUAL)
    assert tuned.n_launches == 147 - 2 - sum(len(c) - 1 for c, _ in tuned.group_launches) - dropped
    # the record replays with no timing launch and issues the same launches
    plan = json.loads(json.dumps(tuned.export_plan()))
    assert [e["unit"] for e in plan["fan_out"]] == kept and all("plain" in e["us"] and "fan" in e["us"] for e in plan["fan_out"])
    replay = InceptionEngine(model, plan=plan, fan_out=True, grouped=True, fast_pools=True, fused_stem=True)
    _same(replay, x, y0, units0, model)
    assert replay.n_timing_launches == 0 and replay.op_names == tuned.op_names
    assert replay.fan_launches == tuned.fan_launches and replay.residual_requants == tuned.residual_requants
    assert replay.export_plan() == plan
    # an engine without the option ignores the field
    plain = InceptionEngine(model, plan=plan, grouped=True, fast_pools=True, fused_stem=True)
    _same(plain, x, y0, units0, model)
    assert FAN not in plain.op_names and plain.fan_launches == [] and "fan_out" not in plain.export_plan()
    assert plain.n_launches == 145 - sum(len(c) - 1 for c, _ in plain.group_launches)
    # a record with no boundary replays with none; stale entries are refused
    none = InceptionEngine(model, plan=dict(plan, fan_out=[]), fan_out=True, grouped=True, fast_pools=True, fused_stem=True)
    _same(none, x, y0, units0, model)
    assert none.op_names == plain.op_names and none.fan_launches == []
    entry = {"unit": 1, "tiles": dict(next(f for f in tuned.fan_candidates if f["unit"] == 1)["tiles"])}
    bad_tile = {"unit": 1, "tiles": {k: 9 for k in entry["tiles"]}}
    for stale in ([dict(entry, unit=0)], [dict(entry, unit=11)], [bad_tile], [entry, entry], [{"unit": 1, "tiles": {"0": 3}}], [{"unit": 1}]):
        with pytest.raises(StalePlan):
            with torch.no_grad():
                InceptionEngine(model, plan=dict(plan, fan_out=stale), fan_out=True, grouped=True, fast_pools=True, fused_stem=True)(x)


# sha256 over "\n".join(op_names) of the engines without the option, at batch 2, as they were before the option existed
PARENT_OP_NAMES = {
    "default": "0b7636cbaef6306eb9583a3f63ca296ca3ac65c2628e3fbbc0eb5468992b590a",
    "fast_pools": "e262f19cb0ed6b8d3b094dda4583530cce8145b9ac47122c75bf555a68978f62",
    "fused_stem": "76fbfc83c65d3a24c6110f3f01b3d6e9becc8a2c60a75710bc5a67859bc73ae7",
    "grouped": "5d686bc55f1dc9ffce1e8a430966a14fa50d8c6686a5199a55267d330e62c9f6",
    "tile_plan": "eabaf7f79ab6216cdc02efb259d05748acd9979e2b91937ed59fd0ee27a256c7",
    "all": "ec35508db011624f54043f3c8580aaacb64b08cde045c2b16daebdbfcd20bf25",
}


@pytest.mark.parametrize("config", list(PARENT_OP_NAMES))
def test_engines_without_the_option_issue_the_launches_they_issued_before(calibrated, default_results, config):
    from hawq_amd.engine_inception import InceptionEngine
    x, y0, units0, _ = default_results(2, True)
    kw = dict(CONFIGS.get(config, {}))
    if "plan" in kw:
        probe = InceptionEngine(calibrated, use_graph=False)
        with torch.no_grad():
            probe(x)
        kw["plan"] = _forced_plan(probe, kw["plan"])
    eng = InceptionEngine(calibrated, **kw)
    _same(eng, x, y0, units0, calibrated)
    assert FAN not in eng.op_names and eng.fan_launches == [] and eng.residual_requants == [] and eng.fan_candidates == []
    digest = hashlib.sha256("\n".join(eng.op_names).encode()).hexdigest()
    print(config, eng.n_launches, digest)
    assert digest == PARENT_OP_NAMES[config]
