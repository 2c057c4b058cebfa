"""InceptionV3's fused plan with grouped conv launches (hawq_amd/engine_inception.py: grouped=True, the ``"groups"`` field of a plan)
against the live reference's fixtures and against the default plan, bit for bit."""
import json

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_gpu_incep_tuned_network import _images, _load_reference_state, _num_tiles

pytestmark = pytest.mark.gpu

GROUP = "hawq_incep_conv_group"


@pytest.fixture(scope="module")
def calibrated():
    from hawq_amd.api import build_quantized_resnet, calibrate
    model = build_quantized_resnet("inceptionv3", "uniform8", seed=1).cuda()
    calibrate(model, _images(2).cuda())
    return model


def _u8(batch):
    return torch.randint(0, 256, (batch, 299, 299, 3), generator=torch.Generator().manual_seed(4 + batch), dtype=torch.uint8).cuda()


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
            assert y.abs().max() > 0 and base.n_launches == 147 and GROUP not in base.op_names
            cache[batch, use_graph] = (x, y, units, y8)
        return cache[batch, use_graph]
    return get


def _forced_groups_plan(eng, tile):
    """a plan for eng's batch shape: tile 0 on every conv launch, and every level of two or more convs that accepts `tile` as a group"""
    from hawq_amd.engine_inception import make_plan
    keys = eng.conv_launches
    groups = [{"convs": lv, "tile": tile} for lv in eng.conv_level_list if len(lv) >= 2 and eng._group_ok(lv, tile)]
    return make_plan(eng._batch, keys, _num_tiles(), [0] * len(keys), [{} for _ in keys], groups)


def _same(eng, x, y0, units0, model):
    with torch.no_grad():
        y = eng(x)
        assert torch.equal(eng(x), y)
    assert torch.equal(y, y0)
    for n, want in units0.items():
        assert np.array_equal(eng.unit_output(n), want), n


@pytest.mark.parametrize("scheme", ["uniform8", "uniform4"])
def test_grouped_plan_matches_reference_golden(scheme):
    from hawq_amd.api import build_quantized_resnet, calibrate
    fx = H.load(f"net_inceptionv3_{scheme}_b2.npz")
    x = _images()
    assert H.sha(x.numpy()) == str(fx["input_sha"])
    model = build_quantized_resnet("inceptionv3", scheme, seed=0).cuda()
    calibrate(model, x.cuda())
    _load_reference_state(model, fx)
    model.invalidate_engine()
    eng = model.engine(grouped=True)
    assert model.engine() is eng and eng.grouped
    with torch.no_grad():
        y = model(x.cuda())
    assert model._engine is eng and eng._graph is not None and eng.n_timing_launches == 0
    assert eng.n_launches == 100
    names = eng.op_names
    assert names.count(GROUP) == 27 and names.count("hawq_incep_conv") == 21
    assert len(eng.group_launches) == 27 and all(t == 3 for _, t in eng.group_launches)
    members = [c for convs, _ in eng.group_launches for c in convs]
    assert len(members) == len(set(members)) == 74
    assert sorted(map(sorted, (c for c, _ in eng.group_launches))) == sorted(lv for lv in eng.conv_level_list if len(lv) >= 2)
    assert len(eng.conv_launches) == 95
    for i, n in enumerate(fx["unit_names"]):
        assert np.array_equal(H.digest(eng.unit_output(str(n))), fx["unit_digest"][i]), n
    assert np.array_equal(y.cpu().numpy(), fx["logits"])
    model.invalidate_engine()
    assert model.engine().grouped is False


@pytest.mark.parametrize("config", ["plain", "tuned", "forced_tiles", "pools_and_stem", "uint8"])
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("batch", [2, 3])
def test_grouped_engine_equals_the_default_engine(calibrated, default_results, batch, use_graph, config):
    from hawq_amd.engine_inception import InceptionEngine
    model = calibrated
    x, y0, units0, y8 = default_results(batch, use_graph)
    if config == "plain":
        eng = InceptionEngine(model, use_graph=use_graph, grouped=True)
        _same(eng, x, y0, units0, model)
        assert eng.n_launches == 100 and eng.op_names.count(GROUP) == 27 and (eng._graph is not None) == use_graph
    elif config == "tuned":
        eng = InceptionEngine(model, use_graph=use_graph, grouped=True, tune=True)
        _same(eng, x, y0, units0, model)
        assert eng.n_timing_launches > 0 and len(eng.group_candidates) == 27
        assert eng.op_names.count(GROUP) == len(eng.group_launches) == sum(g["kept"] for g in eng.group_candidates)
        assert eng.n_launches == 147 - sum(len(c) - 1 for c, _ in eng.group_launches)
    elif config == "forced_tiles":
        probe = InceptionEngine(model, use_graph=False, grouped=True)
        with torch.no_grad():
            probe(x)
        for tile in range(1, _num_tiles() + 1):
            plan = json.loads(json.dumps(_forced_groups_plan(probe, tile)))
            assert len(plan["groups"]) > 0, f"tile {tile} takes no level of the network"
            eng = InceptionEngine(model, use_graph=use_graph, grouped=True, plan=plan)
            _same(eng, x, y0, units0, model)
            assert eng.n_timing_launches == 0
            assert [(sorted(c), t) for c, t in eng.group_launches] == [(sorted(g["convs"]), tile) for g in plan["groups"]]
        assert len(_forced_groups_plan(probe, 3)["groups"]) == 27
    elif config == "pools_and_stem":
        eng = InceptionEngine(model, use_graph=use_graph, grouped=True, fast_pools=True, fused_stem=True)
        _same(eng, x, y0, units0, model)
        assert eng.n_launches == 98 and eng.op_names.count(GROUP) == 27
        fast = [n for n, _ in eng.pool_launches].count("hawq_incep_pool_v")   # the pool launches followed their ops to the new order
        assert fast == eng.op_names.count("hawq_incep_pool_v") > 0 and len(eng.pool_launches) == 49
    else:
        eng = InceptionEngine(model, use_graph=use_graph, grouped=True)
        u8 = _u8(batch)
        with torch.no_grad():
            y = eng.forward_uint8(u8)
            assert torch.equal(eng.forward_uint8(u8), y)
        assert torch.equal(y, y8) and y8.abs().max() > 0
        assert eng.n_launches_u8 == 98 and [op.args[0] for op in eng._ops_u8].count(GROUP) == 27


def test_plans_with_and_without_groups(calibrated, default_results):
    from hawq_amd.engine import StalePlan
    from hawq_amd.engine_inception import InceptionEngine
    model = calibrated
    x, y0, _, _ = default_results(2, True)
    tuned = InceptionEngine(model, grouped=True, tune=True)
    with pytest.raises(RuntimeError):
        InceptionEngine(model, grouped=True).export_plan()
    with torch.no_grad():
        assert torch.equal(tuned(x), y0)
    plan = json.loads(json.dumps(tuned.export_plan()))
    assert [(g["convs"], g["tile"]) for g in plan["groups"]] == tuned.group_launches
    assert all(str(g["tile"]) in g["us"] and "singles" in g["us"] for g in plan["groups"])
    # the recorded groups replay on a fresh grouped engine without a timing launch
    replay = InceptionEngine(model, grouped=True, plan=plan)
    with torch.no_grad():
        assert torch.equal(replay(x), y0)
    assert replay.n_timing_launches == 0 and replay.group_launches == tuned.group_launches and replay.op_names == tuned.op_names
    assert replay.conv_tiles == plan["tiles"] and replay.export_plan() == plan
    # an engine without `grouped` ignores the field: the launch list of an ungrouped replay of the tile plan
    tiles_only = {k: v for k, v in plan.items() if k != "groups"}
    plain, plain_tiles = InceptionEngine(model, plan=plan), InceptionEngine(model, plan=tiles_only)
    with torch.no_grad():
        assert torch.equal(plain(x), y0) and torch.equal(plain_tiles(x), y0)
    assert plain.op_names == plain_tiles.op_names and plain.n_launches == 147 and GROUP not in plain.op_names
    assert plain.group_launches == [] and "groups" not in plain.export_plan()
    # a tile-only plan, as an ungrouped engine exports it, replays on a grouped engine with no grouped launch
    ungrouped = InceptionEngine(model, grouped=True, plan=json.loads(json.dumps(plain_tiles.export_plan())))
    with torch.no_grad():
        assert torch.equal(ungrouped(x), y0)
    assert ungrouped.group_launches == [] and GROUP not in ungrouped.op_names and ungrouped.n_launches == 147
    assert ungrouped.n_timing_launches == 0 and sorted(ungrouped.op_names) == sorted(plain_tiles.op_names)
    # stale groups
    lv = next(lv for lv in tuned.conv_level_list if len(lv) >= 2)
    for groups in ([{"convs": lv, "tile": 9}], [{"convs": lv[:-1] + [95], "tile": 3}], [{"convs": lv[:-1], "tile": 3}],
                   [{"convs": lv, "tile": 3}, {"convs": lv, "tile": 3}]):
        with pytest.raises(StalePlan):
            with torch.no_grad():
                InceptionEngine(model, grouped=True, plan=dict(tiles_only, groups=groups))(x)


def test_tuning_keeps_a_group_only_if_it_beats_its_members(calibrated, default_results):
    from hawq_amd.engine_inception import InceptionEngine
    x, y0, _, _ = default_results(2, True)
    eng = InceptionEngine(calibrated, grouped=True, tune=True, fast_pools=True, fused_stem=True)
    with torch.no_grad():
        assert torch.equal(eng(x), y0)
    assert len(eng.group_candidates) == 27
    kept = []
    for g in eng.group_candidates:
        us, best = g["us"], g["us"][str(g["tile"])]
        tiles = {k: v for k, v in us.items() if k != "singles"}
        singles = sum(eng.conv_us[c][eng.conv_tiles[c]] for c in g["convs"])
        print(g["convs"], "tile", g["tile"], "group us", round(best, 2), "singles us", round(singles, 2), "kept", g["kept"])
        assert us["singles"] == singles and best == min(tiles.values()) and len(tiles) >= 1
        assert g["kept"] == (best < singles)
        if g["kept"]:
            kept.append((g["convs"], g["tile"]))
    assert kept == eng.group_launches
