"""InceptionV3's fused plan on tuned / replayed conv tiles (hawq_amd/engine_inception.py: tune=True, plan=, export_plan) against the
live reference's fixtures and against the default plan, bit for bit."""
import hashlib
import json

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu


def _images(b=2, seed=0):
    from hawq_amd.skeleton import synthetic_images
    return synthetic_images(b, seed=seed, size=299)


def _load_reference_state(model, fx):
    """The reference run's frozen ranges and integer buffers (weights patched where torch-CPU's sqrt moved them) into `model`
    (as tests/test_gpu_inception_network.py loads them)."""
    from hawq_amd.quant_modules import QuantAct, QuantBnConv2d, freeze_model
    acts = [(n, m) for n, m in model.named_modules() if isinstance(m, QuantAct)]
    convs = [(n, m) for n, m in model.named_modules() if isinstance(m, QuantBnConv2d)]
    assert [n for n, _ in acts] == [str(n) for n in fx["act_names"]]
    assert [n for n, _ in convs] == [str(n) for n in fx["conv_names"]]
    for i, (n, m) in enumerate(acts):
        m.x_min.fill_(float(fx["act_x_min"][i])), m.x_max.fill_(float(fx["act_x_max"][i]))
        m.compute_scale()
        assert m.act_scaling_factor.item() == float(fx["act_scale"][i]), n
    freeze_model(model)
    off = 0
    for li, (n, m) in enumerate(convs):
        m.prepare(torch.ones(1))
        w = m.weight_integer.detach().cpu().numpy().copy()
        for l, idx, val in fx["conv_wpatch"]:
            if l == li:
                w.reshape(-1)[idx] = val
        assert hashlib.sha256(np.ascontiguousarray(w.astype(np.int8)).tobytes()).hexdigest() == str(fx["conv_wsha"][li]), n
        co, dev = w.shape[0], m.weight_integer.device
        m.weight_integer = torch.from_numpy(w).to(dev)
        m.convbn_scaling_factor = torch.from_numpy(fx["conv_scale"][off:off + co].copy()).to(dev)
        m.bias_integer = torch.from_numpy(fx["conv_bias"][off:off + co].astype(np.float32)).to(dev)
        m.use_integer_buffers, m._prep_key = True, None
        off += co
    assert off == fx["conv_scale"].size
    return model


@pytest.fixture(scope="module")
def calibrated():
    from hawq_amd.api import build_quantized_resnet, calibrate
    model = build_quantized_resnet("inceptionv3", "uniform8", seed=1).cuda()
    calibrate(model, _images(2).cuda())
    return model


def _num_tiles():
    from hawq_amd import _lib
    return _lib.load().hawq_incep_conv_num_tiles()


def _forced_plan(eng, tile):
    """a plan for eng's current batch shape with `tile` on every conv launch that accepts it and tile 0 elsewhere"""
    from hawq_amd.engine_inception import make_plan
    keys = eng.conv_launches
    tiles = [tile if eng._tile_ok(i, tile) else 0 for i in range(len(keys))]
    return make_plan(eng._batch, keys, _num_tiles(), tiles, [{} for _ in keys])


@pytest.mark.parametrize("scheme", ["uniform8", "uniform4"])
def test_tuned_plan_matches_reference_golden(scheme):
    """On the reference's frozen ranges and integer buffers every unit output and the logits of the tuned plan are the fixture's."""
    from hawq_amd.api import build_quantized_resnet, calibrate
    fx = H.load(f"net_inceptionv3_{scheme}_b2.npz")
    x = _images()
    assert H.sha(x.numpy()) == str(fx["input_sha"])
    model = build_quantized_resnet("inceptionv3", scheme, seed=0).cuda()
    calibrate(model, x.cuda())
    _load_reference_state(model, fx)
    model.invalidate_engine()
    eng = model.engine(tune=True)
    assert model.engine() is eng
    with torch.no_grad():
        y = model(x.cuda())
    assert model._engine is eng and eng.conv_tiles is not None and len(eng.conv_tiles) == 95
    assert eng.n_timing_launches > 0 and eng._graph is not None
    assert eng.n_launches == 147
    names = eng.op_names
    assert names.count("hawq_incep_conv_tiled") == 95 and "hawq_incep_conv" not in names
    for i, n in enumerate(fx["unit_names"]):
        assert np.array_equal(H.digest(eng.unit_output(str(n))), fx["unit_digest"][i]), n
    assert np.array_equal(y.cpu().numpy(), fx["logits"])
    # every measured launch has tile 0's time and the chosen tile is the fastest measured
    for t, us in zip(eng.conv_tiles, eng.conv_us):
        assert 0 in us and t in us and us[t] == min(us.values()) and us[t] <= us[0]
    model.invalidate_engine()
    assert model.engine().conv_tiles is None and model.engine().tune is False


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("batch", [2, 3])
def test_every_tile_forced_everywhere_equals_the_default_plan(calibrated, batch, use_graph):
    from hawq_amd.engine_inception import InceptionEngine
    model = calibrated
    x = _images(batch, seed=11 + batch).cuda()
    base = InceptionEngine(model, use_graph=use_graph)
    with torch.no_grad():
        y0 = base(x)
        assert torch.equal(base(x), y0)
    units0 = {n: base.unit_output(n) for n, _ in model.units()}
    assert y0.abs().max() > 0
    for tile in range(1, _num_tiles() + 1):
        plan = _forced_plan(base, tile)
        assert plan["tiles"].count(tile) > 0, f"tile {tile} is accepted by no conv launch of the network"
        eng = InceptionEngine(model, use_graph=use_graph, plan=json.loads(json.dumps(plan)))
        with torch.no_grad():
            y = eng(x)
            y_again = eng(x)
        assert eng.conv_tiles == plan["tiles"] and eng.n_timing_launches == 0
        assert (eng._graph is not None) == use_graph
        assert torch.equal(y, y0) and torch.equal(y_again, y0), f"tile {tile}"
        for n, want in units0.items():
            assert np.array_equal(eng.unit_output(n), want), (tile, n)


def test_forward_uint8_of_a_tuned_engine_equals_the_default_engine(calibrated):
    from hawq_amd.engine_inception import InceptionEngine
    model = calibrated
    u8 = torch.randint(0, 256, (2, 299, 299, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).cuda()
    base, tuned = InceptionEngine(model), InceptionEngine(model, tune=True)
    with torch.no_grad():
        y0, y1 = base.forward_uint8(u8), tuned.forward_uint8(u8)
        assert torch.equal(tuned.forward_uint8(u8), y1)
    assert torch.equal(y0, y1) and y0.abs().max() > 0
    assert tuned.n_launches_u8 == 145 and base.n_launches_u8 == 145
    # the uint8 plan shares the choice: all its conv launches but conv1 (the stem kernel) are the tuned ones
    assert tuned._ops_u8[1:] == tuned._ops[tuned._at[tuned._convs[0]] + 1:]   # after conv1's launch
    for t in range(1, _num_tiles() + 1):
        forced = InceptionEngine(model, plan=_forced_plan(tuned, t))
        with torch.no_grad():
            assert torch.equal(forced.forward_uint8(u8), y0), t


def test_plan_round_trip_and_stale_plans(calibrated):
    from hawq_amd.engine import StalePlan
    from hawq_amd.engine_inception import InceptionEngine
    model = calibrated
    x = _images(2, seed=5).cuda()
    tuned = model.engine(tune=True)
    with torch.no_grad():
        y = model(x)
    assert tuned.n_timing_launches > 0
    with pytest.raises(RuntimeError):
        InceptionEngine(model).export_plan()
    plan = json.loads(json.dumps(tuned.export_plan()))
    T = _num_tiles()
    assert plan["batch"] == [2, 299, 299] and plan["num_tiles"] == T and plan["tiles"] == tuned.conv_tiles
    assert len(plan["tiles"]) == len(plan["us"]) == plan["n_launches"] == 95
    assert all("0" in us and str(t) in us for t, us in zip(plan["tiles"], plan["us"]))
    replay = model.engine(plan=plan)
    assert replay is not tuned and model.engine() is replay
    with torch.no_grad():
        y2 = model(x)
    assert replay.conv_tiles == plan["tiles"] and replay.n_timing_launches == 0
    assert torch.equal(y, y2)
    assert replay.export_plan() == plan
    with pytest.raises(StalePlan):
        with torch.no_grad():
            replay(_images(3, seed=5).cuda())        # another batch shape
    with torch.no_grad():
        assert torch.equal(replay(x), y)             # the refusal left no half-built plan behind
    bad = dict(plan, tiles=[T + 1] + plan["tiles"][1:])
    with pytest.raises(StalePlan):
        with torch.no_grad():
            InceptionEngine(model, plan=bad)(x)
    bad = dict(plan, num_tiles=T + 1)
    with pytest.raises(StalePlan):
        with torch.no_grad():
            InceptionEngine(model, plan=bad)(x)
    model.invalidate_engine()
    assert model.engine().plan is None and model.engine().conv_tiles is None


def test_default_engine_is_unchanged(calibrated):
    from hawq_amd.engine_inception import InceptionEngine
    model = calibrated
    model.invalidate_engine()
    x = _images(2, seed=5).cuda()
    u8 = torch.randint(0, 256, (2, 299, 299, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).cuda()
    with torch.no_grad():
        model(x)
    eng = model.engine()
    assert isinstance(eng, InceptionEngine) and eng.tune is False and eng.plan is None
    with torch.no_grad():
        eng.forward_uint8(u8)
    assert eng.n_launches == 147 and eng.n_launches_u8 == 145
    names = eng.op_names
    assert names.count("hawq_incep_conv") == 95 and "hawq_incep_conv_tiled" not in names
    assert [op.args[0] for op in eng._ops_u8].count("hawq_incep_conv") == 94
    assert "hawq_incep_conv_tiled" not in [op.args[0] for op in eng._ops_u8]
    assert eng.n_timing_launches == 0 and eng.conv_tiles is None and len(eng.conv_launches) == 95
