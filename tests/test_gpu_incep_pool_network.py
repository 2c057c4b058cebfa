"""InceptionV3's fused plan with ``fast_pools=True`` (hawq_amd/engine_inception.py: the 49 pool / requant launches on
``hawq_incep_pool_v``, hawq_amd/csrc/incep_pool.hip) against the default engine, the live reference's fixtures and the CPU oracle, bit
for bit, and the structure of its launch list."""
import json

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_gpu_incep_tuned_network import _images, _load_reference_state

pytestmark = pytest.mark.gpu

OLD_POOLS = ("hawq_incep_requant", "hawq_incep_maxpool3s2", "hawq_incep_avgpool_branch", "hawq_incep_global_avgpool")


@pytest.fixture(scope="module")
def calibrated():
    from hawq_amd.api import build_quantized_resnet, calibrate
    model = build_quantized_resnet("inceptionv3", "uniform8", seed=0).cuda()
    calibrate(model, _images(2).cuda())
    return model


def _pools(eng):
    """(op index, argument block, op id) of every pool / requant launch, read from the engine's launch records"""
    return [(eng._at[r], r.args[0], r.ref) for r in eng._launches if r.kind == "pool"]


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("batch", [2, 3])
def test_fast_pools_equal_the_default_engine(calibrated, batch, use_graph):
    from hawq_amd.engine_inception import InceptionEngine
    model = calibrated
    x = _images(batch, seed=11 + batch).cuda()
    base, fast = InceptionEngine(model, use_graph=use_graph), InceptionEngine(model, use_graph=use_graph, fast_pools=True)
    with torch.no_grad():
        y0, y1 = base(x), fast(x)
        y2 = fast(x)
    assert (fast._graph is not None) == use_graph
    assert y0.abs().max() > 0 and torch.equal(y1, y0) and torch.equal(y2, y0)
    for n, _ in model.units():
        want = base.unit_output(n)
        assert np.abs(want).max() > 0 and np.array_equal(fast.unit_output(n), want), n


@pytest.mark.parametrize("scheme", ["uniform8", "uniform4"])
def test_fast_pools_match_reference_golden(scheme):
    """On the reference's frozen ranges and integer buffers every unit output and the logits are the fixture's."""
    from hawq_amd.api import build_quantized_resnet, calibrate
    fx = H.load(f"net_inceptionv3_{scheme}_b2.npz")
    x = _images()
    assert H.sha(x.numpy()) == str(fx["input_sha"])
    model = build_quantized_resnet("inceptionv3", scheme, seed=0).cuda()
    calibrate(model, x.cuda())
    _load_reference_state(model, fx)
    model.invalidate_engine()
    eng = model.engine(fast_pools=True)
    assert model.engine() is eng and eng.fast_pools
    with torch.no_grad():
        y = model(x.cuda())
    assert model._engine is eng
    assert eng.op_names.count("hawq_incep_pool_v") == 49
    for i, n in enumerate(fx["unit_names"]):
        assert np.array_equal(H.digest(eng.unit_output(str(n))), fx["unit_digest"][i]), n
    assert np.array_equal(y.cpu().numpy(), fx["logits"])
    model.invalidate_engine()
    assert model.engine().fast_pools is False


def test_tuned_fast_pools_and_forward_uint8_equal_the_default_engine(calibrated):
    from hawq_amd.engine_inception import InceptionEngine
    model = calibrated
    x = _images(2, seed=5).cuda()
    u8 = torch.randint(0, 256, (2, 299, 299, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).cuda()
    base, fast = InceptionEngine(model), InceptionEngine(model, tune=True, fast_pools=True)
    with torch.no_grad():
        assert torch.equal(fast(x), base(x))
        y0, y1 = base.forward_uint8(u8), fast.forward_uint8(u8)
        assert torch.equal(fast.forward_uint8(u8), y1)
    assert torch.equal(y0, y1) and y0.abs().max() > 0
    assert fast.n_timing_launches > 0 and fast.n_launches == 147 and fast.n_launches_u8 == 145
    names_u8 = [op.args[0] for op in fast._ops_u8]
    assert names_u8.count("hawq_incep_pool_v") == 49 and not set(names_u8) & set(OLD_POOLS)


def test_fast_pools_match_the_oracle_on_unseen_images():
    """5 images the ranges were not calibrated on, against oracle/oracle_inception.py (shares no kernel with the plan); the oracle's
    result is the one tests/test_gpu_inception_oracle.py caches for the same images"""
    from hawq_amd.engine_inception import InceptionEngine
    from tests import test_gpu_inception_oracle as O
    batch, seed = 5, 25
    ref = O._oracle("uniform8", seed, batch)
    model = O._model("uniform8")
    x = O._images(batch, seed).cuda()
    eng = InceptionEngine(model, fast_pools=True)
    with torch.no_grad():
        O._assert_engine_equals(eng, eng(x), ref, "fast pools")
        O._assert_engine_equals(eng, eng(x), ref, "fast pools, replay")
    assert eng.op_names.count("hawq_incep_pool_v") == 49


def test_launch_list_and_plan_format(calibrated):
    from hawq_amd.engine_inception import InceptionEngine
    model = calibrated
    x = _images(2, seed=5).cuda()
    u8 = torch.randint(0, 256, (2, 299, 299, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).cuda()
    base, fast = InceptionEngine(model), InceptionEngine(model, fast_pools=True)
    tuned, tuned_fast = InceptionEngine(model, tune=True), InceptionEngine(model, tune=True, fast_pools=True)
    with torch.no_grad():
        y0 = base(x)
        for e in (fast, tuned, tuned_fast):
            assert torch.equal(e(x), y0)
        base.forward_uint8(u8), fast.forward_uint8(u8)
    for e in (base, fast):
        assert e.n_launches == 147 and e.n_launches_u8 == 145
    names = fast.op_names
    assert names.count("hawq_incep_pool_v") == 49 and not set(names) & set(OLD_POOLS)
    assert names.count("hawq_incep_conv") == 95
    assert "hawq_incep_pool_v" not in base.op_names and sum(base.op_names.count(n) for n in OLD_POOLS) == 49
    # launch for launch the same list: only the pool entry points differ, and each keeps its argument block
    assert [i for i, (a, b) in enumerate(zip(base.op_names, names)) if a != b] == [idx for idx, _, _ in _pools(fast)]
    assert [idx for idx, _, _ in _pools(base)] == [idx for idx, _, _ in _pools(fast)]
    assert len(fast.pool_launches) == 49 and all(n == "hawq_incep_pool_v" for n, _ in fast.pool_launches)
    ops = {"hawq_incep_requant": 0, "hawq_incep_maxpool3s2": 1, "hawq_incep_avgpool_branch": 2, "hawq_incep_global_avgpool": 3}
    assert base.pool_launches == [(n, ops[n]) for n in base.op_names if n in ops]
    assert [op for _, op in fast.pool_launches] == [op for _, op in base.pool_launches]
    assert sorted({op for _, op in fast.pool_launches}) == [0, 1, 2, 3]
    for (_, a, _), (_, b, _) in zip(_pools(base), _pools(fast)):
        fa, fb = ({f: getattr(s, f) for f, _ in s._fields_ if f not in ("in_", "out")} for s in (a, b))
        assert fa == fb
    # the plan format does not know about the pools
    p0, p1 = tuned.export_plan(), tuned_fast.export_plan()
    assert set(p1) == set(p0) == {"network", "batch", "launches", "n_launches", "num_tiles", "tiles", "us"}
    assert p1["launches"] == p0["launches"] and p1["n_launches"] == 95
    plan = json.loads(json.dumps(p1))
    for kw in ({}, {"fast_pools": True}):
        e = InceptionEngine(model, plan=plan, **kw)
        with torch.no_grad():
            assert torch.equal(e(x), y0)
        assert e.conv_tiles == plan["tiles"] and e.n_timing_launches == 0
        assert e.op_names.count("hawq_incep_pool_v") == (49 if kw else 0)
