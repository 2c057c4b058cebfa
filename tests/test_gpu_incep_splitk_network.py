"""InceptionV3's fused plan with split-K launches (hawq_amd/engine_inception.py: grouped=True, splitk=..., the ``"splitk"`` field of a
plan) against the default plan and the live reference's fixtures, bit for bit, with the slice count forced."""
import functools
import json

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_gpu_inception_uint8 import _normalise
from tests.test_gpu_incep_group_network import _u8
from tests.test_gpu_incep_tuned_network import _images, _load_reference_state, _num_tiles

pytestmark = pytest.mark.gpu

SPLIT = "hawq_incep_conv_group_splitk"


@functools.lru_cache(maxsize=None)
def _model(scheme):
    """the reference's frozen state of a scheme, and its fixture; loaded once"""
    from hawq_amd.api import build_quantized_resnet, calibrate
    fx = H.load(f"net_inceptionv3_{scheme}_b2.npz")
    model = build_quantized_resnet("inceptionv3", scheme, seed=0).cuda()
    calibrate(model, _images().cuda())
    _load_reference_state(model, fx)
    return model, fx


@pytest.mark.parametrize("scheme,batch", [("uniform8", 1), ("uniform8", 2), ("uniform8", 3), ("uniform4", 1), ("uniform4", 2)])
def test_split_engine_equals_the_default_engine_and_the_reference(scheme, batch):
    from hawq_amd.engine_inception import InceptionEngine
    model, fx = _model(scheme)
    x = (_images() if batch == 2 else _images(batch, seed=11 + batch)).cuda()   # batch 2: the fixture's images
    base, eng = InceptionEngine(model), InceptionEngine(model, grouped=True, splitk=4)
    with torch.no_grad():
        y0, y = base(x), eng(x)
        assert torch.equal(eng(x), y) and torch.equal(eng(x), y) and eng._graph is not None   # two replays of the captured graph
    assert torch.equal(y, y0) and y0.abs().max() > 0
    for n, _ in model.units():
        assert np.array_equal(eng.unit_output(n), base.unit_output(n)), n
    if batch == 2:
        assert np.array_equal(y.cpu().numpy(), fx["logits"])
        for i, n in enumerate(fx["unit_names"]):
            assert np.array_equal(H.digest(eng.unit_output(str(n))), fx["unit_digest"][i]), n
    # a split launch takes the place of the launch it replaces, in every unit (so in every unit kind), and never cuts below 2 steps
    assert eng.n_launches == 100 and eng.op_names.count(SPLIT) == len(eng.splitk_launches) > 0
    assert {eng._convs[c].place for convs, _ in eng.splitk_launches for c in convs} >= set(range(11))
    assert all(len(s) == len(c) and 1 <= min(s) and 1 < max(s) <= 4 for c, s in eng.splitk_launches)
    u8 = _u8(batch)
    with torch.no_grad():
        assert torch.equal(eng.forward_uint8(u8), eng(_normalise(u8.cpu()).cuda()))
    assert [op.args[0] for op in eng._ops_u8].count(SPLIT) == len(eng.splitk_launches)


def test_plans_carry_the_split_launches():
    from hawq_amd.engine import StalePlan
    from hawq_amd.engine_inception import InceptionEngine, make_plan
    model, _ = _model("uniform8")
    x = _images(1, seed=12).cuda()
    forced = InceptionEngine(model, grouped=True, splitk=4)
    with torch.no_grad():
        y0 = forced(x)
    keys, groups = forced.conv_launches, [{"convs": c, "tile": t} for c, t in forced.group_launches]
    unsplit = make_plan(forced._batch, keys, _num_tiles(), [0] * len(keys), [{} for _ in keys], groups)   # tile 0 on every single conv
    plan = json.loads(json.dumps(dict(unsplit, splitk=[{"convs": c, "slices": s} for c, s in forced.splitk_launches])))
    replay = InceptionEngine(model, grouped=True, splitk=True, plan=plan)
    with torch.no_grad():
        assert torch.equal(replay(x), y0)
    assert replay.splitk_launches == forced.splitk_launches and replay.n_timing_launches == 0
    again = json.loads(json.dumps(replay.export_plan()))
    assert [(e["convs"], e["slices"]) for e in again["splitk"]] == forced.splitk_launches
    # without the option the field is ignored; without the field nothing is split
    plain, none = InceptionEngine(model, grouped=True, plan=plan), InceptionEngine(model, grouped=True, splitk=True, plan=unsplit)
    with torch.no_grad():
        assert torch.equal(plain(x), y0) and torch.equal(none(x), y0)
    assert plain.splitk_launches == none.splitk_launches == [] and SPLIT not in plain.op_names + none.op_names
    assert "splitk" not in none.export_plan() and "splitk" not in unsplit
    convs, slices = forced.splitk_launches[0]
    for entry in ({"convs": convs, "slices": [33] * len(convs)}, {"convs": convs, "slices": [1] * len(convs)}, {"convs": convs[:1] + [0], "slices": [2, 2]},
                  {"convs": convs}):
        with pytest.raises(StalePlan), torch.no_grad():
            InceptionEngine(model, grouped=True, splitk=True, plan=dict(plan, splitk=[entry]))(x)


def test_the_option_needs_a_grouped_int8_plan():
    from hawq_amd.engine_inception import InceptionEngine, PlanNotApplicable
    model, _ = _model("uniform4")
    for kw in (dict(splitk=True), dict(splitk=4, grouped=True, nibble=True), dict(splitk=True, grouped=True, fan_out=True)):
        with pytest.raises(PlanNotApplicable):
            InceptionEngine(model, **kw)
    assert InceptionEngine(model, grouped=True).splitk is False
