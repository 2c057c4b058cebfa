"""InceptionV3 uniform4 on a nibble plan with mixed-form groups and split-K launches (hawq_amd/engine_inception.py: nibble=True,
nibble_groups=True, splitk=..., the ``"splitk"`` field of such a plan) against the default plan, bit for bit, at batch 1 with the
slice count forced."""
import json

import pytest
import torch

from tests.test_gpu_inception_uint8 import _normalise
from tests.test_gpu_incep_group_network import _u8
from tests.test_gpu_incep_splitk_network import _model
from tests.test_gpu_incep_tuned_network import _images, _num_tiles

pytestmark = pytest.mark.gpu

SPLIT = "hawq_incep_conv_group_nib_splitk"
NIB = dict(nibble=True, nibble_groups=True)


def test_split_nibble_engine_equals_the_default_engine_and_its_plan_replays():
    from hawq_amd.engine import StalePlan
    from hawq_amd.engine_inception import InceptionEngine, make_plan
    model, _ = _model("uniform4")
    x, u8 = _images(1, seed=12).cuda(), _u8(1)
    base, groups, eng = InceptionEngine(model), InceptionEngine(model, **NIB), InceptionEngine(model, splitk=4, **NIB)
    with torch.no_grad():
        y0, y = base(x), eng(x)
        assert torch.equal(eng(x), y) and torch.equal(eng(x), y) and eng._graph is not None   # two replays of the captured graph
        assert torch.equal(y, y0) and y0.abs().max() > 0 and torch.equal(groups(x), y0)
        assert torch.equal(eng.forward_uint8(u8), base.forward_uint8(u8)) and torch.equal(eng.forward_uint8(u8), eng(_normalise(u8.cpu()).cuda()))
    # a split launch takes the place of the launch it replaces: hawq4 and int8 members, never below 2 steps a slice
    assert eng.op_names.count(SPLIT) == len(eng.splitk_launches) > 0 and [op.args[0] for op in eng._ops_u8].count(SPLIT) == len(eng.splitk_launches)
    assert eng.n_launches == groups.n_launches and eng.group_launches == groups.group_launches
    assert eng.nibble_group_masks == groups.nibble_group_masks and any(eng.nibble_group_masks)
    assert all(len(s) == len(c) and 1 <= min(s) and 1 < max(s) <= 4 for c, s in eng.splitk_launches)
    split = {c for convs, _ in eng.splitk_launches for c in convs}
    assert split & set(eng.nibble_convs) and split - set(eng.nibble_convs)
    # the same launches from a plan: tile 0 on every single int8 conv, the nibble choice and the groups as they are
    keys = eng.conv_launches
    plan = make_plan(eng._batch, keys, _num_tiles(), [0] * len(keys), [{} for _ in keys], nibble=(eng.nibble_convs, {}),
                     nibble_groups=[{"convs": c, "tile": t} for c, t in eng.group_launches],
                     splitk=[{"convs": c, "slices": s} for c, s in eng.splitk_launches])
    plan = json.loads(json.dumps(plan))
    replay = InceptionEngine(model, splitk=True, plan=plan, **NIB)
    with torch.no_grad():
        assert torch.equal(replay(x), y0)
    assert replay.splitk_launches == eng.splitk_launches and replay.n_timing_launches == 0
    assert [(e["convs"], e["slices"]) for e in replay.export_plan()["splitk"]] == eng.splitk_launches
    convs, _ = next((c, s) for c, s in eng.splitk_launches if len(c) > 1)
    with pytest.raises(StalePlan), torch.no_grad():   # part of a level is no issued launch
        InceptionEngine(model, splitk=True, plan=dict(plan, splitk=[{"convs": convs[:-1], "slices": [2] * (len(convs) - 1)}]), **NIB)(x)


def test_the_option_takes_a_nibble_plan_on_mixed_form_groups_only():
    from hawq_amd.engine_inception import InceptionEngine, PlanNotApplicable
    model, _ = _model("uniform4")
    assert InceptionEngine(model, splitk=True, **NIB).splitk is True
    for kw in (dict(nibble=True, nibble_groups=True, nibble_fan=True, splitk=True), dict(nibble=True, splitk=True)):
        with pytest.raises(PlanNotApplicable):
            InceptionEngine(model, **kw)
