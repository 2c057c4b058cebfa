"""InceptionV3 uniform4 on nibble-packed operands with mixed-form grouped launches (hawq_amd/engine_inception.py: nibble=True,
nibble_groups=True) against the default plan, bit for bit."""
import json

import pytest
import torch

from tests.test_gpu_incep_nib_network import default4, model4  # noqa: F401  (the fixtures: model, seed and batch sizes)

pytestmark = pytest.mark.gpu
GROUP_NIB = "hawq_incep_conv_group_nib"


def _forms(eng):
    """per grouped launch (members, hawq4 members by the mask, hawq4 members by the engine's nibble choice)"""
    return [(len(c), bin(m).count("1"), sum(i in eng.nibble_convs for i in c)) for (c, _), m in zip(eng.group_launches, eng.nibble_group_masks)]


@pytest.mark.parametrize("kw", [{}, {"fast_pools": True, "fused_stem": True}], ids=["alone", "fast_pools+fused_stem"])
def test_nibble_groups_equal_the_default_engine(model4, default4, kw):   # noqa: F811
    from hawq_amd.engine_inception import InceptionEngine
    x, y0, u8, y8, _ = default4
    eng = model4.engine(nibble=True, nibble_groups=True, **kw)
    with torch.no_grad():
        y = eng(x)
        assert torch.equal(eng(x), y) and torch.equal(y, y0)
        assert torch.equal(eng.forward_uint8(u8), y8)
    assert eng.n_timing_launches == 0 and eng._graph is not None
    int8 = InceptionEngine(model4, grouped=True, **kw)
    with torch.no_grad():
        int8(x)
    assert eng.n_launches == int8.n_launches and eng.op_names.count(GROUP_NIB) == len(eng.group_launches) == len(int8.group_launches)
    forms = _forms(eng)
    assert all(by_mask == chosen for _, by_mask, chosen in forms)
    assert any(n == k for n, k, _ in forms) and any(0 < k < n for n, k, _ in forms)   # an all-hawq4 launch, and a mixed one
    model4.invalidate_engine()


def test_tuned_nibble_groups_and_their_plan(model4, default4):   # noqa: F811
    from hawq_amd.engine import StalePlan
    from hawq_amd.engine_inception import InceptionEngine
    x, y0, _, _, _ = default4
    tuned = InceptionEngine(model4, nibble=True, nibble_groups=True, tune=True)
    with torch.no_grad():
        assert torch.equal(tuned(x), y0)
    for g in tuned.group_candidates:
        us = {k: v for k, v in g["us"].items() if k != "singles"}
        print(g["convs"], "tile", g["tile"], "group us", us, "singles us", round(g["us"]["singles"], 2), "kept", g["kept"])
        assert g["us"][str(g["tile"])] == min(us.values()) and g["kept"] == (min(us.values()) < g["us"]["singles"])
    assert tuned.group_launches == [(g["convs"], g["tile"]) for g in tuned.group_candidates if g["kept"]]
    plan = json.loads(json.dumps(tuned.export_plan()))
    assert [(g["convs"], g["tile"]) for g in plan["nibble_groups"]] == tuned.group_launches
    replay = InceptionEngine(model4, nibble=True, nibble_groups=True, plan=plan)
    with torch.no_grad():
        assert torch.equal(replay(x), y0)
    assert replay.n_timing_launches == 0 and replay.group_launches == tuned.group_launches and replay.op_names == tuned.op_names
    assert replay.nibble_group_masks == tuned.nibble_group_masks and replay.export_plan() == plan
    plain = InceptionEngine(model4, nibble=True, plan=plan)   # an engine without the option ignores the field
    with torch.no_grad():
        assert torch.equal(plain(x), y0)
    assert GROUP_NIB not in plain.op_names and "nibble_groups" not in plain.export_plan()
    lv = next(lv for lv in tuned.conv_level_list if len(lv) >= 2)
    for groups in ([{"convs": lv[:-1], "tile": 2}], [{"convs": lv, "tile": 3}], [{"convs": lv, "tile": 2}, {"convs": lv, "tile": 2}]):
        with pytest.raises(StalePlan), torch.no_grad():   # not a level; a refused tile; an overlap
            InceptionEngine(model4, nibble=True, nibble_groups=True, plan=dict(plan, nibble_groups=groups))(x)
