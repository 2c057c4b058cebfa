"""InceptionV3's fused plan with the average-pool branches in one launch each (hawq_amd/engine_inception.py: pool_conv=True, the
``"pool_conv"`` field of a plan) against the default engine and the reference's fixture, bit for bit, at batch 2."""
import json

import numpy as np
import pytest

from hawq_amd.plan import StalePlan
from tests import helpers as H
from tests.test_gpu_incep_band_network import _same, frozen   # noqa: F401  (the fixture: model, engine class, plain plan, results)

pytestmark = pytest.mark.gpu
FUSED = "hawq_incep_avgpool_conv"
OPTIONS = {"alone": {}, "groups_fan_pools": dict(grouped=True, fan_out=True, fast_pools=True), "stem_pool": dict(stem_pool=True)}


@pytest.mark.parametrize("scheme", ["uniform8", "uniform4"])
@pytest.mark.parametrize("options", OPTIONS.values(), ids=list(OPTIONS))
def test_pool_conv_engine_equals_the_default_engine_and_the_fixture(frozen, scheme, options):   # noqa: F811
    model, Engine, plain_plan, want = frozen(scheme)
    assert np.array_equal(want[2].cpu().numpy(), H.load(f"net_inceptionv3_{scheme}_b2.npz")["logits"])
    assert FUSED not in json.dumps(plain_plan) and "pool_conv" not in plain_plan and Engine(model).pool_conv is False
    model.invalidate_engine()
    eng, twin = model.engine(pool_conv=True, **options), Engine(model, **options)   # the public way in forwards the keywords
    _same(eng, *want)   # logits, every unit_out and forward_uint8
    twin(want[0])
    assert eng.op_names.count(FUSED) == 9 and len(eng.pool_conv_convs) == 9 and FUSED not in twin.op_names
    assert eng.n_timing_launches == 0 and len(eng.conv_launches) == 95
    # nine pool launches fewer; under grouped the conv was a member of its level's launch and now has a launch of its own; under
    # fan_out a fused slice comes back as residual entry requants of the next unit, one launch each
    own, back = (9 if "grouped" in options else 0), len(eng.residual_requants) - len(twin.residual_requants)
    assert eng.n_launches == twin.n_launches - 9 + own + back and (back > 0) == ("fan_out" in options)
    assert twin.n_launches == {"alone": 147, "groups_fan_pools": 81, "stem_pool": 145}[[k for k, v in OPTIONS.items() if v is options][0]]
    model.invalidate_engine()


def test_tuned_choice_is_consistent_with_its_times_and_replays(frozen):   # noqa: F811
    model, Engine, plain_plan, want = frozen("uniform8")
    eng = Engine(model, pool_conv=True, tune=True, fast_pools=True, grouped=True)
    _same(eng, *want)
    kept = sorted(c for c, us in eng.pool_conv_us.items() if us[1] < us[0])   # a tie goes to the two launches
    assert len(eng.pool_conv_us) == 9 and eng.pool_conv_convs == kept and eng.op_names.count(FUSED) == len(kept)
    plan = json.loads(json.dumps(eng.export_plan()))
    again = Engine(model, pool_conv=True, plan=plan, fast_pools=True, grouped=True)
    _same(again, *want)
    assert plan["pool_conv"] == kept and again.op_names == eng.op_names and again.n_timing_launches == 0
    # a plan without the field fuses nothing, an engine without the option ignores the field, all nine forced replay fused
    forced = {**plain_plan, "pool_conv": sorted(eng.pool_conv_us)}
    for e, n in ((Engine(model, pool_conv=True, plan=plain_plan), 0), (Engine(model, plan=forced), 0), (Engine(model, pool_conv=True, plan=forced), 9)):
        _same(e, *want)
        assert e.op_names.count(FUSED) == n and e.n_timing_launches == 0
    # a grouped plan with all nine forced: its "groups" name whole levels (here every level, on the untuned tile), each is issued on
    # its tile without its fused conv, which gets the launch the pool had
    nine, levels = sorted(eng.pool_conv_us), [{"convs": lv, "tile": 3} for lv in eng.conv_level_list if len(lv) >= 2]
    g9, g0 = (Engine(model, plan={**plan, "groups": levels, "pool_conv": nine}, fast_pools=True, grouped=True, pool_conv=on) for on in (True, False))
    _same(g9, *want)
    g0(want[0])
    assert g9.op_names.count(FUSED) == 9 and g9.n_launches == g0.n_launches and len(g0.group_launches) == len(levels)
    assert g9.group_launches == [([c for c in cv if c not in nine], t) for cv, t in g0.group_launches]
    with pytest.raises(StalePlan):   # conv 0 is the stem's conv1
        Engine(model, pool_conv=True, plan={**plain_plan, "pool_conv": [0]})(want[0])


@pytest.mark.parametrize("options", [dict(nibble=True), dict(grouped=True, splitk=True)], ids=str)
def test_refused_combinations(options):
    from hawq_amd.engine_inception import InceptionEngine, PlanNotApplicable
    with pytest.raises(PlanNotApplicable):
        InceptionEngine(None, pool_conv=True, **options)
