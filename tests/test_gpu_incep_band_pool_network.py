"""InceptionV3's fused plan with the stem's conv + max pool pairs in one launch each (hawq_amd/engine_inception.py: stem_pool=True,
the ``"stem_pool"`` field of a plan) against the default engine, bit for bit, on the reference's frozen state at batch 2."""
import json

import pytest

from hawq_amd.plan import StalePlan
from tests.test_gpu_incep_band_network import _same, frozen   # noqa: F401  (the fixture: model, engine class, plain plan, results)

pytestmark = pytest.mark.gpu
FUSED = "hawq_incep_conv_band_pool"
OPTIONS = {"alone": {}, "pools_stem": dict(fast_pools=True, fused_stem=True), "groups_fan": dict(grouped=True, fan_out=True),
           "stem_band": dict(stem_band=True)}


@pytest.mark.parametrize("scheme", ["uniform8", "uniform4"])
@pytest.mark.parametrize("options", OPTIONS.values(), ids=list(OPTIONS))
def test_stem_pool_engine_equals_the_default_engine(frozen, scheme, options):   # noqa: F811
    model, Engine, plain_plan, want = frozen(scheme)
    assert FUSED not in json.dumps(plain_plan) and "stem_pool" not in plain_plan   # the default engine's (asserted on its op_names there)
    eng, twin = Engine(model, stem_pool=True, **options), Engine(model, **options)
    _same(eng, *want)   # logits, every unit_out and forward_uint8
    twin(want[0])
    assert eng.op_names.count(FUSED) == 2 and eng.stem_pool_convs == [2, 4] and eng.n_launches == twin.n_launches - 2
    assert FUSED not in twin.op_names and eng.n_timing_launches == 0 and len(eng.conv_launches) == 95
    assert eng.stem_band_convs == ([1] if "stem_band" in options else [])   # the pooled launch wins conv3 and conv5


def test_tuned_choice_is_consistent_with_its_times_and_replays(frozen):   # noqa: F811
    model, Engine, plain_plan, want = frozen("uniform8")
    eng = Engine(model, stem_pool=True, tune=True, fast_pools=True)
    _same(eng, *want)
    kept = [c for c in (2, 4) if eng.stem_pool_us[c][1] < eng.stem_pool_us[c][0]]   # a tie goes to the pair
    assert sorted(eng.stem_pool_us) == [2, 4] and eng.stem_pool_convs == kept and eng.op_names.count(FUSED) == len(kept)
    plan = json.loads(json.dumps(eng.export_plan()))
    again = Engine(model, stem_pool=True, plan=plan, fast_pools=True)
    _same(again, *want)
    assert plan["stem_pool"] == kept and again.op_names == eng.op_names and again.n_timing_launches == 0
    # a plan without the field fuses nothing, an engine without the option ignores the field, both pairs forced replay fused
    forced = {**plain_plan, "stem_pool": [2, 4]}
    for e, n in ((Engine(model, stem_pool=True, plan=plain_plan), 0), (Engine(model, plan=forced), 0), (Engine(model, stem_pool=True, plan=forced), 2)):
        _same(e, *want)
        assert e.op_names.count(FUSED) == n and e.n_timing_launches == 0
    with pytest.raises(StalePlan):   # conv2's output is read by conv3
        Engine(model, stem_pool=True, plan={**plain_plan, "stem_pool": [1]})(want[0])
