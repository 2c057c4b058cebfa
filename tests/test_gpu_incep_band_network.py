"""InceptionV3's fused plan with the stem's 3x3 convs on the band kernel (hawq_amd/engine_inception.py: stem_band=True, the
``"stem_band"`` field of a plan) against the default engine, bit for bit, on the reference's frozen state at batch 2."""
import json

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_gpu_incep_tuned_network import _images, _load_reference_state

pytestmark = pytest.mark.gpu
BAND = "hawq_incep_conv_band"


@pytest.fixture(scope="module")
def frozen():
    """scheme -> (model on the reference's frozen state, its engine class, the default engine's exported plan, inputs and results:
    images, uint8 images, logits, unit outputs, uint8 logits): computed once per scheme, never changed"""
    from hawq_amd.api import build_quantized_resnet, calibrate
    from hawq_amd.engine_inception import InceptionEngine
    cache = {}

    def get(scheme):
        if scheme not in cache:
            x = _images().cuda()
            u8 = torch.randint(0, 256, (2, 299, 299, 3), generator=torch.Generator().manual_seed(6), dtype=torch.uint8).cuda()
            model = build_quantized_resnet("inceptionv3", scheme, seed=0).cuda()
            calibrate(model, x)
            _load_reference_state(model, H.load(f"net_inceptionv3_{scheme}_b2.npz"))
            base = InceptionEngine(model, tune=True)
            with torch.no_grad():
                want = (x, u8, base(x), {n: base.unit_output(n) for n, _ in model.units()}, base.forward_uint8(u8))
            assert BAND not in base.op_names and BAND not in json.dumps(base.export_plan()) and not base.stem_band
            cache[scheme] = (model, InceptionEngine, base.export_plan(), want)
        return cache[scheme]
    return get


def _same(eng, x, u8, y0, units0, y80):
    with torch.no_grad():
        y = eng(x)
        assert torch.equal(eng(x), y) and torch.equal(y, y0)
        for n, want in units0.items():
            assert np.array_equal(eng.unit_output(n), want), n
        assert torch.equal(eng.forward_uint8(u8), y80)


@pytest.mark.parametrize("scheme,options", [
    ("uniform8", {}), ("uniform8", dict(fused_stem=True, fast_pools=True, grouped=True, fan_out=True)),
    ("uniform4", dict(nibble=True, nibble_groups=True))], ids=["alone", "stem_pools_groups_fan", "nibble_groups"])
def test_stem_band_engine_equals_the_default_engine(frozen, scheme, options):
    model, Engine, _, want = frozen(scheme)
    eng = Engine(model, stem_band=True, **options)
    _same(eng, *want)
    assert eng.op_names.count(BAND) == 3 and eng.stem_band_convs == [1, 2, 4] and eng.n_timing_launches == 0
    assert len(eng.conv_launches) == 95


def test_tuned_choice_is_consistent_with_its_times_and_replays(frozen):
    model, Engine, plain_plan, want = frozen("uniform8")
    eng = Engine(model, stem_band=True, tune=True, fast_pools=True)
    _same(eng, *want)
    kept = [c for c in (1, 2, 4) if eng.stem_band_us[c] < eng.conv_us[c][eng.conv_tiles[c]]]   # a tie goes to the tile
    assert sorted(eng.stem_band_us) == [1, 2, 4] and eng.stem_band_convs == kept and eng.op_names.count(BAND) == len(kept)
    plan = json.loads(json.dumps(eng.export_plan()))
    again = Engine(model, stem_band=True, plan=plan, fast_pools=True)
    _same(again, *want)
    assert plan["stem_band"] == kept and again.op_names == eng.op_names and again.n_timing_launches == 0
    # a plan without the field replays with no band launch, an engine without the option ignores the field, and every candidate
    # forced is what a replayed plan issues whatever the tuner kept
    forced = {**plain_plan, "stem_band": [1, 2, 4]}
    for e, n in ((Engine(model, stem_band=True, plan=plain_plan), 0), (Engine(model, plan=forced), 0), (Engine(model, stem_band=True, plan=forced), 3)):
        _same(e, *want)
        assert e.op_names.count(BAND) == n
