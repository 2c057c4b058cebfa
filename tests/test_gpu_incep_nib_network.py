"""InceptionV3 uniform4 on nibble-packed operands (hawq_amd/engine_inception.py: nibble=True) against the default plan, bit for bit."""
import json

import pytest
import torch

from tests.test_gpu_incep_group_network import _u8
from tests.test_gpu_incep_tuned_network import _images

pytestmark = pytest.mark.gpu
NIB, POOL_V = "hawq_incep_conv_nib", "hawq_incep_pool_v"


@pytest.fixture(scope="module")
def model4():
    from hawq_amd.api import build_quantized_resnet, calibrate
    model = build_quantized_resnet("inceptionv3", "uniform4", seed=1).cuda()
    calibrate(model, _images(2).cuda())
    return model


@pytest.fixture(scope="module")
def default4(model4):
    """input, logits, uint8 input and logits, launch count of the default engine: computed once, never changed"""
    from hawq_amd.engine_inception import InceptionEngine
    base = InceptionEngine(model4)
    x, u8 = _images(2, seed=13).cuda(), _u8(2)
    with torch.no_grad():
        y, y8 = base(x), base.forward_uint8(u8)
    assert y.abs().max() > 0 and NIB not in base.op_names
    return x, y, u8, y8, base.n_launches


def _check_stored(eng, n_default):
    """same launch list; some tensors and weights really are hawq4, and exactly the convs that read them run on the nibble kernel"""
    names = eng.op_names
    assert eng.n_launches == n_default and names.count(NIB) == len(eng.nibble_convs) > 0 and eng.nibble_tensors
    assert sorted(c for t in eng.nibble_tensors for c in eng._tensors[t].cons) == sorted(eng.nibble_convs)
    for t in eng.nibble_tensors:
        tt = eng._tensors[t]
        assert tt.buf.dtype == torch.uint8 and tt.buf.numel() * 2 == eng.N * tt.h * tt.w * tt.pitch
    for c in eng.nibble_convs:   # the weight bytes of a nibble launch are half its int8 twin's
        a = eng._nib_conv[c]
        assert any(k.data_ptr() == a.wgt and k.numel() * 2 == a.Cout * a.KH * a.KW * a.Cin for k in eng._keep if torch.is_tensor(k))
    (w0, w1), (a0, a1) = eng.nibble_bytes["weights"], eng.nibble_bytes["activations"]
    assert w1 < w0 and a1 < a0


@pytest.mark.parametrize("kw", [{}, {"fast_pools": True, "fused_stem": True}], ids=["alone", "fast_pools+fused_stem"])
def test_nibble_engine_equals_the_default_engine(model4, default4, kw):
    x, y0, u8, y8, n = default4
    eng = model4.engine(nibble=True, **kw)
    with torch.no_grad():
        y = eng(x)
        assert torch.equal(eng(x), y) and torch.equal(y, y0)
        assert torch.equal(eng.forward_uint8(u8), y8)
    assert eng.n_timing_launches == 0 and eng._graph is not None
    _check_stored(eng, n - 2 * bool(kw.get("fused_stem")))
    # every branch-entry requant of a hawq4 tensor writes it through the vectorised family, the only one with that form
    assert kw or eng.op_names.count(POOL_V) == sum(eng._tensors[t].producer == "requant" for t in eng.nibble_tensors) > 0
    model4.invalidate_engine()


def test_tuning_keeps_nibbles_only_where_they_win_and_the_plan_replays(model4, default4):
    from hawq_amd.engine_inception import InceptionEngine
    x, y0, _, _, n = default4
    tuned = InceptionEngine(model4, nibble=True, tune=True)
    with torch.no_grad():
        assert torch.equal(tuned(x), y0)
    assert tuned.n_timing_launches > 0 and tuned.nibble_us and tuned.n_launches == n
    for c, tile in tuned.nibble_convs.items():
        us = tuned.nibble_us[c]
        print("conv", c, tuned.conv_launches[c], "int8 us", tuned.conv_us[c], "nibble us", us)
        assert tile == min(us, key=lambda t: (us[t], t)) and us[tile] < tuned.conv_us[c][tuned.conv_tiles[c]]
    plan = json.loads(json.dumps(tuned.export_plan()))
    assert plan["nibble"] == [[c, t] for c, t in sorted(tuned.nibble_convs.items())]
    replay = InceptionEngine(model4, nibble=True, plan=plan)
    with torch.no_grad():
        assert torch.equal(replay(x), y0)
    assert replay.n_timing_launches == 0 and replay.op_names == tuned.op_names and replay.export_plan() == plan
    plain = InceptionEngine(model4, plan=plan)   # an engine without the option ignores the field
    with torch.no_grad():
        assert torch.equal(plain(x), y0)
    assert NIB not in plain.op_names and "nibble" not in plain.export_plan()


def test_nibble_on_a_uniform8_model_is_not_applicable():
    from hawq_amd.api import build_quantized_resnet, calibrate
    from hawq_amd.engine_inception import InceptionEngine, PlanNotApplicable
    model = build_quantized_resnet("inceptionv3", "uniform8", seed=1).cuda()
    x = _images(2).cuda()
    calibrate(model, x)
    with pytest.raises(PlanNotApplicable, match="nibble"), torch.no_grad():
        InceptionEngine(model, nibble=True)(x)
