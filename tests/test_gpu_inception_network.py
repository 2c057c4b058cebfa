"""Whole-network InceptionV3 on the GPU against the live reference's fixtures (tests/golden/make_inception_golden.py)."""
import hashlib

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu


def _images(b=2):
    from hawq_amd.skeleton import synthetic_images
    return synthetic_images(b, seed=0, size=299)


def _load_reference_state(model, fx):
    """The reference run's frozen ranges and integer buffers (weights patched where torch-CPU's sqrt moved them) into `model`."""
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
        m.prepare(torch.ones(1))   # the weights from the float parameters (scales / biases below are the reference's)
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


def _unit_digests(model, x):
    """logits and per-unit output digests of the module-by-module path"""
    got = {}
    hooks = [m.register_forward_hook(lambda mod, i, o, n=n: got.__setitem__(n, o)) for n, m in model.units()]
    with torch.no_grad():
        y = model.forward_modules(x)
    for h in hooks:
        h.remove()
    return y, {n: H.digest(np.rint((o[0].cpu() / o[1].cpu()).numpy().astype(np.float64))) for n, o in got.items()}


@pytest.mark.parametrize("scheme", ["uniform8", "uniform4"])
def test_inceptionv3_matches_reference_golden(scheme):
    """Calibration through the HIP library gives the reference's ranges and logits; on the reference's frozen ranges and integer
    buffers every unit output and the logits are bit-equal, through the module path and through the fused integer plan."""
    from hawq_amd.api import build_quantized_resnet, calibrate
    from hawq_amd.quant_modules import QuantAct, QuantBnConv2d
    fx = H.load(f"net_inceptionv3_{scheme}_b2.npz")
    x = _images()
    assert H.sha(x.numpy()) == str(fx["input_sha"])
    model = build_quantized_resnet("inceptionv3", scheme, seed=0).cuda()
    calibrate(model, x.cuda())
    acts = [m for _, m in model.named_modules() if isinstance(m, QuantAct)]
    convs = [m for _, m in model.named_modules() if isinstance(m, QuantBnConv2d)]
    same_scales = np.array_equal(np.concatenate([m.convbn_scaling_factor.cpu().numpy().reshape(-1) for m in convs]), fx["conv_scale"])
    same_ranges = all(float(m.x_min) == float(fx["act_x_min"][i]) and float(m.x_max) == float(fx["act_x_max"][i])
                      for i, m in enumerate(acts))
    assert same_ranges or not same_scales   # (a weight scale one ulp off - the sqrt quirk - may move later ranges)
    with torch.no_grad():
        y_own = model(x.cuda()).cpu().numpy()   # frozen: the fused plan
    assert model._engine is not None
    assert np.array_equal(y_own.argmax(1), fx["top1"])
    if same_scales:
        assert np.array_equal(y_own, fx["logits"])
    # the rigorous comparison
    _load_reference_state(model, fx)
    model.invalidate_engine()
    y, digests = _unit_digests(model, x.cuda())
    assert [n for n in digests] == [str(n) for n in fx["unit_names"]]
    for i, n in enumerate(fx["unit_names"]):
        assert np.array_equal(digests[str(n)], fx["unit_digest"][i]), n
    assert np.array_equal(y.cpu().numpy(), fx["logits"])
    with torch.no_grad():
        y_plan = model(x.cuda())
    eng = model.engine()
    for i, n in enumerate(fx["unit_names"]):
        assert np.array_equal(H.digest(eng.unit_output(str(n))), fx["unit_digest"][i]), n
    assert np.array_equal(y_plan.cpu().numpy(), fx["logits"])


def test_inceptionv3_graph_replay_equals_eager_plan_and_module_path():
    """The captured graph, the same launches issued one by one, and the module-by-module path give identical logits
    (calibrated on two images, evaluated on three others)."""
    from hawq_amd.api import build_quantized_resnet, calibrate
    from hawq_amd.engine_inception import InceptionEngine
    model = build_quantized_resnet("inceptionv3", "uniform8", seed=1).cuda()
    calibrate(model, _images(2).cuda())
    from hawq_amd.skeleton import synthetic_images
    x = synthetic_images(3, seed=7, size=299).cuda()
    with torch.no_grad():
        y_graph = model(x)
        y_graph2 = model(x)   # replay of the captured graph
        y_eager = InceptionEngine(model, use_graph=False)(x)
        y_mod = model.forward_modules(x)
    assert model.engine()._graph is not None
    assert torch.equal(y_graph, y_graph2) and torch.equal(y_graph, y_eager)
    assert torch.equal(y_graph, y_mod)
    assert y_graph.abs().max() > 0


def test_inceptionv3_batch_independence_and_quantized_checkpoint(tmp_path):
    """One image gives the same logits alone and inside a batch of 3; a quantized checkpoint loaded into an un-initialised
    (seed=None) model gives the same logits again."""
    from hawq_amd.api import build_quantized_resnet, calibrate, load_quantized_checkpoint, save_quantized_checkpoint
    x = _images(3).cuda()
    model = build_quantized_resnet("inceptionv3", "uniform4", seed=0).cuda()
    calibrate(model, x[:2])
    with torch.no_grad():
        y3 = model(x)
        y1 = model(x[2:3])
    assert torch.equal(y1, y3[2:3]) and y3.abs().max() > 0
    path = tmp_path / "quantized_checkpoint.pth.tar"
    save_quantized_checkpoint(model, path)
    other = load_quantized_checkpoint(build_quantized_resnet("inceptionv3", "uniform4", seed=None).cuda(), str(path))
    with torch.no_grad():
        assert torch.equal(other(x), y3)
