"""Stage handover on the stride-2 grid (hawq_conv_args.out_sub, hawq_amd/engine.py): the last expand launch of stages 1-3 of
resnet50 writes only the block-input pixels the next stage's stride-2 conv1 / identity conv read.  The logits must not move by a
bit - against the same model built with HAWQ_NO_OUT_SUB=1 (the launch list before the change) and against the live reference's
fixture tests/test_gpu_network.py compares this workload with."""
import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu


def _images(extra):
    """The fixture's two calibration images followed by `extra` unseen ones."""
    from hawq_amd.skeleton import synthetic_images
    return torch.cat([synthetic_images(2, 0), synthetic_images(extra, seed=3) * 1.3 + 0.1])


def _model(arch, scheme):
    from hawq_amd.api import calibrate
    from hawq_amd.skeleton import synthetic_images
    model = H.build_model(arch, scheme)
    calibrate(model, synthetic_images(2, 0).cuda())
    return model


def _engine(monkeypatch, model, sub, **kw):
    from hawq_amd.engine import IntegerEngine
    if sub:
        monkeypatch.delenv("HAWQ_NO_OUT_SUB", raising=False)
    else:
        monkeypatch.setenv("HAWQ_NO_OUT_SUB", "1")
    return IntegerEngine(model, **kw)


def _sub_launches(eng):
    """out_sub of every launch of the plan as built (all chains)."""
    out = []
    for e in (eng.subs or [eng]):
        out += [a.out_sub for a in e._conv_args] + [p.expand.out_sub for p in e._er_args]
        assert all(p.er.expand.out_sub == p.expand.out_sub for p in e._er_args)
    return out


@pytest.mark.parametrize("scheme", ["uniform8", "bops_0.5"])   # bops_0.5: hawq4 block inputs at the stage handovers
def test_resnet50_logits_do_not_move(scheme, monkeypatch):
    model = _model("resnet50", scheme)
    fx = H.net_fixture("resnet50", scheme)
    x = _images(1).cuda()   # batch 3
    off = _engine(monkeypatch, model, False)
    ref = off(x).clone()
    assert np.array_equal(ref[:2].cpu().numpy(), fx["logits"])
    assert sum(s >= 2 for s in _sub_launches(off)) == 0
    on = _engine(monkeypatch, model, True)
    y = on(x).clone()
    assert torch.equal(y, ref)
    assert torch.equal(on(x), ref)   # graph replay
    assert np.array_equal(y[:2].cpu().numpy(), fx["logits"])
    assert [s for s in _sub_launches(on) if s] == [2, 2, 2] and not on.overflowed()
    # the plan is the same list of launches; only what the tuner timed may differ
    p_on, p_off = on.export_plan(), off.export_plan()
    for k in ("batch", "chains", "expand_in8", "conv_launches", "pair_launches", "num_conv_tiles", "pair_variant_counts"):
        assert p_on[k] == p_off[k], k
    assert len(p_on["tiles"].split(".")) == len(p_off["tiles"].split("."))
    # uint8 images through the fused stem
    g = torch.Generator().manual_seed(3)
    xu8 = torch.randint(0, 256, (3, 224, 224, 3), dtype=torch.uint8, generator=g).cuda()
    assert torch.equal(on.forward_uint8(xu8), off.forward_uint8(xu8))
    # another batch shape (two concurrent chains: 3 + 2 images) and back
    x5 = _images(3).cuda()
    ref5 = off(x5).clone()
    assert torch.equal(ref5[:3], ref)
    assert torch.equal(on(x5), ref5)
    assert torch.equal(on(x), ref) and torch.equal(on(x), ref)
    # chains = 2 inside one graph, and the int32-residual twin (hawq_conv2d's general path takes out_sub there)
    two = _engine(monkeypatch, model, True, chains=2)
    assert torch.equal(two(x5), ref5) and torch.equal(two(x5), ref5)
    assert len(two.subs) == 2 and [s for s in _sub_launches(two) if s] == [2] * 6
    wide = _engine(monkeypatch, model, True, residual_bits=32, use_graph=False)
    assert torch.equal(wide(x), ref) and [s for s in _sub_launches(wide) if s] == [2, 2, 2]


def test_resnet50b_has_no_subsampled_launch(monkeypatch):
    """The stride sits on the 3x3 conv2 there: conv1 reads every pixel of the block input."""
    model = _model("resnet50b", "uniform8")
    x = _images(1).cuda()
    ref = _engine(monkeypatch, model, False)(x).clone()
    on = _engine(monkeypatch, model, True)
    assert torch.equal(on(x), ref)
    assert not any(_sub_launches(on))
