"""The stage-final 3x3 convs on the next stage's grid (hawq_amd/engine.py: out_sub on quant_convbn2 of stage1.unit3 / stage2.unit4 /
stage3.unit6, res_sub on the expand conv behind it) against the same model built with HAWQ_NO_CONV2_SUB=1, the launch list before
the change: logits and every stored residual must not move by a bit, no uint16 residual may overflow, the plan must round-trip."""
import json

import pytest
import torch

from hawq_amd import _lib
from tests import helpers as H

pytestmark = pytest.mark.gpu


def _engine(monkeypatch, model, on, **kw):
    from hawq_amd.engine import IntegerEngine
    if on:
        monkeypatch.delenv("HAWQ_NO_CONV2_SUB", raising=False)
    else:
        monkeypatch.setenv("HAWQ_NO_CONV2_SUB", "1")
    return IntegerEngine(model, **kw)


def _fields(eng):
    """(launch name, out_sub, res_sub) of every launch that carries one of the fields, all chains."""
    out = []
    for e in (eng.subs or [eng]):
        named = list(zip(e._conv_names, e._conv_args)) + [(n, p.expand) for n, p in zip(e._er_names, e._er_args)]
        out += [(n.split("@")[0], a.out_sub, _lib.res_sub(a)) for n, a in named if a.out_sub >= 2 or _lib.res_sub(a) >= 2]
        assert all(_lib.res_sub(p.er.expand) == _lib.res_sub(p.expand) and p.er.expand.out_sub == p.expand.out_sub for p in e._er_args)
    return sorted(out)


def _taps(eng):
    return [(name, t.clone()) for e in (eng.subs or [eng]) for name, (t, _) in sorted(e.res_taps.items())]


@pytest.mark.parametrize("scheme", ["uniform8", "uniform4"])
def test_resnet50_batch4_does_not_move(scheme, monkeypatch):
    from hawq_amd.api import calibrate
    from hawq_amd.skeleton import synthetic_images
    model = H.build_model("resnet50", scheme)
    calibrate(model, synthetic_images(2, 0).cuda())
    x = torch.cat([synthetic_images(2, 0), synthetic_images(2, seed=3) * 1.3 + 0.1]).cuda()   # batch 4
    off = _engine(monkeypatch, model, False)
    ref = off(x).clone()
    ref_taps = _taps(off)
    # as before: out_sub on the three expand convs, nothing on the 3x3 convs
    assert _fields(off) == sorted((f"stage{s}.unit{u}.quant_convbn3", 2, 0) for s, u in ((1, 3), (2, 4), (3, 6))) and not off.overflowed()
    on = _engine(monkeypatch, model, True)
    y = on(x).clone()
    assert torch.equal(y, ref)
    assert torch.equal(on(x), ref)   # graph replay
    assert not on.overflowed()
    want = sorted([(f"stage{s}.unit{u}.quant_convbn2", 2, 0) for s, u in ((1, 3), (2, 4), (3, 6))] +
                  [(f"stage{s}.unit{u}.quant_convbn3", 0, 2) for s, u in ((1, 3), (2, 4), (3, 6))])
    assert _fields(on) == want
    taps = _taps(on)
    assert [n for n, _ in taps] == [n for n, _ in ref_taps] and len(taps) >= 10
    for (name, t), (_, r) in zip(taps, ref_taps):
        assert torch.equal(t, r), name
    # the same list of launches and launch names; the plan survives a JSON round trip and replays to the same bits
    p_on, p_off = on.export_plan(), off.export_plan()
    for k in ("batch", "chains", "expand_in8", "conv_launches", "pair_launches", "num_conv_tiles", "pair_variant_counts"):
        assert p_on[k] == p_off[k], k
    assert list(on._ops.names) == list(off._ops.names) and len(on._ops) == len(off._ops)
    again = _engine(monkeypatch, model, True, plan=dict(json.loads(json.dumps(p_on)), source="round trip"))
    assert torch.equal(again(x), ref) and again.plan_source == "round trip"
    assert again.export_plan() == p_on
    # a plan that names a kernel which refuses the strided form (22: the weight-stationary kernel, what the stage-1 launch ran before)
    # is stale: the replay does not put another id in its place, the engine tunes afresh
    from hawq_amd.engine import StalePlan
    k = p_on["conv_launches"].index("stage1.unit3.quant_convbn2")
    tiles = p_on["tiles"].split(".")
    tiles[k] = "22"
    with pytest.raises(StalePlan, match="refuses tile 22"):
        on._apply_choice(on._choice()._replace(tiles=[int(t) for t in tiles]))
    assert on.export_plan() == p_on   # nothing was written
    stale = _engine(monkeypatch, model, True, plan=dict(p_on, tiles=".".join(tiles), source="stale"))
    assert torch.equal(stale(x), ref) and stale.plan_source == "tuned in this process"
    # two chains inside one graph
    two = _engine(monkeypatch, model, True, chains=2)
    assert torch.equal(two(x), ref) and torch.equal(two(x), ref)
    assert len(two.subs) == 2 and _fields(two) == sorted(want * 2) and not two.overflowed()


def test_resnet18_and_resnet50b_get_none(monkeypatch):
    from hawq_amd.api import calibrate
    from hawq_amd.skeleton import synthetic_images
    for arch in ("resnet18", "resnet50b"):
        model = H.build_model(arch, "uniform8")
        calibrate(model, synthetic_images(2, 0).cuda())
        x = synthetic_images(3, seed=3).cuda()
        ref = _engine(monkeypatch, model, False)(x).clone()
        on = _engine(monkeypatch, model, True)
        assert torch.equal(on(x), ref) and _fields(on) == []
