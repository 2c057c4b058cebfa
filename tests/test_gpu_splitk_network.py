"""Whole networks with split-K conv launches (hawq_conv2d_splitk) forced through a recorded plan's "splitk" entry: logits bit-equal
to the CPU oracle; plan round trip; the recorded plans of profiles/plans.json still replay without any split launch."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

CANDIDATES = (2, 4, 8, 16, 32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _accepted(a):
    from hawq_amd import _lib
    return [] if a is None else [s for s in CANDIDATES if _lib.load().hawq_conv2d_splitk_ok(C.byref(a), s)]


def _forced_plan(eng):
    """The engine's tuned plan with every pair run as two launches and every launch the library takes split (slice counts
    cycling through the accepted ones, so that every count runs somewhere)."""
    plan = dict(eng.export_plan())
    e = eng.subs[0] if eng.subs else eng
    vals, i = [], 0
    for a in [op.a for op in e._conv_ops] + [x for p in e._er_args for x in (p.expand, p.reduce)]:
        acc = _accepted(a)
        vals.append(acc[i % len(acc)] if acc else 0)
        i += bool(acc)
    plan["splitk"] = ".".join(map(str, vals))
    plan["fused_variants"] = ".".join("0" for _ in e._er_args)
    for pc in plan.get("per_chain", []):
        pc["splitk"], pc["fused_variants"] = plan["splitk"], plan["fused_variants"]
    return plan, sum(v > 0 for v in vals) * max(1, len(eng.subs))   # (every chain runs the same launches)


def _model(arch, scheme):
    from hawq_amd.api import calibrate
    from hawq_amd.skeleton import synthetic_images
    model = H.build_model(arch, scheme)
    calibrate(model, synthetic_images(2, 0).cuda())
    return model


def _forced_engine(model, batch, chains=0):
    from hawq_amd.engine import IntegerEngine
    from hawq_amd.skeleton import synthetic_images
    tuned = IntegerEngine(model, chains=chains)
    tuned(synthetic_images(batch, seed=1).cuda())
    plan, n_split = _forced_plan(tuned)
    eng = IntegerEngine(model, plan=plan, chains=chains)
    return eng, plan, n_split


def _check(model, eng, n_split, batch, seed=5, scale=1.0):
    from hawq_amd.skeleton import synthetic_images
    from oracle import oracle
    x = synthetic_images(batch, seed=seed) * scale
    ref, _ = oracle.forward_int(oracle.extract_float_state(model), x.numpy())
    y1 = eng(x.cuda()).clone()
    y2 = eng(x.cuda()).clone()   # graph replay
    assert eng.plan_source.startswith("replayed")
    assert eng.n_splitk() == n_split > 0
    assert np.array_equal(y1.cpu().numpy(), ref) and torch.equal(y1, y2)
    return x, ref


@pytest.mark.parametrize("batch", [1, 3, 16])
@pytest.mark.parametrize("arch", ["resnet50", "resnet18", "resnet50b"])
def test_uniform8_with_split_k_forced_matches_the_oracle(arch, batch):
    model = _model(arch, "uniform8")
    eng, _, n_split = _forced_engine(model, batch)
    _check(model, eng, n_split, batch)
    assert not eng.overflowed()


@pytest.mark.parametrize("scheme", ["bops_0.5", "uniform4"])
def test_4bit_schedules_with_split_k_on_their_8bit_launches(scheme):
    model = _model("resnet50", scheme)
    eng, _, n_split = _forced_engine(model, 1)
    _check(model, eng, n_split, 1)


def test_uint8_input_with_split_k_forced():
    model = _model("resnet50", "uniform8")
    eng, _, n_split = _forced_engine(model, 1)
    g = torch.Generator().manual_seed(3)
    xu8 = torch.randint(0, 256, (1, 224, 224, 3), dtype=torch.uint8, generator=g)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    t = xu8.permute(0, 3, 1, 2).to(torch.float32).div(255)
    t = t.sub_(torch.tensor(mean).view(1, 3, 1, 1)).div_(torch.tensor(std).view(1, 3, 1, 1))
    from oracle import oracle
    ref, _ = oracle.forward_int(oracle.extract_float_state(model), t.numpy())
    assert np.array_equal(eng.forward_uint8(xu8.cuda(), mean, std).cpu().numpy(), ref)
    assert np.array_equal(eng.forward_uint8(xu8.cuda(), mean, std).cpu().numpy(), ref)   # graph replay
    assert eng.n_splitk() == n_split > 0


def test_two_chain_engine_at_batch_16_with_split_k_forced():
    model = _model("resnet50", "uniform8")
    eng, _, n_split = _forced_engine(model, 16, chains=2)
    _check(model, eng, n_split, 16)
    assert eng.chains == 2 and len(eng.subs) == 2


def test_uint16_overflow_fallback_stays_exact_with_split_k():
    model = _model("resnet18", "uniform8")
    eng, _, n_split = _forced_engine(model, 3)
    from hawq_amd.skeleton import synthetic_images
    from oracle import oracle
    x = synthetic_images(3, seed=3) * 6   # out of calibration: un-clamped residuals beyond 65535
    ref, tr = oracle.forward_int(oracle.extract_float_state(model), x.numpy())
    assert max(int(v.max()) for k, v in tr.items() if k.endswith("quant_act_int32.q")) > 65535
    y = eng(x.cuda())
    assert np.array_equal(y.cpu().numpy(), ref)
    assert eng.overflow_fallbacks == 1 and not eng.overflowed() and eng.n_splitk() == n_split > 0


def test_tuned_batch1_plan_round_trip_and_refused_slice_counts():
    from hawq_amd.engine import IntegerEngine, StalePlan
    from hawq_amd.skeleton import synthetic_images
    model = _model("resnet50", "uniform8")
    x = synthetic_images(1, seed=9).cuda()
    tuned = IntegerEngine(model)
    y = tuned(x).clone()
    plan = tuned.export_plan()
    again = IntegerEngine(model, plan=plan)
    assert torch.equal(again(x), y) and again.plan_source.startswith("replayed")
    assert again.export_plan().get("splitk") == plan.get("splitk")
    assert again.n_splitk() == tuned.n_splitk()
    print("tuned batch-1 plan: split launches", tuned.n_splitk(), "splitk", plan.get("splitk"))
    # a slice count the library refuses (7 divides no conv's K chunk count here)
    forced, _ = _forced_plan(tuned)
    vals = forced["splitk"].split(".")
    vals[next(i for i, v in enumerate(vals) if v != "0")] = "7"
    bad = dict(forced, splitk=".".join(vals))
    with pytest.raises(StalePlan):
        tuned._set_splitk([int(v) for v in bad["splitk"].split(".")])
    eng = IntegerEngine(model, plan=bad)   # the constructor's plan: refused -> tuned instead
    assert torch.equal(eng(x), y) and not eng.plan_source.startswith("replayed")


@pytest.mark.parametrize("key", ["resnet50_uniform8_b16", "resnet50_uniform8_b128"])
def test_recorded_plans_replay_without_split_launches(key):
    from hawq_amd import _lib
    from hawq_amd.engine import IntegerEngine
    from hawq_amd.skeleton import synthetic_images
    with open(os.path.join(ROOT, "profiles", "plans.json")) as f:
        plans = json.load(f)
    plan = plans[key]
    assert "splitk" not in plan and int(plan["num_conv_tiles"]) == _lib.load().hawq_conv2d_num_tiles() == 28
    model = _model("resnet50", "uniform8")
    eng = IntegerEngine(model, plan=plan)
    eng(synthetic_images(int(plan["batch"]), seed=2).cuda())
    assert eng.plan_source.startswith("replayed")
    assert eng.n_splitk() == 0 and not any(eng.splitk_choice())
    assert eng.export_plan()["tiles"] == plan["tiles"] and "splitk" not in eng.export_plan()
