"""The expand-alone ("@solo") launches of ResNet50 on the last variant the library offers them - the newest row of the variant table
of fused_wp.hip that takes the launch - against the same plan on variant 1: logits and every stored residual must not move by a bit, in
one chain and in two; the plan round-trips through JSON; a plan that carries the variant counts from before the table grew is stale
and is re-tuned to the same logits."""
import json
import re

import pytest
import torch

from hawq_amd import plan as _plan
from tests import helpers as H

pytestmark = pytest.mark.gpu

# variants of the expand conv alone before the table grew, by input channels (what plans recorded until then carry)
COUNTS_BEFORE = {64: 1, 128: 1, 256: 3, 512: 4}


def _taps(eng):
    return [(name, t.clone()) for e in (eng.subs or [eng]) for name, (t, _) in sorted(e.res_taps.items())]


def _solo(plan):
    return [k for k, n in enumerate(plan["pair_launches"]) if n.endswith("@solo")]


def _forced(plan, pick):
    """`plan` with every "@solo" entry of "fused_variants" set to pick(count of that launch), in every chain."""
    def fix(d):
        d = dict(d)
        if d.get("fused_variants"):
            parts = d["fused_variants"].split(".")
            for k in _solo(plan):
                parts[k] = str(pick(plan["pair_variant_counts"][k]))
            d["fused_variants"] = ".".join(parts)
        return d
    out = fix(plan)
    if plan.get("per_chain"):
        out["per_chain"] = [fix(p) for p in plan["per_chain"]]
    return out


def _variants(eng):
    return [[p.er.tile if p.fused else 0 for n, p in zip(e._er_names, e._er_args) if n.endswith("@solo")] for e in (eng.subs or [eng])]


@pytest.mark.parametrize("scheme", ["uniform8", "uniform4"])
def test_resnet50_batch4_last_variant_equals_the_first(scheme):
    from hawq_amd.api import calibrate
    from hawq_amd.engine import IntegerEngine, StalePlan
    from hawq_amd.skeleton import synthetic_images
    model = H.build_model("resnet50", scheme)
    calibrate(model, synthetic_images(2, 0).cuda())
    x = torch.cat([synthetic_images(2, 0), synthetic_images(2, seed=3) * 1.3 + 0.1]).cuda()   # batch 4
    for chains in (1, 2):
        tuned = IntegerEngine(model, chains=chains)
        ref = tuned(x).clone()
        p = tuned.export_plan()
        solo = _solo(p)
        counts = [p["pair_variant_counts"][k] for k in solo]
        before = [COUNTS_BEFORE[64 << (int(re.match(r"stage(\d+)\.", p["pair_launches"][k])[1]) - 1)] for k in solo]
        assert len(solo) == 4 and all(c >= b for c, b in zip(counts, before)) and counts != before, counts
        first = IntegerEngine(model, plan=dict(_forced(p, lambda n: 1), source="first"))
        y1 = first(x).clone()
        taps1 = _taps(first)
        assert first.plan_source == "first" and _variants(first) == [[1] * 4] * chains and not first.overflowed()
        assert torch.equal(y1, ref)
        p_last = _forced(p, lambda n: n)
        last = IntegerEngine(model, plan=dict(p_last, source="last"))
        y = last(x).clone()
        assert last.plan_source == "last" and _variants(last) == [counts] * chains
        assert torch.equal(y, y1) and torch.equal(last(x), y1) and not last.overflowed()   # (the second call replays the graph)
        taps = _taps(last)
        assert [n for n, _ in taps] == [n for n, _ in taps1] and len(taps) >= 10 * chains
        for (name, t), (_, r) in zip(taps, taps1):
            assert torch.equal(t, r), name
        # the plan survives a JSON round trip and replays to the same bits
        p_exp = last.export_plan()
        assert p_exp["fused_variants"] == p_last["fused_variants"] and p_exp["pair_variant_counts"] == p["pair_variant_counts"]
        again = IntegerEngine(model, plan=dict(json.loads(json.dumps(p_exp)), source="round trip"))
        assert torch.equal(again(x), y1) and again.plan_source == "round trip" and again.export_plan() == p_exp
        if chains == 1:
            # the counts from before the table grew: stale, and tuned afresh to the same logits
            old = list(p["pair_variant_counts"])
            for k, b in zip(solo, before):
                old[k] = b
            e = last
            with pytest.raises(StalePlan, match="numbered differently"):
                _plan.decode(dict(p_last, pair_variant_counts=old), 0, e._conv_names, len(e._er_args), p["num_conv_tiles"], e._variant_counts())
            stale = IntegerEngine(model, plan=dict(_forced(p, lambda n: 1), pair_variant_counts=old, source="stale"))
            assert torch.equal(stale(x), y1) and stale.plan_source == "tuned in this process"
            assert stale.export_plan()["pair_variant_counts"] == p["pair_variant_counts"]
