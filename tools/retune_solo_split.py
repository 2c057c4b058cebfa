"""Re-decide, in a file of recorded plans, ONLY the expand-alone ("@solo") entries of "fused_variants", and bring "pair_variant_counts"
up to the counts of this library (fused_wp.hip offers the expand conv alone more slice splits and 64-pixel workgroups; a plan recorded
with the old counts is stale and bench.py would tune afresh).

usage: python tools/retune_solo_split.py [--plan profiles/plans.json] [--out FILE] [--only KEY[,KEY...]] [--log FILE.json] [--margin 0.03]
       python tools/retune_solo_split.py --from-log LOG.json [--plan ...] [--out FILE] [--margin 0.03]       (host only, no GPU)

For every workload of the file whose pair list has "@solo" entries this tool
  * builds the workload's engine from its recorded plan with only "pair_variant_counts" replaced by this library's (the recorded ids
    keep their meaning: the numbering is append-only), and checks that it replays;
  * times, for each "@solo" launch, every variant the library reports and the plain hawq_conv2d form (0) with ALL chains launching that
    layer at once, each on its own stream, as IntegerEngine._autotune_joint does - two passes, the faster time of a form counts;
  * decides (`decide`): the forms within `margin` of the fastest are equally good as far as this timing can tell; the recorded form
    stays if it is one of them, else the one with the lowest id wins - timing noise moves no entry, and a newer table row has to beat
    the older ones by more than the noise to be chosen;
  * writes the winner into "fused_variants" (and every "per_chain" entry) and checks that the logits did not move by a bit.
Every other entry, every other workload and the file's formatting stay byte-identical (json.dump(indent=1, sort_keys=True), as
bench.py --save-plan writes it).  The log holds the times behind every decision and the launch shape (pixels per workgroup, slice
split) of every timed variant.

--from-log: table rows that no workload chose are taken out of the variant table again, which renumbers the rows behind them.  This
mode takes the times and shapes a timing run logged, decides by the same rule among the forms THIS library still has (matched by
shape), and writes their ids and this library's counts - from the host-only queries alone."""
import argparse
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hawq_amd import _lib  # noqa: E402

PTR = 16   # dummy non-null pointer: the host-only queries test pointers against NULL and never dereference them


def solo_indices(plan):
    return [k for k, n in enumerate(plan.get("pair_launches") or []) if n.endswith("@solo")]


def variant_shape(er, v):
    """(pixels per workgroup, slice split) of variant `v` of launch `er`, or None for a variant of another kernel family / the plain form."""
    px, ys = C.c_int32(), C.c_int32()
    if v <= 0 or _lib.load().hawq_conv_expand_reduce_variant_shape(C.byref(er), v, C.byref(px), C.byref(ys)) != 0:
        return None
    return [px.value, ys.value]


def host_solo_args(c):
    """The expand conv alone of a bottleneck unit with `c` input channels, as far as the host-only variant queries read it."""
    er = _lib.ExpandReduceArgs()
    e = er.expand
    e.in_, e.wgt, e.bias, e.m, e.e, e.ctab, e.flags, e.res_in, e.out_q = (PTR,) * 9
    e.N, e.H, e.W, e.Cin, e.Cout, e.KH, e.KW, e.stride, e.pad = 1, 7, 7, c, 4 * c, 1, 1, 1, 0
    e.in_bits, e.w_bits, e.epilogue, e.fast_tables, e.res_in_bits = 8, 8, _lib.EPI_RESIDUAL, 1, 16
    e.out_bits, e.q_lo, e.q_hi, e.mq, e.eq, e.m_id_scalar, e.e_id_scalar = 8, 0, 127, 3, 34, 5, 35
    return er


def decide(times, was, margin):
    """The form to run, from {form: time}: `was` if it is within `margin` of the fastest, else the lowest id that is."""
    best = min(times.values())
    good = [v for v, t in times.items() if t * (1.0 - margin) <= best]
    return was if was in good else min(good)


def stage_channels(name):
    """Input channels of the expand conv `stage<s>.unit<u>.quant_convbn3@solo` of a bottleneck ResNet."""
    return 64 << (int(re.match(r"stage(\d+)\.", name)[1]) - 1)


def with_variants(plan, idx, values, counts):
    """`plan` with the "fused_variants" entries `idx` set to `values` in every chain and "pair_variant_counts" set to `counts`;
    nothing else is touched."""
    def fix(d):
        d = dict(d)
        if d.get("fused_variants"):
            parts = d["fused_variants"].split(".")
            for i, v in zip(idx, values):
                parts[i] = str(v)
            d["fused_variants"] = ".".join(parts)
        return d
    out = fix(plan)
    out["pair_variant_counts"] = [int(v) for v in counts]
    if plan.get("per_chain"):
        out["per_chain"] = [fix(p) for p in plan["per_chain"]]
    return out


def retune(key, plan, dev, log, margin):
    import torch

    from hawq_amd.api import build_quantized_resnet, calibrate
    from hawq_amd.engine import IntegerEngine
    from hawq_amd.skeleton import synthetic_images
    from tools.retune_conv2_sub import joint_ms
    m = re.fullmatch(r"(resnet\w+?)_(.+)_b(\d+)", key)
    arch, scheme, batch = m.group(1), m.group(2), int(m.group(3))
    model = build_quantized_resnet(arch, scheme, seed=0).to(dev)
    calibrate(model, synthetic_images(8, seed=0).to(dev))
    x = synthetic_images(batch, seed=1).to(dev)
    # this library's counts: read off a build that leaves every choice to the library (no timing, no launch)
    probe = IntegerEngine(model, use_graph=False, autotune=False, chains=int(plan["chains"]))
    probe._build(batch, x.shape[2], x.shape[3])
    e0 = (probe.subs or [probe])[0]
    assert e0._er_names == plan["pair_launches"], (key, "the recorded plan lists other pairs")
    counts = e0._variant_counts()
    del probe
    idx = solo_indices(plan)
    # append-only numbering: a count may only grow, and only on the expand-alone entries
    assert all(n >= o and (n == o or k in idx) for k, (n, o) in enumerate(zip(counts, plan["pair_variant_counts"]))), (key, counts)
    recorded = [int(plan["fused_variants"].split(".")[k]) for k in idx]
    base = with_variants(plan, idx, recorded, counts)
    eng = IntegerEngine(model, use_graph=True, plan=dict(base, source="replayed"))
    ref = eng(x).clone()
    assert eng.plan_source == "replayed", (key, "the recorded plan was not replayed", eng.plan_source)
    chains = eng.subs or [eng]
    chosen = [sub._choice() for sub in chains]
    entry = log.setdefault(key, {"launches": {}})
    probe_choice = _lib.ConvChoice()
    with torch.cuda.stream(eng.stream):
        for k, was in zip(idx, recorded):
            name = plan["pair_launches"][k]
            forms = list(range(1, counts[k] + 1))
            # the plain form runs the recorded two-launch tile: only where every chain's library still takes it as the launch is built
            if all(_lib.load().hawq_conv2d_choice(C.byref(sub._er_args[k].expand), C.byref(probe_choice)) == 0 for sub in chains):
                forms.append(0)
            assert was in forms, (key, name, was)
            times = {}

            def choose(v):
                for sub in chains:
                    p = sub._er_args[k]
                    p.fused = v != 0
                    if v:
                        p.er.tile = v
            for rnd in range(2):
                for v in forms:
                    choose(v)
                    ms = joint_ms(eng, chains, lambda sub: sub._er_args[k]())
                    times[v] = min(times.get(v, ms), ms)
            best = decide(times, was, margin)
            choose(best)
            for ch in chosen:
                ch.variants[k] = best
            er = chains[0]._er_args[k].er
            entry["launches"][name] = {"recorded": was, "chosen": best, "chosen_shape": variant_shape(er, best),
                                       "variants": counts[k], "shapes": {str(v): variant_shape(er, v) for v in forms if v},
                                       "us_all_chains": {str(v): round(t / 4 * 1e3, 2) for v, t in sorted(times.items())}}
    torch.cuda.synchronize(dev)
    for sub, ch in zip(chains, chosen):
        sub._apply_choice(ch)
        sub.flags.zero_()
    eng._drop_graph()
    assert torch.equal(eng(x), ref), (key, "the logits moved")
    new = eng.export_plan()
    out = with_variants(plan, idx, [chosen[0].variants[k] for k in idx], counts)
    # what the engine exports is what was written: only the re-decided entries and the counts differ from the recorded plan
    for k in new:
        if k != "per_chain":
            assert new[k] == out[k], (key, k)
    for p_new, p_out in zip(new.get("per_chain") or [], out.get("per_chain") or []):
        assert p_new == p_out, key
    del eng
    torch.cuda.empty_cache()
    return out


def from_log(key, plan, logged, margin):
    idx = solo_indices(plan)
    counts, values = list(plan["pair_variant_counts"]), []
    for k in idx:
        name = plan["pair_launches"][k]
        er = host_solo_args(stage_channels(name))
        counts[k] = int(_lib.load().hawq_conv_expand_reduce_variants(C.byref(er)))
        have = {tuple(variant_shape(er, v)): v for v in range(1, counts[k] + 1)}
        was, seen = logged["launches"][name], {}
        for v, us in was["us_all_chains"].items():   # logged id -> id in this library (0 stays 0; a form this library lacks drops out)
            now = 0 if v == "0" else have.get(tuple(was["shapes"][v]))
            if now is not None:
                seen[now] = us
        assert was["recorded"] in seen and (was["recorded"] == 0 or tuple(was["shapes"][str(was["recorded"])]) == tuple(variant_shape(er, was["recorded"]))), (key, name)
        values.append(decide(seen, was["recorded"], margin))
    return with_variants(plan, idx, values, counts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plan", default=os.path.join(ROOT, "profiles", "plans.json"))
    ap.add_argument("--out", default=None, help="where to write the plans (default: --plan, in place)")
    ap.add_argument("--only", default="", help="comma-separated workload keys (default: every workload of the file with @solo entries)")
    ap.add_argument("--log", default=None, help="the times behind every decision, as JSON")
    ap.add_argument("--margin", type=float, default=0.03, help="forms whose times differ by less than this fraction count as equally fast")
    ap.add_argument("--from-log", default=None, metavar="LOG.json", help="host only: decide from the times and shapes a timing run logged")
    args = ap.parse_args()
    with open(args.plan) as f:
        plans = json.load(f)
    only = [k for k in args.only.split(",") if k]
    keys = [k for k in sorted(plans) if (not only or k in only) and solo_indices(plans[k])]
    log = {}
    if args.from_log:
        with open(args.from_log) as f:
            logged = json.load(f)
        for key in keys:
            plans[key] = from_log(key, plans[key], logged[key], args.margin)
    else:
        import torch
        dev = torch.device("cuda:0")
        for key in keys:
            plans[key] = retune(key, plans[key], dev, log, args.margin)
            print(json.dumps({key: log[key]}), flush=True)
    with open(args.out or args.plan, "w") as f:
        json.dump(plans, f, indent=1, sort_keys=True)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            json.dump(log, f, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
