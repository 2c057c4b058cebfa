"""Re-decide, in a file of recorded plans, ONLY the 3x3 launches that run on the next stage's grid (hawq_conv_args.out_sub on a 3x3).

usage: python tools/retune_conv2_sub.py [--plan profiles/plans.json] [--out FILE] [--only KEY[,KEY...]] [--log FILE.json]

The recorded ids of those launches belong to kernels that refuse the strided form (band_v1, band_persist), and a replay is strict: it
does not substitute another id.  For every workload of the file whose launch list has such launches this tool
  * builds the workload's engine from its recorded plan, with the entries of those launches left to the library's own choice
    (tile 0) and their split-K entries cleared, so that every buffer holds valid data;
  * times every tile id the library takes for the launch (hawq_conv2d_choice) with ALL chains launching that layer at once, each on
    its own stream, as IntegerEngine._autotune_joint does - and the split-K counts the library takes, if any;
  * writes the winner into "tiles" (and "splitk", and every "per_chain" entry) of that workload.
Every other entry, every other workload and the file's formatting stay byte-identical (json.dump(indent=1, sort_keys=True), as
bench.py --save-plan writes it); workloads without such launches (ResNet18, ResNet50b) are only checked to replay as they are."""
import argparse
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from hawq_amd import _lib  # noqa: E402


def strided_3x3(e):
    """Indices, in a chain's conv launch list, of the 3x3 launches that carry out_sub."""
    return [k for k, a in enumerate(e._conv_args) if a.out_sub >= 2 and a.KH == 3]


def applicable_tiles(a):
    """Tile ids hawq_conv2d takes for launch `a` (host-only query; `a.tile` is restored)."""
    keep, ids, ch = a.tile, [], _lib.ConvChoice()
    for t in range(1, _lib.load().hawq_conv2d_num_tiles() + 1):
        a.tile = t
        if _lib.load().hawq_conv2d_choice(C.byref(a), C.byref(ch)) == 0:
            ids.append(t)
    a.tile = keep
    return ids


def joint_ms(eng, chains, launch, reps=4):
    """ms of `reps` launches per chain, all chains at once (IntegerEngine._autotune_joint): warm-up round, then the minimum of three."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = None
    for rnd in range(4):
        start.record(eng.stream)
        for sub in chains:
            sub.stream.wait_event(start)
            for _ in range(reps):
                launch(sub)
            j = torch.cuda.Event()
            j.record(sub.stream)
            eng.stream.wait_event(j)
        end.record(eng.stream)
        end.synchronize()
        if rnd:
            t = start.elapsed_time(end)
            best = t if best is None else min(best, t)
    return best


def patched(plan, names, value="0"):
    """`plan` with the "tiles" (and "splitk") entries of the launches `names` set to `value` / 0, in every chain."""
    idx = [plan["conv_launches"].index(n) for n in names]

    def fix(d):
        d = dict(d)
        for key, v in (("tiles", value), ("splitk", "0")):
            if d.get(key):
                parts = d[key].split(".")
                for i in idx:
                    parts[i] = v
                d[key] = ".".join(parts)
        return d
    out = fix(plan)
    if plan.get("per_chain"):
        out["per_chain"] = [fix(p) for p in plan["per_chain"]]
    return out


def retune(key, plan, dev, log):
    from hawq_amd.api import build_quantized_resnet, calibrate
    from hawq_amd.engine import IntegerEngine
    from hawq_amd.skeleton import synthetic_images
    m = re.fullmatch(r"(resnet\w+?)_(.+)_b(\d+)", key)
    arch, scheme, batch = m.group(1), m.group(2), int(m.group(3))
    model = build_quantized_resnet(arch, scheme, seed=0).to(dev)
    calibrate(model, synthetic_images(8, seed=0).to(dev))
    x = synthetic_images(batch, seed=1).to(dev)
    # which launches: read off a build that leaves every choice to the library (no timing, no launch)
    probe = IntegerEngine(model, use_graph=False, autotune=False, chains=int(plan["chains"]))
    probe._build(batch, x.shape[2], x.shape[3])
    e0 = (probe.subs or [probe])[0]
    names = [e0._conv_names[k] for k in strided_3x3(e0)]
    del probe
    if not names:
        eng = IntegerEngine(model, use_graph=True, plan=dict(plan, source="replayed"))
        eng(x)
        assert eng.plan_source == "replayed", (key, eng.plan_source)
        log[key] = {"launches": [], "replays_unchanged": True}
        return plan
    eng = IntegerEngine(model, use_graph=True, plan=dict(patched(plan, names), source="replayed"))
    ref = eng(x).clone()
    assert eng.plan_source == "replayed", (key, "the patched plan was not replayed", eng.plan_source)
    chains = eng.subs or [eng]
    chosen = [sub._choice() for sub in chains]
    entry = log.setdefault(key, {"launches": {}})
    with torch.cuda.stream(eng.stream):
        for name in names:
            k = chains[0]._conv_names.index(name)
            ids = sorted(set.intersection(*(set(applicable_tiles(sub._conv_args[k])) for sub in chains)))
            splits = sorted(set.intersection(*(set(sub._splitk_options(sub._conv_args[k])) for sub in chains)))
            times = {}

            def choose(t):   # t > 0: tile id; t < 0: split-K with -t slices (the unsplit form keeps the fastest tile)
                for sub, ch in zip(chains, chosen):
                    if t > 0:
                        sub._conv_args[k].tile = ch.tiles[k] = t
                    sub._conv_ops[k].splitk = ch.splitk[k] = -t if t < 0 else 0
                    if t < 0:
                        sub._ws.fit(sub._conv_args[k], -t)
            for rnd in range(2):
                for t in ids:
                    choose(t)
                    ms = joint_ms(eng, chains, lambda sub: sub._conv_ops[k]())
                    times[t] = min(times.get(t, ms), ms)
            best = min(times, key=times.get)
            choose(best)
            for s in splits:
                choose(-s)
                times[-s] = joint_ms(eng, chains, lambda sub: sub._conv_ops[k]())
            best = min(times, key=times.get)
            choose(best if best > 0 else min((t for t in times if t > 0), key=times.get))
            if best < 0:
                choose(best)
            entry["launches"][name] = {"chosen": best, "us_all_chains": {str(t): round(v / 4 * 1e3, 2) for t, v in sorted(times.items())}}
    torch.cuda.synchronize(dev)
    for sub, ch in zip(chains, chosen):
        sub._apply_choice(ch)
        sub.flags.zero_()
    eng._drop_graph()
    assert torch.equal(eng(x), ref), (key, "the logits moved")
    new = eng.export_plan()
    # only the strings of the re-decided launches move: everything else must read as it did
    for k in ("batch", "chains", "expand_in8", "conv_launches", "pair_launches", "num_conv_tiles", "pair_variant_counts", "fused_variants",
              "fused_split_tiles"):
        assert new.get(k) == plan.get(k), (key, k)
    out = dict(plan)
    out["tiles"] = new["tiles"]
    for k in ("splitk", "per_chain"):
        if k in new:
            out[k] = new[k]
        else:
            out.pop(k, None)
    idx = {plan["conv_launches"].index(n) for n in names}

    def same_elsewhere(a, b):
        a, b = a.split("."), b.split(".")
        return len(a) == len(b) and all(x == y for i, (x, y) in enumerate(zip(a, b)) if i not in idx)
    assert same_elsewhere(plan["tiles"], out["tiles"]), key
    for p_old, p_new in zip(plan.get("per_chain") or [], out.get("per_chain") or []):
        assert same_elsewhere(p_old["tiles"], p_new["tiles"]), key
    del eng
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plan", default=os.path.join(ROOT, "profiles", "plans.json"))
    ap.add_argument("--out", default=None, help="where to write the plans (default: --plan, in place)")
    ap.add_argument("--only", default="", help="comma-separated workload keys (default: every ResNet workload of the file)")
    ap.add_argument("--log", default=None, help="the times behind every decision, as JSON")
    args = ap.parse_args()
    with open(args.plan) as f:
        plans = json.load(f)
    dev = torch.device("cuda:0")
    only = [k for k in args.only.split(",") if k]
    log = {}
    for key in sorted(plans):
        if (only and key not in only) or not key.startswith("resnet") or "conv_launches" not in plans[key]:
            continue
        plans[key] = retune(key, plans[key], dev, log)
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
