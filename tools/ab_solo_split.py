"""Same-process A/B of the deeper slice splits and 64-pixel workgroups of the expand conv alone (fused_wp.hip).

usage: python tools/ab_solo_split.py --off-plan PARENT_PLANS.json [--plan profiles/plans.json] [--arch resnet50] [--scheme uniform8]
                                     [--batch 128] [--block 100] [--rounds 4] [--out FILE.json]

Builds the workload's engine twice in one process: "on" replays this tree's recorded plan as written, "off" replays the same plan with
every "@solo" entry of "fused_variants" set back to the id the PARENT commit's plans hold for it (passed as a file, e.g.
`git show HEAD~1:profiles/plans.json > parent_plans.json`).  The variant numbering is append-only, so those ids are the parent's kernels
on the parent's grids, and every other launch is the same in both engines.  Checks that both give the same logits, spins the part up
and times alternating blocks of `block` graph replays (off, on, off, on, ...): both engines see one thermal / clock state.  Prints one
JSON line: images/s of every block, the mean ratio, the within-side block spreads, and the verdict - a gain only if EVERY "on" block
beat EVERY "off" block AND the mean ratio exceeds 1 by at least three times the larger within-side spread."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from tools.retune_solo_split import solo_indices, variant_shape, with_variants  # noqa: E402


class _OffPlans(bench.Plans):
    """This tree's plans with the "@solo" entries of every workload set back to the parent's ids."""

    def __init__(self, path, parent_path):
        super().__init__(path, retune=False)
        with open(parent_path) as f:
            parent = json.load(f)
        for key, plan in self.loaded.items():
            idx = solo_indices(plan)
            if not idx or key not in parent:
                continue
            assert parent[key]["pair_launches"] == plan["pair_launches"], key
            old = parent[key]["fused_variants"].split(".")
            self.loaded[key] = with_variants(plan, idx, [int(old[k]) for k in idx], plan["pair_variant_counts"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="resnet50")
    ap.add_argument("--scheme", default="uniform8")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--plan", default=os.path.join(ROOT, "profiles", "plans.json"))
    ap.add_argument("--off-plan", required=True, help="the parent commit's profiles/plans.json")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 4, "at least four blocks per side"
    dev = torch.device("cuda:0")
    model, off, x = bench.setup_workload(args.arch, args.scheme, args.batch, dev, seed=1, plans=_OffPlans(args.plan, args.off_plan))
    _, on, _ = bench.setup_workload(args.arch, args.scheme, args.batch, dev, seed=1, plans=bench.Plans(args.plan, retune=False), model=model)
    y_off, y_on = off(x).clone(), on(x).clone()
    same = bool(torch.equal(y_off, y_on))

    def solo(eng):
        """name -> [variant id, [pixels per workgroup, slice split] or None] of chain 0's "@solo" launches (0: the plain hawq_conv2d form)."""
        e = (eng.subs or [eng])[0]
        return {n: [p.er.tile if p.fused else 0, variant_shape(p.er, p.er.tile if p.fused else 0)]
                for n, p in zip(e._er_names, e._er_args) if n.endswith("@solo")}

    def block(eng, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(eng.stream):
            for _ in range(n):
                eng.run_resident()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def alone_us(eng, reps=20):
        """us per launch of chain 0's "@solo" launches, each alone on the chip (HIP events around `reps` launches, the fastest of three)."""
        e = (eng.subs or [eng])[0]
        out = {}
        with torch.cuda.stream(e.stream):
            for n, p in zip(e._er_names, e._er_args):
                if not n.endswith("@solo"):
                    continue
                best = None
                for rnd in range(4):
                    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record(e.stream)
                    for _ in range(reps):
                        p()
                    end.record(e.stream)
                    end.synchronize()
                    if rnd:
                        t = start.elapsed_time(end) / reps * 1e3
                        best = t if best is None else min(best, t)
                out[n] = round(best, 2)
        return out

    bench.spin_up(off)
    bench.spin_up(on)
    us_off, us_on = alone_us(off), alone_us(on)
    block(off, 5), block(on, 5)
    t_off, t_on = [], []
    for _ in range(args.rounds):
        t_off.append(block(off, args.block))
        t_on.append(block(on, args.block))
    ips = lambda t: round(args.batch * args.block / t, 1)   # noqa: E731
    spread = lambda ts: (max(ts) - min(ts)) / (sum(ts) / len(ts))   # noqa: E731
    ratio = sum(t_off) / sum(t_on)
    every = bool(max(t_on) < min(t_off))
    worst = max(spread(t_off), spread(t_on))
    res = {"workload": f"{args.arch}_{args.scheme}_b{args.batch}", "off_plan_source": off.plan_source, "on_plan_source": on.plan_source,
           "chains": on.chains, "off_solo": solo(off), "on_solo": solo(on),
           "off_solo_alone_us": us_off, "on_solo_alone_us": us_on, "logits_bit_equal": same, "block_forwards": args.block,
           "off_images_per_s": [ips(t) for t in t_off], "on_images_per_s": [ips(t) for t in t_on],
           "off_ms_per_forward": round(sum(t_off) / len(t_off) / args.block * 1e3, 4), "on_ms_per_forward": round(sum(t_on) / len(t_on) / args.block * 1e3, 4),
           "mean_ratio_on_over_off": round(ratio, 4), "off_block_spread": round(spread(t_off), 4), "on_block_spread": round(spread(t_on), 4),
           "every_on_block_faster_than_every_off_block": every,
           "ratio_exceeds_one_by_three_spreads": bool(ratio - 1 >= 3 * worst),
           "gain": bool(every and ratio - 1 >= 3 * worst),
           "overflow": bool(on.overflowed() or off.overflowed())}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
