"""Same-process A/B of the stage-final 3x3 convs on the next stage's grid (out_sub on a 3x3 launch, res_sub behind it).

usage: python tools/ab_conv2_sub.py --off-plan PARENT_PLANS.json [--plan profiles/plans.json] [--arch resnet50] [--scheme uniform8]
                                    [--batch 128] [--block 100] [--rounds 4] [--out FILE.json]

Builds the workload's engine twice in one process: "off" replays the PARENT commit's recorded plans (passed as a file, e.g.
`git show HEAD~1:profiles/plans.json > parent_plans.json`) with HAWQ_NO_CONV2_SUB=1 - the parent's launches -, "on" replays this
tree's plans.  Checks that both give the same logits, spins the part up and times alternating blocks of `block` graph replays
(off, on, off, on, ...): both engines see one thermal / clock state.  Prints one JSON line: images/s of every block, the mean ratio,
the within-side block spreads, and the verdict - a gain only if EVERY "on" block beat EVERY "off" block AND the mean ratio exceeds 1
by at least three times the larger within-side spread."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from hawq_amd import _lib  # noqa: E402


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
    dev = torch.device("cuda:0")

    def build(on, model=None):
        plans = bench.Plans(args.plan if on else args.off_plan, retune=False)
        if on:
            os.environ.pop("HAWQ_NO_CONV2_SUB", None)
        else:
            os.environ["HAWQ_NO_CONV2_SUB"] = "1"
        try:
            return bench.setup_workload(args.arch, args.scheme, args.batch, dev, seed=1, plans=plans, model=model)
        finally:
            os.environ.pop("HAWQ_NO_CONV2_SUB", None)

    model, off, x = build(False)
    _, on, _ = build(True, model)
    y_off, y_on = off(x).clone(), on(x).clone()
    same = bool(torch.equal(y_off, y_on))
    launches = [a for e in (on.subs or [on]) for a in list(e._conv_args) + [p.expand for p in e._er_args]]
    n_c2 = sum(int(a.out_sub >= 2 and a.KH == 3) for a in launches)
    n_rs = sum(int(_lib.res_sub(a) >= 2) for a in launches)

    def block(eng, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(eng.stream):
            for _ in range(n):
                eng.run_resident()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    bench.spin_up(off)
    bench.spin_up(on)
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
           "chains": on.chains, "strided_3x3_launches": n_c2, "res_sub_launches": n_rs, "logits_bit_equal": same, "block_forwards": args.block,
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
