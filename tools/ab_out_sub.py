"""Same-process A/B of the stage handover on the stride-2 grid (hawq_conv_args.out_sub).

usage: python tools/ab_out_sub.py [--arch resnet50] [--scheme uniform8] [--batch 128] [--block 100] [--rounds 4] [--out FILE.json]

Builds the workload's engine twice from the recorded plan (profiles/plans.json) - once with HAWQ_NO_OUT_SUB=1 (every stage-final expand
launch evaluates all pixels: the launch list before the change) and once without - checks that both give the same logits, spins the part
up and times alternating blocks of `block` graph replays (off, on, off, on, ...), as bench.py times uint8 against fp32 input: both engines
see one thermal / clock state.  Prints one JSON line: images/s of every block, the mean ratio, and whether EVERY "on" block beat EVERY
"off" block (anything less is not a gain)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="resnet50")
    ap.add_argument("--scheme", default="uniform8")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--plan", default=os.path.join(ROOT, "profiles", "plans.json"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    plans = bench.Plans(args.plan, retune=False)

    def build(sub, model=None):
        if sub:
            os.environ.pop("HAWQ_NO_OUT_SUB", None)
        else:
            os.environ["HAWQ_NO_OUT_SUB"] = "1"
        try:
            return bench.setup_workload(args.arch, args.scheme, args.batch, dev, seed=1, plans=plans, model=model)
        finally:
            os.environ.pop("HAWQ_NO_OUT_SUB", None)

    model, off, x = build(False)
    _, on, _ = build(True, model)
    y_off, y_on = off(x).clone(), on(x).clone()
    same = bool(torch.equal(y_off, y_on))
    n_sub = sum(int(a.out_sub >= 2) for e in (on.subs or [on]) for a in list(e._conv_args) + [p.expand for p in e._er_args])

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
    ips = lambda t: round(args.batch * args.block / t, 1)
    res = {"workload": f"{args.arch}_{args.scheme}_b{args.batch}", "plan_source": on.plan_source, "chains": on.chains,
           "launches_with_out_sub": n_sub, "logits_bit_equal": same, "block_forwards": args.block,
           "off_images_per_s": [ips(t) for t in t_off], "on_images_per_s": [ips(t) for t in t_on],
           "mean_ratio_on_over_off": round(sum(t_off) / sum(t_on), 4),
           "every_on_block_faster_than_every_off_block": bool(max(t_on) < min(t_off)),
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
