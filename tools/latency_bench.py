"""Small-batch latency with and without split-K conv launches (hawq_conv2d_splitk).

For each network and batch size: tune one plan (the per-launch tuner tries split-K where a launch has fewer output tiles than the
chip has CUs), then replay it two ways in this process - as tuned, and with its "splitk" entry zeroed (today's kernels for every
launch) - alternating blocks of hipGraph replays timed with HIP events after a warm-up.  Both forms run on ONE engine (the same
buffers, two captured graphs), so that buffer placement cannot differ between them.  Per point: median / p10 / p90 ms per forward
over the blocks, split launches, and whether both replays give logits bit-equal to the CPU oracle.  Prints one JSON line.

    python tools/latency_bench.py --arch resnet50 resnet18 --batch 1 2 4 8 16 [--profile-out profiles/X.json]

--profile-out: IntegerEngine.profile_ops() per-launch times (eager launches, median of 20) of both replays at the first and last batch
size of the list, for the first network."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def use_form(eng, graphs, form):
    """Make `form` ("split" / "nosplit") the engine's launch list and captured graph (captured on first use)."""
    for e, sk in zip(eng.subs or [eng], graphs["splitk"][form]):
        e._set_splitk(sk)
    eng._graph = graphs.get(form)
    if eng._graph is None:
        eng.run_resident()   # captures
        torch.cuda.synchronize()
        graphs[form] = eng._graph


def block_ms(eng, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(eng.stream):
        start.record(eng.stream)
        for _ in range(reps):
            eng.run_resident()
        end.record(eng.stream)
    end.synchronize()
    return start.elapsed_time(end) / reps


def stats(v):
    v = np.asarray(v)
    return {"median": round(float(np.median(v)), 5), "p10": round(float(np.percentile(v, 10)), 5),
            "p90": round(float(np.percentile(v, 90)), 5), "blocks": int(v.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", nargs="+", default=["resnet50", "resnet18"])
    ap.add_argument("--scheme", default="uniform8")
    ap.add_argument("--batch", nargs="+", type=int, default=[1, 2, 4, 8, 16])
    ap.add_argument("--seconds", type=float, default=0.6, help="timed seconds per replay form and point (>= 0.5)")
    ap.add_argument("--profile-out", default=None)
    args = ap.parse_args()
    from hawq_amd.api import build_quantized_resnet, calibrate
    from hawq_amd.engine import IntegerEngine
    from hawq_amd.skeleton import synthetic_images
    from oracle import oracle

    dev = torch.device("cuda", 0)
    points, profiles = [], {}
    for ai, arch in enumerate(args.arch):
        model = build_quantized_resnet(arch, args.scheme, seed=0).to(dev)
        calibrate(model, synthetic_images(2, seed=0).to(dev))
        st = oracle.extract_float_state(model)
        for batch in args.batch:
            x = synthetic_images(batch, seed=11)
            ref, _ = oracle.forward_int(st, x.numpy())
            t0 = time.time()
            tuned = IntegerEngine(model)
            tuned(x.to(dev))
            plan = tuned.export_plan()
            tune_s = time.time() - t0
            del tuned
            eng = IntegerEngine(model, plan=plan)
            y = eng(x.to(dev))
            assert eng.plan_source.startswith("replayed")
            chains = eng.subs or [eng]
            graphs = {"splitk": {"split": [e.splitk_choice() for e in chains],
                                 "nosplit": [[0] * len(e.splitk_choice()) for e in chains]}, "split": eng._graph}
            n_split = eng.n_splitk()
            parity = {"split": bool(np.array_equal(y.cpu().numpy(), ref))}
            use_form(eng, graphs, "nosplit")
            parity["nosplit"] = bool(np.array_equal(eng(x.to(dev)).cpu().numpy(), ref))
            forms = ("split", "nosplit")
            # warm-up outside the timed window, then size the blocks: ~20 blocks per form within --seconds
            for k in forms:
                use_form(eng, graphs, k)
                block_ms(eng, 20)
            est = block_ms(eng, 20)
            reps = max(5, int(args.seconds * 1e3 / 20 / est))
            times = {k: [] for k in forms}
            spent = 0.0
            while spent < args.seconds * 1e3 or len(times["split"]) < 10:
                for k in forms:   # interleaved A/B blocks
                    use_form(eng, graphs, k)
                    times[k].append(block_ms(eng, reps))
                spent += reps * min(times["split"][-1], times["nosplit"][-1])
            pt = {"arch": arch, "scheme": args.scheme, "batch": batch, "chains": int(plan["chains"]),
                  "split_launches": n_split, "splitk": plan.get("splitk", ""),
                  "ms_split": stats(times["split"]), "ms_nosplit": stats(times["nosplit"]), "replays_per_block": reps,
                  "speedup": round(float(np.median(times["nosplit"]) / np.median(times["split"])), 4),
                  "parity_split": parity["split"], "parity_nosplit": parity["nosplit"], "tune_s": round(tune_s, 1)}
            points.append(pt)
            print(json.dumps(pt), file=sys.stderr, flush=True)
            if args.profile_out and ai == 0 and batch in (args.batch[0], args.batch[-1]):
                for k in forms:
                    use_form(eng, graphs, k)
                    profiles[f"{arch}_b{batch}_{k}"] = [(n, round(ms, 5)) for n, ms in eng.profile_ops(20)
                                                        if n.startswith(("stage3", "stage4"))]
            use_form(eng, graphs, "split")
            from hawq_amd import _lib
            _lib.call("hawq_graph_destroy", graphs["nosplit"])   # (the engine destroys its own graph, the split form's)
            del eng
            torch.cuda.empty_cache()
    if args.profile_out:
        with open(args.profile_out, "w") as f:
            json.dump(profiles, f, indent=1)
    print(json.dumps({"tool": "latency_bench", "gpu": torch.cuda.get_device_name(0), "points": points}))


if __name__ == "__main__":
    main()
