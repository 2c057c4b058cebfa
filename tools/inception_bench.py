"""InceptionV3 throughput: images per second of the integer network at batch 1 and batch 128 (299 x 299, synthetic weights,
ranges calibrated on 2 images), timed with HIP events around ``--steps`` forwards after ``--warmup``, for the fused integer plan
(hawq_amd/engine_inception.py, graph replay) and for the module-by-module path.  Prints one JSON line per batch size and path.
Per-launch breakdown: run it under ``rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/inception_bench.py ...``.

``--input f32,u8`` times the fused plan fed two ways instead: ``forward`` on normalised fp32 NCHW images and ``forward_uint8`` on the
same images as uint8 NHWC, in ``--blocks`` alternating blocks of ``--steps`` forwards in one process (as bench.py --full does for
the ResNet uint8 entry), and checks that the two give the same logits.  ``--stem-launches K`` then issues the fp32 plan's three stem
launches and ``hawq_incep_stem_u8`` K times each, eagerly, for a kernel trace of just those.

``--tune`` (or ``--plan FILE``) compares the fixed plan (every conv on ``hawq_incep_conv``) with the tuned plan (per-launch conv tiles
of ``hawq_incep_conv_tiled``, timed by the engine or replayed from FILE) of the same calibrated model: ``--blocks`` alternating blocks of
``--steps`` forwards per plan in one process, mean and spread of the blocks per plan, and an assertion that the two plans' logits are
bit-equal.  With ``--tune`` it prints the per-launch table (geometry, microseconds of tile 0, chosen tile, its microseconds) and the
sums over the conv launches; ``--save-plan FILE`` writes the last batch size's plan (``export_plan()``) as JSON.

``--pools`` (alone, or with ``--tune`` / ``--plan FILE``, whose conv tiles both engines then share) compares the plan on the four pool
entry points of inception.hip with the same plan on ``hawq_incep_pool_v`` (``fast_pools=True``): alternating blocks as above, an
assertion that the logits are bit-equal, and a table of the 49 pool / requant launches - each timed alone on the plan's own buffers
(HIP events, 2 untimed + 5 timed launches, the median) with the old and the new kernel, the bytes it has to move (input read once +
output written once, from the shapes) and that byte count over 6.29 TB/s.  ``--skip-pool-table`` leaves the table out (kernel traces).

``--fused-stem`` (alone, or with ``--tune`` / ``--plan FILE`` and / or ``--pools``, which then apply to both engines: the fused-stem
engine replays the other's conv tiles) compares the default fp32 plan with the same plan under ``fused_stem=True`` (one
``hawq_incep_stem_f32`` instead of the input QuantAct's two launches + conv1): alternating blocks as above and an assertion that the
logits are bit-equal.  ``--stem-launches K`` then times, eagerly on the plan's own buffers, the three launches one by one, the three
together and the one launch, K launches each in two alternating rounds, with the one launch's byte floor (fp32 in + int8 out over
6.29 TB/s).

``--grouped`` compares, on one tuned conv tile plan with ``fast_pools=True, fused_stem=True``, the plan without and with grouped conv
launches (``grouped=True``, tuned: the grouped engine times tiles and groups, the other engine replays its tile plan and ignores the
groups): alternating blocks as above, an assertion that the logits are bit-equal, the launch counts, and a table of the candidate
groups - member conv launches, fastest tile, its microseconds, the sum of the members' best single microseconds, kept or not.

``--fan-out`` (alone or with ``--grouped``) compares, on one recorded plan with ``fast_pools=True, fused_stem=True``, the plan without
and with fan-out conv epilogues (``fan_out=True``, tuned: that engine times tiles, groups and boundaries, the other replays its plan
and ignores the ``"fan_out"`` field, so every conv that is no fan-out producer runs on the same tile in both; a third engine replays
the plan without the field and so takes every candidate boundary on the default tiles): alternating blocks as above, an assertion that
the logits are bit-equal, the launch counts, and a table of the boundaries - producer launches + entry requants against fan-out
producer launches + residual requants, in microseconds, kept or not.

    python tools/inception_bench.py [--scheme uniform8] [--steps 5] [--warmup 2] [--paths fused,module]
    python tools/inception_bench.py --input f32,u8 [--blocks 6] [--stem-launches 0]
    python tools/inception_bench.py --tune [--batches 128] [--blocks 6] [--save-plan plan.json]
    python tools/inception_bench.py --plan plan.json --batches 128
    python tools/inception_bench.py --tune --pools --batches 128,1
    python tools/inception_bench.py --fused-stem [--tune --pools] --batches 128,1 --stem-launches 20
    python tools/inception_bench.py --grouped --batches 1,16,128 [--blocks 6]
    python tools/inception_bench.py --fan-out [--grouped] --batches 1,16,128 [--blocks 6]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hawq_amd.api import build_quantized_resnet, calibrate  # noqa: E402
from hawq_amd.skeleton import synthetic_images  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _timed(fn, steps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def compare_inputs(model, args, b, kinds):
    """fp32 ``forward`` against ``forward_uint8`` of one plan, alternating blocks; one JSON line per input kind"""
    eng = model.engine()
    u8 = torch.randint(0, 256, (b, 299, 299, 3), generator=torch.Generator().manual_seed(b), dtype=torch.uint8)
    x = u8.permute(0, 3, 1, 2).to(torch.float32).div(255)
    x = x.sub(torch.tensor(MEAN).view(1, 3, 1, 1)).div(torch.tensor(STD).view(1, 3, 1, 1)).cuda()
    u8 = u8.cuda()
    fns = {"f32": lambda: eng(x), "u8": lambda: eng.forward_uint8(u8, MEAN, STD)}
    with torch.no_grad():
        equal = bool(torch.equal(fns["f32"](), fns["u8"]()))
        for k in kinds:
            for _ in range(args.warmup):
                fns[k]()
        ms = {k: 0.0 for k in kinds}
        for _ in range(args.blocks):
            for k in kinds:
                ms[k] += _timed(fns[k], args.steps)
        for k in kinds:
            per = ms[k] / (args.blocks * args.steps)
            print(json.dumps({"workload": f"inceptionv3_{args.scheme}_b{b}", "path": "fused", "input": k,
                              "ms_per_batch": round(per, 3), "images_per_s": round(b * 1000.0 / per, 1),
                              "launches": eng.n_launches_u8 if k == "u8" else eng.n_launches,
                              "input_bytes": u8.numel() if k == "u8" else x.numel() * 4,
                              "logits_bit_equal": equal}), flush=True)
        if len(kinds) == 2:
            print(json.dumps({"workload": f"inceptionv3_{args.scheme}_b{b}", "u8_over_f32_rate": round(ms["f32"] / ms["u8"], 4)}),
                  flush=True)
        if args.stem_launches:
            # the launches hawq_incep_stem_u8 replaces, and it, eagerly on the plan stream (HIP events around each group of K)
            stem32, stem8 = eng._ops[:eng._at[eng._convs[0]] + 1], eng._ops_u8[:1]   # up to conv1
            with torch.cuda.stream(eng.stream):
                for name, ops in (("f32_stem_launches", stem32), ("hawq_incep_stem_u8", stem8)):
                    def run(ops=ops):
                        for op in ops:
                            op()
                    run()
                    t = _timed(run, args.stem_launches)
                    print(json.dumps({"workload": f"inceptionv3_{args.scheme}_b{b}", "stem": name, "launches": len(ops),
                                      "ms_per_stem": round(t / args.stem_launches, 4)}), flush=True)


def compare_plans(model, args, b):
    """the fixed plan against the tuned (or replayed) plan of one model, alternating blocks; returns the tuned engine"""
    from hawq_amd.engine_inception import InceptionEngine
    x = synthetic_images(b, seed=1, size=299).cuda()
    plan = json.load(open(args.plan)) if args.plan else None
    engines = {"fixed": InceptionEngine(model), "tuned": InceptionEngine(model, tune=plan is None, plan=plan)}
    wl = f"inceptionv3_{args.scheme}_b{b}"
    with torch.no_grad():
        y = {k: e(x) for k, e in engines.items()}
        equal = bool(torch.equal(y["fixed"], y["tuned"]))
        assert equal, "the tuned plan's logits differ from the fixed plan's"
        tuned = engines["tuned"]
        if plan is None:
            keys = ("H", "W", "Cin", "Cout", "KH", "KW", "stride", "pad_h", "pad_w", "epilogue", "out_bits", "ldo", "c_off")
            print(f"# {wl}: conv launch | " + " ".join(keys) + " | tile 0 us | chosen tile | its us | all tiles us")
            for i, (key, t, us) in enumerate(zip(tuned.conv_launches, tuned.conv_tiles, tuned.conv_us)):
                print(f"# {i:2d} | " + " ".join(str(v) for v in key) + f" | {us[0]:.1f} | {t} | {us[t]:.1f} | " +
                      " ".join(f"{k}:{v:.1f}" for k, v in sorted(us.items())))
            s0, s1 = sum(us[0] for us in tuned.conv_us), sum(us[t] for t, us in zip(tuned.conv_tiles, tuned.conv_us))
            print(json.dumps({"workload": wl, "conv_launches": len(tuned.conv_tiles), "conv_us_tile0_sum": round(s0, 1),
                              "conv_us_chosen_sum": round(s1, 1), "timing_launches": tuned.n_timing_launches,
                              "launches_per_tile": {str(t): tuned.conv_tiles.count(t) for t in sorted(set(tuned.conv_tiles))}}),
                  flush=True)
        for e in engines.values():
            for _ in range(args.warmup):
                e(x)
        ms = {k: [] for k in engines}
        for _ in range(args.blocks):
            for k, e in engines.items():
                ms[k].append(_timed(lambda e=e: e(x), args.steps) / args.steps)
        for k, e in engines.items():
            v = ms[k]
            mean = sum(v) / len(v)
            print(json.dumps({"workload": wl, "path": "fused", "plan": k, "ms_per_batch": round(mean, 4),
                              "images_per_s": round(b * 1000.0 / mean, 1), "block_min_ms": round(min(v), 4),
                              "block_max_ms": round(max(v), 4), "blocks": len(v), "steps": args.steps, "launches": e.n_launches,
                              "logits_bit_equal": equal}), flush=True)
        mf, mt = sum(ms["fixed"]) / args.blocks, sum(ms["tuned"]) / args.blocks
        print(json.dumps({"workload": wl, "tuned_over_fixed_rate": round(mf / mt, 4),
                          "fixed_block_spread_ms": round(max(ms["fixed"]) - min(ms["fixed"]), 4),
                          "gain_ms": round(mf - mt, 4)}), flush=True)
    return tuned


STREAM_TBS = 6.29   # what the MI355X streams (profiles/inception.md): the floor of a launch is its bytes over this
POOL_NAMES = ("hawq_incep_requant", "hawq_incep_maxpool3s2", "hawq_incep_avgpool_branch", "hawq_incep_global_avgpool")


def pool_bytes(a, op):
    """bytes a pool launch has to move: its input slice read once and its output slice written once"""
    ho, wo = {0: (a.H, a.W), 1: ((a.H - 3) // 2 + 1, (a.W - 3) // 2 + 1), 2: (a.H, a.W), 3: (1, 1)}[op]
    return a.N * a.C * (a.H * a.W * a.in_bits + ho * wo * a.out_bits) // 8


def pool_blocks(eng):
    """(argument block, op id of hawq_incep_pool_v) of every pool / requant launch of `eng`, in the default plan's order"""
    return [(r.args[0], r.ref) for r in eng._launches if r.kind == "pool"]


def time_pools(eng, reps=5, warmup=2):
    """[(old us, new us or None)] per pool launch of `eng`, each launch alone on the plan's buffers, which hold a forward (every
    pool launch is a pure function of its input buffer, so repeating it changes nothing)"""
    import ctypes as C
    from hawq_amd import _lib
    from hawq_amd.runner import EventTimer
    sp, out = eng.stream.cuda_stream, []
    old_of = {v: k for k, v in _lib.INCEP_POOL_OPS.items()}
    with EventTimer(sp, reps + 1) as ev:
        torch.cuda.synchronize()
        with torch.cuda.stream(eng.stream):
            for a, op in pool_blocks(eng):
                row = []
                for new in (False, True):
                    if new and not _lib.load().hawq_incep_pool_v_ok(C.byref(a), op):
                        row.append(None)
                        continue
                    launch = (lambda: _lib.call("hawq_incep_pool_v", C.byref(a), op, sp)) if new else \
                        (lambda: _lib.call(old_of[op], C.byref(a), sp))
                    row.append(ev.median_us(launch, reps, warmup))
                out.append(tuple(row))
    torch.cuda.synchronize()
    return out


def compare_pools(model, args, b):
    """one plan on the old pool kernels against the same plan with fast_pools=True, alternating blocks; returns the fast engine"""
    from hawq_amd.engine_inception import InceptionEngine
    x = synthetic_images(b, seed=1, size=299).cuda()
    plan = json.load(open(args.plan)) if args.plan else None
    wl = f"inceptionv3_{args.scheme}_b{b}"
    with torch.no_grad():
        old = InceptionEngine(model, tune=args.tune and plan is None, plan=plan)
        y_old = old(x)
        if old.conv_tiles is not None:
            plan = old.export_plan()   # the fast engine replays the same conv tiles: only the pool kernels differ
        fast = InceptionEngine(model, plan=plan, fast_pools=True)
        engines = {"old_pools": old, "fast_pools": fast}
        equal = bool(torch.equal(y_old, fast(x)))
        assert equal, "the logits with fast_pools differ from the old pool kernels'"
        assert old.conv_tiles == fast.conv_tiles and old.n_launches == fast.n_launches
        if not args.skip_pool_table:
            us = time_pools(fast)
            print(f"# {wl}: pool launch | entry point | H W C in_bits out_bits ldo c_off | old us | new us | bytes | floor us (bytes / "
                  f"{STREAM_TBS} TB/s) | issued as")
            for i, ((a, op), (name, _), (t0, t1)) in enumerate(zip(pool_blocks(fast), fast.pool_launches, us)):
                nb = pool_bytes(a, op)
                print(f"# {i:2d} | {POOL_NAMES[op]} | {a.H} {a.W} {a.C} {a.in_bits} {a.out_bits} {a.ldo} {a.c_off} | {t0:.1f} | " +
                      ("refused" if t1 is None else f"{t1:.1f}") + f" | {nb} | {nb / (STREAM_TBS * 1e6):.1f} | {name}")
            s0 = sum(t0 for t0, _ in us)
            s1 = sum(t0 if t1 is None else t1 for t0, t1 in us)
            print(json.dumps({"workload": wl, "pool_launches": len(us), "pool_us_old_sum": round(s0, 1), "pool_us_new_sum": round(s1, 1),
                              "pool_floor_us_sum": round(sum(pool_bytes(a, op) for a, op in pool_blocks(fast)) / (STREAM_TBS * 1e6), 1),
                              "taken_by_pool_v": sum(n == "hawq_incep_pool_v" for n, _ in fast.pool_launches),
                              "slower_launches": [i for i, (t0, t1) in enumerate(us) if t1 is not None and t1 > t0]}), flush=True)
        for e in engines.values():
            for _ in range(args.warmup):
                e(x)
        ms = {k: [] for k in engines}
        for _ in range(args.blocks):
            for k, e in engines.items():
                ms[k].append(_timed(lambda e=e: e(x), args.steps) / args.steps)
        for k, e in engines.items():
            v = ms[k]
            mean = sum(v) / len(v)
            print(json.dumps({"workload": wl, "path": "fused", "plan": "tuned" if e.conv_tiles is not None else "fixed", "pools": k,
                              "ms_per_batch": round(mean, 4), "images_per_s": round(b * 1000.0 / mean, 1),
                              "block_min_ms": round(min(v), 4), "block_max_ms": round(max(v), 4), "blocks": len(v),
                              "steps": args.steps, "launches": e.n_launches, "logits_bit_equal": equal}), flush=True)
        mo, mf = sum(ms["old_pools"]) / args.blocks, sum(ms["fast_pools"]) / args.blocks
        print(json.dumps({"workload": wl, "fast_over_old_rate": round(mo / mf, 4), "gain_ms": round(mo - mf, 4),
                          "old_block_spread_ms": round(max(ms["old_pools"]) - min(ms["old_pools"]), 4),
                          "fast_block_spread_ms": round(max(ms["fast_pools"]) - min(ms["fast_pools"]), 4)}), flush=True)
    return fast


def compare_stems(model, args, b):
    """the default fp32 plan against the same plan with fused_stem=True, alternating blocks; returns the fused-stem engine"""
    from hawq_amd.engine_inception import InceptionEngine
    x = synthetic_images(b, seed=1, size=299).cuda()
    plan = json.load(open(args.plan)) if args.plan else None
    wl = f"inceptionv3_{args.scheme}_b{b}"
    with torch.no_grad():
        base = InceptionEngine(model, tune=args.tune and plan is None, plan=plan, fast_pools=args.pools)
        y0 = base(x)
        if base.conv_tiles is not None:
            plan = base.export_plan()   # the fused-stem engine replays the same conv tiles: only the stem differs
        fused = InceptionEngine(model, plan=plan, fast_pools=args.pools, fused_stem=True)
        engines = {"three_launch_stem": base, "fused_stem": fused}
        equal = bool(torch.equal(y0, fused(x)))
        assert equal, "the logits with fused_stem differ from the default plan's"
        assert base.conv_launches == fused.conv_launches and fused.n_launches == base.n_launches - 2
        assert fused.op_names[0] == "hawq_incep_stem_f32"
        for e in engines.values():
            for _ in range(args.warmup):
                e(x)
        ms = {k: [] for k in engines}
        for _ in range(args.blocks):
            for k, e in engines.items():
                ms[k].append(_timed(lambda e=e: e(x), args.steps) / args.steps)
        for k, e in engines.items():
            v = ms[k]
            mean = sum(v) / len(v)
            print(json.dumps({"workload": wl, "path": "fused", "plan": "tuned" if e.conv_tiles is not None else "fixed",
                              "fast_pools": e.fast_pools, "stem": k, "ms_per_batch": round(mean, 4),
                              "images_per_s": round(b * 1000.0 / mean, 1), "block_min_ms": round(min(v), 4),
                              "block_max_ms": round(max(v), 4), "blocks": len(v), "steps": args.steps, "launches": e.n_launches,
                              "logits_bit_equal": equal}), flush=True)
        m0, m1 = sum(ms["three_launch_stem"]) / args.blocks, sum(ms["fused_stem"]) / args.blocks
        print(json.dumps({"workload": wl, "fused_over_default_rate": round(m0 / m1, 4), "gain_ms": round(m0 - m1, 4),
                          "default_block_spread_ms": round(max(ms["three_launch_stem"]) - min(ms["three_launch_stem"]), 4),
                          "fused_block_spread_ms": round(max(ms["fused_stem"]) - min(ms["fused_stem"]), 4)}), flush=True)
        if args.stem_launches:
            a1 = base._convs[0].args[0]
            ho, wo = (a1.H - 3) // 2 + 1, (a1.W - 3) // 2 + 1
            floor_us = (b * 3 * a1.H * a1.W * 4 + b * ho * wo * a1.Cout) / (STREAM_TBS * 1e6)
            three = base._ops[:base._at[base._convs[0]] + 1]   # up to conv1
            # (name, launches, the engine on whose stream they are issued)
            groups = [(op.args[0], [op], base) for op in three] + [("three_launches", three, base),
                                                                   ("hawq_incep_stem_f32", fused._ops[:1], fused)]
            us = {name: [] for name, _, _ in groups}
            torch.cuda.synchronize()
            for _ in range(2):
                for name, ops, eng in groups:
                    def run(ops=ops):
                        for op in ops:
                            op()
                    with torch.cuda.stream(eng.stream):
                        run()
                        us[name].append(_timed(run, args.stem_launches) * 1000.0 / args.stem_launches)
            for name, ops, _ in groups:
                print(json.dumps({"workload": wl, "stem": name, "launches": len(ops), "us_per_call_rounds": [round(v, 2) for v in us[name]],
                                  "us_per_call": round(min(us[name]), 2)}), flush=True)
            t3, t1 = min(us["three_launches"]), min(us["hawq_incep_stem_f32"])
            print(json.dumps({"workload": wl, "stem_f32_us": round(t1, 2), "three_launches_us": round(t3, 2),
                              "three_over_one": round(t3 / t1, 3), "byte_floor_us": round(floor_us, 2),
                              "stem_f32_over_floor": round(t1 / floor_us, 2)}), flush=True)
    return fused


def compare_grouped(model, args, b):
    """one tuned tile plan (fast pools, fused stem) without and with grouped conv launches, alternating blocks; returns the grouped
    engine"""
    from hawq_amd.engine_inception import InceptionEngine
    x = synthetic_images(b, seed=1, size=299).cuda()
    wl = f"inceptionv3_{args.scheme}_b{b}"
    with torch.no_grad():
        grouped = InceptionEngine(model, tune=True, fast_pools=True, fused_stem=True, grouped=True)
        y1 = grouped(x)
        single = InceptionEngine(model, plan=grouped.export_plan(), fast_pools=True, fused_stem=True)   # the same tiles, no groups
        engines = {"single": single, "grouped": grouped}
        equal = bool(torch.equal(single(x), y1))
        assert equal, "the logits with grouped launches differ from the single launches'"
        assert single.conv_tiles == grouped.conv_tiles and not single.group_launches
        print(f"# {wl}: group | member conv launches (Cout KHxKW each) | fastest tile | group us | sum of members' best single us | kept")
        for i, g in enumerate(grouped.group_candidates):
            keys = [grouped.conv_launches[c] for c in g["convs"]]
            print(f"# {i:2d} | " + " ".join(f"{c}({k[3]} {k[4]}x{k[5]})" for c, k in zip(g["convs"], keys)) +
                  f" | {g['tile']} | {g['us'][str(g['tile'])]:.1f} | {g['us']['singles']:.1f} | {'kept' if g['kept'] else 'singles'}")
        kept = [g for g in grouped.group_candidates if g["kept"]]
        print(json.dumps({"workload": wl, "launches_single": single.n_launches, "launches_grouped": grouped.n_launches,
                          "conv_launches_single": len(single.conv_launches) - 1,
                          "conv_launches_grouped": len(grouped.conv_launches) - 1 - sum(len(g["convs"]) - 1 for g in kept),
                          "groups_kept": len(kept), "groups_rejected": len(grouped.group_candidates) - len(kept),
                          "kept_group_us_sum": round(sum(g["us"][str(g["tile"])] for g in kept), 1),
                          "kept_members_single_us_sum": round(sum(g["us"]["singles"] for g in kept), 1),
                          "tiles_of_kept_groups": {str(t): [g["tile"] for g in kept].count(t) for t in sorted({g["tile"] for g in kept})}}),
              flush=True)
        for e in engines.values():
            for _ in range(args.warmup):
                e(x)
        ms = {k: [] for k in engines}
        for _ in range(args.blocks):
            for k, e in engines.items():
                ms[k].append(_timed(lambda e=e: e(x), args.steps) / args.steps)
        for k, e in engines.items():
            v = ms[k]
            mean = sum(v) / len(v)
            print(json.dumps({"workload": wl, "path": "fused", "plan": "tuned", "fast_pools": True, "fused_stem": True, "convs": k,
                              "ms_per_batch": round(mean, 4), "images_per_s": round(b * 1000.0 / mean, 1),
                              "block_min_ms": round(min(v), 4), "block_max_ms": round(max(v), 4), "blocks": len(v),
                              "steps": args.steps, "launches": e.n_launches, "logits_bit_equal": equal}), flush=True)
        m0, m1 = sum(ms["single"]) / args.blocks, sum(ms["grouped"]) / args.blocks
        print(json.dumps({"workload": wl, "grouped_over_single_rate": round(m0 / m1, 4), "gain_ms": round(m0 - m1, 4),
                          "single_block_spread_ms": round(max(ms["single"]) - min(ms["single"]), 4),
                          "grouped_block_spread_ms": round(max(ms["grouped"]) - min(ms["grouped"]), 4)}), flush=True)
    return grouped


def compare_fan_out(model, args, b):
    """one recorded plan (fast pools, fused stem, grouped or not) without fan-out, with the boundaries the tuner kept and with every
    candidate boundary, alternating blocks; returns the tuned fan-out engine"""
    from hawq_amd.engine_inception import InceptionEngine
    x = synthetic_images(b, seed=1, size=299).cuda()
    wl = f"inceptionv3_{args.scheme}_b{b}"
    opts = dict(fast_pools=True, fused_stem=True, grouped=args.grouped)
    with torch.no_grad():
        fan = InceptionEngine(model, tune=True, fan_out=True, **opts)
        y1 = fan(x)
        plan = fan.export_plan()
        plain = InceptionEngine(model, plan=plan, **opts)   # the same tiles and groups; the field is ignored
        every = InceptionEngine(model, plan={k: v for k, v in plan.items() if k != "fan_out"}, fan_out=True, **opts)
        engines = {"plain": plain, "fan_out": fan, "fan_out_all": every}
        equal = bool(torch.equal(plain(x), y1)) and bool(torch.equal(every(x), y1))
        assert equal, "the logits with fan-out epilogues differ from the plain plan's"
        # (a grouped launch that carries a fan runs on the fan's tile, so only the members are compared)
        assert plain.conv_tiles == fan.conv_tiles and not plain.fan_launches
        assert [c for c, _ in plain.group_launches] == [c for c, _ in fan.group_launches]
        print(f"# {wl}: consumer unit | producer launches (member conv launches @ tile) | producers + entry requants us | "
              f"fan-out producers + residual requants us | kept")
        for f in fan.fan_candidates:
            print(f"# {f['unit']:2d} | " + " ".join(f"[{k}]@{t}" for k, t in f["tiles"].items()) +
                  f" | {f['us']['plain']:.1f} | {f['us']['fan']:.1f} | {'kept' if f['kept'] else 'plain'}")
        kept = [f for f in fan.fan_candidates if f["kept"]]
        print(json.dumps({"workload": wl, "grouped": bool(args.grouped), "launches_plain": plain.n_launches,
                          "launches_fan_out": fan.n_launches, "launches_fan_out_all": every.n_launches,
                          "boundaries_kept": [f["unit"] for f in kept],
                          "boundaries_rejected": [f["unit"] for f in fan.fan_candidates if not f["kept"]],
                          "plain_us_sum": round(sum(f["us"]["plain"] for f in fan.fan_candidates), 1),
                          "fan_us_sum": round(sum(f["us"]["fan"] for f in fan.fan_candidates), 1),
                          "kept_plain_us_sum": round(sum(f["us"]["plain"] for f in kept), 1),
                          "kept_fan_us_sum": round(sum(f["us"]["fan"] for f in kept), 1)}), flush=True)
        for e in engines.values():
            for _ in range(args.warmup):
                e(x)
        ms = {k: [] for k in engines}
        for _ in range(args.blocks):
            for k, e in engines.items():
                ms[k].append(_timed(lambda e=e: e(x), args.steps) / args.steps)
        for k, e in engines.items():
            v = ms[k]
            mean = sum(v) / len(v)
            print(json.dumps({"workload": wl, "path": "fused", "plan": "tuned", "fast_pools": True, "fused_stem": True,
                              "grouped": bool(args.grouped), "epilogues": k, "ms_per_batch": round(mean, 4),
                              "images_per_s": round(b * 1000.0 / mean, 1), "block_min_ms": round(min(v), 4),
                              "block_max_ms": round(max(v), 4), "blocks": len(v), "steps": args.steps, "launches": e.n_launches,
                              "logits_bit_equal": equal}), flush=True)
        m0 = sum(ms["plain"]) / args.blocks
        print(json.dumps({"workload": wl, "grouped": bool(args.grouped),
                          "gain_ms_fan_out": round(m0 - sum(ms["fan_out"]) / args.blocks, 4),
                          "gain_ms_fan_out_all": round(m0 - sum(ms["fan_out_all"]) / args.blocks, 4),
                          "plain_block_spread_ms": round(max(ms["plain"]) - min(ms["plain"]), 4)}), flush=True)
    return fan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scheme", default="uniform8")
    ap.add_argument("--batches", default="1,128")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--paths", default="fused,module")
    ap.add_argument("--input", default=None, help="f32,u8 (or one of them): compare the fused plan's two inputs instead of --paths")
    ap.add_argument("--blocks", type=int, default=6, help="--input: alternating blocks of --steps forwards per kind")
    ap.add_argument("--stem-launches", type=int, default=0,
                    help="--input: then issue each stem form K times (for a kernel trace); --fused-stem: time the stem launches, K each")
    ap.add_argument("--tune", action="store_true", help="compare the fixed plan with the plan on tuned conv tiles")
    ap.add_argument("--plan", default=None, help="like --tune, but replay the conv tile plan of this JSON file instead of timing")
    ap.add_argument("--pools", action="store_true", help="compare the old pool kernels with fast_pools=True on one plan")
    ap.add_argument("--skip-pool-table", action="store_true", help="--pools: do not time the 49 pool launches one by one")
    ap.add_argument("--fused-stem", action="store_true", help="compare the default fp32 plan with fused_stem=True on one plan")
    ap.add_argument("--grouped", action="store_true",
                    help="compare one tuned plan (fast pools, fused stem) without and with grouped conv launches")
    ap.add_argument("--fan-out", action="store_true",
                    help="compare one recorded plan (fast pools, fused stem; grouped with --grouped) without and with fan-out conv epilogues")
    ap.add_argument("--save-plan", default=None, help="--tune / --plan / --grouped / --fan-out: write export_plan() of the last batch size to this file")
    args = ap.parse_args()
    if args.save_plan and not (args.tune or args.plan or args.grouped or args.fan_out):
        ap.error("--save-plan needs --tune, --plan, --grouped or --fan-out: there is no conv tile plan to save otherwise")
    model = build_quantized_resnet("inceptionv3", args.scheme, seed=0).cuda()
    calibrate(model, synthetic_images(2, seed=0, size=299).cuda())
    for b in (int(v) for v in args.batches.split(",")):
        if args.input:
            compare_inputs(model, args, b, args.input.split(","))
            continue
        if args.fan_out or args.grouped or args.tune or args.plan or args.pools or args.fused_stem:
            compare = compare_fan_out if args.fan_out else compare_grouped if args.grouped else compare_stems if args.fused_stem else compare_pools if args.pools else compare_plans
            tuned = compare(model, args, b)
            if args.save_plan:
                with open(args.save_plan, "w") as f:
                    json.dump(tuned.export_plan(), f)
            continue
        x = synthetic_images(b, seed=1, size=299).cuda()
        for path in args.paths.split(","):
            fwd = model if path == "fused" else model.forward_modules
            with torch.no_grad():
                for _ in range(args.warmup):
                    fwd(x)
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(args.steps):
                    fwd(x)
                stop.record()
                torch.cuda.synchronize()
            ms = start.elapsed_time(stop) / args.steps
            print(json.dumps({"workload": f"inceptionv3_{args.scheme}_b{b}", "path": path, "ms_per_batch": round(ms, 3),
                              "images_per_s": round(b * 1000.0 / ms, 1),
                              "launches": model.engine().n_launches if path == "fused" else None}), flush=True)

if __name__ == "__main__":
    main()
