"""InceptionV3 throughput: images per second of the integer network at batch 1 and batch 128 (299 x 299, synthetic weights,
ranges calibrated on 2 images), timed with HIP events around ``--steps`` forwards after ``--warmup``, for the fused integer plan
(hawq_amd/engine_inception.py, graph replay) and for the module-by-module path.  Prints one JSON line per batch size and path.
Per-launch breakdown: run it under ``rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/inception_bench.py ...``.

``--input f32,u8`` times the fused plan fed two ways instead: ``forward`` on normalised fp32 NCHW images and ``forward_uint8`` on the
same images as uint8 NHWC, in ``--blocks`` alternating blocks of ``--steps`` forwards in one process (as bench.py --full does for
the ResNet uint8 entry), and checks that the two give the same logits.  ``--stem-launches K`` then issues the fp32 plan's three stem
launches and ``hawq_incep_stem_u8`` K times each, eagerly, for a kernel trace of just those.

    python tools/inception_bench.py [--scheme uniform8] [--steps 5] [--warmup 2] [--paths fused,module]
    python tools/inception_bench.py --input f32,u8 [--blocks 6] [--stem-launches 0]
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
            stem32, stem8 = eng._ops[:eng._n_stem_ops], eng._ops_u8[:1]
            with torch.cuda.stream(eng.stream):
                for name, ops in (("f32_stem_launches", stem32), ("hawq_incep_stem_u8", stem8)):
                    def run(ops=ops):
                        for op in ops:
                            op()
                    run()
                    t = _timed(run, args.stem_launches)
                    print(json.dumps({"workload": f"inceptionv3_{args.scheme}_b{b}", "stem": name, "launches": len(ops),
                                      "ms_per_stem": round(t / args.stem_launches, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scheme", default="uniform8")
    ap.add_argument("--batches", default="1,128")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--paths", default="fused,module")
    ap.add_argument("--input", default=None, help="f32,u8 (or one of them): compare the fused plan's two inputs instead of --paths")
    ap.add_argument("--blocks", type=int, default=6, help="--input: alternating blocks of --steps forwards per kind")
    ap.add_argument("--stem-launches", type=int, default=0, help="--input: then issue each stem form K times (for a kernel trace)")
    args = ap.parse_args()
    model = build_quantized_resnet("inceptionv3", args.scheme, seed=0).cuda()
    calibrate(model, synthetic_images(2, seed=0, size=299).cuda())
    for b in (int(v) for v in args.batches.split(",")):
        if args.input:
            compare_inputs(model, args, b, args.input.split(","))
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
