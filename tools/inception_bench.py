"""InceptionV3 throughput: images per second of the integer network at batch 1 and batch 128 (299 x 299, synthetic weights,
ranges calibrated on 2 images), timed with HIP events around ``--steps`` forwards after ``--warmup``, for the fused integer plan
(hawq_amd/engine_inception.py, graph replay) and for the module-by-module path.  Prints one JSON line per batch size and path.
Per-launch breakdown: run it under ``rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/inception_bench.py ...``.

    python tools/inception_bench.py [--scheme uniform8] [--steps 5] [--warmup 2] [--paths fused,module]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hawq_amd.api import build_quantized_resnet, calibrate  # noqa: E402
from hawq_amd.skeleton import synthetic_images  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scheme", default="uniform8")
    ap.add_argument("--batches", default="1,128")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--paths", default="fused,module")
    args = ap.parse_args()
    model = build_quantized_resnet("inceptionv3", args.scheme, seed=0).cuda()
    calibrate(model, synthetic_images(2, seed=0, size=299).cuda())
    for b in (int(v) for v in args.batches.split(",")):
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
