"""Oracle logits and unit outputs of the InceptionV3 workload that tools/inception_bench.py times, at its own batch size.

    python tests/golden/make_b128_inception.py [scheme ...]      # writes tests/golden/b128_inceptionv3_<scheme>.npz

tools/inception_bench.py builds: synthetic weights (seed 0), ranges calibrated on synthetic_images(2, seed 0, 299), input
synthetic_images(128, seed 1, 299).  This script pushes exactly that workload through the CPU oracle (oracle/oracle_inception.py
over oracle/hawq_oracle.c - the restatement pinned to the live reference by tests/test_oracle_inception_vs_golden.py), which
calibrates itself on the same two images as one un-frozen forward does, in slices of 4 images, and stores all 128 x 1000 logits,
top-1, a SHA-256 of every unit's 16-bit output (after its q_rescaling_activ; NCHW, int16) per slice, the frozen ranges, and the
input hash, seeds and slice size.

Test infrastructure: consumed by tests/test_gpu_inception_oracle.py and tests/test_oracle_inception_vs_golden.py; hawq_amd/ never
reads it.
"""
from __future__ import annotations

import hashlib
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from hawq_amd.api import build_quantized_resnet  # noqa: E402
from hawq_amd.skeleton import synthetic_images  # noqa: E402
from oracle import oracle_inception  # noqa: E402

SCHEMES = ("uniform8", "uniform4")
BATCH, SLICE, CALIB, CALIB_SEED, SEED, SIZE = 128, 4, 2, 0, 1, 299


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def make(scheme):
    model = build_quantized_resnet("inceptionv3", scheme, seed=0)
    st = oracle_inception.extract_float_state(model)
    oracle_inception.forward_int(st, synthetic_images(CALIB, seed=CALIB_SEED, size=SIZE).numpy(), calibrate=True)
    x = synthetic_images(BATCH, seed=SEED, size=SIZE).numpy()
    names = oracle_inception.unit_names(st)
    logits, unit_sha, t0 = [], [], time.time()
    for b0 in range(0, BATCH, SLICE):
        y, tr = oracle_inception.forward_int(st, x[b0:b0 + SLICE])
        logits.append(y)
        outs = [oracle_inception.unit_output(tr, n) for n in names]
        assert all(np.abs(o).max() < 32768 for o in outs)
        unit_sha.append([sha(o.astype(np.int16)) for o in outs])
        print(f"inceptionv3 {scheme}: images {b0}..{b0 + SLICE - 1} done, {time.time() - t0:.0f} s so far", flush=True)
    logits = np.concatenate(logits).astype(np.float32)
    out = os.path.join(HERE, f"b128_inceptionv3_{scheme}.npz")
    np.savez_compressed(out, logits=logits, top1=logits.argmax(1).astype(np.int64), input_sha=np.array(sha(x)),
                        unit_names=np.array(names), unit_sha=np.array(unit_sha), slice=np.array(SLICE), calib=np.array(CALIB),
                        calib_seed=np.array(CALIB_SEED), seed=np.array(SEED),
                        act_names=np.array([n for n, _, _ in st["ranges"]]),
                        act_x_min=np.array([lo[0] for _, lo, _ in st["ranges"]], np.float32),
                        act_x_max=np.array([hi[0] for _, _, hi in st["ranges"]], np.float32))
    print(f"wrote {out}: {os.path.getsize(out)} bytes", flush=True)


if __name__ == "__main__":
    for s in (sys.argv[1:] or SCHEMES):
        make(s)
