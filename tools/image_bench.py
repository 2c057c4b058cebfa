"""Front end of ``forward_uint8``: time of Resize + CenterCrop for one batch of decoded images, per-image path against the one-launch path.

For both geometries of ``hawq_amd.image.eval_geometry`` ((256, 224) and InceptionV3's (342, 299)) it times, on one batch of
``--batch`` synthetic 375 x 500 images,
  * ``preprocess_batch``        - one host-to-device copy, up to two ``hawq_resample_u8`` launches and two allocations per image, then a stack,
  * ``preprocess_batch_fused``  - one copy of the packed images, one copy of the tables, one ``hawq_image_batch`` launch,
each with the images on the host (pageable tensors, as the decoder leaves them) and with the images already on the device; and, at
(256, 224), a mixed-size batch: the nine geometries of tests/golden/pillow_resize.npz repeated to ``--batch`` images.

Every figure is taken ``--repeats`` times after ``--warmup`` untimed calls, the two paths alternating within each repeat (the machine is
shared: a drift hits both alike).  Per call: HIP-event time (events on the stream around the call) and host wall time (clock around the
call and a device synchronise).  Reported: the median and the range.  Before timing, the two paths' outputs are compared byte for byte.
Writes the table to ``--out`` (markdown) and prints one JSON line per case.

    python tools/image_bench.py [--batch 128] [--repeats 20] [--warmup 3] [--out profiles/image_batch.md] [--box NAME]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hawq_amd import image  # noqa: E402

FIXTURE_GEOMS = [(375, 500), (500, 333), (90, 120), (256, 300), (300, 256), (224, 224), (1000, 1500), (257, 259), (37, 1024)]


def _batch(sizes, seed=0):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in sizes]


def _one(fn):
    """(HIP-event ms, host wall ms) of one call"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop), (time.perf_counter() - t0) * 1e3


def measure(paths, warmup, repeats):
    """paths: {name: callable}; -> {name: {"event_ms": [...], "wall_ms": [...]}} with the paths alternating within each repeat"""
    for _ in range(warmup):
        for fn in paths.values():
            fn()
    torch.cuda.synchronize()
    times = {name: {"event_ms": [], "wall_ms": []} for name in paths}
    for r in range(repeats):
        order = list(paths) if r % 2 == 0 else list(paths)[::-1]
        for name in order:
            ev, wall = _one(paths[name])
            times[name]["event_ms"].append(ev)
            times[name]["wall_ms"].append(wall)
    return times


def _stat(v):
    return statistics.median(v), min(v), max(v)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "image_batch.md"))
    ap.add_argument("--box", default=None, help="label of the machine for the report (default: the device name and architecture)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("image_bench: needs the GPU (a CPU run says nothing about these times)")
    props = torch.cuda.get_device_properties(0)
    box = args.box or f"{props.name} ({getattr(props, 'gcnArchName', '?')})"
    cases = [("375x500", [(375, 500)] * args.batch, geom) for geom in ((256, 224), (342, 299))]
    cases.append(("mixed (nine fixture sizes)", [FIXTURE_GEOMS[i % len(FIXTURE_GEOMS)] for i in range(args.batch)], (256, 224)))
    rows = []
    for label, sizes, (resize, crop) in cases:
        host = _batch(sizes)
        dev = [t.cuda() for t in host]
        plan = image.plan_batch(sizes, resize, crop)
        in_bytes, out_bytes = sum(h * w * 3 for h, w in sizes), len(sizes) * crop * crop * 3
        for place, imgs in (("device", dev), ("host", host)):
            old = lambda imgs=imgs: image.preprocess_batch(imgs, resize, crop)
            new = lambda imgs=imgs: image.preprocess_batch_fused(imgs, resize, crop)
            if not torch.equal(old(), new()):
                sys.exit(f"image_bench: the two paths differ at {label} {resize}/{crop} ({place} images)")
            t = measure({"per_image": old, "fused": new}, args.warmup, args.repeats)
            row = {"images": label, "n": len(sizes), "resize": resize, "crop": crop, "placement": place, "tiles": len(plan.tiles),
                   "lds_bytes": plan.lds_bytes, "fallback": len(plan.fallback), "input_mb": in_bytes / 1e6, "output_mb": out_bytes / 1e6}
            for name in ("per_image", "fused"):
                for kind in ("event_ms", "wall_ms"):
                    row[f"{name}_{kind}"], row[f"{name}_{kind}_min"], row[f"{name}_{kind}_max"] = _stat(t[name][kind])
            row["event_ratio"] = row["fused_event_ms"] / row["per_image_event_ms"]
            row["wall_ratio"] = row["fused_wall_ms"] / row["per_image_wall_ms"]
            rows.append(row)
            print(json.dumps(row))
    f = lambda r, k: f"{r[k]:.3f} ({r[k + '_min']:.3f}-{r[k + '_max']:.3f})"
    lines = ["# Batched Resize + CenterCrop: per-image path against the one-launch path", "",
             f"Measured on one {box} with `python tools/image_bench.py --batch {args.batch} --repeats {args.repeats} --warmup {args.warmup}`: "
             f"median (min-max) of {args.repeats} calls in milliseconds, the two paths alternating; outputs compared byte for byte first.",
             "`event`: HIP events on the stream around the call.  `wall`: host clock around the call and a device synchronise.", "",
             "| images | resize/crop | images on | tiles | LDS bytes | per-image event | fused event | ratio | per-image wall | fused wall | ratio |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} x {r['images']} | {r['resize']}/{r['crop']} | {r['placement']} | {r['tiles']} | {r['lds_bytes']} | "
                     f"{f(r, 'per_image_event_ms')} | {f(r, 'fused_event_ms')} | {r['event_ratio']:.3f} | {f(r, 'per_image_wall_ms')} | "
                     f"{f(r, 'fused_wall_ms')} | {r['wall_ratio']:.3f} |")
    lines += ["", f"Bytes a batch has to move at least (input read once + output written once): "
              + "; ".join(sorted({f"{r['n']} x {r['images']} at {r['resize']}/{r['crop']}: {r['input_mb'] + r['output_mb']:.1f} MB" for r in rows})) + ".", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
