"""From JPEG file bytes in memory to the cropped uint8 batch on the MI355X: host decoding against ``device_decode``.

``--batch`` JPEGs are derived from tests/golden/sample_500x375.jpg by re-encoding it with Pillow (sizes, qualities, subsamplings, with and
without restart markers; see ``SETS``).  Per set it times, at resize / crop 256 / 224,
  (a) host    ``decoded_batches(workers=16)`` (Pillow in 16 threads) + ``preprocess_batch_fused``      - the path before the device decoder,
  (b) device  ``jpeg.decode_jpeg_batch`` + ``preprocess_batch_fused``                                 - ``folder_loader(device_decode=True)``,
as host wall time around the call and a device synchronise, ``--repeats`` times after ``--warmup`` untimed calls, the two alternating
within each repeat; outputs are compared byte for byte first.  Then the three stages of ``hawq_jpeg_decode_batch`` with HIP events
recorded on the stream before stage 1 and behind each stage (a pair brackets one launch and whatever the stream waits for between the two
records).  Reported: median (min-max).  Writes the table to ``--out`` (markdown) and prints one JSON line per set.

    python tools/jpeg_bench.py [--batch 128] [--repeats 20] [--warmup 3] [--out profiles/jpeg_decode.md] [--box NAME]
"""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hawq_amd import _lib, image, jpeg  # noqa: E402

# name -> list of (scale, save options) cycled over the batch
SETS = {
    "375x500 q90 4:2:0": [(1.0, dict(quality=90, subsampling=2))],
    "375x500 q90 4:2:0, restart every MCU row": [(1.0, dict(quality=90, subsampling=2, restart_marker_rows=1))],
    "375x500 q90 4:2:0, restart every 4 MCUs": [(1.0, dict(quality=90, subsampling=2, restart_marker_blocks=4))],
    "mixed sizes / qualities / subsamplings": [(s, dict(quality=q, subsampling=ss)) for s in (0.75, 1.0, 1.5) for q in (75, 90, 95) for ss in (0, 1, 2)],
    "mixed, restart every MCU row": [(s, dict(quality=q, subsampling=ss, restart_marker_rows=1)) for s in (0.75, 1.0, 1.5) for q in (75, 90, 95)
                                     for ss in (0, 1, 2)],
}


def make_set(variants, n):
    from PIL import Image
    with Image.open(os.path.join(ROOT, "tests", "golden", "sample_500x375.jpg")) as im:
        base = im.convert("RGB")
    encoded = []
    for scale, kw in variants:
        pic = base if scale == 1.0 else base.resize((int(base.width * scale), int(base.height * scale)), Image.BILINEAR)
        buf = io.BytesIO()
        pic.save(buf, "JPEG", **kw)
        encoded.append(buf.getvalue())
    return [encoded[i % len(encoded)] for i in range(n)]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stat(v):
    return [statistics.median(v), min(v), max(v)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode.md"))
    ap.add_argument("--box", default=None, help="label of the machine for the report (default: the device name and architecture)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("jpeg_bench: needs the GPU (a CPU run says nothing about these times)")
    props = torch.cuda.get_device_properties(0)
    box = args.box or f"{props.name} ({getattr(props, 'gcnArchName', '?')})"
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    events = []
    for _ in range(4):
        ev = C.c_void_p()
        _lib.check(lib.hawq_event_create(C.byref(ev)))
        events.append(ev)
    rows = []
    for label, variants in SETS.items():
        datas = make_set(variants, args.batch)
        samples = [(d, 0) for d in datas]

        def host():
            imgs, _ = next(iter(image.decoded_batches(samples, len(samples), workers=16)))
            return image.preprocess_batch_fused(imgs, 256, 224, device=dev)

        def device():
            imgs, fallbacks = jpeg.decode_jpeg_batch(datas, dev)
            assert not fallbacks, fallbacks
            return image.preprocess_batch_fused(imgs, 256, 224, device=dev)

        if not torch.equal(host(), device()):
            sys.exit(f"jpeg_bench: the two paths differ at {label}")
        for _ in range(args.warmup):
            host(), device()
        t = {"host": [], "device": []}
        for r in range(args.repeats):
            for name in (("host", "device") if r % 2 == 0 else ("device", "host")):
                t[name].append(wall(host if name == "host" else device))
        # the stages alone: parsed once, planned + uploaded + launched per call
        records = [jpeg.parse_jpeg(d) for d in datas]
        offsets, total = [], 0
        for r in records:
            offsets.append(total)
            total = (total + r.width * r.height * 3 + 15) & ~15
        stages = [[], [], []]
        for k in range(args.warmup + args.repeats):
            _, status = jpeg._launch(records, offsets, total, dev, events)   # reads the status: synchronised
            assert not status.any()
            if k >= args.warmup:
                for s in range(3):
                    ms = C.c_float()
                    _lib.check(lib.hawq_event_elapsed_ms(events[s], events[s + 1], C.byref(ms)))
                    stages[s].append(ms.value)
        row = {"set": label, "n": len(datas), "compressed_mb": sum(map(len, datas)) / 1e6, "decoded_mb": total / 1e6,
               "waves": sum(len(r.intervals) for r in records), "largest_interval_bytes": int(max((r.intervals[:, 1] - r.intervals[:, 0]).max() for r in records)),
               "host_wall_ms": stat(t["host"]), "device_wall_ms": stat(t["device"]), "entropy_ms": stat(stages[0]), "idct_ms": stat(stages[1]),
               "colour_ms": stat(stages[2])}
        row["wall_ratio"] = row["device_wall_ms"][0] / row["host_wall_ms"][0]
        rows.append(row)
        print(json.dumps(row), flush=True)
    f = lambda v: f"{v[0]:.2f} ({v[0 + 1]:.2f}-{v[2]:.2f})"
    lines = ["# JPEG bytes in memory to the cropped batch on the device: host decode against device decode", "",
             f"Measured on one {box} with `python tools/jpeg_bench.py --batch {args.batch} --repeats {args.repeats} --warmup {args.warmup}`: median (min-max) of "
             f"{args.repeats} calls in milliseconds, the two paths alternating; outputs compared byte for byte first.  Resize / crop 256 / 224.",
             "`host`: Pillow in 16 threads + `preprocess_batch_fused`.  `device`: `decode_jpeg_batch` + `preprocess_batch_fused`.  Both: host clock around "
             "the call and a device synchronise.  Stages: HIP events on the stream before stage 1 and behind each stage.", "",
             "| set | MB compressed / decoded | waves | largest interval (bytes) | host wall | device wall | ratio | entropy | IDCT | upsample + colour |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} x {r['set']} | {r['compressed_mb']:.1f} / {r['decoded_mb']:.1f} | {r['waves']} | {r['largest_interval_bytes']} | "
                     f"{f(r['host_wall_ms'])} | {f(r['device_wall_ms'])} | {r['wall_ratio']:.2f} | {f(r['entropy_ms'])} | {f(r['idct_ms'])} | {f(r['colour_ms'])} |")
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
