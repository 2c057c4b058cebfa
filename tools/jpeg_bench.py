"""From JPEG file bytes in memory to the cropped uint8 batch on the MI355X: host decoding against ``device_decode``.

``--batch`` JPEGs are derived from tests/golden/sample_500x375.jpg by re-encoding it with Pillow (sizes, qualities, subsamplings, with and
without restart markers; see ``SETS``).  Per set it times, at resize / crop 256 / 224,
  (a) host    ``decoded_batches(workers=16)`` (Pillow in 16 threads) + ``preprocess_batch_fused``      - the path before the device decoder,
  (b) device  ``jpeg.decode_jpeg_batch`` + ``preprocess_batch_fused``                                 - ``folder_loader(device_decode=True)``,
as host wall time around the call and a device synchronise, ``--repeats`` times after ``--warmup`` untimed calls, the two alternating
within each repeat; outputs are compared byte for byte first.  Then the three stages of ``hawq_jpeg_decode_batch`` with HIP events
recorded on the stream before stage 1 and behind each stage (a pair brackets one launch and whatever the stream waits for between the two
records).  Reported: median (min-max).  Writes the table to ``--out`` (markdown) and prints one JSON line per set.

``--entropy sync`` times the device path with ``entropy="sync"`` (many lanes per long restart interval, ``--sub-bytes`` /
``--min-sync-bytes``) in place of the serial one; ``--entropy both`` times both device paths, alternating with each other and the host
path in one process, so the serial path of that process is the baseline of the other; the table gains the wall time and the entropy
stage of the second path and the decode passes ("rounds") the kernel counted for the largest interval.  ``--sweep`` adds the entropy
stage of the sync path for sub_bytes in 32 / 64 / 128 / 256 and min_sync_bytes in 256 / 1024 / 4096, each row alternating with the
serial stage.  ``--sets`` picks sets by index.

``--progressive`` measures progressive files instead (``PROGRESSIVE_SETS``: the sample re-encoded with ``progressive=True``, and batches
of which a quarter is progressive): host, ``device_decode`` as it is without the option (every progressive file falls back to Pillow on
the calling thread, one after the other) and ``decode_jpeg_batch(progressive=True)``, the three alternating in one process; then the
stages of ``hawq_jpeg_decode_batch_prog`` with HIP events (stage 1: all its levels).  Writes profiles/jpeg_progressive.md.

``--resume`` measures decoding from recorded resume points (``RESUME_SETS``: the baseline set without restart markers, the mixed-size
set and the progressive sets): the index is built per set (build time and bytes per file reported), then ``decode_jpeg_batch(progressive=
True)`` as it is, with ``entropy="sync"``, with ``resume=index`` and Pillow in 16 threads alternate in one process; then the entropy
stage of the three device paths with HIP events, summed over the calls of a batch (one per kind of file), and the entropy stage from
points recorded ``--every`` 256 .. 4096 bytes apart, each alternating with the serial stage.  Writes profiles/jpeg_resume.md.

``--front-end both`` measures the device front end (``decode_jpeg_batch(front_end="device")``) against the host one, the
two alternating in one process on ``FRONT_SETS``: the set with restart markers every MCU row on the serial entropy stage, the set without
markers and the mixed set with ``entropy="sync"``.  Per path the wall time of ``decode_jpeg_batch`` + ``preprocess_batch_fused`` and the
host milliseconds between the call and its first decode launch (parse + plan + upload on the host path; upload, scan, read-back, layout,
fill and read-back on the device path).  Writes profiles/jpeg_front.md.
``--front-end both --progressive`` measures the device front end for progressive files (``progressive="device"``) against
``progressive=True``, both under ``front_end="device"`` and alternating in one process, on ``PROGRESSIVE_SETS``: wall time, host time to the
first decode launch, and the stages of the new route.  Writes profiles/jpeg_front_prog.md.

``--draft`` measures the reduced-size decode (``decode_jpeg_batch(draft=(256, 256))``) on ``DRAFT_SETS``: the sample enlarged
to 1500 x 2000 and 3000 x 4000, with a restart marker every MCU row (serial entropy stage) and without (``entropy="sync"``).  The call
without the option and the call with it alternate in one process, each going first every other time; outputs are compared with Pillow's
draft pipeline first.  Then stages 2 + 3 of both from the HIP events, Pillow in 16 threads with the same draft, and the plane + output
bytes of the two plans.  Writes profiles/jpeg_draft.md.

    python tools/jpeg_bench.py [--batch 128] [--repeats 20] [--warmup 3] [--out profiles/jpeg_decode.md] [--box NAME]
                               [--entropy serial|sync|both] [--sub-bytes N] [--min-sync-bytes N] [--sweep] [--sets 0,1,3] [--progressive]
                               [--resume] [--every N] [--front-end both] [--draft]
"""
import argparse
import ctypes as C
import functools
import io
import json
import os
import statistics
import sys
import time

import numpy as np
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


_P = dict(progressive=True)
# name -> list of (scale, save options) cycled over the batch; every fourth file of a "quarter" set is progressive
PROGRESSIVE_SETS = {
    "375x500 q90 4:2:0, all progressive": [(1.0, dict(quality=90, subsampling=2, **_P))],
    "375x500 q90 4:2:0, all progressive, restart every MCU row": [(1.0, dict(quality=90, subsampling=2, restart_marker_rows=1, **_P))],
    "mixed sizes / qualities / subsamplings, all progressive": [(s, dict(quality=q, subsampling=ss, **_P)) for s in (0.75, 1.0, 1.5) for q in (75, 90, 95)
                                                                 for ss in (0, 1, 2)],
    "375x500 q90 4:2:0, a quarter progressive": [(1.0, dict(quality=90, subsampling=2, **(_P if k == 3 else {}))) for k in range(4)],
    "375x500 q90 4:2:0 restart every MCU row, a quarter progressive": [(1.0, dict(quality=90, subsampling=2, restart_marker_rows=1, **(_P if k == 3 else {})))
                                                                        for k in range(4)],
}


# the sets of --resume: long intervals of both kinds, and the sets with restart markers that the option must leave where they were
RESUME_SETS = {k: SETS[k] for k in ("375x500 q90 4:2:0", "mixed sizes / qualities / subsamplings")}
RESUME_SETS.update(PROGRESSIVE_SETS)
EVERY_SWEEP = (256, 512, 1024, 2048, 4096)
# the sets of --front-end: (set, entropy stage), as profiles/jpeg_sync.md has them
FRONT_SETS = [("375x500 q90 4:2:0, restart every MCU row", "serial"), ("375x500 q90 4:2:0", "sync"), ("mixed sizes / qualities / subsamplings", "sync")]


# the sets of --draft: (label, enlargement of the 375 x 500 sample, save options, entropy stage)
DRAFT_REQUEST = (256, 256)
DRAFT_SETS = [(f"{375 * k}x{500 * k} q90 4:2:0{', restart every MCU row' if rst else ''}", float(k), dict(quality=90, subsampling=2, **rst), "serial" if rst else "sync")
              for k in (4, 8) for rst in (dict(restart_marker_rows=1), {})]


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
    ap.add_argument("--out", default=None, help="default: profiles/jpeg_decode.md, with --progressive profiles/jpeg_progressive.md")
    ap.add_argument("--progressive", action="store_true", help="progressive files: host, device_decode without and with progressive=True")
    ap.add_argument("--box", default=None, help="label of the machine for the report (default: the device name and architecture)")
    ap.add_argument("--entropy", choices=("serial", "sync", "both"), default="serial")
    ap.add_argument("--sub-bytes", type=int, default=jpeg.SUB_BYTES)
    ap.add_argument("--min-sync-bytes", type=int, default=jpeg.MIN_SYNC_BYTES)
    ap.add_argument("--sweep", action="store_true", help="entropy stage of the sync path over a grid of sub_bytes x min_sync_bytes")
    ap.add_argument("--sets", default=None, help="comma-separated indices into SETS (default: all)")
    ap.add_argument("--resume", action="store_true", help="resume points: the serial, sync and resume device paths and Pillow, and a sweep over the distance")
    ap.add_argument("--front-end", choices=("both",), default=None, help="the host and the device front end of decode_jpeg_batch, alternating")
    ap.add_argument("--draft", action="store_true", help="large files: decode_jpeg_batch without and with draft=(256, 256), alternating")
    ap.add_argument("--every", type=int, default=jpeg.RESUME_EVERY, help="distance of the resume points of the wall-time rows")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "jpeg_draft.md" if args.draft else "jpeg_front_prog.md" if args.front_end and args.progressive else "jpeg_front.md" if args.front_end else "jpeg_resume.md" if args.resume else "jpeg_progressive.md" if args.progressive else "jpeg_decode.md")
    paths = ("serial", "sync") if args.entropy == "both" else (args.entropy,)
    sync_of = {"serial": None, "sync": (args.sub_bytes, args.min_sync_bytes)}
    picked = [int(k) for k in args.sets.split(",")] if args.sets else range(len(SETS))
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
    if args.draft:
        return draft(args, box, dev, lib, events)
    if args.front_end and args.progressive:
        return front_end_progressive(args, box, dev, lib, events)
    if args.front_end:
        return front_end(args, box, dev)
    if args.resume:
        return resume(args, box, dev, lib, events)
    if args.progressive:
        return progressive(args, box, dev, lib, events)
    rows, sweep_rows = [], []
    for label, variants in [list(SETS.items())[k] for k in picked]:
        datas = make_set(variants, args.batch)
        samples = [(d, 0) for d in datas]

        def host():
            imgs, _ = next(iter(image.decoded_batches(samples, len(samples), workers=16)))
            return image.preprocess_batch_fused(imgs, 256, 224, device=dev)

        def device(path=paths[0]):
            more = {} if path == "serial" else dict(entropy="sync", sub_bytes=args.sub_bytes, min_sync_bytes=args.min_sync_bytes)
            imgs, fallbacks = jpeg.decode_jpeg_batch(datas, dev, **more)
            assert not fallbacks, fallbacks
            return image.preprocess_batch_fused(imgs, 256, 224, device=dev)

        runs = {"host": host}
        runs.update({p: (lambda p=p: device(p)) for p in paths})
        want = host()
        for p in paths:
            if not torch.equal(want, device(p)):
                sys.exit(f"jpeg_bench: the host path and the {p} device path differ at {label}")
        for _ in range(args.warmup):
            for fn in runs.values():
                fn()
        t = {name: [] for name in runs}
        order = list(runs)
        for r in range(args.repeats):
            for name in order[r % len(order):] + order[:r % len(order)]:   # every path takes every place in turn
                t[name].append(wall(runs[name]))
        # the stages alone: parsed once, planned + uploaded + launched per call
        records = [jpeg.parse_jpeg(d) for d in datas]
        offsets, total = jpeg.output_layout([(r.height, r.width) for r in records])
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        lengths = [int(v) for r in records for v in (r.intervals[:, 1] - r.intervals[:, 0])]

        def staged(pairs, repeats):
            """{key: ([stage 1 ms], [stage 2 ms], [stage 3 ms], [rounds of the largest interval or None])} of (key, sync) pairs, alternating"""
            got = {key: ([], [], [], [None]) for key, _ in pairs}
            for k in range(args.warmup + repeats):
                for key, sync in pairs[k % len(pairs):] + pairs[:k % len(pairs)]:
                    info = {}
                    more = {} if sync is None else dict(sync=sync, info=info)
                    status = jpeg._launch(records, offsets, out, dev, events, **more).cpu()   # reads the status: synchronised
                    assert not status.any()
                    if sync is not None and info["jobs"]:
                        waves = [w for w, _, _ in info["jobs"]]
                        got[key][3][0] = info["rounds"][max(range(len(waves)), key=lambda j: lengths[waves[j]])]
                    if k >= args.warmup:
                        for s in range(3):
                            ms = C.c_float()
                            _lib.check(lib.hawq_event_elapsed_ms(events[s], events[s + 1], C.byref(ms)))
                            got[key][s].append(ms.value)
            return got

        per_path = staged([(p, sync_of[p]) for p in paths], args.repeats)
        stages = per_path[paths[0]]
        row = {"set": label, "n": len(datas), "compressed_mb": sum(map(len, datas)) / 1e6, "decoded_mb": total / 1e6,
               "waves": sum(len(r.intervals) for r in records), "largest_interval_bytes": int(max((r.intervals[:, 1] - r.intervals[:, 0]).max() for r in records)),
               "entropy_ms": stat(stages[0]), "idct_ms": stat(stages[1]), "colour_ms": stat(stages[2])}
        row["host_wall_ms"], row["device_wall_ms"] = stat(t["host"]), stat(t[paths[0]])
        row["wall_ratio"] = row["device_wall_ms"][0] / row["host_wall_ms"][0]
        row["entropy"] = paths[0]
        if "sync" in paths:
            row["sub_bytes"], row["min_sync_bytes"], row["rounds_largest"] = args.sub_bytes, args.min_sync_bytes, per_path["sync"][3][0]
        if len(paths) > 1:
            row["sync_wall_ms"], row["sync_entropy_ms"] = stat(t["sync"]), stat(per_path["sync"][0])
            row["sync_wall_ratio"] = row["sync_wall_ms"][0] / row["host_wall_ms"][0]
        rows.append(row)
        print(json.dumps(row), flush=True)
        if args.sweep:
            for sub in (32, 64, 128, 256):
                for low in (256, 1024, 4096):
                    got = staged([("serial", None), ("sync", (sub, low))], args.repeats)
                    sw = {"set": label, "sub_bytes": sub, "min_sync_bytes": low, "jobs": sum(v >= low for v in lengths), "serial_entropy_ms": stat(got["serial"][0]),
                          "sync_entropy_ms": stat(got["sync"][0]), "rounds_largest": got["sync"][3][0]}
                    sweep_rows.append(sw)
                    print(json.dumps(sw), flush=True)
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
    if args.entropy != "serial":
        lines += ["", f"`device` above is the `{paths[0]}` entropy stage." + (f"  The `sync` one (sub_bytes {args.sub_bytes}, min_sync_bytes {args.min_sync_bytes}), "
                  "alternating with it and the host path in the same process:" if len(paths) > 1 else f"  sub_bytes {args.sub_bytes}, min_sync_bytes {args.min_sync_bytes}."), ""]
    if len(paths) > 1:
        lines += ["| set | serial wall | sync wall | sync / host | serial entropy | sync entropy | serial / sync entropy | rounds of the largest interval |", "|---|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(f"| {r['n']} x {r['set']} | {f(r['device_wall_ms'])} | {f(r['sync_wall_ms'])} | {r['sync_wall_ratio']:.2f} | {f(r['entropy_ms'])} | "
                         f"{f(r['sync_entropy_ms'])} | {r['entropy_ms'][0] / r['sync_entropy_ms'][0]:.1f} | {r['rounds_largest']} |")
    if sweep_rows:
        lines += ["", "## Entropy stage over sub_bytes x min_sync_bytes", "",
                  "Each row: the serial and the sync stage 1 alternating, HIP events around the stage (both kernels of the sync path).", "",
                  "| set | sub_bytes | min_sync_bytes | jobs | serial entropy | sync entropy | rounds of the largest interval |", "|---|---|---|---|---|---|---|"]
        for r in sweep_rows:
            lines.append(f"| {r['set']} | {r['sub_bytes']} | {r['min_sync_bytes']} | {r['jobs']} | {f(r['serial_entropy_ms'])} | {f(r['sync_entropy_ms'])} | {r['rounds_largest']} |")
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


def draft(args, box, dev, lib, events):
    """the ``--draft`` report"""
    picked = [int(k) for k in args.sets.split(",")] if args.sets else range(len(DRAFT_SETS))
    rows = []
    for label, scale, kw, entropy in [DRAFT_SETS[k] for k in picked]:
        datas = make_set([(scale, kw)], args.batch)
        samples = [(d, 0) for d in datas]
        more = {} if entropy == "serial" else dict(entropy="sync", sub_bytes=args.sub_bytes, min_sync_bytes=args.min_sync_bytes)

        def pillow(request):
            decode = image.decode_image if request is None else functools.partial(image.decode_image, draft=request)
            imgs, _ = next(iter(image.decoded_batches(samples, len(samples), workers=16, decode=decode)))
            return image.preprocess_batch_fused(imgs, 256, 224, device=dev)

        def device(request):
            imgs, fallbacks = jpeg.decode_jpeg_batch(datas, dev, draft=request, **more)
            assert not fallbacks, fallbacks
            return image.preprocess_batch_fused(imgs, 256, 224, device=dev)

        for request in (None, DRAFT_REQUEST):
            if not torch.equal(pillow(request), device(request)):
                sys.exit(f"jpeg_bench: Pillow and the device path differ at {label}, draft {request}")
        runs = {"full": lambda: device(None), "draft": lambda: device(DRAFT_REQUEST)}
        for _ in range(args.warmup):
            for fn in runs.values():
                fn()
        t = {name: [] for name in runs}
        order = list(runs)
        for r in range(args.repeats):
            for name in order[r % 2:] + order[:r % 2]:   # each path goes first every other time
                t[name].append(wall(runs[name]))
        t["pillow"] = [wall(lambda: pillow(DRAFT_REQUEST)) for _ in range(args.warmup + args.repeats)][args.warmup:]
        # stages 2 + 3 alone: parsed once, planned + uploaded + launched per call
        records = [jpeg.parse_jpeg(d) for d in datas]
        sync = None if entropy == "serial" else (args.sub_bytes, args.min_sync_bytes)
        row = {"set": label, "entropy": entropy, "n": len(datas), "compressed_mb": sum(map(len, datas)) / 1e6,
               "scale": jpeg.draft_scale(records[0].width, records[0].height, DRAFT_REQUEST)}
        stages = {}
        for name, request in (("full", None), ("draft", DRAFT_REQUEST)):
            plan = jpeg.plan_jpeg_batch(records, draft=request)
            row[name + "_plane_mb"], row[name + "_out_mb"], row[name + "_coef_mb"] = plan.plane_bytes / 1e6, plan.out_bytes / 1e6, plan.coef_blocks * 128 / 1e6
            stages[name] = (plan.out_offsets, torch.empty(plan.out_bytes, dtype=torch.uint8, device=dev), {} if request is None else {"draft": request}, ([], [], []))
        for k in range(args.warmup + args.repeats):
            for name in order[k % 2:] + order[:k % 2]:
                offsets, out, option, got = stages[name]
                status = jpeg._launch(records, offsets, out, dev, events, **({} if sync is None else {"sync": sync}), **option).cpu()   # reads the status: synchronised
                assert not status.any()
                if k >= args.warmup:
                    for s_ in range(3):
                        ms = C.c_float()
                        _lib.check(lib.hawq_event_elapsed_ms(events[s_], events[s_ + 1], C.byref(ms)))
                        got[s_].append(ms.value)
        for name in order:
            got = stages[name][3]
            row[name + "_wall_ms"], row[name + "_entropy_ms"] = stat(t[name]), stat(got[0])
            row[name + "_pixel_ms"] = stat([a + b for a, b in zip(got[1], got[2])])
        row["pillow_wall_ms"] = stat(t["pillow"])
        row["wall_ratio"] = row["draft_wall_ms"][0] / row["full_wall_ms"][0]
        del stages
        torch.cuda.empty_cache()
        rows.append(row)
        print(json.dumps(row), flush=True)
    f = lambda v: f"{v[0]:.2f} ({v[1]:.2f}-{v[2]:.2f})"
    lines = ["# Large JPEGs decoded at reduced size on the device (`draft=`), against the full-size decode", "",
             f"Measured on one {box} with `python tools/jpeg_bench.py --draft --batch {args.batch} --repeats {args.repeats} --warmup {args.warmup}`: median "
             f"(min-max) of {args.repeats} calls in milliseconds, the two device paths alternating in one process, each going first every other time; both compared byte "
             "for byte with Pillow's pipeline (with and without the draft) first.  Resize / crop 256 / 224.",
             f"`full`: `decode_jpeg_batch` as it is + `preprocess_batch_fused`.  `draft`: the same with `draft={DRAFT_REQUEST}`.  `Pillow`: Pillow in 16 threads with "
             "the same draft + `preprocess_batch_fused`.  Wall: host clock around the call and a device synchronise.  Stages: HIP events on the stream around stage 1 "
             f"and around stages 2 + 3 of the decode call alone.  `entropy=\"sync\"` with sub_bytes {args.sub_bytes}, min_sync_bytes {args.min_sync_bytes}.", "",
             "| set | entropy | scale | full wall | draft wall | draft / full | Pillow (draft) wall | full stages 2 + 3 | draft stages 2 + 3 | full entropy | draft entropy |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} x {r['set']} | {r['entropy']} | 1/{r['scale']} | {f(r['full_wall_ms'])} | {f(r['draft_wall_ms'])} | {r['wall_ratio']:.2f} | {f(r['pillow_wall_ms'])} | "
                     f"{f(r['full_pixel_ms'])} | {f(r['draft_pixel_ms'])} | {f(r['full_entropy_ms'])} | {f(r['draft_entropy_ms'])} |")
    lines += ["", "Device buffers of the plan, in MB (the coefficient slab is the same for both):", "",
              "| set | MB compressed | coefficients | full planes | full output | draft planes | draft output |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} x {r['set']} | {r['compressed_mb']:.1f} | {r['full_coef_mb']:.1f} | {r['full_plane_mb']:.1f} | {r['full_out_mb']:.1f} | "
                     f"{r['draft_plane_mb']:.1f} | {r['draft_out_mb']:.1f} |")
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


def front_end(args, box, dev):
    """the ``--front-end both`` report"""
    picked = [int(k) for k in args.sets.split(",")] if args.sets else range(len(FRONT_SETS))
    rows, first = [], {}
    call = _lib.call

    def spy(name, *a):   # when the first decode entry point of a decode_jpeg_batch call is reached
        if name.startswith("hawq_jpeg_decode_batch") and "t" not in first:
            first["t"] = time.perf_counter()
        return call(name, *a)

    _lib.call = spy
    for label, entropy in [FRONT_SETS[k] for k in picked]:
        datas = make_set(SETS[label], args.batch)
        more = {} if entropy == "serial" else dict(entropy="sync", sub_bytes=args.sub_bytes, min_sync_bytes=args.min_sync_bytes)

        def device(front):
            first.clear()
            t0 = time.perf_counter()
            imgs, fallbacks = jpeg.decode_jpeg_batch(datas, dev, front_end=front, **more)
            assert not fallbacks, fallbacks
            first["ms"] = (first["t"] - t0) * 1e3
            return image.preprocess_batch_fused(imgs, 256, 224, device=dev)

        if not torch.equal(device("host"), device("device")):
            sys.exit(f"jpeg_bench: the two front ends differ at {label}")
        for _ in range(args.warmup):
            for front in ("host", "device"):
                device(front)
        t, before = {"host": [], "device": []}, {"host": [], "device": []}
        order = list(t)
        for r in range(args.repeats):
            for front in order[r % 2:] + order[:r % 2]:   # each path goes first every other time
                t[front].append(wall(lambda: device(front)))
                before[front].append(first["ms"])
        info = jpeg.front_scan_host(datas)
        row = {"set": label, "entropy": entropy, "n": len(datas), "compressed_mb": sum(map(len, datas)) / 1e6, "accepted": int((info["defer"] == 0).sum()),
               "waves": int(info["n_intervals"].sum())}
        for front in order:
            row[front + "_wall_ms"], row[front + "_before_launch_ms"] = stat(t[front]), stat(before[front])
        row["wall_ratio"] = row["device_wall_ms"][0] / row["host_wall_ms"][0]
        rows.append(row)
        print(json.dumps(row), flush=True)
    _lib.call = call
    f = lambda v: f"{v[0]:.2f} ({v[1]:.2f}-{v[2]:.2f})"
    lines = ["# The device front end of the JPEG decoder against the host one, alternating in one process", "",
             f"Measured on one {box} with `python tools/jpeg_bench.py --front-end both --batch {args.batch} --repeats {args.repeats} --warmup {args.warmup}`: median "
             f"(min-max) of {args.repeats} calls in milliseconds, the two paths alternating, each going first every other time; outputs compared byte for byte first.  "
             "Resize / crop 256 / 224.", "`host`: `decode_jpeg_batch` as it is (`parse_jpeg` per file, `plan_jpeg_batch`, one upload) + `preprocess_batch_fused`.  "
             "`device`: the same with `front_end=\"device\"` (raw files up, `hawq_jpeg_front_scan`, records back, numpy layout, `hawq_jpeg_front_fill`, blob back, "
             "the library's check).  Wall: host clock around the call and a device synchronise.  Before the launch: host clock from the call to its first "
             f"`hawq_jpeg_decode_batch` / `_sync`.  `entropy=\"sync\"` with sub_bytes {args.sub_bytes}, min_sync_bytes {args.min_sync_bytes}.", "",
             "| set | entropy | accepted by the scan | waves | host wall | device wall | device / host | host: before the launch | device: before the launch |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} x {r['set']} | {r['entropy']} | {r['accepted']} | {r['waves']} | {f(r['host_wall_ms'])} | {f(r['device_wall_ms'])} | {r['wall_ratio']:.2f} | "
                     f"{f(r['host_before_launch_ms'])} | {f(r['device_before_launch_ms'])} |")
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


def front_end_progressive(args, box, dev, lib, events):
    """the ``--front-end both --progressive`` report: ``progressive=True`` against ``progressive="device"``, both under the device front end"""
    picked = [int(k) for k in args.sets.split(",")] if args.sets else range(len(PROGRESSIVE_SETS))
    rows, first = [], {}
    call = _lib.call

    def spy(name, *a):   # when the first decode entry point of a decode_jpeg_batch call is reached
        if name.startswith("hawq_jpeg_decode_batch") and "t" not in first:
            first["t"] = time.perf_counter()
        return call(name, *a)

    for label, variants in [list(PROGRESSIVE_SETS.items())[k] for k in picked]:
        datas = make_set(variants, args.batch)

        def device(option):
            first.clear()
            t0 = time.perf_counter()
            imgs, fallbacks = jpeg.decode_jpeg_batch(datas, dev, front_end="device", progressive=option)
            assert not fallbacks, fallbacks
            first["ms"] = (first["t"] - t0) * 1e3
            return image.preprocess_batch_fused(imgs, 256, 224, device=dev)

        runs = {"python": True, "device": "device"}
        _lib.call = spy
        if not torch.equal(device(True), device("device")):
            sys.exit(f"jpeg_bench: progressive=True and progressive='device' differ at {label}")
        for _ in range(args.warmup):
            for option in runs.values():
                device(option)
        t, before = {name: [] for name in runs}, {name: [] for name in runs}
        order = list(runs)
        for r in range(args.repeats):
            for name in order[r % 2:] + order[:r % 2]:   # each path goes first every other time
                t[name].append(wall(lambda: device(runs[name])))
                before[name].append(first["ms"])
        _lib.call = call
        # the stages of the new route alone: scan, layout, fill and read-back on the host clock, then the decode's launches with HIP events
        info, scans = jpeg.front_scan_prog_host(datas)
        prog = np.flatnonzero((info["defer"] == 0) & (info["reserved"][:, 0] == jpeg.FRONT_KIND_PROG)).tolist()
        sizes = [(int(info["height"][i]), int(info["width"][i])) for i in prog]
        offsets, total = jpeg.output_layout(sizes)
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        front, stages = ([], []), ([], [], [])
        for k in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info_d, scans_d, staged = jpeg._front_scan_prog(datas, dev)
            t1 = time.perf_counter()
            filled = jpeg._front_prog_fill(staged, info_d, scans_d, prog, offsets, out, dev)
            torch.cuda.current_stream(dev).synchronize()
            t2 = time.perf_counter()
            status = jpeg._front_prog_decode(filled, out, dev, events, wait=False).cpu()   # reads the status: synchronised
            assert not status.any()
            if k >= args.warmup:
                front[0].append((t1 - t0) * 1e3)
                front[1].append((t2 - t1) * 1e3)
                for s in range(3):
                    ms = C.c_float()
                    _lib.check(lib.hawq_event_elapsed_ms(events[s], events[s + 1], C.byref(ms)))
                    stages[s].append(ms.value)
        row = {"set": label, "n": len(datas), "progressive": len(prog), "compressed_mb": sum(map(len, datas)) / 1e6, "scans": int(info["reserved"][prog, 1].sum()),
               "blob_mb": filled[0].nbytes / 1e6, "scan_ms": stat(front[0]), "fill_ms": stat(front[1]), "entropy_ms": stat(stages[0]), "idct_ms": stat(stages[1]),
               "colour_ms": stat(stages[2])}
        for name in order:
            row[name + "_wall_ms"], row[name + "_before_launch_ms"] = stat(t[name]), stat(before[name])
        spread = row["python_wall_ms"][2] - row["python_wall_ms"][1]
        row["gain_ms"] = row["python_wall_ms"][0] - row["device_wall_ms"][0]
        row["counts"] = bool(abs(row["gain_ms"]) > spread)   # a difference counts where it exceeds the min-max spread of the old path
        rows.append(row)
        print(json.dumps(row), flush=True)
    f = lambda v: f"{v[0]:.2f} ({v[1]:.2f}-{v[2]:.2f})"
    lines = ["# The device front end for progressive JPEGs against the Python one, alternating in one process", "",
             f"Measured on one {box} with `python tools/jpeg_bench.py --front-end both --progressive --batch {args.batch} --repeats {args.repeats} --warmup {args.warmup}`: "
             f"median (min-max) of {args.repeats} calls in milliseconds, the two paths alternating, each going first every other time; outputs compared byte for byte "
             "first.  Resize / crop 256 / 224.", "`python`: `decode_jpeg_batch(front_end=\"device\", progressive=True)` (the walker defers every progressive file to "
             "`parse_jpeg` and `plan_jpeg_prog_batch`) + `preprocess_batch_fused`.  `device`: the same with `progressive=\"device\"` (`hawq_jpeg_front_scan_prog`, records "
             "back, numpy layout, `hawq_jpeg_front_fill_prog`, blob back with the baseline one, the library's check).  Wall: host clock around the call and a device "
             "synchronise.  Before the launch: host clock from the call to its first `hawq_jpeg_decode_batch*`.  Gain: python wall - device wall, medians; it counts "
             "where it exceeds the min-max spread of the python path in the same run.", "",
             "| set | progressive files | scans | python wall | device wall | gain | counts | python: before the launch | device: before the launch |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} x {r['set']} | {r['progressive']} | {r['scans']} | {f(r['python_wall_ms'])} | {f(r['device_wall_ms'])} | {r['gain_ms']:.2f} | "
                     f"{'yes' if r['counts'] else 'no'} | {f(r['python_before_launch_ms'])} | {f(r['device_before_launch_ms'])} |")
    lines += ["", "The new route alone on the progressive files of the set: upload + `hawq_jpeg_front_scan_prog` + records back, then layout + "
              "`hawq_jpeg_front_fill_prog` + blob back (host clock), then the launches of `hawq_jpeg_decode_batch_prog` (HIP events).", "",
              "| set | blob MB | upload + scan + records back | layout + fill + blob back | entropy, all levels | IDCT | upsample + colour |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} x {r['set']} | {r['blob_mb']:.1f} | {f(r['scan_ms'])} | {f(r['fill_ms'])} | {f(r['entropy_ms'])} | {f(r['idct_ms'])} | {f(r['colour_ms'])} |")
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


def progressive(args, box, dev, lib, events):
    """the ``--progressive`` report"""
    picked = [int(k) for k in args.sets.split(",")] if args.sets else range(len(PROGRESSIVE_SETS))
    rows = []
    for label, variants in [list(PROGRESSIVE_SETS.items())[k] for k in picked]:
        datas = make_set(variants, args.batch)
        samples = [(d, 0) for d in datas]
        records = [jpeg.parse_jpeg(d, progressive=True) for d in datas]
        prog = [r for r in records if isinstance(r, jpeg.JpegProgRecord)]

        def host():
            imgs, _ = next(iter(image.decoded_batches(samples, len(samples), workers=16)))
            return image.preprocess_batch_fused(imgs, 256, 224, device=dev)

        def device(option):
            imgs, fallbacks = jpeg.decode_jpeg_batch(datas, dev, **({"progressive": True} if option else {}))
            assert len(fallbacks) == (0 if option else len(prog)), fallbacks
            return image.preprocess_batch_fused(imgs, 256, 224, device=dev)

        runs = {"host": host, "device": lambda: device(False), "progressive": lambda: device(True)}
        want = host()
        for name in ("device", "progressive"):
            if not torch.equal(want, runs[name]()):
                sys.exit(f"jpeg_bench: the host path and the {name} path differ at {label}")
        for _ in range(args.warmup):
            for fn in runs.values():
                fn()
        t = {name: [] for name in runs}
        order = list(runs)
        for r in range(args.repeats):
            for name in order[r % len(order):] + order[:r % len(order)]:   # every path takes every place in turn
                t[name].append(wall(runs[name]))
        # the stages of the progressive call alone: parsed once, planned + uploaded + launched per call
        offsets, total = jpeg.output_layout([(r.height, r.width) for r in prog])
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        stages = ([], [], [])
        for k in range(args.warmup + args.repeats):
            status = jpeg._launch(prog, offsets, out, dev, events).cpu()   # reads the status: synchronised
            assert not status.any()
            if k >= args.warmup:
                for s in range(3):
                    ms = C.c_float()
                    _lib.check(lib.hawq_event_elapsed_ms(events[s], events[s + 1], C.byref(ms)))
                    stages[s].append(ms.value)
        plan = jpeg.plan_jpeg_prog_batch(prog, offsets, total)
        per_level = {}   # level -> the longest interval of a scan of that level
        for r in prog:
            for s, level in zip(r.scans, jpeg.scan_levels(r.scans)):
                per_level[level] = max(per_level.get(level, 0), int((s.intervals[:, 1] - s.intervals[:, 0]).max()))
        row = {"set": label, "n": len(datas), "progressive": len(prog), "compressed_mb": sum(map(len, datas)) / 1e6, "levels": plan.n_levels, "waves": plan.n_waves,
               "largest_interval_per_level": [per_level[k] for k in sorted(per_level)], "entropy_ms": stat(stages[0]), "idct_ms": stat(stages[1]),
               "colour_ms": stat(stages[2])}
        for name in runs:
            row[name + "_wall_ms"] = stat(t[name])
        rows.append(row)
        print(json.dumps(row), flush=True)
    f = lambda v: f"{v[0]:.2f} ({v[1]:.2f}-{v[2]:.2f})"
    lines = ["# Progressive JPEG bytes in memory to the cropped batch on the device", "",
             f"Measured on one {box} with `python tools/jpeg_bench.py --progressive --batch {args.batch} --repeats {args.repeats} --warmup {args.warmup}`: median "
             f"(min-max) of {args.repeats} calls in milliseconds, the three paths alternating in one process; outputs compared byte for byte first.  Resize / crop "
             "256 / 224.", "`host`: Pillow in 16 threads + `preprocess_batch_fused`.  `device`: `decode_jpeg_batch` as it is without the option (a progressive file "
             "falls back to Pillow on the calling thread) + `preprocess_batch_fused`.  `progressive`: the same with `progressive=True`.  All: host clock around the "
             "call and a device synchronise.  Stages: HIP events around the launches of `hawq_jpeg_decode_batch_prog` for the progressive files of the set alone "
             "(entropy: all its levels).", "",
             "| set | progressive files | MB compressed | host wall | device wall | progressive wall | progressive / host | progressive / device |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} x {r['set']} | {r['progressive']} | {r['compressed_mb']:.1f} | {f(r['host_wall_ms'])} | {f(r['device_wall_ms'])} | "
                     f"{f(r['progressive_wall_ms'])} | {r['progressive_wall_ms'][0] / r['host_wall_ms'][0]:.2f} | {r['progressive_wall_ms'][0] / r['device_wall_ms'][0]:.2f} |")
    lines += ["", "| set | levels | waves | largest interval per level (bytes) | entropy, all levels | IDCT | upsample + colour |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} x {r['set']} | {r['levels']} | {r['waves']} | {' / '.join(map(str, r['largest_interval_per_level']))} | {f(r['entropy_ms'])} | "
                     f"{f(r['idct_ms'])} | {f(r['colour_ms'])} |")
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


def resume(args, box, dev, lib, events):
    """the ``--resume`` report"""
    picked = [int(k) for k in args.sets.split(",")] if args.sets else range(len(RESUME_SETS))
    sync = (args.sub_bytes, args.min_sync_bytes)
    rows = []
    for label, variants in [list(RESUME_SETS.items())[k] for k in picked]:
        datas = make_set(variants, args.batch)
        samples = [(d, 0) for d in datas]
        distinct = list(dict.fromkeys(datas))
        indexes, build_ms, index_bytes = {}, {}, {}
        for every in sorted(set(EVERY_SWEEP) | {args.every}):
            t0 = time.perf_counter()
            indexes[every] = jpeg.build_resume_index(distinct, every=every, progressive=True)
            build_ms[every] = (time.perf_counter() - t0) * 1e3 / len(distinct)
            buf = io.BytesIO()
            indexes[every].save(buf)
            index_bytes[every] = len(buf.getvalue()) / len(distinct)
        index = indexes[args.every]

        def host():
            imgs, _ = next(iter(image.decoded_batches(samples, len(samples), workers=16)))
            return image.preprocess_batch_fused(imgs, 256, 224, device=dev)

        def device(**more):
            imgs, fallbacks = jpeg.decode_jpeg_batch(datas, dev, progressive=True, **more)
            assert not fallbacks, fallbacks
            return image.preprocess_batch_fused(imgs, 256, 224, device=dev)

        runs = {"host": host, "serial": device, "sync": lambda: device(entropy="sync", sub_bytes=sync[0], min_sync_bytes=sync[1]), "resume": lambda: device(resume=index)}
        want = host()
        for name in ("serial", "sync", "resume"):
            if not torch.equal(want, runs[name]()):
                sys.exit(f"jpeg_bench: the host path and the {name} path differ at {label}")
        for _ in range(args.warmup):
            for fn in runs.values():
                fn()
        t = {name: [] for name in runs}
        order = list(runs)
        for r in range(args.repeats):
            for name in order[r % len(order):] + order[:r % len(order)]:   # every path takes every place in turn
                t[name].append(wall(runs[name]))
        # the entropy stage alone, summed over the calls of the batch: parsed once, planned + uploaded + launched per call
        records = [jpeg.parse_jpeg(d, progressive=True) for d in datas]
        kinds = [[(r, d) for r, d in zip(records, datas) if isinstance(r, kind)] for kind in (jpeg.JpegProgRecord, jpeg.JpegRecord)]
        kinds = [k for k in kinds if k]
        outs = []
        for kind in kinds:
            offsets, total = jpeg.output_layout([(r.height, r.width) for r, _ in kind])
            outs.append((offsets, torch.empty(total, dtype=torch.uint8, device=dev)))

        def entropy_ms(path, every=None):
            total = 0.0
            for kind, (offsets, out) in zip(kinds, outs):
                recs = [r for r, _ in kind]
                more = {}
                if path == "sync" and isinstance(recs[0], jpeg.JpegRecord):
                    more = {"sync": sync}
                if path == "resume":
                    more = {"resume": [indexes[every].points(d, r) for r, d in kind]}
                status = jpeg._launch(recs, offsets, out, dev, events, **more).cpu()   # reads the status: synchronised
                assert not status.any()
                ms = C.c_float()
                _lib.check(lib.hawq_event_elapsed_ms(events[0], events[1], C.byref(ms)))
                total += ms.value
            return total

        def staged(pairs):
            got = {key: [] for key in pairs}
            for k in range(args.warmup + args.repeats):
                for key in pairs[k % len(pairs):] + pairs[:k % len(pairs)]:
                    ms = entropy_ms(*key)
                    if k >= args.warmup:
                        got[key].append(ms)
            return got

        stage = staged([("serial",), ("sync",), ("resume", args.every)])
        sweep = {every: staged([("serial",), ("resume", every)]) for every in EVERY_SWEEP}
        lengths = [int(v) for r in records for s in (r.scans if isinstance(r, jpeg.JpegProgRecord) else [r]) for v in (s.intervals[:, 1] - s.intervals[:, 0])]
        row = {"set": label, "n": len(datas), "every": args.every, "largest_interval_bytes": max(lengths), "waves": len(lengths),
               "segments": {every: len(lengths) + sum(len(indexes[every].points(d, r)) for r, d in zip(records, datas)) for every in indexes},
               "index_build_ms_per_file": build_ms, "index_bytes_per_file": index_bytes,
               "entropy_ms": {name: stat(stage[key]) for name, key in (("serial", ("serial",)), ("sync", ("sync",)), ("resume", ("resume", args.every)))},
               "sweep_entropy_ms": {every: {"serial": stat(got[("serial",)]), "resume": stat(got[("resume", every)])} for every, got in sweep.items()}}
        for name in runs:
            row[name + "_wall_ms"] = stat(t[name])
        rows.append(row)
        print(json.dumps(row), flush=True)
    f = lambda v: f"{v[0]:.2f} ({v[1]:.2f}-{v[2]:.2f})"
    lines = ["# JPEG bytes in memory to the cropped batch on the device: long restart intervals from recorded resume points", "",
             f"Measured on one {box} with `python tools/jpeg_bench.py --resume --batch {args.batch} --repeats {args.repeats} --warmup {args.warmup} --every {args.every}`: "
             f"median (min-max) of {args.repeats} calls in milliseconds, the paths alternating in one process; outputs compared byte for byte first.  Resize / crop "
             "256 / 224.", "`Pillow`: Pillow in 16 threads + `preprocess_batch_fused`.  `serial` / `sync` / `resume`: `decode_jpeg_batch(progressive=True)` as it is, with "
             f"`entropy=\"sync\"` (sub_bytes {sync[0]}, min_sync_bytes {sync[1]}; baseline files only) and with `resume=index` (points every {args.every} bytes, the "
             "index built before and held in memory) + `preprocess_batch_fused`.  All: host clock around the call and a device synchronise.  Entropy: HIP events "
             "around stage 1, summed over the calls of a batch (one per kind of file).", "",
             "| set | largest interval (bytes) | Pillow wall | serial wall | sync wall | resume wall | serial entropy | sync entropy | resume entropy |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        e = r["entropy_ms"]
        lines.append(f"| {r['n']} x {r['set']} | {r['largest_interval_bytes']} | {f(r['host_wall_ms'])} | {f(r['serial_wall_ms'])} | {f(r['sync_wall_ms'])} | "
                     f"{f(r['resume_wall_ms'])} | {f(e['serial'])} | {f(e['sync'])} | {f(e['resume'])} |")
    lines += ["", "## Entropy stage over the distance of the points", "", "Each cell: the resume stage 1 (the serial stage 1 alternating with it), HIP events around the stage.", "",
              "| set | " + " | ".join(f"every {v}" for v in EVERY_SWEEP) + " |", "|---|" + "---|" * len(EVERY_SWEEP)]
    for r in rows:
        lines.append(f"| {r['set']} | " + " | ".join(f"{f(r['sweep_entropy_ms'][v]['resume'])} ({r['sweep_entropy_ms'][v]['serial'][0]:.2f})" for v in EVERY_SWEEP) + " |")
    lines += ["", "## The index", "", "Waves without an index, segments with one, build time (one thread, parse + plan + record) and size in the saved `.npz` per distinct file.", "",
              "| set | waves | " + " | ".join(f"segments / ms / bytes at {v}" for v in EVERY_SWEEP) + " |", "|---|---|" + "---|" * len(EVERY_SWEEP)]
    for r in rows:
        lines.append(f"| {r['set']} | {r['waves']} | " + " | ".join(f"{r['segments'][v]} / {r['index_build_ms_per_file'][v]:.2f} / {r['index_bytes_per_file'][v]:.0f}"
                                                                     for v in EVERY_SWEEP) + " |")
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
