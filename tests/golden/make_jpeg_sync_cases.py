"""Writes tests/golden/jpeg_sync_cases.npz: JPEG files without (or with few) restart markers, long enough for the many-lane entropy decoder
(``decode_jpeg_batch(entropy="sync")``), and what Pillow (``Image.open(f).convert("RGB")``) decodes them to.  Encoded
and decoded with Pillow alone; ``noise_64x48_444_tail`` is a Pillow file with 40 bytes put between its last block and EOI, which Pillow
(like the serial decoder) passes over.

    python tests/golden/make_jpeg_sync_cases.py

Archive: ``names``, ``jpeg_<name>`` / ``rgb_<name>`` per case, ``pillow``: version, ``conditions``: JSON of what the set was checked to
contain with tests/jpeg_sync_model.py at ``sub_bytes`` = 16 - the names of the cases that show each condition - and, per case and for
``sub_bytes`` 16 and 128, the sub-sequences ``n`` and the decode passes ``rounds`` of each restart interval.
"""
import json
import os
import sys

import numpy as np
import PIL

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_jpeg_cases import content, encode, pillow_rgb  # noqa: E402


def main():
    rng = np.random.default_rng(2027)
    cases = {}
    cases["noise_144x104_q95_420"] = encode(content("noise", 144, 104, rng), quality=95, subsampling=2)   # more than 1024 x 16 stream bytes
    cases["flat_320x240"] = encode(np.full((240, 320, 3), (200, 30, 90), np.uint8), quality=90)
    # smooth along x, a triangle of period 16 along y: every MCU row decodes alike, which keeps Pillow's RGB small in the archive
    y, x = np.mgrid[0:240, 0:320]
    tri = np.abs((y % 16) - 8) * 12
    cases["smooth_320x240_420"] = encode(np.stack([(x * 255) // 319, 40 + tri + x // 4, 255 - (x * 200) // 319 - tri // 2], -1).astype(np.uint8), quality=90, subsampling=2)
    small = content("noise", 64, 48, rng)
    cases["noise_64x48_444"] = encode(small, quality=90, subsampling=0)
    cases["noise_64x48_422"] = encode(small, quality=90, subsampling=1)
    cases["noise_96x96_gray"] = encode(content("noise", 96, 96, rng), "L", quality=90)
    cases["noise_64x48_opt"] = encode(small, quality=92, subsampling=2, optimize=True)
    cases["noise_64x48_q100"] = encode(small, quality=100, subsampling=2)
    cases["noise_96x64_rstrow"] = encode(content("noise", 96, 64, rng), quality=90, subsampling=2, restart_marker_rows=1)
    whole = cases["noise_64x48_444"]
    assert whole.endswith(b"\xff\xd9")
    cases["noise_64x48_444_tail"] = whole[:-2] + bytes(rng.integers(0, 255, 40).astype(np.uint8)) + whole[-2:]

    from hawq_amd.jpeg import parse_jpeg
    from tests import jpeg_model, jpeg_sync_model
    out, lanes = {}, {}
    shows = {k: [] for k in ("n_above_1024", "rounds_equal_n", "rounds_below_quarter_n", "boundary_on_stuffed_zero", "length_no_multiple", "start_inside_block",
                             "start_in_chroma", "bytes_behind_last_block", "restart_intervals_above_256")}
    for name, data in cases.items():
        rgb = pillow_rgb(data)
        rec = parse_jpeg(data)
        assert np.array_equal(jpeg_model.decode(data), rgb), name
        serial = jpeg_model.coefficients(rec)
        lanes[name] = {}
        for sub_bytes in (16, 128):
            assert all(np.array_equal(a, b) for a, b in zip(serial, jpeg_sync_model.coefficients(rec, sub_bytes))), (name, sub_bytes)
            s = jpeg_sync_model.summary(data, sub_bytes)
            lanes[name][str(sub_bytes)] = {"n": s["n"], "rounds": s["rounds"]}
            if sub_bytes == 16:
                for key in ("boundary_on_stuffed_zero", "length_no_multiple", "start_inside_block", "start_in_chroma", "bytes_behind_last_block"):
                    if s[key]:
                        shows[key].append(name)
                if max(s["n"]) > 1024:
                    shows["n_above_1024"].append(name)
                if any(r == n and n > 8 for r, n in zip(s["rounds"], s["n"])):
                    shows["rounds_equal_n"].append(name)
                if any(4 * r < n for r, n in zip(s["rounds"], s["n"])):
                    shows["rounds_below_quarter_n"].append(name)
        lengths = rec.intervals[:, 1] - rec.intervals[:, 0]
        if len(lengths) > 1 and lengths.min() > 256:
            shows["restart_intervals_above_256"].append(name)
        out["jpeg_" + name], out["rgb_" + name] = np.frombuffer(data, np.uint8), rgb
    missing = [k for k, v in shows.items() if not v]
    assert not missing, missing
    assert "flat_320x240" in shows["rounds_equal_n"] and "noise_144x104_q95_420" in shows["n_above_1024"], shows
    path = os.path.join(HERE, "jpeg_sync_cases.npz")
    np.savez_compressed(path, names=np.array(list(cases)), conditions=np.array(json.dumps({"shows": shows, "lanes": lanes})),
                        pillow=np.array(PIL.__version__), **out)
    size = os.path.getsize(path)
    print(path, size, "bytes,", len(cases), "cases")
    for name in cases:
        print(" ", name, len(cases[name]), "bytes", lanes[name])
    print(shows)
    assert size <= os.path.getsize(os.path.join(HERE, "jpeg_cases.npz")), size


if __name__ == "__main__":
    main()
