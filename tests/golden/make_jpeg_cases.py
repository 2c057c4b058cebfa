"""Writes tests/golden/jpeg_cases.npz: small JPEG files and what Pillow (``Image.open(f).convert("RGB")``) decodes them to - the bytes
the device decoder of hawq_amd.jpeg must reproduce - plus files the device path must refuse.  Encoded and decoded with Pillow alone.

    python tests/golden/make_jpeg_cases.py

Archive: ``names`` (accepted cases), ``jpeg_<name>`` / ``rgb_<name>`` per case; ``refused_names``, ``refused_<name>`` (file bytes),
``refused_reasons`` (what ``parse_jpeg`` must say), ``refused_rgb_<name>`` where Pillow can decode the file; ``conditions``: JSON of what
the set was checked to contain (counted with tests/jpeg_model.py, which is also checked against every case here: stuffed FF 00 bytes, ZRL
symbols, the longest Huffman code a stream really uses - the 16-bit codes come from the standard AC tables, the ``optimize=True`` cases
add custom tables -, files with two distinct quantisation tables, the most restart intervals of one file), ``pillow``: version.
"""
import io
import json
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SIZES = [(1, 1), (8, 8), (13, 17), (16, 16), (31, 33), (40, 23)]   # (width, height)
ENCODINGS = {
    "444": dict(quality=90, subsampling=0),
    "422": dict(quality=90, subsampling=1),
    "420": dict(quality=90, subsampling=2),
    "420rst": dict(quality=90, subsampling=2, restart_marker_blocks=1),
    "opt95": dict(quality=95, optimize=True),
    "q30": dict(quality=30),
    "gray": dict(quality=90),
}


def content(kind, w, h, rng):
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)], -1).astype(np.uint8)


def encode(img, mode="RGB", **kw):
    buf = io.BytesIO()
    Image.fromarray(img).convert(mode).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_rgb(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB"))


def main():
    rng = np.random.default_rng(2026)
    cases = {}
    for w, h in SIZES:
        for kind in ("noise", "smooth"):
            img = content(kind, w, h, rng)
            for name, kw in ENCODINGS.items():
                cases[f"{kind}_{w}x{h}_{name}"] = encode(img, "L" if name == "gray" else "RGB", **kw)
    cases["flat_24x24"] = encode(np.full((24, 24, 3), (200, 30, 90), np.uint8), quality=90)
    board = ((np.indices((32, 32)).sum(0) & 1) * 255).astype(np.uint8)
    cases["checker_32x32_q30"] = encode(np.repeat(board[:, :, None], 3, 2), quality=30)
    noise = content("noise", 40, 24, rng)
    cases["noise_40x24_q100"] = encode(noise, quality=100, subsampling=2)
    cases["noise_40x24_rst1"] = encode(noise, quality=85, subsampling=0, restart_marker_blocks=1)
    cases["noise_40x24_rst2"] = encode(noise, quality=85, subsampling=1, restart_marker_blocks=2)
    cases["noise_40x24_rst4"] = encode(noise, quality=85, subsampling=2, restart_marker_blocks=4)    # 6 MCUs: 4 does not divide them
    cases["noise_40x24_rst7_gray"] = encode(noise, "L", quality=85, restart_marker_blocks=7)          # 15 MCUs
    cases["noise_65x9_420"] = encode(content("noise", 65, 9, rng), quality=90, subsampling=2)

    refused = {}
    smooth = content("smooth", 40, 23, rng)
    refused["progressive"] = (encode(smooth, quality=90, progressive=True), "progressive (SOF2)")
    refused["cmyk"] = (encode(smooth, "CMYK", quality=90), "four components")
    buf = io.BytesIO()
    Image.fromarray(smooth).save(buf, "PNG")
    refused["png"] = (buf.getvalue(), "not a JPEG")
    whole = cases["smooth_40x23_444"]
    refused["cut_header"] = (whole[:whole.index(b"\xff\xc0") + 7], "truncated header")

    from hawq_amd.jpeg import parse_jpeg
    from tests import jpeg_model
    out, stats = {}, {"stuffed": 0, "zrl": 0, "longest_code": 0, "two_qtables": 0, "max_intervals": 0}
    for name, data in cases.items():
        rgb = pillow_rgb(data)
        s = {}
        assert np.array_equal(jpeg_model.decode(data, s), rgb), name
        rec = parse_jpeg(data)
        stats["stuffed"] += s["stuffed"]
        stats["zrl"] += s.get("zrl", 0)
        stats["longest_code"] = max(stats["longest_code"], s.get("longest_code", 0))
        stats["max_intervals"] = max(stats["max_intervals"], s["intervals"])
        stats["two_qtables"] += len({rec.qtables[c[3]].tobytes() for c in rec.components}) > 1
        out["jpeg_" + name], out["rgb_" + name] = np.frombuffer(data, np.uint8), rgb
    assert stats["stuffed"] > 0 and stats["zrl"] > 0 and stats["longest_code"] == 16 and stats["two_qtables"] > 0 and stats["max_intervals"] > 1, stats
    assert pillow_rgb(cases["checker_32x32_q30"]).min() == 0 and pillow_rgb(cases["checker_32x32_q30"]).max() == 255   # the range limit clips
    for name, (data, reason) in refused.items():
        out["refused_" + name] = np.frombuffer(data, np.uint8)
        try:
            out["refused_rgb_" + name] = pillow_rgb(data)
        except Exception:   # the cut file: Pillow refuses it too
            assert name == "cut_header", name
    path = os.path.join(HERE, "jpeg_cases.npz")
    np.savez_compressed(path, names=np.array(list(cases)), refused_names=np.array(list(refused)),
                        refused_reasons=np.array([r for _, r in refused.values()]), conditions=np.array(json.dumps(stats)),
                        pillow=np.array(PIL.__version__), **out)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases,", stats)


if __name__ == "__main__":
    main()
