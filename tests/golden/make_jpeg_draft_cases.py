"""Writes tests/golden/jpeg_draft_cases.npz: small JPEG files and what Pillow decodes them to in draft mode
(``im.draft("RGB", size); im.convert("RGB")``: libjpeg's DCT-domain scaling to 1/2, 1/4, 1/8) - the bytes the reduced-size device decode
of hawq_amd.jpeg (``draft=``) must reproduce.  Encoded and decoded with Pillow alone.

    python tests/golden/make_jpeg_draft_cases.py

Archive: ``names``; per case ``jpeg_<name>`` (file bytes) and, for every scale s of 2, 4, 8 that does not exceed the short side,
``draft_<name>_<s>`` (the requested (width, height)) and ``rgb_<name>_<s>`` (Pillow's RGB after that draft); ``conditions``: JSON of what
the set was checked to contain; ``pillow``: version.  Names say height x width.
"""
import io
import json
import os

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))

SIZES = [(16, 16), (17, 33), (40, 24), (65, 9), (33, 47), (16, 40), (8, 5), (8, 6), (16, 4), (31, 8), (9, 20), (64, 64)]   # (height, width)
SAMPLING = {"444": 0, "422": 1, "420": 2}
CONTENTS = {"noise": 90, "smooth": 30, "block": 100}   # content -> quality
SCALES = (2, 4, 8)


def content(kind, h, w, rng):
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "block":   # 8 x 8 squares of 0 and 255: a reduced block is one flat value, at either end of the range limit
        return np.repeat(((((x // 8) + (y // 8) + 1) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
    return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)], -1).astype(np.uint8)


def encode(img, mode="RGB", **kw):
    buf = io.BytesIO()
    Image.fromarray(img).convert(mode).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_draft(data, size):
    """(size after the draft, RGB)"""
    with Image.open(io.BytesIO(data)) as im:
        im.draft("RGB", size)
        return im.size, np.array(im.convert("RGB"))


def main():
    rng = np.random.default_rng(2027)
    files = {}
    for h, w in SIZES:
        for kind, quality in CONTENTS.items():
            img = content(kind, h, w, rng)
            for name, sub in SAMPLING.items():
                files[f"{kind}_{h}x{w}_{name}"] = encode(img, quality=quality, subsampling=sub)
    n_colour = len(files)
    noise = content("noise", 40, 24, rng)
    files["noise_17x33_gray"] = encode(content("noise", 17, 33, rng), "L", quality=90)
    files["smooth_40x24_gray"] = encode(content("smooth", 40, 24, rng), "L", quality=30)
    files["block_64x64_gray"] = encode(content("block", 64, 64, rng), "L", quality=100)
    files["noise_40x24_420_rst"] = encode(noise, quality=85, subsampling=2, restart_marker_rows=1)
    files["noise_33x47_gray_rst"] = encode(content("noise", 33, 47, rng), "L", quality=85, restart_marker_rows=1)
    files["noise_33x47_420_prog"] = encode(content("noise", 33, 47, rng), quality=90, subsampling=2, progressive=True)
    files["smooth_40x24_422_prog"] = encode(content("smooth", 40, 24, rng), quality=60, subsampling=1, progressive=True)

    out = {}
    cond = {"files": len(files), "colour_files": n_colour, "decodes": 0, "off_grid": 0,
            "zero": {str(s): 0 for s in SCALES}, "full": {str(s): 0 for s in SCALES},
            "narrow_422": {str(s): 0 for s in (2, 4)}, "wide_422": {str(s): 0 for s in (2, 4)}}
    for name, data in files.items():
        out["jpeg_" + name] = np.frombuffer(data, np.uint8)
        with Image.open(io.BytesIO(data)) as im:
            w, h = im.size
        assert f"_{h}x{w}_" in name, name
        for s in SCALES:
            if s > min(h, w):
                continue
            size = (w // s, h // s)
            got, rgb = pillow_draft(data, size)
            assert got == (-(-w // s), -(-h // s)) and rgb.shape == (got[1], got[0], 3), (name, s, got)   # the request yields the intended scale
            out[f"draft_{name}_{s}"], out[f"rgb_{name}_{s}"] = np.array(size, np.int32), rgb
            cond["decodes"] += 1
            cond["off_grid"] += bool(h % (8 * s) or w % (8 * s))
            cond["zero"][str(s)] += bool((rgb == 0).any())
            cond["full"][str(s)] += bool((rgb == 255).any())
            if name.endswith("_422") and s in (2, 4):
                cw = -(-w * (8 // s) // 16)   # samples of a reduced chroma row
                cond["narrow_422" if cw <= 2 else "wide_422"][str(s)] += 1
    assert n_colour == 108 and cond["off_grid"] > 0
    assert all(v > 0 for k in ("zero", "full", "narrow_422", "wide_422") for v in cond[k].values()), cond
    path = os.path.join(HERE, "jpeg_draft_cases.npz")
    np.savez_compressed(path, names=np.array(list(files)), conditions=np.array(json.dumps(cond)), pillow=np.array(PIL.__version__), **out)
    print(path, os.path.getsize(path), "bytes,", len(files), "files,", cond)


if __name__ == "__main__":
    main()
