"""Writes tests/golden/jpeg_prog_cases.npz: progressive JPEG files and what Pillow (``Image.open(f).convert("RGB")``) decodes them to -
the bytes ``hawq_amd.jpeg`` must reproduce with ``progressive=True`` - plus progressive files the device path must refuse.

    python tests/golden/make_jpeg_prog_cases.py

Most files are Pillow's own (``progressive=True``: its ten-scan script, six scans for grayscale; ``restart_marker_rows=1`` adds a DRI and
RSTn markers inside every scan).  The others carry the quantised coefficients of a baseline file of Pillow's under another scan script,
written by ``tests/jpeg_prog_model.write_progressive``; such a file is kept only if Pillow decodes it to the very bytes of the baseline
file, so a wrong writer cannot produce a fixture.

Archive: ``names``, ``jpeg_<name>`` / ``rgb_<name>`` per accepted case; ``refused_names``, ``refused_<name>``, ``refused_reasons``;
``conditions``: JSON of what the set was checked to contain, counted with tests/jpeg_prog_model.py (which is also checked against every
case here): the largest end-of-band run category, correction bits read inside an end-of-band run, ZRL symbols in refinement scans,
single-component scans whose grid is smaller than the slab's, the deepest level, the most restart intervals of a single-component scan;
``pillow``: version.
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

MODES = {"444": dict(subsampling=0), "422": dict(subsampling=1), "420": dict(subsampling=2), "gray": dict()}


def content(kind, w, h, rng):
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)], -1).astype(np.uint8)


def encode(img, mode, quality=90, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).convert("L" if mode == "gray" else "RGB").save(buf, "JPEG", quality=quality, **MODES[mode], **kw)
    return buf.getvalue()


def pillow_rgb(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB"))


def main():
    from hawq_amd.jpeg import parse_jpeg, scan_levels
    from tests import jpeg_model
    from tests import jpeg_prog_model as M

    rng = np.random.default_rng(2027)
    cases = {}
    for w, h in ((1, 1), (7, 9), (16, 16)):
        img = content("noise", w, h, rng)
        for mode in MODES:
            cases[f"noise_{w}x{h}_{mode}"] = encode(img, mode, progressive=True)
    for (w, h), mode in (((13, 17), "422"), ((33, 31), "420"), ((31, 33), "420"), ((65, 9), "444"), ((9, 65), "444")):
        cases[f"noise_{w}x{h}_{mode}"] = encode(content("noise", w, h, rng), mode, progressive=True)
    noise = content("noise", 40, 24, rng)
    for mode in MODES:
        cases[f"noise_40x24_{mode}_rst"] = encode(noise, mode, progressive=True, restart_marker_rows=1)
    cases["smooth_40x24_420"] = encode(content("smooth", 40, 24, rng), "420", progressive=True)
    cases["smooth_33x31_444"] = encode(content("smooth", 33, 31, rng), "444", progressive=True)
    cases["noise_40x24_420_q30"] = encode(noise, "420", quality=30, progressive=True)
    cases["noise_40x24_444_q100"] = encode(noise, "444", quality=100, progressive=True)
    board = ((np.indices((32, 32)).sum(0) & 1) * 255).astype(np.uint8)
    cases["checker_32x32_q30"] = encode(np.repeat(board[:, :, None], 3, 2), "444", quality=30, progressive=True)
    cases["flat_1024x1024_gray"] = encode(np.full((1024, 1024, 3), 77, np.uint8), "gray", progressive=True)

    # other scan scripts over the coefficients of baseline files
    expected = {}

    def rewritten(name, img, mode, script, quality=90):
        base = encode(img, mode, quality=quality)
        rec = parse_jpeg(base)
        data = M.write_progressive(rec, jpeg_model.coefficients(rec), script(rec.ncomp))
        assert np.array_equal(pillow_rgb(data), pillow_rgb(base)), name   # the writer is right, or the file is no fixture
        cases[name], expected[name] = data, pillow_rgb(base)

    noise33, smooth31 = content("noise", 33, 31, rng), content("smooth", 31, 33, rng)
    rewritten("spectral_33x31_420", noise33, "420", M.script_spectral)
    rewritten("spectral_9x65_gray", content("noise", 9, 65, rng), "gray", M.script_spectral)
    rewritten("deep_33x31_420", noise33, "420", M.script_deep)
    rewritten("deep_31x33_444_smooth", smooth31, "444", M.script_deep, quality=100)
    rewritten("tables_13x17_422", content("noise", 13, 17, rng), "422", lambda n: M.script_deep(n, tables=True, top=1))
    rewritten("dri_40x24_420", noise, "420", M.script_dri)
    rewritten("dri_40x24_gray", noise, "gray", M.script_dri)

    # refused
    refused = {}
    whole = cases["smooth_40x24_420"]
    refused["cut_last_scan"] = (whole[:whole.rindex(b"\xff\xda")] + b"\xff\xd9", "progression")
    refused["adobe"] = (whole[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + whole[2:], "Adobe marker")
    rec = parse_jpeg(encode(noise33, "420"))
    comps = jpeg_model.coefficients(rec)
    every = (0, 1, 2)
    dc = dict(comps=every, ss=0, se=0, ah=0, al=0)
    refused["two_components"] = (M.write_progressive(rec, comps, [dc, dict(comps=(1, 2), ss=0, se=0, ah=0, al=0)]), "scan of two components")
    refused["ac_before_dc"] = (M.write_progressive(rec, comps, [dict(comps=(0,), ss=1, se=63, ah=0, al=0), dc]), "progression")
    refused["ah_not_previous_al"] = (M.write_progressive(rec, comps, [dict(comps=every, ss=0, se=0, ah=0, al=2), dict(comps=every, ss=0, se=0, ah=1, al=0)]),
                                     "progression")
    many = [dc] + [dict(comps=(c,), ss=k, se=k, ah=0, al=0) for c in every for k in range(1, 64)]
    assert len(many) > 65
    refused["65_scans"] = (M.write_progressive(rec, comps, many[:65] + [dict(comps=(c,), ss=k, se=63, ah=0, al=0) for c, k in ((1, 2), (2, 1))]), "too many scans")

    out = {}
    stats = {}
    deepest = 0
    for name, data in cases.items():
        rgb = pillow_rgb(data)
        if name in expected:
            assert np.array_equal(rgb, expected[name]), name
        assert np.array_equal(M.decode(data, stats), rgb), name
        deepest = max(deepest, max(scan_levels(parse_jpeg(data, progressive=True).scans)))
        out["jpeg_" + name], out["rgb_" + name] = np.frombuffer(data, np.uint8), rgb
    cond = {"eob_category": stats["eob_category"], "corrections_in_eob_run": stats["corrections_in_eob_run"], "refine_zrl": stats["refine_zrl"],
            "narrower_grid": stats["narrower_grid"], "deepest_level": deepest, "own_grid_intervals": stats["own_grid_intervals"]}
    assert cond["eob_category"] == 14 and cond["corrections_in_eob_run"] > 0 and cond["refine_zrl"] > 0 and cond["narrower_grid"] > 0, cond
    assert cond["deepest_level"] >= 5 and cond["own_grid_intervals"] > 1, cond
    for name, (data, reason) in refused.items():
        out["refused_" + name] = np.frombuffer(data, np.uint8)
    path = os.path.join(HERE, "jpeg_prog_cases.npz")
    np.savez_compressed(path, names=np.array(list(cases)), refused_names=np.array(list(refused)), refused_reasons=np.array([r for _, r in refused.values()]),
                        conditions=np.array(json.dumps(cond)), pillow=np.array(PIL.__version__), **out)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases,", cond)


if __name__ == "__main__":
    main()
