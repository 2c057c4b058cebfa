"""Host side of the one-launch batched Resize + CenterCrop (hawq_amd/csrc/image_batch.hip, hawq_amd.image.plan_batch): the entry
points exist in the header, the ctypes table and the library; ``plan_batch`` cuts every image into tiles that cover the crop exactly
once, fit the LDS budget and read only inside the image, with the coefficient slices of ``bilinear_coeffs``; ``hawq_image_batch_ok``
accepts those tables and refuses damaged ones with a message; the threaded decode stage keeps the serial order.  No GPU: ``_ok``
launches nothing and ``hawq_image_batch`` is never called here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESIZE, CROP = 40, 32
# landscape, portrait, square, one axis equal to resize (x2), both equal, up-scaling, 30x down-scale
SIZES = [(50, 67), (67, 50), (53, 53), (40, 61), (61, 40), (40, 40), (30, 37), (1200, 1200)]


def _ok(plan, desc=None, tiles=None, n_tiles=None, coef_words=None, crop=None, lds_bytes=None):
    """hawq_image_batch_ok on the plan's tables with single arguments replaced -> (verdict, message)"""
    from hawq_amd import _lib
    lib = _lib.load()
    tiles = plan.tiles if tiles is None else tiles
    r = lib.hawq_image_batch_ok(plan.desc if desc is None else desc, len(plan.desc), tiles, len(tiles) if n_tiles is None else n_tiles,
                                plan.coef.ctypes.data, plan.coef.size if coef_words is None else coef_words,
                                plan.crop if crop is None else crop, plan.lds_bytes if lds_bytes is None else lds_bytes)
    return r, lib.hawq_last_error().decode()


def _copy(arr):
    out = type(arr)()
    C.memmove(out, arr, C.sizeof(arr))
    return out


def _band(image, h, w, r0, n, resize=RESIZE, crop=CROP):
    """input rows [y0, y1) the crop rows r0 .. r0+n-1 read, straight from bilinear_coeffs"""
    oh, ow, top, left = image.resize_crop_geometry(h, w, resize, crop)
    if oh == h:
        return top + r0, top + r0 + n
    b = image.bilinear_coeffs(h, oh)[0][top + r0: top + r0 + n]
    return int(b[:, 0].min()), int((b[:, 0] + b[:, 1]).max())


def test_entry_points_are_declared_bound_and_exported():
    from hawq_amd import _lib
    header = open(os.path.join(ROOT, "include", "hawq_mi355.h")).read()
    assert re.search(r"int hawq_image_batch\(const hawq_image_desc \*desc, int32_t n_images, const hawq_image_tile \*tiles, int32_t n_tiles, "
                     r"const int32_t \*coef,\s+uint8_t \*out, int32_t crop, int32_t lds_bytes, void \*stream\);", header)
    assert re.search(r"int hawq_image_batch_ok\(const hawq_image_desc \*host_desc, int32_t n_images, const hawq_image_tile \*host_tiles, "
                     r"int32_t n_tiles,\s+const int32_t \*host_coef, int64_t coef_words, int32_t crop, int32_t lds_bytes\);", header)
    assert re.search(r"int hawq_image_batch_lds_budget\(void\);", header)
    assert len(_lib.SIGNATURES["hawq_image_batch"]) == 9 and len(_lib.SIGNATURES["hawq_image_batch_ok"]) == 8
    assert _lib.SIGNATURES["hawq_image_batch_lds_budget"] == []
    lib = _lib.load()
    for name in ("hawq_image_batch", "hawq_image_batch_ok", "hawq_image_batch_lds_budget"):
        assert hasattr(lib, name)
    assert 0 < lib.hawq_image_batch_lds_budget() <= 65536


def test_ctypes_mirrors_match_the_header_layout(tmp_path):
    """hawq_image_desc / hawq_image_tile against the C compiler's own layout of the header: size and the offset of every field"""
    import subprocess
    from hawq_amd import _lib
    structs = {"hawq_image_desc": _lib.ImageDesc, "hawq_image_tile": _lib.ImageTile}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "hawq_mi355.h")}"', 'int main(void) {']
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ['return 0; }']))
    subprocess.check_call(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    header = open(os.path.join(ROOT, "include", "hawq_mi355.h")).read()
    for cname, cls in structs.items():   # and the header declares no member the mirror lacks
        body = header[header.index(f"typedef struct {cname} {{"):header.index(f"}} {cname};")]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        members = [m for decl in re.findall(r"(?:uint64_t|int32_t) ([^;]+);", body) for m in decl.replace(" ", "").split(",")]
        assert members == [f for f, _ in cls._fields_], cname


def test_plan_tiles_cover_the_crop_fit_the_budget_and_read_inside_the_image():
    from hawq_amd import _lib, image
    budget = _lib.load().hawq_image_batch_lds_budget()
    plan = image.plan_batch(SIZES, RESIZE, CROP)
    assert plan.fallback == [] and len(plan.desc) == len(SIZES) and 0 < plan.lds_bytes <= budget
    pitch = image.band_pitch(CROP)
    assert pitch == 96 and image.band_pitch(31) == 96 and image.band_pitch(299) == 900
    rows_of = {i: [] for i in range(len(SIZES))}
    for t in plan.tiles:
        rows_of[t.image] += list(range(t.row0, t.row0 + t.rows))
        assert 1 <= t.rows <= image.MAX_TILE_ROWS
    worst = 0
    for i, (h, w) in enumerate(SIZES):
        assert rows_of[i] == list(range(CROP)), (h, w)                      # a partition of 0..crop, in order
        d = plan.desc[i]
        oh, ow, top, left = image.resize_crop_geometry(h, w, RESIZE, CROP)
        assert (d.h, d.w, d.oh, d.ow, d.top, d.left, d.skip_h, d.skip_v) == (h, w, oh, ow, top, left, int(ow == w), int(oh == h))
        for t in (t for t in plan.tiles if t.image == i):
            y0, y1 = _band(image, h, w, t.row0, t.rows)
            assert 0 <= y0 < y1 <= h and (y1 - y0) * pitch <= plan.lds_bytes   # rows read lie inside the image, the band inside the LDS
            worst = max(worst, (y1 - y0) * pitch)
        # packed bounds / coefficients == the slices of bilinear_coeffs; columns read lie inside the image
        for skip, b_off, c_off, k, size, out_size, lo in ((d.skip_h, d.hb_off, d.hc_off, d.kh, w, ow, left), (d.skip_v, d.vb_off, d.vc_off, d.kv, h, oh, top)):
            if skip:
                assert lo + CROP <= size
                continue
            b, c, ks = image.bilinear_coeffs(size, out_size)
            assert k == ks
            assert np.array_equal(plan.coef[b_off:b_off + 2 * CROP].reshape(CROP, 2), b[lo:lo + CROP])
            assert np.array_equal(plan.coef[c_off:c_off + k * CROP].reshape(CROP, k), c[lo:lo + CROP])
            assert b[lo:lo + CROP, 0].min() >= 0 and (b[lo:lo + CROP, 0] + b[lo:lo + CROP, 1]).max() <= size
    assert plan.lds_bytes == worst
    assert plan.coef.dtype == np.int32
    assert _ok(plan)[0] == 1 and plan.ok()
    assert max(t.rows for t in plan.tiles if t.image == 0) == 16
    # two images of one size share their coefficient slices
    twice = image.plan_batch([(50, 67), (50, 67), (67, 50)], RESIZE, CROP)
    assert twice.desc[0].hb_off == twice.desc[1].hb_off and twice.desc[0].vc_off == twice.desc[1].vc_off and twice.ok()
    assert twice.coef.size < image.plan_batch([(50, 67), (51, 67), (67, 50)], RESIZE, CROP).coef.size


def test_rows_per_tile_are_the_most_the_budget_holds():
    """Per image: the largest n <= 16 whose worst band over every start row fits, by brute force from bilinear_coeffs; with a small
    budget tiles shrink to one row (the last tile of an image may be shorter than the others) and over-budget images fall back."""
    from hawq_amd import image
    pitch = image.band_pitch(CROP)
    for budget in (None, 20 * pitch, 7 * pitch, 4 * pitch, 3 * pitch):
        plan = image.plan_batch(SIZES, RESIZE, CROP, lds_budget=budget)
        cap = 65536 if budget is None else budget
        for i, (h, w) in enumerate(SIZES):
            want = 0
            for n in range(1, min(16, CROP) + 1):
                if max(y1 - y0 for y0, y1 in (_band(image, h, w, r0, n) for r0 in range(CROP - n + 1))) * pitch <= cap:
                    want = n
            tiles = [t for t in plan.tiles if t.image == i]
            if want == 0:
                assert i in plan.fallback and not tiles and (plan.desc[i].h, plan.desc[i].w) == (0, 0)
                continue
            assert i not in plan.fallback
            assert [t.rows for t in tiles[:-1]] == [want] * (len(tiles) - 1) and 1 <= tiles[-1].rows <= want
            assert sum(t.rows for t in tiles) == CROP
        assert plan.lds_bytes <= cap and plan.ok()
    small = image.plan_batch(SIZES, RESIZE, CROP, lds_budget=3 * pitch)
    assert small.fallback == [SIZES.index((1200, 1200))]
    assert {t.rows for t in small.tiles if t.image in (0, 1, 2)} == {1}          # 50 -> 40: one output row reads three input rows
    assert [t.rows for t in small.tiles if t.image == 5] == [3] * 10 + [2]       # both passes skipped: a band row per output row; a short last tile
    with pytest.raises(ValueError):
        image.plan_batch(SIZES, RESIZE, CROP, lds_budget=65537)


def test_ok_refuses_damaged_tables_with_a_message():
    from hawq_amd import _lib, image
    plan = image.plan_batch(SIZES, RESIZE, CROP)
    assert _ok(plan) == (1, _ok(plan)[1])
    last = len(plan.tiles) - 1

    tiles = _copy(plan.tiles)            # a tile past the crop
    tiles[last].rows += 1
    r, msg = _ok(plan, tiles=tiles)
    assert r == 0 and "outside the crop" in msg

    tiles = _copy(plan.tiles)            # a gap: the second tile of image 0 starts one row late
    tiles[1].row0 += 1
    tiles[1].rows -= 1
    r, msg = _ok(plan, tiles=tiles)
    assert r == 0 and "gap or overlap" in msg

    tiles = _copy(plan.tiles)            # an overlap: it starts one row early
    tiles[1].row0 -= 1
    r, msg = _ok(plan, tiles=tiles)
    assert r == 0 and "gap or overlap" in msg

    r, msg = _ok(plan, n_tiles=last)     # the last image's last rows uncovered
    assert r == 0 and "gap" in msg

    for field in ("hb_off", "hc_off", "vb_off", "vc_off"):   # an offset outside the coefficient table
        desc = _copy(plan.desc)
        setattr(desc[0], field, plan.coef.size - 3)
        r, msg = _ok(plan, desc=desc)
        assert r == 0 and "outside the coefficient table" in msg, field
    r, msg = _ok(plan, coef_words=plan.coef.size - 1)
    assert r == 0 and "outside the coefficient table" in msg

    r, msg = _ok(plan, lds_bytes=_lib.load().hawq_image_batch_lds_budget() + 1)   # lds_bytes above the budget
    assert r == 0 and "LDS budget" in msg
    r, msg = _ok(plan, lds_bytes=plan.lds_bytes - 1)                              # a band larger than lds_bytes
    assert r == 0 and "does not fit lds_bytes" in msg

    desc = _copy(plan.desc)              # the crop window outside the resized image
    desc[0].left = desc[0].ow - CROP + 1
    r, msg = _ok(plan, desc=desc)
    assert r == 0 and "crop window" in msg
    desc = _copy(plan.desc)              # a skipped pass whose window leaves the input
    desc[5].top = 9
    r, msg = _ok(plan, desc=desc)
    assert r == 0 and "crop window" in msg

    desc = _copy(plan.desc)              # bounds that read past the image: image 0's taps applied to a narrower image
    desc[0].w = 30
    r, msg = _ok(plan, desc=desc)
    assert r == 0 and "outside the input size" in msg

    desc = _copy(plan.desc)              # a tile on an image the launch leaves alone
    desc[0].h = desc[0].w = 0
    r, msg = _ok(plan, desc=desc)
    assert r == 0 and "empty descriptor" in msg
    assert _ok(plan)[0] == 1             # the plan itself was never touched


def test_too_small_image_raises():
    from hawq_amd import image
    with pytest.raises(ValueError, match="too small for the crop"):
        image.plan_batch([(50, 67), (10, 200)], 30, 32)


def test_threaded_decode_stage_keeps_the_serial_order():
    """decoded_batches: batches, files within a batch and labels in the order of `samples`, whatever the number of workers; never more
    than the current and the next batch handed to the decoder."""
    import threading
    from hawq_amd import image
    samples = [(f"f{i}", i % 3) for i in range(11)]
    serial = list(image.decoded_batches(samples, 4, 0, decode=lambda p: p.upper()))
    assert [b for b, _ in serial] == [["F0", "F1", "F2", "F3"], ["F4", "F5", "F6", "F7"], ["F8", "F9", "F10"]]
    assert [t for _, t in serial] == [[0, 1, 2, 0], [1, 2, 0, 1], [2, 0, 1]]
    seen, lock = [], threading.Lock()

    def decode(p):
        with lock:
            seen.append(p)
        return p.upper()
    handed = []
    for k, batch in enumerate(image.decoded_batches(samples, 4, 4, decode=decode)):
        handed.append(batch)
        with lock:
            assert set(seen) <= {f"f{i}" for i in range(min(11, 4 * (k + 2)))}   # one batch ahead, no more
    assert handed == serial and sorted(seen) == sorted(p for p, _ in samples)
    assert list(image.decoded_batches(samples, 4, 99, decode=lambda p: p.upper())) == serial   # clamped to 16 threads
    assert list(image.decoded_batches([], 4, 2)) == []


def test_folder_decode_stage_with_workers_equals_the_serial_one(tmp_path):
    pytest.importorskip("PIL")
    import torch
    from PIL import Image
    from hawq_amd import image
    rng = np.random.default_rng(5)
    for c in ("n01", "n02", "n03"):
        (tmp_path / c).mkdir()
        for k in range(3):
            h, w = (int(v) for v in rng.integers(40, 90, 2))
            Image.fromarray(rng.integers(0, 256, (h, w, 3)).astype(np.uint8)).save(tmp_path / c / f"im{k}.jpg", quality=90)
    samples, classes = image.image_folder(str(tmp_path))
    assert classes == ["n01", "n02", "n03"] and len(samples) == 9
    serial = list(image.decoded_batches(samples, 4))
    pooled = list(image.decoded_batches(samples, 4, workers=4))
    assert [t for _, t in pooled] == [t for _, t in serial] == [[0, 0, 0, 1], [1, 1, 2, 2], [2]]
    for (a, _), (b, _) in zip(serial, pooled):
        assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
