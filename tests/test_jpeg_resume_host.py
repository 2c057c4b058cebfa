"""Host side of decoding JPEGs from recorded resume points (hawq_amd/jpeg.py ``build_resume_index`` / ``ResumeIndex`` /
``decode_jpeg_batch(resume=)``, hawq_jpeg_resume_record, hawq_jpeg_resume_ok, csrc/jpeg_resume.h) without a GPU: the
index and its file, which files of a batch take which call (a stub in place of the device call), the checker against hand-broken
segment tables, the planners without the option against the pinned blob bytes, and the recorder and the segment decoders the kernels
compile, built into a stand-alone program under AddressSanitizer + UBSan and run on valid, damaged and stale input."""
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import jpeg_model, jpeg_pins, jpeg_sync_model
from tests import jpeg_prog_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def baseline():
    """{name: file bytes} of jpeg_cases.npz and jpeg_sync_cases.npz"""
    both = {n: d for n, (d, _) in jpeg_model.cases()[0].items()}
    both.update({n: d for n, (d, _) in jpeg_sync_model.cases()[0].items()})
    return both


@functools.lru_cache(maxsize=None)
def progressive():
    return {n: d for n, (d, _) in M.cases()[0].items()}


def touched(data):
    """the file with one byte of its JFIF header changed (the pixel density): it decodes to the same pixels, and is another file"""
    assert data[6:10] == b"JFIF"
    return data[:15] + bytes([data[15] ^ 1]) + data[16:]


# ------------------------------------------------------------------------------------------------------------------ the index
def test_index_holds_points_every_so_many_bytes_and_the_fixtures_hold_the_hard_states():
    from hawq_amd.jpeg import build_resume_index, parse_jpeg
    files = list(progressive().values()) + [jpeg_model.cases()[1]["cmyk"][0], jpeg_model.cases()[1]["png"][0]]
    for every in (16, 64, 1024):
        idx = build_resume_index(files, every=every, progressive=True, workers=2 if every == 64 else 0)
        assert len(idx) == len(progressive()) and idx.every == every   # the refused files have no entry
        for name, data in progressive().items():
            rec = parse_jpeg(data, progressive=True)
            pts = idx.points(data, rec)
            assert pts.dtype == np.int32 and pts.shape[1] == 9, name
            for k, s in enumerate(rec.scans):
                for j, (first, last) in enumerate(s.intervals.tolist()):
                    p = pts[(pts[:, 0] == k) & (pts[:, 1] == j)]
                    at = np.concatenate(([first], p[:, 3]))
                    assert np.all(np.diff(at) >= every) and np.all(p[:, 3] <= last) and np.all(np.diff(p[:, 2]) > 0) and np.all(p[:, 2] > 0), (name, k, j)
                    assert np.all(p[:, 2] < (min(s.restart, s.units - j * s.restart) if s.restart else s.units)), (name, k, j)
                    assert np.all((p[:, 4] >= 0) & (p[:, 4] < 8)) and np.all((p[:, 5] >= 0) & (p[:, 5] < 32768))
                    if s.ss == 0:
                        assert not p[:, 5].any(), name
                    if s.ss > 0 or s.ah > 0:
                        assert not p[:, 6:].any(), name
                    if last - first < every:
                        assert len(p) == 0
        if every == 16:
            fine = idx
    pts = {n: fine.points(d, parse_jpeg(d, progressive=True)) for n, d in progressive().items()}
    # points inside an end-of-band run: in the noise files.  The flat 1024 x 1024 image has none - its AC scans are one run of two
    # bytes, and a point needs `every` bytes behind the one before - but 255 points in its two DC scans of one bit per block
    assert sum(int((p[:, 5] > 0).sum()) for p in pts.values()) > 20 and len(pts["flat_1024x1024_gray"]) > 200
    assert len(pts["noise_33x31_420"]) > 0 and len(pts["deep_33x31_420"]) > 0     # own grid narrower than the padded one; five levels
    assert len(pts["tables_13x17_422"]) > 0                                       # tables redefined between scans
    assert any(len(p) and p[:, 1].max() > 0 for p in pts.values())                # segments inside real restart intervals
    assert sum(int(p[:, 4].any()) for p in pts.values()) > 20                     # points inside a byte
    # without the option a progressive file has no entry; a baseline index knows the predictors of three components
    idx = build_resume_index(list(progressive().values())[:3] + [baseline()["noise_64x48_422"]], every=64)
    assert len(idx) == 1
    (_, p), = idx.entries.values()
    assert len(p) > 3 and p[:, 6].any() and p[:, 7].any() and p[:, 8].any() and not p[:, 0].any() and not p[:, 5].any()
    with pytest.raises(ValueError):
        build_resume_index([], every=0)


def test_save_and_load_give_the_same_index_from_plain_arrays(tmp_path):
    from hawq_amd.jpeg import ResumeIndex, build_resume_index
    files = [baseline()[n] for n in ("noise_64x48_422", "noise_96x64_rstrow", "smooth_8x8_gray")] + [progressive()[n] for n in ("deep_33x31_420", "noise_1x1_gray")]
    idx = build_resume_index(files, every=32, progressive=True)
    path = str(tmp_path / "points.npz")
    idx.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ["crc", "every", "length", "points", "progressive", "start"] and all(z[k].dtype != object for k in z.files)
    back = ResumeIndex.load(path)
    assert back.every == 32 and set(back.entries) == set(idx.entries) and len(back) == 5
    for key, (prog, pts) in idx.entries.items():
        assert back.entries[key][0] == prog and np.array_equal(back.entries[key][1], pts) and back.entries[key][1].dtype == np.int32
    empty = ResumeIndex(64)
    empty.save(path)
    assert len(ResumeIndex.load(path)) == 0
    np.savez(path, every=np.int32(8), length=np.zeros(2, np.int64), crc=np.zeros(2, np.uint32), progressive=np.zeros(2, np.uint8), start=np.array([0, 5, 3]),
             points=np.zeros((3, 9), np.int32))
    with pytest.raises(ValueError):
        ResumeIndex.load(path)


def test_a_changed_byte_or_the_other_kind_makes_the_entry_ignored():
    from hawq_amd.jpeg import build_resume_index, parse_jpeg
    data = baseline()["noise_40x24_rst4"]
    idx = build_resume_index([data, progressive()["noise_33x31_420"]], every=16, progressive=True)
    assert idx.points(data, parse_jpeg(data)) is not None
    assert idx.points(touched(data), parse_jpeg(touched(data))) is None and idx.points(data[:-1], parse_jpeg(data)) is None
    prog = progressive()["noise_33x31_420"]
    assert idx.points(prog, parse_jpeg(prog, progressive=True)) is not None and idx.points(prog, parse_jpeg(data)) is None


# ------------------------------------------------------------------------------------------------------------------ which file takes which call
def test_files_with_an_entry_take_the_resume_call_and_the_rest_go_as_before(monkeypatch):
    from hawq_amd import jpeg
    from hawq_amd.image import decode_image
    base, base_bad, _ = jpeg_model.cases()
    names = ["noise_31x33_420", "noise_40x24_rst4", "smooth_31x33_gray", "noise_13x17_422"]
    prog = ["noise_33x31_420", "deep_33x31_420", "noise_40x24_gray_rst"]
    srcs = [base[n][0] for n in names] + [progressive()[n] for n in prog] + [base_bad["cmyk"][0], touched(base["noise_40x24_rst2"][0])]
    # entries: two baseline files, one progressive file, and the file that has changed since
    idx = jpeg.build_resume_index([srcs[0], srcs[1], srcs[5], base["noise_40x24_rst2"][0]], every=16, progressive=True)
    assert len(idx) == 4
    calls = []

    def launch(records, out_offsets, out, dev, events=None, sync=None, info=None, resume=None):
        kind = "prog" if isinstance(records[0], jpeg.JpegProgRecord) else "base"
        if resume is not None:   # the plan of the call passes both checkers
            plan = jpeg.plan_jpeg_prog_batch(records, out_offsets, out.numel(), None, resume) if kind == "prog" else jpeg.plan_jpeg_batch(records, out_offsets, out.numel(),
                                                                                                                                          None, None, resume)
            assert plan.ok() and plan.resume_ok() and plan.n_segs > plan.n_waves
        for r, off in zip(records, out_offsets):
            rgb = M.pixels(r, M.coefficients(r)) if kind == "prog" else jpeg_model.decode(r.data)
            out[off:off + rgb.size] = torch.from_numpy(rgb.reshape(-1))
        calls.append((kind, resume is not None, sync, [srcs.index(r.data) for r in records]))
        return torch.zeros(len(records), dtype=torch.int32)

    monkeypatch.setattr(jpeg, "_launch", launch)
    for entropy, sync in (("serial", None), ("sync", (jpeg.SUB_BYTES, jpeg.MIN_SYNC_BYTES))):
        calls.clear()
        images, fallbacks = jpeg.decode_jpeg_batch(srcs, device="cpu", entropy=entropy, progressive=True, resume=idx)
        assert calls == [("prog", False, None, [4, 6]), ("prog", True, None, [5]), ("base", False, sync, [2, 3, 8]), ("base", True, None, [0, 1])]
        assert fallbacks == [(7, "four components")]
        for im, src in zip(images, srcs):
            assert torch.equal(im, decode_image(src))
    # without progressive=True the progressive file's entry is of no use; without an index nothing changes
    calls.clear()
    _, fallbacks = jpeg.decode_jpeg_batch(srcs, device="cpu", resume=idx)
    assert calls == [("base", False, None, [2, 3, 8]), ("base", True, None, [0, 1])] and [i for i, _ in fallbacks] == [4, 5, 6, 7]
    calls.clear()
    jpeg.decode_jpeg_batch(srcs, device="cpu", progressive=True, resume=None)
    assert calls == [("prog", False, None, [4, 5, 6]), ("base", False, None, [0, 1, 2, 3, 8])]
    from hawq_amd.image import folder_loader
    with pytest.raises(ValueError):   # the loader wants device_decode with it
        next(folder_loader(".", resume=idx))


# ------------------------------------------------------------------------------------------------------------------ planner and checker
def test_without_the_option_the_planners_write_the_pinned_bytes_and_with_it_the_table_stands_behind_them():
    from hawq_amd import jpeg
    with open(os.path.join(H.GOLDEN, "jpeg_front_end_planner.json")) as f:
        want = json.load(f)
    base, sync, prog = jpeg_pins._records()
    plain = jpeg.plan_jpeg_batch(list(base.values()), resume=None)
    assert type(plain) is jpeg.JpegPlan and jpeg_pins._plan_pin(plain) == want["base/all"]
    assert jpeg_pins._plan_pin(jpeg.plan_jpeg_batch(list(sync.values()), sync=(32, 4096), resume=None)) == want["sync32_4096/all"]
    plain_prog = jpeg.plan_jpeg_prog_batch(list(prog.values()), resume=None)
    assert type(plain_prog) is jpeg.JpegProgPlan and jpeg_pins._plan_pin(plain_prog) == want["prog/all"]
    some = [base[n] for n in ("noise_31x33_422", "noise_40x24_rst4", "smooth_31x33_gray", "noise_16x16_444")]
    assert jpeg_pins._plan_pin(jpeg.plan_jpeg_batch(some, [12288, 32, 8192, 4112], 20000, None, None, None)) == want["base/placed"]
    # with points: the same bytes, then the table
    for records, plain, planner in ((list(base.values()), plain, jpeg.plan_jpeg_batch), (list(prog.values()), plain_prog, jpeg.plan_jpeg_prog_batch)):
        points = [jpeg.record_resume_points(r, 16) for r in records]
        plan = planner(records, resume=points)
        assert plan.ok() and plan.resume_ok()
        assert plan.segs_off == plain.nbytes and np.array_equal(plan.blob[:plain.nbytes], plain.blob[:plain.nbytes])
        assert plan.n_segs == plan.n_waves + sum(len(p) for p in points) and plan.nbytes == (plan.segs_off + 40 * plan.n_segs + 15) // 16 * 16
    with pytest.raises(ValueError):
        jpeg.plan_jpeg_batch(some, sync=(32, 64), resume=[np.zeros((0, 9), np.int32)] * 4)


def _resume_plan(prog):
    from hawq_amd import jpeg
    if prog:
        names = ["noise_13x17_422", "noise_40x24_420_rst", "noise_7x9_gray", "deep_33x31_420", "dri_40x24_420", "flat_1024x1024_gray"]   # the last: a long DC refinement
        records = [jpeg.parse_jpeg(progressive()[n], progressive=True) for n in names]
        return jpeg.plan_jpeg_prog_batch(records, resume=[jpeg.record_resume_points(r, 16) for r in records]), records
    names = ["noise_31x33_420", "noise_40x24_rst4", "smooth_31x33_gray", "noise_64x48_422"]
    records = [jpeg.parse_jpeg(baseline()[n]) for n in names]
    return jpeg.plan_jpeg_batch(records, resume=[jpeg.record_resume_points(r, 16) for r in records]), records


@pytest.mark.parametrize("prog", [False, True], ids=["baseline", "progressive"])
def test_checker_refuses_every_clause_by_one_hand_broken_table_each(prog):
    from hawq_amd import _lib
    lib = _lib.load()
    plan, records = _resume_plan(prog)
    seg_dt = np.dtype(_lib.JpegResumeSeg)
    assert seg_dt.itemsize == 40 and plan.ok() and plan.resume_ok()
    segs0 = plan.blob[plan.segs_off:plan.segs_off + 40 * plan.n_segs].view(seg_dt).copy()
    waves = plan.blob[plan.wave_off:plan.wave_off + 8 * plan.n_waves].view(np.int32).reshape(-1, 2) if prog else None
    refused = 0

    def ok(blob, segs_off=plan.segs_off, n_segs=plan.n_segs, nbytes=plan.nbytes):
        return bool(lib.hawq_jpeg_resume_ok(blob.ctypes.data, nbytes, int(prog), segs_off, n_segs))

    def broken(why, k, field, value, c=None):
        nonlocal refused
        blob = plan.blob[:plan.nbytes].copy()
        segs = blob[plan.segs_off:plan.segs_off + 40 * plan.n_segs].view(seg_dt)
        if c is None:
            segs[field][k] = value
        else:
            segs[field][k][c] = value
        assert not ok(blob), (why, k, field, value)
        assert lib.hawq_last_error().decode().startswith("hawq_jpeg_resume_ok: ") and any(w in lib.hawq_last_error().decode() for w in why.split("|")), (why, lib.hawq_last_error())
        refused += 1

    head = segs0["unit0"] == 0
    later = int(np.flatnonzero(~head)[0])                       # a segment that is not its interval's first ...
    mid = int(np.flatnonzero(~head[:-1] & ~head[1:])[0])         # ... and one with a successor in the same interval
    last = int(np.flatnonzero(~head[:-1] & head[1:])[0])         # the last segment of an interval that has several
    first = int(np.flatnonzero(head[:-1] & ~head[1:])[0])        # the first segment of such an interval
    # the segments of an interval partition its units in order
    broken("partition", mid, "unit0", segs0["unit0"][mid] + 1)
    broken("partition", mid, "n_units", 0)
    broken("partition", mid, "n_units", -1)
    broken("partition", last, "n_units", segs0["n_units"][last] - 1)
    broken("partition", last, "n_units", segs0["n_units"][last] + 1)
    broken("partition", first, "n_units", 1 << 30)
    broken("partition", later, "unit0", 0)
    # the first segment: the interval's first byte, bit 0, zero state
    broken("first segment", first, "byte", segs0["byte"][first] + 1)
    broken("first segment", first, "bit", 1)
    broken("first segment", first, "eobrun", 1)
    for c in range(3):
        broken("first segment", first, "pred", 1, c)
    # a later one: a byte inside the interval and not before its predecessor's, bit 0..7, eobrun 0..32767
    broken("outside its interval", later, "byte", 1 << 30)
    broken("outside its interval", later, "byte", -1)
    broken("before its predecessor", mid + 1, "byte", segs0["byte"][mid] - 1)
    for v in (-1, 8):
        broken("bit outside", later, "bit", v)
    for v in (-1, 32768):
        broken("eobrun outside", later, "eobrun", v)
    # eobrun only in an AC scan, predictors only in a baseline image or a first DC pass, and only of components that are there
    if prog:
        scans = plan.blob[plan.scan_off:plan.scan_off + plan.n_scans * np.dtype(_lib.JpegScan).itemsize].view(np.dtype(_lib.JpegScan))
        of = scans[waves[segs0["wave"], 0]]
        dc_first, dc_refine, ac = (~head) & (of["ss"] == 0) & (of["ah"] == 0), (~head) & (of["ss"] == 0) & (of["ah"] > 0), (~head) & (of["ss"] > 0)
        assert dc_first.any() and dc_refine.any() and ac.any()
        broken("no AC scan", int(np.flatnonzero(dc_first)[0]), "eobrun", 1)
        broken("no AC scan", int(np.flatnonzero(dc_refine)[0]), "eobrun", 1)
        for c in range(3):
            broken("no first DC pass", int(np.flatnonzero(dc_refine)[0]), "pred", 1, c)
            broken("no first DC pass", int(np.flatnonzero(ac)[0]), "pred", -1, c)
        one = int(np.flatnonzero(dc_first & (of["ncomp"] == 1))[0])
        broken("does not have", one, "pred", 1, 1)
        broken("does not have", one, "pred", 1, 2)
        fine = plan.blob[:plan.nbytes].copy()   # what IS allowed there
        fine[plan.segs_off:plan.segs_off + 40 * plan.n_segs].view(seg_dt)["eobrun"][int(np.flatnonzero(ac)[0])] = 32767
        fine[plan.segs_off:plan.segs_off + 40 * plan.n_segs].view(seg_dt)["pred"][one][0] = -5
        assert ok(fine)
    else:
        broken("no AC scan", later, "eobrun", 1)
        gray = int(np.flatnonzero(~head & (segs0["wave"] == sum(len(r.intervals) for r in records[:2])))[0])   # image 2 has one component
        broken("does not have", gray, "pred", 1, 1)
        broken("does not have", gray, "pred", 1, 2)
    # the table itself: inside the blob, aligned, a segment or more per wave, in the order of the wave list
    blob = plan.blob[:plan.nbytes].copy()
    assert ok(blob)
    for off, n in ((plan.segs_off + 8, plan.n_segs - 1), (plan.segs_off + 16, plan.n_segs), (-16, plan.n_segs), (0, plan.n_segs), (1 << 40, plan.n_segs),
                   (plan.segs_off, plan.n_waves - 1), (plan.segs_off, plan.n_segs - 1), (plan.segs_off, plan.n_segs + 1), (plan.segs_off, 1 << 40)):
        assert not ok(blob, off, n), (off, n)
        refused += 1
    assert not ok(blob, nbytes=plan.nbytes - 16)
    broken("wave list|partition", later, "wave", segs0["wave"][later] + 1)
    broken("wave list|partition", plan.n_segs - 1, "wave", plan.n_waves)
    broken("wave list", 0, "wave", -1)
    assert refused >= 30 and ok(plan.blob[:plan.nbytes].copy())


def test_recorder_refuses_a_blob_its_checker_refuses_and_a_table_without_room():
    from hawq_amd import _lib, jpeg
    import ctypes as C
    lib = _lib.load()
    rec = jpeg.parse_jpeg(baseline()["noise_64x48_422"])
    plan = jpeg.plan_jpeg_batch([rec])
    segs, n = np.zeros(4, np.dtype(_lib.JpegResumeSeg)), C.c_int64(0)
    assert lib.hawq_jpeg_resume_record(plan.blob.ctypes.data, plan.nbytes, 0, 16, segs.ctypes.data, 4, C.byref(n)) != 0 and n.value > 4
    assert b"room for 4" in lib.hawq_last_error() and not segs["n_units"][3:].any()
    assert lib.hawq_jpeg_resume_record(plan.blob.ctypes.data, plan.nbytes, 0, 0, segs.ctypes.data, 4, C.byref(n)) != 0
    assert lib.hawq_jpeg_resume_record(plan.blob.ctypes.data, plan.nbytes, 1, 16, segs.ctypes.data, 4, C.byref(n)) != 0   # not a progressive blob
    bad = plan.blob[:plan.nbytes].copy()
    bad[:16].view(np.int32)[1] += 1
    assert lib.hawq_jpeg_resume_record(bad.ctypes.data, plan.nbytes, 0, 16, segs.ctypes.data, 4, C.byref(n)) != 0


# ------------------------------------------------------------------------------------------------------------------ the kernels' text on the host
@functools.lru_cache(maxsize=None)
def _host_check(tmp):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = os.path.join(tmp, "jpeg_resume_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tools", "jpeg_resume_host_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    return exe


@pytest.mark.parametrize("kind", ["base", "prog"])
def test_recorder_and_segment_decoders_on_the_host_under_sanitizers(tmp_path_factory, kind):
    """tools/jpeg_resume_host_check.cpp: csrc/jpeg_resume.h - the recorder of the library and the segment decoders of both entropy kernels
    - built with ASan + UBSan into a program of its own and run as a child process on the planner's blob of ALL fixtures of the kind, at
    every = 16, 64 and 1024: every point is the straight decoder's state, the segments in reverse order give the serial slab and status,
    so do the segments recorded from every stream cut at each eighth byte and with 200 seeded overwrites, and the good file's points on
    the damaged bytes end with a status or a clean result - all without a sanitizer report."""
    from hawq_amd import jpeg
    exe = _host_check(str(tmp_path_factory.getbasetemp()))
    if kind == "prog":
        records = [jpeg.parse_jpeg(d, progressive=True) for d in progressive().values()]
        plan = jpeg.plan_jpeg_prog_batch(records)
        scans = plan.n_scans
    else:
        records = [jpeg.parse_jpeg(d) for d in baseline().values()]
        plan = jpeg.plan_jpeg_batch(records)
        scans = len(records)
    assert plan.ok()
    tmp = tmp_path_factory.mktemp(kind)
    plan.blob[:plan.nbytes].tofile(str(tmp / "blob.bin"))
    r = subprocess.run([exe, kind, str(tmp / "blob.bin"), str(M.HOST_CHECK_SEED)], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    words = r.stdout.split()
    counts = dict(zip(words[0::2], map(int, words[1::2])))
    assert counts["images"] == len(records) and counts["bad"] == 0
    assert counts["points"] > 1000 and counts["points_bit"] > 100 and counts["segments"] >= counts["points"] + 3 * plan.n_waves
    assert (counts["points_eobrun"] > 0) == (kind == "prog")
    assert counts["damaged"] == counts["stale"] == counts["cuts"] + 3 * 200 * scans and counts["cuts"] > scans
    assert counts["damaged_flagged"] > counts["cuts"] // 2 and 0 < counts["stale_flagged"]
