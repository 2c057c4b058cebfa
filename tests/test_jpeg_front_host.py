"""The device front end of the JPEG decoder (csrc/jpeg_front.h + jpeg_front.hip, hawq_amd.jpeg ``front_end="device"``)
without a GPU: the host twin of the scan kernel against ``parse_jpeg`` on the fixtures and on the mutation corpus of tests/jpeg_pins.py,
the numpy layout against ``plan_jpeg_batch``, the checker of the fill, the bookkeeping of ``decode_jpeg_batch`` with stubs in place of
the device calls, and the walker's own text under AddressSanitizer + UBSan in a program of its own."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import jpeg_front_corpus as F
from tests import jpeg_model, jpeg_prog_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(data):
    from hawq_amd.jpeg import UnsupportedJpeg, parse_jpeg
    try:
        return parse_jpeg(data)
    except UnsupportedJpeg:
        return None


def _accepted_fixtures():
    good, _, _ = jpeg_model.cases()
    return list(good) + ["sample"], [good[n][0] for n in good] + [jpeg_model.sample()]


def test_twin_accepts_every_accepted_fixture_with_the_fields_of_the_python_parser():
    from hawq_amd.jpeg import front_scan_host
    names, datas = _accepted_fixtures()
    assert len(names) >= 92 + 1
    info = front_scan_host(datas)
    wrong = {n: why for n, d, o in zip(names, datas, info) for why in [F.record_mismatch(d, o, _parse(d))] if why}
    assert not wrong, wrong
    # the refused files and the progressive ones: deferred, with nothing else in the record
    others = [d for n, d in F.fixture_files() if n.startswith(("refused_", "prog_"))]
    info = front_scan_host(others)
    assert (info["defer"] == 1).all()
    assert not info.view(np.int32).reshape(len(others), -1)[:, 1:].any()


def test_blob_from_twin_info_and_numpy_layout_equals_the_planners():
    from hawq_amd.jpeg import front_layout, front_scan_host, output_layout, parse_jpeg, plan_jpeg_batch
    names, datas = _accepted_fixtures()
    info = front_scan_host(datas)
    for files in (list(range(len(datas))), [3, 17, 40, 41, 77], [len(datas) - 1]):
        plan = plan_jpeg_batch([parse_jpeg(datas[i]) for i in files])
        offsets, total = output_layout(plan.sizes)
        lay = front_layout(info, files, offsets, total)
        assert (lay.nbytes, lay.n_waves, lay.coef_blocks, lay.plane_bytes, lay.out_bytes) == (plan.nbytes, plan.n_waves, plan.coef_blocks, plan.plane_bytes, plan.out_bytes)
        assert np.array_equal(F.host_fill(datas, info, lay), plan.blob[:plan.nbytes])
    # images placed out of order with gaps, as decode_jpeg_batch places them among files of other kinds
    files, offsets = [5, 6, 30, 60], [12288, 32, 8192, 4112]
    plan = plan_jpeg_batch([parse_jpeg(datas[i]) for i in files], offsets, 20000)
    lay = front_layout(info, files, offsets, 20000)
    assert np.array_equal(F.host_fill(datas, info, lay), plan.blob[:plan.nbytes]) and lay.out_bytes == plan.out_bytes


def test_sync_job_table_from_interval_lengths_equals_the_planners():
    from hawq_amd.jpeg import _sync_job_table, parse_jpeg, plan_jpeg_batch
    _, datas = _accepted_fixtures()
    recs = [parse_jpeg(d) for d in datas]
    for sub_bytes, min_sync_bytes in ((16, 64), (32, 4096), (4096, 1)):
        plan = plan_jpeg_batch(recs, sync=(sub_bytes, min_sync_bytes))
        jobs, scratch = _sync_job_table(np.concatenate([np.diff(r.intervals, axis=1).reshape(-1) for r in recs]), sub_bytes, min_sync_bytes)
        assert scratch == plan.scratch_bytes and [tuple(j) for j in jobs.tolist()] == plan.jobs
        assert jobs.tobytes() == plan.blob[plan.jobs_off:plan.jobs_off + 16 * plan.n_jobs].tobytes()


def test_twin_is_sound_and_complete_on_the_mutation_corpus():
    """Whenever the twin accepts, ``parse_jpeg`` accepts with the same fields; whenever ``parse_jpeg`` accepts and the twin defers, the
    code is one of ``FRONT_DEFERS_BY_DESIGN`` - and no unmutated fixture gets one of those."""
    from hawq_amd.jpeg import FRONT_DEFERS_BY_DESIGN, front_scan_host
    files = F.corpus()
    assert len(files) > 5000
    info = front_scan_host(files)
    accepted = both = 0
    for data, o in zip(files, info):
        r = _parse(data)
        if o["defer"] == 0:
            accepted += 1
            assert r is not None, data.hex()
            assert F.record_mismatch(data, o, r) is None, (F.record_mismatch(data, o, r), data.hex())
        elif r is not None:
            assert int(o["defer"]) in FRONT_DEFERS_BY_DESIGN, (int(o["defer"]), data.hex())
        both += r is not None
    assert accepted > 500 and accepted == both   # on this corpus nothing hits a bound of the kernel
    assert set(FRONT_DEFERS_BY_DESIGN) == {2, 3}
    fixtures = front_scan_host([d for _, d in F.fixture_files()])
    assert not np.isin(fixtures["defer"], list(FRONT_DEFERS_BY_DESIGN)).any()


def test_twin_defers_a_header_longer_than_the_kernel_walks_and_python_still_parses_it():
    from hawq_amd.jpeg import front_scan_host
    from tests.jpeg_pins import units
    good, _, _ = jpeg_model.cases()
    base = good["noise_16x16_444"][0]
    com = b"\xff\xfe\x00\x03x"
    plain = sum(1 for label, *_ in units(base) if label.split(".")[0] not in ("SOI", "ecs", "D9"))   # marker segments up to the SOS
    for extra, defer in ((64 - plain, 0), (64 - plain + 1, 2)):
        data = base[:2] + com * extra + base[2:]
        o = front_scan_host([data])[0]
        assert o["defer"] == defer and _parse(data) is not None, (extra, int(o["defer"]))


# ------------------------------------------------------------------------------------------------------------------ the checker of the fill
def test_fill_checker_refuses_every_offset_or_length_pushed_out_of_range():
    from hawq_amd import _lib
    from hawq_amd.jpeg import front_layout, front_scan_host, output_layout, pack_files
    good, _, _ = jpeg_model.cases()
    names = ["noise_13x17_420", "noise_40x24_rst4", "smooth_31x33_gray", "noise_31x33_422"]
    datas = [good[n][0] for n in names]
    info0 = front_scan_host(datas)
    table0, _, total = pack_files(datas)
    offsets, out_bytes = output_layout([(int(o["height"]), int(o["width"])) for o in info0])
    lay = front_layout(info0, range(len(datas)), offsets, out_bytes)
    lib = _lib.load()

    def ok(info=info0, place=lay.place, n=len(datas), table=table0, n_files=len(datas), files_bytes=total, blob_bytes=lay.nbytes):
        return bool(lib.hawq_jpeg_front_fill_ok(info.ctypes.data, place.ctypes.data, n, table.ctypes.data, n_files, files_bytes, blob_bytes))

    assert ok()
    assert not ok(blob_bytes=lay.nbytes - 16) and not ok(blob_bytes=8) and not ok(blob_bytes=1 << 31) and not ok(n=0) and not ok(n_files=len(datas) - 1)
    assert not ok(files_bytes=total - 16)
    assert lib.hawq_last_error().startswith(b"hawq_jpeg_front_fill: ")
    big, refused = 1 << 30, 0

    def mutated(which, change):
        nonlocal refused
        info, place, table = info0.copy(), lay.place.copy(), table0.copy()
        change({"info": info, "place": place, "table": table}[which])
        assert not ok(info, place, table=table), (which, lib.hawq_last_error())
        assert lib.hawq_last_error().startswith(b"hawq_jpeg_front_fill: ")
        refused += 1

    def set_field(i, name, v, c=None):
        def f(arr):
            if c is None:
                arr[name][i] = v
            else:
                arr[name][i][c] = v
        return f

    for i, name in enumerate(names):
        ncomp = 1 if "gray" in name else 3
        length = len(datas[i])
        for field, vals in (("defer", (1, 2)), ("ncomp", (0, 2, 4)), ("n_intervals", (0, -1, big)), ("scan_first", (-1, big)), ("scan_end", (0, length - 1, big))):
            for v in vals:
                mutated("info", set_field(i, field, v))
        for c in range(ncomp):
            for field, vals in (("tq", (-1, 4)), ("td", (-1, 2)), ("ta", (-1, 2))):
                for v in vals:
                    mutated("info", set_field(i, field, v, c))
        for k in set(int(v) for v in info0["tq"][i][:ncomp]):
            for v in (0, -1, length - 63, big):
                mutated("info", set_field(i, "qt_at", v, k))
        for k in set(int(v) for v in info0["td"][i][:ncomp]) | set(2 + int(v) for v in info0["ta"][i][:ncomp]):
            for v in (0, -1, length - 15, big):
                mutated("info", set_field(i, "huff_at", v, k))
        for field in ("qt_off", "dc_off", "ac_off"):
            for c in range(ncomp):
                if lay.place[field][i][c]:
                    for v in (-16, 0, 8, big, lay.nbytes - 16, int(lay.place[field][i][c]) + 4):
                        mutated("place", set_field(i, field, v, c))
                else:
                    mutated("place", set_field(i, field, int(lay.place[field][i][0]), c))   # a shared table placed again
        for field in ("interval_off", "stream_off"):
            for v in (-16, 0, 8, big, lay.nbytes, int(lay.place[field][i]) + 4):
                mutated("place", set_field(i, field, v))
        for v in (-1, len(datas), i - 1 if i else len(datas)):
            mutated("place", set_field(i, "file", v))
        for field, vals in (("offset", (-16, int(table0["offset"][i]) + 8, big)), ("length", (-1, big))):
            for v in vals:
                mutated("table", set_field(i, field, v))
        mutated("table", set_field(i, "length", int(info0["scan_end"][i]) + 1))   # the file ends inside EOI
    # a part laid over the one before it
    mutated("place", lambda p: p["stream_off"].__setitem__(1, p["interval_off"][1]))
    mutated("place", lambda p: p["interval_off"].__setitem__(2, p["stream_off"][1]))
    mutated("table", lambda t: t["offset"].__setitem__(2, t["offset"][1]))
    assert refused > 200 and ok()


def test_scan_refuses_a_bad_file_table_before_it_reads_anything():
    from hawq_amd import _lib
    from hawq_amd.jpeg import _FINFO, pack_files
    good, _, _ = jpeg_model.cases()
    datas = [good["noise_13x17_420"][0], good["noise_40x24_rst4"][0]]
    table0, buf, total = pack_files(datas)
    info = np.zeros(len(datas), _FINFO)
    lib = _lib.load()
    assert lib.hawq_jpeg_front_scan_host(buf.ctypes.data, total, table0.ctypes.data, 2, info.ctypes.data) == 0
    for field, i, v in (("offset", 1, 8), ("offset", 1, 0), ("offset", 0, -16), ("length", 1, total), ("length", 0, -1), ("offset", 1, 1 << 40)):
        table = table0.copy()
        table[field][i] = v
        assert lib.hawq_jpeg_front_scan_host(buf.ctypes.data, total, table.ctypes.data, 2, info.ctypes.data) != 0, (field, i, v)
        assert lib.hawq_last_error().startswith(b"hawq_jpeg_front_scan: ")
        # the device entry point makes the same check before it touches a pointer or launches
        assert lib.hawq_jpeg_front_scan(16, total, 16, table.ctypes.data, 2, 16, None) == 2
    assert lib.hawq_jpeg_front_scan_host(buf.ctypes.data, total, table0.ctypes.data, 0, info.ctypes.data) != 0


# ------------------------------------------------------------------------------------------------------------------ bookkeeping
def _stub_device(monkeypatch):
    """``_front_scan`` replaced by the host twin, ``_front_launch`` and ``_launch`` by the numpy models (status 2 where the model cannot
    decode a stream); returns the log: ("front" | "base" | "prog", how many images) per call"""
    from hawq_amd import jpeg
    log = []

    def decode_into(kind, datas_or_records, offsets, out, model):
        status = torch.zeros(len(offsets), dtype=torch.int32)
        for k, (item, off) in enumerate(zip(datas_or_records, offsets)):
            try:
                rgb = model(item)
            except (ValueError, IndexError):
                status[k] = 2
                continue
            out[off:off + rgb.size] = torch.from_numpy(rgb.reshape(-1))
        log.append((kind, len(offsets)))
        return status

    def launch(records, out_offsets, out, dev, events=None, sync=None, info=None, resume=None):
        if isinstance(records[0], jpeg.JpegProgRecord):
            return decode_into("prog", records, out_offsets, out, lambda r: jpeg_prog_model.decode(r.data))
        return decode_into("base", records, out_offsets, out, lambda r: jpeg_model.decode(r.data))

    def front_launch(staged, info, files, out_offsets, out, dev, events=None, sync=None):
        assert all(info["defer"][i] == 0 for i in files)
        return decode_into("front", [staged[i] for i in files], out_offsets, out, jpeg_model.decode)

    monkeypatch.setattr(jpeg, "_launch", launch)
    monkeypatch.setattr(jpeg, "_front_launch", front_launch)
    monkeypatch.setattr(jpeg, "_front_scan", lambda datas, dev: (jpeg.front_scan_host(datas), datas))
    return log


def test_bookkeeping_with_stubs_equals_the_host_front_end(monkeypatch):
    from hawq_amd.jpeg import decode_jpeg_batch
    from tests.test_gpu_jpeg import damaged_files
    good, bad, _ = jpeg_model.cases()
    prog, prog_bad, _ = jpeg_prog_model.cases()
    a, truncated, damaged, b = damaged_files()
    long_header = good["noise_16x16_444"][0][:2] + b"\xff\xfe\x00\x03x" * 70 + good["noise_16x16_444"][0][2:]   # deferred, then accepted by parse_jpeg
    srcs = [good["noise_13x17_420"][0], bad["progressive"][0], a, truncated, bad["png"][0], bad["cmyk"][0], damaged, long_header, prog["noise_16x16_420"][0],
            good["noise_40x24_rst4"][0], prog_bad["two_components"][0], b, jpeg_model.sample()]
    log = _stub_device(monkeypatch)
    for more in ({}, {"progressive": True}, {"entropy": "sync", "min_sync_bytes": 64, "sub_bytes": 16}):
        del log[:]
        want_images, want_fallbacks = decode_jpeg_batch(srcs, device="cpu", **more)
        host_log = list(log)
        del log[:]
        images, fallbacks = decode_jpeg_batch(srcs, device="cpu", front_end="device", **more)
        assert fallbacks == want_fallbacks and len(fallbacks) >= 5
        assert all(torch.equal(x, y) for x, y in zip(images, want_images))
        assert ("front", 7) in log and ("base", 1) in log and sum(k for _, k in log) == sum(k for _, k in host_log)
        assert (("prog", 2) in log) == bool(more.get("progressive"))
        base = images[0].untyped_storage().data_ptr()
        assert all(im.untyped_storage().data_ptr() == base and im.data_ptr() % 16 == 0 for im in images)
    # nothing for the device front end's launch: none happens
    del log[:]
    images, fallbacks = decode_jpeg_batch([bad["png"][0], bad["progressive"][0]], device="cpu", front_end="device")
    assert log == [] and fallbacks == [(0, "not a JPEG"), (1, "progressive (SOF2)")]


def test_loader_with_the_device_front_end_keeps_order_labels_and_bytes(monkeypatch, tmp_path):
    from hawq_amd import image
    good, bad, _ = jpeg_model.cases()
    _stub_device(monkeypatch)
    files = {"a/0.jpg": good["noise_31x33_444"][0], "a/1.jpg": bad["progressive"][0], "b/0.jpg": good["smooth_40x23_420rst"][0], "b/1.png": bad["png"][0],
             "b/2.jpeg": good["noise_40x24_rst7_gray"][0]}
    for rel, data in files.items():
        (tmp_path / rel).parent.mkdir(exist_ok=True)
        (tmp_path / rel).write_bytes(data)
    seen = []

    def fused(imgs, resize, crop, device=None):
        seen.append([im.clone() for im in imgs])
        return torch.zeros(len(imgs), crop, crop, 3, dtype=torch.uint8)

    monkeypatch.setattr(image, "preprocess_batch_fused", fused)
    got = list(image.folder_loader(str(tmp_path), batch_size=2, resize=24, crop=16, device="cpu", device_decode=True, front_end="device"))
    assert [t.tolist() for _, t in got] == [[0, 0], [1, 1], [1]]
    for im, (rel, data) in zip([im for batch in seen for im in batch], sorted(files.items())):
        assert torch.equal(im, image.decode_image(data)), rel


def test_argument_checks_raise(tmp_path):
    from hawq_amd import image
    from hawq_amd.jpeg import ResumeIndex, decode_jpeg_batch, front_layout, front_scan_host
    good, bad, _ = jpeg_model.cases()
    data = good["noise_13x17_420"][0]
    with pytest.raises(ValueError, match="front_end must be"):
        decode_jpeg_batch([data], device="cpu", front_end="gpu")
    with pytest.raises(ValueError, match="does not take resume"):
        decode_jpeg_batch([data], device="cpu", front_end="device", resume=ResumeIndex(512))
    with pytest.raises(ValueError, match="empty batch"):
        decode_jpeg_batch([], device="cpu", front_end="device")
    (tmp_path / "a").mkdir()
    (tmp_path / "a" / "0.jpg").write_bytes(data)
    with pytest.raises(ValueError, match="needs device_decode"):
        next(image.folder_loader(str(tmp_path), device="cpu", front_end="device"))
    with pytest.raises(ValueError, match="front_end must be"):
        next(image.folder_loader(str(tmp_path), device="cpu", device_decode=True, front_end="both"))
    with pytest.raises(ValueError, match="resume"):
        next(image.folder_loader(str(tmp_path), device="cpu", device_decode=True, front_end="device", resume=ResumeIndex(512)))
    info = front_scan_host([data, bad["png"][0]])
    with pytest.raises(ValueError, match="accepted files"):
        front_layout(info, [0, 1], [0, 1024], 2048)
    with pytest.raises(ValueError, match="accepted files"):
        front_layout(info, [], [], 0)


# ------------------------------------------------------------------------------------------------------------------ the walker under the sanitizers
def test_walker_on_the_host_under_sanitizers_on_every_corpus_file(tmp_path):
    """tools/jpeg_front_check.cpp: the header text the scan kernel compiles, built with ASan + UBSan into a program of its own and run
    as a child process.  Every fixture and every corpus file sits in a heap block of its exact length; the records must equal the
    library's, and the run must end without a sanitizer report."""
    from hawq_amd.jpeg import front_scan_host
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "jpeg_front_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tools", "jpeg_front_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    files = [d for _, d in F.fixture_files()] + F.corpus() + [b"", b"\xff", b"\xff\xd8\xff", b"\xff\xd8\xff\xff", b"\xff\xd8\xff\xc4"]
    info = front_scan_host(files)
    with open(tmp_path / "corpus.bin", "wb") as f:
        f.write(np.int64(len(files)).tobytes())
        for d in files:
            f.write(np.int64(len(d)).tobytes())
            f.write(d)
    info.tofile(str(tmp_path / "expected.bin"))
    r = subprocess.run([exe, str(tmp_path / "corpus.bin"), str(tmp_path / "expected.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    words = r.stdout.split()
    counts = dict(zip(words[0::2], map(int, words[1::2])))
    assert counts["files"] == len(files) and counts["accepted"] == int((info["defer"] == 0).sum()) > 600 and counts["tables"] >= 2 * counts["accepted"]
