"""The device front end for progressive JPEGs (csrc/jpeg_front_prog.h + jpeg_front.hip, hawq_amd.jpeg ``progressive="device"``;
DESIGN.md 12.6) without a GPU: the host twin of the scan kernel against ``parse_jpeg(d, progressive=True)`` on the fixtures and on the
mutation corpus, the numpy layout and a numpy model of the fill against ``plan_jpeg_prog_batch``, the checker of the fill, the
bookkeeping of ``decode_jpeg_batch`` with stubs in place of the device calls, and the walker's own text under AddressSanitizer + UBSan in
a program of its own."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import jpeg_front_corpus as F
from tests import jpeg_front_prog_model as M
from tests import jpeg_model, jpeg_prog_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compare(files):
    """The twin on ``files`` against the Python parser -> (accepted by the twin, accepted by Python, progressive among them)"""
    from hawq_amd.jpeg import FRONT_PROG_DEFERS_BY_DESIGN, JpegProgRecord, front_scan_host, front_scan_prog_host
    info, scans = front_scan_prog_host(files)
    base = front_scan_host(files)
    accepted = both = progressive = 0
    for i, (data, o) in enumerate(zip(files, info)):
        r = M.parse(data)
        both += r is not None
        if o["defer"] == 0:
            accepted += 1
            assert r is not None, data.hex()
            if isinstance(r, JpegProgRecord):
                progressive += 1
                assert M.prog_mismatch(data, o, scans[i], r) is None, (M.prog_mismatch(data, o, scans[i], r), data.hex())
            else:   # a baseline file: the record of the baseline scan, bit for bit, and no scan record
                assert o.tobytes() == base[i].tobytes() and F.record_mismatch(data, o, r) is None and not scans[i].view(np.int32).any(), data.hex()
        else:
            assert o.tobytes() == np.array([int(o["defer"])] + [0] * 31, np.int32).tobytes() and not scans[i].view(np.int32).any()
            if r is not None:
                assert int(o["defer"]) in FRONT_PROG_DEFERS_BY_DESIGN, (int(o["defer"]), data.hex())
    return accepted, both, progressive


def test_twin_accepts_what_the_python_parser_accepts_on_every_fixture():
    names, datas = zip(*F.fixture_files())
    accepted, both, progressive = _compare(list(datas))
    # every accepted fixture of both kinds, and the progressive file among the ones the baseline path refuses
    assert accepted == both == sum(1 for n in names if not n.startswith(("refused_", "prog_refused_"))) + 1
    assert progressive == len(M.prog_fixtures()[0]) + 1 >= 20


def test_twin_is_sound_and_complete_on_the_mutation_corpus():
    """Whenever the twin accepts, ``parse_jpeg(d, progressive=True)`` accepts with the same file fields, scan fields, tables in force and
    levels; whenever Python accepts and the twin defers, the code is one of ``FRONT_PROG_DEFERS_BY_DESIGN`` - and on this corpus nothing is."""
    from hawq_amd.jpeg import FRONT_PROG_DEFERS_BY_DESIGN
    files = F.corpus()
    assert len(files) > 5000
    accepted, both, progressive = _compare(files)
    assert accepted == both and progressive > 1000 and accepted - progressive > 500
    assert set(FRONT_PROG_DEFERS_BY_DESIGN) == {2, 3}


def _segments(data, r, upto_frame=False):
    """marker segments of the progressive file ``data`` with record ``r``: all of them, or those up to its frame header, SOF2 included"""
    pos, count, scan = 2, 0, 0
    while data[pos + 1] != 0xD9:
        count += 1
        if upto_frame and data[pos + 1] == 0xC2:
            break
        if data[pos + 1] == 0xDA:
            pos, scan = r.scans[scan].scan[1], scan + 1
        else:
            pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    return count


def test_twin_defers_at_the_kernels_bounds_and_python_still_parses_the_file():
    """More than 64 marker segments up to the frame header (the baseline walk's bound, which sees the file first) or more than 256 in a
    progressive file in all defer with code 2, and ``parse_jpeg`` takes the file all the same; no unmutated fixture gets such a code"""
    from hawq_amd.jpeg import FRONT_PROG_DEFERS_BY_DESIGN, front_scan_prog_host, parse_jpeg
    names, datas = M.prog_fixtures()
    data = datas[names.index("noise_16x16_420")]
    r = parse_jpeg(data, progressive=True)
    between = r.scans[0].scan[1]
    for at, bound, have in ((between, 256, _segments(data, r)), (2, 64, _segments(data, r, upto_frame=True))):
        for extra, defer in ((bound - have, 0), (bound - have + 1, 2)):
            mutated = data[:at] + M.comment(1) * extra + data[at:]
            o = front_scan_prog_host([mutated])[0][0]
            assert o["defer"] == defer and M.parse(mutated) is not None, (bound, extra, int(o["defer"]))
    fixtures = front_scan_prog_host([d for _, d in F.fixture_files()])[0]
    assert not np.isin(fixtures["defer"], list(FRONT_PROG_DEFERS_BY_DESIGN)).any()


# ------------------------------------------------------------------------------------------------------------------ the blob
def _layout_and_plan(datas, files, out_offsets=None, out_bytes=None, draft=None):
    from hawq_amd.jpeg import front_prog_layout, front_scan_prog_host, output_layout, parse_jpeg, plan_jpeg_prog_batch
    info, scans = front_scan_prog_host(datas)
    plan = plan_jpeg_prog_batch([parse_jpeg(datas[i], progressive=True) for i in files], out_offsets, out_bytes, draft=draft)
    if out_offsets is None:
        out_offsets, out_bytes = output_layout(plan.sizes)
    lay = front_prog_layout(info, scans, files, out_offsets, out_bytes, draft)
    return info, scans, lay, plan


@pytest.mark.parametrize("case", ["all", "noise_16x16_420", "placed", "draft"])
def test_blob_from_twin_records_and_numpy_fill_equals_the_planners(case):
    names, datas = M.prog_fixtures()
    more = {}
    if case in ("all", "draft"):
        files = list(range(len(datas)))
        more = {"draft": (8, 8)} if case == "draft" else {}
    elif case == "placed":   # out of order with gaps, as decode_jpeg_batch places them among files of other kinds: the case of the pins
        placed = sorted(zip((names.index(n) for n in ("noise_40x24_420_rst", "noise_7x9_gray", "tables_13x17_422")), (8192, 48, 4096)))
        files, more = [i for i, _ in placed], {"out_offsets": [off for _, off in placed], "out_bytes": 16384}
    else:
        files = [names.index(case)]
    info, scans, lay, plan = _layout_and_plan(datas, files, **more)
    for f in ("nbytes", "n_scans", "n_levels", "n_waves", "level_start", "coef_blocks", "plane_bytes", "out_bytes", "scan_off", "level_off", "wave_off", "desc_off"):
        assert getattr(lay, f) == getattr(plan, f), f
    assert lay.scans["level"].tolist() == plan.levels
    assert np.array_equal(M.host_fill_prog(datas, info, scans, lay), plan.blob[:plan.nbytes])
    if case == "placed":   # the pins place the images in no ascending order, which the library's checker does not take
        return
    host = np.ascontiguousarray(M.host_fill_prog(datas, info, scans, lay))
    from hawq_amd import _lib
    assert _lib.load().hawq_jpeg_prog_ok(host.ctypes.data, lay.nbytes, lay.coef_blocks, lay.plane_bytes, lay.out_bytes), _lib.load().hawq_last_error()


def test_a_table_in_force_over_several_scans_stands_once_per_image():
    names, datas = M.prog_fixtures()
    info, scans, lay, plan = _layout_and_plan(datas, list(range(len(datas))))
    placed = np.column_stack((lay.place["dc_off"], lay.place["ac_off"]))
    read = np.column_stack((lay.scans["dc_off"], lay.scans["ac_off"]))
    assert (placed != 0).sum() < (read != 0).sum()           # some scan reads a table an earlier one has placed
    assert len(set(placed[placed != 0].tolist())) == (placed != 0).sum() and set(read[read != 0].tolist()) == set(placed[placed != 0].tolist())


# ------------------------------------------------------------------------------------------------------------------ the checker of the fill
def test_fill_checker_refuses_every_offset_or_length_pushed_out_of_range():
    from hawq_amd import _lib
    from hawq_amd.jpeg import front_prog_layout, front_scan_prog_host, output_layout, pack_files
    names, fixtures = M.prog_fixtures()
    picks = ["noise_40x24_420_rst", "noise_7x9_gray", "tables_13x17_422", "noise_16x16_420"]
    datas = [fixtures[names.index(n)] for n in picks] + [jpeg_model.cases()[0]["noise_13x17_420"][0]]   # the last one: baseline
    info0, scans0 = front_scan_prog_host(datas)
    table0, _, total = pack_files(datas)
    files = list(range(len(picks)))
    offsets, out_bytes = output_layout([(int(o["height"]), int(o["width"])) for o in info0[files]])
    lay = front_prog_layout(info0, scans0, files, offsets, out_bytes)
    lib = _lib.load()

    def ok(info=info0, scans=scans0, place=lay.place, n=len(lay.place), table=table0, n_files=len(datas), files_bytes=total, blob_bytes=lay.nbytes):
        return bool(lib.hawq_jpeg_front_fill_prog_ok(info.ctypes.data, scans.ctypes.data, place.ctypes.data, n, table.ctypes.data, n_files, files_bytes, blob_bytes))

    assert ok()
    assert not ok(blob_bytes=lay.nbytes - 16) and not ok(blob_bytes=16) and not ok(blob_bytes=1 << 31) and not ok(n=0) and not ok(n_files=len(picks) - 1)
    assert not ok(files_bytes=total - len(datas[-1]) - 16)
    assert lib.hawq_last_error().startswith(b"hawq_jpeg_front_fill_prog: ")
    big, refused = 1 << 30, 0

    def mutated(which, change):
        nonlocal refused
        arrays = {"info": info0.copy(), "scans": scans0.copy(), "place": lay.place.copy(), "table": table0.copy()}
        change(arrays[which])
        assert not ok(arrays["info"], arrays["scans"], arrays["place"], table=arrays["table"]), (which, lib.hawq_last_error())
        assert lib.hawq_last_error().startswith(b"hawq_jpeg_front_fill_prog: ")
        refused += 1

    def set_field(i, name, v, c=None):
        def f(arr):
            if c is None:
                arr[name][i] = v
            else:
                arr[name][i][c] = v
        return f

    for e, pl in enumerate(lay.place):
        i, k = int(pl["file"]), int(pl["scan"])
        length, s = len(datas[i]), scans0[i, k]
        for field, vals in (("n_intervals", (0, -1, big)), ("scan_first", (-1, big)), ("scan_end", (0, length - 1, big))):
            for v in vals:
                mutated("scans", lambda a, field=field, v=v: a[field].__setitem__((i, k), v))
        for c in range(3):
            if pl["dc_off"][c]:
                for v in (0, -1, length - 15, big):
                    mutated("scans", lambda a, c=c, v=v: a["dc_at"][i, k].__setitem__(c, v))
        if pl["ac_off"]:
            for v in (0, -1, length - 15, big):
                mutated("scans", lambda a, v=v: a["ac_at"].__setitem__((i, k), v))
        for field in ("qt_off", "dc_off"):
            for c in range(3):
                if pl[field][c]:
                    for v in (-16, 8, big, lay.nbytes - 16, int(pl[field][c]) + 4):
                        mutated("place", set_field(e, field, v, c))
        if pl["qt_off"].any():
            for c in range(3):
                if pl["qt_off"][c]:
                    for v in (-1, 4):
                        mutated("info", set_field(i, "tq", v, c))
                    for v in (0, -1, length - 63, big):
                        mutated("info", set_field(i, "qt_at", v, int(info0["tq"][i][c])))
                elif c >= info0["ncomp"][i]:
                    mutated("place", set_field(e, "qt_off", int(pl["qt_off"][0]), c))   # a table of a component the file does not have
        if pl["ac_off"]:
            for v in (-16, 8, big, lay.nbytes - 16, int(pl["ac_off"]) + 4):
                mutated("place", set_field(e, "ac_off", v))
        for field in ("interval_off", "stream_off"):
            for v in (-16, 0, 8, big, lay.nbytes, int(pl[field]) + 4):
                mutated("place", set_field(e, field, v))
        for v in (-1, len(datas), len(datas) - 1, i - 1 if i else len(datas)):   # len(datas) - 1: the baseline file
            mutated("place", set_field(e, "file", v))
        for v in (-1, int(info0["reserved"][i][1]), k - 1 if k else 64):
            mutated("place", set_field(e, "scan", v))
    for i in files:
        for v in (1, 2):
            mutated("info", set_field(i, "defer", v))
        for v in (0, 2, 4):
            mutated("info", set_field(i, "ncomp", v))
        for c, v in ((0, 0), (0, 2), (1, 0), (1, 65), (1, -1)):
            mutated("info", set_field(i, "reserved", v, c))
        for field, vals in (("offset", (-16, int(table0["offset"][i]) + 8, big)), ("length", (-1, big))):
            for v in vals:
                mutated("table", set_field(i, field, v))
        last = int(info0["reserved"][i][1]) - 1
        mutated("table", set_field(i, "length", int(scans0["scan_end"][i, last]) + 1))   # the file ends inside EOI
    # a part laid over the one before it
    mutated("place", lambda p: p["stream_off"].__setitem__(1, p["interval_off"][1]))
    mutated("place", lambda p: p["interval_off"].__setitem__(2, p["stream_off"][1]))
    assert refused > 1000 and ok()


def test_scan_refuses_a_bad_file_table_before_it_reads_anything():
    from hawq_amd import _lib
    from hawq_amd.jpeg import _FINFO, _FSCAN, pack_files
    _, fixtures = M.prog_fixtures()
    datas = fixtures[:2]
    table0, buf, total = pack_files(datas)
    info, scans = np.zeros(2, _FINFO), np.zeros((2, 64), _FSCAN)
    lib = _lib.load()
    assert lib.hawq_jpeg_front_scan_prog_host(buf.ctypes.data, total, table0.ctypes.data, 2, info.ctypes.data, scans.ctypes.data) == 0
    for field, i, v in (("offset", 1, 8), ("offset", 1, 0), ("offset", 0, -16), ("length", 1, total), ("length", 0, -1), ("offset", 1, 1 << 40)):
        table = table0.copy()
        table[field][i] = v
        assert lib.hawq_jpeg_front_scan_prog_host(buf.ctypes.data, total, table.ctypes.data, 2, info.ctypes.data, scans.ctypes.data) != 0, (field, i, v)
        assert lib.hawq_last_error().startswith(b"hawq_jpeg_front_scan_prog: ")
        # the device entry point makes the same check before it touches a pointer or launches
        assert lib.hawq_jpeg_front_scan_prog(16, total, 16, table.ctypes.data, 2, 16, 16, None) == 2


# ------------------------------------------------------------------------------------------------------------------ bookkeeping
def _stub_device(monkeypatch):
    """The device calls replaced: ``_front_scan_prog`` by the host twin, the launches by the numpy models (status 2 where a model cannot
    decode a stream); returns the log: ("front" | "front_prog" | "base" | "prog", how many images) per call"""
    from hawq_amd import jpeg
    log = []

    def decode_into(kind, items, offsets, out, model):
        status = torch.zeros(len(offsets), dtype=torch.int32)
        for k, (item, off) in enumerate(zip(items, offsets)):
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
        assert all(info["defer"][i] == 0 and info["reserved"][i][0] == 0 for i in files)
        return decode_into("front", [staged[i] for i in files], out_offsets, out, jpeg_model.decode)

    def front_prog_fill(staged, info, scans, files, out_offsets, out, dev):
        assert all(info["defer"][i] == 0 and info["reserved"][i][0] == 1 and scans[i, 0]["level"] == 1 for i in files)
        return [staged[i] for i in files], out_offsets

    def front_prog_decode(filled, out, dev, events=None, wait=True):
        return decode_into("front_prog", *filled, out, jpeg_prog_model.decode)

    def scan_prog(datas, dev):
        return (*jpeg.front_scan_prog_host(datas), datas)

    monkeypatch.setattr(jpeg, "_launch", launch)
    monkeypatch.setattr(jpeg, "_front_launch", front_launch)
    monkeypatch.setattr(jpeg, "_front_scan", lambda datas, dev: (jpeg.front_scan_host(datas), datas))
    monkeypatch.setattr(jpeg, "_front_scan_prog", scan_prog)
    monkeypatch.setattr(jpeg, "_front_prog_fill", front_prog_fill)
    monkeypatch.setattr(jpeg, "_front_prog_decode", front_prog_decode)
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
    for more in ({}, {"entropy": "sync", "min_sync_bytes": 64, "sub_bytes": 16}):
        del log[:]
        want_images, want_fallbacks = decode_jpeg_batch(srcs, device="cpu", progressive=True, **more)
        assert ("prog", 2) in log
        del log[:]
        images, fallbacks = decode_jpeg_batch(srcs, device="cpu", front_end="device", progressive="device", **more)
        assert fallbacks == want_fallbacks and len(fallbacks) >= 4
        assert all(torch.equal(x, y) for x, y in zip(images, want_images))
        # the progressive files go the new route, the baseline ones the device front end's, the long header through parse_jpeg
        assert sorted(log) == [("base", 1), ("front", 7), ("front_prog", 2)]
        base = images[0].untyped_storage().data_ptr()
        assert all(im.untyped_storage().data_ptr() == base and im.data_ptr() % 16 == 0 for im in images)
    # progressive files alone, and one the walker defers by design: through parse_jpeg(progressive=True) and _launch as with True
    deferred = prog["noise_7x9_gray"][0][:2] + b"\xff\xfe\x00\x03x" * 70 + prog["noise_7x9_gray"][0][2:]
    del log[:]
    srcs = [prog["noise_16x16_420"][0], deferred, prog["tables_13x17_422"][0]]
    images, fallbacks = decode_jpeg_batch(srcs, device="cpu", front_end="device", progressive="device")
    assert fallbacks == [] and sorted(log) == [("front_prog", 2), ("prog", 1)]
    assert all(torch.equal(x, torch.from_numpy(jpeg_prog_model.decode(d))) for x, d in zip(images, srcs))
    # progressive=True under the device front end stays on its route
    del log[:]
    decode_jpeg_batch(srcs, device="cpu", front_end="device", progressive=True)
    assert log == [("prog", 3)]


def test_loader_passes_the_option_through(monkeypatch, tmp_path):
    from hawq_amd import image
    good, _, _ = jpeg_model.cases()
    prog, _, _ = jpeg_prog_model.cases()
    log = _stub_device(monkeypatch)
    files = {"a/0.jpg": good["noise_31x33_444"][0], "a/1.jpg": prog["noise_16x16_420"][0], "b/0.jpg": prog["noise_7x9_gray"][0]}
    for rel, data in files.items():
        (tmp_path / rel).parent.mkdir(exist_ok=True)
        (tmp_path / rel).write_bytes(data)
    seen = []

    def fused(imgs, resize, crop, device=None):
        seen.append([im.clone() for im in imgs])
        return torch.zeros(len(imgs), crop, crop, 3, dtype=torch.uint8)

    monkeypatch.setattr(image, "preprocess_batch_fused", fused)
    got = list(image.folder_loader(str(tmp_path), batch_size=2, resize=24, crop=16, device="cpu", device_decode=True, front_end="device", progressive="device"))
    assert [t.tolist() for _, t in got] == [[0, 0], [1]] and sorted(log) == [("front", 1), ("front_prog", 1), ("front_prog", 1)]
    for im, (rel, data) in zip([im for batch in seen for im in batch], sorted(files.items())):
        assert torch.equal(im, image.decode_image(data)), rel


def test_argument_checks_raise(tmp_path):
    from hawq_amd import image
    from hawq_amd.jpeg import ResumeIndex, decode_jpeg_batch, front_prog_layout, front_scan_prog_host
    good, bad, _ = jpeg_model.cases()
    data = M.prog_fixtures()[1][0]
    with pytest.raises(ValueError, match="needs front_end='device'"):
        decode_jpeg_batch([data], device="cpu", progressive="device")
    with pytest.raises(ValueError, match="needs front_end='device'"):
        decode_jpeg_batch([data], device="cpu", progressive="device", front_end="host")
    with pytest.raises(ValueError, match="progressive must be"):
        decode_jpeg_batch([data], device="cpu", progressive="host", front_end="device")
    with pytest.raises(ValueError, match="does not take resume"):
        decode_jpeg_batch([data], device="cpu", front_end="device", progressive="device", resume=ResumeIndex(512))
    (tmp_path / "a").mkdir()
    (tmp_path / "a" / "0.jpg").write_bytes(data)
    with pytest.raises(ValueError, match="needs device_decode"):
        next(image.folder_loader(str(tmp_path), device="cpu", progressive="device"))
    with pytest.raises(ValueError, match="needs front_end='device'"):
        next(image.folder_loader(str(tmp_path), device="cpu", device_decode=True, progressive="device"))
    with pytest.raises(ValueError, match="progressive must be"):
        next(image.folder_loader(str(tmp_path), device="cpu", device_decode=True, front_end="device", progressive="gpu"))
    with pytest.raises(ValueError, match="resume"):
        next(image.folder_loader(str(tmp_path), device="cpu", device_decode=True, front_end="device", progressive="device", resume=ResumeIndex(512)))
    info, scans = front_scan_prog_host([data, good["noise_13x17_420"][0], bad["png"][0]])
    for files in ([0, 1], [0, 2], []):
        with pytest.raises(ValueError, match="accepted progressive files"):
            front_prog_layout(info, scans, files, [0, 4096][:len(files)], 8192)


# ------------------------------------------------------------------------------------------------------------------ the walker under the sanitizers
def test_walker_on_the_host_under_sanitizers_on_every_corpus_file(tmp_path):
    """tools/jpeg_front_prog_check.cpp: the header text the scan kernel compiles, with the canonical-table and interval code of the fill,
    built with ASan + UBSan into a program of its own and run as a child process.  Every fixture and every corpus file sits in a heap
    block of its exact length; the records must equal the library's, and the run must end without a sanitizer report."""
    from hawq_amd.jpeg import front_scan_prog_host
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "jpeg_front_prog_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tools", "jpeg_front_prog_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    files = [d for _, d in F.fixture_files()] + F.corpus() + M.phase_files()[::97] + [b"", b"\xff", b"\xff\xd8\xff", b"\xff\xd8\xff\xff", b"\xff\xd8\xff\xc4", b"\xff\xd8\xff\xc2"]
    info, scans = front_scan_prog_host(files)
    with open(tmp_path / "corpus.bin", "wb") as f:
        f.write(np.int64(len(files)).tobytes())
        for d in files:
            f.write(np.int64(len(d)).tobytes())
            f.write(d)
    with open(tmp_path / "expected.bin", "wb") as f:
        for o, s in zip(info, scans):
            f.write(o.tobytes())
            f.write(s.tobytes())
    r = subprocess.run([exe, str(tmp_path / "corpus.bin"), str(tmp_path / "expected.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    words = r.stdout.split()
    counts = dict(zip(words[0::2], map(int, words[1::2])))
    accepted = info["defer"] == 0
    assert counts["files"] == len(files) and counts["baseline"] == int((accepted & (info["reserved"][:, 0] == 0)).sum()) > 600
    assert counts["progressive"] == int((accepted & (info["reserved"][:, 0] == 1)).sum()) > 1000
    assert counts["scans"] == int(info["reserved"][:, 1].sum()) and counts["tables"] >= counts["progressive"]
