"""Host side of the progressive device JPEG decoder (hawq_amd/jpeg.py with ``progressive=True``, hawq_jpeg_prog_ok, csrc/jpeg_prog.h)
without a GPU: the parser's accept / refuse decisions and scan lists, the Python model against real Pillow output
(tests/golden/jpeg_prog_cases.npz, make_jpeg_prog_cases.py), the planner's levels, the blob checker, the fallback bookkeeping with stubs
in place of the two device calls, and the scan decoders the kernel compiles, built into a stand-alone program under AddressSanitizer +
UBSan and run on valid and corrupted streams."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import jpeg_model
from tests import jpeg_prog_model as M
from tests.jpeg_stub import stub_launch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Pillow's scan script: (components, Ss, Se, Ah, Al)
PILLOW_COLOUR = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1),
                 ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
PILLOW_GRAY = [((0,),) + s[1:] for s in PILLOW_COLOUR if 0 in s[0]]
SCRIPTS = {"spectral": M.script_spectral, "deep": M.script_deep, "tables": lambda n: M.script_deep(n, tables=True, top=1), "dri": M.script_dri}


def test_the_fixture_set_holds_what_makes_it_meaningful():
    good, bad, cond = M.cases()
    assert len(good) >= 30 and set(bad) == {"cut_last_scan", "adobe", "two_components", "ac_before_dc", "ah_not_previous_al", "65_scans"}
    assert cond["eob_category"] == 14 and cond["corrections_in_eob_run"] > 0 and cond["refine_zrl"] > 0 and cond["narrower_grid"] > 0
    assert cond["deepest_level"] >= 5 and cond["own_grid_intervals"] > 1


def test_parser_accepts_every_case_with_pillows_geometry_and_the_expected_scans():
    from hawq_amd.jpeg import JpegProgRecord, scan_levels
    good, _, _ = M.cases()
    seen = set()
    for name, (rec, _) in M.model_coefficients().items():
        rgb = good[name][1]
        assert isinstance(rec, JpegProgRecord) and (rec.height, rec.width) == rgb.shape[:2], name
        assert rec.ncomp == (1 if name.endswith("gray") or "_gray_" in name else 3), name
        assert rec.mcus_x == -(-rec.width // (8 * rec.hs)) and rec.mcus_y == -(-rec.height // (8 * rec.vs)), name
        got = [(s.comps, s.ss, s.se, s.ah, s.al) for s in rec.scans]
        kind = name.split("_")[0]
        if kind in SCRIPTS:
            want = [(s["comps"], s["ss"], s["se"], s["ah"], s["al"]) for s in SCRIPTS[kind](rec.ncomp)]
        else:
            want = PILLOW_GRAY if rec.ncomp == 1 else PILLOW_COLOUR
            assert max(scan_levels(rec.scans)) == 3, name
        assert got == want, name
        for s in rec.scans:
            if len(s.comps) > 1:
                assert s.units == rec.mcus_x * rec.mcus_y, name
            else:
                h, v = rec.components[s.comps[0]][1:3]
                assert s.units == -(-(-(-rec.width * h // rec.hs)) // 8) * -(-(-(-rec.height * v // rec.vs)) // 8), name
            assert len(s.intervals) == (-(-s.units // s.restart) if s.restart else 1), name
            assert s.intervals[0, 0] == 0 and s.intervals[-1, 1] == s.scan[1] - s.scan[0] and np.all(s.intervals[1:, 0] == s.intervals[:-1, 1] + 2), name
            assert (s.dc is not None) == (s.ss == 0 and s.ah == 0) and (s.ac is not None) == (s.ss > 0), name
            seen.add((rec.ncomp, rec.hs, rec.vs, bool(s.restart), len(s.comps) > 1))
        assert rec.data[rec.scans[-1].scan[1]:rec.scans[-1].scan[1] + 2] == b"\xff\xd9", name
    assert {k[:3] for k in seen} == {(3, 1, 1), (3, 2, 1), (3, 2, 2), (1, 1, 1)} and {k[3:] for k in seen} == {(False, False), (False, True), (True, False), (True, True)}
    rec = M.model_coefficients()["noise_33x31_420"][0]
    assert rec.own_grid(0) == (5, 4) and (rec.mcus_x * 2, rec.mcus_y * 2) == (6, 4)   # the example of DESIGN.md 12.2
    rec = M.model_coefficients()["tables_13x17_422"][0]
    assert len({id(s.ac) for s in rec.scans if s.ac is not None}) > 2   # tables redefined between scans


def test_parser_refuses_each_recorded_case_with_its_reason_and_without_the_option_every_progressive_file():
    from hawq_amd.jpeg import UnsupportedJpeg, parse_jpeg
    good, bad, _ = M.cases()
    for name, (data, reason) in bad.items():
        with pytest.raises(UnsupportedJpeg) as e:
            parse_jpeg(data, progressive=True)
        assert e.value.reason == reason, (name, e.value.reason)
    for name, (data, _) in good.items():
        for call in (lambda d: parse_jpeg(d), lambda d: parse_jpeg(d, progressive=False)):
            with pytest.raises(UnsupportedJpeg) as e:
                call(data)
            assert e.value.reason == "progressive (SOF2)", name
    # baseline files parse as before
    base, _, _ = jpeg_model.cases()
    for name in ("noise_13x17_420", "noise_40x24_rst4", "smooth_31x33_gray"):
        a, b = parse_jpeg(base[name][0]), parse_jpeg(base[name][0], progressive=True)
        assert type(a) is type(b) and a.scan == b.scan and np.array_equal(a.intervals, b.intervals), name


def _with_scan_byte(data, scan, offset, value):
    """``data`` with the byte ``offset`` behind the ``scan``-th SOS marker replaced"""
    at = -1
    for _ in range(scan + 1):
        at = data.index(b"\xff\xda", at + 1)
    return data[:at + offset] + bytes([value]) + data[at + offset + 1:]


def test_parser_refuses_what_the_progressive_path_does_not_take():
    from hawq_amd.jpeg import UnsupportedJpeg, parse_jpeg
    good, _, _ = M.cases()
    base = good["noise_16x16_444"][0]
    rst = good["noise_40x24_444_rst"][0]
    sos1 = base.index(b"\xff\xda", base.index(b"\xff\xda") + 1)
    dqt = base[base.index(b"\xff\xdb"):base.index(b"\xff\xdb") + 69]
    at_rst = rst.index(b"\xff\xd1")
    last = base.rindex(b"\xff\xda")
    variants = {
        "spectral selection": _with_scan_byte(base, 1, 8, 0),           # Y 1-5 -> Ss 1, Se 0
        "successive approximation": _with_scan_byte(base, 1, 9, 0x0E),   # Al 14
        "AC scan of several components": _with_scan_byte(_with_scan_byte(base, 0, 11, 1), 0, 12, 5),   # the interleaved DC scan with Ss-Se 1-5
        "Huffman table id above 3": _with_scan_byte(base, 1, 6, 0x04),
        "missing table": _with_scan_byte(base, 1, 6, 0x03),
        "scan component order": _with_scan_byte(base, 1, 5, 9),
        "DQT between scans": base[:sos1] + dqt + base[sos1:],
        "marker C2 between scans": base[:sos1] + base[base.index(b"\xff\xc2"):base.index(b"\xff\xc2") + 19] + base[sos1:],
        "truncated scan": base[:-2],
        "restart markers missing or out of order": rst[:at_rst + 1] + b"\xd2" + rst[at_rst + 2:],
        "progression": base[:last] + b"\xff\xd9",
        "sample precision not 8": base.replace(b"\xff\xc2\x00\x11\x08", b"\xff\xc2\x00\x11\x0c", 1),
        "sampling factors": base.replace(b"\xff\xc2\x00\x11\x08\x00\x10\x00\x10\x03\x01\x11", b"\xff\xc2\x00\x11\x08\x00\x10\x00\x10\x03\x01\x12", 1),
    }
    for reason, data in variants.items():
        with pytest.raises(UnsupportedJpeg) as e:
            parse_jpeg(data, progressive=True)
        assert e.value.reason == reason, (reason, e.value.reason)
    # tolerated: a comment and fill bytes between scans, bytes behind EOI
    padded = base[:sos1] + b"\xff\xfe\x00\x05abc" + b"\xff\xff" + base[sos1:] + b"trailing"
    r, r0 = parse_jpeg(padded, progressive=True), parse_jpeg(base, progressive=True)
    assert [padded[s.scan[0]:s.scan[1]] for s in r.scans] == [base[s.scan[0]:s.scan[1]] for s in r0.scans]


def test_python_model_equals_pillow_on_every_fixture():
    good, _, _ = M.cases()
    for name, (rec, comps) in M.model_coefficients().items():
        assert np.array_equal(M.pixels(rec, comps), good[name][1]), name


# ------------------------------------------------------------------------------------------------------------------ planner and checker
def _plan(names=None):
    from hawq_amd.jpeg import plan_jpeg_prog_batch
    recs = M.model_coefficients()
    names = list(recs) if names is None else names
    return plan_jpeg_prog_batch([recs[n][0] for n in names]), names


def _ok(plan, blob=None, nbytes=None, coef=None, planes=None, out=None):
    from hawq_amd import _lib
    blob = plan.blob if blob is None else blob
    return bool(_lib.load().hawq_jpeg_prog_ok(blob.ctypes.data, plan.nbytes if nbytes is None else nbytes, plan.coef_blocks if coef is None else coef,
                                              plan.plane_bytes if planes is None else planes, plan.out_bytes if out is None else out))


def test_planner_computes_the_levels_and_the_checker_passes_its_blob():
    from hawq_amd import _lib
    plan, names = _plan()
    assert plan.ok(), _lib.load().hawq_last_error()
    assert plan.nbytes % 16 == 0 and plan.blob.ctypes.data % 16 == 0 and plan.n_levels == 5
    recs = M.model_coefficients()
    assert plan.n_scans == sum(len(recs[n][0].scans) for n in names) and plan.n_waves == sum(len(s.intervals) for n in names for s in recs[n][0].scans)
    scans = plan.blob[plan.scan_off:plan.scan_off + plan.n_scans * C.sizeof(_lib.JpegScan)].view(np.dtype(_lib.JpegScan))
    assert scans["level"].tolist() == plan.levels and np.all(scans["stream_off"] % 16 == 0) and np.all(scans["interval_off"] % 16 == 0)
    desc = plan.blob[plan.desc_off:plan.desc_off + len(names) * C.sizeof(_lib.JpegDesc)].view(np.dtype(_lib.JpegDesc))
    for field in ("dc_off", "ac_off", "stream_off", "stream_len", "interval_off", "restart", "n_intervals"):
        assert not desc[field].any(), field
    assert plan.coef_blocks == sum(recs[n][0].blocks for n in names) and plan.plane_bytes == plan.coef_blocks * 64
    # Pillow's ten scans make three levels: five first scans, four refinements, the last Y refinement
    one, _ = _plan(["noise_16x16_420"])
    assert one.levels == [1, 1, 1, 1, 1, 2, 2, 2, 2, 3] and one.level_start == [0, 5, 9, 10]
    waves = one.blob[one.wave_off:one.wave_off + 8 * one.n_waves].view(np.int32).reshape(-1, 2)
    assert waves[:, 0].tolist() == list(range(10)) and not waves[:, 1].any()
    assert _plan(["deep_33x31_420"])[0].n_levels == 5 and _plan(["spectral_33x31_420"])[0].n_levels == 1


def test_checker_refuses_every_field_pushed_out_of_range_or_made_inconsistent():
    from hawq_amd import _lib
    plan, names = _plan(["noise_13x17_422", "noise_40x24_420_rst", "noise_7x9_gray", "deep_33x31_420", "dri_40x24_420"])
    lib = _lib.load()
    assert _ok(plan)
    assert not _ok(plan, nbytes=plan.nbytes - 16) and not _ok(plan, nbytes=24)
    assert not _ok(plan, coef=plan.coef_blocks - 1) and not _ok(plan, planes=plan.plane_bytes - 1) and not _ok(plan, out=plan.out_bytes - 16)
    big = 1 << 30
    refused = 0
    scan_dt, desc_dt = np.dtype(_lib.JpegScan), np.dtype(_lib.JpegDesc)
    scans0 = plan.blob[plan.scan_off:plan.scan_off + plan.n_scans * scan_dt.itemsize].view(scan_dt).copy()

    def mutated(change, why=None):
        nonlocal refused
        blob = plan.blob.copy()
        change(blob, blob[plan.desc_off:plan.desc_off + len(names) * desc_dt.itemsize].view(desc_dt),
               blob[plan.scan_off:plan.scan_off + plan.n_scans * scan_dt.itemsize].view(scan_dt))
        assert not _ok(plan, blob), (why, lib.hawq_last_error())
        assert lib.hawq_last_error().startswith(b"hawq_jpeg_decode_batch_prog: ")
        if why:
            assert why in lib.hawq_last_error().decode(), (why, lib.hawq_last_error())
        refused += 1

    def set_hdr(k, v):
        return lambda blob, desc, scans: blob[:32].view(np.int32).__setitem__(k, v)

    hdr0 = plan.blob[:32].view(np.int32).copy()
    for k, vals in ((0, (0, -1, len(names) + 1)), (1, (0, plan.n_waves - 1, plan.n_waves + 1)), (2, (-16, big, hdr0[2] + 4)), (3, (-16, big, hdr0[3] + 4)),
                    (4, (0, plan.n_scans - 1, plan.n_scans + 1, 65 * len(names))), (5, (0, plan.n_levels - 1, plan.n_levels + 1, 65)), (6, (-16, big, hdr0[6] + 4)),
                    (7, (-16, big, hdr0[7] + 4))):
        for v in vals:
            mutated(set_hdr(k, v))

    def set_desc(i, name, v, c=None):
        def f(blob, desc, scans):
            if c is None:
                desc[name][i] = v
            else:
                desc[name][i][c] = v
        return f

    for i in range(len(names)):
        ncomp = 1 if "gray" in names[i] else 3
        for name, vals in (("width", (0, 8193, 4096)), ("height", (0, 8193, 4096)), ("ncomp", (0, 2, 4)), ("hs", (0, 3, 4)), ("vs", (0, 3)), ("mcus_x", (0, 1000)),
                           ("mcus_y", (0, 1000)), ("restart", (1,)), ("n_intervals", (1,)), ("stream_off", (16,)), ("stream_len", (1,)), ("interval_off", (16,)),
                           ("coef_block0", (-1, plan.coef_blocks)), ("plane_off", (-64, plan.plane_bytes)), ("out_off", (-16, plan.out_bytes, 8))):
            for v in vals:
                mutated(set_desc(i, name, v))
        for c in range(ncomp):
            for v in (-16, big, plan.nbytes - 8):
                mutated(set_desc(i, "qt_off", v, c))
            mutated(set_desc(i, "dc_off", 16, c))
            mutated(set_desc(i, "ac_off", 16, c))
    mutated(lambda blob, desc, scans: desc["out_off"].__setitem__(1, desc["out_off"][0]))
    mutated(lambda blob, desc, scans: desc["coef_block0"].__setitem__(2, desc["coef_block0"][1]))

    def set_scan(k, name, v, c=None):
        def f(blob, desc, scans):
            if c is None:
                scans[name][k] = v
            else:
                scans[name][k][c] = v
        return f

    for k in range(plan.n_scans):
        s = scans0[k]
        for name, vals in (("image", (-1, len(names), int(s["image"]) + 1)), ("ncomp", (0, 2, 4)), ("comp0", (-1, 3)), ("ss", (-1, 64, int(s["se"]) + 1)), ("se", (-1, 64)),
                           ("ah", (-1, 15, int(s["ah"]) + 1)), ("al", (-1, 14, int(s["al"]) + 1)), ("restart", (-1, int(s["restart"]) + 1)),
                           ("n_intervals", (0, int(s["n_intervals"]) + 1)), ("interval_off", (-4, big, 2)), ("stream_off", (-16, big, 8)), ("stream_len", (-1, big))):
            for v in vals:
                if name == "restart" and v > 0 and -(-_units(plan, names, k) // v) == s["n_intervals"]:
                    continue   # another restart interval that gives the same number of intervals
                mutated(set_scan(k, name, v))
        for v in {0, int(s["level"]) - 1, int(s["level"]) + 1, 64}:
            mutated(set_scan(k, "level", v))
        if s["ss"] == 0 and s["ah"] == 0:
            for c in range(int(s["ncomp"])):
                for v in (-16, big, plan.nbytes - 8):
                    mutated(set_scan(k, "dc_off", v, c), "Huffman table")
        if s["ss"] > 0:
            for v in (-16, big, plan.nbytes - 8):
                mutated(set_scan(k, "ac_off", v), "Huffman table")
    mutated(set_scan(int(np.flatnonzero(scans0["level"] == 2)[0]), "level", 1), "level")

    # a progression made incomplete in the blob: the last scan of image 0 stops at coefficient 62, or leaves out coefficient 1
    last0 = int(np.flatnonzero(scans0["image"] == 0)[-1])
    mutated(set_scan(last0, "se", 62), "progression: incomplete")
    mutated(set_scan(last0, "ss", 2), "progression: incomplete")

    def drop_last_scan_of_the_batch(blob, desc, scans):
        blob[:32].view(np.int32)[4] -= 1

    mutated(drop_last_scan_of_the_batch)

    def interval(k, j, col, v):
        def f(blob, desc, scans):
            blob[scans["interval_off"][k]:scans["interval_off"][k] + 8 * scans["n_intervals"][k]].view(np.int32).reshape(-1, 2)[j, col] = v
        return f

    rst = int(np.flatnonzero(scans0["n_intervals"] > 1)[0])
    mutated(interval(rst, 0, 0, -1), "restart interval")
    mutated(interval(rst, 1, 1, big), "restart interval")
    mutated(interval(rst, 1, 0, 5000), "restart interval")
    mutated(interval(0, 0, 1, 100000), "restart interval")

    def wave(k, col, v):
        return lambda blob, desc, scans: blob[plan.wave_off:plan.wave_off + 8 * plan.n_waves].view(np.int32).reshape(-1, 2).__setitem__((k, col), v)

    waves0 = plan.blob[plan.wave_off:plan.wave_off + 8 * plan.n_waves].view(np.int32).reshape(-1, 2).copy()
    mutated(wave(0, 0, 1), "wave list")                      # a (scan, interval) twice, another never
    mutated(wave(1, 0, int(waves0[0, 0])), "wave list")
    mutated(wave(plan.n_waves - 1, 0, -1), "wave list")
    mutated(wave(int(np.flatnonzero(waves0[:, 0] == rst)[0]), 1, 1), "wave list")
    first_of_level_2 = plan.level_start[1]
    mutated(wave(first_of_level_2 - 1, 0, int(waves0[first_of_level_2, 0])), "wave list")   # a scan of level 2 under level 1

    def level_start(k, v):
        return lambda blob, desc, scans: blob[plan.level_off:plan.level_off + 4 * (plan.n_levels + 1)].view(np.int32).__setitem__(k, v)

    for k, vals in ((0, (1, -1)), (1, (plan.level_start[1] - 1, plan.level_start[1] + 1, -5, big)), (plan.n_levels, (plan.n_waves - 1, plan.n_waves + 1))):
        for v in vals:
            mutated(level_start(k, v))

    def huff(k, name, length, v):
        def f(blob, desc, scans):
            t = blob[scans["ac_off"][k]:scans["ac_off"][k] + C.sizeof(_lib.JpegHuff)].view(np.dtype(_lib.JpegHuff))
            t[name][0][length] = v
        return f

    ac = int(np.flatnonzero(scans0["ss"] > 0)[0])
    table = plan.blob[scans0["ac_off"][ac]:scans0["ac_off"][ac] + C.sizeof(_lib.JpegHuff)].view(np.dtype(_lib.JpegHuff))
    used = int(np.flatnonzero(table["maxcode"][0] >= 0)[-1])   # the longest code length the table has
    mutated(huff(ac, "maxcode", 2, 4), "Huffman table")       # no 2-bit code is 4
    mutated(huff(ac, "maxcode", 16, -2), "Huffman table")
    mutated(huff(ac, "valptr", used, 250), "Huffman table")   # values behind huffval
    mutated(huff(ac, "mincode", used, -5), "Huffman table")
    assert refused > 1000 and _ok(plan)


def _units(plan, names, k):
    """units of scan k of the plan's scan table, from the parser's records"""
    recs = M.model_coefficients()
    flat = [s for n in names for s in recs[n][0].scans]
    return flat[k].units


# ------------------------------------------------------------------------------------------------------------------ fallback bookkeeping
def _stub_launches(monkeypatch, statuses=None):
    """``jpeg._launch`` replaced by the two models writing into host tensors; ``statuses``: {position among the progressive images:
    status}.  Returns the list of calls: ("base" | "prog", number of records, data_ptr of the output)."""
    return stub_launch(monkeypatch, {"base": lambda r: jpeg_model.decode(r.data), "prog": lambda r: M.pixels(r, M.coefficients(r))},
                       lambda kind, records, out, sync: (kind, len(records), out.data_ptr()), {"prog": statuses or {}})


def test_fallback_bookkeeping_with_stubs_in_place_of_the_device_calls(monkeypatch):
    from hawq_amd.image import decode_image
    from hawq_amd.jpeg import decode_jpeg_batch
    good, bad, _ = M.cases()
    base, base_bad, _ = jpeg_model.cases()
    calls = _stub_launches(monkeypatch, {1: 2})
    srcs = [base["noise_13x17_420"][0], good["noise_13x17_422"][0], base_bad["cmyk"][0], base_bad["png"][0], bad["cut_last_scan"][0], good["deep_33x31_420"][0],
            base["noise_40x24_rst4"][0], good["noise_40x24_gray_rst"][0]]
    images, fallbacks = decode_jpeg_batch(srcs, device="cpu", progressive=True)
    assert fallbacks == [(2, "four components"), (3, "not a JPEG"), (4, "progression"), (5, "device status 2: code not in table")]
    base_ptr = images[0].untyped_storage().data_ptr()
    assert sorted(calls) == [("base", 2, base_ptr), ("prog", 3, base_ptr)]   # the right split, both into the one allocation
    at = 0
    for i, (im, src) in enumerate(zip(images, srcs)):
        assert torch.equal(im, decode_image(src)), i
        assert im.untyped_storage().data_ptr() == base_ptr and im.data_ptr() - base_ptr == at and im.is_contiguous()
        at = (at + im.numel() + 15) & ~15
    # without the option: today's list, one call
    calls.clear()
    images, fallbacks = decode_jpeg_batch(srcs, device="cpu")
    assert [c[:2] for c in calls] == [("base", 2)]
    assert fallbacks == [(1, "progressive (SOF2)"), (2, "four components"), (3, "not a JPEG"), (4, "progressive (SOF2)"), (5, "progressive (SOF2)"),
                         (7, "progressive (SOF2)")]
    for i, (im, src) in enumerate(zip(images, srcs)):
        assert torch.equal(im, decode_image(src)), i
    # only progressive files: no baseline call
    calls.clear()
    images, fallbacks = decode_jpeg_batch([good["noise_7x9_444"][0]], device="cpu", progressive=True)
    assert [c[:2] for c in calls] == [("prog", 1)] and fallbacks == [] and torch.equal(images[0], decode_image(good["noise_7x9_444"][0]))


def test_loader_passes_the_option_through_and_wants_device_decode(monkeypatch, tmp_path):
    from hawq_amd import image
    good, _, _ = M.cases()
    base, base_bad, _ = jpeg_model.cases()
    _stub_launches(monkeypatch)
    files = {"a/0.jpg": base["noise_31x33_444"][0], "a/1.jpg": good["noise_33x31_420"][0], "b/0.jpg": good["noise_40x24_422_rst"][0], "b/1.png": base_bad["png"][0]}
    for rel, data in files.items():
        (tmp_path / rel).parent.mkdir(exist_ok=True)
        (tmp_path / rel).write_bytes(data)
    with pytest.raises(ValueError):
        next(image.folder_loader(str(tmp_path), progressive=True))
    seen = []

    def fused(imgs, resize, crop, device=None):   # stands in for the launch: records what it is handed
        seen.append([im.clone() for im in imgs])
        return torch.zeros(len(imgs), crop, crop, 3, dtype=torch.uint8)

    monkeypatch.setattr(image, "preprocess_batch_fused", fused)
    got = list(image.folder_loader(str(tmp_path), batch_size=3, resize=24, crop=16, device="cpu", device_decode=True, progressive=True))
    assert [t.tolist() for _, t in got] == [[0, 0, 1], [1]]
    for im, (rel, data) in zip([im for batch in seen for im in batch], sorted(files.items())):
        assert torch.equal(im, image.decode_image(data)), rel


# ------------------------------------------------------------------------------------------------------------------ the kernel's decoders on the host
def test_scan_decoders_on_the_host_under_sanitizers_on_valid_and_corrupted_streams(tmp_path):
    """tools/jpeg_prog_host_check.cpp: the header text jpeg_prog_kernel compiles, built with ASan + UBSan into a program of its own and run
    as a child process on the planner's blob of ALL accepted fixtures: golden bytes for the intact files, level by level; a status and no
    sanitizer report for every scan stream truncated at each eighth byte; a status or a clean result and no sanitizer report for 200
    single-byte overwrites per scan stream."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "jpeg_prog_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tools", "jpeg_prog_host_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    plan, names = _plan()
    assert plan.ok()
    good, _, _ = M.cases()
    expected = np.zeros(plan.out_bytes, np.uint8)
    for n, off in zip(names, plan.out_offsets):
        rgb = good[n][1]
        expected[off:off + rgb.size] = rgb.reshape(-1)
    plan.blob[:plan.nbytes].tofile(str(tmp_path / "blob.bin"))
    expected.tofile(str(tmp_path / "expected.bin"))
    r = subprocess.run([exe, str(tmp_path / "blob.bin"), str(tmp_path / "expected.bin"), str(plan.out_bytes), str(M.HOST_CHECK_SEED)], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    words = r.stdout.split()
    counts = dict(zip(words[0::2], map(int, words[1::2])))
    assert counts["images"] == counts["exact"] == len(names) and counts["scans"] == plan.n_scans and counts["levels"] == plan.n_levels
    assert counts["truncations"] == counts["truncations_flagged"] > plan.n_scans
    assert counts["overwrites"] == 200 * plan.n_scans and counts["overwrites_flagged"] > 0
