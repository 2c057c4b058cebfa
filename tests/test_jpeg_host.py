"""Host side of the device JPEG decoder (hawq_amd/jpeg.py, hawq_jpeg_batch_ok, csrc/jpeg_entropy.h + jpeg_pixel.h) without a GPU:
the parser's accept / refuse decisions, the blob checker, the numpy model against real Pillow output (tests/golden/jpeg_cases.npz,
make_jpeg_cases.py), the fallback bookkeeping with a stub in place of the device call, and the kernels' own block / pixel arithmetic
compiled into a stand-alone program under AddressSanitizer + UBSan, on valid and on corrupted streams."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import jpeg_model
from tests.jpeg_stub import stub_launch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


cases, sample = jpeg_model.cases, jpeg_model.sample


def test_the_fixture_set_holds_what_makes_it_meaningful():
    good, bad, cond = cases()
    assert len(good) >= 84 + 8 and set(bad) == {"progressive", "cmyk", "png", "cut_header"}
    assert cond["stuffed"] > 0 and cond["zrl"] > 0 and cond["longest_code"] == 16 and cond["two_qtables"] > 0 and cond["max_intervals"] > 1


def test_parser_accepts_every_case_with_the_geometry_pillow_reports():
    from hawq_amd.jpeg import parse_jpeg
    good, _, _ = cases()
    seen = set()
    for name, (data, rgb) in good.items():
        r = parse_jpeg(data)
        assert (r.height, r.width) == rgb.shape[:2], name
        assert r.ncomp == (1 if name.endswith("gray") else 3), name
        assert r.mcus_x == -(-r.width // (8 * r.hs)) and r.mcus_y == -(-r.height // (8 * r.vs)), name
        mcus = r.mcus_x * r.mcus_y
        assert len(r.intervals) == (-(-mcus // r.restart) if r.restart else 1), name
        assert r.intervals[0, 0] == 0 and r.intervals[-1, 1] == r.scan[1] - r.scan[0], name
        assert np.all(r.intervals[1:, 0] == r.intervals[:-1, 1] + 2), name   # an RSTn marker between two intervals
        assert data[r.scan[1]:r.scan[1] + 2] == b"\xff\xd9", name
        for q in r.qtables.values():
            assert q.dtype == np.uint16 and q.shape == (64,)
        seen.add((r.ncomp, r.hs, r.vs, bool(r.restart)))
    assert seen >= {(3, 1, 1, False), (3, 2, 1, False), (3, 2, 2, False), (3, 2, 2, True), (3, 1, 1, True), (3, 2, 1, True), (1, 1, 1, False), (1, 1, 1, True)}
    r = parse_jpeg(sample())
    assert (r.height, r.width) == (375, 500)


def test_parser_refuses_each_recorded_case_with_its_reason():
    from hawq_amd.jpeg import UnsupportedJpeg, parse_jpeg
    _, bad, _ = cases()
    for name, (data, reason, _) in bad.items():
        with pytest.raises(UnsupportedJpeg) as e:
            parse_jpeg(data)
        assert e.value.reason == reason, name


def _patched(data, marker, offset, value):
    """`data` with the byte `offset` behind the first `marker` replaced"""
    at = data.index(marker) + offset
    return data[:at] + bytes([value]) + data[at + 1:]


def test_parser_refuses_what_the_device_path_does_not_take():
    from hawq_amd.jpeg import UnsupportedJpeg, parse_jpeg
    good, _, _ = cases()
    base = good["noise_16x16_444"][0]
    rst = good["noise_40x24_rst2"][0]
    sos = base.index(b"\xff\xda")
    at_rst = rst.index(b"\xff\xd1")
    variants = {
        "extended sequential (SOF1)": base.replace(b"\xff\xc0", b"\xff\xc1", 1),
        "arithmetic coding": base.replace(b"\xff\xc0", b"\xff\xc9", 1),
        "sample precision not 8": _patched(base, b"\xff\xc0", 4, 12),
        "sampling factors": _patched(base, b"\xff\xc0", 11, 0x12),
        "component ids not 1, 2, 3": _patched(_patched(base, b"\xff\xc0", 10, 7), b"\xff\xda", 5, 7),
        "16-bit quantisation table": _patched(base, b"\xff\xdb", 4, 0x10),
        "Huffman table id above 1": _patched(base, b"\xff\xc4", 4, 0x02),
        "spectral selection or successive approximation": _patched(base, b"\xff\xda", 12, 62),
        "Adobe marker": base[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + base[2:],
        "DNL": base[:sos] + b"\xff\xdc\x00\x04\x00\x10" + base[sos:],
        "several scans": base[:-2] + base[sos:],
        "truncated scan": base[:-2],
        "restart markers missing or out of order": rst[:at_rst + 1] + b"\xd2" + rst[at_rst + 2:],
        "missing table": base[:base.index(b"\xff\xc4")] + base[base.index(b"\xff\xda"):],
        "truncated header": base[:sos + 5],
        "not a JPEG": b"GIF89a" + base,
    }
    for reason, data in variants.items():
        with pytest.raises(UnsupportedJpeg) as e:
            parse_jpeg(data)
        assert e.value.reason == reason, (reason, e.value.reason)
    # tolerated: fill bytes before a marker, a comment segment, bytes behind EOI
    padded = base[:2] + b"\xff\xfe\x00\x05abc" + base[2:sos] + b"\xff\xff" + base[sos:] + b"trailing"
    r, r0 = parse_jpeg(padded), parse_jpeg(base)
    assert padded[r.scan[0]:r.scan[1]] == base[r0.scan[0]:r0.scan[1]]


def test_numpy_model_equals_pillow_on_every_golden_and_the_sample():
    from hawq_amd.image import decode_image
    good, _, _ = cases()
    for name, (data, rgb) in good.items():
        assert np.array_equal(jpeg_model.decode(data), rgb), name
    data = sample()
    assert np.array_equal(jpeg_model.decode(data), decode_image(data).numpy())


# ------------------------------------------------------------------------------------------------------------------ the blob checker
def _plan(names=None):
    from hawq_amd.jpeg import parse_jpeg, plan_jpeg_batch
    good, _, _ = cases()
    names = list(good) if names is None else names
    return plan_jpeg_batch([parse_jpeg(good[n][0]) for n in names]), names


def _ok(plan, blob=None, nbytes=None, coef=None, planes=None, out=None):
    from hawq_amd import _lib
    blob = plan.blob if blob is None else blob
    return bool(_lib.load().hawq_jpeg_batch_ok(blob.ctypes.data, plan.nbytes if nbytes is None else nbytes, plan.coef_blocks if coef is None else coef,
                                               plan.plane_bytes if planes is None else planes, plan.out_bytes if out is None else out))


def test_planner_lays_the_blob_out_aligned_and_the_checker_passes_it():
    from hawq_amd import _lib
    plan, names = _plan()
    assert plan.ok() and plan.nbytes % 16 == 0 and plan.blob.ctypes.data % 16 == 0
    hdr = plan.blob[:16].view(np.int32)
    desc = plan.blob[hdr[2]:hdr[2] + len(names) * C.sizeof(_lib.JpegDesc)].view(np.dtype(_lib.JpegDesc))
    assert hdr[0] == len(names) and hdr[1] == plan.n_waves == int(desc["n_intervals"].sum())
    for field in ("qt_off", "dc_off", "ac_off", "stream_off", "interval_off", "out_off"):
        assert np.all(desc[field] % 16 == 0), field
    assert plan.coef_blocks == sum(int(d["mcus_x"]) * int(d["mcus_y"]) * (1 if d["ncomp"] == 1 else int(d["hs"]) * int(d["vs"]) + 2) for d in desc)
    assert plan.plane_bytes == plan.coef_blocks * 64 and plan.out_offsets == desc["out_off"].tolist()


def test_checker_refuses_every_offset_or_count_pushed_out_of_range():
    from hawq_amd import _lib
    plan, names = _plan(["noise_13x17_420", "noise_40x24_rst4", "smooth_31x33_gray", "noise_31x33_422"])
    assert _ok(plan)
    assert not _ok(plan, nbytes=plan.nbytes - 16) and not _ok(plan, nbytes=8)
    assert not _ok(plan, coef=plan.coef_blocks - 1) and not _ok(plan, planes=plan.plane_bytes - 1) and not _ok(plan, out=plan.out_bytes - 16)
    hdr0 = plan.blob[:16].view(np.int32).copy()
    dsz = C.sizeof(_lib.JpegDesc)
    big = 1 << 30
    refused = 0

    def mutated(change):
        nonlocal refused
        blob = plan.blob.copy()
        change(blob, blob[hdr0[2]:hdr0[2] + len(names) * dsz].view(np.dtype(_lib.JpegDesc)))
        assert not _ok(plan, blob), _lib.load().hawq_last_error()
        assert _lib.load().hawq_last_error().startswith(b"hawq_jpeg_decode_batch: ")
        refused += 1

    def set_hdr(k, v):
        def f(blob, desc):
            blob[:16].view(np.int32)[k] = v
        return f

    for k, vals in ((0, (0, -1, len(names) + 1)), (1, (0, plan.n_waves - 1, plan.n_waves + 1)), (2, (-16, big, hdr0[2] + 4)), (3, (-16, big, hdr0[3] + 4))):
        for v in vals:
            mutated(set_hdr(k, v))

    def set_field(i, name, v, c=None):
        def f(blob, desc):
            if c is None:
                desc[name][i] = v
            else:
                desc[name][i][c] = v
        return f

    for i in range(len(names)):
        ncomp = 1 if "gray" in names[i] else 3
        for name, vals in (("width", (0, 8193, 4096)), ("height", (0, 8193, 4096)), ("ncomp", (0, 2, 4)), ("hs", (0, 3, 4)), ("vs", (0, 3)),
                           ("mcus_x", (0, 1000)), ("mcus_y", (0, 1000)), ("restart", (-1, 1)), ("n_intervals", (0, 77)),
                           ("stream_off", (-16, big, 8)), ("stream_len", (-1, big)), ("interval_off", (-4, big, 2)),
                           ("coef_block0", (-1, plan.coef_blocks)), ("plane_off", (-64, plan.plane_bytes)), ("out_off", (-16, plan.out_bytes, 8))):
            for v in vals:
                mutated(set_field(i, name, v))
        for name in ("qt_off", "dc_off", "ac_off"):
            for c in range(ncomp):
                for v in (-16, big, plan.nbytes - 8):
                    mutated(set_field(i, name, v, c))
    # an image laid over the one before it
    mutated(lambda blob, desc: desc["out_off"].__setitem__(1, desc["out_off"][0]))
    mutated(lambda blob, desc: desc["coef_block0"].__setitem__(2, desc["coef_block0"][1]))

    def interval(i, k, col, v):
        def f(blob, desc):
            blob[desc["interval_off"][i]:desc["interval_off"][i] + 8 * desc["n_intervals"][i]].view(np.int32).reshape(-1, 2)[k, col] = v
        return f

    mutated(interval(1, 0, 0, -1))
    mutated(interval(1, 1, 1, big))
    mutated(interval(1, 1, 0, 5000))   # first byte behind the last
    mutated(interval(0, 0, 1, 100000))

    def wave(k, col, v):
        def f(blob, desc):
            blob[hdr0[3]:hdr0[3] + 8 * hdr0[1]].view(np.int32).reshape(-1, 2)[k, col] = v
        return f

    mutated(wave(0, 0, 1))
    mutated(wave(1, 1, 7))
    mutated(wave(plan.n_waves - 1, 0, -1))

    def huff(i, name, length, v):
        def f(blob, desc):
            t = blob[desc["ac_off"][i][0]:desc["ac_off"][i][0] + C.sizeof(_lib.JpegHuff)].view(np.dtype(_lib.JpegHuff))
            t[name][0][length] = v
        return f

    mutated(huff(0, "maxcode", 2, 4))       # no 2-bit code is 4
    mutated(huff(0, "maxcode", 16, -2))
    mutated(huff(0, "valptr", 16, 250))     # values behind huffval
    mutated(huff(0, "mincode", 16, -5))
    assert refused > 150 and _ok(plan)


# ------------------------------------------------------------------------------------------------------------------ fallback bookkeeping
def _stub_launch(monkeypatch, statuses=None):
    """``jpeg._launch`` replaced by the numpy model; ``statuses``: {position among the device images: status}; logs the images per call"""
    return stub_launch(monkeypatch, {"base": lambda r: jpeg_model.decode(r.data)}, lambda kind, records, out, sync: len(records), {"base": statuses or {}})


def test_fallback_bookkeeping_with_a_stub_in_place_of_the_device_call(monkeypatch):
    from hawq_amd.image import decode_image
    from hawq_amd.jpeg import decode_jpeg_batch
    good, bad, _ = cases()
    calls = _stub_launch(monkeypatch, {1: 1})
    srcs = [good["noise_13x17_420"][0], bad["progressive"][0], good["smooth_31x33_gray"][0], bad["png"][0], bad["cmyk"][0], good["noise_40x24_rst4"][0]]
    images, fallbacks = decode_jpeg_batch(srcs, device="cpu")
    assert calls == [3]
    assert fallbacks == [(1, "progressive (SOF2)"), (2, "device status 1: ran out of bytes"), (3, "not a JPEG"), (4, "four components")]
    base = images[0].untyped_storage().data_ptr()
    for i, (im, src) in enumerate(zip(images, srcs)):
        assert torch.equal(im, decode_image(src)), i
        assert im.untyped_storage().data_ptr() == base and im.data_ptr() % 16 == 0 and im.is_contiguous()
    # nothing for the device: no launch; a file neither decoder takes raises as decode_image does
    images, fallbacks = decode_jpeg_batch([bad["png"][0]], device="cpu")
    assert calls == [3] and fallbacks == [(0, "not a JPEG")] and torch.equal(images[0], decode_image(bad["png"][0]))
    with pytest.raises(Exception) as e:
        decode_jpeg_batch([good["flat_24x24"][0], bad["cut_header"][0]], device="cpu")
    with pytest.raises(type(e.value)):
        decode_image(bad["cut_header"][0])


def test_loader_with_device_decode_keeps_order_labels_and_bytes(monkeypatch, tmp_path):
    from hawq_amd import image
    good, bad, _ = cases()
    _stub_launch(monkeypatch)
    files = {"a/0.jpg": good["noise_31x33_444"][0], "a/1.jpg": bad["progressive"][0], "b/0.jpg": good["smooth_40x23_420rst"][0],
             "b/1.png": bad["png"][0], "b/2.jpeg": good["noise_40x24_rst7_gray"][0]}
    for rel, data in files.items():
        (tmp_path / rel).parent.mkdir(exist_ok=True)
        (tmp_path / rel).write_bytes(data)
    seen = []

    def fused(imgs, resize, crop, device=None):   # stands in for the launch: records what it is handed
        seen.append([im.clone() for im in imgs])
        return torch.zeros(len(imgs), crop, crop, 3, dtype=torch.uint8)

    monkeypatch.setattr(image, "preprocess_batch_fused", fused)
    for workers in (0, 2):
        seen.clear()
        got = list(image.folder_loader(str(tmp_path), batch_size=2, resize=24, crop=16, device="cpu", device_decode=True, workers=workers))
        assert [t.tolist() for _, t in got] == [[0, 0], [1, 1], [1]]
        flat = [im for batch in seen for im in batch]
        for im, (rel, data) in zip(flat, sorted(files.items())):
            assert torch.equal(im, image.decode_image(data)), rel


# ------------------------------------------------------------------------------------------------------------------ the kernels' arithmetic on the host
def test_kernel_arithmetic_on_the_host_under_sanitizers_on_valid_and_corrupted_streams(tmp_path):
    """tools/jpeg_host_check.cpp: the header text the kernels compile, built with ASan + UBSan into a program of its own and run as a child
    process on the planner's blob of ALL accepted fixtures: golden bytes for the intact streams, a status and no sanitizer report for every
    truncation at each eighth byte and for 200 single-byte overwrites per stream."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "jpeg_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tools", "jpeg_host_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    plan, names = _plan()
    assert plan.ok()
    good, _, _ = cases()
    expected = np.zeros(plan.out_bytes, np.uint8)
    for n, off in zip(names, plan.out_offsets):
        rgb = good[n][1]
        expected[off:off + rgb.size] = rgb.reshape(-1)
    plan.blob[:plan.nbytes].tofile(str(tmp_path / "blob.bin"))
    expected.tofile(str(tmp_path / "expected.bin"))
    r = subprocess.run([exe, str(tmp_path / "blob.bin"), str(tmp_path / "expected.bin"), str(plan.out_bytes), str(jpeg_model.HOST_CHECK_SEED)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    words = r.stdout.split()
    counts = dict(zip(words[0::2], map(int, words[1::2])))
    assert counts["images"] == counts["exact"] == len(names)
    assert counts["truncations"] == counts["truncations_flagged"] > len(names)
    assert counts["overwrites"] >= 200 * (len(names) - 4)
