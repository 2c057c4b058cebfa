"""Host side of the many-lane entropy stage of the device JPEG decoder (csrc/jpeg_sync.h, hawq_jpeg_sync_ok, decode_jpeg_batch(entropy=
"sync")) without a GPU: the Python model of the scheme against the serial model, the kernel's own lane function compiled
into a stand-alone program under AddressSanitizer + UBSan against the serial decoder on valid and on corrupted streams, the job-table
checker, and the fallback bookkeeping with a stub in place of the device call."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import jpeg_model, jpeg_sync_model
from tests.jpeg_stub import stub_launch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def everything():
    both = dict(jpeg_model.cases()[0])
    both.update(jpeg_sync_model.cases()[0])
    return both


def test_the_fixture_set_holds_what_makes_it_meaningful():
    good, cond = jpeg_sync_model.cases()
    assert all(cond["shows"][k] for k in ("n_above_1024", "rounds_equal_n", "rounds_below_quarter_n", "boundary_on_stuffed_zero", "length_no_multiple",
                                          "start_inside_block", "start_in_chroma", "bytes_behind_last_block", "restart_intervals_above_256")), cond["shows"]
    assert set(cond["lanes"]) == set(good) and len(good) >= 10
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_sync_cases.npz")) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))


@pytest.mark.parametrize("sub_bytes", [16, 128])
def test_the_models_fixed_point_equals_the_serial_model_on_every_case_and_the_sample(sub_bytes):
    from hawq_amd.jpeg import parse_jpeg
    _, cond = jpeg_sync_model.cases()
    files = {name: data for name, (data, _) in everything().items()}
    files["sample"] = jpeg_model.sample()
    for name, data in files.items():
        rec = parse_jpeg(data)
        report = {}
        got = jpeg_sync_model.coefficients(rec, sub_bytes, report)
        assert all(np.array_equal(a, b) for a, b in zip(jpeg_model.coefficients(rec), got)), name
        for r in report["intervals"]:
            assert 1 <= r["rounds"] <= r["n"] and r["decodes"] >= r["n"], name
        if name in cond["lanes"]:   # what the make script recorded, and the GPU test compares the kernel's count with
            want = cond["lanes"][name][str(sub_bytes)]
            assert [r["n"] for r in report["intervals"]] == want["n"] and [r["rounds"] for r in report["intervals"]] == want["rounds"], name


def test_lane_function_on_the_host_under_sanitizers_equals_the_serial_decoder_on_valid_and_corrupted_streams(tmp_path):
    """tools/jpeg_sync_host_check.cpp: jpeg_sync.h as the kernel compiles it, built with ASan + UBSan into a program of its own and run as
    child processes (each takes every eighth image) on the planner's blob of ALL accepted fixtures of both archives: equal slabs and status
    at sub_bytes 16 / 32 / 64 / 128, equal status (and slabs where it is zero) for every truncation at each eighth byte and 200 single-byte
    overwrites per stream at 16 / 128, a lane decode only where a start changed, and the round counts of the Python model."""
    from hawq_amd.jpeg import parse_jpeg, plan_jpeg_batch
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "jpeg_sync_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tools", "jpeg_sync_host_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    names = list(everything())
    plan = plan_jpeg_batch([parse_jpeg(everything()[n][0]) for n in names])
    assert plan.ok()
    plan.blob[:plan.nbytes].tofile(str(tmp_path / "blob.bin"))
    step = 8
    procs = [subprocess.Popen([exe, str(tmp_path / "blob.bin"), str(jpeg_model.HOST_CHECK_SEED), str(k), str(step)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True) for k in range(step)]
    counts, rounds = {}, {}
    for p in procs:
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0 and not err, (p.returncode, out[-2000:], err[-4000:])
        for line in out.splitlines():
            words = line.split()
            if words[0] == "image":
                rounds[(names[int(words[1])], int(words[3]))] = (int(words[5]), int(words[7]))
            else:
                for key, value in zip(words[0::2], words[1::2]):
                    counts[key] = counts.get(key, 0) + int(value)
    assert counts["images"] == len(names) and counts["runs"] == counts["equal"] == 4 * len(names)
    assert counts["truncations"] == counts["truncations_equal"] > 2 * len(names)
    # every cut costs the image a block - but for the cuts inside the 40 bytes behind the last block of noise_64x48_444_tail, at two sub_bytes
    assert 0 <= counts["truncations"] - counts["truncations_flagged"] <= 2 * (40 // 8 + 1)
    assert counts["overwrites"] == counts["overwrites_equal"] >= 2 * 200 * (len(names) - 4) and counts["overwrites_flagged"] > 0
    assert counts["overruns"] == 0 and counts["hostile_overruns"] == 0
    assert counts["decodes"] == counts["lanes"] + counts["changes"] and counts["hostile_decodes"] == counts["hostile_lanes"] + counts["hostile_changes"]
    _, cond = jpeg_sync_model.cases()
    for name, lanes in cond["lanes"].items():   # (n, rounds) of the file's last interval, as the Python model counted them
        for sub_bytes in (16, 128):
            assert rounds[(name, sub_bytes)] == (lanes[str(sub_bytes)]["n"][-1], lanes[str(sub_bytes)]["rounds"][-1]), (name, sub_bytes)


# ------------------------------------------------------------------------------------------------------------------ the job-table checker
def _plan(sync=(16, 256)):
    from hawq_amd.jpeg import parse_jpeg, plan_jpeg_batch
    good, _, _ = jpeg_model.cases()
    more, _ = jpeg_sync_model.cases()
    files = [good["noise_13x17_420"][0], more["noise_96x64_rstrow"][0], good["noise_40x24_rst4"][0], more["noise_64x48_422"][0], good["smooth_31x33_gray"][0]]
    return plan_jpeg_batch([parse_jpeg(f) for f in files], sync=sync)


def _ok(plan, blob=None, sub_bytes=None, min_sync_bytes=None, jobs_off=None, n_jobs=None, scratch_bytes=None):
    from hawq_amd import _lib
    pick = lambda v, d: d if v is None else v
    blob = plan.blob if blob is None else blob
    ok = bool(_lib.load().hawq_jpeg_sync_ok(blob.ctypes.data, plan.nbytes, pick(sub_bytes, plan.sub_bytes), pick(min_sync_bytes, plan.min_sync_bytes),
                                            pick(jobs_off, plan.jobs_off), pick(n_jobs, plan.n_jobs), pick(scratch_bytes, plan.scratch_bytes)))
    if not ok:
        assert _lib.load().hawq_last_error().startswith(b"hawq_jpeg_decode_batch"), _lib.load().hawq_last_error()
    return ok


def test_planner_appends_the_job_table_and_the_checker_passes_it():
    from hawq_amd import _lib
    from hawq_amd.jpeg import parse_jpeg, plan_jpeg_batch
    plan = _plan()
    assert plan.ok() and plan.sync_ok() and plan.jobs_off % 16 == 0 and plan.nbytes % 16 == 0
    assert 0 < plan.n_jobs < plan.n_waves   # long and short intervals
    jobs = plan.blob[plan.jobs_off:plan.jobs_off + 16 * plan.n_jobs].view(np.dtype(_lib.JpegSyncJob))
    assert [(int(j["wave"]), int(j["n_sub"]), int(j["scratch_off"])) for j in jobs] == plan.jobs
    at = 0
    for wave, n_sub, off in plan.jobs:
        assert off == at and off % 16 == 0
        at += 16 + 32 * n_sub
    assert at == plan.scratch_bytes and C.sizeof(_lib.JpegSyncSub) == 32 and C.sizeof(_lib.JpegSyncJob) == 16
    # without `sync` the blob is the one it was, byte for byte, and the plan says so
    records = [parse_jpeg(d) for d, _ in list(jpeg_model.cases()[0].values())[:12]]
    old, new = plan_jpeg_batch(records), plan_jpeg_batch(records, sync=(32, 4096))
    assert old.n_jobs == 0 and old.scratch_bytes == 0 and new.n_jobs == 0 and new.sync_ok()
    assert np.array_equal(old.blob[:old.nbytes], new.blob[:old.nbytes]) and new.nbytes == old.nbytes
    every = plan_jpeg_batch([parse_jpeg(d) for d, _ in everything().values()], sync=(128, 512))
    assert every.ok() and every.sync_ok() and 0 < every.n_jobs < every.n_waves
    with pytest.raises(ValueError):
        plan_jpeg_batch(records, sync=(18, 64))


def test_checker_refuses_a_job_table_that_does_not_follow_from_the_blob():
    from hawq_amd import _lib
    plan = _plan()
    assert _ok(plan)
    for bad in (0, 12, 18, 4100, 8192, -16):
        assert not _ok(plan, sub_bytes=bad), bad
    assert not _ok(plan, sub_bytes=32)           # every n_sub is wrong now
    assert not _ok(plan, min_sync_bytes=0)
    assert not _ok(plan, min_sync_bytes=32)      # short intervals that would need a job
    assert not _ok(plan, min_sync_bytes=1 << 20) # jobs on intervals shorter than that
    assert not _ok(plan, scratch_bytes=plan.scratch_bytes - 1) and _ok(plan, scratch_bytes=plan.scratch_bytes + 16)
    assert not _ok(plan, n_jobs=plan.n_jobs - 1) and not _ok(plan, n_jobs=plan.n_jobs + 1) and not _ok(plan, n_jobs=-1)
    assert not _ok(plan, jobs_off=plan.jobs_off + 8) and not _ok(plan, jobs_off=plan.nbytes) and not _ok(plan, jobs_off=-16)
    refused = 0

    def mutated(k, field, value):
        nonlocal refused
        blob = plan.blob.copy()
        blob[plan.jobs_off:plan.jobs_off + 16 * plan.n_jobs].view(np.dtype(_lib.JpegSyncJob))[field][k] = value
        assert not _ok(plan, blob), (k, field, value)
        refused += 1

    short = next(w for w in range(plan.n_waves) if w not in [j[0] for j in plan.jobs])
    last = plan.n_jobs - 1
    mutated(last, "wave", plan.n_waves)          # a wave that does not exist
    mutated(0, "wave", -1)
    mutated(1, "wave", plan.jobs[0][0])          # the same wave twice
    mutated(0, "wave", plan.jobs[1][0])          # out of order
    mutated(0 if short < plan.jobs[0][0] else last, "wave", short)   # an interval shorter than min_sync_bytes
    for k in (0, last):
        mutated(k, "n_sub", plan.jobs[k][1] + 1)
        mutated(k, "n_sub", plan.jobs[k][1] - 1)
        mutated(k, "n_sub", 0)
    mutated(1, "scratch_off", plan.jobs[1][2] - 16)   # overlaps the job before it
    mutated(1, "scratch_off", plan.jobs[1][2] + 8)    # unaligned
    mutated(0, "scratch_off", -16)
    mutated(last, "scratch_off", plan.jobs[last][2] + 16)   # runs past scratch_bytes
    mutated(last, "scratch_off", 1 << 40)
    assert refused == 16 and _ok(plan)


# ------------------------------------------------------------------------------------------------------------------ fallback bookkeeping
def _stub_launch(monkeypatch, statuses=None):
    """``jpeg._launch`` replaced by the numpy model; ``statuses``: {position among the device images: status}; logs (images, sync) per call"""
    return stub_launch(monkeypatch, {"base": lambda r: jpeg_model.decode(r.data)}, lambda kind, records, out, sync: (len(records), sync), {"base": statuses or {}})


def test_fallback_bookkeeping_is_the_same_with_either_entropy_stage(monkeypatch):
    from hawq_amd import jpeg
    from hawq_amd.image import decode_image
    good, bad, _ = jpeg_model.cases()
    calls = _stub_launch(monkeypatch, {1: 1})
    srcs = [good["noise_13x17_420"][0], bad["progressive"][0], good["smooth_31x33_gray"][0], bad["png"][0], bad["cmyk"][0], good["noise_40x24_rst4"][0]]
    serial_images, serial_fallbacks = jpeg.decode_jpeg_batch(srcs, device="cpu")
    images, fallbacks = jpeg.decode_jpeg_batch(srcs, device="cpu", entropy="sync")
    assert fallbacks == serial_fallbacks == [(1, "progressive (SOF2)"), (2, "device status 1: ran out of bytes"), (3, "not a JPEG"), (4, "four components")]
    assert calls == [(3, None), (3, (jpeg.SUB_BYTES, jpeg.MIN_SYNC_BYTES))]
    for i, (a, b, src) in enumerate(zip(images, serial_images, srcs)):
        assert torch.equal(a, b) and torch.equal(a, decode_image(src)), i
    jpeg.decode_jpeg_batch(srcs, device="cpu", entropy="sync", sub_bytes=64, min_sync_bytes=256)
    assert calls[-1] == (3, (64, 256))
    with pytest.raises(ValueError):
        jpeg.decode_jpeg_batch(srcs, device="cpu", entropy="bogus")
    with pytest.raises(ValueError):
        jpeg.decode_jpeg_batch(srcs, device="cpu", sub_bytes=64)   # belongs to entropy="sync"
    assert len(calls) == 3


def test_loader_passes_the_entropy_option_through(monkeypatch, tmp_path):
    from hawq_amd import image, jpeg
    good, _, _ = jpeg_model.cases()
    calls = _stub_launch(monkeypatch)
    for k, n in enumerate(("noise_31x33_444", "smooth_40x23_420rst", "noise_40x24_rst7_gray")):
        (tmp_path / ("c%d" % k)).mkdir()
        (tmp_path / ("c%d" % k) / "0.jpg").write_bytes(good[n][0])
    monkeypatch.setattr(image, "preprocess_batch_fused", lambda imgs, resize, crop, device=None: torch.zeros(len(imgs), crop, crop, 3, dtype=torch.uint8))
    list(image.folder_loader(str(tmp_path), batch_size=2, resize=24, crop=16, device="cpu", device_decode=True))
    list(image.folder_loader(str(tmp_path), batch_size=2, resize=24, crop=16, device="cpu", device_decode=True, entropy="sync"))
    assert calls == [(2, None), (1, None), (2, (jpeg.SUB_BYTES, jpeg.MIN_SYNC_BYTES)), (1, (jpeg.SUB_BYTES, jpeg.MIN_SYNC_BYTES))]
