"""The many-lane entropy stage of the device JPEG decoder (hawq_jpeg_decode_batch_sync, decode_jpeg_batch(entropy="sync"),
folder_loader(entropy="sync")) on the MI355X: the same int16 coefficients as the serial stage, hence Pillow's bytes
(tests/golden/jpeg_cases.npz and jpeg_sync_cases.npz).  The C ABI runs with every buffer, the scratch included, between poisoned guards
(tests/guard.py).  The two damaged streams are those of tests/test_gpu_jpeg.py, which tools/jpeg_sync_host_check.cpp has decoded in
bounds under the sanitizers at these sub_bytes (tests/test_jpeg_sync_host.py)."""
import functools

import numpy as np
import pytest
import torch

from tests import guard, jpeg_model, jpeg_sync_model
from tests.test_gpu_jpeg import damaged_files, image_of

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0xA5, 0x5A], ids=["poisonA5", "poison5A"])
def arena(request):
    ar = guard.GuardArena("cuda", poison=request.param)
    yield ar
    ar.check()


@functools.lru_cache(maxsize=None)
def everything():
    """{name: (file bytes, Pillow's RGB)} of both archives"""
    both = dict(jpeg_model.cases()[0])
    both.update(jpeg_sync_model.cases()[0])
    return both


@functools.lru_cache(maxsize=None)
def records():
    from hawq_amd.jpeg import parse_jpeg
    return tuple(parse_jpeg(data) for data, _ in everything().values())


def run_sync(ar, recs, sub_bytes, min_sync_bytes):
    """hawq_jpeg_decode_batch_sync on `recs`, every buffer in the arena -> (plan, out, status, coefficient slab, scratch)"""
    from hawq_amd import _lib
    from hawq_amd.jpeg import plan_jpeg_batch
    plan = plan_jpeg_batch(recs, sync=(sub_bytes, min_sync_bytes))
    assert plan.ok() and plan.sync_ok(), _lib.load().hawq_last_error()
    blob = ar.put(plan.blob[:plan.nbytes], "blob")
    coef = ar.empty(plan.coef_blocks * 64, torch.int16, "coef")
    planes = ar.empty(plan.plane_bytes, torch.uint8, "planes")
    out = ar.empty(plan.out_bytes, torch.uint8, "out")
    status = ar.empty(len(recs), torch.int32, "status")
    scratch = ar.empty(plan.scratch_bytes, torch.uint8, "scratch")
    _lib.call("hawq_jpeg_decode_batch_sync", blob.data_ptr(), plan.blob.ctypes.data, plan.nbytes, coef.data_ptr(), plan.coef_blocks, planes.data_ptr(),
              plan.plane_bytes, out.data_ptr(), plan.out_bytes, status.data_ptr(), sub_bytes, min_sync_bytes, plan.jobs_off, plan.n_jobs, scratch.data_ptr(),
              plan.scratch_bytes, None, torch.cuda.current_stream().cuda_stream)
    ar.check()
    return plan, out.cpu().numpy(), status.cpu().numpy(), coef.cpu().numpy(), scratch.cpu().numpy()


def run_serial(ar, recs):
    from hawq_amd import _lib
    from hawq_amd.jpeg import plan_jpeg_batch
    plan = plan_jpeg_batch(recs)
    assert plan.ok(), _lib.load().hawq_last_error()
    blob = ar.put(plan.blob[:plan.nbytes], "blob")
    coef = ar.empty(plan.coef_blocks * 64, torch.int16, "coef")
    planes = ar.empty(plan.plane_bytes, torch.uint8, "planes")
    out = ar.empty(plan.out_bytes, torch.uint8, "out")
    status = ar.empty(len(recs), torch.int32, "status")
    _lib.call("hawq_jpeg_decode_batch", blob.data_ptr(), plan.blob.ctypes.data, plan.nbytes, coef.data_ptr(), plan.coef_blocks, planes.data_ptr(),
              plan.plane_bytes, out.data_ptr(), plan.out_bytes, status.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    ar.check()
    return plan, out.cpu().numpy(), status.cpu().numpy(), coef.cpu().numpy()


def assert_pillow(plan, out, status, poison):
    names = list(everything())
    assert not status.any(), {n: int(s) for n, s in zip(names, status) if s}
    wrong = [n for i, n in enumerate(names) if not np.array_equal(image_of(plan, out, i), everything()[n][1])]
    assert not wrong, wrong
    gaps = np.ones(plan.out_bytes, bool)   # the bytes between two images belong to nobody
    for (h, w), off in zip(plan.sizes, plan.out_offsets):
        gaps[off:off + h * w * 3] = False
    assert np.all(out[gaps] == poison)


@pytest.mark.parametrize("sub_bytes", [16, 128])
def test_all_fixtures_in_one_sync_call_equal_pillow_inside_guards(arena, sub_bytes):
    plan, out, status, _, _ = run_sync(arena, records(), sub_bytes, 64)
    assert plan.n_jobs > 80   # nearly every interval is a job of the many-lane kernel
    assert_pillow(plan, out, status, arena.poison)


@pytest.mark.parametrize("sub_bytes", [16, 128])
def test_the_coefficient_slab_equals_the_serial_decoder_word_for_word(sub_bytes):
    ar = guard.GuardArena("cuda")
    _, _, status, want = run_serial(ar, records())
    _, _, status_sync, got, _ = run_sync(ar, records(), sub_bytes, 64)
    assert not status.any() and not status_sync.any()
    differ = np.flatnonzero(want != got)
    assert differ.size == 0, (differ.size, differ[:8] // 64)


def test_one_call_mixes_serial_and_many_lane_intervals(arena):
    plan, out, status, _, _ = run_sync(arena, records(), 128, 512)
    lengths = np.concatenate([r.intervals[:, 1] - r.intervals[:, 0] for r in records()])
    assert 0 < plan.n_jobs == int((lengths >= 512).sum()) < plan.n_waves   # both kinds occur
    assert any(len(r.intervals) > 1 and (r.intervals[:, 1] - r.intervals[:, 0]).min() >= 512 for r in records())   # restart intervals as jobs
    assert_pillow(plan, out, status, arena.poison)


def test_sample_through_the_api_at_the_default_parameters():
    from hawq_amd.image import decode_image
    from hawq_amd.jpeg import decode_jpeg_batch
    data = jpeg_model.sample()
    images, fallbacks = decode_jpeg_batch([data], entropy="sync")
    assert fallbacks == [] and torch.equal(images[0].cpu(), decode_image(data))


def test_the_kernel_counts_the_rounds_the_model_counts():
    """Lanes that compared non-canonical states, or a loop that ended early before a lucky write pass, would count otherwise."""
    from hawq_amd.jpeg import parse_jpeg
    good, cond = jpeg_sync_model.cases()
    names = ["flat_320x240", "noise_144x104_q95_420", "noise_64x48_q100", "noise_96x64_rstrow"]
    ar = guard.GuardArena("cuda")
    for sub_bytes in (16, 128):
        plan, _, status, _, scratch = run_sync(ar, [parse_jpeg(good[n][0]) for n in names], sub_bytes, 64)
        assert not status.any()
        got_n = [n_sub for _, n_sub, _ in plan.jobs]
        got_rounds = [int(scratch[off:off + 4].view(np.int32)[0]) for _, _, off in plan.jobs]
        want = [cond["lanes"][n][str(sub_bytes)] for n in names]
        assert got_n == sum((w["n"] for w in want), []) and got_rounds == sum((w["rounds"] for w in want), []), (sub_bytes, got_n, got_rounds)
        assert got_rounds[0] == got_n[0]   # the flat image never synchronises
    assert cond["lanes"]["noise_144x104_q95_420"]["16"]["n"][0] > 1024   # every thread loops


def test_damaged_streams_report_a_status_beside_good_images_inside_guards(arena):
    from hawq_amd.jpeg import parse_jpeg
    good, _, _ = jpeg_model.cases()
    files = damaged_files()
    plan, out, status, _, _ = run_sync(arena, [parse_jpeg(f) for f in files], 16, 64)
    assert plan.n_jobs >= 3
    assert status[0] == 0 and status[3] == 0 and status[1] != 0 and status[2] != 0, status.tolist()
    assert np.array_equal(image_of(plan, out, 0), good["smooth_31x33_420"][1]) and np.array_equal(image_of(plan, out, 3), good["noise_40x24_rst4"][1])


@pytest.mark.parametrize("workers", [0, 2])
def test_folder_loader_with_sync_entropy_equals_the_fused_loader(tmp_path, workers):
    from hawq_amd.image import folder_loader
    good, bad, _ = jpeg_model.cases()
    picks = ["noise_1x1_444", "smooth_8x8_gray", "noise_13x17_422", "noise_16x16_420rst", "smooth_31x33_opt95", "noise_40x23_q30", "flat_24x24",
             "checker_32x32_q30", "noise_40x24_q100", "noise_40x24_rst7_gray", "noise_65x9_420"]
    for k, n in enumerate(picks):
        d = tmp_path / ("class%d" % (k % 3))
        d.mkdir(exist_ok=True)
        (d / (n + ".jpg")).write_bytes(good[n][0])
    (tmp_path / "class0" / "sample.jpeg").write_bytes(jpeg_model.sample())
    (tmp_path / "class1" / "progressive.jpg").write_bytes(bad["progressive"][0])
    (tmp_path / "class2" / "picture.png").write_bytes(bad["png"][0])
    ref = list(folder_loader(str(tmp_path), batch_size=5, resize=40, crop=32, fused=True, workers=workers))
    got = list(folder_loader(str(tmp_path), batch_size=5, resize=40, crop=32, device_decode=True, entropy="sync", workers=workers))
    assert len(got) == len(ref) == 3
    for (gb, gt), (rb, rt) in zip(got, ref):
        assert gb.is_cuda and gb.dtype == torch.uint8 and torch.equal(gt, rt)
        assert torch.equal(gb.cpu(), rb.cpu())
