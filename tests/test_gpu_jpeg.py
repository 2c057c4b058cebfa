"""The batched device JPEG decoder (hawq_jpeg_decode_batch, hawq_amd.jpeg.decode_jpeg_batch, folder_loader(device_decode=True)) on the
MI355X: every output byte equals what Pillow decodes (tests/golden/jpeg_cases.npz, make_jpeg_cases.py).  The C ABI runs with every
buffer between poisoned guards (tests/guard.py).  The two damaged streams of the last ABI test are streams tools/jpeg_host_check.cpp
has already decoded in bounds under the sanitizers (tests/test_jpeg_host.py): here they must report a status, not fault."""

import numpy as np
import pytest
import torch

from tests import guard, jpeg_model
from tests.jpeg_model import cases, sample

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0xA5, 0x5A], ids=["poisonA5", "poison5A"])
def arena(request):
    ar = guard.GuardArena("cuda", poison=request.param)
    yield ar
    ar.check()


def run_abi(ar, records):
    """hawq_jpeg_decode_batch on `records` with blob, coefficient slab, planes, output and status in the arena -> (plan, out, status)"""
    from hawq_amd import _lib
    from hawq_amd.jpeg import plan_jpeg_batch
    plan = plan_jpeg_batch(records)
    assert plan.ok(), _lib.load().hawq_last_error()
    blob = ar.put(plan.blob[:plan.nbytes], "blob")
    coef = ar.empty(plan.coef_blocks * 64, torch.int16, "coef")
    planes = ar.empty(plan.plane_bytes, torch.uint8, "planes")
    out = ar.empty(plan.out_bytes, torch.uint8, "out")
    status = ar.empty(len(records), torch.int32, "status")
    _lib.call("hawq_jpeg_decode_batch", blob.data_ptr(), plan.blob.ctypes.data, plan.nbytes, coef.data_ptr(), plan.coef_blocks, planes.data_ptr(),
              plan.plane_bytes, out.data_ptr(), plan.out_bytes, status.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    ar.check()
    return plan, out.cpu().numpy(), status.cpu().numpy()


def image_of(plan, out, i):
    h, w = plan.sizes[i]
    return out[plan.out_offsets[i]:plan.out_offsets[i] + h * w * 3].reshape(h, w, 3)


def test_all_accepted_fixtures_in_one_call_equal_pillow_inside_guards(arena):
    from hawq_amd.jpeg import parse_jpeg
    good, _, _ = cases()
    names = list(good)
    plan, out, status = run_abi(arena, [parse_jpeg(good[n][0]) for n in names])
    assert not status.any(), {n: int(s) for n, s in zip(names, status) if s}
    wrong = [n for i, n in enumerate(names) if not np.array_equal(image_of(plan, out, i), good[n][1])]
    assert not wrong, wrong
    # the bytes between two images belong to nobody
    gaps = np.ones(plan.out_bytes, bool)
    for (h, w), off in zip(plan.sizes, plan.out_offsets):
        gaps[off:off + h * w * 3] = False
    assert np.all(out[gaps] == arena.poison)


def test_restart_fixtures_run_several_waves_per_image_and_give_the_same_bytes():
    from hawq_amd.jpeg import decode_jpeg_batch, parse_jpeg, plan_jpeg_batch
    good, _, _ = cases()
    names = [n for n in good if "rst" in n and len(parse_jpeg(good[n][0]).intervals) > 1]   # 1x1 .. 16x16 at 4:2:0 are one MCU
    recs = [parse_jpeg(good[n][0]) for n in names]
    assert len(names) >= 8 and {(r.hs, r.vs, r.ncomp) for r in recs} == {(1, 1, 3), (2, 1, 3), (2, 2, 3), (1, 1, 1)}
    assert any(r.mcus_x * r.mcus_y % r.restart for r in recs)   # a last interval shorter than the others
    assert plan_jpeg_batch(recs).n_waves == sum(len(r.intervals) for r in recs) > 2 * len(recs)
    images, fallbacks = decode_jpeg_batch([good[n][0] for n in names])
    assert fallbacks == []
    wrong = [n for n, im in zip(names, images) if not np.array_equal(im.cpu().numpy(), good[n][1])]
    assert not wrong, wrong


def test_mixed_batch_equals_decode_image_and_names_exactly_the_refused(tmp_path):
    from hawq_amd.image import decode_image
    from hawq_amd.jpeg import decode_jpeg_batch
    good, bad, _ = cases()
    (tmp_path / "sample.jpg").write_bytes(sample())
    srcs = [good["noise_31x33_420"][0], bad["progressive"][0], good["smooth_40x23_gray"][0], bad["cmyk"][0], str(tmp_path / "sample.jpg"),
            bad["png"][0], good["noise_40x24_rst2"][0], good["checker_32x32_q30"][0], good["noise_13x17_opt95"][0]]
    images, fallbacks = decode_jpeg_batch(srcs)
    assert fallbacks == [(1, "progressive (SOF2)"), (3, "four components"), (5, "not a JPEG")]
    base = images[0].untyped_storage().data_ptr()
    for i, (im, src) in enumerate(zip(images, srcs)):
        assert im.is_cuda and im.dtype == torch.uint8 and im.is_contiguous() and im.data_ptr() % 16 == 0
        assert im.untyped_storage().data_ptr() == base   # one allocation
        assert torch.equal(im.cpu(), decode_image(src)), i
    for i in (1, 3, 5):
        assert np.array_equal(images[i].cpu().numpy(), bad[("progressive", "cmyk", "png")[(1, 3, 5).index(i)]][2])


def damaged_files():
    """(good A, truncated, overwritten, good B): the damaged two are streams the host checker runs (a cut at a multiple of eight bytes of
    fixture T's stream; one of its seeded overwrites of fixture O's) that ``parse_jpeg`` still accepts and the numpy model cannot decode."""
    from hawq_amd.jpeg import UnsupportedJpeg, parse_jpeg
    good, _, _ = cases()
    names = list(good)
    t_name, o_name = "noise_31x33_444", "noise_40x23_422"
    data = good[t_name][0]
    r = parse_jpeg(data)
    cut = (r.scan[1] - r.scan[0]) // 2 & ~7
    truncated = data[:r.scan[0] + cut] + data[r.scan[1]:]
    rt = parse_jpeg(truncated)
    assert rt.intervals.tolist() == [[0, cut]]
    data = good[o_name][0]
    r = parse_jpeg(data)
    for at, value in jpeg_model.overwrite_draws(jpeg_model.HOST_CHECK_SEED, names.index(o_name), r.scan[1] - r.scan[0]):
        damaged = data[:r.scan[0] + at] + bytes([value]) + data[r.scan[0] + at + 1:]
        try:
            ro = parse_jpeg(damaged)
        except UnsupportedJpeg:
            continue
        if ro.scan != r.scan or not np.array_equal(ro.intervals, r.intervals):
            continue
        try:
            jpeg_model.decode(damaged)
        except (ValueError, IndexError):
            return good["smooth_31x33_420"][0], truncated, damaged, good["noise_40x24_rst4"][0]
    raise AssertionError("no overwrite of the host checker's draws damages the stream")


def test_damaged_streams_report_a_status_beside_good_images_inside_guards(arena):
    from hawq_amd.jpeg import parse_jpeg
    good, _, _ = cases()
    files = damaged_files()
    plan, out, status = run_abi(arena, [parse_jpeg(f) for f in files])
    assert status[0] == 0 and status[3] == 0 and status[1] != 0 and status[2] != 0, status.tolist()
    assert np.array_equal(image_of(plan, out, 0), good["smooth_31x33_420"][1]) and np.array_equal(image_of(plan, out, 3), good["noise_40x24_rst4"][1])


def test_api_hands_damaged_streams_to_the_host_decoder():
    from hawq_amd.image import decode_image
    from hawq_amd.jpeg import decode_jpeg_batch
    a, truncated, damaged, b = damaged_files()
    for bad_file in (truncated, damaged):
        try:
            want = decode_image(bad_file)
        except Exception as e:   # Pillow refuses it: so must the batch
            with pytest.raises(type(e)):
                decode_jpeg_batch([a, bad_file, b])
            continue
        images, fallbacks = decode_jpeg_batch([a, bad_file, b])
        assert [i for i, _ in fallbacks] == [1] and fallbacks[0][1].startswith("device status ")
        assert torch.equal(images[1].cpu(), want)
        assert torch.equal(images[0].cpu(), decode_image(a)) and torch.equal(images[2].cpu(), decode_image(b))


@pytest.mark.parametrize("workers", [0, 2])
def test_folder_loader_with_device_decode_equals_the_fused_loader(tmp_path, workers):
    from hawq_amd.image import folder_loader
    good, bad, _ = cases()
    picks = ["noise_1x1_444", "smooth_8x8_gray", "noise_13x17_422", "noise_16x16_420rst", "smooth_31x33_opt95", "noise_40x23_q30", "flat_24x24",
             "checker_32x32_q30", "noise_40x24_q100", "noise_40x24_rst7_gray", "noise_65x9_420"]
    for k, n in enumerate(picks):
        d = tmp_path / ("class%d" % (k % 3))
        d.mkdir(exist_ok=True)
        (d / (n + ".jpg")).write_bytes(good[n][0])
    (tmp_path / "class0" / "sample.jpeg").write_bytes(sample())
    (tmp_path / "class1" / "progressive.jpg").write_bytes(bad["progressive"][0])
    (tmp_path / "class2" / "picture.png").write_bytes(bad["png"][0])
    ref = list(folder_loader(str(tmp_path), batch_size=5, resize=40, crop=32, fused=True, workers=workers))
    got = list(folder_loader(str(tmp_path), batch_size=5, resize=40, crop=32, device_decode=True, workers=workers))
    assert len(got) == len(ref) == 3
    for (gb, gt), (rb, rt) in zip(got, ref):
        assert gb.is_cuda and gb.dtype == torch.uint8 and torch.equal(gt, rt)
        assert torch.equal(gb.cpu(), rb.cpu())
