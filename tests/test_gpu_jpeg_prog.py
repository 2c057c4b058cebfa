"""The progressive device JPEG decoder (hawq_jpeg_decode_batch_prog, hawq_amd.jpeg.decode_jpeg_batch(progressive=True),
folder_loader(device_decode=True, progressive=True)) on the MI355X: every output byte equals what Pillow decodes
(tests/golden/jpeg_prog_cases.npz, make_jpeg_prog_cases.py), and every word of the coefficient slab equals the Python model's.  The C ABI
runs with every buffer between poisoned guards (tests/guard.py).  The two damaged streams of the last ABI test are streams
tools/jpeg_prog_host_check.cpp has already decoded in bounds under the sanitizers (tests/test_jpeg_prog_host.py): here they must report
a status, not fault."""

import numpy as np
import pytest
import torch

from tests import guard, jpeg_model
from tests import jpeg_prog_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0xA5, 0x5A], ids=["poisonA5", "poison5A"])
def arena(request):
    ar = guard.GuardArena("cuda", poison=request.param)
    yield ar
    ar.check()


def run_abi(ar, records):
    """hawq_jpeg_decode_batch_prog on `records` with blob, coefficient slab, planes, output and status in the arena
    -> (plan, out, status, coefficient slab)"""
    from hawq_amd import _lib
    from hawq_amd.jpeg import plan_jpeg_prog_batch
    plan = plan_jpeg_prog_batch(records)
    assert plan.ok(), _lib.load().hawq_last_error()
    blob = ar.put(plan.blob[:plan.nbytes], "blob")
    coef = ar.empty(plan.coef_blocks * 64, torch.int16, "coef")
    planes = ar.empty(plan.plane_bytes, torch.uint8, "planes")
    out = ar.empty(plan.out_bytes, torch.uint8, "out")
    status = ar.empty(len(records), torch.int32, "status")
    _lib.call("hawq_jpeg_decode_batch_prog", blob.data_ptr(), plan.blob.ctypes.data, plan.nbytes, coef.data_ptr(), plan.coef_blocks, planes.data_ptr(),
              plan.plane_bytes, out.data_ptr(), plan.out_bytes, status.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    ar.check()
    return plan, out.cpu().numpy(), status.cpu().numpy(), coef.cpu().numpy()


def image_of(plan, out, i):
    h, w = plan.sizes[i]
    return out[plan.out_offsets[i]:plan.out_offsets[i] + h * w * 3].reshape(h, w, 3)


def wrong_slabs(names, coef):
    """the cases whose words of the coefficient slab differ from the model's (padding blocks included)"""
    models = M.model_coefficients()
    wrong, at = [], 0
    for n in names:
        want = M.slab(models[n][1])
        if not np.array_equal(coef[at:at + want.size], want):
            wrong.append((n, int(np.flatnonzero(coef[at:at + want.size] != want)[0])))
        at += want.size
    assert at == coef.size
    return wrong


def test_all_accepted_fixtures_in_one_call_equal_pillow_inside_guards(arena):
    good, _, _ = M.cases()
    models = M.model_coefficients()
    names = list(good)
    plan, out, status, _ = run_abi(arena, [models[n][0] for n in names])
    assert plan.n_levels == 5
    assert not status.any(), {n: int(s) for n, s in zip(names, status) if s}
    wrong = [n for i, n in enumerate(names) if not np.array_equal(image_of(plan, out, i), good[n][1])]
    assert not wrong, wrong
    # the bytes between two images belong to nobody
    gaps = np.ones(plan.out_bytes, bool)
    for (h, w), off in zip(plan.sizes, plan.out_offsets):
        gaps[off:off + h * w * 3] = False
    assert np.all(out[gaps] == arena.poison)


def test_coefficient_slab_equals_the_models_word_for_word(arena):
    """a single-component scan walked on the padded grid, or a padding block that received more than its DC, would hide behind the crop"""
    models = M.model_coefficients()
    names = [n for n in models if "flat" not in n]
    _, _, status, coef = run_abi(arena, [models[n][0] for n in names])
    assert not status.any()
    assert wrong_slabs(names, coef) == []


def test_images_of_one_three_and_five_levels_in_one_batch(arena):
    good, _, _ = M.cases()
    models = M.model_coefficients()
    names = ["spectral_33x31_420", "noise_16x16_420", "deep_33x31_420", "spectral_9x65_gray"]
    plan, out, status, coef = run_abi(arena, [models[n][0] for n in names])
    per_image = [max(lv for lv, n in zip(plan.levels, [n for n in names for _ in models[n][0].scans]) if n == name) for name in names]
    assert per_image == [1, 3, 5, 1] and plan.n_levels == 5 and np.diff(plan.level_start).tolist() == [12 + 5 + 4 + 4, 4 + 4, 1 + 4, 4, 4]
    assert not status.any()
    assert [n for i, n in enumerate(names) if not np.array_equal(image_of(plan, out, i), good[n][1])] == []
    assert wrong_slabs(names, coef) == []   # the levels beyond an image's own left it alone


def mixed_sources(tmp_path):
    good, bad, _ = M.cases()
    base, base_bad, _ = jpeg_model.cases()
    (tmp_path / "sample.jpg").write_bytes(jpeg_model.sample())
    srcs = [base["noise_31x33_420"][0], good["noise_33x31_420"][0], base_bad["cmyk"][0], good["noise_40x24_gray_rst"][0], str(tmp_path / "sample.jpg"),
            bad["cut_last_scan"][0], base_bad["png"][0], good["deep_31x33_444_smooth"][0], base["noise_40x24_rst2"][0], good["dri_40x24_420"][0], bad["adobe"][0]]
    return srcs, [(2, "four components"), (5, "progression"), (6, "not a JPEG"), (10, "Adobe marker")]


@pytest.mark.parametrize("entropy", ["serial", "sync"])
def test_mixed_batch_equals_decode_image_and_only_the_refused_fall_back(tmp_path, entropy):
    from hawq_amd.image import decode_image, preprocess_batch_fused
    from hawq_amd.jpeg import decode_jpeg_batch
    srcs, refused = mixed_sources(tmp_path)
    more = {"min_sync_bytes": 64} if entropy == "sync" else {}
    images, fallbacks = decode_jpeg_batch(srcs, entropy=entropy, progressive=True, **more)
    assert fallbacks == refused
    want = [decode_image(s) for s in srcs]
    base = images[0].untyped_storage().data_ptr()
    for i, (im, ref) in enumerate(zip(images, want)):
        assert im.is_cuda and im.dtype == torch.uint8 and im.is_contiguous() and im.data_ptr() % 16 == 0
        assert im.untyped_storage().data_ptr() == base   # one allocation
        assert torch.equal(im.cpu(), ref), i
    assert torch.equal(preprocess_batch_fused(images, 40, 32).cpu(), preprocess_batch_fused(want, 40, 32).cpu())   # read in place
    # without the option the progressive files are the host's, as before
    _, fallbacks = decode_jpeg_batch(srcs, entropy=entropy, **more)
    assert [i for i, _ in fallbacks] == [1, 2, 3, 5, 6, 7, 9, 10] and all(r == "progressive (SOF2)" for i, r in fallbacks if i in (1, 3, 5, 7, 9, 10))


@pytest.mark.parametrize("workers", [0, 2])
def test_folder_loader_with_progressive_equals_the_fused_loader(tmp_path, workers):
    from hawq_amd.image import folder_loader
    good, bad, _ = M.cases()
    base, base_bad, _ = jpeg_model.cases()
    picks = [(good, n) for n in ("noise_1x1_444", "noise_7x9_gray", "noise_13x17_422", "noise_40x24_420_rst", "smooth_33x31_444", "checker_32x32_q30", "deep_33x31_420",
                                 "tables_13x17_422", "dri_40x24_gray", "noise_65x9_444")]
    picks += [(base, n) for n in ("noise_13x17_422", "noise_40x24_rst7_gray", "flat_24x24")]
    for k, (src, n) in enumerate(picks):
        d = tmp_path / ("class%d" % (k % 3))
        d.mkdir(exist_ok=True)
        (d / ("%02d_%s.jpg" % (k, n))).write_bytes(src[n][0])
    (tmp_path / "class1" / "incomplete.jpg").write_bytes(bad["cut_last_scan"][0])
    (tmp_path / "class2" / "picture.png").write_bytes(base_bad["png"][0])
    ref = list(folder_loader(str(tmp_path), batch_size=6, resize=40, crop=32, fused=True, workers=workers))
    got = list(folder_loader(str(tmp_path), batch_size=6, resize=40, crop=32, device_decode=True, progressive=True, workers=workers))
    assert len(got) == len(ref) == 3
    for (gb, gt), (rb, rt) in zip(got, ref):
        assert gb.is_cuda and gb.dtype == torch.uint8 and torch.equal(gt, rt)
        assert torch.equal(gb.cpu(), rb.cpu())


T_NAME, T_SCAN, O_NAME, O_SCAN = "noise_33x31_420", 4, "noise_40x24_422_rst", 5   # Y 6-63 first pass; Y 1-63 refinement with restart markers


def damaged_files():
    """(good A, truncated, overwritten, good B): the damaged two are streams the host checker runs - scan T_SCAN of T_NAME cut at a
    multiple of eight bytes, and the first of the checker's seeded overwrites of scan O_SCAN of O_NAME that ``parse_jpeg`` still accepts
    with the same intervals and the Python model cannot decode."""
    from hawq_amd.jpeg import UnsupportedJpeg, parse_jpeg
    good, _, _ = M.cases()
    models = M.model_coefficients()
    names = list(good)
    data = good[T_NAME][0]
    s = models[T_NAME][0].scans[T_SCAN]
    cut = (s.scan[1] - s.scan[0]) // 2 & ~7
    assert cut > 0
    truncated = data[:s.scan[0] + cut] + data[s.scan[1]:]
    assert parse_jpeg(truncated, progressive=True).scans[T_SCAN].intervals.tolist() == [[0, cut]]
    data = good[O_NAME][0]
    rec = models[O_NAME][0]
    s = rec.scans[O_SCAN]
    index = sum(len(models[n][0].scans) for n in names[:names.index(O_NAME)]) + O_SCAN   # in the scan table of the blob of all fixtures
    for at, value in M.overwrite_draws(M.HOST_CHECK_SEED, index, s.scan[1] - s.scan[0]):
        damaged = data[:s.scan[0] + at] + bytes([value]) + data[s.scan[0] + at + 1:]
        try:
            ro = parse_jpeg(damaged, progressive=True)
        except UnsupportedJpeg:
            continue
        if [x.scan for x in ro.scans] != [x.scan for x in rec.scans] or not np.array_equal(ro.scans[O_SCAN].intervals, s.intervals):
            continue
        try:
            M.coefficients(ro)
        except (ValueError, IndexError, AssertionError):
            return good["smooth_40x24_420"][0], truncated, damaged, good["noise_40x24_gray_rst"][0]
    raise AssertionError("no overwrite of the host checker's draws damages the stream")


def test_damaged_streams_report_a_status_beside_good_images_inside_guards(arena):
    from hawq_amd.jpeg import parse_jpeg
    good, _, _ = M.cases()
    files = damaged_files()
    plan, out, status, _ = run_abi(arena, [parse_jpeg(f, progressive=True) for f in files])
    assert status[0] == 0 and status[3] == 0 and status[1] != 0 and status[2] != 0, status.tolist()
    assert np.array_equal(image_of(plan, out, 0), good["smooth_40x24_420"][1]) and np.array_equal(image_of(plan, out, 3), good["noise_40x24_gray_rst"][1])


def test_api_hands_damaged_progressive_streams_to_the_host_decoder():
    from hawq_amd.image import decode_image
    from hawq_amd.jpeg import decode_jpeg_batch
    a, truncated, damaged, b = damaged_files()
    try:
        want = [decode_image(f) for f in (a, truncated, damaged, b)]
    except Exception as e:   # Pillow refuses a damaged file: so must the batch
        with pytest.raises(type(e)):
            decode_jpeg_batch([a, truncated, damaged, b], progressive=True)
        return
    images, fallbacks = decode_jpeg_batch([a, truncated, damaged, b], progressive=True)
    assert [i for i, _ in fallbacks] == [1, 2] and all(r.startswith("device status ") for _, r in fallbacks)
    for im, ref in zip(images, want):
        assert torch.equal(im.cpu(), ref)
