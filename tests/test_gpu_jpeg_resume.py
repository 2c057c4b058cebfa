"""Decoding JPEGs from recorded resume points (hawq_jpeg_decode_batch_resume / _prog_resume, decode_jpeg_batch(resume=),
folder_loader(resume=)) on the MI355X: one wave per segment of a restart interval gives the int16 coefficients of one
wave per interval, hence Pillow's bytes (tests/golden/jpeg_cases.npz, jpeg_sync_cases.npz, jpeg_prog_cases.npz).  The index is built on
the host.  The C ABI runs with every buffer between poisoned guards (tests/guard.py).  The damaged streams are those of
tests/test_gpu_jpeg.py and tests/test_gpu_jpeg_prog.py, whose segments tools/jpeg_resume_host_check.cpp has decoded in bounds under the
sanitizers (tests/test_jpeg_resume_host.py)."""
import functools

import numpy as np
import pytest
import torch

from tests import guard, jpeg_model, jpeg_sync_model
from tests import jpeg_prog_model as M
from tests import test_gpu_jpeg, test_gpu_jpeg_prog

pytestmark = pytest.mark.gpu
ENTRY = {False: ("hawq_jpeg_decode_batch", "hawq_jpeg_decode_batch_resume"), True: ("hawq_jpeg_decode_batch_prog", "hawq_jpeg_decode_batch_prog_resume")}


@pytest.fixture(params=[0xA5, 0x5A], ids=["poisonA5", "poison5A"])
def arena(request):
    ar = guard.GuardArena("cuda", poison=request.param)
    yield ar
    ar.check()


@functools.lru_cache(maxsize=None)
def fixtures(prog):
    """{name: (file bytes, Pillow's RGB)} of the kind, and the parsed records"""
    from hawq_amd.jpeg import parse_jpeg
    if prog:
        files = dict(M.cases()[0])
    else:
        files = dict(jpeg_model.cases()[0])
        files.update(jpeg_sync_model.cases()[0])
    return files, tuple(parse_jpeg(data, progressive=prog) for data, _ in files.values())


def run_abi(ar, records, every):
    """The records through the C ABI, every buffer in the arena: one wave per interval (every None), or one per segment of the points
    recorded at ``every`` -> (plan, out, status, coefficient slab)"""
    from hawq_amd import _lib
    from hawq_amd.jpeg import JpegProgRecord, plan_jpeg_batch, plan_jpeg_prog_batch, record_resume_points
    prog = isinstance(records[0], JpegProgRecord)
    resume = None if every is None else [record_resume_points(r, every) for r in records]
    plan = plan_jpeg_prog_batch(records, resume=resume) if prog else plan_jpeg_batch(records, resume=resume)
    assert plan.ok() and (resume is None or plan.resume_ok()), _lib.load().hawq_last_error()
    blob = ar.put(plan.blob[:plan.nbytes], "blob")
    coef = ar.empty(plan.coef_blocks * 64, torch.int16, "coef")
    planes = ar.empty(plan.plane_bytes, torch.uint8, "planes")
    out = ar.empty(plan.out_bytes, torch.uint8, "out")
    status = ar.empty(len(records), torch.int32, "status")
    more = () if resume is None else (plan.segs_off, plan.n_segs)
    _lib.call(ENTRY[prog][resume is not None], blob.data_ptr(), plan.blob.ctypes.data, plan.nbytes, coef.data_ptr(), plan.coef_blocks, planes.data_ptr(),
              plan.plane_bytes, out.data_ptr(), plan.out_bytes, status.data_ptr(), *more, None, torch.cuda.current_stream().cuda_stream)
    ar.check()
    return plan, out.cpu().numpy(), status.cpu().numpy(), coef.cpu().numpy()


@functools.lru_cache(maxsize=None)
def serial_slab(prog):
    """the coefficient slab of the serial call on all fixtures of the kind: computed once, compared against by both poisons"""
    _, _, status, coef = run_abi(guard.GuardArena("cuda"), fixtures(prog)[1], None)
    assert not status.any()
    coef.setflags(write=False)
    return coef


@pytest.mark.parametrize("prog", [False, True], ids=["baseline", "progressive"])
def test_all_fixtures_in_one_call_at_every_16_equal_the_serial_slab_and_pillow_inside_guards(arena, prog):
    files, records = fixtures(prog)
    want = serial_slab(prog)
    plan, out, status, coef = run_abi(arena, records, 16)
    assert plan.n_segs > plan.n_waves + 900   # long intervals are cut many times
    assert not status.any(), {n: int(s) for n, s in zip(files, status) if s}
    differ = np.flatnonzero(coef != want)
    assert differ.size == 0, (differ.size, differ[:8] // 64)   # word for word, padding blocks included
    wrong = [n for i, n in enumerate(files) if not np.array_equal(test_gpu_jpeg.image_of(plan, out, i), files[n][1])]
    assert not wrong, wrong
    gaps = np.ones(plan.out_bytes, bool)   # the bytes between two images belong to nobody
    for (h, w), off in zip(plan.sizes, plan.out_offsets):
        gaps[off:off + h * w * 3] = False
    assert np.all(out[gaps] == arena.poison)


def touched(data):
    """the file with one byte of its JFIF header changed: the same pixels, another file - its entry is stale"""
    assert data[6:10] == b"JFIF"
    return data[:15] + bytes([data[15] ^ 1]) + data[16:]


@pytest.mark.parametrize("entropy", ["serial", "sync"])
def test_mixed_batch_with_half_the_entries_and_a_stale_one_equals_decode_image(tmp_path, entropy):
    from hawq_amd.image import decode_image, preprocess_batch_fused
    from hawq_amd.jpeg import build_resume_index, decode_jpeg_batch
    srcs, refused = test_gpu_jpeg_prog.mixed_sources(tmp_path)
    srcs += [jpeg_sync_model.cases()[0][n][0] for n in ("noise_144x104_q95_420", "noise_96x64_rstrow", "noise_64x48_422", "flat_320x240")]
    stale = len(srcs)
    srcs.append(touched(jpeg_sync_model.cases()[0]["noise_64x48_q100"][0]))
    idx = build_resume_index(srcs[0::2] + [jpeg_sync_model.cases()[0]["noise_64x48_q100"][0]], every=16, progressive=True, workers=2)
    assert len(idx) == len([i for i in range(0, len(srcs), 2) if i not in dict(refused)]) + 1 and idx.points(srcs[stale], None) is None
    more = {"min_sync_bytes": 64} if entropy == "sync" else {}
    images, fallbacks = decode_jpeg_batch(srcs, entropy=entropy, progressive=True, resume=idx, **more)
    assert fallbacks == refused
    want = [decode_image(s) for s in srcs]
    base = images[0].untyped_storage().data_ptr()
    for i, (im, ref) in enumerate(zip(images, want)):
        assert im.is_cuda and im.dtype == torch.uint8 and im.is_contiguous() and im.data_ptr() % 16 == 0
        assert im.untyped_storage().data_ptr() == base   # one allocation
        assert torch.equal(im.cpu(), ref), i
    assert torch.equal(preprocess_batch_fused(images, 40, 32).cpu(), preprocess_batch_fused(want, 40, 32).cpu())   # read in place


@pytest.mark.parametrize("prog", [False, True], ids=["baseline", "progressive"])
def test_damaged_streams_with_points_recorded_from_them_report_the_serial_status_inside_guards(arena, prog):
    from hawq_amd.jpeg import parse_jpeg
    files = (test_gpu_jpeg_prog if prog else test_gpu_jpeg).damaged_files()
    records = [parse_jpeg(f, progressive=prog) for f in files]
    _, _, want, _ = run_abi(guard.GuardArena("cuda"), records, None)
    plan, out, status, _ = run_abi(arena, records, 16)
    assert plan.n_segs > plan.n_waves
    assert status[0] == 0 and status[3] == 0 and status[1] != 0 and status[2] != 0, status.tolist()
    assert status[1] == want[1], (status.tolist(), want.tolist())            # one interval: its status
    assert (status != 0).tolist() == (want != 0).tolist()                    # several intervals may fail: one of theirs
    good, names = (M.cases()[0], ("smooth_40x24_420", "noise_40x24_gray_rst")) if prog else (jpeg_model.cases()[0], ("smooth_31x33_420", "noise_40x24_rst4"))
    assert np.array_equal(test_gpu_jpeg.image_of(plan, out, 0), good[names[0]][1]) and np.array_equal(test_gpu_jpeg.image_of(plan, out, 3), good[names[1]][1])


def test_api_hands_damaged_streams_to_the_host_decoder_with_an_index_as_without():
    from hawq_amd.jpeg import build_resume_index, decode_jpeg_batch
    files = list(test_gpu_jpeg.damaged_files()) + list(test_gpu_jpeg_prog.damaged_files())
    idx = build_resume_index(files, every=16, progressive=True)
    assert len(idx) == 8
    try:
        want, want_fallbacks = decode_jpeg_batch(files, progressive=True)
    except Exception as e:   # Pillow refuses a damaged file: so must the batch with the index
        with pytest.raises(type(e)):
            decode_jpeg_batch(files, progressive=True, resume=idx)
        return
    images, fallbacks = decode_jpeg_batch(files, progressive=True, resume=idx)
    assert [i for i, _ in fallbacks] == [i for i, _ in want_fallbacks] == [1, 2, 5, 6]
    for im, ref in zip(images, want):
        assert torch.equal(im.cpu(), ref.cpu())


@pytest.mark.parametrize("workers", [0, 2])
def test_folder_loader_with_an_index_gives_the_batches_it_gives_without(tmp_path, workers):
    from hawq_amd.image import folder_loader
    from hawq_amd.jpeg import build_resume_index
    good, bad, _ = M.cases()
    base, base_bad, _ = jpeg_model.cases()
    long = jpeg_sync_model.cases()[0]
    picks = [(good, n) for n in ("noise_1x1_444", "noise_13x17_422", "noise_40x24_420_rst", "deep_33x31_420", "tables_13x17_422", "noise_40x24_444_q100")]
    picks += [(base, n) for n in ("noise_13x17_422", "noise_40x24_rst7_gray", "flat_24x24")] + [(long, n) for n in ("noise_64x48_422", "noise_96x64_rstrow")]
    root = tmp_path / "images"
    for k, (src, n) in enumerate(picks):
        d = root / ("class%d" % (k % 3))
        d.mkdir(parents=True, exist_ok=True)
        (d / ("%02d_%s.jpg" % (k, n))).write_bytes(src[n][0])
    (root / "class1" / "incomplete.jpg").write_bytes(bad["cut_last_scan"][0])
    (root / "class2" / "picture.png").write_bytes(base_bad["png"][0])
    path = str(tmp_path / "points.npz")
    build_resume_index([src[n][0] for src, n in picks[1:]], every=16, progressive=True).save(path)   # all but one of the files
    ref = list(folder_loader(str(root), batch_size=5, resize=40, crop=32, device_decode=True, progressive=True, workers=workers))
    got = list(folder_loader(str(root), batch_size=5, resize=40, crop=32, device_decode=True, progressive=True, workers=workers, resume=path))
    assert len(got) == len(ref) == 3
    for (gb, gt), (rb, rt) in zip(got, ref):
        assert gb.is_cuda and gb.dtype == torch.uint8 and torch.equal(gt, rt)
        assert torch.equal(gb.cpu(), rb.cpu())
