"""The reduced-size device JPEG decode (``draft=``, desc.scale, jpeg_idct_scaled_kernel / jpeg_colour_scaled_kernel) on
the MI355X: every output byte equals what Pillow decodes in draft mode (tests/golden/jpeg_draft_cases.npz, make_jpeg_draft_cases.py),
through the C ABI with every buffer between poisoned guards (tests/guard.py) and through ``decode_jpeg_batch`` / ``folder_loader`` with
every option the draft composes with.  The damaged stream of the mixed batch is a truncation tools/jpeg_draft_host_check.cpp has
already decoded in bounds under the sanitizers (tests/test_jpeg_draft_host.py): here it must report a status, not fault."""
import functools
import io

import numpy as np
import pytest
import torch

from tests import guard, jpeg_model
from tests import jpeg_draft_model as M

pytestmark = pytest.mark.gpu

DRAFT = (8, 8)   # the mixed batch: 64x64 -> 1/8, 33x47 and 40x24 -> 1/4 and 1/2, 17x33 and 16x16 -> 1/2, 9x20 and 8x6 -> full size


@pytest.fixture(params=[0xA5, 0x5A], ids=["poisonA5", "poison5A"])
def arena(request):
    ar = guard.GuardArena("cuda", poison=request.param)
    yield ar
    ar.check()


def run_abi(ar, records, draft, check=True):
    """hawq_jpeg_decode_batch (or _prog, by the kind of the records) on `records` planned with `draft`, with blob, coefficient slab,
    planes, output and status in the arena -> (plan, out, status); ``check``: the guards are looked at now, not only when the arena goes"""
    from hawq_amd import _lib
    from hawq_amd.jpeg import JpegProgRecord, plan_jpeg_batch, plan_jpeg_prog_batch
    prog = isinstance(records[0], JpegProgRecord)
    plan = (plan_jpeg_prog_batch if prog else plan_jpeg_batch)(records, draft=draft)
    assert plan.ok(), _lib.load().hawq_last_error()
    blob = ar.put(plan.blob[:plan.nbytes], "blob")
    coef = ar.empty(plan.coef_blocks * 64, torch.int16, "coef")
    planes = ar.empty(plan.plane_bytes, torch.uint8, "planes")
    out = ar.empty(plan.out_bytes, torch.uint8, "out")
    status = ar.empty(len(records), torch.int32, "status")
    _lib.call("hawq_jpeg_decode_batch_prog" if prog else "hawq_jpeg_decode_batch", blob.data_ptr(), plan.blob.ctypes.data, plan.nbytes, coef.data_ptr(),
              plan.coef_blocks, planes.data_ptr(), plan.plane_bytes, out.data_ptr(), plan.out_bytes, status.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    if check:
        ar.check()
    return plan, out.cpu().numpy(), status.cpu().numpy()


def image_of(plan, out, i):
    h, w = plan.sizes[i]
    return out[plan.out_offsets[i]:plan.out_offsets[i] + h * w * 3].reshape(h, w, 3)


def test_every_fixture_at_every_scale_equals_pillow_inside_guards(arena):
    """one call per draft request the fixtures record and kind of file: every file that has that request, at the scale it gives it"""
    from hawq_amd.jpeg import parse_jpeg
    groups = {}
    for name, scale, data, draft, rgb in M.flat_cases():
        groups.setdefault((draft, name.endswith("_prog")), []).append((name, scale, data, rgb))
    done, wrong = 0, []
    for (draft, prog), members in groups.items():
        plan, out, status = run_abi(arena, [parse_jpeg(data, progressive=prog) for _, _, data, _ in members], draft, check=False)   # once, behind all calls
        assert not status.any(), (draft, status.tolist())
        for i, (name, scale, _, rgb) in enumerate(members):
            if plan.sizes[i] != rgb.shape[:2] or not np.array_equal(image_of(plan, out, i), rgb):
                wrong.append((name, scale))
        gaps = np.ones(plan.out_bytes, bool)   # the bytes between two images belong to nobody
        for (h, w), off in zip(plan.sizes, plan.out_offsets):
            gaps[off:off + h * w * 3] = False
        assert np.all(out[gaps] == arena.poison), draft
        done += len(members)
    arena.check()
    assert not wrong, wrong
    assert done == len(M.flat_cases()) and any(prog for _, prog in groups)


@functools.lru_cache(maxsize=None)
def mixed():
    """(sources, names): scales 1, 2, 4 and 8 under DRAFT across the three sampling modes, gray, a progressive file, two refused files
    and a damaged stream - a cut at a multiple of eight bytes, which ``parse_jpeg`` still accepts"""
    from hawq_amd.jpeg import draft_scale, parse_jpeg
    files, _ = M.cases()
    bad = jpeg_model.cases()[1]
    names = ["noise_64x64_420", "noise_33x47_444", "smooth_40x24_422", "noise_17x33_gray", "noise_9x20_420", "noise_33x47_420_prog", "block_64x64_444",
             "noise_16x16_422", "noise_8x6_444", "noise_40x24_420_rst", "noise_64x64_422", "noise_9x20_422", "smooth_33x47_420", "smooth_33x47_422",
             "smooth_17x33_444"]
    srcs = [files[n][0] for n in names]
    data = files["noise_33x47_422"][0]
    r = parse_jpeg(data)
    cut = (r.scan[1] - r.scan[0]) // 2 & ~7
    srcs[4:4] = [bad["cmyk"][0], data[:r.scan[0] + cut] + data[r.scan[1]:], bad["png"][0]]
    names[4:4] = ["cmyk", "truncated", "png"]
    assert parse_jpeg(srcs[5]).intervals.tolist() == [[0, cut]]
    scales = {}
    for n, s in zip(names, srcs):
        if n not in ("cmyk", "png"):
            r = parse_jpeg(s, progressive=True)
            scales.setdefault(draft_scale(r.width, r.height, DRAFT), set()).add("gray" if r.ncomp == 1 else (r.hs, r.vs))
    assert set(scales) == {1, 2, 4, 8} and all(scales[s] >= {(1, 1), (2, 1), (2, 2)} for s in (2, 4, 8)), scales
    return srcs, names


@functools.lru_cache(maxsize=None)
def mixed_expected():
    """Pillow's draft decode of every source of the mixed batch, computed once"""
    from hawq_amd.image import decode_image
    return [decode_image(s, draft=DRAFT) for s in mixed()[0]]


def check_mixed(images, fallbacks, plain_fallbacks):
    from hawq_amd.jpeg import output_layout
    srcs, names = mixed()
    want = mixed_expected()
    assert fallbacks == plain_fallbacks and [names[i] for i, _ in fallbacks] == ["cmyk", "truncated", "png"] and fallbacks[1][1].startswith("device status ")
    offsets, total = output_layout([tuple(w.shape[:2]) for w in want])
    base = images[0].untyped_storage().data_ptr()
    for i, (im, w) in enumerate(zip(images, want)):
        assert im.is_cuda and im.dtype == torch.uint8 and im.is_contiguous() and tuple(im.shape) == tuple(w.shape), names[i]
        assert im.untyped_storage().data_ptr() == base and im.data_ptr() - base == offsets[i], names[i]   # one allocation, reduced sizes
        assert torch.equal(im.cpu(), w), names[i]
    assert images[0].untyped_storage().nbytes() == total


def test_mixed_batch_lands_at_the_reduced_offsets_and_names_the_fallbacks_of_the_call_without_draft():
    from hawq_amd.image import decode_image
    from hawq_amd.jpeg import decode_jpeg_batch
    srcs, names = mixed()
    plain, plain_fallbacks = decode_jpeg_batch(srcs, progressive=True)
    images, fallbacks = decode_jpeg_batch(srcs, progressive=True, draft=DRAFT)
    check_mixed(images, fallbacks, plain_fallbacks)
    # the full-size images of the same batch are the call's without the option, byte for byte
    for i in (j for j, n in enumerate(names) if n in ("noise_9x20_420", "noise_9x20_422", "noise_8x6_444", "png")):
        assert torch.equal(images[i], plain[i]) and torch.equal(plain[i].cpu(), decode_image(srcs[i])), names[i]
    assert tuple(images[0].shape) == (8, 8, 3) and tuple(plain[0].shape) == (64, 64, 3)


@pytest.mark.parametrize("how", ["sync", "resume", "front", "front_sync"])
def test_mixed_batch_gives_the_same_bytes_with_every_option_the_draft_composes_with(how):
    from hawq_amd.jpeg import build_resume_index, decode_jpeg_batch, parse_jpeg, plan_jpeg_batch
    srcs, names = mixed()
    more = {}
    if "sync" in how:
        more.update(entropy="sync", sub_bytes=32, min_sync_bytes=1024)
        recs = [parse_jpeg(srcs[names.index(n)]) for n in ("noise_64x64_420", "noise_64x64_422")]
        assert plan_jpeg_batch(recs, sync=(32, 1024), draft=DRAFT).n_jobs == 2   # the 64x64 noise files are jobs
    if how == "resume":
        more["resume"] = build_resume_index(srcs, every=64, progressive=True)
        assert sum(len(p) > 0 for _, p in more["resume"].entries.values()) >= 8
    if "front" in how:
        more["front_end"] = "device"
    plain_fallbacks = decode_jpeg_batch(srcs, progressive=True, **more)[1]
    images, fallbacks = decode_jpeg_batch(srcs, progressive=True, draft=DRAFT, **more)
    check_mixed(images, fallbacks, plain_fallbacks)


def test_a_batch_of_full_size_images_with_draft_equals_the_call_without_it(arena):
    from hawq_amd.jpeg import decode_jpeg_batch, parse_jpeg
    good = jpeg_model.cases()[0]
    names = ["noise_31x33_444", "noise_40x23_422", "smooth_31x33_420", "noise_40x24_rst4", "smooth_31x33_gray", "noise_13x17_opt95"]
    srcs = [good[n][0] for n in names]
    plain, _ = decode_jpeg_batch(srcs)
    for draft in ((40, 40), (24, 17)):   # larger than every file; more than half of every file
        images, fallbacks = decode_jpeg_batch(srcs, draft=draft)
        assert fallbacks == []
        for n, im, p in zip(names, images, plain):
            assert torch.equal(im, p) and np.array_equal(im.cpu().numpy(), good[n][1]), n
    # the ABI with scale 1 in every descriptor: the bytes of the plan whose descriptors say 0
    recs = [parse_jpeg(s) for s in srcs]
    plan1, out1, status1 = run_abi(arena, recs, (40, 40))
    plan0, out0, status0 = run_abi(arena, recs, None)
    assert not status1.any() and not status0.any() and plan1.out_offsets == plan0.out_offsets
    for i, n in enumerate(names):
        assert np.array_equal(image_of(plan1, out1, i), good[n][1]) and np.array_equal(image_of(plan0, out0, i), good[n][1]), n


def test_library_refuses_a_scale_it_does_not_know_and_launches_nothing(arena):
    from hawq_amd import _lib
    from hawq_amd.jpeg import parse_jpeg, plan_jpeg_batch
    files, _ = M.cases()
    plan = plan_jpeg_batch([parse_jpeg(files["noise_33x47_444"][0])], draft=(8, 8))
    desc_off = int(plan.blob[:16].view(np.int32)[2])
    plan.blob[desc_off:desc_off + np.dtype(_lib.JpegDesc).itemsize].view(np.dtype(_lib.JpegDesc))["scale"] = 3
    blob = arena.put(plan.blob[:plan.nbytes], "blob")
    coef = arena.empty(plan.coef_blocks * 64, torch.int16, "coef")
    planes = arena.empty(plan.coef_blocks * 64, torch.uint8, "planes")
    out = arena.empty(33 * 47 * 3 + 15, torch.uint8, "out")
    status = arena.empty(1, torch.int32, "status")
    with pytest.raises(RuntimeError, match="hawq_jpeg_decode_batch: scale is none of 0, 1, 2, 4, 8"):
        _lib.call("hawq_jpeg_decode_batch", blob.data_ptr(), plan.blob.ctypes.data, plan.nbytes, coef.data_ptr(), plan.coef_blocks, planes.data_ptr(),
                  plan.coef_blocks * 64, out.data_ptr(), out.numel(), status.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((out == arena.poison).all()) and bool((status.view(torch.uint8) == arena.poison).all())


def test_folder_loader_with_device_decode_and_draft_equals_the_host_path(tmp_path):
    from PIL import Image

    from hawq_amd.image import folder_loader
    files, _ = M.cases()
    picks = ["noise_64x64_420", "smooth_40x24_422", "noise_33x47_420_prog", "block_64x64_gray", "noise_33x47_444", "noise_40x24_420_rst", "noise_64x64_444",
             "smooth_64x64_422", "noise_33x47_gray_rst"]
    for k, n in enumerate(picks):
        d = tmp_path / ("class%d" % (k % 3))
        d.mkdir(exist_ok=True)
        (d / (n + ".jpg")).write_bytes(files[n][0])
    buf = io.BytesIO()
    Image.fromarray(np.arange(50 * 70 * 3, dtype=np.uint8).reshape(50, 70, 3)).save(buf, "PNG")
    (tmp_path / "class1" / "picture.png").write_bytes(buf.getvalue())
    (tmp_path / "class2" / "cmyk.jpg").write_bytes(jpeg_model.cases()[1]["cmyk"][0])
    ref = list(folder_loader(str(tmp_path), batch_size=4, resize=24, crop=16, fused=True, draft=True))
    full = list(folder_loader(str(tmp_path), batch_size=4, resize=24, crop=16, fused=True))
    assert len(ref) == len(full) == 3 and not all(torch.equal(r.cpu(), f.cpu()) for (r, _), (f, _) in zip(ref, full))   # the draft changes the pixels
    for more in ({}, {"progressive": True}, {"progressive": True, "front_end": "device", "entropy": "sync"}):
        got = list(folder_loader(str(tmp_path), batch_size=4, resize=24, crop=16, device_decode=True, draft=True, **more))
        assert len(got) == 3
        for (gb, gt), (rb, rt) in zip(got, ref):
            assert gb.is_cuda and gb.dtype == torch.uint8 and torch.equal(gt, rt)
            assert torch.equal(gb.cpu(), rb.cpu()), more
