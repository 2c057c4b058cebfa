"""Host side of the reduced-size device JPEG decode (``draft=``) without a GPU: the scale Pillow's draft mode picks, the
numpy model of the reduced inverse DCTs against real Pillow output (tests/golden/jpeg_draft_cases.npz, make_jpeg_draft_cases.py), what
the planners and the device front end's layout write with and without the option, what the blob checkers refuse, the bookkeeping of
``decode_jpeg_batch`` and ``folder_loader`` with a stub in place of the device call, and the kernels' own block / pixel arithmetic
compiled into a stand-alone program under AddressSanitizer + UBSan, on valid and on corrupted streams."""
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import jpeg_draft_model as M
from tests import jpeg_model
from tests.jpeg_stub import stub_launch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLING = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}


def test_the_fixture_set_holds_what_makes_it_meaningful():
    files, cond = M.cases()
    assert cond["colour_files"] == 108 and len(files) == cond["files"] >= 108 + 7 and cond["decodes"] == len(M.flat_cases()) >= 268
    for s in ("2", "4", "8"):
        assert cond["zero"][s] > 0 and cond["full"][s] > 0, s   # both ends of the range limit
    for s in ("2", "4"):
        assert cond["narrow_422"][s] > 0 and cond["wide_422"][s] > 0, s   # replication and the fancy filter
    assert cond["off_grid"] > 0
    kinds = {n.rsplit("_", 1)[1] for n in files}
    assert kinds >= {"444", "422", "420", "gray", "rst", "prog"}
    for name, scale, data, draft, rgb in M.flat_cases():
        h, w = (int(v) for v in name.split("_")[1].split("x"))
        assert M.pillow_scale(w, h, draft) == scale and rgb.shape == (-(-h // scale), -(-w // scale), 3), (name, scale)


def test_numpy_model_equals_pillow_on_every_fixture_at_every_scale():
    wrong = [(name, scale) for name, scale, data, _, rgb in M.flat_cases() if not np.array_equal(M.decode(data, scale), rgb)]
    assert not wrong, wrong


def test_block_sizes_follow_the_sampling():
    for s in (2, 4, 8):
        m = 8 // s
        assert M.block_size(1, 1, 1, 1, s) == m and M.block_size(2, 1, 2, 1, s) == m and M.block_size(2, 2, 2, 2, s) == m
        assert M.block_size(1, 1, 2, 1, s) == m and M.block_size(1, 1, 2, 2, s) == 2 * m


def test_draft_scale_equals_pillows_choice_over_a_grid():
    from PIL import Image

    from hawq_amd.jpeg import draft_scale, draft_scales
    sides = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 100)
    requests = (1, 2, 3, 4, 5, 8, 9, 16, 17, 40, 200)   # some larger than every file
    checked = 0
    for w in sides:
        for h in sides:
            buf = io.BytesIO()
            Image.new("RGB", (w, h)).save(buf, "JPEG")
            for rw in requests:
                for rh in requests:
                    with Image.open(io.BytesIO(buf.getvalue())) as im:
                        im.draft("RGB", (rw, rh))   # no decoding: the size alone
                        s = draft_scale(w, h, (rw, rh))
                        assert s in (1, 2, 4, 8) and im.size == (-(-w // s), -(-h // s)), (w, h, rw, rh, s, im.size)
                    checked += 1
    assert checked == len(sides) ** 2 * len(requests) ** 2
    ws, hs = np.meshgrid(np.array(sides), np.array(sides))
    got = draft_scales(ws.reshape(-1), hs.reshape(-1), (3, 5))
    assert got.dtype == np.int32 and got.tolist() == [draft_scale(w, h, (3, 5)) for w, h in zip(ws.reshape(-1).tolist(), hs.reshape(-1).tolist())]
    assert draft_scale(100, 100, None) == 1 and set(draft_scales(ws.reshape(-1), hs.reshape(-1), None).tolist()) == {1}


def test_bad_draft_arguments_raise_value_error():
    from hawq_amd.image import decode_image, folder_loader
    from hawq_amd.jpeg import decode_jpeg_batch, draft_scale, parse_jpeg, plan_jpeg_batch
    data = M.cases()[0]["noise_16x16_444"][0]
    for bad in ((0, 4), (4, -1), (4,), (1, 2, 3), 7, "ab", (None, 2)):
        with pytest.raises(ValueError):
            draft_scale(16, 16, bad)
        with pytest.raises(ValueError):
            decode_jpeg_batch([data], device="cpu", draft=bad)
        with pytest.raises(ValueError):
            decode_image(data, draft=bad)
        with pytest.raises(ValueError):
            plan_jpeg_batch([parse_jpeg(data)], draft=bad)
    with pytest.raises(ValueError):
        next(folder_loader(".", draft=(2, 2)))


# ------------------------------------------------------------------------------------------------------------------ plans
def _records(names, progressive=False):
    from hawq_amd.jpeg import parse_jpeg
    files, _ = M.cases()
    return [parse_jpeg(files[n][0], progressive=progressive) for n in names]


BASE = ["noise_33x47_444", "smooth_40x24_422", "block_64x64_420", "noise_17x33_gray", "noise_40x24_420_rst", "noise_8x5_422", "noise_65x9_420"]
PROG = ["noise_33x47_420_prog", "smooth_40x24_422_prog"]


def _expected_geometry(r, s):
    """(plane bytes, (height, width)) of record ``r`` at scale ``s``, from the model's block sizes"""
    planes = sum(r.mcus_x * h * r.mcus_y * v * M.block_size(h, v, r.hs, r.vs, s) ** 2 for _, h, v in (c[:3] for c in r.components)) if s > 1 else r.blocks * 64
    return planes, (-(-r.height // s), -(-r.width // s))


def _descs(plan, n, off):
    from hawq_amd import _lib
    return plan.blob[off:off + n * C.sizeof(_lib.JpegDesc)].view(np.dtype(_lib.JpegDesc))


def test_plans_without_draft_are_byte_identical_and_say_scale_zero():
    from hawq_amd.jpeg import plan_jpeg_batch, plan_jpeg_prog_batch
    for planner, recs in ((plan_jpeg_batch, _records(BASE)), (plan_jpeg_prog_batch, _records(PROG, True))):
        plain, none = planner(recs), planner(recs, draft=None)
        assert plain.nbytes == none.nbytes and np.array_equal(plain.blob[:plain.nbytes], none.blob[:none.nbytes])
        desc = _descs(plain, len(recs), int(plain.blob[:16].view(np.int32)[2]))
        assert not desc["scale"].any()
        assert plain.plane_bytes == plain.coef_blocks * 64 and plain.sizes == [(r.height, r.width) for r in recs]
        # a draft that leaves every image at full size: the same blob but for the scale, which says 1
        full = planner(recs, draft=(4000, 4000))
        assert full.ok() and (full.plane_bytes, full.out_bytes, full.sizes, full.out_offsets) == (plain.plane_bytes, plain.out_bytes, plain.sizes, plain.out_offsets)
        d1 = _descs(full, len(recs), int(full.blob[:16].view(np.int32)[2]))
        assert (d1["scale"] == 1).all()
        d1["scale"] = 0
        assert np.array_equal(full.blob[:full.nbytes], plain.blob[:plain.nbytes])


@pytest.mark.parametrize("draft", [(12, 12), (4, 4), (1, 1), (3, 20)])
def test_plans_with_draft_carry_the_scale_and_the_reduced_sizes(draft):
    from hawq_amd.jpeg import draft_scale, plan_jpeg_batch, plan_jpeg_prog_batch
    seen = set()
    for planner, recs in ((plan_jpeg_batch, _records(BASE)), (plan_jpeg_prog_batch, _records(PROG, True))):
        plan = planner(recs, draft=draft)
        assert plan.ok()
        desc = _descs(plan, len(recs), int(plan.blob[:16].view(np.int32)[2]))
        plane_at = out_at = 0
        for i, r in enumerate(recs):
            s = draft_scale(r.width, r.height, draft)
            assert s == M.pillow_scale(r.width, r.height, draft) == desc["scale"][i]
            planes, size = _expected_geometry(r, s)
            assert plan.sizes[i] == size and desc["plane_off"][i] == plane_at and desc["out_off"][i] == out_at == plan.out_offsets[i], (i, s)
            plane_at, out_at = plane_at + planes, (out_at + size[0] * size[1] * 3 + 15) & ~15
            seen.add(s)
        assert plan.plane_bytes == plane_at and plan.out_bytes == out_at and plan.coef_blocks == sum(r.blocks for r in recs)
    assert len(seen) > 1 or draft == (3, 20)


def test_front_layout_with_draft_equals_the_planners_head():
    from hawq_amd import jpeg
    files, _ = M.cases()
    datas = [files[n][0] for n in BASE]
    info = jpeg.front_scan_host(datas)
    assert (info["defer"] == jpeg.FRONT_OK).all()
    for draft in (None, (12, 12), (4, 4), (1, 1)):
        plan = jpeg.plan_jpeg_batch(_records(BASE), draft=draft)
        lay = jpeg.front_layout(info, np.arange(len(datas)), plan.out_offsets, plan.out_bytes, draft)
        assert (lay.nbytes, lay.coef_blocks, lay.plane_bytes, lay.out_bytes) == (plan.nbytes, plan.coef_blocks, plan.plane_bytes, plan.out_bytes)
        assert np.array_equal(lay.head, plan.blob[:lay.head.size]), draft
        assert lay.desc["scale"].tolist() == [0 if draft is None else jpeg.draft_scale(r.width, r.height, draft) for r in _records(BASE)]


def _ok(plan, blob=None, planes=None, out=None):
    from hawq_amd import _lib
    blob = plan.blob if blob is None else blob
    ok = getattr(_lib.load(), plan.checker)(blob.ctypes.data, plan.nbytes, plan.coef_blocks, plan.plane_bytes if planes is None else planes,
                                            plan.out_bytes if out is None else out)
    return bool(ok), _lib.load().hawq_last_error().decode()


def test_checkers_refuse_a_scale_of_three_and_buffers_one_byte_short_of_the_scaled_geometry():
    from hawq_amd import _lib
    from hawq_amd.jpeg import plan_jpeg_batch, plan_jpeg_prog_batch
    dt = np.dtype(_lib.JpegDesc)
    for planner, recs in ((plan_jpeg_batch, _records(BASE)), (plan_jpeg_prog_batch, _records(PROG, True))):
        plan = planner(recs, draft=(4, 4))
        assert plan.plane_bytes < plan.coef_blocks * 64 and _ok(plan)[0]
        ok, why = _ok(plan, planes=plan.plane_bytes - 1)
        assert not ok and "sample planes outside their buffer" in why
        last = plan.out_offsets[-1] + plan.sizes[-1][0] * plan.sizes[-1][1] * 3   # the end of the last image: the buffer's end is aligned up
        assert _ok(plan, out=last)[0]
        ok, why = _ok(plan, out=last - 1)
        assert not ok and "output image outside its buffer" in why
        desc_off = int(plan.blob[:16].view(np.int32)[2])
        for i in range(len(recs)):
            for bad in (3, -1, 5, 6, 7, 16, 1 << 20):
                blob = plan.blob.copy()
                blob[desc_off:desc_off + len(recs) * dt.itemsize].view(dt)["scale"][i] = bad
                ok, why = _ok(plan, blob)
                assert not ok and why.endswith("scale is none of 0, 1, 2, 4, 8"), (i, bad, why)
        # the planes of the full-size geometry do not pass for a smaller scale's, nor the other way round
        full = planner(recs)
        assert not _ok(full, planes=plan.plane_bytes)[0] and not _ok(full, out=plan.out_bytes)[0]


# ------------------------------------------------------------------------------------------------------------------ bookkeeping
def _stub_launch(monkeypatch, statuses=None):
    """tests/jpeg_stub.py with the draft model in place of the launch.  The stub's launch takes today's arguments: the wrapper hands it
    those and keeps ``draft`` for the model; -> the list of (records, draft) per call"""
    from hawq_amd import jpeg
    seen, current = [], {}

    def model(r):
        return M.decode(r.data, jpeg.draft_scale(r.width, r.height, current["draft"]))

    stub_launch(monkeypatch, {"base": model, "prog": model}, lambda kind, records, out, sync: None, {"base": statuses or {}})
    stub = jpeg._launch

    def launch(*args, draft=None, **kw):
        current["draft"] = draft
        seen.append((len(args[0]), draft))
        return stub(*args, **kw)

    monkeypatch.setattr(jpeg, "_launch", launch)
    return seen


def _png(rgb):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "PNG")
    return buf.getvalue()


def test_decode_jpeg_batch_with_draft_through_the_stub(monkeypatch):
    from hawq_amd.image import decode_image
    from hawq_amd.jpeg import decode_jpeg_batch
    files, _ = M.cases()
    bad = jpeg_model.cases()[1]
    calls = _stub_launch(monkeypatch, {1: 1})
    png = _png(np.arange(40 * 30 * 3, dtype=np.uint8).reshape(40, 30, 3))
    names = ["noise_33x47_444", "noise_33x47_420_prog", "smooth_40x24_422", None, "block_64x64_420", "noise_17x33_gray", None, "noise_8x5_422"]
    srcs = [files[n][0] if n else None for n in names]
    srcs[3], srcs[6] = png, bad["cmyk"][0]
    for draft in ((12, 12), (4, 4), (1, 1)):
        calls.clear()
        images, fallbacks = decode_jpeg_batch(srcs, device="cpu", draft=draft)
        # the progressive file is refused without progressive=True, the second baseline image reports a status: both decoded on the host with the draft
        assert calls == [(5, draft)]
        assert fallbacks == [(1, "progressive (SOF2)"), (2, "device status 1: ran out of bytes"), (3, "not a JPEG"), (6, "four components")]
        assert fallbacks == decode_jpeg_batch(srcs, device="cpu")[1]
        base = images[0].untyped_storage().data_ptr()
        for i, (im, src) in enumerate(zip(images, srcs)):
            assert torch.equal(im, decode_image(src, draft=draft)), (draft, i)
            assert im.untyped_storage().data_ptr() == base and im.data_ptr() % 16 == 0 and im.is_contiguous()
        assert tuple(images[3].shape) == (40, 30, 3) and torch.equal(images[3], decode_image(png))   # a PNG is unaffected
        for i in (0, 4):
            h, w = (int(v) for v in names[i].split("_")[1].split("x"))
            s = M.pillow_scale(w, h, draft)
            assert s > 1 and tuple(images[i].shape) == (-(-h // s), -(-w // s), 3)
    # progressive on the device: a call of its own, with the draft
    calls.clear()
    images, fallbacks = decode_jpeg_batch(srcs, device="cpu", draft=(12, 12), progressive=True)
    assert calls == [(1, (12, 12)), (5, (12, 12))] and [i for i, _ in fallbacks] == [2, 3, 6]
    assert all(torch.equal(im, decode_image(src, draft=(12, 12))) for im, src in zip(images, srcs))
    # without the option the launch gets no argument of the new kind
    calls.clear()
    decode_jpeg_batch(srcs[:1], device="cpu")
    assert calls == [(1, None)]


def test_decode_image_with_draft_is_pillows_draft_mode():
    from hawq_amd.image import decode_image
    for name, scale, data, draft, rgb in M.flat_cases()[::7]:
        assert np.array_equal(decode_image(data, draft=draft).numpy(), rgb), (name, scale)
        assert np.array_equal(decode_image(data, draft=None).numpy(), decode_image(data).numpy())


def _tree(tmp_path):
    files, _ = M.cases()
    picks = {"a/0.jpg": "noise_64x64_420", "a/1.jpg": "smooth_40x24_422", "a/2.jpg": "noise_33x47_420_prog", "b/0.jpg": "block_64x64_gray",
             "b/2.jpeg": "noise_33x47_444", "c/0.jpg": "noise_40x24_420_rst"}
    out = {rel: files[n][0] for rel, n in picks.items()}
    out["b/1.png"] = _png(np.arange(50 * 70 * 3, dtype=np.uint8).reshape(50, 70, 3))
    for rel, data in out.items():
        (tmp_path / rel).parent.mkdir(exist_ok=True)
        (tmp_path / rel).write_bytes(data)
    return out


def _pillow_draft_resize_crop(data, resize, crop):
    """Pillow alone: draft (resize, resize) + Resize(resize) + CenterCrop(crop) as torchvision applies them"""
    from PIL import Image

    from hawq_amd.image import resize_crop_geometry
    with Image.open(io.BytesIO(data)) as im:
        im.draft("RGB", (resize, resize))
        im = im.convert("RGB")
        oh, ow, top, left = resize_crop_geometry(im.size[1], im.size[0], resize, crop)
        im = im.resize((ow, oh), Image.BILINEAR).crop((left, top, left + crop, top + crop))
        return np.array(im)


def test_folder_loader_with_draft_on_the_host_path_equals_pillow(monkeypatch, tmp_path):
    from hawq_amd import image
    files = _tree(tmp_path)
    handed = []

    def fused(imgs, resize, crop, device=None):   # stands in for the launch: Pillow's resize + crop of what it is handed
        from PIL import Image
        out = []
        for im in imgs:
            handed.append(tuple(im.shape[:2]))
            oh, ow, top, left = image.resize_crop_geometry(im.shape[0], im.shape[1], resize, crop)
            out.append(torch.from_numpy(np.array(Image.fromarray(im.numpy()).resize((ow, oh), Image.BILINEAR).crop((left, top, left + crop, top + crop)))))
        return torch.stack(out)

    monkeypatch.setattr(image, "preprocess_batch_fused", fused)
    for workers in (0, 2):
        handed.clear()
        got = list(image.folder_loader(str(tmp_path), batch_size=3, resize=12, crop=8, device="cpu", fused=True, workers=workers, draft=True))
        assert [t.tolist() for _, t in got] == [[0, 0, 0], [1, 1, 1], [2]]
        flat = [im for batch, _ in got for im in batch]
        for im, (rel, data) in zip(flat, sorted(files.items())):
            assert np.array_equal(im.numpy(), _pillow_draft_resize_crop(data, 12, 8)), rel
        # reduced where the file is at least twice the request, never below it; the PNG at full size
        assert handed == [(16, 16), (20, 12), (17, 24), (16, 16), (50, 70), (17, 24), (20, 12)]
    plain = list(image.folder_loader(str(tmp_path), batch_size=3, resize=12, crop=8, device="cpu", fused=True))
    assert handed[-7:] == [(64, 64), (40, 24), (33, 47), (64, 64), (50, 70), (33, 47), (40, 24)] and len(plain) == 3


def test_folder_loader_with_device_decode_and_draft_through_the_stub(monkeypatch, tmp_path):
    from hawq_amd import image
    files = _tree(tmp_path)
    calls = _stub_launch(monkeypatch)
    seen = []

    def fused(imgs, resize, crop, device=None):
        seen.extend(im.clone() for im in imgs)
        return torch.zeros(len(imgs), crop, crop, 3, dtype=torch.uint8)

    monkeypatch.setattr(image, "preprocess_batch_fused", fused)
    got = list(image.folder_loader(str(tmp_path), batch_size=3, resize=12, crop=8, device="cpu", device_decode=True, progressive=True, draft=True))
    assert [t.tolist() for _, t in got] == [[0, 0, 0], [1, 1, 1], [2]] and all(d == (12, 12) for _, d in calls)
    for im, (rel, data) in zip(seen, sorted(files.items())):
        assert torch.equal(im, image.decode_image(data, draft=(12, 12))), rel


# ------------------------------------------------------------------------------------------------------------------ the kernels' arithmetic on the host
def test_kernel_arithmetic_on_the_host_under_sanitizers_at_every_scale(tmp_path):
    """tools/jpeg_draft_host_check.cpp: the header text the scaled kernels compile, built with ASan + UBSan into a program of its own and
    run as a child process on the planners' blobs of EVERY fixture at EVERY scale (one plan per file and scale, made with the draft the
    fixture records): golden bytes for the intact streams, planes and images in heap blocks of the scaled geometry's exact size, a status
    and no sanitizer report for every truncation at each eighth byte and for 200 single-byte overwrites per stream."""
    from hawq_amd.jpeg import JpegProgRecord, parse_jpeg, plan_jpeg_batch, plan_jpeg_prog_batch
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "jpeg_draft_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tools", "jpeg_draft_host_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    parts, by_scale, streams = [], {2: 0, 4: 0, 8: 0}, 0
    for name, scale, data, draft, rgb in M.flat_cases():
        rec = parse_jpeg(data, progressive=True)
        prog = isinstance(rec, JpegProgRecord)
        plan = (plan_jpeg_prog_batch if prog else plan_jpeg_batch)([rec], draft=draft)
        assert plan.ok() and plan.sizes == [rgb.shape[:2]], (name, scale)
        expected = np.zeros(plan.out_bytes, np.uint8)
        expected[:rgb.size] = rgb.reshape(-1)
        parts += [np.array([int(prog), plan.nbytes, plan.out_bytes, 0], np.int64).view(np.uint8), plan.blob[:plan.nbytes].copy(), expected]
        by_scale[scale] += 1
        streams += len(rec.scans) if prog else 1
    np.concatenate(parts).tofile(str(tmp_path / "pack.bin"))
    r = subprocess.run([exe, str(tmp_path / "pack.bin"), str(jpeg_model.HOST_CHECK_SEED)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    words = r.stdout.split()
    counts = dict(zip(words[0::2], map(int, words[1::2])))
    n = len(M.flat_cases())
    assert counts["images"] == counts["exact"] == counts["scaled"] == n
    assert (counts["half"], counts["quarter"], counts["eighth"]) == (by_scale[2], by_scale[4], by_scale[8]) and min(by_scale.values()) > 60
    assert counts["streams"] == streams > n
    assert counts["truncations"] == counts["truncations_flagged"] > n
    assert counts["overwrites"] == 200 * streams
