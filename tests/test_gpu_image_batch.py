"""The one-launch batched Resize + CenterCrop (hawq_image_batch, hawq_amd.image.preprocess_batch_fused) on the MI355X: every output
byte equals oracle/pil_resample.py (pinned to real Pillow by tests/golden/pillow_resize.npz) AND the per-image path
``resize_center_crop``.  Small (resize, crop) keep it quick; the kernel's arithmetic does not depend on the size."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

# h, w, fill: landscape, portrait, both axes equal to resize, one axis equal to resize (x2), up-scaling, many taps + several tiles, odd crop
# offsets, clip (x2).  (With Resize(int)'s geometry an image whose short edge equals `resize` keeps its long edge too, so 40 x 61 and
# 61 x 40 skip BOTH passes like 40 x 40, with a crop window off the centre of the long edge.)
BATCH = [(50, 67, None), (67, 50, None), (40, 40, None), (40, 61, None), (61, 40, None), (30, 37, None), (400, 300, None), (41, 41, None),
         (50, 67, 255), (67, 50, 0)]
GEOMS = [(40, 32), (40, 31)]   # crop * 3 a multiple of 4, and not


@functools.lru_cache(maxsize=None)
def _images():
    rng = np.random.default_rng(11)
    out = []
    for h, w, fill in BATCH:
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        img[::7, ::5] = 255
        img[3::11, 2::13] = 0
        if fill is not None:
            img[:] = fill
        img.setflags(write=False)
        out.append(img)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _oracle(resize, crop):
    from oracle import pil_resample
    ref = np.stack([pil_resample.resize_center_crop(im, resize, crop) for im in _images()])
    ref.setflags(write=False)
    return ref


def _host(imgs):
    return [torch.from_numpy(np.array(im)) for im in imgs]


def _differing(got, ref):
    return [i for i in range(len(ref)) if not np.array_equal(got[i], ref[i])]


@pytest.mark.parametrize("resize,crop", GEOMS)
def test_ragged_batch_in_one_call_equals_the_oracle_and_the_per_image_path(resize, crop):
    from hawq_amd.image import preprocess_batch, preprocess_batch_fused, resize_center_crop
    ref = _oracle(resize, crop)
    dev = [t.cuda() for t in _host(_images())]
    got = preprocess_batch_fused(dev, resize, crop)
    assert got.shape == (len(BATCH), crop, crop, 3) and got.dtype == torch.uint8 and got.is_cuda
    got = got.cpu().numpy()
    assert np.array_equal(got, ref), _differing(got, ref)
    per_image = torch.stack([resize_center_crop(t, resize, crop) for t in dev]).cpu().numpy()
    assert np.array_equal(got, per_image), _differing(got, per_image)
    assert np.array_equal(preprocess_batch(dev, resize, crop, fused=True).cpu().numpy(), ref)


@pytest.mark.parametrize("resize,crop", GEOMS)
def test_host_device_and_mixed_images_give_the_same_bytes(resize, crop):
    from hawq_amd.image import preprocess_batch_fused
    ref = _oracle(resize, crop)
    host = _host(_images())
    got = preprocess_batch_fused(host, resize, crop).cpu().numpy()
    assert np.array_equal(got, ref), _differing(got, ref)
    mixed = [t.cuda() if i % 2 else t for i, t in enumerate(host)]
    got = preprocess_batch_fused(mixed, resize, crop).cpu().numpy()
    assert np.array_equal(got, ref), _differing(got, ref)
    strided = [t.cuda() for t in host]
    strided[0] = torch.cat([strided[0], strided[0]], 1)[:, :BATCH[0][1]]   # a non-contiguous view of the same pixels
    assert not strided[0].is_contiguous()
    assert np.array_equal(preprocess_batch_fused(strided, resize, crop).cpu().numpy(), ref)


def test_single_image_and_crop_equal_to_resize():
    from hawq_amd.image import preprocess_batch_fused
    from oracle import pil_resample
    imgs = _images()
    for k in (0, 6, 2):
        got = preprocess_batch_fused(_host(imgs[k:k + 1]), 40, 32).cpu().numpy()
        assert got.shape == (1, 32, 32, 3) and np.array_equal(got[0], _oracle(40, 32)[k]), k
    ref = np.stack([pil_resample.resize_center_crop(im, 40, 40) for im in imgs])
    got = preprocess_batch_fused(_host(imgs), 40, 40).cpu().numpy()
    assert np.array_equal(got, ref), _differing(got, ref)


@pytest.mark.parametrize("resize,crop", GEOMS)
def test_small_lds_budget_one_row_tiles_and_fallback_give_the_same_bytes(resize, crop):
    """3 band rows of LDS: one-row tiles for the resampled images, a short last tile for the copied one, the 400 x 300 image (21 input
    rows per output row) through the per-image path into the same tensor"""
    from hawq_amd.image import band_pitch, plan_batch, preprocess_batch_fused
    budget = 3 * band_pitch(crop)
    plan = plan_batch([im.shape[:2] for im in _images()], resize, crop, lds_budget=budget)
    assert plan.fallback == [6] and plan.lds_bytes <= budget
    assert {t.rows for t in plan.tiles if t.image == 0} == {1} and [t.rows for t in plan.tiles if t.image == 2][-1] == crop % 3
    ref = _oracle(resize, crop)
    for imgs in (_host(_images()), [t.cuda() for t in _host(_images())]):
        got = preprocess_batch_fused(imgs, resize, crop, lds_budget=budget).cpu().numpy()
        assert np.array_equal(got, ref), _differing(got, ref)
    only_fallback = preprocess_batch_fused(_host(_images()[6:7]), resize, crop, lds_budget=budget).cpu().numpy()
    assert np.array_equal(only_fallback[0], ref[6])


@pytest.mark.parametrize("resize,crop", GEOMS)
def test_out_view_inside_a_sentinel_buffer(resize, crop):
    """out= a view at an odd byte offset of a larger buffer: inside equals the oracle, every byte outside keeps the sentinel"""
    from hawq_amd.image import preprocess_batch_fused
    n, size = len(BATCH), len(BATCH) * crop * crop * 3
    for lead in (64, 61):
        buf = torch.full((lead + size + 67,), 0xA5, dtype=torch.uint8, device="cuda")
        view = buf[lead:lead + size].view(n, crop, crop, 3)
        ret = preprocess_batch_fused(_host(_images()), resize, crop, out=view)
        assert ret.data_ptr() == view.data_ptr()
        got = buf.cpu().numpy()
        assert np.array_equal(got[lead:lead + size].reshape(n, crop, crop, 3), _oracle(resize, crop)), lead
        assert (got[:lead] == 0xA5).all() and (got[lead + size:] == 0xA5).all(), lead
    with pytest.raises(ValueError):
        preprocess_batch_fused(_host(_images()), resize, crop, out=torch.empty(n, crop, crop + 1, 3, dtype=torch.uint8, device="cuda")[:, :, :crop])


def test_two_consecutive_host_batches_through_the_reused_staging_buffer():
    """the second batch overwrites the pinned staging buffer the first one was copied from: both must equal the oracle"""
    from hawq_amd.image import preprocess_batch_fused
    imgs = _images()
    first = preprocess_batch_fused(_host(imgs), 40, 32)
    second = preprocess_batch_fused(_host(imgs[::-1]), 40, 32)
    third = preprocess_batch_fused(_host(imgs[3:8]), 40, 31)
    assert np.array_equal(first.cpu().numpy(), _oracle(40, 32))
    assert np.array_equal(second.cpu().numpy(), _oracle(40, 32)[::-1])
    assert np.array_equal(third.cpu().numpy(), _oracle(40, 31)[3:8])


def test_pillow_fixture_in_a_single_fused_call():
    """the nine geometries and the decoded JPEG of tests/golden/pillow_resize.npz: at (256, 224) the crops REAL Pillow recorded, at
    (342, 299) - InceptionV3's geometry, crop * 3 = 897 - the restated algorithm"""
    from hawq_amd.image import preprocess_batch_fused
    from oracle import pil_resample
    from tests.test_host_logic import _synth_image
    fx = H.load("pillow_resize.npz")
    imgs = [_synth_image(int(h), int(w), int(fx["seeds"][i])) for i, (h, w) in enumerate(fx["geoms"])] + [fx["jpeg_decoded"]]
    want = [fx[f"crop_{i}"] for i in range(len(fx["geoms"]))] + [fx["jpeg_crop"]]
    host = [torch.from_numpy(np.ascontiguousarray(im)) for im in imgs]
    got = preprocess_batch_fused(host, 256, 224).cpu().numpy()
    assert [i for i in range(len(want)) if not np.array_equal(got[i], want[i])] == []
    got = preprocess_batch_fused([t.cuda() for t in host], 342, 299).cpu().numpy()
    assert [i for i in range(len(imgs)) if not np.array_equal(got[i], pil_resample.resize_center_crop(imgs[i], 342, 299))] == []


def _jpeg_tree(root, rng, lo, hi):
    from PIL import Image
    for c in ("a", "b", "c"):
        (root / c).mkdir()
        for k in range(3):
            h, w = (int(v) for v in rng.integers(lo, hi, 2))
            yy, xx = np.mgrid[0:h, 0:w]
            pic = np.stack([(xx * 3 + k * 40) % 256, (yy * 2 + xx) % 256, rng.integers(0, 256, (h, w))], -1).astype(np.uint8)
            Image.fromarray(pic).save(root / c / f"{k}.jpg", quality=95)


def test_fused_threaded_folder_loader_equals_the_serial_loader(tmp_path):
    pytest.importorskip("PIL")
    from hawq_amd.image import folder_loader
    _jpeg_tree(tmp_path, np.random.default_rng(3), 45, 120)
    serial = list(folder_loader(str(tmp_path), batch_size=4, resize=40, crop=32))
    fused = list(folder_loader(str(tmp_path), batch_size=4, resize=40, crop=32, fused=True, workers=2))
    assert [tuple(b.shape) for b, _ in fused] == [tuple(b.shape) for b, _ in serial] == [(4, 32, 32, 3), (4, 32, 32, 3), (1, 32, 32, 3)]
    for (b0, t0), (b1, t1) in zip(serial, fused):
        assert torch.equal(t0, t1) and t1.dtype == torch.int64 and b1.is_cuda and torch.equal(b0, b1)
    threaded = list(folder_loader(str(tmp_path), batch_size=4, resize=40, crop=32, workers=2))   # the per-image path behind the thread pool
    assert all(torch.equal(b0, b1) and torch.equal(t0, t1) for (b0, t0), (b1, t1) in zip(serial, threaded))


def test_validate_gives_the_same_accuracy_through_either_loader(tmp_path):
    pytest.importorskip("PIL")
    from hawq_amd.api import calibrate, validate
    from hawq_amd.image import folder_loader
    from hawq_amd.skeleton import synthetic_images
    model = H.build_model("resnet18", "uniform8")
    calibrate(model, synthetic_images(4, seed=0).cuda())
    _jpeg_tree(tmp_path, np.random.default_rng(4), 240, 400)
    a = validate(model, folder_loader(str(tmp_path), batch_size=4), uint8=True)
    b = validate(model, folder_loader(str(tmp_path), batch_size=4, fused=True, workers=2), uint8=True)
    assert a == b and a[2] == 9
