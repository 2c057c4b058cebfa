"""InceptionV3 uint8 input, host side (no GPU): the launch contract of hawq_incep_stem_u8, the conv1 weight packer, the input
table and the per-architecture image geometry."""
import ctypes

import numpy as np
import pytest
import torch

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _good_args():
    """a valid conv1 description; the pointers are never dereferenced by the _ok query"""
    from hawq_amd import _lib
    a = _lib.IncepConvArgs()
    a.in_, a.wgt, a.bias, a.out, a.m, a.ek = None, 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad_h, a.pad_w = 2, 299, 299, 3, 32, 3, 3, 2, 0, 0
    a.epilogue, a.relu, a.q_lo, a.q_hi, a.out_bits, a.ldo, a.c_off = _lib.INCEP_REQUANT, 1, -128, 127, 8, 32, 0
    return a


def _ok(a, x=0x60000, lut=0x70000):
    from hawq_amd import _lib
    return _lib.load().hawq_incep_stem_u8_ok(x, lut, ctypes.byref(a) if a is not None else None)


def test_stem_u8_ok_accepts_conv1_and_refuses_everything_else():
    assert _ok(_good_args()) == 1
    for ldo, c_off, cout, lo, hi in ((48, 16, 32, 0, 15), (16, 0, 16, -8, 7), (64, 0, 48, 0, 127)):
        a = _good_args()
        a.ldo, a.c_off, a.Cout, a.q_lo, a.q_hi = ldo, c_off, cout, lo, hi
        assert _ok(a) == 1, (ldo, c_off, cout)
    a = _good_args()
    a.H, a.W = 3, 3
    assert _ok(a) == 1
    assert _ok(None) == 0
    assert _ok(_good_args(), x=None) == 0
    assert _ok(_good_args(), lut=None) == 0
    assert _ok(_good_args(), lut=0x70002) == 0   # the table is read as dwords
    bad = {
        "in_": 0x80000, "wgt": None, "bias": None, "out": None, "m": None, "ek": None,
        "N": 0, "H": 2, "W": 2, "Cin": 16, "Cout": 24, "KH": 5, "KW": 1, "stride": 1, "pad_h": 1, "pad_w": 1,
        "epilogue": 0, "out_bits": 16, "q_lo": -129, "q_hi": 128, "ldo": 24, "c_off": 8,
    }
    for field, value in bad.items():
        a = _good_args()
        setattr(a, field, value)
        assert _ok(a) == 0, field
    a = _good_args()
    a.epilogue = 2   # REQUANT2
    assert _ok(a) == 0
    a = _good_args()
    a.q_lo, a.q_hi = 5, 4
    assert _ok(a) == 0
    a = _good_args()
    a.ldo, a.c_off = 32, 16   # the slice would run past the row
    assert _ok(a) == 0
    a = _good_args()
    a.out = 0x30008   # the 16-byte stores need an aligned output
    assert _ok(a) == 0
    a = _good_args()
    a.N, a.H, a.W = 1 << 16, 1 << 10, 1 << 10   # more than 2^31 output pixels
    assert _ok(a) == 0


def test_stem_weight_packing_equals_the_conv():
    """k = (kh * 3 + kw) * 3 + c: the dot products of the packed rows with the NHWC window bytes are F.conv2d, exactly."""
    from hawq_amd.engine_inception import pack_stem_u8_weights
    g = torch.Generator().manual_seed(3)
    for cout, cout_p in ((32, 32), (16, 32), (48, 48)):
        w = torch.randint(-128, 128, (cout, 3, 3, 3), generator=g, dtype=torch.int8)
        x = torch.randint(-128, 128, (2, 3, 11, 14), generator=g, dtype=torch.int8)
        packed = pack_stem_u8_weights(w.numpy(), cout_p)
        assert packed.shape == (cout_p, 32) and packed.dtype == np.int8
        assert not packed[:, 27:].any() and not packed[cout:].any()
        ref = torch.nn.functional.conv2d(x.double(), w.double(), stride=2).round().long().numpy()
        xn = x.permute(0, 2, 3, 1).numpy().astype(np.int64)   # NHWC
        N, H, W, _ = xn.shape
        Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        got = np.zeros((N, cout_p, Ho, Wo), np.int64)
        for oy in range(Ho):
            for ox in range(Wo):
                win = xn[:, 2 * oy:2 * oy + 3, 2 * ox:2 * ox + 3, :].reshape(N, 27)   # (kh, kw, c) order
                kv = np.concatenate([win, np.full((N, 5), 99, np.int64)], 1)     # bytes 27..31 meet zero weights
                got[:, :, oy, ox] = kv @ packed.astype(np.int64).T
        assert np.array_equal(got[:, :cout], ref)
        assert not got[:, cout:].any()


def _inception_with_input_range(x_min, x_max):
    from hawq_amd.api import build_quantized_resnet
    q = build_quantized_resnet("inceptionv3", "uniform8", seed=None)
    ia = q.features.q_init_block.q_input_activ
    ia.x_min.fill_(x_min), ia.x_max.fill_(x_max)
    return q, ia


@pytest.mark.parametrize("rng", [(-2.1179, 2.64), (-1.5, 1.9), (-3.0, 0.7)])
def test_input_table_equals_quantising_the_normalised_image(rng):
    """input_quant_lut with InceptionV3's input range = rint(fl(1/S) * Normalize(ToTensor(u))).clamp(lo, hi) for all 3 x 256 entries,
    ToTensor and Normalize spelt as torchvision does them on an image tensor; the engine's table is built from the same
    (fl(1/S), lo, hi) as the fp32 plan's hawq_fakequant_f32 launch."""
    from hawq_amd.engine_inception import InceptionEngine, _rng, _scale
    from hawq_amd.quant_utils import input_quant_lut
    q, ia = _inception_with_input_range(*rng)
    eng = InceptionEngine(q)
    inv, lo, hi = eng._input_quant()
    assert (inv, lo, hi) == (float((1. / _scale(ia)).item()), *_rng(ia)) and (lo, hi) == (-128, 127)
    img = torch.arange(256, dtype=torch.uint8).view(1, 16, 16).expand(3, 16, 16).contiguous()   # C x H x W, every value
    t = img.to(torch.float32).div(255)                                                            # ToTensor
    t = t.sub(torch.tensor(MEAN).view(3, 1, 1)).div(torch.tensor(STD).view(3, 1, 1))            # Normalize
    want = torch.round(torch.tensor(inv, dtype=torch.float32) * t).clamp(lo, hi).to(torch.int8).view(3, 256)
    assert torch.equal(input_quant_lut(inv, MEAN, STD, lo, hi), want)
    assert torch.equal(eng.input_lut(MEAN, STD), want)
    assert int(want.min()) < 0 < int(want.max())


def test_eval_geometry_per_architecture():
    from hawq_amd.image import eval_geometry
    assert eval_geometry("inceptionv3") == (342, 299)
    for arch in ("resnet18", "resnet50", "mobilenetv2_w1"):
        assert eval_geometry(arch) == (256, 224)


def _torchvision_geometry(h, w, size, crop):
    """torchvision Resize(int) on a PIL image (short side -> size, long side int(size * long / short)) + CenterCrop's offsets"""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    ow, oh = (new_short, new_long) if w <= h else (new_long, new_short)
    return oh, ow, int(round((oh - crop) / 2.0)), int(round((ow - crop) / 2.0))


@pytest.mark.parametrize("size,crop", [(342, 299), (256, 224)])
def test_resize_crop_geometry_follows_torchvision(size, crop):
    from hawq_amd.image import resize_crop_geometry
    for h, w in ((500, 375), (375, 500), (342, 342), (299, 400), (640, 343), (1024, 683), (333, 1000), (360, 360), (342, 455)):
        assert resize_crop_geometry(h, w, size, crop) == _torchvision_geometry(h, w, size, crop), (h, w)


def test_pil_resample_oracle_equals_pillow_at_inception_geometry():
    pytest.importorskip("PIL")
    from PIL import Image
    from oracle.pil_resample import resize_center_crop
    rng = np.random.default_rng(5)
    for h, w in ((400, 350), (350, 520), (342, 342), (600, 343)):
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(xx * 5 + yy) % 256, (yy * 3) % 256, rng.integers(0, 256, (h, w))], -1).astype(np.uint8)
        oh, ow, top, left = _torchvision_geometry(h, w, 342, 299)
        want = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))[top:top + 299, left:left + 299]
        got = resize_center_crop(img, 342, 299)
        assert got.shape == (299, 299, 3)
        assert np.array_equal(np.asarray(got), want), (h, w)


def test_forward_uint8_refuses_host_tensors():
    """There is no CPU path: a uint8 batch that is not on the MI355X is refused before any device work."""
    from hawq_amd.engine_inception import InceptionEngine
    q, _ = _inception_with_input_range(-2.1, 2.6)
    with pytest.raises(NotImplementedError):
        InceptionEngine(q).forward_uint8(torch.zeros(1, 299, 299, 3, dtype=torch.uint8))
