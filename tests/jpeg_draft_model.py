"""A numpy restatement of libjpeg's reduced-size decoding (DCT-domain scaling, what Pillow's ``Image.draft`` switches on), written from
jdmaster.c / jidctred.c / jdsample.c as DESIGN.md 12.5 states them, independent of the HIP text.  Coefficients come from the models of
the full-size decoders (tests/jpeg_model.py, tests/jpeg_prog_model.py).  ``decode(data, scale)`` -> uint8 [ceil(H / s), ceil(W / s), 3].
"""
import functools
import json

import numpy as np

from tests import helpers as H
from tests import jpeg_model, jpeg_prog_model

SCALES = (2, 4, 8)


def pillow_scale(width, height, draft):
    """the scale ``Image.draft("RGB", draft)`` picks for a width x height JPEG"""
    k = min(width // draft[0], height // draft[1])
    return next((s for s in (8, 4, 2) if s <= k), 1)


def request_for(width, height, scale):
    """a draft request that gives a width x height file the scale ``scale`` (at most its short side)"""
    return max(width // scale, 1), max(height // scale, 1)


def block_size(h, v, hmax, vmax, scale):
    """samples per block side of a component with sampling (h, v) at 1 / scale (jdmaster.c)"""
    m = n = 8 // scale
    while n < 8 and 2 * h * n <= hmax * m and 2 * v * n <= vmax * m:
        n *= 2
    return n


def _wrap(x):
    """int64 -> the int32 a wrapping 32-bit sum gives"""
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _descale(x, shift):
    return _wrap(_wrap(x) + (1 << (shift - 1))) >> shift


def _pass4(x, shift):
    """one pass of the 4x4 inverse DCT along the last axis of int64 [..., 8] -> [..., 4]"""
    tmp0 = x[..., 0] << 14
    tmp2 = 15137 * x[..., 2] - 6270 * x[..., 6]
    tmp10, tmp12 = tmp0 + tmp2, tmp0 - tmp2
    t0 = -1730 * x[..., 7] + 11893 * x[..., 5] - 17799 * x[..., 3] + 8697 * x[..., 1]
    t2 = -4176 * x[..., 7] - 4926 * x[..., 5] + 7373 * x[..., 3] + 20995 * x[..., 1]
    return _descale(np.stack([tmp10 + t2, tmp12 + t0, tmp12 - t0, tmp10 - t2], -1), shift)


def _pass2(x, shift):
    tmp10 = x[..., 0] << 15
    t0 = -5906 * x[..., 7] + 6967 * x[..., 5] - 10426 * x[..., 3] + 29692 * x[..., 1]
    return _descale(np.stack([tmp10 + t0, tmp10 - t0], -1), shift)


def _limit(x):
    x = x & 0x3FF
    return np.where(x < 128, x + 128, np.where(x < 512, 255, np.where(x < 896, 0, x - 896))).astype(np.uint8)


def idct(coef, qt_zigzag, n):
    """int16 [rows, cols, 64] natural order, uint16 [64] zig-zag order -> uint8 plane [rows * n, cols * n] of the n x n inverse DCT"""
    if n == 8:
        return jpeg_model.idct(coef, qt_zigzag)
    q = np.zeros(64, np.int64)
    q[jpeg_model.NATURAL] = qt_zigzag
    x = (coef.astype(np.int64) * q).reshape(coef.shape[0], coef.shape[1], 8, 8)   # [.., row, column]
    if n == 1:
        s = _limit((x[..., 0, 0] + 4) >> 3)[..., None, None]
    else:
        one, first, second = (_pass4, 12, 19) if n == 4 else (_pass2, 13, 20)
        ws = one(x.swapaxes(-1, -2), first).swapaxes(-1, -2)   # columns first: [.., n rows, 8 columns]
        s = _limit(one(ws, second))
    return s.transpose(0, 2, 1, 3).reshape(coef.shape[0] * n, coef.shape[1] * n)


def pixels(rec, comps, scale):
    """coefficients of the record -> uint8 [ceil(H / scale), ceil(W / scale), 3]"""
    m = 8 // scale
    oh, ow = -(-rec.height // scale), -(-rec.width // scale)
    planes, real = [], []
    for cf, (_, h, v, tq) in zip(comps, (c[:4] for c in rec.components)):
        n = block_size(h, v, rec.hs, rec.vs, scale)
        planes.append(idct(cf, rec.qtables[tq], n))
        real.append((-(-rec.height * v * n // (8 * rec.vs)), -(-rec.width * h * n // (8 * rec.hs))))
    assert real[0] == (oh, ow)
    y = planes[0][:oh, :ow].astype(np.int64)
    if len(planes) == 1:
        return np.repeat(y[:, :, None], 3, 2).astype(np.uint8)
    chroma = []
    for p, (ch, cw) in zip(planes[1:], real[1:]):
        s = p[:ch, :cw]
        if (ch, cw) == (oh, ow):   # 4:4:4, and 4:2:0 whose chroma blocks are twice as large
            up = s.astype(np.int64)
        else:                      # 4:2:2: h2v1, fancy unless the scale is 8 or the row has at most two samples
            assert ch == oh and (rec.hs, rec.vs) == (2, 1)
            up = jpeg_model._h2v1(s) if m > 1 and cw > 2 else np.repeat(s.astype(np.int64), 2, 1)
        chroma.append(up[:oh, :ow] - 128)
    cb, cr = chroma
    rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _coefficients(data):
    from hawq_amd.jpeg import JpegProgRecord, parse_jpeg
    rec = parse_jpeg(data, progressive=True)
    return rec, (jpeg_prog_model if isinstance(rec, JpegProgRecord) else jpeg_model).coefficients(rec)


def decode(data, scale):
    """file bytes -> what Pillow decodes after a draft that picks ``scale`` (1: the full-size models)"""
    rec, comps = _coefficients(bytes(data))
    if scale == 1:
        return jpeg_prog_model.pixels(rec, comps)
    return pixels(rec, comps, scale)


@functools.lru_cache(maxsize=None)
def cases():
    """({name: (file bytes, {scale: ((draft width, draft height), Pillow's RGB)})}, conditions) of jpeg_draft_cases.npz"""
    z = H.load("jpeg_draft_cases.npz")
    out = {}
    for n in (str(n) for n in z["names"]):
        out[n] = (z["jpeg_" + n].tobytes(), {s: (tuple(int(v) for v in z["draft_%s_%d" % (n, s)]), z["rgb_%s_%d" % (n, s)]) for s in SCALES if "rgb_%s_%d" % (n, s) in z.files})
    return out, json.loads(str(z["conditions"]))


def flat_cases():
    """[(name, scale, file bytes, draft request, Pillow's RGB)] of every fixture at every scale it has"""
    return [(n, s, data, draft, rgb) for n, (data, per) in cases()[0].items() for s, (draft, rgb) in per.items()]
