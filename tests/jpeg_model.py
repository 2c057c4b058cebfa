"""A numpy restatement of baseline JPEG decoding as libjpeg-turbo does it (Huffman decoding, ISLOW IDCT, fancy upsampling, YCbCr -> RGB),
written from T.81 and the formulas of DESIGN.md "Device JPEG decode", independent of the HIP code.  It takes the structure of a file
from ``hawq_amd.jpeg.parse_jpeg`` only.  ``decode(data)`` -> uint8 [H, W, 3]; slow (the entropy decoder is a Python loop), for fixtures.
"""
import functools
import json
import os

import numpy as np

from tests import helpers as H

NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
                    57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def _code_book(table):
    """{(length, code): value} of one hawq_jpeg_huff record"""
    book = {}
    mincode, maxcode, valptr, huffval = (table[k][0] for k in ("mincode", "maxcode", "valptr", "huffval"))
    for length in range(1, 17):
        for code in range(int(mincode[length]), int(maxcode[length]) + 1) if maxcode[length] >= 0 else ():
            book[(length, code)] = int(huffval[valptr[length] + code - mincode[length]])
    return book


class _Bits:
    def __init__(self, raw: bytes):
        raw = raw.replace(b"\xff\x00", b"\xff")
        self.bits = np.unpackbits(np.frombuffer(raw, np.uint8)).tolist()
        self.at = 0

    def take(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bits[self.at]
            self.at += 1
        return v

    def symbol(self, book, stats):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bits[self.at]
            self.at += 1
            if (length, code) in book:
                stats["longest_code"] = max(stats.get("longest_code", 0), length)
                return book[(length, code)]
        raise ValueError("no such code")


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def coefficients(rec, stats=None):
    """Quantised coefficients per component: int16 [block rows, block columns, 64] in natural order."""
    stats = {} if stats is None else stats
    comps = []
    for c, (_, h, v, _, _, _) in enumerate(rec.components):
        comps.append(np.zeros((rec.mcus_y * v, rec.mcus_x * h, 64), np.int16))
    books = [(_code_book(rec.huffman[(0, td)]), _code_book(rec.huffman[(1, ta)])) for (_, _, _, _, td, ta) in rec.components]
    mcus = rec.mcus_x * rec.mcus_y
    per = rec.restart or mcus
    stats["intervals"] = len(rec.intervals)
    stats["stuffed"] = stats.get("stuffed", 0) + rec.data[rec.scan[0]:rec.scan[1]].count(b"\xff\x00")
    for k, (first, last) in enumerate(rec.intervals.tolist()):
        br = _Bits(rec.data[rec.scan[0] + first:rec.scan[0] + last])
        pred = [0] * len(comps)
        for m in range(k * per, min((k + 1) * per, mcus)):
            my, mx = divmod(m, rec.mcus_x)
            for c, (_, h, v, _, _, _) in enumerate(rec.components):
                for j in range(v):
                    for i in range(h):
                        blk = comps[c][my * v + j, mx * h + i]
                        s = br.symbol(books[c][0], stats)
                        pred[c] += _extend(br.take(s), s)
                        blk[0] = np.int16(((pred[c] + 0x8000) & 0xFFFF) - 0x8000)
                        at = 1
                        while at < 64:
                            rs = br.symbol(books[c][1], stats)
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                stats["zrl"] = stats.get("zrl", 0) + 1
                                at += 16
                                continue
                            at += r
                            blk[NATURAL[at]] = _extend(br.take(s), s)
                            at += 1
    return comps


def _pass(x, shift):
    """one ISLOW pass along the last axis of int64 [..., 8]"""
    z2, z3 = x[..., 2], x[..., 6]
    z1 = (z2 + z3) * 4433
    tmp2, tmp3 = z1 - z3 * 15137, z1 + z2 * 6270
    tmp0, tmp1 = (x[..., 0] + x[..., 4]) << 13, (x[..., 0] - x[..., 4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3], -1)
    return (out + (1 << (shift - 1))) >> shift


def idct(coef, qt_zigzag):
    """int16 [rows, cols, 64] natural order, uint16 [64] zig-zag order -> uint8 plane [rows * 8, cols * 8]"""
    q = np.zeros(64, np.int64)
    q[NATURAL] = qt_zigzag
    x = (coef.astype(np.int64) * q).reshape(coef.shape[0], coef.shape[1], 8, 8)
    x = _pass(x.swapaxes(-1, -2), 11).swapaxes(-1, -2)   # columns
    x = _pass(x, 18) & 0x3FF
    s = np.where(x < 128, x + 128, np.where(x < 512, 255, np.where(x < 896, 0, x - 896))).astype(np.uint8)
    return s.transpose(0, 2, 1, 3).reshape(coef.shape[0] * 8, coef.shape[1] * 8)


def _h2v1(s):
    s = s.astype(np.int64)
    left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.empty((s.shape[0], s.shape[1] * 2), np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * s + left + 1) >> 2, (3 * s + right + 2) >> 2
    return out


def _h2v2(s):
    s = s.astype(np.int64)
    above, below = np.concatenate([s[:1], s[:-1]]), np.concatenate([s[1:], s[-1:]])
    out = np.empty((s.shape[0] * 2, s.shape[1] * 2), np.int64)
    for row, far in ((0, above), (1, below)):
        t = 3 * s + far
        left, right = np.concatenate([t[:, :1], t[:, :-1]], 1), np.concatenate([t[:, 1:], t[:, -1:]], 1)
        out[row::2, 0::2], out[row::2, 1::2] = (3 * t + left + 8) >> 4, (3 * t + right + 7) >> 4
    return out


def decode(data, stats=None):
    from hawq_amd.jpeg import parse_jpeg
    rec = parse_jpeg(data)
    planes = [idct(cf, rec.qtables[comp[3]]) for cf, comp in zip(coefficients(rec, stats), rec.components)]
    h, w = rec.height, rec.width
    y = planes[0][:h, :w].astype(np.int64)
    if len(planes) == 1:
        return np.repeat(y[:, :, None], 3, 2).astype(np.uint8)
    ch, cw = -(-h // rec.vs), -(-w // rec.hs)
    chroma = []
    for p in planes[1:]:
        s = p[:ch, :cw]
        up = s.astype(np.int64) if rec.hs == 1 else _h2v1(s) if rec.vs == 1 else _h2v2(s)
        chroma.append(up[:h, :w] - 128)
    cb, cr = chroma
    rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8)

HOST_CHECK_SEED = 2026   # the seed tests/test_jpeg_host.py gives tools/jpeg_host_check.cpp


def overwrite_draws(seed, image, stream_len, n=200):
    """The (position, value) pairs tools/jpeg_host_check.cpp overwrites in the stream of image `image` of its blob, for `seed`."""
    mask = (1 << 64) - 1
    rng = (seed * 0x9E3779B97F4A7C15 + image) & mask
    out = []
    for _ in range(n):
        rng = (rng * 6364136223846793005 + 1442695040888963407) & mask
        out.append(((rng >> 33) % stream_len, (rng >> 24) & 0xFF))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """(accepted {name: (file bytes, Pillow's RGB)}, refused {name: (file bytes, reason, Pillow's RGB or None)}, conditions) of jpeg_cases.npz"""
    z = H.load("jpeg_cases.npz")
    good = {str(n): (z["jpeg_" + str(n)].tobytes(), z["rgb_" + str(n)]) for n in z["names"]}
    bad = {str(n): (z["refused_" + str(n)].tobytes(), str(r), z["refused_rgb_" + str(n)] if "refused_rgb_" + str(n) in z.files else None)
           for n, r in zip(z["refused_names"], z["refused_reasons"])}
    return good, bad, json.loads(str(z["conditions"]))


def sample():
    with open(os.path.join(H.GOLDEN, "sample_500x375.jpg"), "rb") as f:
        return f.read()
