"""Progressive JPEG decoding restated in Python / numpy from T.81 annex G (the four scan decoders: DC first, DC refinement, AC first with
end-of-band runs, AC refinement with correction bits), independent of the HIP code; the pixels come from ``jpeg_model.idct`` and the colour
code of the baseline model.  It takes the structure of a file from ``hawq_amd.jpeg.parse_jpeg(progressive=True)`` only.
``coefficients(rec)`` -> the quantised coefficients on the slab's (MCU-padded) grids, ``slab(comps)`` -> the same as the int16 words of
``hawq_jpeg_desc.coef_block0``, ``decode(data)`` -> uint8 [H, W, 3].

``write_progressive`` is the fixtures' own encoder: it re-emits given quantised coefficients under a given scan script, with Huffman tables
of its own in which every symbol a scan uses gets an 8-bit code.  tests/golden/make_jpeg_prog_cases.py accepts a file of it only when
Pillow decodes it to the bytes of the file the coefficients came from.
"""
import functools
import json
import struct

import numpy as np

from tests import helpers as H
from tests import jpeg_model
from tests.jpeg_model import NATURAL, _Bits, _code_book, _extend


def _i16(v):
    return ((int(v) + 0x8000) & 0xFFFF) - 0x8000


def scan_blocks(rec, s, unit):
    """(component, block row, block column) of the blocks of one unit of scan ``s``: an MCU, or one block of the component's own grid"""
    if len(s.comps) > 1:
        my, mx = divmod(unit, rec.mcus_x)
        return [(c, my * rec.components[c][2] + j, mx * rec.components[c][1] + i)
                for c in s.comps for j in range(rec.components[c][2]) for i in range(rec.components[c][1])]
    bw, _ = rec.own_grid(s.comps[0])
    by, bx = divmod(unit, bw)
    return [(s.comps[0], by, bx)]


def _correct(br, blk, n, p1, stats, key):
    stats[key] = stats.get(key, 0) + 1
    if br.take(1) and not (int(blk[n]) & p1):
        blk[n] += p1 if blk[n] >= 0 else -p1


def decode_scan(rec, s, comps, stats):
    """one scan onto ``comps`` (int16 [rows, cols, 64] per component, natural order)"""
    dc_books = [_code_book(t) for t in s.dc] if s.dc is not None else None
    ac_book = _code_book(s.ac) if s.ac is not None else None
    per = s.restart or s.units
    p1 = 1 << s.al
    if len(s.comps) == 1 and len(s.intervals) > 1:
        stats["own_grid_intervals"] = max(stats.get("own_grid_intervals", 0), len(s.intervals))
    for k, (first, last) in enumerate(s.intervals.tolist()):
        br = _Bits(rec.data[s.scan[0] + first:s.scan[0] + last])
        pred, eobrun = [0] * len(s.comps), 0
        for unit in range(k * per, min((k + 1) * per, s.units)):
            for c, by, bx in scan_blocks(rec, s, unit):
                blk = comps[c][by, bx]
                if s.ss == 0 and s.ah == 0:
                    ci = s.comps.index(c)
                    cat = br.symbol(dc_books[ci], stats)
                    pred[ci] += _extend(br.take(cat), cat)
                    blk[0] = _i16(pred[ci] << s.al)
                elif s.ss == 0:
                    if br.take(1):
                        blk[0] |= p1
                elif s.ah == 0:
                    if eobrun:
                        eobrun -= 1
                        continue
                    at = s.ss
                    while at <= s.se:
                        rs = br.symbol(ac_book, stats)
                        r, size = rs >> 4, rs & 15
                        if size:
                            at += r
                            blk[NATURAL[at]] = _i16(_extend(br.take(size), size) << s.al)
                        elif r == 15:
                            at += 15
                        else:
                            stats["eob_category"] = max(stats.get("eob_category", 0), r)
                            eobrun = (1 << r) + br.take(r) - 1
                            break
                        at += 1
                else:
                    at = s.ss
                    if not eobrun:
                        while at <= s.se:
                            rs = br.symbol(ac_book, stats)
                            r, size = rs >> 4, rs & 15
                            if size:
                                assert size == 1
                                value = p1 if br.take(1) else -p1
                            elif r != 15:
                                stats["eob_category"] = max(stats.get("eob_category", 0), r)
                                eobrun = (1 << r) + br.take(r)
                                break
                            else:
                                stats["refine_zrl"] = stats.get("refine_zrl", 0) + 1
                            while at <= s.se:
                                if blk[NATURAL[at]]:
                                    _correct(br, blk, NATURAL[at], p1, stats, "corrections")
                                else:
                                    r -= 1
                                    if r < 0:
                                        break
                                at += 1
                            if size:
                                blk[NATURAL[at]] = value
                            at += 1
                    if eobrun:
                        band = NATURAL[at:s.se + 1]
                        for n in band[blk[band] != 0]:
                            _correct(br, blk, n, p1, stats, "corrections_in_eob_run")
                        eobrun -= 1


def coefficients(rec, stats=None):
    """Quantised coefficients per component after all scans: int16 [block rows, block columns, 64] on the slab's grids."""
    stats = {} if stats is None else stats
    comps = [np.zeros((rec.mcus_y * v, rec.mcus_x * h, 64), np.int16) for _, h, v, _, _, _ in rec.components]
    for s in rec.scans:
        decode_scan(rec, s, comps, stats)
        if len(s.comps) == 1:
            bw, bh = rec.own_grid(s.comps[0])
            rows, cols = comps[s.comps[0]].shape[:2]
            stats["narrower_grid"] = stats.get("narrower_grid", 0) + (bw < cols or bh < rows)
    return comps


def slab(comps):
    """the int16 words of an image's blocks in the coefficient slab: component after component, rows of blocks"""
    return np.concatenate([c.reshape(-1) for c in comps])


def pixels(rec, comps):
    """coefficients -> uint8 [H, W, 3] with the IDCT, upsampling and colour code of the baseline model"""
    planes = [jpeg_model.idct(cf, rec.qtables[comp[3]]) for cf, comp in zip(comps, rec.components)]
    h, w = rec.height, rec.width
    y = planes[0][:h, :w].astype(np.int64)
    if len(planes) == 1:
        return np.repeat(y[:, :, None], 3, 2).astype(np.uint8)
    ch, cw = -(-h // rec.vs), -(-w // rec.hs)
    chroma = []
    for p in planes[1:]:
        sm = p[:ch, :cw]
        up = sm.astype(np.int64) if rec.hs == 1 else jpeg_model._h2v1(sm) if rec.vs == 1 else jpeg_model._h2v2(sm)
        chroma.append(up[:h, :w] - 128)
    cb, cr = chroma
    rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def decode(data, stats=None):
    from hawq_amd.jpeg import parse_jpeg
    rec = parse_jpeg(data, progressive=True)
    return pixels(rec, coefficients(rec, stats))


# ---------------------------------------------------------------------------------------------------------------------- the writer
class _Out:
    """Symbols and raw bits of one scan: recorded first (to learn which symbols the scan uses), then written."""

    def __init__(self):
        self.items = []   # ("sym", value) | ("bits", value, n) | ("rst", n)

    def sym(self, v):
        self.items.append(("sym", v))

    def bits(self, v, n):
        if n:
            self.items.append(("bits", v & ((1 << n) - 1), n))

    def render(self):
        """-> (HUFFVAL of the scan's table, entropy-coded bytes): symbol i of the sorted list has the 8-bit code i"""
        used = sorted({it[1] for it in self.items if it[0] == "sym"}) or [0]
        assert len(used) < 256
        code = {v: i for i, v in enumerate(used)}
        out, acc, n = bytearray(), 0, 0

        def flush_bytes():
            nonlocal acc, n
            while n >= 8:
                b = (acc >> (n - 8)) & 0xFF
                out.append(b)
                if b == 0xFF:
                    out.append(0)
                n -= 8
            acc &= (1 << n) - 1

        for it in self.items:
            if it[0] == "rst":
                if n % 8:
                    acc, n = (acc << (8 - n % 8)) | ((1 << (8 - n % 8)) - 1), n + 8 - n % 8
                flush_bytes()
                out += bytes([0xFF, 0xD0 + (it[1] & 7)])
                continue
            v, k = (code[it[1]], 8) if it[0] == "sym" else (it[1], it[2])
            acc, n = (acc << k) | v, n + k
            flush_bytes()
        if n % 8:
            acc, n = (acc << (8 - n % 8)) | ((1 << (8 - n % 8)) - 1), n + 8 - n % 8
        flush_bytes()
        return used, bytes(out)


def _emit_scan(out, comps, blocks_of, units, restart, ss, se, ah, al):
    """the symbols of one scan (the encoder of the library's jcphuff.c, restated): ``blocks_of(unit)`` -> [(component position, block)]"""
    pred, eobrun, pending = {}, 0, []   # pending: correction bits of the blocks inside the current end-of-band run

    def flush_eobrun():
        nonlocal eobrun
        if eobrun:
            cat = eobrun.bit_length() - 1
            out.sym(cat << 4)
            out.bits(eobrun, cat)
            eobrun = 0
        for b in pending:
            out.bits(b, 1)
        pending.clear()

    for unit in range(units):
        if restart and unit and unit % restart == 0:
            flush_eobrun()
            out.items.append(("rst", unit // restart - 1))
            pred.clear()
        for ci, blk in blocks_of(unit):
            if ss == 0 and ah == 0:
                v = int(blk[0]) >> al
                d = v - pred.get(ci, 0)
                pred[ci] = v
                cat = abs(d).bit_length()
                out.sym(cat)
                out.bits(d if d >= 0 else d - 1, cat)
            elif ss == 0:
                out.bits(int(blk[0]) >> al, 1)
            elif ah == 0:
                r = 0
                for k in range(ss, se + 1):
                    v = int(blk[NATURAL[k]])
                    t = abs(v) >> al
                    if not t:
                        r += 1
                        continue
                    flush_eobrun()
                    while r > 15:
                        out.sym(0xF0)
                        r -= 16
                    cat = t.bit_length()
                    out.sym((r << 4) | cat)
                    out.bits(t if v > 0 else ~t, cat)
                    r = 0
                if r:
                    eobrun += 1
                    if eobrun == 0x7FFF:
                        flush_eobrun()
            else:
                mags = [abs(int(blk[NATURAL[k]])) >> al for k in range(ss, se + 1)]
                last_new = max((i for i, t in enumerate(mags) if t == 1), default=-1)
                r, held = 0, []   # held: correction bits that follow the next symbol
                for i, t in enumerate(mags):
                    if not t:
                        r += 1
                        continue
                    while r > 15 and i <= last_new:
                        flush_eobrun()
                        out.sym(0xF0)
                        r -= 16
                        for b in held:
                            out.bits(b, 1)
                        held = []
                    if t > 1:
                        held.append(t & 1)
                        continue
                    flush_eobrun()
                    out.sym((r << 4) | 1)
                    out.bits(0 if blk[NATURAL[ss + i]] < 0 else 1, 1)
                    for b in held:
                        out.bits(b, 1)
                    held, r = [], 0
                if r or held:
                    eobrun += 1
                    pending.extend(held)
                    if eobrun == 0x7FFF or len(pending) > 900:
                        flush_eobrun()
    flush_eobrun()


def _segment(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + bytes(body)


def write_progressive(rec, comps, script):
    """A progressive file of the frame of ``rec`` (a record of ``parse_jpeg``: size, sampling, quantisation tables) holding the coefficients
    ``comps`` (int16 [rows, cols, 64] per component on the MCU-padded grids), written as the scans of ``script``: a list of dicts with
    ``comps`` (tuple of component indices), ``ss`` ``se`` ``ah`` ``al``, and optionally ``td`` / ``ta`` (the Huffman table ids the scan
    defines and uses, default 0) and ``restart`` (a DRI segment with this value is written before the scan; it stays in force)."""
    out = bytearray(b"\xff\xd8")
    for tq in sorted({c[3] for c in rec.components}):
        out += _segment(0xDB, bytes([tq]) + bytes(rec.qtables[tq].astype(np.uint8)))
    frame = bytes([8]) + struct.pack(">HH", rec.height, rec.width) + bytes([len(rec.components)])
    for cid, h, v, tq, _, _ in rec.components:
        frame += bytes([cid, (h << 4) | v, tq])
    out += _segment(0xC2, frame)
    restart = 0
    for s in script:
        if "restart" in s:
            restart = s["restart"]
            out += _segment(0xDD, struct.pack(">H", restart))
        cs, ss, se, ah, al = s["comps"], s["ss"], s["se"], s["ah"], s["al"]
        if len(cs) > 1:
            units = rec.mcus_x * rec.mcus_y

            def blocks_of(unit, cs=cs):
                my, mx = divmod(unit, rec.mcus_x)
                return [(ci, comps[c][my * rec.components[c][2] + j, mx * rec.components[c][1] + i])
                        for ci, c in enumerate(cs) for j in range(rec.components[c][2]) for i in range(rec.components[c][1])]
        else:
            _, h, v = rec.components[cs[0]][:3]
            bw, bh = -(-(-(-rec.width * h // rec.hs)) // 8), -(-(-(-rec.height * v // rec.vs)) // 8)
            units = bw * bh

            def blocks_of(unit, c=cs[0], bw=bw):
                return [(0, comps[c][unit // bw, unit % bw])]
        rec_out = _Out()
        _emit_scan(rec_out, comps, blocks_of, units, restart, ss, se, ah, al)
        used, stream = rec_out.render()
        td, ta = s.get("td", 0), s.get("ta", 0)
        needs_table = ss > 0 or ah == 0
        if needs_table:
            out += _segment(0xC4, bytes([(0x10 if ss > 0 else 0) | (ta if ss > 0 else td)]) + bytes([0] * 7 + [len(used)] + [0] * 8) + bytes(used))
        head = bytes([len(cs)])
        for c in cs:
            head += bytes([rec.components[c][0], (td << 4) | ta])
        out += _segment(0xDA, head + bytes([ss, se, (ah << 4) | al])) + stream
    return bytes(out + b"\xff\xd9")


def script_spectral(ncomp):
    """spectral selection only: the DC as single-component scans, then bands 1-2 / 3-9 / 10-63 per component"""
    sc = [dict(comps=(c,), ss=0, se=0, ah=0, al=0) for c in range(ncomp)]
    return sc + [dict(comps=(c,), ss=a, se=b, ah=0, al=0) for a, b in ((1, 2), (3, 9), (10, 63)) for c in range(ncomp)]


def script_deep(ncomp, tables=False, top=4):
    """successive approximation one bit at a time: DC Al top -> 0 interleaved, AC Al top -> 0 per component: top + 1 scans of every
    coefficient, so top + 1 levels (five by default); ``tables``: the scans take Huffman table ids 2 and 3 by turns"""
    every = tuple(range(ncomp))
    sc = [dict(comps=every, ss=0, se=0, ah=0, al=top)] + [dict(comps=(c,), ss=1, se=63, ah=0, al=top) for c in range(ncomp)]
    for al in range(top - 1, -1, -1):
        sc += [dict(comps=every, ss=0, se=0, ah=al + 1, al=al)] + [dict(comps=(c,), ss=1, se=63, ah=al + 1, al=al) for c in range(ncomp)]
    if tables:
        for i, s in enumerate(sc):
            s["td"], s["ta"] = 2 + i % 2, 3 - i % 2
    return sc


def script_dri(ncomp):
    """Pillow's script with a restart interval that changes between scans (and is switched off for the last ones)"""
    every = tuple(range(ncomp))
    sc = [dict(comps=every, ss=0, se=0, ah=0, al=1, restart=2), dict(comps=(0,), ss=1, se=5, ah=0, al=2, restart=3)]
    sc += [dict(comps=(c,), ss=1, se=63, ah=0, al=1, restart=5 - c) for c in range(ncomp - 1, 0, -1)]
    sc += [dict(comps=(0,), ss=6, se=63, ah=0, al=2), dict(comps=(0,), ss=1, se=63, ah=2, al=1, restart=7), dict(comps=every, ss=0, se=0, ah=1, al=0, restart=1)]
    sc += [dict(comps=(c,), ss=1, se=63, ah=1, al=0, restart=0) for c in range(ncomp - 1, 0, -1)]
    return sc + [dict(comps=(0,), ss=1, se=63, ah=1, al=0)]


HOST_CHECK_SEED = 2027   # the seed tests/test_jpeg_prog_host.py gives tools/jpeg_prog_host_check.cpp


def overwrite_draws(seed, scan, stream_len, n=200):
    """The (position, value) pairs tools/jpeg_prog_host_check.cpp overwrites in the stream of scan ``scan`` (index into the blob's scan
    table), for ``seed``."""
    return jpeg_model.overwrite_draws(seed, scan, stream_len, n)


@functools.lru_cache(maxsize=None)
def cases():
    """(accepted {name: (file bytes, Pillow's RGB)}, refused {name: (file bytes, reason)}, conditions) of jpeg_prog_cases.npz"""
    z = H.load("jpeg_prog_cases.npz")
    good = {str(n): (z["jpeg_" + str(n)].tobytes(), z["rgb_" + str(n)]) for n in z["names"]}
    bad = {str(n): (z["refused_" + str(n)].tobytes(), str(r)) for n, r in zip(z["refused_names"], z["refused_reasons"])}
    return good, bad, json.loads(str(z["conditions"]))


@functools.lru_cache(maxsize=None)
def model_coefficients():
    """{name: (record, coefficients per component)} of every accepted case, decoded once by the model; read-only for the tests"""
    from hawq_amd.jpeg import parse_jpeg
    out = {}
    for name, (data, _) in cases()[0].items():
        rec = parse_jpeg(data, progressive=True)
        out[name] = (rec, coefficients(rec))
    return out
