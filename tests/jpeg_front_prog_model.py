"""What the tests of the device front end for progressive files (csrc/jpeg_front_prog.h, hawq_amd.jpeg ``progressive="device"``;
DESIGN.md 12.6) share: the comparison of the walker's records with a ``JpegProgRecord``, a numpy model of the fill, and the files that
move a progressive file's markers through every phase of the kernel's passes."""
import functools

import numpy as np

from tests import jpeg_front_corpus as F
from tests import jpeg_prog_model


def parse(data):
    from hawq_amd.jpeg import UnsupportedJpeg, parse_jpeg
    try:
        return parse_jpeg(data, progressive=True)
    except UnsupportedJpeg:
        return None


@functools.lru_cache(maxsize=None)
def prog_fixtures():
    """(names, files) of the accepted progressive fixtures, in the order of the planner pins"""
    prog, _, _ = jpeg_prog_model.cases()
    return list(prog), [prog[n][0] for n in prog]


def _table(data, at):
    from hawq_amd.jpeg import huffman_table
    bits = data[at:at + 16]
    return huffman_table(bits, data[at + 16:at + 16 + sum(bits)])


def prog_mismatch(data, o, scans, r):
    """None when the info record ``o`` and the scan records ``scans`` (the file's 64) of the file ``data`` say what the
    ``JpegProgRecord`` ``r`` says, else which field does not"""
    from hawq_amd.jpeg import scan_levels
    if int(o["defer"]) != 0 or int(o["reserved"][0]) != 1:
        return "defer %d kind %d" % (o["defer"], o["reserved"][0])
    for f in ("width", "height", "ncomp", "hs", "vs"):
        if int(o[f]) != getattr(r, f):
            return f
    if int(o["reserved"][1]) != len(r.scans):
        return "n_scans"
    if any(int(o[f]) for f in ("restart", "n_intervals", "scan_first", "scan_end")) or o["td"].any() or o["ta"].any() or o["huff_at"].any() or o["reserved"][2:].any():
        return "a baseline field of a progressive record"
    for c, comp in enumerate(r.components):
        tq = int(o["tq"][c])
        if tq != comp[3] or not np.array_equal(np.frombuffer(data, np.uint8, 64, int(o["qt_at"][tq])), r.qtables[tq]):
            return "quantisation table"
    if o["tq"][r.ncomp:].any():
        return "ids of a component the file does not have"
    for k, (s, q, level) in enumerate(zip(r.scans, scans, scan_levels(r.scans))):
        got = tuple(int(q[f]) for f in ("ncomp", "comp0", "ss", "se", "ah", "al", "level", "restart", "n_intervals", "scan_first", "scan_end"))
        if got != (len(s.comps), s.comps[0], s.ss, s.se, s.ah, s.al, level, s.restart, len(s.intervals), s.scan[0], s.scan[1]):
            return "scan %d: %r" % (k, got)
        dc = list(s.dc or ())
        for i in range(3):
            if bool(q["dc_at"][i]) != (i < len(dc)) or (i < len(dc) and _table(data, int(q["dc_at"][i])).tobytes() != dc[i].tobytes()):
                return "scan %d: DC table %d" % (k, i)
        if bool(q["ac_at"]) != (s.ac is not None) or (s.ac is not None and _table(data, int(q["ac_at"])).tobytes() != s.ac.tobytes()):
            return "scan %d: AC table" % k
        if q["reserved"]:
            return "scan %d: reserved" % k
    if scans[len(r.scans):].view(np.int32).any():
        return "a record behind the last scan"
    return None


def host_fill_prog(datas, info, scans, lay):
    """What ``hawq_jpeg_front_fill_prog`` and the upload of the head leave in the blob: a numpy model from the walker's records alone"""
    blob = np.zeros(lay.nbytes, np.uint8)
    blob[:lay.head.size] = lay.head

    def put(off, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        blob[off:off + raw.size] = raw

    for pl in lay.place:
        data, o, s = datas[pl["file"]], info[pl["file"]], scans[pl["file"], pl["scan"]]
        for c in range(3):
            if pl["qt_off"][c]:
                put(pl["qt_off"][c], np.frombuffer(data, np.uint8, 64, int(o["qt_at"][o["tq"][c]])).astype(np.uint16))
            if pl["dc_off"][c]:
                put(pl["dc_off"][c], _table(data, int(s["dc_at"][c])))
        if pl["ac_off"]:
            put(pl["ac_off"], _table(data, int(s["ac_at"])))
        put(pl["interval_off"], F.intervals_of(data, int(s["scan_first"]), int(s["scan_end"])))
        put(pl["stream_off"], np.frombuffer(data, np.uint8, int(s["scan_end"] - s["scan_first"]), int(s["scan_first"])))
    return blob


def comment(k):
    """a COM segment with ``k`` bytes of text"""
    return b"\xff\xfe" + bytes([(k + 2) >> 8, (k + 2) & 255]) + b"c" * k


@functools.lru_cache(maxsize=None)
def phase_files():
    """``noise_40x24_420_rst`` (progressive, restart markers in every scan) with a comment in front of its frame header and another
    between its second and third scan: the first of every length 0..1039 beside an empty second one, which moves the markers of every
    scan through all phases of the kernel's 16-byte chunk per lane and its 1 KiB pass, then the second of every length beside an empty
    first one, which moves the later scans alone."""
    from hawq_amd.jpeg import parse_jpeg
    prog, _, _ = jpeg_prog_model.cases()
    data = prog["noise_40x24_420_rst"][0]
    r = parse_jpeg(data, progressive=True)
    assert len(r.scans) >= 3 and all(len(s.intervals) > 1 for s in r.scans)
    sof = data.index(b"\xff\xc2")
    between = r.scans[1].scan[1]   # where the marker behind the second scan stands
    return [data[:sof] + comment(a) + data[sof:between] + comment(b) + data[between:] for a, b in [(k, 0) for k in range(1024 + 16)] + [(0, k) for k in range(1024 + 16)]]
