"""What the tests of the device JPEG front end (csrc/jpeg_front.h, hawq_amd.jpeg ``front_end="device"``) share: the mutation corpus,
the comparison of an info record with a ``JpegRecord``, and a numpy model of the fill."""
import functools

import numpy as np

from tests import jpeg_model, jpeg_pins


@functools.lru_cache(maxsize=None)
def fixture_files():
    """[(name, bytes)]: every accepted baseline fixture, the committed sample, the refused files, and the progressive fixtures"""
    from tests import jpeg_prog_model
    good, bad, _ = jpeg_model.cases()
    prog, prog_bad, _ = jpeg_prog_model.cases()
    out = [(n, good[n][0]) for n in good] + [("sample", jpeg_model.sample())]
    out += [("refused_" + n, bad[n][0]) for n in bad] + [("prog_" + n, prog[n][0]) for n in prog] + [("prog_refused_" + n, prog_bad[n][0]) for n in prog_bad]
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    """Every mutation of ``jpeg_pins``: byte by byte for ``BYTE_FIXTURES``, structural for the other small fixtures; in a fixed order,
    without duplicates."""
    seen, out = set(), []
    for name, (data, every_byte) in jpeg_pins.fixtures().items():
        for _, first, end, n_bytes in jpeg_pins.units(data):
            for mutated in jpeg_pins.mutations(data, first, end, n_bytes if every_byte else 0):
                if mutated not in seen:
                    seen.add(mutated)
                    out.append(mutated)
    return out


def record_mismatch(data, o, r):
    """None when the info record ``o`` of the file ``data`` says what the ``JpegRecord`` ``r`` says, else which field does not"""
    from hawq_amd.jpeg import huffman_table
    if int(o["defer"]) != 0:
        return "defer %d" % o["defer"]
    for f in ("width", "height", "ncomp", "hs", "vs", "restart"):
        if int(o[f]) != getattr(r, f):
            return f
    if int(o["n_intervals"]) != len(r.intervals) or (int(o["scan_first"]), int(o["scan_end"])) != tuple(r.scan):
        return "scan"
    for c, comp in enumerate(r.components):
        tq, td, ta = int(o["tq"][c]), int(o["td"][c]), int(o["ta"][c])
        if (tq, td, ta) != tuple(comp[3:6]):
            return "table ids"
        at = int(o["qt_at"][tq])
        if not np.array_equal(np.frombuffer(data, np.uint8, 64, at), r.qtables[tq]):
            return "quantisation table"
        for cls, tid in ((0, td), (1, ta)):
            at = int(o["huff_at"][2 * cls + tid])
            bits = data[at:at + 16]
            if huffman_table(bits, data[at + 16:at + 16 + sum(bits)]).tobytes() != r.huffman[(cls, tid)].tobytes():
                return "Huffman table"
    for c in range(r.ncomp, 3):
        if o["tq"][c] or o["td"][c] or o["ta"][c]:
            return "ids of a component the file does not have"
    return None


def intervals_of(data, first, end):
    """int32 [n, 2] restart intervals of the entropy-coded bytes data[first:end], by the local marker test"""
    arr = np.frombuffer(data, np.uint8, end - first + 1, first)   # one byte more: the FF of EOI
    at = np.flatnonzero((arr[:-1] == 0xFF) & (arr[1:] != 0) & (arr[1:] != 0xFF))
    iv = np.empty((len(at) + 1, 2), np.int32)
    iv[0, 0], iv[-1, 1] = 0, end - first
    iv[1:, 0], iv[:-1, 1] = at + 2, at
    return iv


def host_fill(datas, info, lay):
    """What ``hawq_jpeg_front_fill`` and the upload of the head leave in the blob: a numpy model from the info records alone"""
    from hawq_amd.jpeg import huffman_table
    blob = np.zeros(lay.nbytes, np.uint8)
    blob[:lay.head.size] = lay.head

    def put(off, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        blob[off:off + raw.size] = raw

    for pl in lay.place:
        data, o = datas[pl["file"]], info[pl["file"]]
        for c in range(int(o["ncomp"])):
            if pl["qt_off"][c]:
                put(pl["qt_off"][c], np.frombuffer(data, np.uint8, 64, int(o["qt_at"][o["tq"][c]])).astype(np.uint16))
            for cls, field, ids in ((0, "dc_off", "td"), (1, "ac_off", "ta")):
                if pl[field][c]:
                    at = int(o["huff_at"][2 * cls + o[ids][c]])
                    bits = data[at:at + 16]
                    put(pl[field][c], huffman_table(bits, data[at + 16:at + 16 + sum(bits)]))
        put(pl["interval_off"], intervals_of(data, int(o["scan_first"]), int(o["scan_end"])))
        put(pl["stream_off"], np.frombuffer(data, np.uint8, int(o["scan_end"] - o["scan_first"]), int(o["scan_first"])))
    return blob
