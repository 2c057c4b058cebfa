"""A Python model of self-synchronising JPEG entropy decoding on raw byte positions, independent of the HIP code.

One restart interval of L stream bytes is cut into n = ceil(L / S) sub-sequences of S raw bytes.  A state is (byte, bit, u, k): the next
unread bit is bit ``bit`` of the data byte at raw offset ``byte`` of the interval (never the 00 of FF 00), the next symbol belongs to
block ``u`` of the MCU and, for k > 0, goes on at coefficient k.  A symbol (Huffman code + extra bits) belongs to the sub-sequence its
first bit lies in.  Lane i guesses (i * S behind a stuffed 00, 0, 0, 0), decodes to the first symbol at or behind (i + 1) * S and keeps
its end state, or None after a decode error (a wrong guess, or damage); then, round after round, a lane whose predecessor has an end
state that differs from the start it last used decodes again from it, until nobody changes.  A predecessor without an end changes
nothing: the lanes behind a real error keep their guesses, and only the chain from lane 0 up to the first lane without an end is true.
``rounds`` counts the decode passes: the speculation is pass 1, so 1 <= rounds <= n.

``Interval`` takes the structure of a file from ``hawq_amd.jpeg.parse_jpeg`` only.  ``coefficients(rec, S)`` has the format of
``tests.jpeg_model.coefficients``.
"""
import numpy as np

from tests.jpeg_model import NATURAL, _extend


def _lut(table):
    """16-bit prefix -> (code length or 0, value) of one hawq_jpeg_huff record"""
    length, value = np.zeros(1 << 16, np.int64), np.zeros(1 << 16, np.int64)
    mincode, maxcode, valptr, huffval = (table[k][0] for k in ("mincode", "maxcode", "valptr", "huffval"))
    for l in range(1, 17):
        for code in range(int(mincode[l]), int(maxcode[l]) + 1) if maxcode[l] >= 0 else ():
            lo, hi = code << (16 - l), (code + 1) << (16 - l)
            length[lo:hi], value[lo:hi] = l, int(huffval[valptr[l] + code - mincode[l]])
    return length.tolist(), value.tolist()


class Interval:
    """Restart interval ``index`` of a parsed file, cut into sub-sequences of ``sub_bytes``."""

    def __init__(self, rec, index, sub_bytes):
        first, last = (int(v) for v in rec.intervals[index])
        raw = rec.data[rec.scan[0] + first:rec.scan[0] + last]
        self.raw, self.S, self.L = raw, sub_bytes, len(raw)
        self.n = -(-self.L // sub_bytes)
        # data bytes and where each one lies; behind the last one: where the next would lie
        data, where, at = [], [], 0
        while at < len(raw):
            c = raw[at]
            if c == 0xFF:
                if at + 1 >= len(raw) or raw[at + 1] != 0:
                    break   # a marker, fill bytes or the end: nothing this model has to read
                data.append(c), where.append(at)
                at += 2
            else:
                data.append(c), where.append(at)
                at += 1
        self.where = where + [at]
        self.index_of = {p: i for i, p in enumerate(self.where)}
        self.nbits = 8 * len(data)
        padded = data + [0, 0, 0, 0]
        self.window = [(padded[i] << 24) | (padded[i + 1] << 16) | (padded[i + 2] << 8) | padded[i + 3] for i in range(len(data) + 1)]
        self.bpm = 1 if rec.ncomp == 1 else rec.hs * rec.vs + 2
        luma = 1 if rec.ncomp == 1 else rec.hs * rec.vs
        self.comp = [0 if u < luma else u - luma + 1 for u in range(self.bpm)]
        self.luts = [(_lut(rec.huffman[(0, td)]), _lut(rec.huffman[(1, ta)])) for (_, _, _, _, td, ta) in rec.components]
        mcus = rec.mcus_x * rec.mcus_y
        per = rec.restart or mcus
        self.mcu0 = index * per
        self.total = (min((index + 1) * per, mcus) - self.mcu0) * self.bpm

    def guess(self, i):
        at = i * self.S
        if i > 0 and self.raw[at] == 0 and self.raw[at - 1] == 0xFF:
            at += 1
        return (at, 0, 0, 0)

    def limit(self, i):
        return (i + 1) * self.S if i + 1 < self.n else 1 << 62

    def _take(self, q, n):
        """n <= 16 bits at absolute data bit q -> value, or None past the data"""
        if q + n > self.nbits:
            return None
        return (self.window[q >> 3] >> (32 - (q & 7) - n)) & ((1 << n) - 1)

    def lane(self, start, limit, emit=None, stop_after=None):
        """Decode the symbols that start in [start, limit).  -> (end state or None after an error, blocks ended, DC sums per component).
        ``emit(kind, component, k, value)`` per symbol with kind "dc" / "ac" / "end"; ``stop_after``: blocks after which to stop."""
        if start is None or start[0] not in self.index_of:
            return None, 0, [0, 0, 0]
        at, bit, u, k = start
        q = 8 * self.index_of[at] + bit
        blocks, sums = 0, [0, 0, 0]
        while self.where[q >> 3] < limit:
            c = self.comp[u]
            length, value = self.luts[c][0 if k == 0 else 1]
            look = (self.window[q >> 3] >> (16 - (q & 7))) & 0xFFFF if q < self.nbits else 0
            if q + 16 > self.nbits:   # zero bits behind the last one
                keep = max(self.nbits - q, 0)
                look &= ~((1 << (16 - keep)) - 1) & 0xFFFF
            l = length[look]
            if l == 0 or q + l > self.nbits:
                return None, blocks, sums
            sym = value[look]
            q += l
            if k == 0:
                if sym > 15:
                    return None, blocks, sums
                v = self._take(q, sym)
                if v is None:
                    return None, blocks, sums
                q += sym
                diff = _extend(v, sym)
                sums[c] += diff
                if emit:
                    emit("dc", c, 0, diff)
                k = 1
                continue
            r, s = sym >> 4, sym & 15
            if s == 0:
                k = 64 if r != 15 else k + 16
            else:
                k += r
                if k > 63:
                    return None, blocks, sums
                v = self._take(q, s)
                if v is None:
                    return None, blocks, sums
                q += s
                if emit:
                    emit("ac", c, k, _extend(v, s))
                k += 1
            if k >= 64:
                k, u = 0, (u + 1) % self.bpm
                blocks += 1
                if emit:
                    emit("end", c, 0, 0)
                if stop_after is not None and blocks >= stop_after:
                    break
        return (self.where[q >> 3], q & 7, u, k), blocks, sums

    def synchronise(self):
        """-> (starts, results, rounds, decodes): the fixed point, what each lane's last decode gave, decode passes, lane decodes in all"""
        n = self.n
        starts = [self.guess(i) for i in range(n)]
        results = [self.lane(starts[i], self.limit(i)) for i in range(n)]
        rounds, decodes = 1, n
        for _ in range(1, n):
            changed = [i for i in range(1, n) if results[i - 1][0] is not None and results[i - 1][0] != starts[i]]
            if not changed:
                break
            for i in changed:   # all of them read the ends of the round before
                starts[i] = results[i - 1][0]
            for i in changed:
                results[i] = self.lane(starts[i], self.limit(i))
            rounds += 1
            decodes += len(changed)
        return starts, results, rounds, decodes


def coefficients(rec, sub_bytes, report=None):
    """The fixed point's coefficients per component: int16 [block rows, block columns, 64], natural order.  ``report``: a dict that
    receives per interval n, rounds, decodes and the true start states."""
    comps = [np.zeros((rec.mcus_y * v, rec.mcus_x * h, 64), np.int16) for (_, h, v, _, _, _) in rec.components]
    for index in range(len(rec.intervals)):
        iv = Interval(rec, index, sub_bytes)
        starts, results, rounds, decodes = iv.synchronise()
        if report is not None:
            report.setdefault("intervals", []).append({"n": iv.n, "rounds": rounds, "decodes": decodes, "starts": starts, "L": iv.L, "interval": iv})
        ordinal, pred = 0, [0, 0, 0]
        for i in range(iv.n):   # the exclusive scan, lane after lane
            if (i > 0 and results[i - 1][0] is None) or ordinal >= iv.total:   # behind an error nothing is true
                break
            state = {"ordinal": ordinal, "pred": list(pred), "blk": None}

            def emit(kind, c, k, value, state=state):
                if state["blk"] is None:
                    m, u = divmod(state["ordinal"], iv.bpm)
                    my, mx = divmod(iv.mcu0 + m, rec.mcus_x)
                    _, h, v, _, _, _ = rec.components[c]
                    i_, j_ = (u % h, u // h) if c == 0 else (0, 0)
                    state["blk"] = comps[c][my * v + j_, mx * h + i_]
                if kind == "dc":
                    state["pred"][c] += value
                    state["blk"][0] = np.int16(((state["pred"][c] + 0x8000) & 0xFFFF) - 0x8000)
                elif kind == "ac":
                    state["blk"][NATURAL[k]] = value
                else:
                    state["ordinal"] += 1
                    state["blk"] = None

            iv.lane(starts[i], iv.limit(i), emit, stop_after=iv.total - ordinal)
            ordinal += results[i][1]
            pred = [p + s for p, s in zip(pred, results[i][2])]
    return comps


def summary(data, sub_bytes):
    """What tests/golden/make_jpeg_sync_cases.py records of one file at ``sub_bytes``: per interval n and rounds, and the conditions the
    fixture set has to contain."""
    from hawq_amd.jpeg import parse_jpeg
    rec = parse_jpeg(data)
    report = {}
    coefficients(rec, sub_bytes, report)
    out = {"n": [], "rounds": [], "decodes": [], "boundary_on_stuffed_zero": False, "length_no_multiple": False, "start_inside_block": False,
           "start_in_chroma": False, "bytes_behind_last_block": False}
    for r in report["intervals"]:
        iv = r["interval"]
        out["n"].append(r["n"]), out["rounds"].append(r["rounds"]), out["decodes"].append(r["decodes"])
        out["boundary_on_stuffed_zero"] |= any(iv.guess(i)[0] != i * sub_bytes for i in range(1, iv.n))
        out["length_no_multiple"] |= r["L"] % sub_bytes != 0
        true = r["starts"][1:]
        out["start_inside_block"] |= any(s[3] > 0 for s in true)
        out["start_in_chroma"] |= any(iv.comp[s[2]] > 0 for s in true)
        # where the last block ends: decode everything from the start as one lane
        end, blocks, _ = iv.lane(iv.guess(0), 1 << 62, stop_after=iv.total)
        assert blocks == iv.total and end is not None
        behind = end[0] + (1 if end[1] else 0)   # the padding bits of a started byte belong to the last block's byte
        if end[1] and iv.raw[end[0]] == 0xFF:
            behind += 1
        out["bytes_behind_last_block"] |= behind < iv.L
    return out


def cases():
    """(accepted {name: (file bytes, Pillow's RGB)}, conditions) of tests/golden/jpeg_sync_cases.npz"""
    import json

    from tests import helpers as H
    z = H.load("jpeg_sync_cases.npz")
    return {str(n): (z["jpeg_" + str(n)].tobytes(), z["rgb_" + str(n)]) for n in z["names"]}, json.loads(str(z["conditions"]))
