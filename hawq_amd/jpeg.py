"""Batched JPEG decoding on the MI355X (DESIGN.md "Device JPEG decode"): file bytes -> uint8 HWC RGB tensors on the device, byte for
byte what ``image.decode_image`` (Pillow: libjpeg-turbo, ISLOW IDCT, fancy upsampling) gives on the host.

Host side, pure Python / numpy, one of each:
- one marker walker (``_parse``) reads a file once, front to back, and refuses (``UnsupportedJpeg``) whatever the device path does not
  take.  ``parse_jpeg`` gives a ``JpegRecord`` for a baseline file and, with ``progressive=True``, a ``JpegProgRecord`` with the list of
  scans for a progressive one (SOF2): the file is baseline until its frame header says otherwise, and only what the two
  kinds do differently at an SOS is written per kind.
- one layout of the baseline blob (``_baseline_layout``: descriptors and the offset of every table, interval list and stream, ``struct
  hawq_jpeg_*`` of include/hawq_mi355.h) and two fillers: ``plan_jpeg_batch`` copies the bytes of baseline records there on the host,
  with ``sync`` also the job table of ``entropy="sync"`` (many lanes per long restart interval) behind them;
  ``hawq_jpeg_front_fill`` writes them on the device (below).  ``plan_jpeg_prog_batch`` packs progressive records with the level of
  every scan into a blob of its own format; one blob writer (``_Blob``) and one plan (``_Plan``) serve both planners.
- one launch (``_launch``) plans into a pinned staging buffer, has the library check the blob, uploads it in one copy and runs
  ``hawq_jpeg_decode_batch`` / ``_sync`` / ``_prog`` (entropy decode -> IDCT -> upsampling + colour) into the caller's output; its tail
  (``_decode``: buffers, entry point, the call) is the device front end's as well.
- one index of resume points (``ResumeIndex``, ``build_resume_index``): the states in which the serial decoder starts a
  unit, recorded once per file by the library on the host; both planners place them as a segment table behind the blob they write
  anyway, and ``_launch`` runs ``hawq_jpeg_decode_batch_resume`` / ``_prog_resume`` on it, one wave per segment of a restart interval.
- one device front end (``_front_scan``, ``front_layout``, ``_front_launch``) beside the host one, opt-in: the raw files
  go up, the library walks the headers, checks the restart markers and writes the baseline blob on the device with the walker of
  csrc/jpeg_front.h; what it defers goes through ``parse_jpeg`` as ever.
- the same for progressive files (``_front_scan_prog``, ``front_prog_layout``, ``_front_prog_fill``), opt-in with
  ``progressive="device"``: one layout of the progressive blob (``_prog_layout``) with the same two fillers, ``plan_jpeg_prog_batch`` on the
  host and ``hawq_jpeg_front_fill_prog`` on the device, from the scan records of the walker of csrc/jpeg_front_prog.h.
- one option for reduced sizes (``draft_scale``, ``check_draft``, ``_plane_bytes``): ``draft=(w, h)`` gives every file the
  scale Pillow's draft mode gives it, the planners and the layout write it into the descriptor and size planes and output by it, and
  stages 2 and 3 of every entry point above produce the reduced image with the library's 4x4 / 2x2 / 1x1 inverse DCTs.
``decode_jpeg_batch`` allocates the output, launches the progressive and the baseline files of a batch and hands every refused or failed
image to the host decoder, with the reason.  ``image.folder_loader(device_decode=True)`` feeds the result to ``preprocess_batch_fused``
in place.
"""
from __future__ import annotations

import bisect
import contextlib
import ctypes as C
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib

MAX_SIDE = 8192
HUFF_BYTES = C.sizeof(_lib.JpegHuff)
_HUFF = np.dtype(_lib.JpegHuff)
_DESC = np.dtype(_lib.JpegDesc)
_HDR = np.dtype(_lib.JpegBatchHdr)
_JOB = np.dtype(_lib.JpegSyncJob)
_PHDR = np.dtype(_lib.JpegProgHdr)
_SCAN = np.dtype(_lib.JpegScan)
_SEG = np.dtype(_lib.JpegResumeSeg)
_FINFO = np.dtype(_lib.JpegFrontInfo)
_FPLACE = np.dtype(_lib.JpegFrontPlace)
_FSCAN = np.dtype(_lib.JpegFrontScanRec)
_FSPLACE = np.dtype(_lib.JpegFrontScanPlace)
MAX_SCANS = 64   # HAWQ_JPEG_PROG_MAX_SCANS
SYNC_SUB_MIN, SYNC_SUB_MAX = 16, 4096   # HAWQ_JPEG_SYNC_SUB_MIN / _MAX
SYNC_JOB_HDR_BYTES, SYNC_SUB_RECORD_BYTES = 16, C.sizeof(_lib.JpegSyncSub)
# entropy="sync" defaults: the fastest row of profiles/jpeg_sync.md on files without restart markers that leaves files with them alone
SUB_BYTES = 32
MIN_SYNC_BYTES = 4096
# resume points: the fastest row of profiles/jpeg_resume.md on progressive files without restart markers that leaves files with them alone
RESUME_EVERY = 512
STATUS_NAMES = {1: "ran out of bytes", 2: "code not in table", 3: "coefficient index past 63", 4: "unexpected marker"}


class UnsupportedJpeg(ValueError):
    """The device decoder does not take this file; ``reason`` says why (the host decoder takes it instead)."""

    def __init__(self, reason: str):
        super().__init__(reason)
        self.reason = reason


class JpegRecord:
    """What ``parse_jpeg`` returns.
    ``width`` ``height``; ``components``: tuple of (id, h, v, quantisation table id, DC table id, AC table id), one or three;
    ``hs`` ``vs``: luma sampling; ``mcus_x`` ``mcus_y``; ``restart``: MCUs per restart interval (0: none);
    ``qtables``: {id: uint16 [64] in zig-zag order, as stored}; ``huffman``: {(class, id): one ``_lib.JpegHuff`` record (numpy)};
    ``scan``: (first byte, one past the last) of the entropy-coded segment in ``data``;
    ``intervals``: int32 [n, 2], first byte and one past the last of each restart interval, relative to ``scan[0]``."""
    __slots__ = ("data", "width", "height", "components", "hs", "vs", "mcus_x", "mcus_y", "restart", "qtables", "huffman", "scan", "intervals")

    @property
    def ncomp(self):
        return len(self.components)

    @property
    def blocks(self):
        return self.mcus_x * self.mcus_y * (1 if self.ncomp == 1 else self.hs * self.vs + 2)


class JpegScan:
    """One scan of a progressive file.  ``comps``: indices into the record's ``components`` (one, or all of them in order); ``ss`` ``se``
    ``ah`` ``al``; ``dc``: the DC table (``_lib.JpegHuff`` record) in force at the SOS per component of the scan when it is a first DC
    scan, ``ac``: the AC table when ``ss > 0``, else None; ``restart``: the restart interval in force, in the scan's units (MCUs of an
    interleaved scan, blocks of the component's own grid otherwise); ``units``: how many there are; ``scan``: (first byte, one past the
    last) of the entropy-coded segment in the file; ``intervals``: int32 [n, 2] relative to ``scan[0]``."""
    __slots__ = ("comps", "ss", "se", "ah", "al", "dc", "ac", "restart", "units", "scan", "intervals")


class JpegProgRecord:
    """What ``parse_jpeg(data, progressive=True)`` returns for a progressive file: the frame fields of ``JpegRecord`` (the Huffman table
    ids of ``components`` are None: they belong to the scans) and ``scans``, the list of ``JpegScan`` in file order."""
    __slots__ = ("data", "width", "height", "components", "hs", "vs", "mcus_x", "mcus_y", "qtables", "scans")
    ncomp = JpegRecord.ncomp
    blocks = JpegRecord.blocks

    def own_grid(self, c):
        """(blocks across, blocks down) of component ``c`` in a scan of its own: what its samples need, not the MCU-padded grid."""
        _, h, v = self.components[c][:3]
        cw, ch = -(-self.width * h // self.hs), -(-self.height * v // self.vs)   # samples
        return -(-cw // 8), -(-ch // 8)


def scan_levels(scans):
    """level(scan) = 1 + the largest level of the earlier scans that share a (component, coefficient) with it, 1 without one."""
    last, levels = np.zeros((3, 64), np.int32), []   # per (component, coefficient): the level of the last scan that covered it
    for s in scans:
        cells = last[s.comps[0]:s.comps[-1] + 1, s.ss:s.se + 1]
        levels.append(int(cells.max()) + 1)
        cells[:] = levels[-1]
    return levels


def huffman_table(bits, values):
    """BITS (16 counts) + HUFFVAL -> one ``_lib.JpegHuff`` record: canonical mincode / maxcode / valptr per code length (T.81 F.2.2.3)."""
    t = np.zeros(1, _HUFF)
    mincode, maxcode, valptr = t["mincode"][0], t["maxcode"][0], t["valptr"][0]
    maxcode[:] = -1
    code = k = 0
    for length in range(1, 17):
        n = int(bits[length - 1])
        if n:
            valptr[length], mincode[length] = k, code
            code, k = code + n, k + n
            maxcode[length] = code - 1
            if code > (1 << length):
                raise UnsupportedJpeg("bad Huffman table")
        code <<= 1
    if k == 0 or k > 256 or k != len(values):
        raise UnsupportedJpeg("bad Huffman table")
    t["huffval"][0][:k] = np.frombuffer(bytes(values), np.uint8)
    return t


# ------------------------------------------------------------------------------------------------------------------ the marker walker
_SOF0, _SOF2, _DHT, _DQT, _DRI, _DNL, _SOS, _EOI, _ADOBE, _COM = 0xC0, 0xC2, 0xC4, 0xDB, 0xDD, 0xDC, 0xDA, 0xD9, 0xEE, 0xFE
_SOF_HUFFMAN = (_SOF0, 0xC1, _SOF2, 0xC3, 0xC5, 0xC6, 0xC7)
_SOF_ARITHMETIC = (0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF)
_SOF_REASON = {0xC1: "extended sequential (SOF1)", _SOF2: "progressive (SOF2)"}


def _frame_header(seg):
    """An SOF segment -> (height, width, [(component id, h, v, quantisation table id)])"""
    bad = UnsupportedJpeg("bad frame header")
    if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
        raise bad
    if seg[0] != 8:
        raise UnsupportedJpeg("sample precision not 8")
    height, width = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
    if height == 0:
        raise UnsupportedJpeg("DNL (height in the scan)")
    if width == 0:
        raise bad
    if seg[5] == 4:
        raise UnsupportedJpeg("four components")
    if seg[5] not in (1, 3):
        raise UnsupportedJpeg("component count")
    return height, width, [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])]


def _huffman_tables(seg, limit, into):
    """A DHT segment into ``into``: {(class, id): record}; ``limit``: the largest table id the frame kind takes"""
    at = 0
    while at < len(seg):
        if at + 17 > len(seg):
            raise UnsupportedJpeg("bad Huffman table")
        tc, th = seg[at] >> 4, seg[at] & 15
        bits = seg[at + 1:at + 17]
        count = sum(bits)
        if tc > 1 or at + 17 + count > len(seg):
            raise UnsupportedJpeg("bad Huffman table")
        if th > limit:
            raise UnsupportedJpeg("Huffman table id above %d" % limit)
        into[(tc, th)] = huffman_table(bits, seg[at + 17:at + 17 + count])
        at += 17 + count


def _quantisation_tables(seg, into):
    """A DQT segment into ``into``: {id: uint16 [64]}"""
    at = 0
    while at < len(seg):
        pq, tq = seg[at] >> 4, seg[at] & 15
        if pq != 0:
            raise UnsupportedJpeg("16-bit quantisation table")
        if tq > 3 or at + 65 > len(seg):
            raise UnsupportedJpeg("bad quantisation table")
        into[tq] = np.frombuffer(seg[at + 1:at + 65], np.uint8).astype(np.uint16)
        at += 65


def _accept_frame(rec, comps):
    """The frame both kinds of file must have: component ids, sampling, sizes.  ``comps``: (id, h, v, quantisation table id, DC table
    id, AC table id) per component, the last two None in a progressive record.  Fills the geometry of ``rec``."""
    if len(comps) == 3:
        if [c[0] for c in comps] != [1, 2, 3]:
            raise UnsupportedJpeg("component ids not 1, 2, 3")
        if (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            raise UnsupportedJpeg("sampling factors")
    elif (comps[0][1], comps[0][2]) != (1, 1):
        raise UnsupportedJpeg("sampling factors")
    if rec.width > MAX_SIDE or rec.height > MAX_SIDE:
        raise UnsupportedJpeg("a side above 8192")
    rec.components, rec.hs, rec.vs = tuple(comps), comps[0][1], comps[0][2]
    rec.mcus_x, rec.mcus_y = -(-rec.width // (8 * rec.hs)), -(-rec.height // (8 * rec.vs))


class _Markers:
    """Every FF xx of a file with xx neither stuffing (00) nor fill (FF): where (``at``), which (``code``), and the indices of those
    that are no RSTn (``ends``): one of these ends an entropy-coded segment."""

    def __init__(self, data):
        arr = np.frombuffer(data, np.uint8)
        ff = np.flatnonzero(arr[:-1] == 0xFF)
        nxt = arr[ff + 1]
        keep = (nxt != 0) & (nxt != 0xFF)
        self.at, self.code = ff[keep], nxt[keep]
        self.at_list, self.ends = self.at.tolist(), np.flatnonzero((self.code & 0xF8) != 0xD0).tolist()

    def entropy_segment(self, start, units, restart, last=False):
        """The entropy-coded segment from ``start`` -> (end: the first marker that is no RSTn, int32 [n, 2] restart intervals relative to
        ``start``), its RSTn markers complete and in order for ``units`` units at ``restart`` per interval.  ``last``: nothing but EOI
        may end it."""
        first = bisect.bisect_left(self.at_list, start)
        k = bisect.bisect_left(self.ends, first)
        if k == len(self.ends):
            raise UnsupportedJpeg("truncated scan")
        stop = self.ends[k]
        end = self.at_list[stop]
        if last and self.code[stop] != _EOI:
            raise UnsupportedJpeg("DNL" if self.code[stop] == _DNL else "several scans")
        expected = -(-units // restart) - 1 if restart else 0
        if stop - first != expected or (expected and ((self.code[first:stop] - np.arange(expected)) & 7).any()):   # RSTn counts modulo 8
            raise UnsupportedJpeg("restart markers missing or out of order")
        intervals = np.empty((expected + 1, 2), np.int32)
        intervals[0, 0], intervals[-1, 1] = 0, end - start
        if expected:
            rst = self.at[first:stop] - start   # the RSTn markers inside
            intervals[1:, 0], intervals[:-1, 1] = rst + 2, rst
        return end, intervals


def _parse(data, progressive, prog):
    """The one walk over a file.  ``progressive``: SOF2 is taken; ``prog``: the file counts as progressive (from the start for
    ``parse_progressive``, else from its SOF2 on): Huffman table ids up to 3, and an SOS adds a scan instead of ending the walk."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise UnsupportedJpeg("not a JPEG")
    qtables, huffman, scans = {}, {}, []
    restart, frame, adobe, pos = 0, None, False, 2

    def need(upto):
        if upto > n:
            raise UnsupportedJpeg("truncated scan" if scans else "truncated header")

    while True:
        need(pos + 2)
        if data[pos] != 0xFF:
            raise UnsupportedJpeg("marker expected")
        while data[pos + 1] == 0xFF:   # fill bytes
            pos += 1
            need(pos + 2)
        marker = data[pos + 1]
        pos += 2
        if marker == _EOI:
            if not scans:
                raise UnsupportedJpeg("no scan")
            break
        if scans and not (marker in (_DHT, _DRI, _COM, _SOS) or 0xE0 <= marker <= 0xEF):
            raise UnsupportedJpeg("DNL" if marker == _DNL else "DQT between scans" if marker == _DQT else "marker %02X between scans" % marker)
        if marker == 0xD8 or marker == 0x01 or 0xD0 <= marker <= 0xD7:
            continue
        need(pos + 2)
        length = (data[pos] << 8) | data[pos + 1]
        if length < 2:
            raise UnsupportedJpeg("bad segment length")
        need(pos + length)
        seg = data[pos + 2:pos + length]
        pos += length
        if marker == _SOF2 and progressive and not prog:   # baseline until here
            if frame is not None:
                raise UnsupportedJpeg("several frames")
            prog = True
        if marker == (_SOF2 if prog else _SOF0):
            if frame is not None:
                raise UnsupportedJpeg("several frames")
            frame = _frame_header(seg)
        elif marker in _SOF_ARITHMETIC:
            raise UnsupportedJpeg("arithmetic coding")
        elif marker in _SOF_HUFFMAN:
            raise UnsupportedJpeg("several frames" if prog else _SOF_REASON.get(marker, "SOF%d" % (marker - _SOF0)))
        elif marker == _DHT:
            _huffman_tables(seg, 3 if prog else 1, huffman)
        elif marker == _DQT:
            _quantisation_tables(seg, qtables)
        elif marker == _DRI:
            if len(seg) != 2:
                raise UnsupportedJpeg("bad restart interval")
            restart = (seg[0] << 8) | seg[1]
        elif marker == _DNL:
            raise UnsupportedJpeg("DNL")
        elif marker == _ADOBE:
            adobe = adobe or seg[:5] == b"Adobe"
        elif marker == _SOS:
            if not scans:   # the first SOS, of a baseline file the only one
                if frame is None:
                    raise UnsupportedJpeg("scan before the frame header")
                if adobe:
                    raise UnsupportedJpeg("Adobe marker")
                rec = JpegProgRecord() if prog else JpegRecord()
                rec.data, rec.qtables = data, qtables
                rec.height, rec.width, frame = frame
                markers = _Markers(data)
            if not prog:
                _accept_frame(rec, _baseline_scan_header(seg, frame, qtables, huffman))
                rec.huffman, rec.restart = huffman, restart
                end, rec.intervals = markers.entropy_segment(pos, rec.mcus_x * rec.mcus_y, restart, last=True)
                rec.scan = (pos, end)
                return rec
            if not scans:
                if any(tq not in qtables for _, _, _, tq in frame):
                    raise UnsupportedJpeg("missing table")
                _accept_frame(rec, [c + (None, None) for c in frame])
                rec.scans = scans
                state = np.full((3, 64), -1, np.int32)   # per (component, coefficient): the Al reached, -1 before its first scan
            if len(scans) == MAX_SCANS:
                raise UnsupportedJpeg("too many scans")
            s = _progressive_scan_header(rec, seg, huffman, state)
            s.restart = restart
            end, s.intervals = markers.entropy_segment(pos, s.units, restart)
            s.scan = (pos, end)
            scans.append(s)
            pos = end
    if state[:len(rec.components)].any():   # something never coded, or not down to Al = 0
        raise UnsupportedJpeg("progression")
    return rec


def parse_jpeg(data, progressive=False):
    """Headers of one JPEG file (bytes) -> ``JpegRecord``, or ``UnsupportedJpeg(reason)`` for anything outside the device path:
    baseline SOF0 with 8-bit samples and tables, one interleaved scan of all components, Huffman table ids 0 and 1, three components
    with ids 1, 2, 3, luma 1x1 / 2x1 / 2x2 and chroma 1x1 without an Adobe marker, or one 1x1 component, restart markers complete
    and in order, both sides at most 8192.  ``progressive``: a progressive Huffman file (SOF2) with the same components, sampling and
    sizes, whose scans form a legal and complete progression (``parse_progressive``), gives a ``JpegProgRecord`` instead of the refusal
    "progressive (SOF2)"; baseline files parse as without it, and Huffman table ids 2 and 3 are taken from the SOF2 marker on."""
    return _parse(data, progressive, False)


def parse_progressive(data) -> JpegProgRecord:
    """Headers and scans of one progressive Huffman JPEG -> ``JpegProgRecord``, or ``UnsupportedJpeg(reason)``.  Accepted: SOF2 with 8-bit
    samples and tables, components and sampling as in the baseline path, no Adobe marker, sides at most 8192; 1 to 64 scans, each of all
    components or of one (AC scans: of one), Ss <= Se <= 63 with Se = 0 when Ss = 0, Al <= 13, Ah = 0 or Al + 1, Huffman table ids 0..3;
    per (component, coefficient) the first scan has Ah = 0, each later one Ah = the previous Al, the DC comes before any AC, and after
    the last scan everything has reached Al = 0 ("progression" otherwise: the library smooths an incomplete file, the device does not);
    between scans only DHT / DRI / COM / APPn segments; restart markers complete and in order per scan; EOI behind the last scan."""
    return _parse(data, True, True)


def _baseline_scan_header(seg, frame, qtables, huffman):
    """The one SOS segment of a baseline file -> its components as (id, h, v, quantisation table id, DC table id, AC table id)"""
    if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
        raise UnsupportedJpeg("bad scan header")
    if seg[0] != len(frame):
        raise UnsupportedJpeg("several scans")
    if seg[-3] != 0 or seg[-2] != 63 or seg[-1] != 0:
        raise UnsupportedJpeg("spectral selection or successive approximation")
    comps = []
    for i, (cid, h, v, tq) in enumerate(frame):
        if seg[1 + 2 * i] != cid:
            raise UnsupportedJpeg("scan component order")
        td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
        if td > 1 or ta > 1:
            raise UnsupportedJpeg("Huffman table id above 1")
        if tq not in qtables or (0, td) not in huffman or (1, ta) not in huffman:
            raise UnsupportedJpeg("missing table")
        comps.append((cid, h, v, tq, td, ta))
    return comps


def _progressive_scan_header(rec, seg, huffman, state) -> JpegScan:
    """One SOS segment of a progressive file: limits, tables in force, and its step in the progression (``state`` is advanced)"""
    ncomp = len(rec.components)
    if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
        raise UnsupportedJpeg("bad scan header")
    ns = seg[0]
    ids = [seg[1 + 2 * i] for i in range(ns)]
    frame_ids = [c[0] for c in rec.components]
    if ns == ncomp:
        if ids != frame_ids:
            raise UnsupportedJpeg("scan component order")
        comps = tuple(range(ncomp))
    elif ns == 1:
        if ids[0] not in frame_ids:
            raise UnsupportedJpeg("scan component order")
        comps = (frame_ids.index(ids[0]),)
    elif ns == 2 and ncomp == 3:
        raise UnsupportedJpeg("scan of two components")
    else:
        raise UnsupportedJpeg("bad scan header")
    s = JpegScan()
    s.comps, s.ss, s.se, s.ah, s.al = comps, seg[-3], seg[-2], seg[-1] >> 4, seg[-1] & 15
    if s.ss > s.se or s.se > 63 or (s.ss == 0 and s.se != 0):
        raise UnsupportedJpeg("spectral selection")
    if s.ss > 0 and ns != 1:
        raise UnsupportedJpeg("AC scan of several components")
    if s.al > 13 or s.ah not in (0, s.al + 1):
        raise UnsupportedJpeg("successive approximation")
    cells = state[comps[0]:comps[-1] + 1, s.ss:s.se + 1]
    # a first scan (Ah = 0) of cells never coded, or a refinement of cells whose last scan stopped at Al = Ah; the DC before any AC
    if np.any(cells != (s.ah if s.ah else -1)) or (s.ss > 0 and state[comps[0], 0] < 0):
        raise UnsupportedJpeg("progression")
    cells[:] = s.al
    s.dc = s.ac = None
    tables = [(seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(ns)]
    if any(td > 3 or ta > 3 for td, ta in tables):
        raise UnsupportedJpeg("Huffman table id above 3")
    if s.ss == 0 and s.ah == 0:
        if any((0, td) not in huffman for td, _ in tables):
            raise UnsupportedJpeg("missing table")
        s.dc = [huffman[(0, td)] for td, _ in tables]
    if s.ss > 0:
        if (1, tables[0][1]) not in huffman:
            raise UnsupportedJpeg("missing table")
        s.ac = huffman[(1, tables[0][1])]
    if ns > 1:
        s.units = rec.mcus_x * rec.mcus_y
    else:
        bw, bh = rec.own_grid(comps[0])
        s.units = bw * bh
    return s


# ------------------------------------------------------------------------------------------------------------------ the planners
def _align16(n: int) -> int:
    return (n + 15) & ~15


def check_draft(draft):
    """``draft`` of ``decode_jpeg_batch``: None, or the requested (width, height) as a pair of positive ints"""
    if draft is None:
        return None
    try:
        w, h = draft
        w, h = int(w), int(h)
    except (TypeError, ValueError):
        raise ValueError(f"draft must be None or a (width, height) pair, not {draft!r}") from None
    if w < 1 or h < 1:
        raise ValueError(f"draft sizes must be positive, not {draft!r}")
    return w, h


def draft_scales(widths, heights, draft):
    """``draft_scale`` over columns: int arrays of file sizes -> int32 array of scales (all 1 for ``draft`` None)"""
    widths, heights = np.asarray(widths, np.int64), np.asarray(heights, np.int64)
    if draft is None:
        return np.ones(widths.shape, np.int32)
    w, h = check_draft(draft)
    k = np.minimum(widths // w, heights // h)
    return np.where(k >= 8, 8, np.where(k >= 4, 4, np.where(k >= 2, 2, 1))).astype(np.int32)


def draft_scale(width, height, draft) -> int:
    """The scale Pillow's ``Image.draft("RGB", draft)`` picks for a ``width`` x ``height`` JPEG: the largest of 8, 4, 2, 1
    that is at most min(width // draft[0], height // draft[1]), 1 when that is 0 or ``draft`` is None.  The decoded image then has
    ``scaled_size`` = ceil(size / scale)."""
    if draft is None:
        return 1
    w, h = check_draft(draft)
    k = min(int(width) // w, int(height) // h)
    return 8 if k >= 8 else 4 if k >= 4 else 2 if k >= 2 else 1


def scaled_size(n, scale):
    """ceil(n / scale): a side of the reduced image (ints or arrays)"""
    return -(-n // scale)


def _plane_bytes(blocks_luma, blocks_chroma, hs, vs, scale):
    """Bytes of an image's sample planes: n x n samples per block, n = 8 // scale per side, twice that for the chroma of a 4:2:0 image
    decoded at a reduced size (jpeg_comp_n of csrc/jpeg_pixel.h); ints or arrays."""
    m = 8 // scale
    nc = np.where((hs == 2) & (vs == 2) & (m < 8), 2 * m, m)
    return blocks_luma * m * m + blocks_chroma * nc * nc


def output_layout(sizes):
    """(height, width) per image -> (offsets, total bytes) of the RGB images one after the other, each at a 16-byte aligned offset"""
    offsets, total = [], 0
    for h, w in sizes:
        offsets.append(total)
        total = _align16(total + h * w * 3)
    return offsets, total


def _blob_bytes(nbytes: int) -> int:
    """``nbytes`` as the size of a blob, whose offsets are int32"""
    if nbytes >= 1 << 31:
        raise ValueError("batch too large for one blob (2 GiB of compressed data)")
    return nbytes


class _Blob:
    """The host blob of a batch while it is laid out: the cursor ``at`` and the parts with their offsets, every one 16-byte aligned."""

    def __init__(self):
        self.at, self.parts = 0, []

    def room(self, nbytes):
        """the offset of ``nbytes`` bytes that ``put`` fills later"""
        off, self.at = self.at, _align16(self.at + nbytes)
        return off

    def put(self, off, arr):
        self.parts.append((off, np.ascontiguousarray(arr).view(np.uint8).reshape(-1)))

    def place(self, arr):
        """``arr`` behind everything so far -> its offset"""
        off = self.room(np.asarray(arr).nbytes)
        self.put(off, arr)
        return off

    def finish(self, reserve):
        """-> the uint8 array with every part in place: ``reserve(nbytes)``, or a fresh zeroed one"""
        nbytes = _blob_bytes(self.at)
        blob = np.zeros(nbytes, np.uint8) if reserve is None else reserve(nbytes)
        for off, raw in self.parts:
            blob[off:off + raw.size] = raw
        return blob


class _Plan:
    """What both planners return.  ``blob``: uint8 array (the first ``nbytes`` bytes count), ``coef_blocks`` / ``plane_bytes`` /
    ``out_bytes``: the sizes of the three device buffers the launch needs, ``out_offsets`` / ``sizes``: where each image lands in the
    output and its (height, width) as decoded: with ``draft`` the reduced ones (the scale itself is in the descriptor)."""
    __slots__ = ("blob", "nbytes", "coef_blocks", "plane_bytes", "out_bytes", "out_offsets", "sizes")
    checker = None   # the library's check of the blob

    def __init__(self):
        self.coef_blocks = self.plane_bytes = self.out_bytes = 0
        self.out_offsets, self.sizes = [], []

    def ok(self) -> bool:
        """The library's checker on the host blob (no GPU work); the reason of a refusal is in ``hawq_last_error``."""
        return bool(getattr(_lib.load(), self.checker)(self.blob.ctypes.data, self.nbytes, self.coef_blocks, self.plane_bytes, self.out_bytes))

    def finish(self, blob, reserve, out_bytes):
        self.blob, self.nbytes = blob.finish(reserve), blob.at
        if out_bytes is not None:
            self.out_bytes = int(out_bytes)
        return self


class JpegPlan(_Plan):
    """What ``plan_jpeg_batch`` returns: ``_Plan`` and ``n_waves``: restart intervals in the batch.  With ``sync``: ``sub_bytes`` /
    ``min_sync_bytes``, ``jobs_off`` / ``n_jobs``: the table of ``hawq_jpeg_sync_job`` in the blob (one per interval of at least
    ``min_sync_bytes``), ``jobs``: the same as (wave, n_sub, scratch offset) tuples, ``scratch_bytes``: the device scratch the launch
    needs."""
    __slots__ = ("n_waves", "sub_bytes", "min_sync_bytes", "jobs_off", "n_jobs", "jobs", "scratch_bytes")
    checker = "hawq_jpeg_batch_ok"

    def sync_ok(self) -> bool:
        """``hawq_jpeg_sync_ok`` on the host blob of a plan made with ``sync`` (after ``ok``; no GPU work)."""
        return bool(_lib.load().hawq_jpeg_sync_ok(self.blob.ctypes.data, self.nbytes, self.sub_bytes, self.min_sync_bytes, self.jobs_off, self.n_jobs,
                                                  self.scratch_bytes))


def _wave_list(ks, counts):
    """int32 [n, 2]: (k, j) for j in range(count), for every k of ``ks`` with its count, in order"""
    counts = np.asarray(counts, np.int64)
    waves = np.empty((int(counts.sum()), 2), np.int32)
    waves[:, 0] = np.repeat(np.asarray(ks), counts)
    waves[:, 1] = np.arange(len(waves)) - np.repeat(np.cumsum(counts) - counts, counts)
    return waves


class JpegResumePlan(JpegPlan):
    """``JpegPlan`` of a plan made with ``resume``: ``segs_off`` / ``n_segs``: the table of ``hawq_jpeg_resume_seg`` in the blob, one segment
    or more per wave, in the order of the wave list."""
    __slots__ = ("segs_off", "n_segs")

    def resume_ok(self) -> bool:
        """``hawq_jpeg_resume_ok`` on the host blob (after ``ok``; no GPU work)."""
        return bool(_lib.load().hawq_jpeg_resume_ok(self.blob.ctypes.data, self.nbytes, 0, self.segs_off, self.n_segs))


def _segment_table(first, units, points):
    """The ``hawq_jpeg_resume_seg`` table of a blob.  ``first`` / ``units``: per wave of its wave list the first byte of the interval and
    how many units it has; ``points``: int [k, 8] resume points as (wave, unit, byte, bit, eobrun, pred x 3).  Every wave gets the
    segment that starts its interval; a point starts another one."""
    n = len(first)
    rows = np.zeros((n + len(points), 8), np.int64)
    rows[:n, 0], rows[:n, 2] = np.arange(n), first
    rows[n:] = points
    rows = rows[np.lexsort((rows[:, 1], rows[:, 0]))]
    segs = np.zeros(len(rows), _SEG)
    segs["wave"], segs["unit0"], segs["byte"], segs["bit"], segs["eobrun"], segs["pred"] = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5:8]
    upto = np.asarray(units, np.int64)[np.clip(rows[:, 0], 0, n - 1)]   # a point of no wave: the checker refuses it
    same = rows[1:, 0] == rows[:-1, 0]
    upto[:-1][same] = rows[1:, 1][same]
    segs["n_units"] = upto - rows[:, 1]
    return segs


def _interval_units(units, restart, n_intervals):
    """units of each of the ``n_intervals`` restart intervals of a scan of ``units`` units"""
    if not restart:
        return np.array([units])
    return np.minimum(restart, units - restart * np.arange(n_intervals))


def _check_sync(sync):
    """(sub_bytes, min_sync_bytes) of ``entropy="sync"`` as ints, inside their ranges"""
    sub_bytes, min_sync_bytes = (int(v) for v in sync)
    if sub_bytes % 4 or not SYNC_SUB_MIN <= sub_bytes <= SYNC_SUB_MAX:
        raise ValueError(f"sub_bytes must be a multiple of 4 in {SYNC_SUB_MIN}..{SYNC_SUB_MAX}, not {sub_bytes}")
    if min_sync_bytes < 1:
        raise ValueError(f"min_sync_bytes must be at least 1, not {min_sync_bytes}")
    return sub_bytes, min_sync_bytes


def _sync_job_table(lengths, sub_bytes, min_sync_bytes):
    """The ``hawq_jpeg_sync_job`` table of a blob.  ``lengths``: stream bytes of every interval in the order of the wave list.  One job
    per interval of at least ``min_sync_bytes``, cut into sub-sequences of ``sub_bytes``, each with its slice of the scratch behind the
    job's before it -> (the table, scratch bytes)"""
    lengths = np.asarray(lengths, np.int64)
    waves = np.flatnonzero(lengths >= min_sync_bytes)
    n_sub = -(-lengths[waves] // sub_bytes)
    ends = np.cumsum(SYNC_JOB_HDR_BYTES + SYNC_SUB_RECORD_BYTES * n_sub)
    jobs = np.zeros(len(waves), _JOB)
    jobs["wave"], jobs["n_sub"], jobs["scratch_off"] = waves, n_sub, ends - (SYNC_JOB_HDR_BYTES + SYNC_SUB_RECORD_BYTES * n_sub)
    return jobs, int(ends[-1]) if len(ends) else 0


# what ``_baseline_layout`` reads of a ``hawq_jpeg_front_info``; ``tq`` ``td`` ``ta``: the quantisation, DC and AC table id per component
_COLS = _FINFO[["width", "height", "ncomp", "hs", "vs", "restart", "n_intervals", "tq", "td", "ta", "scan_first", "scan_end"]]


class FrontLayout:
    """What ``_baseline_layout`` returns.  ``head``: header | descriptors | wave list as bytes, ``place``: per image where its tables,
    intervals and stream go (the ``hawq_jpeg_front_place`` table of the fill), ``desc``: the descriptors, ``nbytes``: the blob's size
    without a job or segment table, ``n_waves`` / ``coef_blocks`` / ``plane_bytes`` / ``out_bytes`` as in ``JpegPlan``."""
    __slots__ = ("head", "place", "desc", "nbytes", "n_waves", "coef_blocks", "plane_bytes", "out_bytes")


def _geometry(lay, desc, o, out_offsets, out_bytes, scales):
    """The geometry half of the descriptors ``desc`` from the columns ``o`` (width, height, ncomp, hs, vs) and every image's share of the
    three device buffers: coefficient slab, planes, output (``out_offsets`` / ``out_bytes`` / ``scales`` as in ``_baseline_layout``);
    their sizes into ``lay``.  Both layouts begin with it."""
    for f in ("width", "height", "ncomp", "hs", "vs"):
        desc[f] = o[f]
    desc["mcus_x"], desc["mcus_y"] = -(-o["width"] // (8 * o["hs"])), -(-o["height"] // (8 * o["vs"]))
    blocks = desc["mcus_x"].astype(np.int64) * desc["mcus_y"] * np.where(o["ncomp"] == 3, o["hs"] * o["vs"] + 2, 1)
    desc["coef_block0"] = np.cumsum(blocks) - blocks
    planes, rgb = blocks * 64, 3 * o["width"].astype(np.int64) * o["height"]
    if scales is not None:
        desc["scale"] = s = np.asarray(scales, np.int64)
        luma = desc["mcus_x"].astype(np.int64) * desc["mcus_y"] * o["hs"] * o["vs"]
        planes = _plane_bytes(luma, blocks - luma, o["hs"], o["vs"], s)
        rgb = 3 * scaled_size(o["width"].astype(np.int64), s) * scaled_size(o["height"].astype(np.int64), s)
    desc["plane_off"] = np.cumsum(planes) - planes
    desc["out_off"] = np.cumsum((rgb + 15) & ~15) - ((rgb + 15) & ~15) if out_offsets is None else out_offsets
    lay.coef_blocks, lay.plane_bytes = int(blocks.sum()), int(planes.sum())
    lay.out_bytes = _align16(int(desc["out_off"][-1] + rgb[-1])) if out_bytes is None else int(out_bytes)


def _first_user(t, colour):
    """``t``: int [n, 3] table ids per component -> per component the first one with its table, 0 for the components a gray image
    (``colour`` false) does not have"""
    used = colour[:, None] | (np.arange(3) == 0)
    return np.stack((0 * t[:, 0], t[:, 1] != t[:, 0], np.where(t[:, 2] == t[:, 0], 0, np.where(t[:, 2] == t[:, 1], 1, 2))), 1) * used, used


def _baseline_layout(o, out_offsets=None, out_bytes=None, scales=None) -> FrontLayout:
    """The one place that knows the blob of ``hawq_jpeg_decode_batch``: header | descriptors | wave list | per image, per component the
    quantisation, DC and AC table it is the first to use, then intervals, then stream - every part at a 16-byte aligned offset; a
    component that shares a table takes the offset of the first one that has it.  ``o``: the columns ``_COLS`` of the images;
    ``out_offsets`` / ``out_bytes``: where each image goes in an output buffer of that size (default: one after the other, 16-byte
    aligned, and the aligned end of the last image).  ``scales``: the scale of every image (1, 2, 4, 8; None: the descriptors say 0, full
    size): planes and output take the reduced sizes.  numpy over the batch, no loop over images.  Two fillers write the bytes of the
    parts at ``place``: ``plan_jpeg_batch`` on the host, ``hawq_jpeg_front_fill`` on the device."""
    n = len(o)
    lay = FrontLayout()
    colour = o["ncomp"] == 3
    desc, place = np.zeros(n, _DESC), np.zeros(n, _FPLACE)
    for f in ("restart", "n_intervals"):
        desc[f] = o[f]
    _geometry(lay, desc, o, out_offsets, out_bytes, scales)
    desc["stream_len"] = o["scan_end"] - o["scan_first"]
    lay.n_waves = int(o["n_intervals"].sum())
    # per image the aligned sizes of its parts in blob order: (quantisation, DC, AC) x 3 components, 0 unless the component is the first
    # to use that table (``first``: per component the first one with its table; a gray image has component 0 alone), intervals, stream
    sizes, first = np.zeros((n, 11), np.int64), {}
    for k, (ids, nbytes) in enumerate((("tq", 128), ("td", HUFF_BYTES), ("ta", HUFF_BYTES))):
        first[ids], used = _first_user(o[ids], colour)
        sizes[:, k:9:3] = (first[ids] == np.arange(3)) * _align16(nbytes)
    sizes[:, 9], sizes[:, 10] = (8 * o["n_intervals"].astype(np.int64) + 15) & ~15, (desc["stream_len"].astype(np.int64) + 15) & ~15
    head = _Blob()
    hdr_off, desc_off, wave_off = head.room(_HDR.itemsize), head.room(desc.nbytes), head.room(8 * lay.n_waves)
    ends = head.at + np.cumsum(sizes.reshape(-1)).reshape(n, 11)
    offs = ends - sizes
    lay.nbytes = _blob_bytes(int(ends[-1, -1]))
    for k, (ids, field) in enumerate((("tq", "qt_off"), ("td", "dc_off"), ("ta", "ac_off"))):
        own = offs[:, k:9:3]
        place[field] = np.where(first[ids] == np.arange(3), own, 0)
        desc[field] = np.take_along_axis(own, first[ids], 1) * used
    place["file"], place["interval_off"], place["stream_off"] = np.arange(n), offs[:, 9], offs[:, 10]
    desc["interval_off"], desc["stream_off"] = offs[:, 9], offs[:, 10]
    hdr = np.array([(n, lay.n_waves, desc_off, wave_off)], _HDR)   # n_images, n_waves, desc_off, wave_off
    for off, table in ((hdr_off, hdr), (desc_off, desc), (wave_off, _wave_list(np.arange(n), o["n_intervals"]))):
        head.put(off, table)
    lay.head, lay.place, lay.desc = head.finish(None), place, desc
    return lay


def plan_jpeg_batch(records, out_offsets=None, out_bytes=None, reserve=None, sync=None, resume=None, draft=None) -> JpegPlan:
    """Pack the records of ``parse_jpeg`` into one host blob laid out by ``_baseline_layout``: the adapter from records to its columns, and
    the host filler that copies table, interval and stream bytes to the offsets it gives.  ``out_offsets`` / ``out_bytes``: where each
    image goes in an output buffer of that size (default: one after the other, 16-byte aligned).  ``reserve(nbytes)`` returns the uint8 array to write
    into (at least nbytes, 16-byte aligned; e.g. a pinned staging buffer); a fresh array without it.  ``sync`` = (sub_bytes,
    min_sync_bytes): append the job table of ``hawq_jpeg_decode_batch_sync`` behind the streams - one job per interval of at least
    ``min_sync_bytes`` bytes, cut into sub-sequences of ``sub_bytes``, with its slice of the scratch.  ``resume``: per record its resume
    points (``ResumeIndex.points``): append the segment table of ``hawq_jpeg_decode_batch_resume`` instead (a ``JpegResumePlan``).
    ``draft``: None, or the (width, height) of Pillow's draft mode: every record gets its ``draft_scale``, and planes, output and
    ``sizes`` take the reduced sizes; without it the blob is the one of a plan made before the option."""
    records = list(records)
    if not records:
        raise ValueError("empty batch")
    if sync is not None and resume is not None:
        raise ValueError("a batch is decoded with entropy='sync' or from resume points, not both")
    # a gray record repeats its one component: the layout reads the table ids of component 0 alone
    cols = [(r.width, r.height, r.ncomp, r.hs, r.vs, r.restart, len(r.intervals)) + tuple(zip(*(c[3:] for c in (r.components * 3)[:3]))) + r.scan for r in records]
    scales = None if draft is None else draft_scales([r.width for r in records], [r.height for r in records], draft)
    lay = _baseline_layout(np.array(cols, _COLS), out_offsets, out_bytes, scales)
    plan, blob = JpegPlan() if resume is None else JpegResumePlan(), _Blob()
    plan.n_waves, plan.coef_blocks, plan.plane_bytes = lay.n_waves, lay.coef_blocks, lay.plane_bytes
    plan.out_offsets, plan.sizes = lay.desc["out_off"].tolist(), [(r.height, r.width) for r in records]
    if scales is not None:
        plan.sizes = [(scaled_size(h, s), scaled_size(w, s)) for (h, w), s in zip(plan.sizes, scales.tolist())]
    blob.put(blob.room(lay.nbytes), lay.head)
    for r, qt, dc, ac, interval_off, stream_off in zip(records, *(lay.place[f].tolist() for f in ("qt_off", "dc_off", "ac_off", "interval_off", "stream_off"))):
        for c, (_, _, _, tq, td, ta) in enumerate(r.components):
            for off, table in ((qt[c], r.qtables[tq]), (dc[c], r.huffman[0, td]), (ac[c], r.huffman[1, ta])):
                if off:   # 0: an earlier component has placed it
                    blob.put(off, table)
        blob.put(interval_off, np.ascontiguousarray(r.intervals, np.int32))
        blob.put(stream_off, np.frombuffer(r.data, np.uint8, r.scan[1] - r.scan[0], r.scan[0]))
    plan.sub_bytes = plan.min_sync_bytes = plan.jobs_off = plan.n_jobs = plan.scratch_bytes = 0
    plan.jobs = []
    if sync is not None:
        sub_bytes, min_sync_bytes = _check_sync(sync)
        jobs, plan.scratch_bytes = _sync_job_table(np.concatenate([r.intervals[:, 1] - r.intervals[:, 0] for r in records]), sub_bytes, min_sync_bytes)
        plan.jobs = [tuple(j) for j in jobs.tolist()]
        plan.sub_bytes, plan.min_sync_bytes, plan.jobs_off, plan.n_jobs = sub_bytes, min_sync_bytes, blob.place(jobs), len(jobs)
    if resume is not None:
        wave0 = np.cumsum([0] + [len(r.intervals) for r in records])
        points = [np.column_stack((wave0[i] + p[:, 1], p[:, 2:])) for i, p in enumerate(resume)]
        segs = _segment_table(np.concatenate([r.intervals[:, 0] for r in records]),
                              np.concatenate([_interval_units(r.mcus_x * r.mcus_y, r.restart, len(r.intervals)) for r in records]), np.concatenate(points))
        plan.segs_off, plan.n_segs = blob.place(segs), len(segs)
    return plan.finish(blob, reserve, lay.out_bytes)


class JpegProgPlan(_Plan):
    """What ``plan_jpeg_prog_batch`` returns: ``_Plan`` and ``n_scans``; ``levels``: the level of every scan, image after image;
    ``n_levels``: the deepest, the number of entropy launches; ``n_waves``: (scan, restart interval) pairs; ``level_start``: where each
    level's waves begin in the wave list (n_levels + 1 entries); ``scan_off`` / ``level_off`` / ``wave_off`` / ``desc_off``: where the
    tables lie in the blob."""
    __slots__ = ("n_scans", "levels", "n_levels", "n_waves", "level_start", "scan_off", "level_off", "wave_off", "desc_off")
    checker = "hawq_jpeg_prog_ok"


class JpegProgResumePlan(JpegProgPlan):
    """``JpegProgPlan`` of a plan made with ``resume``: ``segs_off`` / ``n_segs`` as in ``JpegResumePlan``."""
    __slots__ = ("segs_off", "n_segs")

    def resume_ok(self) -> bool:
        return bool(_lib.load().hawq_jpeg_resume_ok(self.blob.ctypes.data, self.nbytes, 1, self.segs_off, self.n_segs))


# what ``_prog_layout`` reads of an image (of a ``hawq_jpeg_front_info``: ``n_scans`` is word 1 of ``reserved``) and of a scan: the columns
# of a ``hawq_jpeg_front_scan_rec``, where ``dc_at`` / ``ac_at`` need only tell the tables of one image apart (0: none)
_PROG_IMAGE = np.dtype([(f, np.int32) for f in ("width", "height", "ncomp", "hs", "vs")] + [("tq", np.int32, 3), ("n_scans", np.int32)])


class ProgLayout:
    """What ``_prog_layout`` returns.  ``head``: batch header | progressive header | descriptors | scan table | level list | wave lists as
    bytes, ``place``: per scan where its tables, intervals and stream go (the ``hawq_jpeg_front_scan_place`` table of the fill; ``file`` is
    the image's index in the batch), ``desc`` / ``scans`` / ``waves``: the tables in ``head``, ``nbytes``: the blob's size without a
    segment table, the rest as in ``JpegProgPlan``."""
    __slots__ = ("head", "place", "desc", "scans", "waves", "nbytes", "n_scans", "n_levels", "n_waves", "level_start", "desc_off", "scan_off", "level_off", "wave_off",
                 "coef_blocks", "plane_bytes", "out_bytes")


def _prog_layout(im, sc, out_offsets=None, out_bytes=None, scales=None) -> ProgLayout:
    """The one place that knows the blob of ``hawq_jpeg_decode_batch_prog``: batch header | progressive header | descriptors (entropy
    fields zero) | scan table | level list | wave lists, level after level | per image: the quantisation tables its components are the
    first to use, then per scan the DC tables and the AC table no earlier scan of the image has placed, its intervals, its stream -
    every part at a 16-byte aligned offset.  A table in force over several scans stands once: its key is ``dc_at`` / ``ac_at``.  ``im``:
    the columns ``_PROG_IMAGE`` of the images; ``sc``: the ``hawq_jpeg_front_scan_rec`` columns of their scans, image after image, with
    the level of every scan; ``out_offsets`` / ``out_bytes`` / ``scales`` as in ``_baseline_layout``.  numpy over the batch, no loop over
    images or scans.  Two fillers write the bytes of the parts at ``place``: ``plan_jpeg_prog_batch`` on the host,
    ``hawq_jpeg_front_fill_prog`` on the device."""
    n, n_scans = len(im), len(sc)
    lay = ProgLayout()
    desc, scans, place = np.zeros(n, _DESC), np.zeros(n_scans, _SCAN), np.zeros(n_scans, _FSPLACE)
    _geometry(lay, desc, im, out_offsets, out_bytes, scales)
    per_image = im["n_scans"].astype(np.int64)
    image, scan0 = np.repeat(np.arange(n), per_image), np.cumsum(per_image) - per_image
    levels, n_intervals = sc["level"].astype(np.int64), sc["n_intervals"].astype(np.int64)
    lay.n_scans, lay.n_levels, lay.n_waves = n_scans, int(levels.max()), int(n_intervals.sum())
    # the waves of a level: every interval of every scan of that level, in the order of the scan table
    order = np.argsort(levels, kind="stable")
    lay.waves = _wave_list(order, n_intervals[order])
    level_start = np.concatenate(([0], np.cumsum(np.bincount(levels, n_intervals, lay.n_levels + 1)[1:]))).astype(np.int32)
    lay.level_start = level_start.tolist()
    head = _Blob()
    head.room(_HDR.itemsize + _PHDR.itemsize)
    lay.desc_off, lay.scan_off, lay.level_off, lay.wave_off = head.room(desc.nbytes), head.room(scans.nbytes), head.room(level_start.nbytes), head.room(lay.waves.nbytes)
    # per image the quantisation tables; per scan the aligned sizes of its parts in blob order: DC x 3, AC (0 unless the scan is the
    # first of its image to read that table), intervals, stream
    first_q, used_q = _first_user(im["tq"], im["ncomp"] == 3)
    q_sizes = (first_q == np.arange(3)) * used_q * 128
    keys = np.column_stack((sc["dc_at"], sc["ac_at"])).astype(np.int64)
    flat = ((image[:, None] << 32) | keys).reshape(-1)
    _, index, inverse = np.unique(flat, return_index=True, return_inverse=True)
    first_use = index[inverse.reshape(-1)]   # per table slot the first slot of the batch with that table of that image
    read = keys.reshape(-1) != 0
    own = read & (first_use == np.arange(4 * n_scans))
    sizes = np.zeros((n_scans, 6), np.int64)
    sizes[:, :4] = own.reshape(n_scans, 4) * _align16(HUFF_BYTES)
    stream_len = (sc["scan_end"] - sc["scan_first"]).astype(np.int64)
    sizes[:, 4], sizes[:, 5] = (8 * n_intervals + 15) & ~15, (stream_len + 15) & ~15
    q_bytes, scan_bytes = q_sizes.sum(1), sizes.sum(1)
    before = np.cumsum(scan_bytes) - scan_bytes                  # the scans before this one
    offs = (head.at + np.cumsum(q_bytes)[image] + before)[:, None] + np.cumsum(sizes, 1) - sizes
    q_offs = (head.at + np.cumsum(q_bytes) - q_bytes + before[scan0])[:, None] + np.cumsum(q_sizes, 1) - q_sizes
    lay.nbytes = _blob_bytes(int(offs[-1, 5] + sizes[-1, 5]))
    desc["qt_off"] = np.take_along_axis(q_offs, first_q, 1) * used_q
    slot_off = offs[:, :4].reshape(-1)
    table_off, table_place = np.where(read, slot_off[first_use], 0).reshape(n_scans, 4), np.where(own, slot_off, 0).reshape(n_scans, 4)
    scans["image"] = place["file"] = image
    place["scan"] = np.arange(n_scans) - scan0[image]
    for f in ("ncomp", "comp0", "ss", "se", "ah", "al", "level", "restart", "n_intervals"):
        scans[f] = sc[f]
    scans["dc_off"], scans["ac_off"], place["dc_off"], place["ac_off"] = table_off[:, :3], table_off[:, 3], table_place[:, :3], table_place[:, 3]
    scans["interval_off"] = place["interval_off"] = offs[:, 4]
    scans["stream_off"] = place["stream_off"] = offs[:, 5]
    scans["stream_len"] = stream_len
    place["qt_off"][scan0] = np.where(q_sizes > 0, q_offs, 0)
    hdr = np.array([(n, lay.n_waves, lay.desc_off, lay.wave_off)], _HDR)
    phdr = np.array([(n_scans, lay.n_levels, lay.scan_off, lay.level_off)], _PHDR)
    for off, table in ((0, hdr), (_HDR.itemsize, phdr), (lay.desc_off, desc), (lay.scan_off, scans), (lay.level_off, level_start), (lay.wave_off, lay.waves)):
        head.put(off, table)
    lay.head, lay.place, lay.desc, lay.scans = head.finish(None), place, desc, scans
    return lay


def plan_jpeg_prog_batch(records, out_offsets=None, out_bytes=None, reserve=None, resume=None, draft=None) -> JpegProgPlan:
    """Pack the ``JpegProgRecord``s of ``parse_jpeg(progressive=True)`` into the host blob of ``hawq_jpeg_decode_batch_prog``, laid out by
    ``_prog_layout``: the adapter from records to its columns, with the level of every scan (``scan_levels``), and the host filler that
    copies table, interval and stream bytes to the offsets it gives.  ``out_offsets`` / ``out_bytes`` / ``reserve`` / ``resume`` / ``draft``
    as in ``plan_jpeg_batch``: with ``resume`` the segment table of ``hawq_jpeg_decode_batch_prog_resume`` stands behind the streams (a
    ``JpegProgResumePlan``)."""
    records = list(records)
    if not records:
        raise ValueError("empty batch")
    plan, blob = JpegProgPlan() if resume is None else JpegProgResumePlan(), _Blob()
    plan.levels = levels = [lv for r in records for lv in scan_levels(r.scans)]
    im = np.array([(r.width, r.height, r.ncomp, r.hs, r.vs, tuple(c[3] for c in (r.components * 3)[:3]), len(r.scans)) for r in records], _PROG_IMAGE)
    rows, tables = [], []   # per scan the tables it reads: DC x 3, AC, None where it reads none
    for r in records:
        keys = {}           # id of a table record -> its key: a table stays in force over several scans
        for s in r.scans:
            mine = (list(s.dc or ()) + [None] * 3)[:3] + [s.ac]
            at = [0 if t is None else keys.setdefault(id(t), len(keys) + 1) for t in mine]
            rows.append((len(s.comps), s.comps[0], s.ss, s.se, s.ah, s.al, levels[len(rows)], tuple(at[:3]), at[3], s.restart, len(s.intervals), s.scan[0], s.scan[1], 0))
            tables.append(mine)
    scales = None if draft is None else draft_scales(im["width"], im["height"], draft)
    lay = _prog_layout(im, np.array(rows, _FSCAN), out_offsets, out_bytes, scales)
    for f in ("n_scans", "n_levels", "n_waves", "level_start", "scan_off", "level_off", "wave_off", "desc_off", "coef_blocks", "plane_bytes"):
        setattr(plan, f, getattr(lay, f))
    plan.out_offsets, plan.sizes = lay.desc["out_off"].tolist(), [(r.height, r.width) for r in records]
    if scales is not None:
        plan.sizes = [(scaled_size(h, s), scaled_size(w, s)) for (h, w), s in zip(plan.sizes, scales.tolist())]
    blob.put(blob.room(lay.nbytes), lay.head)
    flat = [(r, s) for r in records for s in r.scans]
    for (r, s), mine, qt, dc, ac, interval_off, stream_off in zip(flat, tables, *(lay.place[f].tolist() for f in ("qt_off", "dc_off", "ac_off", "interval_off", "stream_off"))):
        for c, off in enumerate(qt):
            if off:   # in the first scan of an image, for the first component with that table
                blob.put(off, r.qtables[r.components[c][3]])
        for off, table in zip(dc + [ac], mine):
            if off:   # 0: an earlier scan has placed it, or the scan reads none
                blob.put(off, table)
        blob.put(interval_off, np.ascontiguousarray(s.intervals, np.int32))
        blob.put(stream_off, np.frombuffer(r.data, np.uint8, s.scan[1] - s.scan[0], s.scan[0]))
    if resume is not None:
        waves = lay.waves
        heads = waves[:, 1] == 0
        wave_of = np.zeros(plan.n_scans, np.int64)   # a scan's intervals follow one another in the wave list
        wave_of[waves[heads, 0]] = np.flatnonzero(heads)
        scan0 = np.cumsum([0] + [len(r.scans) for r in records])
        points = [np.column_stack((wave_of[np.clip(scan0[i] + p[:, 0], 0, plan.n_scans - 1)] + p[:, 1], p[:, 2:])) for i, p in enumerate(resume)]
        first, units = np.zeros(plan.n_waves, np.int64), np.zeros(plan.n_waves, np.int64)
        for k, (_, s) in enumerate(flat):
            first[wave_of[k]:wave_of[k] + len(s.intervals)] = s.intervals[:, 0]
            units[wave_of[k]:wave_of[k] + len(s.intervals)] = _interval_units(s.units, s.restart, len(s.intervals))
        segs = _segment_table(first, units, np.concatenate(points))
        plan.segs_off, plan.n_segs = blob.place(segs), len(segs)
    return plan.finish(blob, reserve, lay.out_bytes)


# ------------------------------------------------------------------------------------------------------------------ resume points
class ResumeIndex:
    """Resume points of JPEG files, recorded once by ``build_resume_index`` and used by ``decode_jpeg_batch(resume=)``
    every time the same bytes are decoded again.  ``every``: the distance in stream bytes they were recorded at; ``entries``: {(file
    length, CRC-32 of the file): (progressive, points)} with ``points`` int32 [k, 9], per point (scan - 0 in a baseline file, restart
    interval, unit, byte, bit, eobrun, predictor x 3) in the order of the file.  A file whose intervals are all shorter than ``every``
    has an entry without points."""

    def __init__(self, every, entries=None):
        self.every, self.entries = int(every), dict(entries or {})

    def __len__(self):
        return len(self.entries)

    @staticmethod
    def key(data):
        return len(data), zlib.crc32(data)

    def points(self, data, record):
        """The points of the file ``data`` that parsed into ``record``, or None: no entry for these bytes, or one of the other kind."""
        entry = self.entries.get(self.key(data))
        return entry[1] if entry is not None and entry[0] == isinstance(record, JpegProgRecord) else None

    def save(self, path):
        """To a path or a binary file object, as one ``.npz`` of plain arrays: ``every``, per entry ``length`` / ``crc`` / ``progressive`` / ``start`` (its first row of
        ``points``; one more entry at the end), and ``points``."""
        keys = sorted(self.entries)
        counts = [len(self.entries[k][1]) for k in keys]
        with (contextlib.nullcontext(path) if hasattr(path, "write") else open(path, "wb")) as f:   # the name as given: numpy would append .npz
            np.savez(f, every=np.int32(self.every), length=np.array([k[0] for k in keys], np.int64), crc=np.array([k[1] for k in keys], np.uint32),
                     progressive=np.array([self.entries[k][0] for k in keys], np.uint8), start=np.cumsum([0] + counts).astype(np.int64),
                     points=np.concatenate([self.entries[k][1] for k in keys] + [np.zeros((0, 9), np.int32)]))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            start, points = z["start"], np.ascontiguousarray(z["points"], np.int32).reshape(-1, 9)
            n = len(z["length"])
            if len(start) != n + 1 or len(z["crc"]) != n or len(z["progressive"]) != n or np.any(np.diff(start) < 0) or start[0] != 0 or start[-1] != len(points):
                raise ValueError(f"{path}: not a resume index")
            return cls(int(z["every"]), {(int(n), int(c)): (bool(p), points[a:b]) for n, c, p, a, b in zip(z["length"], z["crc"], z["progressive"], start[:-1], start[1:])})


def record_resume_points(record, every):
    """The resume points of one parsed file, int32 [k, 9] as in ``ResumeIndex``: plans it alone and runs ``hawq_jpeg_resume_record`` - the
    serial decoders on the host, no GPU work."""
    prog = isinstance(record, JpegProgRecord)
    plan = plan_jpeg_prog_batch([record]) if prog else plan_jpeg_batch([record])
    scans = record.scans if prog else [record]
    room = plan.n_waves + sum(int(((s.intervals[:, 1] - s.intervals[:, 0]) // every).sum()) for s in scans)
    segs, n = np.zeros(room, _SEG), C.c_int64(0)
    _lib.call("hawq_jpeg_resume_record", plan.blob.ctypes.data, plan.nbytes, int(prog), int(every), segs.ctypes.data, room, C.byref(n))
    segs = segs[:n.value]
    segs = segs[segs["unit0"] > 0]
    points = np.empty((len(segs), 9), np.int32)
    if prog:
        points[:, :2] = plan.blob[plan.wave_off:plan.wave_off + 8 * plan.n_waves].view(np.int32).reshape(-1, 2)[segs["wave"]]
    else:
        points[:, 0], points[:, 1] = 0, segs["wave"]
    points[:, 2], points[:, 3], points[:, 4], points[:, 5], points[:, 6:] = segs["unit0"], segs["byte"], segs["bit"], segs["eobrun"], segs["pred"]
    return points[np.lexsort((points[:, 2], points[:, 1], points[:, 0]))]


def build_resume_index(sources, every=RESUME_EVERY, progressive=False, workers=0) -> ResumeIndex:
    """Paths or bytes of image files -> the ``ResumeIndex`` of those the device path takes (``progressive``: progressive files too), with
    a point at the first unit boundary at least ``every`` stream bytes behind the one before in every restart interval longer than that.
    The recorder is host code of the library and releases the GIL: ``workers`` threads share the files."""
    every = int(every)
    if every < 1:
        raise ValueError(f"every must be at least 1, not {every}")

    def one(source):
        data = read_source(source)
        try:
            record = parse_jpeg(data, progressive=True) if progressive else parse_jpeg(data)
        except UnsupportedJpeg:
            return None
        return ResumeIndex.key(data), (isinstance(record, JpegProgRecord), record_resume_points(record, every))

    sources = list(sources)
    if workers > 0:
        with ThreadPoolExecutor(min(int(workers), 16)) as pool:
            found = list(pool.map(one, sources))
    else:
        found = [one(s) for s in sources]
    return ResumeIndex(every, dict(f for f in found if f is not None))


# ------------------------------------------------------------------------------------------------------------------ the device front end
_FFILE = np.dtype(_lib.JpegFrontFile)
FRONT_OK, FRONT_REFUSED = 0, 1
# Defer codes of the device walker (csrc/jpeg_front.h) on files ``parse_jpeg`` may still accept: bounds of the kernel,
# not properties of the format.  Every other deferred file is one ``parse_jpeg`` refuses.
FRONT_DEFERS_BY_DESIGN = {2: "more than 64 marker segments before the scan", 3: "a file above 1 GiB"}


def pack_files(datas, reserve=None):
    """The raw files one after the other at 16-byte aligned offsets -> (``hawq_jpeg_front_file`` table, uint8 buffer, bytes used);
    ``reserve(nbytes)`` returns the buffer to write into, a fresh one without it."""
    table = np.zeros(len(datas), _FFILE)
    table["length"] = [len(d) for d in datas]
    ends = np.cumsum((table["length"] + 15) & ~15)
    table["offset"] = ends - ((table["length"] + 15) & ~15)
    total = max(int(ends[-1]), 16)
    buf = np.zeros(total, np.uint8) if reserve is None else reserve(total)
    for d, off in zip(datas, table["offset"].tolist()):
        buf[off:off + len(d)] = np.frombuffer(d, np.uint8)
    return table, buf, total


def front_scan_host(datas):
    """``hawq_jpeg_front_scan_host`` on the files ``datas``: the walker of the scan kernel on the host, no GPU work -> one
    ``hawq_jpeg_front_info`` per file (numpy records)."""
    table, buf, total = pack_files(datas)
    info = np.zeros(len(datas), _FINFO)
    _lib.call("hawq_jpeg_front_scan_host", buf.ctypes.data, total, table.ctypes.data, len(datas), info.ctypes.data)
    return info


# ``progressive="device"``: the kind of an accepted file is word 0, its number of scans word 1 of ``reserved``
FRONT_KIND_BASELINE, FRONT_KIND_PROG = 0, 1
# The defer codes of ``hawq_jpeg_front_scan_prog`` on files ``parse_jpeg(data, progressive=True)`` may still accept, as above
FRONT_PROG_DEFERS_BY_DESIGN = {2: "more than 64 marker segments up to the frame header, or more than 256 in a progressive file", 3: "a file above 1 GiB"}


def front_scan_prog_host(datas):
    """``hawq_jpeg_front_scan_prog_host`` on the files ``datas``: the walker of the scan kernel for both kinds on the host, no GPU work
    -> (one ``hawq_jpeg_front_info`` per file, ``hawq_jpeg_front_scan_rec`` [files, 64]: the scans of the progressive ones)."""
    table, buf, total = pack_files(datas)
    info, scans = np.zeros(len(datas), _FINFO), np.zeros((len(datas), MAX_SCANS), _FSCAN)
    _lib.call("hawq_jpeg_front_scan_prog_host", buf.ctypes.data, total, table.ctypes.data, len(datas), info.ctypes.data, scans.ctypes.data)
    return info, scans


def front_layout(info, files, out_offsets, out_bytes, draft=None) -> FrontLayout:
    """``_baseline_layout`` of the accepted files of a scan, for ``hawq_jpeg_front_fill`` to fill.  ``info``: the records of the scan;
    ``files``: indices of accepted ones, ascending; ``out_offsets`` / ``out_bytes``: where each image goes in the output; ``draft``: as in
    ``plan_jpeg_batch``, the scales computed here on the host from the sizes the scan reports."""
    files = np.asarray(files, np.int64)
    o = info[files]
    if len(files) == 0 or (o["defer"] != FRONT_OK).any():
        raise ValueError("front_layout wants accepted files")
    lay = _baseline_layout(o, out_offsets, out_bytes, None if draft is None else draft_scales(o["width"], o["height"], draft))
    lay.place["file"] = files
    return lay


class _Staged:
    """The files of a batch on the device behind ``_front_scan``: ``table`` (host), ``total`` bytes, and the device tensors ``files``,
    ``table_dev`` and ``info_dev``; behind ``_front_scan_prog`` ``scans_dev`` as well."""
    __slots__ = ("table", "total", "files", "table_dev", "info_dev", "scans_dev")


def _stage_files(datas, dev) -> _Staged:
    """Pack the raw files into the pinned staging buffer of their kind and upload them in one copy with their table"""
    s = _Staged()
    st = _staging(dev, "jpeg_files")
    room = _align16(len(datas) * _FFILE.itemsize)   # the table in front of the files
    s.table, _, s.total = pack_files(datas, lambda nbytes: st.reserve(room + nbytes, dev)[0].numpy()[room:])
    st.host.numpy()[:s.table.nbytes] = s.table.view(np.uint8)
    st.upload(room + s.total)
    s.table_dev, s.files = st.dev[:room], st.dev[room:room + s.total]
    return s


def _front_scan(datas, dev):
    """Pack the raw files into the pinned staging buffer of their kind, upload them in one copy with their table, run
    ``hawq_jpeg_front_scan`` and read the info records back (one synchronisation) -> (info, what ``_front_launch`` needs)."""
    with torch.cuda.device(dev):
        s = _stage_files(datas, dev)
        s.info_dev = torch.empty(len(datas) * _FINFO.itemsize, dtype=torch.uint8, device=dev)
        _lib.call("hawq_jpeg_front_scan", s.files.data_ptr(), s.total, s.table_dev.data_ptr(), s.table.ctypes.data, len(datas), s.info_dev.data_ptr(),
                  torch.cuda.current_stream(dev).cuda_stream)
        info = s.info_dev.cpu().numpy().view(_FINFO)
    return info, s


def _front_scan_prog(datas, dev):
    """``_front_scan`` with ``hawq_jpeg_front_scan_prog``: the info records and the scan records come back in one copy (one
    synchronisation) -> (info, scans [files, 64], what ``_front_launch`` and ``_front_prog_fill`` need)."""
    n = len(datas)
    with torch.cuda.device(dev):
        s = _stage_files(datas, dev)
        records = torch.empty(n * (_FINFO.itemsize + MAX_SCANS * _FSCAN.itemsize), dtype=torch.uint8, device=dev)
        s.info_dev, s.scans_dev = records[:n * _FINFO.itemsize], records[n * _FINFO.itemsize:]
        _lib.call("hawq_jpeg_front_scan_prog", s.files.data_ptr(), s.total, s.table_dev.data_ptr(), s.table.ctypes.data, n, s.info_dev.data_ptr(),
                  s.scans_dev.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        host = records.cpu().numpy()
    return host[:n * _FINFO.itemsize].view(_FINFO), host[n * _FINFO.itemsize:].view(_FSCAN).reshape(n, MAX_SCANS), s


def front_prog_layout(info, scans, files, out_offsets, out_bytes, draft=None) -> ProgLayout:
    """``_prog_layout`` of the progressive files a scan accepted, for ``hawq_jpeg_front_fill_prog`` to fill.  ``info`` / ``scans``: the
    records of ``hawq_jpeg_front_scan_prog``; ``files``: indices of accepted progressive ones, ascending; the rest as in ``front_layout``."""
    files = np.asarray(files, np.int64)
    o = info[files]
    if len(files) == 0 or (o["defer"] != FRONT_OK).any() or (o["reserved"][:, 0] != FRONT_KIND_PROG).any():
        raise ValueError("front_prog_layout wants accepted progressive files")
    im = np.zeros(len(files), _PROG_IMAGE)
    for f in ("width", "height", "ncomp", "hs", "vs", "tq"):
        im[f] = o[f]
    im["n_scans"] = o["reserved"][:, 1]
    sc = scans[files][np.arange(MAX_SCANS) < im["n_scans"][:, None]]   # the scans of the files, file after file
    lay = _prog_layout(im, sc, out_offsets, out_bytes, None if draft is None else draft_scales(o["width"], o["height"], draft))
    lay.place["file"] = files[lay.place["file"]]
    return lay


def _front_prog_fill(staged, info, scans, files, out_offsets, out, dev, draft=None):
    """The first half of the device call of ``decode_jpeg_batch(progressive="device")`` for the progressive files the scan accepted: lay
    the blob out, have ``hawq_jpeg_front_fill_prog`` write it from the staged files and start its copy back into pinned memory.  Nothing
    waits here: the caller synchronises the stream once for this blob and the baseline one -> what ``_front_prog_decode`` needs."""
    lay = front_prog_layout(info, scans, files, out_offsets, out.numel(), draft)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        st_blob, st_tab = _staging(dev, "jpeg_front_prog"), _staging(dev, "jpeg_front_prog_tables")
        host_blob, blob = st_blob.reserve(lay.nbytes, dev)
        place_bytes = lay.place.nbytes
        host_tab, tab = st_tab.reserve(place_bytes + lay.head.size, dev)
        host_tab.numpy()[:place_bytes] = lay.place.view(np.uint8)
        host_tab.numpy()[place_bytes:place_bytes + lay.head.size] = lay.head
        st_tab.upload(place_bytes + lay.head.size)
        _lib.call("hawq_jpeg_front_fill_prog", staged.files.data_ptr(), staged.total, staged.table_dev.data_ptr(), staged.table.ctypes.data, len(staged.table),
                  staged.info_dev.data_ptr(), info.ctypes.data, staged.scans_dev.data_ptr(), scans.ctypes.data, tab.data_ptr(), lay.place.ctypes.data, len(lay.place),
                  blob.data_ptr(), lay.nbytes, stream.cuda_stream)
        blob[:lay.head.size].copy_(tab[place_bytes:place_bytes + lay.head.size])
        host_blob[:lay.nbytes].copy_(blob[:lay.nbytes], non_blocking=True)
    return lay, blob, host_blob, len(files)


def _front_prog_decode(filled, out, dev, events=None, wait=True):
    """The second half, behind a synchronisation of the stream (``wait``: made here; not when the caller has made one since the fill):
    hand the blob read back as the host blob to ``hawq_jpeg_decode_batch_prog``, so ``hawq_jpeg_prog_ok`` passes it before any decode
    kernel reads it.  Returns the device status as ``_launch`` does."""
    lay, blob, host_blob, n = filled
    with torch.cuda.device(dev):
        if wait:
            torch.cuda.current_stream(dev).synchronize()
        return _decode("hawq_jpeg_decode_batch_prog", blob, host_blob.numpy().ctypes.data, lay.nbytes, lay.coef_blocks, lay.plane_bytes, n, out, events,
                       torch.cuda.current_stream(dev))[0]


def _front_launch(staged, info, files, out_offsets, out, dev, events=None, sync=None, draft=None):
    """The device call of ``decode_jpeg_batch(front_end="device")`` for the files the scan accepted: lay the blob out, have
    ``hawq_jpeg_front_fill`` write it from the staged files, read it back into pinned memory (the second synchronisation) and hand it as
    the host blob to ``hawq_jpeg_decode_batch`` - or ``_sync``, with the job table computed from the intervals just read back and
    uploaded alone - so the library's checker passes the blob before any decode kernel reads it.  Returns the device status as
    ``_launch`` does."""
    lay = front_layout(info, files, out_offsets, out.numel(), draft)
    n = len(files)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        st_blob, st_tab = _staging(dev, "jpeg_front"), _staging(dev, "jpeg_front_tables")
        room = lay.nbytes + (_JOB.itemsize * lay.n_waves if sync is not None else 0)   # at most one job per interval
        host_blob, blob = st_blob.reserve(room, dev)
        place_bytes = lay.place.nbytes
        host_tab, tab = st_tab.reserve(place_bytes + lay.head.size, dev)
        host_tab.numpy()[:place_bytes] = lay.place.view(np.uint8)
        host_tab.numpy()[place_bytes:place_bytes + lay.head.size] = lay.head
        st_tab.upload(place_bytes + lay.head.size)
        _lib.call("hawq_jpeg_front_fill", staged.files.data_ptr(), staged.total, staged.table_dev.data_ptr(), staged.table.ctypes.data, len(staged.table),
                  staged.info_dev.data_ptr(), info.ctypes.data, tab.data_ptr(), lay.place.ctypes.data, n, blob.data_ptr(), room, stream.cuda_stream)
        blob[:lay.head.size].copy_(tab[place_bytes:place_bytes + lay.head.size])
        host_blob[:lay.nbytes].copy_(blob[:lay.nbytes], non_blocking=True)
        stream.synchronize()
        host = host_blob.numpy()
        nbytes, job_table = lay.nbytes, None
        if sync is not None:
            sub_bytes, min_sync_bytes = _check_sync(sync)
            lengths = [np.diff(host[o:o + 8 * k].view(np.int32).reshape(-1, 2), axis=1).reshape(-1)
                       for o, k in zip(lay.desc["interval_off"].tolist(), lay.desc["n_intervals"].tolist())]
            jobs, scratch_bytes = _sync_job_table(np.concatenate(lengths), sub_bytes, min_sync_bytes)
            host[nbytes:nbytes + jobs.nbytes] = jobs.view(np.uint8)
            if jobs.nbytes:
                blob[nbytes:nbytes + jobs.nbytes].copy_(host_blob[nbytes:nbytes + jobs.nbytes], non_blocking=True)
                st_blob.event = torch.cuda.Event()
                st_blob.event.record()
            job_table = (sub_bytes, min_sync_bytes, nbytes, len(jobs), scratch_bytes)
            nbytes += jobs.nbytes
        return _decode("hawq_jpeg_decode_batch", blob, host.ctypes.data, nbytes, lay.coef_blocks, lay.plane_bytes, n, out, events, stream, sync=job_table)[0]


# ------------------------------------------------------------------------------------------------------------------ the device call
def _staging(dev, key):
    """The pinned ``_Staging`` buffer of image.py for the kind ``key`` on ``dev``: one per kind, as the blobs of a batch are in flight at once."""
    from .image import _STAGING, _Staging
    return _STAGING.setdefault((dev.index, key), _Staging())


def _decode(entry, blob, host_ptr, nbytes, coef_blocks, plane_bytes, n, out, events, stream, more=(), sync=None):
    """The tail of ``_launch`` and ``_front_launch``: allocate the coefficient slab, the planes and the status of ``n`` images and run the
    decode entry point ``entry`` on the device blob ``blob``, whose host copy (``nbytes`` bytes at ``host_ptr``) the library checks first.
    ``more``: the arguments of ``entry`` between the status and the events.  ``sync``: (sub_bytes, min_sync_bytes, jobs_off, n_jobs,
    scratch_bytes) of a blob with a job table: ``entry`` + ``_sync`` and its scratch.  -> (status, scratch or None) on the device."""
    dev, scratch = out.device, None
    if sync is not None:
        *table, scratch_bytes = sync
        scratch = torch.empty(max(scratch_bytes, 16), dtype=torch.uint8, device=dev)
        entry, more = entry + "_sync", (*table, scratch.data_ptr(), scratch_bytes)
    coef = torch.empty(coef_blocks * 64, dtype=torch.int16, device=dev)
    planes = torch.empty(plane_bytes, dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    ev = (C.c_void_p * 4)(*events) if events is not None else None
    _lib.call(entry, blob.data_ptr(), host_ptr, nbytes, coef.data_ptr(), coef_blocks, planes.data_ptr(), plane_bytes, out.data_ptr(), out.numel(), status.data_ptr(),
              *more, ev, stream.cuda_stream)
    return status, scratch


def _launch(records, out_offsets, out, dev, events=None, sync=None, info=None, resume=None, draft=None):
    """The device call of ``decode_jpeg_batch`` for records of one kind: plan into the pinned staging buffer of that kind, check, upload
    in one copy, run the three stages on the current stream, writing into the uint8 device tensor ``out`` at ``out_offsets``.  Returns
    the int32 status per record as a device tensor: reading it synchronises, so the caller does that when everything of the batch is
    enqueued.  ``JpegProgRecord``s: ``hawq_jpeg_decode_batch_prog``.  ``JpegRecord``s: ``hawq_jpeg_decode_batch``, or with ``sync`` =
    (sub_bytes, min_sync_bytes) ``hawq_jpeg_decode_batch_sync``; a dict ``info`` then receives ``jobs`` (the plan's) and ``rounds`` /
    ``decodes`` (what the kernel counted per job; a synchronising read of the scratch).  ``resume``: per record its resume points:
    ``hawq_jpeg_decode_batch_resume`` / ``_prog_resume``, one wave per segment.  ``draft``: to the planner."""
    prog = isinstance(records[0], JpegProgRecord)
    if prog and sync is not None:
        raise ValueError("entropy='sync' does not take progressive records")
    key, entry = ("jpeg_prog", "hawq_jpeg_decode_batch_prog") if prog else ("jpeg", "hawq_jpeg_decode_batch")   # with sync: ``_decode`` picks ``_sync``
    if resume is not None:
        key, entry = key + "_resume", entry + "_resume"
    with torch.cuda.device(dev):
        st = _staging(dev, key)
        reserve = lambda nbytes: st.reserve(nbytes, dev)[0].numpy()   # the plan's blob is ``st.host``, its upload ``st.dev``
        if prog:
            plan = plan_jpeg_prog_batch(records, out_offsets, out.numel(), reserve, resume, draft)
        else:
            plan = plan_jpeg_batch(records, out_offsets, out.numel(), reserve, sync, resume, draft)
        # on the host blob, before anything is uploaded or launched
        if not plan.ok() or (sync is not None and not plan.sync_ok()) or (resume is not None and not plan.resume_ok()):
            raise RuntimeError("libhawq_mi355: " + _lib.load().hawq_last_error().decode())
        st.upload(plan.nbytes)
        status, scratch = _decode(entry, st.dev, plan.blob.ctypes.data, plan.nbytes, plan.coef_blocks, plan.plane_bytes, len(records), out, events,
                                  torch.cuda.current_stream(dev), more=() if resume is None else (plan.segs_off, plan.n_segs),
                                  sync=None if sync is None else (plan.sub_bytes, plan.min_sync_bytes, plan.jobs_off, plan.n_jobs, plan.scratch_bytes))
        if sync is not None and info is not None:
            info["jobs"] = list(plan.jobs)
            host = scratch.cpu().numpy()
            heads = [host[off:off + 8].view(np.int32) for _, _, off in plan.jobs]
            info["rounds"], info["decodes"] = [int(h[0]) for h in heads], [int(h[1]) for h in heads]
        return status


def read_source(source) -> bytes:
    """A path, bytes or a binary file object -> the file's bytes."""
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source)
    if hasattr(source, "read"):
        return source.read()
    with open(source, "rb") as f:
        return f.read()


def decode_jpeg_batch(sources, device=None, entropy="serial", sub_bytes=None, min_sync_bytes=None, progressive=False, resume=None, front_end="host", draft=None):
    """Paths or bytes of image files -> ``(images, fallbacks)``: ``images[i]`` a uint8 [H, W, 3] RGB tensor on the MI355X equal to
    ``image.decode_image(sources[i])``, ``fallbacks`` the list of ``(index, reason)`` of the images the HOST decoder produced: files
    ``parse_jpeg`` refuses (progressive, CMYK, not a JPEG, ...) and files whose device decode reported a status (damaged streams).
    All images are views into one device allocation made by this call, at 16-byte aligned offsets, so ``preprocess_batch_fused`` reads
    them in place.  An error of the host decoder on such a file propagates as it does from ``decode_image``.
    ``entropy``: ``"serial"`` decodes every restart interval with one wave; ``"sync"`` decodes intervals of at least ``min_sync_bytes``
    stream bytes with one lane per ``sub_bytes`` of them (``hawq_jpeg_decode_batch_sync``; defaults ``MIN_SYNC_BYTES`` / ``SUB_BYTES``) -
    the same bytes and the same fallbacks, faster on files without restart markers.
    ``progressive``: progressive files (SOF2) inside the scope of ``parse_progressive`` are decoded on the device as well
    (``hawq_jpeg_decode_batch_prog``, one wave per scan and restart interval, one entropy launch per level of the batch) into the same
    allocation, in a second call beside the one for the baseline files; the rest fall back as before.  ``entropy="sync"`` applies to the
    baseline files only: a progressive scan is decoded by one wave per restart interval.
    ``resume``: a ``ResumeIndex``.  A file it has an entry for (same length, same CRC-32, same kind) is decoded from its recorded resume
    points, one wave per segment of a restart interval (``hawq_jpeg_decode_batch_resume`` / ``_prog_resume``), in a call of its own
    beside those above; every other file goes exactly the way it goes without the option - the same bytes and the same fallbacks.
    ``front_end``: ``"host"`` parses every file with ``parse_jpeg`` and plans the blob in Python.  ``"device"`` uploads the raw files,
    has the MI355X walk the headers and check the restart markers (``hawq_jpeg_front_scan``) and write the blob of the baseline files
    it accepts (``hawq_jpeg_front_fill``); every file it defers - progressive ones, other formats, refused and malformed ones - goes
    through ``parse_jpeg`` exactly as with ``"host"``.  The same bytes and the same fallbacks, at two more synchronisations per batch
    (profiles/jpeg_front.md: it wins on all three measured sets, 11.8 -> 5.1 ms per 128 files with restart markers); not together with
    ``resume``.
    ``progressive="device"`` (needs ``front_end="device"``): the MI355X also walks the progressive files inside the scope of
    ``parse_progressive`` (``hawq_jpeg_front_scan_prog``: one launch for both kinds, with the level of every scan) and writes their blob
    (``hawq_jpeg_front_fill_prog``, one workgroup per scan), which comes back with the baseline one behind the same synchronisation and
    goes to ``hawq_jpeg_decode_batch_prog``; what the walker defers goes through ``parse_jpeg(data, progressive=True)`` as with
    ``True``.  The same bytes and the same fallbacks (profiles/jpeg_front_prog.md says for which batches it was measured to pay).
    ``draft``: None, or a (width, height) pair: every image is decoded at the reduced size Pillow's draft mode gives it,
    ``images[i]`` = ``image.decode_image(sources[i], draft=draft)`` - a JPEG at 1 / ``draft_scale`` of its size, ceil(H / s) x ceil(W / s),
    produced on the device by the library's reduced inverse DCTs, every other format at full size.  It composes with
    every option above; the fallbacks are those of the call without it, and the host decoder takes them with the same draft."""
    from .image import decode_image
    draft = check_draft(draft)
    if front_end not in ("host", "device"):
        raise ValueError(f"front_end must be 'host' or 'device', not {front_end!r}")
    if front_end == "device" and resume is not None:
        raise ValueError("front_end='device' does not take resume")
    if progressive not in (False, True, "device"):
        raise ValueError(f"progressive must be False, True or 'device', not {progressive!r}")
    on_device = isinstance(progressive, str)   # "device": the walk and the blob of progressive files on the MI355X too
    if on_device and front_end != "device":
        raise ValueError("progressive='device' needs front_end='device'")
    if entropy not in ("serial", "sync"):
        raise ValueError(f"entropy must be 'serial' or 'sync', not {entropy!r}")
    if entropy == "serial" and (sub_bytes is not None or min_sync_bytes is not None):
        raise ValueError("sub_bytes / min_sync_bytes belong to entropy='sync'")
    scaled = {} if draft is None else {"draft": draft}   # absent without the option: the launches get today's arguments
    more = {} if entropy == "serial" else {"sync": (SUB_BYTES if sub_bytes is None else int(sub_bytes), MIN_SYNC_BYTES if min_sync_bytes is None else int(min_sync_bytes))}
    datas = [read_source(s) for s in sources]
    if not datas:
        raise ValueError("empty batch")
    dev = torch.device("cuda" if device is None else device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    records, fallbacks, host = {}, [], {}
    info, front, front_prog = None, [], []
    if on_device:
        info, scans, staged = _front_scan_prog(datas, dev)
        accepted = info["defer"] == FRONT_OK
        front = np.flatnonzero(accepted & (info["reserved"][:, 0] == FRONT_KIND_BASELINE)).tolist()
        front_prog = np.flatnonzero(accepted & (info["reserved"][:, 0] == FRONT_KIND_PROG)).tolist()
    elif front_end == "device":
        info, staged = _front_scan(datas, dev)
        front = np.flatnonzero(info["defer"] == FRONT_OK).tolist()
    taken = set(front) | set(front_prog)
    for i, data in enumerate(datas):
        if i in taken:
            continue
        try:
            records[i] = parse_jpeg(data, progressive=True) if progressive else parse_jpeg(data)
        except UnsupportedJpeg as e:
            fallbacks.append((i, e.reason))
            host[i] = decode_image(data, **scaled)
    sizes = [(records[i].height, records[i].width) if i in records else (int(info["height"][i]), int(info["width"][i])) if i in taken else tuple(host[i].shape[:2])
             for i in range(len(datas))]
    if draft is not None:   # what the device decodes comes out reduced; what the host has decoded already is
        sizes = [(h, w) if i in host else (scaled_size(h, s), scaled_size(w, s)) for i, (h, w) in enumerate(sizes) for s in (draft_scale(w, h, draft),)]
    offsets, total = output_layout(sizes)
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    # a file whose entry has no points (no interval longer than the index's distance) has nothing to gain: it goes as without the index
    points = {} if resume is None else {i: p for i, p in ((i, resume.points(datas[i], r)) for i, r in records.items()) if p is not None and len(p)}
    enqueued = []   # (indices, device status): the progressive calls first, the baseline calls second, every status read behind all of them
    for kind, options in ((JpegProgRecord, {}), (JpegRecord, more)):
        for indexed in (False, True) if points else (False,):
            idx = sorted(i for i, r in records.items() if isinstance(r, kind) and (i in points) == indexed)
            if idx:
                if indexed:
                    options = {"resume": [points[i] for i in idx]}
                enqueued.append((idx, _launch([records[i] for i in idx], [offsets[i] for i in idx], out, dev, **options, **scaled)))
    # both fills are enqueued before anything waits: the synchronisation inside ``_front_launch`` brings both blobs back
    filled = _front_prog_fill(staged, info, scans, front_prog, [offsets[i] for i in front_prog], out, dev, **scaled) if front_prog else None
    if front:
        enqueued.append((front, _front_launch(staged, info, front, [offsets[i] for i in front], out, dev, **more, **scaled)))
    if front_prog:
        enqueued.append((front_prog, _front_prog_decode(filled, out, dev, wait=not front)))
    status = {i: st for idx, device_status in enqueued for i, st in zip(idx, device_status.cpu().numpy())}
    for i, st in sorted(status.items()):
        if st != 0:
            fallbacks.append((i, "device status %d: %s" % (st, STATUS_NAMES.get(int(st), "unknown"))))
            host[i] = decode_image(datas[i], **scaled)
            if tuple(host[i].shape[:2]) != sizes[i]:
                raise RuntimeError(f"image {i}: the host decoder gives {tuple(host[i].shape[:2])}, the header {sizes[i]}")
    for i, im in host.items():
        out[offsets[i]:offsets[i] + im.numel()].copy_(im.reshape(-1))
    images = [out[offsets[i]:offsets[i] + h * w * 3].view(h, w, 3) for i, (h, w) in enumerate(sizes)]
    return images, sorted(fallbacks)
