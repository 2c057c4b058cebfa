"""Batched baseline JPEG decoding on the MI355X (DESIGN.md "Device JPEG decode"): file bytes -> uint8 HWC RGB tensors on the device,
byte for byte what ``image.decode_image`` (Pillow: libjpeg-turbo, ISLOW IDCT, fancy upsampling) gives on the host.

Host side, pure Python / numpy: ``parse_jpeg`` reads the headers of one file and refuses (``UnsupportedJpeg``) whatever the device
path does not take; ``plan_jpeg_batch`` packs the descriptors, tables, entropy-coded bytes and restart intervals of a batch into one
blob (``struct hawq_jpeg_*`` of include/hawq_mi355.h); ``decode_jpeg_batch`` uploads it in one pinned copy, runs
``hawq_jpeg_decode_batch`` (entropy decode -> IDCT -> upsampling + colour) and hands every refused or failed image to the host decoder,
with the reason.  ``image.folder_loader(device_decode=True)`` feeds the result to ``preprocess_batch_fused`` in place.
``entropy="sync"`` decodes long restart intervals with many lanes each (``hawq_jpeg_decode_batch_sync``): the planner
appends a job table, ``hawq_jpeg_sync_ok`` checks it, the launch gets a scratch buffer; everything else is the same.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_SIDE = 8192
HUFF_BYTES = C.sizeof(_lib.JpegHuff)
_HUFF = np.dtype(_lib.JpegHuff)
_DESC = np.dtype(_lib.JpegDesc)
_HDR = np.dtype(_lib.JpegBatchHdr)
_JOB = np.dtype(_lib.JpegSyncJob)
SYNC_SUB_MIN, SYNC_SUB_MAX = 16, 4096   # HAWQ_JPEG_SYNC_SUB_MIN / _MAX
SYNC_JOB_HDR_BYTES, SYNC_SUB_RECORD_BYTES = 16, C.sizeof(_lib.JpegSyncSub)
# entropy="sync" defaults: the fastest row of profiles/jpeg_sync.md on files without restart markers that leaves files with them alone
SUB_BYTES = 32
MIN_SYNC_BYTES = 4096
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


_SOF_REASON = {0xC1: "extended sequential (SOF1)", 0xC2: "progressive (SOF2)"}


def parse_jpeg(data) -> JpegRecord:
    """Headers of one JPEG file (bytes) -> ``JpegRecord``, or ``UnsupportedJpeg(reason)`` for anything outside the device path:
    baseline SOF0 with 8-bit samples and tables, one interleaved scan of all components, Huffman table ids 0 and 1, three components
    with ids 1, 2, 3, luma 1x1 / 2x1 / 2x2 and chroma 1x1 without an Adobe marker, or one 1x1 component, restart markers complete
    and in order, both sides at most 8192."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise UnsupportedJpeg("not a JPEG")
    rec = JpegRecord()
    rec.data, rec.qtables, rec.huffman, rec.restart = data, {}, {}, 0
    frame, adobe, pos = None, False, 2

    def need(upto):
        if upto > n:
            raise UnsupportedJpeg("truncated header")

    while True:
        need(pos + 2)
        if data[pos] != 0xFF:
            raise UnsupportedJpeg("marker expected")
        while data[pos + 1] == 0xFF:   # fill bytes
            pos += 1
            need(pos + 2)
        marker = data[pos + 1]
        pos += 2
        if marker == 0xD8 or marker == 0x01 or 0xD0 <= marker <= 0xD7:
            continue
        if marker == 0xD9:
            raise UnsupportedJpeg("no scan")
        need(pos + 2)
        length = (data[pos] << 8) | data[pos + 1]
        if length < 2:
            raise UnsupportedJpeg("bad segment length")
        need(pos + length)
        seg = data[pos + 2:pos + length]
        if marker == 0xC0:
            if frame is not None:
                raise UnsupportedJpeg("several frames")
            if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                raise UnsupportedJpeg("bad frame header")
            if seg[0] != 8:
                raise UnsupportedJpeg("sample precision not 8")
            rec.height, rec.width = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            if rec.height == 0:
                raise UnsupportedJpeg("DNL (height in the scan)")
            if rec.width == 0:
                raise UnsupportedJpeg("bad frame header")
            if seg[5] == 4:
                raise UnsupportedJpeg("four components")
            if seg[5] not in (1, 3):
                raise UnsupportedJpeg("component count")
            frame = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])]
        elif marker in (0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF):
            raise UnsupportedJpeg("arithmetic coding")
        elif marker in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7):
            raise UnsupportedJpeg(_SOF_REASON.get(marker, "SOF%d" % (marker - 0xC0)))
        elif marker == 0xC4:
            at = 0
            while at < len(seg):
                if at + 17 > len(seg):
                    raise UnsupportedJpeg("bad Huffman table")
                tc, th = seg[at] >> 4, seg[at] & 15
                bits = seg[at + 1:at + 17]
                count = sum(bits)
                if tc > 1 or at + 17 + count > len(seg):
                    raise UnsupportedJpeg("bad Huffman table")
                if th > 1:
                    raise UnsupportedJpeg("Huffman table id above 1")
                rec.huffman[(tc, th)] = huffman_table(bits, seg[at + 17:at + 17 + count])
                at += 17 + count
        elif marker == 0xDB:
            at = 0
            while at < len(seg):
                pq, tq = seg[at] >> 4, seg[at] & 15
                if pq != 0:
                    raise UnsupportedJpeg("16-bit quantisation table")
                if tq > 3 or at + 65 > len(seg):
                    raise UnsupportedJpeg("bad quantisation table")
                rec.qtables[tq] = np.frombuffer(seg[at + 1:at + 65], np.uint8).astype(np.uint16)
                at += 65
        elif marker == 0xDD:
            if len(seg) != 2:
                raise UnsupportedJpeg("bad restart interval")
            rec.restart = (seg[0] << 8) | seg[1]
        elif marker == 0xDC:
            raise UnsupportedJpeg("DNL")
        elif marker == 0xEE:
            adobe = adobe or seg[:5] == b"Adobe"
        elif marker == 0xDA:
            break
        pos += length
    # the scan header
    if frame is None:
        raise UnsupportedJpeg("scan before the frame header")
    if adobe:
        raise UnsupportedJpeg("Adobe marker")
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
        if tq not in rec.qtables or (0, td) not in rec.huffman or (1, ta) not in rec.huffman:
            raise UnsupportedJpeg("missing table")
        comps.append((cid, h, v, tq, td, ta))
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
    # the entropy-coded segment: up to the first marker that is no RSTn; behind it nothing but EOI may follow
    start = pos + length
    arr = np.frombuffer(data, np.uint8)
    ff = np.flatnonzero(arr[start:n - 1] == 0xFF) + start
    nxt = arr[ff + 1]
    marks = ff[(nxt != 0) & (nxt != 0xFF)]
    codes = arr[marks + 1]
    ends = np.flatnonzero((codes & 0xF8) != 0xD0)
    if ends.size == 0:
        raise UnsupportedJpeg("truncated scan")
    if codes[ends[0]] != 0xD9:
        raise UnsupportedJpeg("DNL" if codes[ends[0]] == 0xDC else "several scans")
    end = int(marks[ends[0]])
    rst, rst_codes = marks[:ends[0]], codes[:ends[0]]
    mcus = rec.mcus_x * rec.mcus_y
    expected = -(-mcus // rec.restart) - 1 if rec.restart else 0
    if rst.size != expected or not np.array_equal(rst_codes & 7, np.arange(rst.size) & 7):
        raise UnsupportedJpeg("restart markers missing or out of order")
    firsts = np.concatenate([[start], rst + 2]) - start
    lasts = np.concatenate([rst, [end]]) - start
    rec.scan, rec.intervals = (start, end), np.stack([firsts, lasts], 1).astype(np.int32)
    return rec


def _align16(n: int) -> int:
    return (n + 15) & ~15


class JpegPlan:
    """What ``plan_jpeg_batch`` returns.  ``blob``: uint8 array (the first ``nbytes`` bytes count), ``coef_blocks`` / ``plane_bytes`` /
    ``out_bytes``: the sizes of the three device buffers the launch needs, ``out_offsets`` / ``sizes``: where each image lands in the
    output and its (height, width), ``n_waves``: restart intervals in the batch.  With ``sync``: ``sub_bytes`` / ``min_sync_bytes``,
    ``jobs_off`` / ``n_jobs``: the table of ``hawq_jpeg_sync_job`` in the blob (one per interval of at least ``min_sync_bytes``),
    ``jobs``: the same as (wave, n_sub, scratch offset) tuples, ``scratch_bytes``: the device scratch the launch needs."""
    __slots__ = ("blob", "nbytes", "coef_blocks", "plane_bytes", "out_bytes", "out_offsets", "sizes", "n_waves", "sub_bytes", "min_sync_bytes", "jobs_off",
                 "n_jobs", "jobs", "scratch_bytes")

    def ok(self) -> bool:
        """``hawq_jpeg_batch_ok`` on the host blob (no GPU work); the reason of a refusal is in ``hawq_last_error``."""
        return bool(_lib.load().hawq_jpeg_batch_ok(self.blob.ctypes.data, self.nbytes, self.coef_blocks, self.plane_bytes, self.out_bytes))

    def sync_ok(self) -> bool:
        """``hawq_jpeg_sync_ok`` on the host blob of a plan made with ``sync`` (after ``ok``; no GPU work)."""
        return bool(_lib.load().hawq_jpeg_sync_ok(self.blob.ctypes.data, self.nbytes, self.sub_bytes, self.min_sync_bytes, self.jobs_off, self.n_jobs,
                                                  self.scratch_bytes))


def plan_jpeg_batch(records, out_offsets=None, out_bytes=None, reserve=None, sync=None) -> JpegPlan:
    """Pack the records of ``parse_jpeg`` into one host blob: header | descriptors | wave list | per image: quantisation tables, Huffman
    tables, intervals, stream - every part at a 16-byte aligned offset.  ``out_offsets`` / ``out_bytes``: where each image goes in an
    output buffer of that size (default: one after the other, 16-byte aligned).  ``reserve(nbytes)`` returns the uint8 array to write
    into (at least nbytes, 16-byte aligned; e.g. a pinned staging buffer); a fresh array without it.  ``sync`` = (sub_bytes,
    min_sync_bytes): append the job table of ``hawq_jpeg_decode_batch_sync`` behind the streams - one job per interval of at least
    ``min_sync_bytes`` bytes, cut into sub-sequences of ``sub_bytes``, with its slice of the scratch."""
    records = list(records)
    if not records:
        raise ValueError("empty batch")
    n = len(records)
    n_waves = sum(len(r.intervals) for r in records)
    desc_off = _align16(_HDR.itemsize)
    wave_off = _align16(desc_off + n * _DESC.itemsize)
    at = _align16(wave_off + 8 * n_waves)
    desc = np.zeros(n, _DESC)
    parts = []   # (offset, uint8 array)
    plan = JpegPlan()
    coef_at = plane_at = out_at = 0
    offs = []
    for i, r in enumerate(records):
        d = desc[i]
        d["width"], d["height"], d["ncomp"], d["hs"], d["vs"] = r.width, r.height, r.ncomp, r.hs, r.vs
        d["mcus_x"], d["mcus_y"], d["restart"], d["n_intervals"] = r.mcus_x, r.mcus_y, r.restart, len(r.intervals)
        placed = {}
        for c, (_, _, _, tq, td, ta) in enumerate(r.components):
            for field, key, arr in (("qt_off", ("q", tq), r.qtables[tq]), ("dc_off", (0, td), r.huffman[(0, td)]), ("ac_off", (1, ta), r.huffman[(1, ta)])):
                if key not in placed:
                    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
                    placed[key] = at
                    parts.append((at, raw))
                    at = _align16(at + raw.size)
                d[field][c] = placed[key]
        raw = np.ascontiguousarray(r.intervals, np.int32).view(np.uint8).reshape(-1)
        d["interval_off"] = at
        parts.append((at, raw))
        at = _align16(at + raw.size)
        d["stream_off"], d["stream_len"] = at, r.scan[1] - r.scan[0]
        parts.append((at, np.frombuffer(r.data, np.uint8, r.scan[1] - r.scan[0], r.scan[0])))
        at = _align16(at + r.scan[1] - r.scan[0])
        d["coef_block0"], d["plane_off"] = coef_at, plane_at
        coef_at, plane_at = coef_at + r.blocks, plane_at + r.blocks * 64
        off = out_at if out_offsets is None else int(out_offsets[i])
        d["out_off"] = off
        offs.append(off)
        out_at = _align16(off + r.width * r.height * 3)
    plan.sub_bytes = plan.min_sync_bytes = plan.jobs_off = plan.n_jobs = plan.scratch_bytes = 0
    plan.jobs = []
    if sync is not None:
        sub_bytes, min_sync_bytes = (int(v) for v in sync)
        if sub_bytes % 4 or not SYNC_SUB_MIN <= sub_bytes <= SYNC_SUB_MAX:
            raise ValueError(f"sub_bytes must be a multiple of 4 in {SYNC_SUB_MIN}..{SYNC_SUB_MAX}, not {sub_bytes}")
        if min_sync_bytes < 1:
            raise ValueError(f"min_sync_bytes must be at least 1, not {min_sync_bytes}")
        wave = 0
        for r in records:
            for first, last in r.intervals.tolist():
                if last - first >= min_sync_bytes:
                    n_sub = -(-(last - first) // sub_bytes)
                    plan.jobs.append((wave, n_sub, plan.scratch_bytes))
                    plan.scratch_bytes += SYNC_JOB_HDR_BYTES + SYNC_SUB_RECORD_BYTES * n_sub
                wave += 1
        plan.sub_bytes, plan.min_sync_bytes, plan.jobs_off, plan.n_jobs = sub_bytes, min_sync_bytes, at, len(plan.jobs)
        if plan.jobs:
            parts.append((at, np.array(plan.jobs, _JOB).view(np.uint8).reshape(-1)))
        at = _align16(at + _JOB.itemsize * len(plan.jobs))
    if at >= 1 << 31:
        raise ValueError("batch too large for one blob (2 GiB of compressed data)")
    blob = np.zeros(at, np.uint8) if reserve is None else reserve(at)
    hdr = np.zeros(1, _HDR)
    hdr["n_images"], hdr["n_waves"], hdr["desc_off"], hdr["wave_off"] = n, n_waves, desc_off, wave_off
    blob[:_HDR.itemsize] = hdr.view(np.uint8).reshape(-1)
    blob[desc_off:desc_off + desc.nbytes] = desc.view(np.uint8).reshape(-1)
    waves = np.concatenate([np.stack([np.full(len(r.intervals), i, np.int32), np.arange(len(r.intervals), dtype=np.int32)], 1)
                            for i, r in enumerate(records)])
    blob[wave_off:wave_off + waves.nbytes] = waves.view(np.uint8).reshape(-1)
    for off, raw in parts:
        blob[off:off + raw.size] = raw
    plan.blob, plan.nbytes, plan.n_waves = blob, at, n_waves
    plan.coef_blocks, plan.plane_bytes = coef_at, plane_at
    plan.out_bytes = out_at if out_bytes is None else int(out_bytes)
    plan.out_offsets, plan.sizes = offs, [(r.height, r.width) for r in records]
    return plan


def _launch(records, out_offsets, out_bytes, dev, events=None, sync=None, info=None):
    """The device call of ``decode_jpeg_batch``: plan into the pinned staging buffer, check, upload in one copy, run the three stages
    on the current stream.  Returns (uint8 [out_bytes] device tensor, freshly allocated; int32 status per record, on the host - reading
    it is the one synchronisation of the batch).  ``sync`` = (sub_bytes, min_sync_bytes): ``hawq_jpeg_decode_batch_sync``; a dict
    ``info`` then receives ``jobs`` (the plan's) and ``rounds`` / ``decodes`` (what the kernel counted per job)."""
    from .image import _STAGING, _Staging
    lib = _lib.load()
    with torch.cuda.device(dev):
        st = _STAGING.setdefault((dev.index, "jpeg"), _Staging())
        held = {}

        def reserve(nbytes):
            held["host"], held["dev"] = st.reserve(nbytes, dev)
            return held["host"].numpy()

        plan = plan_jpeg_batch(records, out_offsets, out_bytes, reserve, sync)
        if not plan.ok() or (sync is not None and not plan.sync_ok()):   # on the host blob, before anything is uploaded or launched
            raise RuntimeError("libhawq_mi355: " + lib.hawq_last_error().decode())
        st.upload(plan.nbytes)
        out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
        coef = torch.empty(plan.coef_blocks * 64, dtype=torch.int16, device=dev)
        planes = torch.empty(plan.plane_bytes, dtype=torch.uint8, device=dev)
        status = torch.empty(len(records), dtype=torch.int32, device=dev)
        ev = (C.c_void_p * 4)(*events) if events is not None else None
        if sync is None:
            _lib.call("hawq_jpeg_decode_batch", held["dev"].data_ptr(), plan.blob.ctypes.data, plan.nbytes, coef.data_ptr(), plan.coef_blocks,
                      planes.data_ptr(), plan.plane_bytes, out.data_ptr(), out_bytes, status.data_ptr(), ev,
                      torch.cuda.current_stream(dev).cuda_stream)
            return out, status.cpu().numpy()
        scratch = torch.empty(max(plan.scratch_bytes, 16), dtype=torch.uint8, device=dev)
        _lib.call("hawq_jpeg_decode_batch_sync", held["dev"].data_ptr(), plan.blob.ctypes.data, plan.nbytes, coef.data_ptr(), plan.coef_blocks,
                  planes.data_ptr(), plan.plane_bytes, out.data_ptr(), out_bytes, status.data_ptr(), plan.sub_bytes, plan.min_sync_bytes, plan.jobs_off,
                  plan.n_jobs, scratch.data_ptr(), plan.scratch_bytes, ev, torch.cuda.current_stream(dev).cuda_stream)
        status = status.cpu().numpy()
        if info is not None:
            info["jobs"] = list(plan.jobs)
            host = scratch.cpu().numpy()
            heads = [host[off:off + 8].view(np.int32) for _, _, off in plan.jobs]
            info["rounds"], info["decodes"] = [int(h[0]) for h in heads], [int(h[1]) for h in heads]
        return out, status


def read_source(source) -> bytes:
    """A path, bytes or a binary file object -> the file's bytes."""
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source)
    if hasattr(source, "read"):
        return source.read()
    with open(source, "rb") as f:
        return f.read()


def decode_jpeg_batch(sources, device=None, entropy="serial", sub_bytes=None, min_sync_bytes=None):
    """Paths or bytes of image files -> ``(images, fallbacks)``: ``images[i]`` a uint8 [H, W, 3] RGB tensor on the MI355X equal to
    ``image.decode_image(sources[i])``, ``fallbacks`` the list of ``(index, reason)`` of the images the HOST decoder produced: files
    ``parse_jpeg`` refuses (progressive, CMYK, not a JPEG, ...) and files whose device decode reported a status (damaged streams).
    All images are views into one device allocation made by this call, at 16-byte aligned offsets, so ``preprocess_batch_fused`` reads
    them in place.  An error of the host decoder on such a file propagates as it does from ``decode_image``.
    ``entropy``: ``"serial"`` decodes every restart interval with one wave; ``"sync"`` decodes intervals of at least ``min_sync_bytes``
    stream bytes with one lane per ``sub_bytes`` of them (``hawq_jpeg_decode_batch_sync``; defaults ``MIN_SYNC_BYTES`` / ``SUB_BYTES``) -
    the same bytes and the same fallbacks, faster on files without restart markers."""
    from .image import decode_image
    if entropy not in ("serial", "sync"):
        raise ValueError(f"entropy must be 'serial' or 'sync', not {entropy!r}")
    if entropy == "serial" and (sub_bytes is not None or min_sync_bytes is not None):
        raise ValueError("sub_bytes / min_sync_bytes belong to entropy='sync'")
    more = {} if entropy == "serial" else {"sync": (SUB_BYTES if sub_bytes is None else int(sub_bytes), MIN_SYNC_BYTES if min_sync_bytes is None else int(min_sync_bytes))}
    datas = [read_source(s) for s in sources]
    if not datas:
        raise ValueError("empty batch")
    dev = torch.device("cuda" if device is None else device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    records, fallbacks, host = {}, [], {}
    for i, data in enumerate(datas):
        try:
            records[i] = parse_jpeg(data)
        except UnsupportedJpeg as e:
            fallbacks.append((i, e.reason))
            host[i] = decode_image(data)
    sizes = [(records[i].height, records[i].width) if i in records else tuple(host[i].shape[:2]) for i in range(len(datas))]
    offsets, total = [], 0
    for h, w in sizes:
        offsets.append(total)
        total = _align16(total + h * w * 3)
    order = sorted(records)
    if order:
        out, status = _launch([records[i] for i in order], [offsets[i] for i in order], total, dev, **more)
        for i, st in zip(order, status):
            if st != 0:
                fallbacks.append((i, "device status %d: %s" % (st, STATUS_NAMES.get(int(st), "unknown"))))
                host[i] = decode_image(datas[i])
                if tuple(host[i].shape[:2]) != sizes[i]:
                    raise RuntimeError(f"image {i}: the host decoder gives {tuple(host[i].shape[:2])}, the header {sizes[i]}")
    else:
        out = torch.empty(total, dtype=torch.uint8, device=dev)
    for i, im in host.items():
        out[offsets[i]:offsets[i] + im.numel()].copy_(im.reshape(-1))
    images = [out[offsets[i]:offsets[i] + h * w * 3].view(h, w, 3) for i, (h, w) in enumerate(sizes)]
    return images, sorted(fallbacks)
