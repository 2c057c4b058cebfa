"""What the host front end of the device JPEG decoder (hawq_amd/jpeg.py) does, recorded so that a change to it can be checked against
what it did before: the outcome of ``parse_jpeg`` on mutated fixture files, and the blob bytes of the two planners.
tests/golden/make_jpeg_front_end_pins.py writes both as JSON, tests/test_jpeg_front_end_pins.py compares.

Parser.  A file is cut into units by a walker of its own (``units``; it shares nothing with the parser): SOI, every marker segment,
every scan header, the entropy-coded bytes behind a scan header ("ecs"), EOI, and whatever it cannot read ("tail" / "file").  Per unit:
deletion, duplication, and truncation at its end and one byte either side; per byte of a unit outside the entropy-coded bytes, and of
the first two entropy-coded bytes (the two bytes behind the scan header's end), the values 0x00, 0xFF and byte ^ 0x10.  Every input is
parsed with and without ``progressive=True``; an outcome is the refusal's reason or a digest of every slot of the record.
``BYTE_FIXTURES`` get all of this; every other fixture below 1500 bytes and every other refused file gets the structural mutations only,
under one digest: the files of one encoder share their tables byte for byte, so their header bytes say the same thing a hundred times,
at 0.1 ms per parse.
"""
import functools
import hashlib

import numpy as np

from tests import jpeg_model, jpeg_prog_model, jpeg_sync_model

SMALL = 1500
# mutated byte by byte.  Baseline: 4:4:4, 4:2:2, 4:2:0 with restart markers, gray; progressive: gray,
# tables redefined between scans (4:2:2), the deepest progression (4:2:0), restart markers; the refused files that are short
BYTE_FIXTURES = {"base": ["smooth_8x8_444", "smooth_1x1_422", "noise_1x1_420rst", "noise_13x17_gray", "refused_png", "refused_cut_header"],
                 "prog": ["noise_1x1_gray", "tables_13x17_422", "deep_33x31_420", "noise_40x24_gray_rst", "refused_two_components"]}
STANDALONE = (0x01, 0xD8, 0xD9) + tuple(range(0xD0, 0xD8))


def units(data):
    """[(label, first, end, bytes to mutate from first)] covering ``data``"""
    n = len(data)
    if data[:2] != b"\xff\xd8":
        return [("file", 0, n, n)]
    out, pos, seen = [("SOI", 0, 2, 2)], 2, {}

    def label(name):
        seen[name] = seen.get(name, 0) + 1
        return "%s.%d" % (name, seen[name] - 1)

    while pos < n:
        if pos + 2 > n or data[pos] != 0xFF or data[pos + 1] in (0x00, 0xFF) or (data[pos + 1] not in STANDALONE and pos + 4 > n):
            out.append((label("tail"), pos, n, n - pos))
            break
        marker = data[pos + 1]
        end = pos + 2 if marker in STANDALONE else min(n, pos + 2 + ((data[pos + 2] << 8) | data[pos + 3]))
        out.append((label("%02X" % marker), pos, end, end - pos))
        pos = end
        if marker == 0xDA:   # the entropy-coded bytes: up to the first FF that no 00, FF or RSTn follows
            end = pos
            while end < n and not (data[end] == 0xFF and end + 1 < n and data[end + 1] not in (0x00, 0xFF) and not 0xD0 <= data[end + 1] <= 0xD7):
                end += 1
            out.append((label("ecs"), pos, end, min(2, end - pos)))
            pos = end
    return out


def mutations(data, first, end, n_bytes):
    """the mutated files of one unit, in a fixed order"""
    for at in range(first, first + n_bytes):
        for value in (0x00, 0xFF, data[at] ^ 0x10):
            if value != data[at]:
                yield data[:at] + bytes([value]) + data[at + 1:]
    for cut in (end - 1, end, end + 1):
        if cut < len(data):
            yield data[:cut]
    yield data[:first] + data[end:]
    yield data[:end] + data[first:end] + data[end:]


def _sha(raw):
    return hashlib.sha256(raw).hexdigest()


def _plain(value, tables=None):
    """a value of a record as text; ``tables``: {id: index} for the Huffman tables of scans, which count by content and by identity"""
    if type(value) is int:
        return "int %d" % value
    if isinstance(value, np.ndarray):
        text = "array(%s, %s, %s)" % (value.dtype.str, value.shape, _sha(np.ascontiguousarray(value).tobytes()))
        return text if tables is None else "%s#%d" % (text, tables.setdefault(id(value), len(tables)))
    if isinstance(value, (bytes, bytearray)):
        return "bytes(%d, %s)" % (len(value), _sha(bytes(value)))
    if isinstance(value, dict):
        return "{%s}" % ", ".join("%r: %s" % (k, _plain(value[k], tables)) for k in sorted(value))
    if isinstance(value, (list, tuple)):
        return "%s(%s)" % (type(value).__name__, ", ".join(_plain(v, tables) for v in value))
    if hasattr(type(value), "__slots__"):
        return record_text(value, tables)
    return "%s %r" % (type(value).__name__, value)


def record_text(rec, tables=None):
    """every slot of a ``JpegRecord`` / ``JpegProgRecord`` / ``JpegScan``"""
    tables = {} if tables is None else tables
    parts = []
    for slot in type(rec).__slots__:
        value = getattr(rec, slot, "unset")
        parts.append("%s=%s" % (slot, _plain(value, tables if slot in ("dc", "ac", "scans") else None)))
    return "%s(%s)" % (type(rec).__name__, "; ".join(parts))


def outcome(data, progressive):
    from hawq_amd.jpeg import UnsupportedJpeg, parse_jpeg
    try:
        rec = parse_jpeg(data, progressive=True) if progressive else parse_jpeg(data)
    except UnsupportedJpeg as e:
        return "refused: " + e.reason
    except Exception as e:   # not expected; pinned as well
        return "error: " + type(e).__name__
    return "accepted: " + _sha(record_text(rec).encode())


def fixtures():
    """{name: (file bytes, whether its bytes are mutated one by one)} in a fixed order"""
    base, base_bad, _ = jpeg_model.cases()
    prog, prog_bad, _ = jpeg_prog_model.cases()
    out = {}
    for kind, good, bad in (("base", base, base_bad), ("prog", prog, prog_bad)):
        for name in sorted(good):
            if len(good[name][0]) < SMALL or name in BYTE_FIXTURES[kind]:
                out["%s/%s" % (kind, name)] = (good[name][0], name in BYTE_FIXTURES[kind])
        for name in sorted(bad):
            out["%s/refused_%s" % (kind, name)] = (bad[name][0], "refused_" + name in BYTE_FIXTURES[kind])
    return out


def parser_pins():
    """{"fixtures": {name: {"units": {label: SHA-256 over the ordered outcomes of its mutations}, "outcomes": {reason | "accepted": count}}},
    "structural": {name: one SHA-256 over all its units}, "structural_outcomes": {"base" | "prog": the histogram over those fixtures},
    "inputs", "accepted" (inputs that one of the two calls accepts), "reasons" (distinct ones)}"""
    pins = {"fixtures": {}, "structural": {}, "structural_outcomes": {"base": {}, "prog": {}}, "inputs": 0, "accepted": 0}
    for name, (data, every_byte) in fixtures().items():
        per_unit, h = {}, hashlib.sha256()
        histogram = {} if every_byte else pins["structural_outcomes"][name[:4]]
        h.update((outcome(data, False) + "\n" + outcome(data, True) + "\n").encode())   # the file as it is
        for label, first, end, n_bytes in units(data):
            if every_byte:
                h = per_unit[label] = hashlib.sha256()
            for mutated in mutations(data, first, end, n_bytes if every_byte else 0):
                both = [outcome(mutated, progressive) for progressive in (False, True)]
                for got in both:
                    h.update(got.encode() + b"\n")
                    key = "accepted" if got.startswith("accepted: ") else got
                    histogram[key] = histogram.get(key, 0) + 1
                pins["inputs"] += 1
                pins["accepted"] += any(got.startswith("accepted: ") for got in both)
        if every_byte:
            pins["fixtures"][name] = {"units": {label: v.hexdigest() for label, v in per_unit.items()}, "outcomes": dict(sorted(histogram.items()))}
        else:
            pins["structural"][name] = h.hexdigest()
    histograms = [f["outcomes"] for f in pins["fixtures"].values()] + list(pins["structural_outcomes"].values())
    pins["reasons"] = len({k for hist in histograms for k in hist if k.startswith("refused: ")})
    pins["structural_outcomes"] = {k: dict(sorted(v.items())) for k, v in pins["structural_outcomes"].items()}
    return pins


@functools.lru_cache(maxsize=None)
def _records():
    from hawq_amd.jpeg import parse_jpeg
    base = {n: parse_jpeg(d) for n, (d, _) in jpeg_model.cases()[0].items()}
    sync = {n: parse_jpeg(d) for n, (d, _) in jpeg_sync_model.cases()[0].items()}
    prog = {n: parse_jpeg(d, progressive=True) for n, (d, _) in jpeg_prog_model.cases()[0].items()}
    return base, sync, prog


def _plan_pin(plan):
    """nbytes, the blob's bytes and every other attribute of the plan"""
    rest = {slot: getattr(plan, slot) for slot in sorted(s for c in type(plan).__mro__ for s in getattr(c, "__slots__", ())) if slot != "blob"}
    return {"nbytes": int(plan.nbytes), "blob": _sha(plan.blob[:plan.nbytes].tobytes()), "fields": _sha(repr(rest).encode())}


def planner_pins():
    """{label: {"nbytes", "blob": SHA-256 of blob[:nbytes], "fields": SHA-256 of the plan's other attributes}}"""
    from hawq_amd.jpeg import plan_jpeg_batch, plan_jpeg_prog_batch, record_resume_points
    base, sync, prog = _records()
    pins = {"base/all": _plan_pin(plan_jpeg_batch(list(base.values())))}
    for name in ("noise_13x17_420", "noise_40x24_rst4", "smooth_31x33_gray"):
        pins["base/" + name] = _plan_pin(plan_jpeg_batch([base[name]]))
    for pair in ((16, 256), (32, 4096)):
        pins["sync%d_%d/all" % pair] = _plan_pin(plan_jpeg_batch(list(sync.values()), sync=pair))
        for name in ("flat_320x240", "noise_96x64_rstrow", "noise_64x48_422"):
            pins["sync%d_%d/%s" % (pair + (name,))] = _plan_pin(plan_jpeg_batch([sync[name]], sync=pair))
    pins["prog/all"] = _plan_pin(plan_jpeg_prog_batch(list(prog.values())))
    pins["prog/noise_16x16_420"] = _plan_pin(plan_jpeg_prog_batch([prog["noise_16x16_420"]]))
    # images placed out of order, with gaps between them and behind the last
    some = [base[n] for n in ("noise_31x33_422", "noise_40x24_rst4", "smooth_31x33_gray", "noise_16x16_444")]
    pins["base/placed"] = _plan_pin(plan_jpeg_batch(some, [12288, 32, 8192, 4112], 20000))
    pins["sync32_64/placed"] = _plan_pin(plan_jpeg_batch(some, [12288, 32, 8192, 4112], 20000, sync=(32, 64)))
    # the segment table behind the streams, from resume points recorded every 16 stream bytes
    pins["resume16/all"] = _plan_pin(plan_jpeg_batch(list(base.values()), resume=[record_resume_points(r, 16) for r in base.values()]))
    pins["resume16/placed"] = _plan_pin(plan_jpeg_batch(some, [12288, 32, 8192, 4112], 20000, resume=[record_resume_points(r, 16) for r in some]))
    some = [prog[n] for n in ("noise_40x24_420_rst", "noise_7x9_gray", "tables_13x17_422")]
    pins["prog/placed"] = _plan_pin(plan_jpeg_prog_batch(some, [8192, 48, 4096], 16384))
    return pins
