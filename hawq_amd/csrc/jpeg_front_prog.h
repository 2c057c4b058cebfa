// The device front end for progressive files: the marker walk of hawq_amd/jpeg.py with `progressive=True` (`_parse`
// from the SOF2 on, `_progressive_scan_header`, the progression rule over state[3][64], `scan_levels`, `_accept_frame` and
// `_Markers.entropy_segment` per scan) as plain C++ beside the baseline walker of jpeg_front.h, for the device (jpeg_front.hip: one wave
// per file) and for the host (hawq_jpeg_front_scan_prog_host; tools/jpeg_front_prog_check.cpp runs this very text under the sanitizers).
//
// A file is walked as a baseline one first (walk_header / walk_scan, untouched); what that walk refuses is walked here.  Like it, this
// walk accepts a subset of what `parse_jpeg(data, progressive=True)` accepts and gives no reasons.
//
// Bounds: every read is `b[i]` with 0 <= i < n.  The walk ends after HAWQ_JPEG_FRONT_PROG_MAX_SEGMENTS marker segments and
// HAWQ_JPEG_PROG_MAX_SCANS scans; the loops of a scan header run over at most 3 components and 64 coefficients; every other inner loop
// is bounded by a segment's length.
#pragma once
#include "jpeg_front.h"

namespace hawq_jpeg_front {
// The walk between the scans of a file.  On the device it lives in LDS: the tables are indexed with ids and coefficients read from
// the file.
struct prog_walk {
    int64_t pos;            // the next marker
    int32_t sof;            // the SOF2 segment as `sof` of walk_header, 0 before it: the file counts as baseline until then
    int32_t ncomp, restart, segments, n_scans, adobe;
    int32_t huff_at[8];     // [class * 4 + id]: file offset of BITS of the table in force, 0: none
    int32_t state[3][64];   // per (component, coefficient): the Al reached, -1 before its first scan
    int32_t level[3][64];   // the level of the last scan that covered it, 0 before one
};
constexpr int32_t PROG_SCAN = 0, PROG_END = -1;

HAWQ_FRONT_HD void prog_begin(prog_walk &w) {
    w.pos = 2, w.sof = w.ncomp = w.restart = w.segments = w.n_scans = w.adobe = 0;
    for (int k = 0; k < 8; ++k) w.huff_at[k] = 0;
}

// The SOS segment b[seg .. seg + len) of a progressive file: limits, its step in the progression (w.state and w.level advance), the
// tables in force.  Fills `s` but restart, n_intervals and the segment's bounds; `units`: what its restart interval counts.
HAWQ_FRONT_HD int32_t prog_scan_header(const uint8_t *b, int64_t seg, int64_t len, prog_walk &w, const hawq_jpeg_front_info &o, hawq_jpeg_front_scan_rec &s,
                                       int32_t &units) {
    const int32_t refused = HAWQ_JPEG_FRONT_REFUSED;
    if (len < 1 || len != 4 + 2 * (int64_t)b[seg]) return refused;
    const int ns = b[seg];
    int comp0 = 0;
    if (ns == w.ncomp) {   // all components in frame order
        for (int i = 0; i < ns; ++i)
            if (b[seg + 1 + 2 * i] != b[w.sof + 6 + 3 * i]) return refused;
    } else if (ns == 1) {
        comp0 = -1;
        for (int i = w.ncomp - 1; i >= 0; --i)
            if (b[seg + 1] == b[w.sof + 6 + 3 * i]) comp0 = i;
        if (comp0 < 0) return refused;
    } else {
        return refused;    // two of three, or more than the frame has
    }
    const int ss = b[seg + len - 3], se = b[seg + len - 2], ah = b[seg + len - 1] >> 4, al = b[seg + len - 1] & 15;
    if (ss > se || se > 63 || (ss == 0 && se != 0)) return refused;
    if (ss > 0 && ns != 1) return refused;
    if (al > 13 || (ah != 0 && ah != al + 1)) return refused;
    // a first scan (Ah = 0) of cells never coded, or a refinement of cells whose last scan stopped at Al = Ah; the DC before any AC
    const int32_t before = ah ? ah : -1;
    int32_t level = 0;
    for (int c = comp0; c < comp0 + ns; ++c)
        for (int k = ss; k <= se; ++k) {
            if (w.state[c][k] != before) return refused;
            level = w.level[c][k] > level ? w.level[c][k] : level;
        }
    if (ss > 0 && w.state[comp0][0] < 0) return refused;
    ++level;
    for (int c = comp0; c < comp0 + ns; ++c)
        for (int k = ss; k <= se; ++k) w.state[c][k] = al, w.level[c][k] = level;
    s.dc_at[0] = s.dc_at[1] = s.dc_at[2] = s.ac_at = 0;
    for (int i = 0; i < ns; ++i)
        if ((b[seg + 2 + 2 * i] >> 4) > 3 || (b[seg + 2 + 2 * i] & 15) > 3) return refused;
    if (ss == 0 && ah == 0)
        for (int i = 0; i < ns; ++i) {
            const int32_t at = w.huff_at[b[seg + 2 + 2 * i] >> 4];
            if (!at) return refused;   // missing table
            s.dc_at[i] = at;
        }
    if (ss > 0) {
        s.ac_at = w.huff_at[4 + (b[seg + 2] & 15)];
        if (!s.ac_at) return refused;
    }
    s.ncomp = ns, s.comp0 = comp0, s.ss = ss, s.se = se, s.ah = ah, s.al = al, s.level = level;
    if (ns > 1) {   // MCUs
        units = ((o.width + 8 * o.hs - 1) / (8 * o.hs)) * ((o.height + 8 * o.vs - 1) / (8 * o.vs));
    } else {        // the blocks its own samples need, not the MCU-padded grid
        const int h = b[w.sof + 7 + 3 * comp0] >> 4, v = b[w.sof + 7 + 3 * comp0] & 15;
        const int32_t cw = (o.width * h + o.hs - 1) / o.hs, ch = (o.height * v + o.vs - 1) / o.vs;
        units = ((cw + 7) / 8) * ((ch + 7) / 8);
    }
    return PROG_SCAN;
}

// From the marker at w.pos to the next SOS, its header included: PROG_SCAN with `s` filled but n_intervals and scan_end, and `units`;
// PROG_END at the EOI behind the last scan of a complete progression; else the defer code.  The frame's fields of `o` are filled on the
// way; the caller sets w.pos behind the scan's entropy-coded segment and counts the scan.
HAWQ_FRONT_HD int32_t prog_next(const uint8_t *b, int64_t n, prog_walk &w, hawq_jpeg_front_info &o, hawq_jpeg_front_scan_rec &s, int32_t &units) {
    const int32_t refused = HAWQ_JPEG_FRONT_REFUSED;
    if (n > HAWQ_JPEG_FRONT_MAX_BYTES) return HAWQ_JPEG_FRONT_TOO_LARGE;
    if (n < 4 || b[0] != 0xFF || b[1] != 0xD8) return refused;
    for (;;) {
        int64_t pos = w.pos;
        if (pos + 2 > n || b[pos] != 0xFF) return refused;
        while (b[pos + 1] == 0xFF) {   // fill bytes
            ++pos;
            if (pos + 2 > n) return refused;
        }
        const int marker = b[pos + 1];
        pos += 2;
        w.pos = pos;
        if (marker == 0xD9) {
            if (!w.n_scans) return refused;   // no scan
            for (int c = 0; c < w.ncomp; ++c)
                for (int k = 0; k < 64; ++k)
                    if (w.state[c][k] != 0) return refused;   // something never coded, or not down to Al = 0
            return PROG_END;
        }
        if (w.n_scans && !(marker == 0xC4 || marker == 0xDD || marker == 0xFE || marker == 0xDA || (marker >= 0xE0 && marker <= 0xEF))) return refused;
        if (marker == 0xD8 || marker == 0x01 || (marker >= 0xD0 && marker <= 0xD7)) continue;
        if (pos + 2 > n) return refused;
        const int64_t length = ((int64_t)b[pos] << 8) | b[pos + 1];
        if (length < 2 || pos + length > n) return refused;
        const int64_t seg = pos + 2, len = length - 2;
        pos += length;
        w.pos = pos;
        if (++w.segments > HAWQ_JPEG_FRONT_PROG_MAX_SEGMENTS) return HAWQ_JPEG_FRONT_LONG_HEADER;
        if (marker == 0xC2) {
            if (w.sof) return refused;   // several frames
            if (len < 6 || len != 6 + 3 * (int64_t)b[seg + 5] || b[seg] != 8) return refused;
            o.height = (b[seg + 1] << 8) | b[seg + 2], o.width = (b[seg + 3] << 8) | b[seg + 4];
            if (o.height == 0 || o.width == 0 || (b[seg + 5] != 1 && b[seg + 5] != 3)) return refused;
            w.ncomp = b[seg + 5], w.sof = (int32_t)seg;
        } else if (marker >= 0xC0 && marker <= 0xCF && marker != 0xC4 && marker != 0xC8) {
            return refused;   // a baseline frame (the other walk's), another kind of frame, a second one, arithmetic coding
        } else if (marker == 0xC4) {
            for (int64_t at = 0; at < len;) {
                if (at + 17 > len) return refused;
                const int tc = b[seg + at] >> 4, th = b[seg + at] & 15;
                int32_t count = 0;
                for (int k = 1; k <= 16; ++k) count += b[seg + at + k];
                if (tc > 1 || at + 17 + count > len || th > (w.sof ? 3 : 1)) return refused;
                if (huffman_values(b, seg + at + 1) < 0) return refused;
                w.huff_at[tc * 4 + th] = (int32_t)(seg + at + 1);
                at += 17 + count;
            }
        } else if (marker == 0xDB) {
            for (int64_t at = 0; at < len; at += 65) {
                const int pq = b[seg + at] >> 4, tq = b[seg + at] & 15;
                if (pq != 0 || tq > 3 || at + 65 > len) return refused;
                o.qt_at[tq] = (int32_t)(seg + at + 1);
            }
        } else if (marker == 0xDD) {
            if (len != 2) return refused;
            w.restart = (b[seg] << 8) | b[seg + 1];
        } else if (marker == 0xDC) {
            return refused;   // DNL
        } else if (marker == 0xEE) {
            w.adobe = w.adobe || (len >= 5 && b[seg] == 'A' && b[seg + 1] == 'd' && b[seg + 2] == 'o' && b[seg + 3] == 'b' && b[seg + 4] == 'e');
        } else if (marker == 0xDA) {
            if (!w.sof) return refused;   // a scan before the SOF2: the baseline walk's, which has refused it
            if (!w.n_scans) {             // the first SOS: the frame both kinds must have
                if (w.adobe) return refused;
                o.tq[0] = o.tq[1] = o.tq[2] = 0;
                for (int i = 0; i < w.ncomp; ++i) {
                    const int id = b[w.sof + 6 + 3 * i], hv = b[w.sof + 7 + 3 * i], tq = b[w.sof + 8 + 3 * i];
                    if (tq > 3 || !o.qt_at[tq]) return refused;   // missing table
                    o.tq[i] = tq;
                    if (w.ncomp == 3 && id != i + 1) return refused;                                                         // component ids 1, 2, 3
                    if (i == 0 ? !(hv == 0x11 || (w.ncomp == 3 && (hv == 0x21 || hv == 0x22))) : hv != 0x11) return refused;   // sampling factors
                }
                if (o.width > MAX_SIDE || o.height > MAX_SIDE) return refused;
                o.ncomp = w.ncomp, o.hs = b[w.sof + 7] >> 4, o.vs = b[w.sof + 7] & 15;
                for (int c = 0; c < 3; ++c)
                    for (int k = 0; k < 64; ++k) w.state[c][k] = -1, w.level[c][k] = 0;
            }
            if (w.n_scans == HAWQ_JPEG_PROG_MAX_SCANS) return refused;   // too many scans
            const int32_t defer = prog_scan_header(b, seg, len, w, o, s, units);
            if (defer) return defer;
            s.restart = w.restart, s.scan_first = (int32_t)pos;
            return PROG_SCAN;
        }
        // APPn, COM and whatever else carries a length: skipped
    }
}

// RSTn markers a scan of `units` units holds
HAWQ_FRONT_HD int32_t prog_expected_restarts(int32_t units, int32_t restart) { return restart ? (units + restart - 1) / restart - 1 : 0; }

// The serial form of a scan's entropy-coded segment (the kernel does the same with all lanes): from s.scan_first on, the RSTn markers
// count modulo 8 from RST0, the first other marker ends the segment, and there are exactly `expected` RSTn before it.
HAWQ_FRONT_HD int32_t prog_segment(const uint8_t *b, int64_t n, hawq_jpeg_front_scan_rec &s, int32_t expected) {
    int32_t rank = 0;
    for (int64_t i = s.scan_first; i + 1 < n; ++i) {
        if (!is_marker(b[i], b[i + 1])) continue;
        const int code = b[i + 1];
        if ((code & 0xF8) == 0xD0) {
            if ((code & 7) != (rank & 7)) return HAWQ_JPEG_FRONT_REFUSED;
            ++rank;
            continue;
        }
        if (rank != expected) return HAWQ_JPEG_FRONT_REFUSED;
        s.scan_end = (int32_t)i, s.n_intervals = expected + 1;
        return 0;
    }
    return HAWQ_JPEG_FRONT_REFUSED;   // truncated scan
}

// The record of a file the progressive walk has finished with `code` (PROG_END or a defer code) after `n_scans` scans
HAWQ_FRONT_HD void prog_finish(hawq_jpeg_front_info &o, hawq_jpeg_front_scan_rec *scans, int32_t n_scans, int32_t code) {
    if (code == PROG_END) {
        o.reserved[0] = HAWQ_JPEG_FRONT_KIND_PROG, o.reserved[1] = n_scans;
        return;
    }
    clear(o, code);
    for (int32_t k = 0; k < n_scans; ++k) scans[k] = hawq_jpeg_front_scan_rec{};
}

// One file on the host: the twin of the kernel.  `scans`: the file's HAWQ_JPEG_PROG_MAX_SCANS records, zero on entry.
HAWQ_FRONT_HD void walk_file_prog(const uint8_t *b, int64_t n, hawq_jpeg_front_info &o, hawq_jpeg_front_scan_rec *scans, prog_walk &w) {
    walk_file(b, n, o);
    if (o.defer != HAWQ_JPEG_FRONT_REFUSED) return;   // a baseline file, or a bound of the kernel
    clear(o, 0);
    prog_begin(w);
    int32_t code;
    for (;;) {
        hawq_jpeg_front_scan_rec s = hawq_jpeg_front_scan_rec{};
        int32_t units = 0;
        code = prog_next(b, n, w, o, s, units);
        if (code == PROG_SCAN) code = prog_segment(b, n, s, prog_expected_restarts(units, s.restart));
        if (code != PROG_SCAN) break;
        scans[w.n_scans++] = s;
        w.pos = s.scan_end;
    }
    prog_finish(o, scans, w.n_scans, code);
}
}  // namespace hawq_jpeg_front
