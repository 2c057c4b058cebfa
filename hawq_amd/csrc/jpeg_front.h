// The device front end of the baseline JPEG decoder: the marker walk of hawq_amd/jpeg.py (`_parse` without
// `progressive`, with `_frame_header`, `_huffman_tables`, `_quantisation_tables`, `_baseline_scan_header`, `_accept_frame` and
// `_Markers.entropy_segment`) as plain C++ that compiles for the device (jpeg_front.hip: one wave per file) and for the host
// (hawq_jpeg_front_scan_host; tools/jpeg_front_check.cpp runs this very text under the sanitizers).
//
// It accepts a strict subset of what `parse_jpeg(data)` accepts and never says why it does not: anything else gets a defer code, and
// the file goes to the Python parser, which accepts or refuses it with its reason as before.
//
// Bounds: every read is `b[i]` with 0 <= i < n, the file's own length.  The header loop ends after HAWQ_JPEG_FRONT_MAX_SEGMENTS
// marker segments; every inner loop is bounded by a segment's length.
#pragma once
#include <stdint.h>

#include "../../include/hawq_mi355.h"

#if defined(__HIPCC__)
#define HAWQ_FRONT_HD __host__ __device__ inline
#else
#define HAWQ_FRONT_HD inline
#endif

namespace hawq_jpeg_front {
constexpr int MAX_SIDE = 8192;

// FF xx with xx neither stuffing (00) nor fill (FF): the local marker test of an entropy-coded segment
HAWQ_FRONT_HD bool is_marker(uint8_t b0, uint8_t b1) { return b0 == 0xFF && b1 != 0x00 && b1 != 0xFF; }

// BITS of a DHT table at b[at .. at + 16): the number of values when the counts are a code (T.81 C.2: no length holds more codes than
// it has room for) with 1..256 values, else -1
HAWQ_FRONT_HD int32_t huffman_values(const uint8_t *b, int64_t at) {
    int32_t code = 0, k = 0;
    for (int length = 1; length <= 16; ++length) {
        const int32_t c = b[at + length - 1];
        if (c) {
            code += c, k += c;
            if (code > (1 << length)) return -1;
        }
        code <<= 1;
    }
    return k == 0 || k > 256 ? -1 : k;
}

// The walk up to and including the SOS segment.  Fills everything of `o` but n_intervals and scan_end and returns 0 with
// o.scan_first = the first byte behind the scan header, or returns the defer code.
HAWQ_FRONT_HD int32_t walk_header(const uint8_t *b, int64_t n, hawq_jpeg_front_info &o) {
    const int32_t refused = HAWQ_JPEG_FRONT_REFUSED;
    if (n > HAWQ_JPEG_FRONT_MAX_BYTES) return HAWQ_JPEG_FRONT_TOO_LARGE;
    if (n < 4 || b[0] != 0xFF || b[1] != 0xD8) return refused;
    int64_t sof = 0;      // the frame header's segment: per component i its id, h << 4 | v and quantisation table id at sof + 6 + 3 i
    int32_t ncomp = 0, restart = 0, segments = 0;
    bool adobe = false;
    for (int k = 0; k < 4; ++k) o.qt_at[k] = o.huff_at[k] = 0;
    int64_t pos = 2;
    for (;;) {
        if (pos + 2 > n || b[pos] != 0xFF) return refused;
        while (b[pos + 1] == 0xFF) {   // fill bytes
            ++pos;
            if (pos + 2 > n) return refused;
        }
        const int marker = b[pos + 1];
        pos += 2;
        if (marker == 0xD9) return refused;   // no scan
        if (marker == 0xD8 || marker == 0x01 || (marker >= 0xD0 && marker <= 0xD7)) continue;
        if (pos + 2 > n) return refused;
        const int64_t length = ((int64_t)b[pos] << 8) | b[pos + 1];
        if (length < 2 || pos + length > n) return refused;
        const int64_t seg = pos + 2, len = length - 2;
        pos += length;
        if (++segments > HAWQ_JPEG_FRONT_MAX_SEGMENTS) return HAWQ_JPEG_FRONT_LONG_HEADER;
        if (marker == 0xC0) {
            if (ncomp) return refused;   // several frames
            if (len < 6 || len != 6 + 3 * (int64_t)b[seg + 5] || b[seg] != 8) return refused;
            o.height = (b[seg + 1] << 8) | b[seg + 2], o.width = (b[seg + 3] << 8) | b[seg + 4];
            if (o.height == 0 || o.width == 0 || (b[seg + 5] != 1 && b[seg + 5] != 3)) return refused;
            ncomp = b[seg + 5], sof = seg;
        } else if (marker >= 0xC1 && marker <= 0xCF && marker != 0xC4 && marker != 0xC8) {
            return refused;   // another kind of frame, arithmetic coding (DAC among it)
        } else if (marker == 0xC4) {
            for (int64_t at = 0; at < len;) {
                if (at + 17 > len) return refused;
                const int tc = b[seg + at] >> 4, th = b[seg + at] & 15;
                int32_t count = 0;
                for (int k = 1; k <= 16; ++k) count += b[seg + at + k];
                if (tc > 1 || at + 17 + count > len || th > 1) return refused;
                if (huffman_values(b, seg + at + 1) < 0) return refused;
                o.huff_at[tc * 2 + th] = (int32_t)(seg + at + 1);
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
            restart = (b[seg] << 8) | b[seg + 1];
        } else if (marker == 0xDC) {
            return refused;   // DNL
        } else if (marker == 0xEE) {
            adobe = adobe || (len >= 5 && b[seg] == 'A' && b[seg + 1] == 'd' && b[seg + 2] == 'o' && b[seg + 3] == 'b' && b[seg + 4] == 'e');
        } else if (marker == 0xDA) {
            if (!ncomp || adobe) return refused;
            if (len < 1 || len != 4 + 2 * (int64_t)b[seg] || b[seg] != ncomp) return refused;
            if (b[seg + len - 3] != 0 || b[seg + len - 2] != 63 || b[seg + len - 1] != 0) return refused;
            for (int i = 0; i < 3; ++i) o.tq[i] = o.td[i] = o.ta[i] = 0;
            for (int i = 0; i < ncomp; ++i) {
                const int id = b[sof + 6 + 3 * i], hv = b[sof + 7 + 3 * i], tq = b[sof + 8 + 3 * i];
                if (b[seg + 1 + 2 * i] != id) return refused;
                const int td = b[seg + 2 + 2 * i] >> 4, ta = b[seg + 2 + 2 * i] & 15;
                if (td > 1 || ta > 1 || tq > 3) return refused;
                if (!o.qt_at[tq] || !o.huff_at[td] || !o.huff_at[2 + ta]) return refused;   // missing table
                o.tq[i] = tq, o.td[i] = td, o.ta[i] = ta;
                if (ncomp == 3 && id != i + 1) return refused;                              // component ids 1, 2, 3
                if (i == 0 ? !(hv == 0x11 || (ncomp == 3 && (hv == 0x21 || hv == 0x22))) : hv != 0x11) return refused;   // sampling factors
            }
            if (o.width > MAX_SIDE || o.height > MAX_SIDE) return refused;
            o.ncomp = ncomp, o.hs = b[sof + 7] >> 4, o.vs = b[sof + 7] & 15, o.restart = restart;
            o.scan_first = (int32_t)pos;
            return 0;
        }
        // APPn, COM and whatever else carries a length: skipped
    }
}

// RSTn markers an accepted scan holds: ceil(mcus / restart) - 1
HAWQ_FRONT_HD int32_t expected_restarts(const hawq_jpeg_front_info &o) {
    const int32_t mcus = ((o.width + 8 * o.hs - 1) / (8 * o.hs)) * ((o.height + 8 * o.vs - 1) / (8 * o.vs));
    return o.restart ? (mcus + o.restart - 1) / o.restart - 1 : 0;
}

// The serial form of the entropy-coded segment's check (the kernel does the same with all lanes): from o.scan_first on, the RSTn
// markers must count modulo 8 from RST0, there must be exactly `expected_restarts` of them, and the first other marker must be EOI.
HAWQ_FRONT_HD int32_t walk_scan(const uint8_t *b, int64_t n, hawq_jpeg_front_info &o) {
    const int32_t expected = expected_restarts(o);
    int32_t rank = 0;
    for (int64_t i = o.scan_first; i + 1 < n; ++i) {
        if (!is_marker(b[i], b[i + 1])) continue;
        const int code = b[i + 1];
        if ((code & 0xF8) == 0xD0) {
            if ((code & 7) != (rank & 7)) return HAWQ_JPEG_FRONT_REFUSED;
            ++rank;
            continue;
        }
        if (code != 0xD9 || rank != expected) return HAWQ_JPEG_FRONT_REFUSED;
        o.scan_end = (int32_t)i, o.n_intervals = expected + 1;
        return 0;
    }
    return HAWQ_JPEG_FRONT_REFUSED;   // truncated scan
}

// A record with nothing but the defer code set
HAWQ_FRONT_HD void clear(hawq_jpeg_front_info &o, int32_t defer) {
    o = hawq_jpeg_front_info{};
    o.defer = defer;
}

// One file on the host: the twin of the kernel
HAWQ_FRONT_HD void walk_file(const uint8_t *b, int64_t n, hawq_jpeg_front_info &o) {
    clear(o, 0);
    int32_t defer = walk_header(b, n, o);
    if (!defer) defer = walk_scan(b, n, o);
    if (defer) clear(o, defer);
}

// ---- the canonical table and the interval table of the fill, shared with the host assembly of tools/jpeg_front_check.cpp ----------
// mincode / maxcode / valptr of one hawq_jpeg_huff from BITS (T.81 F.2.2.3) as huffman_table of hawq_amd/jpeg.py writes them
HAWQ_FRONT_HD void canonical_codes(const uint8_t *bits, int32_t *mincode, int32_t *maxcode, int32_t *valptr) {
    int32_t code = 0, k = 0;
    mincode[0] = valptr[0] = 0, maxcode[0] = -1;
    for (int length = 1; length <= 16; ++length) {
        const int32_t c = bits[length - 1];
        mincode[length] = valptr[length] = 0, maxcode[length] = -1;
        if (c) {
            valptr[length] = k, mincode[length] = code;
            code += c, k += c;
            maxcode[length] = code - 1;
        }
        code <<= 1;
    }
}
}  // namespace hawq_jpeg_front
