// Self-synchronising entropy decoding of one restart interval with many lanes: the resumable decoder of
// hawq_jpeg_decode_batch_sync.  Plain C++ that compiles for the device (jpeg_decode.hip) and for the host (tools/jpeg_sync_host_check.cpp
// runs this very text under the sanitizers, lane after lane).
//
// The interval's L stream bytes are cut into n = ceil(L / S) sub-sequences of S raw bytes.  A decoder state is (byte, bit, u, k): the
// next unread bit is bit `bit` (0 = first) of the data byte at `byte`, the next symbol belongs to block `u` of the MCU and, for k > 0,
// continues it at coefficient k (k = 0: a DC code comes next).  A symbol - a Huffman code and its extra bits - belongs to the
// sub-sequence its first bit lies in.  The position is canonical: `byte` names a data byte, never the 00 of FF 00 or a fill FF behind a
// first FF (an FF FF* 00 run is the data byte FF at its first position), so two decoders at the same stream bit hold the same state.
//
// Lane i guesses (first + i * S behind a stuffed 00, bit 0, u 0, k 0), decodes the symbols of its sub-sequence and keeps the state
// behind the last one - or none, after a decode error, which under a guess is no error of the image.  Round after round a lane whose
// predecessor HAS an end state that differs from the start it last decoded from decodes again from it; nobody else does.  Lane 0 starts
// true, so after pass r lanes 0 .. r - 1 are true: at most n passes.  The chain of true lanes ends at the first lane without an end
// (the image's error, or whatever lies behind the last block); the lanes behind it keep their guesses and write nothing.
//
// Bounds: as in jpeg_entropy.h the reader takes bytes only through `Src::byte(pos)` with first <= pos < end of the interval.  A lane's
// loop runs at most 8 * S + 8 times (every symbol takes at least one bit of its sub-sequence).  A store goes to coefficient < 64 of a
// block whose ordinal in the interval is below the interval's block count.
#pragma once
#include "jpeg_entropy.h"

// The first JPEG_SYNC_LUT_BITS bits of a code decide most symbols: lut[prefix] = code length << 8 | value, or 0 where JpegBits::symbol's
// loop over the lengths has to decide (longer codes, no code, a value outside huffval).  An entry is that very loop run on the prefix.
enum { JPEG_SYNC_LUT_BITS = 9, JPEG_SYNC_LUT_SIZE = 1 << JPEG_SYNC_LUT_BITS };
HAWQ_HD uint16_t jpeg_sync_lut_entry(const hawq_jpeg_huff *t, int prefix) {
    const int32_t look = prefix << (16 - JPEG_SYNC_LUT_BITS);
    for (int l = 1; l <= JPEG_SYNC_LUT_BITS; ++l) {
        const int32_t code = look >> (16 - l);
        if (code <= t->maxcode[l]) {
            const int32_t at = t->valptr[l] + code - t->mincode[l];
            return at < 0 || at > 255 ? (uint16_t)0 : (uint16_t)((l << 8) | t->huffval[at]);
        }
    }
    return 0;
}

struct JpegSyncTables {   // the Huffman tables dc, ac of component 0, 1, 2 (six in a row) and their prefix tables, in the same order
    const hawq_jpeg_huff *huff;
    const uint16_t *lut;   // [6][JPEG_SYNC_LUT_SIZE]
    HAWQ_HD const hawq_jpeg_huff *table(int c, int is_ac) const { return huff + 2 * c + is_ac; }
    HAWQ_HD const uint16_t *prefix(int c, int is_ac) const { return lut + (2 * c + is_ac) * JPEG_SYNC_LUT_SIZE; }
};

// JpegBits with a position: it can start at a (byte, bit) and says where its next unread bit is.  `acc` keeps the byte the next bit
// lies in (64 bits: up to 32 unread bits and the 7 read ones of their first byte), so leaving a byte knows whether it was an FF.
template <class Src>
struct JpegPosBits {
    Src src;
    int32_t pos, end;   // pos: the next byte to fetch
    uint64_t acc;       // the low `nbits` bits are unread stream bits, oldest highest
    int32_t nbits;
    int32_t dry;        // 0, or why no more bytes come: HAWQ_JPEG_EOF / HAWQ_JPEG_MARKER
    int32_t status;     // first error
    int32_t upos, ubit; // the next unread bit; (nbits + ubit) % 8 == 0, and upos == pos when nbits == 0

    // start at bit `bit` of the data byte at `at` (first <= at <= last)
    HAWQ_HD JpegPosBits(Src s, int32_t at, int32_t bit, int32_t last) : src(s), pos(at), end(last), acc(0), nbits(0), dry(0), status(0), upos(at), ubit(0) {
        if (bit > 0) {
            fill();
            if (nbits >= 8)
                nbits -= bit, ubit = bit;
            else
                fail(dry ? dry : HAWQ_JPEG_EOF);   // no data byte here: not a state the decoder reaches
        }
    }

    HAWQ_HD void fail(int32_t why) {
        if (status == 0) status = why;
    }

    // as JpegBits::fill
    HAWQ_HD void fill() {
        while (nbits <= 24 && dry == 0) {
            if (pos >= end) {
                dry = HAWQ_JPEG_EOF;
                break;
            }
            uint32_t c = src.byte(pos++);
            if (c == 0xFF) {
                uint32_t d = 0xFF;
                while (d == 0xFF && pos < end) d = src.byte(pos++);
                if (d == 0xFF) {
                    dry = HAWQ_JPEG_EOF;
                    break;
                }
                if (d != 0) {
                    dry = HAWQ_JPEG_MARKER;
                    break;
                }
            }
            acc = (acc << 8) | c;
            nbits += 8;
        }
    }

    HAWQ_HD uint32_t peek(int n) const {
        const uint32_t mask = (1u << n) - 1u;
        return (uint32_t)(nbits >= n ? acc >> (nbits - n) : acc << (n - nbits)) & mask;
    }

    // the position behind the data byte `c` at upos: FF is FF FF* 00 (fill() took it as data, so the 00 is there)
    HAWQ_HD void leave_byte(uint32_t c) {
        ++upos;
        if (c == 0xFF) {
            while (upos < end && src.byte(upos) == 0xFF) ++upos;
            ++upos;
        }
    }

    HAWQ_HD void skip(int n) {
        if (n > nbits) {
            fail(dry ? dry : HAWQ_JPEG_EOF);
            nbits = 0;
            return;
        }
        while (n > 0) {   // at most three bytes: n <= 16
            const int rest = 8 - ubit, take = n < rest ? n : rest;
            if (take == rest) {
                leave_byte((uint32_t)(acc >> (nbits - rest)) & 0xFFu);
                ubit = 0;
            } else {
                ubit += take;
            }
            nbits -= take, n -= take;
        }
    }

    HAWQ_HD int32_t receive(int n) {
        if (n == 0) return 0;
        if (nbits < n) fill();
        const uint32_t v = peek(n);
        skip(n);
        return (int32_t)v;
    }

    HAWQ_HD int32_t symbol(const hawq_jpeg_huff *t, const uint16_t *lut) {
        if (nbits < 16) fill();
        const int32_t look = (int32_t)peek(16);
        const uint32_t fast = lut[look >> (16 - JPEG_SYNC_LUT_BITS)];
        if (fast) {
            skip((int)(fast >> 8));
            return (int32_t)(fast & 0xFFu);
        }
        for (int l = 1; l <= 16; ++l) {
            const int32_t code = look >> (16 - l);
            if (code <= t->maxcode[l]) {
                skip(l);
                const int32_t at = t->valptr[l] + code - t->mincode[l];
                if (at < 0 || at > 255) {
                    fail(HAWQ_JPEG_CODE);
                    return 0;
                }
                return t->huffval[at];
            }
        }
        fail(HAWQ_JPEG_CODE);
        return 0;
    }
};

// blocks per MCU, and the component of block u of an MCU
HAWQ_HD int jpeg_sync_bpm(const hawq_jpeg_desc &d) { return d.ncomp == 1 ? 1 : d.hs * d.vs + 2; }
HAWQ_HD int jpeg_sync_comp(const hawq_jpeg_desc &d, int u) { return d.ncomp == 1 || u < d.hs * d.vs ? 0 : u - d.hs * d.vs + 1; }

// state words of struct hawq_jpeg_sync_sub: the byte, and bit | u << 8 | k << 16; byte < 0: no valid state
HAWQ_HD int32_t jpeg_sync_pack(int bit, int u, int k) { return bit | (u << 8) | (k << 16); }

struct JpegSyncSymbol {
    int32_t status;      // 0, or the reader's first error (nothing else below counts then)
    int32_t dc;          // 1: a DC symbol, `value` is the DC difference
    int32_t store;       // >= 0: coefficient index (zig-zag) `value` goes to (AC only)
    int32_t value;
    int32_t block_end;   // the block ended with this symbol: u, k moved to the next block
};

// One symbol from state (u, k) with the reader at its first bit -> the new (u, k), symbol for symbol what jpeg_decode_block does:
// a DC category above 15 is HAWQ_JPEG_CODE, a ZRL that takes k to 64 or beyond ends the block, a run past 63 is HAWQ_JPEG_INDEX.
template <class Src>
HAWQ_HD JpegSyncSymbol jpeg_sync_step(JpegPosBits<Src> &br, const JpegSyncTables &tb, int c, int bpm, int32_t &u, int32_t &k) {
    JpegSyncSymbol r = {0, 0, -1, 0, 0};
    if (k == 0) {
        const int32_t s = br.symbol(tb.table(c, 0), tb.prefix(c, 0));
        if (s > 15) br.fail(HAWQ_JPEG_CODE);
        if (br.status) return r.status = br.status, r;
        r.value = jpeg_extend(br.receive(s), s);
        if (br.status) return r.status = br.status, r;
        r.dc = 1;
        k = 1;   // at least one AC symbol follows
        return r;
    }
    const int32_t rs = br.symbol(tb.table(c, 1), tb.prefix(c, 1));
    if (br.status) return r.status = br.status, r;
    const int run = rs >> 4, sz = rs & 15;
    if (sz == 0) {
        if (run != 15)
            k = 64;   // EOB
        else
            k += 16;  // ZRL
    } else {
        k += run;
        if (k > 63) {
            br.fail(HAWQ_JPEG_INDEX);
            return r.status = br.status, r;
        }
        r.value = jpeg_extend(br.receive(sz), sz);
        if (br.status) return r.status = br.status, r;
        r.store = k;
        ++k;
    }
    if (k >= 64) {
        r.block_end = 1;
        k = 0;
        u = u + 1 == bpm ? 0 : u + 1;
    }
    return r;
}

// where lane i of an interval starting at `first` guesses its start: bit 0 of byte first + i * S, behind a stuffed 00
template <class Src>
HAWQ_HD int32_t jpeg_sync_guess(Src &src, int32_t first, int32_t i, int32_t sub_bytes) {
    const int32_t at = first + i * sub_bytes;
    return i > 0 && src.byte(at) == 0 && src.byte(at - 1) == 0xFF ? at + 1 : at;
}

// the first byte that is no longer lane i's: the last lane takes whatever follows
HAWQ_HD int32_t jpeg_sync_limit(int32_t first, int32_t i, int32_t n_sub, int32_t sub_bytes) {
    return i + 1 < n_sub ? first + (i + 1) * sub_bytes : 0x7FFFFFFF;
}

struct JpegSyncWriter {      // where the write pass stores: all of it follows from the descriptor
    int16_t *coef;           // the image's first block
    int32_t mcu0;            // the interval's first MCU
    int32_t total;           // blocks of the interval
};

// Lane pass over the symbols of one sub-sequence from state (at, uk) to `limit`.
// Without `wr` (speculate / synchronise): stores nothing; sub.end_* = the state behind the last symbol, or -1 after an error;
//   sub.blocks = blocks that ended here, sub.dc[c] = sum of the DC differences of component c here.
// With `wr` (write; the start is true, sub.blocks / sub.dc are the exclusive scans = ordinal of the lane's first block and the
//   predictors there): stores the coefficients of blocks below wr->total and stops there.  Returns the image's error if it lies here.
template <class Src>
HAWQ_HD int32_t jpeg_sync_lane(Src src, const hawq_jpeg_desc &d, const JpegSyncTables &tb, int32_t last, int32_t limit, int32_t sub_bytes, hawq_jpeg_sync_sub &sub,
                               const JpegSyncWriter *wr) {
    const int bpm = jpeg_sync_bpm(d);
    int32_t u = (sub.start_uk >> 8) & 0xFF, k = (sub.start_uk >> 16) & 0xFF;
    int32_t pred[3] = {0, 0, 0}, blocks = 0, ordinal = 0;
    int16_t *blk = nullptr;
    if (wr) {
        ordinal = sub.blocks;
        pred[0] = sub.dc[0], pred[1] = sub.dc[1], pred[2] = sub.dc[2];
        if (sub.start_pos < 0 || ordinal >= wr->total) return 0;
    } else {
        sub.end_pos = -1, sub.end_uk = 0, sub.blocks = 0, sub.dc[0] = sub.dc[1] = sub.dc[2] = 0;
        if (sub.start_pos < 0) return 0;
    }
    if (u >= bpm || k > 63) return 0;   // no state of this image
    JpegPosBits<Src> br(src, sub.start_pos, sub.start_uk & 7, last);
    if (br.status) return wr ? br.status : 0;
    bool fresh = true;   // blk is not that of `ordinal` yet
    for (int32_t n = 0; n < 8 * sub_bytes + 8 && br.upos < limit; ++n) {
        const int c = jpeg_sync_comp(d, u);
        const JpegSyncSymbol s = jpeg_sync_step(br, tb, c, bpm, u, k);
        if (s.status) return wr ? s.status : 0;
        if (wr) {
            if (fresh) {   // ordinal -> (mcu, component, i, j) -> block, as jpeg_decode_interval
                const int32_t m = wr->mcu0 + ordinal / bpm, uu = ordinal % bpm;   // uu == u of the symbol's first bit
                const int32_t mx = m % d.mcus_x, my = m / d.mcus_x;
                const int cb = jpeg_sync_comp(d, uu);
                int64_t comp0 = 0;
                for (int cc = 0; cc < cb; ++cc) comp0 += (int64_t)d.mcus_x * jpeg_comp_h(d, cc) * d.mcus_y * jpeg_comp_v(d, cc);
                const int h = jpeg_comp_h(d, cb), v = jpeg_comp_v(d, cb);
                const int ui = cb == 0 ? uu % h : 0, uj = cb == 0 ? uu / h : 0;
                blk = wr->coef + (comp0 + ((int64_t)my * v + uj) * ((int64_t)d.mcus_x * h) + (int64_t)mx * h + ui) * 64;
                fresh = false;
            }
            if (s.dc) {
                pred[c] = (int32_t)((uint32_t)pred[c] + (uint32_t)s.value);
                blk[0] = (int16_t)(uint16_t)(uint32_t)pred[c];
            } else if (s.store >= 0) {
                blk[jpeg_natural(s.store)] = (int16_t)s.value;
            }
            if (s.block_end) {
                fresh = true;
                if (++ordinal >= wr->total) return 0;
            }
        } else {
            if (s.dc) pred[c] = (int32_t)((uint32_t)pred[c] + (uint32_t)s.value);
            blocks += s.block_end;
        }
    }
    if (!wr && br.upos >= limit) {
        sub.end_pos = br.upos, sub.end_uk = jpeg_sync_pack(br.ubit, u, k);
        sub.blocks = blocks, sub.dc[0] = pred[0], sub.dc[1] = pred[1], sub.dc[2] = pred[2];
    }
    return 0;
}
