// Baseline JPEG entropy decoding (ITU T.81 F.2.2), one restart interval at a time: the bit reader and the per-block decoder of
// hawq_jpeg_decode_batch.  Plain C++ that compiles for the device (jpeg_decode.hip) and for the host (tools/jpeg_host_check.cpp runs
// this very text under the sanitizers on valid and corrupted streams).
//
// Bounds: the reader takes bytes only through `Src::byte(pos)` with first <= pos < end, the bounds of its interval; past them, or
// behind a marker, it hands out zero bits and records why.  Every loop is bounded by a header quantity: MCUs of the interval, blocks of
// an MCU, 64 coefficients, 16 code lengths.  A store goes to coefficient (natural order, < 64) of a block of the interval's own MCUs.
#pragma once
#include <stdint.h>

#include "../../include/hawq_mi355.h"

#if defined(__HIPCC__)
#define HAWQ_HD __host__ __device__ __forceinline__
#define HAWQ_UNROLL _Pragma("unroll")
#else
#define HAWQ_HD inline
#define HAWQ_UNROLL
#endif

// zig-zag index -> natural (row-major) index
HAWQ_HD int jpeg_natural(int k) {
    const uint8_t order[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return order[k & 63];
}

// Src: `uint8_t byte(int32_t pos)` for first <= pos < end (positions relative to the stream).
template <class Src>
struct JpegBits {
    Src src;
    int32_t pos, end;
    uint32_t acc;      // the low `nbits` bits are unread stream bits, oldest highest
    int32_t nbits;
    int32_t dry;       // 0, or why no more bytes come: HAWQ_JPEG_EOF / HAWQ_JPEG_MARKER
    int32_t status;    // first error

    HAWQ_HD JpegBits(Src s, int32_t first, int32_t last) : src(s), pos(first), end(last), acc(0), nbits(0), dry(0), status(0) {}

    HAWQ_HD void fail(int32_t why) {
        if (status == 0) status = why;
    }

    // top up to at least 25 bits while bytes remain; FF 00 is a data byte FF, FF FF .. is fill, FF xx ends the data
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
                if (d == 0xFF) {   // the interval ended inside FF ..
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

    // the next n <= 16 bits, zero-padded behind the last one (looking is no error)
    HAWQ_HD uint32_t peek(int n) const {
        const uint32_t mask = (1u << n) - 1u;
        return (nbits >= n ? acc >> (nbits - n) : acc << (n - nbits)) & mask;
    }

    HAWQ_HD void skip(int n) {
        if (n > nbits) {
            fail(dry ? dry : HAWQ_JPEG_EOF);
            nbits = 0;
        } else {
            nbits -= n;
        }
    }

    // RECEIVE(n), n <= 16
    HAWQ_HD int32_t receive(int n) {
        if (n == 0) return 0;
        if (nbits < n) fill();
        const uint32_t v = peek(n);
        skip(n);
        return (int32_t)v;
    }

    // DECODE: one Huffman symbol, 0 with a status when the bits are no code
    HAWQ_HD int32_t symbol(const hawq_jpeg_huff *t) {
        if (nbits < 16) fill();
        const int32_t look = (int32_t)peek(16);
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

// EXTEND (F.2.2.1), 0 <= s <= 15
HAWQ_HD int32_t jpeg_extend(int32_t v, int s) { return s != 0 && v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// One 8x8 block: DC difference onto `pred`, then the AC run/size pairs.  Non-zero coefficients go to blk[natural index] when `store`
// (the block was zero before); the DC keeps the low 16 bits of the running sum, as the library's JCOEF does.
// Returns the reader's status (0: go on).
template <class Src>
HAWQ_HD int32_t jpeg_decode_block(JpegBits<Src> &br, const hawq_jpeg_huff *dc, const hawq_jpeg_huff *ac, int32_t &pred, int16_t *blk, bool store) {
    const int32_t s = br.symbol(dc);
    if (s > 15) br.fail(HAWQ_JPEG_CODE);
    if (br.status) return br.status;
    const int32_t diff = jpeg_extend(br.receive(s), s);
    pred = (int32_t)((uint32_t)pred + (uint32_t)diff);
    if (br.status) return br.status;
    if (store) blk[0] = (int16_t)(uint16_t)(uint32_t)pred;
    int k = 1;
    for (int n = 1; n < 64 && k < 64; ++n) {   // at most 63 symbols: each one advances k
        const int32_t rs = br.symbol(ac);
        if (br.status) return br.status;
        const int r = rs >> 4, sz = rs & 15;
        if (sz == 0) {
            if (r != 15) break;   // EOB
            k += 16;              // ZRL
            continue;
        }
        k += r;
        if (k > 63) {
            br.fail(HAWQ_JPEG_INDEX);
            return br.status;
        }
        const int32_t v = jpeg_extend(br.receive(sz), sz);
        if (br.status) return br.status;
        if (store) blk[jpeg_natural(k)] = (int16_t)v;
        ++k;
    }
    return 0;
}

// blocks of component c: h x v per MCU
HAWQ_HD int jpeg_comp_h(const hawq_jpeg_desc &d, int c) { return c == 0 ? d.hs : 1; }
HAWQ_HD int jpeg_comp_v(const hawq_jpeg_desc &d, int c) { return c == 0 ? d.vs : 1; }

// What the unit loops tell about every unit they start (jpeg_resume.h records resume points through it); this one listens to nothing.
struct JpegNoHook {
    template <class Bits>
    HAWQ_HD void unit(int32_t, const Bits &, const int32_t *, int32_t) {}
};

// MCUs mcu0 .. mcu0 + n_mcu - 1 of image `d` in raster order from the predictors `pred`, which it advances.  `coef` is the image's
// first block (d.coef_block0 applied by the caller); `dc` / `ac` the tables per component.  Before MCU m of them it calls
// hook.unit(m, reader, predictors, 0).  Returns the status.
template <class Src, class Hook>
HAWQ_HD int32_t jpeg_decode_units(JpegBits<Src> &br, const hawq_jpeg_desc &d, const hawq_jpeg_huff *const *dc, const hawq_jpeg_huff *const *ac, int32_t mcu0,
                                  int32_t n_mcu, int16_t *coef, bool store, int32_t *pred, Hook &hook) {
    int32_t mx = mcu0 % d.mcus_x, my = mcu0 / d.mcus_x;
    for (int32_t m = 0; m < n_mcu; ++m) {
        hook.unit(m, br, pred, 0);
        int64_t comp0 = 0;   // first block of the component
        for (int c = 0; c < d.ncomp; ++c) {
            const int h = jpeg_comp_h(d, c), v = jpeg_comp_v(d, c);
            const int64_t bw = (int64_t)d.mcus_x * h;
            for (int j = 0; j < v; ++j)
                for (int i = 0; i < h; ++i) {
                    const int64_t b = comp0 + ((int64_t)my * v + j) * bw + (int64_t)mx * h + i;
                    if (jpeg_decode_block(br, dc[c], ac[c], pred[c], coef + b * 64, store)) return br.status;
                }
            comp0 += bw * d.mcus_y * v;
        }
        if (++mx == d.mcus_x) mx = 0, ++my;
    }
    return br.status;
}

// One restart interval: the MCUs with the predictors starting at 0.
template <class Src>
HAWQ_HD int32_t jpeg_decode_interval(JpegBits<Src> &br, const hawq_jpeg_desc &d, const hawq_jpeg_huff *const *dc, const hawq_jpeg_huff *const *ac,
                                     int32_t mcu0, int32_t n_mcu, int16_t *coef, bool store) {
    int32_t pred[3] = {0, 0, 0};
    JpegNoHook hook;
    return jpeg_decode_units(br, d, dc, ac, mcu0, n_mcu, coef, store, pred, hook);
}
