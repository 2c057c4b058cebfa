// Progressive JPEG entropy decoding (ITU T.81 G.1, G.2; the arithmetic of the library's jdphuff.c): the four scan decoders of
// hawq_jpeg_decode_batch_prog, one restart interval of one scan at a time, on the bit reader of jpeg_entropy.h.  Plain C++ that
// compiles for the device (jpeg_prog.hip) and for the host (tools/jpeg_prog_host_check.cpp runs this very text under the sanitizers).
//
// A decoder reaches coefficients only through its `Blk` argument:
//   int16_t *open(int64_t b)              block b of the image's slab as 64 coefficients in natural order, readable and writable
//   int16_t *open_fresh(int64_t b)        the same for a first pass, which reads nothing: the band ss .. se of the block is still zero
//   uint64_t history(const int16_t *c)    of an open block: bit k set when the coefficient with zig-zag index k is not zero
//   void close(int64_t b, int ss, int se) done with it: the coefficients with zig-zag index ss .. se may have changed
//   void dc_store(int64_t b, int16_t v)   coefficient 0 of block b = v
//   void dc_or(int64_t b, int16_t bit)    coefficient 0 of block b |= bit
// The host hands out the slab itself; the kernel stages the block in LDS, so that every lane tests the same word (jpeg_prog.hip).
//
// Bounds: whatever the stream holds, a store or read-modify-write goes to zig-zag index ss .. se of a block of the scan's own grid.
// Every loop is bounded by a header quantity: units of the interval, blocks of an MCU, se - ss + 1 coefficients, 16 code lengths.
#pragma once
#include "jpeg_entropy.h"

struct JpegProgState {
    int32_t pred[3];   // DC predictors
    int32_t eobrun;    // blocks still inside an end-of-band run
};

// Al <= 13: the shifts stay inside 32 bits; the store keeps the low 16, as the library's JCOEF does
HAWQ_HD int16_t jpeg_prog_shl16(int32_t v, int al) { return (int16_t)(uint16_t)((uint32_t)v << al); }

// DC, first pass: category, EXTEND, onto the predictor, pred << al
template <class Src, class Blk>
HAWQ_HD int32_t jpeg_prog_dc_first(JpegBits<Src> &br, const hawq_jpeg_huff *dc, int32_t &pred, int al, Blk &blk, int64_t b) {
    const int32_t s = br.symbol(dc);
    if (s > 15) br.fail(HAWQ_JPEG_CODE);
    if (br.status) return br.status;
    const int32_t diff = jpeg_extend(br.receive(s), s);
    if (br.status) return br.status;
    pred = (int32_t)((uint32_t)pred + (uint32_t)diff);
    blk.dc_store(b, jpeg_prog_shl16(pred, al));
    return 0;
}

// DC, refinement: one bit
template <class Src, class Blk>
HAWQ_HD int32_t jpeg_prog_dc_refine(JpegBits<Src> &br, int al, Blk &blk, int64_t b) {
    const int32_t bit = br.receive(1);
    if (br.status) return br.status;
    if (bit) blk.dc_or(b, (int16_t)(1 << al));
    return 0;
}

// AC, first pass, of a block outside an end-of-band run (the caller counts the run down and leaves such a block alone)
template <class Src>
HAWQ_HD int32_t jpeg_prog_ac_first(JpegBits<Src> &br, const hawq_jpeg_huff *ac, int ss, int se, int al, int32_t &eobrun, int16_t *c) {
    for (int k = ss; k <= se; ++k) {   // at most se - ss + 1 symbols: each one advances k
        const int32_t rs = br.symbol(ac);
        if (br.status) return br.status;
        const int r = rs >> 4, s = rs & 15;
        if (s != 0) {
            k += r;
            if (k > se) {
                br.fail(HAWQ_JPEG_INDEX);
                return br.status;
            }
            const int32_t v = jpeg_extend(br.receive(s), s);
            if (br.status) return br.status;
            c[jpeg_natural(k)] = jpeg_prog_shl16(v, al);
        } else if (r == 15) {
            k += 15;   // ZRL
        } else {       // EOBr: this block and eobrun more end here
            eobrun = (1 << r) + br.receive(r) - 1;
            if (br.status) return br.status;
            break;
        }
    }
    return 0;
}

// the correction bit of a coefficient with history
template <class Src>
HAWQ_HD void jpeg_prog_correct(JpegBits<Src> &br, int16_t *at, int32_t p1, int32_t m1) {
    if (br.receive(1) && (*at & p1) == 0) *at = (int16_t)(*at >= 0 ? *at + p1 : *at + m1);
}

// AC, refinement, of every block of the scan: inside an end-of-band run a block still takes correction bits.  `hist`: which
// coefficients of the band had a value when the scan reached the block (Blk::history) - they take correction bits, the others count
// as the zeros of a run; a coefficient placed by this scan is passed at once, so the mask of the open block holds throughout.
template <class Src>
HAWQ_HD int32_t jpeg_prog_ac_refine(JpegBits<Src> &br, const hawq_jpeg_huff *ac, int ss, int se, int al, int32_t &eobrun, int16_t *c, uint64_t hist) {
    const int32_t p1 = 1 << al, m1 = -p1;   // m1: (-1) << al
    int k = ss;
    if (eobrun == 0) {
        for (; k <= se; ++k) {   // at most se - ss + 1 symbols
            const int32_t rs = br.symbol(ac);
            if (br.status) return br.status;
            int r = rs >> 4;
            int32_t s = rs & 15;
            if (s != 0) {
                if (s != 1) {
                    br.fail(HAWQ_JPEG_CODE);
                    return br.status;
                }
                s = br.receive(1) ? p1 : m1;
                if (br.status) return br.status;
            } else if (r != 15) {
                eobrun = (1 << r) + br.receive(r);   // this block included
                if (br.status) return br.status;
                break;
            }
            // pass r coefficients without history (and every one with history, correcting it) up to the place of the new one
            for (; k <= se; ++k) {
                if ((hist >> k) & 1) {
                    jpeg_prog_correct(br, c + jpeg_natural(k), p1, m1);
                    if (br.status) return br.status;
                } else if (--r < 0) {
                    break;
                }
            }
            if (s != 0) {
                if (k > se) {
                    br.fail(HAWQ_JPEG_INDEX);
                    return br.status;
                }
                c[jpeg_natural(k)] = (int16_t)s;
            }
        }
    }
    if (eobrun > 0) {
        uint64_t rest = k <= se ? (hist >> k) << k : 0;   // the coefficients with history from k on: at most se - k + 1 of them
        rest &= se < 63 ? (1ull << (se + 1)) - 1 : ~0ull;
        while (rest) {
            const int at = __builtin_ctzll(rest);
            rest &= rest - 1;
            jpeg_prog_correct(br, c + jpeg_natural(at), p1, m1);
            if (br.status) return br.status;
        }
        --eobrun;
    }
    return 0;
}

// one block of the scan, by its kind
template <class Src, class Blk>
HAWQ_HD int32_t jpeg_prog_block(JpegBits<Src> &br, const hawq_jpeg_scan &sc, const hawq_jpeg_huff *const *dc, const hawq_jpeg_huff *ac, int ci, JpegProgState &st,
                                Blk &blk, int64_t b) {
    if (sc.ss == 0) return sc.ah == 0 ? jpeg_prog_dc_first(br, dc[ci], st.pred[ci], sc.al, blk, b) : jpeg_prog_dc_refine(br, sc.al, blk, b);
    if (sc.ah == 0) {
        if (st.eobrun > 0) {
            --st.eobrun;
            return 0;
        }
        int16_t *c = blk.open_fresh(b);
        const int32_t r = jpeg_prog_ac_first(br, ac, sc.ss, sc.se, sc.al, st.eobrun, c);
        blk.close(b, sc.ss, sc.se);
        return r;
    }
    int16_t *c = blk.open(b);
    const int32_t r = jpeg_prog_ac_refine(br, ac, sc.ss, sc.se, sc.al, st.eobrun, c, blk.history(c));
    blk.close(b, sc.ss, sc.se);
    return r;
}

// the scan's grid: MCUs of the image for an interleaved scan, the component's own blocks for a scan of one component
HAWQ_HD int32_t jpeg_prog_own_w(const hawq_jpeg_desc &d, int c) { return ((d.width * jpeg_comp_h(d, c) + d.hs - 1) / d.hs + 7) / 8; }
HAWQ_HD int32_t jpeg_prog_own_h(const hawq_jpeg_desc &d, int c) { return ((d.height * jpeg_comp_v(d, c) + d.vs - 1) / d.vs + 7) / 8; }
HAWQ_HD int32_t jpeg_prog_units(const hawq_jpeg_desc &d, const hawq_jpeg_scan &sc) {
    return sc.ncomp > 1 ? d.mcus_x * d.mcus_y : jpeg_prog_own_w(d, sc.comp0) * jpeg_prog_own_h(d, sc.comp0);
}
// first block of component c in the image's slab
HAWQ_HD int64_t jpeg_prog_comp0(const hawq_jpeg_desc &d, int c) {
    int64_t at = 0;
    for (int k = 0; k < c && k < 3; ++k) at += (int64_t)d.mcus_x * jpeg_comp_h(d, k) * d.mcus_y * jpeg_comp_v(d, k);
    return at;
}

// Units unit0 .. unit0 + n_units - 1 of scan `sc` of image `d` from the state `st`, which it advances.  dc: the tables of the scan's
// components (first DC pass), ac: the scan's AC table.  Before unit n of them it calls hook.unit(n, reader, predictors, EOBRUN).
// Returns the status.
template <class Src, class Blk, class Hook>
HAWQ_HD int32_t jpeg_prog_units_from(JpegBits<Src> &br, const hawq_jpeg_desc &d, const hawq_jpeg_scan &sc, const hawq_jpeg_huff *const *dc, const hawq_jpeg_huff *ac,
                                     int32_t unit0, int32_t n_units, Blk &blk, JpegProgState &st, Hook &hook) {
    if (sc.ncomp == 1) {
        const int32_t w = jpeg_prog_own_w(d, sc.comp0);
        const int64_t comp0 = jpeg_prog_comp0(d, sc.comp0), bw = (int64_t)d.mcus_x * jpeg_comp_h(d, sc.comp0);
        int32_t bx = unit0 % w, by = unit0 / w;
        for (int32_t n = 0; n < n_units; ++n) {
            hook.unit(n, br, st.pred, st.eobrun);
            if (jpeg_prog_block(br, sc, dc, ac, 0, st, blk, comp0 + by * bw + bx)) return br.status;
            if (++bx == w) bx = 0, ++by;
        }
        return br.status;
    }
    int32_t mx = unit0 % d.mcus_x, my = unit0 / d.mcus_x;
    for (int32_t m = 0; m < n_units; ++m) {
        hook.unit(m, br, st.pred, st.eobrun);
        int64_t comp0 = 0;
        for (int c = 0; c < sc.ncomp; ++c) {
            const int h = jpeg_comp_h(d, c), v = jpeg_comp_v(d, c);
            const int64_t bw = (int64_t)d.mcus_x * h;
            for (int j = 0; j < v; ++j)
                for (int i = 0; i < h; ++i)
                    if (jpeg_prog_block(br, sc, dc, ac, c, st, blk, comp0 + ((int64_t)my * v + j) * bw + (int64_t)mx * h + i)) return br.status;
            comp0 += bw * d.mcus_y * v;
        }
        if (++mx == d.mcus_x) mx = 0, ++my;
    }
    return br.status;
}

// One restart interval: the units with predictors and EOBRUN starting at 0.
template <class Src, class Blk>
HAWQ_HD int32_t jpeg_prog_interval(JpegBits<Src> &br, const hawq_jpeg_desc &d, const hawq_jpeg_scan &sc, const hawq_jpeg_huff *const *dc, const hawq_jpeg_huff *ac,
                                   int32_t unit0, int32_t n_units, Blk &blk) {
    JpegProgState st = {{0, 0, 0}, 0};
    JpegNoHook hook;
    return jpeg_prog_units_from(br, d, sc, dc, ac, unit0, n_units, blk, st, hook);
}
