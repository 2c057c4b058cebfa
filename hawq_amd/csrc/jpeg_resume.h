// Resume points of the serial JPEG entropy decoders: a long restart interval decoded as several segments, each from the
// state the serial decoder had when it started the segment's first unit.  Plain C++ that compiles for the device (jpeg_decode.hip and
// jpeg_prog.hip decode a segment per wave) and for the host (jpeg_resume.hip records the points; tools/jpeg_resume_host_check.cpp runs
// this very text under the sanitizers).
//
// A segment is a restart interval with a start bit and a start state: the unit loops of jpeg_entropy.h / jpeg_prog.h run its units from
// (pred, eobrun) on a reader that starts at the canonical byte (jpeg_sync.h) of the next unread bit and has discarded `bit` bits.  The
// block decoders are those of the serial path, so a store goes where theirs go: to a block of the units the caller hands in.
//
// Recording listens to the unit loops through their hook and takes the position from the bytes the reader fetched (JpegTrackSrc): a new
// segment begins at the first unit boundary at least `every` stream bytes behind the start of the one before it.  The loops leave at the
// first error, so no point lies behind it, and the last segment runs into the same error.
#pragma once
#include "jpeg_prog.h"

// a fresh reader at the data byte of a point, moved to the point's bit; no data byte there: the status a reader out of bytes gives
template <class Src>
HAWQ_HD void jpeg_resume_start(JpegBits<Src> &br, int bit) {
    if (bit > 0) {
        br.fill();
        br.skip(bit);
    }
}

// Segment `s` of a baseline interval whose first MCU is mcu0, on a reader constructed at s.byte.
template <class Src>
HAWQ_HD int32_t jpeg_resume_segment(JpegBits<Src> &br, const hawq_jpeg_desc &d, const hawq_jpeg_huff *const *dc, const hawq_jpeg_huff *const *ac, int32_t mcu0,
                                    const hawq_jpeg_resume_seg &s, int16_t *coef, bool store) {
    jpeg_resume_start(br, s.bit & 7);
    int32_t pred[3] = {s.pred[0], s.pred[1], s.pred[2]};
    JpegNoHook hook;
    return jpeg_decode_units(br, d, dc, ac, mcu0 + s.unit0, s.n_units, coef, store, pred, hook);
}

// Segment `s` of an interval of scan `sc` whose first unit is unit0, on a reader constructed at s.byte.
template <class Src, class Blk>
HAWQ_HD int32_t jpeg_resume_prog_segment(JpegBits<Src> &br, const hawq_jpeg_desc &d, const hawq_jpeg_scan &sc, const hawq_jpeg_huff *const *dc,
                                         const hawq_jpeg_huff *ac, int32_t unit0, const hawq_jpeg_resume_seg &s, Blk &blk) {
    jpeg_resume_start(br, s.bit & 7);
    JpegProgState st = {{s.pred[0], s.pred[1], s.pred[2]}, s.eobrun};
    JpegNoHook hook;
    return jpeg_prog_units_from(br, d, sc, dc, ac, unit0 + s.unit0, s.n_units, blk, st, hook);
}

// ---- recording (host) ------------------------------------------------------------------------------------------------------------
// Where the data bytes lie that a JpegBits took through JpegTrackSrc: the last eight (it holds at most four unread), and the byte the
// reader was at when it last asked - where it went dry, when it did at a marker.
struct JpegPosTrack {
    int32_t ring[8];
    int32_t n;       // data bytes so far
    int32_t cand;    // first byte of the data byte or marker being read
    int32_t in_ff;   // behind an FF: 00 makes it the data byte FF, FF is fill, anything else a marker
};

template <class Src>
struct JpegTrackSrc {
    Src inner;
    JpegPosTrack *t;
    uint8_t byte(int32_t pos) {
        const uint8_t c = inner.byte(pos);
        if (!t->in_ff) {
            t->cand = pos;
            if (c == 0xFF)
                t->in_ff = 1;
            else
                t->ring[t->n++ & 7] = pos;
        } else if (c == 0) {
            t->ring[t->n++ & 7] = t->cand;
            t->in_ff = 0;
        } else if (c != 0xFF) {
            t->in_ff = 0;
        }
        return c;
    }
};

// The canonical position of the reader's next unread bit.  A reader that is dry and empty stands where it went dry: a reader started
// there goes dry in the same way.
template <class Src>
inline void jpeg_resume_position(const JpegBits<JpegTrackSrc<Src>> &br, int32_t &byte, int32_t &bit) {
    const JpegPosTrack &t = *br.src.t;
    if (br.nbits > 0) {
        byte = t.ring[(t.n - (br.nbits + 7) / 8) & 7];
        bit = (8 - br.nbits % 8) % 8;
    } else {
        byte = br.dry == HAWQ_JPEG_MARKER ? t.cand : br.dry ? br.end : br.pos;
        bit = 0;
    }
}

// The hook of the unit loops that cuts the intervals it hears into segments.  Counts every segment; writes those that fit.
struct JpegResumeRecorder {
    hawq_jpeg_resume_seg *segs;
    int64_t max_segs, n;
    int32_t every;
    hawq_jpeg_resume_seg cur;   // the open segment; its n_units is set when it closes

    void open(int32_t wave, int32_t unit0, int32_t byte, int32_t bit, const int32_t *pred, int32_t eobrun) {
        cur = hawq_jpeg_resume_seg{wave, unit0, 0, byte, bit, eobrun, {pred[0], pred[1], pred[2]}, 0};
    }
    void close(int32_t unit_end) {
        cur.n_units = unit_end - cur.unit0;
        if (n < max_segs) segs[n] = cur;
        ++n;
    }
    // an interval of `wave` starts at byte `first` / ends behind `units` units
    void begin(int32_t wave, int32_t first) {
        const int32_t zero[3] = {0, 0, 0};
        open(wave, 0, first, 0, zero, 0);
    }
    void end(int32_t units) { close(units); }

    template <class Src>
    void unit(int32_t u, const JpegBits<JpegTrackSrc<Src>> &br, const int32_t *pred, int32_t eobrun) {
        if (u == 0 || br.status) return;
        int32_t byte, bit;
        jpeg_resume_position(br, byte, bit);
        if (byte - cur.byte < every) return;
        const int32_t wave = cur.wave;
        close(u);
        open(wave, u, byte, bit, pred, eobrun);
    }
};

// One baseline interval [first, last) of wave `wave`, MCUs mcu0 .. mcu0 + n_mcu - 1, decoded into the image's slab `coef` and cut into
// segments.  Returns the status.
template <class Src>
inline int32_t jpeg_resume_record_interval(Src src, const hawq_jpeg_desc &d, const hawq_jpeg_huff *const *dc, const hawq_jpeg_huff *const *ac, int32_t first,
                                           int32_t last, int32_t mcu0, int32_t n_mcu, int16_t *coef, int32_t wave, JpegResumeRecorder &rec) {
    JpegPosTrack t = {{0, 0, 0, 0, 0, 0, 0, 0}, 0, first, 0};
    JpegBits<JpegTrackSrc<Src>> br(JpegTrackSrc<Src>{src, &t}, first, last);
    int32_t pred[3] = {0, 0, 0};
    rec.begin(wave, first);
    const int32_t st = jpeg_decode_units(br, d, dc, ac, mcu0, n_mcu, coef, true, pred, rec);
    rec.end(n_mcu);
    return st;
}

// The same for one interval of scan `sc`; `blk` hands out the image's slab, on which the scans before this one have run.
template <class Src, class Blk>
inline int32_t jpeg_resume_record_prog_interval(Src src, const hawq_jpeg_desc &d, const hawq_jpeg_scan &sc, const hawq_jpeg_huff *const *dc, const hawq_jpeg_huff *ac,
                                                int32_t first, int32_t last, int32_t unit0, int32_t n_units, Blk &blk, int32_t wave, JpegResumeRecorder &rec) {
    JpegPosTrack t = {{0, 0, 0, 0, 0, 0, 0, 0}, 0, first, 0};
    JpegBits<JpegTrackSrc<Src>> br(JpegTrackSrc<Src>{src, &t}, first, last);
    JpegProgState st = {{0, 0, 0}, 0};
    rec.begin(wave, first);
    const int32_t status = jpeg_prog_units_from(br, d, sc, dc, ac, unit0, n_units, blk, st, rec);
    rec.end(n_units);
    return status;
}
