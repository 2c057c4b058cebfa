// The host half of decoding from resume points (jpeg_resume.h): hawq_jpeg_resume_record runs the serial decoders on a
// host blob and cuts its intervals into segments, hawq_jpeg_resume_ok proves a segment table against its blob.  No kernel lives here:
// the segments are decoded by the entropy kernels of jpeg_decode.hip and jpeg_prog.hip.
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "jpeg_resume.h"
#include "jpeg_stages.h"

namespace {
using namespace hawq_jpeg;

// what a wave of either kind of blob decodes
struct WaveInfo {
    int32_t image, scan;     // scan: -1 in a baseline blob
    int32_t first, last;     // its interval
    int32_t unit0, units;    // the interval's first unit in the scan's grid, and how many it has
    int32_t pred_comps;      // predictors in use: the image's components, those of a first DC pass, else 0
    bool eob;                // an AC scan: EOBRUN is in use
};

struct Tables {
    const uint8_t *blob;
    hawq_jpeg_batch_hdr hd;
    hawq_jpeg_prog_hdr ph;
    const hawq_jpeg_desc *desc;
    const int32_t *waves;   // [n_waves][2]
    const hawq_jpeg_scan *scans;
    bool prog;

    Tables(const void *host_blob, bool progressive) : blob((const uint8_t *)host_blob), prog(progressive) {
        memcpy(&hd, blob, sizeof hd);
        memset(&ph, 0, sizeof ph);
        if (prog) memcpy(&ph, blob + sizeof hd, sizeof ph);
        desc = (const hawq_jpeg_desc *)(blob + hd.desc_off);
        waves = (const int32_t *)(blob + hd.wave_off);
        scans = prog ? (const hawq_jpeg_scan *)(blob + ph.scan_off) : nullptr;
    }

    // of a blob its checker has passed
    WaveInfo wave(int32_t w) const {
        WaveInfo wi;
        const int32_t k = waves[2 * w + 1];
        if (prog) {
            const hawq_jpeg_scan &sc = scans[waves[2 * w]];
            const hawq_jpeg_desc &d = desc[sc.image];
            const int32_t *iv = (const int32_t *)(blob + sc.interval_off) + 2 * k;
            const int32_t units = jpeg_prog_units(d, sc);
            wi.image = sc.image, wi.scan = waves[2 * w], wi.first = iv[0], wi.last = iv[1];
            wi.unit0 = sc.restart ? k * sc.restart : 0;
            wi.units = sc.restart ? std::min(sc.restart, units - wi.unit0) : units;
            wi.pred_comps = sc.ss == 0 && sc.ah == 0 ? sc.ncomp : 0;
            wi.eob = sc.ss > 0;
        } else {
            const hawq_jpeg_desc &d = desc[waves[2 * w]];
            const int32_t *iv = (const int32_t *)(blob + d.interval_off) + 2 * k;
            const int32_t mcus = d.mcus_x * d.mcus_y;
            wi.image = waves[2 * w], wi.scan = -1, wi.first = iv[0], wi.last = iv[1];
            wi.unit0 = d.restart ? k * d.restart : 0;
            wi.units = d.restart ? std::min(d.restart, mcus - wi.unit0) : mcus;
            wi.pred_comps = d.ncomp;
            wi.eob = false;
        }
        return wi;
    }
};

struct BlobSrc {   // the reader asks for first <= pos < last of an interval the checker has placed inside the stream
    const uint8_t *stream;
    uint8_t byte(int32_t pos) const { return stream[pos]; }
};

struct SlabBlk {   // the Blk of jpeg_prog.h on a host slab
    int16_t *coef;
    int16_t *open(int64_t b) { return coef + b * 64; }
    int16_t *open_fresh(int64_t b) { return coef + b * 64; }
    uint64_t history(const int16_t *c) const {
        uint64_t m = 0;
        for (int k = 0; k < 64; ++k) m |= (uint64_t)(c[jpeg_natural(k)] != 0) << k;
        return m;
    }
    void close(int64_t, int, int) {}
    void dc_store(int64_t b, int16_t v) { coef[b * 64] = v; }
    void dc_or(int64_t b, int16_t bit) { coef[b * 64] = (int16_t)(coef[b * 64] | bit); }
};

// the waves of image i in decode order: the wave list's order in a baseline blob, scan after scan in a progressive one
void record_image(const Tables &tb, int32_t i, const std::vector<int32_t> &image_waves, JpegResumeRecorder &rec) {
    const hawq_jpeg_desc &d = tb.desc[i];
    std::vector<int16_t> slab((size_t)geometry(d).blocks * 64, 0);
    for (const int32_t w : image_waves) {
        const WaveInfo wi = tb.wave(w);
        if (tb.prog) {
            const hawq_jpeg_scan &sc = tb.scans[wi.scan];
            const hawq_jpeg_huff *dc[3];
            for (int c = 0; c < 3; ++c) dc[c] = (const hawq_jpeg_huff *)(tb.blob + sc.dc_off[c]);   // read by a first DC pass only
            SlabBlk blk{slab.data()};
            jpeg_resume_record_prog_interval(BlobSrc{tb.blob + sc.stream_off}, d, sc, dc, (const hawq_jpeg_huff *)(tb.blob + sc.ac_off), wi.first, wi.last, wi.unit0,
                                             wi.units, blk, w, rec);
        } else {
            const hawq_jpeg_huff *dc[3], *ac[3];
            for (int c = 0; c < 3; ++c) {
                const int cc = c < d.ncomp ? c : 0;
                dc[c] = (const hawq_jpeg_huff *)(tb.blob + d.dc_off[cc]), ac[c] = (const hawq_jpeg_huff *)(tb.blob + d.ac_off[cc]);
            }
            jpeg_resume_record_interval(BlobSrc{tb.blob + d.stream_off}, d, dc, ac, wi.first, wi.last, wi.unit0, wi.units, slab.data(), w, rec);
        }
    }
}
}  // namespace

const char *hawq_jpeg::resume_refusal(const void *host_blob, int64_t blob_bytes, int progressive, int64_t segs_off, int64_t n_segs) {
    if (!host_blob || blob_bytes < (int64_t)sizeof(hawq_jpeg_batch_hdr) || ((uintptr_t)host_blob & 7)) return "no blob, or not 8-byte aligned";
    const Tables tb(host_blob, progressive != 0);
    if (n_segs < tb.hd.n_waves || n_segs > 0x7FFFFFFF) return "fewer segments than waves";
    if (segs_off <= 0 || !inside(segs_off, n_segs * (int64_t)sizeof(hawq_jpeg_resume_seg), blob_bytes, 16)) return "segment table outside the blob";
    const hawq_jpeg_resume_seg *segs = (const hawq_jpeg_resume_seg *)(tb.blob + segs_off);
    int64_t at = 0;
    for (int32_t w = 0; w < tb.hd.n_waves; ++w) {
        const WaveInfo wi = tb.wave(w);
        int32_t unit = 0, byte = wi.first;
        for (bool head = true; at < n_segs && (head || segs[at].wave == w); ++at, head = false) {
            const hawq_jpeg_resume_seg &s = segs[at];
            if (s.wave != w) return "the segments do not follow the wave list";
            if (s.unit0 != unit || s.n_units < 1 || s.n_units > wi.units - unit) return "the segments of an interval do not partition its units in order";
            if (head && (s.byte != wi.first || s.bit != 0 || s.eobrun != 0 || s.pred[0] != 0 || s.pred[1] != 0 || s.pred[2] != 0))
                return "the first segment of an interval does not start at its first byte with a zero state";
            if (s.byte < byte || s.byte > wi.last) return "a segment starts outside its interval or before its predecessor";
            if (s.bit < 0 || s.bit > 7) return "a segment's bit outside 0..7";
            if (s.eobrun < 0 || s.eobrun > 32767) return "a segment's eobrun outside 0..32767";
            if (s.eobrun != 0 && !wi.eob) return "eobrun in a scan that is no AC scan";
            for (int c = wi.pred_comps; c < 3; ++c)
                if (s.pred[c] != 0) return "a predictor in a scan that is no first DC pass, or of a component it does not have";
            unit += s.n_units, byte = s.byte;
        }
        if (unit != wi.units) return "the segments of an interval do not partition its units in order";
    }
    return at == n_segs ? nullptr : "the segments do not follow the wave list";
}

extern "C" int hawq_jpeg_resume_ok(const void *host_blob, int64_t blob_bytes, int32_t progressive, int64_t segs_off, int64_t n_segs) {
    const char *why = resume_refusal(host_blob, blob_bytes, progressive, segs_off, n_segs);
    if (why) hawq_set_error("hawq_jpeg_resume_ok: %s", why);
    return why == nullptr;
}

extern "C" int hawq_jpeg_resume_record(const void *host_blob, int64_t blob_bytes, int32_t progressive, int32_t every, hawq_jpeg_resume_seg *segs, int64_t max_segs,
                                       int64_t *n_segs) {
    HAWQ_REQUIRE(n_segs && max_segs >= 0 && (segs || max_segs == 0), "hawq_jpeg_resume_record: null pointer");
    HAWQ_REQUIRE(every >= 1, "hawq_jpeg_resume_record: every below 1");
    const int64_t any = (int64_t)1 << 62;   // the three device buffers play no part here
    if (!(progressive ? hawq_jpeg_prog_ok(host_blob, blob_bytes, any, any, any) : hawq_jpeg_batch_ok(host_blob, blob_bytes, any, any, any))) return 1;
    const Tables tb(host_blob, progressive != 0);
    // per image its waves in decode order: scan after scan (the scan table's order), a scan's intervals in order
    std::vector<std::vector<int32_t>> image_waves((size_t)tb.hd.n_images);
    std::vector<std::pair<int64_t, int32_t>> order((size_t)tb.hd.n_waves);   // (scan or image, wave): intervals are in order already
    int64_t bound = tb.hd.n_waves;
    for (int32_t w = 0; w < tb.hd.n_waves; ++w) {
        const WaveInfo wi = tb.wave(w);
        order[(size_t)w] = {tb.waves[2 * w], w};
        bound += (wi.last - wi.first) / every;
    }
    std::stable_sort(order.begin(), order.end());
    for (const auto &o : order) image_waves[(size_t)tb.wave(o.second).image].push_back(o.second);
    std::vector<hawq_jpeg_resume_seg> all((size_t)bound);
    JpegResumeRecorder rec{all.data(), bound, 0, every, {}};
    for (int32_t i = 0; i < tb.hd.n_images; ++i) record_image(tb, i, image_waves[(size_t)i], rec);
    std::stable_sort(all.begin(), all.begin() + rec.n, [](const hawq_jpeg_resume_seg &a, const hawq_jpeg_resume_seg &b) { return a.wave < b.wave; });
    *n_segs = rec.n;
    HAWQ_REQUIRE(rec.n <= max_segs, "hawq_jpeg_resume_record: %lld segments, room for %lld", (long long)rec.n, (long long)max_segs);
    if (rec.n) memcpy(segs, all.data(), (size_t)rec.n * sizeof(hawq_jpeg_resume_seg));
    return 0;
}
