// Host run of the resume points of the JPEG entropy decoders (hawq_amd/csrc/jpeg_resume.h - the recorder of hawq_jpeg_resume_record and
// the segment decoders both entropy kernels compile), meant to be built with -fsanitize=address,undefined and run on its own:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_resume_host_check.cpp -o jpeg_resume_host_check
//   jpeg_resume_host_check base|prog BLOB [SEED]
//
// BLOB: a blob of hawq_amd.jpeg.plan_jpeg_batch (base) or plan_jpeg_prog_batch (prog) that the checker of its kind has passed.  At
// every = 16, 64 and 1024, per image:
// 1. every recorded point equals the state of a straight decode at that unit: predictors, EOBRUN, and the position counted from the
//    bits that decode has consumed (not from the recorder's byte tracker).
// 2. the segments decoded in REVERSE order - level by level in a progressive image - give the serial slab word for word and, interval
//    by interval, the serial status.
// 3. per scan, its stream cut at each eighth byte and with one byte overwritten (200 draws, seeded by SEED and the scan's index):
//    recorded from the damaged bytes, the segments give the serial slab and status of those bytes.
// 4. the points of the GOOD stream applied to each damaged one (a stale index) end with a status or a clean result.
// A segment is decoded the way the kernels do it: its units clamped to the interval's, its byte to the interval.  Slabs and streams live
// in heap blocks of their exact size; the reader's source aborts on a position outside its interval; while a segment runs, every block
// outside its own units is poisoned for AddressSanitizer, and the progressive block source aborts on such a block.  Exit 0: all held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../hawq_amd/csrc/jpeg_resume.h"

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#define JPEG_RESUME_CHECK_ASAN 1
#endif
#endif
#if defined(__SANITIZE_ADDRESS__) || defined(JPEG_RESUME_CHECK_ASAN)
#include <sanitizer/asan_interface.h>
#else
#define ASAN_POISON_MEMORY_REGION(p, n) ((void)(p), (void)(n))
#define ASAN_UNPOISON_MEMORY_REGION(p, n) ((void)(p), (void)(n))
#endif

namespace {
[[noreturn]] void die(const char *what, long long a = 0, long long b = 0) {
    fprintf(stderr, "jpeg_resume_host_check: %s (%lld, %lld)\n", what, a, b);
    abort();
}

struct HostSrc {
    const uint8_t *p;
    int32_t first, end;
    uint8_t byte(int32_t pos) const {
        if (pos < first || pos >= end) die("the reader asked for a byte outside its interval", pos, end);
        return p[pos];
    }
};

// the slab of one image; `own`: nullptr, or per block whether the running segment may touch it
struct HostBlk {
    int16_t *coef;
    int64_t blocks;
    const uint8_t *own;
    void inside(int64_t b) const {
        if (b < 0 || b >= blocks) die("block outside the image", b, blocks);
        if (own && !own[b]) die("block outside the segment's units", b, blocks);
    }
    int16_t *open(int64_t b) {
        inside(b);
        return coef + b * 64;
    }
    int16_t *open_fresh(int64_t b) { return open(b); }
    uint64_t history(const int16_t *c) const {
        uint64_t m = 0;
        for (int k = 0; k < 64; ++k) m |= (uint64_t)(c[jpeg_natural(k)] != 0) << k;
        return m;
    }
    void close(int64_t, int, int) {}
    void dc_store(int64_t b, int16_t v) {
        inside(b);
        coef[b * 64] = v;
    }
    void dc_or(int64_t b, int16_t bit) {
        inside(b);
        coef[b * 64] = (int16_t)(coef[b * 64] | bit);
    }
};

std::vector<uint8_t> read_file(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "jpeg_resume_host_check: cannot open %s\n", path);
        exit(2);
    }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

int64_t image_blocks(const hawq_jpeg_desc &d) { return (int64_t)d.mcus_x * d.mcus_y * (d.ncomp == 1 ? 1 : d.hs * d.vs + 2); }

// One scan of a progressive image, or the one scan of a baseline image (prog = false: dc / ac per component, sc holds only what the
// unit arithmetic below reads).
struct Scan {
    bool prog;
    hawq_jpeg_scan sc;
    int32_t index, units;
    hawq_jpeg_huff dc[3], ac[3];
    std::vector<int32_t> iv;   // [n_intervals][2]
    uint8_t *stream;           // heap block of exactly sc.stream_len bytes
};

struct Image {
    hawq_jpeg_desc d;
    std::vector<Scan> scans;   // in level order (stable: file order within a level)
    int64_t blocks;
};

struct Tables {
    const hawq_jpeg_huff *dc[3], *ac[3];
    explicit Tables(const Scan &s) {
        for (int c = 0; c < 3; ++c) dc[c] = &s.dc[c], ac[c] = &s.ac[c];
    }
};

void interval_units(const Scan &s, int32_t k, int32_t &unit0, int32_t &n_units) {
    unit0 = s.sc.restart ? k * s.sc.restart : 0;
    n_units = s.sc.restart ? std::min(s.sc.restart, s.units - unit0) : s.units;
}

// own[b] = 1 for the blocks of units u0 .. u0 + n - 1 of the scan's grid
void mark_units(const Image &im, const Scan &s, int32_t u0, int32_t n, std::vector<uint8_t> &own) {
    const hawq_jpeg_desc &d = im.d;
    own.assign((size_t)im.blocks, 0);
    if (s.prog && s.sc.ncomp == 1) {
        const int32_t w = jpeg_prog_own_w(d, s.sc.comp0);
        const int64_t comp0 = jpeg_prog_comp0(d, s.sc.comp0), bw = (int64_t)d.mcus_x * jpeg_comp_h(d, s.sc.comp0);
        for (int32_t u = u0; u < u0 + n; ++u) own[(size_t)(comp0 + (u / w) * bw + u % w)] = 1;
        return;
    }
    for (int32_t m = u0; m < u0 + n; ++m) {
        const int32_t mx = m % d.mcus_x, my = m / d.mcus_x;
        int64_t comp0 = 0;
        for (int c = 0; c < d.ncomp; ++c) {
            const int h = jpeg_comp_h(d, c), v = jpeg_comp_v(d, c);
            const int64_t bw = (int64_t)d.mcus_x * h;
            for (int j = 0; j < v; ++j)
                for (int i = 0; i < h; ++i) own[(size_t)(comp0 + ((int64_t)my * v + j) * bw + (int64_t)mx * h + i)] = 1;
            comp0 += bw * d.mcus_y * v;
        }
    }
}

// what a straight decode knows at the start of every unit
struct Witness {
    struct At {
        int32_t pred[3], eobrun, pos, nbits, dry;
    };
    std::vector<At> at;
    template <class Bits>
    void unit(int32_t, const Bits &br, const int32_t *pred, int32_t eobrun) {
        at.push_back(At{{pred[0], pred[1], pred[2]}, eobrun, br.pos, br.nbits, br.dry});
    }
};

// interval k of scan s on `stream` / `iv`, straight
template <class Hook>
int32_t run_interval(const Image &im, const Scan &s, const uint8_t *stream, const std::vector<int32_t> &iv, int32_t k, int16_t *coef, Hook &hook) {
    int32_t unit0, n_units;
    interval_units(s, k, unit0, n_units);
    const Tables tb(s);
    JpegBits<HostSrc> br(HostSrc{stream, iv[2 * k], iv[2 * k + 1]}, iv[2 * k], iv[2 * k + 1]);
    if (s.prog) {
        HostBlk blk{coef, im.blocks, nullptr};
        JpegProgState st = {{0, 0, 0}, 0};
        return jpeg_prog_units_from(br, im.d, s.sc, tb.dc, &s.ac[0], unit0, n_units, blk, st, hook);
    }
    int32_t pred[3] = {0, 0, 0};
    return jpeg_decode_units(br, im.d, tb.dc, tb.ac, unit0, n_units, coef, true, pred, hook);
}

// interval k through the recorder: its segments behind `segs`
int32_t record_interval(const Image &im, const Scan &s, const uint8_t *stream, const std::vector<int32_t> &iv, int32_t k, int16_t *coef, int32_t every,
                        std::vector<hawq_jpeg_resume_seg> &segs) {
    int32_t unit0, n_units;
    interval_units(s, k, unit0, n_units);
    const Tables tb(s);
    const int32_t first = iv[2 * k], last = iv[2 * k + 1];
    const size_t had = segs.size(), room = (size_t)(1 + (last - first) / every);
    segs.resize(had + room);
    JpegResumeRecorder rec{segs.data() + had, (int64_t)room, 0, every, {}};
    int32_t st;
    if (s.prog) {
        HostBlk blk{coef, im.blocks, nullptr};
        st = jpeg_resume_record_prog_interval(HostSrc{stream, first, last}, im.d, s.sc, tb.dc, &s.ac[0], first, last, unit0, n_units, blk, k, rec);
    } else {
        st = jpeg_resume_record_interval(HostSrc{stream, first, last}, im.d, tb.dc, tb.ac, first, last, unit0, n_units, coef, k, rec);
    }
    if (rec.n < 1 || rec.n > (int64_t)room) die("the recorder left its bound", rec.n, (long long)room);
    segs.resize(had + (size_t)rec.n);
    return st;
}

// one segment of interval k the way the kernels run it; everything outside its blocks is out of reach meanwhile
int32_t run_segment(const Image &im, const Scan &s, const uint8_t *stream, const std::vector<int32_t> &iv, int32_t k, hawq_jpeg_resume_seg seg, int16_t *coef) {
    int32_t unit0, n_units;
    interval_units(s, k, unit0, n_units);
    const Tables tb(s);
    const int32_t first = iv[2 * k], last = iv[2 * k + 1];
    seg.unit0 = std::min(std::max(seg.unit0, 0), n_units), seg.n_units = std::min(std::max(seg.n_units, 0), n_units - seg.unit0);
    std::vector<uint8_t> own;
    mark_units(im, s, unit0 + seg.unit0, seg.n_units, own);
    for (int64_t b = 0; b < im.blocks; ++b)
        if (!own[(size_t)b]) ASAN_POISON_MEMORY_REGION(coef + b * 64, 128);
    JpegBits<HostSrc> br(HostSrc{stream, first, last}, std::min(std::max(seg.byte, first), last), last);
    int32_t st;
    if (s.prog) {
        HostBlk blk{coef, im.blocks, own.data()};
        st = jpeg_resume_prog_segment(br, im.d, s.sc, tb.dc, &s.ac[0], unit0, seg, blk);
    } else {
        st = jpeg_resume_segment(br, im.d, tb.dc, tb.ac, unit0, seg, coef, true);
    }
    ASAN_UNPOISON_MEMORY_REGION(coef, (size_t)im.blocks * 128);
    return st;
}

// the canonical position of the bit `bits` data bits behind `first`
void canonical(const uint8_t *p, int32_t first, int32_t end, int64_t bits, int32_t &byte, int32_t &bit) {
    int32_t at = first;
    for (int64_t n = bits / 8; n > 0; --n) {
        if (p[at++] == 0xFF) {
            while (at < end && p[at] == 0xFF) ++at;
            ++at;
        }
    }
    byte = at, bit = (int32_t)(bits % 8);
}

// data bytes in the raw bytes [first, pos), pos behind a whole data byte
int64_t data_bytes(const uint8_t *p, int32_t first, int32_t pos) {
    int64_t n = 0;
    for (int32_t at = first; at < pos; ++n)
        if (p[at++] == 0xFF) {
            while (at < pos && p[at] == 0xFF) ++at;
            ++at;
        }
    return n;
}

struct ScanRun {   // a scan on one stream: per interval the status and the segments
    std::vector<int32_t> status;
    std::vector<std::vector<hawq_jpeg_resume_seg>> segs;
};

// the scan through the recorder, interval after interval
ScanRun record_scan(const Image &im, const Scan &s, const uint8_t *stream, const std::vector<int32_t> &iv, int16_t *coef, int32_t every) {
    ScanRun r;
    for (int32_t k = 0; k < s.sc.n_intervals; ++k) {
        r.segs.emplace_back();
        r.status.push_back(record_interval(im, s, stream, iv, k, coef, every, r.segs.back()));
    }
    return r;
}

// the scan's segments in reverse order; -> per interval the first status in segment order, -1 when a segment before the last failed
std::vector<int32_t> run_segments_reversed(const Image &im, const Scan &s, const uint8_t *stream, const std::vector<int32_t> &iv,
                                           const std::vector<std::vector<hawq_jpeg_resume_seg>> &segs, int16_t *coef) {
    std::vector<int32_t> status((size_t)s.sc.n_intervals, 0);
    for (int32_t k = s.sc.n_intervals - 1; k >= 0; --k)
        for (size_t n = segs[(size_t)k].size(); n-- > 0;) {
            const int32_t st = run_segment(im, s, stream, iv, k, segs[(size_t)k][n], coef);
            if (st) status[(size_t)k] = n + 1 == segs[(size_t)k].size() ? st : -1;
        }
    return status;
}

int16_t *copy_slab(const int16_t *from, size_t words) {
    int16_t *p = (int16_t *)malloc(words * sizeof(int16_t));
    memcpy(p, from, words * sizeof(int16_t));
    return p;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc < 3 || (strcmp(argv[1], "base") && strcmp(argv[1], "prog"))) {
        fprintf(stderr, "usage: jpeg_resume_host_check base|prog BLOB [SEED]\n");
        return 2;
    }
    const bool prog = !strcmp(argv[1], "prog");
    const std::vector<uint8_t> blob = read_file(argv[2]);
    const uint64_t seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 1;
    if (blob.size() < sizeof(hawq_jpeg_batch_hdr) + sizeof(hawq_jpeg_prog_hdr)) return 2;
    hawq_jpeg_batch_hdr hd;
    hawq_jpeg_prog_hdr ph;
    memcpy(&hd, blob.data(), sizeof hd);
    memcpy(&ph, blob.data() + sizeof hd, sizeof ph);
    const int32_t everies[3] = {16, 64, 1024};
    long points = 0, points_eob = 0, points_bit = 0, segments = 0, intervals_cut = 0, damaged = 0, damaged_flagged = 0, stale = 0, stale_flagged = 0, bad = 0;
    for (int32_t i = 0; i < hd.n_images; ++i) {
        Image im;
        memcpy(&im.d, blob.data() + hd.desc_off + (size_t)i * sizeof(hawq_jpeg_desc), sizeof(hawq_jpeg_desc));
        const hawq_jpeg_desc &d = im.d;
        im.blocks = image_blocks(d);
        for (int32_t k = 0; k < (prog ? ph.n_scans : 1); ++k) {
            Scan s;
            s.prog = prog;
            memset(&s.sc, 0, sizeof s.sc);
            memset(s.dc, 0, sizeof s.dc);
            memset(s.ac, 0, sizeof s.ac);
            if (prog) {
                memcpy(&s.sc, blob.data() + ph.scan_off + (size_t)k * sizeof(hawq_jpeg_scan), sizeof(hawq_jpeg_scan));
                if (s.sc.image != i) continue;
                s.index = k;
                if (s.sc.ss == 0 && s.sc.ah == 0)
                    for (int c = 0; c < s.sc.ncomp; ++c) memcpy(&s.dc[c], blob.data() + s.sc.dc_off[c], sizeof(hawq_jpeg_huff));
                if (s.sc.ss > 0) memcpy(&s.ac[0], blob.data() + s.sc.ac_off, sizeof(hawq_jpeg_huff));
                s.units = jpeg_prog_units(d, s.sc);
            } else {
                s.index = i;
                s.sc.image = i, s.sc.ncomp = d.ncomp, s.sc.level = 1, s.sc.restart = d.restart, s.sc.n_intervals = d.n_intervals;
                s.sc.interval_off = d.interval_off, s.sc.stream_off = d.stream_off, s.sc.stream_len = d.stream_len;
                for (int c = 0; c < 3; ++c) {
                    memcpy(&s.dc[c], blob.data() + d.dc_off[c < d.ncomp ? c : 0], sizeof(hawq_jpeg_huff));
                    memcpy(&s.ac[c], blob.data() + d.ac_off[c < d.ncomp ? c : 0], sizeof(hawq_jpeg_huff));
                }
                s.units = d.mcus_x * d.mcus_y;
            }
            s.iv.resize((size_t)s.sc.n_intervals * 2);
            memcpy(s.iv.data(), blob.data() + s.sc.interval_off, s.iv.size() * sizeof(int32_t));
            s.stream = (uint8_t *)malloc(s.sc.stream_len ? s.sc.stream_len : 1);
            memcpy(s.stream, blob.data() + s.sc.stream_off, s.sc.stream_len);
            im.scans.push_back(s);
        }
        std::stable_sort(im.scans.begin(), im.scans.end(), [](const Scan &a, const Scan &b) { return a.sc.level < b.sc.level; });
        const size_t words = (size_t)im.blocks * 64;
        // the straight decode, scan after scan; the slab before every scan is kept, and what the decode knew at every unit
        std::vector<int16_t *> before;
        std::vector<std::vector<Witness>> seen(im.scans.size());
        std::vector<std::vector<int32_t>> serial_status(im.scans.size());
        int16_t *serial = (int16_t *)calloc(words, sizeof(int16_t));
        for (size_t at = 0; at < im.scans.size(); ++at) {
            const Scan &s = im.scans[at];
            before.push_back(copy_slab(serial, words));
            for (int32_t k = 0; k < s.sc.n_intervals; ++k) {
                seen[at].emplace_back();
                serial_status[at].push_back(run_interval(im, s, s.stream, s.iv, k, serial, seen[at].back()));
            }
        }
        for (const int32_t every : everies) {
            // 1: record, scan after scan
            std::vector<ScanRun> runs;
            int16_t *slab = (int16_t *)calloc(words, sizeof(int16_t));
            for (size_t at = 0; at < im.scans.size(); ++at) {
                const Scan &s = im.scans[at];
                runs.push_back(record_scan(im, s, s.stream, s.iv, slab, every));
                if (runs.back().status != serial_status[at]) ++bad, fprintf(stderr, "image %d scan %zu every %d: the recorder's status differs\n", i, at, every);
                for (int32_t k = 0; k < s.sc.n_intervals; ++k) {
                    const std::vector<hawq_jpeg_resume_seg> &segs = runs.back().segs[(size_t)k];
                    segments += (long)segs.size();
                    for (size_t n = 1; n < segs.size(); ++n) {
                        const hawq_jpeg_resume_seg &p = segs[n];
                        const Witness::At &w = seen[at][(size_t)k].at[(size_t)p.unit0];
                        bool same = p.pred[0] == w.pred[0] && p.pred[1] == w.pred[1] && p.pred[2] == w.pred[2] && p.eobrun == w.eobrun && p.byte - segs[n - 1].byte >= every;
                        if (w.dry == 0) {
                            int32_t byte, bit;
                            canonical(s.stream, s.iv[2 * k], s.iv[2 * k + 1], 8 * data_bytes(s.stream, s.iv[2 * k], w.pos) - w.nbits, byte, bit);
                            same = same && byte == p.byte && bit == p.bit;
                        }
                        if (!same) ++bad, fprintf(stderr, "image %d scan %zu interval %d every %d: point %zu at unit %d is not the decoder's state\n", i, at, k, every, n, p.unit0);
                        ++points, points_eob += p.eobrun > 0, points_bit += p.bit > 0;
                    }
                }
            }
            if (memcmp(slab, serial, words * sizeof(int16_t))) ++bad, fprintf(stderr, "image %d every %d: the recorder's slab differs\n", i, every);
            // 2: the segments in reverse order, level by level
            memset(slab, 0, words * sizeof(int16_t));
            for (size_t lo = 0; lo < im.scans.size();) {
                size_t hi = lo;
                while (hi < im.scans.size() && im.scans[hi].sc.level == im.scans[lo].sc.level) ++hi;
                for (size_t at = hi; at-- > lo;)
                    if (run_segments_reversed(im, im.scans[at], im.scans[at].stream, im.scans[at].iv, runs[at].segs, slab) != serial_status[at])
                        ++bad, fprintf(stderr, "image %d scan %zu every %d: the segments' status differs\n", i, at, every);
                lo = hi;
            }
            if (memcmp(slab, serial, words * sizeof(int16_t))) ++bad, fprintf(stderr, "image %d every %d: the segments' slab differs\n", i, every);
            free(slab);
            // 3, 4: damaged streams, scan by scan on the slab the scans before it left
            for (size_t at = 0; at < im.scans.size(); ++at) {
                Scan &s = im.scans[at];
                auto damaged_run = [&](const uint8_t *stream, const std::vector<int32_t> &iv) {
                    JpegNoHook none;
                    int16_t *a = copy_slab(before[at], words), *b = copy_slab(before[at], words);
                    std::vector<int32_t> want;
                    for (int32_t k = 0; k < s.sc.n_intervals; ++k) want.push_back(run_interval(im, s, stream, iv, k, a, none));
                    const ScanRun rec = record_scan(im, s, stream, iv, b, every);
                    bool same = rec.status == want && !memcmp(a, b, words * sizeof(int16_t));
                    memcpy(b, before[at], words * sizeof(int16_t));
                    same = same && run_segments_reversed(im, s, stream, iv, rec.segs, b) == want && !memcmp(a, b, words * sizeof(int16_t));
                    if (!same) ++bad, fprintf(stderr, "image %d scan %zu every %d: a damaged stream's segments differ from its serial decode\n", i, at, every);
                    ++damaged;
                    damaged_flagged += std::any_of(want.begin(), want.end(), [](int32_t v) { return v != 0; });
                    // the good stream's points on the damaged bytes
                    memcpy(b, before[at], words * sizeof(int16_t));
                    const std::vector<int32_t> got = run_segments_reversed(im, s, stream, iv, runs[at].segs, b);
                    ++stale;
                    stale_flagged += std::any_of(got.begin(), got.end(), [](int32_t v) { return v != 0; });
                    free(a), free(b);
                };
                for (int32_t cut = 0; cut < s.sc.stream_len; cut += 8) {
                    std::vector<int32_t> iv = s.iv;
                    for (int32_t &v : iv) v = v < cut ? v : cut;
                    uint8_t *part = (uint8_t *)malloc(cut ? cut : 1);
                    memcpy(part, s.stream, cut);
                    damaged_run(part, iv);
                    free(part);
                    ++intervals_cut;
                }
                uint64_t rng = seed * 0x9E3779B97F4A7C15ull + (uint64_t)s.index;
                for (int n = 0; n < 200 && s.sc.stream_len > 0; ++n) {
                    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                    const int32_t pos = (int32_t)((rng >> 33) % (uint64_t)s.sc.stream_len);
                    const uint8_t keep = s.stream[pos];
                    s.stream[pos] = (uint8_t)(rng >> 24);
                    damaged_run(s.stream, s.iv);
                    s.stream[pos] = keep;
                }
            }
        }
        free(serial);
        for (int16_t *p : before) free(p);
        for (Scan &s : im.scans) free(s.stream);
    }
    printf("images %d points %ld points_eobrun %ld points_bit %ld segments %ld cuts %ld damaged %ld damaged_flagged %ld stale %ld stale_flagged %ld bad %ld\n", hd.n_images,
           points, points_eob, points_bit, segments, intervals_cut, damaged, damaged_flagged, stale, stale_flagged, bad);
    return bad == 0 ? 0 : 1;
}
