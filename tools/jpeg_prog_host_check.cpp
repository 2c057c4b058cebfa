// Host run of the progressive JPEG scan decoders (hawq_amd/csrc/jpeg_prog.h - the text jpeg_prog_kernel compiles) with the host IDCT and
// colour text of jpeg_pixel.h, meant to be built with -fsanitize=address,undefined and run on its own:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_prog_host_check.cpp -o jpeg_prog_host_check
//   jpeg_prog_host_check BLOB EXPECTED OUT_BYTES [SEED]
//
// BLOB: a blob of hawq_amd.jpeg.plan_jpeg_prog_batch that hawq_jpeg_prog_ok has passed; EXPECTED: OUT_BYTES bytes, the decoded images at
// the blob's out_off.  1. every image, decoded level by level and interval by interval, gives its expected bytes with status 0.
// 2. hostile input, per scan: its stream truncated at each eighth byte must end with a non-zero status; its stream with one byte
// overwritten (200 draws, seeded by SEED and the scan's index in the scan table) must end with some status or a clean result.  A damaged
// scan runs on the coefficients the scans before it (in level order) left, and every later scan runs behind it on what it left, so the
// refinement decoders meet coefficients no encoder wrote; images of at most 1024 blocks go on through stages 2 and 3.
// Streams, coefficient slabs, planes and images live in heap blocks of their exact size; the reader's source aborts on a position
// outside its interval, and the block source aborts on a block outside the image or on a change outside the scan's band ss .. se, so
// an out-of-bounds access stops the program.  Exit 0: all of that held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../hawq_amd/csrc/jpeg_pixel.h"
#include "../hawq_amd/csrc/jpeg_prog.h"

namespace {
struct HostSrc {
    const uint8_t *p;
    int32_t first, end;
    uint8_t byte(int32_t pos) const {
        if (pos < first || pos >= end) {
            fprintf(stderr, "jpeg_prog_host_check: the reader asked for byte %d outside its interval [%d, %d)\n", pos, first, end);
            abort();
        }
        return p[pos];
    }
};

// the slab of one image, handed out block by block
struct HostBlk {
    int16_t *coef;
    int64_t blocks;
    int16_t before[64];
    void inside(int64_t b) const {
        if (b < 0 || b >= blocks) {
            fprintf(stderr, "jpeg_prog_host_check: block %lld outside the image's %lld\n", (long long)b, (long long)blocks);
            abort();
        }
    }
    int16_t *open(int64_t b) {
        inside(b);
        memcpy(before, coef + b * 64, sizeof before);
        return coef + b * 64;
    }
    int16_t *open_fresh(int64_t b) { return open(b); }
    uint64_t history(const int16_t *c) const {
        uint64_t m = 0;
        for (int k = 0; k < 64; ++k) m |= (uint64_t)(c[jpeg_natural(k)] != 0) << k;
        return m;
    }
    void close(int64_t b, int ss, int se) {
        for (int n = 0; n < 64; ++n) {
            const int zz = jpeg_zigzag_of(n);
            if ((zz < ss || zz > se) && coef[b * 64 + n] != before[n]) {
                fprintf(stderr, "jpeg_prog_host_check: a scan of band %d..%d changed coefficient %d (zig-zag %d)\n", ss, se, n, zz);
                abort();
            }
        }
    }
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
        fprintf(stderr, "jpeg_prog_host_check: cannot open %s\n", path);
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

struct Scan {
    hawq_jpeg_scan sc;
    int32_t index;   // in the blob's scan table
    hawq_jpeg_huff dc[3], ac;
    std::vector<int32_t> iv;   // [n_intervals][2]
    uint8_t *stream;           // heap block of exactly sc.stream_len bytes
};

struct Image {
    hawq_jpeg_desc d;
    uint16_t qt[3][64];
    std::vector<Scan> scans;   // in level order (stable: file order within a level)
};

// one scan, interval by interval, on `stream` with the intervals `iv`
int32_t run_scan(const Image &im, const Scan &s, const uint8_t *stream, const std::vector<int32_t> &iv, int16_t *coef) {
    const hawq_jpeg_huff *dc[3] = {&s.dc[0], &s.dc[1], &s.dc[2]};
    const int32_t units = jpeg_prog_units(im.d, s.sc);
    int32_t status = 0;
    for (int32_t k = 0; k < s.sc.n_intervals; ++k) {
        const int32_t unit0 = s.sc.restart ? k * s.sc.restart : 0, n_units = s.sc.restart ? std::min(s.sc.restart, units - unit0) : units;
        JpegBits<HostSrc> br(HostSrc{stream, iv[2 * k], iv[2 * k + 1]}, iv[2 * k], iv[2 * k + 1]);
        HostBlk blk{coef, image_blocks(im.d), {0}};
        const int32_t st = jpeg_prog_interval(br, im.d, s.sc, dc, &s.ac, unit0, n_units, blk);
        if (st && !status) status = st;
    }
    return status;
}

// stages 2 and 3 of one image
void pixels(const Image &im, const int16_t *coef, std::vector<uint8_t> &rgb) {
    const hawq_jpeg_desc &d = im.d;
    uint8_t *planes = (uint8_t *)malloc((size_t)image_blocks(d) * 64);
    int64_t comp0 = 0;
    for (int c = 0; c < d.ncomp; ++c) {
        const int64_t bw = (int64_t)d.mcus_x * jpeg_comp_h(d, c), bh = (int64_t)d.mcus_y * jpeg_comp_v(d, c);
        for (int64_t b = 0; b < bw * bh; ++b)
            jpeg_idct_block(coef + (comp0 + b) * 64, im.qt[c], planes + comp0 * 64 + (b / bw) * 8 * bw * 8 + (b % bw) * 8, bw * 8);
        comp0 += bw * bh;
    }
    rgb.assign((size_t)d.width * d.height * 3, 0);
    for (int32_t y = 0; y < d.height; ++y)
        for (int32_t x = 0; x < d.width; ++x) jpeg_pixel(d, planes, x, y, rgb.data() + ((size_t)y * d.width + x) * 3);
    free(planes);
}

// scan `at` (position in level order) on a damaged stream, on the slab the scans before it left (`before`), then the scans behind it
int32_t decode_damaged(const Image &im, size_t at, const int16_t *before, const uint8_t *stream, const std::vector<int32_t> &iv, std::vector<uint8_t> &rgb) {
    const size_t words = (size_t)image_blocks(im.d) * 64;
    int16_t *coef = (int16_t *)malloc(words * sizeof(int16_t));
    memcpy(coef, before, words * sizeof(int16_t));
    int32_t status = run_scan(im, im.scans[at], stream, iv, coef);
    for (size_t k = at + 1; k < im.scans.size(); ++k) {
        const int32_t st = run_scan(im, im.scans[k], im.scans[k].stream, im.scans[k].iv, coef);
        if (st && !status) status = st;
    }
    if (image_blocks(im.d) <= 1024) pixels(im, coef, rgb);
    free(coef);
    return status;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: jpeg_prog_host_check BLOB EXPECTED OUT_BYTES [SEED]\n");
        return 2;
    }
    const std::vector<uint8_t> blob = read_file(argv[1]), expected = read_file(argv[2]);
    const int64_t out_bytes = atoll(argv[3]);
    const uint64_t seed = argc > 4 ? strtoull(argv[4], nullptr, 10) : 1;
    if ((int64_t)expected.size() != out_bytes || blob.size() < sizeof(hawq_jpeg_batch_hdr) + sizeof(hawq_jpeg_prog_hdr)) {
        fprintf(stderr, "jpeg_prog_host_check: sizes do not match\n");
        return 2;
    }
    hawq_jpeg_batch_hdr hd;
    hawq_jpeg_prog_hdr ph;
    memcpy(&hd, blob.data(), sizeof hd);
    memcpy(&ph, blob.data() + sizeof hd, sizeof ph);
    long exact = 0, scans = 0, truncations = 0, truncations_flagged = 0, overwrites = 0, overwrites_flagged = 0;
    int32_t levels = 0;
    std::vector<uint8_t> rgb;
    for (int32_t i = 0; i < hd.n_images; ++i) {
        Image im;
        memcpy(&im.d, blob.data() + hd.desc_off + (size_t)i * sizeof(hawq_jpeg_desc), sizeof(hawq_jpeg_desc));
        const hawq_jpeg_desc &d = im.d;
        for (int c = 0; c < 3; ++c) memcpy(im.qt[c], blob.data() + d.qt_off[c < d.ncomp ? c : 0], sizeof im.qt[c]);
        for (int32_t k = 0; k < ph.n_scans; ++k) {
            Scan s;
            memcpy(&s.sc, blob.data() + ph.scan_off + (size_t)k * sizeof(hawq_jpeg_scan), sizeof(hawq_jpeg_scan));
            if (s.sc.image != i) continue;
            s.index = k;
            memset(s.dc, 0, sizeof s.dc);
            memset(&s.ac, 0, sizeof s.ac);
            if (s.sc.ss == 0 && s.sc.ah == 0)
                for (int c = 0; c < s.sc.ncomp; ++c) memcpy(&s.dc[c], blob.data() + s.sc.dc_off[c], sizeof(hawq_jpeg_huff));
            if (s.sc.ss > 0) memcpy(&s.ac, blob.data() + s.sc.ac_off, sizeof(hawq_jpeg_huff));
            s.iv.resize((size_t)s.sc.n_intervals * 2);
            memcpy(s.iv.data(), blob.data() + s.sc.interval_off, s.iv.size() * sizeof(int32_t));
            s.stream = (uint8_t *)malloc(s.sc.stream_len ? s.sc.stream_len : 1);
            memcpy(s.stream, blob.data() + s.sc.stream_off, s.sc.stream_len);
            levels = std::max(levels, s.sc.level);
            im.scans.push_back(s);
        }
        std::stable_sort(im.scans.begin(), im.scans.end(), [](const Scan &a, const Scan &b) { return a.sc.level < b.sc.level; });
        scans += (long)im.scans.size();
        // the intact file, level by level; the slab before every scan is kept for the damaged runs
        const size_t words = (size_t)image_blocks(d) * 64;
        std::vector<int16_t *> before;
        int16_t *coef = (int16_t *)calloc(words, sizeof(int16_t));
        int32_t st = 0;
        for (const Scan &s : im.scans) {
            int16_t *snap = (int16_t *)malloc(words * sizeof(int16_t));
            memcpy(snap, coef, words * sizeof(int16_t));
            before.push_back(snap);
            const int32_t one = run_scan(im, s, s.stream, s.iv, coef);
            if (one && !st) st = one;
        }
        pixels(im, coef, rgb);
        free(coef);
        const bool same = st == 0 && d.out_off + (int64_t)rgb.size() <= out_bytes && memcmp(rgb.data(), expected.data() + d.out_off, rgb.size()) == 0;
        if (!same) {
            size_t at = 0;
            while (st == 0 && at < rgb.size() && rgb[at] == expected[d.out_off + at]) ++at;
            fprintf(stderr, "image %d (%d x %d, %d component(s), %d x %d, %zu scans): status %d, first differing byte %zu\n", i, d.width, d.height, d.ncomp, d.hs,
                    d.vs, im.scans.size(), st, at);
        }
        exact += same;
        for (size_t at = 0; at < im.scans.size(); ++at) {
            Scan &s = im.scans[at];
            // truncations: every interval of the scan clipped to the first `cut` bytes
            for (int32_t cut = 0; cut < s.sc.stream_len; cut += 8) {
                std::vector<int32_t> iv = s.iv;
                for (int32_t &v : iv) v = v < cut ? v : cut;
                uint8_t *part = (uint8_t *)malloc(cut ? cut : 1);
                memcpy(part, s.stream, cut);
                st = decode_damaged(im, at, before[at], part, iv, rgb);
                free(part);
                ++truncations;
                truncations_flagged += st != 0;
            }
            // single-byte overwrites: draws of a 64-bit LCG seeded per scan (tests/jpeg_prog_model.py: overwrite_draws makes the same ones)
            uint64_t rng = seed * 0x9E3779B97F4A7C15ull + (uint64_t)s.index;
            for (int n = 0; n < 200 && s.sc.stream_len > 0; ++n) {
                rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                const int32_t pos = (int32_t)((rng >> 33) % (uint64_t)s.sc.stream_len);
                const uint8_t keep = s.stream[pos];
                s.stream[pos] = (uint8_t)(rng >> 24);
                st = decode_damaged(im, at, before[at], s.stream, s.iv, rgb);
                s.stream[pos] = keep;
                ++overwrites;
                overwrites_flagged += st != 0;
            }
        }
        for (int16_t *p : before) free(p);
        for (Scan &s : im.scans) free(s.stream);
    }
    printf("images %d exact %ld scans %ld levels %d truncations %ld truncations_flagged %ld overwrites %ld overwrites_flagged %ld\n", hd.n_images, exact, scans, levels,
           truncations, truncations_flagged, overwrites, overwrites_flagged);
    return exact == hd.n_images && truncations_flagged == truncations ? 0 : 1;
}
