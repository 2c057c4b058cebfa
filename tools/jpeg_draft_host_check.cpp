// Host run of the reduced-size JPEG decode: the n x n inverse DCTs and the scaled pixel of hawq_amd/csrc/jpeg_pixel.h -
// the text jpeg_idct_scaled_kernel and jpeg_colour_scaled_kernel compile - behind the entropy decoders of jpeg_entropy.h / jpeg_prog.h,
// meant to be built with -fsanitize=address,undefined and run on its own:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_draft_host_check.cpp -o jpeg_draft_host_check
//   jpeg_draft_host_check PACK [SEED]
//
// PACK: entries one after the other, each four int64 (kind: 0 a blob of hawq_amd.jpeg.plan_jpeg_batch, 1 one of plan_jpeg_prog_batch;
// blob bytes; output bytes; 0), the blob, and the expected output (the decoded images at the blob's out_off); the plans are made with
// ``draft`` and their checker has passed them.  1. every image decodes to its expected bytes with status 0, at the scale its descriptor
// names.  2. hostile input, per stream (a baseline image's, or one scan's of a progressive image): truncated at each eighth byte it
// must end with a non-zero status; with one byte overwritten (200 draws, seeded by SEED and the stream's ordinal in the pack) it must
// end with some status or a clean result; both go on through stages 2 and 3 at the image's scale.  Streams, coefficient slabs, planes
// and images live in heap blocks of their exact size - planes and images of the SCALED geometry - and the reader's source aborts on a
// position outside its interval, so an out-of-bounds access stops the program.  Exit 0: all of that held.
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
            fprintf(stderr, "jpeg_draft_host_check: the reader asked for byte %d outside its interval [%d, %d)\n", pos, first, end);
            abort();
        }
        return p[pos];
    }
};

// the slab of one image, handed out block by block (jpeg_prog.h)
struct HostBlk {
    int16_t *coef;
    int64_t blocks;
    void inside(int64_t b) const {
        if (b < 0 || b >= blocks) {
            fprintf(stderr, "jpeg_draft_host_check: block %lld outside the image's %lld\n", (long long)b, (long long)blocks);
            abort();
        }
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
        fprintf(stderr, "jpeg_draft_host_check: cannot open %s\n", path);
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

// One entropy-coded stream: the only one of a baseline image, or one scan of a progressive image
struct Stream {
    hawq_jpeg_scan sc;                 // progressive only
    hawq_jpeg_huff dc[3], ac[3];       // baseline: per component; progressive: dc per scan component, ac[0]
    std::vector<int32_t> iv;           // [n_intervals][2]
    uint8_t *bytes;                    // heap block of exactly `len` bytes
    int32_t len, n_intervals;
};

struct Image {
    hawq_jpeg_desc d;
    bool prog;
    uint16_t qt[3][64];
    std::vector<Stream> streams;       // progressive: in level order (stable: file order within a level)
};

int32_t run_stream(const Image &im, const Stream &s, const uint8_t *bytes, const std::vector<int32_t> &iv, int16_t *coef) {
    const hawq_jpeg_desc &d = im.d;
    const hawq_jpeg_huff *dc[3] = {&s.dc[0], &s.dc[1], &s.dc[2]}, *ac[3] = {&s.ac[0], &s.ac[1], &s.ac[2]};
    int32_t status = 0;
    if (!im.prog) {
        const int32_t mcus = d.mcus_x * d.mcus_y;
        for (int32_t k = 0; k < d.n_intervals; ++k) {
            const int32_t mcu0 = d.restart ? k * d.restart : 0, n_mcu = d.restart ? std::min(d.restart, mcus - mcu0) : mcus;
            JpegBits<HostSrc> br(HostSrc{bytes, iv[2 * k], iv[2 * k + 1]}, iv[2 * k], iv[2 * k + 1]);
            const int32_t st = jpeg_decode_interval(br, d, dc, ac, mcu0, n_mcu, coef, true);
            if (st && !status) status = st;
        }
        return status;
    }
    const int32_t units = jpeg_prog_units(d, s.sc);
    for (int32_t k = 0; k < s.sc.n_intervals; ++k) {
        const int32_t unit0 = s.sc.restart ? k * s.sc.restart : 0, n_units = s.sc.restart ? std::min(s.sc.restart, units - unit0) : units;
        JpegBits<HostSrc> br(HostSrc{bytes, iv[2 * k], iv[2 * k + 1]}, iv[2 * k], iv[2 * k + 1]);
        HostBlk blk{coef, image_blocks(d)};
        const int32_t st = jpeg_prog_interval(br, d, s.sc, dc, &s.ac[0], unit0, n_units, blk);
        if (st && !status) status = st;
    }
    return status;
}

// Stages 2 and 3 at the descriptor's scale; planes and image in heap blocks of the scaled geometry's exact size.  rgb is the caller's to free.
uint8_t *pixels(const Image &im, const int16_t *coef, size_t *rgb_bytes) {
    const hawq_jpeg_desc &d = im.d;
    int64_t plane_bytes = 0;
    for (int c = 0; c < d.ncomp; ++c) plane_bytes += (int64_t)d.mcus_x * jpeg_comp_h(d, c) * d.mcus_y * jpeg_comp_v(d, c) * jpeg_comp_n(d, c) * jpeg_comp_n(d, c);
    uint8_t *planes = (uint8_t *)malloc((size_t)plane_bytes);
    int64_t comp0 = 0, plane0 = 0;
    for (int c = 0; c < d.ncomp; ++c) {
        const int64_t bw = (int64_t)d.mcus_x * jpeg_comp_h(d, c), bh = (int64_t)d.mcus_y * jpeg_comp_v(d, c);
        const int n = jpeg_comp_n(d, c);
        for (int64_t b = 0; b < bw * bh; ++b)
            jpeg_idct_block_n(coef + (comp0 + b) * 64, im.qt[c], n, planes + plane0 + (b / bw) * n * bw * n + (b % bw) * n, bw * n);
        comp0 += bw * bh, plane0 += bw * bh * n * n;
    }
    const int32_t ow = jpeg_out_width(d), oh = jpeg_out_height(d);
    *rgb_bytes = (size_t)ow * oh * 3;
    uint8_t *rgb = (uint8_t *)malloc(*rgb_bytes);
    for (int32_t y = 0; y < oh; ++y)
        for (int32_t x = 0; x < ow; ++x) {
            uint8_t *o = rgb + ((size_t)y * ow + x) * 3;
            if (d.scale > 1)
                jpeg_pixel_scaled(d, planes, x, y, o);
            else
                jpeg_pixel(d, planes, x, y, o);
        }
    free(planes);
    return rgb;
}

// every stream of the image in order on a zeroed slab, stream `damaged` (-1: none) replaced by `bytes` / `iv` -> status, the image in rgb
int32_t decode(const Image &im, int damaged, const uint8_t *bytes, const std::vector<int32_t> *iv, uint8_t **rgb, size_t *rgb_bytes) {
    int16_t *coef = (int16_t *)calloc((size_t)image_blocks(im.d) * 64, sizeof(int16_t));
    int32_t status = 0;
    for (size_t k = 0; k < im.streams.size(); ++k) {
        const Stream &s = im.streams[k];
        const int32_t st = (int)k == damaged ? run_stream(im, s, bytes, *iv, coef) : run_stream(im, s, s.bytes, s.iv, coef);
        if (st && !status) status = st;
    }
    *rgb = pixels(im, coef, rgb_bytes);
    free(coef);
    return status;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: jpeg_draft_host_check PACK [SEED]\n");
        return 2;
    }
    const std::vector<uint8_t> pack = read_file(argv[1]);
    const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    long images = 0, exact = 0, scaled = 0, streams = 0, truncations = 0, truncations_flagged = 0, overwrites = 0, overwrites_flagged = 0;
    long by_scale[9] = {0};
    size_t at = 0;
    while (at < pack.size()) {
        int64_t head[4];
        if (pack.size() - at < sizeof head) {
            fprintf(stderr, "jpeg_draft_host_check: a cut entry\n");
            return 2;
        }
        memcpy(head, pack.data() + at, sizeof head);
        at += sizeof head;
        const int64_t kind = head[0], blob_bytes = head[1], out_bytes = head[2];
        if ((kind != 0 && kind != 1) || blob_bytes < (int64_t)sizeof(hawq_jpeg_batch_hdr) || out_bytes < 0 || (int64_t)(pack.size() - at) < blob_bytes + out_bytes) {
            fprintf(stderr, "jpeg_draft_host_check: a bad entry\n");
            return 2;
        }
        const uint8_t *blob = pack.data() + at, *expected = blob + blob_bytes;
        at += (size_t)(blob_bytes + out_bytes);
        hawq_jpeg_batch_hdr hd;
        hawq_jpeg_prog_hdr ph = {};
        memcpy(&hd, blob, sizeof hd);
        if (kind == 1) memcpy(&ph, blob + sizeof hd, sizeof ph);
        for (int32_t i = 0; i < hd.n_images; ++i, ++images) {
            Image im;
            im.prog = kind == 1;
            memcpy(&im.d, blob + hd.desc_off + (size_t)i * sizeof(hawq_jpeg_desc), sizeof(hawq_jpeg_desc));
            const hawq_jpeg_desc &d = im.d;
            if (d.scale != 0 && d.scale != 1 && d.scale != 2 && d.scale != 4 && d.scale != 8) {
                fprintf(stderr, "jpeg_draft_host_check: image %ld names the scale %d\n", images, d.scale);
                return 2;
            }
            scaled += d.scale > 1;
            ++by_scale[jpeg_scale(d)];
            for (int c = 0; c < 3; ++c) memcpy(im.qt[c], blob + d.qt_off[c < d.ncomp ? c : 0], sizeof im.qt[c]);
            if (!im.prog) {
                Stream s;
                memset(&s.sc, 0, sizeof s.sc);
                for (int c = 0; c < 3; ++c) {
                    const int cc = c < d.ncomp ? c : 0;
                    memcpy(&s.dc[c], blob + d.dc_off[cc], sizeof(hawq_jpeg_huff));
                    memcpy(&s.ac[c], blob + d.ac_off[cc], sizeof(hawq_jpeg_huff));
                }
                s.len = d.stream_len, s.n_intervals = d.n_intervals;
                s.iv.resize((size_t)d.n_intervals * 2);
                memcpy(s.iv.data(), blob + d.interval_off, s.iv.size() * sizeof(int32_t));
                s.bytes = (uint8_t *)malloc(s.len ? s.len : 1);
                memcpy(s.bytes, blob + d.stream_off, s.len);
                im.streams.push_back(s);
            } else {
                for (int32_t k = 0; k < ph.n_scans; ++k) {
                    Stream s;
                    memcpy(&s.sc, blob + ph.scan_off + (size_t)k * sizeof(hawq_jpeg_scan), sizeof(hawq_jpeg_scan));
                    if (s.sc.image != i) continue;
                    memset(s.dc, 0, sizeof s.dc);
                    memset(s.ac, 0, sizeof s.ac);
                    if (s.sc.ss == 0 && s.sc.ah == 0)
                        for (int c = 0; c < s.sc.ncomp; ++c) memcpy(&s.dc[c], blob + s.sc.dc_off[c], sizeof(hawq_jpeg_huff));
                    if (s.sc.ss > 0) memcpy(&s.ac[0], blob + s.sc.ac_off, sizeof(hawq_jpeg_huff));
                    s.len = s.sc.stream_len, s.n_intervals = s.sc.n_intervals;
                    s.iv.resize((size_t)s.sc.n_intervals * 2);
                    memcpy(s.iv.data(), blob + s.sc.interval_off, s.iv.size() * sizeof(int32_t));
                    s.bytes = (uint8_t *)malloc(s.len ? s.len : 1);
                    memcpy(s.bytes, blob + s.sc.stream_off, s.len);
                    im.streams.push_back(s);
                }
                std::stable_sort(im.streams.begin(), im.streams.end(), [](const Stream &a, const Stream &b) { return a.sc.level < b.sc.level; });
            }
            uint8_t *rgb;
            size_t rgb_bytes;
            int32_t st = decode(im, -1, nullptr, nullptr, &rgb, &rgb_bytes);
            const bool same = st == 0 && d.out_off + (int64_t)rgb_bytes <= out_bytes && memcmp(rgb, expected + d.out_off, rgb_bytes) == 0;
            if (!same) {
                size_t diff = 0;
                while (st == 0 && diff < rgb_bytes && d.out_off + (int64_t)diff < out_bytes && rgb[diff] == expected[d.out_off + diff]) ++diff;
                fprintf(stderr, "image %ld (%d x %d at 1/%d, %d component(s), %d x %d): status %d, first differing byte %zu of %zu\n", images, d.width, d.height,
                        jpeg_scale(d), d.ncomp, d.hs, d.vs, st, diff, rgb_bytes);
            }
            free(rgb);
            exact += same;
            for (size_t k = 0; k < im.streams.size(); ++k, ++streams) {
                Stream &s = im.streams[k];
                // truncations: every interval of the stream clipped to the first `cut` bytes
                for (int32_t cut = 0; cut < s.len; cut += 8) {
                    std::vector<int32_t> iv = s.iv;
                    for (int32_t &v : iv) v = v < cut ? v : cut;
                    uint8_t *part = (uint8_t *)malloc(cut ? cut : 1);
                    memcpy(part, s.bytes, cut);
                    st = decode(im, (int)k, part, &iv, &rgb, &rgb_bytes);
                    free(part);
                    free(rgb);
                    ++truncations;
                    truncations_flagged += st != 0;
                }
                // single-byte overwrites: draws of a 64-bit LCG seeded per stream
                uint64_t rng = seed * 0x9E3779B97F4A7C15ull + (uint64_t)streams;
                for (int n = 0; n < 200 && s.len > 0; ++n) {
                    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                    const int32_t pos = (int32_t)((rng >> 33) % (uint64_t)s.len);
                    const uint8_t keep = s.bytes[pos];
                    s.bytes[pos] = (uint8_t)(rng >> 24);
                    st = decode(im, (int)k, s.bytes, &s.iv, &rgb, &rgb_bytes);
                    s.bytes[pos] = keep;
                    free(rgb);
                    ++overwrites;
                    overwrites_flagged += st != 0;
                }
            }
            for (Stream &s : im.streams) free(s.bytes);
        }
    }
    printf("images %ld exact %ld scaled %ld half %ld quarter %ld eighth %ld streams %ld truncations %ld truncations_flagged %ld overwrites %ld overwrites_flagged %ld\n", images,
           exact, scaled, by_scale[2], by_scale[4], by_scale[8], streams, truncations, truncations_flagged, overwrites, overwrites_flagged);
    return exact == images && truncations_flagged == truncations ? 0 : 1;
}
