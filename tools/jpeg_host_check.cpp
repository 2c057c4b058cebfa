// Host run of the JPEG decoder's arithmetic (hawq_amd/csrc/jpeg_entropy.h, jpeg_pixel.h - the text the kernels compile), meant to be built
// with -fsanitize=address,undefined and run on its own:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_host_check.cpp -o jpeg_host_check
//   jpeg_host_check BLOB EXPECTED OUT_BYTES [SEED]
//
// BLOB: a blob of hawq_amd.jpeg.plan_jpeg_batch that hawq_jpeg_batch_ok has passed; EXPECTED: OUT_BYTES bytes, the decoded images at the
// blob's out_off.  1. every image decodes to its expected bytes with status 0.  2. hostile input: every stream truncated at each eighth
// byte must end with a non-zero status; every stream with one byte overwritten (200 draws per stream, seeded by SEED and the image's index) must end with some status;
// both go on through stages 2 and 3.  Streams, coefficient slabs, planes and images live in heap blocks of their exact size, and the
// reader's source aborts on a position outside its interval, so an out-of-bounds access stops the program.  Exit 0: all of that held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../hawq_amd/csrc/jpeg_pixel.h"

namespace {
struct HostSrc {
    const uint8_t *p;
    int32_t first, end;
    uint8_t byte(int32_t pos) const {
        if (pos < first || pos >= end) {
            fprintf(stderr, "jpeg_host_check: the reader asked for byte %d outside its interval [%d, %d)\n", pos, first, end);
            abort();
        }
        return p[pos];
    }
};

std::vector<uint8_t> read_file(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "jpeg_host_check: cannot open %s\n", path);
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

struct Image {
    hawq_jpeg_desc d;
    hawq_jpeg_huff dc[3], ac[3];
    uint16_t qt[3][64];
    std::vector<int32_t> iv;   // [n_intervals][2]
};

// all three stages of one image on `stream` (exactly d.stream_len bytes) with the intervals `iv`; returns the status, rgb = H * W * 3 bytes
int32_t decode(const Image &im, const uint8_t *stream, const std::vector<int32_t> &iv, std::vector<uint8_t> &rgb) {
    const hawq_jpeg_desc &d = im.d;
    const int64_t blocks = image_blocks(d);
    int16_t *coef = (int16_t *)calloc((size_t)blocks * 64, sizeof(int16_t));
    uint8_t *planes = (uint8_t *)malloc((size_t)blocks * 64);
    const hawq_jpeg_huff *dc[3] = {&im.dc[0], &im.dc[1], &im.dc[2]}, *ac[3] = {&im.ac[0], &im.ac[1], &im.ac[2]};
    const int32_t mcus = d.mcus_x * d.mcus_y;
    int32_t status = 0;
    for (int32_t k = 0; k < d.n_intervals; ++k) {
        const int32_t mcu0 = d.restart ? k * d.restart : 0, n_mcu = d.restart ? (d.restart < mcus - mcu0 ? d.restart : mcus - mcu0) : mcus;
        JpegBits<HostSrc> br(HostSrc{stream, iv[2 * k], iv[2 * k + 1]}, iv[2 * k], iv[2 * k + 1]);
        const int32_t st = jpeg_decode_interval(br, d, dc, ac, mcu0, n_mcu, coef, true);
        if (st && !status) status = st;
    }
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
    free(coef);
    free(planes);
    return status;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: jpeg_host_check BLOB EXPECTED OUT_BYTES [SEED]\n");
        return 2;
    }
    const std::vector<uint8_t> blob = read_file(argv[1]), expected = read_file(argv[2]);
    const int64_t out_bytes = atoll(argv[3]);
    const uint64_t seed = argc > 4 ? strtoull(argv[4], nullptr, 10) : 1;
    if ((int64_t)expected.size() != out_bytes || blob.size() < sizeof(hawq_jpeg_batch_hdr)) {
        fprintf(stderr, "jpeg_host_check: sizes do not match\n");
        return 2;
    }
    hawq_jpeg_batch_hdr hd;
    memcpy(&hd, blob.data(), sizeof hd);
    long exact = 0, truncations = 0, truncations_flagged = 0, overwrites = 0, overwrites_flagged = 0;
    std::vector<uint8_t> rgb;
    for (int32_t i = 0; i < hd.n_images; ++i) {
        Image im;
        memcpy(&im.d, blob.data() + hd.desc_off + (size_t)i * sizeof(hawq_jpeg_desc), sizeof(hawq_jpeg_desc));
        const hawq_jpeg_desc &d = im.d;
        for (int c = 0; c < 3; ++c) {
            const int cc = c < d.ncomp ? c : 0;
            memcpy(&im.dc[c], blob.data() + d.dc_off[cc], sizeof(hawq_jpeg_huff));
            memcpy(&im.ac[c], blob.data() + d.ac_off[cc], sizeof(hawq_jpeg_huff));
            memcpy(im.qt[c], blob.data() + d.qt_off[cc], sizeof im.qt[c]);
        }
        im.iv.resize((size_t)d.n_intervals * 2);
        memcpy(im.iv.data(), blob.data() + d.interval_off, im.iv.size() * sizeof(int32_t));
        // the stream in a heap block of its exact size
        uint8_t *stream = (uint8_t *)malloc(d.stream_len ? d.stream_len : 1);
        memcpy(stream, blob.data() + d.stream_off, d.stream_len);
        int32_t st = decode(im, stream, im.iv, rgb);
        const bool same = st == 0 && d.out_off + (int64_t)rgb.size() <= out_bytes && memcmp(rgb.data(), expected.data() + d.out_off, rgb.size()) == 0;
        if (!same) {
            size_t at = 0;
            while (st == 0 && at < rgb.size() && rgb[at] == expected[d.out_off + at]) ++at;
            fprintf(stderr, "image %d (%d x %d, %d component(s), %d x %d): status %d, first differing byte %zu\n", i, d.width, d.height, d.ncomp, d.hs, d.vs,
                    st, at);
        }
        exact += same;
        // truncations: every interval clipped to the first `cut` bytes
        for (int32_t cut = 0; cut < d.stream_len; cut += 8) {
            std::vector<int32_t> iv = im.iv;
            for (int32_t &v : iv) v = v < cut ? v : cut;
            uint8_t *part = (uint8_t *)malloc(cut ? cut : 1);
            memcpy(part, stream, cut);
            st = decode(im, part, iv, rgb);
            free(part);
            ++truncations;
            truncations_flagged += st != 0;
        }
        // single-byte overwrites: draws of a 64-bit LCG seeded per image (tests/jpeg_model.py: overwrite_draws makes the same ones)
        uint64_t rng = seed * 0x9E3779B97F4A7C15ull + (uint64_t)i;
        for (int n = 0; n < 200 && d.stream_len > 0; ++n) {
            rng = rng * 6364136223846793005ull + 1442695040888963407ull;
            const int32_t at = (int32_t)((rng >> 33) % (uint64_t)d.stream_len);
            const uint8_t keep = stream[at];
            stream[at] = (uint8_t)(rng >> 24);
            st = decode(im, stream, im.iv, rgb);
            stream[at] = keep;
            ++overwrites;
            overwrites_flagged += st != 0;
        }
        free(stream);
    }
    printf("images %d exact %ld truncations %ld truncations_flagged %ld overwrites %ld overwrites_flagged %ld\n", hd.n_images, exact, truncations, truncations_flagged, overwrites,
           overwrites_flagged);
    return exact == hd.n_images && truncations_flagged == truncations ? 0 : 1;
}
