// Host run of the many-lane entropy decoder (hawq_amd/csrc/jpeg_sync.h - the text jpeg_sync_kernel compiles) against the serial one
// (jpeg_entropy.h), meant to be built with -fsanitize=address,undefined and run on its own:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_sync_host_check.cpp -o jpeg_sync_host_check
//   jpeg_sync_host_check BLOB [SEED [FIRST STEP]]
//
// (images FIRST, FIRST + STEP, ... of the blob: several processes share a large one)
// BLOB: a blob of hawq_amd.jpeg.plan_jpeg_batch that hawq_jpeg_batch_ok has passed.  The lanes of an interval run one after the other
// with the kernel's own lane function, round structure (a round reads the ends of the round before), scan and write pass; every interval
// of at least one byte goes this way.  1. every image at sub_bytes 16, 32, 64 and 128: the slab equals, block for block, the one
// jpeg_decode_interval writes, the status is equal, the rounds are <= n, and the lane decodes number n + the starts that changed.
// 2. hostile input at sub_bytes 16 and 128: every stream truncated at each eighth byte and with one byte overwritten (200 draws per
// stream, seeded by SEED and the image's index, as tools/jpeg_host_check.cpp): the status equals the serial decoder's, and where it is
// zero so do the slabs.  Stream, slab and scratch live in heap blocks of their exact size, and the readers' source aborts on a position
// outside its interval, so an out-of-bounds access stops the program.  Exit 0: all of that held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../hawq_amd/csrc/jpeg_sync.h"

namespace {
struct HostSrc {
    const uint8_t *p;
    int32_t first, end;
    uint8_t byte(int32_t pos) const {
        if (pos < first || pos >= end) {
            fprintf(stderr, "jpeg_sync_host_check: the reader asked for byte %d outside its interval [%d, %d)\n", pos, first, end);
            abort();
        }
        return p[pos];
    }
};

std::vector<uint8_t> read_file(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "jpeg_sync_host_check: cannot open %s\n", path);
        exit(2);
    }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

int64_t image_blocks(const hawq_jpeg_desc &d) { return (int64_t)d.mcus_x * d.mcus_y * jpeg_sync_bpm(d); }

struct Image {
    hawq_jpeg_desc d;
    hawq_jpeg_huff huff[6];                 // dc, ac per component, as the kernel keeps them in LDS
    uint16_t lut[6][JPEG_SYNC_LUT_SIZE];    // built as the kernel builds them
    std::vector<int32_t> iv;                // [n_intervals][2]
    JpegSyncTables tables() const { return JpegSyncTables{huff, &lut[0][0]}; }
};

struct Tally {
    long rounds_max = 0, n_max = 0, decodes = 0, changes = 0, lanes = 0, round_overruns = 0, rounds_last = 0, n_last = 0;
};

// the serial decoder: one interval after the other into `coef` (zeroed, exactly the image's blocks)
int32_t serial(const Image &im, const uint8_t *stream, const std::vector<int32_t> &iv, int16_t *coef) {
    const hawq_jpeg_desc &d = im.d;
    const hawq_jpeg_huff *dc[3] = {&im.huff[0], &im.huff[2], &im.huff[4]}, *ac[3] = {&im.huff[1], &im.huff[3], &im.huff[5]};
    const int32_t mcus = d.mcus_x * d.mcus_y;
    int32_t status = 0;
    for (int32_t k = 0; k < d.n_intervals; ++k) {
        const int32_t mcu0 = d.restart ? k * d.restart : 0, n_mcu = d.restart ? (d.restart < mcus - mcu0 ? d.restart : mcus - mcu0) : mcus;
        JpegBits<HostSrc> br(HostSrc{stream, iv[2 * k], iv[2 * k + 1]}, iv[2 * k], iv[2 * k + 1]);
        const int32_t st = jpeg_decode_interval(br, d, dc, ac, mcu0, n_mcu, coef, true);
        if (st && !status) status = st;
    }
    return status;
}

// the many-lane decoder, lane after lane
int32_t synced(const Image &im, const uint8_t *stream, const std::vector<int32_t> &iv, int32_t S, int16_t *coef, Tally &tally) {
    const hawq_jpeg_desc &d = im.d;
    const JpegSyncTables tb = im.tables();
    const hawq_jpeg_huff *dc[3] = {&im.huff[0], &im.huff[2], &im.huff[4]}, *ac[3] = {&im.huff[1], &im.huff[3], &im.huff[5]};
    const int32_t mcus = d.mcus_x * d.mcus_y;
    int32_t status = 0;
    for (int32_t k = 0; k < d.n_intervals; ++k) {
        const int32_t mcu0 = d.restart ? k * d.restart : 0, n_mcu = d.restart ? (d.restart < mcus - mcu0 ? d.restart : mcus - mcu0) : mcus;
        const int32_t first = iv[2 * k], last = iv[2 * k + 1];
        if (last - first < 1) {   // no byte, no lane: the serial wave takes it (min_sync_bytes >= 1)
            JpegBits<HostSrc> br(HostSrc{stream, first, last}, first, last);
            const int32_t st = jpeg_decode_interval(br, d, dc, ac, mcu0, n_mcu, coef, true);
            if (st && !status) status = st;
            continue;
        }
        const int32_t n = (last - first + S - 1) / S;
        hawq_jpeg_sync_sub *sub = (hawq_jpeg_sync_sub *)malloc((size_t)n * sizeof(hawq_jpeg_sync_sub));
        HostSrc src{stream, first, last};
        long decodes = 0, changes = 0, rounds = 1;
        for (int32_t i = 0; i < n; ++i) {
            sub[i].start_pos = jpeg_sync_guess(src, first, i, S), sub[i].start_uk = 0;
            jpeg_sync_lane(src, d, tb, last, jpeg_sync_limit(first, i, n, S), S, sub[i], nullptr);
            ++decodes;
        }
        for (int32_t r = 1; r < n; ++r) {
            long changed = 0;
            for (int32_t i = 1; i < n; ++i) {
                const int32_t pos = sub[i - 1].end_pos, uk = sub[i - 1].end_uk;
                if (pos >= 0 && (pos != sub[i].start_pos || uk != sub[i].start_uk)) {
                    sub[i].start_pos = pos, sub[i].start_uk = uk;
                    sub[i].blocks = -1;
                    ++changed;
                }
            }
            if (!changed) break;
            changes += changed;
            for (int32_t i = 0; i < n; ++i) {
                if (sub[i].blocks != -1) continue;
                jpeg_sync_lane(src, d, tb, last, jpeg_sync_limit(first, i, n, S), S, sub[i], nullptr);
                ++decodes;
            }
            ++rounds;
        }
        // the fixed point: nobody would change any more
        for (int32_t i = 1; i < n; ++i)
            if (sub[i - 1].end_pos >= 0 && (sub[i - 1].end_pos != sub[i].start_pos || sub[i - 1].end_uk != sub[i].start_uk)) ++tally.round_overruns;
        if (rounds > n) ++tally.round_overruns;
        tally.rounds_max = rounds > tally.rounds_max ? rounds : tally.rounds_max;
        tally.n_max = n > tally.n_max ? n : tally.n_max;
        tally.rounds_last = rounds, tally.n_last = n;
        tally.decodes += decodes, tally.changes += changes, tally.lanes += n;
        int32_t run[4] = {0, 0, 0, 0};
        bool bad = false;
        for (int32_t i = 0; i < n; ++i) {
            const hawq_jpeg_sync_sub s = sub[i];
            if (bad) sub[i].start_pos = -1;
            sub[i].blocks = run[0];
            for (int c = 0; c < 3; ++c) sub[i].dc[c] = run[1 + c];
            if (s.end_pos < 0) bad = true;
            run[0] += s.blocks;
            for (int c = 0; c < 3; ++c) run[1 + c] = (int32_t)((uint32_t)run[1 + c] + (uint32_t)s.dc[c]);
        }
        const JpegSyncWriter wr{coef, mcu0, n_mcu * jpeg_sync_bpm(d)};
        int32_t st = 0;
        for (int32_t i = 0; i < n; ++i) {
            const int32_t e = jpeg_sync_lane(src, d, tb, last, jpeg_sync_limit(first, i, n, S), S, sub[i], &wr);
            if (e && !st) st = e;
        }
        if (st && !status) status = st;
        free(sub);
    }
    return status;
}

// both decoders on `stream` (exactly its bytes) -> 0: same status and, where it is zero or `always`, the same slab
bool same(const Image &im, const uint8_t *stream, const std::vector<int32_t> &iv, int32_t S, bool always, Tally &tally, int32_t *status_out) {
    const size_t words = (size_t)image_blocks(im.d) * 64;
    int16_t *a = (int16_t *)calloc(words, sizeof(int16_t)), *b = (int16_t *)calloc(words, sizeof(int16_t));
    const int32_t sa = serial(im, stream, iv, a), sb = synced(im, stream, iv, S, b, tally);
    const bool ok = sa == sb && ((sa != 0 && !always) || memcmp(a, b, words * sizeof(int16_t)) == 0);
    if (!ok) {
        size_t at = 0;
        while (at < words && a[at] == b[at]) ++at;
        fprintf(stderr, "%d x %d, %d component(s), %d x %d, sub_bytes %d: status %d serial, %d synchronised; first differing block %zu of %zu\n", im.d.width, im.d.height,
                im.d.ncomp, im.d.hs, im.d.vs, S, sa, sb, at / 64, words / 64);
    }
    free(a);
    free(b);
    *status_out = sa;
    return ok;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: jpeg_sync_host_check BLOB [SEED [FIRST STEP]]\n");
        return 2;
    }
    const std::vector<uint8_t> blob = read_file(argv[1]);
    const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    const int32_t first_image = argc > 4 ? atoi(argv[3]) : 0, step = argc > 4 && atoi(argv[4]) > 0 ? atoi(argv[4]) : 1;
    if (blob.size() < sizeof(hawq_jpeg_batch_hdr)) {
        fprintf(stderr, "jpeg_sync_host_check: no blob\n");
        return 2;
    }
    hawq_jpeg_batch_hdr hd;
    memcpy(&hd, blob.data(), sizeof hd);
    long runs = 0, equal = 0, truncations = 0, truncations_equal = 0, truncations_flagged = 0, overwrites = 0, overwrites_equal = 0, overwrites_flagged = 0;
    Tally intact, hostile;
    const int32_t all_sizes[4] = {16, 32, 64, 128}, two_sizes[2] = {16, 128};
    long images = 0;
    for (int32_t i = first_image; i < hd.n_images; i += step, ++images) {
        Image im;
        memcpy(&im.d, blob.data() + hd.desc_off + (size_t)i * sizeof(hawq_jpeg_desc), sizeof(hawq_jpeg_desc));
        const hawq_jpeg_desc &d = im.d;
        for (int c = 0; c < 3; ++c) {
            const int cc = c < d.ncomp ? c : 0;
            memcpy(&im.huff[2 * c], blob.data() + d.dc_off[cc], sizeof(hawq_jpeg_huff));
            memcpy(&im.huff[2 * c + 1], blob.data() + d.ac_off[cc], sizeof(hawq_jpeg_huff));
            for (int p = 0; p < JPEG_SYNC_LUT_SIZE; ++p)
                im.lut[2 * c][p] = jpeg_sync_lut_entry(&im.huff[2 * c], p), im.lut[2 * c + 1][p] = jpeg_sync_lut_entry(&im.huff[2 * c + 1], p);
        }
        im.iv.resize((size_t)d.n_intervals * 2);
        memcpy(im.iv.data(), blob.data() + d.interval_off, im.iv.size() * sizeof(int32_t));
        uint8_t *stream = (uint8_t *)malloc(d.stream_len ? d.stream_len : 1);
        memcpy(stream, blob.data() + d.stream_off, d.stream_len);
        int32_t st;
        for (int32_t S : all_sizes) {
            ++runs;
            equal += same(im, stream, im.iv, S, true, intact, &st) && st == 0;
            printf("image %d sub_bytes %d n %ld rounds %ld\n", i, S, intact.n_last, intact.rounds_last);   // of its last interval
        }
        for (int32_t S : two_sizes) {
            for (int32_t cut = 0; cut < d.stream_len; cut += 8) {
                std::vector<int32_t> iv = im.iv;
                for (int32_t &v : iv) v = v < cut ? v : cut;
                uint8_t *part = (uint8_t *)malloc(cut ? cut : 1);
                memcpy(part, stream, cut);
                ++truncations;
                truncations_equal += same(im, part, iv, S, false, hostile, &st);
                truncations_flagged += st != 0;
                free(part);
            }
            uint64_t rng = seed * 0x9E3779B97F4A7C15ull + (uint64_t)i;
            for (int n = 0; n < 200 && d.stream_len > 0; ++n) {
                rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                const int32_t at = (int32_t)((rng >> 33) % (uint64_t)d.stream_len);
                const uint8_t keep = stream[at];
                stream[at] = (uint8_t)(rng >> 24);
                ++overwrites;
                overwrites_equal += same(im, stream, im.iv, S, false, hostile, &st);
                overwrites_flagged += st != 0;
                stream[at] = keep;
            }
        }
        free(stream);
    }
    printf("images %ld runs %ld equal %ld truncations %ld truncations_equal %ld truncations_flagged %ld overwrites %ld overwrites_equal %ld overwrites_flagged %ld\n",
           images, runs, equal, truncations, truncations_equal, truncations_flagged, overwrites, overwrites_equal, overwrites_flagged);
    printf("lanes %ld decodes %ld changes %ld rounds_max %ld n_max %ld overruns %ld hostile_lanes %ld hostile_decodes %ld hostile_changes %ld hostile_overruns %ld\n",
           intact.lanes, intact.decodes, intact.changes, intact.rounds_max, intact.n_max, intact.round_overruns, hostile.lanes, hostile.decodes, hostile.changes,
           hostile.round_overruns);
    const bool ok = equal == runs && truncations_equal == truncations && overwrites_equal == overwrites && intact.round_overruns == 0 && hostile.round_overruns == 0 &&
                    intact.decodes == intact.lanes + intact.changes && hostile.decodes == hostile.lanes + hostile.changes;
    return ok ? 0 : 1;
}
