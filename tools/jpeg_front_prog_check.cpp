// Host run of the device JPEG front end's walker for both kinds of file (hawq_amd/csrc/jpeg_front_prog.h over jpeg_front.h - the text
// the scan kernel compiles), meant to be built with -fsanitize=address,undefined and run on its own:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_front_prog_check.cpp -o jpeg_front_prog_check
//   jpeg_front_prog_check CORPUS EXPECTED
//
// CORPUS: int64 count, then per file int64 length and its bytes.  EXPECTED: per file one hawq_jpeg_front_info and
// HAWQ_JPEG_PROG_MAX_SCANS hawq_jpeg_front_scan_rec, what hawq_jpeg_front_scan_prog_host of the library gave.  Every file is copied into
// a heap block of its exact length before the walker sees it, so a read outside the file stops the program; the records must equal the
// expected ones bit for bit.  For every scan of an accepted progressive file the canonical codes of the tables it names are computed
// and its values, its quantisation tables and its segment are read as the fill reads them, and the interval table is built from the
// segment's markers with every rank compared with n_intervals before its store, into a heap block of 8 * n_intervals bytes.
// Exit 0: all of that held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../hawq_amd/csrc/jpeg_front_prog.h"

namespace {
std::vector<uint8_t> read_file(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "jpeg_front_prog_check: cannot open %s\n", path);
        exit(2);
    }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + got);
    fclose(f);
    return v;
}

// the fill's interval table of the segment file[first .. end), serially: false when it is not the one the walker counted
bool intervals(const uint8_t *file, int32_t first, int32_t end, int32_t n_intervals) {
    int32_t *iv = (int32_t *)malloc(8 * (size_t)n_intervals);   // its exact size
    iv[0] = 0, iv[2 * (n_intervals - 1) + 1] = end - first;
    int32_t rank = 0;
    for (int32_t i = first; i < end; ++i) {
        if (!hawq_jpeg_front::is_marker(file[i], file[i + 1])) continue;
        if (rank + 1 < n_intervals) iv[2 * rank + 1] = i - first, iv[2 * rank + 2] = i + 2 - first;
        ++rank;
    }
    bool ok = rank == n_intervals - 1;
    for (int32_t k = 0; k < n_intervals; ++k) ok = ok && iv[2 * k] <= iv[2 * k + 1];
    free(iv);
    return ok;
}
}  // namespace

int main(int argc, char **argv) {
    using namespace hawq_jpeg_front;
    if (argc != 3) {
        fprintf(stderr, "usage: jpeg_front_prog_check CORPUS EXPECTED\n");
        return 2;
    }
    const std::vector<uint8_t> corpus = read_file(argv[1]), expected = read_file(argv[2]);
    const size_t per_file = sizeof(hawq_jpeg_front_info) + HAWQ_JPEG_PROG_MAX_SCANS * sizeof(hawq_jpeg_front_scan_rec);
    int64_t count = 0, at = 8, baseline = 0, progressive = 0, n_scans = 0, tables = 0;
    if (corpus.size() < 8) return 2;
    memcpy(&count, corpus.data(), 8);
    if (count < 0 || expected.size() != (size_t)count * per_file) {
        fprintf(stderr, "jpeg_front_prog_check: %lld files, %zu bytes of records\n", (long long)count, expected.size());
        return 2;
    }
    prog_walk w;
    std::vector<hawq_jpeg_front_scan_rec> scans(HAWQ_JPEG_PROG_MAX_SCANS);
    for (int64_t i = 0; i < count; ++i) {
        int64_t n = 0;
        if (at + 8 > (int64_t)corpus.size()) return 2;
        memcpy(&n, corpus.data() + at, 8);
        at += 8;
        if (n < 0 || n > (int64_t)corpus.size() - at) return 2;
        uint8_t *file = (uint8_t *)malloc(n ? (size_t)n : 1);   // its exact length: the sanitizer sees the first byte outside
        if (n) memcpy(file, corpus.data() + at, (size_t)n);
        at += n;
        hawq_jpeg_front_info o;
        memset(scans.data(), 0, scans.size() * sizeof scans[0]);
        walk_file_prog(n ? file : file + 1, n, o, scans.data(), w);
        const uint8_t *want = expected.data() + i * per_file;
        if (memcmp(&o, want, sizeof o) != 0 || memcmp(scans.data(), want + sizeof o, scans.size() * sizeof scans[0]) != 0) {
            fprintf(stderr, "jpeg_front_prog_check: file %lld: the records differ from the library's (defer %d)\n", (long long)i, o.defer);
            return 1;
        }
        if (o.defer == HAWQ_JPEG_FRONT_OK && o.reserved[0] == HAWQ_JPEG_FRONT_KIND_BASELINE) ++baseline;
        if (o.defer == HAWQ_JPEG_FRONT_OK && o.reserved[0] == HAWQ_JPEG_FRONT_KIND_PROG) {
            ++progressive;
            uint32_t sum = 0;
            for (int c = 0; c < o.ncomp; ++c)
                for (int k = 0; k < 64; ++k) sum += file[o.qt_at[o.tq[c]] + k];
            for (int32_t k = 0; k < o.reserved[1]; ++k) {
                const hawq_jpeg_front_scan_rec &s = scans[k];
                for (int slot = 0; slot < 4; ++slot) {
                    const int32_t src = slot < 3 ? s.dc_at[slot] : s.ac_at;
                    if (!src) continue;
                    int32_t mincode[17], maxcode[17], valptr[17];
                    canonical_codes(file + src, mincode, maxcode, valptr);
                    const int32_t values = huffman_values(file, src);
                    for (int32_t v = 0; v < values; ++v) sum += file[src + 16 + v];   // the values the fill copies
                    if (values < 1) return 1;
                    for (int l = 1; l <= 16; ++l)
                        if (maxcode[l] >= (1 << l)) {
                            fprintf(stderr, "jpeg_front_prog_check: file %lld: a code longer than its length\n", (long long)i);
                            return 1;
                        }
                    ++tables;
                }
                for (int32_t p = s.scan_first; p < s.scan_end + 2; ++p) sum += file[p];
                if (!intervals(file, s.scan_first, s.scan_end, s.n_intervals)) {
                    fprintf(stderr, "jpeg_front_prog_check: file %lld scan %d: the intervals are not the ones the walker counted\n", (long long)i, k);
                    return 1;
                }
                ++n_scans;
            }
            if (sum == 0xFFFFFFFFu) return 1;
        }
        free(file);
    }
    printf("files %lld baseline %lld progressive %lld scans %lld tables %lld\n", (long long)count, (long long)baseline, (long long)progressive, (long long)n_scans,
           (long long)tables);
    return 0;
}
