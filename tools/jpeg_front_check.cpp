// Host run of the device JPEG front end's marker walker (hawq_amd/csrc/jpeg_front.h - the text the scan kernel compiles), meant to be
// built with -fsanitize=address,undefined and run on its own:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_front_check.cpp -o jpeg_front_check
//   jpeg_front_check CORPUS EXPECTED
//
// CORPUS: int64 count, then per file int64 length and its bytes.  EXPECTED: one hawq_jpeg_front_info per file, what
// hawq_jpeg_front_scan_host of the library gave.  Every file is copied into a heap block of its exact length before the walker sees
// it, so a read outside the file stops the program; the record must equal the expected one bit for bit, and for an accepted file the
// canonical codes of every table it names are computed as the fill does.  Exit 0: all of that held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../hawq_amd/csrc/jpeg_front.h"

namespace {
std::vector<uint8_t> read_file(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "jpeg_front_check: cannot open %s\n", path);
        exit(2);
    }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + got);
    fclose(f);
    return v;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: jpeg_front_check CORPUS EXPECTED\n");
        return 2;
    }
    const std::vector<uint8_t> corpus = read_file(argv[1]), expected = read_file(argv[2]);
    int64_t count = 0, at = 8, accepted = 0, tables = 0;
    if (corpus.size() < 8) return 2;
    memcpy(&count, corpus.data(), 8);
    if (count < 0 || expected.size() != (size_t)count * sizeof(hawq_jpeg_front_info)) {
        fprintf(stderr, "jpeg_front_check: %lld files, %zu bytes of records\n", (long long)count, expected.size());
        return 2;
    }
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
        hawq_jpeg_front::walk_file(n ? file : file + 1, n, o);
        if (memcmp(&o, expected.data() + i * sizeof o, sizeof o) != 0) {
            fprintf(stderr, "jpeg_front_check: file %lld: the record differs from the library's (defer %d)\n", (long long)i, o.defer);
            return 1;
        }
        if (o.defer == HAWQ_JPEG_FRONT_OK) {
            ++accepted;
            for (int c = 0; c < o.ncomp; ++c)
                for (int cls = 0; cls < 2; ++cls) {
                    const int32_t src = o.huff_at[2 * cls + (cls ? o.ta[c] : o.td[c])];
                    int32_t mincode[17], maxcode[17], valptr[17];
                    hawq_jpeg_front::canonical_codes(file + src, mincode, maxcode, valptr);
                    const int32_t k = hawq_jpeg_front::huffman_values(file, src);
                    uint32_t sum = 0;
                    for (int32_t v = 0; v < k; ++v) sum += file[src + 16 + v];   // the values the fill copies
                    if (k < 1 || sum == 0xFFFFFFFFu) return 1;
                    for (int l = 1; l <= 16; ++l)
                        if (maxcode[l] >= (1 << l)) {
                            fprintf(stderr, "jpeg_front_check: file %lld: a code longer than its length\n", (long long)i);
                            return 1;
                        }
                    ++tables;
                }
            uint32_t sum = 0;
            for (int c = 0; c < o.ncomp; ++c)
                for (int k = 0; k < 64; ++k) sum += file[o.qt_at[o.tq[c]] + k];
            for (int32_t p = o.scan_first; p < o.scan_end + 2; ++p) sum += file[p];
            if (sum == 0xFFFFFFFFu) return 1;
        }
        free(file);
    }
    printf("files %lld accepted %lld tables %lld\n", (long long)count, (long long)accepted, (long long)tables);
    return 0;
}
