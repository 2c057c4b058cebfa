// The front end of the baseline JPEG decoder on the device (jpeg_front.h): hawq_jpeg_front_scan walks the headers of
// the raw files of a batch and checks their restart markers, one wave per file; hawq_jpeg_front_fill writes the tables, the restart
// intervals and the stream of every accepted file into the blob of hawq_jpeg_decode_batch, one workgroup per file.
// hawq_jpeg_front_scan_prog and hawq_jpeg_front_fill_prog do the same with progressive files as well (jpeg_front_prog.h):
// one wave per file, and one workgroup per scan into the blob of hawq_jpeg_decode_batch_prog.
//
// Bounds.  A file is read at b[i] with 0 <= i < its length, which the host has placed inside the files buffer.  The fill stores only
// into the ranges hawq_jpeg_front_fill_ok has placed inside the blob: 128 bytes per quantisation table, one hawq_jpeg_huff per Huffman
// table, 8 * n_intervals bytes of intervals (a marker's rank is compared with n_intervals before its store) and the stream's length
// rounded up to four bytes, inside its 16-byte aligned slot.
#include <string.h>

#include "common.h"
#include "jpeg_front_prog.h"

namespace {
using namespace hawq_jpeg_front;
constexpr int WAVE = 64;
constexpr int CHUNK = 16;             // bytes of a lane per pass
constexpr int PASS = WAVE * CHUNK;    // bytes of the wave per pass
constexpr int FILL_THREADS = 256;
constexpr int32_t NONE = 0x7FFFFFFF;

// Bytes a .. a + 16 of the file (a: a multiple of 16; zero behind its end) into c, and the markers among a .. a + 15: bit j is set when
// lo <= a + j < hi and the pair at a + j is a marker.  The caller keeps hi <= n - 1, so the pair lies inside the file.
__device__ __forceinline__ uint32_t chunk_markers(const uint8_t *b, int64_t n, int64_t a, int64_t lo, int64_t hi, uint8_t (&c)[CHUNK + 1]) {
    if (a + CHUNK <= n) {   // the file starts at a 16-byte aligned address
        const uint4 w = *(const uint4 *)(b + a);
        const uint32_t words[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < CHUNK; ++j) c[j] = (uint8_t)(words[j >> 2] >> (8 * (j & 3)));
    } else {
#pragma unroll
        for (int j = 0; j < CHUNK; ++j) c[j] = a + j < n ? b[a + j] : (uint8_t)0;
    }
    c[CHUNK] = a + CHUNK < n ? b[a + CHUNK] : (uint8_t)0;
    uint32_t mask = 0;
#pragma unroll
    for (int j = 0; j < CHUNK; ++j)
        if (a + j >= lo && a + j < hi && is_marker(c[j], c[j + 1])) mask |= 1u << j;
    return mask;
}

// markers of the lanes below this one, and of the whole wave
__device__ __forceinline__ int32_t wave_prefix(int32_t count, int lane, int32_t &total) {
    int32_t incl = count;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const int32_t up = __shfl_up(incl, d, WAVE);
        if (lane >= d) incl += up;
    }
    total = __shfl(incl, WAVE - 1, WAVE);
    return incl - count;
}

__device__ __forceinline__ int32_t wave_min(int32_t v) {
#pragma unroll
    for (int d = WAVE / 2; d; d >>= 1) v = min(v, __shfl_xor(v, d, WAVE));
    return v;
}

// The entropy-coded segment from `lo` on with all lanes of a wave, 1 KiB per pass, sixteen bytes per lane: a marker's rank is the running
// base + the markers of the lower lanes + those before it in its own lane.  True when the RSTn markers count modulo 8 from RST0 up to the
// first other marker, there are `expected` of them, and that marker is EOI or `any_end` holds; `stop`: where it stands.
__device__ __forceinline__ bool segment_end(const uint8_t *b, int64_t n, int64_t lo, int32_t expected, bool any_end, int lane, int32_t &stop) {
    const int64_t hi = n - 1;
    int32_t base = 0;
    for (int64_t p = lo & ~(int64_t)(PASS - 1); p < hi; p += PASS) {   // passes at multiples of 1 KiB of the file: lanes before lo find nothing
        const int64_t a = p + lane * CHUNK;
        uint8_t c[CHUNK + 1];
        const uint32_t mask = chunk_markers(b, n, a, lo, hi, c);
        int32_t total;
        int32_t rank = base + wave_prefix(__popc(mask), lane, total);
        int32_t other = NONE, other_code = 0, other_rank = 0, wrong = NONE;   // first marker that is no RSTn; first RSTn out of order
#pragma unroll
        for (int j = 0; j < CHUNK; ++j) {
            if (!(mask >> j & 1)) continue;
            const int code = c[j + 1];
            if ((code & 0xF8) == 0xD0) {
                if ((code & 7) != (rank & 7) && wrong == NONE) wrong = (int32_t)(a + j);
            } else if (other == NONE) {
                other = (int32_t)(a + j), other_code = code, other_rank = rank;
            }
            ++rank;
        }
        stop = wave_min(other);
        if (__any(wrong < stop)) return false;   // an RSTn out of order before the segment's end
        if (stop != NONE) {
            const int owner = __ffsll((unsigned long long)__ballot(other == stop)) - 1;
            other_code = __shfl(other_code, owner, WAVE), other_rank = __shfl(other_rank, owner, WAVE);
            return (any_end || other_code == 0xD9) && other_rank == expected;
        }
        base += total;
    }
    return false;   // truncated
}

// A file as a baseline one into the record `o` in LDS: the header walk is the same in all lanes, the segment's check is the wave's.
// The record while it is filled lies in LDS because the walker indexes its table offsets with ids it reads from the file.  Every lane
// writes the same value to the same word, and a wave's LDS accesses complete in order
__device__ __forceinline__ void baseline_file(const uint8_t *b, int64_t n, hawq_jpeg_front_info &o, int lane) {
    clear(o, 0);
    int32_t defer = walk_header(b, n, o);
    if (!defer) {
        const int32_t expected = expected_restarts(o);
        int32_t stop;
        if (segment_end(b, n, o.scan_first, expected, false, lane, stop)) o.scan_end = stop, o.n_intervals = expected + 1;
        else defer = HAWQ_JPEG_FRONT_REFUSED;
    }
    if (defer) clear(o, defer);
}

// One wave per file.
__global__ __launch_bounds__(WAVE) void jpeg_front_scan_kernel(const uint8_t *files, const hawq_jpeg_front_file *table, hawq_jpeg_front_info *info) {
    __shared__ hawq_jpeg_front_info o;
    baseline_file(files + table[blockIdx.x].offset, table[blockIdx.x].length, o, threadIdx.x);
    if (threadIdx.x == 0) info[blockIdx.x] = o;
}

// One wave per file: as a baseline file first, and what that walk refuses as a progressive one (walk_file_prog of jpeg_front_prog.h,
// with the wave's check of every scan's segment).  The walk, the record and the scan's record lie in LDS as above.
__global__ __launch_bounds__(WAVE) void jpeg_front_scan_prog_kernel(const uint8_t *files, const hawq_jpeg_front_file *table, hawq_jpeg_front_info *info,
                                                                    hawq_jpeg_front_scan_rec *scans) {
    const int lane = threadIdx.x;
    const uint8_t *b = files + table[blockIdx.x].offset;
    const int64_t n = table[blockIdx.x].length;
    hawq_jpeg_front_scan_rec *mine = scans + (int64_t)blockIdx.x * HAWQ_JPEG_PROG_MAX_SCANS;
    __shared__ hawq_jpeg_front_info o;
    __shared__ prog_walk w;
    __shared__ hawq_jpeg_front_scan_rec s;
    baseline_file(b, n, o, lane);
    if (o.defer == HAWQ_JPEG_FRONT_REFUSED) {
        clear(o, 0);
        prog_begin(w);
        int32_t code;
        for (;;) {
            s = hawq_jpeg_front_scan_rec{};
            int32_t units = 0, stop;
            code = prog_next(b, n, w, o, s, units);
            if (code != PROG_SCAN) break;
            const int32_t expected = prog_expected_restarts(units, s.restart);
            if (!segment_end(b, n, s.scan_first, expected, true, lane, stop)) {
                code = HAWQ_JPEG_FRONT_REFUSED;
                break;
            }
            s.scan_end = stop, s.n_intervals = expected + 1;
            if (lane == 0) mine[w.n_scans] = s;   // n_scans < HAWQ_JPEG_PROG_MAX_SCANS: prog_next has refused the scan otherwise
            ++w.n_scans;
            w.pos = stop;
        }
        if (lane == 0) prog_finish(o, mine, w.n_scans, code);   // lane 0 has written the scans' records and takes them back
        else if (code != PROG_END) clear(o, code);
    }
    if (lane == 0) info[blockIdx.x] = o;
}

// The canonical hawq_jpeg_huff of the table whose BITS stand at b[src], by the first 256 threads of a workgroup
__device__ __forceinline__ void fill_huff(const uint8_t *b, int64_t n, int64_t src, hawq_jpeg_huff *h, int t) {
    // thread l <= 16 owns code length l: the canonical assignment up to it (T.81 C.2)
    int32_t code = 0, k = 0, mincode = 0, maxcode = -1, valptr = 0;
    for (int length = 1; length <= 16; ++length) {
        const int32_t count = b[src + length - 1];
        if (length == t && count) valptr = k, mincode = code, maxcode = code + count - 1;
        code = (code + count) << 1, k += count;
    }
    if (t <= 16) h->mincode[t] = mincode, h->maxcode[t] = maxcode, h->valptr[t] = valptr;
    if (t < k && src + 16 + t < n) h->huffval[t] = b[src + 16 + t];   // k <= 256 in a table the scan has accepted
}

// The entropy-coded segment b[first .. end) in whole dwords to `stream_off` by the whole workgroup, and its interval table to
// `interval_off` by the first wave: the scan's second marker pass
__device__ __forceinline__ void fill_segment(const uint8_t *b, int64_t n, int64_t first, int64_t end, int32_t n_intervals, uint8_t *blob, int32_t interval_off,
                                             int32_t stream_off, int t) {
    uint32_t *dst = (uint32_t *)(blob + stream_off);
    for (int64_t w = t; 4 * w < end - first; w += FILL_THREADS) {
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * w + k < end - first) word |= (uint32_t)b[first + 4 * w + k] << (8 * k);
        dst[w] = word;
    }
    if (t >= WAVE) return;
    int32_t *iv = (int32_t *)(blob + interval_off);
    if (t == 0) iv[0] = 0, iv[2 * (n_intervals - 1) + 1] = (int32_t)(end - first);
    int32_t base = 0;
    for (int64_t p = first & ~(int64_t)(PASS - 1); p < end && n_intervals > 1; p += PASS) {
        const int64_t a = p + t * CHUNK;
        uint8_t c[CHUNK + 1];
        const uint32_t mask = chunk_markers(b, n, a, first, end, c);
        int32_t total;
        int32_t rank = base + wave_prefix(__popc(mask), t, total);
#pragma unroll
        for (int j = 0; j < CHUNK; ++j) {
            if (!(mask >> j & 1)) continue;
            if (rank + 1 < n_intervals) iv[2 * rank + 1] = (int32_t)(a + j - first), iv[2 * rank + 2] = (int32_t)(a + j + 2 - first);
            ++rank;
        }
        base += total;
    }
}

// One workgroup per accepted file.
__global__ __launch_bounds__(FILL_THREADS) void jpeg_front_fill_kernel(const uint8_t *files, const hawq_jpeg_front_file *table, const hawq_jpeg_front_info *info,
                                                                       const hawq_jpeg_front_place *place, uint8_t *blob) {
    const int t = threadIdx.x;
    const hawq_jpeg_front_place &pl = place[blockIdx.x];
    const hawq_jpeg_front_info &o = info[pl.file];
    const uint8_t *b = files + table[pl.file].offset;
    const int64_t n = table[pl.file].length;
    for (int c = 0; c < o.ncomp; ++c) {
        if (pl.qt_off[c] && t < 64) ((uint16_t *)(blob + pl.qt_off[c]))[t] = b[o.qt_at[o.tq[c]] + t];
        for (int cls = 0; cls < 2; ++cls) {
            const int32_t off = cls ? pl.ac_off[c] : pl.dc_off[c];
            if (off) fill_huff(b, n, o.huff_at[cls * 2 + (cls ? o.ta[c] : o.td[c])], (hawq_jpeg_huff *)(blob + off), t);
        }
    }
    fill_segment(b, n, o.scan_first, o.scan_end, o.n_intervals, blob, pl.interval_off, pl.stream_off, t);
}

// One workgroup per scan of an accepted progressive file: a batch has ten times as many scans as files, each with a marker pass of its
// own that one wave makes, so a workgroup per file would make ten of them one after the other.
__global__ __launch_bounds__(FILL_THREADS) void jpeg_front_fill_prog_kernel(const uint8_t *files, const hawq_jpeg_front_file *table, const hawq_jpeg_front_info *info,
                                                                            const hawq_jpeg_front_scan_rec *scans, const hawq_jpeg_front_scan_place *place,
                                                                            uint8_t *blob) {
    const int t = threadIdx.x;
    const hawq_jpeg_front_scan_place &pl = place[blockIdx.x];
    const hawq_jpeg_front_info &o = info[pl.file];
    const hawq_jpeg_front_scan_rec &s = scans[(int64_t)pl.file * HAWQ_JPEG_PROG_MAX_SCANS + pl.scan];
    const uint8_t *b = files + table[pl.file].offset;
    const int64_t n = table[pl.file].length;
    for (int c = 0; c < 3; ++c) {
        if (pl.qt_off[c] && t < 64) ((uint16_t *)(blob + pl.qt_off[c]))[t] = b[o.qt_at[o.tq[c]] + t];
        if (pl.dc_off[c]) fill_huff(b, n, s.dc_at[c], (hawq_jpeg_huff *)(blob + pl.dc_off[c]), t);
    }
    if (pl.ac_off) fill_huff(b, n, s.ac_at, (hawq_jpeg_huff *)(blob + pl.ac_off), t);
    fill_segment(b, n, s.scan_first, s.scan_end, s.n_intervals, blob, pl.interval_off, pl.stream_off, t);
}

const char *table_refusal(const hawq_jpeg_front_file *host_table, int32_t n_files, int64_t files_bytes) {
    if (!host_table || n_files < 1) return "no file table";
    int64_t at = 0;
    for (int32_t i = 0; i < n_files; ++i) {
        const hawq_jpeg_front_file &f = host_table[i];
        if (f.offset < at || f.offset % 16 || f.length < 0 || f.offset > files_bytes || f.length > files_bytes - f.offset)
            return "a file is not 16-byte aligned, outside the buffer, or not behind the one before it";
        at = f.offset + f.length;
    }
    return nullptr;
}

const char *fill_refusal(const hawq_jpeg_front_info *host_info, const hawq_jpeg_front_place *host_place, int32_t n, const hawq_jpeg_front_file *host_table,
                         int32_t n_files, int64_t files_bytes, int64_t blob_bytes) {
    if (!host_info || !host_place || n < 1) return "no info records or no placement table";
    if (blob_bytes < 16 || blob_bytes >= ((int64_t)1 << 31)) return "blob size outside 16 .. 2 GiB";
    if (const char *why = table_refusal(host_table, n_files, files_bytes)) return why;
    int64_t cursor = 16;   // behind the batch header at least
    int32_t last_file = -1;
    for (int32_t e = 0; e < n; ++e) {
        const hawq_jpeg_front_place &pl = host_place[e];
        if (pl.file <= last_file || pl.file >= n_files) return "a placement names no file, or not one behind the entry before it";
        last_file = pl.file;
        const hawq_jpeg_front_info &o = host_info[pl.file];
        const int64_t len = host_table[pl.file].length;
        if (o.defer != HAWQ_JPEG_FRONT_OK) return "a placement names a file the scan did not accept";
        if (o.ncomp != 1 && o.ncomp != 3) return "component count";
        if (o.scan_first < 0 || o.scan_end < o.scan_first || o.scan_end > len - 2) return "the scan lies outside its file";
        if (o.n_intervals < 1 || o.n_intervals - 1 > (o.scan_end - o.scan_first) / 2) return "more restart intervals than the scan has room for";
        auto put = [&](int32_t off, int64_t size) {
            if (off < cursor || off % 16 || size > blob_bytes - off) return false;
            cursor = off + size;
            return true;
        };
        for (int c = 0; c < o.ncomp; ++c) {
            if (o.tq[c] < 0 || o.tq[c] > 3 || o.td[c] < 0 || o.td[c] > 1 || o.ta[c] < 0 || o.ta[c] > 1) return "table id out of range";
            const int32_t src[3] = {o.qt_at[o.tq[c]], o.huff_at[o.td[c]], o.huff_at[2 + o.ta[c]]};
            const int64_t need[3] = {64, 16, 16}, size[3] = {128, (int64_t)sizeof(hawq_jpeg_huff), (int64_t)sizeof(hawq_jpeg_huff)};
            const int32_t off[3] = {pl.qt_off[c], pl.dc_off[c], pl.ac_off[c]};
            const int32_t *ids[3] = {o.tq, o.td, o.ta};
            for (int k = 0; k < 3; ++k) {
                if (src[k] < 1 || src[k] > len - need[k]) return "a table lies outside its file";
                bool placed = false;
                for (int earlier = 0; earlier < c; ++earlier) placed = placed || ids[k][earlier] == ids[k][c];
                if (placed != (off[k] == 0)) return "a table is placed twice or not at all";
                if (off[k] && !put(off[k], size[k])) return "a table's place is outside the blob, unaligned, or not behind the part before it";
            }
        }
        if (!put(pl.interval_off, 8 * (int64_t)o.n_intervals)) return "the intervals' place is outside the blob, unaligned, or not behind the part before it";
        if (!put(pl.stream_off, ((int64_t)(o.scan_end - o.scan_first) + 3) & ~(int64_t)3))
            return "the stream's place is outside the blob, unaligned, or not behind the part before it";
    }
    return nullptr;
}
const char *fill_prog_refusal(const hawq_jpeg_front_info *host_info, const hawq_jpeg_front_scan_rec *host_scans, const hawq_jpeg_front_scan_place *host_place,
                              int32_t n, const hawq_jpeg_front_file *host_table, int32_t n_files, int64_t files_bytes, int64_t blob_bytes) {
    if (!host_info || !host_scans || !host_place || n < 1) return "no info records, no scan records or no placement table";
    if (blob_bytes < 32 || blob_bytes >= ((int64_t)1 << 31)) return "blob size outside 32 .. 2 GiB";
    if (const char *why = table_refusal(host_table, n_files, files_bytes)) return why;
    int64_t cursor = 32;   // behind the batch header and the progressive header at least
    int32_t last_file = -1, last_scan = -1;
    for (int32_t e = 0; e < n; ++e) {
        const hawq_jpeg_front_scan_place &pl = host_place[e];
        if (pl.file < 0 || pl.file >= n_files || pl.file < last_file) return "a placement names no file, or one before the entry before it";
        if (pl.file != last_file) last_scan = -1;
        last_file = pl.file;
        const hawq_jpeg_front_info &o = host_info[pl.file];
        const int64_t len = host_table[pl.file].length;
        if (o.defer != HAWQ_JPEG_FRONT_OK || o.reserved[0] != HAWQ_JPEG_FRONT_KIND_PROG) return "a placement names a file the scan did not accept as progressive";
        if (o.reserved[1] < 1 || o.reserved[1] > HAWQ_JPEG_PROG_MAX_SCANS) return "scan count";
        if (pl.scan <= last_scan || pl.scan >= o.reserved[1]) return "a placement names no scan of its file, or not one behind the entry before it";
        last_scan = pl.scan;
        const hawq_jpeg_front_scan_rec &s = host_scans[(int64_t)pl.file * HAWQ_JPEG_PROG_MAX_SCANS + pl.scan];
        if (o.ncomp != 1 && o.ncomp != 3) return "component count";
        if (s.scan_first < 0 || s.scan_end < s.scan_first || s.scan_end > len - 2) return "the scan lies outside its file";
        if (s.n_intervals < 1 || s.n_intervals - 1 > (s.scan_end - s.scan_first) / 2) return "more restart intervals than the scan has room for";
        auto put = [&](int32_t off, int64_t size) {
            if (off < cursor || off % 16 || size > blob_bytes - off) return false;
            cursor = off + size;
            return true;
        };
        for (int c = 0; c < 3; ++c) {
            if (!pl.qt_off[c]) continue;
            if (c >= o.ncomp || o.tq[c] < 0 || o.tq[c] > 3) return "a quantisation table of no component, or table id out of range";
            if (o.qt_at[o.tq[c]] < 1 || o.qt_at[o.tq[c]] > len - 64) return "a table lies outside its file";
            if (!put(pl.qt_off[c], 128)) return "a table's place is outside the blob, unaligned, or not behind the part before it";
        }
        for (int k = 0; k < 4; ++k) {
            const int32_t off = k < 3 ? pl.dc_off[k] : pl.ac_off, src = k < 3 ? s.dc_at[k] : s.ac_at;
            if (!off) continue;
            if (src < 1 || src > len - 16) return "a table lies outside its file";
            if (!put(off, (int64_t)sizeof(hawq_jpeg_huff))) return "a table's place is outside the blob, unaligned, or not behind the part before it";
        }
        if (!put(pl.interval_off, 8 * (int64_t)s.n_intervals)) return "the intervals' place is outside the blob, unaligned, or not behind the part before it";
        if (!put(pl.stream_off, ((int64_t)(s.scan_end - s.scan_first) + 3) & ~(int64_t)3))
            return "the stream's place is outside the blob, unaligned, or not behind the part before it";
    }
    return nullptr;
}
}  // namespace

extern "C" int hawq_jpeg_front_scan_host(const void *host_files, int64_t files_bytes, const hawq_jpeg_front_file *host_table, int32_t n_files,
                                         hawq_jpeg_front_info *host_info) {
    HAWQ_REQUIRE(host_files && host_info, "hawq_jpeg_front_scan_host: null pointer");
    const char *why = table_refusal(host_table, n_files, files_bytes);
    HAWQ_REQUIRE(!why, "hawq_jpeg_front_scan: %s", why);
    for (int32_t i = 0; i < n_files; ++i) walk_file((const uint8_t *)host_files + host_table[i].offset, host_table[i].length, host_info[i]);
    return 0;
}

extern "C" int hawq_jpeg_front_scan(const void *files, int64_t files_bytes, const hawq_jpeg_front_file *table, const hawq_jpeg_front_file *host_table,
                                    int32_t n_files, hawq_jpeg_front_info *info, void *stream) {
    HAWQ_REQUIRE(files && table && info, "hawq_jpeg_front_scan: null pointer");
    HAWQ_REQUIRE(((uintptr_t)files & 15) == 0, "hawq_jpeg_front_scan: files not 16-byte aligned");
    const char *why = table_refusal(host_table, n_files, files_bytes);
    HAWQ_REQUIRE(!why, "hawq_jpeg_front_scan: %s", why);
    hipLaunchKernelGGL(jpeg_front_scan_kernel, dim3((unsigned)n_files), dim3(WAVE), 0, (hipStream_t)stream, (const uint8_t *)files, table, info);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int hawq_jpeg_front_fill_ok(const hawq_jpeg_front_info *host_info, const hawq_jpeg_front_place *host_place, int32_t n,
                                       const hawq_jpeg_front_file *host_table, int32_t n_files, int64_t files_bytes, int64_t blob_bytes) {
    const char *why = fill_refusal(host_info, host_place, n, host_table, n_files, files_bytes, blob_bytes);
    if (why) hawq_set_error("hawq_jpeg_front_fill: %s", why);
    return why == nullptr;
}

extern "C" int hawq_jpeg_front_fill(const void *files, int64_t files_bytes, const hawq_jpeg_front_file *table, const hawq_jpeg_front_file *host_table, int32_t n_files,
                                    const hawq_jpeg_front_info *info, const hawq_jpeg_front_info *host_info, const hawq_jpeg_front_place *place,
                                    const hawq_jpeg_front_place *host_place, int32_t n, void *blob, int64_t blob_bytes, void *stream) {
    HAWQ_REQUIRE(files && table && info && place && blob, "hawq_jpeg_front_fill: null pointer");
    HAWQ_REQUIRE(((uintptr_t)files & 15) == 0 && ((uintptr_t)blob & 15) == 0, "hawq_jpeg_front_fill: files or blob not 16-byte aligned");
    const char *why = fill_refusal(host_info, host_place, n, host_table, n_files, files_bytes, blob_bytes);
    HAWQ_REQUIRE(!why, "hawq_jpeg_front_fill: %s", why);
    hipStream_t s = (hipStream_t)stream;
    HAWQ_CHECK_HIP(hipMemsetAsync(blob, 0, (size_t)blob_bytes, s));
    hipLaunchKernelGGL(jpeg_front_fill_kernel, dim3((unsigned)n), dim3(FILL_THREADS), 0, s, (const uint8_t *)files, table, info, place, (uint8_t *)blob);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int hawq_jpeg_front_scan_prog_host(const void *host_files, int64_t files_bytes, const hawq_jpeg_front_file *host_table, int32_t n_files,
                                              hawq_jpeg_front_info *host_info, hawq_jpeg_front_scan_rec *host_scans) {
    HAWQ_REQUIRE(host_files && host_info && host_scans, "hawq_jpeg_front_scan_prog_host: null pointer");
    const char *why = table_refusal(host_table, n_files, files_bytes);
    HAWQ_REQUIRE(!why, "hawq_jpeg_front_scan_prog: %s", why);
    memset(host_scans, 0, (size_t)n_files * HAWQ_JPEG_PROG_MAX_SCANS * sizeof(hawq_jpeg_front_scan_rec));
    prog_walk w;
    for (int32_t i = 0; i < n_files; ++i)
        walk_file_prog((const uint8_t *)host_files + host_table[i].offset, host_table[i].length, host_info[i], host_scans + (int64_t)i * HAWQ_JPEG_PROG_MAX_SCANS, w);
    return 0;
}

extern "C" int hawq_jpeg_front_scan_prog(const void *files, int64_t files_bytes, const hawq_jpeg_front_file *table, const hawq_jpeg_front_file *host_table,
                                         int32_t n_files, hawq_jpeg_front_info *info, hawq_jpeg_front_scan_rec *scans, void *stream) {
    HAWQ_REQUIRE(files && table && info && scans, "hawq_jpeg_front_scan_prog: null pointer");
    HAWQ_REQUIRE(((uintptr_t)files & 15) == 0, "hawq_jpeg_front_scan_prog: files not 16-byte aligned");
    const char *why = table_refusal(host_table, n_files, files_bytes);
    HAWQ_REQUIRE(!why, "hawq_jpeg_front_scan_prog: %s", why);
    hipStream_t s = (hipStream_t)stream;
    HAWQ_CHECK_HIP(hipMemsetAsync(scans, 0, (size_t)n_files * HAWQ_JPEG_PROG_MAX_SCANS * sizeof(hawq_jpeg_front_scan_rec), s));
    hipLaunchKernelGGL(jpeg_front_scan_prog_kernel, dim3((unsigned)n_files), dim3(WAVE), 0, s, (const uint8_t *)files, table, info, scans);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int hawq_jpeg_front_fill_prog_ok(const hawq_jpeg_front_info *host_info, const hawq_jpeg_front_scan_rec *host_scans,
                                            const hawq_jpeg_front_scan_place *host_place, int32_t n, const hawq_jpeg_front_file *host_table, int32_t n_files,
                                            int64_t files_bytes, int64_t blob_bytes) {
    const char *why = fill_prog_refusal(host_info, host_scans, host_place, n, host_table, n_files, files_bytes, blob_bytes);
    if (why) hawq_set_error("hawq_jpeg_front_fill_prog: %s", why);
    return why == nullptr;
}

extern "C" int hawq_jpeg_front_fill_prog(const void *files, int64_t files_bytes, const hawq_jpeg_front_file *table, const hawq_jpeg_front_file *host_table,
                                         int32_t n_files, const hawq_jpeg_front_info *info, const hawq_jpeg_front_info *host_info,
                                         const hawq_jpeg_front_scan_rec *scans, const hawq_jpeg_front_scan_rec *host_scans, const hawq_jpeg_front_scan_place *place,
                                         const hawq_jpeg_front_scan_place *host_place, int32_t n, void *blob, int64_t blob_bytes, void *stream) {
    HAWQ_REQUIRE(files && table && info && scans && place && blob, "hawq_jpeg_front_fill_prog: null pointer");
    HAWQ_REQUIRE(((uintptr_t)files & 15) == 0 && ((uintptr_t)blob & 15) == 0, "hawq_jpeg_front_fill_prog: files or blob not 16-byte aligned");
    const char *why = fill_prog_refusal(host_info, host_scans, host_place, n, host_table, n_files, files_bytes, blob_bytes);
    HAWQ_REQUIRE(!why, "hawq_jpeg_front_fill_prog: %s", why);
    hipStream_t s = (hipStream_t)stream;
    HAWQ_CHECK_HIP(hipMemsetAsync(blob, 0, (size_t)blob_bytes, s));
    hipLaunchKernelGGL(jpeg_front_fill_prog_kernel, dim3((unsigned)n), dim3(FILL_THREADS), 0, s, (const uint8_t *)files, table, info, scans, place, (uint8_t *)blob);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
