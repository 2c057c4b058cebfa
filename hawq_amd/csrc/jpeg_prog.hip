// hawq_jpeg_decode_batch_prog: a batch of progressive (SOF2, Huffman) JPEGs -> tight uint8 RGB, the bytes libjpeg-turbo gives for a
// complete progressive file - which are the bytes of the baseline file of the same coefficients.  Only stage 1 is new: the scans fill
// the coefficient slab of hawq_jpeg_decode_batch, and stages 2 and 3 are its kernels, launched unchanged (jpeg_stages.h).
//   1 entropy   one 64-lane workgroup (one wave) per (image, scan, restart interval), one launch per LEVEL of the batch: the scans of
//               a level write disjoint int16 words of the slab (hawq_mi355.h), so they run side by side, and a level starts when the
//               one before it is done (stream order).  As in jpeg_entropy_kernel every lane runs the same decoder (jpeg_prog.h) on the
//               same state, the stream comes through the 256-byte LDS window and the scan's Huffman tables are copied into LDS.
//               Refinement scans branch on coefficient values, so the block an AC scan works on is staged in LDS: 64 lanes load its
//               64 coefficients in one access, one ballot turns them into the mask of coefficients with history that the decoder
//               tests in registers, every lane updates the same LDS words, and when the block is left the lanes whose coefficient
//               lies in the scan's band ss .. se store it back, 16 bits each - never a word another scan of the level owns.  A first
//               AC pass reads nothing: its stage starts as zeros.  DC scans touch coefficient 0 alone and never branch on it: lane 0
//               stores it.
//   1 (resume)  hawq_jpeg_decode_batch_prog_resume: one wave per SEGMENT of a restart interval of a scan, started at a recorded resume
//               point (jpeg_resume.h): a bit position, the predictors and EOBRUN there.  A block belongs to one segment,
//               so the staged block needs no new ordering; a level's launch holds the segments of the level's waves.
// Everything the kernel indexes with comes from the blob, and hawq_jpeg_prog_ok (and hawq_jpeg_resume_ok for the segment table) has
// passed that blob on the host before any launch.
#include <string.h>

#include "common.h"
#include "jpeg_resume.h"
#include "jpeg_stages.h"

namespace {
using namespace hawq_jpeg;

// The coefficients of the image of one wave.  All lanes hold the same decoder state, so all of them write the same values into the
// staged block; each lane then stores the word it owns.
struct LdsBlock {
    int16_t *coef;    // global: the image's first block
    int16_t *stage;   // LDS [64]
    int lane;
    __device__ __forceinline__ int16_t *open(int64_t b) {
        __syncthreads();   // the stores of the block before this one have read the stage
        stage[lane] = coef[b * 64 + lane];
        __syncthreads();
        return stage;
    }
    // a first pass reads nothing and its band of the block is still zero (the slab was zeroed, the progression is legal): no load
    __device__ __forceinline__ int16_t *open_fresh(int64_t) {
        __syncthreads();
        stage[lane] = 0;
        __syncthreads();
        return stage;
    }
    // one ballot instead of a read per coefficient: lane k looks at the coefficient with zig-zag index k
    __device__ __forceinline__ uint64_t history(const int16_t *c) const { return __ballot(c[jpeg_natural(lane)] != 0); }
    __device__ __forceinline__ void close(int64_t b, int ss, int se) {
        __syncthreads();
        const int zz = jpeg_zigzag_of(lane);
        if (zz >= ss && zz <= se) coef[b * 64 + lane] = stage[lane];
    }
    __device__ __forceinline__ void dc_store(int64_t b, int16_t v) {
        if (lane == 0) coef[b * 64] = v;
    }
    __device__ __forceinline__ void dc_or(int64_t b, int16_t bit) {
        if (lane == 0) coef[b * 64] = (int16_t)(coef[b * 64] | bit);
    }
};

// RESUME (hawq_jpeg_decode_batch_prog_resume): workgroup x decodes segment wave0 + x of the table at segs_off - the units, the start
// position and the state its entry names (jpeg_resume.h), the units clamped to those of the entry's interval.
template <bool RESUME>
__global__ __launch_bounds__(WAVE) void jpeg_prog_kernel(const uint8_t *__restrict__ blob, int16_t *coef, int32_t *__restrict__ status, int32_t wave0, int64_t segs_off) {
    __shared__ hawq_jpeg_huff tables[3];   // DC per component of the scan, or the AC table in [0]
    __shared__ uint8_t window[WINDOW];
    __shared__ int16_t stage[64];
    const hawq_jpeg_batch_hdr hd = *(const hawq_jpeg_batch_hdr *)blob;
    const hawq_jpeg_prog_hdr ph = *(const hawq_jpeg_prog_hdr *)(blob + sizeof(hawq_jpeg_batch_hdr));
    const int lane = threadIdx.x;
    hawq_jpeg_resume_seg seg = {};
    int32_t wave_at = wave0 + (int32_t)blockIdx.x;
    if constexpr (RESUME) {
        seg = ((const hawq_jpeg_resume_seg *)(blob + segs_off))[wave_at];
        wave_at = seg.wave;
        if (wave_at < 0 || wave_at >= hd.n_waves) return;
    }
    const hawq_jpeg_prog_wave w = ((const hawq_jpeg_prog_wave *)(blob + hd.wave_off))[wave_at];
    const hawq_jpeg_scan sc = ((const hawq_jpeg_scan *)(blob + ph.scan_off))[w.scan];
    const hawq_jpeg_desc d = ((const hawq_jpeg_desc *)(blob + hd.desc_off))[sc.image];
    const bool dc_first = sc.ss == 0 && sc.ah == 0, ac = sc.ss > 0;
    for (int c = 0; c < 3; ++c) {
        const bool used = dc_first ? c < sc.ncomp : (ac && c == 0);
        if (used) {   // uniform
            const uint32_t *src = (const uint32_t *)(blob + (dc_first ? sc.dc_off[c] : sc.ac_off));
            uint32_t *dst = (uint32_t *)&tables[c];
            for (int k = lane; k < (int)(sizeof(hawq_jpeg_huff) / 4); k += WAVE) dst[k] = src[k];
        }
    }
    __syncthreads();
    const hawq_jpeg_huff *dc[3];
    for (int c = 0; c < 3; ++c) dc[c] = &tables[c];
    const int32_t *iv = (const int32_t *)(blob + sc.interval_off) + 2 * w.interval;
    const int32_t first = iv[0], last = iv[1];
    const int32_t units = jpeg_prog_units(d, sc);
    const int32_t unit0 = sc.restart ? w.interval * sc.restart : 0;
    const int32_t n_units = sc.restart ? min(sc.restart, units - unit0) : units;
    WindowSrc src{blob + sc.stream_off, window, -WINDOW, last, lane};
    LdsBlock blk{coef + d.coef_block0 * 64, stage, lane};
    int32_t st;
    if constexpr (RESUME) {
        seg.unit0 = min(max(seg.unit0, 0), n_units), seg.n_units = min(max(seg.n_units, 0), n_units - seg.unit0);
        JpegBits<WindowSrc> br(src, min(max(seg.byte, first), last), last);
        st = jpeg_resume_prog_segment(br, d, sc, dc, &tables[0], unit0, seg, blk);
    } else {
        JpegBits<WindowSrc> br(src, first, last);
        st = jpeg_prog_interval(br, d, sc, dc, &tables[0], unit0, n_units, blk);
    }
    if (lane == 0 && st != 0) atomicCAS(&status[sc.image], 0, st);
}

struct Cover {
    int8_t al[3][64];      // -1: not yet covered
    int32_t level[3][64];  // level of the last scan that covered it
};

const char *prog_refusal(const void *host_blob, int64_t blob_bytes, int64_t coef_blocks, int64_t plane_bytes, int64_t out_bytes) {
    if (!host_blob || blob_bytes < (int64_t)(sizeof(hawq_jpeg_batch_hdr) + sizeof(hawq_jpeg_prog_hdr)) || ((uintptr_t)host_blob & 7)) return "no blob, or not 8-byte aligned";
    const uint8_t *blob = (const uint8_t *)host_blob;
    hawq_jpeg_batch_hdr hd;
    hawq_jpeg_prog_hdr ph;
    memcpy(&hd, blob, sizeof hd);
    memcpy(&ph, blob + sizeof hd, sizeof ph);
    if (hd.n_images <= 0 || hd.n_images > 65535 || hd.n_waves <= 0) return "image or wave count out of range";
    if (ph.n_scans < hd.n_images || ph.n_scans > (int64_t)hd.n_images * HAWQ_JPEG_PROG_MAX_SCANS) return "scan count out of range";
    if (ph.n_levels < 1 || ph.n_levels > HAWQ_JPEG_PROG_MAX_SCANS) return "level count out of range";
    if (!inside(hd.desc_off, (int64_t)hd.n_images * (int64_t)sizeof(hawq_jpeg_desc), blob_bytes, 16)) return "descriptors outside the blob";
    if (!inside(hd.wave_off, (int64_t)hd.n_waves * (int64_t)sizeof(hawq_jpeg_prog_wave), blob_bytes, 16)) return "wave list outside the blob";
    if (!inside(ph.scan_off, (int64_t)ph.n_scans * (int64_t)sizeof(hawq_jpeg_scan), blob_bytes, 16)) return "scan table outside the blob";
    if (!inside(ph.level_off, ((int64_t)ph.n_levels + 1) * 4, blob_bytes, 16)) return "level list outside the blob";
    const hawq_jpeg_desc *desc = (const hawq_jpeg_desc *)(blob + hd.desc_off);
    const hawq_jpeg_prog_wave *waves = (const hawq_jpeg_prog_wave *)(blob + hd.wave_off);
    const hawq_jpeg_scan *scans = (const hawq_jpeg_scan *)(blob + ph.scan_off);
    const int32_t *level_start = (const int32_t *)(blob + ph.level_off);
    int64_t coef_at = 0, plane_at = 0, out_at = 0;
    int32_t scan_at = 0, deepest = 0;
    for (int32_t i = 0; i < hd.n_images; ++i) {
        const hawq_jpeg_desc &d = desc[i];
        if (const char *why = frame_refusal(d)) return why;
        const Geometry g = geometry(d);
        if (d.restart != 0 || d.n_intervals != 0 || d.stream_off != 0 || d.stream_len != 0 || d.interval_off != 0) return "a descriptor's entropy fields are not zero";
        for (int c = 0; c < 3; ++c)
            if (d.dc_off[c] != 0 || d.ac_off[c] != 0) return "a descriptor's entropy fields are not zero";
        for (int c = 0; c < d.ncomp; ++c)
            if (!inside(d.qt_off[c], 128, blob_bytes, 2)) return "quantisation table outside the blob";
        if (d.coef_block0 < coef_at || g.blocks > coef_blocks - d.coef_block0) return "coefficient blocks outside the slab or overlapping";
        if (d.plane_off < plane_at || g.plane_bytes > plane_bytes - d.plane_off) return "sample planes outside their buffer or overlapping";
        if (d.out_off < out_at || (d.out_off & 15) || g.out_bytes > out_bytes - d.out_off) return "output image outside its buffer, overlapping or unaligned";
        coef_at = d.coef_block0 + g.blocks, plane_at = d.plane_off + g.plane_bytes, out_at = d.out_off + g.out_bytes;
        // the image's scans
        Cover cover;
        memset(cover.al, -1, sizeof cover.al);
        memset(cover.level, 0, sizeof cover.level);
        int32_t n = 0;
        for (; scan_at < ph.n_scans && scans[scan_at].image == i; ++scan_at, ++n) {
            const hawq_jpeg_scan &sc = scans[scan_at];
            if (n == HAWQ_JPEG_PROG_MAX_SCANS) return "too many scans of one image";
            if (sc.ncomp != 1 && sc.ncomp != d.ncomp) return "a scan of neither one nor all components";
            if (sc.comp0 < 0 || sc.comp0 >= d.ncomp || (sc.ncomp > 1 && sc.comp0 != 0)) return "a scan's components outside the image's";
            if (sc.ss < 0 || sc.ss > sc.se || sc.se > 63 || (sc.ss == 0 && sc.se != 0)) return "a scan's spectral selection out of range";
            if (sc.ss > 0 && sc.ncomp != 1) return "an AC scan of several components";
            if (sc.al < 0 || sc.al > 13 || (sc.ah != 0 && sc.ah != sc.al + 1)) return "a scan's successive approximation out of range";
            int32_t level = 1;
            for (int c = sc.comp0; c < sc.comp0 + sc.ncomp; ++c)
                for (int k = sc.ss; k <= sc.se; ++k) {
                    if (cover.al[c][k] < 0 ? sc.ah != 0 : (sc.ah == 0 || sc.ah != cover.al[c][k])) return "progression: a scan does not continue where the last one stopped";
                    if (k > 0 && cover.al[c][0] < 0) return "progression: AC before the component's DC";
                    if (cover.level[c][k] >= level) level = cover.level[c][k] + 1;
                }
            if (sc.level != level) return "a scan's level is not the one its predecessors give";
            for (int c = sc.comp0; c < sc.comp0 + sc.ncomp; ++c)
                for (int k = sc.ss; k <= sc.se; ++k) cover.al[c][k] = (int8_t)sc.al, cover.level[c][k] = level;
            deepest = level > deepest ? level : deepest;
            const int32_t units = jpeg_prog_units(d, sc);
            if (sc.restart < 0 || sc.n_intervals != (sc.restart ? (units + sc.restart - 1) / sc.restart : 1)) return "interval count does not follow from the restart interval";
            if (sc.ss == 0 && sc.ah == 0)
                for (int c = 0; c < sc.ncomp; ++c) {
                    if (!inside(sc.dc_off[c], sizeof(hawq_jpeg_huff), blob_bytes, 4)) return "Huffman table outside the blob";
                    if (const char *why = huff_refusal((const hawq_jpeg_huff *)(blob + sc.dc_off[c]))) return why;
                }
            if (sc.ss > 0) {
                if (!inside(sc.ac_off, sizeof(hawq_jpeg_huff), blob_bytes, 4)) return "Huffman table outside the blob";
                if (const char *why = huff_refusal((const hawq_jpeg_huff *)(blob + sc.ac_off))) return why;
            }
            if (!inside(sc.stream_off, sc.stream_len, blob_bytes, 16)) return "stream outside the blob";
            if (!inside(sc.interval_off, (int64_t)sc.n_intervals * 8, blob_bytes, 4)) return "interval list outside the blob";
            const int32_t *iv = (const int32_t *)(blob + sc.interval_off);
            for (int32_t k = 0; k < sc.n_intervals; ++k)
                if (iv[2 * k] < 0 || iv[2 * k] > iv[2 * k + 1] || iv[2 * k + 1] > sc.stream_len) return "restart interval outside its stream";
        }
        if (n == 0) return "an image without scans, or the scan table is not in image order";
        for (int c = 0; c < d.ncomp; ++c)
            for (int k = 0; k < 64; ++k)
                if (cover.al[c][k] != 0) return "progression: incomplete";
    }
    if (scan_at != ph.n_scans) return "the scan table is not in image order";
    if (ph.n_levels != deepest) return "level count is not the deepest level";
    // the wave lists
    if (level_start[0] != 0 || level_start[ph.n_levels] != hd.n_waves) return "level list does not span the wave list";
    for (int32_t level = 1; level <= ph.n_levels; ++level) {
        int64_t at = level_start[level - 1];
        for (int32_t s = 0; s < ph.n_scans; ++s)
            if (scans[s].level == level)
                for (int32_t k = 0; k < scans[s].n_intervals; ++k, ++at)
                    if (at < 0 || at >= hd.n_waves || waves[at].scan != s || waves[at].interval != k) return "wave list does not name every interval once, in order, under its level";
        if (at != level_start[level]) return "wave list does not name every interval once, in order, under its level";
    }
    return nullptr;
}
}  // namespace

extern "C" int hawq_jpeg_prog_ok(const void *host_blob, int64_t blob_bytes, int64_t coef_blocks, int64_t plane_bytes, int64_t out_bytes) {
    const char *why = prog_refusal(host_blob, blob_bytes, coef_blocks, plane_bytes, out_bytes);
    if (why) hawq_set_error("hawq_jpeg_decode_batch_prog: %s", why);
    return why == nullptr;
}

namespace {
// segs: nullptr, or the host blob's segment table - one wave per segment instead of one per interval
int decode_prog(const char *name, const void *blob, const void *host_blob, int64_t blob_bytes, int16_t *coef, int64_t coef_blocks, uint8_t *planes, int64_t plane_bytes,
                uint8_t *out, int64_t out_bytes, int32_t *status, int64_t segs_off, int64_t n_segs, void *const *events, void *stream) {
    HAWQ_REQUIRE(blob && coef && planes && out && status, "%s: null pointer", name);
    const char *why = prog_refusal(host_blob, blob_bytes, coef_blocks, plane_bytes, out_bytes);
    if (!why && n_segs >= 0) why = resume_refusal(host_blob, blob_bytes, 1, segs_off, n_segs);
    HAWQ_REQUIRE(!why, "%s: %s", name, why);
    hipStream_t s = (hipStream_t)stream;
    hawq_jpeg_batch_hdr hd;
    hawq_jpeg_prog_hdr ph;
    memcpy(&hd, host_blob, sizeof hd);
    memcpy(&ph, (const uint8_t *)host_blob + sizeof hd, sizeof ph);
    const hawq_jpeg_desc *desc = (const hawq_jpeg_desc *)((const uint8_t *)host_blob + hd.desc_off);
    const int32_t *level_start = (const int32_t *)((const uint8_t *)host_blob + ph.level_off);
    const hawq_jpeg_resume_seg *segs = n_segs >= 0 ? (const hawq_jpeg_resume_seg *)((const uint8_t *)host_blob + segs_off) : nullptr;
    HAWQ_CHECK_HIP(hipMemsetAsync(coef, 0, (size_t)coef_blocks * 128, s));
    HAWQ_CHECK_HIP(hipMemsetAsync(status, 0, (size_t)hd.n_images * sizeof(int32_t), s));
    if (events) HAWQ_CHECK_HIP(hipEventRecord((hipEvent_t)events[0], s));
    int64_t seg_at = 0;
    for (int32_t level = 1; level <= ph.n_levels; ++level) {
        if (segs) {   // the segments stand in wave order: those of this level's waves are the next ones
            int64_t seg_end = seg_at;
            while (seg_end < n_segs && segs[seg_end].wave < level_start[level]) ++seg_end;
            hipLaunchKernelGGL((jpeg_prog_kernel<true>), dim3((unsigned)(seg_end - seg_at)), dim3(WAVE), 0, s, (const uint8_t *)blob, coef, status, (int32_t)seg_at,
                               segs_off);
            seg_at = seg_end;
        } else {
            const int32_t n = level_start[level] - level_start[level - 1];   // >= 1: n_levels is the deepest level a scan has
            hipLaunchKernelGGL((jpeg_prog_kernel<false>), dim3((unsigned)n), dim3(WAVE), 0, s, (const uint8_t *)blob, coef, status, level_start[level - 1], (int64_t)0);
        }
        HAWQ_CHECK_HIP(hipGetLastError());
    }
    if (events) HAWQ_CHECK_HIP(hipEventRecord((hipEvent_t)events[1], s));
    return launch_pixel_stages(blob, desc, hd.n_images, coef, planes, out, events, s);
}
}  // namespace

extern "C" int hawq_jpeg_decode_batch_prog(const void *blob, const void *host_blob, int64_t blob_bytes, int16_t *coef, int64_t coef_blocks, uint8_t *planes,
                                           int64_t plane_bytes, uint8_t *out, int64_t out_bytes, int32_t *status, void *const *events, void *stream) {
    return decode_prog("hawq_jpeg_decode_batch_prog", blob, host_blob, blob_bytes, coef, coef_blocks, planes, plane_bytes, out, out_bytes, status, 0, -1, events, stream);
}

extern "C" int hawq_jpeg_decode_batch_prog_resume(const void *blob, const void *host_blob, int64_t blob_bytes, int16_t *coef, int64_t coef_blocks, uint8_t *planes,
                                                  int64_t plane_bytes, uint8_t *out, int64_t out_bytes, int32_t *status, int64_t segs_off, int64_t n_segs,
                                                  void *const *events, void *stream) {
    HAWQ_REQUIRE(n_segs >= 0, "hawq_jpeg_decode_batch_prog_resume: segment count negative");
    return decode_prog("hawq_jpeg_decode_batch_prog_resume", blob, host_blob, blob_bytes, coef, coef_blocks, planes, plane_bytes, out, out_bytes, status, segs_off, n_segs,
                       events, stream);
}
