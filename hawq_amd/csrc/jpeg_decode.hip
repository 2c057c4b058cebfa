// hawq_jpeg_decode_batch: a batch of baseline JPEGs -> tight uint8 RGB, the bytes libjpeg-turbo (ISLOW, fancy upsampling) gives.
// Three launches on one stream; the per-block and per-pixel arithmetic is jpeg_entropy.h / jpeg_pixel.h, shared with the host checker.
//   1 entropy   one 64-lane workgroup (one wave) per (image, restart interval).  Huffman decoding is serial, so every lane runs the
//               same decoder on the same state; the lanes share the work that is parallel: they fetch the stream 256 bytes at a time into
//               an LDS window (one byte per lane and load, masked at the interval's end) and copy the image's Huffman tables into LDS.
//               Lane 0 alone stores coefficients, into the pre-zeroed slab, and the status.
//   2 idct      eight lanes per 8x8 block: dequantise + column pass into LDS, row pass + range limit -> sample planes (pitch = padded width).
//   3 colour    one thread per output pixel: fancy upsampling of the chroma planes, YCbCr -> RGB.
//   2, 3 (scaled) images with desc.scale = 2, 4, 8 take jpeg_idct_scaled_kernel / jpeg_colour_scaled_kernel instead: the
//               n x n inverse DCTs of the library's DCT-domain scaling into smaller planes, and one thread per pixel of the reduced image.
//               Launched only when the batch has such an image; the two kernels above return at once for it.
//   1 (sync)    hawq_jpeg_decode_batch_sync: intervals of at least min_sync_bytes go to jpeg_sync_kernel instead - one workgroup per interval,
//               one lane per sub_bytes of it, speculative starts synchronised round after round (jpeg_sync.h); the same coefficients.
//   1 (resume)  hawq_jpeg_decode_batch_resume: one wave per SEGMENT of a restart interval - the serial kernel started at a recorded
//               resume point (jpeg_resume.h): a bit position and the predictors there; the same coefficients.
// Everything the kernels index with comes from the blob, and hawq_jpeg_batch_ok (and hawq_jpeg_sync_ok for the job table,
// hawq_jpeg_resume_ok for the segment table) has passed that blob on the host before any launch.
#include <string.h>

#include "common.h"
#include "jpeg_resume.h"
#include "jpeg_stages.h"
#include "jpeg_sync.h"

namespace {
using namespace hawq_jpeg;   // jpeg_stages.h: geometry, the checks and the stream window shared with jpeg_prog.hip
constexpr int IDCT_THREADS = 256;   // 32 blocks of 8 lanes
constexpr int SYNC_THREADS = 1024;  // lanes of one long interval (hawq_jpeg_decode_batch_sync)

const char *batch_refusal(const void *host_blob, int64_t blob_bytes, int64_t coef_blocks, int64_t plane_bytes, int64_t out_bytes) {
    if (!host_blob || blob_bytes < (int64_t)sizeof(hawq_jpeg_batch_hdr) || ((uintptr_t)host_blob & 7)) return "no blob, or not 8-byte aligned";
    const uint8_t *blob = (const uint8_t *)host_blob;
    hawq_jpeg_batch_hdr hd;
    memcpy(&hd, blob, sizeof hd);
    if (hd.n_images <= 0 || hd.n_images > 65535 || hd.n_waves <= 0) return "image or wave count out of range";
    if (!inside(hd.desc_off, (int64_t)hd.n_images * (int64_t)sizeof(hawq_jpeg_desc), blob_bytes, 16)) return "descriptors outside the blob";
    if (!inside(hd.wave_off, (int64_t)hd.n_waves * (int64_t)sizeof(hawq_jpeg_wave), blob_bytes, 16)) return "wave list outside the blob";
    const hawq_jpeg_desc *desc = (const hawq_jpeg_desc *)(blob + hd.desc_off);
    const hawq_jpeg_wave *waves = (const hawq_jpeg_wave *)(blob + hd.wave_off);
    int64_t coef_at = 0, plane_at = 0, out_at = 0, wave_at = 0;
    for (int32_t i = 0; i < hd.n_images; ++i) {
        const hawq_jpeg_desc &d = desc[i];
        if (const char *why = frame_refusal(d)) return why;
        const Geometry g = geometry(d);
        if (d.restart < 0 || d.n_intervals != (d.restart ? (g.mcus + d.restart - 1) / d.restart : 1)) return "interval count does not follow from the restart interval";
        for (int c = 0; c < d.ncomp; ++c) {
            if (!inside(d.qt_off[c], 128, blob_bytes, 2)) return "quantisation table outside the blob";
            if (!inside(d.dc_off[c], sizeof(hawq_jpeg_huff), blob_bytes, 4) || !inside(d.ac_off[c], sizeof(hawq_jpeg_huff), blob_bytes, 4))
                return "Huffman table outside the blob";
            for (int k = 0; k < 2; ++k) {
                if (const char *why = huff_refusal((const hawq_jpeg_huff *)(blob + (k ? d.ac_off[c] : d.dc_off[c])))) return why;
            }
        }
        if (!inside(d.stream_off, d.stream_len, blob_bytes, 16)) return "stream outside the blob";
        if (!inside(d.interval_off, (int64_t)d.n_intervals * 8, blob_bytes, 4)) return "interval list outside the blob";
        const int32_t *iv = (const int32_t *)(blob + d.interval_off);
        for (int32_t k = 0; k < d.n_intervals; ++k)
            if (iv[2 * k] < 0 || iv[2 * k] > iv[2 * k + 1] || iv[2 * k + 1] > d.stream_len) return "restart interval outside its stream";
        if (d.coef_block0 < coef_at || g.blocks > coef_blocks - d.coef_block0) return "coefficient blocks outside the slab or overlapping";
        if (d.plane_off < plane_at || g.plane_bytes > plane_bytes - d.plane_off) return "sample planes outside their buffer or overlapping";
        if (d.out_off < out_at || (d.out_off & 15) || g.out_bytes > out_bytes - d.out_off) return "output image outside its buffer, overlapping or unaligned";
        coef_at = d.coef_block0 + g.blocks, plane_at = d.plane_off + g.plane_bytes, out_at = d.out_off + g.out_bytes;
        for (int32_t k = 0; k < d.n_intervals; ++k, ++wave_at)
            if (wave_at >= hd.n_waves || waves[wave_at].image != i || waves[wave_at].interval != k) return "wave list does not name every interval once, in order";
    }
    if (wave_at != hd.n_waves) return "wave list longer than the intervals";
    return nullptr;
}

// ---- stage 1 ---------------------------------------------------------------------------------------------------------------------
// The stream comes through the 256-byte LDS window of jpeg_stages.h (WindowSrc).
// RESUME (hawq_jpeg_decode_batch_resume): workgroup x decodes segment x of the table at segs_off - the units, the start position and the
// predictors its entry names (jpeg_resume.h), the units clamped to those of the entry's interval.
template <bool RESUME>
__global__ __launch_bounds__(WAVE) void jpeg_entropy_kernel(const uint8_t *__restrict__ blob, int16_t *__restrict__ coef, int32_t *__restrict__ status, int32_t skip_from,
                                                            int64_t segs_off) {
    __shared__ hawq_jpeg_huff tables[6];   // dc, ac per component
    __shared__ uint8_t window[WINDOW];
    const hawq_jpeg_batch_hdr hd = *(const hawq_jpeg_batch_hdr *)blob;
    const int lane = threadIdx.x;
    hawq_jpeg_resume_seg seg = {};
    int32_t wave_at = (int32_t)blockIdx.x;
    if constexpr (RESUME) {
        seg = ((const hawq_jpeg_resume_seg *)(blob + segs_off))[blockIdx.x];
        wave_at = seg.wave;
    }
    if (wave_at < 0 || wave_at >= hd.n_waves) return;
    const hawq_jpeg_wave w = ((const hawq_jpeg_wave *)(blob + hd.wave_off))[wave_at];
    const hawq_jpeg_desc d = ((const hawq_jpeg_desc *)(blob + hd.desc_off))[w.image];
    const hawq_jpeg_huff *dc[3], *ac[3];
    for (int c = 0; c < 3; ++c) {
        const int cc = c < d.ncomp ? c : 0;
        const uint32_t *sd = (const uint32_t *)(blob + d.dc_off[cc]), *sa = (const uint32_t *)(blob + d.ac_off[cc]);
        uint32_t *td = (uint32_t *)&tables[2 * c], *ta = (uint32_t *)&tables[2 * c + 1];
        for (int k = lane; k < (int)(sizeof(hawq_jpeg_huff) / 4); k += WAVE) td[k] = sd[k], ta[k] = sa[k];
        dc[c] = &tables[2 * c], ac[c] = &tables[2 * c + 1];
    }
    __syncthreads();
    const int32_t *iv = (const int32_t *)(blob + d.interval_off) + 2 * w.interval;
    const int32_t first = iv[0], last = iv[1];
    if (skip_from > 0 && last - first >= skip_from) return;   // a job of jpeg_sync_kernel (uniform: after the only barrier so far)
    const int32_t mcus = d.mcus_x * d.mcus_y;
    const int32_t mcu0 = d.restart ? w.interval * d.restart : 0;
    const int32_t n_mcu = d.restart ? min(d.restart, mcus - mcu0) : mcus;
    WindowSrc src{blob + d.stream_off, window, -WINDOW, last, lane};
    int32_t st;
    if constexpr (RESUME) {
        seg.unit0 = min(max(seg.unit0, 0), n_mcu), seg.n_units = min(max(seg.n_units, 0), n_mcu - seg.unit0);
        JpegBits<WindowSrc> br(src, min(max(seg.byte, first), last), last);
        st = jpeg_resume_segment(br, d, dc, ac, mcu0, seg, coef + d.coef_block0 * 64, lane == 0);
    } else {
        JpegBits<WindowSrc> br(src, first, last);
        st = jpeg_decode_interval(br, d, dc, ac, mcu0, n_mcu, coef + d.coef_block0 * 64, lane == 0);
    }
    if (lane == 0 && st != 0) atomicCAS(&status[w.image], 0, st);
}

// ---- stage 1, long intervals -----------------------------------------------------------------------------------------------------
// One workgroup per job (jpeg_sync.h); thread t takes sub-sequences t, t + SYNC_THREADS, ...  The lanes diverge: each
// reads its own bytes straight from the blob through the cache.  Per sub-sequence state lives in the job's scratch slice; the barriers
// order its reads and writes (a round reads the neighbours' end states in one phase and writes its own in the next).
struct GlobalSrc {
    const uint8_t *stream;
    __device__ __forceinline__ uint8_t byte(int32_t pos) const { return stream[pos]; }
};

__global__ __launch_bounds__(SYNC_THREADS) void jpeg_sync_kernel(const uint8_t *blob, int16_t *coef, int32_t *status, int64_t jobs_off, int32_t sub_bytes,
                                                                 uint8_t *scratch) {
    __shared__ hawq_jpeg_huff tables[6];   // dc, ac per component
    __shared__ uint16_t luts[6][JPEG_SYNC_LUT_SIZE];
    __shared__ int32_t seg[SYNC_THREADS][4];
    __shared__ int32_t all_decodes, first_bad;
    const hawq_jpeg_batch_hdr hd = *(const hawq_jpeg_batch_hdr *)blob;
    const int t = threadIdx.x;
    const hawq_jpeg_sync_job job = ((const hawq_jpeg_sync_job *)(blob + jobs_off))[blockIdx.x];
    const hawq_jpeg_wave w = ((const hawq_jpeg_wave *)(blob + hd.wave_off))[job.wave];
    const hawq_jpeg_desc d = ((const hawq_jpeg_desc *)(blob + hd.desc_off))[w.image];
    const JpegSyncTables tb{tables, &luts[0][0]};
    for (int c = 0; c < 3; ++c) {
        const int cc = c < d.ncomp ? c : 0;
        const uint32_t *sd = (const uint32_t *)(blob + d.dc_off[cc]), *sa = (const uint32_t *)(blob + d.ac_off[cc]);
        uint32_t *td = (uint32_t *)&tables[2 * c], *ta = (uint32_t *)&tables[2 * c + 1];
        for (int k = t; k < (int)(sizeof(hawq_jpeg_huff) / 4); k += SYNC_THREADS) td[k] = sd[k], ta[k] = sa[k];
    }
    if (t == 0) all_decodes = 0, first_bad = 0x7FFFFFFF;
    __syncthreads();
    for (int k = t; k < 6 * JPEG_SYNC_LUT_SIZE; k += SYNC_THREADS) luts[k / JPEG_SYNC_LUT_SIZE][k % JPEG_SYNC_LUT_SIZE] = jpeg_sync_lut_entry(&tables[k / JPEG_SYNC_LUT_SIZE], k % JPEG_SYNC_LUT_SIZE);
    __syncthreads();
    const int32_t *iv = (const int32_t *)(blob + d.interval_off) + 2 * w.interval;
    const int32_t first = iv[0], last = iv[1], n = job.n_sub;
    const int32_t mcus = d.mcus_x * d.mcus_y;
    const int32_t mcu0 = d.restart ? w.interval * d.restart : 0;
    const int32_t n_mcu = d.restart ? min(d.restart, mcus - mcu0) : mcus;
    hawq_jpeg_sync_job_hdr *jh = (hawq_jpeg_sync_job_hdr *)(scratch + job.scratch_off);
    hawq_jpeg_sync_sub *sub = (hawq_jpeg_sync_sub *)(jh + 1);
    GlobalSrc src{blob + d.stream_off};
    int32_t decodes = 0, rounds = 1;
    // speculate
    for (int32_t i = t; i < n; i += SYNC_THREADS) {
        hawq_jpeg_sync_sub s;
        s.start_pos = jpeg_sync_guess(src, first, i, sub_bytes), s.start_uk = 0;
        jpeg_sync_lane(src, d, tb, last, jpeg_sync_limit(first, i, n, sub_bytes), sub_bytes, s, nullptr);
        sub[i] = s;
        ++decodes;
    }
    __syncthreads();
    // synchronise: at most n decode passes in all, since pass r leaves lanes 0 .. r - 1 with their true states.  A lane without a valid
    // end (a wrong guess that ran into an error, or damage) changes nothing behind it.
    for (int32_t r = 1; r < n; ++r) {
        int changed = 0;
        for (int32_t i = t; i < n; i += SYNC_THREADS) {
            if (i == 0) continue;
            const int32_t pos = sub[i - 1].end_pos, uk = sub[i - 1].end_uk;
            if (pos >= 0 && (pos != sub[i].start_pos || uk != sub[i].start_uk)) {
                sub[i].start_pos = pos, sub[i].start_uk = uk;
                sub[i].blocks = -1;   // decode again in this round
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
        for (int32_t i = t; i < n; i += SYNC_THREADS) {
            if (sub[i].blocks != -1) continue;
            hawq_jpeg_sync_sub s = sub[i];
            jpeg_sync_lane(src, d, tb, last, jpeg_sync_limit(first, i, n, sub_bytes), sub_bytes, s, nullptr);
            sub[i] = s;
            ++decodes;
        }
        __syncthreads();
        ++rounds;
    }
    // place: exclusive scan of the block counts and DC sums, a contiguous segment per thread; the lanes behind the first one without
    // an end do not start at a true state and write nothing
    const int32_t per = (n + SYNC_THREADS - 1) / SYNC_THREADS;
    const int32_t lo = min(n, t * per), hi = min(n, lo + per);
    int32_t run[4] = {0, 0, 0, 0};
    for (int32_t i = lo; i < hi; ++i) {
        if (sub[i].end_pos < 0) {
            atomicMin(&first_bad, i);
            break;   // the sums behind it are not used
        }
        run[0] += sub[i].blocks;
        for (int c = 0; c < 3; ++c) run[1 + c] = (int32_t)((uint32_t)run[1 + c] + (uint32_t)sub[i].dc[c]);
    }
    for (int c = 0; c < 4; ++c) seg[t][c] = run[c];
    __syncthreads();
    if (t < 4) {   // column t of the segment sums
        uint32_t at = 0;
        for (int k = 0; k * per < n; ++k) {   // the segments that hold a sub-sequence (k < SYNC_THREADS: per * SYNC_THREADS >= n)
            const uint32_t v = (uint32_t)seg[k][t];
            seg[k][t] = (int32_t)at;
            at += v;
        }
    }
    __syncthreads();
    for (int c = 0; c < 4; ++c) run[c] = seg[t][c];
    for (int32_t i = lo; i < hi; ++i) {
        const hawq_jpeg_sync_sub s = sub[i];
        if (i > first_bad) sub[i].start_pos = -1;
        sub[i].blocks = run[0];
        for (int c = 0; c < 3; ++c) sub[i].dc[c] = run[1 + c];
        run[0] += s.blocks;
        for (int c = 0; c < 3; ++c) run[1 + c] = (int32_t)((uint32_t)run[1 + c] + (uint32_t)s.dc[c]);
    }
    __syncthreads();
    // write
    const JpegSyncWriter wr{coef + d.coef_block0 * 64, mcu0, n_mcu * jpeg_sync_bpm(d)};
    for (int32_t i = t; i < n; i += SYNC_THREADS) {
        hawq_jpeg_sync_sub s = sub[i];
        const int32_t st = jpeg_sync_lane(src, d, tb, last, jpeg_sync_limit(first, i, n, sub_bytes), sub_bytes, s, &wr);
        if (st != 0) atomicCAS(&status[w.image], 0, st);
    }
    atomicAdd(&all_decodes, decodes);
    __syncthreads();
    if (t == 0) jh->rounds = rounds, jh->decodes = all_decodes, jh->reserved[0] = jh->reserved[1] = 0;
}

// ---- stage 2 ---------------------------------------------------------------------------------------------------------------------
// Eight lanes per block: lane x runs column x into the block's workspace in LDS, then lane y runs row y out of it.
__global__ __launch_bounds__(IDCT_THREADS) void jpeg_idct_kernel(const uint8_t *__restrict__ blob, const int16_t *__restrict__ coef, uint8_t *__restrict__ planes) {
    __shared__ int32_t ws[IDCT_THREADS / 8][64];
    const hawq_jpeg_batch_hdr hd = *(const hawq_jpeg_batch_hdr *)blob;
    const hawq_jpeg_desc &d = ((const hawq_jpeg_desc *)(blob + hd.desc_off))[blockIdx.y];   // read in place: qt_off is indexed by the component
    if (d.scale > 1) return;   // jpeg_idct_scaled_kernel's (uniform: before the barrier)
    const int slot = threadIdx.x >> 3, lane8 = threadIdx.x & 7;
    int64_t b = (int64_t)blockIdx.x * (IDCT_THREADS / 8) + slot;   // block of the image, component after component
    int64_t comp0 = 0, bw = 0;
    int comp = -1;
    for (int c = 0; c < d.ncomp && comp < 0; ++c) {
        bw = (int64_t)d.mcus_x * jpeg_comp_h(d, c);
        const int64_t n = bw * d.mcus_y * jpeg_comp_v(d, c);
        if (b < n)
            comp = c;
        else
            b -= n, comp0 += n;
    }
    if (comp >= 0) jpeg_idct_column(coef + (d.coef_block0 + comp0 + b) * 64, (const uint16_t *)(blob + d.qt_off[comp]), lane8, ws[slot]);
    __syncthreads();
    if (comp >= 0) {
        const int64_t by = b / bw, bx = b - by * bw, pitch = bw * 8;
        jpeg_idct_row(ws[slot], lane8, planes + d.plane_off + comp0 * 64 + (by * 8 + lane8) * pitch + bx * 8);
    }
}

// The same for an image with scale 2, 4 or 8: the n x n inverse DCT, n = jpeg_comp_n of the block's component, into planes of pitch
// block columns x n.  Lane x runs column x when the row pass reads it, lane y < n runs row y.
__global__ __launch_bounds__(IDCT_THREADS) void jpeg_idct_scaled_kernel(const uint8_t *__restrict__ blob, const int16_t *__restrict__ coef, uint8_t *__restrict__ planes) {
    __shared__ int32_t ws[IDCT_THREADS / 8][64];
    const hawq_jpeg_batch_hdr hd = *(const hawq_jpeg_batch_hdr *)blob;
    const hawq_jpeg_desc &d = ((const hawq_jpeg_desc *)(blob + hd.desc_off))[blockIdx.y];
    if (d.scale <= 1) return;   // jpeg_idct_kernel's (uniform: before the barrier)
    const int slot = threadIdx.x >> 3, lane8 = threadIdx.x & 7;
    int64_t b = (int64_t)blockIdx.x * (IDCT_THREADS / 8) + slot;
    int64_t comp0 = 0, plane0 = 0, bw = 0;   // blocks and plane bytes of the components before the block's
    int comp = -1, n = 0;
    for (int c = 0; c < d.ncomp && comp < 0; ++c) {
        bw = (int64_t)d.mcus_x * jpeg_comp_h(d, c);
        n = jpeg_comp_n(d, c);
        const int64_t blocks = bw * d.mcus_y * jpeg_comp_v(d, c);
        if (b < blocks)
            comp = c;
        else
            b -= blocks, comp0 += blocks, plane0 += blocks * n * n;
    }
    if (comp >= 0) jpeg_idct_column_n(coef + (d.coef_block0 + comp0 + b) * 64, (const uint16_t *)(blob + d.qt_off[comp]), n, lane8, ws[slot]);
    __syncthreads();
    if (comp >= 0 && lane8 < n) {
        const int64_t by = b / bw, bx = b - by * bw, pitch = bw * n;
        jpeg_idct_row_n(ws[slot], n, lane8, planes + d.plane_off + plane0 + (by * n + lane8) * pitch + bx * n);
    }
}

// ---- stage 3 ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jpeg_colour_kernel(const uint8_t *__restrict__ blob, const uint8_t *__restrict__ planes, uint8_t *__restrict__ out) {
    const hawq_jpeg_batch_hdr hd = *(const hawq_jpeg_batch_hdr *)blob;
    const hawq_jpeg_desc d = ((const hawq_jpeg_desc *)(blob + hd.desc_off))[blockIdx.y];
    if (d.scale > 1) return;   // jpeg_colour_scaled_kernel's
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)d.width * d.height) return;
    const int32_t y = (int32_t)(p / d.width), x = (int32_t)(p - (int64_t)y * d.width);
    uint8_t rgb[3];
    jpeg_pixel(d, planes + d.plane_off, x, y, rgb);
    uint8_t *o = out + d.out_off + p * 3;
    o[0] = rgb[0], o[1] = rgb[1], o[2] = rgb[2];
}

__global__ __launch_bounds__(256) void jpeg_colour_scaled_kernel(const uint8_t *__restrict__ blob, const uint8_t *__restrict__ planes, uint8_t *__restrict__ out) {
    const hawq_jpeg_batch_hdr hd = *(const hawq_jpeg_batch_hdr *)blob;
    const hawq_jpeg_desc d = ((const hawq_jpeg_desc *)(blob + hd.desc_off))[blockIdx.y];
    if (d.scale <= 1) return;   // jpeg_colour_kernel's
    const int32_t ow = jpeg_out_width(d);
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)ow * jpeg_out_height(d)) return;
    const int32_t y = (int32_t)(p / ow), x = (int32_t)(p - (int64_t)y * ow);
    uint8_t rgb[3];
    jpeg_pixel_scaled(d, planes + d.plane_off, x, y, rgb);
    uint8_t *o = out + d.out_off + p * 3;
    o[0] = rgb[0], o[1] = rgb[1], o[2] = rgb[2];
}
}  // namespace

int hawq_jpeg::launch_pixel_stages(const void *blob, const hawq_jpeg_desc *host_desc, int32_t n_images, const int16_t *coef, uint8_t *planes, uint8_t *out,
                                   void *const *events, hipStream_t s) {
    // [0]: the full-size images, which the two kernels of old decode; [1]: the scaled ones.  A kind without an image launches nothing.
    int64_t max_blocks[2] = {0, 0}, max_pixels[2] = {0, 0};
    for (int32_t i = 0; i < n_images; ++i) {
        const Geometry g = geometry(host_desc[i]);
        const int k = host_desc[i].scale > 1;
        max_blocks[k] = g.blocks > max_blocks[k] ? g.blocks : max_blocks[k];
        max_pixels[k] = g.out_bytes / 3 > max_pixels[k] ? g.out_bytes / 3 : max_pixels[k];
    }
    if (max_blocks[0]) {
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks[0] + IDCT_THREADS / 8 - 1) / (IDCT_THREADS / 8)), (unsigned)n_images), dim3(IDCT_THREADS), 0, s,
                           (const uint8_t *)blob, coef, planes);
        HAWQ_CHECK_HIP(hipGetLastError());
    }
    if (max_blocks[1]) {
        hipLaunchKernelGGL(jpeg_idct_scaled_kernel, dim3((unsigned)((max_blocks[1] + IDCT_THREADS / 8 - 1) / (IDCT_THREADS / 8)), (unsigned)n_images), dim3(IDCT_THREADS),
                           0, s, (const uint8_t *)blob, coef, planes);
        HAWQ_CHECK_HIP(hipGetLastError());
    }
    if (events) HAWQ_CHECK_HIP(hipEventRecord((hipEvent_t)events[2], s));
    if (max_pixels[0]) {
        hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((max_pixels[0] + 255) / 256), (unsigned)n_images), dim3(256), 0, s, (const uint8_t *)blob,
                           (const uint8_t *)planes, out);
        HAWQ_CHECK_HIP(hipGetLastError());
    }
    if (max_pixels[1]) {
        hipLaunchKernelGGL(jpeg_colour_scaled_kernel, dim3((unsigned)((max_pixels[1] + 255) / 256), (unsigned)n_images), dim3(256), 0, s, (const uint8_t *)blob,
                           (const uint8_t *)planes, out);
        HAWQ_CHECK_HIP(hipGetLastError());
    }
    if (events) HAWQ_CHECK_HIP(hipEventRecord((hipEvent_t)events[3], s));
    return 0;
}

namespace {
// the job table against the blob batch_refusal has passed
const char *sync_refusal(const void *host_blob, int64_t blob_bytes, int32_t sub_bytes, int32_t min_sync_bytes, int64_t jobs_off, int32_t n_jobs, int64_t scratch_bytes) {
    if (!host_blob || blob_bytes < (int64_t)sizeof(hawq_jpeg_batch_hdr) || ((uintptr_t)host_blob & 7)) return "no blob, or not 8-byte aligned";
    if (sub_bytes < HAWQ_JPEG_SYNC_SUB_MIN || sub_bytes > HAWQ_JPEG_SYNC_SUB_MAX || sub_bytes % 4) return "sub_bytes is no multiple of 4 in 16..4096";
    if (min_sync_bytes < 1) return "min_sync_bytes below 1";
    if (n_jobs < 0 || scratch_bytes < 0) return "job count or scratch size negative";
    const uint8_t *blob = (const uint8_t *)host_blob;
    hawq_jpeg_batch_hdr hd;
    memcpy(&hd, blob, sizeof hd);
    if (hd.n_images <= 0 || hd.n_waves <= 0 || n_jobs > hd.n_waves) return "more jobs than waves";
    if (!inside(hd.desc_off, (int64_t)hd.n_images * (int64_t)sizeof(hawq_jpeg_desc), blob_bytes, 16)) return "descriptors outside the blob";
    if (!inside(hd.wave_off, (int64_t)hd.n_waves * (int64_t)sizeof(hawq_jpeg_wave), blob_bytes, 16)) return "wave list outside the blob";
    if (!inside(jobs_off, (int64_t)n_jobs * (int64_t)sizeof(hawq_jpeg_sync_job), blob_bytes, 16)) return "job table outside the blob";
    const hawq_jpeg_desc *desc = (const hawq_jpeg_desc *)(blob + hd.desc_off);
    const hawq_jpeg_wave *waves = (const hawq_jpeg_wave *)(blob + hd.wave_off);
    const hawq_jpeg_sync_job *jobs = (const hawq_jpeg_sync_job *)(blob + jobs_off);
    int64_t scratch_at = 0;
    int32_t wave_at = 0, long_waves = 0;
    for (int32_t k = 0; k <= n_jobs; ++k) {
        // the waves between the previous job's and this one's (behind the last job: the rest) are short
        const int32_t upto = k < n_jobs ? jobs[k].wave : hd.n_waves;
        if (upto < wave_at || upto > hd.n_waves || (k < n_jobs && upto == hd.n_waves)) return "a job names no wave, or the jobs are out of order";
        for (int32_t w = wave_at; w <= upto && w < hd.n_waves; ++w) {
            if (waves[w].image < 0 || waves[w].image >= hd.n_images) return "wave list names no image";
            const hawq_jpeg_desc &d = desc[waves[w].image];
            if (waves[w].interval < 0 || waves[w].interval >= d.n_intervals || !inside(d.interval_off, (int64_t)d.n_intervals * 8, blob_bytes, 4))
                return "wave list names no interval";
            const int32_t *iv = (const int32_t *)(blob + d.interval_off) + 2 * waves[w].interval;
            if (iv[0] < 0 || iv[0] > iv[1] || iv[1] > d.stream_len || !inside(d.stream_off, d.stream_len, blob_bytes, 16)) return "restart interval outside its stream";
            const int32_t len = iv[1] - iv[0];
            long_waves += len >= min_sync_bytes;
            if (w < upto) {
                if (len >= min_sync_bytes) return "an interval of at least min_sync_bytes has no job";
                continue;
            }
            if (len < min_sync_bytes) return "a job on an interval shorter than min_sync_bytes";
            if (jobs[k].n_sub != (len + sub_bytes - 1) / sub_bytes) return "a job's n_sub does not follow from its interval";
            const int64_t need = (int64_t)sizeof(hawq_jpeg_sync_job_hdr) + (int64_t)jobs[k].n_sub * (int64_t)sizeof(hawq_jpeg_sync_sub);
            if (jobs[k].scratch_off < scratch_at || !inside(jobs[k].scratch_off, need, scratch_bytes, 16)) return "a job's scratch slice outside the scratch or overlapping";
            scratch_at = jobs[k].scratch_off + need;
        }
        wave_at = upto + 1;
    }
    return long_waves == n_jobs ? nullptr : "the jobs do not name every long interval once";
}

int decode_batch(const void *blob, const void *host_blob, int64_t blob_bytes, int16_t *coef, int64_t coef_blocks, uint8_t *planes, int64_t plane_bytes, uint8_t *out,
                 int64_t out_bytes, int32_t *status, int32_t sub_bytes, int32_t skip_from, int64_t jobs_off, int32_t n_jobs, void *scratch, int64_t segs_off,
                 int64_t n_segs, void *const *events, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    hawq_jpeg_batch_hdr hd;
    memcpy(&hd, host_blob, sizeof hd);
    const hawq_jpeg_desc *desc = (const hawq_jpeg_desc *)((const uint8_t *)host_blob + hd.desc_off);
    HAWQ_CHECK_HIP(hipMemsetAsync(coef, 0, (size_t)coef_blocks * 128, s));
    HAWQ_CHECK_HIP(hipMemsetAsync(status, 0, (size_t)hd.n_images * sizeof(int32_t), s));
    if (events) HAWQ_CHECK_HIP(hipEventRecord((hipEvent_t)events[0], s));
    if (n_segs > 0)   // one wave per segment (hawq_jpeg_decode_batch_resume)
        hipLaunchKernelGGL((jpeg_entropy_kernel<true>), dim3((unsigned)n_segs), dim3(WAVE), 0, s, (const uint8_t *)blob, coef, status, 0, segs_off);
    else
        hipLaunchKernelGGL((jpeg_entropy_kernel<false>), dim3((unsigned)hd.n_waves), dim3(WAVE), 0, s, (const uint8_t *)blob, coef, status, skip_from, (int64_t)0);
    HAWQ_CHECK_HIP(hipGetLastError());
    if (n_jobs > 0) {
        hipLaunchKernelGGL(jpeg_sync_kernel, dim3((unsigned)n_jobs), dim3(SYNC_THREADS), 0, s, (const uint8_t *)blob, coef, status, jobs_off, sub_bytes,
                           (uint8_t *)scratch);
        HAWQ_CHECK_HIP(hipGetLastError());
    }
    if (events) HAWQ_CHECK_HIP(hipEventRecord((hipEvent_t)events[1], s));
    return launch_pixel_stages(blob, desc, hd.n_images, coef, planes, out, events, s);
}
}  // namespace

extern "C" int hawq_jpeg_batch_ok(const void *host_blob, int64_t blob_bytes, int64_t coef_blocks, int64_t plane_bytes, int64_t out_bytes) {
    const char *why = batch_refusal(host_blob, blob_bytes, coef_blocks, plane_bytes, out_bytes);
    if (why) hawq_set_error("hawq_jpeg_decode_batch: %s", why);
    return why == nullptr;
}

extern "C" int hawq_jpeg_decode_batch(const void *blob, const void *host_blob, int64_t blob_bytes, int16_t *coef, int64_t coef_blocks, uint8_t *planes,
                                      int64_t plane_bytes, uint8_t *out, int64_t out_bytes, int32_t *status, void *const *events, void *stream) {
    HAWQ_REQUIRE(blob && coef && planes && out && status, "hawq_jpeg_decode_batch: null pointer");
    const char *why = batch_refusal(host_blob, blob_bytes, coef_blocks, plane_bytes, out_bytes);
    HAWQ_REQUIRE(!why, "hawq_jpeg_decode_batch: %s", why);
    return decode_batch(blob, host_blob, blob_bytes, coef, coef_blocks, planes, plane_bytes, out, out_bytes, status, 0, 0, 0, 0, nullptr, 0, 0, events, stream);
}

extern "C" int hawq_jpeg_sync_ok(const void *host_blob, int64_t blob_bytes, int32_t sub_bytes, int32_t min_sync_bytes, int64_t jobs_off, int32_t n_jobs,
                                 int64_t scratch_bytes) {
    const char *why = sync_refusal(host_blob, blob_bytes, sub_bytes, min_sync_bytes, jobs_off, n_jobs, scratch_bytes);
    if (why) hawq_set_error("hawq_jpeg_decode_batch_sync: %s", why);
    return why == nullptr;
}

extern "C" int hawq_jpeg_decode_batch_sync(const void *blob, const void *host_blob, int64_t blob_bytes, int16_t *coef, int64_t coef_blocks, uint8_t *planes,
                                           int64_t plane_bytes, uint8_t *out, int64_t out_bytes, int32_t *status, int32_t sub_bytes, int32_t min_sync_bytes,
                                           int64_t jobs_off, int32_t n_jobs, void *scratch, int64_t scratch_bytes, void *const *events, void *stream) {
    HAWQ_REQUIRE(blob && coef && planes && out && status && (scratch || n_jobs == 0), "hawq_jpeg_decode_batch_sync: null pointer");
    const char *why = batch_refusal(host_blob, blob_bytes, coef_blocks, plane_bytes, out_bytes);
    if (!why) why = sync_refusal(host_blob, blob_bytes, sub_bytes, min_sync_bytes, jobs_off, n_jobs, scratch_bytes);
    HAWQ_REQUIRE(!why, "hawq_jpeg_decode_batch_sync: %s", why);
    return decode_batch(blob, host_blob, blob_bytes, coef, coef_blocks, planes, plane_bytes, out, out_bytes, status, sub_bytes, min_sync_bytes, jobs_off, n_jobs, scratch,
                        0, 0, events, stream);
}

extern "C" int hawq_jpeg_decode_batch_resume(const void *blob, const void *host_blob, int64_t blob_bytes, int16_t *coef, int64_t coef_blocks, uint8_t *planes,
                                             int64_t plane_bytes, uint8_t *out, int64_t out_bytes, int32_t *status, int64_t segs_off, int64_t n_segs,
                                             void *const *events, void *stream) {
    HAWQ_REQUIRE(blob && coef && planes && out && status, "hawq_jpeg_decode_batch_resume: null pointer");
    const char *why = batch_refusal(host_blob, blob_bytes, coef_blocks, plane_bytes, out_bytes);
    if (!why) why = resume_refusal(host_blob, blob_bytes, 0, segs_off, n_segs);
    HAWQ_REQUIRE(!why, "hawq_jpeg_decode_batch_resume: %s", why);
    return decode_batch(blob, host_blob, blob_bytes, coef, coef_blocks, planes, plane_bytes, out, out_bytes, status, 0, 0, 0, 0, nullptr, segs_off, n_segs, events, stream);
}
