// Resize + CenterCrop of a ragged batch of decoded images in one launch (include/hawq_mi355.h: hawq_image_batch).
// The arithmetic is resample_u8_kernel's (adapters.hip), i.e. Pillow's ImagingResampleHorizontal_8bpc / ...Vertical_8bpc: int32
// coefficients with 22 fractional bits, accumulator started at 2^21, >> 22, clipped to 0..255, and ROUNDED TO 8 BITS BETWEEN THE
// PASSES.  What changes is where the intermediate lives and how the work is cut:
//   one workgroup = one entry of the tile table = up to 16 consecutive crop rows of one image;
//   horizontal pass: the crop columns of the input rows y0 .. y1-1 those output rows read, global -> uint8 LDS band [y1-y0][pitch];
//     a lane owns a pixel (three bytes of one input row per tap, one coefficient load per tap for the three channels);
//   vertical pass: band -> out; a lane owns one ALIGNED dword of the output row, so the store is one global dword wherever the
//     whole dword belongs to the row, and byte stores at a row's two ends (crop * 3 need not be a multiple of 4: row r of
//     the batch tensor starts at byte r * crop * 3, at any alignment).  The band bytes under that dword are two aligned LDS dwords
//     shifted together.  Consecutive lanes read consecutive LDS dwords: conflict-free.
// A skipped pass (resized size == input size: Pillow copies) moves the bytes without arithmetic.
// Indices: every per-element index comes from the tile and the lane by additions; 64-bit arithmetic only forms row base addresses.
#include <limits.h>

#include <vector>

#include "common.h"

namespace {
constexpr int LDS_BUDGET = 65536;   // two workgroups share a CU's 160 KiB
constexpr int THREADS = 256;

__host__ __device__ inline int band_pitch(int crop) { return (crop * 3 + 3) & ~3; }

// input rows [y0, y1) the crop rows row0 .. row0+rows-1 read; vb = this image's vertical bounds (unused when skip_v)
__host__ __device__ inline void band_rows(const hawq_image_desc &d, const int32_t *vb, int row0, int rows, int *y0, int *y1) {
    if (d.skip_v) {
        *y0 = d.top + row0, *y1 = d.top + row0 + rows;
        return;
    }
    int lo = INT_MAX, hi = 0;
    for (int r = row0; r < row0 + rows; ++r) {
        const int f = vb[2 * r], n = vb[2 * r + 1];
        lo = f < lo ? f : lo;
        hi = f + n > hi ? f + n : hi;
    }
    *y0 = lo, *y1 = hi;
}

__host__ __device__ inline int clip8(int ss) {
    ss >>= 22;
    return ss < 0 ? 0 : (ss > 255 ? 255 : ss);
}

// four values 0..255 -> one dword, byte 0 first.  On the device through pack4_fast (v_cvt_pk_i16_i32 + v_perm_b32), not as
// q0 | q1 << 8 | ...: hipcc folds each (shift, clip, shift, clip, or) pair of that form into one v_ashr_pk_u8_i32 and ORs the other
// pair over its upper half, which it takes to be zero; on the MI355X that half came back holding bits of the destination register's
// previous value, and byte 2 of every output dword was wrong by a few units (in whichever order the four were combined).
__host__ __device__ inline uint32_t pack4_u8(int q0, int q1, int q2, int q3) {
#ifdef __HIP_DEVICE_COMPILE__
    return (uint32_t)pack4_fast(q0, q1, q2, q3);
#else
    return (uint32_t)q0 | ((uint32_t)q1 << 8) | ((uint32_t)q2 << 16) | ((uint32_t)q3 << 24);
#endif
}

// One lane's share of a tile's horizontal pass: items (band row b, crop column o) in row-major order, THREADS apart per lane.
// A lane owns a pixel: three bytes of one input row per tap, one coefficient load per tap for the three channels.
__host__ __device__ inline void horizontal_items(const hawq_image_desc &d, const int32_t *__restrict__ coef, int crop, int pitch, int y0, int nb, int lane,
                                                 uint8_t *band) {
    const uint8_t *img = reinterpret_cast<const uint8_t *>(d.base);
    const int32_t *hb = coef + d.hb_off, *hc = coef + d.hc_off;
    int b = 0, o = lane;
    while (o >= crop) o -= crop, ++b;
    while (b < nb) {
        const uint8_t *row = img + (size_t)(y0 + b) * (size_t)d.w * 3;
        int q0, q1, q2;
        if (d.skip_h) {
            const uint8_t *p = row + (size_t)(d.left + o) * 3;
            q0 = p[0], q1 = p[1], q2 = p[2];
        } else {
            const int x0 = hb[2 * o], kn = hb[2 * o + 1];
            const int32_t *k = hc + o * d.kh;
            const uint8_t *p = row + (size_t)x0 * 3;
            int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
            for (int x = 0; x < kn; ++x, p += 3) {
                const int c = k[x];
                s0 += (int)p[0] * c, s1 += (int)p[1] * c, s2 += (int)p[2] * c;
            }
            q0 = clip8(s0), q1 = clip8(s1), q2 = clip8(s2);
        }
        uint8_t *dst = band + b * pitch + o * 3;
        dst[0] = (uint8_t)q0, dst[1] = (uint8_t)q1, dst[2] = (uint8_t)q2;
        o += THREADS;
        while (o >= crop) o -= crop, ++b;
    }
}

// One lane's share of the vertical pass: items (tile row rr, ALIGNED dword g of that output row), THREADS apart per lane.  orow + 4g - a
// is 4-byte aligned (a = the row's first byte within its dword), so the store is one dword wherever the whole dword belongs to the row
// and byte stores at the row's two ends.  The band bytes under that dword are two aligned LDS dwords shifted together.
__host__ __device__ inline void vertical_items(const hawq_image_desc &d, const hawq_image_tile &t, const int32_t *__restrict__ coef, int crop, int pitch, int y0,
                                               int lane, const uint8_t *band, uint8_t *out) {
    const int crop3 = crop * 3;
    const int npd = pitch >> 2;     // dwords of a band row
    const int NG = npd + 1;         // aligned dwords a row of crop3 bytes can touch, at any alignment of its first byte
    const int32_t *vb = coef + d.vb_off, *vc = coef + d.vc_off;
    const uint32_t *bandw = reinterpret_cast<const uint32_t *>(band);
    int rr = 0, g = lane;
    while (g >= NG) g -= NG, ++rr;
    while (rr < t.rows) {
        const int r = t.row0 + rr;
        uint8_t *orow = out + ((size_t)t.image * crop + r) * (size_t)crop3;
        const int a = (int)(reinterpret_cast<uintptr_t>(orow) & 3);
        const int j0 = 4 * g - a;   // row byte under byte 0 of output dword g (< 0: before the row)
        if (j0 < crop3) {
            // band bytes j0 .. j0+3 of a row = dwords q, q+1 shifted right by s bytes (dwords outside the row feed only bytes outside it)
            const int s = (4 - a) & 3, q = (j0 - s) >> 2;
            const bool has_lo = q >= 0, has_hi = q + 1 < npd;
            const int qlo = has_lo ? q : 0, qhi = has_hi ? q + 1 : 0;
            uint32_t w;
            if (d.skip_v) {
                const uint32_t *br = bandw + (d.top + r - y0) * npd;
                const uint32_t lo = has_lo ? br[qlo] : 0u, hi = has_hi ? br[qhi] : 0u;
                w = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * s));
            } else {
                const int f = vb[2 * r], kn = vb[2 * r + 1];
                const int32_t *k = vc + r * d.kv;
                const uint32_t *br = bandw + (f - y0) * npd;
                int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21, s3 = 1 << 21;
                for (int y = 0; y < kn; ++y, br += npd) {
                    const uint32_t lo = has_lo ? br[qlo] : 0u, hi = has_hi ? br[qhi] : 0u;
                    const uint32_t v = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * s));
                    const int c = k[y];
                    s0 += (int)(v & 255u) * c, s1 += (int)((v >> 8) & 255u) * c, s2 += (int)((v >> 16) & 255u) * c, s3 += (int)(v >> 24) * c;
                }
                w = pack4_u8(clip8(s0), clip8(s1), clip8(s2), clip8(s3));
            }
            if (j0 >= 0 && j0 + 4 <= crop3) {
                *reinterpret_cast<uint32_t *>(orow + j0) = w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (j0 + i >= 0 && j0 + i < crop3) orow[j0 + i] = (uint8_t)(w >> (8 * i));
            }
        }
        g += THREADS;
        while (g >= NG) g -= NG, ++rr;
    }
}

__global__ __launch_bounds__(THREADS) void image_batch_kernel(const hawq_image_desc *__restrict__ desc, const hawq_image_tile *__restrict__ tiles,
                                                              const int32_t *__restrict__ coef, uint8_t *__restrict__ out, int crop, int lds_bytes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t band[];
    const hawq_image_tile t = tiles[blockIdx.x];
    const hawq_image_desc d = desc[t.image];
    const int pitch = band_pitch(crop);
    int y0, y1;
    band_rows(d, coef + d.vb_off, t.row0, t.rows, &y0, &y1);
    const int nb = y1 - y0;
    if (nb <= 0 || nb > lds_bytes / pitch) return;   // hawq_image_batch_ok refuses such a table; never write past the band
    horizontal_items(d, coef, crop, pitch, y0, nb, (int)threadIdx.x, band);
    __syncthreads();
    vertical_items(d, t, coef, crop, pitch, y0, (int)threadIdx.x, band, out);
}

// why the launch does not take these (host) tables, or nullptr
const char *batch_refusal(const hawq_image_desc *desc, int n_images, const hawq_image_tile *tiles, int n_tiles, const int32_t *coef,
                          long long coef_words, int crop, int lds_bytes) {
    static thread_local char msg[256];
    if (!desc || !tiles || !coef) return "null table";
    if (n_images <= 0 || n_tiles <= 0 || crop <= 0 || coef_words < 0) return "empty batch or bad crop";
    if (crop > (1 << 20) / 3) return "crop too large";
    if (lds_bytes <= 0 || lds_bytes > LDS_BUDGET) {
        snprintf(msg, sizeof msg, "lds_bytes %d outside 1..%d (the LDS budget)", lds_bytes, LDS_BUDGET);
        return msg;
    }
    const int pitch = band_pitch(crop);
    // one pass of one image: its bounds and coefficient slices inside the table, every (first, taps) inside 0..in_size, taps <= ksize
    auto pass = [&](int i, const char *which, int b_off, int c_off, int ksize, int in_size) -> bool {
        if (ksize <= 0 || ksize > (1 << 20) || b_off < 0 || c_off < 0 || (long long)b_off + 2ll * crop > coef_words ||
            (long long)c_off + (long long)crop * ksize > coef_words) {
            snprintf(msg, sizeof msg, "image %d: %s bounds / coefficient offsets (%d, %d, ksize %d) outside the coefficient table of %lld words", i,
                     which, b_off, c_off, ksize, coef_words);
            return false;
        }
        for (int o = 0; o < crop; ++o) {
            const int f = coef[b_off + 2 * o], n = coef[b_off + 2 * o + 1];
            if (f < 0 || n < 0 || n > ksize || (long long)f + n > in_size) {
                snprintf(msg, sizeof msg, "image %d: %s bounds of output %d (first %d, taps %d) outside the input size %d or ksize %d", i, which, o, f,
                         n, in_size, ksize);
                return false;
            }
        }
        return true;
    };
    for (int i = 0; i < n_images; ++i) {
        const hawq_image_desc &d = desc[i];
        if (d.h == 0 && d.w == 0) continue;   // left to another path: it must take no tile (below)
        if (d.h <= 0 || d.w <= 0 || (long long)d.h * d.w * 3 >= (1ll << 31)) {
            snprintf(msg, sizeof msg, "image %d: bad size %d x %d", i, d.h, d.w);
            return msg;
        }
        if ((d.skip_v && d.oh != d.h) || (d.skip_h && d.ow != d.w)) {
            snprintf(msg, sizeof msg, "image %d: a skipped pass needs the resized size to equal the input's", i);
            return msg;
        }
        if (d.top < 0 || d.left < 0 || (long long)d.top + crop > d.oh || (long long)d.left + crop > d.ow) {
            snprintf(msg, sizeof msg, "image %d: crop window (top %d, left %d, crop %d) outside the resized image %d x %d", i, d.top, d.left, crop,
                     d.oh, d.ow);
            return msg;
        }
        if (!d.skip_h && !pass(i, "horizontal", d.hb_off, d.hc_off, d.kh, d.w)) return msg;
        if (!d.skip_v && !pass(i, "vertical", d.vb_off, d.vc_off, d.kv, d.h)) return msg;
    }
    // tiles: inside the crop, each image's rows covered exactly once, every band inside lds_bytes
    std::vector<int> next(n_images, 0);   // tiles of an image come in row order: the next row each image expects
    for (int k = 0; k < n_tiles; ++k) {
        const hawq_image_tile &t = tiles[k];
        if (t.image < 0 || t.image >= n_images || t.row0 < 0 || t.rows <= 0 || (long long)t.row0 + t.rows > crop) {
            snprintf(msg, sizeof msg, "tile %d (image %d, rows %d + %d) outside the crop of %d rows or the batch", k, t.image, t.row0, t.rows, crop);
            return msg;
        }
        if (t.row0 != next[t.image]) {
            snprintf(msg, sizeof msg, "tile %d: image %d expects row %d next, the tile starts at %d (gap or overlap)", k, t.image, next[t.image],
                     t.row0);
            return msg;
        }
        next[t.image] = t.row0 + t.rows;
        const hawq_image_desc &d = desc[t.image];
        if (d.h == 0 && d.w == 0) {
            snprintf(msg, sizeof msg, "tile %d: image %d has an empty descriptor (h = w = 0: not part of the launch)", k, t.image);
            return msg;
        }
        int y0, y1;
        band_rows(d, coef + d.vb_off, t.row0, t.rows, &y0, &y1);
        if (y1 <= y0 || (long long)(y1 - y0) * pitch > lds_bytes) {
            snprintf(msg, sizeof msg, "tile %d: band of %d rows x %d bytes does not fit lds_bytes %d", k, y1 - y0, pitch, lds_bytes);
            return msg;
        }
    }
    for (int i = 0; i < n_images; ++i)
        if (next[i] != crop && !(desc[i].h == 0 && desc[i].w == 0)) {
            snprintf(msg, sizeof msg, "image %d: tiles cover rows 0..%d of %d (gap)", i, next[i], crop);
            return msg;
        }
    return nullptr;
}
}  // namespace

extern "C" int hawq_image_batch_lds_budget(void) { return LDS_BUDGET; }

extern "C" int hawq_image_batch_ok(const hawq_image_desc *host_desc, int32_t n_images, const hawq_image_tile *host_tiles, int32_t n_tiles,
                                   const int32_t *host_coef, int64_t coef_words, int32_t crop, int32_t lds_bytes) {
    const char *why = batch_refusal(host_desc, n_images, host_tiles, n_tiles, host_coef, coef_words, crop, lds_bytes);
    if (why) hawq_set_error("hawq_image_batch: %s", why);
    return why == nullptr;
}

extern "C" int hawq_image_batch(const hawq_image_desc *desc, int32_t n_images, const hawq_image_tile *tiles, int32_t n_tiles, const int32_t *coef,
                                uint8_t *out, int32_t crop, int32_t lds_bytes, void *stream) {
    HAWQ_REQUIRE(desc && tiles && coef && out, "hawq_image_batch: null pointer");
    HAWQ_REQUIRE(n_images > 0 && n_tiles > 0 && crop > 0 && crop <= (1 << 20) / 3, "hawq_image_batch: empty batch or bad crop");
    HAWQ_REQUIRE(lds_bytes > 0 && lds_bytes <= LDS_BUDGET, "hawq_image_batch: lds_bytes %d outside 1..%d (the LDS budget)", lds_bytes, LDS_BUDGET);
    static const bool attrs = hipFuncSetAttribute((const void *)image_batch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BUDGET) == hipSuccess;
    HAWQ_REQUIRE(attrs, "hawq_image_batch: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    hipLaunchKernelGGL(image_batch_kernel, dim3((unsigned)n_tiles), dim3(THREADS), (size_t)lds_bytes, (hipStream_t)stream, desc, tiles, coef, out, crop,
                       lds_bytes);
    HAWQ_CHECK_HIP(hipGetLastError());
    return 0;
}
