// What jpeg_decode.hip and jpeg_prog.hip share: the geometry of an accepted image, the checks both blob checkers make, the stream
// window of the entropy kernels, and the launch of stages 2 and 3 (whose kernels live in jpeg_decode.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg_pixel.h"

namespace hawq_jpeg {
constexpr int WAVE = 64;
constexpr int WINDOW = 256;   // stream bytes in LDS
constexpr int MAX_SIDE = 8192;

struct Geometry {
    int64_t blocks, plane_bytes, out_bytes;
    int32_t mcus;
};

// block / byte counts of an image whose sampling and size have been checked
inline Geometry geometry(const hawq_jpeg_desc &d) {
    Geometry g;
    g.mcus = d.mcus_x * d.mcus_y;
    g.blocks = (int64_t)g.mcus * (d.ncomp == 1 ? 1 : d.hs * d.vs + 2);
    g.plane_bytes = 0;   // n x n samples per block, n = 8 at full size (jpeg_comp_n)
    for (int c = 0; c < d.ncomp; ++c) g.plane_bytes += (int64_t)g.mcus * jpeg_comp_h(d, c) * jpeg_comp_v(d, c) * jpeg_comp_n(d, c) * jpeg_comp_n(d, c);
    g.out_bytes = (int64_t)jpeg_out_width(d) * jpeg_out_height(d) * 3;
    return g;
}

inline bool inside(int64_t off, int64_t len, int64_t total, int align) { return off >= 0 && len >= 0 && off % align == 0 && off <= total && len <= total - off; }

// size, sampling and MCU counts of a descriptor: nullptr, or why not
inline const char *frame_refusal(const hawq_jpeg_desc &d) {
    if (d.width < 1 || d.height < 1 || d.width > MAX_SIDE || d.height > MAX_SIDE) return "image size outside 1..8192";
    const bool gray = d.ncomp == 1 && d.hs == 1 && d.vs == 1;
    const bool colour = d.ncomp == 3 && ((d.hs == 1 && d.vs == 1) || (d.hs == 2 && d.vs == 1) || (d.hs == 2 && d.vs == 2));
    if (!gray && !colour) return "component count or sampling factors not supported";
    if (d.mcus_x != (d.width + 8 * d.hs - 1) / (8 * d.hs) || d.mcus_y != (d.height + 8 * d.vs - 1) / (8 * d.vs)) return "MCU counts do not follow from the size";
    if (d.scale != 0 && d.scale != 1 && d.scale != 2 && d.scale != 4 && d.scale != 8) return "scale is none of 0, 1, 2, 4, 8";
    return nullptr;
}

// the canonical assignment (T.81 C.2) with every value inside huffval: nullptr, or why not
inline const char *huff_refusal(const hawq_jpeg_huff *t) {
    int codes = 0;
    int32_t code = 0, values = 0;
    for (int l = 1; l <= 16; ++l, code <<= 1) {
        if (t->maxcode[l] < -1 || t->maxcode[l] >= (1 << l)) return "Huffman table: maxcode out of range";
        if (t->maxcode[l] >= 0) {
            if (t->mincode[l] != code || t->maxcode[l] < code || t->valptr[l] != values) return "Huffman table: not canonical";
            values += t->maxcode[l] - code + 1;
            if (values > 256) return "Huffman table: values outside huffval";
            code = t->maxcode[l] + 1;
            ++codes;
        }
    }
    return codes ? nullptr : "Huffman table missing";
}

#if defined(__HIPCC__)
// The stream through a 256-byte LDS window.  Every lane calls byte() with the same position (the decoder's state is the same in all
// lanes), so the refill is taken by the whole wave; a lane loads only positions inside [0, end) of its interval's stream.
struct WindowSrc {
    const uint8_t *stream;   // global
    uint8_t *win;            // LDS [WINDOW]
    int32_t base, end, lane;
    __device__ __forceinline__ uint8_t byte(int32_t pos) {
        if (pos < base || pos >= base + WINDOW) {
            __syncthreads();   // single-wave workgroup: orders the LDS reads of the old window before the new one is written
            base = pos & ~(WINDOW - 1);
            for (int k = 0; k < WINDOW / WAVE; ++k) {
                const int32_t at = base + k * WAVE + lane;
                win[k * WAVE + lane] = at < end ? stream[at] : (uint8_t)0;
            }
            __syncthreads();
        }
        return win[pos - base];
    }
};
#endif

// Stages 2 and 3 on `stream` for the n_images descriptors of `blob` (device; host_desc: the same descriptors on the host): dequantise +
// IDCT coef -> planes, upsampling + colour planes -> out.  events: NULL or four; [2] and [3] are recorded behind the two stages.
int launch_pixel_stages(const void *blob, const hawq_jpeg_desc *host_desc, int32_t n_images, const int16_t *coef, uint8_t *planes, uint8_t *out, void *const *events,
                        hipStream_t stream);

// The segment table of a resume call (jpeg_resume.hip) against a host blob the checker of its kind has passed: nullptr, or why not.
const char *resume_refusal(const void *host_blob, int64_t blob_bytes, int progressive, int64_t segs_off, int64_t n_segs);
}  // namespace hawq_jpeg
