// Stages 2 and 3 of hawq_jpeg_decode_batch as functions of one block / one pixel, for the device (jpeg_decode.hip) and the host
// (tools/jpeg_host_check.cpp): dequantisation + the 8x8 ISLOW inverse DCT of jidctint.c, and fancy (triangle) chroma upsampling +
// YCbCr -> RGB of jdsample.c / jdcolor.c, in the integers those files use.  Behind them the same two stages at the reduced sizes of
// the library's DCT-domain scaling: the 4x4, 2x2 and 1x1 inverse DCTs of jidctred.c and the pixel of a scaled image.
#pragma once
#include "jpeg_entropy.h"

// natural index -> zig-zag index (the quantisation table is kept as DQT stores it)
HAWQ_HD int jpeg_zigzag_of(int n) {
    const uint8_t zz[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                            41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                            46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
    return zz[n & 63];
}

// the library's range_limit table behind the +128 level shift, on a 10-bit index
HAWQ_HD uint8_t jpeg_range_limit(int32_t x) {
    x &= 0x3FF;
    return (uint8_t)(x < 128 ? x + 128 : x < 512 ? 255 : x < 896 ? 0 : x - 896);
}

// One-dimensional pass of jpeg_idct_islow on eight inputs; sums wrap in 32 bits (exact for every stream an encoder writes: the
// library's INT32 design), the descale is an arithmetic shift with rounding.
HAWQ_HD void jpeg_idct_1d(const int32_t *in, int32_t *out, int shift) {
    typedef uint32_t u;
    const u c298 = 2446, c390 = 3196, c541 = 4433, c765 = 6270, c899 = 7373, c1175 = 9633, c1501 = 12299, c1847 = 15137, c1961 = 16069, c2053 = 16819,
            c2562 = 20995, c3072 = 25172;
    u z2 = (u)in[2], z3 = (u)in[6];
    u z1 = (z2 + z3) * c541;
    u tmp2 = z1 - z3 * c1847;
    u tmp3 = z1 + z2 * c765;
    z2 = (u)in[0], z3 = (u)in[4];
    u tmp0 = (z2 + z3) << 13, tmp1 = (z2 - z3) << 13;
    const u tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = (u)in[7], tmp1 = (u)in[5], tmp2 = (u)in[3], tmp3 = (u)in[1];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    u z4 = tmp1 + tmp3;
    const u z5 = (z3 + z4) * c1175;
    tmp0 *= c298, tmp1 *= c2053, tmp2 *= c3072, tmp3 *= c1501;
    z1 *= 0u - c899, z2 *= 0u - c2562, z3 *= 0u - c1961, z4 *= 0u - c390;
    z3 += z5, z4 += z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    const u half = 1u << (shift - 1);
    out[0] = (int32_t)(tmp10 + tmp3 + half) >> shift;
    out[7] = (int32_t)(tmp10 - tmp3 + half) >> shift;
    out[1] = (int32_t)(tmp11 + tmp2 + half) >> shift;
    out[6] = (int32_t)(tmp11 - tmp2 + half) >> shift;
    out[2] = (int32_t)(tmp12 + tmp1 + half) >> shift;
    out[5] = (int32_t)(tmp12 - tmp1 + half) >> shift;
    out[3] = (int32_t)(tmp13 + tmp0 + half) >> shift;
    out[4] = (int32_t)(tmp13 - tmp0 + half) >> shift;
}

// CONST_BITS = 13, PASS1_BITS = 2: columns descale by 11 into the workspace, rows by 18.
// Column x of a block: coef [64] natural order, qt [64] zig-zag order -> ws[y * 8 + x], y < 8.
HAWQ_HD void jpeg_idct_column(const int16_t *coef, const uint16_t *qt, int x, int32_t *ws) {
    int32_t in[8], col[8];
    HAWQ_UNROLL
    for (int y = 0; y < 8; ++y) in[y] = (int32_t)coef[y * 8 + x] * (int32_t)qt[jpeg_zigzag_of(y * 8 + x)];
    jpeg_idct_1d(in, col, 11);
    HAWQ_UNROLL
    for (int y = 0; y < 8; ++y) ws[y * 8 + x] = col[y];
}

// Row y of the workspace -> the row's 8 samples
HAWQ_HD void jpeg_idct_row(const int32_t *ws, int y, uint8_t *out) {
    int32_t in[8], row[8];
    HAWQ_UNROLL
    for (int x = 0; x < 8; ++x) in[x] = ws[y * 8 + x];
    jpeg_idct_1d(in, row, 18);
    HAWQ_UNROLL
    for (int x = 0; x < 8; ++x) out[x] = jpeg_range_limit(row[x]);
}

// A whole block in one thread (the host's form; the kernel gives a block's columns, then rows, to eight lanes): 8 rows of 8 samples at
// out, rows `pitch` bytes apart.
HAWQ_HD void jpeg_idct_block(const int16_t *coef, const uint16_t *qt, uint8_t *out, int64_t pitch) {
    int32_t ws[64];
    for (int x = 0; x < 8; ++x) jpeg_idct_column(coef, qt, x, ws);
    for (int y = 0; y < 8; ++y) jpeg_idct_row(ws, y, out + y * pitch);
}

HAWQ_HD int32_t jpeg_clampi(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// The chroma sample the library's fancy upsampling gives output pixel (x, y).  p: the component's plane, `pitch` bytes a row, of which
// cw x ch samples are real; neighbours past an edge repeat the last real row / column.
HAWQ_HD int32_t jpeg_upsample(const uint8_t *p, int64_t pitch, int32_t cw, int32_t ch, int hs, int vs, int32_t x, int32_t y) {
    if (hs == 1) return p[(int64_t)y * pitch + x];
    const int32_t i = x >> 1, ia = jpeg_clampi((x & 1) ? i + 1 : i - 1, 0, cw - 1);   // near and far column
    if (vs == 1) {   // h2v1: (3 near + far + 1 or 2) >> 2
        const uint8_t *r = p + (int64_t)y * pitch;
        return (3 * r[i] + r[ia] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int32_t j = y >> 1, ja = jpeg_clampi((y & 1) ? j + 1 : j - 1, 0, ch - 1);
    const uint8_t *rn = p + (int64_t)j * pitch, *rf = p + (int64_t)ja * pitch;
    const int32_t t = 3 * rn[i] + rf[i], ta = 3 * rn[ia] + rf[ia];
    return (3 * t + ta + ((x & 1) ? 7 : 8)) >> 4;
}

// RGB of output pixel (x, y) of image d, whose sample planes start at `planes` (d.plane_off applied by the caller)
HAWQ_HD void jpeg_pixel(const hawq_jpeg_desc &d, const uint8_t *planes, int32_t x, int32_t y, uint8_t *rgb) {
    const int64_t ypitch = (int64_t)d.mcus_x * d.hs * 8, cpitch = (int64_t)d.mcus_x * 8;
    const int32_t Y = planes[(int64_t)y * ypitch + x];
    if (d.ncomp == 1) {
        rgb[0] = rgb[1] = rgb[2] = (uint8_t)Y;
        return;
    }
    const int64_t ysize = ypitch * d.mcus_y * d.vs * 8, csize = cpitch * d.mcus_y * 8;
    const int32_t cw = (d.width + d.hs - 1) / d.hs, ch = (d.height + d.vs - 1) / d.vs;
    const int32_t cb = jpeg_upsample(planes + ysize, cpitch, cw, ch, d.hs, d.vs, x, y) - 128;
    const int32_t cr = jpeg_upsample(planes + ysize + csize, cpitch, cw, ch, d.hs, d.vs, x, y) - 128;
    rgb[0] = (uint8_t)jpeg_clampi(Y + ((91881 * cr + 32768) >> 16), 0, 255);
    rgb[1] = (uint8_t)jpeg_clampi(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255);
    rgb[2] = (uint8_t)jpeg_clampi(Y + ((116130 * cb + 32768) >> 16), 0, 255);
}

// ---- reduced-size decoding (desc.scale = 2, 4, 8) -----------------------------------------------------------------
HAWQ_HD int jpeg_scale(const hawq_jpeg_desc &d) { return d.scale > 1 ? d.scale : 1; }

// Samples per block side of component c (jdmaster.c): 8 / scale, doubled for the chroma of a 4:2:0 image, whose plane then has the
// output size.  8 at full size.
HAWQ_HD int jpeg_comp_n(const hawq_jpeg_desc &d, int c) {
    const int m = 8 / jpeg_scale(d);
    return (c > 0 && d.hs == 2 && d.vs == 2 && m < 8) ? 2 * m : m;
}

HAWQ_HD int32_t jpeg_out_width(const hawq_jpeg_desc &d) { return (d.width + jpeg_scale(d) - 1) / jpeg_scale(d); }
HAWQ_HD int32_t jpeg_out_height(const hawq_jpeg_desc &d) { return (d.height + jpeg_scale(d) - 1) / jpeg_scale(d); }

// One-dimensional passes of jpeg_idct_4x4 / jpeg_idct_2x2 on the eight inputs of a column or workspace row (in[4], and in[2] / in[6]
// of the 2x2, are not read); sums wrap in 32 bits as above.
HAWQ_HD void jpeg_idct_1d_4(const int32_t *in, int32_t *out, int shift) {
    typedef uint32_t u;
    const u tmp0 = (u)in[0] << 14, tmp2 = (u)in[2] * 15137u - (u)in[6] * 6270u;
    const u tmp10 = tmp0 + tmp2, tmp12 = tmp0 - tmp2;
    const u t0 = (u)in[1] * 8697u - (u)in[3] * 17799u + (u)in[5] * 11893u - (u)in[7] * 1730u;
    const u t2 = (u)in[1] * 20995u + (u)in[3] * 7373u - (u)in[5] * 4926u - (u)in[7] * 4176u;
    const u half = 1u << (shift - 1);
    out[0] = (int32_t)(tmp10 + t2 + half) >> shift;
    out[3] = (int32_t)(tmp10 - t2 + half) >> shift;
    out[1] = (int32_t)(tmp12 + t0 + half) >> shift;
    out[2] = (int32_t)(tmp12 - t0 + half) >> shift;
}

HAWQ_HD void jpeg_idct_1d_2(const int32_t *in, int32_t *out, int shift) {
    typedef uint32_t u;
    const u tmp10 = (u)in[0] << 15;
    const u t0 = (u)in[1] * 29692u - (u)in[3] * 10426u + (u)in[5] * 6967u - (u)in[7] * 5906u;
    const u half = 1u << (shift - 1);
    out[0] = (int32_t)(tmp10 + t0 + half) >> shift;
    out[1] = (int32_t)(tmp10 - t0 + half) >> shift;
}

// does the row pass of the n x n inverse DCT read workspace column x?
HAWQ_HD bool jpeg_idct_reads_column(int n, int x) { return n == 8 || (n == 4 && x != 4) || (n == 2 && (x == 0 || (x & 1))) || x == 0; }

// Column x of a block for the n x n inverse DCT, n = 1, 2, 4, 8 -> ws[y * 8 + x], y < n (n = 1: the dequantised DC alone).  Columns
// the row pass does not read are left alone.
HAWQ_HD void jpeg_idct_column_n(const int16_t *coef, const uint16_t *qt, int n, int x, int32_t *ws) {
    if (n == 8) return jpeg_idct_column(coef, qt, x, ws);
    if (!jpeg_idct_reads_column(n, x)) return;
    int32_t in[8], col[4];
    HAWQ_UNROLL
    for (int y = 0; y < 8; ++y) in[y] = (int32_t)coef[y * 8 + x] * (int32_t)qt[jpeg_zigzag_of(y * 8 + x)];
    if (n == 4) {
        jpeg_idct_1d_4(in, col, 12);
        HAWQ_UNROLL
        for (int y = 0; y < 4; ++y) ws[y * 8 + x] = col[y];
    } else if (n == 2) {
        jpeg_idct_1d_2(in, col, 13);
        ws[x] = col[0], ws[8 + x] = col[1];
    } else {
        ws[0] = in[0];
    }
}

// Row y < n of that workspace -> the row's n samples
HAWQ_HD void jpeg_idct_row_n(const int32_t *ws, int n, int y, uint8_t *out) {
    if (n == 8) return jpeg_idct_row(ws, y, out);
    int32_t in[8], row[4];
    HAWQ_UNROLL
    for (int x = 0; x < 8; ++x) in[x] = jpeg_idct_reads_column(n, x) ? ws[y * 8 + x] : 0;
    if (n == 4) {
        jpeg_idct_1d_4(in, row, 19);
        HAWQ_UNROLL
        for (int x = 0; x < 4; ++x) out[x] = jpeg_range_limit(row[x]);
    } else if (n == 2) {
        jpeg_idct_1d_2(in, row, 20);
        out[0] = jpeg_range_limit(row[0]), out[1] = jpeg_range_limit(row[1]);
    } else {
        out[0] = jpeg_range_limit((int32_t)((uint32_t)in[0] + 4u) >> 3);
    }
}

// A whole block in one thread: n rows of n samples at out, rows `pitch` bytes apart
HAWQ_HD void jpeg_idct_block_n(const int16_t *coef, const uint16_t *qt, int n, uint8_t *out, int64_t pitch) {
    int32_t ws[64];
    for (int x = 0; x < 8; ++x) jpeg_idct_column_n(coef, qt, n, x, ws);
    for (int y = 0; y < n; ++y) jpeg_idct_row_n(ws, n, y, out + y * pitch);
}

// RGB of pixel (x, y) of the reduced image of d (scale 2, 4 or 8), x < jpeg_out_width, y < jpeg_out_height.  The planes lie component
// after component, each (block rows * n) rows of pitch (block columns * n) with n = jpeg_comp_n.  The chroma planes of 4:4:4 and 4:2:0
// have the output size; those of 4:2:2 are h2v1: the fancy filter above over the real samples when 8 / scale > 1 and more than two of
// them stand in a row, else output x takes sample x >> 1 (jdsample.c).
HAWQ_HD void jpeg_pixel_scaled(const hawq_jpeg_desc &d, const uint8_t *planes, int32_t x, int32_t y, uint8_t *rgb) {
    const int n0 = jpeg_comp_n(d, 0), nc = jpeg_comp_n(d, 1);
    const int64_t ypitch = (int64_t)d.mcus_x * d.hs * n0, cpitch = (int64_t)d.mcus_x * nc;
    const int32_t Y = planes[(int64_t)y * ypitch + x];
    if (d.ncomp == 1) {
        rgb[0] = rgb[1] = rgb[2] = (uint8_t)Y;
        return;
    }
    const int64_t ysize = ypitch * d.mcus_y * d.vs * n0, csize = cpitch * d.mcus_y * nc;
    const uint8_t *pb = planes + ysize + (int64_t)y * cpitch, *pr = pb + csize;
    int32_t cb, cr;
    if (d.hs == 2 && d.vs == 1) {
        const int32_t cw = (d.width * nc + 15) / 16;   // real samples of a chroma row
        const int32_t i = x >> 1;
        if (nc > 1 && cw > 2) {
            const int32_t ia = jpeg_clampi((x & 1) ? i + 1 : i - 1, 0, cw - 1), r = (x & 1) ? 2 : 1;
            cb = (3 * pb[i] + pb[ia] + r) >> 2, cr = (3 * pr[i] + pr[ia] + r) >> 2;
        } else {
            cb = pb[i], cr = pr[i];
        }
    } else {
        cb = pb[x], cr = pr[x];
    }
    cb -= 128, cr -= 128;
    rgb[0] = (uint8_t)jpeg_clampi(Y + ((91881 * cr + 32768) >> 16), 0, 255);
    rgb[1] = (uint8_t)jpeg_clampi(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255);
    rgb[2] = (uint8_t)jpeg_clampi(Y + ((116130 * cb + 32768) >> 16), 0, 255);
}
