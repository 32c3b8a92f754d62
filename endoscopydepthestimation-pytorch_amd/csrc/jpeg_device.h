// Device helpers of libjpeg's decoder arithmetic, shared by the frame reader (jpeg.hip) and the JPEG round trip of the training
// augmentations (augment.hip): jidctint.c inverse DCT, jdmaster.c range limiting, jdsample.c fancy chroma upsampling and jdcolor.c
// YCbCr -> RGB, each bit for bit.
#pragma once

#include "common.h"

namespace endo {

// jidctint.c (jpeg_idct_islow), one dimension.  CONST_BITS = 13, PASS1_BITS = 2.
__device__ __forceinline__ void idct_islow_1d(const int (&v)[8], int (&o)[8], int shift) {
    int z2 = v[2], z3 = v[6];
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 + z3 * (-15137);
    int tmp3 = z1 + z2 * 6270;
    z2 = v[0]; z3 = v[4];
    int tmp0 = (z2 + z3) << 13;
    int tmp1 = (z2 - z3) << 13;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = v[7]; tmp1 = v[5]; tmp2 = v[3]; tmp3 = v[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const int rnd = 1 << (shift - 1);
    o[0] = (tmp10 + tmp3 + rnd) >> shift; o[7] = (tmp10 - tmp3 + rnd) >> shift;
    o[1] = (tmp11 + tmp2 + rnd) >> shift; o[6] = (tmp11 - tmp2 + rnd) >> shift;
    o[2] = (tmp12 + tmp1 + rnd) >> shift; o[5] = (tmp12 - tmp1 + rnd) >> shift;
    o[3] = (tmp13 + tmp0 + rnd) >> shift; o[4] = (tmp13 - tmp0 + rnd) >> shift;
}

// libjpeg's IDCT range-limit table (jdmaster.c prepare_range_limit_table), index masked to 10 bits, centre offset included
__device__ __forceinline__ uint8_t idct_range_limit(int x) {
    const int i = x & 1023;
    return static_cast<uint8_t>(i < 128 ? i + 128 : i < 512 ? 255 : i < 896 ? 0 : i - 896);
}

// jdsample.c: "fancy" (triangle filter) chroma upsampling, evaluated at one full-resolution position
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, int stride, int cw, int ch, int hs, int vs, int yy, int xx) {
    if (hs == 1) return p[static_cast<int64_t>(yy) * stride + xx];          // 4:4:4
    const int cx = xx >> 1, odd = xx & 1;
    if (vs == 1) {          // h2v1_fancy_upsample
        const uint8_t* r = p + static_cast<int64_t>(yy) * stride;
        const int t = r[cx];
        if (!odd) return cx == 0 ? t : (3 * t + r[cx - 1] + 1) >> 2;
        return cx == cw - 1 ? t : (3 * t + r[cx + 1] + 2) >> 2;
    }
    // h2v2_fancy_upsample: 3/4 nearer row + 1/4 further row, then the same horizontally; edges replicate
    const int cy = yy >> 1;
    const int other = (yy & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
    const uint8_t* r0 = p + static_cast<int64_t>(cy) * stride;
    const uint8_t* r1 = p + static_cast<int64_t>(other) * stride;
    const int t = 3 * r0[cx] + r1[cx];
    if (!odd) return cx == 0 ? (t * 4 + 8) >> 4 : (t * 3 + 3 * r0[cx - 1] + r1[cx - 1] + 8) >> 4;
    return cx == cw - 1 ? (t * 4 + 7) >> 4 : (t * 3 + 3 * r0[cx + 1] + r1[cx + 1] + 7) >> 4;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// jdcolor.c ycc_rgb_convert with the tables of build_ycc_rgb_table written out (SCALEBITS 16)
__device__ __forceinline__ void ycc_to_rgb(int y, int cb, int cr, int (&rgb)[3]) {
    const int xb = cb - 128, xr = cr - 128;
    rgb[0] = clamp255(y + ((91881 * xr + 32768) >> 16));
    rgb[1] = clamp255(y + ((-22554 * xb + 32768 - 46802 * xr) >> 16));
    rgb[2] = clamp255(y + ((116130 * xb + 32768) >> 16));
}

}  // namespace endo
