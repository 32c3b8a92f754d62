// OpenCV's 8-bit HSV -> RGB (color_hsv: HSV2RGB_b -> HSV2RGB_native), shared by the training augmentations (augment.hip, hue range 180:
// cv2.COLOR_HSV2RGB) and the test-phase colour display (evaluate.hip, hue range 256: cv2.COLOR_HSV2BGR_FULL).
#pragma once

#include "jpeg_device.h"

namespace endo {

// hscale = 6 / HRANGE; s = S / 255, v = V / 255, h = fmod(H * hscale, 6), the six-sector table, out = cvRound(x * 255): every operation
// a separate float rounding.  rgb = {r, g, b}; cv2's BGR orders take them in reverse.
template <int HRANGE>
__device__ __forceinline__ void hsv_to_rgb(int hh, int ss, int vv, int (&rgb)[3]) {
#pragma clang fp contract(off)
    const float s = static_cast<float>(ss) * (1.0f / 255.0f);
    const float v = static_cast<float>(vv) * (1.0f / 255.0f);
    float r, g, b;
    if (s == 0.0f) {
        r = g = b = v;
    } else {
        float h = static_cast<float>(hh) * (6.0f / static_cast<float>(HRANGE));
        h = fmodf(h, 6.0f);
        int sector = static_cast<int>(floorf(h));
        h -= static_cast<float>(sector);
        if (static_cast<unsigned>(sector) >= 6u) { sector = 0; h = 0.0f; }
        const float t1 = v * (1.0f - s), t2 = v * (1.0f - s * h), t3 = v * (1.0f - s * (1.0f - h));
        // sector_data {b, g, r} = {1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0} over tab = {v, t1, t2, t3}, one nibble per sector
        const int shift = 4 * (5 - sector);
        const int bi = (0x113002 >> shift) & 15, gi = (0x300211 >> shift) & 15, ri = (0x021130 >> shift) & 15;
        b = bi == 0 ? v : (bi == 1 ? t1 : (bi == 2 ? t2 : t3));
        g = gi == 0 ? v : (gi == 1 ? t1 : (gi == 2 ? t2 : t3));
        r = ri == 0 ? v : (ri == 1 ? t1 : (ri == 2 ? t2 : t3));
    }
    rgb[0] = clamp255(static_cast<int>(rintf(r * 255.0f)));
    rgb[1] = clamp255(static_cast<int>(rintf(g * 255.0f)));
    rgb[2] = clamp255(static_cast<int>(rintf(b * 255.0f)));
}

}  // namespace endo
