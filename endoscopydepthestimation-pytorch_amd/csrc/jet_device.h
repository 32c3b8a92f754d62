// COLORMAP_JET restated from its piecewise-linear curves, shared by the test-phase depth display (evaluate.hip) and the training /
// validation panels (display.hip).  PARITY UNPINNED against cv2 itself (it is not installed): cv2 interpolates its own table in float32
// and may differ from this on entries within a float32 rounding of .5.
#pragma once

#include <cstdint>

namespace endo {

// entry i of a [256][3] table as B, G, R: x = i / 255, channel = clip(min(4x + a, c - 4x), 0, 1), x 255 rounded half to even (fp64, as the
// numpy restatement tests/evaluate_restate.jet)
__device__ __forceinline__ void jet_fill(uint8_t (*table)[3], int i) {
#pragma clang fp contract(off)
    const double x = static_cast<double>(i) / 255.0;
    const double r = fmin(fmax(fmin(4.0 * x - 1.5, 4.5 - 4.0 * x), 0.0), 1.0);
    const double g = fmin(fmax(fmin(4.0 * x - 0.5, 3.5 - 4.0 * x), 0.0), 1.0);
    const double b = fmin(fmax(fmin(4.0 * x + 0.5, 2.5 - 4.0 * x), 0.0), 1.0);
    table[i][0] = static_cast<uint8_t>(rint(255.0 * b));
    table[i][1] = static_cast<uint8_t>(rint(255.0 * g));
    table[i][2] = static_cast<uint8_t>(rint(255.0 * r));
}

}  // namespace endo
