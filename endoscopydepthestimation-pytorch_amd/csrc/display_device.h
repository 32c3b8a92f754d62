// What display.hip (the training / validation panel) and evaluate_validation.hip (evaluate.py's validation panel) share: the make_grid
// geometry and addressing, and the per-pixel forms of a depth section (0.7-era norm_ip -> COLORMAP_JET index) and of a draw_flow
// section.  Both files are compiled with -ffp-contract=off: every operation below rounds on its own, as numpy and torch evaluate it.
#pragma once

#include <cmath>

#include "common.h"
#include "hsv_device.h"

namespace endo {

constexpr int kDispThreads = 256;
constexpr int kDispBandRows = 8;                // frame rows per reduce block
constexpr int kDispNrow = 8, kDispPad = 2;      // make_grid(nrow = 8, padding = 2)

struct DisplayGeom {
    int n, h, w;
    int xmaps, ymaps, pad;      // make_grid: min(8, N) columns of frames, ceil(N / xmaps) rows, padding (0 when N = 1)
    int gh, gw;                 // one section: (H + 2) ymaps + 2 by (W + 2) xmaps + 2, or H by W when N = 1
    int bands;                  // reduce blocks per frame
};

static inline DisplayGeom display_geom(int n, int h, int w) {
    DisplayGeom g;
    g.n = n; g.h = h; g.w = w;
    g.bands = (h + kDispBandRows - 1) / kDispBandRows;
    if (n == 1) {
        g.xmaps = g.ymaps = 1;
        g.pad = 0;
        g.gh = h;
        g.gw = w;
    } else {
        g.xmaps = n < kDispNrow ? n : kDispNrow;
        g.ymaps = (n + g.xmaps - 1) / g.xmaps;
        g.pad = kDispPad;
        g.gh = (h + kDispPad) * g.ymaps + kDispPad;
        g.gw = (w + kDispPad) * g.xmaps + kDispPad;
    }
    return g;
}

// N, H, W in range and a panel of `sections` stacked grids addressable with 32-bit rows and byte columns
static inline bool display_sizes_in_range(int n, int h, int w, int sections) {
    if (!frames_sizes_ok(n, h, w)) return false;
    const int64_t xmaps = n < kDispNrow ? n : kDispNrow, ymaps = (n + xmaps - 1) / xmaps;
    const int64_t gh = (static_cast<int64_t>(h) + kDispPad) * ymaps + kDispPad, gw = (static_cast<int64_t>(w) + kDispPad) * xmaps + kDispPad;
    return sections * gh <= INT32_MAX && 3 * gw <= INT32_MAX;
}

// draw_flow's y component on the grid: flows_display[..., 1] * h / w with the GRID's height and width (two float32 roundings)
__device__ __forceinline__ float flow_fy(float y, float gh, float gw) { return __fdiv_rn(__fmul_rn(y, gh), gw); }

// np.sqrt(fx * fx + fy * fy) in float32
__device__ __forceinline__ float flow_v(float fx, float fy) { return sqrtf(__fadd_rn(__fmul_rn(fx, fx), __fmul_rn(fy, fy))); }

// the larger of a and b, a NaN kept (np.max propagates it; v >= +0 otherwise)
__device__ __forceinline__ float max_keep_nan(float a, float b) { return (b > a || b != b) ? b : a; }

// grid coordinate -> frame coordinate along one axis: the frame index along the axis and the position inside the frame, -1 on padding
__device__ __forceinline__ int grid_axis(int at, int size, int pad, int& cell) {
    if (pad == 0) { cell = 0; return at; }
    const int t = at - pad;
    if (t < 0) { cell = 0; return -1; }
    cell = t / (size + pad);
    const int inside = t - cell * (size + pad);
    return inside < size ? inside : -1;
}

// norm_ip(img, float(min), float(max))'s divisor: max - min + 1e-5 is a Python float, rounded once to float32
__device__ __forceinline__ float norm_divisor(float lo, float hi) {
    return __double2float_rn(__dadd_rn(__dsub_rn(static_cast<double>(hi), static_cast<double>(lo)), 1.0e-5));
}

// make_grid normalisation (0.7-era norm_ip): clamp, subtract min, divide; then np.uint8(255 x): the COLORMAP_JET index
__device__ __forceinline__ int norm_jet_index(float d, float lo, float hi, float den) {
    const float x = __fdiv_rn(__fsub_rn(fminf(fmaxf(d, lo), hi), lo), den);
    const float v = __fmul_rn(255.0f, x);
    return v > 0.0f ? min(static_cast<int>(v), 255) : 0;
}

// draw_flow for one grid pixel: fx = x, fy = y Hg / Wg, ang = atan2(fy, fx) + pi, v = |(fx, fy)|, H = ang 180 / pi / 2, S = 255,
// V = min(v / max_v, 1) 255 (0 where that is NaN: max_v = 0 and v = 0), cv2.COLOR_HSV2BGR then BGR -> RGB.  The padding is +0 in
// both components.  atan2 in fp64, rounded once: the correctly rounded float32 angle (ocml's atan2f may be an ulp off).
__device__ __forceinline__ void flow_pixel_rgb(float fx, float y, float ghf, float gwf, float vmax, int (&rgb)[3]) {
    const float pi_f = static_cast<float>(M_PI);                       // np.pi added to a float32 array
    const float hue_scale = static_cast<float>(180.0 / M_PI / 2.0);    // 180 / np.pi / 2 multiplied into a float32 array
    const float fy = flow_fy(y, ghf, gwf);
    const float t = __fdiv_rn(flow_v(fx, fy), vmax);
    int val = 0;
    if (t == t) {
        const float s = __fmul_rn(fminf(t, 1.0f), 255.0f);
        val = s > 0.0f ? min(static_cast<int>(s), 255) : 0;
    }
    const float ang = __fadd_rn(__double2float_rn(atan2(static_cast<double>(fy), static_cast<double>(fx))), pi_f);
    const int hue = static_cast<int>(__fmul_rn(ang, hue_scale));
    hsv_to_rgb<180>(hue, 255, val, rgb);          // cv2.COLOR_HSV2BGR, then BGR -> RGB: rgb as it comes
}

}  // namespace endo
