// Training / validation display panels -- reference train.py:353-371 (training) and 460-478 (validation): per pair half
// utils.display_color_depth_sparse_flow_dense_flow and draw_flow, stacked by stack_and_display (utils.py:868-900, 965-994) over
// torchvision 0.7-era make_grid -- for a whole batch on the device; and the validation pass's running means (train.py:446-456).
// tests/display_restate.py is the numpy statement every panel is checked against, bit for bit.
//
// The panel is one uint8 R, G, B image (HWC) of eight sections stacked top to bottom: c1, d1, sf1, df1, c2, d2, sf2, df2, each the
// make_grid(nrow = 8, padding = 2, pad_value = 0) of the batch; N = 1 is the frame itself, no padding (make_grid's squeeze(0)).
// Two launches whatever N:
//   reduce  one block per (band of 8 rows, frame, pair half): the band's min and max of the displayed depth b * d (make_grid's
//           normalize = True, scale_each = True) and its maximum flow magnitude v of the sparse flow (draw_flow's max_v; the grid's
//           padding has v = 0 and never raises it)
//   write   one block per panel row: the partials the row needs, reduced in LDS, then every pixel of the row formed once
// numpy's and torch's float32 arithmetic (and Python's fp64 of the running means) rounds every operation on its own.  The file is compiled
// with -ffp-contract=off (__graft_entry__.py): HIP's __fmul_rn / __fadd_rn / __dmul_rn / __dadd_rn are plain operators that the default
// contraction would fuse into an fma across the inlined calls.  Square roots are sqrtf (correctly rounded; __fsqrt_rn is the native one).
#include <cmath>

#include "common.h"
#include "display_device.h"          // the make_grid geometry and the depth / flow pixel forms, shared with evaluate_validation.hip
#include "jet_device.h"

namespace endo {

constexpr int kDispPartial = 4;                 // floats per partial: depth min, depth max, sparse-flow max v, (unused)

static bool display_sizes_ok(int n, int h, int w) { return display_sizes_in_range(n, h, w, 8); }

static int64_t display_workspace_bytes(int n, int h) {
    const int64_t floats = 2 * static_cast<int64_t>(n) * ((h + kDispBandRows - 1) / kDispBandRows) * kDispPartial;
    return (floats * static_cast<int64_t>(sizeof(float)) + 255) & ~static_cast<int64_t>(255);
}

struct DisplayParams {
    const float* colors_1;  const float* colors_2;      // [N][3][H][W] the masked network input (train.py:272-273)
    const float* depths_1;  const float* depths_2;      // [N][1][H][W] scaled depth; displayed as depth * boundary
    const float* boundaries;                            // [N][1][H][W]
    const float* sparse_1;  const float* sparse_2;      // [N][2][H][W] masked sparse flows (train.py:295-296)
    const float* dense_1;   const float* dense_2;       // [N][2][H][W] masked flows from depth (train.py:297-298)
    DisplayGeom g;
    float* partials;                                    // [2][N][bands][kDispPartial]
    uint8_t* out;                                       // [8 gh][gw][3] R, G, B
};

// trunc(clip(255 (0.5 c + 0.5), 0, 255)): torch's c * 0.5 + 0.5 (two roundings), then tensorboardX's float-image conversion
__device__ __forceinline__ int panel_u8(float c) {
    const float v = __fmul_rn(__fadd_rn(__fmul_rn(c, 0.5f), 0.5f), 255.0f);
    return v > 0.0f ? min(static_cast<int>(v), 255) : 0;
}

__global__ void __launch_bounds__(kDispThreads) display_reduce_kernel(const DisplayParams q) {
    __shared__ float s_red[3][kDispThreads / 64];
    const DisplayGeom g = q.g;
    const int band = blockIdx.x, f = blockIdx.y, half = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t plane = static_cast<int64_t>(g.h) * g.w;
    const float* depth = (half ? q.depths_2 : q.depths_1) + f * plane;
    const float* bnd = q.boundaries + f * plane;
    const float* sx = (half ? q.sparse_2 : q.sparse_1) + 2 * f * plane;
    const float* sy = sx + plane;
    const float gh = static_cast<float>(g.gh), gw = static_cast<float>(g.gw);
    const int r0 = band * kDispBandRows, r1 = min(g.h, r0 + kDispBandRows);
    float lo = INFINITY, hi = -INFINITY, vmax = 0.0f;
    for (int64_t i = static_cast<int64_t>(r0) * g.w + threadIdx.x; i < static_cast<int64_t>(r1) * g.w; i += kDispThreads) {
        const float d = __fmul_rn(depth[i], bnd[i]);          // scaled_depth_maps * boundaries (train.py:356)
        lo = fminf(lo, d);
        hi = fmaxf(hi, d);
        vmax = max_keep_nan(vmax, flow_v(sx[i], flow_fy(sy[i], gh, gw)));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_down(lo, off, 64));
        hi = fmaxf(hi, __shfl_down(hi, off, 64));
        vmax = max_keep_nan(vmax, __shfl_down(vmax, off, 64));
    }
    if (lane == 0) { s_red[0][wave] = lo; s_red[1][wave] = hi; s_red[2][wave] = vmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < kDispThreads / 64; ++i) {
            lo = fminf(lo, s_red[0][i]);
            hi = fmaxf(hi, s_red[1][i]);
            vmax = max_keep_nan(vmax, s_red[2][i]);
        }
        float* p = q.partials + ((static_cast<int64_t>(half) * g.n + f) * g.bands + band) * kDispPartial;
        p[0] = lo;
        p[1] = hi;
        p[2] = vmax;
        p[3] = 0.0f;
    }
}

__global__ void __launch_bounds__(kDispThreads) display_write_kernel(const DisplayParams q) {
    __shared__ uint8_t s_jet[256][3];                                  // B G R
    __shared__ float s_lo[kDispNrow], s_hi[kDispNrow], s_den[kDispNrow];     // the depth range of each frame of this grid row
    __shared__ float s_v[kDispThreads / 64];
    const DisplayGeom g = q.g;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x;
    const int section = row / g.gh;
    const int half = section >> 2, kind = section & 3;                // kind: 0 colour, 1 depth, 2 sparse flow, 3 dense flow
    int gy;
    const int hh = grid_axis(row - section * g.gh, g.h, g.pad, gy);
    const int64_t plane = static_cast<int64_t>(g.h) * g.w;
    float vmax = 0.0f;
    if (kind == 1) {
        jet_fill(s_jet, threadIdx.x);          // COLORMAP_JET (jet_device.h)
        for (int x = wave; x < g.xmaps; x += kDispThreads / 64) {
            const int f = gy * g.xmaps + x;
            if (f >= g.n) break;
            const float* p = q.partials + (static_cast<int64_t>(half) * g.n + f) * g.bands * kDispPartial;
            float lo = INFINITY, hi = -INFINITY;
            for (int b = lane; b < g.bands; b += 64) {
                lo = fminf(lo, p[b * kDispPartial]);
                hi = fmaxf(hi, p[b * kDispPartial + 1]);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                lo = fminf(lo, __shfl_down(lo, off, 64));
                hi = fmaxf(hi, __shfl_down(hi, off, 64));
            }
            if (lane == 0) {
                s_lo[x] = lo;
                s_hi[x] = hi;
                s_den[x] = norm_divisor(lo, hi);          // norm_ip(img, float(t.min()), float(t.max()))
            }
        }
        __syncthreads();
    } else if (kind >= 2) {
        // draw_flow(sparse flows)'s np.max(v) of this pair half, which its dense flows reuse (utils.py:979-980)
        const float* p = q.partials + static_cast<int64_t>(half) * g.n * g.bands * kDispPartial;
        for (int i = threadIdx.x; i < g.n * g.bands; i += kDispThreads) vmax = max_keep_nan(vmax, p[static_cast<int64_t>(i) * kDispPartial + 2]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) vmax = max_keep_nan(vmax, __shfl_down(vmax, off, 64));
        if (lane == 0) s_v[wave] = vmax;
        __syncthreads();
        vmax = s_v[0];
        for (int i = 1; i < kDispThreads / 64; ++i) vmax = max_keep_nan(vmax, s_v[i]);
    }
    const float ghf = static_cast<float>(g.gh), gwf = static_cast<float>(g.gw);
    const float* colors = half ? q.colors_2 : q.colors_1;
    const float* depth = half ? q.depths_2 : q.depths_1;
    const float* flow = kind == 2 ? (half ? q.sparse_2 : q.sparse_1) : (half ? q.dense_2 : q.dense_1);
    uint8_t* dst = q.out + static_cast<int64_t>(row) * g.gw * 3;
    for (int c = threadIdx.x; c < g.gw; c += kDispThreads) {
        int gx;
        const int ww = grid_axis(c, g.w, g.pad, gx);
        const int f = gy * g.xmaps + gx;
        const bool inside = hh >= 0 && ww >= 0 && f < g.n;
        const int64_t at = inside ? static_cast<int64_t>(hh) * g.w + ww : 0;
        int rgb[3] = {0, 0, 0};
        if (kind == 0) {
            if (inside) {
                const float* col = colors + 3 * f * plane + at;
                rgb[0] = panel_u8(col[0]);
                rgb[1] = panel_u8(col[plane]);
                rgb[2] = panel_u8(col[2 * plane]);
            }
        } else if (kind == 1) {
            // make_grid normalisation (0.7-era norm_ip): clamp, subtract min, divide; then np.uint8(255 x), COLORMAP_JET, BGR -> RGB.
            // The padding is 0 before the colormap: JET entry 0.
            int idx = 0;
            if (inside) {
                const float d = __fmul_rn(depth[f * plane + at], q.boundaries[f * plane + at]);
                idx = norm_jet_index(d, s_lo[gx], s_hi[gx], s_den[gx]);
            }
            rgb[0] = s_jet[idx][2];
            rgb[1] = s_jet[idx][1];
            rgb[2] = s_jet[idx][0];
        } else {
            // draw_flow (flow_pixel_rgb); the padding is +0 in both components
            float fx = 0.0f, y = 0.0f;
            if (inside) {
                fx = flow[2 * f * plane + at];
                y = flow[(2 * f + 1) * plane + at];
            }
            flow_pixel_rgb(fx, y, ghf, gwf, vmax, rgb);
        }
        dst[3 * c] = static_cast<uint8_t>(rgb[0]);
        dst[3 * c + 1] = static_cast<uint8_t>(rgb[1]);
        dst[3 * c + 2] = static_cast<uint8_t>(rgb[2]);
    }
}

// train.py:446-456 on the device, fp64 with the Python float's roundings: a NaN total leaves the means as they are; otherwise batch 0
// takes the losses and batch k > 0 forms (mean k + loss) / (k + 1.0).  history (or null): row `batch` gets the means after the update.
__global__ void validation_accumulate_kernel(const float* __restrict__ losses, int batch, double* __restrict__ means,
                                             double* __restrict__ history) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double total = static_cast<double>(losses[0]);
    if (!isnan(total)) {
        const double k = static_cast<double>(batch);
        for (int i = 0; i < 3; ++i) {
            const double loss = static_cast<double>(losses[i]);          // loss.item() of a float32 tensor
            means[i] = batch == 0 ? loss : __ddiv_rn(__dadd_rn(__dmul_rn(means[i], k), loss), __dadd_rn(k, 1.0));
        }
    }
    if (history) {
        for (int i = 0; i < 3; ++i) history[3 * static_cast<int64_t>(batch) + i] = means[i];
    }
}

}  // namespace endo

using namespace endo;

extern "C" int64_t endo_display_workspace_bytes(int n, int h, int w) {
    if (!display_sizes_ok(n, h, w)) return -1;
    return display_workspace_bytes(n, h);
}

extern "C" int endo_display_panel_shape(int n, int h, int w, int* rows, int* cols) {
    if (!rows || !cols || !display_sizes_ok(n, h, w)) return ENDO_E_BADARG;
    const DisplayGeom g = display_geom(n, h, w);
    *rows = 8 * g.gh;
    *cols = g.gw;
    return 0;
}

extern "C" int endo_display(const float* colors_1, const float* colors_2, const float* depths_1, const float* depths_2, const float* boundaries,
                            const float* sparse_flows_1, const float* sparse_flows_2, const float* flows_1, const float* flows_2, int n, int h,
                            int w, uint8_t* out, void* workspace, int64_t workspace_bytes, void* stream_) {
    if (!colors_1 || !colors_2 || !depths_1 || !depths_2 || !boundaries || !sparse_flows_1 || !sparse_flows_2 || !flows_1 || !flows_2 || !out ||
        !workspace)
        return ENDO_E_BADARG;
    if (!display_sizes_ok(n, h, w) || workspace_bytes < display_workspace_bytes(n, h)) return ENDO_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const DisplayGeom g = display_geom(n, h, w);
    const DisplayParams q{colors_1, colors_2, depths_1, depths_2, boundaries, sparse_flows_1, sparse_flows_2, flows_1, flows_2, g,
                          static_cast<float*>(workspace), out};
    const double pixels = static_cast<double>(n) * h * w;
    // reads per pixel and pair half: 13 floats (reduce: depth, boundary, sparse flow; write: colours, depth, boundary, both flows); writes: the panel
    ProfScope prof(kProfSmall, stream, 0.0, 2.0 * pixels * 4.0 * (2 * 4 + 3 + 2) + 8.0 * g.gh * static_cast<double>(g.gw) * 3.0);
    display_reduce_kernel<<<dim3(g.bands, n, 2), kDispThreads, 0, stream>>>(q);
    ENDO_LAUNCH_CHECK();
    display_write_kernel<<<dim3(8 * g.gh), kDispThreads, 0, stream>>>(q);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_validation_accumulate(const float* losses, int batch_index, double* means, double* history, void* stream_) {
    if (!losses || !means || batch_index < 0) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    validation_accumulate_kernel<<<1, 64, 0, stream>>>(losses, batch_index, means, history);
    ENDO_LAUNCH_CHECK();
    return 0;
}
