// The validation phase of evaluate.py (reference evaluate.py:201-274) for a whole batch on the device: the 12-section panel of
// utils.display_color_sparse_depth_dense_depth_warped_depth_sparse_flow_dense_flow (twice) and stack_and_display (utils.py:894-954), the
// point clouds of utils.point_cloud_from_depth for frame 1 of every pair, and the error measures the reference defines for this
// comparison and never calls: AbsRelError and Threshold (losses.py:189-227).  tests/evaluate_validation_restate.py is the numpy statement
// the panel and the measures are checked against; the point rows are endo_point_cloud's, bit for bit.
//
// The panel is one uint8 R, G, B image (HWC) of twelve sections stacked top to bottom: c1 sd1 d1 wd1 sf1 df1 c2 sd2 d2 wd2 sf2 df2, each
// the make_grid(nrow = 8, padding = 2, pad_value = 0) of the batch (display_device.h).  Against display.hip's panel: the depth sections
// share ONE (min, max) per pair half, taken over the whole batch of scaled_depth * boundaries (utils.py:921-922) and applied, clamped,
// to the sparse and the warped depths as well; draw_flow runs on the DENSE flows first and its max_v scales the sparse flows
// (utils.py:942-943); the colour section is (0.5 c + 0.5) * boundaries.
//
// Three launches whatever N, no atomics, no memset:
//   reduce  one block per (band of 8 rows, pair, half): the band's min and max of b * d, its maximum dense-flow magnitude and (half 0)
//           its count of point-cloud pixels
//   scan    one block: exclusive prefix of the N * bands point counts (pair-major), the pairs' offsets, each half's range and max_v
//   write   one block per panel row, one per (band, pair) for the point rows, ordered inside a row by cloud_device.h's rank, and one per
//           (pair, half) that runs depth_metrics_block, the device function that is endo_depth_metrics' whole kernel, so the two
//           entries return the same bits (three IEEE divisions per pixel make a sample one compute unit's arithmetic, about as long
//           as the panel rows take beside it)
// Compiled with -ffp-contract=off, as display.hip is and for its reason: every operation rounds on its own.
#include <algorithm>
#include <cmath>

#include "cloud_device.h"
#include "common.h"
#include "display_device.h"
#include "jet_device.h"

namespace endo {

constexpr int kValSections = 12;
constexpr int kValPartial = 4;          // floats per band partial: depth min, depth max, dense-flow max v, (unused)
constexpr int kValFinal = 4;            // floats per pair half after the scan: depth min, depth max, norm_ip's divisor, max_v
static_assert(kDispThreads == kCloudThreads, "the reduce and write blocks use cloud_device.h's 256-thread helpers");

// ---------------------------------------------------------------------------------------------
// AbsRelError and Threshold of one sample -- losses.py:194-227 -- by one block of 256 threads.  Per-pixel terms with torch's float32
// operations (IEEE division; eps is the Python float added into a float32 tensor):
//   abs rel     (m |d - s|) / (eps + s)
//   threshold   m max(d m / (eps + s), s / (eps + d m)) + (1 - m) 10, a NaN side kept as torch.max keeps it; 0 * inf = NaN compares false
// The abs-rel terms and the mask are summed in fp64 and rounded once to float32; the three counts are integers.  out[4] = abs rel,
// sigma 1, 2, 3: float32 quotients by the mask sum (an empty mask: 0 / 0 = NaN in all four, as the reference's).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float max_torch(float a, float b) { return (a != a || b != b) ? NAN : fmaxf(a, b); }

struct MetricSums {
    double rel, mask;
    int c1, c2, c3;
};

__device__ __forceinline__ void metric_terms(float d, float s, float m, float eps, MetricSums& a) {
    const float t2 = static_cast<float>(1.25 * 1.25), t3 = static_cast<float>(1.25 * 1.25 * 1.25);          // exact in float32
    const float es = __fadd_rn(eps, s);
    a.rel += static_cast<double>(__fdiv_rn(__fmul_rn(m, fabsf(__fsub_rn(d, s))), es));
    a.mask += static_cast<double>(m);
    const float dm = __fmul_rn(d, m);
    const float ratio = max_torch(__fdiv_rn(dm, es), __fdiv_rn(s, __fadd_rn(eps, dm)));
    const float t = __fadd_rn(__fmul_rn(m, ratio), __fmul_rn(__fsub_rn(1.0f, m), 10.0f));
    a.c1 += t < 1.25f ? 1 : 0;
    a.c2 += t < t2 ? 1 : 0;
    a.c3 += t < t3 ? 1 : 0;
}

__device__ void depth_metrics_block(const float* __restrict__ depth, const float* __restrict__ sparse, const float* __restrict__ mask,
                                    int64_t pixels, float eps, float* __restrict__ out) {
    __shared__ double s_sum[2][kDispThreads / 64];
    __shared__ int s_cnt[3][kDispThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    MetricSums a{0.0, 0.0, 0, 0, 0};
#pragma unroll 4
    for (int64_t i = threadIdx.x; i < pixels; i += kDispThreads) metric_terms(depth[i], sparse[i], mask[i], eps, a);
    double rel = a.rel, msum = a.mask;
    int c1 = a.c1, c2 = a.c2, c3 = a.c3;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        rel += __shfl_down(rel, off, 64);
        msum += __shfl_down(msum, off, 64);
        c1 += __shfl_down(c1, off, 64);
        c2 += __shfl_down(c2, off, 64);
        c3 += __shfl_down(c3, off, 64);
    }
    if (lane == 0) { s_sum[0][wave] = rel; s_sum[1][wave] = msum; s_cnt[0][wave] = c1; s_cnt[1][wave] = c2; s_cnt[2][wave] = c3; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < kDispThreads / 64; ++i) {
            rel += s_sum[0][i]; msum += s_sum[1][i];
            c1 += s_cnt[0][i]; c2 += s_cnt[1][i]; c3 += s_cnt[2][i];
        }
        const float den = __double2float_rn(msum);
        out[0] = __fdiv_rn(__double2float_rn(rel), den);
        out[1] = __fdiv_rn(static_cast<float>(c1), den);
        out[2] = __fdiv_rn(static_cast<float>(c2), den);
        out[3] = __fdiv_rn(static_cast<float>(c3), den);
    }
}

__global__ void __launch_bounds__(kDispThreads) depth_metrics_kernel(const float* __restrict__ depth, const float* __restrict__ sparse,
                                                                     const float* __restrict__ mask, int64_t pixels, float eps,
                                                                     float* __restrict__ out) {
    const int64_t f = blockIdx.x;
    depth_metrics_block(depth + f * pixels, sparse + f * pixels, mask + f * pixels, pixels, eps, out + 4 * f);
}

// ---------------------------------------------------------------------------------------------
struct ValParams {
    const float* colors[2];          // [N][3][H][W] masked colours (evaluate.py:189-190)
    const float* boundaries;         // [N][1][H][W]
    const float* depths[2];          // [N][1][H][W] scaled depths, unmasked (evaluate.py:196-199)
    const float* sparse_depths[2];   // [N][1][H][W]
    const float* sparse_masks[2];    // [N][1][H][W]
    const float* warped[2];          // [N][1][H][W] warped depths 2 -> 1 and 1 -> 2 (evaluate.py:218-223)
    const float* sparse_flows[2];    // [N][2][H][W] masked sparse flows (evaluate.py:191-192)
    const float* flows[2];           // [N][2][H][W] masked flows from depth (evaluate.py:215-216)
    const float* k;                  // [N][3][3]
    DisplayGeom g;
    float eps;
    int downsampling;
    uint8_t* panel;                  // [12 gh][gw][3] R, G, B
    float* metrics;                  // [N][2][4]
    float* points;                   // [N H W][6]
    int64_t* offsets;                // [N + 1]
    float* partials;                 // workspace [2][N][bands][kValPartial]
    int64_t* band_offsets;           // workspace [N][bands]: counts after `reduce`, exclusive offsets after `scan`
    float* finals;                   // workspace [2][kValFinal]
};

// trunc(clip(255 ((0.5 c + 0.5) b))): utils.py:912, then the writer's (and evaluate.py:270's) float-image conversion
__device__ __forceinline__ int val_color_u8(float c, float b) {
    const float v = __fmul_rn(__fmul_rn(__fadd_rn(__fmul_rn(c, 0.5f), 0.5f), b), 255.0f);
    return v > 0.0f ? min(static_cast<int>(v), 255) : 0;
}

__global__ void __launch_bounds__(kDispThreads) val_reduce_kernel(const ValParams q) {
    __shared__ float s_red[3][kDispThreads / 64];
    __shared__ int s_keep[kDispThreads / 64];
    const DisplayGeom g = q.g;
    const int band = blockIdx.x, f = blockIdx.y, half = blockIdx.z;
    const int64_t plane = static_cast<int64_t>(g.h) * g.w;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* depth = q.depths[half] + f * plane;
    const float* bnd = q.boundaries + f * plane;
    const float* dx = q.flows[half] + 2 * f * plane;
    const float* dy = dx + plane;
    const float gh = static_cast<float>(g.gh), gw = static_cast<float>(g.gw);
    const int r0 = band * kDispBandRows, r1 = min(g.h, r0 + kDispBandRows);
    float lo = INFINITY, hi = -INFINITY, vmax = 0.0f;
    int keep = 0;
    for (int r = r0; r < r1; ++r) {
        const int64_t base = static_cast<int64_t>(r) * g.w;
        for (int w = threadIdx.x; w < g.w; w += kDispThreads) {
            const float b = bnd[base + w];
            const float d = __fmul_rn(depth[base + w], b);          // scaled_depth_maps * boundaries (evaluate.py:230)
            lo = fminf(lo, d);
            hi = fmaxf(hi, d);
            vmax = max_keep_nan(vmax, flow_v(dx[base + w], flow_fy(dy[base + w], gh, gw)));
            keep += cloud_pixel_keep(q.downsampling, r, w, b) ? 1 : 0;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_down(lo, off, 64));
        hi = fmaxf(hi, __shfl_down(hi, off, 64));
        vmax = max_keep_nan(vmax, __shfl_down(vmax, off, 64));
        keep += __shfl_down(keep, off, 64);
    }
    if (lane == 0) { s_red[0][wave] = lo; s_red[1][wave] = hi; s_red[2][wave] = vmax; s_keep[wave] = keep; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < kDispThreads / 64; ++i) {
            lo = fminf(lo, s_red[0][i]);
            hi = fmaxf(hi, s_red[1][i]);
            vmax = max_keep_nan(vmax, s_red[2][i]);
            keep += s_keep[i];
        }
        const int64_t at = static_cast<int64_t>(f) * g.bands + band;
        float* p = q.partials + (static_cast<int64_t>(half) * g.n * g.bands + at) * kValPartial;
        p[0] = lo;
        p[1] = hi;
        p[2] = vmax;
        p[3] = 0.0f;
        if (half == 0) q.band_offsets[at] = keep;
    }
}

// the bands' offsets and the pairs' (cloud_scan_block, on the pair-major list), then each half's range and max_v
__global__ void __launch_bounds__(kScanThreads) val_scan_kernel(const ValParams q) {
    __shared__ float s_red[3][kScanThreads / 64];
    const DisplayGeom g = q.g;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t items = static_cast<int64_t>(g.n) * g.bands;
    cloud_scan_block(q.band_offsets, g.n, g.bands, q.offsets);
    // torch.min / torch.max of the half's b * d over the whole batch, and draw_flow(dense flows)'s np.max(v)
    for (int half = 0; half < 2; ++half) {
        const float* p = q.partials + static_cast<int64_t>(half) * items * kValPartial;
        float lo = INFINITY, hi = -INFINITY, vmax = 0.0f;
        for (int64_t i = t; i < items; i += kScanThreads) {
            lo = fminf(lo, p[i * kValPartial]);
            hi = fmaxf(hi, p[i * kValPartial + 1]);
            vmax = max_keep_nan(vmax, p[i * kValPartial + 2]);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo = fminf(lo, __shfl_down(lo, off, 64));
            hi = fmaxf(hi, __shfl_down(hi, off, 64));
            vmax = max_keep_nan(vmax, __shfl_down(vmax, off, 64));
        }
        __syncthreads();          // s_red is free again
        if (lane == 0) { s_red[0][wave] = lo; s_red[1][wave] = hi; s_red[2][wave] = vmax; }
        __syncthreads();
        if (t == 0) {
            for (int i = 1; i < kScanThreads / 64; ++i) {
                lo = fminf(lo, s_red[0][i]);
                hi = fmaxf(hi, s_red[1][i]);
                vmax = max_keep_nan(vmax, s_red[2][i]);
            }
            float* out = q.finals + half * kValFinal;
            out[0] = lo;
            out[1] = hi;
            out[2] = norm_divisor(lo, hi);          // make_grid(range = (min.item(), max.item()))
            out[3] = vmax;
        }
    }
}

// the point rows of one band of frame 1 of pair f, rows in order (cloud_device.h's pieces, on the unmasked scaled depth; the colours
// are display_u8's, as the test phase takes them)
__device__ void val_cloud_band(const ValParams& q, int f, int band) {
    const DisplayGeom g = q.g;
    int64_t at = q.band_offsets[static_cast<int64_t>(f) * g.bands + band];          // where this chunk's points start
    const float* kf = q.k + static_cast<int64_t>(f) * 9;
    const float fx = kf[0], cx = kf[2], fy = kf[4], cy = kf[5];
    const int64_t plane = static_cast<int64_t>(g.h) * g.w;
    const int r0 = band * kDispBandRows, r1 = min(g.h, r0 + kDispBandRows);
    for (int h = r0; h < r1; ++h) {
        if (h % q.downsampling != 0) continue;
        const int64_t pix0 = static_cast<int64_t>(f) * plane + static_cast<int64_t>(h) * g.w;
        const float* col = q.colors[0] + static_cast<int64_t>(f) * 3 * plane + static_cast<int64_t>(h) * g.w;
        for (int w0 = 0; w0 < g.w; w0 += kDispThreads) {
            const int w = w0 + threadIdx.x;
            const bool keep = w < g.w && cloud_pixel_keep(q.downsampling, h, w, q.boundaries[pix0 + w]);
            int total;
            const int rank = cloud_chunk_rank(keep, total);
            if (keep) {
                const float d = q.depths[0][pix0 + w];
                float x, y;
                cloud_back_project(w, h, fx, cx, fy, cy, d, x, y);
                float* dst = q.points + (at + rank) * 6;
                dst[0] = x; dst[1] = y; dst[2] = d;
                dst[3] = static_cast<float>(display_u8(col[w]));
                dst[4] = static_cast<float>(display_u8(col[plane + w]));
                dst[5] = static_cast<float>(display_u8(col[2 * plane + w]));
            }
            at += total;
        }
    }
}

// blockIdx.y = 0: the error measures of (pair, half) blockIdx.x -- one compute unit's work each, dispatched first so that the panel
// rows run beside them; 1 .. 12: row blockIdx.x of section blockIdx.y - 1; 13: the point rows of band blockIdx.x of the pair-major list
__global__ void __launch_bounds__(kDispThreads) val_write_kernel(const ValParams q) {
    __shared__ uint8_t s_jet[256][3];          // B G R
    const DisplayGeom g = q.g;
    if (blockIdx.y == 0) {
        if (blockIdx.x < 2u * g.n) {
            const int f = blockIdx.x >> 1, half = blockIdx.x & 1;
            const int64_t plane = static_cast<int64_t>(g.h) * g.w;
            depth_metrics_block(q.depths[half] + f * plane, q.sparse_depths[half] + f * plane, q.sparse_masks[half] + f * plane, plane,
                                q.eps, q.metrics + static_cast<int64_t>(blockIdx.x) * 4);
        }
        return;
    }
    if (blockIdx.y == kValSections + 1) {
        if (blockIdx.x < static_cast<int64_t>(g.n) * g.bands) val_cloud_band(q, blockIdx.x / g.bands, blockIdx.x % g.bands);
        return;
    }
    if (static_cast<int>(blockIdx.x) >= g.gh) return;
    const int section = blockIdx.y - 1;
    const int half = section / 6, kind = section % 6;          // kind: 0 c, 1 sd, 2 d, 3 wd, 4 sf, 5 df
    int gy;
    const int hh = grid_axis(blockIdx.x, g.h, g.pad, gy);
    const int64_t plane = static_cast<int64_t>(g.h) * g.w;
    const float* fin = q.finals + half * kValFinal;
    const float lo = fin[0], hi = fin[1], den = fin[2], vmax = fin[3];
    if (kind >= 1 && kind <= 3) {
        jet_fill(s_jet, threadIdx.x);          // COLORMAP_JET (jet_device.h)
        __syncthreads();
    }
    const float ghf = static_cast<float>(g.gh), gwf = static_cast<float>(g.gw);
    const float* depth = kind == 1 ? q.sparse_depths[half] : kind == 2 ? q.depths[half] : q.warped[half];
    const float* flow = kind == 4 ? q.sparse_flows[half] : q.flows[half];
    uint8_t* dst = q.panel + (static_cast<int64_t>(section) * g.gh + blockIdx.x) * g.gw * 3;
    for (int64_t c = threadIdx.x; c < g.gw; c += kDispThreads) {
        int gx;
        const int ww = grid_axis(static_cast<int>(c), g.w, g.pad, gx);
        const int f = gy * g.xmaps + gx;
        const bool inside = hh >= 0 && ww >= 0 && f < g.n;
        const int64_t at = inside ? static_cast<int64_t>(hh) * g.w + ww : 0;
        int rgb[3] = {0, 0, 0};
        if (kind == 0) {
            if (inside) {
                const float* col = q.colors[half] + 3 * f * plane + at;
                const float b = q.boundaries[f * plane + at];
                rgb[0] = val_color_u8(col[0], b);
                rgb[1] = val_color_u8(col[plane], b);
                rgb[2] = val_color_u8(col[2 * plane], b);
            }
        } else if (kind <= 3) {
            // the half's range on every depth section (utils.py:924-940); the padding is 0 before the colormap: JET entry 0
            int idx = 0;
            if (inside) {
                float d = depth[f * plane + at];
                if (kind == 2) d = __fmul_rn(d, q.boundaries[f * plane + at]);
                idx = norm_jet_index(d, lo, hi, den);
            }
            rgb[0] = s_jet[idx][2];
            rgb[1] = s_jet[idx][1];
            rgb[2] = s_jet[idx][0];
        } else {
            // draw_flow (flow_pixel_rgb) with the dense flows' max_v on both sections; the padding is +0 in both components
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

struct ValLayout {
    int64_t partials, band_offsets, finals, total;
};

static ValLayout val_layout(int n, int h) {
    const int64_t items = static_cast<int64_t>(n) * ((h + kDispBandRows - 1) / kDispBandRows);
    ValLayout l;
    l.partials = 0;
    l.band_offsets = align256(2 * items * kValPartial * static_cast<int64_t>(sizeof(float)));
    l.finals = l.band_offsets + align256(items * static_cast<int64_t>(sizeof(int64_t)));
    l.total = l.finals + align256(2 * kValFinal * static_cast<int64_t>(sizeof(float)));
    return l;
}

// N, H, W in range and one section's rows and columns 32-bit numbers (the write kernel addresses sections by blockIdx.y and bytes in 64 bits)
static bool val_sizes_ok(int n, int h, int w) {
    if (!frames_sizes_ok(n, h, w)) return false;
    const int64_t xmaps = n < kDispNrow ? n : kDispNrow, ymaps = (n + xmaps - 1) / xmaps;
    const int64_t gh = (static_cast<int64_t>(h) + kDispPad) * ymaps + kDispPad, gw = (static_cast<int64_t>(w) + kDispPad) * xmaps + kDispPad;
    return gh <= INT32_MAX && gw <= INT32_MAX;
}

}  // namespace endo

using namespace endo;

extern "C" int endo_depth_metrics(const float* scaled_depths, const float* sparse_depths, const float* sparse_masks, int n, int h, int w,
                                  float eps, float* out, void* stream_) {
    if (!scaled_depths || !sparse_depths || !sparse_masks || !out) return ENDO_E_BADARG;
    if (!frames_sizes_ok(n, h, w)) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t pixels = static_cast<int64_t>(h) * w;
    ProfScope prof(kProfSmall, stream, 0.0, static_cast<double>(n) * pixels * 12.0);
    depth_metrics_kernel<<<n, kDispThreads, 0, stream>>>(scaled_depths, sparse_depths, sparse_masks, pixels, eps, out);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t endo_evaluate_validation_workspace_bytes(int n, int h, int w) {
    if (!val_sizes_ok(n, h, w)) return -1;
    return val_layout(n, h).total;
}

extern "C" int endo_evaluate_validation_panel_shape(int n, int h, int w, int* rows, int* cols) {
    if (!rows || !cols || !display_sizes_in_range(n, h, w, kValSections)) return ENDO_E_BADARG;          // 12 gh is an int
    const DisplayGeom g = display_geom(n, h, w);
    *rows = kValSections * g.gh;
    *cols = g.gw;
    return 0;
}

extern "C" int endo_evaluate_validation(const float* colors_1, const float* colors_2, const float* boundaries, const float* depths_1,
                                        const float* depths_2, const float* sparse_depths_1, const float* sparse_depths_2,
                                        const float* sparse_masks_1, const float* sparse_masks_2, const float* warped_2_to_1,
                                        const float* warped_1_to_2, const float* sparse_flows_1, const float* sparse_flows_2,
                                        const float* flows_1, const float* flows_2, const float* intrinsics, int n, int h, int w, float eps,
                                        int is_hsv, int point_cloud_downsampling, uint8_t* panel, float* metrics, float* points,
                                        int64_t* offsets, void* workspace, int64_t workspace_bytes, void* stream_) {
    if (!colors_1 || !colors_2 || !boundaries || !depths_1 || !depths_2 || !sparse_depths_1 || !sparse_depths_2 || !sparse_masks_1 ||
        !sparse_masks_2 || !warped_2_to_1 || !warped_1_to_2 || !sparse_flows_1 || !sparse_flows_2 || !flows_1 || !flows_2 || !intrinsics ||
        !panel || !metrics || !points || !offsets || !workspace)
        return ENDO_E_BADARG;
    if (!val_sizes_ok(n, h, w) || is_hsv != 0 || point_cloud_downsampling <= 0) return ENDO_E_BADARG;
    const ValLayout l = val_layout(n, h);
    if (workspace_bytes < l.total || reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    char* ws = static_cast<char*>(workspace);
    const DisplayGeom g = display_geom(n, h, w);
    const ValParams q{{colors_1, colors_2}, boundaries, {depths_1, depths_2}, {sparse_depths_1, sparse_depths_2},
                      {sparse_masks_1, sparse_masks_2}, {warped_2_to_1, warped_1_to_2}, {sparse_flows_1, sparse_flows_2},
                      {flows_1, flows_2}, intrinsics, g, eps, point_cloud_downsampling, panel, metrics, points, offsets,
                      reinterpret_cast<float*>(ws + l.partials), reinterpret_cast<int64_t*>(ws + l.band_offsets),
                      reinterpret_cast<float*>(ws + l.finals)};
    const double pixels = static_cast<double>(n) * h * w;
    // floats read per pixel: reduce 4 + 3 per half; write 4 + 1 + 2 + 1 + 2 + 2 per half, and 5 for the point rows; written: the panel
    // and up to 24 bytes per pixel of point rows
    ProfScope prof(kProfSmall, stream, 0.0,
                   pixels * 4.0 * (2 * 7 + 2 * 12 + 5) + pixels * 24.0 + static_cast<double>(kValSections) * g.gh * g.gw * 3.0);
    val_reduce_kernel<<<dim3(g.bands, n, 2), kDispThreads, 0, stream>>>(q);
    ENDO_LAUNCH_CHECK();
    val_scan_kernel<<<1, kScanThreads, 0, stream>>>(q);
    ENDO_LAUNCH_CHECK();
    const int64_t items = static_cast<int64_t>(n) * g.bands;
    const int64_t across = std::max<int64_t>(std::max<int64_t>(items, g.gh), 2 * n);
    val_write_kernel<<<dim3(static_cast<unsigned>(across), kValSections + 2), kDispThreads, 0, stream>>>(q);
    ENDO_LAUNCH_CHECK();
    return 0;
}
