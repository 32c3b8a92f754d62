// Test-phase outputs -- reference evaluate.py:317-345 (per frame: colour display, depth display through COLORMAP_JET, the colour|depth
// panel of cv2.hconcat and the coloured point cloud of utils.point_cloud_from_depth, utils.py:825-852) for a whole batch on the device.
// tests/evaluate_restate.py is the numpy statement every output is checked against, bit for bit.
//
// Three launches whatever the batch size:
//   rows   one block per (frame, row): masked depth d = b * pred, the row's maximum of d and its count of kept pixels
//   scan   one block: exclusive prefix of the N * H row counts (frame-major, so each frame's points follow the previous frame's) and
//          each frame's maximum of d from its row maxima
//   write  one block per (frame, row): each pixel's colour display formed once, written to the panel and, when kept, to the point
//          cloud at the row's offset, ordered inside the row by cloud_device.h's chunk rank
// numpy's float32 arithmetic rounds every operation on its own: contraction is off and the roundings are explicit.
#include <cmath>

#include "cloud_device.h"
#include "common.h"
#include "hsv_device.h"
#include "jet_device.h"

namespace endo {

struct EvalParams {
    const float* colors;          // [N][3][H][W] boundaries * colours_1 (normalised, masked)
    const float* boundaries;      // [N][H][W]
    const float* pred;            // [N][H][W]
    const float* k;               // [N][3][3]
    int frames, height, width, is_hsv, downsampling;
    float* depth;                 // [N][H][W]
    uint8_t* panels;              // [N][H][2W][3] B G R
    float* points;                // [N * H * W][6]
    int64_t* frame_offsets;       // [N + 1]
    int64_t* row_offsets;         // [N * H] workspace: counts after `rows`, exclusive offsets after `scan`
    float* row_max;               // [N * H] workspace
    float* frame_max;             // [N] workspace
};

__global__ void __launch_bounds__(kCloudThreads) eval_rows_kernel(const EvalParams q) {
    __shared__ float s_max[4];
    const int h = blockIdx.x, f = blockIdx.y;
    const int64_t row = static_cast<int64_t>(f) * q.height + h;
    const int64_t base = row * q.width;
    int cnt = 0;
    float mx = -INFINITY;
    for (int w = threadIdx.x; w < q.width; w += kCloudThreads) {
        const float bnd = q.boundaries[base + w];
        const float d = __fmul_rn(bnd, q.pred[base + w]);          // (boundaries * predicted_depth_maps_1), evaluate.py:338
        q.depth[base + w] = d;
        mx = fmaxf(mx, d);
        cnt += cloud_wave_count(cloud_pixel_keep(q.downsampling, h, w, bnd));          // (no thresholds: evaluate.py:340)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_down(mx, off, 64));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
    cnt = cloud_block_count(cnt);          // (its barrier publishes s_max too)
    if (threadIdx.x == 0) {
        q.row_offsets[row] = cnt;
        q.row_max[row] = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    }
}

// the rows' offsets and the frames' (cloud_scan_block), then each frame's maximum
__global__ void __launch_bounds__(kScanThreads) eval_scan_kernel(const EvalParams q) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    cloud_scan_block(q.row_offsets, q.frames, q.height, q.frame_offsets);
    // np.max(depth_map) of each frame: one wave per frame over its row maxima
    for (int f = wave; f < q.frames; f += kScanThreads / 64) {
        float mx = -INFINITY;
        for (int h = lane; h < q.height; h += 64) mx = fmaxf(mx, q.row_max[static_cast<int64_t>(f) * q.height + h]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_down(mx, off, 64));
        if (lane == 0) q.frame_max[f] = mx;
    }
}

// np.uint8(b * x) of a float32 b in [0, 1] and a uint8 x (evaluate.py:336-337)
__device__ __forceinline__ int masked_u8(float b, int x) {
    const float v = __fmul_rn(b, static_cast<float>(x));
    return v > 0.0f ? min(static_cast<int>(v), 255) : 0;
}

__global__ void __launch_bounds__(kCloudThreads) eval_write_kernel(const EvalParams q) {
    __shared__ uint8_t s_jet[256][3];          // B G R
    const int h = blockIdx.x, f = blockIdx.y;
    jet_fill(s_jet, threadIdx.x);          // COLORMAP_JET (jet_device.h)
    __syncthreads();
    int64_t at = q.row_offsets[static_cast<int64_t>(f) * q.height + h];          // where this chunk's points start
    const float mx = q.frame_max[f];
    const float* kf = q.k + static_cast<int64_t>(f) * 9;
    const float fx = kf[0], cx = kf[2], fy = kf[4], cy = kf[5];
    const int64_t plane = static_cast<int64_t>(q.height) * q.width;
    const int64_t pix0 = (static_cast<int64_t>(f) * q.height + h) * q.width;
    const float* col = q.colors + static_cast<int64_t>(f) * 3 * plane + static_cast<int64_t>(h) * q.width;
    uint8_t* panel = q.panels + pix0 * 6;          // this row of the (H, 2W, 3) panel
    for (int w0 = 0; w0 < q.width; w0 += kCloudThreads) {
        const int w = w0 + threadIdx.x;
        bool keep = false;
        float bnd = 0.0f, d = 0.0f;
        int bgr[3] = {0, 0, 0};
        if (w < q.width) {
            bnd = q.boundaries[pix0 + w];
            d = q.depth[pix0 + w];
            keep = cloud_pixel_keep(q.downsampling, h, w, bnd);
            const int c0 = display_u8(col[w]), c1 = display_u8(col[plane + w]), c2 = display_u8(col[2 * plane + w]);
            if (q.is_hsv) {          // cv2.COLOR_HSV2BGR_FULL of (H, S, V) = (c0, c1, c2)
                int rgb[3];
                hsv_to_rgb<256>(c0, c1, c2, rgb);
                bgr[0] = rgb[2]; bgr[1] = rgb[1]; bgr[2] = rgb[0];
            } else {                 // cv2.COLOR_RGB2BGR
                bgr[0] = c2; bgr[1] = c1; bgr[2] = c0;
            }
            bgr[0] = masked_u8(bnd, bgr[0]); bgr[1] = masked_u8(bnd, bgr[1]); bgr[2] = masked_u8(bnd, bgr[2]);
            // np.uint8(255 * d / np.max(d)) (evaluate.py:339): 255 * d rounded, divided by the maximum, truncated.  A frame whose maximum
            // is 0 (0 / 0 in the reference) takes index 0 everywhere.
            int idx = 0;
            if (mx > 0.0f) {
                const float v = __fdiv_rn(__fmul_rn(255.0f, d), mx);
                idx = v > 0.0f ? min(static_cast<int>(v), 255) : 0;
            }
            uint8_t* left = panel + static_cast<int64_t>(w) * 3;
            uint8_t* right = panel + (static_cast<int64_t>(q.width) + w) * 3;
            left[0] = static_cast<uint8_t>(bgr[0]); left[1] = static_cast<uint8_t>(bgr[1]); left[2] = static_cast<uint8_t>(bgr[2]);
            right[0] = s_jet[idx][0]; right[1] = s_jet[idx][1]; right[2] = s_jet[idx][2];
        }
        int total;
        const int rank = cloud_chunk_rank(keep, total);
        if (keep) {
            float x, y;
            cloud_back_project(w, h, fx, cx, fy, cy, d, x, y);
            float* dst = q.points + (at + rank) * 6;
            dst[0] = x; dst[1] = y; dst[2] = d;
            dst[3] = static_cast<float>(bgr[2]);
            dst[4] = static_cast<float>(bgr[1]);
            dst[5] = static_cast<float>(bgr[0]);
        }
        at += total;
    }
}

struct EvalLayout {
    int64_t row_offsets, row_max, frame_max, total;
};

static EvalLayout eval_layout(int frames, int height) {
    const int64_t rows = static_cast<int64_t>(frames) * height;
    EvalLayout l;
    l.row_offsets = 0;
    l.row_max = align256(rows * static_cast<int64_t>(sizeof(int64_t)));
    l.frame_max = l.row_max + align256(rows * static_cast<int64_t>(sizeof(float)));
    l.total = l.frame_max + align256(static_cast<int64_t>(frames) * sizeof(float));
    return l;
}

}  // namespace endo

using namespace endo;

extern "C" int64_t endo_evaluate_workspace_bytes(int frames, int height, int width) {
    if (!frames_sizes_ok(frames, height, width)) return -1;
    return eval_layout(frames, height).total;
}

extern "C" int endo_evaluate(const float* colors, const float* boundaries, const float* predictions, const float* intrinsics, int frames,
                             int height, int width, int is_hsv, int point_cloud_downsampling, float* depth, uint8_t* panels, float* points,
                             int64_t* frame_offsets, void* workspace, int64_t workspace_bytes, void* stream_) {
    if (!colors || !boundaries || !predictions || !intrinsics || !depth || !panels || !points || !frame_offsets || !workspace) return ENDO_E_BADARG;
    if (!frames_sizes_ok(frames, height, width) || (is_hsv != 0 && is_hsv != 1) || point_cloud_downsampling <= 0) return ENDO_E_BADARG;
    const EvalLayout l = eval_layout(frames, height);
    if (workspace_bytes < l.total) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    char* ws = static_cast<char*>(workspace);
    const EvalParams q{colors, boundaries, predictions, intrinsics, frames, height, width, is_hsv, point_cloud_downsampling, depth, panels,
                       points, frame_offsets, reinterpret_cast<int64_t*>(ws + l.row_offsets), reinterpret_cast<float*>(ws + l.row_max),
                       reinterpret_cast<float*>(ws + l.frame_max)};
    const double pixels = static_cast<double>(frames) * height * width;
    ProfScope prof(kProfSmall, stream, 0.0, pixels * (4.0 * 5 + 4.0 + 6.0 + 24.0));
    eval_rows_kernel<<<dim3(height, frames), kCloudThreads, 0, stream>>>(q);
    ENDO_LAUNCH_CHECK();
    eval_scan_kernel<<<1, kScanThreads, 0, stream>>>(q);
    ENDO_LAUNCH_CHECK();
    eval_write_kernel<<<dim3(height, frames), kCloudThreads, 0, stream>>>(q);
    ENDO_LAUNCH_CHECK();
    return 0;
}
