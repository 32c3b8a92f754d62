// Test output in the electromagnetic tracker's frame -- reference utils.py:1316-1355 (write_test_output_with_initial_pose: colour
// image, depth image through display_depth_map / COLORMAP_JET, utils.py:773-781) with utils.py:1246-1295
// (point_cloud_from_depth_and_initial_pose: each frame's cloud normalised to a z range of 20 units, then moved by that frame's rotation
// and translation, so a whole sequence lands in one coordinate system), for a whole batch on the device.
// tests/evaluate_posed_restate.py is the numpy statement every output is checked against, bit for bit.
//
// Three launches whatever the batch size, with the geometry of evaluate.hip:
//   rows   one block per (frame, row): masked depth d = b * pred; the row's count of WRITTEN pixels, the minimum and maximum of d over
//          its KEPT pixels (h % ds == 0, w % ds == 0, b > 0.5) and over all its pixels.  With thresholds the written set is a subset of the
//          kept set (utils.py:1285-1288), so the colour display is formed here too; the z range is that of the kept set
//          (utils.py:1260-1271 comes before the threshold test)
//   scan   one block: exclusive prefix of the N * H row counts, frame-major; each frame's (z_min, z_max) over its kept pixels, (+inf, -inf)
//          when there is none, and its whole-map (min, max)
//   write  one block per (frame, row): colour image, depth image and, for written pixels, the transformed point at the row's offset,
//          ordered inside the row by cloud_device.h's chunk rank
// numpy rounds every float32 / float64 operation on its own: the file is compiled with -ffp-contract=off and the roundings are explicit.
#include <cmath>

#include "cloud_device.h"
#include "common.h"
#include "hsv_device.h"
#include "jet_device.h"

namespace endo {

struct PosedParams {
    const float* colors;          // [N][3][H][W] boundaries * colours_1 (normalised, masked)
    const float* boundaries;      // [N][H][W]
    const float* pred;            // [N][H][W]
    const float* k;               // [N][3][3]
    const double* rotations;      // [N][3][3]
    const double* translations;   // [N][3]
    int frames, height, width, is_hsv, downsampling, use_thresholds;
    float min_threshold, max_threshold;
    float* depth;                 // [N][H][W]
    uint8_t* color_images;        // [N][H][W][3]
    uint8_t* depth_images;        // [N][H][W][3] B G R
    float* points;                // [N * H * W][6]
    int64_t* frame_offsets;       // [N + 1]
    float* frame_ranges;          // [N][2] z_min, z_max over the kept pixels
    int64_t* row_offsets;         // [N * H] workspace: counts after `rows`, exclusive offsets after `scan`
    float* row_stats;             // [N * H][4] workspace: kept min, kept max, whole min, whole max
    float* frame_whole;           // [N][2] workspace: whole-map min, max
};

// The colour image's three channels at pixel w of a row (utils.py:1331-1336).  RGB input: its channels as they are (the reference has no
// RGB -> BGR swap here); HSV input: cv2.COLOR_HSV2BGR_FULL, so B, G, R.
__device__ __forceinline__ void posed_color(const PosedParams& q, const float* col, int64_t plane, int w, int (&img)[3]) {
    const int c0 = posed_u8(col[w]), c1 = posed_u8(col[plane + w]), c2 = posed_u8(col[2 * plane + w]);
    if (q.is_hsv) {
        int rgb[3];
        hsv_to_rgb<256>(c0, c1, c2, rgb);
        img[0] = rgb[2]; img[1] = rgb[1]; img[2] = rgb[0];
    } else {
        img[0] = c0; img[1] = c1; img[2] = c2;
    }
}

// utils.py:1285-1291: with both thresholds, a kept pixel is written when max(r, g, b) >= max_threshold and min(r, g, b) <= min_threshold
__device__ __forceinline__ bool posed_written(const PosedParams& q, const int (&img)[3]) {
    if (!q.use_thresholds) return true;
    const int hi = max(img[0], max(img[1], img[2])), lo = min(img[0], min(img[1], img[2]));
    return static_cast<float>(hi) >= q.max_threshold && static_cast<float>(lo) <= q.min_threshold;
}

__global__ void __launch_bounds__(kCloudThreads) posed_rows_kernel(const PosedParams q) {
    __shared__ float s_stat[4][4];
    const int h = blockIdx.x, f = blockIdx.y;
    const int64_t row = static_cast<int64_t>(f) * q.height + h;
    const int64_t base = row * q.width;
    const int64_t plane = static_cast<int64_t>(q.height) * q.width;
    const float* col = q.colors + static_cast<int64_t>(f) * 3 * plane + static_cast<int64_t>(h) * q.width;
    int cnt = 0;
    float kmin = INFINITY, kmax = -INFINITY, amin = INFINITY, amax = -INFINITY;
    for (int w = threadIdx.x; w < q.width; w += kCloudThreads) {
        const float bnd = q.boundaries[base + w];
        const float d = __fmul_rn(bnd, q.pred[base + w]);          // (boundaries * scaled_depth_maps_1), utils.py:1321
        q.depth[base + w] = d;
        amin = fminf(amin, d);
        amax = fmaxf(amax, d);
        bool written = cloud_pixel_keep(q.downsampling, h, w, bnd);          // utils.py:1262
        if (written) {
            kmin = fminf(kmin, d);
            kmax = fmaxf(kmax, d);
            if (q.use_thresholds) {
                int img[3];
                posed_color(q, col, plane, w, img);
                written = posed_written(q, img);
            }
        }
        cnt += cloud_wave_count(written);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        kmin = fminf(kmin, __shfl_down(kmin, off, 64));
        kmax = fmaxf(kmax, __shfl_down(kmax, off, 64));
        amin = fminf(amin, __shfl_down(amin, off, 64));
        amax = fmaxf(amax, __shfl_down(amax, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        s_stat[wv][0] = kmin; s_stat[wv][1] = kmax; s_stat[wv][2] = amin; s_stat[wv][3] = amax;
    }
    cnt = cloud_block_count(cnt);          // (its barrier publishes s_stat too)
    if (threadIdx.x == 0) q.row_offsets[row] = cnt;
    if (threadIdx.x < 4) {
        const int j = threadIdx.x;
        const float a = s_stat[0][j], b = s_stat[1][j], c = s_stat[2][j], e = s_stat[3][j];
        q.row_stats[row * 4 + j] = (j & 1) ? fmaxf(fmaxf(a, b), fmaxf(c, e)) : fminf(fminf(a, b), fminf(c, e));
    }
}

// the rows' offsets and the frames' (cloud_scan_block); then one wave per frame reduces the frame's row statistics
__global__ void __launch_bounds__(kScanThreads) posed_scan_kernel(const PosedParams q) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    cloud_scan_block(q.row_offsets, q.frames, q.height, q.frame_offsets);
    for (int f = wave; f < q.frames; f += kScanThreads / 64) {
        float kmin = INFINITY, kmax = -INFINITY, amin = INFINITY, amax = -INFINITY;
        for (int h = lane; h < q.height; h += 64) {
            const float* s = q.row_stats + (static_cast<int64_t>(f) * q.height + h) * 4;
            kmin = fminf(kmin, s[0]);
            kmax = fmaxf(kmax, s[1]);
            amin = fminf(amin, s[2]);
            amax = fmaxf(amax, s[3]);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            kmin = fminf(kmin, __shfl_down(kmin, off, 64));
            kmax = fmaxf(kmax, __shfl_down(kmax, off, 64));
            amin = fminf(amin, __shfl_down(amin, off, 64));
            amax = fmaxf(amax, __shfl_down(amax, off, 64));
        }
        if (lane == 0) {
            q.frame_ranges[2 * f] = kmin;
            q.frame_ranges[2 * f + 1] = kmax;
            q.frame_whole[2 * f] = amin;
            q.frame_whole[2 * f + 1] = amax;
        }
    }
}

__global__ void __launch_bounds__(kCloudThreads) posed_write_kernel(const PosedParams q) {
    __shared__ uint8_t s_jet[256][3];          // B G R
    const int h = blockIdx.x, f = blockIdx.y;
    jet_fill(s_jet, threadIdx.x);          // COLORMAP_JET (jet_device.h)
    __syncthreads();
    int64_t at = q.row_offsets[static_cast<int64_t>(f) * q.height + h];          // where this chunk's points start
    const float amin = q.frame_whole[2 * f], amax = q.frame_whole[2 * f + 1];
    const float span = __fsub_rn(amax, amin);
    // scale = 20.0 / (z_max - z_min), utils.py:1271: float32 under numpy 2's scalar promotion
    const float scale = __fdiv_rn(20.0f, __fsub_rn(q.frame_ranges[2 * f + 1], q.frame_ranges[2 * f]));
    const float* kf = q.k + static_cast<int64_t>(f) * 9;
    const float fx = kf[0], cx = kf[2], fy = kf[4], cy = kf[5];
    const double* rot = q.rotations + static_cast<int64_t>(f) * 9;
    const double* tr = q.translations + static_cast<int64_t>(f) * 3;
    const int64_t plane = static_cast<int64_t>(q.height) * q.width;
    const int64_t pix0 = (static_cast<int64_t>(f) * q.height + h) * q.width;
    const float* col = q.colors + static_cast<int64_t>(f) * 3 * plane + static_cast<int64_t>(h) * q.width;
    for (int w0 = 0; w0 < q.width; w0 += kCloudThreads) {
        const int w = w0 + threadIdx.x;
        bool write = false;
        float d = 0.0f;
        int img[3] = {0, 0, 0};
        if (w < q.width) {
            const float bnd = q.boundaries[pix0 + w];
            d = q.depth[pix0 + w];
            posed_color(q, col, plane, w, img);
            write = cloud_pixel_keep(q.downsampling, h, w, bnd) && posed_written(q, img);
            uint8_t* ci = q.color_images + (pix0 + w) * 3;
            ci[0] = static_cast<uint8_t>(img[0]); ci[1] = static_cast<uint8_t>(img[1]); ci[2] = static_cast<uint8_t>(img[2]);
            // display_depth_map, utils.py:777-780: abs((d - min) / (max - min) * 255), above 255 -> 255, at or below 0 -> 0, truncated.
            // A frame whose maximum equals its minimum (0 / 0 in the reference) takes index 0 everywhere.
            int idx = 0;
            if (span > 0.0f) {
                const float v = fabsf(__fmul_rn(__fdiv_rn(__fsub_rn(d, amin), span), 255.0f));
                idx = v > 255.0f ? 255 : (v > 0.0f ? static_cast<int>(v) : 0);
            }
            uint8_t* di = q.depth_images + (pix0 + w) * 3;
            di[0] = s_jet[idx][0]; di[1] = s_jet[idx][1]; di[2] = s_jet[idx][2];
        }
        int total;
        const int rank = cloud_chunk_rank(write, total);
        if (write) {
            // utils.py:1277-1280: (w - cx) / fx * z in float32, each coordinate times the float32 scale, then R p + t in float64:
            // ((R_i0 p_x + R_i1 p_y) + R_i2 p_z) + t_i, every product and sum rounded, the result rounded to float32 (utils.py:1293)
            float x, y;
            cloud_back_project(w, h, fx, cx, fy, cy, d, x, y);
            const double px = static_cast<double>(__fmul_rn(x, scale));
            const double py = static_cast<double>(__fmul_rn(y, scale));
            const double pz = static_cast<double>(__fmul_rn(d, scale));
            float* dst = q.points + (at + rank) * 6;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double s01 = __dadd_rn(__dmul_rn(rot[3 * i], px), __dmul_rn(rot[3 * i + 1], py));
                const double s012 = __dadd_rn(s01, __dmul_rn(rot[3 * i + 2], pz));
                dst[i] = __double2float_rn(__dadd_rn(s012, tr[i]));
            }
            dst[3] = static_cast<float>(img[2]);          // r, g, b = channels 2, 1, 0 of the colour image (utils.py:1282-1284)
            dst[4] = static_cast<float>(img[1]);
            dst[5] = static_cast<float>(img[0]);
        }
        at += total;
    }
}

struct PosedLayout {
    int64_t row_offsets, row_stats, frame_whole, total;
};

static PosedLayout posed_layout(int frames, int height) {
    const int64_t rows = static_cast<int64_t>(frames) * height;
    PosedLayout l;
    l.row_offsets = 0;
    l.row_stats = align256(rows * static_cast<int64_t>(sizeof(int64_t)));
    l.frame_whole = l.row_stats + align256(rows * 4 * static_cast<int64_t>(sizeof(float)));
    l.total = l.frame_whole + align256(static_cast<int64_t>(frames) * 2 * sizeof(float));
    return l;
}

}  // namespace endo

using namespace endo;

extern "C" int64_t endo_evaluate_posed_workspace_bytes(int frames, int height, int width) {
    if (!frames_sizes_ok(frames, height, width)) return -1;
    return posed_layout(frames, height).total;
}

extern "C" int endo_evaluate_posed(const float* colors, const float* boundaries, const float* predictions, const float* intrinsics,
                                   const double* rotations, const double* translations, int frames, int height, int width, int is_hsv,
                                   int point_cloud_downsampling, int use_thresholds, float min_threshold, float max_threshold, float* depth,
                                   uint8_t* color_images, uint8_t* depth_images, float* points, int64_t* frame_offsets, float* frame_ranges,
                                   void* workspace, int64_t workspace_bytes, void* stream_) {
    if (!colors || !boundaries || !predictions || !intrinsics || !rotations || !translations || !depth || !color_images || !depth_images ||
        !points || !frame_offsets || !frame_ranges || !workspace)
        return ENDO_E_BADARG;
    if (!frames_sizes_ok(frames, height, width) || (is_hsv != 0 && is_hsv != 1) || point_cloud_downsampling <= 0 ||
        (use_thresholds != 0 && use_thresholds != 1))
        return ENDO_E_BADARG;
    if (use_thresholds && (std::isnan(min_threshold) || std::isnan(max_threshold))) return ENDO_E_BADARG;
    const PosedLayout l = posed_layout(frames, height);
    if (workspace_bytes < l.total) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    char* ws = static_cast<char*>(workspace);
    const PosedParams q{colors, boundaries, predictions, intrinsics, rotations, translations, frames, height, width, is_hsv,
                        point_cloud_downsampling, use_thresholds, min_threshold, max_threshold, depth, color_images, depth_images, points,
                        frame_offsets, frame_ranges, reinterpret_cast<int64_t*>(ws + l.row_offsets),
                        reinterpret_cast<float*>(ws + l.row_stats), reinterpret_cast<float*>(ws + l.frame_whole)};
    const double pixels = static_cast<double>(frames) * height * width;
    ProfScope prof(kProfSmall, stream, 0.0, pixels * (4.0 * 5 + 4.0 + 4.0 + 4.0 * 4 + 6.0 + 24.0));
    posed_rows_kernel<<<dim3(height, frames), kCloudThreads, 0, stream>>>(q);
    ENDO_LAUNCH_CHECK();
    posed_scan_kernel<<<1, kScanThreads, 0, stream>>>(q);
    ENDO_LAUNCH_CHECK();
    posed_write_kernel<<<dim3(height, frames), kCloudThreads, 0, stream>>>(q);
    ENDO_LAUNCH_CHECK();
    return 0;
}
