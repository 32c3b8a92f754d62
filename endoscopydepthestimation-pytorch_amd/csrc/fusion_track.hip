// Frame-to-model alignment on the signed distance itself: every pixel of a depth map is back-projected under its frame's scale and
// pose, the trilinear tsdf of fusion.hip's volume sampled there (fusion_sample_device.h, the render kernel's sampler) is the pixel's
// signed distance to the model, and the normal equations of one Gauss-Newton step over the seven parameters of a similarity are
// summed per frame.  The reference has no code for this step; tests/fusion_track_restate.py is the numpy statement -- the per-pixel
// float32 numbers bit for bit, the fp64 sums up to their order of addition -- and include/endo_hip.h (endo_fusion_track) states the
// order of the operations.  Solving and stepping stay on the host (fusion.TSDFVolume.track): 40 doubles per frame and iteration.
//
//   pixels   a wave owns an 8 x 8 tile of pixels, a block 16 x 16 (the render kernel's shape: neighbouring pixels read neighbouring
//            cells), and a block walks kTrackTiles consecutive tiles of ONE frame, in tile order: a thread has kTrackTiles pixels and
//            keeps its 40 fp64 accumulators in registers over them.  Per pixel: 8 weights, 8 tsdf values, a few dozen fp32
//            operations, 40 fp64 multiply-adds.  Then once per thread: the wave's shuffle tree per sum, the block's four waves in
//            order through LDS, and the block's 40 partials to the workspace.
//   sums     one block per frame adds the frame's partials: lane l of a sum's wave takes blocks l, l + 64, ... in order, then the
//            wave's tree; it writes the frame's flag.  No atomics: the same arguments give the same bytes.
//
// numpy rounds every float32 operation on its own.  The file is compiled with -ffp-contract=off, as its siblings are (the fp64
// products and additions are then two roundings as well), and the float32 arithmetic is written with explicit-rounding intrinsics.
#include <cmath>

#include "common.h"
#include "fusion_device.h"
#include "fusion_sample_device.h"

namespace endo {

constexpr int kTrackTile = 8;                              // a wave's pixel tile: kTrackTile x kTrackTile
constexpr int kTrackThreads = 256;
constexpr int kTrackWaves = kTrackThreads / kWave;
constexpr int kTrackBlockTile = 2 * kTrackTile;            // a block's: 2 x 2 waves
constexpr int kTrackTiles = 4;                             // block tiles a block walks: a thread's pixels
constexpr int kTrackSums = 40;                             // count, sum r^2, sum |r|, max |r|, sum |y|^2, Jt r (7), upper JtJ (28)
constexpr int kTrackMax = 3;                               // the one sum that is a maximum

static_assert(kTrackTile * kTrackTile == kWave && kTrackThreads == 4 * kWave, "a lane owns one pixel of a tile, a block 2 x 2 tiles");
static_assert(5 + 7 + 28 == kTrackSums, "the layout of the header");

struct TrackParams {
    FusionVolume vol;
    const float* depth;           // [N][H][W]
    const float* boundaries;      // [N][H][W]
    const float* k;               // [N][3][3]
    const double* rotations;      // [N][3][3]
    const double* translations;   // [N][3]
    const float* scales;          // [N] or null
    int height, width, tiles_x, tiles;          // tiles: block tiles of a frame
    float min_weight, trunc, inv_vs, per_unit;          // per_unit = trunc * inv_vs
    double* partials;             // [N][blocks][kTrackSums]
    float* residual;              // [N][H][W] or null
    float* valid;                 // [N][H][W] or null
    float* gradient;              // [N][H][W][3] or null
};

inline int track_tiles(int extent) { return (extent + kTrackBlockTile - 1) / kTrackBlockTile; }
inline int64_t track_blocks(int height, int width) {
    return (static_cast<int64_t>(track_tiles(height)) * track_tiles(width) + kTrackTiles - 1) / kTrackTiles;
}

__device__ __forceinline__ bool scale_ok(float s) { return s > 0.0f && s < INFINITY; }

__global__ void __launch_bounds__(kTrackThreads) fusion_track_kernel(const TrackParams q) {
    __shared__ double s_part[kTrackWaves][kTrackSums];
    const FusionVolume& g = q.vol;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = blockIdx.y;
    const float scale = q.scales ? q.scales[f] : 1.0f;
    const bool frame_ok = scale_ok(scale);
    const float* kf = q.k + static_cast<int64_t>(f) * 9;
    const double* rot = q.rotations + static_cast<int64_t>(f) * 9;
    const double* tr = q.translations + static_cast<int64_t>(f) * 3;
    float rf[9], tf[3];
#pragma unroll
    for (int a = 0; a < 9; ++a) rf[a] = static_cast<float>(rot[a]);
#pragma unroll
    for (int a = 0; a < 3; ++a) tf[a] = static_cast<float>(tr[a]);
    const float fx = kf[0], cx = kf[2], fy = kf[4], cy = kf[5];

    double acc[kTrackSums];
#pragma unroll
    for (int j = 0; j < kTrackSums; ++j) acc[j] = 0.0;

#pragma unroll 1
    for (int step = 0; step < kTrackTiles; ++step) {
        const int tile = blockIdx.x * kTrackTiles + step;
        if (tile >= q.tiles) break;          // (the same for the whole block)
        const int u = (tile % q.tiles_x) * kTrackBlockTile + (wave & 1) * kTrackTile + (lane & (kTrackTile - 1));
        const int v = (tile / q.tiles_x) * kTrackBlockTile + (wave >> 1) * kTrackTile + lane / kTrackTile;
        if (u >= q.width || v >= q.height) continue;
        const int64_t pix = (static_cast<int64_t>(f) * q.height + v) * q.width + u;
        float r = 0.0f, n[3] = {0.0f, 0.0f, 0.0f}, y[3];
        bool sample = false;
        Cell c;
        if (frame_ok && q.boundaries[pix] > 0.5f) {
            const float d = q.depth[pix];
            if (d > 0.0f && d < INFINITY) {
                const float dx = __fdiv_rn(__fsub_rn(static_cast<float>(u), cx), fx);
                const float dy = __fdiv_rn(__fsub_rn(static_cast<float>(v), cy), fy);
                const float sd = __fmul_rn(scale, d);
                float x[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float w = __fadd_rn(__fadd_rn(__fmul_rn(rf[3 * a], dx), __fmul_rn(rf[3 * a + 1], dy)), rf[3 * a + 2]);
                    y[a] = __fmul_rn(sd, w);
                    x[a] = __fadd_rn(tf[a], y[a]);
                }
                sample = locate_point(g, q.inv_vs, x, c) && weights_ok(g, c, q.min_weight);
            }
        }
        if (sample) {
            float grad[3];
            const float phi = trilinear_gradient(g, c, grad);
            r = __fmul_rn(phi, q.trunc);
#pragma unroll
            for (int a = 0; a < 3; ++a) n[a] = __fmul_rn(grad[a], q.per_unit);
            float jf[7];
            jf[0] = __fsub_rn(__fmul_rn(y[1], n[2]), __fmul_rn(y[2], n[1]));
            jf[1] = __fsub_rn(__fmul_rn(y[2], n[0]), __fmul_rn(y[0], n[2]));
            jf[2] = __fsub_rn(__fmul_rn(y[0], n[1]), __fmul_rn(y[1], n[0]));
            jf[3] = n[0]; jf[4] = n[1]; jf[5] = n[2];
            jf[6] = __fadd_rn(__fadd_rn(__fmul_rn(n[0], y[0]), __fmul_rn(n[1], y[1])), __fmul_rn(n[2], y[2]));
            const float y2 = __fadd_rn(__fadd_rn(__fmul_rn(y[0], y[0]), __fmul_rn(y[1], y[1])), __fmul_rn(y[2], y[2]));
            const double rd = static_cast<double>(r), ra = fabs(rd);
            double jd[7];
#pragma unroll
            for (int i = 0; i < 7; ++i) jd[i] = static_cast<double>(jf[i]);
            acc[0] += 1.0;
            acc[1] += rd * rd;
            acc[2] += ra;
            acc[kTrackMax] = fmax(acc[kTrackMax], ra);
            acc[4] += static_cast<double>(y2);
            int at = 12;
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                acc[5 + i] += jd[i] * rd;
#pragma unroll
                for (int j = i; j < 7; ++j) acc[at++] += jd[i] * jd[j];
            }
        }
        if (q.residual) q.residual[pix] = r;
        if (q.valid) q.valid[pix] = sample ? 1.0f : 0.0f;
        if (q.gradient) {
#pragma unroll
            for (int a = 0; a < 3; ++a) q.gradient[pix * 3 + a] = n[a];
        }
    }

#pragma unroll
    for (int j = 0; j < kTrackSums; ++j) {
        double w = acc[j];
        if (j == kTrackMax) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) w = fmax(w, __shfl_down(w, off, kWave));
        } else {
            w = wave_sum(w);
        }
        if (lane == 0) s_part[wave][j] = w;
    }
    __syncthreads();
    if (threadIdx.x < kTrackSums) {
        const int j = threadIdx.x;
        double w = s_part[0][j];
        for (int i = 1; i < kTrackWaves; ++i) w = j == kTrackMax ? fmax(w, s_part[i][j]) : w + s_part[i][j];
        q.partials[(static_cast<int64_t>(f) * gridDim.x + blockIdx.x) * kTrackSums + j] = w;
    }
}

// a frame's partials in a fixed order: lane l of the sum's wave takes blocks l, l + 64, ..., then the wave's tree
__global__ void __launch_bounds__(kTrackThreads) fusion_track_sums_kernel(const double* __restrict__ partials, int blocks,
                                                                          const float* __restrict__ scales, double* __restrict__ sums,
                                                                          int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = blockIdx.x;
    const double* part = partials + static_cast<int64_t>(f) * blocks * kTrackSums;
    for (int j = wave; j < kTrackSums; j += kTrackWaves) {
        double w = 0.0;
        if (j == kTrackMax) {
            for (int i = lane; i < blocks; i += kWave) w = fmax(w, part[static_cast<int64_t>(i) * kTrackSums + j]);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) w = fmax(w, __shfl_down(w, off, kWave));
        } else {
            for (int i = lane; i < blocks; i += kWave) w += part[static_cast<int64_t>(i) * kTrackSums + j];
            w = wave_sum(w);
        }
        if (lane == 0) sums[static_cast<int64_t>(f) * kTrackSums + j] = w;
    }
    if (threadIdx.x == 0) flags[f] = scale_ok(scales ? scales[f] : 1.0f) ? ENDO_FUSION_FRAME_OK : ENDO_FUSION_FRAME_BAD_SCALE;
}

}  // namespace endo

using namespace endo;

extern "C" int endo_fusion_track_tile(int which) {
    return which == 0 || which == 1 ? kTrackBlockTile : (which == 2 ? kTrackTiles : ENDO_E_BADARG);
}

extern "C" int64_t endo_fusion_track_workspace_bytes(int frames, int height, int width) {
    if (!frames_sizes_ok(frames, height, width)) return -1;
    return align256(static_cast<int64_t>(frames) * track_blocks(height, width) * kTrackSums * static_cast<int64_t>(sizeof(double)));
}

extern "C" int endo_fusion_track(const double* origin, double voxel_size, double truncation, int nx, int ny, int nz, const float* tsdf,
                                 const float* weight, const float* depth, const float* boundaries, const float* intrinsics,
                                 const double* rotations, const double* translations, const float* scales, int frames, int height,
                                 int width, float min_weight, double* sums, int32_t* flags, float* residual, float* valid,
                                 float* gradient, void* workspace, int64_t workspace_bytes, void* stream_) {
    if (!depth || !boundaries || !intrinsics || !rotations || !translations || !sums || !flags || !workspace) return ENDO_E_BADARG;
    if (std::isnan(min_weight)) return ENDO_E_BADARG;
    const int64_t need = endo_fusion_track_workspace_bytes(frames, height, width);
    if (need < 0 || workspace_bytes < need) return ENDO_E_BADARG;
    if (nx > kMaxAxis) return ENDO_E_BADARG;
    TrackParams p;
    // (the colour planes take no part: the tsdf plane stands in for them in the volume's checks and is never read through `color`)
    if (!make_volume(origin, voxel_size, nx, ny, nz, const_cast<float*>(tsdf), const_cast<float*>(weight), const_cast<float*>(tsdf), p.vol))
        return ENDO_E_BADARG;
    p.vol.color = nullptr;
    const float trunc = static_cast<float>(truncation);
    if (!(trunc > 0.0f) || !std::isfinite(trunc)) return ENDO_E_BADARG;
    p.depth = depth; p.boundaries = boundaries; p.k = intrinsics; p.rotations = rotations; p.translations = translations; p.scales = scales;
    p.height = height; p.width = width; p.tiles_x = track_tiles(width); p.tiles = track_tiles(height) * p.tiles_x;
    p.min_weight = min_weight; p.trunc = trunc; p.inv_vs = 1.0f / p.vol.vs;
    p.per_unit = trunc * p.inv_vs;          // (-ffp-contract=off: one rounding, the restatement's)
    p.partials = static_cast<double*>(workspace);
    p.residual = residual; p.valid = valid; p.gradient = gradient;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t blocks = track_blocks(height, width);
    const double pixels = static_cast<double>(frames) * height * width;
    ProfScope prof(kProfSmall, stream, pixels * 150.0, pixels * (8.0 + 64.0 + (residual ? 4.0 : 0.0) + (valid ? 4.0 : 0.0) + (gradient ? 12.0 : 0.0)));
    fusion_track_kernel<<<dim3(static_cast<unsigned>(blocks), frames), kTrackThreads, 0, stream>>>(p);
    ENDO_LAUNCH_CHECK();
    fusion_track_sums_kernel<<<frames, kTrackThreads, 0, stream>>>(p.partials, static_cast<int>(blocks), scales, sums, flags);
    ENDO_LAUNCH_CHECK();
    return 0;
}
