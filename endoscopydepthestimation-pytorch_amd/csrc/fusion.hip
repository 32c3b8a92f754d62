// Volumetric fusion of a sequence's posed depth maps into one surface: a truncated signed distance function (TSDF) on a voxel grid,
// averaged over the frames that saw a voxel, and its zero crossings on the grid's edges as coloured points.  The reference has no code
// for this step (its posed test output, utils.py:1316-1355, ends at one cloud per frame); tests/fusion_restate.py is the numpy float32
// statement every plane and row is held to, bit for bit.
//
//   clear      tsdf = 1, weight = 0, colour = 0
//   frames     one block per frame (the pre-pass): z_min / z_max of boundaries * depth over the kept pixels (b > 0.5), the frame's
//              scale -- the caller's, or the posed output's own 20.0f / (z_max - z_min), evaluate_posed.hip:150-151 -- its flag, and
//              its row of the frame table: the pose transposed and rounded to fp32, the intrinsics, the scale, the far bound
//              s z_max + trunc and the four image-cone planes of the culling test
//   integrate  one launch for the whole batch.  A thread owns 4 consecutive x voxels (16-byte loads and stores on each of the five
//              planes) and keeps their 20 values in registers across the frame loop: the volume is read and written once per batch.
//              A wave owns a box of kBoxX x kBoxY x kBoxZ voxels; a block's four waves lie side by side in x (256 contiguous bytes per
//              row and plane).  Before it loads anything a wave tests the box's bounding sphere against every frame -- behind the
//              camera, beyond the far bound, outside the image cone -- and a wave no frame can touch loads and stores nothing.  The
//              test reads the frame table at wave-uniform addresses and branches the same way in every lane.  It is conservative: the
//              sphere is a voxel wider than the box (fp32 rounding of the test is orders below that for any grid whose voxels fp32 can
//              tell apart), the cone a pixel wider than the image (half for rint, half for the rounding of u and v), and every
//              plane's distance is scaled by the norm of its own normal, so a pose matrix that is no rotation is culled correctly
//              too.  ENDO_FUSION_NO_CULL turns the test off; the volume's bytes are the same either way.
//              The frames of a call are applied in order inside each thread: no atomics, the same bytes on every call.
//   count      one block per (k, j) row of voxels: the row's number of surface edges, by ballots (cloud_device.h), then the one-block
//              exclusive scan of the nz * ny counts; the total is left for the caller's one 8-byte read
//   extract    one block per row: rows (x, y, z, r, g, b) at the row's offset, voxels in i order and per voxel the edges +x, +y, +z,
//              ranked inside a chunk of 256 voxels by the three ballots
//   The volume, the edge test, the ranks and the row pass are in fusion_device.h: fusion_mesh.hip makes a triangle mesh of the same rows.
//
// numpy rounds every float32 operation on its own.  The file is compiled with -ffp-contract=off, as display.hip is, and the arithmetic
// the restatement shares is written with explicit-rounding intrinsics besides: a contracted multiply-add anywhere in the update would
// change the volume's bytes.
#include <cmath>

#include "cloud_device.h"
#include "common.h"
#include "fusion_device.h"

namespace endo {

constexpr int kFusionThreads = 256;
constexpr int kBoxX = 16, kBoxY = 4, kBoxZ = 4;          // a wave's box: 4 threads of 4 voxels in x, 4 rows, 4 slices
constexpr int kBlockX = kBoxX * (kFusionThreads / kWave);
constexpr int kFrameFloats = 32;                         // a row of the frame table
// half the diagonal between the box's outermost voxel centres, (7.5, 1.5, 1.5) voxels, plus one voxel
constexpr float kCullRadius = 8.8f;

static_assert(kBoxX * kBoxY * kBoxZ == 4 * kWave, "a lane owns four voxels");

enum FrameSlot {
    kRt = 0,            // [9] the rotation transposed
    kT = 9,             // [3]
    kFx = 12, kFy = 13, kCx = 14, kCy = 15,
    kScale = 16, kFar = 17,
    kCone = 18,         // [4] the slopes of the planes p_x <= a p_z (u high), p_x >= a p_z (u low), then the same for p_y (v)
    kConeNorm = 22,     // [4] the norms of their normals
    kZNorm = 26,        // the norm of the rotation's third column (p_z's gradient)
    kActive = 27,       // 1.0f: the frame contributes
};

// p_r = (Rt[r][0] d_x + Rt[r][1] d_y) + Rt[r][2] d_z
__device__ __forceinline__ float camera_coordinate(const float* rt, float dx, float dy, float dz) {
    return __fadd_rn(__fadd_rn(__fmul_rn(rt[0], dx), __fmul_rn(rt[1], dy)), __fmul_rn(rt[2], dz));
}

__global__ void __launch_bounds__(kFusionThreads) fusion_clear_kernel(FusionVolume q, int64_t quads) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kFusionThreads;
    float4* t = reinterpret_cast<float4*>(q.tsdf);
    float4* w = reinterpret_cast<float4*>(q.weight);
    float4* c = reinterpret_cast<float4*>(q.color);
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kFusionThreads + threadIdx.x; i < quads; i += stride) {
        t[i] = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        w[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        c[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        c[quads + i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        c[2 * quads + i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

struct FramesParams {
    const float* depth;           // [N][H][W]
    const float* boundaries;      // [N][H][W]
    const float* k;               // [N][3][3]
    const double* rotations;      // [N][3][3]
    const double* translations;   // [N][3]
    const float* scales;          // [N] or null
    int height, width;
    float trunc;
    float* table;                 // [N][kFrameFloats]
    int32_t* flags;               // [N]
};

__global__ void __launch_bounds__(kFusionThreads) fusion_frames_kernel(const FramesParams q) {
    __shared__ float s_min[kFusionThreads / kWave], s_max[kFusionThreads / kWave], s_raw[kFusionThreads / kWave];
    const int f = blockIdx.x;
    const int64_t pixels = static_cast<int64_t>(q.height) * q.width;
    const float* dep = q.depth + f * pixels;
    const float* bnd = q.boundaries + f * pixels;
    float zmin = INFINITY, zmax = -INFINITY, zraw = -INFINITY;          // zraw: of the depths the samples read (b = 1: zmax itself)
    for (int64_t i = threadIdx.x; i < pixels; i += kFusionThreads) {
        const float b = bnd[i];
        if (b > 0.5f) {
            const float d = __fmul_rn(b, dep[i]);
            zmin = fminf(zmin, d);
            zmax = fmaxf(zmax, d);
            zraw = fmaxf(zraw, dep[i]);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        zmin = fminf(zmin, __shfl_down(zmin, off, kWave));
        zmax = fmaxf(zmax, __shfl_down(zmax, off, kWave));
        zraw = fmaxf(zraw, __shfl_down(zraw, off, kWave));
    }
    if ((threadIdx.x & 63) == 0) {
        s_min[threadIdx.x >> 6] = zmin;
        s_max[threadIdx.x >> 6] = zmax;
        s_raw[threadIdx.x >> 6] = zraw;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    zmin = fminf(fminf(s_min[0], s_min[1]), fminf(s_min[2], s_min[3]));
    zmax = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    zraw = fmaxf(fmaxf(s_raw[0], s_raw[1]), fmaxf(s_raw[2], s_raw[3]));
    float* row = q.table + static_cast<int64_t>(f) * kFrameFloats;
    const double* rot = q.rotations + static_cast<int64_t>(f) * 9;
    const double* tr = q.translations + static_cast<int64_t>(f) * 3;
    float rt[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) rt[3 * r + c] = static_cast<float>(rot[3 * c + r]);
    const float* kf = q.k + static_cast<int64_t>(f) * 9;
    const float fx = kf[0], cx = kf[2], fy = kf[4], cy = kf[5];
    int flag = ENDO_FUSION_FRAME_OK;
    float scale = 0.0f;
    if (zmin > zmax) {
        flag = ENDO_FUSION_FRAME_EMPTY;
    } else if (q.scales) {
        scale = q.scales[f];
    } else if (zmin == zmax) {
        flag = ENDO_FUSION_FRAME_ZERO_RANGE;
    } else {
        scale = __fdiv_rn(20.0f, __fsub_rn(zmax, zmin));          // evaluate_posed.hip:150-151
    }
    if (flag == ENDO_FUSION_FRAME_OK && !(scale > 0.0f && scale < INFINITY)) flag = ENDO_FUSION_FRAME_BAD_SCALE;
    for (int i = 0; i < 9; ++i) row[kRt + i] = rt[i];
    for (int i = 0; i < 3; ++i) row[kT + i] = static_cast<float>(tr[i]);
    row[kFx] = fx; row[kFy] = fy; row[kCx] = cx; row[kCy] = cy;
    row[kScale] = scale;
    row[kFar] = __fadd_rn(__fmul_rn(scale, fmaxf(zmax, zraw)), q.trunc);
    // the image cone, a pixel wider than the image: u in [-1, W] <=> a_lo p_z <= p_x <= a_hi p_z for p_z > 0.  A focal length that is
    // not positive and finite gives slopes and norms whose test is never true (NaN or -inf on the left of its `>`).
    const bool fx_ok = fx > 0.0f && fx < INFINITY, fy_ok = fy > 0.0f && fy < INFINITY;
    const float a[4] = {fx_ok ? (static_cast<float>(q.width) - cx) / fx : INFINITY, fx_ok ? (-1.0f - cx) / fx : -INFINITY,
                        fy_ok ? (static_cast<float>(q.height) - cy) / fy : INFINITY, fy_ok ? (-1.0f - cy) / fy : -INFINITY};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float* r0 = rt + (i < 2 ? 0 : 3);
        const float n0 = r0[0] - a[i] * rt[6], n1 = r0[1] - a[i] * rt[7], n2 = r0[2] - a[i] * rt[8];
        row[kCone + i] = a[i];
        row[kConeNorm + i] = sqrtf(n0 * n0 + n1 * n1 + n2 * n2);
    }
    row[kZNorm] = sqrtf(rt[6] * rt[6] + rt[7] * rt[7] + rt[8] * rt[8]);
    row[kActive] = flag == ENDO_FUSION_FRAME_OK ? 1.0f : 0.0f;
    for (int i = kActive + 1; i < kFrameFloats; ++i) row[i] = 0.0f;
    q.flags[f] = flag;
}

struct IntegrateParams {
    FusionVolume vol;
    const float* depth;
    const float* boundaries;
    const uint8_t* colors;        // [N][H][W][3]
    const float* table;
    int frames, height, width, cull;
    float trunc, max_weight;
};

// can frame `fr` touch the sphere of radius r around the point whose camera coordinates are (px, py, pz)?  Every comparison is
// written so that a NaN keeps the frame.
__device__ __forceinline__ bool frame_touches(const float* fr, float px, float py, float pz, float r) {
    const float rz = r * fr[kZNorm];
    if (pz + rz <= 0.0f) return false;                        // behind the camera
    if (pz - rz > fr[kFar]) return false;                     // every sample occluded: sdf < -trunc
    if (px - fr[kCone + 0] * pz > r * fr[kConeNorm + 0]) return false;
    if (fr[kCone + 1] * pz - px > r * fr[kConeNorm + 1]) return false;
    if (py - fr[kCone + 2] * pz > r * fr[kConeNorm + 2]) return false;
    if (fr[kCone + 3] * pz - py > r * fr[kConeNorm + 3]) return false;
    return true;
}

__global__ void __launch_bounds__(kFusionThreads) fusion_integrate_kernel(const IntegrateParams q) {
    const FusionVolume& g = q.vol;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bx0 = blockIdx.x * kBlockX + wave * kBoxX, by0 = blockIdx.y * kBoxY, bz0 = blockIdx.z * kBoxZ;
    if (bx0 >= g.nx) return;          // (the whole wave)

    // the box's sphere against every frame: all of it from wave-uniform values
    const float r = kCullRadius * g.vs;
    const float mx = g.ox + static_cast<float>(bx0 + kBoxX / 2) * g.vs;
    const float my = g.oy + static_cast<float>(by0 + kBoxY / 2) * g.vs;
    const float mz = g.oz + static_cast<float>(bz0 + kBoxZ / 2) * g.vs;
    if (q.cull) {
        bool any = false;
        for (int f = 0; f < q.frames && !any; ++f) {
            const float* fr = q.table + static_cast<int64_t>(f) * kFrameFloats;
            if (fr[kActive] == 0.0f) continue;
            const float dx = mx - fr[kT], dy = my - fr[kT + 1], dz = mz - fr[kT + 2];
            any = frame_touches(fr, camera_coordinate(fr + kRt, dx, dy, dz), camera_coordinate(fr + kRt + 3, dx, dy, dz),
                                camera_coordinate(fr + kRt + 6, dx, dy, dz), r);
        }
        if (!any) return;
    }

    const int i0 = bx0 + (lane & 3) * 4, j = by0 + ((lane >> 2) & 3), k = bz0 + (lane >> 4);
    const bool inside = i0 < g.nx && j < g.ny && k < g.nz;          // (nx % 4 == 0: a thread's four voxels are inside together)
    const int64_t voxels = static_cast<int64_t>(g.nx) * g.ny * g.nz;
    const int64_t idx = (static_cast<int64_t>(k) * g.ny + j) * g.nx + i0;
    float t[4] = {1.0f, 1.0f, 1.0f, 1.0f}, w[4] = {0.0f, 0.0f, 0.0f, 0.0f}, col[3][4] = {};
    if (inside) {
        const float4 vt = *reinterpret_cast<const float4*>(g.tsdf + idx), vw = *reinterpret_cast<const float4*>(g.weight + idx);
        t[0] = vt.x; t[1] = vt.y; t[2] = vt.z; t[3] = vt.w;
        w[0] = vw.x; w[1] = vw.y; w[2] = vw.z; w[3] = vw.w;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float4 vc = *reinterpret_cast<const float4*>(g.color + c * voxels + idx);
            col[c][0] = vc.x; col[c][1] = vc.y; col[c][2] = vc.z; col[c][3] = vc.w;
        }
    }
    const float cy = voxel_centre(g.oy, j, g.vs), cz = voxel_centre(g.oz, k, g.vs);
    float cxs[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) cxs[e] = voxel_centre(g.ox, i0 + e, g.vs);
    const float wmax = static_cast<float>(q.width - 1), hmax = static_cast<float>(q.height - 1);
    const float neg_trunc = -q.trunc;
    const int64_t pixels = static_cast<int64_t>(q.height) * q.width;
    bool changed = false;

    for (int f = 0; f < q.frames; ++f) {
        const float* fr = q.table + static_cast<int64_t>(f) * kFrameFloats;
        if (fr[kActive] == 0.0f) continue;
        if (q.cull) {
            const float dx = mx - fr[kT], dy = my - fr[kT + 1], dz = mz - fr[kT + 2];
            if (!frame_touches(fr, camera_coordinate(fr + kRt, dx, dy, dz), camera_coordinate(fr + kRt + 3, dx, dy, dz),
                               camera_coordinate(fr + kRt + 6, dx, dy, dz), r))
                continue;
        }
        if (!inside) continue;
        const float fx = fr[kFx], fy = fr[kFy], pcx = fr[kCx], pcy = fr[kCy], s = fr[kScale];
        const float dy = __fsub_rn(cy, fr[kT + 1]), dz = __fsub_rn(cz, fr[kT + 2]);
        const float* dep = q.depth + f * pixels;
        const float* bnd = q.boundaries + f * pixels;
        const uint8_t* img = q.colors + f * pixels * 3;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float dx = __fsub_rn(cxs[e], fr[kT]);
            const float px = camera_coordinate(fr + kRt, dx, dy, dz);
            const float py = camera_coordinate(fr + kRt + 3, dx, dy, dz);
            const float pz = camera_coordinate(fr + kRt + 6, dx, dy, dz);
            const float u = rintf(__fadd_rn(__fmul_rn(fx, __fdiv_rn(px, pz)), pcx));
            const float v = rintf(__fadd_rn(__fmul_rn(fy, __fdiv_rn(py, pz)), pcy));
            if (!(pz > 0.0f && u >= 0.0f && u <= wmax && v >= 0.0f && v <= hmax)) continue;
            const int64_t pix = static_cast<int64_t>(static_cast<int>(v)) * q.width + static_cast<int>(u);
            if (!(bnd[pix] > 0.5f)) continue;
            const float z = dep[pix];
            if (!(z > 0.0f && z < INFINITY)) continue;
            const float sdf = __fsub_rn(__fmul_rn(s, z), pz);
            if (sdf < neg_trunc) continue;
            const float val = fminf(1.0f, __fdiv_rn(sdf, q.trunc));
            const float w0 = w[e], w1 = __fadd_rn(w0, 1.0f);
            t[e] = __fdiv_rn(__fadd_rn(__fmul_rn(t[e], w0), val), w1);
#pragma unroll
            for (int c = 0; c < 3; ++c)
                col[c][e] = __fdiv_rn(__fadd_rn(__fmul_rn(col[c][e], w0), static_cast<float>(img[pix * 3 + c])), w1);
            w[e] = fminf(w1, q.max_weight);
            changed = true;
        }
    }
    if (!changed) return;
    *reinterpret_cast<float4*>(g.tsdf + idx) = make_float4(t[0], t[1], t[2], t[3]);
    *reinterpret_cast<float4*>(g.weight + idx) = make_float4(w[0], w[1], w[2], w[3]);
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(g.color + c * voxels + idx) = make_float4(col[c][0], col[c][1], col[c][2], col[c][3]);
}

__global__ void __launch_bounds__(kCloudThreads) fusion_count_kernel(const ExtractParams q) {
    const int j = blockIdx.x, k = blockIdx.y;
    const int64_t row = static_cast<int64_t>(k) * q.vol.ny + j;
    int cnt = 0;
    for (int i = threadIdx.x; i < q.vol.nx; i += kCloudThreads) {
        float ta;
        const int edges = surface_edges(q, i, j, k, row * q.vol.nx + i, ta);
        cnt += cloud_wave_count(edges & 1) + cloud_wave_count(edges & 2) + cloud_wave_count(edges & 4);
    }
    cnt = cloud_block_count(cnt);
    if (threadIdx.x == 0) q.offsets[row] = cnt;
}

__global__ void __launch_bounds__(kScanThreads) fusion_scan_kernel(const ExtractParams q) {
    cloud_scan_block(q.offsets, 1, q.vol.ny * q.vol.nz, q.total);
}

__global__ void __launch_bounds__(kCloudThreads) fusion_write_kernel(const ExtractParams q) { fusion_write_rows<false>(q); }

}  // namespace endo

using namespace endo;

extern "C" int endo_fusion_tile(int which) {
    return which == 0 ? kBoxX : (which == 1 ? kBoxY : (which == 2 ? kBoxZ : ENDO_E_BADARG));
}

extern "C" int64_t endo_fusion_workspace_bytes(int frames, int height, int width) {
    if (!frames_sizes_ok(frames, height, width)) return -1;
    return align256(static_cast<int64_t>(frames) * kFrameFloats * static_cast<int64_t>(sizeof(float)));
}

extern "C" int64_t endo_fusion_extract_workspace_bytes(int nx, int ny, int nz) {
    if (!volume_sizes_ok(nx, ny, nz)) return -1;
    return align256(static_cast<int64_t>(ny) * nz * static_cast<int64_t>(sizeof(int64_t)));
}

extern "C" int endo_fusion_clear(int nx, int ny, int nz, float* tsdf, float* weight, float* color, void* stream_) {
    const double zero[3] = {0.0, 0.0, 0.0};
    FusionVolume g;
    if (!make_volume(zero, 1.0, nx, ny, nz, tsdf, weight, color, g)) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t quads = static_cast<int64_t>(nx) * ny * nz / 4;
    const int64_t blocks = (quads + kFusionThreads - 1) / kFusionThreads;
    ProfScope prof(kProfSmall, stream, 0.0, static_cast<double>(quads) * 80.0);
    fusion_clear_kernel<<<static_cast<unsigned>(blocks < 16384 ? blocks : 16384), kFusionThreads, 0, stream>>>(g, quads);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_fusion_integrate(const float* depth, const float* boundaries, const uint8_t* colors, const float* intrinsics,
                                     const double* rotations, const double* translations, const float* scales, int frames, int height,
                                     int width, const double* origin, double voxel_size, double truncation, float max_weight, int nx,
                                     int ny, int nz, float* tsdf, float* weight, float* color, int32_t* flags, int options,
                                     void* workspace, int64_t workspace_bytes, void* stream_) {
    if (!depth || !boundaries || !colors || !intrinsics || !rotations || !translations || !flags || !workspace) return ENDO_E_BADARG;
    if (options & ~ENDO_FUSION_NO_CULL) return ENDO_E_BADARG;
    const int64_t need = endo_fusion_workspace_bytes(frames, height, width);
    if (need < 0 || workspace_bytes < need) return ENDO_E_BADARG;
    IntegrateParams p;
    if (!make_volume(origin, voxel_size, nx, ny, nz, tsdf, weight, color, p.vol)) return ENDO_E_BADARG;
    const float trunc = static_cast<float>(truncation);
    if (!(trunc > 0.0f) || !std::isfinite(trunc) || !(max_weight >= 1.0f) || !std::isfinite(max_weight)) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    float* table = static_cast<float*>(workspace);
    const FramesParams fp{depth, boundaries, intrinsics, rotations, translations, scales, height, width, trunc, table, flags};
    p.depth = depth; p.boundaries = boundaries; p.colors = colors; p.table = table;
    p.frames = frames; p.height = height; p.width = width; p.cull = (options & ENDO_FUSION_NO_CULL) ? 0 : 1;
    p.trunc = trunc; p.max_weight = max_weight;
    const double voxels = static_cast<double>(nx) * ny * nz, pixels = static_cast<double>(frames) * height * width;
    ProfScope prof(kProfSmall, stream, 0.0, voxels * 40.0 + pixels * 11.0);          // (every box in view)
    fusion_frames_kernel<<<frames, kFusionThreads, 0, stream>>>(fp);
    ENDO_LAUNCH_CHECK();
    const dim3 grid((nx + kBlockX - 1) / kBlockX, (ny + kBoxY - 1) / kBoxY, (nz + kBoxZ - 1) / kBoxZ);
    fusion_integrate_kernel<<<grid, kFusionThreads, 0, stream>>>(p);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_fusion_count(const double* origin, double voxel_size, int nx, int ny, int nz, const float* tsdf, const float* weight,
                                 const float* color, float min_weight, int64_t* total, void* workspace, int64_t workspace_bytes,
                                 void* stream_) {
    ExtractParams q;
    const int err = extract_params(origin, voxel_size, nx, ny, nz, tsdf, weight, color, min_weight, total, workspace, workspace_bytes,
                                   endo_fusion_extract_workspace_bytes(nx, ny, nz), q);
    if (err) return err;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfSmall, stream, 0.0, static_cast<double>(nx) * ny * nz * 24.0);
    fusion_count_kernel<<<dim3(ny, nz), kCloudThreads, 0, stream>>>(q);
    ENDO_LAUNCH_CHECK();
    fusion_scan_kernel<<<1, kScanThreads, 0, stream>>>(q);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_fusion_extract(const double* origin, double voxel_size, int nx, int ny, int nz, const float* tsdf, const float* weight,
                                   const float* color, float min_weight, float* rows, int64_t capacity, int64_t* total, void* workspace,
                                   int64_t workspace_bytes, void* stream_) {
    ExtractParams q;
    const int err = extract_params(origin, voxel_size, nx, ny, nz, tsdf, weight, color, min_weight, total, workspace, workspace_bytes,
                                   endo_fusion_extract_workspace_bytes(nx, ny, nz), q);
    if (err) return err;
    if (capacity < 0 || (capacity > 0 && !rows)) return ENDO_E_BADARG;
    if (capacity == 0) return 0;
    q.rows = rows;
    q.capacity = capacity;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfSmall, stream, 0.0, static_cast<double>(nx) * ny * nz * 24.0 + static_cast<double>(capacity) * 48.0);
    fusion_write_kernel<<<dim3(ny, nz), kCloudThreads, 0, stream>>>(q);
    ENDO_LAUNCH_CHECK();
    return 0;
}
