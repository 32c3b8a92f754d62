// What the surface extraction of fusion.hip (points) and fusion_mesh.hip (a triangle mesh on the same points) share: the volume, which
// grid edges hold a surface point, their ranks inside a chunk of a voxel row, the rows themselves, and the argument checks of the
// entries.  Both files are compiled with -ffp-contract=off and every float operation here is an explicit-rounding intrinsic:
// tests/fusion_restate.py and tests/fusion_mesh_restate.py are the numpy float32 statements, matched bit for bit.
#pragma once

#include <cmath>

#include "cloud_device.h"
#include "common.h"

namespace endo {

constexpr int64_t kMaxVoxels = static_cast<int64_t>(1) << 40;

struct FusionVolume {
    float* tsdf;
    float* weight;
    float* color;          // [3][nz][ny][nx]
    int nx, ny, nz;
    float ox, oy, oz, vs;
};

__device__ __forceinline__ float voxel_centre(float o, int idx, float vs) {
    return __fadd_rn(o, __fmul_rn(__fadd_rn(static_cast<float>(idx), 0.5f), vs));
}

struct ExtractParams {
    FusionVolume vol;
    float min_weight;
    int64_t* offsets;          // [nz * ny] counts after the count kernel, exclusive offsets after the scan
    int64_t* total;            // [2]: 0, the total (cloud_scan_block's offsets of one group)
    float* rows;               // [capacity][6]
    int64_t capacity;
    float* normals;            // [capacity][3], the mesh's vertex pass only
};

// bit e of the result: the edge from voxel (i, j, k) to its +x (0), +y (1), +z (2) neighbour holds a surface point
__device__ __forceinline__ int surface_edges(const ExtractParams& q, int i, int j, int k, int64_t idx, float& ta) {
    const FusionVolume& g = q.vol;
    ta = g.tsdf[idx];
    if (!(g.weight[idx] >= q.min_weight)) return 0;
    const int64_t step[3] = {1, g.nx, static_cast<int64_t>(g.nx) * g.ny};
    const bool has[3] = {i + 1 < g.nx, j + 1 < g.ny, k + 1 < g.nz};
    int edges = 0;
#pragma unroll
    for (int e = 0; e < 3; ++e)
        if (has[e] && g.weight[idx + step[e]] >= q.min_weight && (ta < 0.0f) != (g.tsdf[idx + step[e]] < 0.0f)) edges |= 1 << e;
    return edges;
}

// cloud_chunk_rank for up to three rows per thread: the rank of this thread's first row among the rows of a chunk of kCloudThreads
// voxels, voxel by voxel and +x, +y, +z inside a voxel, and the chunk's number of rows.  Every thread of the block calls.
__device__ __forceinline__ int edge_chunk_rank(int edges, int& total) {
    __shared__ int s_wave[kCloudThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bx = __ballot(edges & 1), by = __ballot(edges & 2), bz = __ballot(edges & 4);
    if (lane == 0) s_wave[wave] = __popcll(bx) + __popcll(by) + __popcll(bz);
    __syncthreads();
    const unsigned long long lower = (1ull << lane) - 1ull;
    int rank = __popcll(bx & lower) + __popcll(by & lower) + __popcll(bz & lower);
    for (int i = 0; i < wave; ++i) rank += s_wave[i];
    total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
    return rank;
}

// The tsdf's central difference at a voxel without its division, g_x = t[min(i + 1, nx - 1)] - t[max(i - 1, 0)] and likewise g_y, g_z:
// neighbours as they stand, whatever their weight (an unobserved voxel holds 1, free space).
__device__ __forceinline__ void tsdf_gradient(const FusionVolume& g, int i, int j, int k, int64_t idx, float out[3]) {
    const int64_t sy = g.nx, sz = static_cast<int64_t>(g.nx) * g.ny;
    out[0] = __fsub_rn(g.tsdf[idx + (i + 1 < g.nx ? 1 : 0)], g.tsdf[idx - (i > 0 ? 1 : 0)]);
    out[1] = __fsub_rn(g.tsdf[idx + (j + 1 < g.ny ? sy : 0)], g.tsdf[idx - (j > 0 ? sy : 0)]);
    out[2] = __fsub_rn(g.tsdf[idx + (k + 1 < g.nz ? sz : 0)], g.tsdf[idx - (k > 0 ? sz : 0)]);
}

// The write pass of one (k, j) row of voxels, by its block: rows (x, y, z, r, g, b) at the row's offset, voxels in i order and per
// voxel the edges +x, +y, +z, ranked inside a chunk of kCloudThreads voxels by the three ballots.  kNormals: each row's unit normal
// as well, the gradients of the edge's two voxels interpolated with the row's own lambda, (0, 0, 0) where its length is 0 or not finite.
template <bool kNormals>
__device__ __forceinline__ void fusion_write_rows(const ExtractParams& q) {
    const FusionVolume& g = q.vol;
    const int j = blockIdx.x, k = blockIdx.y;
    const int64_t row = static_cast<int64_t>(k) * g.ny + j;
    const int64_t voxels = static_cast<int64_t>(g.nx) * g.ny * g.nz;
    const int64_t step[3] = {1, g.nx, static_cast<int64_t>(g.nx) * g.ny};
    int64_t at = q.offsets[row];
    for (int i0 = 0; i0 < g.nx; i0 += kCloudThreads) {
        const int i = i0 + threadIdx.x;
        const int64_t idx = row * g.nx + i;
        float ta = 0.0f;
        const int edges = i < g.nx ? surface_edges(q, i, j, k, idx, ta) : 0;
        int total;
        int rank = edge_chunk_rank(edges, total);
        if (edges) {
            const float c[3] = {voxel_centre(g.ox, i, g.vs), voxel_centre(g.oy, j, g.vs), voxel_centre(g.oz, k, g.vs)};
            const float ca[3] = {g.color[idx], g.color[voxels + idx], g.color[2 * voxels + idx]};
            float ga[3] = {0.0f, 0.0f, 0.0f};
            if (kNormals) tsdf_gradient(g, i, j, k, idx, ga);
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                if (!(edges & (1 << e))) continue;
                const int64_t nb = idx + step[e];
                const float lambda = __fdiv_rn(ta, __fsub_rn(ta, g.tsdf[nb]));
                const int64_t dst = at + rank;
                ++rank;
                if (dst >= q.capacity) continue;          // (a caller that allocated fewer rows than the count: nothing outside them)
                float* o = q.rows + dst * 6;
#pragma unroll
                for (int a = 0; a < 3; ++a) o[a] = a == e ? __fadd_rn(c[a], __fmul_rn(lambda, g.vs)) : c[a];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {          // r, g, b = channels 2, 1, 0, as the posed writer reads them
                    const float cb = g.color[(2 - ch) * voxels + nb];
                    o[3 + ch] = rintf(__fadd_rn(ca[2 - ch], __fmul_rn(lambda, __fsub_rn(cb, ca[2 - ch]))));
                }
                if (kNormals) {
                    float gb[3], v[3];
                    tsdf_gradient(g, i + (e == 0), j + (e == 1), k + (e == 2), nb, gb);
#pragma unroll
                    for (int a = 0; a < 3; ++a) v[a] = __fadd_rn(ga[a], __fmul_rn(lambda, __fsub_rn(gb[a], ga[a])));
                    // (sqrtf is the correctly rounded square root; __fsqrt_rn is the native one, an ulp off in one row of seven)
                    const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(v[0], v[0]), __fmul_rn(v[1], v[1])), __fmul_rn(v[2], v[2])));
                    const bool unit = len > 0.0f && len < INFINITY;
#pragma unroll
                    for (int a = 0; a < 3; ++a) q.normals[dst * 3 + a] = unit ? __fdiv_rn(v[a], len) : 0.0f;
                }
            }
        }
        at += total;
    }
}

inline bool volume_sizes_ok(int nx, int ny, int nz) {
    if (nx <= 0 || ny <= 0 || nz <= 0 || nx % 4 != 0) return false;
    if (ny > 65535 || nz > 65535) return false;          // the (y, z) grid of the row kernels
    return static_cast<int64_t>(nx) * ny * nz <= kMaxVoxels;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline bool make_volume(const double* origin, double voxel_size, int nx, int ny, int nz, float* tsdf, float* weight, float* color,
                        FusionVolume& g) {
    if (!origin || !tsdf || !weight || !color || !volume_sizes_ok(nx, ny, nz)) return false;
    if (!aligned16(tsdf) || !aligned16(weight) || !aligned16(color)) return false;
    if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2])) return false;
    const float vs = static_cast<float>(voxel_size);
    if (!(vs > 0.0f) || !std::isfinite(vs)) return false;
    g = FusionVolume{tsdf, weight, color, nx, ny, nz, static_cast<float>(origin[0]), static_cast<float>(origin[1]),
                     static_cast<float>(origin[2]), vs};
    return std::isfinite(g.ox) && std::isfinite(g.oy) && std::isfinite(g.oz);
}

// the arguments the count and the write entries share, into q (rows, normals and capacity left empty); `needed`: the workspace's bytes
inline int extract_params(const double* origin, double voxel_size, int nx, int ny, int nz, const float* tsdf, const float* weight,
                          const float* color, float min_weight, int64_t* total, void* workspace, int64_t workspace_bytes, int64_t needed,
                          ExtractParams& q) {
    if (!total || !workspace || std::isnan(min_weight)) return ENDO_E_BADARG;
    if (!make_volume(origin, voxel_size, nx, ny, nz, const_cast<float*>(tsdf), const_cast<float*>(weight), const_cast<float*>(color), q.vol))
        return ENDO_E_BADARG;
    if (workspace_bytes < needed) return ENDO_E_BADARG;
    q.min_weight = min_weight;
    q.offsets = static_cast<int64_t*>(workspace);
    q.total = total;
    q.rows = nullptr;
    q.capacity = 0;
    q.normals = nullptr;
    return 0;
}

}  // namespace endo
