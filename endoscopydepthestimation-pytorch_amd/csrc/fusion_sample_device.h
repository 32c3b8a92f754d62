// The trilinear sampler of the TSDF volume, shared by fusion_render.hip (a ray's samples) and fusion_track.hip (a depth map's
// back-projected pixels): the cell of a point, the interpolant's value and gradient over it, and the eight-weights rule of a cell.
// Both files are compiled with -ffp-contract=off and every float operation here is an explicit-rounding intrinsic:
// tests/fusion_render_restate.py (_locate, _value, _value_gradient, _weights_ok) is the numpy float32 statement, matched bit for bit.
#pragma once

#include "common.h"
#include "fusion_device.h"

namespace endo {

constexpr int kMaxAxis = 1 << 24;                          // float(index) exact

struct Cell {
    int64_t idx;                  // of its base voxel
    int i, j, k;
    float r[3];
};

__device__ __forceinline__ float lerp_rn(float a, float b, float r) { return __fadd_rn(a, __fmul_rn(r, __fsub_rn(b, a))); }

// the cell of the point x: g_a = (x_a - origin_a) inv_vs - 0.5, base floor(g_a), fraction g_a - base; false: a corner outside the grid
__device__ __forceinline__ bool locate_point(const FusionVolume& g, float inv_vs, const float x[3], Cell& c) {
    const float o[3] = {g.ox, g.oy, g.oz};
    const int dims[3] = {g.nx, g.ny, g.nz};
    float base[3];
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float gc = __fsub_rn(__fmul_rn(__fsub_rn(x[a], o[a]), inv_vs), 0.5f);
        base[a] = floorf(gc);
        c.r[a] = __fsub_rn(gc, base[a]);
        inside = inside && base[a] >= 0.0f && base[a] <= static_cast<float>(dims[a] - 2);          // (a NaN is outside)
    }
    if (!inside) return false;
    c.i = static_cast<int>(base[0]);
    c.j = static_cast<int>(base[1]);
    c.k = static_cast<int>(base[2]);
    c.idx = (static_cast<int64_t>(c.k) * g.ny + c.j) * g.nx + c.i;
    return true;
}

// the trilinear value of plane p over the cell: along x, then y, then z
__device__ __forceinline__ float trilinear(const float* p, const FusionVolume& g, const Cell& c) {
    const int64_t sy = g.nx, sz = static_cast<int64_t>(g.nx) * g.ny;
    const float* v = p + c.idx;
    const float a00 = lerp_rn(v[0], v[1], c.r[0]), a10 = lerp_rn(v[sy], v[sy + 1], c.r[0]);
    const float a01 = lerp_rn(v[sz], v[sz + 1], c.r[0]), a11 = lerp_rn(v[sz + sy], v[sz + sy + 1], c.r[0]);
    return lerp_rn(lerp_rn(a00, a10, c.r[1]), lerp_rn(a01, a11, c.r[1]), c.r[2]);
}

// the same value of the tsdf with the gradient of the interpolant (per voxel, not per unit length) from the differences it forms
__device__ __forceinline__ float trilinear_gradient(const FusionVolume& g, const Cell& c, float grad[3]) {
    const int64_t sy = g.nx, sz = static_cast<int64_t>(g.nx) * g.ny;
    const float* v = g.tsdf + c.idx;
    const float rx = c.r[0], ry = c.r[1], rz = c.r[2];
    const float d00 = __fsub_rn(v[1], v[0]), d10 = __fsub_rn(v[sy + 1], v[sy]);
    const float d01 = __fsub_rn(v[sz + 1], v[sz]), d11 = __fsub_rn(v[sz + sy + 1], v[sz + sy]);
    const float a00 = __fadd_rn(v[0], __fmul_rn(rx, d00)), a10 = __fadd_rn(v[sy], __fmul_rn(rx, d10));
    const float a01 = __fadd_rn(v[sz], __fmul_rn(rx, d01)), a11 = __fadd_rn(v[sz + sy], __fmul_rn(rx, d11));
    grad[0] = lerp_rn(lerp_rn(d00, d10, ry), lerp_rn(d01, d11, ry), rz);
    const float e0 = __fsub_rn(a10, a00), e1 = __fsub_rn(a11, a01);
    const float b0 = __fadd_rn(a00, __fmul_rn(ry, e0)), b1 = __fadd_rn(a01, __fmul_rn(ry, e1));
    grad[1] = lerp_rn(e0, e1, rz);
    grad[2] = __fsub_rn(b1, b0);
    return __fadd_rn(b0, __fmul_rn(rz, grad[2]));
}

// the cell rule of endo_fusion_mesh_count: all eight voxels of the cell have weight >= min_weight
__device__ __forceinline__ bool weights_ok(const FusionVolume& g, const Cell& c, float min_weight) {
    const int64_t sy = g.nx, sz = static_cast<int64_t>(g.nx) * g.ny;
    const float* w = g.weight + c.idx;
    return w[0] >= min_weight && w[1] >= min_weight && w[sy] >= min_weight && w[sy + 1] >= min_weight && w[sz] >= min_weight &&
           w[sz + 1] >= min_weight && w[sz + sy] >= min_weight && w[sz + sy + 1] >= min_weight;
}

}  // namespace endo
