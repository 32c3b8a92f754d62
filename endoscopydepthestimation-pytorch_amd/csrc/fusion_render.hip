// The fused TSDF volume seen from a pose: one ray per pixel marched through the volume of fusion.hip to the first zero crossing of the
// trilinear tsdf, with the surface's depth, colour and normal there.  The reference has no code for this step;
// tests/fusion_render_restate.py is the numpy float32 statement every output is held to, bit for bit, and include/endo_hip.h
// (endo_fusion_render) states the order of the operations.
//
//   marks    one block per (y, z) row of bricks.  A brick is kBrick^3 cells -- the cells whose base voxel lies in it -- so it covers
//            (kBrick + 1)^3 voxels, one voxel of overlap with its +x, +y, +z neighbours: a cell then needs ONE mark, its base voxel's.
//            The mark: the brick holds a voxel with weight >= min_weight and tsdf <= 0.  The block walks the row in x, 81 coalesced
//            voxel rows per chunk of 31 bricks, a thread per x column, and ORs nine columns per brick through LDS.
//   march    a wave owns an 8 x 8 tile of pixels, a block 16 x 16: neighbouring rays read neighbouring cells, so a wave's 8 x 64
//            corner loads fall into a few dozen 128-byte lines instead of 512.  A ray takes its samples t_k = k dt in order, k clipped
//            to its passage through the grid (slabs a voxel wider than the grid, two samples of margin: samples outside the grid are
//            invalid anyway).  Per sample: the cell; its brick's mark -- a byte from a table of 32 KB at 256^3, which stays in the
//            vector L1 -- and only for a marked brick the eight tsdf values, and only for f <= 0 the eight weights; in an unmarked
//            brick the ray jumps to just before the brick's far face instead of asking for the same mark again.  The ending sample
//            found, sample k - 1 is evaluated (skipped or not, it is needed now: the rule of the header), and on a hit both samples
//            once more in full: gradients from the eight values held, the three colour planes.  So the march itself carries a dozen
//            registers across its loop and every wave fetches 3 planes only at its 2 bracketing samples.
//            ENDO_FUSION_NO_SKIP marches without the marks (and without their launch); the bytes are the same either way.
//
// numpy rounds every float32 operation on its own.  The file is compiled with -ffp-contract=off, as fusion.hip is, and the arithmetic
// the restatement shares is written with explicit-rounding intrinsics besides (the sampler: fusion_sample_device.h).  What is NOT shared, and need not be: the clip of k,
// which only has to be conservative.
#include <cmath>

#include "common.h"
#include "fusion_device.h"
#include "fusion_sample_device.h"

namespace endo {

constexpr int kBrick = 8;                                  // cells per brick and axis
constexpr int kMarkThreads = 256;
constexpr int kMarkBricks = (kMarkThreads - 1) / kBrick;   // bricks per chunk of a row: 31, over 31 * 8 + 1 = 249 columns
constexpr int kTile = 8;                                   // a wave's pixel tile: kTile x kTile
constexpr int kRenderThreads = 256;
constexpr int kBlockTile = 2 * kTile;                      // a block's: 2 x 2 waves
constexpr int kMaxSamples = 1 << 20;

static_assert(kTile * kTile == kWave && kRenderThreads == 4 * kWave, "a lane owns one pixel, a block 2 x 2 tiles");
static_assert(kMarkBricks * kBrick + 1 <= kMarkThreads, "a thread per column of a chunk");

inline int brick_count(int n) { return (n + kBrick - 1) / kBrick; }

__global__ void __launch_bounds__(kMarkThreads) fusion_render_mark_kernel(const FusionVolume g, float min_weight, uint8_t* marks, int nbx,
                                                                          int nby) {
    __shared__ int s_column[kMarkThreads];
    const int by = blockIdx.x, bz = blockIdx.y;
    const int y0 = by * kBrick, z0 = bz * kBrick;
    const int y1 = min(y0 + kBrick, g.ny - 1), z1 = min(z0 + kBrick, g.nz - 1);          // inclusive: the overlap voxel
    const int64_t sy = g.nx, sz = static_cast<int64_t>(g.nx) * g.ny;
    for (int b0 = 0; b0 < nbx; b0 += kMarkBricks) {
        const int x = b0 * kBrick + threadIdx.x;
        int any = 0;
        if (threadIdx.x <= kMarkBricks * kBrick && x < g.nx) {
            for (int z = z0; z <= z1; ++z)
                for (int y = y0; y <= y1; ++y) {
                    const int64_t idx = z * sz + y * sy + x;
                    any |= (g.weight[idx] >= min_weight && g.tsdf[idx] <= 0.0f) ? 1 : 0;
                }
        }
        s_column[threadIdx.x] = any;
        __syncthreads();
        if (threadIdx.x < kMarkBricks && b0 + threadIdx.x < nbx) {
            int mark = 0;
#pragma unroll
            for (int e = 0; e <= kBrick; ++e) mark |= s_column[threadIdx.x * kBrick + e];
            marks[(static_cast<int64_t>(bz) * nby + by) * nbx + b0 + threadIdx.x] = static_cast<uint8_t>(mark);
        }
        __syncthreads();
    }
}

struct RenderParams {
    FusionVolume vol;
    const float* k;               // [N][3][3]
    const double* rotations;      // [N][3][3]
    const double* translations;   // [N][3]
    const float* scales;          // [N] or null
    const float* boundaries;      // [N][H][W] or null
    const uint8_t* marks;         // [nbz][nby][nbx] or null (no skipping)
    int nbx, nby;
    int height, width;
    float min_weight, step_length, inv_vs;          // step * vs; 1 / vs
    float* depth;                 // [N][H][W]
    float* mask;                  // [N][H][W]
    uint8_t* colors;              // [N][H][W][3]
    float* normals;               // [N][H][W][3]
};

struct Ray {
    float t[3], w[3], dt;         // x(t) = t + t_k w
    float pace[3];                // samples per cell along each axis, 1 / |dt w_a / vs| (the brick jump's; no part of the contract)
};

// the cell of sample n; false: a corner outside the grid
__device__ __forceinline__ bool locate(const FusionVolume& g, float inv_vs, const Ray& ray, int n, Cell& c) {
    const float tk = __fmul_rn(static_cast<float>(n), ray.dt);
    float x[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = __fadd_rn(ray.t[a], __fmul_rn(tk, ray.w[a]));
    return locate_point(g, inv_vs, x, c);
}

// the samples first..last the ray can have inside the grid, conservatively; false: none
__device__ __forceinline__ bool clip_samples(const FusionVolume& g, const Ray& ray, int& first, int& last) {
    if (!(ray.dt > 0.0f && ray.dt < INFINITY)) return false;
    const float o[3] = {g.ox, g.oy, g.oz};
    const int dims[3] = {g.nx, g.ny, g.nz};
    float lo = 0.0f, hi = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(fabsf(ray.w[a]) < INFINITY && fabsf(ray.t[a]) < INFINITY)) return false;          // every x is NaN or infinite: outside
        const float low = o[a] - g.vs, high = o[a] + static_cast<float>(dims[a] + 1) * g.vs;
        if (ray.w[a] == 0.0f) {
            if (!(ray.t[a] >= low && ray.t[a] <= high)) return false;
        } else {
            const float t1 = (low - ray.t[a]) / ray.w[a], t2 = (high - ray.t[a]) / ray.w[a];
            lo = fmaxf(lo, fminf(t1, t2));
            hi = fminf(hi, fmaxf(t1, t2));
        }
    }
    if (!(lo <= hi)) return false;
    const float cap = static_cast<float>(kMaxSamples);
    first = static_cast<int>(fminf(fmaxf(floorf(lo / ray.dt) - 2.0f, 1.0f), cap + 1.0f));
    last = static_cast<int>(fminf(fmaxf(ceilf(hi / ray.dt) + 2.0f, 0.0f), cap));
    return first <= last;
}

// In an unmarked brick: how many of the NEXT samples still have their cell's base voxel in this brick, conservatively -- they would
// each find the same mark.  Per axis the cells to the face the ray moves towards, less kJumpSlack, times the samples per cell; one
// sample less than that.  The slack covers what fp32 can move a sample's grid coordinate by (2^-23 of its coordinate in cells: grids
// up to 10^5 cells from the origin), the lost sample the rounding of the product.  A ray that does not move gets the cap.
constexpr float kJumpSlack = 0.015625f;
__device__ __forceinline__ int samples_to_leave(const Ray& ray, const Cell& c) {
    const int base[3] = {c.i, c.j, c.k};
    float samples = 1048576.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float in_brick = static_cast<float>(base[a] % kBrick) + c.r[a];          // [0, kBrick)
        const float cells = (ray.w[a] > 0.0f ? static_cast<float>(kBrick) - in_brick : in_brick) - kJumpSlack;
        samples = fminf(samples, cells * ray.pace[a]);          // (0 * inf = NaN: the axis does not bound)
    }
    return samples >= 2.0f ? static_cast<int>(samples) - 1 : 0;
}

__global__ void __launch_bounds__(kRenderThreads) fusion_render_kernel(const RenderParams q) {
    const FusionVolume& g = q.vol;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = blockIdx.x * kBlockTile + (wave & 1) * kTile + (lane & (kTile - 1));
    const int v = blockIdx.y * kBlockTile + (wave >> 1) * kTile + lane / kTile;
    const int f = blockIdx.z;
    if (u >= q.width || v >= q.height) return;
    const int64_t pix = (static_cast<int64_t>(f) * q.height + v) * q.width + u;
    float depth = 0.0f, hit = 0.0f, normal[3] = {0.0f, 0.0f, 0.0f};
    uint8_t color[3] = {0, 0, 0};

    const float scale = q.scales ? q.scales[f] : 1.0f;
    const bool cast = scale > 0.0f && scale < INFINITY && (!q.boundaries || q.boundaries[pix] > 0.5f);
    Ray ray;
    int first = 0, last = -1;
    if (cast) {
        const float* kf = q.k + static_cast<int64_t>(f) * 9;
        const double* rot = q.rotations + static_cast<int64_t>(f) * 9;
        const double* tr = q.translations + static_cast<int64_t>(f) * 3;
        const float dx = __fdiv_rn(__fsub_rn(static_cast<float>(u), kf[2]), kf[0]);
        const float dy = __fdiv_rn(__fsub_rn(static_cast<float>(v), kf[5]), kf[4]);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            ray.t[a] = static_cast<float>(tr[a]);
            ray.w[a] = __fadd_rn(__fadd_rn(__fmul_rn(static_cast<float>(rot[3 * a]), dx), __fmul_rn(static_cast<float>(rot[3 * a + 1]), dy)),
                                 static_cast<float>(rot[3 * a + 2]));
        }
        ray.dt = __fdiv_rn(q.step_length, sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), 1.0f)));
        if (!clip_samples(g, ray, first, last)) last = -1;
#pragma unroll
        for (int a = 0; a < 3; ++a) ray.pace[a] = 1.0f / fabsf(ray.dt * ray.w[a] * q.inv_vs);
    }

    // the first valid sample with f <= 0
    int end = 0;
    Cell cb;
    for (int n = first; n <= last; ++n) {
        if (!locate(g, q.inv_vs, ray, n, cb)) continue;
        if (q.marks && !q.marks[(static_cast<int64_t>(cb.k / kBrick) * q.nby + cb.j / kBrick) * q.nbx + cb.i / kBrick]) {
            n += samples_to_leave(ray, cb);
            continue;
        }
        if (!(trilinear(g.tsdf, g, cb) <= 0.0f)) continue;
        if (!weights_ok(g, cb, q.min_weight)) continue;
        end = n;
        break;
    }
    Cell ca;
    if (end > 1 && locate(g, q.inv_vs, ray, end - 1, ca) && weights_ok(g, ca, q.min_weight)) {
        float ga[3], gb[3];
        const float fa = trilinear_gradient(g, ca, ga);
        if (fa > 0.0f) {
            const float fb = trilinear_gradient(g, cb, gb);
            const float lambda = __fdiv_rn(fa, __fsub_rn(fa, fb));
            const float ts = __fadd_rn(__fmul_rn(static_cast<float>(end - 1), ray.dt), __fmul_rn(lambda, ray.dt));
            depth = __fdiv_rn(ts, scale);
            hit = 1.0f;
            const int64_t voxels = static_cast<int64_t>(g.nx) * g.ny * g.nz;
            float nv[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float* plane = g.color + a * voxels;
                const float blended = rintf(lerp_rn(trilinear(plane, g, ca), trilinear(plane, g, cb), lambda));
                color[a] = static_cast<uint8_t>(fminf(fmaxf(blended, 0.0f), 255.0f));          // (a NaN: 0)
                nv[a] = lerp_rn(ga[a], gb[a], lambda);
            }
            const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(nv[0], nv[0]), __fmul_rn(nv[1], nv[1])), __fmul_rn(nv[2], nv[2])));
            const bool unit = len > 0.0f && len < INFINITY;
#pragma unroll
            for (int a = 0; a < 3; ++a) normal[a] = unit ? __fdiv_rn(nv[a], len) : 0.0f;
        }
    }
    q.depth[pix] = depth;
    q.mask[pix] = hit;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        q.colors[pix * 3 + a] = color[a];
        q.normals[pix * 3 + a] = normal[a];
    }
}

}  // namespace endo

using namespace endo;

extern "C" int endo_fusion_render_tile(int which) {
    return which == 0 || which == 1 ? kTile : (which >= 2 && which <= 4 ? kBrick : ENDO_E_BADARG);
}

extern "C" int64_t endo_fusion_render_workspace_bytes(int frames, int height, int width, int nx, int ny, int nz) {
    if (!frames_sizes_ok(frames, height, width) || !volume_sizes_ok(nx, ny, nz) || nx > kMaxAxis) return -1;
    if (height > 65535 * kBlockTile) return -1;          // the (x, y, frame) grid of the march
    return align256(static_cast<int64_t>(brick_count(nx)) * brick_count(ny) * brick_count(nz));
}

extern "C" int endo_fusion_render(const double* origin, double voxel_size, double truncation, int nx, int ny, int nz, const float* tsdf,
                                  const float* weight, const float* color, const float* intrinsics, const double* rotations,
                                  const double* translations, const float* scales, const float* boundaries, int frames, int height,
                                  int width, float min_weight, float step, int options, float* depth, float* mask, uint8_t* colors,
                                  float* normals, void* workspace, int64_t workspace_bytes, void* stream_) {
    if (!intrinsics || !rotations || !translations || !depth || !mask || !colors || !normals || !workspace) return ENDO_E_BADARG;
    if (options & ~ENDO_FUSION_NO_SKIP) return ENDO_E_BADARG;
    if (std::isnan(min_weight)) return ENDO_E_BADARG;
    const int64_t need = endo_fusion_render_workspace_bytes(frames, height, width, nx, ny, nz);
    if (need < 0 || workspace_bytes < need) return ENDO_E_BADARG;
    RenderParams p;
    if (!make_volume(origin, voxel_size, nx, ny, nz, const_cast<float*>(tsdf), const_cast<float*>(weight), const_cast<float*>(color), p.vol))
        return ENDO_E_BADARG;
    const float trunc = static_cast<float>(truncation);
    if (!(trunc > 0.0f) || !std::isfinite(trunc)) return ENDO_E_BADARG;
    const float step_length = step * p.vol.vs;          // (-ffp-contract=off: one rounding, the restatement's)
    if (!(step > 0.0f) || !(step_length > 0.0f) || !(step_length <= trunc)) return ENDO_E_BADARG;
    // a ray's samples inside the grid: the diagonal, bounded by the three sides, in steps
    if ((static_cast<double>(nx) + ny + nz + 6.0) / static_cast<double>(step) > static_cast<double>(kMaxSamples)) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const bool skip = !(options & ENDO_FUSION_NO_SKIP);
    p.k = intrinsics; p.rotations = rotations; p.translations = translations; p.scales = scales; p.boundaries = boundaries;
    p.marks = skip ? static_cast<const uint8_t*>(workspace) : nullptr;
    p.nbx = brick_count(nx); p.nby = brick_count(ny);
    p.height = height; p.width = width;
    p.min_weight = min_weight; p.step_length = step_length; p.inv_vs = 1.0f / p.vol.vs;
    p.depth = depth; p.mask = mask; p.colors = colors; p.normals = normals;
    const double voxels = static_cast<double>(nx) * ny * nz, pixels = static_cast<double>(frames) * height * width;
    ProfScope prof(kProfSmall, stream, 0.0, (skip ? voxels * 8.0 : 0.0) + pixels * 23.0);          // (the marks' pass and the outputs)
    if (skip) {
        fusion_render_mark_kernel<<<dim3(p.nby, brick_count(nz)), kMarkThreads, 0, stream>>>(p.vol, min_weight,
                                                                                             static_cast<uint8_t*>(workspace), p.nbx, p.nby);
        ENDO_LAUNCH_CHECK();
    }
    const dim3 grid((width + kBlockTile - 1) / kBlockTile, (height + kBlockTile - 1) / kBlockTile, frames);
    fusion_render_kernel<<<grid, kRenderThreads, 0, stream>>>(p);
    ENDO_LAUNCH_CHECK();
    return 0;
}
