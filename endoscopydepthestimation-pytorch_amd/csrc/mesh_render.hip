// A triangle mesh seen from a pose: the ray through every pixel centre against the triangles, the nearest hit kept, with its depth,
// triangle, barycentric coordinates, face normal and colour.  What the CT model -- the reference's yardstick, its README, step 4 -- looks
// like from a frame's camera.  The reference has no code for this step; tests/mesh_render_restate.py is the numpy float32 statement every
// output is held to, bit for bit, and include/endo_hip.h (endo_mesh_render) states the order of the operations.
//
//   clear     a 64-bit key per pixel to "no hit", the queue's count to 0, the frames' flags
//   setup     a thread per (frame, triangle): the three vertices in camera coordinates and a conservative box of the pixels whose ray can
//             pass the test (the span rule of the header makes that a statement about float numbers, not about exact geometry).  A
//             triangle behind the camera or with an empty box is done; a box of at most kSmallBox pixels is tested in place; any other is
//             appended to the queue (one wave-wide atomic add per wave; the order of the entries varies, the result does not).  A
//             triangle with a vertex that is not in front of the camera has no projection: its box is the image.
//   queue     a wave per queued (frame, triangle), kTile x kTile pixels of its box per step, a lane per pixel; the waves of a fixed grid
//             stride over the entries, whose count each reads once
//   resolve   a thread per pixel: the winning key's triangle once more, in full, for the outputs
//
// Hits meet in the keys by a 64-bit atomic minimum in HBM: (bits of t) << 32 | face.  t is finite and > 0, so its bits order as t does:
// the minimum is the nearest hit and of equal t the lowest face, whatever the order of arrival.  A lane reads the key first and leaves
// the atomic out when it cannot win: keys only fall, so a stale value only errs towards trying.
// ENDO_MESH_BRUTE gives every triangle the whole image as its box and drops no triangle but those with an index out of range; the
// bytes are the same either way.
//
// numpy rounds every float32 operation on its own: the file is compiled with -ffp-contract=off and the shared arithmetic is written with
// explicit-rounding intrinsics besides.  f(P, Q) = P_x Q_y - P_y Q_x from two rounded products gives f(Q, P) = -f(P, Q) exactly, which a
// fused multiply-add would break: two triangles on one edge must see the same magnitude there.
#include <cmath>

#include "common.h"

namespace endo {

constexpr int kTile = 8;                 // the queue pass: a wave's pixels per step, kTile x kTile
constexpr int kSmallBox = 16;            // boxes of at most this many pixels are tested by the setup thread itself
constexpr int kThreads = 256;
constexpr int kQueueBlocksPerCu = 4;

static_assert(kTile * kTile == kWave, "a lane per pixel of a tile");

struct MeshParams {
    const float* vertices;        // [V][stride]
    int64_t stride;
    int vertex_count;
    const int32_t* faces;         // [T][3]
    int triangles;
    const float* k;               // [N][3][3]
    const double* rotations;      // [N][3][3]
    const double* translations;   // [N][3]
    const float* scales;          // [N] or null
    const float* boundaries;      // [N][H][W] or null
    int frames, height, width, options;
    unsigned long long* keys;     // [N][H][W]
    unsigned long long* queue_count;
    unsigned long long* queue;    // [N * T]: frame << 32 | triangle
    float* depth;
    float* mask;
    int32_t* triangle;
    float* barycentric;
    float* normals;
    uint8_t* colors;
    int32_t* flags;
};

constexpr unsigned long long kNoHit = ~0ull;

struct Frame {
    float r[9], t[3], fx, cx, fy, cy;
};

__device__ __forceinline__ bool scale_ok(float s) { return s > 0.0f && s < INFINITY; }

__device__ __forceinline__ Frame load_frame(const MeshParams& q, int f) {
    Frame fr;
    const double* rot = q.rotations + static_cast<int64_t>(f) * 9;
    const double* tr = q.translations + static_cast<int64_t>(f) * 3;
    const float* kf = q.k + static_cast<int64_t>(f) * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) fr.r[i] = static_cast<float>(rot[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) fr.t[i] = static_cast<float>(tr[i]);
    fr.fx = kf[0]; fr.cx = kf[2]; fr.fy = kf[4]; fr.cy = kf[5];
    return fr;
}

// the face's three indices, all inside 0 .. V - 1; false: the face is never hit and none of its vertices is read
__device__ __forceinline__ bool load_face(const MeshParams& q, int tri, int idx[3]) {
    const int32_t* face = q.faces + static_cast<int64_t>(tri) * 3;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        idx[c] = face[c];
        ok = ok && idx[c] >= 0 && idx[c] < q.vertex_count;
    }
    return ok;
}

// p = Rt (x - T): the difference first, then (R[0][a] q0 + R[1][a] q1) + R[2][a] q2
__device__ __forceinline__ void camera_vertex(const Frame& fr, const float* x, float p[3]) {
    float d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] = __fsub_rn(x[a], fr.t[a]);
#pragma unroll
    for (int a = 0; a < 3; ++a)
        p[a] = __fadd_rn(__fadd_rn(__fmul_rn(fr.r[a], d[0]), __fmul_rn(fr.r[3 + a], d[1])), __fmul_rn(fr.r[6 + a], d[2]));
}

__device__ __forceinline__ float edge(float px, float py, float qx, float qy) { return __fsub_rn(__fmul_rn(px, qy), __fmul_rn(py, qx)); }

struct Hit {
    float u, v, w, det, t;
};

// the test of the header for pixel (pu, pv) against camera-space vertices p[corner][axis]
__device__ __forceinline__ bool ray_test(const Frame& fr, const float p[3][3], int pu, int pv, int options, Hit& h) {
    const float dx = __fdiv_rn(__fsub_rn(static_cast<float>(pu), fr.cx), fr.fx);
    const float dy = __fdiv_rn(__fsub_rn(static_cast<float>(pv), fr.cy), fr.fy);
    float sx[3], sy[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        sx[c] = __fsub_rn(p[c][0], __fmul_rn(dx, p[c][2]));
        sy[c] = __fsub_rn(p[c][1], __fmul_rn(dy, p[c][2]));
    }
    h.u = edge(sx[2], sy[2], sx[1], sy[1]);
    h.v = edge(sx[0], sy[0], sx[2], sy[2]);
    h.w = edge(sx[1], sy[1], sx[0], sy[0]);
    bool inside = (h.u >= 0.0f && h.v >= 0.0f && h.w >= 0.0f) || (h.u <= 0.0f && h.v <= 0.0f && h.w <= 0.0f);
    inside = inside && !(sx[0] > 0.0f && sx[1] > 0.0f && sx[2] > 0.0f) && !(sx[0] < 0.0f && sx[1] < 0.0f && sx[2] < 0.0f);
    inside = inside && !(sy[0] > 0.0f && sy[1] > 0.0f && sy[2] > 0.0f) && !(sy[0] < 0.0f && sy[1] < 0.0f && sy[2] < 0.0f);
    h.det = __fadd_rn(__fadd_rn(h.u, h.v), h.w);
    h.t = __fdiv_rn(__fadd_rn(__fadd_rn(__fmul_rn(h.u, p[0][2]), __fmul_rn(h.v, p[1][2])), __fmul_rn(h.w, p[2][2])), h.det);
    if (!inside || !(h.det != 0.0f) || !(h.t > 0.0f && h.t < INFINITY)) return false;
    if ((options & ENDO_MESH_CULL_BACK) && h.det < 0.0f) return false;
    if ((options & ENDO_MESH_CULL_FRONT) && h.det > 0.0f) return false;
    return true;
}

__device__ __forceinline__ void offer(unsigned long long* key, float t, int tri) {
    const unsigned long long mine = (static_cast<unsigned long long>(__float_as_uint(t)) << 32) | static_cast<unsigned int>(tri);
    if (__hip_atomic_load(key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > mine) atomicMin(key, mine);
}

struct Box {
    int x0, x1, y0, y1;          // inclusive, inside the image; x0 > x1: empty
};

// One axis of the box.  With every p_z > 0 and a focal length > 0 the sheared coordinate p_x - d(u) p_z of a vertex falls as u grows and
// changes sign where u = f p_x / p_z + c, so all three are > 0 left of the smallest such u and < 0 right of the largest: the span rule
// refuses those pixels.  The margin covers the rounding of both sides, some 2^-21 of the coordinate (1 / 16 pixel and 2^-19 of it); whatever is not finite
// gives the whole axis.
__device__ __forceinline__ void box_axis(float focal, float centre, const float p[3][3], int axis, int size, int& lo, int& hi) {
    lo = 0;
    hi = size - 1;
    float low = INFINITY, high = -INFINITY;
    bool finite = focal > 0.0f && focal < INFINITY && fabsf(centre) < INFINITY;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float at = focal * (p[c][axis] / p[c][2]) + centre;
        finite = finite && fabsf(at) < INFINITY;
        low = fminf(low, at);
        high = fmaxf(high, at);
    }
    if (!finite) return;
    low -= 0.0625f + (fabsf(low) + fabsf(centre)) * 1.9073486328125e-6f;
    high += 0.0625f + (fabsf(high) + fabsf(centre)) * 1.9073486328125e-6f;
    const float last = static_cast<float>(size - 1);
    if (high < 0.0f || low > last) {
        lo = 1;
        hi = 0;
        return;
    }
    lo = static_cast<int>(fmaxf(floorf(low), 0.0f));
    hi = static_cast<int>(fminf(ceilf(high), last));
}

// the triangle's vertices in camera coordinates and its box; false: no pixel can hit it
__device__ __forceinline__ bool prepare(const MeshParams& q, const Frame& fr, const int idx[3], float p[3][3], Box& box) {
#pragma unroll
    for (int c = 0; c < 3; ++c) camera_vertex(fr, q.vertices + static_cast<int64_t>(idx[c]) * q.stride, p[c]);
    box = Box{0, q.width - 1, 0, q.height - 1};
    if (q.options & ENDO_MESH_BRUTE) return true;
    // all three at or behind the camera plane: U, V, W of one sign make t a mean of numbers <= 0, never > 0
    if (p[0][2] <= 0.0f && p[1][2] <= 0.0f && p[2][2] <= 0.0f) return false;
    if (!(p[0][2] > 0.0f && p[1][2] > 0.0f && p[2][2] > 0.0f)) return true;          // across the plane, or NaN: the image
    box_axis(fr.fx, fr.cx, p, 0, q.width, box.x0, box.x1);
    box_axis(fr.fy, fr.cy, p, 1, q.height, box.y0, box.y1);
    return box.x0 <= box.x1 && box.y0 <= box.y1;
}

__global__ void __launch_bounds__(kThreads) mesh_clear_kernel(const MeshParams q, int64_t pixels) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i < pixels) q.keys[i] = kNoHit;
    if (i == 0) *q.queue_count = 0ull;
    if (i < q.frames && q.flags) q.flags[i] = scale_ok(q.scales ? q.scales[i] : 1.0f) ? ENDO_FUSION_FRAME_OK : ENDO_FUSION_FRAME_BAD_SCALE;
}

__global__ void __launch_bounds__(kThreads) mesh_setup_kernel(const MeshParams q) {
    const int64_t tri64 = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const int f = blockIdx.y;
    const int lane = threadIdx.x & 63;
    bool queued = false;
    int tri = 0;
    if (tri64 < q.triangles && scale_ok(q.scales ? q.scales[f] : 1.0f)) {
        tri = static_cast<int>(tri64);
        int idx[3];
        if (load_face(q, tri, idx)) {
            const Frame fr = load_frame(q, f);
            float p[3][3];
            Box box;
            if (prepare(q, fr, idx, p, box)) {
                const int bw = box.x1 - box.x0 + 1, bh = box.y1 - box.y0 + 1;
                if (static_cast<int64_t>(bw) * bh <= kSmallBox) {
                    unsigned long long* keys = q.keys + static_cast<int64_t>(f) * q.height * q.width;
                    for (int pv = box.y0; pv <= box.y1; ++pv)
                        for (int pu = box.x0; pu <= box.x1; ++pu) {
                            Hit h;
                            if (ray_test(fr, p, pu, pv, q.options, h)) offer(keys + static_cast<int64_t>(pv) * q.width + pu, h.t, tri);
                        }
                } else {
                    queued = true;
                }
            }
        }
    }
    // one atomic per wave: the lanes that queue take consecutive slots behind the wave's base
    const unsigned long long want = __ballot(queued);
    if (want) {
        const int leader = __ffsll(static_cast<long long>(want)) - 1;
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(q.queue_count, static_cast<unsigned long long>(__popcll(want)));
        base = __shfl(base, leader, kWave);
        if (queued) {
            const int64_t slot = static_cast<int64_t>(base) + __popcll(want & ((1ull << lane) - 1ull));
            if (slot < static_cast<int64_t>(q.frames) * q.triangles)          // (always: each (frame, triangle) queues at most once)
                q.queue[slot] = (static_cast<unsigned long long>(f) << 32) | static_cast<unsigned int>(tri);
        }
    }
}

__global__ void __launch_bounds__(kThreads) mesh_queue_kernel(const MeshParams q) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kThreads / kWave) + (threadIdx.x >> 6);
    const int64_t waves = static_cast<int64_t>(gridDim.x) * (kThreads / kWave);
    const int64_t capacity = static_cast<int64_t>(q.frames) * q.triangles;
    int64_t count = static_cast<int64_t>(__hip_atomic_load(q.queue_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));          // read once
    if (count < 0 || count > capacity) count = capacity;
    for (int64_t e = wave; e < count; e += waves) {
        const unsigned long long entry = q.queue[e];
        const int f = static_cast<int>(entry >> 32), tri = static_cast<int>(entry & 0xffffffffull);
        if (f < 0 || f >= q.frames || tri < 0 || tri >= q.triangles) continue;
        int idx[3];
        if (!load_face(q, tri, idx)) continue;
        const Frame fr = load_frame(q, f);
        float p[3][3];
        Box box;
        if (!prepare(q, fr, idx, p, box)) continue;
        unsigned long long* keys = q.keys + static_cast<int64_t>(f) * q.height * q.width;
        for (int y = box.y0; y <= box.y1; y += kTile)
            for (int x = box.x0; x <= box.x1; x += kTile) {
                const int pu = x + (lane & (kTile - 1)), pv = y + lane / kTile;
                Hit h;
                if (pu <= box.x1 && pv <= box.y1 && ray_test(fr, p, pu, pv, q.options, h))
                    offer(keys + static_cast<int64_t>(pv) * q.width + pu, h.t, tri);
            }
    }
}

__global__ void __launch_bounds__(kThreads) mesh_resolve_kernel(const MeshParams q) {
    const int pixels = q.height * q.width;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const int f = blockIdx.y;
    if (i >= pixels) return;
    const int64_t pix = static_cast<int64_t>(f) * pixels + i;
    float depth = 0.0f, hit = 0.0f, bary[3] = {0.0f, 0.0f, 0.0f}, normal[3] = {0.0f, 0.0f, 0.0f};
    int32_t face = -1;
    uint8_t color[3] = {0, 0, 0};
    const float scale = q.scales ? q.scales[f] : 1.0f;
    const unsigned long long key = q.keys[pix];
    const int tri = static_cast<int>(key & 0xffffffffull);
    int idx[3];
    if (scale_ok(scale) && key != kNoHit && (!q.boundaries || q.boundaries[pix] > 0.5f) && tri >= 0 && tri < q.triangles && load_face(q, tri, idx)) {
        const Frame fr = load_frame(q, f);
        const float* x[3];
        float p[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[c] = q.vertices + static_cast<int64_t>(idx[c]) * q.stride;
            camera_vertex(fr, x[c], p[c]);
        }
        Hit h;
        if (ray_test(fr, p, i % q.width, i / q.width, q.options, h)) {          // (it passed once: the same numbers)
            depth = __fdiv_rn(h.t, scale);
            hit = 1.0f;
            face = tri;
            bary[0] = __fdiv_rn(h.u, h.det);
            bary[1] = __fdiv_rn(h.v, h.det);
            bary[2] = __fdiv_rn(h.w, h.det);
            float e1[3], e2[3], nv[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                e1[a] = __fsub_rn(x[1][a], x[0][a]);
                e2[a] = __fsub_rn(x[2][a], x[0][a]);
            }
            nv[0] = edge(e1[1], e1[2], e2[1], e2[2]);
            nv[1] = edge(e1[2], e1[0], e2[2], e2[0]);
            nv[2] = edge(e1[0], e1[1], e2[0], e2[1]);
            const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(nv[0], nv[0]), __fmul_rn(nv[1], nv[1])), __fmul_rn(nv[2], nv[2])));
            const bool unit = len > 0.0f && len < INFINITY;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float value = unit ? __fdiv_rn(nv[a], len) : 0.0f;
                normal[a] = h.det < 0.0f ? -value : value;          // det > 0: the front, whose normal already faces the camera
            }
            if (q.colors) {
#pragma unroll
                for (int byte = 0; byte < 3; ++byte) {          // rows hold r, g, b = planes 2, 1, 0; byte c is plane c
                    const int col = 5 - byte;
                    const float mixed = __fadd_rn(__fadd_rn(__fmul_rn(bary[0], x[0][col]), __fmul_rn(bary[1], x[1][col])), __fmul_rn(bary[2], x[2][col]));
                    color[byte] = static_cast<uint8_t>(fminf(fmaxf(rintf(mixed), 0.0f), 255.0f));          // (a NaN: 0)
                }
            }
        }
    }
    q.depth[pix] = depth;
    if (q.mask) q.mask[pix] = hit;
    if (q.triangle) q.triangle[pix] = face;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (q.barycentric) q.barycentric[pix * 3 + a] = bary[a];
        if (q.normals) q.normals[pix * 3 + a] = normal[a];
        if (q.colors) q.colors[pix * 3 + a] = color[a];
    }
}

inline bool aligned_to(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

}  // namespace endo

using namespace endo;

extern "C" int endo_mesh_render_tile(int which) {
    return which == 0 || which == 1 ? kTile : (which == 2 ? kSmallBox : (which == 3 ? kThreads : ENDO_E_BADARG));
}

extern "C" int64_t endo_mesh_render_workspace_bytes(int frames, int height, int width, int64_t triangles) {
    if (!frames_sizes_ok(frames, height, width) || triangles < 0 || triangles > INT32_MAX) return -1;
    return align256(static_cast<int64_t>(frames) * height * width * 8) + 256 + align256(static_cast<int64_t>(frames) * triangles * 8);
}

extern "C" int endo_mesh_render(const float* vertices, int64_t vertex_stride, int64_t vertex_count, const int32_t* faces, int64_t triangles,
                                const float* intrinsics, const double* rotations, const double* translations, const float* scales,
                                const float* boundaries, int frames, int height, int width, int options, float* depth, float* mask,
                                int32_t* triangle, float* barycentric, float* normals, uint8_t* colors, int32_t* flags, void* workspace,
                                int64_t workspace_bytes, void* stream_) {
    if (!intrinsics || !rotations || !translations || !depth || !workspace) return ENDO_E_BADARG;
    if (options & ~(ENDO_MESH_CULL_BACK | ENDO_MESH_CULL_FRONT | ENDO_MESH_BRUTE)) return ENDO_E_BADARG;
    if ((options & ENDO_MESH_CULL_BACK) && (options & ENDO_MESH_CULL_FRONT)) return ENDO_E_BADARG;
    if (vertex_count < 0 || vertex_count > INT32_MAX || vertex_stride < 3 || (vertex_count > 0 && !vertices)) return ENDO_E_BADARG;
    if (triangles < 0 || (triangles > 0 && !faces)) return ENDO_E_BADARG;
    if (colors && vertex_stride < 6) return ENDO_E_BADARG;
    const int64_t need = endo_mesh_render_workspace_bytes(frames, height, width, triangles);
    if (need < 0 || workspace_bytes < need) return ENDO_E_BADARG;
    if (!aligned_to(vertices, 4) || !aligned_to(faces, 4) || !aligned_to(intrinsics, 4) || !aligned_to(rotations, 8) ||
        !aligned_to(translations, 8) || !aligned_to(scales, 4) || !aligned_to(boundaries, 4) || !aligned_to(depth, 4) ||
        !aligned_to(mask, 4) || !aligned_to(triangle, 4) || !aligned_to(barycentric, 4) || !aligned_to(normals, 4) ||
        !aligned_to(flags, 4) || !aligned_to(workspace, 8))
        return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t pixels = static_cast<int64_t>(frames) * height * width;
    MeshParams p;
    p.vertices = vertices; p.stride = vertex_stride; p.vertex_count = static_cast<int>(vertex_count);
    p.faces = faces; p.triangles = static_cast<int>(triangles);
    p.k = intrinsics; p.rotations = rotations; p.translations = translations; p.scales = scales; p.boundaries = boundaries;
    p.frames = frames; p.height = height; p.width = width; p.options = options;
    char* base = static_cast<char*>(workspace);
    p.keys = reinterpret_cast<unsigned long long*>(base);
    p.queue_count = reinterpret_cast<unsigned long long*>(base + align256(pixels * 8));
    p.queue = reinterpret_cast<unsigned long long*>(base + align256(pixels * 8) + 256);
    p.depth = depth; p.mask = mask; p.triangle = triangle; p.barycentric = barycentric; p.normals = normals; p.colors = colors;
    p.flags = flags;
    ProfScope prof(kProfSmall, stream, 0.0, static_cast<double>(frames) * triangles * 48.0 + static_cast<double>(pixels) * 50.0);
    const int64_t cleared = pixels > frames ? pixels : frames;
    mesh_clear_kernel<<<static_cast<unsigned int>((cleared + kThreads - 1) / kThreads), kThreads, 0, stream>>>(p, pixels);
    ENDO_LAUNCH_CHECK();
    if (triangles > 0) {
        mesh_setup_kernel<<<dim3(static_cast<unsigned int>((triangles + kThreads - 1) / kThreads), frames), kThreads, 0, stream>>>(p);
        ENDO_LAUNCH_CHECK();
        mesh_queue_kernel<<<device_cu_count() * kQueueBlocksPerCu, kThreads, 0, stream>>>(p);
        ENDO_LAUNCH_CHECK();
    }
    mesh_resolve_kernel<<<dim3((height * width + kThreads - 1) / kThreads, frames), kThreads, 0, stream>>>(p);
    ENDO_LAUNCH_CHECK();
    return 0;
}
