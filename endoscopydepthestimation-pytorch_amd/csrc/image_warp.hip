// Image warping (reference models.py:317-336, 377-429): the frame-2 coordinates of frame-1 pixels as planes of their own, and the
// bilinear sampler behind images_warping / _bilinear_interpolate -- F.grid_sample (bilinear, align_corners=False) on the grid
// (2u/W - 1, 2v/H - 1) with its three padding modes -- forward and backward.  Gather kernels, one thread per output pixel, grid-stride:
// a pixel's taps and weights are formed once and serve all C channels, so a call reads u, v and C planes (four L2-served taps per
// value) and writes C planes; the image gradient is scattered with one fp32 atomic per valid tap and channel into a buffer the call
// zeroes itself (endo_depth_warp_bwd's form).  No workspace, every output written in full.
// Behind them the photometric term (endo_photometric_fwd / _bwd): coordinates, sampler and MaskedL1Loss as one forward and one backward
// kernel that share the helpers above; its workspace is one plane.
#include "common.h"
#include "geometry_device.h"
#include "loss_device.h"

#include <float.h>
#include <limits.h>

namespace endo {

// ------------------------------------------------------------------------------------------
// warp coordinates (models.py:377-429): flow_fwd_kernel / flow_bwd_kernel of geometry.hip without the ((. - x) / W, (. - y) / H) of
// _flow_from_depth.  A masked-out pixel has zt = 1e30 and lands at u ~ 0, v ~ 0 (the reference's own behaviour).
// ------------------------------------------------------------------------------------------
// flow_fwd_kernel's  z2 = w_z + d q_z,  zt = 1e30 (1 - m) + m z2,  u2 = (w_x + d q_x) / zt,  v2 likewise, with the fused
// multiply-adds the compiler forms for it there written out and contraction off: left to itself it fuses other pairs here (packed
// math), and FlowfromDepthLayer's output would no longer be ((u - x) / W, (v - y) / H) of these planes bit for bit.
__device__ __forceinline__ void project_pixel(const Camera& cam, float qx, float qy, float qz, float d, float m, float& u2, float& v2) {
#pragma clang fp contract(off)
    const float z2 = fmaf(d, qz, cam.w[2]);
    const float zt = fmaf(1.0e30f, 1.0f - m, m * z2);
    u2 = fmaf(d, qx, cam.w[0]) / zt;
    v2 = fmaf(d, qy, cam.w[1]) / zt;
}

__global__ void __launch_bounds__(256) warp_coord_fwd_kernel(const float* __restrict__ depth, const float* __restrict__ mask,
                                                             const float* __restrict__ t, const float* __restrict__ R,
                                                             const float* __restrict__ K, float* __restrict__ u,
                                                             float* __restrict__ v, int h, int w) {
    __shared__ Camera cam;
    const int n = blockIdx.y;
    load_camera(K, R, t, n, &cam);
    const int hw = h * w;
    const int64_t base = static_cast<int64_t>(n) * hw;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
        const int yy = i / w, xx = i - yy * w;
        const float x = static_cast<float>(xx), y = static_cast<float>(yy);
        float qx, qy, qz;
        ray(cam, x, y, qx, qy, qz);
        float u2, v2;
        project_pixel(cam, qx, qy, qz, depth[base + i], mask[base + i], u2, v2);
        u[base + i] = u2;
        v[base + i] = v2;
    }
}

__global__ void __launch_bounds__(256) warp_coord_bwd_kernel(const float* __restrict__ gu_in, const float* __restrict__ gv_in,
                                                             const float* __restrict__ depth, const float* __restrict__ mask,
                                                             const float* __restrict__ t, const float* __restrict__ R,
                                                             const float* __restrict__ K, float* __restrict__ gdepth, int h, int w) {
    __shared__ Camera cam;
    const int n = blockIdx.y;
    load_camera(K, R, t, n, &cam);
    const int hw = h * w;
    const int64_t base = static_cast<int64_t>(n) * hw;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
        const int yy = i / w, xx = i - yy * w;
        float qx, qy, qz;
        ray(cam, static_cast<float>(xx), static_cast<float>(yy), qx, qy, qz);
        const float d = depth[base + i], m = mask[base + i];
        const float z2 = cam.w[2] + d * qz;
        const float zt = 1.0e30f * (1.0f - m) + m * z2;
        const float nx = cam.w[0] + d * qx;
        const float ny = cam.w[1] + d * qy;
        const float gu = gu_in ? gu_in[base + i] : 0.0f;
        const float gv = gv_in ? gv_in[base + i] : 0.0f;
        // u2 = nx / zt :  d u2 / d d = qx / zt - nx / zt^2 * (m qz)
        const float gzt = -(gu * nx + gv * ny) / (zt * zt);
        gdepth[base + i] = gu * qx / zt + gv * qy / zt + gzt * m * qz;
    }
}

// ------------------------------------------------------------------------------------------
// the sampler (models.py:325-336).  ATen's coordinate transforms for align_corners=False on the source location of make_taps:
//   zeros       none: taps outside the image read 0
//   border      ix clipped to [0, W - 1]; d ix' / d ix = 1 strictly inside, 0 on and beyond the ends
//   reflection  ix reflected over [-0.5, W - 0.5] (period 2 W; +1 on an even number of flips, -1 on an odd one), then clipped as above
// The reflection takes the remainder by the period 2 W and folds its upper half back: the remainder is exact, so this is ATen's
// fmod(., W) with the parity of floor(. / W) without an integer conversion of the quotient.
// ------------------------------------------------------------------------------------------
enum { kPadZeros = 0, kPadBorder = 1, kPadReflection = 2 };

// the coordinate after the padding mode's transform; mult: d (result) / d (coord)
__device__ __forceinline__ float pad_coordinate(float coord, float size, int mode, float& mult) {
    mult = 1.0f;
    if (mode == kPadZeros) return coord;
    if (mode == kPadReflection) {
        const float lo = -0.5f, span = size;
        float in = coord - lo;
        if (coord < lo) { in = lo - coord; mult = -1.0f; }
        const float extra = fmodf(in, 2.0f * span);
        if (extra < span) {
            coord = extra + lo;
        } else {
            coord = 2.0f * span - extra + lo;
            mult = -mult;
        }
    }
    if (coord <= 0.0f) { mult = 0.0f; return 0.0f; }
    if (coord >= size - 1.0f) { mult = 0.0f; return size - 1.0f; }
    return coord;
}

struct ModeTaps {
    Taps tp;
    float mx, my;          // d ix' / d ix, d iy' / d iy of the padding mode: 0, +1 or -1
    bool finite;           // false: the source location is NaN or infinite -- the pixel samples nothing (ATen leaves that case undefined)
};

// make_taps with the padding mode's transform between the source location and its floor.  Range tests in float, as there: a huge or
// non-finite coordinate never reaches an integer conversion or a load.
__device__ __forceinline__ ModeTaps make_mode_taps(float u2, float v2, int w, int h, int mode) {
    ModeTaps q;
    Taps& tp = q.tp;
    const float fw = static_cast<float>(w), fh = static_cast<float>(h);
    const float gx = 2.0f * (u2 / fw) - 1.0f;
    const float gy = 2.0f * (v2 / fh) - 1.0f;
    float ix = (gx + 1.0f) * (fw * 0.5f) - 0.5f;
    float iy = (gy + 1.0f) * (fh * 0.5f) - 0.5f;
    q.finite = (fabsf(ix) <= FLT_MAX) && (fabsf(iy) <= FLT_MAX);          // false for NaN as well
    if (!q.finite) { ix = 0.0f; iy = 0.0f; }                               // any finite location: the flags below are all cleared
    ix = pad_coordinate(ix, fw, mode, q.mx);
    iy = pad_coordinate(iy, fh, mode, q.my);
    const float xw = floorf(ix), yn = floorf(iy);
    const float wx = ix - xw, ee = 1.0f - wx;
    const float ny = iy - yn, ss = 1.0f - ny;
    tp.wnw = ss * ee; tp.wne = ss * wx; tp.wsw = ny * ee; tp.wse = ny * wx;
    tp.fx = wx; tp.fy = ny;
    tp.vw = q.finite && (xw >= 0.0f) && (xw <= fw - 1.0f);
    tp.ve = q.finite && (xw + 1.0f >= 0.0f) && (xw + 1.0f <= fw - 1.0f);
    tp.vn = q.finite && (yn >= 0.0f) && (yn <= fh - 1.0f);
    tp.vs = q.finite && (yn + 1.0f >= 0.0f) && (yn + 1.0f <= fh - 1.0f);
    const bool any = (tp.vw || tp.ve) && (tp.vn || tp.vs);
    tp.x0 = any ? static_cast<int>(xw) : 0;
    tp.y0 = any ? static_cast<int>(yn) : 0;
    if (!q.finite) q.mx = q.my = 0.0f;
    return q;
}

__global__ void __launch_bounds__(256) image_warp_fwd_kernel(const float* __restrict__ images, const float* __restrict__ u,
                                                             const float* __restrict__ v, float* __restrict__ warped,
                                                             int c, int h, int w, int mode) {
    const int n = blockIdx.y;
    const int hw = h * w;
    const int64_t cbase = static_cast<int64_t>(n) * hw;          // coordinate planes
    const int64_t ibase = cbase * c;                             // image planes
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
        const ModeTaps q = make_mode_taps(u[cbase + i], v[cbase + i], w, h, mode);
        const Taps& tp = q.tp;
        const bool val[4] = {tp.vw && tp.vn, tp.ve && tp.vn, tp.vw && tp.vs, tp.ve && tp.vs};
        const int o = tp.y0 * w + tp.x0;          // taps o, o + 1, o + w, o + w + 1: each read only where its flag says it is in range
        for (int ch = 0; ch < c; ++ch) {
            const float* __restrict__ src = images + ibase + static_cast<int64_t>(ch) * hw;
            float s[4] = {0.f, 0.f, 0.f, 0.f};
            if (val[0]) s[0] = src[o];
            if (val[1]) s[1] = src[o + 1];
            if (val[2]) s[2] = src[o + w];
            if (val[3]) s[3] = src[o + w + 1];
            float acc = tp.wnw * s[0];
            acc = fmaf(tp.wne, s[1], acc);
            acc = fmaf(tp.wsw, s[2], acc);
            acc = fmaf(tp.wse, s[3], acc);
            warped[ibase + static_cast<int64_t>(ch) * hw + i] = acc;
        }
    }
}

// gimg: null = no image gradient (no atomics); gu / gv: null = that coordinate gradient is not wanted; the image values are read only
// when one of them is.
__global__ void __launch_bounds__(256) image_warp_bwd_kernel(const float* __restrict__ gw, const float* __restrict__ images,
                                                             const float* __restrict__ u, const float* __restrict__ v,
                                                             float* gimg, float* __restrict__ gu, float* __restrict__ gv,
                                                             int c, int h, int w, int mode) {
    const int n = blockIdx.y;
    const int hw = h * w;
    const int64_t cbase = static_cast<int64_t>(n) * hw;
    const int64_t ibase = cbase * c;
    const bool coords = gu || gv;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
        const ModeTaps q = make_mode_taps(u[cbase + i], v[cbase + i], w, h, mode);
        const Taps& tp = q.tp;
        const bool val[4] = {tp.vw && tp.vn, tp.ve && tp.vn, tp.vw && tp.vs, tp.ve && tp.vs};
        const float wt[4] = {tp.wnw, tp.wne, tp.wsw, tp.wse};
        const int off[4] = {0, 1, w, w + 1};
        const int o = tp.y0 * w + tp.x0;
        const float sfrac = 1.0f - tp.fy, efrac = 1.0f - tp.fx;
        float gix = 0.f, giy = 0.f;
        for (int ch = 0; ch < c; ++ch) {
            const int64_t plane = ibase + static_cast<int64_t>(ch) * hw;
            const float g = gw[plane + i];
            float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!val[k]) continue;
                if (coords) s[k] = images[plane + o + off[k]];
                // nothing to add for a zero cotangent: under a mask-weighted loss that is every masked-out pixel, and those all land on
                // pixel (0, 0) (above) -- their atomics on one address would be served one after the other
                const float a = wt[k] * g;
                if (gimg && a != 0.0f) atomicAdd(gimg + plane + o + off[k], a);
            }
            // d out / d ix', d out / d iy' of this channel (warp_grad_d1's form), summed over the channels
            gix = fmaf(fmaf(s[3] - s[2], tp.fy, (s[1] - s[0]) * sfrac), g, gix);
            giy = fmaf(fmaf(s[3] - s[1], tp.fx, (s[2] - s[0]) * efrac), g, giy);
        }
        // grid_sample's W / 2 times the grid's 2 / W is 1; what is left is the padding mode's multiplier
        if (gu) gu[cbase + i] = q.mx * gix;
        if (gv) gv[cbase + i] = q.my * giy;
    }
}

// ------------------------------------------------------------------------------------------
// The photometric term: warp coordinates -> bilinear sample of the other frame's colours -> MaskedL1Loss (losses.py:82-91) against this
// frame's colours under the intersect mask, as ONE forward and ONE backward kernel; gridDim.z = the directions of the call (1 for
// endo_photometric_fwd, 2 for the loss head: z = 0 frame 1 against frame 2 sampled at the pose 1-wrt-2, z = 1 the roles swapped).
// The module chain is six launches and three intermediate tensors (u, v, the warped image) per direction.  The colours get no
// gradient, so nothing is scattered: the only gradient is to the pixel's own depth, and the forward kernel -- which has the taps, the
// colours and the camera in registers -- leaves the UNSCALED derivative d (sum_c m |c1 - warped|) / d depth of its pixel in one plane.
// The per-sample scale 1 / (eps + sum m) is known only after the reduction; the backward kernel is  grad = coef_n * plane.
// Per term the arithmetic is the chain's: project_pixel, make_mode_taps, image_warp_fwd_kernel's fmaf order, sparse_l1_reduce's
// m * |f - fh|, image_warp_bwd_kernel's gix / giy and warp_coord_bwd_kernel's chain rule (with the cotangent -sgn(c1 - warped) m).
// ------------------------------------------------------------------------------------------
struct PhotoArgs {
    const float* colors_1[2];        // this direction's own frame (the target of the L1)
    const float* colors_2[2];        // the frame that is sampled
    const float* depth[2];
    const float* inter[2];           // one-channel intersect masks
    const float* t[2];
    const float* R[2];
    const float* mask;
    const float* K;
    double* stats;                   // [directions][n][2]: sum m sum_c |c1 - warped|, sum m   (zeroed by the caller)
    float* plane[2];                 // unscaled d numerator / d depth
    float* grad[2];                  // backward: d loss / d depth
    const float* upstream[2];        // backward: d (caller's total) / d (this direction's term), one device float each
    int n, c, h, w, mode, accumulate;
    float eps;
};

constexpr int kPhotoItems = 4;          // pixels per thread of the forward kernel (its grid; the kernel itself is grid-stride)

__global__ void __launch_bounds__(256) photometric_fwd_kernel(const PhotoArgs a) {
    __shared__ Camera cam;
    __shared__ double scratch[2 * 4];
    const int n = blockIdx.y, z = blockIdx.z;
    const int h = a.h, w = a.w, c = a.c, mode = a.mode;
    // (no dynamic index into the kernel argument)
    const float* __restrict__ c1 = z ? a.colors_1[1] : a.colors_1[0];
    const float* __restrict__ c2 = z ? a.colors_2[1] : a.colors_2[0];
    const float* __restrict__ depth = z ? a.depth[1] : a.depth[0];
    const float* __restrict__ inter = z ? a.inter[1] : a.inter[0];
    float* __restrict__ plane = z ? a.plane[1] : a.plane[0];
    load_camera(a.K, z ? a.R[1] : a.R[0], z ? a.t[1] : a.t[0], n, &cam);
    const int hw = h * w;
    const int64_t base = static_cast<int64_t>(n) * hw;          // one-channel planes
    const int64_t ibase = base * c;                             // colour planes
    float part[2] = {0.f, 0.f};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
        const int yy = i / w, xx = i - yy * w;
        float qx, qy, qz;
        ray(cam, static_cast<float>(xx), static_cast<float>(yy), qx, qy, qz);
        const float d = depth[base + i], m = a.mask[base + i], mi = inter[base + i];
        float u2, v2;
        project_pixel(cam, qx, qy, qz, d, m, u2, v2);
        const ModeTaps q = make_mode_taps(u2, v2, w, h, mode);
        const Taps& tp = q.tp;
        const bool val[4] = {tp.vw && tp.vn, tp.ve && tp.vn, tp.vw && tp.vs, tp.ve && tp.vs};
        const int o = tp.y0 * w + tp.x0;          // taps o, o + 1, o + w, o + w + 1: each read only where its flag says it is in range
        const float sfrac = 1.0f - tp.fy, efrac = 1.0f - tp.fx;
        float num = 0.f, gix = 0.f, giy = 0.f;
        for (int ch = 0; ch < c; ++ch) {
            const float* __restrict__ src = c2 + ibase + static_cast<int64_t>(ch) * hw;
            float s[4] = {0.f, 0.f, 0.f, 0.f};
            if (val[0]) s[0] = src[o];
            if (val[1]) s[1] = src[o + 1];
            if (val[2]) s[2] = src[o + w];
            if (val[3]) s[3] = src[o + w + 1];
            float acc = tp.wnw * s[0];
            acc = fmaf(tp.wne, s[1], acc);
            acc = fmaf(tp.wsw, s[2], acc);
            acc = fmaf(tp.wse, s[3], acc);
            const float diff = c1[ibase + static_cast<int64_t>(ch) * hw + i] - acc;
            num += mi * fabsf(diff);
            const float g = -(sgn(diff) * mi);          // d (m |c1 - warped|) / d warped
            gix = fmaf(fmaf(s[3] - s[2], tp.fy, (s[1] - s[0]) * sfrac), g, gix);
            giy = fmaf(fmaf(s[3] - s[1], tp.fx, (s[2] - s[0]) * efrac), g, giy);
        }
        part[0] += num;
        part[1] += mi;
        float gd = 0.f;
        if (q.finite) {          // a non-finite coordinate sampled nothing: zero gradient (and no 0 * inf below)
            const float gu = q.mx * gix, gv = q.my * giy;
            const float z2 = cam.w[2] + d * qz;
            const float zt = 1.0e30f * (1.0f - m) + m * z2;
            const float nx = cam.w[0] + d * qx;
            const float ny = cam.w[1] + d * qy;
            const float gzt = -(gu * nx + gv * ny) / (zt * zt);
            gd = gu * qx / zt + gv * qy / zt + gzt * m * qz;
        }
        plane[base + i] = gd;
    }
    block_sum_atomic<2>(part, a.stats + 2 * (static_cast<int64_t>(z) * a.n + n), scratch);
}

// loss = mean_n num_n / (eps + den_n)
__global__ void photometric_finalize_kernel(const double* stats, float* loss, int n, float eps) {
    if (threadIdx.x != 0) return;
    *loss = masked_l1_mean(stats, n, eps);
}

// grad_depth = upstream / N / (eps + den_n) * plane: one writer per element, no atomics; accumulate adds to what is there
__global__ void __launch_bounds__(256) photometric_bwd_kernel(const PhotoArgs a) {
    const int n = blockIdx.y, z = blockIdx.z;
    const float* __restrict__ plane = z ? a.plane[1] : a.plane[0];
    float* __restrict__ grad = z ? a.grad[1] : a.grad[0];
    const float up = *(z ? a.upstream[1] : a.upstream[0]);
    const float coef = masked_l1_coef(up / static_cast<float>(a.n), a.stats + 2 * (static_cast<int64_t>(z) * a.n + n), a.eps);
    const int hw = a.h * a.w;
    const int64_t base = static_cast<int64_t>(n) * hw;
    if (a.accumulate) {          // the product rounded, then added: what accumulate = 0 writes, plus what was there (no fused multiply-add)
#pragma clang fp contract(off)
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
            const float g = coef * plane[base + i];
            grad[base + i] = grad[base + i] + g;
        }
    } else {
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) grad[base + i] = coef * plane[base + i];
    }
}

// h * w is a plane index held in an int, and the grid-stride loop steps past it by up to 1024 * 256 before it stops
inline bool plane_fits(int h, int w) {
    return static_cast<int64_t>(h) * w <= static_cast<int64_t>(INT_MAX) - 1024 * 256;
}

}  // namespace endo

using namespace endo;

extern "C" int endo_warp_coordinates_fwd(const float* depth, const float* mask, const float* t, const float* R, const float* K,
                                         float* u, float* v, int n, int h, int w, void* stream_) {
    if (!depth || !mask || !t || !R || !K || !u || !v || n <= 0 || h <= 0 || w <= 0 || !plane_fits(h, w)) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfGeometry, stream, 0.0, 4.0 * 4.0 * n * h * w);
    warp_coord_fwd_kernel<<<dim3(plane_blocks(h * w, 256), n), 256, 0, stream>>>(depth, mask, t, R, K, u, v, h, w);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_warp_coordinates_bwd(const float* grad_u, const float* grad_v, const float* depth, const float* mask,
                                         const float* t, const float* R, const float* K, float* grad_depth, int n, int h, int w,
                                         void* stream_) {
    if (!depth || !mask || !t || !R || !K || !grad_depth || n <= 0 || h <= 0 || w <= 0 || !plane_fits(h, w)) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfGeometry, stream, 0.0, 5.0 * 4.0 * n * h * w);
    warp_coord_bwd_kernel<<<dim3(plane_blocks(h * w, 256), n), 256, 0, stream>>>(grad_u, grad_v, depth, mask, t, R, K, grad_depth, h, w);
    ENDO_LAUNCH_CHECK();
    return 0;
}

static bool image_warp_sizes_ok(int n, int c, int h, int w, int padding_mode) {
    return n > 0 && c > 0 && h > 0 && w > 0 && plane_fits(h, w) && padding_mode >= kPadZeros && padding_mode <= kPadReflection;
}

extern "C" int endo_image_warp_fwd(const float* images, const float* u, const float* v, float* warped, int n, int c, int h, int w,
                                   int padding_mode, void* stream_) {
    if (!images || !u || !v || !warped || !image_warp_sizes_ok(n, c, h, w, padding_mode)) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfGeometry, stream, 0.0, (2.0 + 2.0 * c) * 4.0 * n * h * w);
    image_warp_fwd_kernel<<<dim3(plane_blocks(h * w, 256), n), 256, 0, stream>>>(images, u, v, warped, c, h, w, padding_mode);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_image_warp_bwd(const float* grad_warped, const float* images, const float* u, const float* v, float* grad_images,
                                   float* grad_u, float* grad_v, int n, int c, int h, int w, int padding_mode, void* stream_) {
    if (!grad_warped || !images || !u || !v || !image_warp_sizes_ok(n, c, h, w, padding_mode)) return ENDO_E_BADARG;
    if (!grad_images && !grad_u && !grad_v) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfGeometry, stream, 0.0, (4.0 + 4.0 * c) * 4.0 * n * h * w);
    if (grad_images) ENDO_CHECK(hipMemsetAsync(grad_images, 0, sizeof(float) * static_cast<size_t>(n) * c * h * w, stream));
    image_warp_bwd_kernel<<<dim3(plane_blocks(h * w, 256), n), 256, 0, stream>>>(grad_warped, images, u, v, grad_images, grad_u, grad_v,
                                                                                 c, h, w, padding_mode);
    ENDO_LAUNCH_CHECK();
    return 0;
}

// ---- the photometric term (include/endo_hip.h) ----
extern "C" int64_t endo_photometric_workspace_floats(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return -1;
    return (static_cast<int64_t>(n) * h * w + 3) / 4 * 4;
}

// Both kernels for `dirs` directions (common.h; head.hip calls it with dirs = 2).  phase 1: the forward kernel (the caller has zeroed
// stats); phase 2: the backward kernel.  Pointer pairs: [0] direction 0, [1] direction 1 (unused when dirs = 1).
int endo_photometric_phase(int phase, int dirs, const float* const* colors_1, const float* const* colors_2, const float* const* depth,
                           const float* mask, const float* const* inter, const float* const* t, const float* const* R, const float* K,
                           double* stats, float* const* plane, const float* const* upstream, float* const* grad, int accumulate, int n,
                           int c, int h, int w, float eps, int padding_mode, hipStream_t stream) {
    PhotoArgs a{};
    for (int z = 0; z < dirs; ++z) {
        if (phase == 1) {
            a.colors_1[z] = colors_1[z]; a.colors_2[z] = colors_2[z]; a.depth[z] = depth[z]; a.inter[z] = inter[z];
            a.t[z] = t[z]; a.R[z] = R[z];
        } else {
            a.upstream[z] = upstream[z]; a.grad[z] = grad[z];
        }
        a.plane[z] = plane[z];
    }
    a.mask = mask; a.K = K; a.stats = stats;
    a.n = n; a.c = c; a.h = h; a.w = w; a.mode = padding_mode; a.accumulate = accumulate; a.eps = eps;
    const dim3 grid(plane_blocks(h * w, 256), n, dirs);
    if (phase == 1) {
        // four pixels per thread (grid-stride): every block ends in two fp64 atomics on its sample's sums, all samples' sums share a cache
        // line or two, and atomics on one line are served one after the other (~8 ns each) -- at one pixel per thread the
        // 2 560 blocks of a batch of 8 at 256 x 320 spent 34 us there
        const dim3 fwd_grid(plane_blocks((h * w + kPhotoItems - 1) / kPhotoItems, 256), n, dirs);
        photometric_fwd_kernel<<<fwd_grid, 256, 0, stream>>>(a);
    } else {
        photometric_bwd_kernel<<<grid, 256, 0, stream>>>(a);
    }
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_photometric_fwd(const float* colors_1, const float* colors_2, const float* depth, const float* mask,
                                    const float* intersect, const float* t, const float* R, const float* K, float* loss, double* stats,
                                    float* workspace, int n, int c, int h, int w, float eps, int padding_mode, void* stream_) {
    if (!colors_1 || !colors_2 || !depth || !mask || !intersect || !t || !R || !K || !loss || !stats || !workspace ||
        !image_warp_sizes_ok(n, c, h, w, padding_mode))
        return ENDO_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0 || reinterpret_cast<uintptr_t>(stats) % 8 != 0) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // depth, mask, intersect, C planes of colors_1, the four-tap gather of C planes of colors_2 (L2-served), the derivative plane written
    ProfScope prof(kProfLoss, stream, 0.0, (4.0 + 2.0 * c) * 4.0 * n * h * w);
    ENDO_CHECK(hipMemsetAsync(stats, 0, sizeof(double) * 2 * n, stream));
    const int rc = endo_photometric_phase(1, 1, &colors_1, &colors_2, &depth, mask, &intersect, &t, &R, K, stats, &workspace, nullptr,
                                          nullptr, 0, n, c, h, w, eps, padding_mode, stream);
    if (rc) return rc;
    photometric_finalize_kernel<<<1, 64, 0, stream>>>(stats, loss, n, eps);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_photometric_bwd(const float* grad_loss, const double* stats, const float* workspace, float* grad_depth,
                                    int accumulate, int n, int h, int w, float eps, void* stream_) {
    if (!grad_loss || !stats || !workspace || !grad_depth || n <= 0 || h <= 0 || w <= 0 || !plane_fits(h, w) ||
        (accumulate != 0 && accumulate != 1))
        return ENDO_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0 || reinterpret_cast<uintptr_t>(stats) % 8 != 0) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfLoss, stream, 0.0, (2.0 + accumulate) * 4.0 * n * h * w);
    float* plane = const_cast<float*>(workspace);
    return endo_photometric_phase(2, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, const_cast<double*>(stats),
                                  &plane, &grad_loss, &grad_depth, accumulate, n, 1, h, w, eps, 0, stream);
}
