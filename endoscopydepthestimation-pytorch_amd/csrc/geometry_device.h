// Device helpers shared by geometry.hip and image_warp.hip: the per-sample camera maps, the ray of a pixel, the bilinear taps of a
// sample position, and the grid of the one-thread-per-pixel kernels.
#pragma once

#include "common.h"

namespace endo {

// ------------------------------------------------------------------------------------------
// camera maps (reference models.py:391-399 / 492-499 / 531-532)
//   M  = K R^T K^-1,  w  = -K R^T t          (frame-1 pixel + depth -> frame-2 homogeneous pixel)
//   M2 = K R   K^-1,  w2 =  K t              (only the z row / z entry is ever used)
// ------------------------------------------------------------------------------------------
struct Camera {
    float m[9];
    float w[3];
    float m2z[3];
    float w2z;
};

__device__ inline void mat3_mul(const double* a, const double* b, double* c) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[i * 3 + j] = a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j];
}

__device__ inline void camera_setup(const float* K, const float* R, const float* t, Camera* cam) {
    double k[9], r[9], rt[9], ki[9], tv[3];
    for (int i = 0; i < 9; ++i) { k[i] = K[i]; r[i] = R[i]; }
    for (int i = 0; i < 3; ++i) { tv[i] = t[i]; for (int j = 0; j < 3; ++j) rt[i * 3 + j] = r[j * 3 + i]; }
    const double det = k[0] * (k[4] * k[8] - k[5] * k[7]) - k[1] * (k[3] * k[8] - k[5] * k[6]) +
                       k[2] * (k[3] * k[7] - k[4] * k[6]);
    const double id = 1.0 / det;
    ki[0] = (k[4] * k[8] - k[5] * k[7]) * id; ki[1] = (k[2] * k[7] - k[1] * k[8]) * id; ki[2] = (k[1] * k[5] - k[2] * k[4]) * id;
    ki[3] = (k[5] * k[6] - k[3] * k[8]) * id; ki[4] = (k[0] * k[8] - k[2] * k[6]) * id; ki[5] = (k[2] * k[3] - k[0] * k[5]) * id;
    ki[6] = (k[3] * k[7] - k[4] * k[6]) * id; ki[7] = (k[1] * k[6] - k[0] * k[7]) * id; ki[8] = (k[0] * k[4] - k[1] * k[3]) * id;
    double krt[9], m[9], kr[9], m2[9];
    mat3_mul(k, rt, krt);
    mat3_mul(krt, ki, m);
    mat3_mul(k, r, kr);
    mat3_mul(kr, ki, m2);
    for (int i = 0; i < 9; ++i) cam->m[i] = static_cast<float>(m[i]);
    for (int i = 0; i < 3; ++i)
        cam->w[i] = static_cast<float>(-(krt[i * 3] * tv[0] + krt[i * 3 + 1] * tv[1] + krt[i * 3 + 2] * tv[2]));
    for (int j = 0; j < 3; ++j) cam->m2z[j] = static_cast<float>(m2[6 + j]);
    cam->w2z = static_cast<float>(k[6] * tv[0] + k[7] * tv[1] + k[8] * tv[2]);
}

__device__ __forceinline__ void load_camera(const float* K, const float* R, const float* t, int n, Camera* shared_cam) {
    if (threadIdx.x == 0) camera_setup(K + 9 * n, R + 9 * n, t + 3 * n, shared_cam);
    __syncthreads();
}

__device__ __forceinline__ void ray(const Camera& c, float x, float y, float& qx, float& qy, float& qz) {
    qx = fmaf(c.m[1], y, c.m[0] * x) + c.m[2];
    qy = fmaf(c.m[4], y, c.m[3] * x) + c.m[5];
    qz = fmaf(c.m[7], y, c.m[6] * x) + c.m[8];
}

// ------------------------------------------------------------------------------------------
// bilinear taps of grid_sample (models.py:325-336; bilinear, zeros padding, align_corners=False) at the pixel coordinate (u2, v2).
// Source location of the CPU grid_sample path: ix = (gx + 1) * (W / 2) - 0.5, gx = 2 (u / W) - 1.
// ------------------------------------------------------------------------------------------
struct Taps {
    float wnw, wne, wsw, wse;   // bilinear weights
    int x0, y0;                 // north-west tap (valid flags say which taps are in range)
    bool vw, ve, vn, vs;        // column west/east, row north/south in range
    float fx, fy;               // fractional parts (w, n in ATen's naming)
};

__device__ __forceinline__ Taps make_taps(float u2, float v2, int w, int h) {
    Taps tp;
    const float fw = static_cast<float>(w), fh = static_cast<float>(h);
    const float gx = 2.0f * (u2 / fw) - 1.0f;
    const float gy = 2.0f * (v2 / fh) - 1.0f;
    const float ix = (gx + 1.0f) * (fw * 0.5f) - 0.5f;
    const float iy = (gy + 1.0f) * (fh * 0.5f) - 0.5f;
    const float xw = floorf(ix), yn = floorf(iy);
    const float wx = ix - xw, ee = 1.0f - wx;
    const float ny = iy - yn, ss = 1.0f - ny;
    tp.wnw = ss * ee; tp.wne = ss * wx; tp.wsw = ny * ee; tp.wse = ny * wx;
    tp.fx = wx; tp.fy = ny;
    // range tests in float so that huge / non-finite coordinates never reach an int conversion
    tp.vw = (xw >= 0.0f) && (xw <= fw - 1.0f);
    tp.ve = (xw + 1.0f >= 0.0f) && (xw + 1.0f <= fw - 1.0f);
    tp.vn = (yn >= 0.0f) && (yn <= fh - 1.0f);
    tp.vs = (yn + 1.0f >= 0.0f) && (yn + 1.0f <= fh - 1.0f);
    const bool any = (tp.vw || tp.ve) && (tp.vn || tp.vs);
    tp.x0 = any ? static_cast<int>(xw) : 0;
    tp.y0 = any ? static_cast<int>(yn) : 0;
    return tp;
}

inline int plane_blocks(int hw, int threads) {
    int b = (hw + threads - 1) / threads;
    return b < 1 ? 1 : (b > 1024 ? 1024 : b);
}

}  // namespace endo
