// The losses' arithmetic, once: every formula below is inlined by the module kernels (losses.hip) AND by the fused kernels that
// evaluate the same loss inside another pass (geometry.hip consistency_*, distill.hip, image_warp.hip photometric_*, head.hip), so
// "the fused kernels compute what the modules compute" holds by construction.  fp32 per element, fp64 per-sample sums.
// (Not here: the consistency losses' per-pixel gradient pair -- losses.hip ratio_bwd_kernel says why.)
// A form is an ordinary int argument: every kernel passes a compile-time constant, which folds after inlining; only the one-wave
// consistency finalize passes its run-time value.
#pragma once

#include "common.h"

namespace endo {

__device__ __forceinline__ float sgn(float v) { return (v > 0.f) ? 1.f : ((v < 0.f) ? -1.f : 0.f); }

// ------------------------------------------------------------------------------------------
// Masked L1 (SparseMaskedL1Loss losses.py:62-66, its Display form 74-79, MaskedL1Loss 82-91).  Sums of a sample: [sum m |f - fh|, sum m].
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float masked_l1_term(const double* s, float eps) { return static_cast<float>(s[0]) / (eps + static_cast<float>(s[1])); }

__device__ __forceinline__ float masked_l1_mean(const double* stats, int n, float eps) {
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc += masked_l1_term(stats + 2 * i, eps);
    return acc / static_cast<float>(n);
}

// d loss / d (m |f - fh|) of a sample's elements under the upstream factor g of the sample's term
__device__ __forceinline__ float masked_l1_coef(float g, const double* s, float eps) { return g / (eps + static_cast<float>(s[1])); }

// ------------------------------------------------------------------------------------------
// The four depth-consistency losses between a depth map (a), the other frame's warped into it (b) and a mask (m); per sample num / den:
//   kFormDistance    NormalizedDistanceLoss          (losses.py:112-146)  sums  m a, m, m |P - Pw|_1, m (a + |b|);   den = s3 + 1e-5 mu, term 2 num / den
//   kFormL2          NormalizedL2Loss                (losses.py:94-109)   sums  m a, m, m (a-b)^2, m (a^2+b^2);      den = 0.5 s3 + 1e-5 mu^2, mu constant
//   kFormL1          NormalizedL1Loss                (losses.py:149-164)  sums  m a, m, m |a-b|, m (|a|+|b|);        den = 0.5 s3 + 1e-5 mu, mu differentiated
//   kFormWeightedL2  NormalizedWeightedMaskedL2Loss  (losses.py:35-54)    sums  m (a-b)^2, m (a^2+b^2);              den = 0.5 s1 + eps,
//                    batch value sum_n w_n term_n / sum_n w_n with w_n = translation_weight
// mu = sum m a / (eps + sum m).  P = depth * (ax, ay, 1) with ax = (x - cx) / fx, ay = (y - cy) / fy: the distance form's pixel ray.
// ------------------------------------------------------------------------------------------
enum ConsistencyForm {
    kFormDistance = ENDO_CONSISTENCY_DISTANCE,
    kFormL2 = ENDO_CONSISTENCY_L2,
    kFormL1 = ENDO_CONSISTENCY_L1,
    kFormWeightedL2 = ENDO_CONSISTENCY_WEIGHTED_L2
};
constexpr int kFormCount = 4;

constexpr int form_sums(int form) { return form == kFormWeightedL2 ? 2 : 4; }
constexpr int form_num_index(int form) { return form == kFormWeightedL2 ? 0 : 2; }          // where a sample's numerator is among its sums

// The intrinsics the distance form's pixel rays need, loaded once per block; the other forms hold nothing.
template <int F>
struct RayIntrinsics {
    __device__ RayIntrinsics(const float*, int) {}
    __device__ float ax(int) const { return 0.f; }
    __device__ float ay(int) const { return 0.f; }
};
template <>
struct RayIntrinsics<kFormDistance> {
    float fx, fy, cx, cy;
    __device__ RayIntrinsics(const float* K, int n) : fx(K[9 * n + 0]), fy(K[9 * n + 4]), cx(K[9 * n + 2]), cy(K[9 * n + 5]) {}
    __device__ float ax(int xx) const { return (static_cast<float>(xx) - cx) / fx; }
    __device__ float ay(int yy) const { return (static_cast<float>(yy) - cy) / fy; }
};

// one pixel into its thread's partial sums (form_sums(form) of them); ax, ay are read by the distance form only
__device__ __forceinline__ void form_accumulate(int form, float m, float a, float b, float ax, float ay, float* part) {
    if (form == kFormWeightedL2) {
        part[0] += m * (a - b) * (a - b);
        part[1] += m * (a * a + b * b);
        return;
    }
    part[0] += m * a;
    part[1] += m;
    if (form == kFormDistance) {
        part[2] += m * fabsf(ax * a - ax * b) + m * fabsf(ay * a - ay * b) + m * fabsf(a - b);
        part[3] += m * (a + fabsf(b));
    } else {
        part[2] += (form == kFormL2) ? m * (a - b) * (a - b) : m * fabsf(a - b);
        part[3] += (form == kFormL2) ? m * (a * a + b * b) : m * (fabsf(a) + fabsf(b));
    }
}

__device__ __forceinline__ float form_den(int form, const double* s, float eps) {
    if (form == kFormWeightedL2) return 0.5f * static_cast<float>(s[1]) + eps;
    const float mean_value = static_cast<float>(s[0]) / (eps + static_cast<float>(s[1]));
    if (form == kFormDistance) return 1.0e-5f * mean_value + static_cast<float>(s[3]);
    return 0.5f * static_cast<float>(s[3]) + ((form == kFormL2) ? 1.0e-5f * mean_value * mean_value : 1.0e-5f * mean_value);
}

__device__ __forceinline__ float form_term(int form, float num, float den) { return (form == kFormDistance) ? 2.0f * num / den : num / den; }

// (d loss / d num, d loss / d den) of a sample under the upstream factor g of its term
__device__ __forceinline__ void form_coefs(int form, float g, float num, float den, float& cnum, float& cden) {
    if (form == kFormDistance) {
        cnum = 2.0f * g / den;
        cden = -2.0f * g * num / (den * den);
    } else {
        cnum = g / den;
        cden = -g * num / (den * den);
    }
}

// the L1 form's third constant: d (1e-5 mu) / d a per masked pixel
__device__ __forceinline__ float form_cmean(int form, const double* s, float eps) {
    return (form == kFormL1) ? 1.0e-5f / (eps + static_cast<float>(s[1])) : 0.f;
}

// the weighted form's per-sample weight from the translations (losses.py:44-48)
__device__ __forceinline__ float translation_weight(const float* __restrict__ t, int i) {
    const float tx = t[3 * i], ty = t[3 * i + 1], tz = t[3 * i + 2];
    return 1.0f / (1.0e-8f + sqrtf(tx * tx + ty * ty + tz * tz));
}

// ------------------------------------------------------------------------------------------
// ScaleInvariantLoss (losses.py:22-32): r = log(m p + eps) - log(m q + eps); sums of a sample [sum r^2, sum r, sum m] = [R2, R1, S];
// term R2 / S + R1^2 / S^2.  MaskedScaleInvariantLoss (losses.py:173-186) has the same term over [sum m r^2, sum m r, sum m] with
// r SELECTED (torch.where), not multiplied: where sparse < 0.5 the unselected branch holds log(0) = -inf.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float scale_inv_ratio(float p, float q, float m, float eps, float& up, float& uq) {
    up = m * p + eps;
    uq = m * q + eps;
    return logf(up) - logf(uq);
}

__device__ __forceinline__ float masked_log_ratio(float est, float sparse, float eps) {
    return (sparse < 0.5f) ? 0.f : logf(est + eps) - logf(sparse);
}

__device__ __forceinline__ void scale_inv_accumulate(float p, float q, float m, float eps, float (&part)[3]) {
    float up, uq;
    const float r = scale_inv_ratio(p, q, m, eps, up, uq);
    part[0] += r * r;
    part[1] += r;
    part[2] += m;
}

// the mean over n samples of R2 / S + R1^2 / S^2
__device__ __forceinline__ float scale_inv_mean(const double* stats, int n) {
    float acc = 0.f;
    for (int i = 0; i < n; ++i) {
        const float r2 = static_cast<float>(stats[3 * i]), r1 = static_cast<float>(stats[3 * i + 1]), wsum = static_cast<float>(stats[3 * i + 2]);
        acc += r2 / wsum + (r1 * r1) / (wsum * wsum);
    }
    return acc / static_cast<float>(n);
}

// d loss / d r = c2 r + c1 of a sample's elements under the upstream factor g of the sample's term
__device__ __forceinline__ void scale_inv_coefs(float g, const double* s, float& c2, float& c1) {
    const float wsum = static_cast<float>(s[2]);
    c2 = 2.0f * g / wsum;
    c1 = 2.0f * g * static_cast<float>(s[1]) / (wsum * wsum);
}

__device__ __forceinline__ void scale_inv_grad(float p, float q, float m, float eps, float c2, float c1, float& gp, float& gq) {
    float up, uq;
    const float gr = c2 * scale_inv_ratio(p, q, m, eps, up, uq) + c1;
    gp = gr * m / up;
    gq = -gr * m / uq;
}

}  // namespace endo
