// Self-supervised losses: per-sample masked reductions (wave shuffle -> LDS -> one fp64 atomic per
// block), a one-wave finalize, and elementwise backward kernels.  HBM-bound.
#include "common.h"

namespace endo {

constexpr int kLossThreads = 256;
constexpr int kLossItems = 8;

inline dim3 reduce_grid(int hw, int n) { return dim3((hw + kLossThreads * kLossItems - 1) / (kLossThreads * kLossItems), n); }
inline dim3 apply_grid(int hw, int n) {
    int b = (hw + 255) / 256;
    return dim3(b > 1024 ? 1024 : b, n);
}

// ---- SparseMaskedL1Loss (losses.py:62-66) -------------------------------------------------
__global__ void __launch_bounds__(kLossThreads) sparse_l1_reduce(const float* __restrict__ f, const float* __restrict__ fh,
                                                                 const float* __restrict__ mask, double* stats, int c, int hw) {
    __shared__ double scratch[2 * (kLossThreads / 64)];
    const int n = blockIdx.y;
    const int64_t mbase = static_cast<int64_t>(n) * hw, fbase = mbase * c;
    float part[2] = {0.f, 0.f};
    for (int i = blockIdx.x * kLossThreads * kLossItems + threadIdx.x, k = 0; k < kLossItems && i < hw; ++k, i += kLossThreads) {
        const float m = mask[mbase + i];
        float a = 0.f;
        for (int ch = 0; ch < c; ++ch) {
            const int64_t o = fbase + static_cast<int64_t>(ch) * hw + i;
            a += m * fabsf(f[o] - fh[o]);
        }
        part[0] += a;
        part[1] += m;
    }
    block_sum_atomic<2>(part, stats + 2 * n, scratch);
}

__global__ void sparse_l1_finalize(const double* stats, float* loss, int n, float eps) {
    if (threadIdx.x != 0) return;
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc += static_cast<float>(stats[2 * i]) / (eps + static_cast<float>(stats[2 * i + 1]));
    *loss = acc / static_cast<float>(n);
}

__device__ __forceinline__ float sgn(float v) { return (v > 0.f) ? 1.f : ((v < 0.f) ? -1.f : 0.f); }

__global__ void __launch_bounds__(256) sparse_l1_bwd_kernel(const float* __restrict__ gloss, const float* __restrict__ f,
                                                            const float* __restrict__ fh, const float* __restrict__ mask,
                                                            const double* __restrict__ stats, float* __restrict__ gf,
                                                            float* __restrict__ gfh, int nsamples, int c, int hw, float eps) {
    const int n = blockIdx.y;
    const float coef = *gloss / static_cast<float>(nsamples) / (eps + static_cast<float>(stats[2 * n + 1]));
    const int64_t mbase = static_cast<int64_t>(n) * hw, fbase = mbase * c;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
        const float m = mask[mbase + i] * coef;
        for (int ch = 0; ch < c; ++ch) {
            const int64_t o = fbase + static_cast<int64_t>(ch) * hw + i;
            const float s = sgn(f[o] - fh[o]) * m;
            if (gf) gf[o] = s;
            if (gfh) gfh[o] = -s;
        }
    }
}

// ---- NormalizedDistanceLoss (losses.py:122-146) ----------------------------------------------
__global__ void __launch_bounds__(kLossThreads) norm_dist_reduce(const float* __restrict__ d, const float* __restrict__ dw,
                                                                 const float* __restrict__ mask, const float* __restrict__ K,
                                                                 double* stats, int h, int w) {
    __shared__ double scratch[4 * (kLossThreads / 64)];
    const int n = blockIdx.y;
    const int hw = h * w;
    const int64_t base = static_cast<int64_t>(n) * hw;
    const float fx = K[9 * n + 0], fy = K[9 * n + 4], cx = K[9 * n + 2], cy = K[9 * n + 5];
    float part[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = blockIdx.x * kLossThreads * kLossItems + threadIdx.x, k = 0; k < kLossItems && i < hw; ++k, i += kLossThreads) {
        const int yy = i / w, xx = i - yy * w;
        const float ax = (static_cast<float>(xx) - cx) / fx;
        const float ay = (static_cast<float>(yy) - cy) / fy;
        const float m = mask[base + i], a = d[base + i], b = dw[base + i];
        part[0] += m * a;
        part[1] += m;
        part[2] += m * fabsf(ax * a - ax * b) + m * fabsf(ay * a - ay * b) + m * fabsf(a - b);
        part[3] += m * (a + fabsf(b));
    }
    block_sum_atomic<4>(part, stats + 4 * n, scratch);
}

__device__ __forceinline__ float norm_dist_den(const double* s, float eps) {
    const float mean_value = static_cast<float>(s[0]) / (eps + static_cast<float>(s[1]));
    return 1.0e-5f * mean_value + static_cast<float>(s[3]);
}

__global__ void norm_dist_finalize(const double* stats, float* loss, int n, float eps) {
    if (threadIdx.x != 0) return;
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc += 2.0f * static_cast<float>(stats[4 * i + 2]) / norm_dist_den(stats + 4 * i, eps);
    *loss = acc / static_cast<float>(n);
}

__global__ void __launch_bounds__(256) norm_dist_bwd_kernel(const float* __restrict__ gloss, const float* __restrict__ d,
                                                            const float* __restrict__ dw, const float* __restrict__ mask,
                                                            const float* __restrict__ K, const double* __restrict__ stats,
                                                            float* __restrict__ gd, float* __restrict__ gdw, int nsamples,
                                                            int h, int w, float eps) {
    const int n = blockIdx.y;
    const int hw = h * w;
    const int64_t base = static_cast<int64_t>(n) * hw;
    const float fx = K[9 * n + 0], fy = K[9 * n + 4], cx = K[9 * n + 2], cy = K[9 * n + 5];
    const float den = norm_dist_den(stats + 4 * n, eps);
    const float g = *gloss / static_cast<float>(nsamples);
    const float cnum = 2.0f * g / den;                                              // d loss / d num
    const float cden = -2.0f * g * static_cast<float>(stats[4 * n + 2]) / (den * den);   // d loss / d den
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
        const int yy = i / w, xx = i - yy * w;
        const float ax = (static_cast<float>(xx) - cx) / fx;
        const float ay = (static_cast<float>(yy) - cy) / fy;
        const float m = mask[base + i], a = d[base + i], b = dw[base + i];
        const float t = ax * sgn(ax * a - ax * b) + ay * sgn(ay * a - ay * b) + sgn(a - b);
        if (gd) gd[base + i] = m * (cnum * t + cden);
        if (gdw) gdw[base + i] = m * (-cnum * t + cden * sgn(b));
    }
}

// ---- ScaleInvariantLoss (losses.py:22-32) ----------------------------------------------------
__global__ void __launch_bounds__(kLossThreads) scale_inv_reduce(const float* __restrict__ p, const float* __restrict__ q,
                                                                 const float* __restrict__ b, double* stats, int hw, float eps) {
    __shared__ double scratch[3 * (kLossThreads / 64)];
    const int n = blockIdx.y;
    const int64_t base = static_cast<int64_t>(n) * hw;
    float part[3] = {0.f, 0.f, 0.f};
    for (int i = blockIdx.x * kLossThreads * kLossItems + threadIdx.x, k = 0; k < kLossItems && i < hw; ++k, i += kLossThreads) {
        const float m = b[base + i];
        const float r = logf(m * p[base + i] + eps) - logf(m * q[base + i] + eps);
        part[0] += r * r;
        part[1] += r;
        part[2] += m;
    }
    block_sum_atomic<3>(part, stats + 3 * n, scratch);
}

__global__ void scale_inv_finalize(const double* stats, float* loss, int n) {
    if (threadIdx.x != 0) return;
    float acc = 0.f;
    for (int i = 0; i < n; ++i) {
        const float r2 = static_cast<float>(stats[3 * i]), r1 = static_cast<float>(stats[3 * i + 1]), wsum = static_cast<float>(stats[3 * i + 2]);
        acc += r2 / wsum + (r1 * r1) / (wsum * wsum);
    }
    *loss = acc / static_cast<float>(n);
}

__global__ void __launch_bounds__(256) scale_inv_bwd_kernel(const float* __restrict__ gloss, const float* __restrict__ p,
                                                            const float* __restrict__ q, const float* __restrict__ b,
                                                            const double* __restrict__ stats, float* __restrict__ gp,
                                                            float* __restrict__ gq, int nsamples, int hw, float eps) {
    const int n = blockIdx.y;
    const int64_t base = static_cast<int64_t>(n) * hw;
    const float wsum = static_cast<float>(stats[3 * n + 2]);
    const float g = *gloss / static_cast<float>(nsamples);
    const float c2 = 2.0f * g / wsum;                                               // * r
    const float c1 = 2.0f * g * static_cast<float>(stats[3 * n + 1]) / (wsum * wsum);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
        const float m = b[base + i];
        const float up = m * p[base + i] + eps, uq = m * q[base + i] + eps;
        const float r = logf(up) - logf(uq);
        const float gr = c2 * r + c1;
        if (gp) gp[base + i] = gr * m / up;
        if (gq) gq[base + i] = -gr * m / uq;
    }
}

// ---- NormalizedL2Loss (losses.py:99-109), NormalizedL1Loss (losses.py:154-164), NormalizedWeightedMaskedL2Loss (losses.py:40-54) ----
// One reduce / apply pair for the three ratio losses over (a, b, mask): per sample  num / den,
//   L2:        num = sum m (a-b)^2, den = 0.5 sum m (a^2+b^2) + 1e-5 mu^2   (mu = sum m a / (eps + sum m): a constant in the backward, no_grad)
//   L1:        num = sum m |a-b|,   den = 0.5 sum m (|a|+|b|) + 1e-5 mu     (mu is differentiated: one more per-sample constant in d den / d a)
//   weighted:  num = sum m (a-b)^2, den = 0.5 sum m (a^2+b^2) + eps,        batch = sum_n w_n num/den / sum_n w_n
// stats: n x 4 fp64.  L2 / L1: [sum m a, sum m, num, den sum].  weighted: [num, den sum, w_n, sum w] -- the last two written by the finalize.
enum RatioForm { kNormL2 = 0, kNormL1 = 1, kWeightedL2 = 2 };

template <int F>
__global__ void __launch_bounds__(kLossThreads) ratio_reduce(const float* __restrict__ d, const float* __restrict__ dw,
                                                             const float* __restrict__ mask, double* stats, int hw) {
    constexpr int K = (F == kWeightedL2) ? 2 : 4;
    __shared__ double scratch[K * (kLossThreads / 64)];
    const int n = blockIdx.y;
    const int64_t base = static_cast<int64_t>(n) * hw;
    float part[K];
#pragma unroll
    for (int k = 0; k < K; ++k) part[k] = 0.f;
    for (int i = blockIdx.x * kLossThreads * kLossItems + threadIdx.x, k = 0; k < kLossItems && i < hw; ++k, i += kLossThreads) {
        const float m = mask[base + i], a = d[base + i], b = dw[base + i];
        if constexpr (F == kWeightedL2) {
            part[0] += m * (a - b) * (a - b);
            part[1] += m * (a * a + b * b);
        } else {
            part[0] += m * a;
            part[1] += m;
            part[2] += (F == kNormL2) ? m * (a - b) * (a - b) : m * fabsf(a - b);
            part[3] += (F == kNormL2) ? m * (a * a + b * b) : m * (fabsf(a) + fabsf(b));
        }
    }
    block_sum_atomic<K>(part, stats + 4 * n, scratch);
}

template <int F>
__device__ __forceinline__ float ratio_den(const double* s, float eps) {
    if (F == kWeightedL2) return 0.5f * static_cast<float>(s[1]) + eps;
    const float mean_value = static_cast<float>(s[0]) / (eps + static_cast<float>(s[1]));
    return 0.5f * static_cast<float>(s[3]) + ((F == kNormL2) ? 1.0e-5f * mean_value * mean_value : 1.0e-5f * mean_value);
}

template <int F>
__global__ void norm_ratio_finalize(const double* stats, float* loss, int n, float eps) {
    if (threadIdx.x != 0) return;
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc += static_cast<float>(stats[4 * i + 2]) / ratio_den<F>(stats + 4 * i, eps);
    *loss = acc / static_cast<float>(n);
}

// weights from the translations (losses.py:44-48), the weighted batch value, and [w_n, sum w] for the backward
__global__ void weighted_l2_finalize(double* stats, const float* __restrict__ t, float* loss, int n, float eps) {
    if (threadIdx.x != 0) return;
    float acc = 0.f, wsum = 0.f;
    for (int i = 0; i < n; ++i) {
        const float tx = t[3 * i], ty = t[3 * i + 1], tz = t[3 * i + 2];
        const float wgt = 1.0f / (1.0e-8f + sqrtf(tx * tx + ty * ty + tz * tz));
        acc += static_cast<float>(stats[4 * i]) / ratio_den<kWeightedL2>(stats + 4 * i, eps) * wgt;
        wsum += wgt;
        stats[4 * i + 2] = static_cast<double>(wgt);
    }
    for (int i = 0; i < n; ++i) stats[4 * i + 3] = static_cast<double>(wsum);
    *loss = acc / wsum;
}

template <int F>
__global__ void __launch_bounds__(256) ratio_bwd_kernel(const float* __restrict__ gloss, const float* __restrict__ d,
                                                        const float* __restrict__ dw, const float* __restrict__ mask,
                                                        const double* __restrict__ stats, float* __restrict__ gd,
                                                        float* __restrict__ gdw, int nsamples, int hw, float eps) {
    const int n = blockIdx.y;
    const int64_t base = static_cast<int64_t>(n) * hw;
    const double* s = stats + 4 * n;
    const float den = ratio_den<F>(s, eps);
    const float num = static_cast<float>(s[(F == kWeightedL2) ? 0 : 2]);
    const float g = (F == kWeightedL2) ? *gloss * static_cast<float>(s[2]) / static_cast<float>(s[3]) : *gloss / static_cast<float>(nsamples);
    const float cnum = g / den;                    // d loss / d num
    const float cden = -g * num / (den * den);     // d loss / d den
    const float cmean = (F == kNormL1) ? 1.0e-5f / (eps + static_cast<float>(s[1])) : 0.f;   // d (1e-5 mu) / d a, per masked pixel
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
        const float m = mask[base + i], a = d[base + i], b = dw[base + i];
        float ta, tb, da, db;                      // d num / d a (= -d num / d b), d den / d a, d den / d b, each per unit of mask
        if (F == kNormL1) {
            ta = sgn(a - b);
            da = 0.5f * sgn(a) + cmean;
            db = 0.5f * sgn(b);
        } else {
            ta = 2.0f * (a - b);
            da = a;
            db = b;
        }
        tb = -ta;
        if (gd) gd[base + i] = m * (cnum * ta + cden * da);
        if (gdw) gdw[base + i] = m * (cnum * tb + cden * db);
    }
}

// ---- MaskedScaleInvariantLoss (losses.py:173-186) -----------------------------------------------
// r is SELECTED (torch.where), not multiplied: where sparse < 0.5 the unselected branch holds log(0) = -inf.  The mask and the
// sparse >= 0.5 test are independent: a masked pixel with sparse depth in (0, 0.5) has r = 0 and still counts in sum m.
// stats: n x 3 fp64 [sum m r^2, sum m r, sum m]; the batch value is scale_inv_finalize's.
__device__ __forceinline__ float masked_log_ratio(float est, float sparse, float eps) {
    return (sparse < 0.5f) ? 0.f : logf(est + eps) - logf(sparse);
}

__global__ void __launch_bounds__(kLossThreads) masked_scale_inv_reduce(const float* __restrict__ est, const float* __restrict__ sparse,
                                                                        const float* __restrict__ mask, double* stats, int hw, float eps) {
    __shared__ double scratch[3 * (kLossThreads / 64)];
    const int n = blockIdx.y;
    const int64_t base = static_cast<int64_t>(n) * hw;
    float part[3] = {0.f, 0.f, 0.f};
    for (int i = blockIdx.x * kLossThreads * kLossItems + threadIdx.x, k = 0; k < kLossItems && i < hw; ++k, i += kLossThreads) {
        const float m = mask[base + i];
        const float r = masked_log_ratio(est[base + i], sparse[base + i], eps);
        part[0] += m * (r * r);
        part[1] += m * r;
        part[2] += m;
    }
    block_sum_atomic<3>(part, stats + 3 * n, scratch);
}

__global__ void __launch_bounds__(256) masked_scale_inv_bwd_kernel(const float* __restrict__ gloss, const float* __restrict__ est,
                                                                   const float* __restrict__ sparse, const float* __restrict__ mask,
                                                                   const double* __restrict__ stats, float* __restrict__ gest,
                                                                   int nsamples, int hw, float eps) {
    const int n = blockIdx.y;
    const int64_t base = static_cast<int64_t>(n) * hw;
    const float wsum = static_cast<float>(stats[3 * n + 2]);
    const float g = *gloss / static_cast<float>(nsamples);
    const float c2 = 2.0f * g / wsum;                                               // * r
    const float c1 = 2.0f * g * static_cast<float>(stats[3 * n + 1]) / (wsum * wsum);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
        const float e = est[base + i], s = sparse[base + i];
        float v = 0.f;
        if (!(s < 0.5f)) v = mask[base + i] * (c2 * (logf(e + eps) - logf(s)) + c1) / (e + eps);
        gest[base + i] = v;
    }
}

// ---- SparseMaskedL1LossDisplay (losses.py:74-79): sparse_l1_reduce's sums, the (N,) vector instead of the batch mean -------
__global__ void sparse_l1_display_finalize(const double* stats, float* out, int n, float eps) {
    for (int i = threadIdx.x; i < n; i += blockDim.x)
        out[i] = static_cast<float>(stats[2 * i]) / (eps + static_cast<float>(stats[2 * i + 1]));
}

__global__ void __launch_bounds__(256) sparse_l1_display_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ f,
                                                                    const float* __restrict__ fh, const float* __restrict__ mask,
                                                                    const double* __restrict__ stats, float* __restrict__ gf,
                                                                    float* __restrict__ gfh, int c, int hw, float eps) {
    const int n = blockIdx.y;
    const float coef = gout[n] / (eps + static_cast<float>(stats[2 * n + 1]));
    const int64_t mbase = static_cast<int64_t>(n) * hw, fbase = mbase * c;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
        const float m = mask[mbase + i] * coef;
        for (int ch = 0; ch < c; ++ch) {
            const int64_t o = fbase + static_cast<int64_t>(ch) * hw + i;
            const float s = sgn(f[o] - fh[o]) * m;
            if (gf) gf[o] = s;
            if (gfh) gfh[o] = -s;
        }
    }
}

template <int F>
int ratio_fwd(const float* depth, const float* warped, const float* mask, const float* translations, float* loss, double* stats, int n,
              int hw, float eps, hipStream_t stream) {
    ProfScope prof(kProfLoss, stream, 0.0, 4.0 * 3.0 * n * hw);
    ENDO_CHECK(hipMemsetAsync(stats, 0, sizeof(double) * 4 * n, stream));
    ratio_reduce<F><<<reduce_grid(hw, n), kLossThreads, 0, stream>>>(depth, warped, mask, stats, hw);
    if (F == kWeightedL2)
        weighted_l2_finalize<<<1, 64, 0, stream>>>(stats, translations, loss, n, eps);
    else
        norm_ratio_finalize<F><<<1, 64, 0, stream>>>(stats, loss, n, eps);
    ENDO_LAUNCH_CHECK();
    return 0;
}

template <int F>
int ratio_bwd(const float* grad_loss, const float* depth, const float* warped, const float* mask, const double* stats, float* grad_depth,
              float* grad_warped, int n, int hw, float eps, hipStream_t stream) {
    ProfScope prof(kProfLoss, stream, 0.0, 4.0 * 5.0 * n * hw);
    ratio_bwd_kernel<F><<<apply_grid(hw, n), 256, 0, stream>>>(grad_loss, depth, warped, mask, stats, grad_depth, grad_warped, n, hw, eps);
    ENDO_LAUNCH_CHECK();
    return 0;
}

}  // namespace endo

using namespace endo;

extern "C" int endo_sparse_l1_fwd(const float* flows, const float* flows_hat, const float* mask, float* loss, double* stats, int n,
                                  int c, int hw, float eps, void* stream_) {
    return endo_sparse_l1_fwd_impl(flows, flows_hat, mask, loss, stats, n, c, hw, eps, 1, static_cast<hipStream_t>(stream_));
}

// zero = 0: the caller has zeroed `stats` (the loss head)
int endo_sparse_l1_fwd_impl(const float* flows, const float* flows_hat, const float* mask, float* loss, double* stats, int n, int c, int hw,
                            float eps, int zero, hipStream_t stream) {
    if (!flows || !flows_hat || !mask || !loss || !stats || n <= 0 || c <= 0 || hw <= 0) return ENDO_E_BADARG;
    ProfScope prof(kProfLoss, stream, 0.0, 4.0 * (2.0 * c + 1.0) * n * hw);
    if (zero) ENDO_CHECK(hipMemsetAsync(stats, 0, sizeof(double) * 2 * n, stream));
    sparse_l1_reduce<<<reduce_grid(hw, n), kLossThreads, 0, stream>>>(flows, flows_hat, mask, stats, c, hw);
    sparse_l1_finalize<<<1, 64, 0, stream>>>(stats, loss, n, eps);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_sparse_l1_bwd(const float* grad_loss, const float* flows, const float* flows_hat, const float* mask,
                                  const double* stats, float* grad_flows, float* grad_hat, int n, int c, int hw, float eps,
                                  void* stream_) {
    if (!grad_loss || !flows || !flows_hat || !mask || !stats || n <= 0 || c <= 0 || hw <= 0) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfLoss, stream, 0.0, 4.0 * (3.0 * c + 1.0) * n * hw);
    sparse_l1_bwd_kernel<<<apply_grid(hw, n), 256, 0, stream>>>(grad_loss, flows, flows_hat, mask, stats, grad_flows, grad_hat, n,
                                                                  c, hw, eps);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_norm_dist_fwd(const float* depth, const float* warped, const float* intersect, const float* K, float* loss,
                                  double* stats, int n, int h, int w, float eps, void* stream_) {
    if (!depth || !warped || !intersect || !K || !loss || !stats || n <= 0 || h <= 0 || w <= 0) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfLoss, stream, 0.0, 4.0 * 3.0 * n * h * w);
    ENDO_CHECK(hipMemsetAsync(stats, 0, sizeof(double) * 4 * n, stream));
    norm_dist_reduce<<<reduce_grid(h * w, n), kLossThreads, 0, stream>>>(depth, warped, intersect, K, stats, h, w);
    norm_dist_finalize<<<1, 64, 0, stream>>>(stats, loss, n, eps);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_norm_dist_bwd(const float* grad_loss, const float* depth, const float* warped, const float* intersect,
                                  const float* K, const double* stats, float* grad_depth, float* grad_warped, int n, int h, int w,
                                  float eps, void* stream_) {
    if (!grad_loss || !depth || !warped || !intersect || !K || !stats || n <= 0 || h <= 0 || w <= 0) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfLoss, stream, 0.0, 4.0 * 5.0 * n * h * w);
    norm_dist_bwd_kernel<<<apply_grid(h * w, n), 256, 0, stream>>>(grad_loss, depth, warped, intersect, K, stats, grad_depth,
                                                                    grad_warped, n, h, w, eps);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_scale_inv_fwd(const float* pred, const float* goal, const float* boundary, float* loss, double* stats, int n,
                                  int hw, float eps, void* stream_) {
    if (!pred || !goal || !boundary || !loss || !stats || n <= 0 || hw <= 0) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfLoss, stream, 0.0, 4.0 * 3.0 * n * hw);
    ENDO_CHECK(hipMemsetAsync(stats, 0, sizeof(double) * 3 * n, stream));
    scale_inv_reduce<<<reduce_grid(hw, n), kLossThreads, 0, stream>>>(pred, goal, boundary, stats, hw, eps);
    scale_inv_finalize<<<1, 64, 0, stream>>>(stats, loss, n);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_scale_inv_bwd(const float* grad_loss, const float* pred, const float* goal, const float* boundary,
                                  const double* stats, float* grad_pred, float* grad_goal, int n, int hw, float eps,
                                  void* stream_) {
    if (!grad_loss || !pred || !goal || !boundary || !stats || n <= 0 || hw <= 0) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfLoss, stream, 0.0, 4.0 * 5.0 * n * hw);
    scale_inv_bwd_kernel<<<apply_grid(hw, n), 256, 0, stream>>>(grad_loss, pred, goal, boundary, stats, grad_pred, grad_goal, n,
                                                                 hw, eps);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_norm_l2_fwd(const float* depth, const float* warped, const float* mask, float* loss, double* stats, int n, int hw,
                                float eps, void* stream_) {
    if (!depth || !warped || !mask || !loss || !stats || n <= 0 || hw <= 0) return ENDO_E_BADARG;
    return ratio_fwd<kNormL2>(depth, warped, mask, nullptr, loss, stats, n, hw, eps, static_cast<hipStream_t>(stream_));
}

extern "C" int endo_norm_l2_bwd(const float* grad_loss, const float* depth, const float* warped, const float* mask, const double* stats,
                                float* grad_depth, float* grad_warped, int n, int hw, float eps, void* stream_) {
    if (!grad_loss || !depth || !warped || !mask || !stats || n <= 0 || hw <= 0) return ENDO_E_BADARG;
    return ratio_bwd<kNormL2>(grad_loss, depth, warped, mask, stats, grad_depth, grad_warped, n, hw, eps, static_cast<hipStream_t>(stream_));
}

extern "C" int endo_norm_l1_fwd(const float* depth, const float* warped, const float* mask, float* loss, double* stats, int n, int hw,
                                float eps, void* stream_) {
    if (!depth || !warped || !mask || !loss || !stats || n <= 0 || hw <= 0) return ENDO_E_BADARG;
    return ratio_fwd<kNormL1>(depth, warped, mask, nullptr, loss, stats, n, hw, eps, static_cast<hipStream_t>(stream_));
}

extern "C" int endo_norm_l1_bwd(const float* grad_loss, const float* depth, const float* warped, const float* mask, const double* stats,
                                float* grad_depth, float* grad_warped, int n, int hw, float eps, void* stream_) {
    if (!grad_loss || !depth || !warped || !mask || !stats || n <= 0 || hw <= 0) return ENDO_E_BADARG;
    return ratio_bwd<kNormL1>(grad_loss, depth, warped, mask, stats, grad_depth, grad_warped, n, hw, eps, static_cast<hipStream_t>(stream_));
}

extern "C" int endo_weighted_l2_fwd(const float* depth, const float* warped, const float* mask, const float* translations, float* loss,
                                    double* stats, int n, int hw, float eps, void* stream_) {
    if (!depth || !warped || !mask || !translations || !loss || !stats || n <= 0 || hw <= 0) return ENDO_E_BADARG;
    return ratio_fwd<kWeightedL2>(depth, warped, mask, translations, loss, stats, n, hw, eps, static_cast<hipStream_t>(stream_));
}

extern "C" int endo_weighted_l2_bwd(const float* grad_loss, const float* depth, const float* warped, const float* mask,
                                    const double* stats, float* grad_depth, float* grad_warped, int n, int hw, float eps, void* stream_) {
    if (!grad_loss || !depth || !warped || !mask || !stats || n <= 0 || hw <= 0) return ENDO_E_BADARG;
    return ratio_bwd<kWeightedL2>(grad_loss, depth, warped, mask, stats, grad_depth, grad_warped, n, hw, eps, static_cast<hipStream_t>(stream_));
}

extern "C" int endo_masked_scale_inv_fwd(const float* est, const float* sparse, const float* mask, float* loss, double* stats, int n,
                                         int hw, float eps, void* stream_) {
    if (!est || !sparse || !mask || !loss || !stats || n <= 0 || hw <= 0) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfLoss, stream, 0.0, 4.0 * 3.0 * n * hw);
    ENDO_CHECK(hipMemsetAsync(stats, 0, sizeof(double) * 3 * n, stream));
    masked_scale_inv_reduce<<<reduce_grid(hw, n), kLossThreads, 0, stream>>>(est, sparse, mask, stats, hw, eps);
    scale_inv_finalize<<<1, 64, 0, stream>>>(stats, loss, n);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_masked_scale_inv_bwd(const float* grad_loss, const float* est, const float* sparse, const float* mask,
                                         const double* stats, float* grad_est, int n, int hw, float eps, void* stream_) {
    if (!grad_loss || !est || !sparse || !mask || !stats || n <= 0 || hw <= 0) return ENDO_E_BADARG;
    if (!grad_est) return 0;          // the one gradient there is was not requested
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfLoss, stream, 0.0, 4.0 * 4.0 * n * hw);
    masked_scale_inv_bwd_kernel<<<apply_grid(hw, n), 256, 0, stream>>>(grad_loss, est, sparse, mask, stats, grad_est, n, hw, eps);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_sparse_l1_display_fwd(const float* flows, const float* flows_hat, const float* mask, float* out, double* stats, int n,
                                          int c, int hw, float eps, void* stream_) {
    if (!flows || !flows_hat || !mask || !out || !stats || n <= 0 || c <= 0 || hw <= 0) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfLoss, stream, 0.0, 4.0 * (2.0 * c + 1.0) * n * hw);
    ENDO_CHECK(hipMemsetAsync(stats, 0, sizeof(double) * 2 * n, stream));
    sparse_l1_reduce<<<reduce_grid(hw, n), kLossThreads, 0, stream>>>(flows, flows_hat, mask, stats, c, hw);
    sparse_l1_display_finalize<<<1, 64, 0, stream>>>(stats, out, n, eps);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_sparse_l1_display_bwd(const float* grad_out, const float* flows, const float* flows_hat, const float* mask,
                                          const double* stats, float* grad_flows, float* grad_hat, int n, int c, int hw, float eps,
                                          void* stream_) {
    if (!grad_out || !flows || !flows_hat || !mask || !stats || n <= 0 || c <= 0 || hw <= 0) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfLoss, stream, 0.0, 4.0 * (3.0 * c + 1.0) * n * hw);
    sparse_l1_display_bwd_kernel<<<apply_grid(hw, n), 256, 0, stream>>>(grad_out, flows, flows_hat, mask, stats, grad_flows, grad_hat, c,
                                                                          hw, eps);
    ENDO_LAUNCH_CHECK();
    return 0;
}
