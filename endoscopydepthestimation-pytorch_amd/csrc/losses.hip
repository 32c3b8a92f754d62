// Self-supervised losses: per-sample masked reductions (wave shuffle -> LDS -> one fp64 atomic per
// block), a one-wave finalize, and elementwise backward kernels.  HBM-bound.  The formulas: loss_device.h.
#include "common.h"
#include "loss_device.h"

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
    *loss = masked_l1_mean(stats, n, eps);
}

// per_sample = 0: `up` is d / d (the batch mean), one float; 1: d / d (each sample's term), n floats (the Display form)
__global__ void __launch_bounds__(256) sparse_l1_bwd_kernel(const float* __restrict__ up, int per_sample, const float* __restrict__ f,
                                                            const float* __restrict__ fh, const float* __restrict__ mask,
                                                            const double* __restrict__ stats, float* __restrict__ gf,
                                                            float* __restrict__ gfh, int nsamples, int c, int hw, float eps) {
    const int n = blockIdx.y;
    const float coef = masked_l1_coef(per_sample ? up[n] : *up / static_cast<float>(nsamples), stats + 2 * n, eps);
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
    const RayIntrinsics<kFormDistance> k9(K, n);
    float part[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = blockIdx.x * kLossThreads * kLossItems + threadIdx.x, k = 0; k < kLossItems && i < hw; ++k, i += kLossThreads) {
        const int yy = i / w, xx = i - yy * w;
        form_accumulate(kFormDistance, mask[base + i], d[base + i], dw[base + i], k9.ax(xx), k9.ay(yy), part);
    }
    block_sum_atomic<4>(part, stats + 4 * n, scratch);
}

__global__ void norm_dist_finalize(const double* stats, float* loss, int n, float eps) {
    if (threadIdx.x != 0) return;
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc += form_term(kFormDistance, static_cast<float>(stats[4 * i + 2]), form_den(kFormDistance, stats + 4 * i, eps));
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
    const RayIntrinsics<kFormDistance> k9(K, n);
    float cnum, cden;
    form_coefs(kFormDistance, *gloss / static_cast<float>(nsamples), static_cast<float>(stats[4 * n + 2]), form_den(kFormDistance, stats + 4 * n, eps),
               cnum, cden);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
        const int yy = i / w, xx = i - yy * w;
        const float ax = k9.ax(xx), ay = k9.ay(yy);
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
        scale_inv_accumulate(p[base + i], q[base + i], b[base + i], eps, part);
    }
    block_sum_atomic<3>(part, stats + 3 * n, scratch);
}

__global__ void scale_inv_finalize(const double* stats, float* loss, int n) {
    if (threadIdx.x != 0) return;
    *loss = scale_inv_mean(stats, n);
}

__global__ void __launch_bounds__(256) scale_inv_bwd_kernel(const float* __restrict__ gloss, const float* __restrict__ p,
                                                            const float* __restrict__ q, const float* __restrict__ b,
                                                            const double* __restrict__ stats, float* __restrict__ gp,
                                                            float* __restrict__ gq, int nsamples, int hw, float eps) {
    const int n = blockIdx.y;
    const int64_t base = static_cast<int64_t>(n) * hw;
    float c2, c1;
    scale_inv_coefs(*gloss / static_cast<float>(nsamples), stats + 3 * n, c2, c1);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
        float vp, vq;
        scale_inv_grad(p[base + i], q[base + i], b[base + i], eps, c2, c1, vp, vq);
        if (gp) gp[base + i] = vp;
        if (gq) gq[base + i] = vq;
    }
}

// ---- NormalizedL2Loss (losses.py:99-109), NormalizedL1Loss (losses.py:154-164), NormalizedWeightedMaskedL2Loss (losses.py:40-54) ----
// One reduce / apply pair for the three ratio losses over (a, b, mask), F = kFormL2, kFormL1 or kFormWeightedL2 (loss_device.h).
// stats: n x 4 fp64.  L2 / L1: [sum m a, sum m, num, den sum].  weighted: [num, den sum, w_n, sum w] -- the last two written by the finalize.

template <int F>
__global__ void __launch_bounds__(kLossThreads) ratio_reduce(const float* __restrict__ d, const float* __restrict__ dw,
                                                             const float* __restrict__ mask, double* stats, int hw) {
    constexpr int K = form_sums(F);
    __shared__ double scratch[K * (kLossThreads / 64)];
    const int n = blockIdx.y;
    const int64_t base = static_cast<int64_t>(n) * hw;
    float part[K];
#pragma unroll
    for (int k = 0; k < K; ++k) part[k] = 0.f;
    for (int i = blockIdx.x * kLossThreads * kLossItems + threadIdx.x, k = 0; k < kLossItems && i < hw; ++k, i += kLossThreads) {
        form_accumulate(F, mask[base + i], d[base + i], dw[base + i], 0.f, 0.f, part);
    }
    block_sum_atomic<K>(part, stats + 4 * n, scratch);
}

template <int F>
__global__ void norm_ratio_finalize(const double* stats, float* loss, int n, float eps) {
    if (threadIdx.x != 0) return;
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc += form_term(F, static_cast<float>(stats[4 * i + 2]), form_den(F, stats + 4 * i, eps));
    *loss = acc / static_cast<float>(n);
}

// weights from the translations (losses.py:44-48), the weighted batch value, and [w_n, sum w] for the backward
__global__ void weighted_l2_finalize(double* stats, const float* __restrict__ t, float* loss, int n, float eps) {
    if (threadIdx.x != 0) return;
    float acc = 0.f, wsum = 0.f;
    for (int i = 0; i < n; ++i) {
        const float wgt = translation_weight(t, i);
        acc += form_term(kFormWeightedL2, static_cast<float>(stats[4 * i]), form_den(kFormWeightedL2, stats + 4 * i, eps)) * wgt;
        wsum += wgt;
        stats[4 * i + 2] = static_cast<double>(wgt);
    }
    for (int i = 0; i < n; ++i) stats[4 * i + 3] = static_cast<double>(wsum);
    *loss = acc / wsum;
}

// (The per-pixel pair below is written here and once more in geometry.hip's consistency_bwd_kernel, not in loss_device.h: the compiler
// rounds  cnum * ta + cden * da  differently in the two places -- packed multiplies and an add here, a fused multiply-add there -- and
// each kernel keeps the rounding it had.)
template <int F>
__global__ void __launch_bounds__(256) ratio_bwd_kernel(const float* __restrict__ gloss, const float* __restrict__ d,
                                                        const float* __restrict__ dw, const float* __restrict__ mask,
                                                        const double* __restrict__ stats, float* __restrict__ gd,
                                                        float* __restrict__ gdw, int nsamples, int hw, float eps) {
    const int n = blockIdx.y;
    const int64_t base = static_cast<int64_t>(n) * hw;
    const double* s = stats + 4 * n;
    const float g = (F == kFormWeightedL2) ? *gloss * static_cast<float>(s[2]) / static_cast<float>(s[3]) : *gloss / static_cast<float>(nsamples);
    float cnum, cden;
    form_coefs(F, g, static_cast<float>(s[form_num_index(F)]), form_den(F, s, eps), cnum, cden);
    const float cmean = form_cmean(F, s, eps);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
        const float m = mask[base + i], a = d[base + i], b = dw[base + i];
        float ta, tb, da, db;                      // d num / d a (= -d num / d b), d den / d a, d den / d b, each per unit of mask
        if (F == kFormL1) {
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
// The mask and the sparse >= 0.5 test of masked_log_ratio are independent: a masked pixel with sparse depth in (0, 0.5) has r = 0 and
// still counts in sum m.  stats: n x 3 fp64 [sum m r^2, sum m r, sum m]; the batch value is scale_inv_finalize's.
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
    float c2, c1;
    scale_inv_coefs(*gloss / static_cast<float>(nsamples), stats + 3 * n, c2, c1);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
        const float e = est[base + i], s = sparse[base + i];
        float v = 0.f;
        if (!(s < 0.5f)) v = mask[base + i] * (c2 * masked_log_ratio(e, s, eps) + c1) / (e + eps);
        gest[base + i] = v;
    }
}

// ---- SparseMaskedL1LossDisplay (losses.py:74-79): sparse_l1_reduce's sums, the (N,) vector instead of the batch mean -------
__global__ void sparse_l1_display_finalize(const double* stats, float* out, int n, float eps) {
    for (int i = threadIdx.x; i < n; i += blockDim.x)
        out[i] = masked_l1_term(stats + 2 * i, eps);
}

template <int F>
int ratio_fwd(const float* depth, const float* warped, const float* mask, const float* translations, float* loss, double* stats, int n,
              int hw, float eps, hipStream_t stream) {
    ProfScope prof(kProfLoss, stream, 0.0, 4.0 * 3.0 * n * hw);
    ENDO_CHECK(hipMemsetAsync(stats, 0, sizeof(double) * 4 * n, stream));
    ratio_reduce<F><<<reduce_grid(hw, n), kLossThreads, 0, stream>>>(depth, warped, mask, stats, hw);
    if (F == kFormWeightedL2)
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
    sparse_l1_bwd_kernel<<<apply_grid(hw, n), 256, 0, stream>>>(grad_loss, 0, flows, flows_hat, mask, stats, grad_flows, grad_hat, n,
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
    return ratio_fwd<kFormL2>(depth, warped, mask, nullptr, loss, stats, n, hw, eps, static_cast<hipStream_t>(stream_));
}

extern "C" int endo_norm_l2_bwd(const float* grad_loss, const float* depth, const float* warped, const float* mask, const double* stats,
                                float* grad_depth, float* grad_warped, int n, int hw, float eps, void* stream_) {
    if (!grad_loss || !depth || !warped || !mask || !stats || n <= 0 || hw <= 0) return ENDO_E_BADARG;
    return ratio_bwd<kFormL2>(grad_loss, depth, warped, mask, stats, grad_depth, grad_warped, n, hw, eps, static_cast<hipStream_t>(stream_));
}

extern "C" int endo_norm_l1_fwd(const float* depth, const float* warped, const float* mask, float* loss, double* stats, int n, int hw,
                                float eps, void* stream_) {
    if (!depth || !warped || !mask || !loss || !stats || n <= 0 || hw <= 0) return ENDO_E_BADARG;
    return ratio_fwd<kFormL1>(depth, warped, mask, nullptr, loss, stats, n, hw, eps, static_cast<hipStream_t>(stream_));
}

extern "C" int endo_norm_l1_bwd(const float* grad_loss, const float* depth, const float* warped, const float* mask, const double* stats,
                                float* grad_depth, float* grad_warped, int n, int hw, float eps, void* stream_) {
    if (!grad_loss || !depth || !warped || !mask || !stats || n <= 0 || hw <= 0) return ENDO_E_BADARG;
    return ratio_bwd<kFormL1>(grad_loss, depth, warped, mask, stats, grad_depth, grad_warped, n, hw, eps, static_cast<hipStream_t>(stream_));
}

extern "C" int endo_weighted_l2_fwd(const float* depth, const float* warped, const float* mask, const float* translations, float* loss,
                                    double* stats, int n, int hw, float eps, void* stream_) {
    if (!depth || !warped || !mask || !translations || !loss || !stats || n <= 0 || hw <= 0) return ENDO_E_BADARG;
    return ratio_fwd<kFormWeightedL2>(depth, warped, mask, translations, loss, stats, n, hw, eps, static_cast<hipStream_t>(stream_));
}

extern "C" int endo_weighted_l2_bwd(const float* grad_loss, const float* depth, const float* warped, const float* mask,
                                    const double* stats, float* grad_depth, float* grad_warped, int n, int hw, float eps, void* stream_) {
    if (!grad_loss || !depth || !warped || !mask || !stats || n <= 0 || hw <= 0) return ENDO_E_BADARG;
    return ratio_bwd<kFormWeightedL2>(grad_loss, depth, warped, mask, stats, grad_depth, grad_warped, n, hw, eps, static_cast<hipStream_t>(stream_));
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
    sparse_l1_bwd_kernel<<<apply_grid(hw, n), 256, 0, stream>>>(grad_out, 1, flows, flows_hat, mask, stats, grad_flows, grad_hat, n, c,
                                                                  hw, eps);
    ENDO_LAUNCH_CHECK();
    return 0;
}
