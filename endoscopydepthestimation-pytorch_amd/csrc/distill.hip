// The teacher-student term (reference utils.py:1462-1482, learn_from_teacher): ScaleInvariantLoss (losses.py:22-32) on |student| against
// |teacher| under the boundary mask, both frames, forward and backward, as two launches: one reduction over the 2n sample rows (frame 1's
// n samples, then frame 2's) and one apply pass whose first block also writes the loss values and the guard flag.  The apply pass forms
// the two logarithms again instead of reading a plane the reduction would have stored: 4 floats moved per element instead of 5, and
// the kernels are bound by their launches at the sizes of a training step anyway.  The arithmetic is
// loss_device.h's scale_inv_* with |.| on both maps.
#include "common.h"
#include "loss_device.h"

namespace endo {

constexpr int kDistillThreads = 256;
constexpr int kDistillItems = 8;          // elements per thread of a reduce block: 2048 per block, as losses.hip's reductions

struct DistillMaps {
    const float* pred[2];
    const float* goal[2];
    float* grad[2];
};

__device__ __forceinline__ void distill_accumulate(float p, float g, float m, float eps, float (&part)[3]) {
    scale_inv_accumulate(fabsf(p), fabsf(g), m, eps, part);
}

// V = 4: hw is a multiple of 4 and every map starts on 16 bytes, so each sample row does too; V = 1: any hw, any alignment.
// Either way block x of a row covers elements [2048 x, 2048 (x + 1)).
template <int V>
__global__ void __launch_bounds__(kDistillThreads) distill_reduce(DistillMaps maps, const float* __restrict__ b, double* stats, int n, int hw,
                                                                  float eps) {
    __shared__ double scratch[3 * (kDistillThreads / 64)];
    const int row = blockIdx.y, frame = row >= n ? 1 : 0, sample = row - frame * n;
    const int64_t base = static_cast<int64_t>(sample) * hw;
    const float* __restrict__ p = maps.pred[frame] + base;
    const float* __restrict__ g = maps.goal[frame] + base;
    const float* __restrict__ m = b + base;
    float part[3] = {0.f, 0.f, 0.f};
    if (V == 4) {
        const int hw4 = hw >> 2;
        for (int i = blockIdx.x * (kDistillThreads * kDistillItems / 4) + threadIdx.x, k = 0; k < kDistillItems / 4 && i < hw4;
             ++k, i += kDistillThreads) {
            const float4 pv = reinterpret_cast<const float4*>(p)[i], gv = reinterpret_cast<const float4*>(g)[i];
            const float4 mv = reinterpret_cast<const float4*>(m)[i];
            distill_accumulate(pv.x, gv.x, mv.x, eps, part);
            distill_accumulate(pv.y, gv.y, mv.y, eps, part);
            distill_accumulate(pv.z, gv.z, mv.z, eps, part);
            distill_accumulate(pv.w, gv.w, mv.w, eps, part);
        }
    } else {
        for (int i = blockIdx.x * kDistillThreads * kDistillItems + threadIdx.x, k = 0; k < kDistillItems && i < hw; ++k, i += kDistillThreads)
            distill_accumulate(p[i], g[i], m[i], eps, part);
    }
    block_sum_atomic<3>(part, stats + 3 * row, scratch);
}

__device__ __forceinline__ float distill_grad(float p, float g, float m, float eps, float c2, float c1) {
    float gp, gg;
    scale_inv_grad(fabsf(p), fabsf(g), m, eps, c2, c1, gp, gg);
    return gp * sgn(p);
}

template <int V, int ACC>
__global__ void __launch_bounds__(kDistillThreads) distill_apply(DistillMaps maps, const float* __restrict__ b, const double* __restrict__ stats,
                                                                 float* losses, float weight, int n, int hw, float eps) {
    const int row = blockIdx.y, frame = row >= n ? 1 : 0, sample = row - frame * n;
    if (blockIdx.x == 0 && row == 0 && threadIdx.x == 0) {          // the loss values and the guard of train.py:317, on the device
        const float distill = weight * 0.5f * (scale_inv_mean(stats, n) + scale_inv_mean(stats + 3 * n, n));
        const float total = ACC ? losses[0] + distill : distill;
        const float bad = (isnan(total) || isinf(total)) ? 1.f : 0.f;
        losses[0] = total;
        if (ACC) {
            losses[3] = (losses[3] != 0.f || bad != 0.f) ? 1.f : 0.f;          // a flag the loss head raised stays raised
        } else {
            losses[1] = 0.f;
            losses[2] = 0.f;
            losses[3] = bad;
        }
        losses[4] = distill;
    }
    const int64_t base = static_cast<int64_t>(sample) * hw;
    const float* __restrict__ p = maps.pred[frame] + base;
    const float* __restrict__ g = maps.goal[frame] + base;
    const float* __restrict__ m = b + base;
    float* __restrict__ out = maps.grad[frame] + base;
    float c2, c1;
    scale_inv_coefs(weight * 0.5f / static_cast<float>(n), stats + 3 * row, c2, c1);          // under d distill / d L_s
    if (V == 4) {
        const int hw4 = hw >> 2;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw4; i += gridDim.x * blockDim.x) {
            const float4 pv = reinterpret_cast<const float4*>(p)[i], gv = reinterpret_cast<const float4*>(g)[i];
            const float4 mv = reinterpret_cast<const float4*>(m)[i];
            float4 o = {distill_grad(pv.x, gv.x, mv.x, eps, c2, c1), distill_grad(pv.y, gv.y, mv.y, eps, c2, c1),
                        distill_grad(pv.z, gv.z, mv.z, eps, c2, c1), distill_grad(pv.w, gv.w, mv.w, eps, c2, c1)};
            if (ACC) {
                const float4 a = reinterpret_cast<const float4*>(out)[i];
                o.x += a.x;
                o.y += a.y;
                o.z += a.z;
                o.w += a.w;
            }
            reinterpret_cast<float4*>(out)[i] = o;
        }
    } else {
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
            const float v = distill_grad(p[i], g[i], m[i], eps, c2, c1);
            out[i] = ACC ? out[i] + v : v;
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace endo

using namespace endo;

extern "C" int endo_distill_head(const float* pred_1, const float* pred_2, const float* goal_1, const float* goal_2, const float* boundaries,
                                 float weight, float eps, int accumulate, float* losses, float* grad_pred_1, float* grad_pred_2, double* stats,
                                 int n, int hw, void* stream_) {
    if (!pred_1 || !pred_2 || !goal_1 || !goal_2 || !boundaries || !losses || !grad_pred_1 || !grad_pred_2 || !stats) return ENDO_E_BADARG;
    if (n <= 0 || hw <= 0 || 2 * static_cast<int64_t>(n) > 65535 || (accumulate != 0 && accumulate != 1) || !(weight >= 0.f)) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfLoss, stream, 0.0, 4.0 * (7.0 + accumulate) * 2.0 * n * hw);
    DistillMaps maps = {{pred_1, pred_2}, {goal_1, goal_2}, {grad_pred_1, grad_pred_2}};
    const bool vec = (hw & 3) == 0 && aligned16(pred_1) && aligned16(pred_2) && aligned16(goal_1) && aligned16(goal_2) && aligned16(boundaries) &&
                     aligned16(grad_pred_1) && aligned16(grad_pred_2);
    ENDO_CHECK(hipMemsetAsync(stats, 0, sizeof(double) * 3 * 2 * n, stream));
    const int per_block = kDistillThreads * kDistillItems;
    const dim3 rgrid((hw + per_block - 1) / per_block, 2 * n);
    const int items = vec ? hw >> 2 : hw;
    int ablocks = (items + kDistillThreads - 1) / kDistillThreads;
    if (ablocks > 1024) ablocks = 1024;
    const dim3 agrid(ablocks, 2 * n);
    if (vec) {
        distill_reduce<4><<<rgrid, kDistillThreads, 0, stream>>>(maps, boundaries, stats, n, hw, eps);
        if (accumulate)
            distill_apply<4, 1><<<agrid, kDistillThreads, 0, stream>>>(maps, boundaries, stats, losses, weight, n, hw, eps);
        else
            distill_apply<4, 0><<<agrid, kDistillThreads, 0, stream>>>(maps, boundaries, stats, losses, weight, n, hw, eps);
    } else {
        distill_reduce<1><<<rgrid, kDistillThreads, 0, stream>>>(maps, boundaries, stats, n, hw, eps);
        if (accumulate)
            distill_apply<1, 1><<<agrid, kDistillThreads, 0, stream>>>(maps, boundaries, stats, losses, weight, n, hw, eps);
        else
            distill_apply<1, 0><<<agrid, kDistillThreads, 0, stream>>>(maps, boundaries, stats, losses, weight, n, hw, eps);
    }
    ENDO_LAUNCH_CHECK();
    return 0;
}
