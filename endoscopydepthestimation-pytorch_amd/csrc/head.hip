// The loss head of a training iteration as ONE call: everything between the two network outputs and the gradient that goes back
// into the network (reference train.py:279-315 forward, and its autograd backward) -- depth scaling, flow from depth, boundary
// masking, sparse-flow loss, depth warping both ways, depth-consistency loss, the weighted sum, and the whole backward chain
// down to d loss / d prediction.  It composes the library's own entry points (geometry.hip, losses.hip), so the arithmetic is
// the modules'; what it removes is ~60 autograd nodes and as many host round trips between ~45 small launches: in the traced
// step the GPU sat idle for 0.35 ms there.  The backward half runs unconditionally (it is cheap); the caller still decides on
// the non-finite guard from the loss value before it differentiates the network.
// endo_loss_head_photo is the same body with the photometric term (image_warp.hip) in both directions: three launches more.
// endo_loss_head_forms is either of the two with the depth-consistency loss chosen (geometry.hip ConsistencyForm): the same launches.
#include "common.h"
#include "loss_device.h"

namespace endo {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// out = a + b + c + d  (c, d may be null)
__global__ void __launch_bounds__(256) head_add_kernel(float* __restrict__ out, const float* __restrict__ a, const float* __restrict__ b,
                                                       const float* __restrict__ c, const float* __restrict__ d, int64_t count) {
    for (int64_t i = (blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x) * 4; i < count; i += static_cast<int64_t>(gridDim.x) * blockDim.x * 4) {
        if (i + 3 < count) {
            f32x4 v = *reinterpret_cast<const f32x4*>(a + i);
            const f32x4 vb = *reinterpret_cast<const f32x4*>(b + i);
            v += vb;
            if (c) v += *reinterpret_cast<const f32x4*>(c + i);
            if (d) v += *reinterpret_cast<const f32x4*>(d + i);
            *reinterpret_cast<f32x4*>(out + i) = v;
        } else {
            for (int64_t k = i; k < count; ++k) out[k] = a[k] + b[k] + (c ? c[k] : 0.f) + (d ? d[k] : 0.f);
        }
    }
}

// losses[0..2] = total, dcl, sfl as train.py:299-315 forms them (fp32), losses[3] = 1 when the total is NaN / Inf (train.py:317) else 0: sfl = w_sfl * 0.5 * (a + b), dcl likewise, total = dcl + sfl;
// up[0] = d total / d (each sparse-flow term), up[1] = d total / d (each consistency term)
// out_j = a_j * mask (per sample, broadcast over a_j's channels) for up to six tensors in ONE launch: blockIdx.z = job.  The arithmetic of
// endo_mask_mul (geometry.hip mask_mul_kernel), which the head used to call once per tensor: six launches of ~5 us each, alone on the chip.
struct MaskMulJobs {
    const float* a[6];
    float* out[6];
    int c[6];
};
__global__ void __launch_bounds__(256) head_mask_mul_kernel(const MaskMulJobs jobs, const float* __restrict__ mask, int hw) {
    const int n = blockIdx.y;
    const float* __restrict__ a = jobs.a[0];
    float* __restrict__ out = jobs.out[0];
    int c = jobs.c[0];
#pragma unroll
    for (int j = 1; j < 6; ++j)
        if (blockIdx.z == j) { a = jobs.a[j]; out = jobs.out[j]; c = jobs.c[j]; }          // (no dynamic index into the kernel argument)
    const int64_t mbase = static_cast<int64_t>(n) * hw;
    const int64_t abase = mbase * c;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
        const float m = mask[mbase + i];
        for (int k = 0; k < c; ++k) out[abase + static_cast<int64_t>(k) * hw + i] = a[abase + static_cast<int64_t>(k) * hw + i] * m;
    }
}

__global__ void head_combine_kernel(const float* __restrict__ parts, float c_sfl, const float* __restrict__ dcl_weighted, float* __restrict__ losses,
                                    float* __restrict__ up) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const float sfl = c_sfl * (parts[0] + parts[1]);
        const float dcl = dcl_weighted[0];          // dcl_weight * 0.5 * (term_1 + term_2), from the fused consistency kernel
        const float total = dcl + sfl;
        losses[0] = total;
        losses[1] = dcl;
        losses[2] = sfl;
        losses[3] = (isnan(total) || isinf(total)) ? 1.f : 0.f;          // the guard of train.py:317, decided on the device
        up[0] = c_sfl;
    }
}

// head_combine_kernel with the photometric term: the two directions' terms from their reduction tables ([2][n][2] doubles:
// photometric_fwd_kernel's sums, image_warp.hip) by loss_device.h's masked_l1_mean, losses[4] = c_photo * (term_1 + term_2)
// added to the total before the non-finite test; up[2] = d total / d (each photometric term)
__global__ void head_combine_photo_kernel(const float* __restrict__ parts, float c_sfl, const float* __restrict__ dcl_weighted,
                                          const double* __restrict__ photo_stats, int n, float photo_eps, float c_photo,
                                          float* __restrict__ losses, float* __restrict__ up) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const float sfl = c_sfl * (parts[0] + parts[1]);
        const float dcl = dcl_weighted[0];
        const float photo = c_photo * (masked_l1_mean(photo_stats, n, photo_eps) + masked_l1_mean(photo_stats + 2 * n, n, photo_eps));
        const float total = dcl + sfl + photo;
        losses[0] = total;
        losses[1] = dcl;
        losses[2] = sfl;
        losses[3] = (isnan(total) || isinf(total)) ? 1.f : 0.f;
        losses[4] = photo;
        up[0] = c_sfl;
        up[2] = c_photo;
    }
}

}  // namespace endo

using namespace endo;

// (endo_consistency_phase: geometry.hip, declared in common.h)

// (endo_warp_consistency -- the depth-warp + consistency-loss chain as two fused kernels -- lives in geometry.hip.)

// The carving of endo_loss_head's workspace (offsets in floats), the one statement of it: endo_loss_head takes its pieces from here and
// endo_loss_head_planes reports the planes display.hip renders.  Every piece starts on a 4-float boundary, so plane-sized pieces stay
// 16-byte aligned when p % 4 == 0 (head_add_kernel copes otherwise).
struct HeadLayout {
    int64_t scaled_1, scaled_2;          // depth-scaled predictions
    int64_t flow_1, flow_2;              // flow from depth: raw, then masked in place
    int64_t msf_1, msf_2;                // sparse flows * boundary
    int64_t msm_1, msm_2;                // sparse flow masks * boundary
    int64_t cons;                        // endo_consistency_phase's own carving (warped, intersect, sums)
    int64_t g_flow_1, g_flow_2;          // d / d masked flow, then masked in place = d / d raw flow
    int64_t g_s1, g_s2;                  // d loss / d scaled depth: the flow terms, then += the consistency terms
    int64_t dstats;                      // fp64 reduction tables (depth scaling, sparse-flow loss, distance loss)
    int64_t parts, up, ratio;
    int64_t photo_1, photo_2;            // endo_loss_head_photo only: the photometric term's derivative planes, behind everything else
    int64_t end;
};

static HeadLayout head_layout(int n, int h, int w, bool photo = false) {
    const int64_t p = static_cast<int64_t>(n) * h * w;
    int64_t at = 0;
    auto take = [&](int64_t count) { const int64_t q = at; at += (count + 3) / 4 * 4; return q; };
    HeadLayout l;
    l.scaled_1 = take(p);       l.scaled_2 = take(p);
    l.flow_1 = take(2 * p);     l.flow_2 = take(2 * p);
    l.msf_1 = take(2 * p);      l.msf_2 = take(2 * p);
    l.msm_1 = take(p);          l.msm_2 = take(p);
    l.cons = take(endo_warp_consistency_workspace_floats(n, h, w));
    l.g_flow_1 = take(2 * p);   l.g_flow_2 = take(2 * p);
    l.g_s1 = take(p);           l.g_s2 = take(p);
    l.dstats = take(2 * (2 * 8 * n + 2 * n + 2 * 2 * n + 2 * 4 * n));
    l.parts = take(8);           // sfl_1, sfl_2, dcl_1, dcl_2
    l.up = take(4);              // upstream gradients of the four terms
    l.ratio = take(4);           // depth-scaling's second output (unused by the loss)
    l.photo_1 = l.photo_2 = at;
    if (photo) { l.photo_1 = take(p); l.photo_2 = take(p); }
    l.end = at;
    return l;
}

extern "C" int64_t endo_loss_head_workspace_floats(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return -1;
    const int64_t p = static_cast<int64_t>(n) * h * w;
    return 34 * p + 128 * n + 256;
}

extern "C" int64_t endo_loss_head_photo_workspace_floats(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return -1;
    const int64_t p = static_cast<int64_t>(n) * h * w;
    return 36 * p + 128 * n + 264;
}

// The body of endo_loss_head, endo_loss_head_photo and endo_loss_head_forms.  photo = false: colors_*, photo_weight and padding_mode are
// unused, losses has four floats, and the launches, values and workspace layout are endo_loss_head's.  form, form_eps: the
// depth-consistency loss (ENDO_CONSISTENCY_*) and its module's eps, handed to endo_consistency_phase.
static int loss_head_impl(bool photo, int form, float form_eps, const float* colors_1, const float* colors_2, float photo_weight, int padding_mode,
                          const float* pred_1, const float* pred_2, const float* boundaries, const float* sparse_depths_1,
                              const float* sparse_depths_2, const float* sparse_depth_masks_1, const float* sparse_depth_masks_2,
                              const float* sparse_flows_1, const float* sparse_flows_2, const float* sparse_flow_masks_1,
                              const float* sparse_flow_masks_2, const float* t_1_wrt_2, const float* r_1_wrt_2, const float* t_2_wrt_1,
                              const float* r_2_wrt_1, const float* intrinsics, float sfl_weight, float dcl_weight, float eps,
                              float* losses, float* grad_pred_1, float* grad_pred_2, float* workspace, int n, int h, int w, void* stream_) {
    if (!pred_1 || !pred_2 || !boundaries || !sparse_depths_1 || !sparse_depths_2 || !sparse_depth_masks_1 || !sparse_depth_masks_2 ||
        !sparse_flows_1 || !sparse_flows_2 || !sparse_flow_masks_1 || !sparse_flow_masks_2 || !t_1_wrt_2 || !r_1_wrt_2 || !t_2_wrt_1 ||
        !r_2_wrt_1 || !intrinsics || !losses || !grad_pred_1 || !grad_pred_2 || !workspace || n <= 0 || h <= 0 || w <= 0)
        return ENDO_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int hw = h * w;
    // ---- workspace carving (floats): head_layout ----
    const HeadLayout l = head_layout(n, h, w, photo);
    float* scaled_1 = workspace + l.scaled_1;  float* scaled_2 = workspace + l.scaled_2;
    float* flow_1 = workspace + l.flow_1;      float* flow_2 = workspace + l.flow_2;
    float* msf_1 = workspace + l.msf_1;        float* msf_2 = workspace + l.msf_2;
    float* msm_1 = workspace + l.msm_1;        float* msm_2 = workspace + l.msm_2;
    float* cons_ws = workspace + l.cons;
    float* g_flow_1 = workspace + l.g_flow_1;  float* g_flow_2 = workspace + l.g_flow_2;
    float* g_s1 = workspace + l.g_s1;          float* g_s2 = workspace + l.g_s2;
    double* dstats = reinterpret_cast<double*>(workspace + l.dstats);
    double* ds_stats_1 = dstats;            double* ds_stats_2 = ds_stats_1 + 8 * n;
    double* ds_work_1 = ds_stats_2 + 8 * n; double* ds_work_2 = ds_work_1 + n;
    double* l1_stats_1 = ds_work_2 + n;     double* l1_stats_2 = l1_stats_1 + 2 * n;
    double* nd_stats_1 = l1_stats_2 + 2 * n; double* nd_stats_2 = nd_stats_1 + 4 * n;
    float* parts = workspace + l.parts;
    float* up = workspace + l.up;
    float* ratio = workspace + l.ratio;
    int rc;
#define HEAD(call) do { rc = (call); if (rc) return rc; } while (0)
    // ---- forward (train.py:279-315) ----
    // one memset for the reduction tables of both frames' depth scaling (forward sums, backward work) and sparse-flow losses: 22 n doubles
    // (with the photometric term: + its 2 x 2 n sums, which take the first half of the unused table behind them)
    double* photo_stats = nd_stats_1;
    ENDO_CHECK(hipMemsetAsync(dstats, 0, sizeof(double) * (2 * 8 * n + 2 * n + 2 * 2 * n + (photo ? 2 * 2 * n : 0)), stream));
    HEAD(endo_depth_scale_fwd_impl(pred_1, sparse_depths_1, sparse_depth_masks_1, scaled_1, ratio, ds_stats_1, n, hw, eps, 0, stream));
    HEAD(endo_depth_scale_fwd_impl(pred_2, sparse_depths_2, sparse_depth_masks_2, scaled_2, ratio + 1, ds_stats_2, n, hw, eps, 0, stream));
    HEAD(endo_flow_from_depth_fwd(scaled_1, boundaries, t_1_wrt_2, r_1_wrt_2, intrinsics, flow_1, n, h, w, stream_));
    HEAD(endo_flow_from_depth_fwd(scaled_2, boundaries, t_2_wrt_1, r_2_wrt_1, intrinsics, flow_2, n, h, w, stream_));
    {
        int bx = (hw + 255) / 256;
        bx = bx > 1024 ? 1024 : bx;
        MaskMulJobs jobs{{sparse_flow_masks_1, sparse_flow_masks_2, sparse_flows_1, sparse_flows_2, flow_1, flow_2},
                         {msm_1, msm_2, msf_1, msf_2, flow_1, flow_2}, {1, 1, 2, 2, 2, 2}};
        head_mask_mul_kernel<<<dim3(bx, n, 6), 256, 0, stream>>>(jobs, boundaries, hw);
        ENDO_LAUNCH_CHECK();
    }
    HEAD(endo_sparse_l1_fwd_impl(msf_1, flow_1, msm_1, parts + 0, l1_stats_1, n, 2, hw, 1.0f, 0, stream));
    HEAD(endo_sparse_l1_fwd_impl(msf_2, flow_2, msm_2, parts + 1, l1_stats_2, n, 2, hw, 1.0f, 0, stream));
    // depth warp both ways + depth-consistency loss: the two fused kernels of endo_warp_consistency (geometry.hip); the forward one
    // leaves dcl_weight * 0.5 * (term_1 + term_2) in parts[4] and the backward coefficients in its workspace
    HEAD(endo_consistency_phase(1, scaled_1, scaled_2, boundaries, t_1_wrt_2, r_1_wrt_2, t_2_wrt_1, r_2_wrt_1, intrinsics, dcl_weight, eps,
                                parts + 4, g_s1, g_s2, cons_ws, n, h, w, 0, form, form_eps, stream));
    // the photometric term, both directions in one kernel: each frame's masked colours against the other's sampled at its own scaled
    // depth, under the intersect mask the consistency kernel has just written
    const float* ph_c1[2] = {colors_1, colors_2};
    const float* ph_c2[2] = {colors_2, colors_1};
    const float* ph_depth[2] = {scaled_1, scaled_2};
    const float* ph_t[2] = {t_1_wrt_2, t_2_wrt_1};
    const float* ph_r[2] = {r_1_wrt_2, r_2_wrt_1};
    float* ph_plane[2] = {workspace + l.photo_1, workspace + l.photo_2};
    if (photo) {
        float* inter_1 = nullptr;
        float* inter_2 = nullptr;
        endo_consistency_intersect_planes(cons_ws, n, h, w, &inter_1, &inter_2);
        const float* ph_inter[2] = {inter_1, inter_2};
        HEAD(endo_photometric_phase(1, 2, ph_c1, ph_c2, ph_depth, boundaries, ph_inter, ph_t, ph_r, intrinsics, photo_stats, ph_plane, nullptr,
                                    nullptr, 0, n, 3, h, w, 1.0f, padding_mode, stream));
        head_combine_photo_kernel<<<1, 64, 0, stream>>>(parts, static_cast<float>(static_cast<double>(sfl_weight) * 0.5), parts + 4, photo_stats,
                                                        n, 1.0f, static_cast<float>(static_cast<double>(photo_weight) * 0.5), losses, up);
    } else {
        head_combine_kernel<<<1, 64, 0, stream>>>(parts, static_cast<float>(static_cast<double>(sfl_weight) * 0.5), parts + 4, losses, up);
    }
    ENDO_LAUNCH_CHECK();
    // ---- backward ----
    HEAD(endo_sparse_l1_bwd(up + 0, msf_1, flow_1, msm_1, l1_stats_1, nullptr, g_flow_1, n, 2, hw, 1.0f, stream_));
    HEAD(endo_sparse_l1_bwd(up + 0, msf_2, flow_2, msm_2, l1_stats_2, nullptr, g_flow_2, n, 2, hw, 1.0f, stream_));
    {
        int bx = (hw + 255) / 256;
        bx = bx > 1024 ? 1024 : bx;
        MaskMulJobs jobs{{g_flow_1, g_flow_2}, {g_flow_1, g_flow_2}, {2, 2}};
        head_mask_mul_kernel<<<dim3(bx, n, 2), 256, 0, stream>>>(jobs, boundaries, hw);
        ENDO_LAUNCH_CHECK();
    }
    // the flow terms initialise d loss / d scaled depth (every element written), the consistency kernel adds its own
    HEAD(endo_flow_from_depth_bwd(g_flow_1, scaled_1, boundaries, t_1_wrt_2, r_1_wrt_2, intrinsics, g_s1, n, h, w, stream_));
    HEAD(endo_flow_from_depth_bwd(g_flow_2, scaled_2, boundaries, t_2_wrt_1, r_2_wrt_1, intrinsics, g_s2, n, h, w, stream_));
    HEAD(endo_consistency_phase(2, scaled_1, scaled_2, boundaries, t_1_wrt_2, r_1_wrt_2, t_2_wrt_1, r_2_wrt_1, intrinsics, dcl_weight, eps,
                                parts + 4, g_s1, g_s2, cons_ws, n, h, w, 0, form, form_eps, stream));
    if (photo) {          // += the photometric terms: stream order, one writer per element
        const float* ph_up[2] = {up + 2, up + 2};
        float* ph_grad[2] = {g_s1, g_s2};
        HEAD(endo_photometric_phase(2, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, photo_stats, ph_plane, ph_up,
                                    ph_grad, 1, n, 3, h, w, 1.0f, 0, stream));
    }
    HEAD(endo_depth_scale_bwd_impl(g_s1, nullptr, pred_1, sparse_depths_1, ds_stats_1, grad_pred_1, ds_work_1, n, hw, eps, 0, stream));
    HEAD(endo_depth_scale_bwd_impl(g_s2, nullptr, pred_2, sparse_depths_2, ds_stats_2, grad_pred_2, ds_work_2, n, hw, eps, 0, stream));
#undef HEAD
    return 0;
}

extern "C" int endo_loss_head(const float* pred_1, const float* pred_2, const float* boundaries, const float* sparse_depths_1,
                              const float* sparse_depths_2, const float* sparse_depth_masks_1, const float* sparse_depth_masks_2,
                              const float* sparse_flows_1, const float* sparse_flows_2, const float* sparse_flow_masks_1,
                              const float* sparse_flow_masks_2, const float* t_1_wrt_2, const float* r_1_wrt_2, const float* t_2_wrt_1,
                              const float* r_2_wrt_1, const float* intrinsics, float sfl_weight, float dcl_weight, float eps,
                              float* losses, float* grad_pred_1, float* grad_pred_2, float* workspace, int n, int h, int w, void* stream_) {
    return loss_head_impl(false, ENDO_CONSISTENCY_DISTANCE, 1.0e-5f, nullptr, nullptr, 0.0f, 0, pred_1, pred_2, boundaries, sparse_depths_1,
                          sparse_depths_2, sparse_depth_masks_1, sparse_depth_masks_2, sparse_flows_1, sparse_flows_2, sparse_flow_masks_1,
                          sparse_flow_masks_2, t_1_wrt_2, r_1_wrt_2, t_2_wrt_1, r_2_wrt_1, intrinsics, sfl_weight, dcl_weight, eps, losses,
                          grad_pred_1, grad_pred_2, workspace, n, h, w, stream_);
}

extern "C" int endo_loss_head_photo(const float* pred_1, const float* pred_2, const float* boundaries, const float* sparse_depths_1,
                                    const float* sparse_depths_2, const float* sparse_depth_masks_1, const float* sparse_depth_masks_2,
                                    const float* sparse_flows_1, const float* sparse_flows_2, const float* sparse_flow_masks_1,
                                    const float* sparse_flow_masks_2, const float* t_1_wrt_2, const float* r_1_wrt_2, const float* t_2_wrt_1,
                                    const float* r_2_wrt_1, const float* intrinsics, const float* colors_1, const float* colors_2,
                                    float sfl_weight, float dcl_weight, float photo_weight, float eps, int padding_mode, float* losses,
                                    float* grad_pred_1, float* grad_pred_2, float* workspace, int n, int h, int w, void* stream_) {
    if (!colors_1 || !colors_2 || padding_mode < 0 || padding_mode > 2 || !(photo_weight >= 0.0f)) return ENDO_E_BADARG;
    return loss_head_impl(true, ENDO_CONSISTENCY_DISTANCE, 1.0e-5f, colors_1, colors_2, photo_weight, padding_mode, pred_1, pred_2, boundaries,
                          sparse_depths_1, sparse_depths_2, sparse_depth_masks_1, sparse_depth_masks_2, sparse_flows_1, sparse_flows_2,
                          sparse_flow_masks_1, sparse_flow_masks_2, t_1_wrt_2, r_1_wrt_2, t_2_wrt_1, r_2_wrt_1, intrinsics, sfl_weight, dcl_weight,
                          eps, losses, grad_pred_1, grad_pred_2, workspace, n, h, w, stream_);
}

extern "C" int endo_loss_head_forms(const float* pred_1, const float* pred_2, const float* boundaries, const float* sparse_depths_1,
                                    const float* sparse_depths_2, const float* sparse_depth_masks_1, const float* sparse_depth_masks_2,
                                    const float* sparse_flows_1, const float* sparse_flows_2, const float* sparse_flow_masks_1,
                                    const float* sparse_flow_masks_2, const float* t_1_wrt_2, const float* r_1_wrt_2, const float* t_2_wrt_1,
                                    const float* r_2_wrt_1, const float* intrinsics, const float* colors_1, const float* colors_2,
                                    float sfl_weight, float dcl_weight, float photo_weight, float eps, int padding_mode, float* losses,
                                    float* grad_pred_1, float* grad_pred_2, float* workspace, int n, int h, int w, int form, float form_eps,
                                    void* stream_) {
    if (!endo_consistency_form_ok(form, form_eps) || !(photo_weight >= 0.0f)) return ENDO_E_BADARG;
    const bool photo = photo_weight > 0.0f;          // without the term: endo_loss_head's launches, four losses, colours unread
    if (photo && (!colors_1 || !colors_2 || padding_mode < 0 || padding_mode > 2)) return ENDO_E_BADARG;
    return loss_head_impl(photo, form, form_eps, colors_1, colors_2, photo_weight, padding_mode, pred_1, pred_2, boundaries, sparse_depths_1,
                          sparse_depths_2, sparse_depth_masks_1, sparse_depth_masks_2, sparse_flows_1, sparse_flows_2, sparse_flow_masks_1,
                          sparse_flow_masks_2, t_1_wrt_2, r_1_wrt_2, t_2_wrt_1, r_2_wrt_1, intrinsics, sfl_weight, dcl_weight, eps, losses,
                          grad_pred_1, grad_pred_2, workspace, n, h, w, stream_);
}

extern "C" int endo_loss_head_planes(int n, int h, int w, int64_t* offsets) {
    if (!offsets || n <= 0 || h <= 0 || w <= 0) return ENDO_E_BADARG;
    const HeadLayout l = head_layout(n, h, w);
    const int64_t planes[6] = {l.scaled_1, l.scaled_2, l.flow_1, l.flow_2, l.msf_1, l.msf_2};
    for (int i = 0; i < 6; ++i) offsets[i] = planes[i];
    return 0;
}
