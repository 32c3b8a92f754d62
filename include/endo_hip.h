/*
 * endo_hip.h -- C ABI of libendo_hip.so, the MI355X (gfx950) implementation of the training hot
 * path of EndoscopyDepthEstimation-Pytorch.
 *
 * The reference has no native layer: its "operator interface" for this path is a set of
 * torch.nn.Module classes whose forward() bottoms out in ATen kernels.  Each
 * entry point below replaces the ATen op sequence behind one of those modules; the file:line it
 * replaces is cited on every declaration.  The Python mirror of the reference's module API
 * (endoscopydepthestimation-pytorch_amd/{models,losses}.py) binds these symbols with ctypes --
 * INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - all pointers are DEVICE pointers to contiguous fp32 (or, where said, fp64 / u8 / i32) data on
 *     the current HIP device; images are NCHW; hw = H*W
 *   - the caller owns every buffer; the library keeps no pointer past the call (network handles
 *     excepted: endo_net_create/destroy own their descriptor tables only, never activations)
 *   - every call launches asynchronously on `stream` (a hipStream_t passed as void*), never
 *     synchronises the device, and is re-entrant per stream
 *   - return value: 0 = ok, > 0 = hipError_t, < 0 = argument error (ENDO_E_*)
 *   - `stats` / `work` arguments are small fp64 device scratch arrays that the call zeroes itself;
 *     the forward call's `stats` must be handed unchanged to the matching backward call
 *
 * Workspace contract (every entry point; tests/test_gpu_workspace_contract.py holds the library to it with guard bands around, and
 * NaN poison inside, every buffer the Python side allocates -- DESIGN.md 2.1)
 *   1. A call writes nothing outside [ptr, ptr + size) of the buffers it is given, where size is what the matching endo_*_floats /
 *      endo_*_bytes query returned (for an output tensor: its documented shape).  Where an argument carries the size
 *      (workspace_bytes), a short buffer is ENDO_E_BADARG, not an overrun.
 *   2. The contents of a workspace or output buffer ON ENTRY are ignored: whatever a call reads from one, it has written itself
 *      earlier in the same call.  NaN, stale results of another shape, or zeros give the same result.
 *   SCRATCH (no meaning once the call's work has passed `stream`): gradws, the 16-bit families' `ws`, winner_scratch, row_offsets, and
 *   the workspaces of endo_warp_consistency, endo_jpeg_decode_crop, endo_augment, endo_evaluate, endo_evaluate_posed, endo_display and
 *   endo_evaluate_validation.
 *   STATE, i.e. written by one call and read by a later one, so the caller must leave it untouched in between:
 *     - `tape` (both network families): written by *_fwd, read (never written) by the matching *_bwd;
 *     - `stats` of the geometry / loss modules, forward to backward (above);
 *     - the workspace of endo_loss_head: on return it holds the six planes endo_loss_head_planes describes, which endo_display
 *       reads; scratch again from the next endo_loss_head on it;
 *     - `grads` (ACCUMULATED into), `params`, `momentum`, `bn_running`, and the means / history of endo_validation_accumulate.
 *   An output whose documented extent depends on the data (the point rows of endo_point_cloud / endo_evaluate /
 *   endo_evaluate_validation: *count_out, frame_offsets, offsets) is written up to that extent only; rows behind it keep whatever
 *   they held.
 */
#ifndef ENDO_HIP_H
#define ENDO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENDO_E_BADARG (-1)
#define ENDO_E_UNSUPPORTED (-2)

/* library identification: returns ENDO_ABI_VERSION (bumped whenever the set of entry points or a signature changes).
 * 2: round 2 (adds the tiled warp entries, endo_relative_poses, endo_loss_head, endo_set_option, endo_net_tape_offset,
 * endo_jpeg_*, endo_point_brightness).
 * 3: round 3 -- kernel-form / precision options move from the process to the network handle: endo_net_set_option /
 * endo_net_get_option REPLACE endo_set_option and endo_set_wgrad_overlap (removed; no environment defaults any more);
 * adds endo_warp_consistency and endo_warp_fallback_blocks.
 * 4: round 3 -- the 16-bit-storage family (endo_net16_*, endo_net16h_*, endo_bf16_*, endo_f16_*).
 * 5: round 4 -- the non-finite-loss guard moves onto the device: endo_loss_head writes a FOURTH float (the flag),
 * endo_sgd_clip_step takes a `skip_flag` device pointer; endo_net16_offset what = 7; adds endo_hsv_full.
 * 6: round 6 -- adds endo_warp_consistency_bytes, the option ENDO_OPT_TD_PERSIST and the value ENDO_OPT_WINO_DGRAD = 3; since then
 * (unchanged by additions) endo_augment, endo_augment_workspace_bytes, endo_augment_frame_bytes and the endo_augment_frame
 * record; then endo_evaluate and endo_evaluate_workspace_bytes; then endo_loss_head_planes, endo_display, endo_display_workspace_bytes,
 * endo_display_panel_shape and endo_validation_accumulate; then endo_depth_metrics, endo_evaluate_validation,
 * endo_evaluate_validation_workspace_bytes and endo_evaluate_validation_panel_shape -- entry points only, no existing signature
 * changes: additive, so the version stays 6; then the option "MFMA X3" (id 6: fp32 products as three-term bf16 splits; retired and not reused) and the values
 * ENDO_OPT_WINO_FWD = 3 / 4 and ENDO_OPT_WGRAD_F34 = 2 are removed -- no entry point and no signature changes.
 * 7: the plan of a pass can be read: adds endo_net_last_plan, endo_net_plan_query, endo_net_plan_name and the option
 * ENDO_OPT_CHIP_DIVISOR; no existing signature changes; since then (unchanged by additions) endo_norm_l2_*, endo_norm_l1_*,
 * endo_weighted_l2_*, endo_masked_scale_inv_* and endo_sparse_l1_display_* (_fwd / _bwd each); then endo_warp_coordinates_* and
 * endo_image_warp_* (_fwd / _bwd each); then endo_photometric_workspace_floats, endo_photometric_fwd / _bwd,
 * endo_loss_head_photo_workspace_floats and endo_loss_head_photo; then endo_distill_head; then endo_evaluate_posed and
 * endo_evaluate_posed_workspace_bytes; then endo_warp_consistency_forms and endo_loss_head_forms. */
#define ENDO_ABI_VERSION 7
int endo_abi_version(void);
/* hipGetErrorString for positive codes, a fixed string for ENDO_E_* */
const char* endo_error_string(int code);

/* ---------------------------------------------------------------------------------------------
 * DepthScalingLayer.forward -- reference models.py:346-363
 * stats: n x 8 fp64  [sum sd*bin, sum bin, sum smap, sum above, sum smap^2, scale, std, -]
 * ratio: 1 fp32 = mean over the (N x N) broadcast of std_j / scale_i (the reference divides a
 *        (N,) tensor by a (N,1,1,1) tensor before torch.mean -- models.py:363)
 * ------------------------------------------------------------------------------------------- */
int endo_depth_scale_fwd(const float* pred, const float* sparse_depth, const float* sparse_mask,
                         float* scaled, float* ratio, double* stats,
                         int n, int hw, float eps, void* stream);
/* grad_scaled / grad_ratio may be NULL (output unused); work: n fp64 */
int endo_depth_scale_bwd(const float* grad_scaled, const float* grad_ratio,
                         const float* pred, const float* sparse_depth, const double* stats,
                         float* grad_pred, double* work,
                         int n, int hw, float eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * FlowfromDepthLayer.forward -- reference models.py:370-374 -> 433-451 -> 377-429
 * t: n x 3, R: n x 9 (row major), K: n x 9; flow: n x 2 x H x W
 * ------------------------------------------------------------------------------------------- */
int endo_flow_from_depth_fwd(const float* depth, const float* mask, const float* t, const float* R,
                             const float* K, float* flow, int n, int h, int w, void* stream);
int endo_flow_from_depth_bwd(const float* grad_flow, const float* depth, const float* mask,
                             const float* t, const float* R, const float* K, float* grad_depth,
                             int n, int h, int w, void* stream);

/* ---------------------------------------------------------------------------------------------
 * DepthWarpingLayer.forward -- reference models.py:460-465 -> 469-554, sampler models.py:325-336
 * (F.grid_sample bilinear / zeros / align_corners=False on the grid (2u/W-1, 2v/H-1))
 * warped, intersect: n x 1 x H x W.  Backward: grad_d1 written, grad_d2 zeroed then scatter-added.
 * ------------------------------------------------------------------------------------------- */
int endo_depth_warp_fwd(const float* depth_1, const float* depth_2, const float* mask,
                        const float* t, const float* R, const float* K,
                        float* warped, float* intersect,
                        int n, int h, int w, float eps, void* stream);
int endo_depth_warp_bwd(const float* grad_warped, const float* depth_1, const float* depth_2,
                        const float* mask, const float* t, const float* R, const float* K,
                        float* grad_d1, float* grad_d2,
                        int n, int h, int w, float eps, void* stream);
/* The same with an explicit LDS source-tile shape (geometry.hip "LDS-staged depth warp"): tile_h x tile_w in
 * {8x32, 16x32, 16x64, 32x32, 32x64}, or 0 x 0 for the L2-gather kernels; ENDO_E_UNSUPPORTED otherwise.  The entry points
 * above use the shape the sweep under profiles/ settled on.  Results do not depend on the shape (forward bit-identical,
 * the d2 gradient up to the order of its atomic additions). */
int endo_depth_warp_fwd_tiled(const float* depth_1, const float* depth_2, const float* mask,
                              const float* t, const float* R, const float* K,
                              float* warped, float* intersect,
                              int n, int h, int w, float eps, int tile_h, int tile_w, void* stream);
int endo_depth_warp_bwd_tiled(const float* grad_warped, const float* depth_1, const float* depth_2,
                              const float* mask, const float* t, const float* R, const float* K,
                              float* grad_d1, float* grad_d2,
                              int n, int h, int w, float eps, int tile_h, int tile_w, void* stream);
/* Test hook: blocks of the tiled kernels since the last reset whose source box did not fit the LDS staging buffers and that took
 * the gather path instead (large / divergent motion, e.g. the gap-scaled poses of BASELINE configs[4]); per process and device.
 * Copies two counters from the device (synchronises); either pointer may be null. */
int endo_warp_fallback_blocks(long long* forward, long long* backward, int reset);

/* ---------------------------------------------------------------------------------------------
 * _warp_coordinate_generate -- reference models.py:377-429: where the frame-1 pixels land in frame 2.
 * depth, mask, u, v: n x H x W (the reference's n x H x W x 1); t, R, K as above.  The arithmetic is endo_flow_from_depth_fwd's
 * before its ((u - x) / W, (v - y) / H): camera maps in fp64, zt = 1e30 (1 - m) + m z2, u = (w_x + d q_x) / zt.  A masked-out
 * pixel therefore lands at u ~ 0, v ~ 0, as in the reference.
 * Backward: grad_depth written in full; grad_u or grad_v may be NULL (= zero).
 * ------------------------------------------------------------------------------------------- */
int endo_warp_coordinates_fwd(const float* depth, const float* mask, const float* t, const float* R,
                              const float* K, float* u, float* v, int n, int h, int w, void* stream);
int endo_warp_coordinates_bwd(const float* grad_u, const float* grad_v, const float* depth, const float* mask,
                              const float* t, const float* R, const float* K, float* grad_depth,
                              int n, int h, int w, void* stream);

/* ---------------------------------------------------------------------------------------------
 * images_warping / _bilinear_interpolate -- reference models.py:317-336: F.grid_sample (bilinear, align_corners=False) of `images` on
 * the grid (2u/W - 1, 2v/H - 1), i.e. at the source location (u - 0.5, v - 0.5).
 * images, warped: n x C x H x W (any C >= 1); u, v: n x H x W pixel coordinates.
 * padding_mode: 0 zeros, 1 border (source location clipped to [0, W - 1]), 2 reflection (reflected over [-0.5, W - 0.5], then
 * clipped) -- ATen's transforms for align_corners=False; anything else is ENDO_E_BADARG.
 * A pixel whose source location is not finite (NaN or infinite u, v, or a u so large that the location overflows) gives 0 and gets
 * zero gradients in every mode; ATen's result there is undefined (it converts the location to an integer).
 * Backward: each of grad_images, grad_u, grad_v may be NULL, and its work is then skipped.  grad_images is zeroed by the call and
 * then scatter-added (fp32 atomics: the order of a pixel's additions is not fixed; zero terms are skipped, which spares the atomics of
 * the masked-out pixels of endo_warp_coordinates_fwd -- they all sample at pixel (0, 0) -- under a mask-weighted loss);
 * grad_u, grad_v are written in full and carry
 * the padding mode's factor 0 / +1 / -1 (grid_sample's W / 2 times the grid's 2 / W is 1).  No workspace.
 * ------------------------------------------------------------------------------------------- */
int endo_image_warp_fwd(const float* images, const float* u, const float* v, float* warped,
                        int n, int c, int h, int w, int padding_mode, void* stream);
int endo_image_warp_bwd(const float* grad_warped, const float* images, const float* u, const float* v,
                        float* grad_images, float* grad_u, float* grad_v,
                        int n, int c, int h, int w, int padding_mode, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The photometric term as one forward and one backward kernel: the chain
 *   [u, v] = _warp_coordinate_generate(depth, mask, t, R, K);  warped = images_warping(colors_2, u, v, padding_mode);
 *   loss = MaskedL1Loss(eps)([colors_1, warped, intersect])        (reference models.py:317-336, 377-429, losses.py:82-91)
 * with the per-term arithmetic of endo_warp_coordinates_fwd, endo_image_warp_fwd and endo_sparse_l1_fwd, without the planes u, v and
 * warped.  colors_1, colors_2: n x C x H x W (any C >= 1); depth, mask, intersect: n x 1 x H x W; t n x 3, R / K n x 9.
 * loss: one fp32 = mean over samples of num_n / (eps + den_n), num_n = sum intersect * sum_c |colors_1 - warped|, den_n = sum intersect
 * (once, not C times).  stats: n x 2 fp64 [num_n, den_n], zeroed by the call (fp64 atomics, one per block and sum: the order of the
 * additions is not fixed).  workspace: 16-byte aligned, endo_photometric_workspace_floats(n, h, w) floats; its contents on entry are
 * ignored, nothing outside it is written, and on return it holds d num_n / d depth per pixel -- STATE for endo_photometric_bwd.
 * Only the depth is differentiated.  A pixel whose coordinate is not finite samples nothing (warped = 0) and gets zero gradient.
 * Backward: grad_depth (n x 1 x H x W) = *grad_loss / n / (eps + den_n) * workspace; accumulate = 0 writes every element, 1 adds to
 * what is there (one writer per element, no atomics); anything else is ENDO_E_BADARG.  n, h, w, eps: the forward call's.
 * ------------------------------------------------------------------------------------------- */
int64_t endo_photometric_workspace_floats(int n, int h, int w);
int endo_photometric_fwd(const float* colors_1, const float* colors_2, const float* depth, const float* mask,
                         const float* intersect, const float* t, const float* R, const float* K,
                         float* loss, double* stats, float* workspace,
                         int n, int c, int h, int w, float eps, int padding_mode, void* stream);
int endo_photometric_bwd(const float* grad_loss, const double* stats, const float* workspace, float* grad_depth,
                         int accumulate, int n, int h, int w, float eps, void* stream);


/* ---------------------------------------------------------------------------------------------
 * SparseMaskedL1Loss.forward -- reference losses.py:62-66
 * flows, flows_hat: n x c x H x W; mask: n x 1 x H x W; stats: n x 2 fp64 [sum m|f-f^|, sum m]
 * ------------------------------------------------------------------------------------------- */
int endo_sparse_l1_fwd(const float* flows, const float* flows_hat, const float* mask,
                       float* loss, double* stats, int n, int c, int hw, float eps, void* stream);
/* grad_flows / grad_hat may be NULL when that input needs no gradient */
int endo_sparse_l1_bwd(const float* grad_loss, const float* flows, const float* flows_hat,
                       const float* mask, const double* stats, float* grad_flows, float* grad_hat,
                       int n, int c, int hw, float eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * NormalizedDistanceLoss.forward -- reference losses.py:122-146
 * stats: n x 4 fp64 [sum m*d, sum m, sum m|P-Pw|_1, sum m(d+|dw|)]
 * ------------------------------------------------------------------------------------------- */
int endo_norm_dist_fwd(const float* depth, const float* warped, const float* intersect,
                       const float* K, float* loss, double* stats,
                       int n, int h, int w, float eps, void* stream);
int endo_norm_dist_bwd(const float* grad_loss, const float* depth, const float* warped,
                       const float* intersect, const float* K, const double* stats,
                       float* grad_depth, float* grad_warped,
                       int n, int h, int w, float eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ScaleInvariantLoss.forward -- reference losses.py:22-32
 * stats: n x 3 fp64 [sum r^2, sum r, sum b]
 * ------------------------------------------------------------------------------------------- */
int endo_scale_inv_fwd(const float* pred, const float* goal, const float* boundary,
                       float* loss, double* stats, int n, int hw, float eps, void* stream);
int endo_scale_inv_bwd(const float* grad_loss, const float* pred, const float* goal,
                       const float* boundary, const double* stats,
                       float* grad_pred, float* grad_goal, int n, int hw, float eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The rest of the reference's losses.py.  As above: asynchronous on `stream`, ENDO_E_BADARG before any device work, `stats` is
 * zeroed by the forward and read by the backward, a NULL gradient pointer means that gradient is not requested.  All maps
 * n x hw fp32 (hw = C * H * W of one sample); masks, sparse depths and translations get no gradient.  Additive: the version stays 7.
 * MaskedL1Loss (losses.py:87-91) is endo_sparse_l1_* with c image channels and its n x 1 x H x W mask.
 *
 * NormalizedL2Loss.forward -- reference losses.py:99-109
 * stats: n x 4 fp64 [sum m*d, sum m, sum m(d-dw)^2, sum m(d^2+dw^2)]; the mean depth is a constant in the backward (no_grad)
 * ------------------------------------------------------------------------------------------- */
int endo_norm_l2_fwd(const float* depth, const float* warped, const float* mask,
                     float* loss, double* stats, int n, int hw, float eps, void* stream);
int endo_norm_l2_bwd(const float* grad_loss, const float* depth, const float* warped, const float* mask,
                     const double* stats, float* grad_depth, float* grad_warped,
                     int n, int hw, float eps, void* stream);
/* NormalizedL1Loss.forward -- reference losses.py:154-164
 * stats: n x 4 fp64 [sum m*d, sum m, sum m|d-dw|, sum m(|d|+|dw|)]; the mean depth IS differentiated (d 1e-5 mu / d depth) */
int endo_norm_l1_fwd(const float* depth, const float* warped, const float* mask,
                     float* loss, double* stats, int n, int hw, float eps, void* stream);
int endo_norm_l1_bwd(const float* grad_loss, const float* depth, const float* warped, const float* mask,
                     const double* stats, float* grad_depth, float* grad_warped,
                     int n, int hw, float eps, void* stream);
/* NormalizedWeightedMaskedL2Loss.forward -- reference losses.py:40-54.  translations: n x 3; the weights 1 / (1e-8 + |t_n|) are
 * formed on the device.  stats: n x 4 fp64 [sum m(d-dw)^2, sum m(d^2+dw^2), w_n, sum_n w_n] */
int endo_weighted_l2_fwd(const float* depth, const float* warped, const float* mask, const float* translations,
                         float* loss, double* stats, int n, int hw, float eps, void* stream);
int endo_weighted_l2_bwd(const float* grad_loss, const float* depth, const float* warped, const float* mask,
                         const double* stats, float* grad_depth, float* grad_warped,
                         int n, int hw, float eps, void* stream);
/* MaskedScaleInvariantLoss.forward -- reference losses.py:173-186.  r = 0 where sparse < 0.5 (selected, not multiplied), else
 * log(est + eps) - log(sparse).  stats: n x 3 fp64 [sum m r^2, sum m r, sum m].  The gradient goes to the estimations only. */
int endo_masked_scale_inv_fwd(const float* est, const float* sparse, const float* mask,
                              float* loss, double* stats, int n, int hw, float eps, void* stream);
int endo_masked_scale_inv_bwd(const float* grad_loss, const float* est, const float* sparse, const float* mask,
                              const double* stats, float* grad_est, int n, int hw, float eps, void* stream);
/* SparseMaskedL1LossDisplay.forward -- reference losses.py:74-79: endo_sparse_l1_fwd's sums, out: the (n,) per-sample vector and
 * no batch mean; grad_out: (n,) */
int endo_sparse_l1_display_fwd(const float* flows, const float* flows_hat, const float* mask,
                               float* out, double* stats, int n, int c, int hw, float eps, void* stream);
int endo_sparse_l1_display_bwd(const float* grad_out, const float* flows, const float* flows_hat,
                               const float* mask, const double* stats, float* grad_flows, float* grad_hat,
                               int n, int c, int hw, float eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The loss head of a training iteration in one call -- reference train.py:279-315 (depth scaling, flow from depth, boundary
 * masking, sparse-flow loss, depth warping both ways, depth-consistency loss, weighted sum) AND its backward down to
 * d loss / d prediction, composed from the entry points above (same kernels, same arithmetic; the modules remain for callers
 * that want the pieces).  pred_*: n x 1 x H x W network outputs; the other inputs are the batch tensors of train.py:245-270
 * (sparse flows n x 2 x H x W; t n x 3, R / K n x 9).  losses: FOUR fp32 on the device = total, depth-consistency, sparse-flow
 * (weights applied: w * 0.5 * (term_1 + term_2)) and the guard flag of train.py:317 (1.0 when the total is NaN / Inf, else 0.0).
 * grad_pred_*: n x 1 x H x W, written.  workspace: 16-byte aligned, endo_loss_head_workspace_floats(n, h, w) floats; its contents on entry
 * are ignored and nothing outside those floats is written; on return it is STATE until the next call on it (endo_loss_head_planes).  The caller
 * feeds grad_pred_* to endo_net_bwd without waiting for the host and hands &losses[3] (or its all-reduced sum) to
 * endo_sgd_clip_step as `skip_flag`: the reference's guarded branch also runs backward() and then a step() that changes nothing
 * (train.py:318-321).
 * ------------------------------------------------------------------------------------------- */
int64_t endo_loss_head_workspace_floats(int n, int h, int w);
int endo_loss_head(const float* pred_1, const float* pred_2, const float* boundaries,
                   const float* sparse_depths_1, const float* sparse_depths_2,
                   const float* sparse_depth_masks_1, const float* sparse_depth_masks_2,
                   const float* sparse_flows_1, const float* sparse_flows_2,
                   const float* sparse_flow_masks_1, const float* sparse_flow_masks_2,
                   const float* t_1_wrt_2, const float* r_1_wrt_2, const float* t_2_wrt_1, const float* r_2_wrt_1,
                   const float* intrinsics, float sfl_weight, float dcl_weight, float eps,
                   float* losses, float* grad_pred_1, float* grad_pred_2, float* workspace,
                   int n, int h, int w, void* stream);
/* offsets[6] (host int64, in floats from `workspace`) of six planes endo_loss_head leaves in its workspace: the scaled depths 1 and 2
 * (n x 1 x H x W each), the masked flows from depth 1 and 2 and the masked sparse flows 1 and 2 (n x 2 x H x W each) -- what
 * endo_display renders after a training or validation call, without a recompute.  The head's own carving, one function for both.
 * ENDO_E_BADARG for bad sizes or a null `offsets`. */
int endo_loss_head_planes(int n, int h, int w, int64_t* offsets);

/* endo_loss_head with the photometric term (above) in both directions added to the total:
 *   photo = photo_weight * 0.5 * (P(colors_1, colors_2 sampled at scaled depth 1, pose 1-wrt-2, intersect mask 1) + the roles swapped)
 * colors_*: n x 3 x H x W, the masked network inputs; the intersect masks are the ones the depth-consistency term has just formed, the
 * L1's eps is 1 (the reference module's default); padding_mode as endo_image_warp_fwd.  losses: FIVE fp32 = total (now dcl + sfl +
 * photo), dcl, sfl, the guard flag (which covers the new total), photo -- the first four keep endo_loss_head's positions.  The term's
 * depth gradients are added to those of the other terms before the depth scaling's backward, in stream order.  workspace:
 * endo_loss_head_photo_workspace_floats(n, h, w) floats under endo_loss_head's contract; endo_loss_head_planes' offsets hold for it
 * too.  ENDO_E_BADARG also for null colours, a padding mode outside 0..2 and a photo_weight that is negative or NaN.  With
 * photo_weight = 0 the values are endo_loss_head's (the term is still evaluated); callers without the term call endo_loss_head. */
int64_t endo_loss_head_photo_workspace_floats(int n, int h, int w);
int endo_loss_head_photo(const float* pred_1, const float* pred_2, const float* boundaries,
                         const float* sparse_depths_1, const float* sparse_depths_2,
                         const float* sparse_depth_masks_1, const float* sparse_depth_masks_2,
                         const float* sparse_flows_1, const float* sparse_flows_2,
                         const float* sparse_flow_masks_1, const float* sparse_flow_masks_2,
                         const float* t_1_wrt_2, const float* r_1_wrt_2, const float* t_2_wrt_1, const float* r_2_wrt_1,
                         const float* intrinsics, const float* colors_1, const float* colors_2,
                         float sfl_weight, float dcl_weight, float photo_weight, float eps, int padding_mode,
                         float* losses, float* grad_pred_1, float* grad_pred_2, float* workspace,
                         int n, int h, int w, void* stream);

/* The teacher-student term of a distillation iteration, both frames, forward AND backward, in one call -- reference
 * utils.py:1462-1482 (learn_from_teacher: torch.abs of both networks' outputs, ScaleInvariantLoss per frame under the boundary mask,
 * 0.5 * the sum) and losses.py:22-32.  Per frame f and sample s, with r = log(b |p| + eps) - log(b |g| + eps):
 *   S = sum b, R1 = sum r, R2 = sum r^2, L_s = R2 / S + R1^2 / S^2, term_f = mean_s L_s, distill = weight * 0.5 * (term_1 + term_2)
 *   d distill / d p_i = weight * 0.5 / n * (2 r_i / S + 2 R1 / S^2) * b_i * sgn(p_i) / (b_i |p_i| + eps),  sgn(0) = 0 as torch.abs
 * fp32 per element, fp64 sums (endo_scale_inv_*'s arithmetic).  pred_*: the student's outputs, goal_*: the teacher's (no gradient),
 * n x 1 x H x W each, of any sign; hw = H * W.  Two launches and the zeroing of `stats`.
 * losses: FIVE fp32 on the device = total, dcl, sfl, flag, distill -- endo_loss_head's four positions and the term fifth, as in
 * endo_loss_head_photo.  accumulate = 0: total = distill, dcl = sfl = 0, flag = 1.0 when the total is NaN / Inf else 0.0, grad_pred_*
 * written; what losses and grad_pred_* held on entry is ignored.  accumulate = 1: losses[0..3] and grad_pred_* hold what an
 * endo_loss_head earlier on the same stream left: total += distill, the flag stays 1 when it was 1 and becomes 1 when the new total
 * is not finite, dcl and sfl are kept, the term's gradient is ADDED to grad_pred_*.  losses[4] = distill in both.
 * stats: 2n x 3 fp64 [sum r^2, sum r, sum b], frame 1's n samples first; zeroed by the call, its contents on entry ignored.
 * ENDO_E_BADARG before any device work for null pointers, n or hw <= 0, accumulate not 0 / 1 and a weight that is negative or NaN.
 * Additive: the version stays 7. */
int endo_distill_head(const float* pred_1, const float* pred_2, const float* goal_1, const float* goal_2,
                      const float* boundaries, float weight, float eps, int accumulate,
                      float* losses, float* grad_pred_1, float* grad_pred_2, double* stats,
                      int n, int hw, void* stream);

/* Depth warp both ways + depth-consistency loss, forward AND backward, in one call -- reference models.py:454-554 (DepthWarpingLayer,
 * once per direction), losses.py:112-146 (NormalizedDistanceLoss, once per direction), train.py:305-314, and their backward:
 *   loss[0] = dcl_weight * 0.5 * (NDL(depth_1, warp(depth_2 -> 1)) + NDL(depth_2, warp(depth_1 -> 2)))
 *   grad_depth_k = d loss / d depth_k  (through the loss terms, the sampling grids and the sampled images)
 * depth_k: the (scaled) depth maps N x 1 x H x W; poses and intrinsics as endo_loss_head.  This is the chain BASELINE.json's second
 * metric times ("depth-warp fwd+bwd ms / pair").  workspace: endo_warp_consistency_workspace_floats(n, h, w) floats, 16-byte aligned:
 * scratch -- contents on entry ignored, nothing outside those floats written, as for loss and grad_depth_k (every element written). */
int64_t endo_warp_consistency_workspace_floats(int n, int h, int w);
/* algorithmic HBM bytes of one call (160 B per pixel of a frame pair, both directions, forward and backward) */
int64_t endo_warp_consistency_bytes(int n, int h, int w);
int endo_warp_consistency(const float* depth_1, const float* depth_2, const float* boundaries, const float* t_1_wrt_2,
                          const float* r_1_wrt_2, const float* t_2_wrt_1, const float* r_2_wrt_1, const float* intrinsics,
                          float dcl_weight, float eps, float* loss, float* grad_depth_1, float* grad_depth_2,
                          float* workspace, int n, int h, int w, void* stream);

/* The depth-consistency loss of the two calls below: which of the reference's four losses compares a depth map (a), the other frame's
 * warped into it (b) and the intersect mask (m).  Each is the arithmetic of its module's entry points above, inside the fused kernels:
 *   ENDO_CONSISTENCY_DISTANCE     NormalizedDistanceLoss          -- reference losses.py:112-146 (endo_norm_dist_*; its eps is the class
 *                                 default 1e-5 and form_eps is checked, then unused)
 *   ENDO_CONSISTENCY_L2           NormalizedL2Loss                -- reference losses.py:94-109  (endo_norm_l2_*), class default eps 1e-3
 *   ENDO_CONSISTENCY_L1           NormalizedL1Loss                -- reference losses.py:149-164 (endo_norm_l1_*), class default eps 1e-3
 *   ENDO_CONSISTENCY_WEIGHTED_L2  NormalizedWeightedMaskedL2Loss  -- reference losses.py:35-54   (endo_weighted_l2_*), class default eps 1;
 *                                 each direction's term is weighted over the batch by 1 / (1e-8 + |t_n|) of THAT direction's
 *                                 translations (t_1_wrt_2 for frame 1's term), as the reference's student training hands them over
 *                                 (utils.py:1700-1703)
 * A sample whose intersect mask is empty gives NaN under L2 and L1 (0 / 0, as the reference) and 0 under WEIGHTED_L2. */
#define ENDO_CONSISTENCY_DISTANCE 0
#define ENDO_CONSISTENCY_L2 1
#define ENDO_CONSISTENCY_L1 2
#define ENDO_CONSISTENCY_WEIGHTED_L2 3

/* endo_warp_consistency with the loss chosen -- reference models.py:454-554 once per direction, the loss class above once per direction,
 * train.py:305-314 with that class in NormalizedDistanceLoss's place, and their backward.  Arguments, workspace
 * (endo_warp_consistency_workspace_floats) and contract are endo_warp_consistency's; form = ENDO_CONSISTENCY_DISTANCE runs exactly that
 * call.  The other forms cost one launch more (the one-wave finalize that leaves the backward kernel's per-sample coefficients).
 * ENDO_E_BADARG also for an unknown form and a form_eps that is not finite and positive.  Additive: the version stays 7. */
int endo_warp_consistency_forms(const float* depth_1, const float* depth_2, const float* boundaries, const float* t_1_wrt_2,
                                const float* r_1_wrt_2, const float* t_2_wrt_1, const float* r_2_wrt_1, const float* intrinsics,
                                float dcl_weight, float eps, float* loss, float* grad_depth_1, float* grad_depth_2,
                                float* workspace, int n, int h, int w, int form, float form_eps, void* stream);

/* endo_loss_head / endo_loss_head_photo with the depth-consistency loss chosen -- reference train.py:279-315 with the class above in
 * NormalizedDistanceLoss's place (train.py:211, 305-314), and its backward.  Arguments as endo_loss_head_photo, then form and form_eps.
 * photo_weight > 0: endo_loss_head_photo's launches, FIVE losses, endo_loss_head_photo_workspace_floats.  photo_weight == 0: the
 * photometric term is not evaluated -- endo_loss_head's launches, FOUR losses, endo_loss_head_workspace_floats, and colors_* and
 * padding_mode are not read (the colours may be null).  endo_loss_head_planes' offsets hold in both.  form =
 * ENDO_CONSISTENCY_DISTANCE runs exactly endo_loss_head's / endo_loss_head_photo's kernels.  ENDO_E_BADARG also for an unknown form
 * and a form_eps that is not finite and positive.  Additive: the version stays 7. */
int endo_loss_head_forms(const float* pred_1, const float* pred_2, const float* boundaries,
                         const float* sparse_depths_1, const float* sparse_depths_2,
                         const float* sparse_depth_masks_1, const float* sparse_depth_masks_2,
                         const float* sparse_flows_1, const float* sparse_flows_2,
                         const float* sparse_flow_masks_1, const float* sparse_flow_masks_2,
                         const float* t_1_wrt_2, const float* r_1_wrt_2, const float* t_2_wrt_1, const float* r_2_wrt_1,
                         const float* intrinsics, const float* colors_1, const float* colors_2,
                         float sfl_weight, float dcl_weight, float photo_weight, float eps, int padding_mode,
                         float* losses, float* grad_pred_1, float* grad_pred_2, float* workspace,
                         int n, int h, int w, int form, float form_eps, void* stream);


/* ---------------------------------------------------------------------------------------------
 * train.py glue that is pure elementwise work between the modules
 *   endo_mask_mul: out[n,c,hw] = a[n,c,hw] * mask[n,0,hw]   (train.py:272-273, 293-298)
 * ------------------------------------------------------------------------------------------- */
int endo_mask_mul(const float* a, const float* mask, float* out, int n, int c, int hw, void* stream);

/* ---------------------------------------------------------------------------------------------
 * FCDenseNet57 -- reference models.py:100-194 (layers models.py:19-97)
 *
 * The network is driven through a handle that fixes (N, H, W) and owns only host-side launch
 * tables.  Parameters, gradients, BN buffers, activations and gradient workspaces live in caller
 * memory (torch tensors):
 *   params     fp32, the 210 trainable tensors packed in the reference's .parameters() order
 *   grads      fp32, same packing; endo_net_bwd ACCUMULATES into it (two forwards share one
 *              backward accumulation per step, train.py:276-277, 325)
 *   bn_running fp32, running_mean then running_var of the 49 BN layers in module order
 *   tape       fp32 activation workspace of endo_net_tape_floats() elements, written by fwd and
 *              read by bwd (one tape per forward call that will be differentiated).  fwd ignores what it
 *              held on entry (it clears the regions it accumulates into) and writes nothing outside those
 *              elements; between fwd and bwd it is STATE; bwd does not write it.
 *   gradws     fp32 gradient workspace of endo_net_gradws_floats() elements (scratch for bwd: contents on
 *              entry ignored, nothing outside those elements written, nothing kept from call to call).
 *              With several sample groups both sizes are groups x endo_net_group_stride() and each group
 *              works inside its own stride.  The fixed-size scratch regions inside both (split-K partials,
 *              weight-gradient partials, bias and final-convolution partials) are bounds over every input
 *              endo_net_create_grouped accepts; DESIGN.md 2.1 lists the inputs that come closest to each.
 *   out        n x 1 x H x W, every element written.
 * ------------------------------------------------------------------------------------------- */
typedef struct endo_net endo_net;

int endo_net_create(endo_net** out, int n, int h, int w);
/* Grouped batch: `groups` independent forward / backward passes of n samples each -- the two frames of a training
 * pair, train.py:276-277 -- run inside every kernel launch: x / out / grad_out hold groups * n samples, each
 * group keeps its own BatchNorm batch statistics (so the result equals `groups` separate calls, running statistics
 * updated in group order), parameter gradients sum over the groups.  tape and gradws are then groups *
 * endo_net_group_stride() floats (what endo_net_tape_floats / endo_net_gradws_floats return).  groups <= 4. */
int endo_net_create_grouped(endo_net** out, int n, int h, int w, int groups);
int endo_net_groups(const endo_net* net);
/* Kernel-form / precision options of ONE network handle (the reference's modules are independent objects, train.py:191,
 * 206-211: two models in one process, or a second thread configuring its own model, never change this one's arithmetic).
 * endo_net_create* sets the defaults below; nothing is read from the environment.  endo_net_set_option returns the previous
 * value, ENDO_E_BADARG for a null handle or an unknown option (the retired id 6 included); it takes effect with the next endo_net_fwd / endo_net_bwd on
 * that handle (a forward and the backward that differentiates it must run under the same ENDO_OPT_MFMA_BF16 value).
 * Every setting but ENDO_OPT_MFMA_BF16 computes the same function up to fp32 summation order; tests use
 * ENDO_OPT_WINO_MIN_TILES = 1 to reach the Winograd kernels at small sizes.
 *   ENDO_OPT_WINO_FWD        dense-layer forward at the fine levels: 0 direct convolution, 1 (or any other non-zero value) Winograd F(2x2,3x3),
 *                            5 (default since round 5) = F(4x4,3x3) for the launches whose 64 x 16 blocks fill the chip (level 0 at 256 x 320; csrc/wino4_fwd_kernels.h)
 *                            and F(2x2,3x3) below: +3 % frame-pairs/s; the depth is 5e-6 of its maximum from fp64 instead of 1e-6, against the
 *                            1e-4 of the parity target
 *   ENDO_OPT_WINO_DGRAD      fused base-channel data gradient at the fine levels: 0 direct, 1 Winograd with phase-skewed workers, one block per tile,
 *                            2 Winograd, the round-2 kernel, 3 (default) = 1 as persistent blocks that walk a run of tiles where that form applies
 *                            (csrc/dgrad_wino3p_kernels.h: at most 144 base channels; it also forms the final convolution's weight gradient of the
 *                            last up block's base channels)
 *   ENDO_OPT_DGRAD_VEC       new-channel data-gradient passes: 2 (default) = persistent blocks that walk a run of tiles (csrc/dgrad_newmap_kernels.h),
 *                            1 = one block per tile with 16-byte DMA of the gradient tiles, 0 = the same with dword DMA
 *   ENDO_OPT_WINO_MIN_TILES  tiles per launch from which a Winograd kernel is chosen (default 1024)
 *   ENDO_OPT_MFMA_BF16       NOT the same function: 1 = the dense layers' convolution kernels round their MFMA operands to bf16
 *                            (v_mfma_f32_16x16x16_bf16; fp32 accumulation, fp32 tensors in memory) -- the mixed-precision mode of
 *                            BASELINE configs[2], with its own tolerance; default 0 = fp32 operands.
 *                            Development values 2 * mask (mask bit 0 weight gradients, 1 forward, 2 data gradients) select families
 *   ENDO_OPT_WGRAD_OVERLAP   endo_net_bwd runs the weight gradients on a side stream of its own, overlapped with the data-gradient
 *                            chain and joined before it returns: 1 (default) = forked behind every gradient preparation;
 *                            2 = in the fused dense blocks ONE fork per block, behind its last preparation (its four weight gradients
 *                            start later; 22 instead of 55 event record / wait pairs per pass); 0 puts them back in line on the
 *                            caller's stream (clean per-kernel timings)
 *   ENDO_OPT_WGRAD_F34       dense-layer weight gradient where the height is a multiple of 16 and the width of 4 (levels 0-4 at 256 x 320): 1 (default) = in the
 *                            Winograd domain, F(3x3, 4x4) -- 36 multiplications per 4 x 4 tile of the output gradient instead of 144,
 *                            fp32 throughout (csrc/wgrad_f34_kernels.h); 0 = the direct kernels.  Ignored where ENDO_OPT_MFMA_BF16
 *                            selects rounded operands for the weight gradients.
 *   ENDO_OPT_FINAL_VIRTUAL   1 (default) = the data gradient of the final 1x1 convolution (models.py:167, 186), g(pixel) * w[channel] with
 *                            g = grad_out * sign(pre), is not written to the 192 level-0 gradient planes: g goes to one plane and the last up
 *                            block's backward kernels form the product where they first touch a channel (two passes over 1 GB less per
 *                            step at 16 x 256 x 320); the forward sum of that convolution over the 180 input channels of the network's last dense
 *                            layer is formed by that layer's F(4x4,3x3) launch (final_fwd_kernel reads 12 planes instead of 192), and the first
 *                            convolution's gradient preparation (G = d + P x + Q, bias gradient) is folded into its weight-gradient kernel;
 *                            0 = the separate kernels (final_bwd_data_kernel, the full final_fwd_kernel, prep_dy) as before.  Same function up
 *                            to summation order.
 *   ENDO_OPT_TD_PERSIST      transition-down layers (models.py:56-67) with 96 / 144 channels on whole 32 x 8 tiles (levels 0 / 1 of configs[1]) as
 *                            persistent blocks that keep the 1x1 weights in LDS: bit 0 (1) = the data gradient (csrc/td_dgrad_kernels.h; also the
 *                            128-pixel-run kernel where the pooled rows have no whole code dwords), bit 1 (2) = the training-mode forward
 *                            (csrc/td_fwd_kernels.h).  Default 3; 0 = the per-tile kernels (conv_dma_kernel).  Same function up to summation order.
 *   ENDO_OPT_CHIP_DIVISOR    d >= 1 (default 1; smaller values count as 1): plan as if the chip had 1 / d of its compute units.  Every comparison of
 *                            the plan that asks whether a launch fills the chip sees its tile or chunk count times d (the tile counts of the forward
 *                            and transition-up forms and the split-K slice arithmetic, the Winograd data gradient's tiles, the F(3x3,4x4) and
 *                            n-split minimums of the weight gradients), and the persistent launches are sized for 1 / d of the device's compute
 *                            units (at least one), rounded as each launch rounds.  Shape and alignment conditions are untouched.  For tests: a
 *                            grid of 1 / d of the benchmark's pixels takes the benchmark grid's kernel forms, and its persistent blocks walk as
 *                            many tiles each.  Same function up to summation order. */
#define ENDO_OPT_WINO_FWD 0
#define ENDO_OPT_WINO_DGRAD 1
#define ENDO_OPT_DGRAD_VEC 2
#define ENDO_OPT_WINO_MIN_TILES 3
#define ENDO_OPT_MFMA_BF16 4
#define ENDO_OPT_WGRAD_OVERLAP 5
/* id 6 is retired and not reused */
#define ENDO_OPT_WGRAD_F34 7
#define ENDO_OPT_FINAL_VIRTUAL 8
#define ENDO_OPT_TD_PERSIST 9
#define ENDO_OPT_CHIP_DIVISOR 10
#define ENDO_OPT_COUNT 11
int endo_net_set_option(endo_net* net, int option_id, int value);
int endo_net_get_option(const endo_net* net, int option_id);
int64_t endo_net_group_stride(const endo_net* net);
void endo_net_destroy(endo_net* net);
int64_t endo_net_param_floats(void);                 /* 1 374 865 */
int64_t endo_net_bn_floats(void);                    /* 2 * sum of BN widths */
int64_t endo_net_tape_floats(const endo_net* net);
int64_t endo_net_gradws_floats(const endo_net* net);
/* offset (in floats) of the i-th trainable tensor inside params/grads, i in [0, 210) */
int64_t endo_net_param_offset(int index);
/* offset of running_mean / running_var of the i-th BN layer inside bn_running, i in [0, 49) */
int64_t endo_net_bn_offset(int bn_index, int which /*0 mean, 1 var*/);

/* x: n x 3 x H x W (already multiplied by the boundary, train.py:272-273); out: n x 1 x H x W >= 0.
 * training != 0: batch statistics + running-stat update (momentum 0.1, eps 1e-5); 0: running stats.
 * The tape is always required (it also holds the level buffers the forward pass works in). */
int endo_net_fwd(endo_net* net, const float* params, float* bn_running, const float* x, float* out,
                 float* tape, int training, void* stream);
/* grad_out: n x 1 x H x W; x: the forward call's input.  Accumulates parameter gradients into grads.
 * The tape must come from a endo_net_fwd call with the same params, x and training flag. */
int endo_net_bwd(endo_net* net, const float* params, const float* x, const float* tape,
                 const float* grad_out, float* grads, float* gradws, int training, void* stream);
/* layout queries (tests inspect intermediate activations through these):
 * channel count of level buffer `level` (0..5) and its offset (floats) inside the tape */
int endo_net_level_channels(int level);
int64_t endo_net_act_offset(const endo_net* net, int level);
/* more of the tape's layout, for tests that rebuild the activation pattern a forward pass took (which ReLU inputs were
 * positive -- models.py:24, which pixel each 2x2 max-pool kept -- models.py:66, the sign under the final |.| --
 * models.py:186) so that gradients can be compared against an exact evaluation on the SAME pattern:
 *   ENDO_TAPE_PRE     (index ignored)        float offset of the final conv's pre-activation, n x 1 x H x W
 *   ENDO_TAPE_BN_SAVED index = BN layer in module order (0..48): float offset of its (mean, rstd) pairs, 2 per channel
 *   ENDO_TAPE_POOL    index = level 0..4:    BYTE offset of the argmax codes of that level's max-pool,
 *                                            n x C x H/2 x W/2 bytes, code = 2 * (row & 1) + (col & 1)
 * Offsets are inside one group's tape; group g of a grouped handle starts endo_net_group_stride() floats further.
 * Returns -1 for a bad argument. */
#define ENDO_TAPE_PRE 0
#define ENDO_TAPE_BN_SAVED 1
#define ENDO_TAPE_POOL 2
int64_t endo_net_tape_offset(const endo_net* net, int what, int index);

/* The plan of a pass: which kernel form every launch takes (csrc/net.hip: FwdPlan / BwdPlan), decided once at the top of endo_net_fwd /
 * endo_net_bwd from the grid, the handle's options, the training flag and the alignment of the pass's pointers.
 *   endo_net_last_plan   the plan the last endo_net_fwd (pass = ENDO_PASS_FWD) / endo_net_bwd (ENDO_PASS_BWD) on this handle followed
 *   endo_net_plan_query  the plan such a call WOULD follow with these pointers: the same two functions decide it, nothing is launched and
 *                        no pointer is dereferenced (any addresses of the right alignment do, on a machine without a GPU too).  The forward
 *                        query reads params, bn_running and tape; the backward query params, x, tape, grads and gradws.
 * Both write the plan as entries of four int32: (kind, index, level, value), every field of the plan's struct once, and return the
 * number of int32 written (ENDO_PLAN_MAX_INTS is enough for either pass).  ENDO_E_BADARG: a null handle or `out`, an unknown pass, a
 * pointer the pass reads is null, a buffer too short for the whole plan (its contents are then unspecified) -- and, from
 * endo_net_last_plan, a pass that has not run on this handle yet.
 *   index  dense layer 0..43 (= 4 * block + layer; blocks 0-4 the down path, 5 the bottleneck, 6-10 the up path, coarsest first) for
 *          DENSE_FWD*, DENSE_WGRAD and NEWMAP (the pass into layer j - 1's maps, j = 1..3); dense block 0..10 for BLOCK_BWD, BASE_PASS and
 *          WINO3_LAYOUT; level 0..4 for the transitions (TD_*: the level the transition-down reads, TU_*: the level the transition-up
 *          writes); 0 for the plan-wide fields
 *   level  the resolution level 0..5 the launch works at, -1 for plan-wide fields
 *   value  an enumerator of the kind (endo_net_plan_name gives its name) or, for the kinds marked [n], a number (0 / 1 for flags).
 *          NEWMAP, BASE_PASS and WINO3_LAYOUT of a block whose BLOCK_BWD is PerLayer are decided but not followed.
 * endo_net_plan_name(kind, value): the enumerator's name, the kind's own name for value = -1, NULL for anything else (static strings). */
#define ENDO_PASS_FWD 0
#define ENDO_PASS_BWD 1
#define ENDO_PLAN_MAX_INTS 1024
/* forward plan */
#define ENDO_PLAN_DENSE_FWD 0                 /* Wino4 Wino2_32x16 Wino2_32x8 SplitK Direct32x8 Direct16x8 DirectAuto */
#define ENDO_PLAN_DENSE_FWD_KSPLIT 1          /* [n] K slices of SplitK, else 0 */
#define ENDO_PLAN_DENSE_FWD_CHUNK_WEIGHTS 2   /* [n] the layer's prepared weights are in the direct kernel's K-chunk order */
#define ENDO_PLAN_FWD_BF16 3                  /* [n] */
#define ENDO_PLAN_WINO4_WEIGHTS 4             /* [n] */
#define ENDO_PLAN_FUSE_FINAL 5                /* [n] */
#define ENDO_PLAN_TD_FWD 6                    /* PerTile Persistent */
#define ENDO_PLAN_TU_FWD 7                    /* Upsample Subpix */
/* backward plan */
#define ENDO_PLAN_BLOCK_BWD 8                 /* PerLayer Fused */
#define ENDO_PLAN_NEWMAP 9                    /* Bf16 Persistent Vec16 Dword */
#define ENDO_PLAN_BASE_PASS 10                /* Block8 Block8Bf16 Wino3 Wino3Persistent Wino8 */
#define ENDO_PLAN_WINO3_LAYOUT 11             /* [n] */
#define ENDO_PLAN_DENSE_WGRAD 12              /* F34 NSplit Taps Direct */
#define ENDO_PLAN_TD_WGRAD 13                 /* Plain Dma */
#define ENDO_PLAN_TD_DGRAD 14                 /* Persistent Runs128 Dma Staged */
#define ENDO_PLAN_TU_WGRAD 15                 /* Subpix Taps Direct */
#define ENDO_PLAN_TU_DGRAD 16                 /* Subpix32x8 Subpix16x8 Subpix16x4 Plain */
#define ENDO_PLAN_WGRAD_OVERLAP 17            /* [n] ENDO_OPT_WGRAD_OVERLAP as set */
#define ENDO_PLAN_BF16_WGRAD 18               /* [n] */
#define ENDO_PLAN_BF16_DGRAD 19               /* [n] */
#define ENDO_PLAN_DGRAD_WEIGHTS 20            /* [n] */
#define ENDO_PLAN_USE_VIRT 21                 /* [n] */
#define ENDO_PLAN_VIRT_BASE 22                /* [n] */
#define ENDO_PLAN_VIRT_BASE_W 23              /* [n] */
#define ENDO_PLAN_MATERIALISE 24              /* [n] channels written out by the final convolution's data-gradient kernel */
#define ENDO_PLAN_C_FIRST 25                  /* [n] first channel of the final convolution's weight-gradient kernel */
#define ENDO_PLAN_FIRST_WGRAD 26              /* F34Prep F34 Taps Direct */
#define ENDO_PLAN_KIND_COUNT 27
int endo_net_last_plan(const endo_net* net, int pass, int32_t* out, int capacity);
int endo_net_plan_query(const endo_net* net, int pass, int training, const float* params, float* bn_running, const float* x,
                        float* tape, float* grads, float* gradws, int32_t* out, int capacity);
const char* endo_net_plan_name(int kind, int value);

/* ---------------------------------------------------------------------------------------------
 * WEIGHT-GRADIENT BRICKS of the fp32 family: each call is ONE weight-gradient launch of endo_net_bwd -- the network's own parameter
 * struct (WgradParams), launcher and template arguments, reached through the very function endo_net_bwd switches over the forms
 * in (csrc/net.hip: launch_dense_wgrad / launch_first_wgrad / launch_td_wgrad / launch_tu_wgrad) -- so that a test can hold a single
 * kernel to fp64 on operands of its own.  fp32 operands only (the ENDO_OPT_MFMA_BF16 forms stay with the network).  Additive: the
 * version stays 7.  Not covered by a brick: prep_dy_kernel, the bn_bwd_finalize kernels, final_bwd_weight_kernel.
 *
 *   kind  ENDO_WGRAD_DENSE  3x3, a = relu(bn(x)), 12 output channels     form: an enumerator of ENDO_PLAN_DENSE_WGRAD (F34 NSplit Taps Direct)
 *         ENDO_WGRAD_FIRST  3x3, a = x, cin <= 16, cout % 12 == 0        form: of ENDO_PLAN_FIRST_WGRAD (F34Prep F34 Taps Direct)
 *         ENDO_WGRAD_TD     1x1, a = relu(bn(x)), G un-routed            form: of ENDO_PLAN_TD_WGRAD (Plain Dma)
 *         ENDO_WGRAD_TU     3x3, a = nearest x2 of x                     form: of ENDO_PLAN_TU_WGRAD (Subpix Taps Direct)
 *
 * dw[co][ci][ky][kx] += sum over samples and pixels p of G[co][p] * a[ci][p + (ky - 1, kx - 1)] (a = 0 outside the image; 1x1: no
 * taps).  dw is fp32 [cout][cin][ks][ks], ACCUMULATED into; nothing outside it (and `scratch`, and prep_bias) is written.
 * Operands are planar fp32 with explicit strides, as the network holds them: sample s belongs to group s / group_n (group_n 0 or n:
 * one group; n a multiple of group_n, at most 4 groups) and is number nl = s % group_n in it;
 *   in      channel c of sample s starts at in + group * in_gs + nl * in_ns + c * in_cs: rows of in_w floats on the h x w grid (TU:
 *           the (h / 2) x (w / 2) grid).  The caller owns cin * in_cs floats from every sample's start (the F34 and Dma forms
 *           read them through a buffer descriptor of that extent and mask what lies outside the image; values there must be finite).
 *   dy      the prepared gradient G, channel co at dy + group * gs + nl * dy_ns + co * dy_cs, rows of dy_w floats on the h x w grid
 *           (TD: the pooled (h / 2) x (w / 2) grid); cout * dy_cs floats from every sample's start.
 *   saved / gamma / beta   DENSE and TD: a = relu(fma(x, sc, sh)), sc = gamma[c] * saved[2 c + 1], sh = fma(-saved[2 c], sc, beta[c]);
 *           group g reads saved + g * gs.  Ignored (may be null) for FIRST and TU.
 *   dy_idx  TD: bytes laid out as dy's floats (channel stride dy_cs BYTES, sample stride idx_ns, group stride 4 * gs bytes): the
 *           window position 2 * (row & 1) + (col & 1) that receives the pooled value.  h and w even.
 *   prep_x / prep_p / prep_q / prep_bias   FIRST, F34Prep only: dy holds the raw gradient d and the kernel forms G = d + P x + Q
 *           (prep_x laid out as dy; P, Q per output channel, group g at + g * gs) and adds sum G into prep_bias[cout] (may be null).
 *   scratch at least endo_wgrad_brick_scratch_floats(kind, form) floats (contents on entry ignored; 0: may be null).
 * endo_wgrad_brick_ok: 1 if the form accepts these operands, else 0 -- the form's own predicate of the plan (alignment of pointers
 *   and strides, channel counts, descriptor range) WITHOUT the tile / chunk minimum that makes the plan prefer another form at small
 *   sizes.  Needs no device and dereferences nothing.
 * endo_wgrad_brick: asynchronous on `stream`.  ENDO_E_BADARG before any device work for null pointers, sizes <= 0, strides
 *   shorter than what they span, scratch_cap below the query, an unknown (kind, form) or one whose endo_wgrad_brick_ok is 0.
 * endo_wgrad_brick_f34_batch: `count` (1..4) DENSE F34 launches, layer k into scratch slice k (scratch_cap >= count *
 *   endo_wgrad_brick_scratch_floats(DENSE, F34)), then ONE batched reduction -- what a fused dense block does.
 * ------------------------------------------------------------------------------------------- */
#define ENDO_WGRAD_DENSE 0
#define ENDO_WGRAD_FIRST 1
#define ENDO_WGRAD_TD 2
#define ENDO_WGRAD_TU 3
typedef struct endo_wgrad_operands {
    const float* in;
    int64_t in_ns;
    int32_t in_cs, in_w;
    const float* dy;
    int64_t dy_ns;
    int32_t dy_cs, dy_w;
    const float* saved;
    const float* gamma;
    const float* beta;
    const uint8_t* dy_idx;
    int64_t idx_ns;
    int64_t gs, in_gs;
    const float* prep_x;
    const float* prep_p;
    const float* prep_q;
    float* prep_bias;
    float* dw;
    int32_t group_n;
    int32_t n, h, w, cin, cout;
} endo_wgrad_operands;
int64_t endo_wgrad_brick_scratch_floats(int kind, int form);
int endo_wgrad_brick_ok(int kind, int form, const endo_wgrad_operands* a);
int endo_wgrad_brick(int kind, int form, const endo_wgrad_operands* a, float* scratch, int64_t scratch_cap, void* stream);
int endo_wgrad_brick_f34_batch(const endo_wgrad_operands* layers, int count, float* scratch, int64_t scratch_cap, void* stream);

/* ---------------------------------------------------------------------------------------------
 * clip_grad_norm_(params, max_norm) + SGD(momentum) -- reference train.py:327-328, 202
 * grads are scaled in place by grad_scale (1/world after the all-reduce) and then by the clip
 * coefficient min(1, max_norm / (norm + 1e-6)); momentum buf = mu * buf + g; p -= lr * buf.
 * first_step != 0: buf = g.  norm_out: 2 fp64 [sum of squares, pre-clip global L2 norm], written by the call.
 * skip_flag: null, or one fp32 on the device -- when it is non-zero (the non-finite-loss guard of train.py:317-322, endo_loss_head's
 * losses[3], summed over ranks by the gradient all-reduce) parameters and momentum are left untouched; norm_out is still written.
 * ------------------------------------------------------------------------------------------- */
int endo_sgd_clip_step(float* params, float* grads, float* momentum, double* norm_out,
                       int64_t count, float lr, float mu, float max_norm, float grad_scale,
                       int first_step, const float* skip_flag, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sparse SfM scatter -- reference utils.py:460-612 (get_torch_training_data) for a batch of pairs of ONE
 * sequence, on the device.  points [P][4] fp64 (homogeneous), projections [B][2][3][4] fp64,
 * extrinsics [B][2][4][4] fp64, visibility [B][P][2] (> 0.5 = the point is seen in that frame of the pair),
 * clean [P] or NULL (utils.py:496-497), mask [H][W] uint8 (255 = inside the endoscope boundary).
 * Outputs, zero-filled by the call, NCHW with the frame index outermost: depth_masks / depths / flow_masks
 * [2][B][1][H][W], flows [2][B][2][H][W] (u then v, divided by W and H; entries with |flow| > 5 zeroed,
 * utils.py:566-569,603-606).  depths are multiplied by depth_multiplier (1 = the reference function;
 * 1 / global_scale folds in dataset.py:391-392).  Pixel collisions: the highest point index wins (numpy
 * fancy-index assignment).  winner_scratch: 2*B*H*W int32 of workspace (scratch: contents on entry ignored,
 * nothing outside it written; the four outputs are written in full).
 * ------------------------------------------------------------------------------------------- */
int endo_sparse_scatter(const double* points, int n_points, const double* projections, const double* extrinsics,
                        const float* visibility, const float* clean, const uint8_t* mask, int batch, int height, int width,
                        float depth_multiplier, int32_t* winner_scratch, float* depth_masks, float* depths, float* flow_masks,
                        float* flows, void* stream);

/* Relative camera motion of a batch of frame pairs -- reference dataset.py:384-399, on the device.
 * pair_extrinsics [B][2][4][4] fp64 (world-to-camera of frame 1 and frame 2); scale = the sequence's estimated global scale.
 * relative = E_1 inv(E_2) in fp64;  r_1_wrt_2 [B][3][3] = fp32(relative[:3,:3]);  t_1_wrt_2 [B][3] = fp32(relative[:3,3] / scale);
 * r_2_wrt_1 = r_1_wrt_2^T;  t_2_wrt_1 = -r_1_wrt_2^T t_1_wrt_2 in fp32 -- the four pose tensors of a training batch, with no
 * host arithmetic and no host-to-device copy per sample. */
int endo_relative_poses(const double* pair_extrinsics, int batch, double scale,
                        float* r_1_wrt_2, float* t_1_wrt_2, float* r_2_wrt_1, float* t_2_wrt_1, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Coloured point cloud of one depth map -- reference utils.py:823-852 (point_cloud_from_depth), the per-frame
 * back-projection of evaluate.py:272,340.  depth, mask [H][W] fp32; color_bgr [H][W][3] uint8 (cv2 order);
 * intrinsics [3][3] fp32.  A pixel is kept when h % downsampling == 0, w % downsampling == 0, mask > 0.5 and, with
 * use_threshold != 0, max(r,g,b) >= max_threshold && min(r,g,b) <= min_threshold.  points receives
 * (x, y, z, r, g, b) = ((w - cx) / fx * z, (h - cy) / fy * z, z, r, g, b) per kept pixel in row-major pixel order
 * (capacity H * W rows of 6 floats); *count_out the number of rows written.  row_offsets: H + 1 int32 of workspace
 * (scratch: contents on entry ignored, nothing outside it written; rows of `points` behind *count_out are not written).
 * ------------------------------------------------------------------------------------------- */
int endo_point_cloud(const float* depth, const uint8_t* color_bgr, const float* mask, const float* intrinsics, int height,
                     int width, int downsampling, int use_threshold, float min_threshold, float max_threshold,
                     int32_t* row_offsets, float* points, int32_t* count_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Colour frames from the sequence folder's .jpg files -- reference utils.py:441-457 (get_pair_color_imgs: cv2.imread,
 * cv2.resize(img, (0, 0), fx = fy = 1 / downsampling), crop [start_h:end_h, start_w:end_w], BGR2RGB), utils.py:72-83
 * (get_test_color_img) and dataset.py:148,446-451 (albumentations Normalize(0.5, 0.5) + img_to_tensor).
 * Baseline / extended-sequential Huffman JPEG, 8 bit, one interleaved scan; grey, 4:4:4, 4:2:2 (h2v1) and 4:2:0 (h2v2);
 * restart intervals.  Anything else (progressive, arithmetic, 12 bit, CMYK) returns ENDO_E_UNSUPPORTED.
 *   endo_jpeg_info            host only.  info[16]: width, height, components, hmax, vmax, MCUs across, MCUs down,
 *                             (blocks across, blocks down) per component, total 8x8 blocks, restart interval, 0.
 *   endo_jpeg_entropy_decode  host only: the coefficient blocks the device stage starts from -- total_blocks x 64 int16,
 *                             component planes one after the other, blocks row-major inside a plane, coefficients in
 *                             natural (row-major, de-zigzagged) order, not dequantised; quant: [3][64] uint16, natural order.
 *   endo_jpeg_workspace_bytes bytes of `staging` (host; pinned for an asynchronous copy) and of `workspace` (device).  Both are
 *                             scratch: contents on entry ignored, nothing outside workspace_bytes written.
 *   endo_jpeg_decode_crop     parses and Huffman-decodes on the calling thread into `staging`, copies to `workspace` on
 *                             `stream` and launches the inverse DCT and the resize/crop kernels there.  out_hwc: device
 *                             uint8 [H][W][3] (rgb_order != 0: R,G,B as rgb_mode "rgb"; 0: B,G,R as cv2.imread) or NULL;
 *                             out_chw: device fp32 [3][H][W] = (v - 127.5) * (1 / 127.5) or NULL.  `staging` must stay
 *                             untouched until `stream` has passed the call.  Pixel values are those of libjpeg's default
 *                             decoder (JDCT_ISLOW, fancy upsampling) followed by cv2's 8-bit INTER_LINEAR arithmetic.
 * ------------------------------------------------------------------------------------------- */
int endo_jpeg_info(const uint8_t* data, int64_t size, int32_t* info);
int endo_jpeg_entropy_decode(const uint8_t* data, int64_t size, int16_t* blocks, int64_t capacity_blocks, uint16_t* quant);
int64_t endo_jpeg_workspace_bytes(const uint8_t* data, int64_t size);
int endo_jpeg_decode_crop(const uint8_t* data, int64_t size, double downsampling, int start_h, int end_h, int start_w,
                          int end_w, int rgb_order, uint8_t* out_hwc, float* out_chw, void* staging, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Contaminated-point filter, the per-pixel half -- reference utils.py:339-404 (get_clean_point_list), dataset.py:96-111.
 * imgs [frames][H][W][3] uint8 in cv2 order (B, G, R) as utils.get_color_imgs returns them (values, before the / 255);
 * points [P][4] fp64; projections [frames][3][4], extrinsics [frames][4][4] fp64; visibility [P][frames] fp32
 * (view_indexes_per_point); mask [H][W] uint8.  For frame f and point p (outputs [frames][P]): valid = visible > 0.5, projects
 * to 0 <= u <= W-1, 0 <= v <= H-1 with camera depth > 0, and mask[round(v)][round(u)] == 255 (round half to even); depth = the
 * camera depth; brightness = max(B, G, R) of cv2.bilateralFilter(img / 255, d, sigma_color, sigma_space) at that pixel (circular
 * window of radius d / 2, BORDER_REFLECT_101, colour distance |db| + |dg| + |dr|), evaluated only there.
 * ------------------------------------------------------------------------------------------- */
int endo_point_brightness(const uint8_t* imgs, int frames, int height, int width, const double* points, int n_points,
                          const double* projections, const double* extrinsics, const float* visibility, const uint8_t* mask,
                          int d, double sigma_color, double sigma_space, int32_t* valid, double* depth, float* brightness,
                          void* stream);

/* cv2.cvtColor(img, COLOR_BGR2HSV_FULL) (blue_index 0) / COLOR_RGB2HSV_FULL (blue_index 2) on 8-bit interleaved pixels -- the reader's
 * HSV input mode, reference utils.py:449-450, 80-81 and dataset.py:434-442 (`--use_hsv_colorspace`).  OpenCV's scalar fixed-point
 * arithmetic (H over [0, 256), tables round((255 << 12) / v), round((256 << 12) / (6 diff))); PARITY UNPINNED against cv2 itself (no
 * converted image in the reference tree).  src [pixels][3] uint8; out_u8 [pixels][3] (H, S, V) and / or out_f32 [3][pixels] =
 * (x / 255 - 0.5) / 0.5 (dataset.py:446-451); either may be null, src == out_u8 is allowed. */
int endo_hsv_full(const uint8_t* src, int64_t pixels, int blue_index, uint8_t* out_u8, float* out_f32, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training-phase augmentations -- reference train.py:121-142 (albumentations 0.4.6: OneOf colour / OneOf quality / OneOf noise),
 * applied to each frame of a pair with its own draws at dataset.py:432-447, then Normalize(0.5, 0.5) (dataset.py:446-451).
 * One record per frame says what that frame drew (host memory; built by augment.py from its sampler):
 *   colour   bit 0: every channel through rgb_lut (RandomBrightnessContrast then RandomGamma, composed on the host);
 *            bit 1: cv2.COLOR_RGB2HSV (8 bit, hue in [0, 180)) -> hsv_lut[0 / 1 / 2] on H / S / V -> cv2.COLOR_HSV2RGB
 *            (HueSaturationValue; OpenCV's scalar paths, PARITY UNPINNED against cv2 itself)
 *   spatial  0 none; 1 cv2.blur (BORDER_REFLECT_101); 2 cv2.medianBlur (BORDER_REPLICATE); 3 MotionBlur: cv2.filter2D with the
 *            k x k 0/1 mask `motion` (bit i * k + j = row i, column j; normalised to sum 1), BORDER_REFLECT_101, the mean of the
 *            marked taps rounded half to even (cv2's float path may differ by 1 at exact ties: unpinned).  ksize 3, 5 or 7.
 *   jpeg     1: JpegCompression, cv2.imencode(".jpg") + cv2.imdecode of the RGB array read as B, G, R: 4:2:0, libjpeg-turbo's
 *            islow FDCT and quantisation with the tables `quant` (natural order, luma then chroma, entries in [1, 255]), decoded
 *            as libjpeg (islow IDCT, fancy upsampling).  Bit-identical to libjpeg-turbo.
 *   noise    1 GaussNoise: clip(float(v) + sigma * n, 0, 255) truncated, n independent per pixel and channel;
 *            2 IAAAdditiveGaussianNoise: clip(round_half_even(v + sigma * n), 0, 255), one n per pixel shared by its 3 channels.
 *            n from Philox4x32-10 (key `seed`, counter (pixel, frame, 0, 0)) + Box-Muller: independent of the launch geometry.
 * ------------------------------------------------------------------------------------------- */
typedef struct endo_augment_frame {
    int32_t colour;
    int32_t spatial;
    int32_t ksize;
    int32_t jpeg;
    int32_t noise;
    float sigma;
    uint32_t seed[2];
    uint32_t motion[2];
    int32_t reserved[6];
    uint8_t rgb_lut[256];
    uint8_t hsv_lut[3][256];
    uint16_t quant[2][64];
} endo_augment_frame;
/* sizeof(endo_augment_frame) (1344), for bindings that mirror the record */
int endo_augment_frame_bytes(void);
/* device workspace bytes of endo_augment for `frames` frames of height x width (-1 for bad sizes).  The workspace is scratch: contents on
 * entry ignored, nothing outside workspace_bytes written; out_u8 / out_f32 are written in full. */
int64_t endo_augment_workspace_bytes(int frames, int height, int width);
/* src: device uint8 [frames][H][W][3] RGB (read only); params: HOST array of `frames` records, copied to the workspace on `stream`
 * (pinned memory for an asynchronous copy; untouched until `stream` has passed the call); out_u8: device uint8 [frames][H][W][3]
 * and / or out_f32: device fp32 [frames][3][H][W] = (v - 127.5) * (1 / 127.5); either may be NULL, out_u8 == src is allowed.
 * Five launches whatever the records hold (colour, spatial, JPEG encode, JPEG decode, noise + normalise).  H, W >= 4.
 * ENDO_E_BADARG for null pointers, bad sizes or a short workspace; ENDO_E_UNSUPPORTED for a record out of range (checked before the
 * workspace size: an unknown op code, ksize not in {3, 5, 7}, an empty or oversized motion mask, a quantisation entry outside
 * [1, 255], a negative or non-finite sigma). */
int endo_augment(const uint8_t* src, const endo_augment_frame* params, int frames, int height, int width, uint8_t* out_u8,
                 float* out_f32, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Test-phase outputs of a batch -- reference evaluate.py:329-345 (colour display, depth display, cv2.hconcat panel, point cloud)
 * with utils.py:825-865 (point_cloud_from_depth, write_point_cloud), for N frames at once; numpy's float32 roundings, bit for bit.
 * colors [N][3][H][W] fp32: boundaries * colours_1 (the masked, Normalize(0.5, 0.5) network input); boundaries [N][1][H][W] fp32 in
 * {0, 1}; predictions [N][1][H][W] fp32 (the network's output, >= 0); intrinsics [N][3][3] fp32.  Writes
 *   depth          [N][1][H][W] fp32   d = boundaries * predictions
 *   panels         [N][H][2W][3] uint8 B, G, R: columns [0, W) the colour display u8(b * C(u8(255 * (0.5 c + 0.5)))), C = RGB -> BGR
 *                                      or, is_hsv = 1, cv2.COLOR_HSV2BGR_FULL (OpenCV's 8-bit float path; PARITY UNPINNED against cv2);
 *                                      columns [W, 2W) COLORMAP_JET[u8(fl(255 d) / max(d))] (a frame whose max(d) is 0: entry 0
 *                                      everywhere; JET restated from its piecewise-linear curves, PARITY UNPINNED against cv2)
 *   points         capacity N * H * W rows of (x, y, z, r, g, b) fp32: every pixel with h % downsampling == 0, w % downsampling == 0
 *                                      and boundary > 0.5, frame-major, row-major inside a frame: endo_point_cloud's rows of (d, the
 *                                      colour display, b, K) bit for bit
 *   frame_offsets  [N + 1] int64       frame f's rows are [frame_offsets[f], frame_offsets[f + 1])
 * Three launches whatever N.  N <= 65535, N * H * W < 2^31.  ENDO_E_BADARG for null pointers, bad sizes, is_hsv not 0 / 1,
 * downsampling < 1 or a short workspace. */
/* device workspace bytes of endo_evaluate (-1 for bad sizes).  The workspace is scratch: contents on entry ignored, nothing outside
 * workspace_bytes written; depth, panels and frame_offsets are written in full, `points` up to frame_offsets[frames] rows. */
int64_t endo_evaluate_workspace_bytes(int frames, int height, int width);
int endo_evaluate(const float* colors, const float* boundaries, const float* predictions, const float* intrinsics, int frames,
                  int height, int width, int is_hsv, int point_cloud_downsampling, float* depth, uint8_t* panels, float* points,
                  int64_t* frame_offsets, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Test output in the electromagnetic tracker's frame -- reference utils.py:1316-1355 (write_test_output_with_initial_pose: colour image,
 * depth image) with utils.py:1246-1295 (point_cloud_from_depth_and_initial_pose) and utils.py:773-781 (display_depth_map), for N frames
 * at once; numpy's float32 / float64 roundings under numpy 2's scalar promotion, bit for bit.  colors, boundaries, predictions,
 * intrinsics: as endo_evaluate.  rotations [N][3][3] fp64 and translations [N][3] fp64: each frame's pose in the tracker's frame
 * (reader.read_initial_pose_file).  Writes
 *   depth          [N][1][H][W] fp32    d = boundaries * predictions
 *   color_images   [N][H][W][3] uint8   u8(255 * clip(0.5 c + 0.5, 0, 1)), NOT multiplied by the boundary again and WITHOUT an RGB -> BGR
 *                                       swap: channel k of an RGB input is channel k of the image, as the reference hands it to
 *                                       cv2.imwrite; is_hsv = 1: cv2.COLOR_HSV2BGR_FULL of it, so B, G, R (PARITY UNPINNED against cv2)
 *   depth_images   [N][H][W][3] uint8   B, G, R: COLORMAP_JET[u8(|(d - min) / (max - min) * 255|)] with the frame's whole-map min and max,
 *                                       above 255 -> 255, at or below 0 -> 0 (a frame with max == min, 0 / 0 in the reference: entry 0)
 *   points         capacity N * H * W rows of (x, y, z, r, g, b) fp32, frame-major, row-major inside a frame: every KEPT pixel
 *                                       (h % downsampling == 0, w % downsampling == 0, boundary > 0.5) that, with use_thresholds = 1,
 *                                       also has max(r, g, b) >= max_threshold and min(r, g, b) <= min_threshold.
 *                                       p = ((w - cx) / fx * d, (h - cy) / fy * d, d) * scale in fp32, scale = 20 / (z_max - z_min) over
 *                                       the frame's KEPT pixels; (x, y, z) = fp32(((R_i0 p_x + R_i1 p_y) + R_i2 p_z) + t_i) in fp64, no
 *                                       contraction; (r, g, b) = channels (2, 1, 0) of the colour image, as the reference reads them
 *   frame_offsets  [N + 1] int64        frame f's rows are [frame_offsets[f], frame_offsets[f + 1])
 *   frame_ranges   [N][2] fp32          (z_min, z_max) of the frame's kept pixels; (+inf, -inf) when there is none (the reference raises
 *                                       ZeroDivisionError there).  z_max == z_min: scale = inf and the frame's coordinates are not finite,
 *                                       as in the reference
 * Three launches whatever N.  N <= 65535, N * H * W < 2^31.  ENDO_E_BADARG for null pointers, bad sizes, is_hsv or use_thresholds not
 * 0 / 1, NaN thresholds in use, downsampling < 1 or a short workspace. */
/* device workspace bytes of endo_evaluate_posed (-1 for bad sizes).  The workspace is scratch: contents on entry ignored, nothing
 * outside workspace_bytes written; depth, both images, frame_offsets and frame_ranges are written in full, `points` up to
 * frame_offsets[frames] rows.  The outputs and the workspace must not overlap the inputs or one another: the write launch reads the
 * boundaries and the row offsets again after frame_ranges and depth have been written. */
int64_t endo_evaluate_posed_workspace_bytes(int frames, int height, int width);
int endo_evaluate_posed(const float* colors, const float* boundaries, const float* predictions, const float* intrinsics,
                        const double* rotations, const double* translations, int frames, int height, int width, int is_hsv,
                        int point_cloud_downsampling, int use_thresholds, float min_threshold, float max_threshold, float* depth,
                        uint8_t* color_images, uint8_t* depth_images, float* points, int64_t* frame_offsets, float* frame_ranges,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Display panel of a training or validation batch -- reference train.py:353-371 / 460-478 (utils.display_color_depth_sparse_flow_
 * dense_flow for both frames, draw_flow, stack_and_display, utils.py:868-900, 965-994, over torchvision 0.7-era make_grid; always
 * color_reverse = True, as train.py passes it).  out: [8 rows_per_section][cols][3] uint8 R, G, B (endo_display_panel_shape), the
 * sections c1, d1, sf1, df1, c2, d2, sf2, df2 top to bottom, each make_grid(nrow = 8, padding = 2, pad_value = 0) of the batch
 * (N = 1: the frame itself, unpadded) -- what a tensorboardX SummaryWriter.add_image stores for the reference's float image:
 *   c   trunc(clip(255 (0.5 c + 0.5)))                         colors_k [N][3][H][W]: the masked network input (train.py:272-273)
 *   d   COLORMAP_JET[u8(255 norm(b d))], B, G, R -> R, G, B    depths_k [N][1][H][W] (multiplied by `boundaries` [N][1][H][W] here),
 *       norm per frame: (clamp(x) - min) / fl32(max - min + 1e-5)   padding: JET entry 0
 *   sf  draw_flow(sparse_flows_k) [N][2][H][W]                  HSV (trunc(ang 90 / pi), 255, trunc(min(v / max_v, 1) 255)), cv2's
 *   df  draw_flow(flows_k, max_v of sf)  [N][2][H][W]           8-bit COLOR_HSV2BGR then BGR -> RGB; padding black; max_v = 0: V = 0
 * numpy's / torch's float32 roundings throughout, the angle the correctly rounded float32 atan2.  JET and the HSV conversion are
 * restated (PARITY UNPINNED against cv2, not installed).  Two launches whatever N.  N <= 65535, N * H * W < 2^31.  workspace: 16-byte
 * aligned, endo_display_workspace_bytes(n, h, w) bytes, scratch: contents on entry ignored, nothing outside those bytes written; `out` is
 * written in full.  ENDO_E_BADARG for null pointers, bad sizes or a short workspace. */
int64_t endo_display_workspace_bytes(int n, int h, int w);
int endo_display_panel_shape(int n, int h, int w, int* rows, int* cols);
int endo_display(const float* colors_1, const float* colors_2, const float* depths_1, const float* depths_2, const float* boundaries,
                 const float* sparse_flows_1, const float* sparse_flows_2, const float* flows_1, const float* flows_2, int n, int h, int w,
                 uint8_t* out, void* workspace, int64_t workspace_bytes, void* stream);

/* Running means of the validation pass -- reference train.py:446-456, in fp64 with the Python float's roundings.  losses: the
 * device [total, dcl, sfl] floats of batch `batch_index` (endo_loss_head's first three); means: 3 fp64 on the device, updated in
 * place: unchanged when the total is NaN (Inf is accumulated), the losses at batch 0, (mean k + loss) / (k + 1.0) at batch k > 0.
 * history: null, or fp64 [>= batch_index + 1][3] whose row batch_index receives the means after the update (train.py:481-483 logs
 * them per batch).  One single-thread launch. */
int endo_validation_accumulate(const float* losses, int batch_index, double* means, double* history, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Depth error measures against the sparse reconstruction -- reference losses.py:189-227 (AbsRelError.forward, Threshold.forward; the
 * reference defines them and calls them nowhere).  scaled_depths, sparse_depths, sparse_masks [N][1][H][W] fp32; out [N][4] fp32:
 * per sample the absolute relative error and sigma 1, 2, 3 (the share of masked pixels whose ratio is below 1.25, 1.25^2, 1.25^3).
 * Per-pixel terms with torch's float32 operations and IEEE division:
 *   abs rel     (m |d - s|) / (eps + s)
 *   threshold   m max(d m / (eps + s), s / (eps + d m)) + (1 - m) 10    (torch.max: a NaN side is kept; 0 * inf = NaN counts nowhere)
 * The abs-rel terms and the mask are summed in fp64 and rounded once, the counts are integers, the four quotients are float32.  An
 * empty mask gives NaN in all four (the reference's 0 / 0).  One launch, one block per sample; no workspace: nothing but out[N][4] is
 * written, and all of it.  N <= 65535, N * H * W < 2^31.  ENDO_E_BADARG for null pointers or bad sizes. */
int endo_depth_metrics(const float* scaled_depths, const float* sparse_depths, const float* sparse_masks, int n, int h, int w, float eps,
                       float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Validation-phase outputs of a batch of pairs -- reference evaluate.py:201-274: the 12-section picture of
 * utils.display_color_sparse_depth_dense_depth_warped_depth_sparse_flow_dense_flow (both frames) and stack_and_display
 * (utils.py:894-954, over torchvision 0.7-era make_grid; color_reverse = True, rgb_mode = "rgb"), the point cloud of
 * utils.point_cloud_from_depth (utils.py:825-852), and the measures of endo_depth_metrics for both frames.  Inputs, fp32:
 *   colors_k [N][3][H][W] the masked network input (evaluate.py:189-190); boundaries [N][1][H][W]; depths_k [N][1][H][W] the scaled
 *   depth, unmasked; sparse_depths_k, sparse_masks_k [N][1][H][W]; warped_2_to_1 / warped_1_to_2 [N][1][H][W] (evaluate.py:218-223);
 *   sparse_flows_k, flows_k [N][2][H][W] the masked sparse flows and flows from depth (evaluate.py:191-192, 215-216); intrinsics
 *   [N][3][3].
 * Writes
 *   panel    [12 rows_per_section][cols][3] uint8 R, G, B (endo_evaluate_validation_panel_shape): c1 sd1 d1 wd1 sf1 df1 c2 sd2 d2 wd2
 *            sf2 df2 top to bottom, each make_grid(nrow = 8, padding = 2, pad_value = 0) of the batch (N = 1: the frame itself) -- the
 *            bytes of evaluate.py:269-270's np.uint8(image_display * 255) and of the writer's add_image:
 *     c        trunc(fl(fl(fl(0.5 c + 0.5) b) 255)): masked pixels are 0
 *     sd d wd  COLORMAP_JET[u8(255 norm(x))], B, G, R -> R, G, B, x = sparse depth, b * depth, warped depth; norm(x) =
 *              (clamp(x, min, max) - min) / fl32(max - min + 1e-5) with ONE (min, max) per frame side: of b * depth over the whole
 *              batch (utils.py:921-922); padding: JET entry 0
 *     df sf    draw_flow(flows_k), then draw_flow(sparse_flows_k, max_v of df) (utils.py:942-943: the dense flows set the scale,
 *              the other way round from endo_display); HSV as endo_display's, padding black, max_v = 0: V = 0
 *   metrics  [N][2][4] fp32: endo_depth_metrics' four numbers of (depths_k, sparse_depths_k, sparse_masks_k), the same bits
 *   points   capacity N * H * W rows of (x, y, z, r, g, b) fp32: frame 1 of every pair, every pixel with h % downsampling == 0,
 *            w % downsampling == 0 and boundary > 0.5, pair-major, row-major inside a frame: endo_point_cloud's rows of (depths_1
 *            UNMASKED, u8(255 (0.5 c + 0.5)) of colors_1, boundaries, K) bit for bit
 *   offsets  [N + 1] int64: pair f's rows are [offsets[f], offsets[f + 1])
 * Deviations from the reference: it forms the point colours with cv2.COLOR_HSV2BGR_FULL whatever the colour space
 * (evaluate.py:202-203), which scrambles RGB input; here they are the frame's own R, G, B, as the test phase takes them
 * (evaluate.py:329-334).  is_hsv = 1 (the float COLOR_HSV2RGB_FULL path of the colour section) is not implemented: ENDO_E_BADARG.
 * numpy's / torch's float32 roundings throughout; JET and the HSV conversion are restated (PARITY UNPINNED against cv2).
 * Three launches whatever N.  Every H, W >= 1 with N <= 65535 and N * H * W < 2^31 (one section's rows and columns must be 32-bit
 * numbers; endo_evaluate_validation_panel_shape also needs 12 rows_per_section to be one).  workspace: 16-byte aligned,
 * endo_evaluate_validation_workspace_bytes(n, h, w) bytes (-1 for bad sizes), scratch: contents on entry ignored, nothing outside
 * those bytes written; panel, metrics and offsets are written in full, `points` up to offsets[N] rows.  ENDO_E_BADARG for null
 * pointers, bad sizes, is_hsv != 0, downsampling < 1, a misaligned or a short workspace. */
int64_t endo_evaluate_validation_workspace_bytes(int n, int h, int w);
int endo_evaluate_validation_panel_shape(int n, int h, int w, int* rows, int* cols);
int endo_evaluate_validation(const float* colors_1, const float* colors_2, const float* boundaries, const float* depths_1,
                             const float* depths_2, const float* sparse_depths_1, const float* sparse_depths_2,
                             const float* sparse_masks_1, const float* sparse_masks_2, const float* warped_2_to_1,
                             const float* warped_1_to_2, const float* sparse_flows_1, const float* sparse_flows_2, const float* flows_1,
                             const float* flows_2, const float* intrinsics, int n, int h, int w, float eps, int is_hsv,
                             int point_cloud_downsampling, uint8_t* panel, float* metrics, float* points, int64_t* offsets,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* live per-kernel-family timing for bench.py's roofline line: HIP events recorded on the launch
 * stream around every entry of the selected families.  family_mask: bit f enables family f
 * (0 = off, -1 = all); calling it also discards previously recorded events.  endo_prof_read
 * synchronises on the recorded events and returns totals (ms, launches, algorithmic flops/bytes) of the TIMED launches.
 * endo_prof_sample(period): time one launch in `period` of each enabled family (default 1 = every launch) -- two events around a
 * launch on the caller's stream serialise it with its neighbours, and a family of 44 launches per step then costs the step 3 %; a
 * period coprime with the family's launches per step visits every launch of the step in rotation.  endo_prof_seen: launches of
 * an enabled family since endo_prof_enable, timed or not. */
#define ENDO_PROF_FAMILIES 16
int endo_prof_enable(int family_mask);
int endo_prof_sample(int period);
int endo_prof_seen(int family, int64_t* launches);
int endo_prof_read(int family, double* total_ms, int64_t* launches, double* total_flops, double* total_bytes);
const char* endo_prof_family_name(int family);

/* ---------------------------------------------------------------------------------------------
 * bf16-STORAGE family (BASELINE configs[2] / [4]): bf16 level buffers in 32-channel blocks
 * ([n][t / blk][h][w][blk] bf16; blk = t is plain channels-last) and the convolution over them on the bf16 matrix cores
 * (v_mfma_f32_16x16x32_bf16, fp32 accumulation), with BatchNorm + ReLU applied once per staged element (reference models.py:19-28:
 * DenseLayer; 70-80: TransitionUp).
 *   endo_bf16_pack_nhwc / unpack_nhwc   fp32 NCHW <-> a channel slice of a bf16 buffer (round to nearest even); blk 0 = t
 *   endo_bf16_conv_weights              W[cout][cin][ks][ks] fp32 -> the kernel's bf16 layout (endo_bf16_conv_weight_elems elements)
 *   endo_bf16_conv                      out[.., oc0 : oc0 + cout] = conv_ks([nearest x2]([relu(x * scale + shift)])) + bias
 *                                       bn: [cin][2] fp32 (scale, shift) or null; out_sums: [cout][2] fp64, accumulated, or null
 * Constraints: ks in {1, 3}; cin, cout, oc0, out_blk multiples of 4; ic0, in_blk multiples of 8; t a multiple of blk.
 * ------------------------------------------------------------------------------------------- */
int endo_bf16_pack_nhwc(const float* x, void* out, int n, int c, int h, int w, int t, int blk, int oc0, void* stream);
int endo_bf16_unpack_nhwc(const void* in, float* x, int n, int c, int h, int w, int t, int blk, int ic0, void* stream);
int64_t endo_bf16_conv_weight_elems(int cout, int cin, int ks);
int endo_bf16_conv_weights(const float* w, int cout, int cin, int ks, void* out, void* stream);
int endo_bf16_conv(const void* in, int in_t, int in_blk, int ic0, int cin, const float* bn, const void* wgt, const float* bias, void* out,
                   int out_t, int out_blk, int oc0, int cout, double* out_sums, int n, int h, int w, int ks, int ups, void* stream);
/* FCDenseNet57 FORWARD over bf16 level buffers (reference models.py:171-187): same parameters / running statistics / input / output
 * tensors as endo_net_fwd (fp32), activations stored as bf16 in 32-channel blocks, BatchNorm statistics and the output in fp32.  The input is
 * rounded to bf16 on the way in.  training != 0: batch statistics + running-statistics update; 0: running statistics (the
 * evaluate.py path).  tape: endo_net16_tape_bytes() bytes of device memory, 256-byte aligned.  H and W multiples of 32.
 * endo_net16_bwd: its backward pass.  tape: the forward call's tape, untouched since; grad_out: fp32 [n][1][H][W]; grads: the flat
 * fp32 parameter-gradient buffer (offsets of endo_net_param_offset), ACCUMULATED into; ws: endo_net16_bwd_workspace_bytes() bytes (scratch: contents on entry ignored, nothing outside them written -- every
 * launch is checked against that size),
 * 256-byte aligned; training as in the forward call (0: BatchNorm as a fixed affine map).  Gradients between layers are stored as
 * bf16; BatchNorm sums (fp64), parameter gradients and the deferred BatchNorm terms (fp32) are not. */
typedef struct endo_net16 endo_net16;
/* n_per_group x groups samples per call (groups 1 or 2): every group has its own BatchNorm batch statistics and the running statistics are
 * updated with group 0's first -- one call with groups = 2 equals the reference's two network calls of a training step (train.py:276-277) */
int endo_net16_create(endo_net16** out, int n_per_group, int h, int w, int groups);
void endo_net16_destroy(endo_net16* net);
int64_t endo_net16_tape_bytes(const endo_net16* net);
int endo_net16_fwd(endo_net16* net, const float* params, float* bn_running, const float* x, float* out, void* tape, int training,
                   void* stream);
int64_t endo_net16_bwd_workspace_bytes(const endo_net16* net);
/* 1 (default): endo_net16_bwd runs the weight gradients on a side stream of its own, forked from and joined back into the caller's
 * stream by events before it returns; 0: everything in line on the caller's stream */
int endo_net16_set_wgrad_overlap(endo_net16* net, int on);
/* The same family over IEEE HALF storage (BASELINE configs[4]: "mixed fp16 storage / fp32 accum"): identical signatures and buffer
 * layouts (csrc/net16h.hip compiles the bf16 sources with another element type), v_mfma_f32_16x16x32_f16, and a power-of-two gradient
 * scale chosen per backward call from max |grad_out| (per-pixel gradients of a mean loss are far below half's smallest normal):
 * stored gradients carry it, parameter gradients leave without it.  endo_f16_pack_nhwc / unpack_nhwc: the layout helpers for half. */
int endo_net16h_create(endo_net16** out, int n_per_group, int h, int w, int groups);
void endo_net16h_destroy(endo_net16* net);
int64_t endo_net16h_tape_bytes(const endo_net16* net);
int endo_net16h_fwd(endo_net16* net, const float* params, float* bn_running, const float* x, float* out, void* tape, int training,
                    void* stream);
int64_t endo_net16h_bwd_workspace_bytes(const endo_net16* net);
int endo_net16h_set_wgrad_overlap(endo_net16* net, int on);
int64_t endo_net16h_offset(const endo_net16* net, int what, int index);
int endo_net16h_bwd(endo_net16* net, const float* params, const void* tape, const float* grad_out, float* grads, void* ws, int training,
                    void* stream);
int endo_f16_pack_nhwc(const float* x, void* out, int n, int c, int h, int w, int t, int blk, int oc0, void* stream);
int endo_f16_unpack_nhwc(const void* in, float* x, int n, int c, int h, int w, int t, int blk, int ic0, void* stream);
/* the forward brick over half storage: endo_bf16_conv_weight_elems / _conv_weights / _conv with the other element type */
int64_t endo_f16_conv_weight_elems(int cout, int cin, int ks);
int endo_f16_conv_weights(const float* w, int cout, int cin, int ks, void* out, void* stream);
int endo_f16_conv(const void* in, int in_t, int in_blk, int ic0, int cin, const float* bn, const void* wgt, const float* bias, void* out,
                  int out_t, int out_blk, int oc0, int cout, double* out_sums, int n, int h, int w, int ks, int ups, void* stream);
/* ---------------------------------------------------------------------------------------------
 * BACKWARD BRICKS of the 16-bit-storage family: each entry is ONE launch of endo_net16_bwd / endo_net16h_bwd (the network's own
 * parameter struct, launcher and template arguments), so that a test can hold a single kernel to fp64.  endo_bf16_* over bf16,
 * endo_f16_* over half; buffers are [n][t / blk][h][w][blk] (blk 0 = t).  All are asynchronous on `stream` and return ENDO_E_BADARG
 * before any device work for null pointers, sizes <= 0, channel ranges outside their buffer and the alignments named below.
 * Additive: the version stays 7.  Not covered by a brick: bf16_prep_dy_kernel, the two bn_finalize kernels, bf16_final_bwd_kernel.
 *
 * endo_bf16_dgrad_weights: W[cout][cin][ks][ks] fp32 -> the DATA-GRADIENT layout (rows = the layer's input channels in groups of 48,
 *   k = its output channels, taps flipped; endo_bf16_dgrad_weight_elems elements), one layer through the kernel that converts all of
 *   them.  rot / rot_n: row r < rot_n holds input channel (r + rot) % rot_n (0, 0 = none).  base / koff: rows below `base` (a
 *   multiple of 48; ks = 3, koff + cout <= 32) are stored as the dense-block kernel's LDS image -- output channel co at k = koff + co,
 *   16-byte slot k / 8 at position (k / 8) XOR (row >> 1) & 3; rows from `base` on have co at k = co.
 *
 * endo_bf16_wgrad: dw[co][(ci + rot) % rot_n][ky][kx] += sum over pixels of G[co][y][x] * a[ci][y + ky - 1][x + kx - 1] (ks = 1: no taps),
 *   dw fp32 [cout][cin_w][ks][ks], ACCUMULATED into; nothing outside it is written.  a: channels [ac0, ac0 + cin) of the forward
 *   buffer (a_t channels; the last 8-channel unit is read whole: ac0 + cin rounded up to 8 <= a_t), on the (h / 2) x (w / 2) grid
 *   if ups (nearest x2).  saved non-null: a = relu(x * sc + sh) rounded to the storage type, sc = gamma[pc] * saved[2 pc + 1],
 *   sh = fma(-saved[2 pc], sc, beta[pc]), pc = (ci + rot) % rot_n for ci < rot_n; sample n uses the table gs_saved floats further on
 *   if n >= group_n > 0 (n <= 2 group_n).  g: channels [gc0, gc0 + cout) of the prepared gradient (g_t channels) on the h x w grid,
 *   or -- g_idx non-null, ks = 1 -- on the pooled (h / 2) x (w / 2) grid with g_idx [n][h / 2][w / 2][cout] bytes naming the window
 *   position 2 dy + dx that receives the value.  cin_w: input channels of dw (0 = cin).  gscale: {S, 1 / S} or null: dw receives the
 *   sum times 1 / S.  partial: scratch of partial_cap floats, at least endo_bf16_wgrad_partial_floats(n, h, w, cin, cout, ks) (a
 *   shorter one is ENDO_E_BADARG; contents on entry ignored).  cin, cout % 4, ac0 % 8, a_blk % 8, gc0 % 4, g_blk % 4; ks = 1: cout,
 *   gc0, g_blk % 8; h, w even with ups or g_idx; cin_w <= cin; rot < rot_n <= cin.
 *
 * endo_bf16_dgrad_bn: the data gradient of BN -> ReLU -> conv with respect to input channels [co_off, co_off + cout) of a layer with
 *   layer_cin inputs and gcount outputs: dz = conv(g[gc0 : gc0 + gcount], wgt) with wgt from endo_bf16_dgrad_weights(gcount outputs,
 *   layer_cin inputs), da = [x * sc + sh > 0] * dz (sc, sh as above at (ci + rot) % rot_n), out[ci] += sc * da (read-modify-write,
 *   stored with stochastic rounding keyed by position and sr_salt: the same inputs give the same bits), out_sums[2 ci] += sum da,
 *   out_sums[2 ci + 1] += sum da * x (fp64, ACCUMULATED; group 1's gs_out_sums doubles later; out_sums_slot_stride > 0: eight copies
 *   that many doubles apart, a block adds to one of them and the reader adds them up).  out and x: out_t channels, same positions.
 *   ks = 3, in_idx null: a dense layer's new-map sub-range (co_off a multiple of 48, gc0 % 4);  ks = 1 with in_idx: the transition
 *   down (co_off = 0, cout = layer_cin, gcount and gc0 % 8, h and w even, g and in_idx on the (h / 2) x (w / 2) grid, in_idx
 *   [n][h / 2][w / 2][gcount] bytes).  Any other combination is ENDO_E_BADARG.
 *
 * endo_bf16_dgrad_sumpool: transition up: dz = conv3x3(g[gc0 : gc0 + gcount], wgt) on the h x w grid (even), its 2 x 2 sums added
 *   to channels [oc0, oc0 + cout) of the (h / 2) x (w / 2) buffer `out` (read-modify-write, stochastic rounding); out_sums[2 c] +=
 *   the pixel sum of what channel c received (fp64 [cout][2], ACCUMULATED).  gc0 % 8, oc0 % 4.
 *
 * endo_bf16_dgrad_block: a dense block's four layers with respect to its base channels [0, c0) in one launch: d is the gradient
 *   buffer (t channels; the layers' prepared gradients at [gc0 + 12 j, + 12), gc0 >= c0, gc0 % 8; base channels read-modify-written),
 *   x the forward buffer of the same geometry; wgt / saved / gamma / beta / sums: HOST arrays of four device pointers (layer j:
 *   weights from endo_bf16_dgrad_weights(12, c0 + 12 j, 3, rot, rot_n, c0, {0, 12, 8, 20}[j]), its tables, its fp64 sums as above).
 *   c0 a multiple of 48.
 * ------------------------------------------------------------------------------------------- */
int64_t endo_bf16_dgrad_weight_elems(int cout, int cin, int ks);
int endo_bf16_dgrad_weights(const float* w, int cout, int cin, int ks, int rot, int rot_n, int base, int koff, void* out, void* stream);
int64_t endo_bf16_wgrad_partial_floats(int n, int h, int w, int cin, int cout, int ks);
int endo_bf16_wgrad(const void* a, int a_t, int a_blk, int ac0, int cin, int cin_w, int ups, const float* saved, const float* gamma,
             const float* beta, int rot, int rot_n, int group_n, int64_t gs_saved, const void* g, int g_t, int g_blk, int gc0, int cout,
             const void* g_idx, const float* gscale, float* partial, int64_t partial_cap, float* dw, int n, int h, int w, int ks,
             void* stream);
int endo_bf16_dgrad_bn(const void* g, int g_t, int g_blk, int gc0, int gcount, const void* wgt, int layer_cin, void* out, const void* x, int out_t,
                int out_blk, int co_off, int cout, const float* saved, const float* gamma, const float* beta, int rot, int rot_n, int group_n,
                int64_t gs_saved, double* out_sums, int64_t gs_out_sums, int64_t out_sums_slot_stride, unsigned sr_salt, const void* in_idx,
                int n, int h, int w, int ks, void* stream);
int endo_bf16_dgrad_sumpool(const void* g, int g_t, int g_blk, int gc0, int gcount, const void* wgt, void* out, int out_t, int out_blk, int oc0,
                     int cout, double* out_sums, unsigned sr_salt, int n, int h, int w, void* stream);
int endo_bf16_dgrad_block(void* d, const void* x, int t, int blk, int gc0, int c0, const void* const* wgt, const float* const* saved,
                   const float* const* gamma, const float* const* beta, double* const* sums, int rot, int rot_n, int group_n,
                   int64_t gs_saved, int64_t gs_sums, int64_t sums_slot_stride, unsigned sr_salt, int n, int h, int w, void* stream);
int64_t endo_f16_dgrad_weight_elems(int cout, int cin, int ks);
int endo_f16_dgrad_weights(const float* w, int cout, int cin, int ks, int rot, int rot_n, int base, int koff, void* out, void* stream);
int64_t endo_f16_wgrad_partial_floats(int n, int h, int w, int cin, int cout, int ks);
int endo_f16_wgrad(const void* a, int a_t, int a_blk, int ac0, int cin, int cin_w, int ups, const float* saved, const float* gamma,
             const float* beta, int rot, int rot_n, int group_n, int64_t gs_saved, const void* g, int g_t, int g_blk, int gc0, int cout,
             const void* g_idx, const float* gscale, float* partial, int64_t partial_cap, float* dw, int n, int h, int w, int ks,
             void* stream);
int endo_f16_dgrad_bn(const void* g, int g_t, int g_blk, int gc0, int gcount, const void* wgt, int layer_cin, void* out, const void* x, int out_t,
                int out_blk, int co_off, int cout, const float* saved, const float* gamma, const float* beta, int rot, int rot_n, int group_n,
                int64_t gs_saved, double* out_sums, int64_t gs_out_sums, int64_t out_sums_slot_stride, unsigned sr_salt, const void* in_idx,
                int n, int h, int w, int ks, void* stream);
int endo_f16_dgrad_sumpool(const void* g, int g_t, int g_blk, int gc0, int gcount, const void* wgt, void* out, int out_t, int out_blk, int oc0,
                     int cout, double* out_sums, unsigned sr_salt, int n, int h, int w, void* stream);
int endo_f16_dgrad_block(void* d, const void* x, int t, int blk, int gc0, int c0, const void* const* wgt, const float* const* saved,
                   const float* const* gamma, const float* const* beta, double* const* sums, int rot, int rot_n, int group_n,
                   int64_t gs_saved, int64_t gs_sums, int64_t sums_slot_stride, unsigned sr_salt, int n, int h, int w, void* stream);
/* byte offsets into the tape (what 0: final pre-activation fp32; 1: (mean, rstd) of BatchNorm `index` in module order; 2: max-pool
 * codes of transition down `index` ([n][h / 2][w / 2][cout] bytes); 3: level buffer `index`) or the backward workspace (4: gradient
 * buffer of level `index`); 5: channels of level buffer `index`; 7: bytes between two sample groups' (mean, rstd) tables.  Level buffers: [n][t / 32][h][w][32] bf16, channels [0, S) the
 * down path, [S, S + 48) the transition-up output, [S + 48, S + 96) the up block's maps (S = 96 + 48 level; bottleneck: 288 + 48). */
int64_t endo_net16_offset(const endo_net16* net, int what, int index);
int endo_net16_bwd(endo_net16* net, const float* params, const void* tape, const float* grad_out, float* grads, void* ws, int training,
                   void* stream);

/* ---------------------------------------------------------------------------------------------
 * Similarity registration by iterative closest point (csrc/registration.hip) -- the reference's README, step 4: after evaluate.py,
 * "apply a registration algorithm that is able to estimate a similarity transformation to register the predicted point clouds to the
 * corresponding CT model to calculate residual errors".  The reference has no code for it.  The per-point work is here; the 3 x 3
 * similarity estimate is the host's, in fp64, from the 20 sums (registration.py).  An additive part of ABI 7.
 *
 * Point rows are fp32 x, y, z at a row stride in floats (>= 3: (P, 6) clouds and plain (K, 3) arrays alike), on the device.
 * `transform` (13 doubles: scale, the rotation row-major, the translation; a row becomes scale * R row + t), `centre` and
 * `source_centre` (3 doubles) are HOST arrays, read during the call; all must be finite.
 *
 * endo_registration_tile(which): 0 = source rows per block of the search, 1 = target rows per LDS stage (the two macros below).
 * endo_registration_prepared_bytes(k): size of the prepared copy of a k-row target, 1 <= k <= 2^31 - 1 (-1 outside).
 * endo_registration_prepare: writes the whole prepared copy: the centre, then per row the centred coordinates (fp64 difference, rounded
 *   to fp32) as the search's operand (-2 x, -2 y, -2 z, |.|^2), padded to a multiple of the target tile with rows that never win.
 *   STATE: read by every later endo_registration_match on it.
 * endo_registration_match: one ICP iteration.  Each of the m source rows is moved by `transform` in fp64, taken relative to the target
 *   centre and rounded to fp32; index[i] (int32) is the row of `target` nearest to it by the score |t|^2 - 2 x.t in fp32 (exact brute
 *   force over all k rows; of equal scores the lowest index; the target's coordinates must be finite and their squares within fp32); distance[i] (fp32) is the distance from the moved point to that row,
 *   formed in fp64 by direct differences against `target` (the caller's rows, the ones `prepared` was made from) and rounded once.
 *   sums (20 doubles, device), over the rows whose fp64 distance is <= cap (+inf keeps all; NaN is ENDO_E_BADARG):
 *   [0] n, [1] sum d, [2] sum d^2, [3] max d (0 when n = 0), [4..6] sum s, [7..9] sum t, [10] sum |s|^2, [11 + 3 i + j] sum t_i s_j,
 *   s = the UNMOVED source row - source_centre, t = the matched target row - the target centre, all in fp64.  Per-block partials in the
 *   workspace are added in a fixed order, without floating-point atomics: equal inputs give equal bytes.
 *   workspace: endo_registration_workspace_bytes(m, k) bytes, SCRATCH.
 * endo_similarity_apply: out row = scale * R row + t in fp64, rounded to fp32; columns 3 .. stride - 1 are copied.  out has the
 *   stride of rows and may be rows itself.
 * ------------------------------------------------------------------------------------------- */
#define ENDO_REGISTRATION_SOURCE_TILE 64
#define ENDO_REGISTRATION_TARGET_TILE 1024
int endo_registration_tile(int which);
int64_t endo_registration_prepared_bytes(int64_t k);
int64_t endo_registration_workspace_bytes(int64_t m, int64_t k);
int endo_registration_prepare(const float* target, int64_t target_stride, int64_t k, const double* centre, void* prepared,
                              int64_t prepared_bytes, void* stream);
int endo_registration_match(const float* source, int64_t source_stride, int64_t m, const double* transform, const void* prepared,
                            const float* target, int64_t target_stride, int64_t k, const double* source_centre, double cap,
                            int32_t* index, float* distance, double* sums, void* workspace, int64_t workspace_bytes, void* stream);
int endo_similarity_apply(const float* rows, int64_t stride, int64_t m, const double* transform, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Volumetric fusion of posed depth maps (csrc/fusion.hip): a truncated signed distance function on a voxel grid, averaged over the
 * frames that saw a voxel, and its zero crossings as coloured points.  The reference has no code for it; tests/fusion_restate.py is
 * the numpy float32 statement of the arithmetic, which the planes and rows match bit for bit.  An additive part of ABI 7.
 *
 * A volume is five fp32 planes of nz x ny x nx voxels, x fastest, on the device and 16-byte aligned: tsdf, weight and color
 * ([3][nz][ny][nx]).  They are STATE: endo_fusion_clear initialises them (tsdf 1, weight 0, colour 0), endo_fusion_integrate updates
 * them.  nx % 4 == 0; ny, nz <= 65535; nx ny nz <= 2^40.  Voxel (i, j, k) has its centre at origin + (index + 0.5) * voxel_size, in
 * fp32 from `origin` (3 HOST doubles, finite) and voxel_size rounded to fp32.
 *
 * endo_fusion_tile(which): the box of voxels one wave of the integrate kernel owns, 0 = x, 1 = y, 2 = z.
 * endo_fusion_workspace_bytes(n, h, w): endo_fusion_integrate's workspace for n frames of h x w (-1 outside endo_evaluate_posed's sizes).
 * endo_fusion_integrate: n frames in order, two launches.  depth and boundaries [n][h][w] fp32 (endo_evaluate_posed's depth and its
 *   mask), colors [n][h][w][3] uint8 (its colour images), intrinsics [n][3][3] fp32, rotations [n][3][3] and translations [n][3] fp64
 *   (a pose maps scaled camera coordinates to the volume's frame, x = R (s x_cam) + t), scales [n] fp32 or NULL: all on the device.
 *   Per voxel centre c and frame, in fp32 with every operation rounded: d = c - t; p = Rt d; u = rint(fx p_x / p_z + cx), v likewise;
 *   the sample counts when p_z > 0, 0 <= u <= w - 1, 0 <= v <= h - 1, boundaries[v][u] > 0.5, z = depth[v][u] finite and > 0 and
 *   sdf = s z - p_z >= -truncation; then tsdf <- (tsdf weight + min(1, sdf / truncation)) / (weight + 1), each colour plane
 *   likewise with the pixel's byte (plane c from byte c), weight <- min(weight + 1, max_weight).
 *   scales NULL: s = 20.0f / (z_max - z_min) over the frame's pixels with boundaries > 0.5 of boundaries * depth, endo_evaluate_posed's
 *   own scale.  flags [n] int32, device, written for every frame: ENDO_FUSION_FRAME_OK; _EMPTY (no such pixel); _ZERO_RANGE (z_max ==
 *   z_min with scales NULL); _BAD_SCALE (a scale that is not finite and positive).  Only OK frames touch the volume.
 *   options: ENDO_FUSION_NO_CULL integrates without the per-wave visibility test; the planes' bytes are the same either way.
 *   truncation > 0, max_weight >= 1.  workspace: SCRATCH (the per-frame table).
 * endo_fusion_extract_workspace_bytes(nx, ny, nz): the workspace of the next two entries (-1 for sizes outside the above).
 * endo_fusion_count: two launches.  An edge from a voxel to its +x, +y or +z neighbour holds a surface point when both weights are
 *   >= min_weight and exactly one of the two tsdf values is negative.  total (2 int64, device) receives 0 and the number of such edges;
 *   the workspace receives every (k, j) row's offset and is read by endo_fusion_extract (STATE between the two calls).
 * endo_fusion_extract: one launch after endo_fusion_count with the same arguments: rows (capacity x 6 fp32) receives, in (k, j, i)
 *   order and +x, +y, +z inside a voxel, x, y, z (the voxel's centre with the edge's coordinate advanced by lambda * voxel_size,
 *   lambda = t_a / (t_a - t_b)) and r, g, b = rint(col_a + lambda (col_b - col_a)) of colour planes 2, 1, 0.  Rows at or past
 *   `capacity` are not written.  capacity 0 is valid.
 * ------------------------------------------------------------------------------------------- */
#define ENDO_FUSION_NO_CULL 1
#define ENDO_FUSION_FRAME_OK 0
#define ENDO_FUSION_FRAME_EMPTY 1
#define ENDO_FUSION_FRAME_ZERO_RANGE 2
#define ENDO_FUSION_FRAME_BAD_SCALE 3
int endo_fusion_tile(int which);
int64_t endo_fusion_workspace_bytes(int frames, int height, int width);
int endo_fusion_clear(int nx, int ny, int nz, float* tsdf, float* weight, float* color, void* stream);
int endo_fusion_integrate(const float* depth, const float* boundaries, const uint8_t* colors, const float* intrinsics,
                          const double* rotations, const double* translations, const float* scales, int frames, int height, int width,
                          const double* origin, double voxel_size, double truncation, float max_weight, int nx, int ny, int nz,
                          float* tsdf, float* weight, float* color, int32_t* flags, int options, void* workspace,
                          int64_t workspace_bytes, void* stream);
int64_t endo_fusion_extract_workspace_bytes(int nx, int ny, int nz);
int endo_fusion_count(const double* origin, double voxel_size, int nx, int ny, int nz, const float* tsdf, const float* weight,
                      const float* color, float min_weight, int64_t* total, void* workspace, int64_t workspace_bytes, void* stream);
int endo_fusion_extract(const double* origin, double voxel_size, int nx, int ny, int nz, const float* tsdf, const float* weight,
                        const float* color, float min_weight, float* rows, int64_t capacity, int64_t* total, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The fused surface as a triangle mesh (csrc/fusion_mesh.hip): marching cubes on the volume above.  The vertices are
 * endo_fusion_extract's rows, byte for byte and in its order: every triangle corner lies on a grid edge whose two voxels differ in
 * sign, and the extraction has one row per such edge.  Added here: which three rows form each triangle, and a unit normal per row.
 * tests/fusion_mesh_restate.py is the numpy float32 statement, matched bit for bit.  An additive part of ABI 7.
 *
 * A cell is the voxels (i..i+1, j..j+1, k..k+1), 0 <= i < nx - 1 and likewise j, k; its corner c is voxel (i + (c & 1),
 * j + ((c >> 1) & 1), k + ((c >> 2) & 1)) and its case the sum of (tsdf[c] < 0) << c.  Cell edge e = 4 a + p runs along axis a from its
 * start corner, p = (bit o0 of the start corner) + 2 (bit o1), o0 < o1 the other two axes; its vertex is the row of the start corner's
 * voxel, edge a.  A cell takes part when all eight weights are >= min_weight.  The case table is built by rule
 * (tools/gen_fusion_mesh_table.py writes csrc/fusion_mesh_table.h): at most 5 triangles per case, 820 over the 256 cases, triangle
 * normals (right-hand rule) from negative to positive tsdf, and two cells that share a face cut it the same way: the mesh of a volume
 * whose cells all take part is closed.
 *
 * endo_fusion_mesh_case(index, edges): HOST only, no device work.  Returns the case's number of triangles and, with edges != NULL,
 *   its 15 cell-edge ids (3 per triangle, in order, padded with -1); -1 for an index outside 0..255.
 * endo_fusion_mesh_workspace_bytes(nx, ny, nz): the workspace of the next three entries (-1 for sizes outside the volume's).
 * endo_fusion_mesh_count: two launches.  totals (4 int64, device) receives 0, P, 0, T: P endo_fusion_count's number, T the number of
 *   triangles of the cells that take part; the workspace receives every (k, j) voxel row's and cell row's offset and is read by the
 *   next two entries (STATE between the calls).
 * endo_fusion_mesh_vertices: one launch after endo_fusion_mesh_count with the same arguments: rows (capacity x 6 fp32) as
 *   endo_fusion_extract writes them, and normals (capacity x 3 fp32): with g_x = t[min(i + 1, nx - 1)] - t[max(i - 1, 0)] and g_y, g_z
 *   likewise at a voxel (no division; neighbours as they stand, whatever their weight), v = g_a + lambda (g_b - g_a) per component
 *   for the row's edge a -> b and its own lambda, n = v / sqrt((v_x v_x + v_y v_y) + v_z v_z), every fp32 operation rounded on its
 *   own, and n = (0, 0, 0) where that length is 0 or not finite.  Rows at or past `capacity` are not written.
 * endo_fusion_mesh_faces: one launch after endo_fusion_mesh_count with the same arguments: faces (capacity x 3 int32) receives the
 *   row indices of the triangles, cells in (k, j, i) order and a cell's triangles in table order.  Faces at or past `capacity` are not
 *   written.  Rows that no cell taking part touches stay unreferenced.
 *   Faces are int32: a capacity above 2^31 - 1 is ENDO_E_BADARG in both entries, and where P or T as counted exceeds it the launch
 *   writes no face (the caller has read both and reports it).  capacity 0 is valid in both.
 * ------------------------------------------------------------------------------------------- */
int endo_fusion_mesh_case(int index, int32_t* edges);
int64_t endo_fusion_mesh_workspace_bytes(int nx, int ny, int nz);
int endo_fusion_mesh_count(const double* origin, double voxel_size, int nx, int ny, int nz, const float* tsdf, const float* weight,
                           const float* color, float min_weight, int64_t* totals, void* workspace, int64_t workspace_bytes,
                           void* stream);
int endo_fusion_mesh_vertices(const double* origin, double voxel_size, int nx, int ny, int nz, const float* tsdf, const float* weight,
                              const float* color, float min_weight, float* rows, float* normals, int64_t capacity, int64_t* totals,
                              void* workspace, int64_t workspace_bytes, void* stream);
int endo_fusion_mesh_faces(const double* origin, double voxel_size, int nx, int ny, int nz, const float* tsdf, const float* weight,
                           const float* color, float min_weight, int32_t* faces, int64_t capacity, int64_t* totals, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The fused volume seen from a pose (csrc/fusion_render.hip): one ray per pixel marched to the first zero crossing of the trilinear
 * tsdf, with depth, colour and normal there.  The reference has no code for it; tests/fusion_render_restate.py is the numpy float32
 * statement, matched bit for bit.  An additive part of ABI 7.  Every fp32 operation below is rounded on its own, in the order written.
 *
 * The frame.  R = the rotation rounded to fp32, T = the translation rounded to fp32 (a pose maps scaled camera coordinates to the
 *   volume's frame, x = R (s x_cam) + t, as in endo_fusion_integrate), fx, cx, fy, cy from intrinsics, s = scales[f] or 1 with scales
 *   NULL.  A frame whose s is not finite and positive casts no ray.  L = step * voxel_size (step in voxels; step > 0, L <= truncation,
 *   and (nx + ny + nz + 6) / step <= 2^20), I = 1 / voxel_size.
 * The ray of pixel (u, v).  d_x = (float(u) - cx) / fx, d_y = (float(v) - cy) / fy, d_z = 1, so the ray parameter is the scaled camera
 *   depth s z.  w_r = (R[r][0] d_x + R[r][1] d_y) + R[r][2];  dt = L / sqrt((d_x d_x + d_y d_y) + 1): `step` voxels of distance per
 *   sample for every pixel.  A pixel with boundaries != NULL and not boundaries[v][u] > 0.5, or whose dt is not finite and positive,
 *   casts no ray.
 * Sample k = 1, 2, ... 2^20, on a grid that does not depend on which samples are evaluated: t_k = float(k) dt, x_a = T_a + t_k w_a,
 *   g_a = (x_a - origin_a) I - 0.5, cell c_a = floor(g_a), fractions r_a = g_a - c_a.  The sample is VALID when 0 <= c_a <= n_a - 2 on
 *   every axis and all eight voxels (c_x + 0/1, c_y + 0/1, c_z + 0/1) have weight >= min_weight: endo_fusion_mesh_count's cell rule.
 *   lerp(p, q, r) = p + r (q - p).  Its value: f = lerp(lerp(a00, a10, r_y), lerp(a01, a11, r_y), r_z) with a_yz = lerp(t_0yz, t_1yz, r_x)
 *   over the tsdf; a plane's value at the sample likewise.  Its gradient, from the same differences: with d_yz = t_1yz - t_0yz,
 *   a_yz = t_0yz + r_x d_yz, e_z = a_1z - a_0z, b_z = a_0z + r_y e_z:  G_x = lerp(lerp(d00, d10, r_y), lerp(d01, d11, r_y), r_z),
 *   G_y = lerp(e_0, e_1, r_z), G_z = b_1 - b_0 (and f = b_0 + r_z G_z, the same number).
 * The outcome.  The first valid sample k with f <= 0 ends the ray.  It is a HIT when k > 1, sample k - 1 is valid and its value f' > 0:
 *   lambda = f' / (f' - f), t* = float(k - 1) dt + lambda dt.  Otherwise the ray ends without a hit (the camera inside or behind the
 *   surface, or an unobserved gap in front of it).  A ray no sample ends is a miss.  Samples outside the grid are invalid, so the
 *   kernel clips k to the ray's passage through the grid, conservatively; a grid that lies beyond sample 2^20 of a ray is not seen.
 * The outputs, device, all 0 where there is no hit:  depth [n][h][w] fp32 = t* / s;  mask [n][h][w] fp32 = 1;  colors [n][h][w][3]
 *   uint8: byte c = min(max(rint(lerp(plane c at sample k - 1, plane c at sample k, lambda)), 0), 255), the byte order
 *   endo_fusion_integrate took;  normals [n][h][w][3] fp32: v = lerp(G', G, lambda) per component, n = v / sqrt((v_x v_x + v_y v_y) +
 *   v_z v_z), (0, 0, 0) where that length is 0 or not finite: from the surface towards free space, as endo_fusion_mesh_vertices'.
 * Empty-space skipping.  A first launch marks every brick: brick (bx, by, bz) is the cells whose base voxel has c_a / B = b_a, so it
 *   covers voxels b_a B .. b_a B + B on every axis (one voxel shared with the next brick), and its mark is "holds a voxel with
 *   weight >= min_weight and tsdf <= 0".  A sample whose cell lies in an unmarked brick has eight positive corners or is invalid: it
 *   cannot end a ray and is not evaluated.  The ending sample found, sample k - 1 is evaluated whether its brick is marked or not.
 *   ENDO_FUSION_NO_SKIP marches without marks (one launch); every output byte is the same either way.
 *
 * endo_fusion_render_tile(which): 0, 1: the pixel tile of one wave (x, y); 2, 3, 4: B, the brick's cells (x, y, z).
 * endo_fusion_render_workspace_bytes(n, h, w, nx, ny, nz): the workspace (the marks); -1 outside endo_fusion_integrate's sizes,
 *   for nx > 2^24 or h > 65535 * 16.
 * endo_fusion_render: two launches whatever n is, no host read.  The volume as in endo_fusion_extract plus its truncation; intrinsics
 *   [n][3][3] fp32, rotations [n][3][3] and translations [n][3] fp64, scales [n] fp32 or NULL, boundaries [n][h][w] fp32 or NULL: all on
 *   the device.  ENDO_E_BADARG before any device work for a NULL or misaligned plane, a NULL output, sizes outside the above, a step
 *   outside its bounds, a NaN min_weight, unknown options or a workspace that is too small.  The planes are only read.  workspace: SCRATCH.
 * ------------------------------------------------------------------------------------------- */
#define ENDO_FUSION_NO_SKIP 2
int endo_fusion_render_tile(int which);
int64_t endo_fusion_render_workspace_bytes(int frames, int height, int width, int nx, int ny, int nz);
int endo_fusion_render(const double* origin, double voxel_size, double truncation, int nx, int ny, int nz, const float* tsdf,
                       const float* weight, const float* color, const float* intrinsics, const double* rotations,
                       const double* translations, const float* scales, const float* boundaries, int frames, int height, int width,
                       float min_weight, float step, int options, float* depth, float* mask, uint8_t* colors, float* normals,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A frame tracked against the fused volume (csrc/fusion_track.hip): every pixel of a depth map back-projected under its frame's scale
 * and pose, the trilinear tsdf sampled there -- the pixel's signed distance to the model -- and the normal equations of one
 * Gauss-Newton step over a similarity (rotation, translation, log-scale), summed per frame.  The reference has no code for it;
 * tests/fusion_track_restate.py is the numpy statement: the per-pixel fp32 numbers bit for bit, the fp64 sums up to their order of
 * addition.  An additive part of ABI 7.  Every fp32 operation below is rounded on its own, in the order written.
 *
 * The frame.  R, T, fx, cx, fy, cy, I = 1 / voxel_size as in endo_fusion_render; s = scales[f] or 1 with scales NULL.  A frame whose s
 *   is not finite and positive has no sample: flag ENDO_FUSION_FRAME_BAD_SCALE, sums 0.  Every other frame: ENDO_FUSION_FRAME_OK.
 * The pixel (u, v) with depth d, the camera's z.  d_x = (float(u) - cx) / fx, d_y = (float(v) - cy) / fy,
 *   w_a = (R[a][0] d_x + R[a][1] d_y) + R[a][2], y_a = (s d) w_a, x_a = T_a + y_a;  the cell c_a and fractions r_a of x as of a sample
 *   of endo_fusion_render.  The pixel is a SAMPLE when boundaries[v][u] > 0.5, d is finite and > 0, 0 <= c_a <= n_a - 2 on every axis
 *   and all eight voxels of the cell have weight >= min_weight.  Then with (f, G) the value and gradient of endo_fusion_render:
 *   r = f truncation, n_a = G_a (truncation I): the signed distance, positive in free space, and its gradient per unit length.
 * The Jacobian of r under x' = (1 + sigma) exp([omega]x) (x - T) + T + tau, the increment in the volume's frame about the camera centre:
 *   J = (y x n, n, n . y) with (y x n)_0 = y_1 n_2 - y_2 n_1, _1 = y_2 n_0 - y_0 n_2, _2 = y_0 n_1 - y_1 n_0 and
 *   n . y = (n_0 y_0 + n_1 y_1) + n_2 y_2, seven fp32 numbers; q = (y_0 y_0 + y_1 y_1) + y_2 y_2.
 * The sums, 40 doubles per frame over its samples, J, r and q converted to fp64 and multiplied and added there:
 *   [0] the number of samples, [1] sum r r, [2] sum |r|, [3] max |r|, [4] sum q, [5 + i] sum J_i r (i < 7), and from [12] on the upper
 *   triangle of sum J_i J_j row by row: (0,0) .. (0,6), (1,1) .. (1,6), ... (6,6).  The order of addition is fixed -- a thread's
 *   pixels in order, lanes, waves and blocks in fixed trees, no atomics -- so the same arguments give the same bytes; it is not part
 *   of the contract otherwise.
 *
 * endo_fusion_track_tile(which): 0, 1: the pixel tile of one block (x, y); 2: the consecutive tiles of a frame a block walks.
 * endo_fusion_track_workspace_bytes(n, h, w): the workspace (the blocks' partial sums); -1 outside endo_fusion_integrate's sizes.
 * endo_fusion_track: two launches whatever n is, no host read.  The volume as in endo_fusion_render without its colour planes; depth
 *   and boundaries [n][h][w] fp32, intrinsics [n][3][3] fp32, rotations [n][3][3] and translations [n][3] fp64, scales [n] fp32 or NULL:
 *   all on the device.  Outputs, device: sums [n][40] fp64, flags [n] int32, and three that may each be NULL: residual [n][h][w] fp32 = r,
 *   valid [n][h][w] fp32 = 1, gradient [n][h][w][3] fp32 = n, all 0 where the pixel is no sample.  ENDO_E_BADARG before any device work
 *   for a NULL or misaligned plane, a NULL input or sums or flags, sizes outside the above (nx > 2^24), a NaN min_weight or a
 *   workspace that is too small.  The planes are only read.  workspace: SCRATCH.
 * ------------------------------------------------------------------------------------------- */
int endo_fusion_track_tile(int which);
int64_t endo_fusion_track_workspace_bytes(int frames, int height, int width);
int endo_fusion_track(const double* origin, double voxel_size, double truncation, int nx, int ny, int nz, const float* tsdf,
                      const float* weight, const float* depth, const float* boundaries, const float* intrinsics,
                      const double* rotations, const double* translations, const float* scales, int frames, int height, int width,
                      float min_weight, double* sums, int32_t* flags, float* residual, float* valid, float* gradient, void* workspace,
                      int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A triangle mesh seen from a pose (csrc/mesh_render.hip): the ray through every pixel centre against the triangles, the nearest hit
 * kept -- what the CT model looks like from a frame's camera, the dense depth a prediction is measured against.  The reference has no
 * code for it (its README, step 4, leaves the comparison with the CT model to another tool); tests/mesh_render_restate.py is the numpy
 * float32 statement, matched bit for bit.  An additive part of ABI 7.  Every fp32 operation below is rounded on its own, in the order
 * written.
 *
 * The mesh.  vertices: fp32 rows, `vertex_stride` floats apart: x, y, z and, with a stride >= 6, r, g, b in columns 3, 4, 5
 *   (endo_fusion_extract's rows); V = vertex_count <= 2^31 - 1.  faces: T x 3 int32, T = triangles <= 2^31 - 1.  A face with an index
 *   outside 0 .. V - 1 is never hit and none of its vertices is read.  Both on the device; V = 0 and T = 0 are valid.
 * The frame.  R, T, fx, cx, fy, cy and s as in endo_fusion_render (x = R (s x_cam) + t).  A frame whose s is not finite and positive
 *   renders nothing: flag ENDO_FUSION_FRAME_BAD_SCALE; every other frame ENDO_FUSION_FRAME_OK.
 * A vertex x in (scaled) camera coordinates: q = x - T, p_a = (R[0][a] q_0 + R[1][a] q_1) + R[2][a] q_2.
 * Pixel (u, v) against triangle (a, b, c), their p written a, b, c:  d_x = (float(u) - cx) / fx, d_y = (float(v) - cy) / fy;  the
 *   sheared vertices A_x = a_x - d_x a_z, A_y = a_y - d_y a_z, B and C likewise;  f(P, Q) = P_x Q_y - P_y Q_x (two rounded products, then
 *   the difference, so f(Q, P) = -f(P, Q) exactly: no fused multiply-add);  U = f(C, B), V = f(A, C), W = f(B, A);
 *   det = (U + V) + W;  t = ((U a_z + V b_z) + W c_z) / det.  The pixel HITS the triangle when
 *     U, V, W are all >= 0 or all <= 0;
 *     neither A_x, B_x, C_x nor A_y, B_y, C_y are all > 0 or all < 0 (the span rule: in exact arithmetic it follows from the line
 *       above; in fp32 it keeps three nearly collinear products from agreeing by rounding far away from the triangle, and it makes
 *       the pixel box below a statement about these very numbers);
 *     det != 0, and t is finite and > 0.
 *   Two triangles on one edge see the same sheared vertices and the same |f| with opposite sign, and zero is inclusive: a closed
 *   mesh has no cracks.  det > 0 is the FRONT: the face whose right-hand-rule normal (b - a) x (c - a) points to the camera,
 *   endo_fusion_mesh_faces' outside.  ENDO_MESH_CULL_BACK refuses det < 0, ENDO_MESH_CULL_FRONT det > 0.
 *   The pixel's hit is the triangle with the smallest t and of equal t the lowest face index.  A pixel with boundaries != NULL and
 *   not boundaries[v][u] > 0.5 has no hit.
 * The outputs, device, all 0 where there is no hit except triangle, -1 there; every one but depth may be NULL:
 *   depth [n][h][w] fp32 = t / s;  mask [n][h][w] fp32 = 1;  triangle [n][h][w] int32;
 *   barycentric [n][h][w][3] fp32 = U / det, V / det, W / det, the weights of a, b, c;
 *   normals [n][h][w][3] fp32: with e = b - a, g = c - a of the rows' x, y, z:  v = (e_y g_z - e_z g_y, e_z g_x - e_x g_z,
 *     e_x g_y - e_y g_x) (f again), n = v / sqrt((v_x v_x + v_y v_y) + v_z v_z) as endo_fusion_mesh_vertices normalises, (0, 0, 0) where
 *     that length is 0 or not finite, and -n where det < 0: towards the camera;
 *   colors [n][h][w][3] uint8, only with a stride >= 6: byte c = min(max(rint((beta_0 col_a + beta_1 col_b) + beta_2 col_c), 0), 255)
 *     of column 5 - c (beta the barycentric output): rows hold r, g, b = colour planes 2, 1, 0, so byte c is plane c, the byte order
 *     of endo_fusion_render's colours;
 *   flags [n] int32.
 * The pixel box.  With a_z, b_z, c_z all > 0 and fx > 0, A_x falls as u grows and changes sign about u = fx a_x / a_z + cx: left of the
 *   smallest of the three such numbers all are > 0, right of the largest all < 0, and the span rule refuses.  The kernel tests the
 *   pixels between them, 1 / 16 pixel and 2^-19 of the coordinate wider, clipped to the image; a triangle with a vertex that is not in
 *   front of the camera, or a number that is not finite, takes the whole image; one with a_z, b_z, c_z all <= 0 is dropped (t would be
 *   a mean of numbers <= 0).  ENDO_MESH_BRUTE tests every pixel against every triangle; every output byte is the same either way.
 *
 * endo_mesh_render_tile(which): 0, 1: the pixel tile of one wave of the queue pass (x, y); 2: the largest box, in pixels, the setup
 *   pass tests in place; 3: the threads of a block.
 * endo_mesh_render_workspace_bytes(n, h, w, triangles): 8 bytes per pixel (the keys), 256 (the queue's count) and 8 per (frame,
 *   triangle) (the queue), each rounded up to 256; -1 outside endo_evaluate_posed's sizes or for triangles outside 0 .. 2^31 - 1.
 * endo_mesh_render: four launches whatever n is (two with T = 0), no host read: clear, setup (a thread per frame and triangle), queue
 *   (a wave per queued triangle) and resolve (a thread per pixel); hits meet in a 64-bit atomic minimum per pixel on
 *   (bits of t) << 32 | face.  intrinsics [n][3][3] fp32, rotations [n][3][3] and translations [n][3] fp64, scales [n] fp32 or NULL,
 *   boundaries [n][h][w] fp32 or NULL: all on the device.  ENDO_E_BADARG before any device work for a NULL or misaligned input, a
 *   NULL depth, a stride < 3, colors with a stride < 6, both cull bits, unknown options, sizes outside the above or a workspace that
 *   is too small.  The mesh is only read.  workspace: SCRATCH.
 * ------------------------------------------------------------------------------------------- */
#define ENDO_MESH_CULL_BACK 1
#define ENDO_MESH_CULL_FRONT 2
#define ENDO_MESH_BRUTE 4
int endo_mesh_render_tile(int which);
int64_t endo_mesh_render_workspace_bytes(int frames, int height, int width, int64_t triangles);
int endo_mesh_render(const float* vertices, int64_t vertex_stride, int64_t vertex_count, const int32_t* faces, int64_t triangles,
                     const float* intrinsics, const double* rotations, const double* translations, const float* scales,
                     const float* boundaries, int frames, int height, int width, int options, float* depth, float* mask,
                     int32_t* triangle, float* barycentric, float* normals, uint8_t* colors, int32_t* flags, void* workspace,
                     int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ENDO_HIP_H */
