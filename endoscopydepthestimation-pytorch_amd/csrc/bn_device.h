// BatchNorm + ReLU backward on registers and the per-channel sum reduction of the fp32 convolution kernels.
//
// A data-gradient epilogue holds, per lane, x and the incoming gradient d of some pixels of ONE channel and that channel's constants
// (scale = gamma * rstd, beta, mean, rstd).  Per pixel:  xcen = x - mean;  z = xcen * scale + beta;  dz = z > 0 ? d : 0;  the channel's
// sums s1 += dz, s2 += dz * xhat (xhat = xcen * rstd);  and the data gradient through BN, scale * dz, which every kernel adds to its own
// total in its own form.  The sums leave the block in four steps: the sum over the wave's four 16-lane rows, one LDS slot per
// (wave, channel, sum), the kernel's barrier, then the waves added in fp64 in wave order and ONE atomicAdd per (channel, sum).  The
// forward statistics (sum, sum of squares) leave a block the same way.
//
// The pixel step exists in these rounding variants; they are NOT interchangeable (a kernel's results are pinned bit for bit):
//   xhat per pixel   scalar; s2 += dz * (xcen * rstd)                 bn_relu_bwd_xhat: conv_dma EPI_DGRAD_BN (prefetched operands), dgrad_dense,
//                                                                     dgrad_block, td_dgrad, td_dgrad_small; in place: conv_epilogue EPI_DGRAD_BN
//   xcen, rstd once  scalar; s2 = fma(dz, xcen, s2), sum * rstd        in place: dgrad_newmap, dgrad_wino8
//   packed pairs     compiler-made v_pk; as xcen, total by fma        in place: dgrad_block8
//   packed pairs     inline assembly; as xcen, total by v_pk_fma      wino3_epilogue (dgrad_wino3_device.h): dgrad_wino3, dgrad_wino3p
//
// Helpers take their accumulators by reference and keep the statement order of the kernels.  A kernel calls one only where its device
// code stays the same instruction for instruction (tools/isa_diff.py against the build before): these kernels are tuned against their
// register budgets, and the same arithmetic behind a function boundary is often scheduled differently -- by-value forms of the row sum
// reordered a third of the library's kernels and made dgrad_block8 spill.  The stage and the flush stay in the kernels for that
// reason: as functions they changed the order in which most kernels form their LDS addresses.
#pragma once

#include "common.h"

namespace endo {

// -> dz.  s2 += dz * (xcen * rstd): the product with xhat is rounded per pixel
__device__ __forceinline__ float bn_relu_bwd_xhat(float x, float d, float scale, float beta, float mean, float rstd, float& s1, float& s2) {
    const float xcen = x - mean;
    const float z = fmaf(xcen, scale, beta);
    const float dz = z > 0.f ? d : 0.f;
    s1 += dz;
    s2 += dz * (xcen * rstd);
    return dz;
}

// both sums over the wave's four 16-lane rows, in every lane (float or double)
template <typename T>
__device__ __forceinline__ void bn_rows_sum(T& s1, T& s2) {
    s1 += __shfl_xor(s1, 16, 64); s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 16, 64); s2 += __shfl_xor(s2, 32, 64);
}

}  // namespace endo
