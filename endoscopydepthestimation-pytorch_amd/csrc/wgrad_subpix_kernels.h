// Weight gradient of the transition-up convolution (nearest x2 -> conv3x3 48 -> 48, reference models.py:70-80) in
// sub-pixel form.  The forward pass is nine products M[r][c] = W'[r][c] X'[r][c] on the LOW-resolution grid (conv_dma_kernels.h,
// tu_fwd_subpix_kernel: r, c in {-, 0, +}, X' the separable difference image, W' the tap sums over rows(r) x cols(c)) and
// out(2y + a, 2x + b) = M[ra][cb] + M[ra][0] + M[0][cb] + M[0][0].  So, with g_ab[y][x] = dY[2y + a][2x + b],
//     Gt[r][c]            = dM[r][c]: rows g0, g0 + g1, g1 for r = -, 0, +; columns likewise on b
//     dW'[r][c][co][ci]   = sum over low-res pixels of Gt[r][c][co] * X'[r][c][ci]                                  (9 of them)
//     dW[co][ci][ky][kx]  = sum over the r with ky in rows(r), the c with kx in cols(c) of dW'[r][c][co][ci]
// -- 9 instead of 36 pixel-sized correlations (1/4 of the MACs), and the x2 gather disappears.
//
// Kernel shape = wgrad_nsplit_kernels.h with the roles the data dictates: the SHIFTED operand is the low-resolution
// activation (a 3-row x 40-column window of the block's 16 input channels, LDS-DMA, two buffers): a lane reads the 3 x 4 values
// around its two pixels and forms both pixels' nine X' in registers; M = 16 input channels, one MFMA row group per (r, c).  The other
// operand, dY, is used unshifted and by one lane only, so each lane loads its 2 rows x 4 consecutive full-resolution values per
// cout group straight into registers (one float4 per row: two low-res pixels x two column phases) and forms the nine Gt with five
// additions.  blockIdx.y = third of the input channels; all four waves hold the same 9 x 3 accumulators (r, c) x cout group and split
// the 32 pixels of a chunk (chunk = one low-res row segment); their sums are added through LDS at the end, so a block writes ONE
// partial sum of its 9 matrices.  Blocks own contiguous chunk ranges; tu_wgrad_subpix_reduce_kernel adds the partial sums and
// scatters every dW' entry onto the 1, 3 or 9 original taps it stands for.
#pragma once

#include "conv_dma_kernels.h"
#include "wgrad_kernels.h"

namespace endo {

constexpr int kSpSeg = 32;                         // low-res pixels per chunk
constexpr int kSpCols = kSpSeg + 8;                // window columns: 4-pixel aligned halo on both sides
constexpr int kSpMap = 3 * kSpCols;                // floats per channel window (rows y-1, y, y+1)
constexpr int kSpCh = 16;                          // input channels per block
constexpr int kSpBuf = kSpCh * kSpMap;             // floats per buffer
constexpr int kSpUnits = kSpBuf / 4;               // 480 float4 per window
constexpr int kSpAcc = 9 * 3;                      // accumulators: (r, c) x cout group
constexpr int kSpLds = 2 * kSpBuf > kSpAcc * 256 ? 2 * kSpBuf : kSpAcc * 256;          // the two windows, then the block's sum

__global__ void __launch_bounds__(kConvThreads) tu_wgrad_subpix_kernel(const WgradParams p, float* __restrict__ partial, int chunks_per_block) {
    __shared__ __attribute__((aligned(16))) float smem[kSpLds];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15;
    const int lk = lane >> 4;
    const int xl = 16 * (wave >> 1) + 4 * lk + 2 * (wave & 1);      // this lane's two pixels of a chunk: xl, xl + 1
    const int ci_base = blockIdx.y * kSpCh;
    const int segs = (p.w + kSpSeg - 1) / kSpSeg;      // p.h, p.w: the LOW-resolution grid
    const int chunks_total = segs * p.h * p.n;
    const int c_begin = blockIdx.x * chunks_per_block;
    const int c_end = min(c_begin + chunks_per_block, chunks_total);

    // row li of every row group reads x[ci_base + li][y + oy][x + ox]: window row oy + 1, window column x - x0 + 4 + ox
    const int aoff = li * kSpMap + 4 + xl - 1;

    f32x4 acc[9][3];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int g = 0; g < 3; ++g) acc[t][g] = f32x4{0.f, 0.f, 0.f, 0.f};

    const float* pad_zero = g_pad_consts + 4;
    // this thread's units of the activation window (chunk independent)
    constexpr int kSlots = (kSpUnits + kConvThreads - 1) / kConvThreads;      // 2
    int w_off[kSlots], w_row[kSlots], w_col[kSlots];
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
        const int e = k * kConvThreads + tid;
        const int ch = e / (kSpMap / 4);
        const int r = e - ch * (kSpMap / 4);
        w_row[k] = r / (kSpCols / 4);
        w_col[k] = 4 * (r - w_row[k] * (kSpCols / 4));
        w_off[k] = (ci_base + ch) * p.in_cs + w_row[k] * p.in_w + w_col[k];
    }
    int64_t d_off[3];          // this lane's cout rows of dY
#pragma unroll
    for (int g = 0; g < 3; ++g) d_off[g] = static_cast<int64_t>(16 * g + li) * p.dy_cs + 2 * xl;

    int i_n = c_begin / (segs * p.h);
    int i_y = (c_begin - i_n * segs * p.h) / segs;
    int i_seg = c_begin - (i_n * p.h + i_y) * segs;

    f32x4 raw[3][2];           // dY of the chunk in flight: [cout group][row phase a] = (xl, b = 0), (xl, 1), (xl + 1, 0), (xl + 1, 1)
    bool raw_ok = false;

    auto issue = [&](int buf) {
        const int x0 = i_seg * kSpSeg;
        const WgSample sm(p, i_n);
        float* s_x = smem + buf * kSpBuf;
        const float* x_base = p.in + sm.in_off(p) + static_cast<int64_t>(i_y - 1) * p.in_w + x0 - 4;
#pragma unroll
        for (int k = 0; k < kSlots; ++k) {
            const int e0 = k * kConvThreads + wave * 64;
            if (e0 < kSpUnits) {
                const bool ok = static_cast<unsigned>(i_y - 1 + w_row[k]) < static_cast<unsigned>(p.h) &&
                                static_cast<unsigned>(x0 - 4 + w_col[k]) < static_cast<unsigned>(p.w);
                const float* src = ok ? x_base + w_off[k] : pad_zero;
                if (e0 + lane < kSpUnits) __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(s_x + 4 * e0), 16, 0, 0);
            }
        }
        // full-resolution rows 2 y, 2 y + 1, columns 2 (x0 + xl) .. + 3  (p.w is a multiple of 4 and xl is even: both pixels are in or out)
        const float* d_base = p.dy + sm.dy_off(p) + static_cast<int64_t>(2 * i_y) * p.dy_w + 2 * x0;
        raw_ok = x0 + xl < p.w;
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int a = 0; a < 2; ++a)
                raw[g][a] = *reinterpret_cast<const f32x4*>(raw_ok ? d_base + d_off[g] + a * p.dy_w : pad_zero);
        if (++i_seg == segs) {
            i_seg = 0;
            if (++i_y == p.h) { i_y = 0; ++i_n; }
        }
    };

    if (c_begin < c_end) issue(0);
    int buf = 0;
    for (int chunk = c_begin; chunk < c_end; ++chunk, buf ^= 1) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        f32x4 cur[3][2];
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int a = 0; a < 2; ++a) cur[g][a] = raw_ok ? raw[g][a] : f32x4{0.f, 0.f, 0.f, 0.f};
        if (chunk + 1 < c_end) issue(buf ^ 1);

        const float* s_x = smem + buf * kSpBuf + aoff;
        float v[3][4];          // rows y-1, y, y+1; columns xl-1 .. xl+2
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cx = 0; cx < 4; ++cx) v[r][cx] = s_x[r * kSpCols + cx];
        float t[3][4];          // row classes -, 0, +
#pragma unroll
        for (int cx = 0; cx < 4; ++cx) {
            t[0][cx] = v[0][cx] - v[1][cx];
            t[1][cx] = v[1][cx];
            t[2][cx] = v[2][cx] - v[1][cx];
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            float a[9];
#pragma unroll
            for (int rc = 0; rc < 3; ++rc) {
                a[rc * 3 + 0] = t[rc][e] - t[rc][e + 1];
                a[rc * 3 + 1] = t[rc][e + 1];
                a[rc * 3 + 2] = t[rc][e + 2] - t[rc][e + 1];
            }
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                const float v00 = cur[g][0][2 * e], v01 = cur[g][0][2 * e + 1], v10 = cur[g][1][2 * e], v11 = cur[g][1][2 * e + 1];
                const float top = v00 + v01, bot = v10 + v11;
                const float gt[9] = {v00, top, v01, v00 + v10, top + bot, v01 + v11, v10, bot, v11};
#pragma unroll
                for (int tt = 0; tt < 9; ++tt) acc[tt][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tt], gt[tt], acc[tt][g], 0, 0, 0);
            }
        }
    }

    // the block's sum: wave 0 lays its accumulators down, waves 1 and 2 add theirs, wave 3 adds its own and writes
    // partial[(((bx * 3 + by) * 9 + rc) * 3 + g) * 4 + r][lane] = D[ci 4 lk + r][cout 16 g + li]
    __syncthreads();
    float* out = partial + (static_cast<int64_t>(blockIdx.x) * gridDim.y + blockIdx.y) * (kSpAcc * 256);
#pragma unroll
    for (int turn = 0; turn < 4; ++turn) {
        if (wave == turn) {
#pragma unroll
            for (int tt = 0; tt < 9; ++tt)
#pragma unroll
                for (int g = 0; g < 3; ++g)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = ((tt * 3 + g) * 4 + r) * 64 + lane;
                        if (turn == 0) smem[i] = acc[tt][g][r];
                        else if (turn < 3) smem[i] += acc[tt][g][r];
                        else out[i] = smem[i] + acc[tt][g][r];
                    }
        }
        if (turn < 3) __syncthreads();
    }
}

// grid (3 * 9 * 3 = 81 row blocks, slices of the partial blocks): sum, then scatter onto the original taps
__global__ void __launch_bounds__(256) tu_wgrad_subpix_reduce_kernel(const float* __restrict__ partial, int blocks, int cin, float* __restrict__ dw) {
    const int rb = blockIdx.x;                         // (by * 9 + rc) * 3 + g
    const int g = rb % 3, rc = (rb / 3) % 9, by = rb / kSpAcc;
    const int per = (blocks + gridDim.y - 1) / gridDim.y;
    const int b0 = blockIdx.y * per, b1 = min(blocks, b0 + per);
    const int64_t stride = static_cast<int64_t>(3) * kSpAcc * 256;
    const float* src = partial + static_cast<int64_t>(rb) * 256 + threadIdx.x;
    float s = 0.f;
    for (int b = b0; b < b1; ++b) s += src[b * stride];
    if (b0 >= b1) return;
    const int lane = threadIdx.x & 63, r = threadIdx.x >> 6;
    const int ci = by * kSpCh + 4 * (lane >> 4) + r;
    const int co = 16 * g + (lane & 15);
    // original taps summed into W'[r][c]: rows(-) = {0}, rows(0) = {0, 1, 2}, rows(+) = {2}; columns likewise (tu_phase_weights_kernel)
    const int rr = rc / 3, cc = rc % 3;
    const int ky0 = rr == 2 ? 2 : 0, ky1 = rr == 0 ? 0 : 2;
    const int kx0 = cc == 2 ? 2 : 0, kx1 = cc == 0 ? 0 : 2;
    float* dst = dw + (static_cast<int64_t>(co) * cin + ci) * 9;
    for (int ky = ky0; ky <= ky1; ++ky)
        for (int kx = kx0; kx <= kx1; ++kx) atomicAdd(dst + ky * 3 + kx, s);
}

constexpr int kSpMaxBlocks = 170;                  // x 3 channel thirds: one round of the chip at two blocks per compute unit
constexpr int64_t kSpScratchFloats = static_cast<int64_t>(kSpMaxBlocks) * 3 * kSpAcc * 256;      // 3.5 M floats

// p: h, w = the LOW-resolution grid; in = low-res activations (48 channels); dy = full-resolution gradient (48 maps)
inline bool tu_wgrad_subpix_ok(const WgradParams& p) {
    return p.cin == 3 * kSpCh && p.cout == 48 && (p.w % 4 == 0) && (p.in_w % 4 == 0) && (p.in_cs % 4 == 0) && (p.in_ns % 4 == 0) &&
           (p.dy_w % 8 == 0) && (p.dy_cs % 4 == 0) && (p.dy_ns % 4 == 0) && (reinterpret_cast<uintptr_t>(p.in) % 16 == 0) &&
           (reinterpret_cast<uintptr_t>(p.dy) % 16 == 0);
}

inline int launch_tu_wgrad_subpix(const WgradParams& p, float* scratch, hipStream_t stream) {
    const int chunks_total = ((p.w + kSpSeg - 1) / kSpSeg) * p.h * p.n;
    int blocks = kSpMaxBlocks;
    if (blocks > chunks_total) blocks = chunks_total;
    const int per = (chunks_total + blocks - 1) / blocks;
    blocks = (chunks_total + per - 1) / per;
    tu_wgrad_subpix_kernel<<<dim3(blocks, 3), kConvThreads, 0, stream>>>(p, scratch, per);
    ENDO_LAUNCH_CHECK();
    tu_wgrad_subpix_reduce_kernel<<<dim3(3 * kSpAcc, 4), 256, 0, stream>>>(scratch, blocks, p.cin, p.dw);
    ENDO_LAUNCH_CHECK();
    return 0;
}

}  // namespace endo
