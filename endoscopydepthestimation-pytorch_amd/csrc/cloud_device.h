// What the point-cloud writers share -- endo_point_cloud (scatter.hip), the test phase (evaluate.hip), the posed test output
// (evaluate_posed.hip) and the validation phase (evaluate_validation.hip): which pixels become points (utils.py:836), their pinhole
// back-projection (utils.py:838-840), the ordered compaction of a row's kept pixels, the block-wide count of a `rows` kernel and the
// one-block exclusive scan that turns the counts into offsets.  Two of those files are compiled with -ffp-contract=off and two
// without: every float operation below is an explicit-rounding intrinsic, which the compiler never contracts, so the header means the
// same in all four.
#pragma once

#include "common.h"

namespace endo {

constexpr int kCloudThreads = 256;          // a rows / write block: four waves, 256 pixels of a row per chunk
constexpr int kScanThreads = 1024;          // the one block of a scan kernel

// every `downsampling`-th pixel inside the mask (utils.py:836, 1262)
__device__ __forceinline__ bool cloud_pixel_keep(int downsampling, int h, int w, float bnd) {
    return h % downsampling == 0 && w % downsampling == 0 && bnd > 0.5f;
}

// utils.py:838-840 with the reference's operation order, (w - cx) / fx * z: three roundings per coordinate
__device__ __forceinline__ void cloud_back_project(int w, int h, float fx, float cx, float fy, float cy, float z, float& x, float& y) {
    x = __fmul_rn(__fdiv_rn(__fsub_rn(static_cast<float>(w), cx), fx), z);
    y = __fmul_rn(__fdiv_rn(__fsub_rn(static_cast<float>(h), cy), fy), z);
}

// np.uint8(255 * (0.5 * c + 0.5)), evaluate.py:329-330: three roundings, then truncation (c in [-1, 1] keeps it in [0, 255])
__device__ __forceinline__ int display_u8(float c) {
    const float v = __fmul_rn(255.0f, __fadd_rn(__fmul_rn(0.5f, c), 0.5f));
    return v > 0.0f ? min(static_cast<int>(v), 255) : 0;
}

// np.uint8(255 * clip(c * 0.5 + 0.5, 0, 1)), utils.py:1331-1334: display_u8 with the clamp ahead of the last product
__device__ __forceinline__ int posed_u8(float c) {
    float v = __fadd_rn(__fmul_rn(c, 0.5f), 0.5f);
    if (v < 0.0f) v = 0.0f;
    if (v > 1.0f) v = 1.0f;
    v = __fmul_rn(255.0f, v);
    return v > 0.0f ? min(static_cast<int>(v), 255) : 0;          // (a NaN colour: 0)
}

// Rank of this thread's pixel among the kept pixels of a chunk of kCloudThreads consecutive pixels, in pixel order, and the chunk's
// count of kept pixels: lower lanes of the wave by ballot and popcount, lower waves by the per-wave counts in LDS.  Every thread of
// the block calls, once per chunk; every thread reads the same four counts, so a caller adds `total` to a base it keeps in a register.
// Two barriers: the first puts the four counts in front of their readers; the second keeps the next chunk's counts (the next call)
// behind this chunk's readers.
__device__ __forceinline__ int cloud_chunk_rank(bool keep, int& total) {
    __shared__ int s_wave[kCloudThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(bal);
    __syncthreads();
    int rank = __popcll(bal & ((1ull << lane) - 1ull));
    for (int i = 0; i < wave; ++i) rank += s_wave[i];
    total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
    return rank;
}

// The count of a `rows` kernel, in two steps.  cloud_wave_count: how many lanes of this wave hold `keep`, by ballot, so the count needs
// no shuffle reduction behind the row loop (as a chain of six dependent shuffles of its own, after the caller's, it cost
// endo_evaluate_posed 0.4 us of its 20 per call).  In a strided row loop the last pass runs on a part of the wave: the lanes outside
// count as not kept, and the wave's lane 0, which has the lowest pixel, takes part in every pass its wave makes, so the sum it keeps
// is the wave's.
__device__ __forceinline__ int cloud_wave_count(bool keep) { return __popcll(__ballot(keep)); }

// cloud_block_count: the sum over a block of kCloudThreads threads of the waves' counts (each read from its wave's lane 0), returned
// to every thread.  One barrier, after the four counts are stored: LDS that the caller wrote before the call (its own per-wave
// partials) is published by it as well.
__device__ __forceinline__ int cloud_block_count(int wave_cnt) {
    __shared__ int s_cnt[kCloudThreads / 64];
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = wave_cnt;
    __syncthreads();
    return s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// Exclusive prefix of counts[0 .. items) in place by the one block of kScanThreads threads: thread t owns the items
// [t * chunk, (t + 1) * chunk); the block scans the per-thread sums, then each thread rewrites its items.  items = groups * per_group,
// group-major (a frame's rows, a pair's bands): offsets[g] = the first offset of group g, offsets[groups] = the total.  The first
// barrier puts the waves' sums in front of their readers; the second puts every rewritten item in front of the threads that copy the
// groups' offsets from them.
__device__ __forceinline__ void cloud_scan_block(int64_t* counts, int groups, int per_group, int64_t* offsets) {
    __shared__ int64_t s_wave[kScanThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t items = static_cast<int64_t>(groups) * per_group;
    const int64_t chunk = (items + kScanThreads - 1) / kScanThreads;
    const int64_t i0 = min(items, t * chunk), i1 = min(items, i0 + chunk);
    int64_t sum = 0;
    for (int64_t i = i0; i < i1; ++i) sum += counts[i];
    int64_t incl = sum;          // inclusive prefix inside the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int64_t acc = incl - sum;
    for (int i = 0; i < wave; ++i) acc += s_wave[i];
    for (int64_t i = i0; i < i1; ++i) {
        const int64_t c = counts[i];
        counts[i] = acc;
        acc += c;
    }
    if (t == kScanThreads - 1) {
        int64_t total = 0;
        for (int i = 0; i < kScanThreads / 64; ++i) total += s_wave[i];
        offsets[groups] = total;
    }
    __syncthreads();
    for (int g = t; g < groups; g += kScanThreads) offsets[g] = counts[static_cast<int64_t>(g) * per_group];
}

}  // namespace endo
