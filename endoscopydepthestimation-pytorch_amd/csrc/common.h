// Shared device helpers for libendo_hip.so (gfx950 only; wave = 64 lanes).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <utility>

#include "../../include/endo_hip.h"

#define ENDO_CHECK(expr)                                 \
    do {                                                 \
        hipError_t _e = (expr);                          \
        if (_e != hipSuccess) return static_cast<int>(_e); \
    } while (0)

#define ENDO_LAUNCH_CHECK() ENDO_CHECK(hipGetLastError())

namespace endo {

constexpr int kWave = 64;

// workspace sections start on 256-byte boundaries
inline int64_t align256(int64_t v) { return (v + 255) & ~static_cast<int64_t>(255); }

// a batch of frames a (row, frame) grid can index (blockIdx.y < 65536) and whose pixels a 32-bit number counts
inline bool frames_sizes_ok(int frames, int height, int width) {
    return frames > 0 && frames <= 65535 && height > 0 && width > 0 && static_cast<int64_t>(frames) * height * width <= INT32_MAX;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;
}

// BN-backward sums (sum dz, sum dz * xhat per channel) are added up with fp64 atomics, one per value, block and step of a
// data-gradient kernel.  Atomics on ONE address are served one after the other (~8 ns each on this part: thousands of blocks of
// a full-resolution launch queue up behind each other, and a block's next s_waitcnt vmcnt(0) waits for its own to be
// acknowledged -- 40 % of the new-channel passes' time, tools/nl_bench).  So the sums live in kBnSlots copies, `slot_stride`
// doubles apart (0 = a single copy): a block adds to the copy its index selects, the readers add the copies up.  Eight copies
// bring a full-resolution launch down to a few hundred atomics per address (a few us) and keep the readers' prologue short.
constexpr int kBnSlots = 8;

__device__ __forceinline__ int64_t bn_slot_offset(int64_t slot_stride) {
    return static_cast<int64_t>((blockIdx.x + 11 * blockIdx.z) & (kBnSlots - 1)) * slot_stride;
}

__device__ __forceinline__ double bn_slot_sum(const double* __restrict__ s, int64_t slot_stride) {
    if (slot_stride == 0) return s[0];
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < kBnSlots; ++k) t += s[k * slot_stride];
    return t;
}

// bf16 operands for v_mfma_f32_16x16x16_bf16 (the "bf16 operands" mode, ENDO_OPT_MFMA_BF16): four consecutive k values of a lane,
// rounded to nearest even by v_cvt_pk_bf16_f32 (gfx950), two per dword.  One such MFMA replaces four v_mfma_f32_16x16x4_f32 whose
// k-steps hold the same 16 k values: lane group lk carries k = 4 lk + i in both forms.
typedef short bf16x4_bits __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x4_bits pack_bf16x4(float a, float b, float c, float d) {
    // through the compiler's own conversion (one v_cvt_pk_bf16_f32 per pair), NOT inline assembly: the hazard recogniser must see
    // the VALU write to insert the wait states an MFMA needs before it reads those registers
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
    const bf16x2_t lo = __builtin_convertvector(f32x2_t{a, b}, bf16x2_t), hi = __builtin_convertvector(f32x2_t{c, d}, bf16x2_t);
    return __builtin_bit_cast(bf16x4_bits, u32x2_t{__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi)});
}

// eight consecutive k values of a lane for v_mfma_f32_16x16x32_bf16 (gfx950: twice the k of the x16 form in the same 16-18 cycles,
// tools/mfma_rate_probe)
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_acc __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8_t pack_bf16x8(float a, float b, float c, float d, float e, float f, float g, float h) {
    typedef float f32x8_t __attribute__((ext_vector_type(8)));
    return __builtin_convertvector(f32x8_t{a, b, c, d, e, f, g, h}, bf16x8_t);
}

typedef unsigned u32x4_bits __attribute__((ext_vector_type(4)));

// Block-wide sum of K per-thread partials, one fp64 atomic per value per block.
// scratch: K * (blockDim/64) doubles of LDS.  All threads must call.
template <int K>
__device__ __forceinline__ void block_sum_atomic(const float (&part)[K], double* dst, double* scratch) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nwave = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double v = wave_sum(static_cast<double>(part[k]));
        if (lane == 0) scratch[k * nwave + wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double v = 0.0;
        for (int i = 0; i < nwave; ++i) v += scratch[threadIdx.x * nwave + i];
        atomicAdd(dst + threadIdx.x, v);
    }
    __syncthreads();
}

// XCD-aware block -> work-item remap.  Workgroup b is observed to run on XCD b % 8 (8 XCDs, each with a
// private 4 MiB L2; MI355X_MICROARCH.md).  Giving XCD k the contiguous range [k*T/8, (k+1)*T/8) of a
// row-major tile grid puts horizontally / vertically adjacent tiles -- which share halo cache lines --
// behind the same L2.  Purely a locality hint: the map is a bijection on [0, T) for any T.
__device__ __forceinline__ int xcd_remap(int b, int total) {
    const int xcd = b & 7, idx = b >> 3;
    const int q = total >> 3, r = total & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// ---- persistent launches (dgrad_wino3p, td_dgrad, td_fwd): bpg blocks per group walk the group's t_total tiles -------------------------
// Block r of a group (0 <= r < bpg) takes tiles begin, begin + step, ... < end.  With bpg a multiple of 8, the blocks of an XCD (bpg / 8
// per group) share one contiguous range of the group's tiles and walk it INTERLEAVED: block idx takes tiles T0 + idx, T0 + idx + bpg / 8,
// ... -- at any time the XCD's blocks work on neighbouring tiles, whose haloed input windows then meet in the XCD's L2.  (dgrad_wino3p:
// with a contiguous run per block a 10 x 40 window of 8 x 32 pixels, 48 maps, was fetched again by the block's next tile ~60 us later,
// after 16 MB of other traffic: 1.8 GB of HBM fetch per level-0 launch for 1.1 GB algorithmic.)  Otherwise one contiguous run per block.
struct TileWalk {
    int begin, end, step;
};

__host__ __device__ __forceinline__ TileWalk persistent_tile_walk(int r, int bpg, int t_total) {
    if ((bpg & 7) == 0) {
        const int q = bpg >> 3, xcd = r & 7, idx = r >> 3;
        return {static_cast<int>(static_cast<int64_t>(xcd * q) * t_total / bpg) + idx, static_cast<int>(static_cast<int64_t>((xcd + 1) * q) * t_total / bpg), q};
    }
    return {static_cast<int>(static_cast<int64_t>(r) * t_total / bpg), static_cast<int>(static_cast<int64_t>(r + 1) * t_total / bpg), 1};
}

// blocks per group: `blocks` shared by `groups`, rounded down to a multiple of 8 (the XCD split above) from 8 on, at most one per tile
inline int persistent_bpg(int blocks, int groups, int tiles_per_group) {
    int bpg = blocks / groups;
    if (bpg >= 8) bpg &= ~7;
    if (bpg > tiles_per_group) bpg = tiles_per_group;
    return bpg < 1 ? 1 : bpg;
}

// ---- launch plumbing -----------------------------------------------------------------------------------------------------------------
// compute units of the current device, looked up once per device (the persistent kernels launch one or two blocks per CU)
inline int device_cu_count() {
    static std::mutex mu;
    static std::map<int, int> cus;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    int& n = cus[dev];
    if (n <= 0 && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 0;
    return n > 0 ? n : 256;          // (a failed query: the MI355X's count; the launch itself then reports the error)
}

// The dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) belongs to the pair (kernel, device): raised when a launch needs more
// than the pair was last given, never on a steady-state launch.  Up to 48 KiB need no attribute.  Keyed by function address (many kernels
// share a signature); one mutex, as independent handles may launch from several threads.
inline hipError_t ensure_dynamic_lds(const void* fn, size_t bytes) {
    if (bytes <= 48 * 1024) return hipSuccess;
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, size_t> given;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    size_t& g = given[{fn, dev}];
    if (bytes <= g) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes));
    if (e == hipSuccess) g = bytes;
    return e;
}

// kernel<<<grid, block, smem, stream>>>(args...) behind ensure_dynamic_lds; returns the launch's error (ENDO_LAUNCH_CHECK's)
template <typename... Params, typename... Args>
inline hipError_t launch_dyn(void (*kernel)(Params...), dim3 grid, dim3 block, size_t smem, hipStream_t stream, Args&&... args) {
    const hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), smem);
    if (e != hipSuccess) return e;
    kernel<<<grid, block, smem, stream>>>(std::forward<Args>(args)...);
    return hipGetLastError();
}

// A stream of the handle's own beside the caller's ("main") stream -- both network families run their weight gradients on one.  Work issued
// on it after fork_after(main) follows everything issued on main so far; after join_into(main), main follows everything issued on it.
// A pass joins on EVERY exit path once it may have forked (its forking part runs in a lambda, the join behind it): an error return never
// leaves the side stream running against the caller's buffers.
struct SideStream {
    hipStream_t stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;

    // on first use, on the caller's device: the stream and both events, or (an error) none of them
    hipError_t create() {
        if (stream) return hipSuccess;
        SideStream s;
        hipError_t e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.ev_fork, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.ev_join, hipEventDisableTiming);
        if (e == hipSuccess) *this = s;
        else s.destroy();
        return e;
    }
    hipError_t fork_after(hipStream_t main) const {
        const hipError_t e = hipEventRecord(ev_fork, main);
        return e != hipSuccess ? e : hipStreamWaitEvent(stream, ev_fork, 0);
    }
    hipError_t join_into(hipStream_t main) const {
        const hipError_t e = hipEventRecord(ev_join, stream);
        return e != hipSuccess ? e : hipStreamWaitEvent(main, ev_join, 0);
    }
    void destroy() {
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (stream) (void)hipStreamDestroy(stream);
        *this = SideStream();
    }
};

}  // namespace endo

// geometry.hip / losses.hip, used by head.hip: the public entry points with their reduction tables' memset optional (zero = 0: the caller has
// zeroed them -- the loss head does so for all of its tables with one memset).  Not part of the C ABI.
int endo_depth_scale_fwd_impl(const float* pred, const float* sparse_depth, const float* sparse_mask, float* scaled, float* ratio, double* stats,
                              int n, int hw, float eps, int zero, hipStream_t stream);
int endo_depth_scale_bwd_impl(const float* grad_scaled, const float* grad_ratio, const float* pred, const float* sparse_depth, const double* stats,
                              float* grad_pred, double* work, int n, int hw, float eps, int zero, hipStream_t stream);
int endo_sparse_l1_fwd_impl(const float* flows, const float* flows_hat, const float* mask, float* loss, double* stats, int n, int c, int hw,
                            float eps, int zero, hipStream_t stream);

// geometry.hip, used by head.hip: the fused depth-warp + consistency-loss kernels (endo_warp_consistency), forward (phase 1: memset,
// forward kernel, and -- unless the caller asks for the loss only at the end -- the one-wave finalize) and backward (phase 2).  Not part
// of the C ABI.  zero_grads: 1 = the forward kernel zeroes grad_depth_* and the backward kernel also writes the loss (the stand-alone
// call); 0 = the caller has initialised grad_depth_* (the loss head: its flow terms) and reads the loss between the phases.
int endo_consistency_phase(int phase, const float* depth_1, const float* depth_2, const float* boundaries, const float* t_1_wrt_2,
                           const float* r_1_wrt_2, const float* t_2_wrt_1, const float* r_2_wrt_1, const float* intrinsics, float dcl_weight,
                           float eps, float* loss, float* grad_depth_1, float* grad_depth_2, float* workspace, int n, int h, int w,
                           int zero_grads, int form, float form_eps, hipStream_t stream);
// geometry.hip: a loss form ENDO_CONSISTENCY_* (include/endo_hip.h) and a finite, positive eps for it
bool endo_consistency_form_ok(int form, float form_eps);
// geometry.hip: where phase 1 leaves the two intersect masks (n x h x w floats each) in endo_consistency_phase's workspace
void endo_consistency_intersect_planes(float* workspace, int n, int h, int w, float** inter_1, float** inter_2);

// image_warp.hip, used by head.hip: the photometric term's forward kernel (phase 1; the caller has zeroed stats, [dirs][n][2] doubles)
// and backward kernel (phase 2) for dirs = 1 or 2 directions in one launch.  Each pointer argument holds one entry per direction; phase
// 1 reads colors_1 .. R and writes stats and plane, phase 2 reads stats, plane and upstream (one device float per direction) and writes
// (accumulate = 0) or adds to (1) grad.  Not part of the C ABI.
int endo_photometric_phase(int phase, int dirs, const float* const* colors_1, const float* const* colors_2, const float* const* depth,
                           const float* mask, const float* const* inter, const float* const* t, const float* const* R, const float* K,
                           double* stats, float* const* plane, const float* const* upstream, float* const* grad, int accumulate, int n,
                           int c, int h, int w, float eps, int padding_mode, hipStream_t stream);

namespace endo {

// live profiling hooks (prof.hip)
struct ProfScope {
    int family;
    hipStream_t stream;
    void* slot;
    ProfScope(int family, hipStream_t stream, double flops, double bytes);
    ~ProfScope();
};

enum ProfFamily {
    kProfConv3x3Dense = 0,   // dense-layer conv3x3 Cin->12 forward (BN+ReLU fused on load)
    kProfConv3x3Up = 1,      // transition-up conv3x3 48->48 forward (nearest x2 fused on load)
    kProfConv1x1Pool = 2,    // transition-down conv1x1 + maxpool forward
    kProfConvFirst = 3,      // first conv 3->48
    kProfConvFinal = 4,      // final conv 192->1 + abs (fwd and bwd)
    kProfDgradDense = 5,     // dense-layer dgrad + BN/ReLU backward
    kProfWgradDense = 6,     // dense-layer wgrad
    kProfDgradOther = 7,     // transition dgrads
    kProfWgradOther = 8,     // transition / first conv wgrads
    kProfSmall = 9,          // BN finalize / dY preparation / misc
    kProfGeometry = 10,      // depth scaling, flow, warp
    kProfLoss = 11,          // loss reductions
    kProfOptimizer = 12,     // clip + SGD
};

}  // namespace endo
