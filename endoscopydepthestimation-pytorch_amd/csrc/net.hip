// FC-DenseNet57 forward / backward schedule on the HIP kernels of conv_kernels.h / wgrad_kernels.h.
//
// Data layout in HBM (all fp32, NCHW planar, caller-owned):
//   one "level buffer" U_L per resolution level L = 0..4 (H>>L x W>>L) holding, as channel planes,
//       [0,48)              transition-up output of the up path
//       [48, 48+C_L)        down-block input            (C_L = 48 + 48 L)
//       [48+C_L, 96+C_L)    the 4 x 12 maps the down block adds
//       [96+C_L, 144+C_L)   the 4 x 12 maps the up block adds
//   and U_5 (bottleneck, H>>5) = [0,288) input, [288,336) new maps.
//   Every convolution reads a channel range of a level buffer and writes a disjoint range of the
//   same (or the next) level buffer, so torch.cat (reference models.py:46,48,52,79) never happens:
//   the skip connection is simply the range [48, 96+C_L) that both paths address.
//   The gradient workspace mirrors this layout.
// Training-mode BatchNorm: per-channel sum / sum^2 (fp64) are produced once, by the epilogue of the
// kernel that writes the channel, and consumed by every later BN over it (each with its own
// gamma/beta and running statistics).
#include <new>
#include <vector>

#include "dgrad_kernels.h"
#include "dgrad_block_kernels.h"
#include "dgrad_newmap_kernels.h"
#include "td_dgrad_kernels.h"
#include "td_fwd_kernels.h"
#include "wgrad_taps_kernels.h"
#include "wgrad1x1_kernels.h"
#include "wgrad_nsplit_kernels.h"
#include "wgrad_f34_kernels.h"
#include "wgrad_subpix_kernels.h"
#include "wino_fwd_kernels.h"
#include "wino4_fwd_kernels.h"
#include "dgrad_wino_kernels.h"
#include "dgrad_wino3_kernels.h"
#include "net_arch.h"

namespace endo {

int run_dgrad_wino3_nl4(const DgradBlockParams& p, const float* const* u, hipStream_t stream);          // dgrad_wino3.hip
bool dgrad_wino3p_applies(const DgradBlockParams& p);
int run_dgrad_wino3p_nl4(const DgradBlockParams& p, const float* const* u, int blocks, double* fw_parts, int* blocks_used, hipStream_t stream);

constexpr int kSideStreamFromLevel = 0;      // weight gradients of levels >= this run on the side stream (in-job A/B: 0 -> -4.7 %, 1 -> -3 %, 2 -> -1.8 % step time)

// what this family adds to the network's modules (net_arch.h)
struct ConvP : ConvDesc { int64_t u = -1, ud = -1; };      // u / ud: offsets of the layer's Winograd-domain forward / data-gradient weights (dense layers), floats
using BnP = BnDesc;                              // saved statistics and backward scratch: pairs from `before`

struct Table : ModuleTable<ConvP> {
    WinoWeightTable wino;                 // the 44 dense layers' forward weights in Winograd form (wino_fwd_kernels.h)
    WinoWeightTable wino4;                // the same layers in F(4x4, 3x3) form (wino4_fwd_kernels.h): u_off in floats of ITS buffer
    int64_t wino4_floats = 0;
    int64_t wino_floats = 0;
    WinoDgradTable wino_dgrad;            // and their data-gradient weights over the base channels of their block (dgrad_wino_kernels.h)
    int64_t wino_dgrad_floats = 0;
};

inline int level_channels(int level) { return level < kLevels ? 144 + down_in(level) : kBottIn + kNew; }

static const Table& table() {
    static Table* t = [] {
        Table* tb = new Table();
        // Winograd-domain weights of the dense layers, layer after layer in module order -- forward: kWinoUStride floats per input channel;
        // data gradient: per dense block, the 16-channel groups of its base channels, for each of its layers
        WinoWeightTable& wt = tb->wino;
        WinoDgradTable& wd = tb->wino_dgrad;
        wt.layers = 0; wt.start[0] = 0;
        wd.layers = 0; wd.start[0] = 0;
        for (const ConvDesc& m : arch().convs) {
            if (!is_dense(m.role)) continue;
            ConvP& c = tb->conv(m);
            const int l = wt.layers++;
            c.u = tb->wino_floats;
            wt.cin[l] = c.cin; wt.cout[l] = c.cout; wt.w_off[l] = c.w; wt.u_off[l] = c.u;
            wt.start[l + 1] = wt.start[l] + c.cin * 16;
            tb->wino_floats += static_cast<int64_t>(c.cin) * kWinoUStride;
            wd.layers++;
            c.ud = tb->wino_dgrad_floats;
            wd.cin[l] = c.cin; wd.groups[l] = dense_base(m) / 16; wd.w_off[l] = c.w; wd.u_off[l] = c.ud;
            wd.start[l + 1] = wd.start[l] + 16 * wd.groups[l] * 12;
            tb->wino_dgrad_floats += static_cast<int64_t>(wd.groups[l]) * kWinoDgradSlice;
        }
        tb->wino4 = wt;
        for (int l = 0; l < wt.layers; ++l) { tb->wino4.u_off[l] = tb->wino4_floats; tb->wino4_floats += static_cast<int64_t>(wt.cin[l]) * kW4UStride; }
        return tb;
    }();
    return *t;
}

}  // namespace endo

using namespace endo;

namespace endo { struct FwdPlan; struct BwdPlan; }

struct endo_net {
    int n, h, w;           // n = samples per group
    int groups;            // independent forward / backward passes batched into every launch (each with its own BN statistics)
    int64_t gs;            // floats between two groups' tapes and between their gradient workspaces
    struct Level { int h, w, t; int64_t plane; int64_t act, grad; int64_t sums; int64_t pq; } lv[kLevels + 1];
    int64_t pre_off;       // final conv pre-activation (floats, tape)
    int64_t saved_off;     // BN saved mean/rstd (floats, tape), 2 per BN channel
    int64_t idx_off[kLevels];   // pool argmax codes (byte offsets from tape base)
    int64_t sums_off;      // fp64 per-channel sums (byte offset, 8-aligned)
    int64_t sums_bytes;
    int64_t tape_floats;
    int64_t partial_off;   // split-K partial sums of the coarse-level dense layers (floats, tape)
    int64_t wino_off;      // Winograd-domain forward weights of the dense layers (floats, tape; group 0's copy serves all groups)
    int64_t wino4_off;     // the same in F(4x4, 3x3) form
    int64_t pq_off;        // floats, gradws: P then Q per level channel
    int64_t pq_floats;
    int64_t scratch_off;   // byte offset in gradws of fp64 BN scratch
    int64_t scratch_bytes;
    int64_t slot_stride;   // doubles between the kBnSlots copies of the BN scratch (common.h)
    int64_t wg_scratch_off;   // float offset in gradws of the weight-gradient partial sums (wgrad_nsplit_kernels.h)
    int64_t tuw_scratch_off;  // float offset in gradws of the transition-up data-gradient weights (tu_subpix_dgrad_weights_kernel)
    int64_t wd_off;           // float offset in gradws of the Winograd-domain data-gradient weights (group 0's copy serves all groups)
    int64_t gplane_off;       // float offset in gradws of g = grad_out * sign(pre), one plane per sample (final_g_kernel)
    int64_t bias_parts_off;   // float offset in gradws (group 0's) of prep_dy's per-block sums of G (BiasParts), bias_parts_floats long
    int64_t fw_parts_off;     // float offset in gradws (group 0's) of the persistent base pass's final-conv weight partials (kFwPartBlocks x 192 doubles)
    int64_t bias_parts_floats;
    int64_t gradws_floats;
    // Weight gradients run on a side stream: a layer's wgrad depends only on its prepared dY and the forward tape, nothing on the
    // backward chain depends on it (it only adds into the flat gradient), so it overlaps the data-gradient chain -- which at the
    // coarse levels is a string of launches too small to fill the chip.  Forked after every prep_dy, joined once at the end.
    SideStream side;
    // kernel-form / precision options of THIS network (endo_net_set_option): two networks in one process never change each
    // other's arithmetic, and a thread stepping one model is not affected by another thread configuring a second one
    int opt[ENDO_OPT_COUNT];
    // copies of the plans the last endo_net_fwd / endo_net_bwd on this handle followed (endo_net_last_plan); null until that pass has run
    FwdPlan* last_fwd;
    BwdPlan* last_bwd;
};

namespace endo {

// ---------------------------------------------------------------------------------------------
// small kernels
// ---------------------------------------------------------------------------------------------

// Conv-bias gradients (sum of the prepared G over pixels and samples, train.py's loss.backward() through models.py's convolutions): prep_dy's blocks
// used to add their sums to bias_grad[c] with one float atomic each -- 3 840 atomics of a level-0 launch on the ONE cache line that holds a
// layer's 12 bias gradients, served one after the other at ~8 ns: 31 of the launch's 57 us (tools/prep_bench: 24.7 us without them, the rate of a
// plain read-2-write-1 pass).  Now a block stores its sum (plain store, its own slot) and ONE launch at the end of the backward pass adds up
// the slots of every prep_dy launch in a fixed order (bias_reduce_kernel): no serialised atomics, and the same bits in every run.
constexpr int kBiasPartChannels = 2048;          // channels prepared per backward pass: 1 776 at FC-DenseNet57 (all conv outputs but the final one)
constexpr int kBiasPartLaunches = 64;
constexpr int kFwPartBlocks = 512;          // persistent blocks whose final-conv weight partials fit the workspace (dgrad_wino3p_kernels.h, FW)
struct BiasReduceTable {
    int n;
    struct Entry { const float* parts; float* bias; int count; int nparts; } e[kBiasPartLaunches];
};
struct BiasParts {          // owned by endo_net_bwd's frame, filled by prep_dy
    BiasReduceTable table;
    int64_t used;           // floats of the region handed out
};

// per BN layer (up to four): its backward sums, saved statistics, parameters and parameter gradients, offset to the first
// channel of the range a launch works on
struct BnFin4 {
    const double* scratch[4];
    const float* saved[4];
    const float* gamma[4];
    float* ggamma[4];
    float* gbeta[4];
};

// G = dbuf + P x + Q in place for a channel range (the deferred mean terms of every BN that consumed
// the channel), and bias gradient += sum G.
// nl > 0: the range's consumers INSIDE its dense block (fin: nl BN layers) have just been differentiated by one fused pass and
// their deferred terms are not in P, Q yet: every block derives them from the pass's sums (the arithmetic of
// bn_bwd_finalize4_kernel, term by term), and the first block of a (channel, group) also adds the BN parameter gradients.
// This takes the separate finalize launch between the pass and this kernel off the backward chain.
// vg: the range's raw gradient is not in dbuf but is the final convolution's rank-one data gradient g(pixel) * vw[channel]
// (DgradBlockParams::vg): read the one plane g instead (first writer of the range).
__global__ void __launch_bounds__(256) prep_dy_kernel(float* __restrict__ dbuf, const float* __restrict__ x, int64_t ns, int plane,
                                                      const float* __restrict__ pq_p, const float* __restrict__ pq_q,
                                                      float* bias_grad, int group_n, int64_t gs, const BnFin4 fin, int nl,
                                                      double count, int training, int64_t slot_stride,
                                                      const float* __restrict__ vg, const float* __restrict__ vw, float* __restrict__ parts) {
    __shared__ double scratch[4];
    const int c = blockIdx.y;
    const int grp = blockIdx.z / group_n, n = blockIdx.z - grp * group_n;      // grouped batch: per-group buffers, shared bias gradient
    float pc = pq_p[grp * gs + c], qc = pq_q[grp * gs + c];
    if (nl > 0) {
        const int64_t go = grp * gs;
        double dp = 0.0, dq = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= nl) break;
            const double s1 = bn_slot_sum(fin.scratch[j] + go / 2 + 2 * c, slot_stride);          // block-uniform addresses
            const double s2 = bn_slot_sum(fin.scratch[j] + go / 2 + 2 * c + 1, slot_stride);
            if (blockIdx.x == 0 && n == 0 && threadIdx.x == 0) {
                atomicAdd(fin.ggamma[j] + c, static_cast<float>(s2));
                atomicAdd(fin.gbeta[j] + c, static_cast<float>(s1));
            }
            if (training) {
                const double mean = fin.saved[j][go + 2 * c], rstd = fin.saved[j][go + 2 * c + 1];
                const double scale = fin.gamma[j][c] * rstd;
                const double k = scale * rstd * s2 / count;
                dp += static_cast<double>(static_cast<float>(-k));
                dq += static_cast<double>(static_cast<float>(-scale * s1 / count + k * mean));
            }
        }
        pc += static_cast<float>(dp);
        qc += static_cast<float>(dq);
    }
    const int64_t base = grp * gs + n * ns + static_cast<int64_t>(c) * plane;
    const float* vg_n = vg ? vg + grp * gs + static_cast<int64_t>(n) * plane : nullptr;          // (block-uniform)
    const float wf = vg ? vw[c] : 0.f;
    float part = 0.f;
    if ((plane & 3) == 0 && !vg_n) {
        // two iterations' loads in flight per thread (round 5: +0.2 % on the step in three alternating in-job runs; non-temporal loads of x: +-0)
        const int stride = gridDim.x * blockDim.x * 4;
        int i = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
        for (; i + stride < plane; i += 2 * stride) {
            f32x4 g0 = *reinterpret_cast<const f32x4*>(dbuf + base + i);
            f32x4 g1 = *reinterpret_cast<const f32x4*>(dbuf + base + i + stride);
            const f32x4 x0 = *reinterpret_cast<const f32x4*>(x + base + i);
            const f32x4 x1 = *reinterpret_cast<const f32x4*>(x + base + i + stride);
#pragma unroll
            for (int e = 0; e < 4; ++e) { g0[e] += fmaf(pc, x0[e], qc); part += g0[e]; }
#pragma unroll
            for (int e = 0; e < 4; ++e) { g1[e] += fmaf(pc, x1[e], qc); part += g1[e]; }
            *reinterpret_cast<f32x4*>(dbuf + base + i) = g0;
            *reinterpret_cast<f32x4*>(dbuf + base + i + stride) = g1;
        }
        for (; i < plane; i += stride) {
            f32x4 g = *reinterpret_cast<const f32x4*>(dbuf + base + i);
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + base + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) { g[e] += fmaf(pc, xv[e], qc); part += g[e]; }
            *reinterpret_cast<f32x4*>(dbuf + base + i) = g;
        }
    } else if ((plane & 3) == 0) {
        for (int i = (blockIdx.x * blockDim.x + threadIdx.x) * 4; i < plane; i += gridDim.x * blockDim.x * 4) {
            f32x4 g;
            if (vg_n) {
                const f32x4 gv = *reinterpret_cast<const f32x4*>(vg_n + i);
                g = f32x4{gv[0] * wf, gv[1] * wf, gv[2] * wf, gv[3] * wf};
            } else {
                g = *reinterpret_cast<const f32x4*>(dbuf + base + i);
            }
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + base + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) { g[e] += fmaf(pc, xv[e], qc); part += g[e]; }
            *reinterpret_cast<f32x4*>(dbuf + base + i) = g;
        }
    } else {
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += gridDim.x * blockDim.x) {
            const float g = (vg_n ? vg_n[i] * wf : dbuf[base + i]) + fmaf(pc, x[base + i], qc);
            dbuf[base + i] = g;
            part += g;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double v = wave_sum(static_cast<double>(part));
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0 && bias_grad) {
        const float t = static_cast<float>(scratch[0] + scratch[1] + scratch[2] + scratch[3]);
        // parts: [channel][sample of all groups][block]: added up by bias_reduce_kernel at the end of the backward pass (BiasParts)
        if (parts) parts[(static_cast<int64_t>(c) * gridDim.z + blockIdx.z) * gridDim.x + blockIdx.x] = t;
        else atomicAdd(bias_grad + c, t);
    }
}

// bias[c] += sum of prep_dy's per-block sums, one wave per (launch, channel), fixed order
__global__ void __launch_bounds__(256) bias_reduce_kernel(const BiasReduceTable tb) {
    const BiasReduceTable::Entry& e = tb.e[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = blockIdx.y * 4 + wave; c < e.count; c += gridDim.y * 4) {
        const float* src = e.parts + static_cast<int64_t>(c) * e.nparts;
        double t = 0.0;
        for (int i = lane; i < e.nparts; i += 64) t += static_cast<double>(src[i]);
        t = wave_sum(t);
        if (lane == 0) e.bias[c] += static_cast<float>(t);
    }
}

// BN parameter gradients from the dgrad epilogue's sums, and the deferred dx terms:
//   dx = scale*dz - scale*S1/M - scale*rstd*(S2/M)*(x - mean)   =>   P += -scale*rstd*S2/M,
//   Q += -scale*S1/M + scale*rstd*S2/M*mean          (S1 = sum dz, S2 = sum dz*xhat)
__global__ void bn_bwd_finalize_kernel(const double* __restrict__ scratch, const float* __restrict__ saved,
                                       const float* __restrict__ gamma, float* __restrict__ ggamma, float* __restrict__ gbeta,
                                       float* __restrict__ pq_p, float* __restrict__ pq_q, int c_count, double count, int training,
                                       int64_t gs, int64_t slot_stride) {
    // blockIdx.y = sample group: its own sums, statistics and deferred terms; the parameter gradients add up over groups
    scratch += blockIdx.y * (gs / 2); saved += blockIdx.y * gs; pq_p += blockIdx.y * gs; pq_q += blockIdx.y * gs;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < c_count; c += gridDim.x * blockDim.x) {
        const double s1 = bn_slot_sum(scratch + 2 * c, slot_stride), s2 = bn_slot_sum(scratch + 2 * c + 1, slot_stride);
        atomicAdd(ggamma + c, static_cast<float>(s2));
        atomicAdd(gbeta + c, static_cast<float>(s1));
        if (training) {
            const double mean = saved[2 * c], rstd = saved[2 * c + 1];
            const double scale = gamma[c] * rstd;
            const double k = scale * rstd * s2 / count;
            pq_p[c] += static_cast<float>(-k);
            pq_q[c] += static_cast<float>(-scale * s1 / count + k * mean);
        }
    }
}

// the same for up to four BN layers of a dense block over channels they share: one launch, one read-modify-write of
// P and Q
__global__ void bn_bwd_finalize4_kernel(const BnFin4 a, int nl, float* __restrict__ pq_p, float* __restrict__ pq_q, int c_count, double count,
                                        int training, int64_t gs, int64_t slot_stride) {
    const int64_t go = blockIdx.y * gs;          // sample group offset (floats)
    pq_p += go; pq_q += go;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < c_count; c += gridDim.x * blockDim.x) {
        double dp = 0.0, dq = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= nl) break;          // nl = layers in use (block-uniform)
            const double s1 = bn_slot_sum(a.scratch[j] + go / 2 + 2 * c, slot_stride);
            const double s2 = bn_slot_sum(a.scratch[j] + go / 2 + 2 * c + 1, slot_stride);
            atomicAdd(a.ggamma[j] + c, static_cast<float>(s2));
            atomicAdd(a.gbeta[j] + c, static_cast<float>(s1));
            if (training) {
                const double mean = a.saved[j][go + 2 * c], rstd = a.saved[j][go + 2 * c + 1];
                const double scale = a.gamma[j][c] * rstd;
                const double k = scale * rstd * s2 / count;
                // same rounding sequence as four single-layer finalizes: each term is rounded to fp32 before it is added
                dp += static_cast<double>(static_cast<float>(-k));
                dq += static_cast<double>(static_cast<float>(-scale * s1 / count + k * mean));
            }
        }
        if (training) {
            pq_p[c] += static_cast<float>(dp);
            pq_q[c] += static_cast<float>(dq);
        }
    }
}

// Tap-summed weights of the transition-up forward in sub-pixel form (conv_dma_kernels.h, tu_fwd_subpix_kernel) in the layout the kernel
// DMAs: out[ci][rc = 3 r + c][48] = W'[r][c][co][ci] = sum over ky in rows(r), kx in cols(c) of w[co][ci][ky][kx], with r, c in {-, 0, +}
// and rows(-) = {0}, rows(0) = {0, 1, 2}, rows(+) = {2} (tu_tap_range); summed in fp32 in (ky, kx) order.  Couts past `cout` are zeros.
__host__ __device__ inline void tu_tap_range(int r, int& k0, int& k1) { k0 = r == 2 ? 2 : 0; k1 = r == 0 ? 0 : 2; }

__global__ void tu_phase_weights_kernel(const float* __restrict__ w, int cout, int cin, float* __restrict__ out) {
    const int total = cin * kTuW9;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int co = i % 48;
        const int rc = (i / 48) % 9;
        const int ci = i / kTuW9;
        float v = 0.f;
        if (co < cout) {
            const float* src = w + (static_cast<int64_t>(co) * cin + ci) * 9;
            int ky0, ky1, kx0, kx1;
            tu_tap_range(rc / 3, ky0, ky1);
            tu_tap_range(rc % 3, kx0, kx1);
            for (int ky = ky0; ky <= ky1; ++ky)
                for (int kx = kx0; kx <= kx1; ++kx) v += src[ky * 3 + kx];
        }
        out[i] = v;
    }
}

// The same nine matrices for the transition-up DATA gradient (conv_dma_kernels.h, tu_dgrad_subpix_kernel), transposed:
// out[co][rc = 3 r + c][48] = W'[r][c][co][ci].  Cins past `cin` are zeros.
__global__ void tu_subpix_dgrad_weights_kernel(const float* __restrict__ w, int cout, int cin, float* __restrict__ out) {
    const int total = cout * kTuW9;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int ci = i % 48;
        const int rc = (i / 48) % 9;
        const int co = i / kTuW9;
        float v = 0.f;
        if (ci < cin) {
            const float* src = w + (static_cast<int64_t>(co) * cin + ci) * 9;
            int ky0, ky1, kx0, kx1;
            tu_tap_range(rc / 3, ky0, ky1);
            tu_tap_range(rc % 3, kx0, kx1);
            for (int ky = ky0; ky <= ky1; ++ky)
                for (int kx = kx0; kx <= kx1; ++kx) v += src[ky * 3 + kx];
        }
        out[i] = v;
    }
}

// split-K epilogue of the coarse-level dense layers: out = bias + sum over K slices of the partial sums,
// plus the per-channel sum / sum^2 that later BN layers need.  grid (x blocks, channel, sample).
__global__ void __launch_bounds__(256) finalize_partial_kernel(const float* __restrict__ partial, int64_t split_stride, int ksplit,
                                                               int64_t pns, int plane, const float* __restrict__ bias,
                                                               float* __restrict__ out, int64_t out_ns, double* out_sums,
                                                               int group_n, int64_t gs) {
    __shared__ double scratch[2 * 4];
    const int c = blockIdx.y;
    const int grp = blockIdx.z / group_n, n = blockIdx.z - grp * group_n;
    partial += grp * gs; out += grp * gs;
    if (out_sums) out_sums += grp * (gs / 2);
    const float b = bias[c];
    float part[2] = {0.f, 0.f};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += gridDim.x * blockDim.x) {
        float v = b;
        for (int s = 0; s < ksplit; ++s) v += partial[s * split_stride + n * pns + static_cast<int64_t>(c) * plane + i];
        out[n * out_ns + static_cast<int64_t>(c) * plane + i] = v;
        part[0] += v;
        part[1] += v * v;
    }
    if (out_sums) block_sum_atomic<2>(part, out_sums + 2 * c, scratch);          // (block-uniform) no statistics in inference mode
}

// final 1x1 conv 192 -> 1 and |.| (reference models.py:186).  HBM-bound: reads each plane once.
// c_first > 0: `pre` already holds the sum over channels [0, c_first) (wino4_fwd_kernel<true>, the last dense layer's launch) and only the rest is read
__global__ void __launch_bounds__(256) final_fwd_kernel(const float* __restrict__ u, int64_t ns, int plane, int cin,
                                                        const float* __restrict__ wgt, const float* __restrict__ bias,
                                                        float* __restrict__ pre, float* __restrict__ out, int group_n, int64_t gs, int c_first) {
    __shared__ float s_w[192];
    for (int c = threadIdx.x; c < cin; c += blockDim.x) s_w[c] = wgt[c];
    __syncthreads();
    // u and pre live in the sample group's tape, out is the caller's [groups * group_n] tensor
    const int grp = blockIdx.y / group_n, n = blockIdx.y - grp * group_n;
    u += grp * gs;
    if (pre) pre += grp * gs;
    out += static_cast<int64_t>(grp) * group_n * plane;
    const bool vec = (plane & 3) == 0;
    if (vec) {
        for (int i = (blockIdx.x * blockDim.x + threadIdx.x) * 4; i < plane; i += gridDim.x * blockDim.x * 4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            if (c_first > 0) acc = *reinterpret_cast<const f32x4*>(pre + static_cast<int64_t>(n) * plane + i);
            const float* src = u + n * ns + i;
            for (int c = c_first; c < cin; ++c) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(src + static_cast<int64_t>(c) * plane);
                const float wc = s_w[c];
                acc[0] = fmaf(v[0], wc, acc[0]); acc[1] = fmaf(v[1], wc, acc[1]);
                acc[2] = fmaf(v[2], wc, acc[2]); acc[3] = fmaf(v[3], wc, acc[3]);
            }
            const float b = bias[0];
            f32x4 o;
            for (int e = 0; e < 4; ++e) { acc[e] += b; o[e] = fabsf(acc[e]); }
            if (pre) *reinterpret_cast<f32x4*>(pre + static_cast<int64_t>(n) * plane + i) = acc;
            *reinterpret_cast<f32x4*>(out + static_cast<int64_t>(n) * plane + i) = o;
        }
    } else {
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += gridDim.x * blockDim.x) {
            float acc = c_first > 0 ? pre[static_cast<int64_t>(n) * plane + i] : 0.f;
            for (int c = c_first; c < cin; ++c) acc = fmaf(u[n * ns + static_cast<int64_t>(c) * plane + i], s_w[c], acc);
            acc += bias[0];
            if (pre) pre[static_cast<int64_t>(n) * plane + i] = acc;
            out[static_cast<int64_t>(n) * plane + i] = fabsf(acc);
        }
    }
}

__device__ __forceinline__ float sign_of(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// g = gout * sign(pre): the one plane the final convolution's data gradient g * w[c] is made of (DgradBlockParams::vg) -- the kernels of the
// last up block form the 192 products themselves instead of reading them back from 192 planes
__global__ void __launch_bounds__(256) final_g_kernel(const float* __restrict__ gout, const float* __restrict__ pre, float* __restrict__ g,
                                                      int plane, int group_n, int64_t gs) {
    const int grp = blockIdx.y / group_n, n = blockIdx.y - grp * group_n;
    gout += static_cast<int64_t>(blockIdx.y) * plane; pre += grp * gs + static_cast<int64_t>(n) * plane; g += grp * gs + static_cast<int64_t>(n) * plane;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += gridDim.x * blockDim.x) g[i] = gout[i] * sign_of(pre[i]);
}

// dbuf[c] = (gout * sign(pre)) * w[c] for planes [c_first, cin) (first writer of the level-0 gradient buffer)
__global__ void __launch_bounds__(256) final_bwd_data_kernel(const float* __restrict__ gout, const float* __restrict__ pre,
                                                             const float* __restrict__ wgt, float* __restrict__ dbuf,
                                                             int64_t ns, int plane, int cin, int group_n, int64_t gs, int c_first) {
    __shared__ float s_w[192];
    for (int c = threadIdx.x; c < cin; c += blockDim.x) s_w[c] = wgt[c];
    __syncthreads();
    const int grp = blockIdx.y / group_n, n = blockIdx.y - grp * group_n;
    gout += static_cast<int64_t>(grp) * group_n * plane; pre += grp * gs; dbuf += grp * gs;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += gridDim.x * blockDim.x) {
        const float g = gout[static_cast<int64_t>(n) * plane + i] * sign_of(pre[static_cast<int64_t>(n) * plane + i]);
        for (int c = c_first; c < cin; ++c) dbuf[n * ns + static_cast<int64_t>(c) * plane + i] = g * s_w[c];
    }
}

// dw[c] += sum g * u[c]; channel index cin is the bias (sum g).  grid (cin + 1, slices, n): float4 streaming,
// two independent accumulators; g = gout * sign(pre) is recomputed from two L2-resident planes.
// c_first: the channels below it are left to the last up block's persistent base pass (dgrad_wino3p_kernels.h, FW); grid.x = cin - c_first + 1
__global__ void __launch_bounds__(256) final_bwd_weight_kernel(const float* __restrict__ gout, const float* __restrict__ pre,
                                                               const float* __restrict__ u, int64_t ns, int plane, int cin,
                                                               int group_n, int64_t gs, float* __restrict__ gw, float* __restrict__ gb, int c_first) {
    __shared__ double scratch[4];
    const int c = c_first + blockIdx.x;
    const int grp = blockIdx.z / group_n, n = blockIdx.z - grp * group_n;
    const float* gp = gout + static_cast<int64_t>(blockIdx.z) * plane;
    const float* pp = pre + grp * gs + static_cast<int64_t>(n) * plane;
    const float* up = u + grp * gs + n * ns + static_cast<int64_t>(c < cin ? c : 0) * plane;
    float part = 0.f, part2 = 0.f;
    if ((plane & 3) == 0) {
        const int stride = gridDim.y * blockDim.x * 4;
        for (int i = (blockIdx.y * blockDim.x + threadIdx.x) * 4; i < plane; i += stride) {
            const f32x4 gv = *reinterpret_cast<const f32x4*>(gp + i);
            const f32x4 pv = *reinterpret_cast<const f32x4*>(pp + i);
            f32x4 uv = {1.f, 1.f, 1.f, 1.f};
            if (c < cin) uv = *reinterpret_cast<const f32x4*>(up + i);
            part += gv[0] * sign_of(pv[0]) * uv[0] + gv[1] * sign_of(pv[1]) * uv[1];
            part2 += gv[2] * sign_of(pv[2]) * uv[2] + gv[3] * sign_of(pv[3]) * uv[3];
        }
    } else {
        for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < plane; i += gridDim.y * blockDim.x)
            part += gp[i] * sign_of(pp[i]) * (c < cin ? up[i] : 1.f);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double v = wave_sum(static_cast<double>(part + part2));
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float t = static_cast<float>(scratch[0] + scratch[1] + scratch[2] + scratch[3]);
        if (c < cin) atomicAdd(gw + c, t); else atomicAdd(gb, t);
    }
}

// dW_final[c] += sum over the persistent base pass's blocks of its partial: one wave per channel, fixed order (fp64)
__global__ void __launch_bounds__(64) final_w_reduce_kernel(const double* __restrict__ parts, int nblocks, int count, float* __restrict__ gw) {
    const int c = blockIdx.x;
    double t = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 64) t += parts[static_cast<int64_t>(b) * count + c];
    t = wave_sum(t);
    if (threadIdx.x == 0) atomicAdd(gw + c, static_cast<float>(t));
}

// ---------------------------------------------------------------------------------------------
// the plan: which kernel form every launch of a pass takes
// ---------------------------------------------------------------------------------------------
// Filled once at the top of endo_net_fwd / endo_net_bwd by plan_fwd / plan_bwd (below the parameter fillers they share with the launch
// functions) from the network, its options (documented in include/endo_hip.h), the pass's pointers and the training flag.  The launch
// functions switch on it and the weight-preparation launches read the same entries, so a layer's prepared weights are in the layout the
// kernel that runs reads, by construction.  Dense blocks are numbered the way the weight tables are laid out: 0-4 the down path,
// 5 the bottleneck, 6-10 the up path (coarsest first); dense layer j of block b is entry 4 b + j.
constexpr int kBlocks = 2 * kLevels + 1, kDense = kBlocks * kLayers;

enum class DenseFwd { Wino4, Wino2_32x16, Wino2_32x8, SplitK, Direct32x8, Direct16x8, DirectAuto };          // F(4x4, 3x3) | F(2x2, 3x3) by tile | direct kernels
struct FwdPlan {
    struct Dense {
        DenseFwd form;
        int ksplit;                   // K slices of SplitK
        bool chunk_weights;           // the layer's slot of the prepared weights holds the direct kernel's K-chunk order (WinoWeightTable::mode 1)
    } dense[kDense];
    bool bf16;                        // bf16 MFMA operands: direct kernels only, no prepared weights
    bool wino4_weights;               // the F(4x4, 3x3) weights are prepared
    bool fuse_final;                  // the network's last dense layer also forms the final convolution's sum over its 180 input channels
    bool td_persistent[kLevels];      // td_fwd_kernels.h instead of the per-tile kernel
    bool tu_subpix[kLevels];          // by the level the transition writes: the sub-pixel form instead of upsample-then-convolve
};

enum class NewMap { Bf16, Persistent, Vec16, Dword };
enum class BasePass { Block8, Block8Bf16, Wino3, Wino3Persistent, Wino8 };
enum class DenseWgrad { F34, NSplit, Taps, Direct };
enum class TdDgrad { Persistent, Runs128, Dma, Staged };
enum class TuWgrad { Subpix, Taps, Direct };
enum class TuDgrad { Subpix32x8, Subpix16x8, Subpix16x4, Plain };
enum class FirstWgrad { F34Prep, F34, Taps, Direct };
struct BwdPlan {
    struct Block {
        bool fused;                   // new-map passes + one base pass (dgrad_block_kernels.h) instead of four per-layer data gradients
        NewMap newmap[kLayers];       // [j]: the pass into layer j-1's maps from layers j..3 (j = 1..3)
        BasePass base;
        bool wino3_layout;            // its layers' data-gradient weights in the phase-skewed kernels' U layout (dgrad_wino_weights_kernel, layout 1)
    } block[kBlocks];
    DenseWgrad wgrad[kDense];
    bool td_wgrad_dma[kLevels];
    TdDgrad td_dgrad[kLevels];
    TuWgrad tu_wgrad[kLevels];        // both by the level whose gradient the transition reads
    TuDgrad tu_dgrad[kLevels];
    int overlap;                      // ENDO_OPT_WGRAD_OVERLAP as set
    bool bf16_wgrad, bf16_dgrad;      // operands rounded to bf16 in the kernels that have such a form
    bool dgrad_weights;               // the Winograd-domain data-gradient weights are prepared
    // final convolution (FinalVirt) and first convolution
    bool use_virt;                    // the last up block forms the final convolution's data gradient where it first touches a channel ...
    bool virt_base;                   // ... its base pass too
    bool virt_base_w;                 // ... which then also forms that convolution's weight gradient of the base channels
    int materialise;                  // channels [0, materialise) are written out by final_bwd_data_kernel
    int c_first;                      // final_bwd_weight_kernel starts at this channel
    FirstWgrad first;
};

// ---------------------------------------------------------------------------------------------
// schedule helpers
// ---------------------------------------------------------------------------------------------
struct Ctx {
    const endo_net* net;
    const float* params;
    float* bn_running;
    float* tape;
    float* grads;
    float* gradws;
    int training;
    hipStream_t stream;
    BiasParts* bias_parts = nullptr;
    const float* x = nullptr;              // endo_net_bwd: the caller's image tensor
    const FwdPlan* fwd = nullptr;          // the pass's plan (one of the two)
    const BwdPlan* bwd = nullptr;

    int nt() const { return net->n * net->groups; }      // samples of all groups
    // context of the weight-gradient side stream, ordered after everything issued so far on the main stream
    int fork_wgrad(Ctx& side, int level) const {
        side = *this;
        if (!net->side.stream || !bwd->overlap || level < kSideStreamFromLevel) return 0;          // run in line
        ENDO_CHECK(net->side.fork_after(stream));
        side.stream = net->side.stream;
        return 0;
    }
    float* act(int level) const { return tape + net->lv[level].act; }
    float* gbuf(int level) const { return gradws + net->lv[level].grad; }
    double* sums(int level) const { return reinterpret_cast<double*>(reinterpret_cast<char*>(tape) + net->sums_off) + net->lv[level].sums; }
    // where a kernel accumulates the per-channel sum / sum^2 of what it stores: nowhere in inference mode (running statistics are
    // used, reference evaluate.py:317-345), which drops the reductions and their atomics from every epilogue
    double* out_sums(int level, int channel) const { return training ? sums(level) + 2 * channel : nullptr; }
    float* saved(const BnP& b) const { return tape + net->saved_off + 2 * b.before; }
    double* scratch(const BnP& b) const { return reinterpret_cast<double*>(reinterpret_cast<char*>(gradws) + net->scratch_off) + 2 * b.before; }
    float* pq_p(int level) const { return gradws + net->pq_off + 2 * net->lv[level].pq; }
    float* pq_q(int level) const { return pq_p(level) + net->lv[level].t; }
    uint8_t* idx(int level) const { return reinterpret_cast<uint8_t*>(tape) + net->idx_off[level]; }
};

static void fill_bn_in(const Ctx& c, ConvParams& p, const BnP& b, int level, int ic0) {
    const auto& lv = c.net->lv[level];
    p.in_sums = c.sums(level) + 2 * ic0;
    p.gamma = c.params + b.g;
    p.beta = c.params + b.b;
    p.running_mean = c.bn_running + b.run;
    p.running_var = c.bn_running + b.run + b.c;
    p.saved = c.tape ? c.saved(b) : nullptr;
    p.count = static_cast<double>(c.net->n) * lv.h * lv.w;      // per sample group
    p.eps = kBnEps;
    p.momentum = kBnMomentum;
    p.training = c.training;
}

static void fill_in(const Ctx& c, ConvParams& p, const float* base, int level, int ic0, int cin) {
    const auto& lv = c.net->lv[level];
    p.in = base + ic0 * lv.plane;
    p.in_ns = lv.t * lv.plane;
    p.in_cs = static_cast<int>(lv.plane);
    p.in_w = lv.w;
    p.cin = cin;
}

static void fill_out(const Ctx& c, ConvParams& p, float* base, int level, int oc0, int cout) {
    const auto& lv = c.net->lv[level];
    p.out = base + oc0 * lv.plane;
    p.out_ns = lv.t * lv.plane;
    p.out_cs = static_cast<int>(lv.plane);
    p.out_w = lv.w;
    p.cout = cout;
}

static void fill_grid(const Ctx& c, ConvParams& p, int level) {
    const auto& lv = c.net->lv[level];
    p.n = c.nt(); p.h = lv.h; p.w = lv.w;
    p.group_n = c.net->n; p.gs = c.net->gs; p.in_gs = c.net->gs; p.out_gs = c.net->gs;      // tape / workspace pointers by default
}

static double conv_flops(const endo_net* net, int level, int cin, int cout, int ks) {
    return 2.0 * net->n * net->groups * net->lv[level].plane * cin * cout * ks * ks;
}

// Defaults of the per-handle options (endo_net_set_option; include/endo_hip.h documents every value).  plan_fwd / plan_bwd are their only readers.
static void default_options(int (&opt)[ENDO_OPT_COUNT]) {
    opt[ENDO_OPT_WINO_FWD] = 5;          // F(4x4, 3x3) where its 64 x 16 blocks fill the chip (level 0 of configs[1]), F(2x2, 3x3) below: depth 5e-6 of its maximum from fp64 against the 1e-4 of the parity target
    opt[ENDO_OPT_WINO_DGRAD] = 3;
    opt[ENDO_OPT_DGRAD_VEC] = 2;
    opt[ENDO_OPT_WINO_MIN_TILES] = 1024;
    opt[ENDO_OPT_MFMA_BF16] = 0;
    opt[ENDO_OPT_WGRAD_OVERLAP] = 1;
    opt[ENDO_OPT_WGRAD_F34] = 1;
    opt[ENDO_OPT_FINAL_VIRTUAL] = 1;
    opt[ENDO_OPT_TD_PERSIST] = 3;
    opt[ENDO_OPT_CHIP_DIVISOR] = 1;
}
// ENDO_OPT_CHIP_DIVISOR d: every does-it-fill-the-chip comparison of the plan sees its tile / chunk count times d, and the persistent launches
// get 1 / d of the compute units -- a small grid then takes the forms, and its blocks walk the runs of tiles, of a grid d times its size
static long chip_divisor(const endo_net* net) { const int d = net->opt[ENDO_OPT_CHIP_DIVISOR]; return d < 1 ? 1 : d; }
static int persistent_cus(const endo_net* net) { const int cus = static_cast<int>(device_cu_count() / chip_divisor(net)); return cus < 1 ? 1 : cus; }
// ENDO_OPT_MFMA_BF16 as a mask of kernel families -- bit 0: weight gradients, bit 1: forward, bit 2: data gradients of the dense layers (1 = all three)
static int bf16_mask(const int* opt) { const int v = opt[ENDO_OPT_MFMA_BF16]; return v == 1 ? 7 : (v >> 1); }

// Dense block b (numbering: FwdPlan): level-buffer channels [ic0, ic0 + c0) are its input ("base"), layer j reads [ic0, ic0 + c0 + 12 j)
// and writes the 12 maps behind them
struct DenseBlock { int level, ic0, c0; const BnP* bn; const ConvP* cv; bool base_overwrite; };          // base_overwrite: the backward pass is the first writer of the base channels' gradient
static DenseBlock dense_block(int b) {
    const Table& tb = table();
    if (b < kLevels) return {b, 48, down_in(b), tb.down_bn[b], tb.down_conv[b], false};
    if (b == kLevels) return {kLevels, 0, kBottIn, tb.bott_bn, tb.bott_conv, true};
    const int i = b - kLevels - 1, l = kLevels - 1 - i;
    return {l, 0, up_in(l), tb.up_bn[i], tb.up_conv[i], l > 0};
}
static long tile_count(const Ctx& c, int level, int tx, int ty) {          // tx x ty pixel tiles of a launch over the level, partial ones included
    const auto& lv = c.net->lv[level];
    return static_cast<long>((lv.w + tx - 1) / tx) * ((lv.h + ty - 1) / ty) * c.nt() * chip_divisor(c.net);
}

// dense layer forward: BN -> ReLU -> conv3x3 -> +12 channels (reference models.py:19-28, 44-52), with the weights where `form` reads them
static ConvParams dense_fwd_params(const Ctx& c, const DenseBlock& k, int j, DenseFwd form) {
    const ConvP& cv = k.cv[j];
    const int oc0 = k.ic0 + k.c0 + kGrowth * j;
    ConvParams p{};
    fill_grid(c, p, k.level);
    fill_in(c, p, c.act(k.level), k.level, k.ic0, cv.cin);
    fill_bn_in(c, p, k.bn[j], k.level, k.ic0);
    p.wgt = c.params + cv.w; p.bias = c.params + cv.b; p.w_cout = cv.cout; p.w_cin = cv.cin;
    fill_out(c, p, c.act(k.level), k.level, oc0, cv.cout);
    p.out_sums = c.out_sums(k.level, oc0);
    // the prepared weights live in group 0's tape: they are shared by the groups
    if (form == DenseFwd::Wino4) p.wgt = c.tape + c.net->wino4_off + cv.u / kWinoUStride * kW4UStride;
    if (form == DenseFwd::Wino2_32x16 || form == DenseFwd::Wino2_32x8) p.wgt = c.tape + c.net->wino_off + cv.u;
    return p;
}

// transition down: BN -> ReLU -> conv1x1 -> maxpool2 into the next level (models.py:56-67)
static ConvParams td_fwd_params(const Ctx& c, int level) {
    const BnP& b = table().td_bn[level];
    const ConvP& cv = table().td_conv[level];
    const int next = level + 1;
    const int oc0 = next < kLevels ? 48 : 0;
    ConvParams p{};
    fill_grid(c, p, level);
    fill_in(c, p, c.act(level), level, 48, cv.cin);
    fill_bn_in(c, p, b, level, 48);
    p.wgt = c.params + cv.w; p.bias = c.params + cv.b; p.w_cout = cv.cout; p.w_cin = cv.cin;
    fill_out(c, p, c.act(next), next, oc0, cv.cout);
    p.out_idx = c.idx(level);      // [n][cout][pooled plane] bytes, channel index relative to `out`
    p.idx_ns = static_cast<int64_t>(cv.cout) * c.net->lv[next].plane;
    p.out_sums = c.out_sums(next, oc0);
    return p;
}

static FwdPlan plan_fwd(const Ctx& c) {
    const int* opt = c.net->opt;
    const int mode = opt[ENDO_OPT_WINO_FWD];
    const long min_tiles = opt[ENDO_OPT_WINO_MIN_TILES];
    FwdPlan pl{};
    pl.bf16 = (bf16_mask(opt) & 2) != 0;
    // mode 5 prepares the F(4x4, 3x3) weights whether or not a layer takes that form this pass (at small sizes none does)
    pl.wino4_weights = !pl.bf16 && mode == 5;
    for (int b = 0; b < kBlocks; ++b) {
        const DenseBlock k = dense_block(b);
        // Fine levels: Winograd on the matrix cores, from ENDO_OPT_WINO_MIN_TILES tiles per launch on.  F(4x4, 3x3), 36 instead of 64 products
        // per 16 pixels (wino4_fwd_kernels.h), while its 64 x 16 blocks fill the chip (level 0 of configs[1]: at level 1 they no longer do, measured
        // slower); below that F(2x2, 3x3), 4/9 of the multiply-accumulates (wino_fwd_kernels.h), on 32 x 16 pixel tiles while they fill the chip
        // several times over, 32 x 8 below that.
        const long t64x16 = tile_count(c, k.level, 64, 16), t32x16 = tile_count(c, k.level, 32, 16), t32x8 = tile_count(c, k.level, 32, 8);
        const long t16x16 = tile_count(c, k.level, 16, 16), t16x8 = tile_count(c, k.level, 16, 8);
        const bool big = t32x16 >= min_tiles, small = t32x8 >= (min_tiles * 3) / 4;
        const bool wino4_tiles = mode == 5 && !pl.bf16 && 2 * t64x16 >= min_tiles;
        const bool wino2_tiles = mode != 0 && !pl.bf16 && (big || small);
        for (int j = 0; j < kLayers; ++j) {
            FwdPlan::Dense& d = pl.dense[b * kLayers + j];
            const int nchunks = (k.cv[j].cin + 15) / 16;
            // Where the tile counts rule Winograd out the level's layers run a direct kernel and their weights are prepared in its K-chunk order.  (A
            // layer that a Winograd kernel's own shape check sends to the direct kernel reads the original weights.)
            d.chunk_weights = !pl.bf16 && !wino4_tiles && !wino2_tiles;
            if (wino4_tiles && wino4_fwd_ok(dense_fwd_params(c, k, j, DenseFwd::Wino4))) {
                d.form = DenseFwd::Wino4;
            } else if (wino2_tiles && wino_fwd_ok(dense_fwd_params(c, k, j, DenseFwd::Wino2_32x16))) {
                // (round 5, in-job A/B of the level-1 launch: K-chunks of 8 channels, 3 or 4 LDS stages, 4 blocks per CU -- all within +-0.2 % of 32 x 8 with 2 stages)
                d.form = big ? DenseFwd::Wino2_32x16 : DenseFwd::Wino2_32x8;
            } else if (t32x16 < 512 && t16x16 < 384 && t16x8 < 512 && nchunks >= 4) {
                // Coarse levels have too few 16x8 tiles to fill 256 CUs and a long K loop (Cin up to 372): slice K over
                // blockIdx.y, write raw partial sums, and let a small kernel add them up (+ bias, + BN statistics).
                // Scratch bound: slices * N * plane <= (768 / tiles + 1) * 128 * tiles <= 98304 + 65536 floats per channel.
                int want = static_cast<int>(((t16x8 < 256 ? 512 : 768) + t16x8 - 1) / t16x8);
                if (want > nchunks) want = nchunks;
                const int per = (nchunks + want - 1) / want;
                d.form = DenseFwd::SplitK;
                d.ksplit = (nchunks + per - 1) / per;
            } else {
                // Tile shape by block count (tools/conv_bench, Cin = 228 at 128x160): the launch wants >= ~1000 blocks.
                //   16 samples: 32x16 (640 blocks) 257 us, 32x8 (1280) 216 us;   8 samples: 16x16 (640) 143 us, 16x8 (1280) 125 us
                // level 0 stays on 32x16: in the training step (A/B of two library builds inside one job) it is 5 % faster than 32x8,
                // although the isolated microbenchmark prefers 32x8 by 5 %
                d.form = (t32x16 < 1024 && t32x8 >= 1024) ? DenseFwd::Direct32x8
                       : (t32x16 < 1024 && t16x8 >= 768) ? DenseFwd::Direct16x8 : DenseFwd::DirectAuto;
            }
        }
    }
    pl.fuse_final = opt[ENDO_OPT_FINAL_VIRTUAL] && pl.dense[kDense - 1].form == DenseFwd::Wino4;
    for (int l = 0; l < kLevels; ++l) {
        // levels 0 / 1 of configs[1] (96 / 144 channels, whole 32 x 8 tiles): persistent blocks, weights LDS-resident, all output channels per tile (td_fwd_kernels.h)
        pl.td_persistent[l] = (opt[ENDO_OPT_TD_PERSIST] & 2) && !pl.bf16 && c.training && td_fwd_ok(td_fwd_params(c, l));
        const ConvP& tu = table().tu_conv[kLevels - 1 - l];
        pl.tu_subpix[l] = c.net->lv[l + 1].w % 4 == 0 && tu.cout == kNew && tu.cin % 4 == 0;
    }
    return pl;
}

static int dense_fwd(const Ctx& c, int b, int j) {
    const DenseBlock k = dense_block(b);
    const FwdPlan::Dense& d = c.fwd->dense[b * kLayers + j];
    const ConvP& cv = k.cv[j];
    const auto& lv = c.net->lv[k.level];
    const int oc0 = k.ic0 + k.c0 + kGrowth * j;
    ConvParams p = dense_fwd_params(c, k, j, d.form);
    ProfScope prof(kProfConv3x3Dense, c.stream, conv_flops(c.net, k.level, cv.cin, cv.cout, 3),
                   4.0 * c.nt() * lv.plane * (cv.cin + cv.cout));
    // the launches that run on K-chunks of 16 channels take the chunk-ordered copy of the weights the pass prepared for this layer
    const float* chunk_weights = d.chunk_weights ? c.tape + c.net->wino_off + cv.u : nullptr;
    const bool bf16 = c.fwd->bf16;          // (the same tile shapes)
    switch (d.form) {
        case DenseFwd::Wino4:
            if (c.fwd->fuse_final && b == kBlocks - 1 && j == kLayers - 1) { p.fin_w = c.params + table().final_.w + k.ic0; p.fin_out = c.tape + c.net->pre_off; }
            return launch_wino4_fwd(p, c.stream);
        case DenseFwd::Wino2_32x16:
            return launch_wino_fwd<2, 4, 2>(p, c.stream);
        case DenseFwd::Wino2_32x8:
            return launch_wino_fwd<1, 4, 3>(p, c.stream);
        case DenseFwd::SplitK: {
            float* partial = c.tape + c.net->partial_off;
            p.ksplit = d.ksplit;
            p.split_stride = static_cast<int64_t>(c.net->n) * cv.cout * lv.plane;      // inside one group's tape
            p.out = partial; p.out_ns = static_cast<int64_t>(cv.cout) * lv.plane;
            p.bias = nullptr; p.out_sums = nullptr;
            p.wgt_chunks = chunk_weights;
            int rc = bf16 ? launch_conv_dma<3, 16, 1, IN_BNRELU, EPI_FWD, 1, 2, 2, 1, 1>(p, c.stream)
                          : launch_conv_dma<3, 16, 1, IN_BNRELU, EPI_FWD, 1, 2, 2, 1>(p, c.stream);
            if (rc) return rc;
            int bx = static_cast<int>((lv.plane + 255) / 256);
            bx = bx > 8 ? 8 : bx;
            finalize_partial_kernel<<<dim3(bx, cv.cout, c.nt()), 256, 0, c.stream>>>(
                partial, p.split_stride, d.ksplit, p.out_ns, static_cast<int>(lv.plane), c.params + cv.b, c.act(k.level) + oc0 * lv.plane,
                lv.t * lv.plane, c.out_sums(k.level, oc0), c.net->n, c.net->gs);
            ENDO_LAUNCH_CHECK();
            return 0;
        }
        case DenseFwd::Direct32x8:
            return bf16 ? launch_conv_dma<3, 4, 1, IN_BNRELU, EPI_FWD, 2, 4, 2, 1, 1>(p, c.stream) : launch_conv_dma<3, 4, 1, IN_BNRELU, EPI_FWD, 2, 4, 2, 1>(p, c.stream);
        case DenseFwd::Direct16x8:
            return bf16 ? launch_conv_dma<3, 8, 1, IN_BNRELU, EPI_FWD, 1, 2, 2, 1, 1>(p, c.stream) : launch_conv_dma<3, 8, 1, IN_BNRELU, EPI_FWD, 1, 2, 2, 1>(p, c.stream);
        case DenseFwd::DirectAuto:
            if (bf16) return launch_conv_dma_auto<3, 4, 1, IN_BNRELU, EPI_FWD, 8, 2, 1, 1>(p, c.stream);
            p.wgt_chunks = chunk_weights;          // (only the KC = 16 instantiation the auto choice ends in for few tiles reads it)
            return launch_conv_dma_auto<3, 4, 1, IN_BNRELU, EPI_FWD, 8, 2, 1>(p, c.stream);
    }
    return ENDO_E_BADARG;
}

static int td_fwd(const Ctx& c, int level) {
    const ConvP& cv = table().td_conv[level];
    const ConvParams p = td_fwd_params(c, level);
    ProfScope prof(kProfConv1x1Pool, c.stream, conv_flops(c.net, level, cv.cin, cv.cout, 1),
                   4.0 * c.nt() * c.net->lv[level].plane * (cv.cin + cv.cout / 4.0));
    if (c.fwd->td_persistent[level]) return launch_td_fwd(p, persistent_cus(c.net), c.stream);
    if (c.fwd->bf16) return launch_conv_dma_auto<1, 8, 3, IN_BNRELU, EPI_FWD_POOL, 4, 2, 1, 1>(p, c.stream);
    return launch_conv_dma_auto<1, 8, 3, IN_BNRELU, EPI_FWD_POOL, 4>(p, c.stream);    // 32x8 tiles: -6 % in the in-job A/B (Q = 6 was 10 % slower; round 5: K-chunks of 16 channels +-0, of 32 +40 % on the family, Q = 6 with 16 +14 %)
}

// transition up: nearest x2 -> conv3x3 48->48 into channels [0,48) of the finer level (models.py:70-80)
static int tu_fwd(const Ctx& c, int level, int src_level, int src_c0, const ConvP& cv) {
    ProfScope prof(kProfConv3x3Up, c.stream, conv_flops(c.net, level, cv.cin, cv.cout, 3),
                   4.0 * c.nt() * c.net->lv[level].plane * (cv.cin / 4.0 + cv.cout));
    if (c.fwd->tu_subpix[level]) {
        // sub-pixel form: nine products per low-resolution pixel, 1/4 of the direct MACs.  The tap-summed weights
        // go to the (idle) split-K scratch of group 0's tape; they are shared by all groups.
        float* w3 = c.tape + c.net->partial_off;
        tu_phase_weights_kernel<<<(cv.cin * kTuW9 + 255) / 256, 256, 0, c.stream>>>(c.params + cv.w, cv.cout, cv.cin, w3);
        ENDO_LAUNCH_CHECK();
        ConvParams p{};
        fill_grid(c, p, src_level);                     // the launch runs over the low-resolution pixels
        fill_in(c, p, c.act(src_level), src_level, src_c0, cv.cin);
        p.wgt = w3; p.w_cout = cv.cout; p.w_cin = cv.cin;
        p.bias = c.params + cv.b;
        fill_out(c, p, c.act(level), level, 0, cv.cout);
        p.out_sums = c.out_sums(level, 0);
        return launch_tu_fwd_subpix(p, c.stream);
    }
    ConvParams p{};
    fill_grid(c, p, level);
    fill_in(c, p, c.act(src_level), src_level, src_c0, cv.cin);
    p.wgt = c.params + cv.w; p.bias = c.params + cv.b; p.w_cout = cv.cout; p.w_cin = cv.cin;
    fill_out(c, p, c.act(level), level, 0, cv.cout);
    p.out_sums = c.out_sums(level, 0);
    return launch_conv_dma_auto<3, 4, 3, IN_UPSAMPLE, EPI_FWD>(p, c.stream);
}

// The final convolution's data gradient as the "virtual" content of the level-0 gradient buffer (DgradBlockParams::vg): vg = the plane
// g = grad_out * sign(pre) in the gradient workspace, vw = the 192 final-conv weights, gw = that tensor's gradient.  Which passes of the last up
// block form it is in the plan (BwdPlan::use_virt, virt_base, virt_base_w); what is left has been materialised by final_bwd_data_kernel.
struct FinalVirt { const float* vg; const float* vw; float* gw; };

static int prep_dy(const Ctx& c, int level, int c0, int count, float* bias_grad, const BnFin4* fin = nullptr, int nl = 0, const FinalVirt* fv = nullptr) {
    const auto& lv = c.net->lv[level];
    BnFin4 none{};
    int bx = static_cast<int>((lv.plane + 4095) / 4096);      // 16 pixels per thread
    bx = bx < 1 ? 1 : (bx > 32 ? 32 : bx);
    float* parts = nullptr;
    if (bias_grad && c.bias_parts) {          // a full table is an error, not a silent fall-back to the kernel's atomics (whose order is not fixed)
        BiasParts& bp = *c.bias_parts;
        const int64_t need = static_cast<int64_t>(count) * c.nt() * bx;
        if (bp.table.n >= kBiasPartLaunches || bp.used + need > c.net->bias_parts_floats) return ENDO_E_UNSUPPORTED;          // (sized from the network table: endo_net_create_grouped)
        parts = c.gradws + c.net->bias_parts_off + bp.used;
        bp.table.e[bp.table.n++] = {parts, bias_grad, count, c.nt() * bx};
        bp.used += need;
    }
    ProfScope prof(kProfSmall, c.stream, 0.0, 12.0 * c.nt() * lv.plane * count);
    prep_dy_kernel<<<dim3(bx, count, c.nt()), 256, 0, c.stream>>>(c.gbuf(level) + c0 * lv.plane, c.act(level) + c0 * lv.plane,
                                                                     lv.t * lv.plane, static_cast<int>(lv.plane), c.pq_p(level) + c0,
                                                                     c.pq_q(level) + c0, bias_grad, c.net->n, c.net->gs, fin ? *fin : none, fin ? nl : 0,
                                                                     static_cast<double>(c.net->n) * lv.h * lv.w, c.training, c.net->slot_stride,
                                                                     fv ? fv->vg : nullptr, fv ? fv->vw + c0 : nullptr, parts);
    ENDO_LAUNCH_CHECK();
    return 0;
}

// BN parameter gradients + deferred dx terms for channels [first, first + count) of the layer's input
// (ic0 = level-buffer channel of the layer's first input channel)
static int bn_finalize(const Ctx& c, const BnP& b, int level, int ic0, int first = 0, int count = -1) {
    const auto& lv = c.net->lv[level];
    if (count < 0) count = b.c - first;
    if (count <= 0) return 0;
    ProfScope prof(kProfSmall, c.stream, 0.0, 0.0);
    bn_bwd_finalize_kernel<<<dim3((count + 127) / 128, c.net->groups), 128, 0, c.stream>>>(c.scratch(b) + 2 * first, c.saved(b) + 2 * first, c.params + b.g + first,
                                                                       c.grads + b.g + first, c.grads + b.b + first,
                                                                       c.pq_p(level) + ic0 + first, c.pq_q(level) + ic0 + first, count,
                                                                       static_cast<double>(c.net->n) * lv.h * lv.w, c.training, c.net->gs, c.net->slot_stride);
    ENDO_LAUNCH_CHECK();
    return 0;
}

static void fill_wgrad_grid(const Ctx& c, WgradParams& p, int level) {
    const auto& lv = c.net->lv[level];
    p.n = c.nt(); p.h = lv.h; p.w = lv.w;
    p.group_n = c.net->n; p.gs = c.net->gs; p.in_gs = c.net->gs;
    p.tiles_x = (lv.w + kWgTileX - 1) / kWgTileX;
    p.tiles_y = (lv.h + kWgTileY - 1) / kWgTileY;
}

// ---- parameter fillers of the backward launches whose form the plan decides (plan_bwd asks the kernels' _ok predicates on what they return) ----
static WgradParams dense_wgrad_params(const Ctx& c, const DenseBlock& k, int j) {
    const auto& lv = c.net->lv[k.level];
    const BnP& b = k.bn[j];
    const ConvP& cv = k.cv[j];
    const int oc0 = k.ic0 + k.c0 + kGrowth * j;
    WgradParams p{};
    fill_wgrad_grid(c, p, k.level);
    p.in = c.act(k.level) + k.ic0 * lv.plane; p.in_ns = lv.t * lv.plane; p.in_cs = static_cast<int>(lv.plane); p.in_w = lv.w; p.cin = cv.cin;
    p.saved = c.saved(b); p.gamma = c.params + b.g; p.beta = c.params + b.b;
    p.dy = c.gbuf(k.level) + oc0 * lv.plane; p.dy_ns = lv.t * lv.plane; p.dy_cs = static_cast<int>(lv.plane); p.dy_w = lv.w; p.cout = cv.cout;
    p.dw = c.grads + cv.w;
    return p;
}

static void fill_dgrad_block(const Ctx& c, DgradBlockParams& p, int level) {
    const auto& lv = c.net->lv[level];
    p.n = c.nt(); p.h = lv.h; p.w = lv.w;
    p.group_n = c.net->n; p.gs = c.net->gs; p.slot_stride = c.net->slot_stride;
    p.g_ns = lv.t * lv.plane; p.g_cs = static_cast<int>(lv.plane); p.g_w = lv.w;
    p.ns = lv.t * lv.plane; p.cs = static_cast<int>(lv.plane);
}

// Gradient into the 12 new maps of layer j-1 of a dense block from ALL its consumers inside the block (layers j..3) in one pass.
// a: the same BN layers for the prep_dy that folds their finalize.  (vg / vw are the launch's to set: no predicate reads them.)
static DgradBlockParams newmap_params(const Ctx& c, const DenseBlock& k, int j, BnFin4* a = nullptr) {
    const auto& lv = c.net->lv[k.level];
    const int nl = kLayers - j;
    const int t0 = k.c0 + kGrowth * (j - 1);          // index of the target channels inside the consumers' inputs
    DgradBlockParams p{};
    fill_dgrad_block(c, p, k.level);
    p.g = c.gbuf(k.level) + (k.ic0 + k.c0 + kGrowth * j) * lv.plane;
    p.x = c.act(k.level) + (k.ic0 + t0) * lv.plane;
    p.out = c.gbuf(k.level) + (k.ic0 + t0) * lv.plane;
    p.count = kGrowth;
    p.acc_from = 0;          // a later consumer (next block / transition) wrote these maps first -- or nobody, where the final convolution's gradient is formed here
    p.w_ci_off = t0;
    for (int l = 0; l < nl; ++l) {
        const BnP& b = k.bn[j + l];
        p.wgt[l] = c.params + k.cv[j + l].w; p.w_cin[l] = k.cv[j + l].cin;
        p.saved[l] = c.saved(b) + 2 * t0; p.gamma[l] = c.params + b.g + t0; p.beta[l] = c.params + b.b + t0;
        p.scratch[l] = c.scratch(b) + 2 * t0;
        if (a) { a->scratch[l] = p.scratch[l]; a->saved[l] = p.saved[l]; a->gamma[l] = p.gamma[l]; a->ggamma[l] = c.grads + b.g + t0; a->gbeta[l] = c.grads + b.b + t0; }
    }
    return p;
}

// base channels of a dense block, all four layers in one pass
static DgradBlockParams base_pass_params(const Ctx& c, const DenseBlock& k) {
    const auto& lv = c.net->lv[k.level];
    DgradBlockParams p{};
    fill_dgrad_block(c, p, k.level);
    p.g = c.gbuf(k.level) + (k.ic0 + k.c0) * lv.plane;
    p.x = c.act(k.level) + k.ic0 * lv.plane;
    p.out = c.gbuf(k.level) + k.ic0 * lv.plane;
    p.count = k.c0;
    p.acc_from = k.base_overwrite ? k.c0 : 0;
    p.w_ci_off = 0;
    for (int j = 0; j < kLayers; ++j) {
        p.wgt[j] = c.params + k.cv[j].w; p.w_cin[j] = k.cv[j].cin;
        p.saved[j] = c.saved(k.bn[j]); p.gamma[j] = c.params + k.bn[j].g; p.beta[j] = c.params + k.bn[j].b;
        p.scratch[j] = c.scratch(k.bn[j]);
    }
    return p;
}

static WgradParams td_wgrad_params(const Ctx& c, int level) {
    const BnP& b = table().td_bn[level];
    const ConvP& cv = table().td_conv[level];
    const int next = level + 1, oc0 = next < kLevels ? 48 : 0;
    const auto& lv = c.net->lv[level];
    const auto& nx = c.net->lv[next];
    WgradParams p{};
    fill_wgrad_grid(c, p, level);
    p.in = c.act(level) + 48 * lv.plane; p.in_ns = lv.t * lv.plane; p.in_cs = static_cast<int>(lv.plane); p.in_w = lv.w; p.cin = cv.cin;
    p.saved = c.saved(b); p.gamma = c.params + b.g; p.beta = c.params + b.b;
    p.dy = c.gbuf(next) + oc0 * nx.plane; p.dy_ns = nx.t * nx.plane; p.dy_cs = static_cast<int>(nx.plane); p.dy_w = nx.w; p.cout = cv.cout;
    p.dy_idx = c.idx(level); p.idx_ns = static_cast<int64_t>(cv.cout) * nx.plane;
    p.dw = c.grads + cv.w;
    return p;
}

static ConvParams td_dgrad_params(const Ctx& c, int level) {
    const BnP& b = table().td_bn[level];
    const ConvP& cv = table().td_conv[level];
    const int next = level + 1, oc0 = next < kLevels ? 48 : 0;
    const auto& lv = c.net->lv[level];
    ConvParams p{};
    fill_grid(c, p, level);
    fill_in(c, p, c.gbuf(next), next, oc0, cv.cout);
    p.in_idx = c.idx(level); p.idx_ns = static_cast<int64_t>(cv.cout) * c.net->lv[next].plane;   // channel index relative to p.in
    p.wgt = c.params + cv.w; p.w_cout = cv.cout; p.w_cin = cv.cin;
    fill_out(c, p, c.gbuf(level), level, 48, cv.cin);
    p.x = c.act(level) + 48 * lv.plane; p.x_ns = lv.t * lv.plane; p.x_cs = static_cast<int>(lv.plane);
    p.bn_saved = c.saved(b); p.bn_gamma = c.params + b.g; p.bn_beta = c.params + b.b;
    p.bn_scratch = c.scratch(b); p.bn_slot_stride = c.net->slot_stride;
    p.acc_from = 0;
    return p;
}

// weight gradient of the transition up that wrote channels [0, 48) of `level`; subpix: as the sub-pixel form takes it (it walks the low-resolution grid)
static WgradParams tu_wgrad_params(const Ctx& c, int level, bool subpix) {
    const ConvP& cv = table().tu_conv[kLevels - 1 - level];
    const int src_level = level + 1, src_c0 = src_level == kLevels ? kBottIn : up_in(src_level);
    const auto& lv = c.net->lv[level];
    const auto& sv = c.net->lv[src_level];
    WgradParams p{};
    fill_wgrad_grid(c, p, level);
    p.in = c.act(src_level) + src_c0 * sv.plane; p.in_ns = sv.t * sv.plane; p.in_cs = static_cast<int>(sv.plane); p.in_w = sv.w; p.cin = cv.cin;
    p.dy = c.gbuf(level); p.dy_ns = lv.t * lv.plane; p.dy_cs = static_cast<int>(lv.plane); p.dy_w = lv.w; p.cout = cv.cout;
    p.dw = c.grads + cv.w;
    if (subpix) { p.h = sv.h; p.w = sv.w; }
    return p;
}

// first conv 3 -> 48: weight gradient (the image needs no data gradient)
static WgradParams first_wgrad_params(const Ctx& c) {
    const auto& lv = c.net->lv[0];
    WgradParams p{};
    fill_wgrad_grid(c, p, 0);
    p.in = c.x; p.in_ns = 3 * lv.plane; p.in_cs = static_cast<int>(lv.plane); p.in_w = lv.w; p.cin = 3;
    p.in_gs = c.net->n * p.in_ns;                 // the caller's image tensor
    p.dy = c.gbuf(0) + 48 * lv.plane; p.dy_ns = lv.t * lv.plane; p.dy_cs = static_cast<int>(lv.plane); p.dy_w = lv.w; p.cout = kFirst;
    p.dw = c.grads + table().first.w;
    return p;
}

static BwdPlan plan_bwd(const Ctx& c) {
    const int* opt = c.net->opt;
    const int wino_dgrad = opt[ENDO_OPT_WINO_DGRAD];
    const long min_tiles = opt[ENDO_OPT_WINO_MIN_TILES];
    BwdPlan pl{};
    pl.overlap = opt[ENDO_OPT_WGRAD_OVERLAP];
    pl.bf16_wgrad = (bf16_mask(opt) & 1) != 0;
    pl.bf16_dgrad = (bf16_mask(opt) & 4) != 0;
    // operands of a dense-layer weight gradient: rounded to bf16, else fp32 MFMA -- and only the latter has a Winograd-domain form
    const bool f34 = opt[ENDO_OPT_WGRAD_F34] && !pl.bf16_wgrad;
    const long fill = chip_divisor(c.net);
    const long f34_min_tiles = (min_tiles / 4 + fill - 1) / fill;          // from 256 tiles of 4 x 4 pixels: levels 0-4 of configs[1] (level 5 is 8 x 10)
    // the data-gradient weights are transformed whenever a Winograd form is selected, whether or not a block takes one this pass (at small sizes none does)
    pl.dgrad_weights = wino_dgrad != 0 && !pl.bf16_dgrad;
    for (int b = 0; b < kBlocks; ++b) {
        const DenseBlock k = dense_block(b);
        const auto& lv = c.net->lv[k.level];
        BwdPlan::Block& bl = pl.block[b];
        //   fine levels : per layer (last to first) prep + wgrad + a dgrad restricted to the NEW channels the layer
        //                 reads (they carry the layer-to-layer dependency); then ONE fused dgrad for the base channels
        //                 of all four layers (dgrad_block_kernels.h) -- 3x less HBM traffic than four full dgrads
        //   otherwise   : the per-layer path (few tiles: parallelism comes from splitting channels over blocks)
        const DgradBlockParams base = base_pass_params(c, k);
        bl.fused = dgrad_block_ok(base);
        // base pass at the fine levels: Winograd F(2x2, 3x3), 48 instead of 108 MFMAs per 64 pixels and step (dgrad_wino_kernels.h) -- the phase-skewed
        // kernel (ENDO_OPT_WINO_DGRAD 1 / 3, at most DgradWino3Geom::kMaxCount base channels), as persistent blocks where that form applies (3), else the round-2 kernel
        const long wtiles = static_cast<long>(lv.w / 32) * (lv.h / 8) * c.nt() * fill;
        if (pl.bf16_dgrad) bl.base = BasePass::Block8Bf16;
        else if (wino_dgrad != 0 && dgrad_wino_ok(base) && wtiles >= min_tiles)
            bl.base = !((wino_dgrad == 1 || wino_dgrad == 3) && dgrad_wino3_ok(base)) ? BasePass::Wino8
                    : (wino_dgrad == 3 && dgrad_wino3p_applies(base)) ? BasePass::Wino3Persistent : BasePass::Wino3;
        else bl.base = BasePass::Block8;          // 512-thread blocks: +15 % over the 4-wave kernel (tools/conv_bench)
        bl.wino3_layout = bl.base == BasePass::Wino3 || bl.base == BasePass::Wino3Persistent;
        for (int j = 1; j < kLayers; ++j) {
            const DgradBlockParams p = newmap_params(c, k, j);
            const bool vec = dgrad_block_vec_ok(p);          // 16-byte DMA of the gradient tiles
            bl.newmap[j] = (pl.bf16_dgrad && vec) ? NewMap::Bf16 : (vec && opt[ENDO_OPT_DGRAD_VEC] >= 2 && dgrad_newmap_ok(p)) ? NewMap::Persistent
                         : (vec && opt[ENDO_OPT_DGRAD_VEC] != 0) ? NewMap::Vec16 : NewMap::Dword;
        }
        for (int j = 0; j < kLayers; ++j) {
            const WgradParams p = dense_wgrad_params(c, k, j);
            pl.wgrad[b * kLayers + j] = (f34 && wgrad_f34_ok(p, f34_min_tiles)) ? DenseWgrad::F34 : wgrad_nsplit_ok(p, fill) ? DenseWgrad::NSplit
                                      : wgrad_taps_ok(p) ? DenseWgrad::Taps : DenseWgrad::Direct;
        }
    }
    for (int l = 0; l < kLevels; ++l) {
        const auto& sv = c.net->lv[l + 1];
        pl.td_wgrad_dma[l] = wgrad1x1_dma_ok(td_wgrad_params(c, l));
        // pooled rows of whole code dwords -> LDS-DMA kernel; otherwise the register-staged one
        // levels 0 / 1 of configs[1] (96 / 144 channels, whole 32 x 8 tiles): persistent blocks, weights LDS-resident, 16-byte DMA (td_dgrad_kernels.h)
        // pooled rows without whole code dwords (level 4 of configs[1]: 8 x 10): 128-pixel runs, the routed gradient expanded on its way into
        // LDS -- 46 instead of the register-staged kernel's 100 us.  (At levels 2 / 3 the LDS-DMA kernel stays: 103 / 63 against 139 / 69 us, tools/td_bench)
        const ConvParams td = td_dgrad_params(c, l);
        const bool persist = (opt[ENDO_OPT_TD_PERSIST] & 1) && !pl.bf16_dgrad;
        pl.td_dgrad[l] = (persist && td_dgrad_ok(td)) ? TdDgrad::Persistent : (persist && sv.w % 4 != 0 && td_dgrad_small_ok(td)) ? TdDgrad::Runs128
                       : sv.w % 4 == 0 ? TdDgrad::Dma : TdDgrad::Staged;
        const ConvP& tu = table().tu_conv[kLevels - 1 - l];
        pl.tu_wgrad[l] = tu_wgrad_subpix_ok(tu_wgrad_params(c, l, true)) ? TuWgrad::Subpix : wgrad_taps_ok(tu_wgrad_params(c, l, false), true) ? TuWgrad::Taps : TuWgrad::Direct;
        // Sub-pixel data gradient, tile shape by block count (round 6): on 32 x 8 tiles the launch of level 4 is 32 blocks and that of level 3 128 -- each walking all 24 K-chunks,
        // 93 and 103 us for 0.1 and 0.4 GFLOP.  16 x 8 / 16 x 4 tiles where 32 x 8 ones leave the chip under-filled.
        pl.tu_dgrad[l] = !(sv.w % 4 == 0 && tu.cin == kNew && tu.cout == kNew) ? TuDgrad::Plain : tile_count(c, l + 1, 32, 8) >= 1024 ? TuDgrad::Subpix32x8
                       : tile_count(c, l + 1, 16, 8) >= 512 ? TuDgrad::Subpix16x8 : TuDgrad::Subpix16x4;
    }
    // The final convolution's data gradient is rank one: dX[c] = g * w[c], g = grad_out * sign(pre).  Writing it out (192 planes, 1 GB
    // at 16 x 256 x 320) only for the last up block to read it back costs two passes over the level-0 buffer; instead g goes to one
    // plane and that block's kernels form the products where they first touch a channel (FinalVirt) -- where the block takes the
    // fused path, and for its base channels where the phase-skewed Winograd kernel runs; what is left is materialised as before.
    // ... and where that kernel runs as persistent blocks it also forms sum g * x[c] of the base channels it streams: the final
    // convolution's weight gradient of those channels (round 6: final_bwd_weight_kernel then reads 48 + 1 instead of 192 + 1 planes)
    const BwdPlan::Block& last = pl.block[kBlocks - 1];
    const int last_base = dense_block(kBlocks - 1).c0;
    pl.use_virt = opt[ENDO_OPT_FINAL_VIRTUAL] && last.fused;
    pl.virt_base = pl.use_virt && last.wino3_layout;
    pl.virt_base_w = pl.use_virt && last.base == BasePass::Wino3Persistent;
    pl.materialise = !pl.use_virt ? 192 : (pl.virt_base ? 0 : last_base);
    pl.c_first = pl.virt_base_w ? last_base : 0;
    // First convolution: the F(3x3, 4x4) form can prepare the gradient itself (G = d + P x + Q, bias gradient = sum G: WgradParams::prep_x): this is the LAST kernel
    // of the backward pass, nothing else is on the chip, and prep_dy's own pass over 3 x 48 planes would be 0.1 ms of the step
    const WgradParams first = first_wgrad_params(c);
    pl.first = (f34 && wgrad_f34_raw_ok(first, f34_min_tiles)) ? (opt[ENDO_OPT_FINAL_VIRTUAL] ? FirstWgrad::F34Prep : FirstWgrad::F34)
             : wgrad_taps_ok(first) ? FirstWgrad::Taps : FirstWgrad::Direct;
    return pl;
}

// ---- the weight-gradient launches by planned form.  endo_net_bwd and the weight-gradient bricks (endo_wgrad_brick, the end of this file) both go
// through these four functions: nothing else switches over the forms, so a brick launches what the network launches.  bf16: the network's
// ENDO_OPT_MFMA_BF16 operand rounding (the bricks are fp32-operand only) ----
// batch / slice: the F(3x3, 4x4) form leaves its partial sums in scratch slice `slice` and its reduction to the caller's batched launch
static int launch_dense_wgrad(DenseWgrad form, const WgradParams& p, float* scratch, hipStream_t stream, F34ReduceBatch* batch = nullptr, int slice = 0,
                              bool bf16 = false) {
    switch (form) {
        case DenseWgrad::F34: return launch_wgrad_f34(p, scratch + (batch ? slice : 0) * kF34ScratchFloats, stream, batch);          // Winograd F(3x3, 4x4)
        case DenseWgrad::NSplit: return launch_wgrad_nsplit(p, scratch, stream, bf16);
        case DenseWgrad::Taps: return bf16 ? launch_wgrad_taps<12, IN_BNRELU, 1>(p, stream) : launch_wgrad_taps<12, IN_BNRELU>(p, stream);
        case DenseWgrad::Direct: return launch_wgrad<3, 1, IN_BNRELU, DY_PLAIN>(p, stream);
    }
    return ENDO_E_BADARG;
}

// transition down, 1x1 on the un-routed pooled gradient: the LDS-DMA kernel where whole code dwords allow it (BwdPlan::td_wgrad_dma), else the plain one
static int launch_td_wgrad(bool dma, const WgradParams& p, hipStream_t stream, bool bf16 = false) {
    return !dma ? launch_wgrad1x1(p, stream) : bf16 ? launch_wgrad1x1_dma<1>(p, stream) : launch_wgrad1x1_dma<0>(p, stream);
}

// transition up; p as tu_wgrad_params(.., form == Subpix) fills it (the sub-pixel form walks the low-resolution grid)
static int launch_tu_wgrad(TuWgrad form, const WgradParams& p, float* scratch, hipStream_t stream) {
    switch (form) {
        case TuWgrad::Subpix: return launch_tu_wgrad_subpix(p, scratch, stream);
        case TuWgrad::Taps: return launch_wgrad_taps<12, IN_UPSAMPLE>(p, stream);
        case TuWgrad::Direct: return launch_wgrad<3, 1, IN_UPSAMPLE, DY_PLAIN>(p, stream);
    }
    return ENDO_E_BADARG;
}

// first convolution, 3 -> 48 channels: in the F(3x3, 4x4) form the four sets of 12 output channels share one launch (the tap-folded kernel runs a
// 108-row GEMM with 3 of 16 columns in use, four times: 216 us alone on the chip at the very end of the backward)
static int launch_first_wgrad(FirstWgrad form, const WgradParams& p, float* scratch, hipStream_t stream) {
    switch (form) {
        case FirstWgrad::F34Prep: return launch_wgrad_f34<0, true, true>(p, scratch, stream);
        case FirstWgrad::F34: return launch_wgrad_f34<0, true>(p, scratch, stream);
        case FirstWgrad::Taps: return launch_wgrad_taps<12, IN_PLAIN>(p, stream);
        case FirstWgrad::Direct: return launch_wgrad<3, 3, IN_PLAIN, DY_PLAIN>(p, stream);
    }
    return ENDO_E_BADARG;
}

static int dense_wgrad(const Ctx& c, int b, int j, F34ReduceBatch* batch = nullptr, int slice = 0) {
    const DenseBlock k = dense_block(b);
    const ConvP& cv = k.cv[j];
    const auto& lv = c.net->lv[k.level];
    const WgradParams p = dense_wgrad_params(c, k, j);
    float* scratch = c.gradws + c.net->wg_scratch_off;
    ProfScope prof(kProfWgradDense, c.stream, conv_flops(c.net, k.level, cv.cin, cv.cout, 3), 4.0 * c.nt() * lv.plane * (cv.cin + cv.cout));
    return launch_dense_wgrad(c.bwd->wgrad[b * kLayers + j], p, scratch, c.stream, batch, slice, c.bwd->bf16_wgrad);
}

// dense layer backward: bias grad + deferred-term fold, wgrad, dgrad fused with ReLU/BN backward
static int dense_bwd(const Ctx& c, int b, int j, int acc_from) {
    const DenseBlock k = dense_block(b);
    const BnP& bn = k.bn[j];
    const ConvP& cv = k.cv[j];
    const int level = k.level, ic0 = k.ic0, oc0 = k.ic0 + k.c0 + kGrowth * j;
    const auto& lv = c.net->lv[level];
    int rc = prep_dy(c, level, oc0, cv.cout, c.grads + cv.b);
    if (rc) return rc;
    {
        Ctx cw;
        rc = c.fork_wgrad(cw, level);
        if (rc) return rc;
        rc = dense_wgrad(cw, b, j);
        if (rc) return rc;
    }
    {
        ConvParams p{};
        fill_grid(c, p, level);
        fill_in(c, p, c.gbuf(level), level, oc0, cv.cout);
        p.wgt = c.params + cv.w; p.w_cout = cv.cout; p.w_cin = cv.cin;
        fill_out(c, p, c.gbuf(level), level, ic0, cv.cin);
        p.x = c.act(level) + ic0 * lv.plane; p.x_ns = lv.t * lv.plane; p.x_cs = static_cast<int>(lv.plane);
        p.bn_saved = c.saved(bn); p.bn_gamma = c.params + bn.g; p.bn_beta = c.params + bn.b;
        p.bn_scratch = c.scratch(bn); p.bn_slot_stride = c.net->slot_stride;
        p.acc_from = acc_from - ic0;
        ProfScope prof(kProfDgradDense, c.stream, conv_flops(c.net, level, cv.cin, cv.cout, 3), 4.0 * c.nt() * lv.plane * (3.0 * cv.cin + cv.cout));
        rc = launch_dgrad_dense_auto(p, c.stream);
        if (rc) return rc;
    }
    return bn_finalize(c, bn, level, ic0);
}

template <int NL>
static int launch_newmap(NewMap form, const DgradBlockParams& p, int cus, hipStream_t stream) {
    switch (form) {
        case NewMap::Bf16: return launch_dgrad_block<NL, 2, 3, 1, 0, 4, 1>(p, stream);
        case NewMap::Persistent: return launch_dgrad_newmap<NL>(p, cus, stream);          // dgrad_newmap_kernels.h
        case NewMap::Vec16: return launch_dgrad_block<NL, 2, 3, 1, 0, 4>(p, stream);
        case NewMap::Dword: return launch_dgrad_block<NL, 2, 3>(p, stream);
    }
    return ENDO_E_BADARG;
}

// Backward of a whole dense block (4 layers), fused path or per-layer path as planned (BwdPlan::Block); DenseBlock::base_overwrite: the base
// channels have no gradient yet (first writer) instead of accumulating.
// fv: the block's gradient-buffer range starts out as the final convolution's rank-one data gradient (the last up block, level 0), which
// is never written: the first touch of every channel forms it (FinalVirt)
static int dense_block_bwd(const Ctx& c, int b, const FinalVirt* fv = nullptr) {
    const DenseBlock k = dense_block(b);
    const BwdPlan::Block& bl = c.bwd->block[b];
    const int level = k.level, ic0 = k.ic0, c0 = k.c0, new0 = ic0 + c0;
    const auto& lv = c.net->lv[level];
    if (!bl.fused) {
        for (int j = kLayers - 1; j >= 0; --j) {
            const int acc_from = (j == kLayers - 1 && k.base_overwrite) ? new0 : 0;
            int rc = dense_bwd(c, b, j, acc_from < ic0 ? ic0 : acc_from);
            if (rc) return rc;
        }
        return 0;
    }
    BnFin4 pending{};          // BN layers whose sums over the next prepared maps the last new-channel pass produced (folded into prep_dy)
    int pending_nl = 0;
    F34ReduceBatch red{};      // the block's F(3x3, 4x4) weight gradients reduce their partial sums in ONE launch behind the last of them
    for (int j = kLayers - 1; j >= 0; --j) {
        // (with fv: layer 3's maps have no gradient in the buffer yet -- prep_dy is their first writer; the maps of layers 2..0 were
        // written, from the virtual content, by the new-channel passes below)
        // (round 5, in-job A/B: a separate one-block finalize launch in front of a prologue-free prep_dy makes this kernel family 0.15 ms per step
        // faster and the step none: 18.15 against 18.15 ms -- the 33 extra launches cost what the prologues did)
        int rc = prep_dy(c, level, new0 + kGrowth * j, kGrowth, c.grads + k.cv[j].b, &pending, pending_nl, (fv && j == kLayers - 1) ? fv : nullptr);
        if (rc) return rc;
        // ENDO_OPT_WGRAD_OVERLAP 1: fork after every prep_dy; 2: ONE fork per dense block, after its last prep_dy (nothing rewrites a
        // prepared G before the join, so the four weight gradients may start late; 55 -> 22 event record / wait pairs per backward pass)
        const bool defer = c.bwd->overlap == 2;
        if (!defer || j == 0) {
            Ctx cw;
            rc = c.fork_wgrad(cw, level);
            if (rc) return rc;
            for (int jj = defer ? kLayers - 1 : j; jj >= j; --jj) {
                rc = dense_wgrad(cw, b, jj, &red, jj);
                if (rc) return rc;
            }
            if (j == 0 && red.count > 0) {          // (the side stream runs its launches in order: all four are ahead of this one)
                ProfScope prof(kProfSmall, cw.stream, 0.0, 0.0);          // (not a convolution launch: kept out of the weight-gradient family's per-launch figures)
                rc = launch_wgrad_f34_reduce_batch(red, cw.stream);
                if (rc) return rc;
            }
        }
        if (j > 0) {
            // The layer-to-layer dependency only needs G_j..G_3 final, and this way every new map is read (x) and
            // read-modify-written (gradient) once instead of once per consumer -- 180 instead of 252 plane passes per block.
            const int nl = kLayers - j;
            BnFin4 a{};
            DgradBlockParams p = newmap_params(c, k, j, &a);
            if (fv) { p.vg = fv->vg; p.vw = fv->vw + ic0 + p.w_ci_off; }
            ProfScope prof(kProfDgradDense, c.stream, 2.0 * c.nt() * lv.plane * kGrowth * kGrowth * 9 * nl,
                           4.0 * c.nt() * lv.plane * (3.0 * kGrowth + kGrowth * nl));
            const int cus = bl.newmap[j] == NewMap::Persistent ? persistent_cus(c.net) : 0;
            rc = nl == 1 ? launch_newmap<1>(bl.newmap[j], p, cus, c.stream) : nl == 2 ? launch_newmap<2>(bl.newmap[j], p, cus, c.stream) : launch_newmap<3>(bl.newmap[j], p, cus, c.stream);
            if (rc) return rc;
            pending = a;          // consumed by the prep_dy of these 12 maps at the top of the next iteration
            pending_nl = nl;
        }
    }
    {
        DgradBlockParams p = base_pass_params(c, k);
        const bool virt = fv && c.bwd->virt_base;
        if (virt) { p.vg = fv->vg; p.vw = fv->vw + ic0; }
        ProfScope prof(kProfDgradDense, c.stream, 2.0 * c.nt() * lv.plane * c0 * kGrowth * 9 * kLayers,
                       4.0 * c.nt() * lv.plane * (3.0 * c0 + kGrowth * kLayers));
        // the layers' Winograd-domain weights, in the U layout the plan had endo_net_bwd transform them to (BwdPlan::Block::wino3_layout)
        const float* ub = c.gradws + c.net->wd_off;
        const float* const u[4] = {ub + k.cv[0].ud, ub + k.cv[1].ud, ub + k.cv[2].ud, ub + k.cv[3].ud};
        int rc = 0;
        switch (bl.base) {
            case BasePass::Block8Bf16: rc = launch_dgrad_block8<4, 1>(p, c.stream); break;
            case BasePass::Block8: rc = launch_dgrad_block8<4>(p, c.stream); break;
            case BasePass::Wino8: rc = launch_dgrad_wino8<4>(p, u, c.stream); break;
            case BasePass::Wino3: rc = run_dgrad_wino3_nl4(p, u, c.stream); break;
            case BasePass::Wino3Persistent: {
                // persistent blocks, one per CU; with virt_base_w they leave per-block partials of dW_final[ic0 .. ic0 + c0), added up here
                double* fwp = (virt && c.bwd->virt_base_w) ? reinterpret_cast<double*>(c.gradws + c.net->fw_parts_off) : nullptr;
                int used = 0;
                rc = run_dgrad_wino3p_nl4(p, u, std::min(persistent_cus(c.net), kFwPartBlocks), fwp, &used, c.stream);
                if (rc == 0 && fwp) {
                    final_w_reduce_kernel<<<c0, 64, 0, c.stream>>>(fwp, used, c0, fv->gw + ic0);
                    ENDO_LAUNCH_CHECK();
                }
                break;
            }
        }
        if (rc) return rc;
    }
    {
        BnFin4 a;
        for (int j = 0; j < kLayers; ++j) {
            a.scratch[j] = c.scratch(k.bn[j]); a.saved[j] = c.saved(k.bn[j]); a.gamma[j] = c.params + k.bn[j].g;
            a.ggamma[j] = c.grads + k.bn[j].g; a.gbeta[j] = c.grads + k.bn[j].b;
        }
        ProfScope prof(kProfSmall, c.stream, 0.0, 0.0);
        bn_bwd_finalize4_kernel<<<dim3((c0 + 127) / 128, c.net->groups), 128, 0, c.stream>>>(a, kLayers, c.pq_p(level) + ic0, c.pq_q(level) + ic0, c0,
                                                                         static_cast<double>(c.net->n) * lv.h * lv.w, c.training, c.net->gs,
                                                                         c.net->slot_stride);
        ENDO_LAUNCH_CHECK();
    }
    return 0;
}

static int td_bwd(const Ctx& c, int level) {
    const BnP& b = table().td_bn[level];
    const ConvP& cv = table().td_conv[level];
    const int next = level + 1;
    const auto& lv = c.net->lv[level];
    int rc = prep_dy(c, next, next < kLevels ? 48 : 0, cv.cout, c.grads + cv.b);
    if (rc) return rc;
    {
        const WgradParams p = td_wgrad_params(c, level);
        Ctx cw;
        rc = c.fork_wgrad(cw, level);
        if (rc) return rc;
        ProfScope prof(kProfWgradOther, cw.stream, conv_flops(c.net, level, cv.cin, cv.cout, 1), 4.0 * c.nt() * lv.plane * cv.cin);
        rc = launch_td_wgrad(c.bwd->td_wgrad_dma[level], p, cw.stream, c.bwd->bf16_wgrad);
        if (rc) return rc;
    }
    {
        const ConvParams p = td_dgrad_params(c, level);
        ProfScope prof(kProfDgradOther, c.stream, conv_flops(c.net, level, cv.cin, cv.cout, 1), 4.0 * c.nt() * lv.plane * 3.0 * cv.cin);
        switch (c.bwd->td_dgrad[level]) {
            case TdDgrad::Persistent: rc = launch_td_dgrad(p, persistent_cus(c.net), c.stream); break;
            case TdDgrad::Runs128: rc = launch_td_dgrad_small(p, c.stream); break;
            case TdDgrad::Dma: rc = c.bwd->bf16_dgrad ? launch_conv_dma_auto<1, 16, 2, IN_UNPOOL, EPI_DGRAD_BN, 4, 2, 1, 1>(p, c.stream)
                                                      : launch_conv_dma_auto<1, 16, 2, IN_UNPOOL, EPI_DGRAD_BN, 4>(p, c.stream); break;
            case TdDgrad::Staged: rc = launch_conv_auto<1, 16, 3, IN_UNPOOL, EPI_DGRAD_BN, 4>(p, c.stream); break;
        }
        if (rc) return rc;
    }
    return bn_finalize(c, b, level, 48);
}

static int tu_bwd(const Ctx& c, int level, int src_level, int src_c0, const ConvP& cv) {
    const auto& lv = c.net->lv[level];
    int rc = prep_dy(c, level, 0, cv.cout, c.grads + cv.b);
    if (rc) return rc;
    {
        const TuWgrad form = c.bwd->tu_wgrad[level];
        const WgradParams p = tu_wgrad_params(c, level, form == TuWgrad::Subpix);
        Ctx cw;
        rc = c.fork_wgrad(cw, level);
        if (rc) return rc;
        ProfScope prof(kProfWgradOther, cw.stream, conv_flops(c.net, level, cv.cin, cv.cout, 3), 4.0 * c.nt() * lv.plane * (cv.cin / 4.0 + cv.cout));
        rc = launch_tu_wgrad(form, p, c.gradws + c.net->wg_scratch_off, cw.stream);
        if (rc) return rc;
    }
    ProfScope prof(kProfDgradOther, c.stream, conv_flops(c.net, level, cv.cin, cv.cout, 3), 4.0 * c.nt() * lv.plane * (cv.cout + cv.cin / 4.0));
    const TuDgrad form = c.bwd->tu_dgrad[level];
    if (form == TuDgrad::Plain) {
        ConvParams p{};
        fill_grid(c, p, level);
        fill_in(c, p, c.gbuf(level), level, 0, cv.cout);
        p.wgt = c.params + cv.w; p.w_cout = cv.cout; p.w_cin = cv.cin;
        fill_out(c, p, c.gbuf(src_level), src_level, src_c0, cv.cin);
        return launch_conv_dma_auto<3, 4, 3, IN_PLAIN, EPI_DGRAD_SUMPOOL, 4>(p, c.stream);
    }
    // sub-pixel form on the low-resolution grid: the four stride-2 phases of dY, transformed at read time into 9 x 48 pseudo input
    // channels (1/4 of the MACs); the weights have their own scratch (the n-split scratch belongs to the side stream)
    float* wd = c.gradws + c.net->tuw_scratch_off;
    tu_subpix_dgrad_weights_kernel<<<(cv.cout * kTuW9 + 255) / 256, 256, 0, c.stream>>>(c.params + cv.w, cv.cout, cv.cin, wd);
    ENDO_LAUNCH_CHECK();
    ConvParams p{};
    fill_grid(c, p, src_level);
    fill_in(c, p, c.gbuf(level), level, 0, cv.cout);          // strides of the full-resolution gradient buffer
    p.wgt = wd; p.w_cout = cv.cin; p.w_cin = cv.cout;
    fill_out(c, p, c.gbuf(src_level), src_level, src_c0, cv.cin);
    if (form == TuDgrad::Subpix32x8) return launch_tu_dgrad_subpix<2, 4>(p, c.stream);
    if (form == TuDgrad::Subpix16x8) return launch_tu_dgrad_subpix<1, 2>(p, c.stream);
    return launch_tu_dgrad_subpix<1, 1>(p, c.stream);
}

static int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

}  // namespace endo

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int endo_net_create_grouped(endo_net** out, int n, int h, int w, int groups) {
    if (!out || n <= 0 || h <= 0 || w <= 0 || groups <= 0) return ENDO_E_BADARG;
    if (groups > kMaxGroups) return ENDO_E_UNSUPPORTED;
    if ((h % 32) != 0 || (w % 32) != 0) return ENDO_E_UNSUPPORTED;   // 5 poolings + exact centre crop (models.py:93-97)
    const Table& tb = table();
    endo_net* net = new (std::nothrow) endo_net();
    if (!net) return ENDO_E_BADARG;
    net->n = n; net->h = h; net->w = w; net->groups = groups;
    net->last_fwd = nullptr; net->last_bwd = nullptr;
    default_options(net->opt);
    int64_t off = 0, sums = 0, pq = 0;
    for (int l = 0; l <= kLevels; ++l) {
        auto& lv = net->lv[l];
        lv.h = h >> l; lv.w = w >> l; lv.t = level_channels(l);
        lv.plane = static_cast<int64_t>(lv.h) * lv.w;
        lv.act = off; lv.grad = off;
        off += align_up(static_cast<int64_t>(n) * lv.t * lv.plane, 64);
        lv.sums = sums; sums += 2 * lv.t;
        lv.pq = pq; pq += lv.t;
    }
    const int64_t acts = off;
    net->pre_off = off; off += align_up(static_cast<int64_t>(n) * h * w, 64);
    net->saved_off = off; off += align_up(2 * arch().bn_width, 64);
    int64_t byte_off = off * 4;
    for (int l = 0; l < kLevels; ++l) {
        net->idx_off[l] = byte_off;
        byte_off += align_up(static_cast<int64_t>(n) * (down_in(l) + kNew) * net->lv[l + 1].plane, 256);
    }
    net->sums_off = byte_off;
    net->sums_bytes = sums * 8;
    byte_off += align_up(net->sums_bytes, 256);
    net->partial_off = byte_off / 4;
    byte_off += static_cast<int64_t>(kGrowth) * 163840 * 4;     // bound: see dense_fwd
    net->wino_off = byte_off / 4;
    byte_off += align_up(tb.wino_floats * 4, 256);
    net->wino4_off = byte_off / 4;
    byte_off += align_up(tb.wino4_floats * 4, 256);
    net->tape_floats = byte_off / 4;
    net->pq_off = acts;
    net->pq_floats = 2 * pq;
    net->scratch_off = align_up((acts + net->pq_floats) * 4, 256);
    net->slot_stride = align_up(arch().bn_width * 2, 32);
    net->scratch_bytes = net->slot_stride * 8 * kBnSlots;
    net->wg_scratch_off = (net->scratch_off + align_up(net->scratch_bytes, 256)) / 4;
    net->tuw_scratch_off = net->wg_scratch_off + std::max(std::max(kNsScratchFloats, kSpScratchFloats), 4 * kF34ScratchFloats);          // four slices: the layers of a dense block reduce in one launch
    net->wd_off = align_up(net->tuw_scratch_off + kNew * kTuW9, 64);
    net->gplane_off = align_up(net->wd_off + tb.wino_dgrad_floats, 64);
    net->bias_parts_off = net->gplane_off + align_up(static_cast<int64_t>(n) * h * w, 64);
    net->bias_parts_floats = static_cast<int64_t>(kBiasPartChannels) * n * groups * 32;
    {   // the BiasParts limits against THIS network's table: one prep_dy launch per convolution with a bias, its output channels in all
        int launches = 0, channels = 0;
        for (const ConvDesc& m : arch().convs)
            if (m.role != Role::Final) { ++launches; channels += m.cout; }
        if (launches > kBiasPartLaunches || channels > kBiasPartChannels) { delete net; return ENDO_E_UNSUPPORTED; }
    }
    net->fw_parts_off = net->bias_parts_off + align_up(net->bias_parts_floats, 64);
    net->gradws_floats = net->fw_parts_off + 2 * static_cast<int64_t>(kFwPartBlocks) * kFinalIn;
    // one stride for both buffers keeps the kernels' group arithmetic to a single number; the caller allocates
    // groups * gs floats for each when groups > 1 (the two sizes differ by a few per cent)
    net->gs = align_up(net->tape_floats > net->gradws_floats ? net->tape_floats : net->gradws_floats, 64);
    *out = net;
    return 0;
}

extern "C" int endo_net_create(endo_net** out, int n, int h, int w) { return endo_net_create_grouped(out, n, h, w, 1); }

static bool option_id_ok(int id) { return id >= 0 && id < ENDO_OPT_COUNT && id != 6; }          // 6: retired (include/endo_hip.h)

extern "C" int endo_net_set_option(endo_net* net, int option_id, int value) {
    if (!net || !option_id_ok(option_id)) return ENDO_E_BADARG;
    const int old = net->opt[option_id];
    net->opt[option_id] = value;
    return old;
}

extern "C" int endo_net_get_option(const endo_net* net, int option_id) {
    if (!net || !option_id_ok(option_id)) return ENDO_E_BADARG;
    return net->opt[option_id];
}

extern "C" void endo_net_destroy(endo_net* net) {
    if (!net) return;
    net->side.destroy();
    delete net->last_fwd;
    delete net->last_bwd;
    delete net;
}
extern "C" int64_t endo_net_param_floats(void) { return arch().param_floats; }
extern "C" int64_t endo_net_bn_floats(void) { return arch().bn_floats; }
extern "C" int64_t endo_net_tape_floats(const endo_net* net) { return !net ? 0 : (net->groups > 1 ? net->groups * net->gs : net->tape_floats); }
extern "C" int64_t endo_net_gradws_floats(const endo_net* net) { return !net ? 0 : (net->groups > 1 ? net->groups * net->gs : net->gradws_floats); }
extern "C" int endo_net_groups(const endo_net* net) { return net ? net->groups : 0; }
extern "C" int64_t endo_net_group_stride(const endo_net* net) { return net ? net->gs : 0; }
extern "C" int64_t endo_net_param_offset(int index) {
    if (index < 0 || index >= static_cast<int>(arch().param_offsets.size())) return -1;
    return arch().param_offsets[index];
}
extern "C" int64_t endo_net_bn_offset(int bn_index, int which) {
    if (bn_index < 0 || bn_index >= static_cast<int>(arch().bns.size()) || which < 0 || which > 1) return -1;
    return arch().bns[bn_index].run + which * arch().bns[bn_index].c;
}
extern "C" int endo_net_level_channels(int level) { return (level < 0 || level > kLevels) ? -1 : level_channels(level); }
extern "C" int64_t endo_net_act_offset(const endo_net* net, int level) { return (!net || level < 0 || level > kLevels) ? -1 : net->lv[level].act; }

extern "C" int64_t endo_net_tape_offset(const endo_net* net, int what, int index) {
    if (!net) return -1;
    switch (what) {
        case ENDO_TAPE_PRE: return net->pre_off;
        case ENDO_TAPE_BN_SAVED:
            if (index < 0 || index >= static_cast<int>(arch().bns.size())) return -1;
            return net->saved_off + 2 * arch().bns[index].before;
        case ENDO_TAPE_POOL:
            if (index < 0 || index >= kLevels) return -1;
            return net->idx_off[index];
        default: return -1;
    }
}

extern "C" int endo_net_fwd(endo_net* net, const float* params, float* bn_running, const float* x, float* out, float* tape,
                            int training, void* stream_) {
    if (!net || !params || !bn_running || !x || !out || !tape) return ENDO_E_BADARG;
    const Table& tb = table();
    Ctx c{net, params, bn_running, tape, nullptr, nullptr, training, static_cast<hipStream_t>(stream_)};
    const FwdPlan plan = plan_fwd(c);
    c.fwd = &plan;
    if (!net->last_fwd) net->last_fwd = new (std::nothrow) FwdPlan;
    if (net->last_fwd) *net->last_fwd = plan;
    for (int g = 0; g < net->groups; ++g)
        ENDO_CHECK(hipMemsetAsync(reinterpret_cast<char*>(tape + g * net->gs) + net->sums_off, 0, net->sums_bytes, c.stream));
    if (!plan.bf16) {          // dense-layer weights in Winograd form or in the direct kernel's chunk order, as each layer's planned form reads them: all 44 layers in one launch
        ProfScope prof(kProfSmall, c.stream, 0.0, 4.0 * (tb.wino_floats + tb.wino_floats * 9 / 16));
        WinoWeightTable wt = tb.wino;
        for (int l = 0; l < wt.layers; ++l) wt.mode[l] = plan.dense[l].chunk_weights ? 1 : 0;
        wino_fwd_weights_kernel<<<(wt.start[wt.layers] + 255) / 256, 256, 0, c.stream>>>(wt, params, tape + net->wino_off);
        ENDO_LAUNCH_CHECK();
        if (plan.wino4_weights) wino4_fwd_weights_kernel<<<(tb.wino4.start[tb.wino4.layers] + 255) / 256, 256, 0, c.stream>>>(tb.wino4, params, tape + net->wino4_off);
        ENDO_LAUNCH_CHECK();
    }
    int rc;
    {   // first conv 3 -> 48 into level-0 channels [48, 96)
        ConvParams p{};
        fill_grid(c, p, 0);
        p.in = x; p.in_ns = 3 * net->lv[0].plane; p.in_cs = static_cast<int>(net->lv[0].plane); p.in_w = net->w; p.cin = 3;
        p.in_gs = net->n * p.in_ns;                 // x is the caller's [groups * n][3][H][W] tensor
        p.wgt = params + tb.first.w; p.bias = params + tb.first.b; p.w_cout = kFirst; p.w_cin = 3;
        fill_out(c, p, c.act(0), 0, 48, kFirst);
        p.out_sums = c.out_sums(0, 48);
        ProfScope prof(kProfConvFirst, c.stream, conv_flops(net, 0, 3, kFirst, 3), 4.0 * c.nt() * net->lv[0].plane * (3 + kFirst));
        rc = launch_conv_dma_auto<3, 4, 3, IN_PLAIN, EPI_FWD>(p, c.stream);
        if (rc) return rc;
    }
    for (int b = 0; b < kBlocks; ++b) {          // down path: block, transition down; bottleneck; up path: transition up, block
        if (b > kLevels) {
            const int i = b - kLevels - 1, l = kLevels - 1 - i;
            rc = tu_fwd(c, l, l + 1, (i == 0) ? kBottIn : up_in(l + 1), tb.tu_conv[i]);
            if (rc) return rc;
        }
        for (int j = 0; j < kLayers; ++j) {
            rc = dense_fwd(c, b, j);
            if (rc) return rc;
        }
        if (b < kLevels) {
            rc = td_fwd(c, b);
            if (rc) return rc;
        }
    }
    {
        const auto& lv = net->lv[0];
        const int c_first = plan.fuse_final ? up_in(0) + kGrowth * (kLayers - 1) : 0;          // 180: the last layer's launch has summed channels [0, 180) into `pre`
        ProfScope prof(kProfConvFinal, c.stream, 2.0 * c.nt() * lv.plane * kFinalIn, 4.0 * c.nt() * lv.plane * (kFinalIn + 2 - c_first));
        int bx = static_cast<int>((lv.plane / 4 + 255) / 256);
        bx = bx < 1 ? 1 : bx;
        final_fwd_kernel<<<dim3(bx, c.nt()), 256, 0, c.stream>>>(c.act(0), lv.t * lv.plane, static_cast<int>(lv.plane), kFinalIn,
                                                                 params + tb.final_.w, params + tb.final_.b, tape + net->pre_off, out,
                                                                 net->n, net->gs, c_first);
        ENDO_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int endo_net_bwd(endo_net* net, const float* params, const float* x, const float* tape, const float* grad_out,
                            float* grads, float* gradws, int training, void* stream_) {
    if (!net || !params || !x || !tape || !grad_out || !grads || !gradws) return ENDO_E_BADARG;
    const Table& tb = table();
    Ctx c{net, params, nullptr, const_cast<float*>(tape), grads, gradws, training, static_cast<hipStream_t>(stream_)};
    c.x = x;
    const BwdPlan plan = plan_bwd(c);
    c.bwd = &plan;
    if (!net->last_bwd) net->last_bwd = new (std::nothrow) BwdPlan;
    if (net->last_bwd) *net->last_bwd = plan;
    BiasParts bias_parts{};
    c.bias_parts = &bias_parts;
    ENDO_CHECK(net->side.create());          // side stream of the weight gradients (see endo_net), created on first use on the caller's device
    // zero the deferred-term tables and the BN reduction scratch
    for (int g = 0; g < net->groups; ++g)
        ENDO_CHECK(hipMemsetAsync(gradws + g * net->gs + net->pq_off, 0,
                                  static_cast<size_t>(net->scratch_off + net->scratch_bytes - net->pq_off * 4), c.stream));
    if (plan.dgrad_weights) {          // data-gradient weights of the dense layers in Winograd form, each block's in the U layout its planned base pass reads: one launch
        ProfScope prof(kProfSmall, c.stream, 0.0, 4.0 * 2.0 * tb.wino_dgrad_floats);
        int layout1_blocks = 0;
        for (int b = 0; b < kBlocks; ++b) layout1_blocks |= plan.block[b].wino3_layout ? 1 << b : 0;
        dgrad_wino_weights_kernel<<<(tb.wino_dgrad.start[tb.wino_dgrad.layers] + 255) / 256, 256, 0, c.stream>>>(tb.wino_dgrad, params, gradws + net->wd_off, layout1_blocks);
        ENDO_LAUNCH_CHECK();
    }
    auto body = [&]() -> int {          // everything that may fork the side stream: the join below is reached on every exit path (SideStream)
    int rc;
    const FinalVirt virt{gradws + net->gplane_off, params + tb.final_.w, grads + tb.final_.w};
    {   // final convolution (what the last up block forms itself: BwdPlan::use_virt)
        const auto& lv = net->lv[0];
        const int materialise = plan.materialise;
        {   // final conv weight / bias gradient: reads only grad_out and the tape, so it goes to the side stream first
            Ctx cw;
            rc = c.fork_wgrad(cw, 0);
            if (rc) return rc;
            const int c_first = plan.c_first;          // (the channels below it are the persistent base pass's)
            int by = static_cast<int>((lv.plane + 256 * 16 - 1) / (256 * 16));       // 16 pixels per thread
            by = by < 1 ? 1 : (by > 16 ? 16 : by);
            ProfScope prof(kProfConvFinal, cw.stream, 2.0 * c.nt() * lv.plane * (kFinalIn - c_first), 4.0 * c.nt() * lv.plane * (kFinalIn - c_first + 2));
            final_bwd_weight_kernel<<<dim3(kFinalIn - c_first + 1, by, c.nt()), 256, 0, cw.stream>>>(grad_out, tape + net->pre_off, c.act(0), lv.t * lv.plane,
                                                                         static_cast<int>(lv.plane), kFinalIn, net->n, net->gs, grads + tb.final_.w,
                                                                         grads + tb.final_.b, c_first);
            ENDO_LAUNCH_CHECK();
        }
        ProfScope prof(kProfConvFinal, c.stream, 2.0 * c.nt() * lv.plane * kFinalIn, 4.0 * c.nt() * lv.plane * (materialise + 2));
        if (plan.use_virt) {
            int bx = static_cast<int>((lv.plane + 1023) / 1024);
            final_g_kernel<<<dim3(bx, c.nt()), 256, 0, c.stream>>>(grad_out, tape + net->pre_off, gradws + net->gplane_off, static_cast<int>(lv.plane), net->n, net->gs);
            ENDO_LAUNCH_CHECK();
        }
        if (materialise > 0) {
            int bx = static_cast<int>((lv.plane + 255) / 256);
            final_bwd_data_kernel<<<dim3(bx, c.nt()), 256, 0, c.stream>>>(grad_out, tape + net->pre_off, params + tb.final_.w, c.gbuf(0),
                                                                          lv.t * lv.plane, static_cast<int>(lv.plane), materialise, net->n, net->gs, 0);
            ENDO_LAUNCH_CHECK();
        }
    }
    for (int b = kBlocks - 1; b >= 0; --b) {          // the forward pass's order, backwards
        if (b < kLevels) {
            rc = td_bwd(c, b);
            if (rc) return rc;
        }
        rc = dense_block_bwd(c, b, (b == kBlocks - 1 && plan.use_virt) ? &virt : nullptr);
        if (rc) return rc;
        if (b > kLevels) {
            const int i = b - kLevels - 1, l = kLevels - 1 - i;
            rc = tu_bwd(c, l, l + 1, (i == 0) ? kBottIn : up_in(l + 1), tb.tu_conv[i]);
            if (rc) return rc;
        }
    }
    {   // first conv: bias grad + weight grad (the image needs no gradient)
        WgradParams p = first_wgrad_params(c);
        const auto& lv = net->lv[0];
        if (plan.first == FirstWgrad::F34Prep) {
            p.prep_x = c.act(0) + 48 * lv.plane;
            p.prep_p = c.pq_p(0) + 48; p.prep_q = c.pq_q(0) + 48;
            p.prep_bias = grads + tb.first.b;
        } else {
            rc = prep_dy(c, 0, 48, kFirst, grads + tb.first.b);
            if (rc) return rc;
        }
        Ctx cw;
        rc = c.fork_wgrad(cw, 0);
        if (rc) return rc;
        ProfScope prof(kProfWgradOther, cw.stream, conv_flops(net, 0, 3, kFirst, 3), 4.0 * c.nt() * lv.plane * (3 + kFirst));
        rc = launch_first_wgrad(plan.first, p, gradws + net->wg_scratch_off, cw.stream);
        if (rc) return rc;
    }
    if (bias_parts.table.n > 0) {          // the conv-bias gradients from prep_dy's per-block sums (BiasParts): one launch for the whole pass
        ProfScope prof(kProfSmall, c.stream, 0.0, 4.0 * bias_parts.used);
        bias_reduce_kernel<<<dim3(bias_parts.table.n, 8), 256, 0, c.stream>>>(bias_parts.table);
        ENDO_LAUNCH_CHECK();
    }
    return 0;
    };
    const int rc_body = body();
    ENDO_CHECK(net->side.join_into(c.stream));          // the caller's stream continues only after every weight gradient has landed
    return rc_body;
}

// ---- the plan, readable (include/endo_hip.h: endo_net_last_plan / endo_net_plan_query / endo_net_plan_name) ----
namespace endo {

// One name table per ENDO_PLAN_* kind whose value is a choice of kernel form (enumerators in the order of the enum classes above; two-way choices
// are the plans' bools, false first); kinds with a null table carry a plain number.
struct PlanKind { const char* name; const char* const* values; int count; };
static const char* const kDenseFwdNames[] = {"Wino4", "Wino2_32x16", "Wino2_32x8", "SplitK", "Direct32x8", "Direct16x8", "DirectAuto"};
static const char* const kNewMapNames[] = {"Bf16", "Persistent", "Vec16", "Dword"};
static const char* const kBasePassNames[] = {"Block8", "Block8Bf16", "Wino3", "Wino3Persistent", "Wino8"};
static const char* const kDenseWgradNames[] = {"F34", "NSplit", "Taps", "Direct"};
static const char* const kTdDgradNames[] = {"Persistent", "Runs128", "Dma", "Staged"};
static const char* const kTuWgradNames[] = {"Subpix", "Taps", "Direct"};
static const char* const kTuDgradNames[] = {"Subpix32x8", "Subpix16x8", "Subpix16x4", "Plain"};
static const char* const kFirstWgradNames[] = {"F34Prep", "F34", "Taps", "Direct"};
static const char* const kTdFwdNames[] = {"PerTile", "Persistent"};
static const char* const kTuFwdNames[] = {"Upsample", "Subpix"};
static const char* const kBlockBwdNames[] = {"PerLayer", "Fused"};
static const char* const kTdWgradNames[] = {"Plain", "Dma"};
static_assert(static_cast<int>(DenseFwd::DirectAuto) == 6 && static_cast<int>(NewMap::Dword) == 3 && static_cast<int>(BasePass::Wino8) == 4 &&
              static_cast<int>(DenseWgrad::Direct) == 3 && static_cast<int>(TdDgrad::Staged) == 3 && static_cast<int>(TuWgrad::Direct) == 2 &&
              static_cast<int>(TuDgrad::Plain) == 3 && static_cast<int>(FirstWgrad::Direct) == 3, "the name tables follow the enums");
static const PlanKind kPlanKinds[ENDO_PLAN_KIND_COUNT] = {
    {"dense_fwd", kDenseFwdNames, 7}, {"dense_fwd_ksplit", nullptr, 0}, {"dense_fwd_chunk_weights", nullptr, 0}, {"fwd_bf16", nullptr, 0},
    {"wino4_weights", nullptr, 0}, {"fuse_final", nullptr, 0}, {"td_fwd", kTdFwdNames, 2}, {"tu_fwd", kTuFwdNames, 2},
    {"block_bwd", kBlockBwdNames, 2}, {"newmap", kNewMapNames, 4}, {"base_pass", kBasePassNames, 5}, {"wino3_layout", nullptr, 0},
    {"dense_wgrad", kDenseWgradNames, 4}, {"td_wgrad", kTdWgradNames, 2}, {"td_dgrad", kTdDgradNames, 4}, {"tu_wgrad", kTuWgradNames, 3},
    {"tu_dgrad", kTuDgradNames, 4}, {"wgrad_overlap", nullptr, 0}, {"bf16_wgrad", nullptr, 0}, {"bf16_dgrad", nullptr, 0},
    {"dgrad_weights", nullptr, 0}, {"use_virt", nullptr, 0}, {"virt_base", nullptr, 0}, {"virt_base_w", nullptr, 0},
    {"materialise", nullptr, 0}, {"c_first", nullptr, 0}, {"first_wgrad", kFirstWgradNames, 4},
};

// (kind, index, level, value) per field; writes only while the entries fit, always counts
struct PlanWriter {
    int32_t* out; int capacity; int count = 0;
    void put(int kind, int index, int level, int value) {
        if (count + 4 <= capacity) { out[count] = kind; out[count + 1] = index; out[count + 2] = level; out[count + 3] = value; }
        count += 4;
    }
};

static void write_plan(const FwdPlan& pl, PlanWriter& w) {
    for (int i = 0; i < kDense; ++i) {
        const int level = dense_block(i / kLayers).level;
        w.put(ENDO_PLAN_DENSE_FWD, i, level, static_cast<int>(pl.dense[i].form));
        w.put(ENDO_PLAN_DENSE_FWD_KSPLIT, i, level, pl.dense[i].ksplit);
        w.put(ENDO_PLAN_DENSE_FWD_CHUNK_WEIGHTS, i, level, pl.dense[i].chunk_weights);
    }
    w.put(ENDO_PLAN_FWD_BF16, 0, -1, pl.bf16);
    w.put(ENDO_PLAN_WINO4_WEIGHTS, 0, -1, pl.wino4_weights);
    w.put(ENDO_PLAN_FUSE_FINAL, 0, -1, pl.fuse_final);
    for (int l = 0; l < kLevels; ++l) {
        w.put(ENDO_PLAN_TD_FWD, l, l, pl.td_persistent[l]);
        w.put(ENDO_PLAN_TU_FWD, l, l, pl.tu_subpix[l]);
    }
}

static void write_plan(const BwdPlan& pl, PlanWriter& w) {
    for (int b = 0; b < kBlocks; ++b) {
        const int level = dense_block(b).level;
        const BwdPlan::Block& bl = pl.block[b];
        w.put(ENDO_PLAN_BLOCK_BWD, b, level, bl.fused);
        for (int j = 1; j < kLayers; ++j) w.put(ENDO_PLAN_NEWMAP, b * kLayers + j, level, static_cast<int>(bl.newmap[j]));
        w.put(ENDO_PLAN_BASE_PASS, b, level, static_cast<int>(bl.base));
        w.put(ENDO_PLAN_WINO3_LAYOUT, b, level, bl.wino3_layout);
    }
    for (int i = 0; i < kDense; ++i) w.put(ENDO_PLAN_DENSE_WGRAD, i, dense_block(i / kLayers).level, static_cast<int>(pl.wgrad[i]));
    for (int l = 0; l < kLevels; ++l) {
        w.put(ENDO_PLAN_TD_WGRAD, l, l, pl.td_wgrad_dma[l]);
        w.put(ENDO_PLAN_TD_DGRAD, l, l, static_cast<int>(pl.td_dgrad[l]));
        w.put(ENDO_PLAN_TU_WGRAD, l, l, static_cast<int>(pl.tu_wgrad[l]));
        w.put(ENDO_PLAN_TU_DGRAD, l, l, static_cast<int>(pl.tu_dgrad[l]));
    }
    w.put(ENDO_PLAN_WGRAD_OVERLAP, 0, -1, pl.overlap);
    w.put(ENDO_PLAN_BF16_WGRAD, 0, -1, pl.bf16_wgrad);
    w.put(ENDO_PLAN_BF16_DGRAD, 0, -1, pl.bf16_dgrad);
    w.put(ENDO_PLAN_DGRAD_WEIGHTS, 0, -1, pl.dgrad_weights);
    w.put(ENDO_PLAN_USE_VIRT, 0, -1, pl.use_virt);
    w.put(ENDO_PLAN_VIRT_BASE, 0, -1, pl.virt_base);
    w.put(ENDO_PLAN_VIRT_BASE_W, 0, -1, pl.virt_base_w);
    w.put(ENDO_PLAN_MATERIALISE, 0, -1, pl.materialise);
    w.put(ENDO_PLAN_C_FIRST, 0, -1, pl.c_first);
    w.put(ENDO_PLAN_FIRST_WGRAD, 0, 0, static_cast<int>(pl.first));
}

template <typename Plan>
static int serialise_plan(const Plan& pl, int32_t* out, int capacity) {
    PlanWriter w{out, capacity};
    write_plan(pl, w);
    return w.count <= capacity ? w.count : ENDO_E_BADARG;          // (a short buffer: part of the plan is in it, which the error says not to read)
}

}  // namespace endo

extern "C" int endo_net_last_plan(const endo_net* net, int pass, int32_t* out, int capacity) {
    if (!net || !out || capacity < 0) return ENDO_E_BADARG;
    if (pass == ENDO_PASS_FWD) return net->last_fwd ? serialise_plan(*net->last_fwd, out, capacity) : ENDO_E_BADARG;
    if (pass == ENDO_PASS_BWD) return net->last_bwd ? serialise_plan(*net->last_bwd, out, capacity) : ENDO_E_BADARG;
    return ENDO_E_BADARG;
}

extern "C" int endo_net_plan_query(const endo_net* net, int pass, int training, const float* params, float* bn_running, const float* x,
                                   float* tape, float* grads, float* gradws, int32_t* out, int capacity) {
    if (!net || !out || capacity < 0 || !params || !tape) return ENDO_E_BADARG;
    if (pass == ENDO_PASS_FWD) {          // the Ctx of endo_net_fwd
        if (!bn_running) return ENDO_E_BADARG;
        const Ctx c{net, params, bn_running, tape, nullptr, nullptr, training, nullptr};
        return serialise_plan(plan_fwd(c), out, capacity);
    }
    if (pass == ENDO_PASS_BWD) {          // the Ctx of endo_net_bwd
        if (!x || !grads || !gradws) return ENDO_E_BADARG;
        Ctx c{net, params, nullptr, tape, grads, gradws, training, nullptr};
        c.x = x;
        return serialise_plan(plan_bwd(c), out, capacity);
    }
    return ENDO_E_BADARG;
}

extern "C" const char* endo_net_plan_name(int kind, int value) {
    if (kind < 0 || kind >= ENDO_PLAN_KIND_COUNT) return nullptr;
    const PlanKind& k = kPlanKinds[kind];
    if (value == -1) return k.name;
    return (k.values && value >= 0 && value < k.count) ? k.values[value] : nullptr;
}

// ---- WEIGHT-GRADIENT BRICKS of the fp32 family (include/endo_hip.h): one weight-gradient launch of endo_net_bwd on the caller's operands ----
namespace {

int brick_forms(int kind) { return kind == ENDO_WGRAD_DENSE || kind == ENDO_WGRAD_FIRST ? 4 : kind == ENDO_WGRAD_TD ? 2 : kind == ENDO_WGRAD_TU ? 3 : 0; }
bool brick_form_ok(int kind, int form) { return form >= 0 && form < brick_forms(kind); }

// the WgradParams the network's fillers (dense_wgrad_params, first_wgrad_params, td_wgrad_params, tu_wgrad_params) would hand the launch
WgradParams brick_params(int kind, int form, const endo_wgrad_operands& a) {
    WgradParams p{};
    p.n = a.n; p.h = a.h; p.w = a.w;
    p.group_n = a.group_n > 0 ? a.group_n : a.n; p.gs = a.gs; p.in_gs = a.in_gs;
    p.tiles_x = (a.w + kWgTileX - 1) / kWgTileX;
    p.tiles_y = (a.h + kWgTileY - 1) / kWgTileY;
    p.in = a.in; p.in_ns = a.in_ns; p.in_cs = a.in_cs; p.in_w = a.in_w; p.cin = a.cin;
    p.dy = a.dy; p.dy_ns = a.dy_ns; p.dy_cs = a.dy_cs; p.dy_w = a.dy_w; p.cout = a.cout;
    p.dw = a.dw;
    if (kind == ENDO_WGRAD_DENSE || kind == ENDO_WGRAD_TD) { p.saved = a.saved; p.gamma = a.gamma; p.beta = a.beta; }
    if (kind == ENDO_WGRAD_TD) { p.dy_idx = a.dy_idx; p.idx_ns = a.idx_ns; }
    if (kind == ENDO_WGRAD_FIRST && static_cast<FirstWgrad>(form) == FirstWgrad::F34Prep) {
        p.prep_x = a.prep_x; p.prep_p = a.prep_p; p.prep_q = a.prep_q; p.prep_bias = a.prep_bias;
    }
    if (kind == ENDO_WGRAD_TU && static_cast<TuWgrad>(form) == TuWgrad::Subpix) { p.h = a.h / 2; p.w = a.w / 2; }          // the low-resolution grid
    return p;
}

// sizes, strides and the pointers every form of the kind reads (what no kernel predicate looks at)
bool brick_operands_ok(int kind, int form, const endo_wgrad_operands& a) {
    if (!a.in || !a.dy || !a.dw || a.n <= 0 || a.h <= 0 || a.w <= 0 || a.cin <= 0 || a.cout <= 0 || a.group_n < 0) return false;
    const bool half_in = kind == ENDO_WGRAD_TU, half_dy = kind == ENDO_WGRAD_TD;
    if ((half_in || half_dy) && (a.h % 2 != 0 || a.w % 2 != 0)) return false;
    const int64_t in_h = half_in ? a.h / 2 : a.h, in_w = half_in ? a.w / 2 : a.w, dy_h = half_dy ? a.h / 2 : a.h, dy_w = half_dy ? a.w / 2 : a.w;
    if (a.in_w < in_w || a.in_cs < in_h * a.in_w || a.in_ns < static_cast<int64_t>(a.cin) * a.in_cs) return false;
    if (a.dy_w < dy_w || a.dy_cs < dy_h * a.dy_w || a.dy_ns < static_cast<int64_t>(a.cout) * a.dy_cs) return false;
    const int group_n = a.group_n > 0 ? a.group_n : a.n;
    if (a.n % group_n != 0 || a.n / group_n > kMaxGroups) return false;
    if (a.n / group_n > 1 && (a.gs < group_n * a.dy_ns || a.in_gs < group_n * a.in_ns)) return false;
    if (kind == ENDO_WGRAD_DENSE && a.cout != kGrowth) return false;
    if (kind == ENDO_WGRAD_FIRST && (a.cin > 16 || a.cout % 12 != 0 || a.cout / 12 > 16)) return false;
    if ((kind == ENDO_WGRAD_DENSE || kind == ENDO_WGRAD_TD) && (!a.saved || !a.gamma || !a.beta)) return false;
    if (kind == ENDO_WGRAD_TD && (!a.dy_idx || a.idx_ns < static_cast<int64_t>(a.cout) * a.dy_cs)) return false;
    if (kind == ENDO_WGRAD_FIRST && static_cast<FirstWgrad>(form) == FirstWgrad::F34Prep && (!a.prep_x || !a.prep_p || !a.prep_q)) return false;
    return true;
}

// the form's own predicate, as plan_bwd asks it, without the tile / chunk minimum (a brick launches the form at any size)
bool brick_predicate(int kind, int form, const WgradParams& p) {
    switch (kind) {
        case ENDO_WGRAD_DENSE:
            switch (static_cast<DenseWgrad>(form)) {
                case DenseWgrad::F34: return wgrad_f34_ok(p, 0);
                case DenseWgrad::NSplit: return wgrad_nsplit_shape_ok(p);
                case DenseWgrad::Taps: return wgrad_taps_ok(p);
                case DenseWgrad::Direct: return true;
            }
            return false;
        case ENDO_WGRAD_FIRST:
            switch (static_cast<FirstWgrad>(form)) {
                case FirstWgrad::F34Prep:
                case FirstWgrad::F34: return wgrad_f34_raw_ok(p, 0);
                case FirstWgrad::Taps: return wgrad_taps_ok(p);
                case FirstWgrad::Direct: return true;
            }
            return false;
        case ENDO_WGRAD_TD: return form == 0 || wgrad1x1_dma_ok(p);
        case ENDO_WGRAD_TU:
            switch (static_cast<TuWgrad>(form)) {
                case TuWgrad::Subpix: return tu_wgrad_subpix_ok(p);
                case TuWgrad::Taps: return wgrad_taps_ok(p, true);
                case TuWgrad::Direct: return true;
            }
            return false;
    }
    return false;
}

}  // namespace

extern "C" int64_t endo_wgrad_brick_scratch_floats(int kind, int form) {
    if (!brick_form_ok(kind, form)) return ENDO_E_BADARG;
    if (kind == ENDO_WGRAD_DENSE) return static_cast<DenseWgrad>(form) == DenseWgrad::F34 ? kF34ScratchFloats : static_cast<DenseWgrad>(form) == DenseWgrad::NSplit ? kNsScratchFloats : 0;
    if (kind == ENDO_WGRAD_FIRST) return static_cast<FirstWgrad>(form) == FirstWgrad::F34Prep || static_cast<FirstWgrad>(form) == FirstWgrad::F34 ? kF34ScratchFloats : 0;
    if (kind == ENDO_WGRAD_TU) return static_cast<TuWgrad>(form) == TuWgrad::Subpix ? kSpScratchFloats : 0;
    return 0;
}

extern "C" int endo_wgrad_brick_ok(int kind, int form, const endo_wgrad_operands* a) {
    if (!a || !brick_form_ok(kind, form) || !brick_operands_ok(kind, form, *a)) return 0;
    return brick_predicate(kind, form, brick_params(kind, form, *a)) ? 1 : 0;
}

extern "C" int endo_wgrad_brick(int kind, int form, const endo_wgrad_operands* a, float* scratch, int64_t scratch_cap, void* stream) {
    if (!endo_wgrad_brick_ok(kind, form, a)) return ENDO_E_BADARG;
    const int64_t need = endo_wgrad_brick_scratch_floats(kind, form);
    if (need > 0 && (!scratch || scratch_cap < need)) return ENDO_E_BADARG;
    const WgradParams p = brick_params(kind, form, *a);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (kind) {
        case ENDO_WGRAD_DENSE: return launch_dense_wgrad(static_cast<DenseWgrad>(form), p, scratch, s);
        case ENDO_WGRAD_FIRST: return launch_first_wgrad(static_cast<FirstWgrad>(form), p, scratch, s);
        case ENDO_WGRAD_TD: return launch_td_wgrad(form != 0, p, s);
        case ENDO_WGRAD_TU: return launch_tu_wgrad(static_cast<TuWgrad>(form), p, scratch, s);
    }
    return ENDO_E_BADARG;
}

extern "C" int endo_wgrad_brick_f34_batch(const endo_wgrad_operands* layers, int count, float* scratch, int64_t scratch_cap, void* stream) {
    const int f34 = static_cast<int>(DenseWgrad::F34);
    if (!layers || count < 1 || count > 4 || !scratch || scratch_cap < count * kF34ScratchFloats) return ENDO_E_BADARG;
    for (int k = 0; k < count; ++k)
        if (!endo_wgrad_brick_ok(ENDO_WGRAD_DENSE, f34, layers + k)) return ENDO_E_BADARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    F34ReduceBatch red{};
    for (int k = 0; k < count; ++k) {
        const int rc = launch_dense_wgrad(DenseWgrad::F34, brick_params(ENDO_WGRAD_DENSE, f34, layers[k]), scratch, s, &red, k);
        if (rc) return rc;
    }
    return launch_wgrad_f34_reduce_batch(red, s);
}
