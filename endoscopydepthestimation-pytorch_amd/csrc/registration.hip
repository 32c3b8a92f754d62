// Similarity registration of a predicted point cloud to a model by iterative closest point: the per-point work of the step the reference
// leaves to another tool -- README step 4: after evaluate.py, "apply a registration algorithm that is able to estimate a similarity
// transformation to register the predicted point clouds to the corresponding CT model to calculate residual errors".  There is no
// reference code for it; tests/registration_restate.py is the numpy fp64 statement the device results are held to.
//
//   prepare  once per target: each row minus the centre (fp64), rounded to fp32, stored as the search's A operand
//            (-2 t_x, -2 t_y, -2 t_z, |t|^2), padded to a multiple of kTargetTile rows with (0, 0, 0, +inf), which a strict comparison
//            against a running minimum that starts at +inf never takes
//   match    one ICP iteration: block = kSourceTile source rows against every target row.  A source row is moved by the fp64 transform,
//            taken relative to the target centre and rounded to fp32: x.  The score |t|^2 - 2 x.t orders the targets as the distance
//            does and is one v_mfma_f32_16x16x4_f32 per 16 targets x 16 sources: A = the prepared rows, B = (x_x, x_y, x_z, 1), C = 0
//            (bit for bit the fmaf chain over k = 0..3, so well defined).  Targets sit on the rows, sources on the columns: a lane
//            receives four target rows of ONE source per instruction.  Keeping (score, index) per result would cost three or more vector
//            instructions per result on the lanes the matrix instruction itself runs on, more than the product, so the
//            scan keeps less: the minimum over the 16 results of kStepsPerUpdate instructions (v_minimum3_f32, half an instruction per
//            result), compared strictly against the running minimum, and WHICH update took it -- updates come in increasing index, so
//            the first of equal minima stays.  At the end each lane forms the 16 scores of its winning update again with the same fmaf
//            chain from the prepared rows, takes the first lowest, and the four lane groups of a column are combined once on
//            (score, index), lexicographically: of equal scores the lowest index wins.  Exact brute force: every pair is scored; there
//            is no spatial grid (that needs a device sort).  v_minimum3_f32 hands a NaN on: a target row whose score
//            is NaN (coordinates that are not finite, or whose squares overflow float32) hides its update's other rows too.
//            The winner's distance is then formed again in fp64 by direct differences between the moved point (not rounded) and the
//            caller's ORIGINAL target row, so the cancellation in the score only decides between nearly equidistant targets.
//            The 20 sums over the rows with d <= cap go through per-block partials in the workspace, added by one block in a fixed
//            order: no floating-point atomics, the same bytes on every call.
//   apply    rows moved by an fp64 transform, the columns behind z copied
// Built with -mllvm -amdgpu-mfma-vgpr-form: the matrix instruction's results land in ordinary vector registers, where v_minimum3_f32
// reads them; without it the compiler puts them in accumulation registers and copies each result out first (5 % of the match's time).
#include <cmath>

#include "common.h"

namespace endo {

constexpr int kRegThreads = 256;
constexpr int kRegWaves = kRegThreads / kWave;
constexpr int kSourceTile = kRegWaves * 16;                        // source rows per block: one 16-source B operand per wave
constexpr int kStepsPerUpdate = 4;                                 // 16-row matrix instructions per update of the running minimum
constexpr int kTargetTile = 1024;                                  // target rows per LDS stage (ENDO_REGISTRATION_TARGET_TILE)
constexpr int kStageLoads = kTargetTile / kRegThreads;             // float4 per thread and stage
constexpr int kSums = 20;
constexpr int64_t kPreparedHeader = 256;                           // bytes: the centre (3 doubles) ahead of the rows

static_assert(kSourceTile == ENDO_REGISTRATION_SOURCE_TILE && kTargetTile == ENDO_REGISTRATION_TARGET_TILE, "header and kernel disagree");
static_assert(kSourceTile <= kRegThreads && kTargetTile % kRegThreads == 0 && kTargetTile % (16 * kStepsPerUpdate) == 0, "tile geometry");

struct Similarity {
    double scale, r[9], t[3];
};

__device__ __forceinline__ double moved_coordinate(const Similarity& q, int i, double x, double y, double z) {
    return q.scale * (q.r[3 * i] * x + q.r[3 * i + 1] * y + q.r[3 * i + 2] * z) + q.t[i];
}

__global__ void __launch_bounds__(kRegThreads) registration_prepare_kernel(const float* __restrict__ target, int64_t stride, int64_t k,
                                                                           int64_t padded, double cx, double cy, double cz,
                                                                           char* __restrict__ prepared) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kRegThreads + threadIdx.x;
    if (i < kPreparedHeader / 8)          // the whole header: the centre, then zeros
        reinterpret_cast<double*>(prepared)[i] = i == 0 ? cx : (i == 1 ? cy : (i == 2 ? cz : 0.0));
    if (i >= padded) return;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, INFINITY);
    if (i < k) {
        const float* row = target + i * stride;
        const float x = static_cast<float>(static_cast<double>(row[0]) - cx);
        const float y = static_cast<float>(static_cast<double>(row[1]) - cy);
        const float z = static_cast<float>(static_cast<double>(row[2]) - cz);
        v = make_float4(-2.0f * x, -2.0f * y, -2.0f * z, fmaf(z, z, fmaf(y, y, x * x)));
    }
    reinterpret_cast<float4*>(prepared + kPreparedHeader)[i] = v;
}

struct MatchParams {
    const float* source;
    int64_t source_stride;
    int m;
    Similarity q;
    const char* prepared;
    const float* target;
    int64_t target_stride;
    int64_t padded;          // prepared rows, a multiple of kTargetTile
    double sx, sy, sz;       // source centre
    double cap;
    int* index;
    float* distance;
    double* partials;        // [blocks][kSums]
};

__global__ void __launch_bounds__(kRegThreads) registration_match_kernel(const MatchParams p) {
    __shared__ f32x4_acc s_tile[kTargetTile];          // (the native vector type: a float4 array stays in scratch memory)
    __shared__ int s_best[kSourceTile];
    __shared__ double s_part[kRegWaves][kSums];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int comp = lane >> 4;          // k of the operands: x, y, z, 1
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kSourceTile;
    const double* centre = reinterpret_cast<const double*>(p.prepared);
    const double cx = centre[0], cy = centre[1], cz = centre[2];
    const f32x4_acc* rows = reinterpret_cast<const f32x4_acc*>(p.prepared + kPreparedHeader);

    // B operand: component `comp` of this lane's source; a row past m searches from the origin and is dropped below
    float b = comp == 3 ? 1.0f : 0.0f;
    {
        const int64_t row = row0 + wave * 16 + (lane & 15);
        if (row < p.m && comp < 3) {
            const float* s = p.source + row * p.source_stride;
            const double c = comp == 0 ? cx : (comp == 1 ? cy : cz);
            b = static_cast<float>(moved_coordinate(p.q, comp, s[0], s[1], s[2]) - c);
        }
    }

    float best = INFINITY;
    int update = 0;          // the update (16 * kStepsPerUpdate target rows) that holds the running minimum

    const float* lds = reinterpret_cast<const float*>(s_tile);
    f32x4_acc stage[kStageLoads];
#pragma unroll
    for (int j = 0; j < kStageLoads; ++j) stage[j] = rows[j * kRegThreads + tid];
    for (int64_t base = 0; base < p.padded; base += kTargetTile) {
        __syncthreads();          // the previous stage has been read
#pragma unroll
        for (int j = 0; j < kStageLoads; ++j) s_tile[j * kRegThreads + tid] = stage[j];
        __syncthreads();
        const int64_t next = base + kTargetTile < p.padded ? base + kTargetTile : base;          // (the last stage again: not used)
#pragma unroll
        for (int j = 0; j < kStageLoads; ++j) stage[j] = rows[next + j * kRegThreads + tid];
        const int update0 = static_cast<int>(base / (16 * kStepsPerUpdate));
#pragma unroll 2
        for (int s = 0; s < kTargetTile / 16; s += kStepsPerUpdate) {
            float a[kStepsPerUpdate];
#pragma unroll
            for (int u = 0; u < kStepsPerUpdate; ++u) a[u] = lds[((s + u) * 16 + (lane & 15)) * 4 + comp];          // bank 4 (lane & 15) + comp
            float mn = 0.0f;
#pragma unroll
            for (int u = 0; u < kStepsPerUpdate; ++u) {
                const f32x4_acc d = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b, f32x4_acc{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
                const float m2 = u == 0 ? __builtin_elementwise_minimum(d[0], d[1])
                                        : __builtin_elementwise_minimum(__builtin_elementwise_minimum(mn, d[0]), d[1]);
                mn = __builtin_elementwise_minimum(__builtin_elementwise_minimum(m2, d[2]), d[3]);
            }
            const bool take = mn < best;
            best = take ? mn : best;
            update = take ? update0 + s / kStepsPerUpdate : update;
        }
    }

    // the winning update's scores again, in increasing index: row = (update * kStepsPerUpdate + u) * 16 + 4 * (lane >> 4) + register
    {
        float xs[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) xs[c] = __shfl(b, (lane & 15) + 16 * c, kWave);
        float sc = INFINITY;
        int idx = update * kStepsPerUpdate * 16 + comp * 4;
#pragma unroll
        for (int u = 0; u < kStepsPerUpdate; ++u) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int cand = (update * kStepsPerUpdate + u) * 16 + comp * 4 + r;
                const f32x4_acc t = rows[cand];
                const float score = fmaf(t[3], 1.0f, fmaf(t[2], xs[2], fmaf(t[1], xs[1], t[0] * xs[0])));
                const bool take = score < sc;
                sc = take ? score : sc;
                idx = take ? cand : idx;
            }
        }
        // the column's four lane groups, lowest (score, index) first
#pragma unroll
        for (int off = 16; off < 64; off <<= 1) {
            const float osc = __shfl_xor(sc, off, kWave);
            const int oidx = __shfl_xor(idx, off, kWave);
            const bool take = osc < sc || (osc == sc && oidx < idx);
            sc = take ? osc : sc;
            idx = take ? oidx : idx;
        }
        if (lane < 16) s_best[wave * 16 + lane] = idx;
    }
    __syncthreads();

    // one thread per source row: the exact distance to the winner and the row's terms of the sums
    double v[kSums];
#pragma unroll
    for (int j = 0; j < kSums; ++j) v[j] = 0.0;
    const int64_t row = row0 + tid;
    if (tid < kSourceTile && row < p.m) {
        const float* s = p.source + row * p.source_stride;
        const double x = s[0], y = s[1], z = s[2];
        const int idx = s_best[tid];
        const float* t = p.target + static_cast<int64_t>(idx) * p.target_stride;
        const double tx = t[0], ty = t[1], tz = t[2];
        const double dx = moved_coordinate(p.q, 0, x, y, z) - tx;
        const double dy = moved_coordinate(p.q, 1, x, y, z) - ty;
        const double dz = moved_coordinate(p.q, 2, x, y, z) - tz;
        const double d2 = dx * dx + dy * dy + dz * dz;
        const double d = sqrt(d2);
        p.index[row] = idx;
        p.distance[row] = static_cast<float>(d);
        if (d <= p.cap) {
            const double sv[3] = {x - p.sx, y - p.sy, z - p.sz};
            const double tv[3] = {tx - cx, ty - cy, tz - cz};
            v[0] = 1.0; v[1] = d; v[2] = d2; v[3] = d;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                v[4 + i] = sv[i];
                v[7 + i] = tv[i];
#pragma unroll
                for (int j = 0; j < 3; ++j) v[11 + 3 * i + j] = tv[i] * sv[j];
            }
            v[10] = sv[0] * sv[0] + sv[1] * sv[1] + sv[2] * sv[2];
        }
    }
#pragma unroll
    for (int j = 0; j < kSums; ++j) {
        double w = v[j];
        if (j == 3) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) w = fmax(w, __shfl_down(w, off, kWave));
        } else {
            w = wave_sum(w);
        }
        if (lane == 0) s_part[wave][j] = w;
    }
    __syncthreads();
    if (tid < kSums) {
        double w = s_part[0][tid];
        for (int i = 1; i < kRegWaves; ++i) w = tid == 3 ? fmax(w, s_part[i][tid]) : w + s_part[i][tid];
        p.partials[static_cast<int64_t>(blockIdx.x) * kSums + tid] = w;
    }
}

// the blocks' partials in a fixed order: lane l of the sum's wave takes blocks l, l + 64, ..., then the wave's tree
__global__ void __launch_bounds__(kRegThreads) registration_sums_kernel(const double* __restrict__ partials, int64_t blocks,
                                                                        double* __restrict__ sums) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = wave; j < kSums; j += kRegWaves) {
        double w = 0.0;
        if (j == 3) {
            for (int64_t i = lane; i < blocks; i += kWave) w = fmax(w, partials[i * kSums + j]);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) w = fmax(w, __shfl_down(w, off, kWave));
        } else {
            for (int64_t i = lane; i < blocks; i += kWave) w += partials[i * kSums + j];
            w = wave_sum(w);
        }
        if (lane == 0) sums[j] = w;
    }
}

__global__ void __launch_bounds__(kRegThreads) similarity_apply_kernel(const float* __restrict__ rows, int64_t stride, int64_t m,
                                                                       const Similarity q, float* __restrict__ out) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kRegThreads + threadIdx.x;
    if (i >= m) return;
    const float* s = rows + i * stride;
    float* o = out + i * stride;
    const double x = s[0], y = s[1], z = s[2];
    const float ox = static_cast<float>(moved_coordinate(q, 0, x, y, z));
    const float oy = static_cast<float>(moved_coordinate(q, 1, x, y, z));
    const float oz = static_cast<float>(moved_coordinate(q, 2, x, y, z));
    o[0] = ox; o[1] = oy; o[2] = oz;
    for (int64_t c = 3; c < stride; ++c) o[c] = s[c];
}

static int64_t padded_rows(int64_t k) { return (k + kTargetTile - 1) / kTargetTile * kTargetTile; }
static int64_t match_blocks(int64_t m) { return (m + kSourceTile - 1) / kSourceTile; }

static bool similarity_ok(const double* transform, Similarity& q) {
    for (int i = 0; i < 13; ++i)
        if (!std::isfinite(transform[i])) return false;
    q.scale = transform[0];
    for (int i = 0; i < 9; ++i) q.r[i] = transform[1 + i];
    for (int i = 0; i < 3; ++i) q.t[i] = transform[10 + i];
    return true;
}

}  // namespace endo

using namespace endo;

extern "C" int endo_registration_tile(int which) {
    return which == 0 ? kSourceTile : (which == 1 ? kTargetTile : ENDO_E_BADARG);
}

extern "C" int64_t endo_registration_prepared_bytes(int64_t k) {
    if (k <= 0 || k > INT32_MAX) return -1;
    return kPreparedHeader + padded_rows(k) * static_cast<int64_t>(sizeof(float4));
}

extern "C" int64_t endo_registration_workspace_bytes(int64_t m, int64_t k) {
    if (m <= 0 || m > INT32_MAX || k <= 0 || k > INT32_MAX) return -1;
    return align256(match_blocks(m) * kSums * static_cast<int64_t>(sizeof(double)));
}

extern "C" int endo_registration_prepare(const float* target, int64_t target_stride, int64_t k, const double* centre, void* prepared,
                                         int64_t prepared_bytes, void* stream_) {
    if (!target || !centre || !prepared || target_stride < 3) return ENDO_E_BADARG;
    const int64_t need = endo_registration_prepared_bytes(k);
    if (need < 0 || prepared_bytes < need) return ENDO_E_BADARG;
    if (!std::isfinite(centre[0]) || !std::isfinite(centre[1]) || !std::isfinite(centre[2])) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t padded = padded_rows(k);
    ProfScope prof(kProfSmall, stream, 0.0, static_cast<double>(k) * 12.0 + static_cast<double>(padded) * 16.0);
    registration_prepare_kernel<<<static_cast<unsigned>(padded / kRegThreads), kRegThreads, 0, stream>>>(
        target, target_stride, k, padded, centre[0], centre[1], centre[2], static_cast<char*>(prepared));
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_registration_match(const float* source, int64_t source_stride, int64_t m, const double* transform, const void* prepared,
                                       const float* target, int64_t target_stride, int64_t k, const double* source_centre, double cap,
                                       int32_t* index, float* distance, double* sums, void* workspace, int64_t workspace_bytes,
                                       void* stream_) {
    if (!source || !transform || !prepared || !target || !source_centre || !index || !distance || !sums || !workspace)
        return ENDO_E_BADARG;
    if (source_stride < 3 || target_stride < 3 || std::isnan(cap)) return ENDO_E_BADARG;
    const int64_t need = endo_registration_workspace_bytes(m, k);
    if (need < 0 || workspace_bytes < need) return ENDO_E_BADARG;
    MatchParams p;
    if (!similarity_ok(transform, p.q)) return ENDO_E_BADARG;
    if (!std::isfinite(source_centre[0]) || !std::isfinite(source_centre[1]) || !std::isfinite(source_centre[2])) return ENDO_E_BADARG;
    p.source = source; p.source_stride = source_stride; p.m = static_cast<int>(m);
    p.prepared = static_cast<const char*>(prepared);
    p.target = target; p.target_stride = target_stride; p.padded = padded_rows(k);
    p.sx = source_centre[0]; p.sy = source_centre[1]; p.sz = source_centre[2];
    p.cap = cap;
    p.index = index; p.distance = distance; p.partials = static_cast<double*>(workspace);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t blocks = match_blocks(m);
    const double pairs = static_cast<double>(m) * static_cast<double>(p.padded);
    ProfScope prof(kProfSmall, stream, 8.0 * pairs, static_cast<double>(blocks) * static_cast<double>(p.padded) * 16.0);
    registration_match_kernel<<<static_cast<unsigned>(blocks), kRegThreads, 0, stream>>>(p);
    ENDO_LAUNCH_CHECK();
    registration_sums_kernel<<<1, kRegThreads, 0, stream>>>(p.partials, blocks, sums);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_similarity_apply(const float* rows, int64_t stride, int64_t m, const double* transform, float* out, void* stream_) {
    if (!rows || !transform || !out || stride < 3 || m < 0 || m > INT32_MAX) return ENDO_E_BADARG;
    Similarity q;
    if (!similarity_ok(transform, q)) return ENDO_E_BADARG;
    if (m == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfSmall, stream, 0.0, static_cast<double>(m) * static_cast<double>(stride) * 8.0);
    similarity_apply_kernel<<<static_cast<unsigned>((m + kRegThreads - 1) / kRegThreads), kRegThreads, 0, stream>>>(rows, stride, m, q, out);
    ENDO_LAUNCH_CHECK();
    return 0;
}
