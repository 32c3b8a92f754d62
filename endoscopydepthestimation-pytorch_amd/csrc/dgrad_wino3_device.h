// The steps of a phase-skewed Winograd F(2x2, 3x3) data-gradient step, shared by dgrad_wino3_kernel (one block per tile) and
// dgrad_wino3p_kernel (persistent blocks).  dgrad_wino3_kernels.h's header describes the phases; a kernel's geometry struct G gives the
// dY tile's LDS strides (kCS, kCols) and where a lane's patches start in a map (kPatch0).  Accumulators go by reference and every step
// keeps the statement order it had inside the kernels: both kernels sit at the edge of their register budget, and tools/isa_diff.py on
// dgrad_wino3.hip's device assembly before and after is the check to rerun when a step here or its call changes (as functions the
// steps are scheduled a little differently from the lambdas they were: 222 / 241 / 255 registers against 224 / 245 / 256, no scratch).
#pragma once

#include "dgrad_wino_kernels.h"

namespace endo {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// the BN constants of all NL layers: s_bn[layer][channel] = (scale, beta, mean, rstd), one ds_read_b128 per step (wino3_read_bn)
template <int NL, int THREADS>
__device__ __forceinline__ void wino3_build_bn(const DgradBlockParams& p, int64_t grp_off, int tid, float* s_bn) {
    for (int i = tid; i < NL * p.count; i += THREADS) {
        const int l = i / p.count, ch = i - l * p.count;
        const float mean = p.saved[l][grp_off + 2 * ch], rstd = p.saved[l][grp_off + 2 * ch + 1];
        *reinterpret_cast<f32x4*>(s_bn + 4 * i) = f32x4{p.gamma[l][ch] * rstd, p.beta[l][ch], mean, rstd};
    }
}
__device__ __forceinline__ f32x4 wino3_read_bn(const float* s_bn, int count, int gq, int l, int li) {
    return *reinterpret_cast<const f32x4*>(s_bn + 4 * (l * count + gq * 16 + li));
}

// ---- T: the lane's 4x4 patches of layer l's 12 maps, raw, into av (24 8-byte reads): LDS rows 2 w4 .. 2 w4 + 3, two aligned column
//         pairs from kPatch0 + 2 li on; row r's pairs land in av[quad][2 r], av[quad][2 r + 1] ----
template <class G>
__device__ __forceinline__ void wino3_load_patches(const float* s_g, int l, int w4, int lk, int li, f32x2 (&av)[3][8]) {
#pragma unroll
    for (int quad = 0; quad < 3; ++quad) {
        const float* a_base = s_g + (l * 12 + quad * 4 + lk) * G::kCS + G::kPatch0 + (2 * w4) * G::kCols + 2 * li;
#pragma unroll
        for (int row = 0; row < 4; ++row) {
            av[quad][2 * row] = *reinterpret_cast<const f32x2*>(a_base + row * G::kCols);
            av[quad][2 * row + 1] = *reinterpret_cast<const f32x2*>(a_base + row * G::kCols + 2);
        }
    }
}
// ... transformed in place: V = B^T d B, xi = 4 a + i at av[quad][2 a + (i >> 1)][i & 1]
__device__ __forceinline__ void wino3_transform_inplace(f32x2 (&av)[3][8]) {
#pragma unroll
    for (int quad = 0; quad < 3; ++quad) {
        // B^T d on the column pairs (c0, c1) | (c2, c3): rows (d0 - d2, d1 + d2, d2 - d1, d1 - d3) -- 8 packed adds
        // (there is no packed subtract and clang scalarises a - b on ext-vectors: the difference is a packed add with the neg bits set;
        // operands here come from LDS reads, never straight from an MFMA -- the hazard recogniser does not look into inline assembly)
        auto sub2 = [](const f32x2 a, const f32x2 b) { f32x2 r; asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b)); return r; };
        const f32x2 l0 = av[quad][0], h0 = av[quad][1], l1 = av[quad][2], h1 = av[quad][3];
        const f32x2 l2 = av[quad][4], h2 = av[quad][5], l3 = av[quad][6], h3 = av[quad][7];
        const f32x2 tl[4] = {sub2(l0, l2), l1 + l2, sub2(l2, l1), sub2(l1, l3)};
        const f32x2 th[4] = {sub2(h0, h2), h1 + h2, sub2(h2, h1), sub2(h1, h3)};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            // (.) B: (v0, v1) = (c0 - c2, c1 + c2), (v2, v3) = (c2 - c1, c1 - c3) -- one packed add each: the operand-select bits pick c2 for
            // both halves / c1 for both halves, the neg bits the signs (clang turns the same arithmetic on ext-vectors into moves + xor)
            f32x2 v01, v23;
            asm("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(v01) : "v"(tl[a]), "v"(th[a]));
            asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[1,0]" : "=v"(v23) : "v"(th[a]), "v"(tl[a]));
            av[quad][2 * a] = v01;
            av[quad][2 * a + 1] = v23;
        }
    }
}

// ---- M: 16 transform-domain GEMMs over the layer's 12 dY maps: M = this wave's row of 16 tiles, N = the worker's 16 channels; ub = the
//         worker's weight buffer.  after(pair) runs behind the four MFMAs of pair = 4 quad + a (0 .. 11) ----
template <class After>
__device__ __forceinline__ void wino3_mfmas(const float* ub, int lk, int li, const f32x2 (&av)[3][8], f32x4 (&acc)[16], After after) {
#pragma unroll
    for (int quad = 0; quad < 3; ++quad) {
        const float* b_base = ub + ((quad * 4 + lk) * 4 * 16 + li) * 4;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(b_base + a * 64);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (quad == 0) acc[4 * a + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[quad][2 * a + (i >> 1)][i & 1], b[i], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                else acc[4 * a + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[quad][2 * a + (i >> 1)][i & 1], b[i], acc[4 * a + i], 0, 0, 0);
            }
            after(quad * 4 + a);
        }
    }
}

// ---- E: output transform A^T M A (tiles 4 lk + e), the layer's ReLU mask + BN backward, accumulated over the layers into `total`;
//         -> the lane's sums (s1, s2) of the step, before the sum over the wave's rows (each kernel's own) ----
// On register pairs: the output transform runs on the tile pairs (e, e + 1) of the accumulators (adjacent registers of an MFMA result),
// BN + ReLU backward on the pixel pairs (k, k + 1) of x / the running total (adjacent registers of a 16-byte load); the per-pixel
// select between the two (dz = z > 0 ? d : 0) writes its results where the second layout wants them: the transposition.
// The pixel step is the packed-pair, inline-assembly rounding variant of bn_device.h: s2 = fma(dz, xcen, s2), times rstd once.
__device__ __forceinline__ void wino3_epilogue(const f32x4 (&acc)[16], const f32x4 (&xc)[2][2], f32x4 (&total)[2][2], const f32x4 bn, float& s1, float& s2) {
    const f32x2 sb = {bn[0], bn[1]}, mr = {bn[2], bn[3]};          // (scale, beta), (mean, rstd)
    const float rstd = bn[3];
    f32x2 s1v = {0.f, 0.f}, s2v = {0.f, 0.f};
    f32x2 minus1 = {-1.f, -1.f};
    asm("" : "+v"(minus1));          // opaque: with a visible constant the fma below folds back into a subtraction, which is scalarised
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {          // tiles e = 2 hh, 2 hh + 1 = the lane's column half hh
        f32x2 u0r[4], u1r[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const f32x2 m0 = {acc[c][2 * hh], acc[c][2 * hh + 1]}, m1 = {acc[4 + c][2 * hh], acc[4 + c][2 * hh + 1]};
            const f32x2 m2 = {acc[8 + c][2 * hh], acc[8 + c][2 * hh + 1]}, m3 = {acc[12 + c][2 * hh], acc[12 + c][2 * hh + 1]};
            u0r[c] = m0 + m1 + m2;
            u1r[c] = __builtin_elementwise_fma(m2 + m3, minus1, m1);          // m1 - m2 - m3 (compiler-made instructions here: they read MFMA results, and the MFMA -> VALU wait states are the compiler's to insert)
        }
        // d[r][cx] over the tile pair: pixel k = 2 (e & 1) + cx of the column half
        const f32x2 d[2][2] = {{u0r[0] + u0r[1] + u0r[2], __builtin_elementwise_fma(u0r[2] + u0r[3], minus1, u0r[1])},
                               {u1r[0] + u1r[1] + u1r[2], __builtin_elementwise_fma(u1r[2] + u1r[3], minus1, u1r[1])}};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
#pragma unroll
            for (int ee = 0; ee < 2; ++ee) {          // pixels k = 2 ee, 2 ee + 1
                const f32x2 x2 = {xc[r][hh][2 * ee], xc[r][hh][2 * ee + 1]};
                f32x2 xcen, z;
                asm("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(xcen) : "v"(x2), "v"(mr));              // x - mean
                asm("v_pk_fma_f32 %0, %1, %2, %2 op_sel:[0,0,1] op_sel_hi:[1,0,1]" : "=v"(z) : "v"(xcen), "v"(sb));                     // xcen * scale + beta
                const f32x2 dz = {z[0] > 0.f ? d[r][0][ee] : 0.f, z[1] > 0.f ? d[r][1][ee] : 0.f};
                s1v += dz;
                s2v = __builtin_elementwise_fma(dz, xcen, s2v);
                f32x2 t2 = {total[r][hh][2 * ee], total[r][hh][2 * ee + 1]};
                asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(t2) : "v"(dz), "v"(sb));                                    // total += dz * scale
                total[r][hh][2 * ee] = t2[0];
                total[r][hh][2 * ee + 1] = t2[1];
            }
        }
    }
    s1 = s1v[0] + s1v[1];
    s2 = s2v[0] + s2v[1];
    s2 *= rstd;
}

// an M phase ends at a block barrier behind lgkmcnt(0) only: the DMA of the next weight slice stays in flight across it
__device__ __forceinline__ void wino3_phase_end_m() {
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

// The BN-backward sums of a tile (or a run of tiles) leave the block: s_red = [worker][G::kMaxSteps][4 waves][16][2] fp32.  One fp64 atomic
// per (worker, step, channel, sum): the 4 waves' partials added in a fixed order.  Steps as the kernels walk them: worker w's whole
// groups w, w + 2, ... (NL layers each), then -- odd group count -- its NL / 2 layers of the last group.
template <int NL, class G>
__device__ __forceinline__ void wino3_flush_sums(const DgradBlockParams& p, int64_t grp_off, int tid, const float* s_red, int nsteps, int nfull, int ngroups) {
    for (int i = tid; i < 2 * nsteps * 32; i += G::kThreads) {
        const int w = i / (nsteps * 32), rem = i - w * nsteps * 32;
        const int s = rem >> 5, j2 = rem & 31;
        const float* red = s_red + (w * G::kMaxSteps + s) * G::kRedStep + j2;
        const double t = static_cast<double>(red[0]) + static_cast<double>(red[32]) + static_cast<double>(red[64]) + static_cast<double>(red[96]);
        const int gi = s / NL;
        const int gq = gi < nfull ? 2 * gi + w : ngroups - 1;
        const int l = gi < nfull ? s - gi * NL : s - nfull * NL + w * (NL / 2);
        double* sc = l == 0 ? p.scratch[0] : l == 1 ? p.scratch[1] : l == 2 ? p.scratch[2] : p.scratch[3];          // (no dynamic index into the kernel argument)
        atomicAdd(sc + bn_slot_offset(p.slot_stride) + grp_off / 2 + 2 * (gq * 16) + j2, t);
    }
}

}  // namespace endo
