// The row arithmetic of AdaptiveWeightProposal.feature_integration (networks/dpnerf/awp.py:49-77) and of its backward, written once for
// the scan kernels (kernel_awp_integrate.hip) and the fused h_local backward (k_local_consumers_bwd, kernel_mam.hip).  AS WRITTEN in the
// reference, the cumprod of :69-73 runs along the CHANNEL axis of the previous sample's row:
//   e[s,c] = exp(-f[s,c] dist[s]),  alpha = 1 - e (0 on the last sample),  dist[s] = (z[s+1] - z[s]) |d|,
//   Q[0,c] = 1,  Q[s+1,c] = prod_{c' <= c} om[s,c'],  om = 1 - alpha + 1e-10,   out[c] = sum_s alpha[s,c] Q[s,c] f[s,c].
// Backward, with g[c] = d out[c]:
//   d f[s,c]  = g[c] Q[s,c] (a + f dist e)                                   direct
//             - dist e Sfx[s+1,c] / om[s,c],  Sfx[s+1,c] = sum_{c'' >= c} g[c''] a[s+1,c''] f[s+1,c''] Q[s+1,c'']      through Q of the next row
//   d dist[s] = sum_c (g[c] Q[s,c] f - Sfx[s+1,c] / om[s,c]) f e             -> d z, d rays_d
// A ray's channels lie along the lanes of a lane group, CPL consecutive channels per lane; the group supplies the cross-lane steps.
#pragma once

#include "ray_math.h"       // ray_norm: |d| of dist
#include "wave_ops.h"

namespace evd {

// 64 lanes per ray: wave scans, the total read from lane 63
struct AwpWaveGroup {
    static __device__ __forceinline__ float excl_mul(float v) { return dpp_f32<0x138>(1.f, wave_scan_mul_dpp(v)); }     // product over the lanes to the left
    static __device__ __forceinline__ float sum_right(float v) {                                                         // sum over the lanes to the right
        const float incl = wave_scan_add_dpp(v);
        return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, incl), 63)) - incl;
    }
    static __device__ __forceinline__ float sum(float v) {
        return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wave_scan_add_dpp(v)), 63));
    }
};
// 16 lanes per ray, four rays per wavefront: 4-step scans inside a DPP row
struct AwpRowGroup {
    static __device__ __forceinline__ float excl_mul(float v) { return dpp_f32<0x111>(1.f, row_scan_mul_dpp(v)); }
    static __device__ __forceinline__ float sum_right(float v) { return row_scan_add_right_dpp(v) - v; }
    static __device__ __forceinline__ float sum(float v) { return row_sum_dpp(v); }
};

// z[s+1] - z[s], 0 on the last sample, and dist[s] = (z[s+1] - z[s]) |d| (awp.py:61-63); s <= S - 1
__device__ __forceinline__ float awp_dz(const float* zz, int s, bool last) { return last ? 0.f : __fsub_rn(zz[s + 1], zz[s]); }
__device__ __forceinline__ float awp_dist(const float* zz, int s, int S, float norm) { return s < S - 1 ? __fmul_rn(__fsub_rn(zz[s + 1], zz[s]), norm) : 0.f; }
__device__ __forceinline__ float awp_e(float f, float dist) { return exp_fast(-__fmul_rn(f, dist)); }
__device__ __forceinline__ float awp_om(float e) { return __fadd_rn(e, 1e-10f); }     // the backward's 1 - alpha + 1e-10

// Q of the NEXT sample row: the inclusive product over the channels of this row's om; local = the lane's own product om[0] ... om[CPL-1]
template <class G, int CPL>
__device__ __forceinline__ void awp_next_q(const float (&om)[CPL], float local, float (&Qn)[CPL]) {
    float excl = G::excl_mul(local);
#pragma unroll
    for (int q = 0; q < CPL; ++q) { excl *= om[q]; Qn[q] = excl; }
}

// Forward row s: acc += alpha Q f, Q <- next row's.  more: s < S - 1 (the last sample's alpha is 0).  GUARD: channels c0 + q >= C are padding
// (f = 0) and leave the product alone.
template <class G, int CPL, bool GUARD>
__device__ __forceinline__ void awp_fwd_row(const float (&f)[CPL], float dist, bool more, int c0, int C, float (&acc)[CPL], float (&Q)[CPL]) {
    float om[CPL], local = 1.f;
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        const float alpha = more ? __fadd_rn(-awp_e(f[q], dist), 1.f) : 0.f;          // awp.py:66-67
        acc[q] = __fadd_rn(acc[q], __fmul_rn(__fmul_rn(alpha, Q[q]), f[q]));
        om[q] = (!GUARD || c0 + q < C) ? __fadd_rn(-alpha, 1.f + 1e-10f) : 1.f;
        local *= om[q];
    }
    awp_next_q<G, CPL>(om, local, Q);
}

// Backward row s.  fc, ec, Q: this row's f, e and Q; fn: row s + 1's f; dist, dist_n: of rows s and s + 1; last: s is the last sample (its
// alpha is 0); more2: s + 2 < S, row s + 1 is not.  Fills d f, the next row's Q and e; returns this lane's part of d dist[s] (sum it with G::sum).
// RCP: 1 / om by v_rcp_f32 (1 ulp) instead of the IEEE division (~10 instructions).
template <class G, int CPL, bool GUARD, bool RCP>
__device__ __forceinline__ float awp_bwd_row(const float (&fc)[CPL], const float (&ec)[CPL], const float (&Q)[CPL], const float (&fn)[CPL],
                                             const float (&g)[CPL], float dist, float dist_n, bool last, bool more2, int c0, int C,
                                             float (&df)[CPL], float (&Qn)[CPL], float (&en)[CPL]) {
    float e[CPL], om[CPL], local = 1.f;
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        e[q] = last ? 1.f : ec[q];
        om[q] = (!GUARD || c0 + q < C) ? awp_om(e[q]) : 1.f;
        local *= om[q];
    }
    // Q of the next row (as awp_next_q) and the suffix sums over the channels of G[s+1, c] = g a f Q of that row
    float Gn[CPL], lsum = 0.f, excl = G::excl_mul(local);
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        excl *= om[q]; Qn[q] = excl;
        en[q] = more2 ? awp_e(fn[q], dist_n) : 1.f;
        const float an = more2 ? __fadd_rn(-en[q], 1.f) : 0.f;
        Gn[q] = last ? 0.f : g[q] * an * fn[q] * Qn[q];
        lsum += Gn[q];
    }
    float sfx = G::sum_right(lsum), ddist = 0.f;
#pragma unroll
    for (int q = CPL - 1; q >= 0; --q) {
        sfx += Gn[q];                                                             // channels >= this one
        const float a = last ? 0.f : __fadd_rn(-e[q], 1.f);
        const float through = last ? 0.f : (RCP ? sfx * __builtin_amdgcn_rcpf(om[q]) : sfx / om[q]);
        const float ga = g[q] * Q[q] * fc[q] - through;                           // d out / d a[s,c]
        df[q] = last ? 0.f : g[q] * Q[q] * a + ga * dist * e[q];
        ddist += last ? 0.f : ga * fc[q] * e[q];
    }
    return ddist;
}

}  // namespace evd
