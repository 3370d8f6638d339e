// The 16 x 16 float32 MFMA tile product of the blur kernel networks (kernel_rigid_blur.hip, kernel_sparse_blur.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace evd {

typedef float rb_f4 __attribute__((ext_vector_type(4)));

// One wavefront, one 16 x 16 tile: acc[i] (row 4 (lane / 16) + i, column lane % 16) += sum_k A[m sa_m + k sa_k] B[n sb_n + k sb_k], m < Mv,
// k < K (A is guarded: parameters are read in place; B is a zero-padded LDS array).
__device__ __forceinline__ rb_f4 rb_tile(rb_f4 acc, const float* A, int sa_m, int sa_k, int Mv, int K, const float* B, int sb_n, int sb_k) {
    const int lane = threadIdx.x & 63, mn = lane & 15, kq = lane >> 4;
    const bool am = mn < Mv;
    const float* a = A + (am ? mn : 0) * sa_m;
    const float* b = B + mn * sb_n;
    for (int k0 = 0; k0 < K; k0 += 16) {
        float av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 4 * u + kq;
            const bool in = am && k < K;
            av[u] = a[(in ? k : 0) * sa_k];
            av[u] = in ? av[u] : 0.f;
            bv[u] = k < K ? b[k * sb_k] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
    }
    return acc;
}
__device__ __forceinline__ rb_f4 rb_zero() {
    rb_f4 z;
    z[0] = z[1] = z[2] = z[3] = 0.f;
    return z;
}

}  // namespace evd
