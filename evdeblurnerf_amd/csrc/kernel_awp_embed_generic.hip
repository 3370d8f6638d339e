// Forward of the AWP sample embedding on float32 rows (awp_embed_generic.h): one Linear + bias + ReLU layer per launch.
// reference: networks/dpnerf/awp.py:98-100.
#include "awp_embed_generic.h"
#include "mlp_device.h"

namespace evd {

// v_mfma_f32_32x32x2f32 as in k_gen_dgrad (kernel_nerf_train_generic.hip): lane l gives A[l & 31][l >> 5] and B[l >> 5][l & 31]; register r
// of the result is D[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31].  Here A = the weight block (row = output column m, summed index k),
// B = the input rows (column = sample).  One wavefront owns 32 samples and keeps its half of their input rows in registers: slot t of lane
// half hh is k = 2 t + hh, so step t adds k = 2 t and 2 t + 1 -- k ascends, whatever the grid.  The workgroup's four wavefronts share the
// [32, K] weight block of 32 output columns: read in place (K contiguous floats per row) into LDS once, rows of 33 floats so that both the
// transposing write and the A-operand read are conflict-free.
template <int K>
__global__ __launch_bounds__(256, 2) void k_gen_linear_relu(const GenLinear a) {
    constexpr int LD = 33;
    __shared__ float wt[K * LD];            // wt[k * LD + j]: Wm[m0 + j, k]
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, hh = lane >> 5;
    const long s = ((long)blockIdx.x * 4 + (tid >> 6)) * 32 + n;
    const bool valid = s < a.nsamp;         // every thread stays for the barriers; a row past nsamp is neither read nor written
    float x[K / 2];
    const float* xrow = a.X + (valid ? s : 0) * a.ldx;
#pragma unroll
    for (int i = 0; i < K / 8; ++i) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(xrow + 8 * i), hi = *reinterpret_cast<const f32x4*>(xrow + 8 * i + 4);
        x[4 * i] = hh ? lo[1] : lo[0];
        x[4 * i + 1] = hh ? lo[3] : lo[2];
        x[4 * i + 2] = hh ? hi[1] : hi[0];
        x[4 * i + 3] = hh ? hi[3] : hi[2];
        if (!valid) x[4 * i] = x[4 * i + 1] = x[4 * i + 2] = x[4 * i + 3] = 0.f;
    }
    for (int m0 = 0; m0 < AWPG_W; m0 += 32) {
        for (int idx = tid; idx < 32 * K; idx += 256) {
            const int j = idx / K, k = idx % K;
            wt[k * LD + j] = a.Wm[(size_t)(m0 + j) * K + k];
        }
        __syncthreads();
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int t = 0; t < K / 2; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wt[(2 * t + hh) * LD + n], x[t], acc, 0, 0, 0);
        __syncthreads();                    // the block is free for the next 32 columns
        if (valid) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int m = m0 + 8 * q + 4 * hh;
                const f32x4 b = *reinterpret_cast<const f32x4*>(a.bias + m);
                f32x4 y;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = b[e] + acc[4 * q + e];
                    y[e] = v > 0.f ? v : 0.f;
                }
                *reinterpret_cast<f32x4*>(a.out + s * AWPG_W + m) = y;
                if (a.out2) *reinterpret_cast<f32x4*>(a.out2 + s * AWPG_W + m) = y;
            }
        }
    }
}

int launch_gen_linear_relu(int K, const GenLinear& a, hipStream_t st) {
    const dim3 grid((unsigned)cdiv(a.nsamp, 128)), block(256);
    switch (K) {
    case 64: hipLaunchKernelGGL(k_gen_linear_relu<64>, grid, block, 0, st, a); break;
    case 128: hipLaunchKernelGGL(k_gen_linear_relu<128>, grid, block, 0, st, a); break;
    case 256: hipLaunchKernelGGL(k_gen_linear_relu<256>, grid, block, 0, st, a); break;
    default: return fail(EVD_E_INVALID, "evd_awp_embed_f32_forward: no kernel for %d input columns (built: 64, 128, 256)", K);
    }
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // namespace evd
