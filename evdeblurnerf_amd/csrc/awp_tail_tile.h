// Device helpers of the AWP tail kernels (awp_tail.h), each step stated once: the 16 x 16 MFMA tile and its two hand-tuned forms (tile16*),
// where a tile's result sits in a lane (TileLane: the epilogue of EVERY tile), which wavefront takes a tile (TileJobs), the P-sized products
// built on these (mm / lin / wacc / bacc), the per-sample loop (each_sample) and its register-row products, the softmaxes, fold_rows.
#pragma once

#include "awp_tail.h"
#include "wave_ops.h"

namespace evd {

// threadIdx.x behind an opaque barrier: hipcc otherwise hoists every helper's per-thread index arithmetic (i / N, n % K, the strided
// offsets of ~40 calls) out of the ray loop and spills it (measured: 278 / 368 spilled registers at 512 threads)
__device__ __forceinline__ int at_tid() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

// The sample-sized products on the exact-float32 matrix core (v_mfma_f32_16x16x4_f32 = an fmaf chain in k order): one wavefront, one
// 16 x 16 tile  D[m][n] += sum_k A[m sa_m + k sa_k] B[k sb_k + n sb_n],  m < Mv, n < Nv, k < K (operands outside are zeros); four
// k-steps of operands are loaded in front of their four MFMAs.  Lane l holds A[m = l % 16][k = l / 16], B[k = l / 16][n = l % 16] and
// the results D[4 (l / 16) + i][l % 16] in acc[i] (TileLane).  On the vector ALU these were the lane-serial loops over the 128 samples of a
// ray: the attention sums (8 k cycles of a 64 k-cycle forward), MAM.linear on the intra sums (28 k), its two transposes in the backward (35 k).
typedef float f32x4v __attribute__((ext_vector_type(4)));
static_assert(AT_NT == 512, "the MAM.linear weight gradient is eight 16 x 16 tiles, one per wavefront");
__device__ __forceinline__ f32x4v tile16(f32x4v acc, const float* A, int sa_m, int sa_k, int Mv, const float* B, int sb_k, int sb_n, int Nv,
                                         int K) {
    const int lane = at_tid() & 63, mn = lane & 15, kq = lane >> 4;
    const bool am = mn < Mv, bn = mn < Nv;
    const float* a = A + (am ? mn : 0) * sa_m;
    const float* b = B + (bn ? mn : 0) * sb_n;
    int k0 = 0;
    for (; k0 + 32 <= K; k0 += 32) {                       // eight k-steps of operands in flight (a trip costs one LDS round trip, whatever its width)
        float av[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = k0 + 4 * u + kq;
            av[u] = a[k * sa_k];
            bv[u] = b[k * sb_k];
            av[u] = am ? av[u] : 0.f;
            bv[u] = bn ? bv[u] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
    }
    for (; k0 < K; k0 += 16) {
        float av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 4 * u + kq;
            const bool in = k < K;
            const int kc = in ? k : 0;
            av[u] = a[kc * sa_k];
            bv[u] = b[kc * sb_k];
            av[u] = (am && in) ? av[u] : 0.f;
            bv[u] = (bn && in) ? bv[u] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
    }
    return acc;
}
__device__ __forceinline__ f32x4v zero4() {
    f32x4v z;
    z[0] = z[1] = z[2] = z[3] = 0.f;
    return z;
}
// MAM.linear on the intra sums (the forward's h_intra -> ls): D[m][n] = sum_{k < 64} X[m][k] W[n][k] with both operands rows of 64 floats
// in global memory.  xrow / wrow: the lane's rows X[m = l % 16], W[n = l % 16].  A lane's four k-steps of a row are ONE 16-byte load:
// float4 number 4 jj + l / 16 of the row, jj < 4, whose component c is the operand of MFMA 4 jj + c -- k = 16 jj + 4 (l / 16) + c on both
// operands, a permuted k order that is this product's own (all eight loads are issued in front of the sixteen MFMAs).
__device__ __forceinline__ f32x4v tile16_h_intra(const float* xrow, const float* wrow, int tid) {
    const int kq = (tid & 63) >> 4;
    const float4* xa = reinterpret_cast<const float4*>(xrow) + kq;
    const float4* wbp = reinterpret_cast<const float4*>(wrow) + kq;
    float4 a[4], b[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) { a[jj] = xa[4 * jj]; b[jj] = wbp[4 * jj]; }
    f32x4v acc = zero4();
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj].x, b[jj].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj].y, b[jj].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj].z, b[jj].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj].w, b[jj].w, acc, 0, 0, 0);
    }
    return acc;
}
// The sample sum of the d MAM.linear.weight tile: acc[m][n] += sum_{s < S} A[s lda] B[s ldb], A the lane's column m = l % 16 of d ls (LDS),
// B the lane's column n = l % 16 of h_intra (global: 64 contiguous bytes per sample and tile).  k = sample: lane l takes the samples
// s0 + 4 u + l / 16, u < 32, of a 128-sample trip; all 32 global operands are requested before the first LDS operand and MFMA (a sample
// past the end reads the last one and multiplies zeros).
__device__ __forceinline__ f32x4v tile16_samples(f32x4v acc, const float* A, int lda, const float* B, int ldb, int S, int tid) {
    const int kq = (tid & 63) >> 4;
    for (int s0 = 0; s0 < S; s0 += 128) {
        float bv[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) {
            const int sx = s0 + 4 * u + kq;
            bv[u] = B[(long)(sx < S ? sx : S - 1) * ldb];
        }
#pragma unroll
        for (int u = 0; u < 32; ++u) {
            const int sx = s0 + 4 * u + kq;
            const float av = sx < S ? A[sx * lda] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, sx < S ? bv[u] : 0.f, acc, 0, 0, 0);
        }
    }
    return acc;
}

// Where a tile16 result sits in this lane: acc[i] is row r0 + i of column c, the tail's counterpart of mt_each (mfma_f32_tile.h) on at_tid().
struct TileLane {
    int r0, c;
    __device__ __forceinline__ explicit TileLane(int tid = at_tid()) { const int lane = tid & 63; r0 = 4 * (lane >> 4); c = lane & 15; }
    template <class F> __device__ __forceinline__ void rows(int M, F&& f) const {       // f(i, row) for the lane's elements in the tile's first M rows
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (r0 + i < M) f(i, r0 + i);
    }
};

// Every product of the chain is a handful of 16 x 16 tiles; a tile goes to the wavefront whose number the running job counter names (the
// same sequence in every thread and for every ray: a parameter's gradient tile is always added by the same lanes).
struct TileJobs {
    int next;
    __device__ __forceinline__ bool mine() { return ((next++) & (AT_NT / 64 - 1)) == (at_tid() >> 6); }
};
// out[m som + n] (+)= act(bias[n] + sum_k A[m sam + k sak] B[n sbn + k sbk]),  m < M <= 16
template <int ACT, bool ACC>
__device__ __forceinline__ void mm(TileJobs& jobs, float* out, int som, const float* A, int sam, int sak, const float* B, int sbn, int sbk,
                                   const float* bias, int M, int N, int K) {
    const TileLane t;
    for (int n0 = 0; n0 < N; n0 += 16) {
        if (!jobs.mine()) continue;
        const f32x4v acc = tile16(zero4(), A, sam, sak, M, B + n0 * sbn, sbk, sbn, min(16, N - n0), K);
        if (n0 + t.c < N) {
            const float bv = bias ? bias[n0 + t.c] : 0.f;
            t.rows(M, [&](int i, int m) {
                float v = acc[i] + bv;
                if (ACT == 1) v = fmaxf(v, 0.f);
                if (ACC) out[m * som + n0 + t.c] += v;
                else out[m * som + n0 + t.c] = v;
            });
        }
    }
}
// y = x W^T (+ b) with W [N, K] row-major (nn.Linear / 1x1 convolution)
template <int ACT>
__device__ __forceinline__ void lin(TileJobs& jobs, float* out, int som, const float* x, int ldx, const float* W, const float* b, int M, int N, int K) {
    mm<ACT, false>(jobs, out, som, x, ldx, 1, W, K, 1, b, M, N, K);
}
// part[n K + k] += sum_m G[m sgm + n] X[m sxm + k]  (weight gradient of y = x W^T)
__device__ __forceinline__ void wacc(TileJobs& jobs, float* part, const float* G, int sgm, const float* X, int sxm, int M, int N, int K) {
    const TileLane t;
    for (int n0 = 0; n0 < N; n0 += 16)
        for (int k0 = 0; k0 < K; k0 += 16) {
            if (!jobs.mine()) continue;
            float old[4];                                   // (the partial row lives in L2: its read is in flight while the tile is computed)
            t.rows(16, [&](int i, int n) { old[i] = (k0 + t.c < K && n0 + n < N) ? part[(n0 + n) * K + k0 + t.c] : 0.f; });
            const f32x4v acc = tile16(zero4(), G + n0, 1, sgm, min(16, N - n0), X + k0, sxm, 1, min(16, K - k0), M);
            if (k0 + t.c < K) t.rows(N - n0, [&](int i, int n) { part[(n0 + n) * K + k0 + t.c] = old[i] + acc[i]; });
        }
}
// part[n] += sum_m G[m sgm + n]: the same tile against a column of ones (`one` points at a 1.0f in LDS)
__device__ __forceinline__ void bacc(TileJobs& jobs, float* part, const float* G, int sgm, int M, int N, const float* one) {
    const TileLane t;
    for (int n0 = 0; n0 < N; n0 += 16) {
        if (!jobs.mine()) continue;
        const f32x4v acc = tile16(zero4(), G + n0, 1, sgm, min(16, N - n0), one, 0, 0, 16, M);
        if (t.c == 0) t.rows(N - n0, [&](int i, int n) { part[n0 + n] += acc[i]; });
    }
}
// softmax of a row, in place, by one wavefront; the row (n <= 256) stays in registers between the two reductions
__device__ __forceinline__ void softmax_row(float* a, int n) {
    const int lane = at_tid() & 63;
    float v[4], m = -INFINITY, t = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        v[u] = lane + 64 * u < n ? a[lane + 64 * u] : -INFINITY;
        m = fmaxf(m, v[u]);
    }
    m = wave_max(m);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        v[u] = lane + 64 * u < n ? expf(v[u] - m) : 0.f;
        t += v[u];
    }
    t = 1.0f / wave_sum_dpp(t);
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (lane + 64 * u < n) a[lane + 64 * u] = v[u] * t;
}
// d logit = a (d a - sum a d a), in place of d a
__device__ __forceinline__ void softmax_row_bwd(const float* a, float* da, int n) {
    const int lane = at_tid() & 63;
    float av[4], dv[4], c = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const bool in = lane + 64 * u < n;
        av[u] = in ? a[lane + 64 * u] : 0.f;
        dv[u] = in ? da[lane + 64 * u] : 0.f;
        c = fmaf(av[u], dv[u], c);
    }
    c = wave_sum_dpp(c);
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (lane + 64 * u < n) da[lane + 64 * u] = av[u] * (dv[u] - c);
}
// the P x P attention map: a row per lane, serially (10 elements; a wavefront per row would cost a row of the S-sized map each)
__device__ __forceinline__ void softmax_small(float* a, int n) {
    float m = -INFINITY, t = 0.f;
    for (int j = 0; j < n; ++j) m = fmaxf(m, a[j]);
    for (int j = 0; j < n; ++j) {
        const float e = expf(a[j] - m);
        a[j] = e;
        t += e;
    }
    t = 1.0f / t;
    for (int j = 0; j < n; ++j) a[j] *= t;
}
__device__ __forceinline__ void softmax_small_bwd(const float* a, float* da, int n) {
    float c = 0.f;
    for (int j = 0; j < n; ++j) c = fmaf(a[j], da[j], c);
    for (int j = 0; j < n; ++j) da[j] = a[j] * (da[j] - c);
}
// ... whose rows go to the lanes of the LAST wavefront (the others are busy with the S-sized map): does thread tid own row `row`?
__device__ __forceinline__ bool small_softmax_row(int tid, int P, int& row) {
    row = tid - (AT_NT - 64);
    return tid >= AT_NT - 64 && row < P;
}

// The per-sample phases: AT_LPS lanes share a sample row, f(s, hf) for this thread's rows s and its share hf < AT_LPS of the row's outputs
// (tid: the ray loop's at_tid())
template <class F> __device__ __forceinline__ void each_sample(int tid, int S, F&& f) {
    const int sl = tid / AT_LPS, hf = tid % AT_LPS;
    for (int s0 = 0; s0 < S; s0 += AT_NT / AT_LPS) {
        const int s = s0 + sl;
        if (s < S) f(s, hf);
    }
}

// Register-row products of the per-sample phases: a lane holds a sample's row in registers, the weights are LDS broadcasts.  The loads of a
// batch of weight rows are issued together IN FRONT of their multiply-adds: hipcc otherwise emits load, wait, four multiply-adds, load, ...
// (measured: 40 k cycles for the MAM.linear step instead of 6 k -- every ds_read's latency exposed, with one wavefront per SIMD).
// o[j] += sum_k W[j K + k] x[k], j < NO
template <int K, int NO, int NJ>
__device__ __forceinline__ void rows_dot(const float* W, const float (&x)[K], float (&o)[NO]) {
#pragma unroll
    for (int j0 = 0; j0 < NO; j0 += NJ) {
        float4 w[NJ][K / 4];
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
            for (int k = 0; k < K / 4; ++k) w[jj][k] = reinterpret_cast<const float4*>(W + (j0 + jj) * K)[k];
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            float a0 = 0.f, a1 = 0.f;
#pragma unroll
            for (int k = 0; k < K / 4; ++k) {
                a0 = fmaf(w[jj][k].x, x[4 * k], a0); a1 = fmaf(w[jj][k].y, x[4 * k + 1], a1);
                a0 = fmaf(w[jj][k].z, x[4 * k + 2], a0); a1 = fmaf(w[jj][k].w, x[4 * k + 3], a1);
            }
            o[j0 + jj] += a0 + a1;
        }
    }
}
// o[n] += sum_m g[m] W[m ldw + n], n < NO (the transposed product in outer-product form: NM rows of W at a time)
template <int M, int NO, int NM>
__device__ __forceinline__ void cols_acc(const float* W, int ldw, const float (&g)[M], float (&o)[NO]) {
#pragma unroll
    for (int m0 = 0; m0 < M; m0 += NM) {
        float4 w[NM][NO / 4];
#pragma unroll
        for (int mm_ = 0; mm_ < NM; ++mm_)
#pragma unroll
            for (int n = 0; n < NO / 4; ++n) w[mm_][n] = reinterpret_cast<const float4*>(W + (m0 + mm_) * ldw)[n];
#pragma unroll
        for (int mm_ = 0; mm_ < NM; ++mm_)
#pragma unroll
            for (int n = 0; n < NO / 4; ++n) {
                o[4 * n] = fmaf(g[m0 + mm_], w[mm_][n].x, o[4 * n]); o[4 * n + 1] = fmaf(g[m0 + mm_], w[mm_][n].y, o[4 * n + 1]);
                o[4 * n + 2] = fmaf(g[m0 + mm_], w[mm_][n].z, o[4 * n + 2]); o[4 * n + 3] = fmaf(g[m0 + mm_], w[mm_][n].w, o[4 * n + 3]);
            }
    }
}
// the same over the P sub-exposures (a run-time count <= 16): o[n] += sum_p col[p cs] rows[p ld + n], n < NO
template <int NO>
__device__ __forceinline__ void p_acc(const float* col, int cs, const float* rows, int ld, int P, float (&o)[NO]) {
    for (int p0 = 0; p0 < P; p0 += 4) {
        float g[4];
        float4 w[4][NO / 4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int pp = p0 + u < P ? p0 + u : P - 1;
            g[u] = p0 + u < P ? col[pp * cs] : 0.f;
#pragma unroll
            for (int n = 0; n < NO / 4; ++n) w[u][n] = reinterpret_cast<const float4*>(rows + pp * ld)[n];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int n = 0; n < NO / 4; ++n) {
                o[4 * n] = fmaf(g[u], w[u][n].x, o[4 * n]); o[4 * n + 1] = fmaf(g[u], w[u][n].y, o[4 * n + 1]);
                o[4 * n + 2] = fmaf(g[u], w[u][n].z, o[4 * n + 2]); o[4 * n + 3] = fmaf(g[u], w[u][n].w, o[4 * n + 3]);
            }
    }
}
// out[p so] = rows[p ld .. + 16] . x for p = p0, p0 + AT_LPS, ... (the logits / their gradients of a sample against the sub-exposures' rows)
__device__ __forceinline__ void p_dot16(float* out, int so, const float* rows, int ld, int p0, int P, const float (&x)[AT_MID]) {
    for (int pa = p0; pa < P; pa += 2 * AT_LPS) {
        const int pb = pa + AT_LPS < P ? pa + AT_LPS : pa;
        float4 wa[4], wb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            wa[k] = reinterpret_cast<const float4*>(rows + pa * ld)[k];
            wb[k] = reinterpret_cast<const float4*>(rows + pb * ld)[k];
        }
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            a = fmaf(wa[k].x, x[4 * k], a); a = fmaf(wa[k].y, x[4 * k + 1], a); a = fmaf(wa[k].z, x[4 * k + 2], a); a = fmaf(wa[k].w, x[4 * k + 3], a);
            b = fmaf(wb[k].x, x[4 * k], b); b = fmaf(wb[k].y, x[4 * k + 1], b); b = fmaf(wb[k].z, x[4 * k + 2], b); b = fmaf(wb[k].w, x[4 * k + 3], b);
        }
        out[pa * so] = a;
        if (pa + AT_LPS < P) out[pb * so] = b;
    }
}

// sum over the partial rows b = first, first + 4, ... < n of src[b stride + col]: four rows in flight per thread, folded (0 + 1) + (2 + 3)
template <class T> __device__ __forceinline__ T fold_rows(const T* src, long stride, long col, int n, int first) {
    T acc[4] = {0, 0, 0, 0};
    int b = first;
    for (; b + 12 < n; b += 16)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] += src[(long)(b + 4 * u) * stride + col];
    for (; b < n; b += 4) acc[0] += src[(long)b * stride + col];
    return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

}  // namespace evd
