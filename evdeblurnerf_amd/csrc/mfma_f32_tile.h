// The float32 tile networks (kernel_rigid_blur.hip, kernel_sparse_blur.hip, kernel_view_embed.hip; DESIGN.md, "The float32 tile
// networks"): what their kernels share.  A workgroup of four wavefronts takes tiles of 16 rows; every product is a set of 16 x 16 float32
// MFMA tiles (mt_tile) whose operands sit in zero-padded LDS rows behind a constant one; a tile's epilogue walks a lane's four accumulator
// elements (mt_each).  The backward forms every weight gradient as products d Y^T X over the row dimension (MtMat), expanded into a
// per-tile job table in LDS (mt_jobs), accumulated in registers across the workgroup's tiles (mt_accumulate) and left as per-workgroup
// partial tiles (mt_store_partials); the reduce kernel maps a flat gradient element back to its tile (MtTensor) and sums the workgroups
// in index order (mt_reduce_sum).  The host side builds both tables with one builder (MtPlan), so the writing and the reading side of
// the partial buffer are numbered by the same code.  No atomics anywhere: two runs give the same bits.
#pragma once

#include "evd_common.h"

namespace evd {

constexpr int MT_NT = 256;            // threads of a workgroup
constexpr int MT_NW = MT_NT / 64;     // its wavefronts
constexpr int MT_TR = 16;             // rows of a tile
constexpr int MT_MAX_MATS = 16, MT_MAX_TENSORS = 16;

typedef float mt_f4 __attribute__((ext_vector_type(4)));

// One wavefront, one 16 x 16 tile: acc[i] (row 4 (lane / 16) + i, column lane % 16) += sum_k A[m sa_m + k sa_k] B[n sb_n + k sb_k], m < Mv,
// k < K (A is guarded: parameters are read in place; B is a zero-padded LDS array).
__device__ __forceinline__ mt_f4 mt_tile(mt_f4 acc, const float* A, int sa_m, int sa_k, int Mv, int K, const float* B, int sb_n, int sb_k) {
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
__device__ __forceinline__ mt_f4 mt_zero() {
    mt_f4 z;
    z[0] = z[1] = z[2] = z[3] = 0.f;
    return z;
}

// The epilogue of a tile whose first unit is m0: f(unit m, tile column n = lane % 16, value) for the lane's four elements with m < width
template <class F> __device__ __forceinline__ void mt_each(mt_f4 acc, int m0, int width, F&& f) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + 4 * (lane >> 4) + i;
        if (m < width) f(m, lane & 15, acc[i]);
    }
}
// h[n][m] = relu(acc + bias[m])
__device__ __forceinline__ void mt_store_relu(float* h, int stride, mt_f4 acc, const float* bias, int m0, int width) {
    mt_each(acc, m0, width, [&](int m, int n, float v) { h[n * stride + m] = act(EVD_ACT_RELU, v + bias[m]); });
}
// back through the ReLU: dp[n][m] = h[n][m] > 0 ? acc : 0
__device__ __forceinline__ void mt_gate_relu(float* dp, int dstride, const float* h, int hstride, mt_f4 acc, int m0, int width) {
    mt_each(acc, m0, width, [&](int m, int n, float v) { dp[n * dstride + m] = h[n * hstride + m] > 0.f ? v : 0.f; });
}

__device__ __forceinline__ void mt_zero_lds(float* f, int count) {
    for (int i = threadIdx.x; i < count; i += MT_NT) f[i] = 0.f;
    __syncthreads();
}
template <class S> __device__ __forceinline__ void mt_zero_lds(S& s) { mt_zero_lds(reinterpret_cast<float*>(&s), (int)(sizeof(S) / sizeof(float))); }

// ---- weight gradients -------------------------------------------------------------------------------------------------------------------
// One product d Y^T X over a tile's 16 rows: `ntl` column tiles per row tile, numbered from tile_base on; its operands as float offsets
// into the kernel's LDS, with their row strides.  A bias gradient is the column that a constant one behind X adds.
struct MtMat {
    int tile_base, ntl, dy_off, dy_stride, x_off, x_stride;
};
struct MtMats {                       // parameter of a backward kernel
    MtMat m[MT_MAX_MATS];
    int n, n_tiles;
};
// A tensor of the flat gradient, row-major [rows, width] at `off`: its columns [0, split) are columns col0 ... of product a, the rest
// columns 0 ... of product b
struct MtTensor {
    long off;
    int width, split, col0, base_a, ntl_a, base_b, ntl_b;
};
struct MtTensors {                    // parameter of a reduce kernel
    MtTensor t[MT_MAX_TENSORS];
    int n, n_tiles;
    long end;                         // the flat gradient's size so far
};

// Host side: the products and the tensors, each in the order they are added.  A kernel's capacity (job table, accumulator registers) is the
// tile count of this same arithmetic at the entry's shape limits, evaluated at compile time.
struct MtPlan {
    MtMats mats;
    MtTensors ten;
    constexpr MtMat add_mat(int rows, int cols, int dy_off, int dy_stride, int x_off, int x_stride) {
        const MtMat m = {mats.n_tiles, (cols + 15) / 16, dy_off, dy_stride, x_off, x_stride};
        if (mats.n < MT_MAX_MATS) mats.m[mats.n] = m;
        ++mats.n;
        ten.n_tiles = mats.n_tiles += (rows + 15) / 16 * m.ntl;
        return m;
    }
    constexpr void add_tensor(int rows, int width, const MtMat& a, int col0 = 0) { add_tensor(rows, width, a, col0, width, a); }
    constexpr void add_tensor(int rows, int width, const MtMat& a, int col0, int split, const MtMat& b) {
        const MtTensor t = {ten.end, width, split, col0, a.tile_base, a.ntl, b.tile_base, b.ntl};
        if (ten.n < MT_MAX_TENSORS) ten.t[ten.n] = t;
        ++ten.n;
        ten.end += (long)rows * width;
    }
};
// The one capacity check: a plan the kernel was not compiled for is refused, not left to overrun LDS
inline int mt_check(const char* who, const MtPlan& p, int max_tiles) {
    if (p.mats.n > MT_MAX_MATS || p.ten.n > MT_MAX_TENSORS || p.mats.n_tiles > max_tiles)
        return fail(EVD_E_INVALID, "%s: internal error: a plan of %d products, %d tensors, %d weight-gradient tiles exceeds the built %d, %d, %d", who,
                    p.mats.n, p.ten.n, p.mats.n_tiles, MT_MAX_MATS, MT_MAX_TENSORS, max_tiles);
    return EVD_OK;
}
inline size_t mt_partial_floats(long blocks, int n_tiles) { return (size_t)blocks * n_tiles * 256; }

// Plain float slots behind a caller's pointer, for the two entries whose workspace byte counts predate the 256-byte slots of Workspace
// (evd_common.h) and are part of their ABI.  Used like Workspace: one layout function per entry, the query is that function with a null base.
struct FloatSlots {
    explicit FloatSlots(void* base) : base_(static_cast<float*>(base)) {}
    float* take(size_t count) {
        const size_t at = used_;
        used_ += count;
        return base_ ? base_ + at : nullptr;
    }
    size_t bytes() const { return sizeof(float) * used_; }
private:
    float* base_; size_t used_ = 0;
};

// jobs[t - first] = (d Y offset, d Y stride, X offset, X stride) of the weight-gradient tiles first <= t < first + cap of the plan
__device__ __forceinline__ void mt_jobs(int4* jobs, const MtMats& M, int first, int cap) {
    for (int i = threadIdx.x; i < cap && first + i < M.n_tiles; i += MT_NT) {
        const int t = first + i;
        MtMat m = M.m[0];                 // (selected field by field: the descriptors stay in scalar registers, no indexed load)
#pragma unroll
        for (int j = 1; j < MT_MAX_MATS; ++j)
            if (j < M.n && t >= M.m[j].tile_base) m = M.m[j];
        const int local = t - m.tile_base;
        jobs[i] = make_int4(m.dy_off + (local / m.ntl) * 16, m.dy_stride, m.x_off + (local % m.ntl) * 16, m.x_stride);
    }
}

// wg[i] += d Y^T X over the 16 rows in LDS, for the wavefront's resident tiles first + wave + MT_NW i.  FENCE: one tile's operands in
// flight at a time.
template <int TPW, bool FENCE>
__device__ __forceinline__ void mt_accumulate(mt_f4 (&wg)[TPW], const int4* jobs, const float* lds, int n_tiles, int first) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int t = wv + MT_NW * i;
        if (first + t < n_tiles) {
            const int4 j = jobs[t];
            const float* dy = lds + j.x + (lane & 15);
            const float* X = lds + j.z + (lane & 15);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int row = 4 * u + (lane >> 4);
                wg[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(dy[row * j.y], X[row * j.w], wg[i], 0, 0, 0);
            }
        }
        if (FENCE) asm volatile("" ::: "memory");
    }
}

// the workgroup's partial tiles: partial[blockIdx.x][tile][16][16]
template <int TPW> __device__ __forceinline__ void mt_store_partials(const mt_f4 (&wg)[TPW], float* partial, int n_tiles, int first) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int t = first + wv + MT_NW * i;
        if (t < n_tiles) {
            float* out = partial + ((long)blockIdx.x * n_tiles + t) * 256;
#pragma unroll
            for (int j = 0; j < 4; ++j) out[(4 * (lane >> 4) + j) * 16 + (lane & 15)] = wg[i][j];
        }
    }
}

// ---- reduce ---------------------------------------------------------------------------------------------------------------------------------
// element e of the flat gradient (e >= T.t[0].off): the workgroups' partial tiles in workgroup order
__device__ __forceinline__ float mt_reduce_sum(const MtTensors& T, const float* partial, int n_blocks, long e) {
    int ti = 0;
#pragma unroll
    for (int i = 1; i < MT_MAX_TENSORS; ++i) ti += (i < T.n && e >= T.t[i].off) ? 1 : 0;
    const MtTensor& t = T.t[ti];
    const long local = e - t.off;
    const int m = (int)(local / t.width);
    int n = (int)(local % t.width);
    long tile;
    if (n < t.split) {
        n += t.col0;
        tile = t.base_a + (m >> 4) * t.ntl_a + (n >> 4);
    } else {
        n -= t.split;
        tile = t.base_b + (m >> 4) * t.ntl_b + (n >> 4);
    }
    const float* p = partial + tile * 256 + (m & 15) * 16 + (n & 15);
    float a = 0.f;
    for (int g = 0; g < n_blocks; ++g) a += p[(long)g * T.n_tiles * 256];
    return a;
}

// sum, in ray order, of column `col` of the rows of image img's rays; an image without rays gets zero.  `every`: a caller whose rows all
// belong to one global image says so, and ids is not read (two loops: the flag is not tested per ray)
__device__ __forceinline__ float mt_rows_of_image_sum(const long* ids, long R, long img, const float* rows, long row_stride, int col, bool every = false) {
    float a = 0.f;
    if (every) {
        for (long r = 0; r < R; ++r) a += rows[r * row_stride + col];
    } else {
        for (long r = 0; r < R; ++r)
            if (ids[r] == img) a += rows[r * row_stride + col];
    }
    return a;
}

}  // namespace evd
