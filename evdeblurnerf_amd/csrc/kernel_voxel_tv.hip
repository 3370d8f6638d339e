// PDRF backbone: the TV regulariser of the tri-plane grids, TVLoss.forward over one plane / line (voxnerf.py:306-324), value and gradient.
#include "mlp_device.h"
#include "voxel.h"

namespace evd {

// TVLoss.forward (voxnerf.py:306-324) on a channel-last tensor [H][W][C]; accumulates sum dh^2, sum dw^2.
// HBM-bound (every grid value is read once per training iteration): one thread = 4 channels of one texel, float4
// loads of the texel, its lower and its right neighbour (both re-read from L1/L2), rows strided over blockIdx.y,
// double accumulators, one partial pair per block (summed by k_tv_finish).
__device__ __forceinline__ void tv_body(const float* __restrict__ x, int H, int W, int C, double* __restrict__ acc2, int bxi, int byi, int bx, int by) {
    __shared__ double red[2][4];
    const int vec_per_row = W * (C / 4);
    double sh = 0.0, sw = 0.0;
    for (int hh = byi; hh < H; hh += by) {
        const float* row = x + (long)hh * W * C;
        for (int t = bxi * 256 + threadIdx.x; t < vec_per_row; t += bx * 256) {
            const int wq = t / (C / 4);
            const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * (long)t);
            float ph = 0.f, pw = 0.f;
            if (hh + 1 < H) {
                const f32x4 d = *reinterpret_cast<const f32x4*>(row + (long)W * C + 4 * (long)t) - v;
                ph = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
            }
            if (wq + 1 < W) {
                const f32x4 d = *reinterpret_cast<const f32x4*>(row + 4 * (long)t + C) - v;
                pw = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
            }
            sh += (double)ph;
            sw += (double)pw;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { sh += __shfl_xor(sh, off, 64); sw += __shfl_xor(sw, off, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sh; red[1][threadIdx.x >> 6] = sw; }
    __syncthreads();
    if (threadIdx.x == 0) {         // one partial pair per block (4096 same-address double atomics serialise for ~0.2 ms)
        const int b = byi * bx + bxi;
        acc2[2 * b] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        acc2[2 * b + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    }
}
__global__ __launch_bounds__(256) void k_tv(const float* __restrict__ x, int H, int W, int C, double* __restrict__ acc2) {
    tv_body(x, H, W, C, acc2, blockIdx.x, blockIdx.y, gridDim.x, gridDim.y);
}
__host__ __device__ inline int tv_bx(int W, int C) { const long v = ((long)W * (C / 4) + 255) / 256; return (int)(v < 64 ? v : 64); }
__host__ __device__ inline int tv_by(int H) { return H < 64 ? H : 64; }
// the six tensors of a level in one launch: job i's partial pairs at acc + i * 2 * TV_MAX_BLOCKS, as k_tv_finish reads them
__global__ __launch_bounds__(256) void k_tv_level(const TvJobs jobs, double* __restrict__ acc) {
    int i = 0;
    while (i + 1 < jobs.n && (int)blockIdx.x >= jobs.j[i + 1].blk0) ++i;
    const TvJob jb = jobs.j[i];
    const int lb = (int)blockIdx.x - jb.blk0, bx = tv_bx(jb.W, jb.C), by = tv_by(jb.H);
    tv_body(jb.x, jb.H, jb.W, jb.C, acc + (size_t)i * 2 * TV_MAX_BLOCKS, lb % bx, lb / bx, bx, by);
}

__global__ __launch_bounds__(256) void k_tv_finish(const double* __restrict__ part, TvShape s, float* __restrict__ out) {
    // total = sum_i reg(plane_i) * 1e-2 + reg(line_i) * 1e-3,  reg = 2 (h_tv / count_h + w_tv / count_w)  (voxnerf.py:126-130)
    __shared__ double red[2][4];
    double total = 0.0;
    for (int i = 0; i < 6; ++i) {
        const double* p = part + (long)i * 2 * TV_MAX_BLOCKS;
        double sh = 0.0, sw = 0.0;
        for (int b = threadIdx.x; b < s.blocks[i]; b += blockDim.x) { sh += p[2 * b]; sw += p[2 * b + 1]; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { sh += __shfl_xor(sh, off, 64); sw += __shfl_xor(sw, off, 64); }
        __syncthreads();
        if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sh; red[1][threadIdx.x >> 6] = sw; }
        __syncthreads();
        const double h_tv = red[0][0] + red[0][1] + red[0][2] + red[0][3], w_tv = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        const double ch = (double)s.C[i] * (s.H[i] - 1) * s.W[i];
        double cw = (double)s.C[i] * s.H[i] * (s.W[i] - 1);
        if (cw < 1.0) cw = 1.0;
        total += 2.0 * (h_tv / ch + w_tv / cw) * (i < 3 ? 1e-2 : 1e-3);
    }
    if (threadIdx.x == 0) out[0] = (float)total;
}

// d (TV_loss_app) / d grid, added into `grad` scaled by d loss (a device scalar) x weight (1e-2 planes | 1e-3 lines) (voxnerf.py:126-130, 306-324):
// reg = 2 (sum dh^2 / count_h + sum dw^2 / count_w)  =>  d reg / d x = 4 ((dh_prev - dh_next) / count_h + (dw_prev - dw_next) / count_w)
__device__ __forceinline__ void tv_bwd_body(const float* __restrict__ x, int H, int W, int C, const float* __restrict__ d_loss, float weight, float* __restrict__ grad,
                                            int block, int nblocks) {
    const float scale = d_loss[0] * weight;
    const long per_row = (long)W * (C / 4), total = per_row * H;
    const float kh = H > 1 ? 4.f * scale / ((float)C * (H - 1) * W) : 0.f;
    const float cw = fmaxf((float)C * H * (W - 1), 1.f), kw = 4.f * scale / cw;
    for (long v = (long)block * 256 + threadIdx.x; v < total; v += (long)nblocks * 256) {
        const int hh = (int)(v / per_row);
        const long r = v % per_row;
        const int wq = (int)(r / (C / 4));
        const float* px = x + v * 4;
        const f32x4 c = *reinterpret_cast<const f32x4*>(px);
        f32x4 gsum = {0.f, 0.f, 0.f, 0.f};
        if (hh > 0) gsum += (c - *reinterpret_cast<const f32x4*>(px - (long)W * C)) * kh;
        if (hh + 1 < H) gsum -= (*reinterpret_cast<const f32x4*>(px + (long)W * C) - c) * kh;
        if (wq > 0) gsum += (c - *reinterpret_cast<const f32x4*>(px - C)) * kw;
        if (wq + 1 < W) gsum -= (*reinterpret_cast<const f32x4*>(px + C) - c) * kw;
        f32x4* gd = reinterpret_cast<f32x4*>(grad + v * 4);
        *gd = *gd + gsum;
    }
}
__global__ __launch_bounds__(256) void k_tv_bwd(const float* __restrict__ x, int H, int W, int C, const float* __restrict__ d_loss, float weight, float* __restrict__ grad) {
    tv_bwd_body(x, H, W, C, d_loss, weight, grad, blockIdx.x, gridDim.x);
}
// the six tensors of a level in one launch (voxel.h TvJobs)
__global__ __launch_bounds__(256) void k_tv_bwd_level(const TvJobs jobs, const float* __restrict__ d_loss) {
    int i = 0;
    while (i + 1 < jobs.n && (int)blockIdx.x >= jobs.j[i + 1].blk0) ++i;
    const TvJob jb = jobs.j[i];
    if (jb.grad) tv_bwd_body(jb.x, jb.H, jb.W, jb.C, d_loss, jb.weight, jb.grad, (int)blockIdx.x - jb.blk0, jb.nblk);
}

int launch_tv(const float* x, int H, int W, int C, double* acc2, int* blocks, hipStream_t st) {
    if (C % 4) return fail(EVD_E_INVALID, "evd_voxel_tv_loss: component count %d is not a multiple of 4", C);
    const long vec_per_row = (long)W * (C / 4);
    const unsigned bx = (unsigned)(cdiv(vec_per_row, 256) < 64 ? cdiv(vec_per_row, 256) : 64);
    const unsigned by = (unsigned)(H < 64 ? H : 64);
    *blocks = (int)(bx * by);
    k_tv<<<dim3(bx, by), 256, 0, st>>>(x, H, W, C, acc2);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int launch_tv_level(TvJobs& jobs, double* partials, TvShape* shape, hipStream_t st) {
    int total = 0;
    for (int i = 0; i < jobs.n; ++i) {
        TvJob& j = jobs.j[i];
        if (j.C % 4) return fail(EVD_E_INVALID, "evd_voxel_tv_loss: component count %d is not a multiple of 4", j.C);
        j.blk0 = total;
        j.nblk = tv_bx(j.W, j.C) * tv_by(j.H);
        shape->C[i] = j.C; shape->H[i] = j.H; shape->W[i] = j.W; shape->blocks[i] = j.nblk;
        total += j.nblk;
    }
    k_tv_level<<<(unsigned)total, 256, 0, st>>>(jobs, partials);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int launch_tv_finish(const double* acc, const TvShape& s, float* out, hipStream_t st) {
    k_tv_finish<<<1, 256, 0, st>>>(acc, s, out);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int launch_tv_bwd(const float* x, int H, int W, int C, const float* d_loss, float weight, float* grad, hipStream_t st) {
    const long total = (long)H * W * (C / 4);
    k_tv_bwd<<<(unsigned)(cdiv(total, 256) < 4096 ? cdiv(total, 256) : 4096), 256, 0, st>>>(x, H, W, C, d_loss, weight, grad);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int launch_tv_bwd_level(TvJobs& jobs, const float* d_loss, hipStream_t st) {
    int total = 0;
    for (int i = 0; i < jobs.n; ++i) {
        TvJob& j = jobs.j[i];
        const long vecs = (long)j.H * j.W * (j.C / 4);
        j.blk0 = total;
        j.nblk = j.grad ? (int)(cdiv(vecs, 256L) < 4096 ? cdiv(vecs, 256L) : 4096) : 0;
        total += j.nblk;
    }
    if (total == 0) return EVD_OK;
    k_tv_bwd_level<<<(unsigned)total, 256, 0, st>>>(jobs, d_loss);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // namespace evd
