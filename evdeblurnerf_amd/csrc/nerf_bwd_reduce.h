#pragma once

#include "nerf_bwd_frags.h"

namespace evd {

struct WreduceParams {
    const float* partial;
    int nparts, RT, NC, CT;            // NC = CT + 1 when the bias column rides along
    const int* rowmap;                 // [RT * 32] -> row of dW (or -1)
    const int* colmap;                 // [CT * 32] -> column of dW (or -1)
    float* dW;
    int ld;
    float* db;                         // or null
    const unsigned* maxbits;
    int accum = 0;                     // 1: add into dW / db (the caller's persistent gradient buffers) instead of overwriting them
    long part_stride = 0;              // floats between two workgroups' block sets (0: RT * NC * 1024, the sets of ONE layer back to back)
};

// A block sums 64 float4 columns of the partials (4 slices of the workgroup list, folded through LDS), then scatters
// the 256 sums: accumulator element (rt, c, lane, i) -> dW[rowmap[..]][colmap[..]]
static __device__ __forceinline__ void wgrad_reduce_block(const WreduceParams& p, int bx) {
    __shared__ f32x4 fold[4][64];
    const long per = (long)p.RT * p.NC * 1024, v4 = (long)bx * 64 + (threadIdx.x & 63);
    const long pstride = p.part_stride ? p.part_stride : per;
    const int slice = threadIdx.x >> 6;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (v4 * 4 < per) {
        const f32x4* src = reinterpret_cast<const f32x4*>(p.partial) + v4;
#pragma unroll 4
        for (int q = slice; q < p.nparts; q += 4) s += src[(long)q * (pstride / 4)];
    }
    fold[slice][threadIdx.x & 63] = s;
    __syncthreads();
    if (slice != 0 || v4 * 4 >= per) return;
    s = (fold[0][threadIdx.x] + fold[1][threadIdx.x]) + (fold[2][threadIdx.x] + fold[3][threadIdx.x]);
    const float inv = grad_scale(*p.maxbits, true);
    const long idx = v4 * 4;
    const int lane = (idx >> 4) & 63, c = (int)((idx >> 10) % p.NC), rt = (int)((idx >> 10) / p.NC), nc = lane & 31;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = (int)(idx & 15) + k, nr = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        const int row = p.rowmap[rt * 32 + nr];
        if (row < 0) continue;
        if (c < p.CT) {
            const int col = p.colmap[c * 32 + nc];
            if (col >= 0) {            // (row, col) is hit by exactly one thread of one launch: a plain read-modify-write
                float* w = p.dW + (long)row * p.ld + col;
                *w = p.accum ? *w + s[k] * inv : s[k] * inv;
            }
        } else if (nc == 0 && p.db) {
            p.db[row] = p.accum ? p.db[row] + s[k] * inv : s[k] * inv;
        }
    }
}
static __global__ __launch_bounds__(256) void k_wgrad_reduce(const WreduceParams p) { wgrad_reduce_block(p, blockIdx.x); }

// several layers' reductions in one launch (blockIdx.y = layer; the fused backward of voxel_bwd_fused64.h leaves all its layers' blocks
// in one set per workgroup); a layer whose gradient is not wanted has RT = 0
constexpr int WREDUCE_MAX_JOBS = 5;
struct WreduceJobs { WreduceParams j[WREDUCE_MAX_JOBS]; };
static __global__ __launch_bounds__(256) void k_wgrad_reduce_jobs(const WreduceJobs jobs) { wgrad_reduce_block(jobs.j[blockIdx.y], blockIdx.x); }

}  // namespace evd
