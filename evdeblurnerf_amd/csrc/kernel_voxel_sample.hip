// PDRF backbone (reference networks/pdrf/voxnerf.py): the tri-plane feature gather, VoxelNeRFBase.sample / compute_appfeature
// (voxnerf.py:203-208,132-151), in three forms; launch_voxel_sample picks one by shape and grid precision.
// The planes are kept CHANNEL-LAST on the device ([H][W][C], lines [L][C]) so that one bilinear tap of one plane is one contiguous
// 64..256-byte read instead of C strided ones.
#include "voxel_taps.h"

namespace evd {

// F.grid_sample(bilinear, zeros, align_corners=True) x 6 (voxel_taps.h), product, basis_mat.
//
// Phase 1 (gather): work item = (sample, group of 4 channels); the 4 plane taps and 2 line taps of an item are
// loaded BRANCH-FREE (out-of-range taps read a clamped address and get weight 0 -- the zero padding) and all items of
// a thread are issued ahead of their use, 6-12 independent 8/16-byte loads per lane in flight at 4 wavefronts per SIMD (the grids are
// far larger than L2: this phase is a random gather served by Infinity Cache / HBM).
// Phase 2 (basis_mat, voxnerf.py:151): out^T[f, sample] = basis[f, :] . coef[sample, :] for the block's 32 samples on
// the exact-float32 MFMA (v_mfma_f32_32x32x2_f32 = an fmaf chain in k order), by wavefront 0 of the block.
constexpr int VS_STRIDE = VS_MAXC + 1;      // odd row stride: conflict-free column reads in phase 2
static_assert(VS_SAMPLES * VS_STRIDE >= 3 * 16 * 64 + 32 * 33, "the coefficient array doubles as the reduction buffer + output tile");

typedef Taps<long> VsTaps;

// GC channels per work item (4, or 8 when every n_comp is a multiple of 8): the gather is bound by the rate at which the texture
// path takes lane addresses (PMC: TCP_TOTAL_CACHE_ACCESSES = one per lane and load; 1171 per wavefront, 300 k cycles per CU), so
// the wider the per-lane load, the fewer of them: 8 float16 channels = one 16-byte load per tap.
template <bool HALF, int GC>
__global__ __launch_bounds__(256, 4) void k_voxel_sample(const GridParams g, const float* __restrict__ pts, long n,
                                                      float* __restrict__ out, int out_stride, int out_col) {
    __shared__ __attribute__((aligned(16))) float coef[VS_SAMPLES * VS_STRIDE];
    __shared__ __attribute__((aligned(16))) VsTaps taps[VS_SAMPLES * 3];
    constexpr int NV = GC / 4;                   // 4-channel vectors per item
    const int ctot = g.n_comp[0] + g.n_comp[1] + g.n_comp[2];
    const int ng = ctot / GC;
    const long s0 = blockIdx.x * (long)VS_SAMPLES;
    const int items = VS_SAMPLES * ng;
    // phase 2's operand, fetched first so that its latency hides behind the gather: the basis_mat GEMM of the block's 32 samples is
    // split along k over the four wavefronts (a quarter of the components each), every lane keeps its <= 16 basis values in registers
    const bool ksplit = g.app_dim <= 32 && ctot % 8 == 0;
    const int wv = threadIdx.x >> 6, kq = ctot / 4;
    float bq[VS_MAXC / 8];
    if (ksplit) {
        const int lane = threadIdx.x & 63, frow = min(lane & 31, g.app_dim - 1);
        const float* bw = g.basis + (long)frow * ctot + wv * kq + (lane >> 5);
#pragma unroll
        for (int j = 0; j < VS_MAXC / 8; ++j) bq[j] = 2 * j < kq ? bw[2 * j] : 0.f;
    }
    if (threadIdx.x < VS_SAMPLES * 3) {          // phase 0: the tap geometry of every (sample, component) of the block, once
        const int sl = threadIdx.x / 3, i = threadIdx.x % 3;
        const long s = s0 + sl < n ? s0 + sl : n - 1;
        const float pt[3] = {pts[s * 3], pts[s * 3 + 1], pts[s * 3 + 2]};
        VsTaps tp;
        tap_offsets_weights<long>(tap_geometry(g, pt, i), true, tp);
        taps[threadIdx.x] = tp;
    }
    __syncthreads();
    constexpr int UNR = GC == 8 ? 2 : 3;         // n_comp (64,16,16): 32 samples x 12 (24) groups = 1.5 (3) items per thread
    for (int base = threadIdx.x; base < items; base += UNR * 256) {
        VsItem it[UNR][NV];
        int sl[UNR], grp[UNR];
        bool on[UNR];
#pragma unroll
        for (int q = 0; q < UNR; ++q) {             // all tap loads of the thread's items in flight together
            const int t = base + q * 256;
            on[q] = t < items;
            sl[q] = on[q] ? t / ng : 0;
            grp[q] = on[q] ? t % ng : 0;
            const ChannelOf ch = channel_component(grp[q] * GC, g.n_comp[0], g.n_comp[1]);
            const int i = ch.i, c4 = ch.c;
            const VsTaps& tp = taps[sl[q] * 3 + i];
            const float* pl = sel3(i, g.plane[0], g.plane[1], g.plane[2]) + c4;
            const _Float16* plh = sel3(i, g.plane_h[0], g.plane_h[1], g.plane_h[2]) + c4;
            const float* li = sel3(i, g.line[0], g.line[1], g.line[2]) + c4;
            const _Float16* lih = sel3(i, g.line_h[0], g.line_h[1], g.line_h[2]) + c4;
            if (HALF && GC == 8) {                  // one 16-byte load per tap
                typedef _Float16 f16x8v __attribute__((ext_vector_type(8)));
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const f16x8v v = *reinterpret_cast<const f16x8v*>(plh + tp.ip[k]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) it[q][e >> 2].p[k][e & 3] = (float)v[e];
                }
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const f16x8v v = *reinterpret_cast<const f16x8v*>(lih + tp.il[k]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) it[q][e >> 2].l[k][e & 3] = (float)v[e];
                }
            } else {
#pragma unroll
                for (int v = 0; v < NV; ++v) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) it[q][v].p[k] = vs_load<HALF>(pl, plh, tp.ip[k] + 4 * v);
#pragma unroll
                    for (int k = 0; k < 2; ++k) it[q][v].l[k] = vs_load<HALF>(li, lih, tp.il[k] + 4 * v);
                }
            }
#pragma unroll
            for (int v = 0; v < NV; ++v) {
#pragma unroll
                for (int k = 0; k < 4; ++k) it[q][v].wp[k] = tp.wp[k];
#pragma unroll
                for (int k = 0; k < 2; ++k) it[q][v].wl[k] = tp.wl[k];
            }
        }
#pragma unroll
        for (int q = 0; q < UNR; ++q) {
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const f32x4 cf = vs_finish(it[q][v]);
                if (on[q]) {
                    float* dst = &coef[sl[q] * VS_STRIDE + grp[q] * GC + 4 * v];      // odd row stride: scalar stores
#pragma unroll
                    for (int k = 0; k < 4; ++k) dst[k] = cf[k];
                }
            }
        }
    }
    __syncthreads();
    if (ksplit) {
        const int lane = threadIdx.x & 63, col = lane & 31, hh = lane >> 5;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float* cf = coef + col * VS_STRIDE + wv * kq + hh;
#pragma unroll
        for (int j = 0; j < VS_MAXC / 8; ++j)
            if (2 * j < kq) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[j], cf[2 * j], acc, 0, 0, 0);
        __syncthreads();                         // every wavefront has read its coefficients: the array becomes the reduction buffer
        if (wv > 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) coef[((wv - 1) * 16 + r) * 64 + lane] = acc[r];
        }
        __syncthreads();
        // wavefront 0 sums the four partial tiles, applies the activation and transposes the tile through LDS; then ALL threads store:
        // a lane per (sample, feature), 128-byte runs per sample row (the rows of the level's input matrix are 380 / 508 bytes apart:
        // stored straight from the accumulator layout they were 16.8 M scattered 4-byte writes per launch -- 100 us of a 160 us kernel)
        float* ot = coef + 3 * 16 * 64;           // [32 samples][33]
        if (wv == 0) {
#pragma unroll
            for (int w = 0; w < 3; ++w)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] += coef[(w * 16 + r) * 64 + lane];
#pragma unroll
            for (int r = 0; r < 16; ++r) ot[col * 33 + (r & 3) + 8 * (r >> 2) + 4 * hh] = act(g.app_act, acc[r]);
        }
        __syncthreads();
        for (int t = threadIdx.x; t < VS_SAMPLES * 32; t += 256) {
            const int sl = t >> 5, f = t & 31;
            if (s0 + sl < n && f < g.app_dim) out[(s0 + sl) * (long)out_stride + out_col + f] = ot[sl * 33 + f];
        }
        return;
    }
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x, col = lane & 31, hh = lane >> 5;
    for (int f0 = 0; f0 < g.app_dim; f0 += 32) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const int frow = min(f0 + col, g.app_dim - 1);
        const float* bw = g.basis + (long)frow * ctot + hh;
        const float* cf = coef + col * VS_STRIDE + hh;
        for (int kk = 0; kk < ctot; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bw[kk], cf[kk], acc, 0, 0, 0);
        const long s = s0 + col;
        if (s < n) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int f = f0 + 8 * q + 4 * hh;
                float* o = out + s * (long)out_stride + out_col + f;
                if (f + 3 < g.app_dim && ((out_stride | out_col) & 3) == 0) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = act(g.app_act, acc[4 * q + e]);
                    *reinterpret_cast<f32x4*>(o) = v;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (f + e < g.app_dim) o[e] = act(g.app_act, acc[4 * q + e]);
                }
            }
        }
    }
}

// Wavefront-autonomous form of the gather (the one the shipped levels run: every n_comp a multiple of 8, app_dim <= 32).
// PMC + in-kernel stamps of the block-cooperative kernel above (profiles/r02_pmc_voxel.txt): it is neither bandwidth- nor VALU-bound
// but a chain of latencies separated by block barriers (points -> geometry | barrier | gather | barrier | basis GEMM | barrier | reduce |
// barrier | store: 22 k cycles per 32 samples, 4 blocks per CU) -- with L2-resident toy grids it runs at the same speed.  Here a
// WAVEFRONT owns 16 samples from the point load to the store and never waits for another wavefront: geometry of its 48 (sample,
// component) pairs on 48 lanes -> its own LDS slice -> 3 items per lane (16 samples x 12 groups of 8 channels, 18 16-byte loads in
// flight) -> coefficients in LDS -> out^T = basis . coef^T on v_mfma_f32_16x16x4_f32 (2 feature tiles x ctot / 4 steps) -> transposed
// through LDS -> 128-byte runs per sample row.  The 4 wavefronts of a SIMD run their chains independently, so one wavefront's
// matrix work and stores overlap the others' gathers.  (Measured and dropped: persistent wavefronts walking 8 sample groups each so
// that the block's basis_mat load is paid once -- 0.539 / 0.516 / 0.530 ms per c2f render with 1024 / 2048 / 512 blocks against
// 0.521 ms for one group per wavefront: the other wavefronts already hide that prologue.)
constexpr int VW_SAMPLES = 16;                  // samples per wavefront
constexpr int VW_WAVES = 4;                     // wavefronts per block
// LDS slice of one wavefront: tap table, then the coefficient rows [16][ctot + 1] (later the output tile [16][33])
__host__ __device__ constexpr size_t vw_basis_bytes(int ctot) { return (size_t)32 * (ctot + 1) * 4 + 16 - ((size_t)32 * (ctot + 1) * 4) % 16; }
constexpr int VW_OS = 36;                       // row stride of the output tile in LDS (floats): 16-byte aligned rows
__host__ __device__ constexpr size_t vw_slice_bytes(int ctot) { return ((VW_SAMPLES * 3 * sizeof(VsTaps) + (size_t)VW_SAMPLES * (ctot + 1 > VW_OS ? ctot + 1 : VW_OS) * 4) + 15) & ~(size_t)15; }
// OCC: wavefronts per SIMD the kernel is compiled for (registers <= 512 / OCC)
template <bool HALF, int OCC>
__global__ __launch_bounds__(64 * VW_WAVES, OCC) void k_voxel_sample_w(const GridParams g, const float* __restrict__ pts, long n,
                                                                float* __restrict__ out, int out_stride, int out_col) {
    extern __shared__ __attribute__((aligned(16))) char vw_smem[];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ctot = g.n_comp[0] + g.n_comp[1] + g.n_comp[2];
    const int cstride = ctot + 1;                // odd row stride (ctot is a multiple of 8): conflict-free column reads of the GEMM
    float* bs = reinterpret_cast<float*>(vw_smem);                       // basis_mat [32][ctot + 1], shared by the block
    char* slice = vw_smem + vw_basis_bytes(ctot) + (size_t)wv * vw_slice_bytes(ctot);
    VsTaps* taps = reinterpret_cast<VsTaps*>(slice);
    float* coef = reinterpret_cast<float*>(slice + VW_SAMPLES * 3 * sizeof(VsTaps));
    const int ng = ctot / 8;
    const long s0 = ((long)blockIdx.x * VW_WAVES + wv) * VW_SAMPLES;
    // basis_mat -> LDS: the loads are issued first and land while the geometry is computed
    constexpr int NBV = (32 * VS_MAXC / 4 + 64 * VW_WAVES - 1) / (64 * VW_WAVES);
    f32x4 bv[NBV];
    const int nb4 = g.app_dim * ctot / 4;
#pragma unroll
    for (int q = 0; q < NBV; ++q) {
        const int i4 = threadIdx.x + q * 64 * VW_WAVES;
        bv[q] = i4 < nb4 ? *reinterpret_cast<const f32x4*>(g.basis + 4 * i4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (s0 < n && lane < VW_SAMPLES * 3) {       // geometry of this wavefront's (sample, component) pairs
        const int sl = lane / 3, i = lane % 3;
        const long s = s0 + sl < n ? s0 + sl : n - 1;
        const float pt[3] = {pts[s * 3], pts[s * 3 + 1], pts[s * 3 + 2]};
        VsTaps tp;
        tap_offsets_weights<long>(tap_geometry(g, pt, i), true, tp);
        taps[lane] = tp;
    }
#pragma unroll
    for (int q = 0; q < NBV; ++q) {
        const int i4 = threadIdx.x + q * 64 * VW_WAVES;
        if (i4 < nb4) {
            const int f = (4 * i4) / ctot, c = (4 * i4) % ctot;      // ctot is a multiple of 4: the 4 values stay in one row
#pragma unroll
            for (int e = 0; e < 4; ++e) bs[f * cstride + c + e] = bv[q][e];
        }
    }
    __syncthreads();                             // the only block-wide barrier: basis_mat visible (also orders the tap tables)
    if (s0 >= n) return;
    const int items = VW_SAMPLES * ng;
    typedef _Float16 f16x8v __attribute__((ext_vector_type(8)));
    constexpr int UNR = 3;                       // 16 samples x 12 groups = 3 items per lane
    constexpr int NRAW = HALF ? 1 : 2;           // 16-byte loads per tap
    for (int base = lane; base < items; base += UNR * 64) {
        f32x4 rawp[UNR][4][NRAW], rawl[UNR][2][NRAW];    // the taps as loaded (float16 x 8 in one f32x4 register quad, or 2 x float32 x 4)
        int sl[UNR], grp[UNR], comp[UNR];
        bool on[UNR];
#pragma unroll
        for (int q = 0; q < UNR; ++q) {
            const int t = base + q * 64;
            on[q] = t < items;
            sl[q] = on[q] ? t / ng : 0;
            grp[q] = on[q] ? t % ng : 0;
            const ChannelOf ch = channel_component(grp[q] * 8, g.n_comp[0], g.n_comp[1]);
            const int i = ch.i, c8 = ch.c;
            comp[q] = i;
            const VsTaps& tp = taps[sl[q] * 3 + i];
            if (HALF) {
                const _Float16* plh = sel3(i, g.plane_h[0], g.plane_h[1], g.plane_h[2]) + c8;
                const _Float16* lih = sel3(i, g.line_h[0], g.line_h[1], g.line_h[2]) + c8;
#pragma unroll
                for (int k = 0; k < 4; ++k) rawp[q][k][0] = *reinterpret_cast<const f32x4*>(plh + tp.ip[k]);
#pragma unroll
                for (int k = 0; k < 2; ++k) rawl[q][k][0] = *reinterpret_cast<const f32x4*>(lih + tp.il[k]);
            } else {
                const float* pl = sel3(i, g.plane[0], g.plane[1], g.plane[2]) + c8;
                const float* li = sel3(i, g.line[0], g.line[1], g.line[2]) + c8;
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int v = 0; v < NRAW; ++v) rawp[q][k][v] = *reinterpret_cast<const f32x4*>(pl + tp.ip[k] + 4 * v);
#pragma unroll
                for (int k = 0; k < 2; ++k)
#pragma unroll
                    for (int v = 0; v < NRAW; ++v) rawl[q][k][v] = *reinterpret_cast<const f32x4*>(li + tp.il[k] + 4 * v);
            }
        }
#pragma unroll
        for (int q = 0; q < UNR; ++q) {
            const VsTaps& tp = taps[sl[q] * 3 + comp[q]];
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                VsItem it;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (HALF) {
                        const f16x8v h8 = __builtin_bit_cast(f16x8v, rawp[q][k][0]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) it.p[k][e] = (float)h8[4 * v + e];
                    } else {
                        it.p[k] = rawp[q][k][HALF ? 0 : v];
                    }
                    it.wp[k] = tp.wp[k];
                }
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    if (HALF) {
                        const f16x8v h8 = __builtin_bit_cast(f16x8v, rawl[q][k][0]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) it.l[k][e] = (float)h8[4 * v + e];
                    } else {
                        it.l[k] = rawl[q][k][HALF ? 0 : v];
                    }
                    it.wl[k] = tp.wl[k];
                }
                const f32x4 cf = vs_finish(it);
                if (on[q]) {
                    float* dst = &coef[sl[q] * cstride + grp[q] * 8 + 4 * v];
#pragma unroll
                    for (int k = 0; k < 4; ++k) dst[k] = cf[k];
                }
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // this wavefront's LDS writes before its own reads: program order
    __builtin_amdgcn_wave_barrier();
    // out^T[f, sample] = sum_k basis[f, k] coef[sample, k]:  D lane l, reg r = feature 16 tile + 4 (l / 16) + r, sample l % 16
    const int col = lane & 15, kh = lane >> 4;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const float* b0 = bs + min(col, g.app_dim - 1) * cstride + kh;
    const float* b1 = bs + min(16 + col, g.app_dim - 1) * cstride + kh;
    const float* cf = coef + col * cstride + kh;
    // The k loop runs in groups of four steps (ctot is a multiple of 8; a last half group where it is not one of 16): the twelve LDS
    // operands of the NEXT group are read before the eight MFMAs of the current one are issued, so the matrix core never waits for a
    // ds_read (in-kernel stamps, 16 samples: 4.2 k cycles for this phase with every step waiting for its own three reads).
    {
        float pb0[4], pb1[4], pc[4];
        auto fetch = [&](int kk, int cnt) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) { pb0[j] = b0[kk + 4 * j]; pb1[j] = b1[kk + 4 * j]; pc[j] = cf[kk + 4 * j]; }
        };
        int kk = 0;
        fetch(0, ctot >= 16 ? 4 : ctot / 4);
        for (; kk + 16 <= ctot; kk += 16) {
            float cb0[4], cb1[4], cc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { cb0[j] = pb0[j]; cb1[j] = pb1[j]; cc[j] = pc[j]; }
            const int left = ctot - (kk + 16);
            if (left > 0) fetch(kk + 16, left >= 16 ? 4 : left / 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(cb0[j], cc[j], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(cb1[j], cc[j], acc[1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j)                          // the half group (its operands are in the prefetch registers)
            if (kk + 4 * j < ctot) {
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(pb0[j], pc[j], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(pb1[j], pc[j], acc[1], 0, 0, 0);
            }
    }
    __builtin_amdgcn_wave_barrier();             // every lane has read its coefficients: the slice becomes the output tile [16][VW_OS]
#pragma unroll
    for (int tile = 0; tile < 2; ++tile) {
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (16 * tile + 4 * kh + r) < g.app_dim ? act(g.app_act, acc[tile][r]) : 0.f;
        *reinterpret_cast<f32x4*>(&coef[col * VW_OS + 16 * tile + 4 * kh]) = v;      // rows of 36 floats: 16-byte aligned
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (g.app_dim == 32) {                        // a lane stores 8 consecutive features of a sample: 128-byte runs per sample row, two 16-byte
        const int sl = lane >> 2, f0 = 8 * (lane & 3);      // stores per lane (the rows of the level's input matrix are only 4-byte aligned)
        if (s0 + sl < n) {
            typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
            const f32x4 a = *reinterpret_cast<const f32x4*>(&coef[sl * VW_OS + f0]), b = *reinterpret_cast<const f32x4*>(&coef[sl * VW_OS + f0 + 4]);
            float* o = out + (s0 + sl) * (long)out_stride + out_col + f0;
            *reinterpret_cast<f32x4u*>(o) = a;
            *reinterpret_cast<f32x4u*>(o + 4) = b;
        }
    } else {
        for (int t = lane; t < VW_SAMPLES * 32; t += 64) {
            const int sl = t >> 5, f = t & 31;
            if (s0 + sl < n && f < g.app_dim) out[(s0 + sl) * (long)out_stride + out_col + f] = coef[sl * VW_OS + f];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// k_voxel_sample_m (float16 grids): the gather rebuilt around what actually bounds it.  An ablation build of k_voxel_sample_w WITHOUT its grid loads
// runs at 70.1 us against 74.0 us with them (profiles/r06_gather_ablation.log): the kernel was never bound by the gather -- it issues ~3000
// vector instructions per wavefront and 16 samples (static count of its ISA: interpolation with compare / select per element, float16 ->
// float32 conversions, 64-bit tap offsets, the coefficient round trip through LDS for a float32 16 x 16 x 4 GEMM of 48 MFMAs with three LDS
// reads each, the output transposed through LDS), and at four wavefronts per SIMD that IS its duration.  Here:
//   * a lane's work item is (sample = lane % 16, 8-channel group = 4 q + lane / 16), q = 0 .. ctot / 32 - 1: exactly the B-operand layout of
//     v_mfma_f32_16x16x32_f16 (lane holds k = 8 (lane / 16) .. + 7 of column lane % 16) -- the eight coefficients a lane computes ARE its
//     operand, nothing goes through LDS;
//   * out^T[f, sample] = sum_k basis[f, k] coef[sample, k] on the float16 matrix core in the split form the float32-grade modes use everywhere
//     (hi = f16(x), lo = f16(x - hi); A_hi B_hi + A_hi B_lo + A_lo B_hi, float32 accumulate: 2^-21 relative per product): 18 MFMAs of 16 cycles
//     instead of 48 of 32; the split basis_mat operands are made once per workgroup in LDS (12 KiB), the workgroups are persistent.  As in
//     the backward's phase 1, both operands are brought to [2^13, 2^14) by powers of two before the split -- one per basis row (feature) and
//     one per sample, taken over ALL of the sample's coefficients (the three k steps add into one tile) -- and the product is scaled back
//     exactly: without them a grid at 2^-10 put the coefficients into float16 subnormals (2^-7 of the feature lost) and one at 2^10 made
//     them inf;
//   * the D layout (feature 4 (lane / 16) + r of sample lane % 16) is four consecutive floats of a sample's output row: stored straight from the
//     accumulators, no transposition;
//   * 32-bit tap offsets; float16 value converted to float32, then one fused multiply-add with the weight (the float16 copies are
//     saturated to the finite range when they are made, so a zero weight needs no guard).
// Float32 grids keep k_voxel_sample_w: there this form measures equal (67.1 vs 67.0 us) and that kernel's float32 matrix product is exact.
typedef Taps<int> VmTaps;          // 48 bytes
constexpr int VM_WAVES = 4;

__global__ __launch_bounds__(64 * VM_WAVES, 3) void k_voxel_sample_m(const GridParams g, const float* __restrict__ pts, long n,
                                                                       float* __restrict__ out, int out_stride, int out_col) {
    __shared__ __attribute__((aligned(16))) f16x8 a_hi[2 * 3 * 64], a_lo[2 * 3 * 64];        // [feature tile][k step][lane]
    __shared__ __attribute__((aligned(16))) VmTaps taps_all[VM_WAVES][16 * 3];
    __shared__ float a_inv[32];                                                                // 1 / the power-of-two scale of each A row
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c0n = g.n_comp[0], c1n = g.n_comp[1], ctot = c0n + c1n + g.n_comp[2], steps = ctot / 32, F = g.app_dim;
    // the split A operands, made by the first two wavefronts: entry (tile, step, lane) = basis[16 tile + lane % 16][32 step + 8 (lane / 16) .. + 7]
    // x a power of two per basis row (feature) that brings the row's largest magnitude into [2^13, 2^14) (pow2_scale_f16); a lane holds all
    // three steps of its (tile, lane), the four lanes of a row meet by two shuffles
    if (threadIdx.x < 128) {
        const int l = threadIdx.x & 63, tl = threadIdx.x >> 6, f = 16 * tl + (l & 15);
        float v[3][8], m = 0.f;
#pragma unroll
        for (int st = 0; st < 3; ++st)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                v[st][j] = (f < F && st < steps) ? g.basis[(long)f * ctot + 32 * st + 8 * (l >> 4) + j] : 0.f;
                m = fmaxf(m, fabsf(v[st][j]));
            }
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        float inv;
        const float sc = pow2_scale_f16(m, &inv);
#pragma unroll
        for (int st = 0; st < 3; ++st) {
            f16x8 hi, lo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x = v[st][j] * sc;
                hi[j] = (_Float16)x;
                lo[j] = (_Float16)(x - (float)hi[j]);
            }
            a_hi[(tl * 3 + st) * 64 + l] = hi;
            a_lo[(tl * 3 + st) * 64 + l] = lo;
        }
        if (l < 16) a_inv[f] = inv;
    }
    __syncthreads();
    VmTaps* taps = taps_all[wv];
    const int col = lane & 15, kb = lane >> 4;
    const long tiles = (n + 15) / 16;
    for (long tile = (long)blockIdx.x * VM_WAVES + wv; tile < tiles; tile += (long)gridDim.x * VM_WAVES) {
        const long s0 = tile * 16;
        // (measured and dropped: the NEXT tile's points fetched here, one tile ahead -- 57.8 vs 56.7 us: their latency is not what the tile waits for)
        if (lane < 48) {                              // geometry of this wavefront's (sample, component) pairs, once each
            const int sl = lane / 3, i = lane % 3;
            const long s = s0 + sl < n ? s0 + sl : n - 1;
            const float pt[3] = {pts[s * 3], pts[s * 3 + 1], pts[s * 3 + 2]};
            VmTaps tp;
            tap_offsets_weights<long>(tap_geometry(g, pt, i), true, tp);          // <long> into an int record: computed in 64 bits, then truncated, as this kernel always has
            taps[lane] = tp;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        f32x4 rawp[3][4], rawl[3][2];                 // a tap's eight float16 values: one 16-byte load
        int tix[3];                                   // the item's row of the tap table: the weights are read again when the values have landed
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (q < steps) {
                const ChannelOf ch = channel_component(32 * q + 8 * kb, c0n, c1n);
                const int i = ch.i, c8 = ch.c;
                tix[q] = col * 3 + i;
                struct { int ip[4], il[2]; } tq[3];
#pragma unroll
                for (int k = 0; k < 4; ++k) tq[q].ip[k] = taps[tix[q]].ip[k];
#pragma unroll
                for (int k = 0; k < 2; ++k) tq[q].il[k] = taps[tix[q]].il[k];
                const _Float16* plh = sel3(i, g.plane_h[0], g.plane_h[1], g.plane_h[2]) + c8;
                const _Float16* lih = sel3(i, g.line_h[0], g.line_h[1], g.line_h[2]) + c8;
#pragma unroll
                for (int k = 0; k < 4; ++k) rawp[q][k] = *reinterpret_cast<const f32x4*>(plh + tq[q].ip[k]);
#pragma unroll
                for (int k = 0; k < 2; ++k) rawl[q][k] = *reinterpret_cast<const f32x4*>(lih + tq[q].il[k]);
            }
        }
        // The B operand's scale: a power of two that brings the sample's largest |coefficient| (over the four lanes of its column) into
        // [2^13, 2^14), so that the hi / lo split keeps 2^-22 of it -- unscaled, small coefficients fell into float16 subnormals and ones
        // above 65504 became inf (and the lo term NaN).  The three k steps add into one tile, so the scale is that of the running maximum
        // over the steps so far: when a step raises it, the tile is first multiplied by the ratio of the two powers of two (<= 1: exact).
        f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        float bm = 0.f, b_inv = 0.f;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (q < steps) {
                float cf[8];
                struct { float wp[4], wl[2]; } tq[3];
#pragma unroll
                for (int k = 0; k < 4; ++k) tq[q].wp[k] = taps[tix[q]].wp[k];
#pragma unroll
                for (int k = 0; k < 2; ++k) tq[q].wl[k] = taps[tix[q]].wl[k];
                float pv[8], lv[8];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const f16x8 h = __builtin_bit_cast(f16x8, rawp[q][k]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) pv[e] = k == 0 ? (float)h[e] * tq[q].wp[0] : __builtin_fmaf((float)h[e], tq[q].wp[k], pv[e]);
                }
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const f16x8 h = __builtin_bit_cast(f16x8, rawl[q][k]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) lv[e] = k == 0 ? (float)h[e] * tq[q].wl[0] : __builtin_fmaf((float)h[e], tq[q].wl[k], lv[e]);
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) cf[e] = pv[e] * lv[e];
                float m = bm;
#pragma unroll
                for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(cf[e]));
                m = fmaxf(m, __shfl_xor(m, 16));
                m = fmaxf(m, __shfl_xor(m, 32));
                float inv;
                const float sc = pow2_scale_f16(m, &inv);
                if (q > 0) {
                    const float ratio = sc * b_inv;   // new scale / old scale
#pragma unroll
                    for (int tl = 0; tl < 2; ++tl) acc[tl] *= ratio;
                }
                bm = m;
                b_inv = inv;
                f16x8 bh, bl;
#pragma unroll
                for (int e = 0; e < 8; e += 2) {
                    const float x0 = cf[e] * sc, x1 = cf[e + 1] * sc;
                    const f16x2 h2 = __builtin_convertvector(f32x2{x0, x1}, f16x2);
                    const f16x2 l2 = __builtin_convertvector(f32x2{x0 - (float)h2[0], x1 - (float)h2[1]}, f16x2);
                    bh[e] = h2[0]; bh[e + 1] = h2[1];
                    bl[e] = l2[0]; bl[e + 1] = l2[1];
                }
#pragma unroll
                for (int tl = 0; tl < 2; ++tl) {
                    const f16x8 ah = a_hi[(tl * 3 + q) * 64 + lane], al = a_lo[(tl * 3 + q) * 64 + lane];
                    acc[tl] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acc[tl], 0, 0, 0);
                    acc[tl] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc[tl], 0, 0, 0);
                    acc[tl] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc[tl], 0, 0, 0);
                }
            }
        }
        // D: lane (col = sample, kb), register r = feature 16 tl + 4 kb + r: four consecutive floats of the sample's output row
        if (s0 + col < n) {
            typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
            float* o = out + (s0 + col) * (long)out_stride + out_col;
#pragma unroll
            for (int tl = 0; tl < 2; ++tl) {
                const int f0 = 16 * tl + 4 * kb;
                f32x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = (acc[tl][r] * b_inv) * a_inv[f0 + r];       // both scales are powers of two: exact
                if (g.app_act != EVD_ACT_NONE) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = act(g.app_act, v[r]);
                }
                if (f0 + 3 < F) *reinterpret_cast<f32x4u*>(o + f0) = v;
                else
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (f0 + r < F) o[f0 + r] = v[r];
            }
        }
        __builtin_amdgcn_wave_barrier();              // the tap table is rewritten by the next tile
    }
}

int launch_voxel_sample(const GridParams& g, bool half_grids, const float* pts, long n, float* out, int out_stride, int out_col, hipStream_t st) {
    const bool wide = (g.n_comp[0] % 8 == 0) && (g.n_comp[1] % 8 == 0) && (g.n_comp[2] % 8 == 0);
    if (wide && g.app_dim <= 32) {
        const unsigned blocks = (unsigned)cdiv(n, (long)VW_SAMPLES * VW_WAVES);
        const int ct = g.n_comp[0] + g.n_comp[1] + g.n_comp[2];
        const size_t lds = vw_basis_bytes(ct) + VW_WAVES * vw_slice_bytes(ct);
        // float16 grids: k_voxel_sample_m where the channels come in 32-wide k steps and the tap offsets fit 32 bits, else k_voxel_sample_w;
        // float32 grids: k_voxel_sample_w compiled for three blocks per CU (168 registers; by default 174 = two)
        long pmax_h = 0;
        for (int i = 0; i < 3; ++i) {
            const long pe = (long)g.grid[i == 2 ? 1 : 0] * g.grid[i == 0 ? 1 : 2] * g.n_comp[i];
            pmax_h = pe > pmax_h ? pe : pmax_h;
        }
        if (half_grids && ct % 32 == 0 && ct <= 96 && pmax_h < (1L << 31)) {
            const long tiles = cdiv(n, 16L * VM_WAVES), cap = 8L * device_cus();
            const unsigned mb = (unsigned)(tiles < cap ? tiles : cap);
            // (three wavefronts per SIMD, 168 registers with the operand scaling, no spills; compiled for four -- 128 registers, 34 spilled -- it runs 70 instead of 57 us)
            k_voxel_sample_m<<<mb, 64 * VM_WAVES, 0, st>>>(g, pts, n, out, out_stride, out_col);
            EVD_LAUNCH_CHECK();
            return EVD_OK;
        }
        if (half_grids) k_voxel_sample_w<true, 4><<<blocks, 64 * VW_WAVES, lds, st>>>(g, pts, n, out, out_stride, out_col);
        else k_voxel_sample_w<false, 3><<<blocks, 64 * VW_WAVES, lds, st>>>(g, pts, n, out, out_stride, out_col);
        EVD_LAUNCH_CHECK();
        return EVD_OK;
    }
    if (half_grids && wide) k_voxel_sample<true, 8><<<cdiv(n, VS_SAMPLES), 256, 0, st>>>(g, pts, n, out, out_stride, out_col);
    else if (half_grids) k_voxel_sample<true, 4><<<cdiv(n, VS_SAMPLES), 256, 0, st>>>(g, pts, n, out, out_stride, out_col);
    else if (wide) k_voxel_sample<false, 8><<<cdiv(n, VS_SAMPLES), 256, 0, st>>>(g, pts, n, out, out_stride, out_col);
    else k_voxel_sample<false, 4><<<cdiv(n, VS_SAMPLES), 256, 0, st>>>(g, pts, n, out, out_stride, out_col);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // namespace evd
