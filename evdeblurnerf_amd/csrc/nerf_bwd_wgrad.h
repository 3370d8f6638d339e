// Training backward, weight gradients: dW = d y . x^T over all samples, on the tile steps of bwd_tile.h.  A wavefront owns RPW row
// tiles x all column tiles of dW in accumulators and walks the sample tiles with a grid stride; partial sums go to a float32 scratch
// (nerf_bwd_reduce.h sums them), bias gradients ride along as a column of ones.  k_wgrad: the half-precision kernel; k_wgrad_split: the
// split-float16 (float32-grade) form.
#pragma once

#include "nerf_bwd_frags.h"

namespace evd {

struct WgradParams {
    const char* store;
    long tiles, tile_bytes;
    int y_slot, x_slot, bias;       // bias: the bias gradient rides along as column CT
    float* partial;         // [gridDim.x][RT][CT + BIAS][64][16] float32
};

constexpr int WGRAD_NT = 512;      // 8 wavefronts; one sample tile per iteration (one barrier each)
constexpr int wgrad_cpg(int RT, int CT) { return cceil(CT, 8 / RT); }      // column tiles per wavefront group

// RT row tiles (fragments y_slot .. ; YSINGLE: one fragment, 16 channels) x CT column tiles (fragments x_slot ..).
// The 8 wavefronts of a workgroup share every sample tile: wavefront w owns row tile w % RT and the column tiles of its
// group w / RT in accumulators; it transposes its own gradient block, and (w < CT) the activation block of column tile w,
// which it publishes through LDS for the others.  The stored fragments arrive by LDS-DMA (bt_dma4) into a ring of WG_RING tiles per
// wavefront, WG_RING - 1 tiles ahead of their use, with counted vmcnt waits; only the owning wavefront reads its slots, so the ring needs
// no barrier.  (Measured: a ring of 4 with a single-buffered exchange runs at the same speed; with the products or the barrier ablated
// the kernel is no faster: it is bound by its stream of fragment loads at ~3.7 TB/s.)
constexpr int WG_RING = 3;
constexpr int wgrad_ring_bytes() { return WG_RING * 8 * 4 * 1024; }        // [WG_RING][8 wavefronts][4 fragments][1 KiB]
constexpr int wgrad_lds_bytes(int CT) { return wgrad_ring_bytes() + 2 * CT * 2 * 1024; }

template <int PREC, int RT, int CT, bool YSINGLE>
__global__ __launch_bounds__(WGRAD_NT) void k_wgrad(const WgradParams p) {
    constexpr int CPG = wgrad_cpg(RT, CT);
    static_assert(8 % RT == 0 && CT <= 8 && (!YSINGLE || RT == 1), "shape of the block");
    extern __shared__ __attribute__((aligned(16))) char wsm[];
    char* raw = wsm;                                          // the DMA ring
    char* xs = wsm + wgrad_ring_bytes();                      // [2][CT][2][1 KiB] transposed activation blocks
    const int NC = CT + (p.bias ? 1 : 0);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), n = lane & 31, h = lane >> 5;
    const int rt = wave % RT, c0 = (wave / RT) * CPG;
    const bool xown = wave < CT, bias_own = p.bias && wave < RT;
    W4 sel0, sel1;
    bt_selectors<PREC, false>(n, h, sel0, sel1);
    const W4 zf = {{0u, 0u, 0u, 0u}};
    f32x16 acc[CPG], accb;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        accb[i] = 0.f;
#pragma unroll
        for (int c = 0; c < CPG; ++c) acc[c][i] = 0.f;
    }
    // this wavefront's four fragments of a tile: y0, y1 (row tile rt), x0, x1 (column tile `wave`); absent ones (single-fragment
    // gradients, wavefronts beyond CT) re-load y0 so that every tile costs the same four DMA instructions (vmcnt accounting)
    const long oy0 = (long)(p.y_slot + 2 * rt) * 1024, oy1 = YSINGLE ? oy0 : oy0 + 1024;
    const long ox0 = xown ? (long)(p.x_slot + 2 * wave) * 1024 : oy0, ox1 = xown ? ox0 + 1024 : oy0;
    const unsigned ring0 = lds_offset_of(raw) + wave * 4096;
    auto issue = [&](long t, int stage) {
        if (t >= p.tiles) return;
        const char* g = p.store + t * p.tile_bytes + lane * 16;
        bt_dma4(__builtin_amdgcn_readfirstlane(ring0 + stage * (8 * 4096)), g + oy0, g + oy1 - 1024, g + ox0 - 2048, g + ox1 - 3072);
    };
    const long stride = gridDim.x;
    long t = blockIdx.x;
#pragma unroll
    for (int k = 0; k < WG_RING - 1; ++k) issue(t + k * stride, k);
    for (int it = 0; t < p.tiles; t += stride, ++it) {
        issue(t + (WG_RING - 1) * stride, (it + WG_RING - 1) % WG_RING);
        bt_ring_wait((t + stride < p.tiles ? 1 : 0) + (t + 2 * stride < p.tiles ? 1 : 0));
        const char* rw = raw + ((it % WG_RING) * 8 + wave) * 4096 + lane * 16;
        const W4 y0 = *reinterpret_cast<const W4*>(rw), y1 = YSINGLE ? zf : *reinterpret_cast<const W4*>(rw + 1024);
        W4 yt[2], xt[2];
        transpose_block<PREC>(y0, y1, sel0, sel1, yt);
        char* xb = xs + (it & 1) * (CT * 2048);
        if (xown) {
            const W4 x0 = *reinterpret_cast<const W4*>(rw + 2048), x1 = *reinterpret_cast<const W4*>(rw + 3072);
            transpose_block<PREC>(x0, x1, sel0, sel1, xt);
            bt_xt_store(xb, wave, lane, xt);
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < CPG; ++c) {
            if (c0 + c < CT) {
                bt_xt_load(xb, c0 + c, lane, xt);
                bt_prod<PREC>(acc[c], yt, xt);
            }
        }
        if (bias_own) bt_bias<PREC, false>(accb, yt, n, 0);
    }
    float* out = p.partial + (((long)blockIdx.x * RT + rt) * NC) * 1024 + lane * 16;
#pragma unroll
    for (int c = 0; c < CPG; ++c)
        if (c0 + c < CT) bt_put(out + (c0 + c) * 1024, acc[c]);
    if (bias_own) bt_put(out + CT * 1024, accb);
}

// The split-float16 (float32-grade) form: both operands are (hi, lo) pairs; each half is transposed on its own (exact), the products
// are yh xh into acc and yh xl + yl xh into a second accumulator (scaled by 2^11, like the forward's cross terms).  Plain global loads
// (no DMA ring: this mode is for gradient fidelity, the half-precision kernel above is the fast one).  Blocks whose accumulators
// would not fit (RT x CT = 8 x 8) walk the sample tiles once per half of their columns.
template <int RT, int CT, bool YSINGLE>
__global__ __launch_bounds__(WGRAD_NT) void k_wgrad_split(const WgradParams p) {
    constexpr int CPG = wgrad_cpg(RT, CT), PASSES = CPG > 4 ? 2 : 1, CPP = CPG / PASSES, FB = 2048, PREC = EVD_PREC_F16;
    static_assert(8 % RT == 0 && CT <= 8 && (!YSINGLE || RT == 1) && CPG % PASSES == 0, "shape of the block");
    extern __shared__ __attribute__((aligned(16))) char wsm[];
    char* xs = wsm;                                           // [2][CT][hi q0, hi q1, lo q0, lo q1][1 KiB]
    const int NC = CT + (p.bias ? 1 : 0);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), n = lane & 31, h = lane >> 5;
    const int rt = wave % RT, c0 = (wave / RT) * CPG;
    const bool xown = wave < CT, bias_own = p.bias && wave < RT;
    W4 sel0, sel1;
    bt_selectors<PREC, false>(n, h, sel0, sel1);
    const W4 zf = {{0u, 0u, 0u, 0u}};
    float* out = p.partial + (((long)blockIdx.x * RT + rt) * NC) * 1024 + lane * 16;
    auto put = [&](int c, const f32x16& a, const f32x16& ax) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = fmaf(ax[4 * q + i], 4.8828125e-4f, a[4 * q + i]);
            *reinterpret_cast<f32x4*>(out + c * 1024 + 4 * q) = v;
        }
    };
    int it = 0;
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        f32x16 acc[CPP], accx[CPP], accb, accbx;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            accb[i] = accbx[i] = 0.f;
#pragma unroll
            for (int c = 0; c < CPP; ++c) acc[c][i] = accx[c][i] = 0.f;
        }
        for (long t = blockIdx.x; t < p.tiles; t += gridDim.x, ++it) {
            const char* g = p.store + t * p.tile_bytes + lane * 16;
            const W4 y0h = frag_load<W4, FB>(g, p.y_slot + 2 * rt), y0l = frag_load<W4, FB>(g + 1024, p.y_slot + 2 * rt);
            const W4 y1h = YSINGLE ? zf : frag_load<W4, FB>(g, p.y_slot + 2 * rt + 1), y1l = YSINGLE ? zf : frag_load<W4, FB>(g + 1024, p.y_slot + 2 * rt + 1);
            W4 yth[2], ytl[2];
            transpose_block<PREC>(y0h, y1h, sel0, sel1, yth);
            transpose_block<PREC>(y0l, y1l, sel0, sel1, ytl);
            char* xb = xs + (it & 1) * (CT * 4096);
            if (xown) {
                const W4 x0h = frag_load<W4, FB>(g, p.x_slot + 2 * wave), x0l = frag_load<W4, FB>(g + 1024, p.x_slot + 2 * wave);
                const W4 x1h = frag_load<W4, FB>(g, p.x_slot + 2 * wave + 1), x1l = frag_load<W4, FB>(g + 1024, p.x_slot + 2 * wave + 1);
                W4 xth[2], xtl[2];
                transpose_block<PREC>(x0h, x1h, sel0, sel1, xth);
                transpose_block<PREC>(x0l, x1l, sel0, sel1, xtl);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    *reinterpret_cast<W4*>(xb + (wave * 4 + q) * 1024 + lane * 16) = xth[q];
                    *reinterpret_cast<W4*>(xb + (wave * 4 + 2 + q) * 1024 + lane * 16) = xtl[q];
                }
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < CPP; ++c) {
                const int col = c0 + ps * CPP + c;
                if (col < CT) {
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const W4 xh = *reinterpret_cast<const W4*>(xb + (col * 4 + q) * 1024 + lane * 16);
                        const W4 xl = *reinterpret_cast<const W4*>(xb + (col * 4 + 2 + q) * 1024 + lane * 16);
                        acc[c] = mfma_half<PREC>(yth[q], xh, acc[c]);
                        accx[c] = mfma_half<PREC>(yth[q], xl, accx[c]);
                        accx[c] = mfma_half<PREC>(ytl[q], xh, accx[c]);
                    }
                }
            }
            if (bias_own && ps == 0) {
                bt_bias<PREC, false>(accb, yth, n, 0);
                bt_bias<PREC, false>(accbx, ytl, n, 0);
            }
        }
#pragma unroll
        for (int c = 0; c < CPP; ++c)
            if (c0 + ps * CPP + c < CT) put(c0 + ps * CPP + c, acc[c], accx[c]);
        if (bias_own && ps == 0) put(CT, accb, accbx);
    }
}

template <int PREC, int RT, int CT, bool YSINGLE>
static int launch_wgrad(const WgradParams& p, int blocks, hipStream_t st) {
    if constexpr (PREC == EVD_PREC_F16X3) {
        const size_t lds = (size_t)2 * CT * 4096;
        EVD_SET_MAX_LDS((&k_wgrad_split<RT, CT, YSINGLE>), lds);
        hipLaunchKernelGGL((k_wgrad_split<RT, CT, YSINGLE>), dim3(blocks), dim3(WGRAD_NT), lds, st, p);
    } else {
        const size_t lds = wgrad_lds_bytes(CT);
        EVD_SET_MAX_LDS((&k_wgrad<PREC, RT, CT, YSINGLE>), lds);
        hipLaunchKernelGGL((k_wgrad<PREC, RT, CT, YSINGLE>), dim3(blocks), dim3(WGRAD_NT), lds, st, p);
    }
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // namespace evd
