// The half-precision training backwards (nerf_bwd_wgrad.h, nerf_bwd_fused.h, voxel_bwd_fused64.h, awp_bwd_fused.h; DESIGN.md, "The
// training backward: each tile step once"): the tile steps their kernels share.  Everything works on stored 1 KiB fragments (W4: one
// lane's 16 bytes of a 32-sample x 16-channel block, samples along the lanes).  A weight gradient d y . x^T contracts over samples, so
// each 32 x 32 block is first transposed ON THE MATRIX CORE (the stored fragments as the A operand against 0/1 selectors as B return it
// with samples along the accumulator registers: transpose_block), converted back to half precision (exact) and fed to the product MFMAs
// (bt_prod); a bias gradient rides along as a product with a column of ones (bt_bias).  A dgrad accumulator goes back to two fragments
// (bt_frags), masked by [stored activation != 0] (bt_mask).  Stored fragments reach the wgrad kernels by LDS-DMA into a ring (bt_dma2 /
// bt_dma4, bt_ring_wait); accumulator blocks leave through bt_put, and the one-wavefront-per-tile kernels fold theirs with bt_fold4.
#pragma once

#include "mlp_pipe.h"

namespace evd {

struct W4 { unsigned w[4]; };

template <int PREC> __device__ __forceinline__ f32x16 mfma_half(const W4& a, const W4& b, const f32x16& c) {
    if constexpr (PREC == EVD_PREC_BF16) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

template <int PREC> __device__ __forceinline__ unsigned half_one_pair() { return PREC == EVD_PREC_BF16 ? 0x3f803f80u : 0x3c003c00u; }

// half-precision value k (0, 1) of a fragment word as float32
template <int PREC> __device__ __forceinline__ float half_value(unsigned word, int k) {
    const unsigned short bits = (unsigned short)(word >> (16 * k));
    if constexpr (PREC == EVD_PREC_BF16) return __uint_as_float((unsigned)bits << 16);
    else return (float)__builtin_bit_cast(_Float16, bits);
}

// Transposition selectors: sel0[kk][n] = (n == kk), sel1[kk][n] = (n == 16 + kk); lane (n = lane & 31, h = lane >> 5) holds kk = 8 h .. 8 h + 7
// of column n.  REMADE: for the kernels that make them where they are used (a dozen VALU instructions) instead of keeping them in registers
// next to their accumulators -- the lane coordinates go through an opaque copy, so the compiler cannot hoist the result out of the tile loop.
template <int PREC, bool REMADE> __device__ __forceinline__ void bt_selectors(int n, int h, W4& sel0, W4& sel1) {
    if constexpr (REMADE) asm volatile("" : "+v"(n), "+v"(h));
    const unsigned one = half_one_pair<PREC>();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int kk = 8 * h + 2 * e;
        sel0.w[e] = (n == kk ? (one & 0xffffu) : 0u) | (n == kk + 1 ? (one & 0xffff0000u) : 0u);
        sel1.w[e] = (n == 16 + kk ? (one & 0xffffu) : 0u) | (n == 17 + kk ? (one & 0xffff0000u) : 0u);
    }
}
// The column of ones at position c: as the B operand of a product with a transposed gradient block it leaves the block's row sums (the bias
// gradient) in column c of the accumulator and adds nothing to the other columns
template <int PREC, bool REMADE> __device__ __forceinline__ W4 bt_ones(int n, int c) {
    if constexpr (REMADE) asm volatile("" : "+v"(n));
    const unsigned v = n == c ? half_one_pair<PREC>() : 0u;
    return W4{{v, v, v, v}};
}

// the 32-channel x 32-sample block held by fragments (f0, f1), returned sample-major: operand q (16 samples) of a
// lane = channel column (lane & 31) of the block; both MFMA operand roles read it the same way.  SINGLE: one stored fragment (a
// 32 x 16 block; f1 is all zero and not multiplied): one MFMA
template <int PREC, bool SINGLE = false>
__device__ __forceinline__ void transpose_block(const W4& f0, const W4& f1, const W4& sel0, const W4& sel1, W4 (&t)[2]) {
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 d = mfma_half<PREC>(f0, sel0, zero);
    if constexpr (!SINGLE) d = mfma_half<PREC>(f1, sel1, d);
    typename POps<PREC>::B b;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
#pragma unroll
        for (int e = 0; e < 4; ++e) POps<PREC>::template set_pair<false>(b, e, d[8 * q + 2 * e], d[8 * q + 2 * e + 1]);
#pragma unroll
        for (int e = 0; e < 4; ++e) t[q].w[e] = b.w[e];
    }
}

// the wavefronts' exchange of transposed activation blocks through LDS: block c of buffer xb = two 1 KiB operands
__device__ __forceinline__ void bt_xt_store(char* xb, int c, int lane, const W4 (&xt)[2]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) *reinterpret_cast<W4*>(xb + (c * 2 + q) * 1024 + lane * 16) = xt[q];
}
__device__ __forceinline__ void bt_xt_load(const char* xb, int c, int lane, W4 (&xt)[2]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) xt[q] = *reinterpret_cast<const W4*>(xb + (c * 2 + q) * 1024 + lane * 16);
}

// wgrad of one (gradient block, activation block) pair, both already transposed; and the block's row sums into column c of `a`
template <int PREC> __device__ __forceinline__ void bt_prod(f32x16& a, const W4 (&yt)[2], const W4 (&xt)[2]) {
    a = mfma_half<PREC>(yt[0], xt[0], a);
    a = mfma_half<PREC>(yt[1], xt[1], a);
}
template <int PREC, bool REMADE> __device__ __forceinline__ void bt_bias(f32x16& a, const W4 (&yt)[2], int n, int c) {
    const W4 o = bt_ones<PREC, REMADE>(n, c);
    a = mfma_half<PREC>(yt[0], o, a);
    a = mfma_half<PREC>(yt[1], o, a);
}

// 32 output rows of a dgrad tile (accumulator rows (i & 3) + 8 (i >> 2) + 4 h as pairs) as the two fragments of the next gradient
template <int PREC> __device__ __forceinline__ void bt_frags(const f32x16& d, W4& o0, W4& o1) {
    typename POps<PREC>::B o2[2];
#pragma unroll
    for (int k = 0; k < 8; ++k) POps<PREC>::template set_pair<false>(o2[k >> 2], k & 3, d[2 * k], d[2 * k + 1]);
    o0 = __builtin_bit_cast(W4, o2[0]);
    o1 = __builtin_bit_cast(W4, o2[1]);
}
// gradient . [stored activation != 0]: the ReLU pattern of the layer below (POps::mask_act holds the formula)
template <int PREC> __device__ __forceinline__ void bt_mask(W4& g, const W4& a) {
    typename POps<PREC>::B b = __builtin_bit_cast(typename POps<PREC>::B, g);
    POps<PREC>::mask_act(b, __builtin_bit_cast(typename POps<PREC>::B, a));
    g = __builtin_bit_cast(W4, b);
}

// The two fragments of a 32-row dgrad output tile (already rounded to half precision) written as float32 ROWS: this lane's sample,
// features 16 f + 8 g + 4 h + 0..3 of the tile for fragment f, half g -- what k_frags_to_rows makes of the stored fragments
// (voxel_train_kernel.h), without the round trip.  row = the sample's row + the tile's first feature; 16-byte aligned (checked by the
// launcher).
template <int PREC> __device__ __forceinline__ void frag_pair_to_row(const W4& f0, const W4& f1, float* row, int h, float inv) {
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const W4& fr = f ? f1 : f0;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            f32x4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = half_value<PREC>(fr.w[2 * g + (k >> 1)], k & 1) * inv;
            *reinterpret_cast<f32x4*>(row + 16 * f + 8 * g + 4 * h) = v;
        }
    }
}

// One tile's four 1 KiB fragments by LDS-DMA (one global_load_lds_dwordx4 = one fragment, no registers in flight) to the LDS offset dst
// (wavefront-uniform) .. dst + 4 KiB.  The instruction's immediate moves the source and the LDS destination together, so piece k's address
// is given less k KiB.  bt_dma2: two adjacent pairs (a0, a0 + 1 KiB | a1 + 2 KiB, a1 + 3 KiB), two address registers; bt_dma4: four
// independent pieces.  Either way a tile costs a wavefront four VM instructions: what bt_ring_wait counts.
__device__ __forceinline__ void bt_dma2(unsigned dst, const char* a0, const char* a1) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, off\n\tglobal_load_lds_dwordx4 %1, off offset:1024\n\t"
                 "global_load_lds_dwordx4 %2, off offset:2048\n\tglobal_load_lds_dwordx4 %2, off offset:3072\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(a0), "v"(a1), "s"(dst) : "memory");
}
__device__ __forceinline__ void bt_dma4(unsigned dst, const char* a0, const char* a1, const char* a2, const char* a3) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %5\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, off\n\tglobal_load_lds_dwordx4 %2, off offset:1024\n\t"
                 "global_load_lds_dwordx4 %3, off offset:2048\n\tglobal_load_lds_dwordx4 %4, off offset:3072\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "s"(dst) : "memory");
}
// a tile's four pieces have landed when at most (tiles issued after it: `later`, at most 2) x 4 are still outstanding
__device__ __forceinline__ void bt_ring_wait(int later) {
    if (later == 2) wait_vmcnt<8>();
    else if (later == 1) wait_vmcnt<4>();
    else wait_vmcnt<0>();
}

// an accumulator block to its slot (a partial block in global memory or an exchange block in LDS): dst = the lane's 16 floats
__device__ __forceinline__ void bt_put(float* dst, const f32x16& a) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 v = {a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]};
        *reinterpret_cast<f32x4*>(dst + 4 * q) = v;
    }
}

// ---- the one-wavefront-per-tile kernels (voxel_bwd_fused64.h, awp_bwd_fused.h): W^T of all layers in LDS, four wavefronts -------------
// nfrag W^T fragments of a stream staged at fragment `first` of wl, by the 256 threads
__device__ __forceinline__ void bt_stage_wt(char* wl, int first, const char* src, int nfrag, int tid) {
    for (int i = tid; i < nfrag * 64; i += 256) *reinterpret_cast<f32x4*>(wl + first * 1024 + i * 16) = *reinterpret_cast<const f32x4*>(src + (long)i * 16);
}
__device__ __forceinline__ W4 bt_wt(const char* wl, int f, int lane) { return *reinterpret_cast<const W4*>(wl + f * 1024 + lane * 16); }

// wgrad of a 64-row gradient g against the XB 32-column blocks of x into acc[a0 + XB yb + xb]; BIAS: its two row tiles' sums into columns
// bcol, bcol + 1 of acc[abias].  The selectors are re-made here instead of living in registers next to up to 304 accumulators.
template <int PREC, int XB, bool BIAS, int NB>
__device__ __forceinline__ void bt_wgrad64(f32x16 (&acc)[NB], int a0, int abias, int bcol, int lane, const W4 (&g)[4], const W4 (&x)[2 * XB]) {
    const int n = lane & 31, h = lane >> 5;
    W4 yt[2][2], xt[2], sel0, sel1;
    bt_selectors<PREC, true>(n, h, sel0, sel1);
#pragma unroll
    for (int yb = 0; yb < 2; ++yb) transpose_block<PREC>(g[2 * yb], g[2 * yb + 1], sel0, sel1, yt[yb]);
#pragma unroll
    for (int xb = 0; xb < XB; ++xb) {
        transpose_block<PREC>(x[2 * xb], x[2 * xb + 1], sel0, sel1, xt);
#pragma unroll
        for (int yb = 0; yb < 2; ++yb) bt_prod<PREC>(acc[a0 + XB * yb + xb], yt[yb], xt);
    }
    if constexpr (BIAS) {
#pragma unroll
        for (int yb = 0; yb < 2; ++yb) bt_bias<PREC, true>(acc[abias], yt[yb], n, bcol + yb);
    }
}
// output tile r of a dgrad over 64 gradient rows: W^T fragments w0 + 4 r .. (LDS) times the four gradient fragments
template <int PREC> __device__ __forceinline__ f32x16 bt_dgrad64(const char* wl, int w0, int r, int lane, const W4 (&g)[4]) {
    f32x16 d = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) d = mfma_half<PREC>(bt_wt(wl, w0 + 4 * r + j, lane), g[j], d);
    return d;
}
// One 64 -> 64 layer: wgrad of (gradient g, input activations x) with the bias columns, dgrad through W^T to the input's gradient gout,
// masked by x
template <int PREC, int NB>
__device__ __forceinline__ void bt_layer64(f32x16 (&acc)[NB], int a0, int abias, int bcol, const char* wl, int w0, int lane, const W4 (&g)[4],
                                           const W4 (&x)[4], W4 (&gout)[4]) {
    bt_wgrad64<PREC, 2, true>(acc, a0, abias, bcol, lane, g, x);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        bt_frags<PREC>(bt_dgrad64<PREC>(wl, w0, r, lane, g), gout[2 * r], gout[2 * r + 1]);
        bt_mask<PREC>(gout[2 * r], x[2 * r]);
        bt_mask<PREC>(gout[2 * r + 1], x[2 * r + 1]);
    }
}

// The workgroup's four accumulator sets folded through LDS (fold: [4 wavefronts][1024] floats): one partial block set per workgroup
template <int NB> __device__ __forceinline__ void bt_fold4(const f32x16 (&acc)[NB], float* fold, float* part, int wave, int lane) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        bt_put(fold + wave * 1024 + lane * 16, acc[b]);
        __syncthreads();
        f32x4 s = *reinterpret_cast<const f32x4*>(fold + wave * 256 + lane * 4);
#pragma unroll
        for (int w = 1; w < 4; ++w) s += *reinterpret_cast<const f32x4*>(fold + w * 1024 + wave * 256 + lane * 4);
        *reinterpret_cast<f32x4*>(part + b * 1024 + wave * 256 + lane * 4) = s;
        __syncthreads();
    }
}

}  // namespace evd
