// Training backward, wgrad(l) WITH dgrad(l) in one launch (round 4; asked for since round 1).  Both read the layer's gradient fragments
// G = d loss / d pre-activation [OUT = 256 channels x 32 samples] of every tile: k_wgrad to add G X^T to dW, k_dgrad_layer to form
// d X = W^T G.  Here the wgrad workgroup (8 wavefronts, wavefront w = row tile w of dW, RT = 8) also produces d X: after the tile's barrier
// all 16 gradient fragments lie in the LDS-DMA ring in exactly the form the matrix core takes as its B operand; wavefront w (< TO)
// multiplies them by the 16 A fragments of rows 32 w .. 32 w + 31 of W^T, which stay RESIDENT for its whole life (registers plus a few
// LDS slots of its own: no weight traffic at all), applies the ReLU pattern of the layer below and stores its two fragments of d X.  Per
// tile the pair moved 65 KiB (dgrad: G in, mask, d X out; wgrad: G, X in); fused it is 49 KiB.
// FusedLayer states the per-tile phases once; k_wgrad_dgrad and k_wgrad_dgrad_p are two schedules of them.
#pragma once

#include "nerf_bwd_wgrad.h"

namespace evd {

struct WgradFusedParams {
    WgradParams w;
    const char* wt;         // W^T fragment stream of the layer (tile-major, 16 k-steps per tile: pack.h layer_transposed)
    char* out_store;        // the store again, writable
    int mask_slot, out_slot;
    int y_last_slot = -1;   // RT < 8: the slot of the LAST row tile's fragment pair when it does not follow the others (-1: it does)
    const char* ygen_wt = nullptr;      // YGEN: W^T stream of the 16-row layer ABOVE (8 output tiles x 1 k-step), see FusedLayer
    // optional: the first rows_tiles output tiles of d X leave as float32 rows [nsamp, rows_stride] (loss scale removed) instead of fragments
    float* rows = nullptr;
    int rows_stride = 0, rows_tiles = 0;
    long nsamp = 0;
    const unsigned* maxbits = nullptr;
};

// W^T fragments per wavefront kept in LDS instead of registers: the two-barrier kernel (128 + 16 accumulators: with all 64 registers of
// W^T it spilled into its loop, and a scratch reload drains the VM counter); the pipelined one (no bias accumulator: its 16 registers hold
// two more W^T fragments and the second set of transposed gradient fragments)
constexpr int FUSED_WL = 6, FUSED_WL_P = 4;
// LDS: the DMA ring, XBUFS exchange buffers of CT transposed activation blocks, [8 wavefronts][WLMAX][1 KiB] of W^T
constexpr int fused_wl_offset(int CT, int XBUFS) { return wgrad_ring_bytes() + XBUFS * CT * 2048; }
constexpr int fused_lds_bytes(int CT, int XBUFS, int WLMAX) { return fused_wl_offset(CT, XBUFS) + 8 * WLMAX * 1024; }

// One wavefront's state and per-tile phases of a fused layer (wavefront w: row tile w of dW, column-tile block w of the exchange, output
// tile w of d X).
// RT_ < 8 (round 5: sigma_net.1 = [geo rows | sigma row], 4 + 1 row tiles): wavefronts RT_ .. 7 own no gradient rows (no wgrad products,
// no partial blocks), the dgrad runs over the first KD gradient fragments (the last row tile may be a single fragment: KD = 2 RT_ - 1).
// YGEN (round 5: color_net.1 under the 3-row color_net.2): the layer's gradient G is not read but FORMED -- every wavefront fetches the pair
// [gradient fragment of the layer above (16 rows) | ReLU bit-mask fragment of this layer's output] at y_slot (2 KiB, the same for all
// eight: L2 hits) in place of its 2 KiB of G, multiplies its 32 rows of the upper layer's W^T (one resident A fragment) with it, masks,
// and puts the two fragments where the DMA would have put them.  The upper layer's dgrad launch, its 16 KiB write and this kernel's
// 16 KiB read of G per tile are gone.
// ROWS: the first rows_tiles output tiles of d X leave as float32 rows (WgradFusedParams::rows) instead of fragments.
template <int PREC, int CT, int TO, int OMASK, int RT_, int KD, bool YGEN, bool ROWS, int WLMAX, int XBUFS>
struct FusedLayer {
    static_assert(!YGEN || (RT_ == 8 && KD == 16), "a formed gradient has all 8 row tiles");
    static_assert(is_half_prec(PREC) && CT <= 8 && TO <= 8 && (OMASK == 0 || TO <= CT), "half-precision fragments, 8 x 32 gradient rows; a masked d X tile is a column tile of X");
    static_assert(RT_ <= 8 && KD <= 2 * RT_ && KD > 2 * (RT_ - 1), "k-steps of the dgrad = the gradient fragments of the RT_ row tiles");
    static constexpr int WL = KD > WLMAX + 2 ? WLMAX : 0;
    typedef POps<PREC> O;
    const WgradFusedParams& fp;
    char *raw, *xs, *wl;        // the DMA ring; [XBUFS][CT][2][1 KiB] transposed activation blocks; the last WL of each wavefront's W^T fragments
    int lane, wave, n, h;
    bool xown, yown, down;
    long oy, ox;
    unsigned ring0;
    W4 wt[KD - WL], w2;
    f32x16 acc[CT];

    // prologue: rows 32 w .. of W^T, KD A fragments, resident -- KD - WL in registers, the last WL in this wavefront's own LDS slots
    __device__ __forceinline__ FusedLayer(const WgradFusedParams& fp_, char* wsm) : fp(fp_) {
        const WgradParams& p = fp.w;
        raw = wsm;
        xs = wsm + wgrad_ring_bytes();
        wl = wsm + fused_wl_offset(CT, XBUFS);
        pipe_fp16_saturate<PREC>();
        lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), n = lane & 31, h = lane >> 5;
        // (activation block w belongs to wavefront w.  Also measured, round 5: with no mask the LAST CT wavefronts taking the blocks, so that in
        // the 8 x 4 / 8 x 5 launches the dgrad wavefronts do not transpose as well -- same box 13.55 / 13.56 / 13.56 against 13.52 / 13.58 / 13.56 ms
        // per iteration: the wait moves between the two barriers)
        xown = wave < CT, yown = wave < RT_, down = wave < TO;
#pragma unroll
        for (int i = 0; i < 16; ++i)
#pragma unroll
            for (int c = 0; c < CT; ++c) acc[c][i] = 0.f;
#pragma unroll
        for (int j = 0; j < KD; ++j) {
            const W4 f = *reinterpret_cast<const W4*>(fp.wt + ((long)(down ? wave : 0) * KD + j) * 1024 + lane * 16);    // (wavefronts beyond TO: tile 0 again, unused)
            if (j < KD - WL) wt[j] = f;
            else *reinterpret_cast<W4*>(wl + (wave * WL + (j - (KD - WL))) * 1024 + lane * 16) = f;
        }
        // the tile's four fragments of this wavefront: y0, y1 (adjacent: one address) and x0, x1 (wavefronts beyond CT: the y pair again)
        // (wavefronts beyond RT_: row tile 0's pair again, unused -- every tile costs every wavefront the same four DMA instructions)
        const int ys = (YGEN || !yown) ? p.y_slot : (RT_ < 8 && wave == RT_ - 1 && fp.y_last_slot >= 0) ? fp.y_last_slot : p.y_slot + 2 * wave;
        oy = (long)ys * 1024 + lane * 16;
        ox = (xown ? (long)(p.x_slot + 2 * wave) * 1024 : (long)ys * 1024) + lane * 16 - 2048;
        ring0 = lds_offset_of(raw) + wave * 4096;
        w2 = W4{{0u, 0u, 0u, 0u}};
        if constexpr (YGEN) w2 = *reinterpret_cast<const W4*>(fp.ygen_wt + (long)wave * 1024 + lane * 16);       // rows 32 w .. of the upper layer's W^T
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the weight fragments have landed: the counted waits count the ring's DMA only
        if constexpr (YGEN) asm volatile("" : "+v"(w2.w[0]), "+v"(w2.w[1]), "+v"(w2.w[2]), "+v"(w2.w[3]));
#pragma unroll
        for (int j = 0; j < KD - WL; ++j) asm volatile("" : "+v"(wt[j].w[0]), "+v"(wt[j].w[1]), "+v"(wt[j].w[2]), "+v"(wt[j].w[3]));
    }

    __device__ __forceinline__ void issue(long t, int stage) const {
        if (t >= fp.w.tiles) return;
        const char* g = fp.w.store + t * fp.w.tile_bytes;
        bt_dma2(__builtin_amdgcn_readfirstlane(ring0 + stage * (8 * 4096)), g + oy, g + ox);
    }

    // phase A of the tile in ring slot `slot`, exchange buffer `buf`: this wavefront's gradient pair (formed, if YGEN) transposed into yt,
    // its activation pair transposed into the exchange buffer.  The selectors are re-made per tile instead of living in 8 registers next to
    // the accumulators and W^T: the kernel spilled into its loop, and scratch loads drain the VM counter.
    __device__ __forceinline__ void phase_a(int slot, int buf, W4 (&yt)[2]) const {
        W4 sel0, sel1;
        bt_selectors<PREC, true>(n, h, sel0, sel1);
        char* rw = raw + (slot * 8 + wave) * 4096 + lane * 16;
        W4 y[2] = {*reinterpret_cast<const W4*>(rw), *reinterpret_cast<const W4*>(rw + 1024)};
        if constexpr (YGEN) {           // y = (gradient fragment of the layer above, this layer's ReLU bits) -> this wavefront's two fragments of G
            const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const f32x16 d = mfma_half<PREC>(w2, y[0], zero);
            // byte j of a lane's 16 mask bytes = the ReLU bits of fragment j (mlp_pipe.h mask_from_bits): fragments 2 w, 2 w + 1 are one half
            // of word w / 2 -- read as ONE dword (indexing the four words by the wavefront number would go through scratch)
            const unsigned mw = *reinterpret_cast<const unsigned*>(rw + 1024 + 4 * (wave >> 1)) >> (16 * (wave & 1));
            bt_frags<PREC>(d, y[0], y[1]);
#pragma unroll
            for (int f = 0; f < 2; ++f)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned two = (mw >> (8 * f + 2 * e)) & 3u;
                    y[f].w[e] &= ((0u - (two & 1u)) & 0xffffu) | ((0u - (two >> 1)) & 0xffff0000u);
                }
            *reinterpret_cast<W4*>(rw) = y[0];                 // where the dgrad of all eight wavefronts reads G (behind the next barrier)
            *reinterpret_cast<W4*>(rw + 1024) = y[1];
        }
        if (KD == 2 * RT_ - 1 && wave == RT_ - 1) y[1] = W4{{0u, 0u, 0u, 0u}};       // the last row tile is ONE fragment: what lies behind it in the store is not this layer's (0 x inf = nan)
        if (RT_ == 8 || yown) transpose_block<PREC>(y[0], y[1], sel0, sel1, yt);
        if (xown) {
            const W4 x0 = *reinterpret_cast<const W4*>(rw + 2048), x1 = *reinterpret_cast<const W4*>(rw + 3072);
            W4 xt[2];
            transpose_block<PREC>(x0, x1, sel0, sel1, xt);
            bt_xt_store(xs + buf * (CT * 2048), wave, lane, xt);
        }
    }

    __device__ __forceinline__ void products(int buf, const W4 (&yt)[2]) {
        if (!(RT_ == 8 || yown)) return;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            W4 xt[2];
            bt_xt_load(xs + buf * (CT * 2048), c, lane, xt);
            bt_prod<PREC>(acc[c], yt, xt);
        }
    }

    // d X tile `wave` of sample tile t = W^T rows . G: gradient fragment j sits in wavefront j / 2's ring slot, fragment j & 1
    __device__ __forceinline__ void dgrad(int slot, long t) const {
        if (!down) return;
        f32x16 d = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const char* gb = raw + (slot * 8) * 4096 + lane * 16;
        const char* rw = raw + (slot * 8 + wave) * 4096 + lane * 16;
#pragma unroll
        for (int j = 0; j < KD; ++j) {
            const W4 gj = *reinterpret_cast<const W4*>(gb + (j >> 1) * 4096 + (j & 1) * 1024);
            const W4 wj = j < KD - WL ? wt[j] : *reinterpret_cast<const W4*>(wl + (wave * WL + (j - (KD - WL))) * 1024 + lane * 16);
            d = mfma_half<PREC>(wj, gj, d);
        }
        W4 o[2];
        bt_frags<PREC>(d, o[0], o[1]);
        char* dst = fp.out_store + t * fp.w.tile_bytes + (long)(fp.out_slot + 2 * wave) * 1024 + lane * 16;
        // The ReLU pattern of the layer below = [its stored activation != 0], and the activation fragments 2 w, 2 w + 1 are the X operand
        // this wavefront fetched for its column tile: still in its ring slot.  (The separate dgrad kernel reads the bit-mask fragment; a
        // load of it here -- tracked by the compiler or not -- either drains the ring's prefetch or races with its own wait.)
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            if (OMASK != 0) bt_mask<PREC>(o[f], *reinterpret_cast<const W4*>(rw + 2048 + f * 1024));
            // (plain stores: the next launch reads these d X fragments at once; non-temporal measured 10.91 vs 10.89 ms per iteration, round 6)
            if (!(ROWS && wave < fp.rows_tiles)) *reinterpret_cast<W4*>(dst + f * 1024) = o[f];
        }
        if (ROWS && wave < fp.rows_tiles) {
            const long smp = t * 32 + n;
            if (smp < fp.nsamp) frag_pair_to_row<PREC>(o[0], o[1], fp.rows + smp * fp.rows_stride + 32 * wave, h, grad_scale(*fp.maxbits, true));
        }
    }

    // this wavefront's row of the workgroup's partial block set, NC blocks wide; returns where block c goes
    __device__ __forceinline__ float* store_partials(int NC) const {
        float* out = fp.w.partial + (((long)blockIdx.x * 8 + wave) * NC) * 1024 + lane * 16;
#pragma unroll
        for (int c = 0; c < CT; ++c) bt_put(out + c * 1024, acc[c]);
        return out;
    }
};

// The two-barrier schedule: [phase A] barrier [products, bias, dgrad] barrier.  The second barrier orders the ring: the DMA issued at the
// top of iteration i overwrites the slot every wavefront read G from in iteration i - 1.
template <int PREC, int CT, int TO, int OMASK, int RT_ = 8, int KD_ = 16, bool YGEN = false, bool ROWS = false>
__global__ __launch_bounds__(WGRAD_NT) void k_wgrad_dgrad(const WgradFusedParams fp) {
    extern __shared__ __attribute__((aligned(16))) char wsm[];
    FusedLayer<PREC, CT, TO, OMASK, RT_, KD_, YGEN, ROWS, FUSED_WL, 1> L(fp, wsm);
    const WgradParams& p = fp.w;
    const bool bias_own = p.bias != 0 && L.yown;
    f32x16 accb;
#pragma unroll
    for (int i = 0; i < 16; ++i) accb[i] = 0.f;
    const long stride = gridDim.x;
    long t = blockIdx.x;
#pragma unroll
    for (int k = 0; k < WG_RING - 1; ++k) L.issue(t + k * stride, k);
    for (int it = 0; t < p.tiles; t += stride, ++it) {
        L.issue(t + (WG_RING - 1) * stride, (it + WG_RING - 1) % WG_RING);
        bt_ring_wait((t + stride < p.tiles ? 1 : 0) + (t + 2 * stride < p.tiles ? 1 : 0));
        W4 yt[2];
        L.phase_a(it % WG_RING, 0, yt);
        __syncthreads();
        L.products(0, yt);
        if (bias_own) bt_bias<PREC, true>(accb, yt, L.n, 0);       // (the column of ones re-made per tile, like the selectors)
        L.dgrad(it % WG_RING, t);
        __syncthreads();            // every wavefront is done with this tile's ring slots before any of them issues into the oldest one
    }
    if (RT_ < 8 && !L.yown) return;           // (the reduce reads RT_ row tiles of every workgroup's 8-tile set: WreduceParams::part_stride)
    float* out = L.store_partials(CT + (p.bias ? 1 : 0));
    if (bias_own) bt_put(out + CT * 1024, accb);
}

// k_wgrad_dgrad_p (round 6): the same launch for a layer WITHOUT a bias gradient (the PDRF levels of every shipped config:
// rgb_add_bias off, sigma_net has none), software-pipelined by one tile with ONE barrier per tile.
// The stamps of k_wgrad_dgrad (profiles/r05_wgrad_dgrad_stamps.log) show a tile as: [transposes, exchange write: 19-27 %] barrier [products:
// MFMA-bound] [dgrad: MFMA-bound] barrier -- all eight wavefronts in the same phase at the same time, so the two wavefronts of a SIMD fight
// for the matrix pipe in the product phases and leave it idle in the others (the pipe is busy 28-39 %).  Here
//   * the transposed activation blocks are double-buffered and the DMA for tile t + 2 is issued BEHIND the tile's barrier: the barrier at the
//     top of tile t proves that every wavefront has left tile t - 1, which is what both the ring slot and the exchange buffer wait for -- the
//     second barrier is gone;
//   * phase A of tile t + 1 (gradient forming, both transposes, exchange write) runs INSIDE tile t, and the two halves of the workgroup take
//     it at different places: wavefronts 0-3 (one per SIMD) run products -> A -> dgrad, wavefronts 4-7 A -> products -> dgrad, so that a
//     SIMD's two wavefronts are in complementary phases (matrix pipe beside LDS / VALU work);
//   * no bias accumulator (FUSED_WL_P: 4 instead of 6 W^T fragments per wavefront in LDS: 32 KiB); LDS = 96 (ring) + 32 (exchange, CT = 8)
//     + 32 = 160 KiB.
template <int PREC, int CT, int TO, int OMASK, int RT_ = 8, int KD_ = 16, bool YGEN = false, bool ROWS = false>
__global__ __launch_bounds__(WGRAD_NT) void k_wgrad_dgrad_p(const WgradFusedParams fp) {
    extern __shared__ __attribute__((aligned(16))) char wsm[];
    FusedLayer<PREC, CT, TO, OMASK, RT_, KD_, YGEN, ROWS, FUSED_WL_P, 2> L(fp, wsm);
    const WgradParams& p = fp.w;
    const long stride = gridDim.x;
    long t = blockIdx.x;
    // prologue: tiles 0 and 1 in flight, phase A of tile 0
    L.issue(t, 0);
    L.issue(t + stride, 1);
    W4 yt[2] = {{{0u, 0u, 0u, 0u}}, {{0u, 0u, 0u, 0u}}};
    if (t < p.tiles) {
        bt_ring_wait(t + stride < p.tiles ? 1 : 0);
        L.phase_a(0, 0, yt);
    }
    for (int it = 0; t < p.tiles; t += stride, ++it) {
        __syncthreads();                // exchange buffer it & 1 and (YGEN) the formed gradient of tile `it` are complete; every wavefront has left tile it - 1
        L.issue(t + 2 * stride, (it + 2) % WG_RING);
        const bool has_next = t + stride < p.tiles;
        const int slot = it % WG_RING, nslot = (it + 1) % WG_RING, buf = it & 1;
        W4 ytn[2] = {{{0u, 0u, 0u, 0u}}, {{0u, 0u, 0u, 0u}}};
        // the DMA of tile it + 1 has landed when at most the four pieces of tile it + 2 (issued above) are outstanding; the stores of tile
        // it - 1 are older than those and complete with it
        // (each phase's code exists ONCE, in a two-trip loop whose trips a wavefront takes in its own order: with the two orders written out
        // hipcc spilled 130-150 registers beside the 128 accumulators + 48 registers of W^T)
#pragma unroll 1
        for (int ph = 0; ph < 2; ++ph) {
            const bool do_products = (L.wave < 4) == (ph == 0);
            if (do_products) {
                L.products(buf, yt);
            } else if (has_next) {
                bt_ring_wait(t + 2 * stride < p.tiles ? 1 : 0);
                L.phase_a(nslot, buf ^ 1, ytn);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        L.dgrad(slot, t);
        __builtin_amdgcn_sched_barrier(0);
        yt[0] = ytn[0];
        yt[1] = ytn[1];
    }
    if (RT_ < 8 && !L.yown) return;
    L.store_partials(CT);
}

template <int PREC, int CT, int TO, int OMASK, int RT_ = 8, int KD_ = 16, bool YGEN = false, bool ROWS = false>
static int launch_wgrad_dgrad(const WgradFusedParams& p, int blocks, hipStream_t st) {
    if (ROWS != (p.rows != nullptr)) return fail(EVD_E_INVALID, "k_wgrad_dgrad: the row output goes with the ROWS instantiation");
    // a layer without a bias gradient: the pipelined one-barrier form; the two-barrier kernel otherwise
    if (!p.w.bias && CT <= 5) {
        if constexpr (CT <= 5) {
            constexpr size_t ldsp = fused_lds_bytes(CT, 2, FUSED_WL_P);
            EVD_SET_MAX_LDS((&k_wgrad_dgrad_p<PREC, CT, TO, OMASK, RT_, KD_, YGEN, ROWS>), ldsp);
            hipLaunchKernelGGL((k_wgrad_dgrad_p<PREC, CT, TO, OMASK, RT_, KD_, YGEN, ROWS>), dim3(blocks), dim3(WGRAD_NT), ldsp, st, p);
            EVD_LAUNCH_CHECK();
            return EVD_OK;
        }
    }
    constexpr size_t lds = fused_lds_bytes(CT, 1, FUSED_WL);
    EVD_SET_MAX_LDS((&k_wgrad_dgrad<PREC, CT, TO, OMASK, RT_, KD_, YGEN, ROWS>), lds);
    hipLaunchKernelGGL((k_wgrad_dgrad<PREC, CT, TO, OMASK, RT_, KD_, YGEN, ROWS>), dim3(blocks), dim3(WGRAD_NT), lds, st, p);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // namespace evd
