// Training backward, one dgrad layer: d x = (W^T d y) . [x > 0] on the software pipeline of the forward kernel (mlp_pipe.h): W^T is the
// streamed A operand, the incoming gradient fragments are the B operand, the outgoing ones are multiplied by the ReLU pattern of the
// saved activation in the epilogue and stored.
#pragma once

#include "nerf_bwd_frags.h"

namespace evd {

struct DgradParams {
    const char* wstream;    // W^T as a fragment stream (pack.h), one layer
    char* store;
    long tile_bytes;        // stride of a 32-sample tile in the store
    int in_slot, extra_slot, mask_slot, out_slot;
    // optional: max |output| in true units (the loss scale behind *maxbits removed) -> atomicMax on *absmax_out (float bits), one per workgroup
    unsigned* absmax_out = nullptr;
    const unsigned* maxbits = nullptr;
};

// One dgrad layer: KTOT k-steps in (NIN contiguous fragments from in_slot, already masked by their producer, plus one more
// from extra_slot if EXTRA), TILES 32-row tiles out, multiplied by the ReLU pattern of the activation fragments at mask_slot
// (OMASK) before they are stored: what the next dgrad layer and the wgrad kernel read is d loss / d pre-activation.
// 8 wavefronts x 32 samples per workgroup.
template <int PREC, int KTOT, int TILES, int NIN, bool EXTRA, int OMASK, int NT>
__global__ __launch_bounds__(NT, NT / 256) void k_dgrad_layer(const DgradParams p) {
    typedef PipeCfg<PREC, 1, NT> C;
    typedef typename C::O O;
    typedef typename O::B B;
    typedef LayerDesc<KTOT, TILES, 1, false, false, 0, 0, true, 0, 0, 0, false, 0, -1, false, 0, 0, -1> L;
    constexpr int NCH = cceil(KTOT * TILES, C::FPC), FB = C::FB;
    static_assert(NIN + (EXTRA ? 1 : 0) == KTOT, "k-steps of the layer");    // (a layer shorter than the prefetch depth reads the zero padding of its chunk)
    extern __shared__ __attribute__((aligned(16))) char smem[];

    pipe_fp16_saturate<PREC>();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    PStream<C, true, NCH> st;
    st.start_issue(p.wstream, smem, tid);
    float* zb = reinterpret_cast<float*>(smem + C::RING);       // the dgrad layers have no bias: a block of zeros
    for (int i = tid; i < (TILES + 1) * 32; i += NT) zb[i] = 0.f;
    char* al = p.store + ((long)blockIdx.x * (NT / 64) + wave) * p.tile_bytes + lane * 16;

    B in[1][KTOT], out[1][2 * TILES], oma[OMASK == 1 ? 2 * TILES : 1];
    MaskFrag omb[1];
#pragma unroll
    for (int j = 0; j < NIN; ++j) in[0][j] = frag_load<B, FB>(al, p.in_slot + j);
    if constexpr (EXTRA) in[0][NIN] = frag_load<B, FB>(al, p.extra_slot);
    if constexpr (OMASK == 1) {
#pragma unroll
        for (int j = 0; j < 2 * TILES; ++j) oma[j] = frag_load<B, FB>(al, p.mask_slot + j);
    } else if constexpr (OMASK == 2) {
        omb[0] = frag_load<MaskFrag, FB>(al, p.mask_slot);          // the bit-mask fragment (nerf_mlp.h M_H0 ..)
    }
    const void* om = OMASK == 1 ? static_cast<const void*>(oma) : static_cast<const void*>(omb);
    char* actl[1] = {al + (long)p.out_slot * FB};
    float* nofrow[1] = {nullptr};
    Pipe<C> pp;
    st.start_wait();
    pipe_prime<C, L>(st, pp, zb, lane);
    pipe_layer<C, L, decltype(st), 2 * TILES, true, OMASK>(st, pp, in, out, nullptr, zb, lane, nofrow, actl, om);
    pipe_flush<C, L>(pp, out);
#pragma unroll
    for (int j = 2 * TILES - 2; j < 2 * TILES; ++j) {
        if constexpr (OMASK == 1) O::mask_act(out[0][j], oma[j]);
        else if constexpr (OMASK == 2) O::mask_bits(out[0][j], omb[0], j);
        act_store<FB>(actl[0], j, out[0][j]);
    }
    if constexpr (is_half_prec(PREC)) {
        if (p.absmax_out) {              // (what a separate pass over the stored fragments computed: k_frag_absmax, 110 us at 1.3 M samples x 128)
            float m = 0.f;
#pragma unroll
            for (int j = 0; j < 2 * TILES; ++j) {
                const W4 f = __builtin_bit_cast(W4, out[0][j]);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float v = half_value<PREC>(f.w[e >> 1], e & 1);
                    m = v != v ? __builtin_huge_valf() : fmaxf(m, fabsf(v));          // (a NaN is recorded as +inf, like k_awp_bwd_fused and k_mam_local_bwd)
                }
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
            __syncthreads();             // (the ring is not read any more: its first words carry the wavefronts' maxima)
            float* part = reinterpret_cast<float*>(smem);
            if (lane == 0) part[wave] = m;
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < NT / 64; ++w) m = fmaxf(m, part[w]);
                // (thousands of atomicMax on one word serialise at the L2 -- 75 -> 309 us for this launch --: only a workgroup that would raise
                // the word as it reads it now sends one; positive floats order like their bit patterns)
                const unsigned mb = __float_as_uint(m * grad_scale(*p.maxbits, true));
                if (m > 0.f && mb > *reinterpret_cast<volatile unsigned*>(p.absmax_out)) atomicMax(p.absmax_out, mb);
            }
        }
    }
}

template <int PREC, int KTOT, int TILES, int NIN, bool EXTRA, int OMASK>
static int launch_dgrad(const DgradParams& p, long tiles, hipStream_t st) {
    constexpr int NT = is_half_prec(PREC) ? 512 : 256;          // the split mode's fragments need the whole register file: one wavefront per SIMD
    typedef PipeCfg<PREC, 1, NT> C;
    const size_t lds = C::RING + (TILES + 1) * 128;
    EVD_SET_MAX_LDS((&k_dgrad_layer<PREC, KTOT, TILES, NIN, EXTRA, OMASK, NT>), lds);
    hipLaunchKernelGGL((k_dgrad_layer<PREC, KTOT, TILES, NIN, EXTRA, OMASK, NT>), dim3((unsigned)(tiles / (NT / 64))), dim3(NT), lds, st, p);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // namespace evd
