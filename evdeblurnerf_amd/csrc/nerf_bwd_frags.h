// Training backward, gradient fragments and loss scale: the power-of-two loss scale (grad_scale, k_absmax), d raw -> the gradient fragments
// of the output heads (k_grad_frags), stored fragments read back (frag_load, frag_values), and the gradient of a positional encoding from
// its gradient fragments (k_pe_bwd).  Slots: nerf_mlp.h, namespace astore.
#pragma once

#include "bwd_tile.h"
#include "nerf_train.h"

namespace evd {

// 2^s with max * 2^s in [512, 1024); `bits` = float bits of max |d raw| (0: no gradient at all)
__device__ __forceinline__ float grad_scale(unsigned bits, bool inverse) {
    const float m = __uint_as_float(bits);
    if (!(m > 0.f) || !(m < 3.0e38f)) return 1.f;
    int e;
    (void)frexpf(m, &e);                                 // m = f 2^e, f in [0.5, 1)
    return ldexpf(1.f, inverse ? e - 10 : 10 - e);
}

static __global__ __launch_bounds__(256) void k_absmax(const float* __restrict__ x, long n, unsigned* __restrict__ out) {
    __shared__ float part[4];
    float m = 0.f;
    const long n4 = n >> 2, stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {          // float4 body (the gradient rows are 16-byte aligned)
        const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
    }
    for (long i = 4 * n4 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) m = fmaxf(m, fabsf(x[i]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    // one atomic per block: thousands of same-address atomicMax (one per wavefront, as first written) serialise at the L2 and cost
    // more than the read of the whole array
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
        if (m > 0.f) atomicMax(out, __float_as_uint(m));
    }
}

template <int PREC>
__global__ __launch_bounds__(256) void k_grad_frags(const float* __restrict__ d_raw, long nsamp, const unsigned* __restrict__ maxbits,
                                                    char* __restrict__ store, long tiles) {
    typedef POps<PREC> O;
    typedef typename O::B B;
    pipe_fp16_saturate<PREC>();
    const long idx = (long)blockIdx.x * 256 + threadIdx.x, tile = idx >> 6;
    if (tile >= tiles) return;
    const int lane = idx & 63, n = lane & 31, h = lane >> 5;
    const long smp = tile * 32 + n;
    const float s = grad_scale(*maxbits, false);
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    if (h == 0 && smp < nsamp) g = *reinterpret_cast<const f32x4*>(d_raw + smp * 4);
    B rgb, al;
    O::zero(rgb);
    O::zero(al);
    O::template set_pair<false>(rgb, 0, g[0] * s, g[1] * s);
    O::template set_pair<false>(rgb, 1, g[2] * s, 0.f);
    O::template set_pair<false>(al, 0, g[3] * s, 0.f);
    constexpr int FB = frag_bytes(PREC);
    char* a = store + tile * astore::tile_bytes(PREC) + lane * 16;
    act_store<FB>(a, astore::G_RGB, rgb);
    act_store<FB>(a, astore::G_ALPHA, al);
}

template <class B, int FB = 1024> __device__ __forceinline__ B frag_load(const char* lane_base, int slot) {
    static_assert(sizeof(B) == 16 || (sizeof(B) == 32 && FB == 2048), "16-byte fragments, or hi / lo pairs in 2 KiB slots");
    if constexpr (sizeof(B) == 16) {
        return __builtin_bit_cast(B, *reinterpret_cast<const f32x4*>(lane_base + (long)slot * FB));
    } else {
        struct Two { f32x4 a, b; };
        Two t;
        t.a = *reinterpret_cast<const f32x4*>(lane_base + (long)slot * FB);
        t.b = *reinterpret_cast<const f32x4*>(lane_base + (long)slot * FB + 1024);
        return __builtin_bit_cast(B, t);
    }
}

// the 8 values of one lane of a stored fragment as float32 (split mode: hi + lo / 2048)
template <int PREC> __device__ __forceinline__ void frag_values(const char* lane_base, int slot, float (&v)[8]) {
    constexpr int FB = frag_bytes(PREC);
    const MaskFrag f = frag_load<MaskFrag, FB>(lane_base, slot);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = half_value<PREC>(f.w[e >> 1], e & 1);
    if constexpr (PREC == EVD_PREC_F16X3) {
        const MaskFrag l = __builtin_bit_cast(MaskFrag, *reinterpret_cast<const f32x4*>(lane_base + (long)slot * FB + 1024));
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaf(half_value<PREC>(l.w[e >> 1], e & 1), 4.8828125e-4f, v[e]);
    }
}

// Gradient of a positional encoding (embedding.py:88-98) from its gradient fragments (KSN fragments at `slot`, the encoding's own
// arrangement: position q = 8 j + e holds, for q < 3 L, d sin (lane half 0) / d cos (half 1) of x_{q % 3} 2^{q / 3}; q = 3 L:
// (d x_0 | d x_1); q = 3 L + 1: (d x_2 | -)) -> d x rows [n, 3] float32, loss scale removed.  x: rows of x_stride floats,
// one per `per` samples (1: points; S: the ray's view direction).
template <int PREC, int L, int KSN>
__global__ __launch_bounds__(256) void k_pe_bwd(const char* __restrict__ store, long tile_bytes, int slot, long nsamp, const float* __restrict__ x,
                                                int x_stride, int per, const unsigned* __restrict__ maxbits, float* __restrict__ dx, int accumulate) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x, tile = idx >> 6;
    const int lane = idx & 63, n = lane & 31, h = lane >> 5;
    const long smp = tile * 32 + n;
    if (tile * 32 >= nsamp) return;
    const long sc = smp < nsamp ? smp : nsamp - 1;
    float xv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) xv[c] = x[(sc / per) * x_stride + c];
    float g[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < KSN; ++j) {
        float fv[8];
        frag_values<PREC>(store + tile * tile_bytes + lane * 16, slot + j, fv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int q = 8 * j + e;
            const float v = fv[e];
            if (q < 3 * L) {
                const float fr = (float)(1 << (q / 3)), a = xv[q % 3] * fr;
                // d sin = cos, d cos = -sin.  The half-precision modes take them from the hardware unit, as their forward does (sin_or_cos_hw:
                // absolute error ~2^-20 against gradient fragments rounded at 2^-11; libm's cosf / sinf with their range reduction were 57 M VALU
                // instructions per launch -- profiles/r05_pmc_train_step.txt --, the float32-grade mode keeps them)
                const float tr = POps<PREC>::kFastTrig ? sin_or_cos_hw(a, h == 0 ? 1 : 0) : (h == 0 ? cosf(a) : sinf(a));
                g[q % 3] += h == 0 ? v * tr * fr : -v * tr * fr;
            } else if (q == 3 * L) {
                g[h] += v;                       // (x_0 | x_1)
            } else if (q == 3 * L + 1 && h == 0) {
                g[2] += v;
            }
        }
    }
    const float inv = grad_scale(*maxbits, true);
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = (g[c] + __shfl_xor(g[c], 32)) * inv;
    if (h == 0 && smp < nsamp) {
#pragma unroll
        for (int c = 0; c < 3; ++c) dx[smp * 3 + c] = accumulate ? dx[smp * 3 + c] + g[c] : g[c];
    }
}

}  // namespace evd
