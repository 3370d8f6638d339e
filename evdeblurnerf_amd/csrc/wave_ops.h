// Wave-level and row-level primitives (64-wide wavefronts) and the fast activations of the compositing scan (kernels_composite.hip); the
// loss, AWP-scan, MAM, AWP-tail and voxel kernels share the DPP scans and sums.
//
// Two families.  They associate the 64 terms differently, so a kernel that moves from one to the other changes the last bits of its sums:
//   shuffle (__shfl_*, an LDS crossbar round trip per step): float64 values, which DPP does not move in one instruction, integer flag
//            words, and the kernels that are not bound by the reduction (k_composite, k_points_bwd, k_sample_pdf_merge, k_numerics_flags)
//   DPP     (lane exchange inside the VALU): the float32 scans and sums of the bandwidth-bound kernels
#pragma once

#include "evd_common.h"

namespace evd {

constexpr int WAVE = 64;

// ------------------------------------------------------------------------------------------------
// shuffle family: butterfly sums (the result in every lane) and Hillis-Steele inclusive scans
template <class T>                       // float or double
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}
// maximum over the 64 lanes
__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// bitwise OR over the 64 lanes
__device__ __forceinline__ unsigned wave_or(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off, WAVE);
    return v;
}
// inclusive product scan over the 64 lanes
__device__ __forceinline__ float wave_scan_mul(float v, int lane) {
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        float o = __shfl_up(v, off, WAVE);
        if (lane >= off) v *= o;
    }
    return v;
}
__device__ __forceinline__ double wave_scan_add_d(double v, int lane) {
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        double o = __shfl_up(v, off, WAVE);
        if (lane >= off) v += o;
    }
    return v;
}

// ------------------------------------------------------------------------------------------------
// DPP (data-parallel primitive) wave operations: register-to-register lane exchange inside the VALU, no LDS
// crossbar round trip (which is what __shfl / ds_bpermute costs).  dpp_ctrl codes: quad_perm 0x00-0xFF,
// row_shr:n 0x110+n, wave_shl:1 0x130, wave_shr:1 0x138, row_mirror 0x140, row_half_mirror 0x141,
// row_bcast:15 0x142, row_bcast:31 0x143 (gfx9 family).
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp_f32(float old, float src) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src), CTRL, ROW_MASK, 0xf, false));
}
// inclusive product scan over the 64 lanes (Kogge-Stone inside rows of 16, then row broadcasts)
__device__ __forceinline__ float wave_scan_mul_dpp(float v) {
    v *= dpp_f32<0x111>(1.f, v);
    v *= dpp_f32<0x112>(1.f, v);
    v *= dpp_f32<0x114>(1.f, v);
    v *= dpp_f32<0x118>(1.f, v);
    v *= dpp_f32<0x142, 0xa>(1.f, v);     // rows 1, 3 <- lane 15 of the row below
    v *= dpp_f32<0x143, 0xc>(1.f, v);     // rows 2, 3 <- lane 31
    return v;
}
// inclusive sum scan over the 64 lanes
__device__ __forceinline__ float wave_scan_add_dpp(float v) {
    v += dpp_f32<0x111>(0.f, v);
    v += dpp_f32<0x112>(0.f, v);
    v += dpp_f32<0x114>(0.f, v);
    v += dpp_f32<0x118>(0.f, v);
    v += dpp_f32<0x142, 0xa>(0.f, v);
    v += dpp_f32<0x143, 0xc>(0.f, v);
    return v;
}
// inclusive product over the lanes <= this one of the 16-lane DPP row
__device__ __forceinline__ float row_scan_mul_dpp(float v) {
    v *= dpp_f32<0x111>(1.f, v);
    v *= dpp_f32<0x112>(1.f, v);
    v *= dpp_f32<0x114>(1.f, v);
    v *= dpp_f32<0x118>(1.f, v);
    return v;
}
// inclusive sum over the lanes >= this one of the row (row_shl:n 0x100+n)
__device__ __forceinline__ float row_scan_add_right_dpp(float v) {
    v += dpp_f32<0x101>(0.f, v);
    v += dpp_f32<0x102>(0.f, v);
    v += dpp_f32<0x104>(0.f, v);
    v += dpp_f32<0x108>(0.f, v);
    return v;
}
// sum over the 16 lanes of a row, left in every lane of the row (lanes that are switched off contribute 0)
__device__ __forceinline__ float row_sum_dpp(float v) {
    v += dpp_f32<0xb1>(0.f, v);           // quad_perm [1,0,3,2]
    v += dpp_f32<0x4e>(0.f, v);           // quad_perm [2,3,0,1]
    v += dpp_f32<0x141>(0.f, v);          // row_half_mirror
    v += dpp_f32<0x140>(0.f, v);          // row_mirror
    return v;
}
// sum over the 64 lanes, result uniform (in an SGPR-backed value)
__device__ __forceinline__ float wave_sum_dpp(float v) {
    v = row_sum_dpp(v);
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0)) +
           __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16)) +
           __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32)) +
           __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
}
// sum over the 64 lanes, valid in LANE 63 only (row sums, then the two row broadcasts of the scan): 6 DPP adds, no readlane
__device__ __forceinline__ float wave_sum_to63(float v) {
    v = row_sum_dpp(v);
    v += dpp_f32<0x142, 0xa>(0.f, v);
    v += dpp_f32<0x143, 0xc>(0.f, v);
    return v;
}

// e^x on the hardware exp2 (v_exp_f32, 1 ulp) behind one multiply: relative error <= 1e-6 for |x| <= 16 against ~20 instructions of the
// IEEE expf -- the AWP scans evaluate one exponential per (sample, channel) and were bound by the instruction count, not by HBM
__device__ __forceinline__ float exp_fast(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

// activations of the bandwidth-form scan: sigmoid with the hardware exp2 and reciprocal (relative error ~3e-7; the
// IEEE expf + division of evd::act() made the scan VALU-bound: 3.8 instead of 5.2 TB/s)
__device__ __forceinline__ float act_fast(int code, float x) {
    if (code == EVD_ACT_SIGMOID) return __builtin_amdgcn_rcpf(1.f + __expf(-x));
    if (code == EVD_ACT_RELU) return x > 0.f ? x : (x == x ? 0.f : x);     // NaN propagates, as in act() and torch.relu
    if (code == EVD_ACT_NONE) return x;
    return act(code, x);
}

}  // namespace evd
