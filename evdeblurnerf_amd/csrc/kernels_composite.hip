// raw2outputs: the alpha-compositing scan of the render path and its backward (reference networks/nerf.py:74-129,
// networks/pdrf/voxnerf.py:153-201): density on the first S-1 samples, last alpha forced to 1, T = exclusive cumprod(1 - alpha) as a
// wavefront product scan.  HBM-bound: reads raw (4C B) + z (4 B), writes weights (4 B) per sample.  The ray front end is in
// kernels_rays.hip, the resampling that consumes the weights in kernels_sample_pdf.hip.
//
//   kernel                 serves                                      a lane owns            activation  exp
//   k_composite            any channel count / layout, any S           sample l of each 64    act         expf     as torch evaluates them
//   k_composite_rows       C == 4, S <= 256                            SPL consecutive ones   act_fast    expf     act() made it VALU-bound (wave_ops.h)
//   k_composite_il         C == 4, S <= 256, the renderer's layouts    l, 64 + l, ...         act_fast    __expf   hardware exp2: |error of alpha| <= 1e-7
//   k_composite_rows_bwd   backward of the C == 4 forms                SPL consecutive ones   act         expf     recomputes k_composite's values
//   k_composite_feat_bwd   backward of the G-channel feature composite SPL consecutive ones   act         expf     (+ the [S, G] row block in contiguous pieces)
//   k_weighted_channels    sum_s w x: colour maps with n_rgb != 3, feature maps
//
// The arithmetic of a sample inside the row is written once (composite_dist, composite_density, composite_alpha).  What a form does to
// memory around it -- the raw noise it adds, the density it returns -- stays in the kernel: a helper that holds those accesses changes the
// code of k_composite_il and k_composite_rows (SPL 3: 71 -> 73 VGPRs, 7 -> 6 waves); so does a shared transmittance scan of the row forms.
// Row end: k_composite and the row forms branch on i < S - 1 around the step; k_composite_il runs it in every lane (the next z comes by
// DPP, the activations are template constants), guards only the noise / density accesses and selects the forced alpha in the last chunk
// alone; it has no rmnear (the dispatch keeps such calls away).  Noise: the forward forms add it under `if (noise)`, the backward adds 0.f
// where there is none -- that differs only in the sign of a zero raw density, which no activation tells apart.
#include "ray_math.h"
#include "wave_ops.h"

namespace evd {

constexpr bool ACT_IEEE = false, ACT_FAST = true, EXP_IEEE = false, EXP_HW = true;

// One sample inside the row (nerf.py:106-112, voxnerf.py:171-183), z and zn its depth and the next one's:
//   dist = (zn - z) |d|,   density = act(raw + noise), 0 where zn <= rmnear (if rmnear > 0),   alpha = 1 - exp(-density dist)
__device__ __forceinline__ float composite_dist(float z, float zn, float norm) { return __fmul_rn(__fsub_rn(zn, z), norm); }
__device__ __forceinline__ float rmnear_mask(float zn, float rmnear) { return zn > rmnear ? 1.f : 0.f; }
template <bool FAST>
__device__ __forceinline__ float composite_density(int sigma_act, float sraw, float zn, float rmnear) {
    float dens = FAST ? act_fast(sigma_act, sraw) : act(sigma_act, sraw);
    if (rmnear > 0.f) dens = rmnear_mask(zn, rmnear) * dens;
    return dens;
}
template <bool HW>
__device__ __forceinline__ float composite_alpha(float dens, float dist) {
    return __fadd_rn(-(HW ? __expf(-__fmul_rn(dens, dist)) : expf(-__fmul_rn(dens, dist))), 1.f);
}

// what one lane of the three-channel forms writes per ray: acc, depth and the colour map (on a white background the missing opacity is
// added to every channel)
__device__ __forceinline__ void composite_write_ray3(long r, float a_sum, float d_sum, float c0, float c1, float c2, int white_bkgd,
                                                     float* out_map, float* acc, float* depth) {
    if (acc) acc[r] = a_sum;
    if (depth) depth[r] = d_sum;
    if (out_map) {
        const float bg = white_bkgd ? 1.f - a_sum : 0.f;
        out_map[r * 3] = white_bkgd ? c0 + bg : c0;
        out_map[r * 3 + 1] = white_bkgd ? c1 + bg : c1;
        out_map[r * 3 + 2] = white_bkgd ? c2 + bg : c2;
    }
}

template <int NRGB>
__global__ __launch_bounds__(256) void k_composite(const float* __restrict__ raw, const float* __restrict__ z,
                                                   const float* __restrict__ rays_d, int rd_stride, long R, int S, int C,
                                                   int sigma_ch, int rgb_ch0, int n_rgb, int rgb_act, int sigma_act,
                                                   int white_bkgd, float rmnear, const float* __restrict__ noise,
                                                   float* __restrict__ out_map, float* __restrict__ density,
                                                   float* __restrict__ acc, float* __restrict__ weights,
                                                   float* __restrict__ depth) {
    const int lane = threadIdx.x & 63;
    const long r = blockIdx.x * (long)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= R) return;
    const float norm = ray_norm(rays_d + r * rd_stride);
    const float* rw = raw + r * (long)S * C;
    const float* zz = z + r * (long)S;
    float carry = 1.f, a_sum = 0.f, d_sum = 0.f;
    float csum[NRGB > 0 ? NRGB : 1];
#pragma unroll
    for (int c = 0; c < NRGB; ++c) csum[c] = 0.f;
    for (int base = 0; base < S; base += 64) {
        const int i = base + lane;
        const bool valid = i < S;
        float alpha = 0.f, zi = 0.f;
        float rgbv[NRGB > 0 ? NRGB : 1];
        if (valid) {
            zi = zz[i];
            float sraw;
            if (NRGB == 3 && C == 4) {   // fast path: one 16-byte load per sample
                const float4 v = reinterpret_cast<const float4*>(rw)[i];
                const float vv[4] = {v.x, v.y, v.z, v.w};
                sraw = vv[sigma_ch];
#pragma unroll
                for (int c = 0; c < NRGB; ++c) rgbv[c] = vv[rgb_ch0 + c];
            } else {
                sraw = rw[(long)i * C + sigma_ch];
#pragma unroll
                for (int c = 0; c < NRGB; ++c) rgbv[c] = rw[(long)i * C + rgb_ch0 + c];
            }
            if (i < S - 1) {
                const float dist = composite_dist(zi, zz[i + 1], norm);
                if (noise) sraw = __fadd_rn(sraw, noise[r * (long)(S - 1) + i]);
                const float dens = composite_density<ACT_IEEE>(sigma_act, sraw, zz[i + 1], rmnear);
                if (density) density[r * (long)(S - 1) + i] = dens;
                alpha = composite_alpha<EXP_IEEE>(dens, dist);
            } else {
                alpha = 1.f;
            }
        }
        const float om = valid ? __fadd_rn(-alpha, 1.f) : 1.f;
        const float incl = wave_scan_mul(om, lane);
        float excl = __shfl_up(incl, 1, WAVE);
        if (lane == 0) excl = 1.f;
        const float T = carry * excl;
        const float w = valid ? alpha * T : 0.f;
        carry *= __shfl(incl, 63, WAVE);
        if (valid && weights) weights[r * (long)S + i] = w;
        a_sum += w;
        d_sum += w * zi;
#pragma unroll
        for (int c = 0; c < NRGB; ++c) csum[c] += valid ? w * act(rgb_act, rgbv[c]) : 0.f;
    }
    a_sum = wave_sum(a_sum);
    d_sum = wave_sum(d_sum);
#pragma unroll
    for (int c = 0; c < NRGB; ++c) csum[c] = wave_sum(csum[c]);
    if (lane == 0) {
        if (acc) acc[r] = a_sum;
        if (depth) depth[r] = d_sum;
        if (out_map) {
#pragma unroll
            for (int c = 0; c < NRGB; ++c) out_map[r * n_rgb + c] = white_bkgd ? csum[c] + (1.f - a_sum) : csum[c];
        }
    }
}

// raw2outputs, bandwidth form (C == 4, three colour channels, S <= 64 * SPL): one wavefront per ray, every lane owns
// SPL CONSECUTIVE samples, so all of a ray's loads (SPL float4 of raw + SPL floats of z per lane, 2.5 KiB per
// wavefront at S = 128) are issued before the first dependent instruction.
template <int SPL, int RPW>
__global__ __launch_bounds__(256) void k_composite_rows(const float* __restrict__ raw, const float* __restrict__ z,
                                                        const float* __restrict__ rays_d, int rd_stride, long R, int S,
                                                        int sigma_ch, int rgb_ch0, int rgb_act, int sigma_act, int white_bkgd,
                                                        float rmnear, const float* __restrict__ noise,
                                                        float* __restrict__ out_map, float* __restrict__ density,
                                                        float* __restrict__ acc, float* __restrict__ weights, float* __restrict__ depth) {
    const int lane = threadIdx.x & 63;
    const long r0 = (blockIdx.x * (long)(blockDim.x >> 6) + (threadIdx.x >> 6)) * RPW;   // RPW consecutive rays per wavefront
    if (r0 >= R) return;
    const int i0 = lane * SPL;
    float4 v[RPW][SPL];
    float zi[RPW][SPL + 1];
    float dd[RPW][3];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {             // every load of the wavefront's rays first
        const long r = min(r0 + q, R - 1);
        const float4* rw = reinterpret_cast<const float4*>(raw + r * (long)S * 4);
        const float* zz = z + r * (long)S;
#pragma unroll
        for (int j = 0; j < SPL; ++j) {
            const int i = min(i0 + j, S - 1);
            v[q][j] = rw[i];
            zi[q][j] = zz[i];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) dd[q][c] = rays_d[r * rd_stride + c];
    }
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        const long r = r0 + q;
        if (r >= R) break;
        const float norm = ray_norm(dd[q]);
        zi[q][SPL] = dpp_f32<0x130>(0.f, zi[q][0]);          // wave_shl:1 -- the next lane's first z
        float alpha[SPL], om[SPL];
#pragma unroll
        for (int j = 0; j < SPL; ++j) {
            const int i = i0 + j;
            const float vv[4] = {v[q][j].x, v[q][j].y, v[q][j].z, v[q][j].w};
            float sraw = vv[sigma_ch];
            if (i < S - 1) {
                const float dist = composite_dist(zi[q][j], zi[q][j + 1], norm);
                if (noise) sraw = __fadd_rn(sraw, noise[r * (long)(S - 1) + i]);
                const float dens = composite_density<ACT_FAST>(sigma_act, sraw, zi[q][j + 1], rmnear);
                if (density) density[r * (long)(S - 1) + i] = dens;
                alpha[j] = composite_alpha<EXP_IEEE>(dens, dist);
            } else {
                alpha[j] = i == S - 1 ? 1.f : 0.f;     // last sample: alpha forced to 1 (nerf.py:113-114); beyond S: nothing
            }
            om[j] = i < S ? __fadd_rn(-alpha[j], 1.f) : 1.f;
        }
        float local = om[0];
#pragma unroll
        for (int j = 1; j < SPL; ++j) local *= om[j];
        const float incl = wave_scan_mul_dpp(local);
        float T = dpp_f32<0x138>(1.f, incl);           // wave_shr:1 -> exclusive product; lane 0 keeps 1
        float a_sum = 0.f, d_sum = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
        float w[SPL];
#pragma unroll
        for (int j = 0; j < SPL; ++j) {
            const float vv[4] = {v[q][j].x, v[q][j].y, v[q][j].z, v[q][j].w};
            w[j] = (i0 + j < S) ? alpha[j] * T : 0.f;
            T *= om[j];
            a_sum += w[j];
            d_sum += w[j] * zi[q][j];
            c0 += w[j] * act_fast(rgb_act, vv[rgb_ch0]);
            c1 += w[j] * act_fast(rgb_act, vv[rgb_ch0 + 1]);
            c2 += w[j] * act_fast(rgb_act, vv[rgb_ch0 + 2]);
        }
        if (weights) {
            float* wo = weights + r * (long)S + i0;
            if (SPL == 2 && (S & 1) == 0) {
                if (i0 < S) *reinterpret_cast<float2*>(wo) = make_float2(w[0], w[1]);
            } else if (SPL == 4 && (S & 3) == 0) {
                if (i0 < S) *reinterpret_cast<float4*>(wo) = make_float4(w[0], w[1], w[2], w[3]);
            } else {
#pragma unroll
                for (int j = 0; j < SPL; ++j) if (i0 + j < S) wo[j] = w[j];
            }
        }
        a_sum = wave_sum_dpp(a_sum);
        d_sum = wave_sum_dpp(d_sum);
        c0 = wave_sum_dpp(c0);
        c1 = wave_sum_dpp(c1);
        c2 = wave_sum_dpp(c2);
        if (lane == 0) composite_write_ray3(r, a_sum, d_sum, c0, c1, c2, white_bkgd, out_map, acc, depth);
    }
}

typedef float cs_f4 __attribute__((ext_vector_type(4)));     // native vectors: the non-temporal builtins do not take HIP's float4 / float2

// raw2outputs, interleaved form: lane l owns samples l, 64 + l, ... (NCH chunks of 64), so that every load / store instruction
// of the wavefront covers ONE contiguous run (k_composite_rows' lane owns consecutive samples: its 16-byte loads are 32 B apart and every
// 128-byte line is requested by two instructions).  The transmittance is one DPP product scan per chunk with the running product carried
// across chunks; channel layout and activations are template constants (k_composite_rows selects them at run time: a select chain per
// dynamic register index and a switch per activation).  All loads of the wavefront's RPW rays are issued before the first dependent
// instruction; the streamed raw / z / weights rows move with non-temporal accesses (NT).  A persistent form with the next group's loads
// in flight under the current group's arithmetic (k_composite_stream) measured 0.55 of 8 TB/s against 0.64 (rows) and 0.72 (this): removed.
template <int NCH, int RPW, int SIGMA_CH, int RGB_ACT, int SIGMA_ACT, bool NT>
__global__ __launch_bounds__(256) void k_composite_il(const float* __restrict__ raw, const float* __restrict__ z,
                                                      const float* __restrict__ rays_d, int rd_stride, long R, int S, int white_bkgd,
                                                      float* __restrict__ out_map, float* __restrict__ acc, float* __restrict__ weights,
                                                      float* __restrict__ depth, const float* __restrict__ noise, float* __restrict__ density) {
    constexpr int RGB0 = SIGMA_CH == 0 ? 1 : 0;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);              // scalar: the ray index and every row base stay in SGPRs
    const long r0 = (blockIdx.x * (long)(blockDim.x >> 6) + wave) * RPW;
    if (r0 >= R) return;
    cs_f4 v[RPW][NCH];
    float zi[RPW][NCH];
    float dd[RPW][3];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        const long r = min(r0 + q, R - 1);
        const cs_f4* rw = reinterpret_cast<const cs_f4*>(raw + r * (long)S * 4);
        const float* zz = z + r * (long)S;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int i = c + 1 < NCH ? c * 64 + lane : min(c * 64 + lane, S - 1);     // only the last chunk can run past the row
            v[q][c] = NT ? __builtin_nontemporal_load(rw + i) : rw[i];
            zi[q][c] = NT ? __builtin_nontemporal_load(zz + i) : zz[i];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) dd[q][c] = rays_d[r * rd_stride + c];
    }
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        const long r = r0 + q;
        if (r >= R) break;
        const float norm = ray_norm(dd[q]);
        float carry = 1.f, a_sum = 0.f, d_sum = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int i = c * 64 + lane;
            // the next sample's z: the next lane's, and for lane 63 the next chunk's lane 0
            const float z_up = c + 1 < NCH ? __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, zi[q][c + 1 < NCH ? c + 1 : 0]))) : 0.f;
            const float zn = dpp_f32<0x130>(z_up, zi[q][c]);              // wave_shl:1, lane 63 keeps `old`
            const cs_f4 v4 = v[q][c];
            // noise / density: the training node's optional extras (nerf.py:106-111 raw noise; the activated density it returns)
            float sraw = SIGMA_CH == 0 ? v4.x : v4.w;
            const float dist = composite_dist(zi[q][c], zn, norm);
            if (noise && i < S - 1) sraw = __fadd_rn(sraw, noise[r * (long)(S - 1) + i]);
            const float dens = composite_density<ACT_FAST>(SIGMA_ACT, sraw, zn, 0.f);
            if (density && i < S - 1) density[r * (long)(S - 1) + i] = dens;
            float alpha = composite_alpha<EXP_HW>(dens, dist);
            float om = __fadd_rn(-alpha, 1.f);
            if (c + 1 == NCH) {                                           // the row's last sample (alpha forced to 1, nerf.py:113-114) and the lanes behind it
                alpha = i < S - 1 ? alpha : (i == S - 1 ? 1.f : 0.f);
                om = i < S - 1 ? om : (i == S - 1 ? 0.f : 1.f);
            }
            const float incl = wave_scan_mul_dpp(om);
            const float T = carry * dpp_f32<0x138>(1.f, incl);            // wave_shr:1 -> exclusive product; lane 0 keeps 1
            if (c + 1 < NCH) carry *= __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, incl), 63));
            const float w = alpha * T;                                    // (alpha = 0 behind the row's end)
            if (weights && (c + 1 < NCH || i < S)) {
                float* wo = weights + r * (long)S + i;
                if (NT) __builtin_nontemporal_store(w, wo); else *wo = w;
            }
            a_sum += w;
            d_sum += w * zi[q][c];
            c0 += w * act_fast(RGB_ACT, RGB0 ? v4.y : v4.x);
            c1 += w * act_fast(RGB_ACT, RGB0 ? v4.z : v4.y);
            c2 += w * act_fast(RGB_ACT, RGB0 ? v4.w : v4.z);
        }
        a_sum = wave_sum_to63(a_sum);
        d_sum = wave_sum_to63(d_sum);
        c0 = wave_sum_to63(c0);
        c1 = wave_sum_to63(c1);
        c2 = wave_sum_to63(c2);
        if (lane == 63) composite_write_ray3(r, a_sum, d_sum, c0, c1, c2, white_bkgd, out_map, acc, depth);
    }
}

// derivative of evd::act / act_fast at x (y = the activation's value where that is cheaper)
__device__ __forceinline__ float act_grad(int code, float x) {
    switch (code) {
    case EVD_ACT_RELU: return x > 0.f ? 1.f : 0.f;
    case EVD_ACT_SIGMOID: { const float y = 1.f / (1.f + expf(-x)); return y * (1.f - y); }
    case EVD_ACT_EXP: return expf(x);
    case EVD_ACT_SIGMOID1: { const float y = 1.f / (expf(-x) + 1.f); return 1.002f * y * (1.f - y); }
    case EVD_ACT_SOFTPLUS: { const float t = x - 1.f; return t > 20.f ? 1.f : 1.f / (1.f + expf(-t)); }
    case EVD_ACT_TANH: { const float y = tanhf(x); return 1.f - y * y; }
    default: return 1.f;
    }
}

// Backward of raw2outputs: d raw from the gradients of (out_map, depth, acc, weights).
// Same decomposition as k_composite_rows (a wavefront per ray, SPL consecutive samples per lane); the forward quantities
// are recomputed.  With G_i = dL/dw_i = g_map . rgb_i + g_depth z_i + g_acc + g_w_i (- sum g_map for a white background):
//   dL/d rgb_i = g_map w_i,      dL/d sigma_i = dist_i (G_i T_{i+1} - sum_{j>i} G_j w_j)      (no division: T_i (1 - alpha_i) = T_{i+1})
// the suffix sum is total - inclusive prefix (one DPP add scan); the last sample's alpha is the constant 1.
template <int SPL>
__global__ __launch_bounds__(256) void k_composite_rows_bwd(const float* __restrict__ raw, const float* __restrict__ z,
                                                            const float* __restrict__ rays_d, int rd_stride, long R, int S,
                                                            int sigma_ch, int rgb_ch0, int rgb_act, int sigma_act, int white_bkgd,
                                                            float rmnear, const float* __restrict__ noise,
                                                            const float* __restrict__ g_map, const float* __restrict__ g_depth,
                                                            const float* __restrict__ g_acc, const float* __restrict__ g_w,
                                                            float* __restrict__ d_raw, float* __restrict__ d_rays_d, int d_rd_stride) {
    const int lane = threadIdx.x & 63;
    const long r = blockIdx.x * (long)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= R) return;
    const int i0 = lane * SPL;
    const float4* rw = reinterpret_cast<const float4*>(raw + r * (long)S * 4);
    const float* zz = z + r * (long)S;
    float4 v[SPL];
    float zi[SPL + 1], gw[SPL];
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        const int i = min(i0 + j, S - 1);
        v[j] = rw[i];
        zi[j] = zz[i];
        gw[j] = g_w ? g_w[r * (long)S + i] : 0.f;
    }
    const float* d = rays_d + r * rd_stride;
    const float norm = ray_norm(d);
    const float gm[3] = {g_map ? g_map[r * 3] : 0.f, g_map ? g_map[r * 3 + 1] : 0.f, g_map ? g_map[r * 3 + 2] : 0.f};
    const float gd = g_depth ? g_depth[r] : 0.f;
    const float ga = (g_acc ? g_acc[r] : 0.f) - (white_bkgd ? gm[0] + gm[1] + gm[2] : 0.f);
    zi[SPL] = dpp_f32<0x130>(0.f, zi[0]);
    float alpha[SPL], om[SPL], dist[SPL], spre[SPL], mask[SPL], densm[SPL];
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        const int i = i0 + j;
        const float vv[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
        dist[j] = 0.f; spre[j] = 0.f; mask[j] = 1.f; densm[j] = 0.f;
        if (i < S - 1) {
            dist[j] = composite_dist(zi[j], zi[j + 1], norm);
            spre[j] = vv[sigma_ch] + (noise ? noise[r * (long)(S - 1) + i] : 0.f);
            if (rmnear > 0.f) mask[j] = rmnear_mask(zi[j + 1], rmnear);
            densm[j] = composite_density<ACT_IEEE>(sigma_act, spre[j], zi[j + 1], rmnear);
            alpha[j] = composite_alpha<EXP_IEEE>(densm[j], dist[j]);
        } else {
            alpha[j] = i == S - 1 ? 1.f : 0.f;
        }
        om[j] = i < S ? __fadd_rn(-alpha[j], 1.f) : 1.f;
    }
    float local = om[0];
#pragma unroll
    for (int j = 1; j < SPL; ++j) local *= om[j];
    const float incl = wave_scan_mul_dpp(local);
    float T = dpp_f32<0x138>(1.f, incl);
    float w[SPL], G[SPL], Tn[SPL], rgbv[SPL][3], lsum = 0.f;
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        const float vv[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
        w[j] = (i0 + j < S) ? alpha[j] * T : 0.f;
        T *= om[j];
        Tn[j] = T;                                          // T_{i+1}
#pragma unroll
        for (int c = 0; c < 3; ++c) rgbv[j][c] = act(rgb_act, vv[rgb_ch0 + c]);
        G[j] = gm[0] * rgbv[j][0] + gm[1] * rgbv[j][1] + gm[2] * rgbv[j][2] + gd * zi[j] + ga + gw[j];
        lsum += G[j] * w[j];
    }
    const float pre_incl = wave_scan_add_dpp(lsum);          // inclusive prefix of the lanes' sums of G w
    const float total = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pre_incl), 63));
    float run = pre_incl - lsum;                             // exclusive prefix at this lane's first sample
    float dn = 0.f;                                          // this lane's share of |d| dL/d|d|
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        const int i = i0 + j;
        run += G[j] * w[j];
        if (i < S) {
            const float vv[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
            float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 3; ++c) o[rgb_ch0 + c] = gm[c] * w[j] * act_grad(rgb_act, vv[rgb_ch0 + c]);
            if (i < S - 1) {
                const float suffix = total - run;            // sum_{j > i} G_j w_j
                const float q = dist[j] * (G[j] * Tn[j] - suffix);      // dL / d density_i
                o[sigma_ch] = q * mask[j] * act_grad(sigma_act, spre[j]);
                dn += q * densm[j];
            }
            reinterpret_cast<float4*>(d_raw + r * (long)S * 4)[i] = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
    // alpha_i depends on the ray direction through dist_i = dz_i |d| only: dL/d|d| = sum_i (dL/d density_i) density_i / |d|, and
    // d|d| / d d = d / |d|
    if (d_rays_d) {
        dn = wave_sum_dpp(dn);
        if (lane == 0) {
            const float k = dn / (norm * norm);
#pragma unroll
            for (int c = 0; c < 3; ++c) d_rays_d[r * d_rd_stride + c] = k * d[c];
        }
    }
}

// Backward of the FEATURE composite (composite_feature levels, voxnerf.py:223-229): fmap_c = sum_i w_i act(rows_ic) over G geo channels,
// the density from channel sigma_ch of raw [R, S, C].  k_composite_rows_bwd's scan (a wavefront per ray, SPL consecutive samples per lane,
// forward quantities recomputed) between two passes over the ray's [S, G] row block, which is what moves the bytes (S (8 G + 24) per ray):
//   A  the block is read in CONTIGUOUS pieces of whole samples (<= 64 samples, <= 1024 floats: element e of a piece by lane e mod 64; a
//      lane-per-sample walk would stride by the 4 G bytes of a row) into LDS, then lane l sums g_fmap . act(rows) of the piece's sample l
//      in channel order -> dot_i
//   B  G_i = dot_i + g_depth z_i + g_acc + g_w_i, d density and d rays_d exactly as k_composite_rows_bwd; w_i is left in LDS
//   C  d rows_ic = g_fmap_c w_i act'(rows_ic), written in the same contiguous order; the rows come from LDS when the ray is one piece
//      (S = 64, G = 15: 960 floats), else they are read again (the second read of a ray's few KiB is served by the caches)
// Without g_fmap, A is skipped and C writes zeros.  The four wavefronts of a workgroup share nothing but the barriers, so every
// wavefront runs the full trip counts (a ragged last workgroup works on row R - 1 again and stores nothing).
template <int SPL>
__global__ __launch_bounds__(256) void k_composite_feat_bwd(const float* __restrict__ raw, int C, int sigma_ch, const float* __restrict__ rows, int G,
                                                            int rows_act, const float* __restrict__ z, const float* __restrict__ rays_d,
                                                            int rd_stride, long R, int S, int sigma_act, float rmnear,
                                                            const float* __restrict__ noise, const float* __restrict__ g_fmap,
                                                            const float* __restrict__ g_depth, const float* __restrict__ g_acc,
                                                            const float* __restrict__ g_w, float* __restrict__ d_raw, float* __restrict__ d_rows,
                                                            float* __restrict__ d_rays_d, int d_rd_stride) {
    constexpr int TILE = 1024;
    __shared__ float s_tile[4][TILE], s_dot[4][256], s_w[4][256], s_g[4][128];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long r_own = blockIdx.x * 4L + wv;
    const bool live = r_own < R;
    const long r = live ? r_own : R - 1;
    const int TS = min(64, TILE / G);                        // samples per piece
    const bool single = S <= TS;
    const float* rw = rows + r * (long)S * G;
    float* tile = s_tile[wv];
    // ---- A
    if (g_fmap) {
        for (int c = lane; c < G; c += 64) s_g[wv][c] = g_fmap[r * G + c];
        for (int s0 = 0; s0 < S; s0 += TS) {
            const int ns = min(TS, S - s0), ne = ns * G;
            if (s0) __syncthreads();                         // the piece before this one has been summed
            for (int e = lane; e < ne; e += 64) tile[e] = rw[(long)s0 * G + e];
            __syncthreads();
            if (lane < ns) {
                float dsum = 0.f;
                for (int c = 0; c < G; ++c) dsum = fmaf(s_g[wv][c], act(rows_act, tile[lane * G + c]), dsum);
                s_dot[wv][s0 + lane] = dsum;
            }
        }
        __syncthreads();
    }
    // ---- B
    const int i0 = lane * SPL;
    const float* zz = z + r * (long)S;
    float sr[SPL], zi[SPL + 1], gw[SPL], dot[SPL];
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        const int i = min(i0 + j, S - 1);
        sr[j] = raw[(r * (long)S + i) * C + sigma_ch];
        zi[j] = zz[i];
        gw[j] = g_w ? g_w[r * (long)S + i] : 0.f;
        dot[j] = g_fmap ? s_dot[wv][i] : 0.f;
    }
    const float* d = rays_d + r * rd_stride;
    const float norm = ray_norm(d);
    const float gd = g_depth ? g_depth[r] : 0.f;
    const float ga = g_acc ? g_acc[r] : 0.f;
    zi[SPL] = dpp_f32<0x130>(0.f, zi[0]);
    float alpha[SPL], om[SPL], dist[SPL], spre[SPL], mask[SPL], densm[SPL];
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        const int i = i0 + j;
        dist[j] = 0.f; spre[j] = 0.f; mask[j] = 1.f; densm[j] = 0.f;
        if (i < S - 1) {
            dist[j] = composite_dist(zi[j], zi[j + 1], norm);
            spre[j] = sr[j] + (noise ? noise[r * (long)(S - 1) + i] : 0.f);
            if (rmnear > 0.f) mask[j] = rmnear_mask(zi[j + 1], rmnear);
            densm[j] = composite_density<ACT_IEEE>(sigma_act, spre[j], zi[j + 1], rmnear);
            alpha[j] = composite_alpha<EXP_IEEE>(densm[j], dist[j]);
        } else {
            alpha[j] = i == S - 1 ? 1.f : 0.f;
        }
        om[j] = i < S ? __fadd_rn(-alpha[j], 1.f) : 1.f;
    }
    float local = om[0];
#pragma unroll
    for (int j = 1; j < SPL; ++j) local *= om[j];
    const float incl = wave_scan_mul_dpp(local);
    float T = dpp_f32<0x138>(1.f, incl);
    float w[SPL], Gv[SPL], Tn[SPL], lsum = 0.f;
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        w[j] = (i0 + j < S) ? alpha[j] * T : 0.f;
        T *= om[j];
        Tn[j] = T;                                          // T_{i+1}
        Gv[j] = dot[j] + gd * zi[j] + ga + gw[j];
        lsum += Gv[j] * w[j];
        if (i0 + j < S) s_w[wv][i0 + j] = w[j];
    }
    const float pre_incl = wave_scan_add_dpp(lsum);
    const float total = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pre_incl), 63));
    float run = pre_incl - lsum;
    float dn = 0.f;
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        const int i = i0 + j;
        run += Gv[j] * w[j];
        if (i < S) {
            float ds = 0.f;
            if (i < S - 1) {
                const float suffix = total - run;            // sum_{j > i} G_j w_j
                const float q = dist[j] * (Gv[j] * Tn[j] - suffix);
                ds = q * mask[j] * act_grad(sigma_act, spre[j]);
                dn += q * densm[j];
            }
            if (live) {
                float* o = d_raw + (r * (long)S + i) * C;
                if (C == 4) {
                    *reinterpret_cast<float4*>(o) = make_float4(sigma_ch == 0 ? ds : 0.f, sigma_ch == 1 ? ds : 0.f, sigma_ch == 2 ? ds : 0.f, sigma_ch == 3 ? ds : 0.f);
                } else {
                    for (int c = 0; c < C; ++c) o[c] = c == sigma_ch ? ds : 0.f;
                }
            }
        }
    }
    if (d_rays_d) {
        dn = wave_sum_dpp(dn);
        if (lane == 0 && live) {
            const float k = dn / (norm * norm);
#pragma unroll
            for (int c = 0; c < 3; ++c) d_rays_d[r * d_rd_stride + c] = k * d[c];
        }
    }
    __syncthreads();                                         // s_w is complete
    // ---- C
    float* dr = d_rows + r * (long)S * G;
    const int ne = S * G, qi = 64 / G, qc = 64 % G;
    int i = lane / G, c = lane % G;
    for (int e = lane; e < ne; e += 64) {
        float v = 0.f;
        if (g_fmap) {
            const float x = single ? tile[e] : rw[e];
            v = s_g[wv][c] * s_w[wv][i] * act_grad(rows_act, x);
        }
        if (live) dr[e] = v;
        i += qi; c += qc;
        if (c >= G) { c -= G; ++i; }
    }
}

// out[r, f] = sum_s w[r, s] * x[r, s, ch0 + f] (optionally through an activation): used for n_rgb != 3 colour
// maps (PBE 15-channel features, voxnerf.py:226) and for feature compositing (nerf.py:119).  One block per ray.
__global__ void k_weighted_channels(const float* __restrict__ x, const float* __restrict__ w, long R, int S, int Cx, int ch0,
                                    int F, int act_code, int add_white, float* __restrict__ out) {
    const long r = blockIdx.x;
    for (int f = threadIdx.x; f < F; f += blockDim.x) {
        float s = 0.f, a = 0.f;
        for (int i = 0; i < S; ++i) {
            const float wi = w[r * (long)S + i];
            s += wi * act(act_code, x[(r * (long)S + i) * Cx + ch0 + f]);
            a += wi;
        }
        out[r * (long)F + f] = add_white ? s + (1.f - a) : s;
    }
}

}  // namespace evd

using namespace evd;

// S <= 256 -> the 64-sample chunks of a ray: NCH of the interleaved form, SPL of the row forms and of the backward
#define EVD_BY_CHUNKS(S, LAUNCH) do { if ((S) <= 64) LAUNCH(1); else if ((S) <= 128) LAUNCH(2); else if ((S) <= 192) LAUNCH(3); else LAUNCH(4); } while (0)

extern "C" {

int evd_raw2outputs(const float* raw, const float* z, const float* rays_d, int rays_d_stride, long R, int S, int C,
                    int sigma_ch, int rgb_ch0, int n_rgb, int rgb_act, int sigma_act, int white_bkgd,
                    float rmnear_thresh, const float* noise,
                    float* out_map, float* density, float* acc, float* weights, float* depth,
                    const float* feature, int F, float* fmap, void* stream) {
    EVD_REQUIRE(raw && z && rays_d && R >= 0 && S >= 1 && C >= 1, "evd_raw2outputs: bad arguments");
    EVD_REQUIRE(sigma_ch >= 0 && sigma_ch < C && rgb_ch0 >= 0 && rgb_ch0 + n_rgb <= C, "evd_raw2outputs: channel layout out of range");
    EVD_REQUIRE(!(fmap || (n_rgb != 3 && out_map)) || weights, "evd_raw2outputs: weights output required for feature maps");
    if (R == 0) return EVD_OK;
    hipStream_t st = as_stream(stream);
    if (n_rgb == 3 && C == 4 && S <= 256 && !(rmnear_thresh > 0.f) && sigma_act == EVD_ACT_RELU &&
        ((sigma_ch == 3 && rgb_ch0 == 0 && rgb_act == EVD_ACT_SIGMOID) ||
         (sigma_ch == 0 && rgb_ch0 == 1 && (rgb_act == EVD_ACT_RELU || rgb_act == EVD_ACT_NONE)))) {
        // interleaved form: the two channel layouts / activation sets the renderer produces (NeRF: rgb sigmoid, sigma last; PDRF levels:
        // sigma first, colour already sigmoided -> relu (coarse) / none (fine)), with the training node's raw noise / density output (not
        // rmnear); non-temporal loads / stores, rays per wavefront by R
        const int il_rpw = R >= (1L << 17) ? 4 : R >= (1L << 14) ? 2 : 1;     // >= 4 workgroups per CU before rays share a wavefront
#define EVD_IL(NCH, RPW, SC, RA) k_composite_il<NCH, RPW, SC, RA, EVD_ACT_RELU, true><<<(unsigned)cdiv(R, 4 * RPW), 256, 0, st>>>(raw, z, rays_d, rays_d_stride, R, S, white_bkgd, out_map, acc, weights, depth, noise, density)
#define EVD_IL_LAYOUT(NCH, RPW) do { if (sigma_ch == 3) EVD_IL(NCH, RPW, 3, EVD_ACT_SIGMOID); else if (rgb_act == EVD_ACT_RELU) EVD_IL(NCH, RPW, 0, EVD_ACT_RELU); else EVD_IL(NCH, RPW, 0, EVD_ACT_NONE); } while (0)
#define EVD_IL_RPW(NCH) do { if (il_rpw == 4) EVD_IL_LAYOUT(NCH, 4); else if (il_rpw == 1) EVD_IL_LAYOUT(NCH, 1); else EVD_IL_LAYOUT(NCH, 2); } while (0)
        EVD_BY_CHUNKS(S, EVD_IL_RPW);
#undef EVD_IL_RPW
#undef EVD_IL_LAYOUT
#undef EVD_IL
    } else if (n_rgb == 3 && C == 4 && S <= 256) {
        // bandwidth form: every lane owns SPL consecutive samples, two rays per wavefront
#define EVD_ROWS(SPL) k_composite_rows<SPL, 2><<<cdiv(R, 8), 256, 0, st>>>(raw, z, rays_d, rays_d_stride, R, S, sigma_ch, rgb_ch0, rgb_act, sigma_act, \
                                                                   white_bkgd, rmnear_thresh, noise, out_map, density, acc, weights, depth)
        EVD_BY_CHUNKS(S, EVD_ROWS);
#undef EVD_ROWS
    } else if (n_rgb == 3) {
        k_composite<3><<<cdiv(R, 4), 256, 0, st>>>(raw, z, rays_d, rays_d_stride, R, S, C, sigma_ch, rgb_ch0, n_rgb, rgb_act, sigma_act,
                                                   white_bkgd, rmnear_thresh, noise, out_map, density, acc, weights, depth);
    } else {
        k_composite<0><<<cdiv(R, 4), 256, 0, st>>>(raw, z, rays_d, rays_d_stride, R, S, C, sigma_ch, rgb_ch0, n_rgb, rgb_act, sigma_act,
                                                   white_bkgd, rmnear_thresh, noise, nullptr, density, acc, weights, depth);
        if (out_map && n_rgb > 0)
            k_weighted_channels<<<R, 64, 0, st>>>(raw, weights, R, S, C, rgb_ch0, n_rgb, rgb_act, white_bkgd, out_map);
    }
    EVD_LAUNCH_CHECK();
    if (fmap && feature && F > 0) {
        k_weighted_channels<<<R, F >= 256 ? 256 : 64, 0, st>>>(feature, weights, R, S, F, 0, F, EVD_ACT_NONE, 0, fmap);
        EVD_LAUNCH_CHECK();
    }
    return EVD_OK;
}

int evd_raw2outputs_bwd(const float* raw, const float* z, const float* rays_d, int rays_d_stride, long R, int S, int C,
                        int sigma_ch, int rgb_ch0, int n_rgb, int rgb_act, int sigma_act, int white_bkgd, float rmnear_thresh,
                        const float* noise, const float* g_map, const float* g_depth, const float* g_acc, const float* g_weights,
                        float* d_raw, void* stream) {
    return evd_raw2outputs_bwd_rays(raw, z, rays_d, rays_d_stride, R, S, C, sigma_ch, rgb_ch0, n_rgb, rgb_act, sigma_act, white_bkgd, rmnear_thresh,
                                    noise, g_map, g_depth, g_acc, g_weights, d_raw, nullptr, 0, stream);
}

int evd_raw2outputs_bwd_rays(const float* raw, const float* z, const float* rays_d, int rays_d_stride, long R, int S, int C,
                             int sigma_ch, int rgb_ch0, int n_rgb, int rgb_act, int sigma_act, int white_bkgd, float rmnear_thresh,
                             const float* noise, const float* g_map, const float* g_depth, const float* g_acc, const float* g_weights,
                             float* d_raw, float* d_rays_d, int d_rays_d_stride, void* stream) {
    EVD_REQUIRE(raw && z && rays_d && d_raw && R >= 0 && S >= 1, "evd_raw2outputs_bwd: bad arguments");
    EVD_REQUIRE(!d_rays_d || d_rays_d_stride >= 3, "evd_raw2outputs_bwd_rays: d_rays_d needs a row stride >= 3");
    EVD_REQUIRE(C == 4 && n_rgb == 3 && S <= 256, "evd_raw2outputs_bwd: built for [R,S,4] raw with three colour channels and S <= 256 (got C=%d n_rgb=%d S=%d)", C, n_rgb, S);
    EVD_REQUIRE(sigma_ch >= 0 && sigma_ch < 4 && rgb_ch0 >= 0 && rgb_ch0 + 3 <= 4 && (sigma_ch < rgb_ch0 || sigma_ch >= rgb_ch0 + 3),
                "evd_raw2outputs_bwd: channel layout out of range");
    if (R == 0) return EVD_OK;
    hipStream_t st = as_stream(stream);
#define EVD_BWD(SPL) k_composite_rows_bwd<SPL><<<cdiv(R, 4), 256, 0, st>>>(raw, z, rays_d, rays_d_stride, R, S, sigma_ch, rgb_ch0, rgb_act, sigma_act, \
                                                                          white_bkgd, rmnear_thresh, noise, g_map, g_depth, g_acc, g_weights, d_raw, d_rays_d, d_rays_d_stride)
    EVD_BY_CHUNKS(S, EVD_BWD);
#undef EVD_BWD
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_raw2outputs_feat_bwd(const float* raw, int C, int sigma_ch, const float* rows, int G, int rows_act, const float* z,
                             const float* rays_d, int rays_d_stride, const float* noise, int sigma_act, float rmnear_thresh, long R, int S,
                             const float* g_fmap, const float* g_depth, const float* g_acc, const float* g_weights,
                             float* d_raw, float* d_rows, float* d_rays_d, int d_rays_d_stride, void* stream) {
    EVD_REQUIRE(raw && rows && z && rays_d && d_raw && d_rows && R >= 0, "evd_raw2outputs_feat_bwd: bad arguments");
    EVD_REQUIRE(G >= 1 && G <= 128 && S >= 1 && S <= 256, "evd_raw2outputs_feat_bwd: built for 1..128 feature channels and 1..256 samples (got G=%d S=%d)", G, S);
    EVD_REQUIRE(C >= 1 && sigma_ch >= 0 && sigma_ch < C && rays_d_stride >= 3, "evd_raw2outputs_feat_bwd: channel layout out of range");
    EVD_REQUIRE(!d_rays_d || d_rays_d_stride >= 3, "evd_raw2outputs_feat_bwd: d_rays_d needs a row stride >= 3");
    if (R == 0) return EVD_OK;
    hipStream_t st = as_stream(stream);
#define EVD_FBWD(SPL) k_composite_feat_bwd<SPL><<<(unsigned)cdiv(R, 4), 256, 0, st>>>(raw, C, sigma_ch, rows, G, rows_act, z, rays_d, rays_d_stride, R, S, sigma_act, \
                                                                                     rmnear_thresh, noise, g_fmap, g_depth, g_acc, g_weights, d_raw, d_rows, d_rays_d, d_rays_d_stride)
    EVD_BY_CHUNKS(S, EVD_FBWD);
#undef EVD_FBWD
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // extern "C"
