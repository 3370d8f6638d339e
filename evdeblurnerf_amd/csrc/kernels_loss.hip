// Loss-side pixel ops: sub-exposure weighted sums, camera response functions, fused blur / event loss reductions.  All HBM-bound and
// tiny; the point of fusing them is one launch + one packed partial-sum vector per step (which is what the ranks all-reduce) instead of
// dozens of ATen launches.  (The AWP scan is in kernel_awp_integrate.hip, the EDI image kernels in kernels_edi_prior.hip.)
#include "evd_common.h"
#include "wave_ops.h"

namespace evd {

// CRF parameters travel as a kernel argument (scalar loads, wave-uniform).  networks/tonemapping.py:16-22
constexpr int CRF_MAX_IN = 8;
struct CrfParams {
    int map_type;       // 0 none, 1 gamma, 2 learn
    int E;              // extra features
    float inv_gamma;
    float b3;
    float w0[16 * CRF_MAX_IN], b0[16], w1[256], b1[16], w2[256], b2[16], w3[16];
};
// The flat parameter layout of evd_crf_get_params / evd_crf_load_params and of evd_event_loss_bwd's d_params:
// w0 [16][CRF_MAX_IN] (rows padded), b0 [16], w1 [16][16], b1, w2 [16][16], b2, w3 [16], b3.
enum CrfLayout { O_W0 = 0, O_B0 = O_W0 + 16 * CRF_MAX_IN, O_W1 = O_B0 + 16, O_B1 = O_W1 + 256, O_W2 = O_B1 + 16, O_B2 = O_W2 + 256, O_W3 = O_B2 + 16,
                 O_B3 = O_W3 + 16, CRF_NPARAM = O_B3 + 1 };
template <class P, class F>
static void crf_walk(P& p, F visit) {      // visit(member, offset in the flat layout, floats)
    visit(p.w0, O_W0, 16 * CRF_MAX_IN); visit(p.b0, O_B0, 16);
    visit(p.w1, O_W1, 256); visit(p.b1, O_B1, 16);
    visit(p.w2, O_W2, 256); visit(p.b2, O_B2, 16);
    visit(p.w3, O_W3, 16); visit(&p.b3, O_B3, 1);
}

__device__ __forceinline__ float crf_gamma(const CrfParams& c, float v) { return c.map_type == 1 ? powf(v, c.inv_gamma) : v; }
__device__ __forceinline__ float crf_learn_out(float s, float v) { return 1.f / (1.f + expf(-(s * 0.1f + v))); }

// CRF.forward for one channel value, networks/tonemapping.py:59-93
__device__ __forceinline__ float crf_apply(const CrfParams& c, float v, const float* feat, bool skip_learn) {
    if (c.map_type == 0) return v;
    v = crf_gamma(c, v);
    if (!skip_learn && c.map_type == 2) {
        // every index into the parameter block is a compile-time constant (w0 rows are padded to CRF_MAX_IN): the weights
        // stay scalar loads from the kernel-argument buffer.  (A runtime-strided w0[j * nin + k] made hipcc copy the whole
        // 2.4 KB block to scratch, per lane.)
        float in[CRF_MAX_IN];
        in[0] = v;
#pragma unroll
        for (int e = 1; e < CRF_MAX_IN; ++e) in[e] = (feat && e - 1 < c.E) ? feat[e - 1] : 0.f;
        float h[16], h2[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            float s = c.b0[j];
#pragma unroll
            for (int k = 0; k < CRF_MAX_IN; ++k) s = fmaf(c.w0[j * CRF_MAX_IN + k], in[k], s);   // padded columns are zero
            h[j] = fmaxf(s, 0.f);
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            float s = c.b1[j];
#pragma unroll
            for (int k = 0; k < 16; ++k) s = fmaf(c.w1[j * 16 + k], h[k], s);
            h2[j] = fmaxf(s, 0.f);
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            float s = c.b2[j];
#pragma unroll
            for (int k = 0; k < 16; ++k) s = fmaf(c.w2[j * 16 + k], h2[k], s);
            h[j] = fmaxf(s, 0.f);
        }
        float s = c.b3;
#pragma unroll
        for (int k = 0; k < 16; ++k) s = fmaf(c.w3[k], h[k], s);
        v = crf_learn_out(s, v);
    }
    return v;
}
// d crf(x) / dx for the non-learnable response curves (identity, gamma): tonemapping.py:64-68
__device__ __forceinline__ float crf_grad_simple(const CrfParams& c, float x) {
    if (c.map_type == 1) return c.inv_gamma * powf(x, c.inv_gamma - 1.f);
    return 1.f;
}

__device__ __forceinline__ float luma_of(int standard, float r, float g, float b) {
    if (standard == 0) return 0.299f * r + 0.587f * g + 0.114f * b;        // rec601, tonemapping.py:128-129
    if (standard == 1) return 0.2126f * r + 0.7152f * g + 0.0722f * b;     // rec709
    return (r + g + b) / 3.f;                                              // avg
}

__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < nw; ++i) s += red[i];
    return s;
}

// rbk_weighted_sum, networks/dpnerf/blurmodel.py:112-127
__global__ void k_weighted_sum(const float* __restrict__ x, const float* __restrict__ ccw, long R, int P, int C,
                               float* __restrict__ out) {
    const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (idx >= R * C) return;
    const long r = idx / C;
    const int c = idx % C;
    float s = 0.f;
    for (int p = 0; p < P; ++p) s += x[(r * P + p) * (long)C + c] * ccw[r * P + p];
    out[idx] = s;
}

__global__ void k_crf_forward(const CrfParams crf, const float* __restrict__ x, const float* __restrict__ feat,
                              int feat_per_channel, int skip_learn, int luma, long n, float* __restrict__ out) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* f = feat ? (feat_per_channel ? feat + (i * 3 + c) * crf.E : feat + i * crf.E) : nullptr;
        v[c] = crf_apply(crf, x[i * 3 + c], f, skip_learn);
    }
    if (luma < 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[i * 3 + c] = v[c];
    } else {
        out[i] = luma_of(luma, v[0], v[1], v[2]);
    }
}

// spec: run_nerf.py:443-497 + networks/renderer.py:327-336.  The terms of one (pixel, colour channel): the five squared errors into se
// (entries that do not apply stay as they are) and the three weighted sums, which are also written out where wanted.
__device__ __forceinline__ void blur_loss_lane(const CrfParams& crf, int skip_learn, const float* __restrict__ rgb_p,
                                               const float* __restrict__ rgb0_p, const float* __restrict__ w1, const float* __restrict__ w2,
                                               const float* __restrict__ tgt, const float* __restrict__ tgt0, long r, int ch, int P,
                                               float* __restrict__ o_rgb, float* __restrict__ o_rgb1, float* __restrict__ o_awp, float (&se)[5]) {
    float a = 0.f, b = 0.f, c = 0.f;
    for (int p = 0; p < P; ++p) {
        const float wa = w1[r * P + p], wb = w2 ? w2[r * P + p] : 0.f;
        const float f = rgb_p[(r * P + p) * 3 + ch];
        a += f * wa;
        c += f * wb;
        if (rgb0_p) b += rgb0_p[(r * P + p) * 3 + ch] * wa;
    }
    const float t = tgt[r * 3 + ch];
    float d = crf_apply(crf, a, nullptr, skip_learn) - t;
    se[0] = d * d;
    if (o_rgb) o_rgb[r * 3 + ch] = a;
    if (rgb0_p) {
        d = crf_apply(crf, b, nullptr, skip_learn) - t;
        se[1] = d * d;
        if (o_rgb1) o_rgb1[r * 3 + ch] = b;
    }
    if (w2) {
        d = crf_apply(crf, c, nullptr, skip_learn) - t;
        se[2] = d * d;
        if (o_awp) o_awp[r * 3 + ch] = c;
    }
    if (tgt0) {
        const float t0 = tgt0[r * 3 + ch];
        d = crf_apply(crf, rgb_p[(r * P) * 3 + ch], nullptr, skip_learn) - t0;     // rgb_pts[:, 0] renderer.py:374
        se[3] = d * d;
        if (rgb0_p) {
            d = crf_apply(crf, rgb0_p[(r * P) * 3 + ch], nullptr, skip_learn) - t0;
            se[4] = d * d;
        }
    }
}

__global__ __launch_bounds__(256) void k_blur_loss(const CrfParams crf, int skip_learn, const float* __restrict__ rgb_p,
                                                   const float* __restrict__ rgb0_p, const float* __restrict__ w1,
                                                   const float* __restrict__ w2, const float* __restrict__ tgt,
                                                   const float* __restrict__ tgt0, long R, int P, float* __restrict__ partial,
                                                   float* __restrict__ o_rgb, float* __restrict__ o_rgb1, float* __restrict__ o_awp) {
    // one lane per (pixel, colour channel): a 1024-pixel blur batch is 3072 lanes in 48 small blocks instead of 4 busy ones
    __shared__ float red[8];
    const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long r = idx / 3;
    const int ch = (int)(idx % 3);
    float se[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    float cnt = 0.f;
    if (r < R) {
        cnt = 1.f;
        blur_loss_lane(crf, skip_learn, rgb_p, rgb0_p, w1, w2, tgt, tgt0, r, ch, P, o_rgb, o_rgb1, o_awp, se);
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const float s = block_sum(se[k], red);
        if (threadIdx.x == 0 && s != 0.f) atomicAdd(partial + k, s);
    }
    const float n = block_sum(cnt, red);
    if (threadIdx.x == 0) atomicAdd(partial + 5, n);
}

// ---- the deterministic forms (evd_crf_set_deterministic; run_nerf.py:50): a bounded grid walks the batch with a grid-stride loop, every lane
// sums its elements in index order, the workgroup sum (block_sum: a fixed shuffle tree, then the wavefronts in order) goes to the handle's
// buffer of per-workgroup partials, and k_det_fold -- ONE wavefront -- adds them in workgroup order and performs the call's single
// out[k] += sum.  No floating-point atomic: the same bits for the same batch.
constexpr int DET_BLOCKS = 256;         // workgroups of a deterministic loss launch at most = rows of the handle's buffer

__global__ __launch_bounds__(64) void k_det_fold(const float* __restrict__ wg, int blocks, int K, float* __restrict__ out) {
    for (int k = threadIdx.x; k < K; k += 64) {
        float s = 0.f;
        int b = 0;
        for (; b + 8 <= blocks; b += 8) {             // eight loads in flight, added in workgroup order
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = wg[(long)(b + j) * K + k];
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[j];
        }
        for (; b < blocks; ++b) s += wg[(long)b * K + k];
        out[k] += s;
    }
}

__global__ __launch_bounds__(256) void k_blur_loss_det(const CrfParams crf, int skip_learn, const float* __restrict__ rgb_p,
                                                       const float* __restrict__ rgb0_p, const float* __restrict__ w1,
                                                       const float* __restrict__ w2, const float* __restrict__ tgt,
                                                       const float* __restrict__ tgt0, long R, int P, float* __restrict__ wg,
                                                       float* __restrict__ o_rgb, float* __restrict__ o_rgb1, float* __restrict__ o_awp) {
    __shared__ float red[8];
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (long idx = blockIdx.x * 256L + threadIdx.x; idx < 3 * R; idx += gridDim.x * 256L) {
        float se[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        blur_loss_lane(crf, skip_learn, rgb_p, rgb0_p, w1, w2, tgt, tgt0, idx / 3, (int)(idx % 3), P, o_rgb, o_rgb1, o_awp, se);
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[k] += se[k];
        acc[5] += 1.f;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float s = block_sum(acc[k], red);
        if (threadIdx.x == 0) wg[blockIdx.x * 6 + k] = s;
    }
}

// Backward of k_blur_loss ("next" row f-1, slice): with g[k] = dL/d partial[k] (k = 0..4) and a = sum_p w1 rgb_p etc.
//   d a = 2 g0 (crf(a) - t) crf'(a),  d b = 2 g1 (..rgb0..),  d c = 2 g2 (..w2..),  pts0 terms act on p = 0;
//   d rgb_p[p] = d a w1[p] + d c w2[p],   d rgb0_p[p] = d b w1[p],   d w1[p] = d a . rgb_p[p] + d b . rgb0_p[p],   d w2[p] = d c . rgb_p[p].
// One lane per (pixel, channel); d w1 / d w2 sum the three channels of a pixel with two DPP adds inside the lane triple... the
// triples straddle wavefront rows, so the channel sum goes through atomicAdd on the zero-initialised outputs instead.
struct BlurBwdCoef { float da, db, dc; };
__device__ __forceinline__ BlurBwdCoef blur_bwd_coef(const CrfParams& crf, int skip_learn, const float* __restrict__ rgb_p,
                                                     const float* __restrict__ rgb0_p, const float* __restrict__ w1, const float* __restrict__ w2,
                                                     const float* __restrict__ tgt, long r, int ch, int P, float g0, float g1, float g2) {
    float a = 0.f, b = 0.f, c = 0.f;
    for (int p = 0; p < P; ++p) {
        const float wa = w1[r * P + p], wb = w2 ? w2[r * P + p] : 0.f;
        const float f = rgb_p[(r * P + p) * 3 + ch];
        a += f * wa;
        c += f * wb;
        if (rgb0_p) b += rgb0_p[(r * P + p) * 3 + ch] * wa;
    }
    const float t = tgt[r * 3 + ch];
    BlurBwdCoef k;
    k.da = 2.f * g0 * (crf_apply(crf, a, nullptr, skip_learn) - t) * crf_grad_simple(crf, a);
    k.db = rgb0_p ? 2.f * g1 * (crf_apply(crf, b, nullptr, skip_learn) - t) * crf_grad_simple(crf, b) : 0.f;
    k.dc = w2 ? 2.f * g2 * (crf_apply(crf, c, nullptr, skip_learn) - t) * crf_grad_simple(crf, c) : 0.f;
    return k;
}
// sub-exposure p of (pixel r, channel ch): writes d rgb_p / d rgb0_p, returns this channel's terms of d w1[q] and d w2[q]
struct BlurBwdW { float w1, w2; };
__device__ __forceinline__ BlurBwdW blur_bwd_sub(const CrfParams& crf, int skip_learn, const float* __restrict__ rgb_p,
                                                 const float* __restrict__ rgb0_p, const float* __restrict__ w1, const float* __restrict__ w2,
                                                 const float* __restrict__ tgt0, long r, int ch, int p, int P, const BlurBwdCoef& k, float g3, float g4,
                                                 float* __restrict__ d_rgb_p, float* __restrict__ d_rgb0_p) {
    const long q = r * P + p;
    const float f = rgb_p[q * 3 + ch], f0 = rgb0_p ? rgb0_p[q * 3 + ch] : 0.f;
    float dr = k.da * w1[q] + (w2 ? k.dc * w2[q] : 0.f), dr0 = k.db * w1[q];
    if (p == 0 && tgt0) {                           // pts0 / EDI-prior terms on the p = 0 render (renderer.py:374)
        const float t0 = tgt0[r * 3 + ch];
        dr += 2.f * g3 * (crf_apply(crf, f, nullptr, skip_learn) - t0) * crf_grad_simple(crf, f);
        if (rgb0_p) dr0 += 2.f * g4 * (crf_apply(crf, f0, nullptr, skip_learn) - t0) * crf_grad_simple(crf, f0);
    }
    d_rgb_p[q * 3 + ch] = dr;
    if (d_rgb0_p) d_rgb0_p[q * 3 + ch] = dr0;
    return BlurBwdW{k.da * f + k.db * f0, k.dc * f};
}

__global__ __launch_bounds__(64) void k_blur_loss_bwd(const CrfParams crf, int skip_learn, const float* __restrict__ rgb_p,
                                                      const float* __restrict__ rgb0_p, const float* __restrict__ w1,
                                                      const float* __restrict__ w2, const float* __restrict__ tgt,
                                                      const float* __restrict__ tgt0, long R, int P, float g0, float g1, float g2,
                                                      float g3, float g4, const float* __restrict__ gdev, float* __restrict__ d_rgb_p,
                                                      float* __restrict__ d_rgb0_p, float* __restrict__ d_w1, float* __restrict__ d_w2) {
    if (gdev) { g0 = gdev[0]; g1 = gdev[1]; g2 = gdev[2]; g3 = gdev[3]; g4 = gdev[4]; }      // dL/d partial from device memory (no host copy)
    const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long r = idx / 3;
    const int ch = (int)(idx % 3);
    if (r >= R) return;
    const BlurBwdCoef k = blur_bwd_coef(crf, skip_learn, rgb_p, rgb0_p, w1, w2, tgt, r, ch, P, g0, g1, g2);
    for (int p = 0; p < P; ++p) {
        const long q = r * P + p;
        const BlurBwdW dw = blur_bwd_sub(crf, skip_learn, rgb_p, rgb0_p, w1, w2, tgt0, r, ch, p, P, k, g3, g4, d_rgb_p, d_rgb0_p);
        if (d_w1) atomicAdd(d_w1 + q, dw.w1);
        if (d_w2 && w2) atomicAdd(d_w2 + q, dw.w2);
    }
}

// The deterministic form: one lane per PIXEL, which adds the three channel terms of d w1 / d w2 in channel order and writes the sum
__global__ __launch_bounds__(64) void k_blur_loss_bwd_det(const CrfParams crf, int skip_learn, const float* __restrict__ rgb_p,
                                                          const float* __restrict__ rgb0_p, const float* __restrict__ w1,
                                                          const float* __restrict__ w2, const float* __restrict__ tgt,
                                                          const float* __restrict__ tgt0, long R, int P, float g0, float g1, float g2,
                                                          float g3, float g4, const float* __restrict__ gdev, float* __restrict__ d_rgb_p,
                                                          float* __restrict__ d_rgb0_p, float* __restrict__ d_w1, float* __restrict__ d_w2) {
    if (gdev) { g0 = gdev[0]; g1 = gdev[1]; g2 = gdev[2]; g3 = gdev[3]; g4 = gdev[4]; }
    const long r = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (r >= R) return;
    BlurBwdCoef k[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) k[ch] = blur_bwd_coef(crf, skip_learn, rgb_p, rgb0_p, w1, w2, tgt, r, ch, P, g0, g1, g2);
    for (int p = 0; p < P; ++p) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const BlurBwdW dw = blur_bwd_sub(crf, skip_learn, rgb_p, rgb0_p, w1, w2, tgt0, r, ch, p, P, k[ch], g3, g4, d_rgb_p, d_rgb0_p);
            s1 += dw.w1;
            s2 += dw.w2;
        }
        if (d_w1) d_w1[r * P + p] = s1;
        if (d_w2 && w2) d_w2[r * P + p] = s2;
    }
}

// spec: run_nerf.py:518-570 + utils/events.py:260-284.  The learnable event-CRF (a 1+E -> 16 -> 16 -> 16 -> 1 MLP per
// colour value, ~650 FMAs) is evaluated 12 times per event (start/end x fine/coarse x 3 channels): one LANE per
// evaluation, 16 lanes per event (lane = 4 which + channel, channel 3 idle), the luma / log-difference assembled with
// quad and row DPP moves; weights are wave-uniform scalar loads from the kernel argument.
struct EventLane {
    int sub, which, c, ch;      // lane of the 16-lane group; which: 0 end, 1 start, 2 end0, 3 start0; channel; the colour mask's channel
    long ii;                    // event index, clamped into the batch
    bool on, have0, eval;       // the event exists; the coarse pair is given; this lane evaluates a CRF
    float cn, cp;
    const float* src;           // the colour input this lane reads
};
// blk: the 16-event block of the batch this workgroup is on (the default kernels: blockIdx.x; the deterministic ones walk several)
__device__ __forceinline__ EventLane event_lane(const float* start, const float* end, const float* start0, const float* end0, const float* cum_neg,
                                                const float* cum_pos, const unsigned char* cmask, long N, long blk) {
    EventLane L;
    L.sub = threadIdx.x & 15; L.which = L.sub >> 2; L.c = L.sub & 3;
    const long i = blk * (long)(blockDim.x >> 4) + (threadIdx.x >> 4);
    L.on = i < N;
    L.ii = L.on ? i : N - 1;
    L.have0 = start0 && end0;
    L.eval = L.c < 3 && (L.which < 2 || L.have0);
    L.cn = cum_neg[L.ii]; L.cp = cum_pos[L.ii];
    L.ch = 0;
    if (cmask) for (int k = 0; k < 3; ++k) if (cmask[L.ii * 3 + k]) L.ch = k;
    L.src = L.which == 0 ? end : L.which == 1 ? start : L.which == 2 ? end0 : start0;
    return L;
}
// whether the lane's CRF evaluation sees the event's (cum_neg, cum_pos) as extra features: 'pos-neg' run_nerf.py:522-523, 'color-pos-neg'
// :524-531 (the colour mask's channel only; the others see zeros, which is what an evaluation without features sees)
__device__ __forceinline__ bool event_sees_bii(const EventLane& L, int add_bii_feat) {
    return add_bii_feat == 1 || (add_bii_feat == 2 && L.c == L.ch);
}
// The quad's three tone-mapped channel values -> luma, log-luma; the event's bii (run_nerf.py:518-519) and colour weight
struct EventChain { float lum, lg, bii, w; };
__device__ __forceinline__ EventChain event_chain(const EventLane& L, float v, int tonemap_only, float thr_neg, float thr_pos, bool masked,
                                                  float cw0, float cw1, float cw2, int has_cw) {
    const float v0 = dpp_f32<0x00>(0.f, v), v1 = dpp_f32<0x55>(0.f, v), v2 = dpp_f32<0xaa>(0.f, v);      // quad_perm broadcasts of lanes 0, 1, 2
    const float sel[3] = {v0, v1, v2}, cw[3] = {cw0, cw1, cw2};
    EventChain k;
    k.lum = tonemap_only ? sel[L.ch] : luma_of(0, v0, v1, v2);
    k.lg = logf(k.lum + 1e-5f);
    k.bii = __fadd_rn(__fmul_rn(thr_neg, L.cn), __fmul_rn(thr_pos, L.cp));
    k.w = (masked && has_cw) ? cw[L.ch] : 1.f;
    return k;
}

// this lane's terms of the 16-event block blk, ADDED to s_f (fine), s_c (coarse), s_w (weight); every lane of the workgroup calls it (DPP moves)
__device__ __forceinline__ void event_loss_terms(const CrfParams& crf, int skip_learn, int add_bii_feat, int tonemap_only,
                                                 const float* __restrict__ start, const float* __restrict__ end,
                                                 const float* __restrict__ start0, const float* __restrict__ end0,
                                                 const float* __restrict__ cum_neg, const float* __restrict__ cum_pos,
                                                 float thr_neg, float thr_pos, const unsigned char* __restrict__ cmask,
                                                 float cw0, float cw1, float cw2, int has_cw, long N, long blk, float& s_f, float& s_c, float& s_w) {
    const EventLane L = event_lane(start, end, start0, end0, cum_neg, cum_pos, cmask, N, blk);
    float v = 0.f;
    if (L.eval) {
        const float f[2] = {L.cn, L.cp};
        v = crf_apply(crf, L.src[L.ii * 3 + L.c], event_sees_bii(L, add_bii_feat) ? f : nullptr, skip_learn);
    }
    const EventChain ev = event_chain(L, v, tonemap_only, thr_neg, thr_pos, cmask != nullptr, cw0, cw1, cw2, has_cw);
    // pred = log(luma(end)) - log(luma(start)): quads 0 - 1 (fine) and 2 - 3 (coarse) of the 16-lane group
    const float pred = ev.lg - dpp_f32<0x104>(0.f, ev.lg);                        // row_shl:4 -> lane l reads lane l + 4
    const float d = pred - ev.bii, w = ev.w;
    if (L.on && L.sub == 0) { s_f += d * d * w; s_w += w; }
    if (L.on && L.sub == 8 && L.have0) s_c += d * d * w;
}

__global__ __launch_bounds__(256) void k_event_loss(const CrfParams crf, int skip_learn, int add_bii_feat, int tonemap_only,
                                                    const float* __restrict__ start, const float* __restrict__ end,
                                                    const float* __restrict__ start0, const float* __restrict__ end0,
                                                    const float* __restrict__ cum_neg, const float* __restrict__ cum_pos,
                                                    float thr_neg, float thr_pos, const unsigned char* __restrict__ cmask,
                                                    float cw0, float cw1, float cw2, int has_cw, long N, float* __restrict__ partial) {
    __shared__ float red[8];
    float s_f = 0.f, s_c = 0.f, s_w = 0.f;
    event_loss_terms(crf, skip_learn, add_bii_feat, tonemap_only, start, end, start0, end0, cum_neg, cum_pos, thr_neg, thr_pos, cmask, cw0, cw1, cw2,
                     has_cw, N, blockIdx.x, s_f, s_c, s_w);
    const float a = block_sum(s_f, red), b = block_sum(s_c, red), cc = block_sum(s_w, red);
    if (threadIdx.x == 0) {
        atomicAdd(partial + 0, a);
        atomicAdd(partial + 1, b);
        atomicAdd(partial + 2, cc);
    }
}

// the deterministic form (see k_blur_loss_det): workgroup b walks the 16-event blocks b, b + gridDim.x, ...
__global__ __launch_bounds__(256) void k_event_loss_det(const CrfParams crf, int skip_learn, int add_bii_feat, int tonemap_only,
                                                        const float* __restrict__ start, const float* __restrict__ end,
                                                        const float* __restrict__ start0, const float* __restrict__ end0,
                                                        const float* __restrict__ cum_neg, const float* __restrict__ cum_pos,
                                                        float thr_neg, float thr_pos, const unsigned char* __restrict__ cmask,
                                                        float cw0, float cw1, float cw2, int has_cw, long N, float* __restrict__ wg) {
    __shared__ float red[8];
    float s_f = 0.f, s_c = 0.f, s_w = 0.f;
    for (long blk = blockIdx.x; blk * 16 < N; blk += gridDim.x)
        event_loss_terms(crf, skip_learn, add_bii_feat, tonemap_only, start, end, start0, end0, cum_neg, cum_pos, thr_neg, thr_pos, cmask, cw0, cw1, cw2,
                         has_cw, N, blk, s_f, s_c, s_w);
    const float a = block_sum(s_f, red), b = block_sum(s_c, red), cc = block_sum(s_w, red);
    if (threadIdx.x == 0) {
        wg[blockIdx.x * 3 + 0] = a;
        wg[blockIdx.x * 3 + 1] = b;
        wg[blockIdx.x * 3 + 2] = cc;
    }
}

// ------------------------------------------------------------------------------------------------
// Backward of k_event_loss ("next" row f-1, slice): gradients of  g_f * partial[0] + g_c * partial[1]  w.r.t. the four colour
// inputs and w.r.t. the parameters of the learnable event-CRF (d_params in the CrfLayout order).  Same lane set-up as the forward kernel;
// every lane re-runs its CRF evaluation keeping the three hidden layers, back-propagates  d out -> d (input, parameters),  the parameter
// contributions are summed over the wavefront with DPP adds, over the block in LDS and added to the global gradient once per block.
// The 16-event block blk on this workgroup (every lane calls it).  pacc: the LDS accumulator of the parameter sums -- the workgroup's,
// added to with LDS float atomics (OWN = false), or this WAVEFRONT's own slot, added to by its lane 0 alone (OWN = true: the deterministic form)
template <bool OWN>
__device__ __forceinline__ void event_loss_bwd_block(const CrfParams& crf, int skip_learn, int add_bii_feat, int tonemap_only,
                                                     const float* __restrict__ start, const float* __restrict__ end,
                                                     const float* __restrict__ start0, const float* __restrict__ end0,
                                                     const float* __restrict__ cum_neg, const float* __restrict__ cum_pos,
                                                     float thr_neg, float thr_pos, const unsigned char* __restrict__ cmask,
                                                     float cw0, float cw1, float cw2, int has_cw, long N, long blk, float g_f, float g_c,
                                                     float* __restrict__ d_start, float* __restrict__ d_end,
                                                     float* __restrict__ d_start0, float* __restrict__ d_end0, float* pacc) {
    const int lane = threadIdx.x & 63;
    const EventLane L = event_lane(start, end, start0, end0, cum_neg, cum_pos, cmask, N, blk);
    const int which = L.which, c = L.c, ch = L.ch;
    const bool active = L.on && L.eval;
    const bool learn = crf.map_type == 2 && !skip_learn;
    // ---- forward of this lane's evaluation (the MLP of crf_apply), hidden layers kept
    float in[CRF_MAX_IN], h1[16], h2[16], h3[16];
#pragma unroll
    for (int e = 0; e < CRF_MAX_IN; ++e) in[e] = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) h1[j] = h2[j] = h3[j] = 0.f;      // idle lanes take part in the parameter sums below: their products must be 0, not 0 x garbage
    float v = 0.f, xg = 0.f, dgamma = 1.f;
    if (L.eval) {
        const float x = L.src[L.ii * 3 + c];
        xg = crf_gamma(crf, x);
        dgamma = crf_grad_simple(crf, x);
        v = xg;
        if (learn) {
            in[0] = xg;
            if (event_sees_bii(L, add_bii_feat)) { in[1] = L.cn; in[2] = L.cp; }      // (the entry checks extra_features == 2)
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                float s = crf.b0[j];
#pragma unroll
                for (int k = 0; k < CRF_MAX_IN; ++k) s = fmaf(crf.w0[j * CRF_MAX_IN + k], in[k], s);
                h1[j] = fmaxf(s, 0.f);
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                float s = crf.b1[j];
#pragma unroll
                for (int k = 0; k < 16; ++k) s = fmaf(crf.w1[j * 16 + k], h1[k], s);
                h2[j] = fmaxf(s, 0.f);
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                float s = crf.b2[j];
#pragma unroll
                for (int k = 0; k < 16; ++k) s = fmaf(crf.w2[j * 16 + k], h2[k], s);
                h3[j] = fmaxf(s, 0.f);
            }
            float s = crf.b3;
#pragma unroll
            for (int k = 0; k < 16; ++k) s = fmaf(crf.w3[k], h3[k], s);
            v = crf_learn_out(s, xg);
        }
    }
    // ---- luma / log-difference chain (as k_event_loss) and its derivative
    const EventChain ev = event_chain(L, v, tonemap_only, thr_neg, thr_pos, cmask != nullptr, cw0, cw1, cw2, has_cw);
    const float lum = ev.lum, lg = ev.lg;
    const float nxt = dpp_f32<0x104>(0.f, lg), prv = dpp_f32<0x114>(0.f, lg);   // row_shl:4 / row_shr:4: the partner quad's log-luma
    const bool is_end = (which & 1) == 0;
    const float pred = is_end ? lg - nxt : prv - lg;
    const float g = which < 2 ? g_f : g_c;
    const float d_lg = (is_end ? 1.f : -1.f) * 2.f * g * ev.w * (pred - ev.bii);
    const float d_lum = d_lg / (lum + 1e-5f);
    const float coef[3] = {0.299f, 0.587f, 0.114f};
    float d_v = 0.f;
    if (active) d_v = tonemap_only ? (c == ch ? d_lum : 0.f) : d_lum * coef[c];
    // ---- CRF backward
    float d_x = d_v;
    if (learn) {
        const float dz = d_v * v * (1.f - v);          // through the sigmoid of (0.1 s + x)
        const float ds = 0.1f * dz;
        float dh3[16], dh2[16], dh1[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) dh3[k] = h3[k] > 0.f ? ds * crf.w3[k] : 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) a = fmaf(crf.w2[j * 16 + k], dh3[j], a);
            dh2[k] = h2[k] > 0.f ? a : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) a = fmaf(crf.w1[j * 16 + k], dh2[j], a);
            dh1[k] = h1[k] > 0.f ? a : 0.f;
        }
        float din0 = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) din0 = fmaf(crf.w0[j * CRF_MAX_IN], dh1[j], din0);
        d_x = (dz + din0) * dgamma;
        // parameter contributions, summed over the wavefront, then into the block's LDS accumulator
        auto add = [&](int idx, float val) {
            const float t = wave_sum_dpp(val);
            if (lane == 0) {
                if (OWN) pacc[idx] += t;
                else atomicAdd(&pacc[idx], t);
            }
        };
#pragma unroll
        for (int j = 0; j < 16; ++j) {
#pragma unroll
            for (int k = 0; k < 3; ++k) add(O_W0 + j * CRF_MAX_IN + k, dh1[j] * in[k]);
            add(O_B0 + j, dh1[j]);
            add(O_B1 + j, dh2[j]);
            add(O_B2 + j, dh3[j]);
            add(O_W3 + j, ds * h3[j]);
        }
        add(O_B3, ds);
#pragma unroll 4
        for (int j = 0; j < 16; ++j)
#pragma unroll
            for (int k = 0; k < 16; ++k) { add(O_W1 + j * 16 + k, dh2[j] * h1[k]); add(O_W2 + j * 16 + k, dh3[j] * h2[k]); }
    } else {
        d_x = d_v * dgamma;
    }
    if (active) {
        float* dst = which == 0 ? d_end : which == 1 ? d_start : which == 2 ? d_end0 : d_start0;
        if (dst) dst[L.ii * 3 + c] = d_x;
    }
}

__global__ __launch_bounds__(256) void k_event_loss_bwd(const CrfParams crf, int skip_learn, int add_bii_feat, int tonemap_only,
                                                        const float* __restrict__ start, const float* __restrict__ end,
                                                        const float* __restrict__ start0, const float* __restrict__ end0,
                                                        const float* __restrict__ cum_neg, const float* __restrict__ cum_pos,
                                                        float thr_neg, float thr_pos, const unsigned char* __restrict__ cmask,
                                                        float cw0, float cw1, float cw2, int has_cw, long N, float g_f, float g_c,
                                                        const float* __restrict__ gdev, float* __restrict__ d_start, float* __restrict__ d_end,
                                                        float* __restrict__ d_start0, float* __restrict__ d_end0,
                                                        float* __restrict__ d_params) {
    __shared__ float pacc[CRF_NPARAM];
    if (gdev) { g_f = gdev[0]; g_c = gdev[1]; }
    for (int i = threadIdx.x; i < CRF_NPARAM; i += blockDim.x) pacc[i] = 0.f;
    __syncthreads();
    event_loss_bwd_block<false>(crf, skip_learn, add_bii_feat, tonemap_only, start, end, start0, end0, cum_neg, cum_pos, thr_neg, thr_pos, cmask,
                                cw0, cw1, cw2, has_cw, N, blockIdx.x, g_f, g_c, d_start, d_end, d_start0, d_end0, pacc);
    if (crf.map_type == 2 && !skip_learn && d_params) {
        __syncthreads();
        for (int k = threadIdx.x; k < CRF_NPARAM; k += blockDim.x) if (pacc[k] != 0.f) atomicAdd(d_params + k, pacc[k]);
    }
}

// The deterministic form: workgroup b walks the 16-event blocks b, b + gridDim.x, ...; a wavefront's parameter sums (a fixed DPP tree over
// its lanes) are added to the wavefront's OWN LDS slot in block order, the four slots are folded in wavefront order and the workgroup's
// row of partials goes to the handle's buffer (k_det_fold adds the rows in workgroup order).  No LDS and no global float atomic.
__global__ __launch_bounds__(256) void k_event_loss_bwd_det(const CrfParams crf, int skip_learn, int add_bii_feat, int tonemap_only,
                                                            const float* __restrict__ start, const float* __restrict__ end,
                                                            const float* __restrict__ start0, const float* __restrict__ end0,
                                                            const float* __restrict__ cum_neg, const float* __restrict__ cum_pos,
                                                            float thr_neg, float thr_pos, const unsigned char* __restrict__ cmask,
                                                            float cw0, float cw1, float cw2, int has_cw, long N, float g_f, float g_c,
                                                            const float* __restrict__ gdev, float* __restrict__ d_start, float* __restrict__ d_end,
                                                            float* __restrict__ d_start0, float* __restrict__ d_end0, float* __restrict__ wg) {
    __shared__ float pacc[4][CRF_NPARAM];
    if (gdev) { g_f = gdev[0]; g_c = gdev[1]; }
    for (int i = threadIdx.x; i < 4 * CRF_NPARAM; i += blockDim.x) (&pacc[0][0])[i] = 0.f;
    __syncthreads();
    for (long blk = blockIdx.x; blk * 16 < N; blk += gridDim.x)
        event_loss_bwd_block<true>(crf, skip_learn, add_bii_feat, tonemap_only, start, end, start0, end0, cum_neg, cum_pos, thr_neg, thr_pos, cmask,
                                   cw0, cw1, cw2, has_cw, N, blk, g_f, g_c, d_start, d_end, d_start0, d_end0, pacc[threadIdx.x >> 6]);
    __syncthreads();
    for (int k = threadIdx.x; k < CRF_NPARAM; k += blockDim.x) wg[(long)blockIdx.x * CRF_NPARAM + k] = ((pacc[0][k] + pacc[1][k]) + pacc[2][k]) + pacc[3][k];
}

}  // namespace evd

using namespace evd;

struct evd_crf {
    CrfParams p;
    // evd_crf_set_deterministic: the loss entries on this handle launch their deterministic forms; wg [DET_BLOCKS][CRF_NPARAM] holds the
    // per-workgroup partials of the launch in flight (allocated on first enable)
    bool deterministic = false;
    DevBuf wg;
};
static unsigned det_grid(long work_blocks) { return (unsigned)(work_blocks < DET_BLOCKS ? work_blocks : DET_BLOCKS); }

// argument rules common to the event-loss entries
static int event_check(const char* who, const evd_crf* crf_ev, int add_bii_feat, int tonemap_only, const void* start, const void* end,
                       const void* cum_neg, const void* cum_pos, const void* color_mask, bool outputs, long N) {
    EVD_REQUIRE(crf_ev && start && end && cum_neg && cum_pos && outputs && N >= 0, "%s: bad arguments", who);
    EVD_REQUIRE(add_bii_feat >= 0 && add_bii_feat <= 2, "%s: add_bii_feat %d", who, add_bii_feat);
    EVD_REQUIRE(add_bii_feat == 0 || crf_ev->p.map_type != 2 || crf_ev->p.E == 2, "%s: bii features need extra_features == 2", who);
    EVD_REQUIRE(!color_mask || tonemap_only, "%s: a colour mask needs tonemap_only (3-channel luma, utils/events.py:262)", who);
    EVD_REQUIRE(add_bii_feat != 2 || color_mask, "%s: color-pos-neg features need the colour mask", who);
    return EVD_OK;
}
struct ColorWeights {
    float c[3];
    int given;
    explicit ColorWeights(const float* cw) : c{cw ? cw[0] : 1.f, cw ? cw[1] : 1.f, cw ? cw[2] : 1.f}, given(cw != nullptr) {}
};

extern "C" {

int evd_weighted_sum(const float* x, const float* ccw, long R, int P, int C, float* out, void* stream) {
    EVD_REQUIRE(R >= 0 && P >= 1 && C >= 1 && out, "evd_weighted_sum: bad arguments");
    if (R == 0) return EVD_OK;
    k_weighted_sum<<<cdiv(R * C, 256), 256, 0, as_stream(stream)>>>(x, ccw, R, P, C, out);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_crf_create(const evd_crf_desc* d, evd_crf** out) {
    EVD_REQUIRE(d && out, "evd_crf_create: null argument");
    EVD_REQUIRE(d->map_type >= 0 && d->map_type <= 2, "evd_crf_create: map_type %d", d->map_type);
    EVD_REQUIRE(d->extra_features >= 0 && d->extra_features < CRF_MAX_IN, "evd_crf_create: extra_features %d", d->extra_features);
    evd_crf* c = new evd_crf();
    memset(&c->p, 0, sizeof(c->p));
    c->p.map_type = d->map_type;
    c->p.E = d->extra_features;
    c->p.inv_gamma = (float)(1.0 / (double)(d->gamma != 0.f ? d->gamma : 2.2f));   // x ** (1. / gamma), tonemapping.py:68
    if (d->map_type == 2) {
        for (int k = 0; k < 4; ++k)
            if (!d->w[k] || !d->b[k]) { delete c; return fail(EVD_E_INVALID, "evd_crf_create: learn CRF needs 4 weight/bias pairs"); }
        const int nin = 1 + d->extra_features;
        memset(c->p.w0, 0, sizeof(c->p.w0));
        for (int j = 0; j < 16; ++j) memcpy(c->p.w0 + j * CRF_MAX_IN, d->w[0] + j * nin, sizeof(float) * nin);    // rows padded to CRF_MAX_IN
        memcpy(c->p.b0, d->b[0], sizeof(float) * 16);
        memcpy(c->p.w1, d->w[1], sizeof(float) * 256);
        memcpy(c->p.b1, d->b[1], sizeof(float) * 16);
        memcpy(c->p.w2, d->w[2], sizeof(float) * 256);
        memcpy(c->p.b2, d->b[2], sizeof(float) * 16);
        memcpy(c->p.w3, d->w[3], sizeof(float) * 16);
        c->p.b3 = d->b[3][0];
    }
    *out = c;
    return EVD_OK;
}

void evd_crf_destroy(evd_crf* c) {
    if (!c) return;
    c->wg.release();
    delete c;
}

int evd_crf_set_deterministic(evd_crf* c, int on) {
    EVD_REQUIRE(c, "evd_crf_set_deterministic: null handle");
    if (on && !c->wg.p) {
        int rc = c->wg.alloc(sizeof(float) * (size_t)DET_BLOCKS * CRF_NPARAM);
        if (rc) return rc;
    }
    c->deterministic = on != 0;
    return EVD_OK;
}

int evd_crf_forward(const evd_crf* crf, const float* x, const float* feat, int feat_per_channel, int skip_learn,
                    int luma, long n, float* out, void* stream) {
    EVD_REQUIRE(crf && n >= 0 && out && luma <= 2, "evd_crf_forward: bad arguments");
    if (n == 0) return EVD_OK;
    k_crf_forward<<<cdiv(n, 256), 256, 0, as_stream(stream)>>>(crf->p, x, feat, feat_per_channel, skip_learn, luma, n, out);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_blur_loss_reduce(const evd_crf* crf_rgb, int skip_learn, const float* rgb_p, const float* rgb0_p,
                         const float* w1, const float* w2, const float* tgt, const float* tgt0, long R, int P,
                         float* partial, float* out_rgb, float* out_rgb1, float* out_awp, void* stream) {
    EVD_REQUIRE(crf_rgb && rgb_p && w1 && tgt && partial && R >= 0 && P >= 1, "evd_blur_loss_reduce: bad arguments");
    if (R == 0) return EVD_OK;
    if (crf_rgb->deterministic) {
        float* wg = (float*)crf_rgb->wg.p;
        const unsigned blocks = det_grid(cdiv(3 * R, 256));
        k_blur_loss_det<<<blocks, 256, 0, as_stream(stream)>>>(crf_rgb->p, skip_learn, rgb_p, rgb0_p, w1, w2, tgt, tgt0, R, P, wg, out_rgb, out_rgb1, out_awp);
        EVD_LAUNCH_CHECK();
        k_det_fold<<<1, 64, 0, as_stream(stream)>>>(wg, (int)blocks, 6, partial);
        EVD_LAUNCH_CHECK();
        return EVD_OK;
    }
    k_blur_loss<<<cdiv(3 * R, 64), 64, 0, as_stream(stream)>>>(crf_rgb->p, skip_learn, rgb_p, rgb0_p, w1, w2, tgt, tgt0, R, P, partial,
                                                             out_rgb, out_rgb1, out_awp);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

static int blur_loss_bwd(const evd_crf* crf_rgb, int skip_learn, const float* rgb_p, const float* rgb0_p, const float* w1, const float* w2,
                         const float* tgt, const float* tgt0, long R, int P, const float* g_partial, const float* g_dev, float* d_rgb_p,
                         float* d_rgb0_p, float* d_w1, float* d_w2, void* stream) {
    EVD_REQUIRE(crf_rgb && rgb_p && w1 && tgt && (g_partial || g_dev) && d_rgb_p && R >= 0 && P >= 1, "evd_blur_loss_bwd: bad arguments");
    EVD_REQUIRE(crf_rgb->p.map_type != 2 || skip_learn, "evd_blur_loss_bwd: learnable CRF on the image branch is not built (shipped configs: gamma / none)");
    if (R == 0) return EVD_OK;
    hipStream_t st = as_stream(stream);
    if (d_w1) EVD_HIP(hipMemsetAsync(d_w1, 0, sizeof(float) * (size_t)R * P, st));
    if (d_w2) EVD_HIP(hipMemsetAsync(d_w2, 0, sizeof(float) * (size_t)R * P, st));
    const float zero5[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    const float* g = g_partial ? g_partial : zero5;
    if (crf_rgb->deterministic) {
        k_blur_loss_bwd_det<<<cdiv(R, 64), 64, 0, st>>>(crf_rgb->p, skip_learn, rgb_p, rgb0_p, w1, w2, tgt, tgt0, R, P, g[0], g[1], g[2], g[3], g[4], g_dev,
                                                        d_rgb_p, rgb0_p ? d_rgb0_p : nullptr, d_w1, d_w2);
        EVD_LAUNCH_CHECK();
        return EVD_OK;
    }
    k_blur_loss_bwd<<<cdiv(3 * R, 64), 64, 0, st>>>(crf_rgb->p, skip_learn, rgb_p, rgb0_p, w1, w2, tgt, tgt0, R, P, g[0], g[1], g[2], g[3], g[4], g_dev,
                                                    d_rgb_p, rgb0_p ? d_rgb0_p : nullptr, d_w1, d_w2);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_blur_loss_bwd(const evd_crf* crf_rgb, int skip_learn, const float* rgb_p, const float* rgb0_p, const float* w1, const float* w2,
                      const float* tgt, const float* tgt0, long R, int P, const float* g_partial, float* d_rgb_p, float* d_rgb0_p,
                      float* d_w1, float* d_w2, void* stream) {
    EVD_REQUIRE(g_partial, "evd_blur_loss_bwd: bad arguments");
    return blur_loss_bwd(crf_rgb, skip_learn, rgb_p, rgb0_p, w1, w2, tgt, tgt0, R, P, g_partial, nullptr, d_rgb_p, d_rgb0_p, d_w1, d_w2, stream);
}

int evd_blur_loss_bwd_dev(const evd_crf* crf_rgb, int skip_learn, const float* rgb_p, const float* rgb0_p, const float* w1, const float* w2,
                          const float* tgt, const float* tgt0, long R, int P, const float* g_partial_dev, float* d_rgb_p, float* d_rgb0_p,
                          float* d_w1, float* d_w2, void* stream) {
    EVD_REQUIRE(g_partial_dev, "evd_blur_loss_bwd_dev: bad arguments");
    return blur_loss_bwd(crf_rgb, skip_learn, rgb_p, rgb0_p, w1, w2, tgt, tgt0, R, P, nullptr, g_partial_dev, d_rgb_p, d_rgb0_p, d_w1, d_w2, stream);
}

int evd_event_loss_reduce(const evd_crf* crf_ev, int skip_learn, int add_bii_feat, int tonemap_only,
                          const float* start, const float* end, const float* start0, const float* end0,
                          const float* cum_neg, const float* cum_pos, float thr_neg, float thr_pos,
                          const unsigned char* color_mask, const float* color_weight, long N,
                          float* partial, void* stream) {
    if (int e = event_check("evd_event_loss_reduce", crf_ev, add_bii_feat, tonemap_only, start, end, cum_neg, cum_pos, color_mask, partial != nullptr, N)) return e;
    if (N == 0) return EVD_OK;
    const ColorWeights cw(color_weight);
    if (crf_ev->deterministic) {
        float* wg = (float*)crf_ev->wg.p;
        const unsigned blocks = det_grid(cdiv(N, 16));
        k_event_loss_det<<<blocks, 256, 0, as_stream(stream)>>>(crf_ev->p, skip_learn, add_bii_feat, tonemap_only, start, end, start0, end0,
                                                                cum_neg, cum_pos, thr_neg, thr_pos, color_mask, cw.c[0], cw.c[1], cw.c[2], cw.given, N, wg);
        EVD_LAUNCH_CHECK();
        k_det_fold<<<1, 64, 0, as_stream(stream)>>>(wg, (int)blocks, 3, partial);
        EVD_LAUNCH_CHECK();
        return EVD_OK;
    }
    k_event_loss<<<cdiv(N, 16), 256, 0, as_stream(stream)>>>(crf_ev->p, skip_learn, add_bii_feat, tonemap_only, start, end, start0, end0,
                                                              cum_neg, cum_pos, thr_neg, thr_pos, color_mask, cw.c[0], cw.c[1], cw.c[2],
                                                              cw.given, N, partial);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_crf_param_count(void) { return CRF_NPARAM; }

// The handle keeps the (625 + padding) CRF parameters on the HOST (they travel as a kernel argument): get / load exchange them
// with a host array in the gradient layout of evd_event_loss_bwd, so a caller that trains the event-CRF copies 2.8 KB per step.
int evd_crf_get_params(const evd_crf* c, float* host) {
    EVD_REQUIRE(c && host && c->p.map_type == 2, "evd_crf_get_params: needs a learn CRF and a host array");
    crf_walk(c->p, [&](const float* m, int off, int n) { memcpy(host + off, m, sizeof(float) * n); });
    return EVD_OK;
}

int evd_crf_load_params(evd_crf* c, const float* host) {
    EVD_REQUIRE(c && host && c->p.map_type == 2, "evd_crf_load_params: needs a learn CRF and a host array");
    crf_walk(c->p, [&](float* m, int off, int n) { memcpy(m, host + off, sizeof(float) * n); });
    for (int j = 0; j < 16; ++j)
        for (int k = 1 + c->p.E; k < CRF_MAX_IN; ++k) c->p.w0[j * CRF_MAX_IN + k] = 0.f;      // padding columns stay zero
    return EVD_OK;
}

static int event_loss_bwd(const evd_crf* crf_ev, int skip_learn, int add_bii_feat, int tonemap_only,
                          const float* start, const float* end, const float* start0, const float* end0,
                          const float* cum_neg, const float* cum_pos, float thr_neg, float thr_pos,
                          const unsigned char* color_mask, const float* color_weight, long N, float g_fine, float g_coarse, const float* g_dev,
                          float* d_start, float* d_end, float* d_start0, float* d_end0, float* d_params, void* stream) {
    if (int e = event_check("evd_event_loss_bwd", crf_ev, add_bii_feat, tonemap_only, start, end, cum_neg, cum_pos, color_mask, d_start && d_end, N)) return e;
    hipStream_t st = as_stream(stream);
    if (d_params) EVD_HIP(hipMemsetAsync(d_params, 0, sizeof(float) * CRF_NPARAM, st));
    if (N == 0) return EVD_OK;
    const ColorWeights cw(color_weight);
    if (crf_ev->deterministic) {
        float* wg = (float*)crf_ev->wg.p;
        const unsigned blocks = det_grid(cdiv(N, 16));
        k_event_loss_bwd_det<<<blocks, 256, 0, st>>>(crf_ev->p, skip_learn, add_bii_feat, tonemap_only, start, end, start0, end0, cum_neg, cum_pos,
                                                     thr_neg, thr_pos, color_mask, cw.c[0], cw.c[1], cw.c[2], cw.given, N, g_fine, g_coarse, g_dev,
                                                     d_start, d_end, (start0 && end0) ? d_start0 : nullptr, (start0 && end0) ? d_end0 : nullptr, wg);
        EVD_LAUNCH_CHECK();
        if (d_params && crf_ev->p.map_type == 2 && !skip_learn) {
            k_det_fold<<<1, 64, 0, st>>>(wg, (int)blocks, CRF_NPARAM, d_params);
            EVD_LAUNCH_CHECK();
        }
        return EVD_OK;
    }
    k_event_loss_bwd<<<cdiv(N, 16), 256, 0, st>>>(crf_ev->p, skip_learn, add_bii_feat, tonemap_only, start, end, start0, end0, cum_neg, cum_pos,
                                                  thr_neg, thr_pos, color_mask, cw.c[0], cw.c[1], cw.c[2], cw.given, N, g_fine, g_coarse, g_dev,
                                                  d_start, d_end, (start0 && end0) ? d_start0 : nullptr, (start0 && end0) ? d_end0 : nullptr, d_params);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_event_loss_bwd(const evd_crf* crf_ev, int skip_learn, int add_bii_feat, int tonemap_only,
                       const float* start, const float* end, const float* start0, const float* end0,
                       const float* cum_neg, const float* cum_pos, float thr_neg, float thr_pos,
                       const unsigned char* color_mask, const float* color_weight, long N, float g_fine, float g_coarse,
                       float* d_start, float* d_end, float* d_start0, float* d_end0, float* d_params, void* stream) {
    return event_loss_bwd(crf_ev, skip_learn, add_bii_feat, tonemap_only, start, end, start0, end0, cum_neg, cum_pos, thr_neg, thr_pos, color_mask,
                          color_weight, N, g_fine, g_coarse, nullptr, d_start, d_end, d_start0, d_end0, d_params, stream);
}

int evd_event_loss_bwd_dev(const evd_crf* crf_ev, int skip_learn, int add_bii_feat, int tonemap_only,
                           const float* start, const float* end, const float* start0, const float* end0,
                           const float* cum_neg, const float* cum_pos, float thr_neg, float thr_pos,
                           const unsigned char* color_mask, const float* color_weight, long N, const float* g_partial_dev,
                           float* d_start, float* d_end, float* d_start0, float* d_end0, float* d_params, void* stream) {
    EVD_REQUIRE(g_partial_dev, "evd_event_loss_bwd_dev: bad arguments");
    return event_loss_bwd(crf_ev, skip_learn, add_bii_feat, tonemap_only, start, end, start0, end0, cum_neg, cum_pos, thr_neg, thr_pos, color_mask,
                          color_weight, N, 0.f, 0.f, g_partial_dev, d_start, d_end, d_start0, d_end0, d_params, stream);
}

}  // extern "C"
