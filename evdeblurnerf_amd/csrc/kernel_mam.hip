// AWP consumer, the per-sample part of the MotionAggregationModule: reference networks/dpnerf/mam.py:72-74 (x_local ->
// self.linear, 64 -> 32 on EVERY sample of every sub-exposure ray) and CorrelationModule.forward :29-33 (a 1x1 attention logit per sample,
// one softmax along the samples and one along the sub-exposures, the two softmax-weighted sums of the `curves`).  As written that is a
// Linear over [R P S, 64], a Conv2d, two softmaxes, two multiplies and two reductions over [R, 32, P, S] tensors -- and the same again
// in the backward.  Because the linear map commutes with the weighted sums (the softmax weights of a row / a column sum to 1) and a
// constant added to every logit leaves a softmax unchanged,
//
//      logit[p,s]         = v . (W h[p,s] + b)         = u . h[p,s] + const,        u = W^T v   (64 floats)
//      curver_inter[:,p]  = sum_s alpha[p,s] (W h[p,s] + b) = W (sum_s alpha[p,s] h[p,s]) + b,   alpha = softmax over s
//      curves_intra[:,s]  = sum_p beta[p,s]  (W h[p,s] + b) = W (sum_p beta[p,s]  h[p,s]) + b,   beta  = softmax over p
//
// so the per-sample work is ONE dot product and two weighted sums of h_local itself; the 64 -> 32 map is applied by the caller to the
// [R, P, 64] and [R, S, 64] results (per-ray sized).  h_local [R P, S, 64] float32 is the AWP embedding's output (awp_embed_kernel.h).
//
// HBM-bound: the forward reads h_local twice (logits, then sums: the softmax needs every logit of the ray first; a ray's 64 P S floats
// -- 320 KiB at P = 10, S = 128 -- do not fit the LDS), the backward reads it once and writes d h_local once.
#include "awp_integrate.h"
#include "evd_common.h"
#include "wave_ops.h"

namespace evd {

constexpr int MAM_C = 64, MAM_MAXP = 16, MAM_MAXS = 512;

__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ void fma4(float4& acc, float s, float4 v) {
    acc.x = fmaf(s, v.x, acc.x); acc.y = fmaf(s, v.y, acc.y); acc.z = fmaf(s, v.z, acc.z); acc.w = fmaf(s, v.w, acc.w);
}

// One workgroup per ray; 16 row-groups of 16 lanes, a row-group owns the samples s = g, g + 16, ... of EVERY sub-exposure p (so the
// softmax over p and the intra sum stay inside the group) and a lane 4 of the 64 channels.  A wavefront's four groups read four
// consecutive samples: 1 KiB contiguous per load instruction.
__global__ __launch_bounds__(256) void k_mam_local_fwd(const float* __restrict__ h, const float* __restrict__ u, int P, int S,
                                                       float* __restrict__ h_inter, float* __restrict__ h_intra,
                                                       float* __restrict__ alpha, float* __restrict__ beta) {
    extern __shared__ float lds[];
    float* A = lds;                         // [P][S] logits, then alpha
    float* Bt = A + P * S;                  // [P][S] beta
    float* rmax = Bt + P * S;               // [P] row max, [P] row sum
    float* rsum = rmax + MAM_MAXP;
    float* red = rsum + MAM_MAXP;           // [4 waves][P][64] partial inter sums
    const long b = blockIdx.x;
    const int tid = threadIdx.x, g = tid >> 4, l = tid & 15, wave = tid >> 6, lane = tid & 63;
    const float4* h4 = reinterpret_cast<const float4*>(h) + b * (long)P * S * 16;
    const float4 u4 = reinterpret_cast<const float4*>(u)[l];

    for (int s = g; s < S; s += 16) {
#pragma unroll
        for (int p = 0; p < MAM_MAXP; ++p)
            if (p < P) {
                const float d = row_sum_dpp(dot4(h4[((long)p * S + s) * 16 + l], u4));
                if (l == 0) A[p * S + s] = d;
            }
    }
    __syncthreads();
    // the softmax along the samples: one wavefront per sub-exposure
    for (int p = wave; p < P; p += 4) {
        float m = -INFINITY;
        for (int s = lane; s < S; s += 64) m = fmaxf(m, A[p * S + s]);
        m = wave_max(m);
        float t = 0.f;
        for (int s = lane; s < S; s += 64) t += __expf(A[p * S + s] - m);
        t = wave_sum_dpp(t);
        if (lane == 0) { rmax[p] = m; rsum[p] = t; }
    }
    __syncthreads();
    // the softmax along the sub-exposures: one thread per sample; both weights to LDS and to the saved tensors
    for (int s = tid; s < S; s += 256) {
        float m = -INFINITY, t = 0.f;
        for (int p = 0; p < P; ++p) m = fmaxf(m, A[p * S + s]);
        for (int p = 0; p < P; ++p) t += __expf(A[p * S + s] - m);
        const float it = 1.f / t;
        for (int p = 0; p < P; ++p) {
            const float a = A[p * S + s];
            const float al = __expf(a - rmax[p]) / rsum[p], be = __expf(a - m) * it;
            A[p * S + s] = al;
            Bt[p * S + s] = be;
            alpha[(b * P + p) * S + s] = al;
            beta[(b * P + p) * S + s] = be;
        }
    }
    __syncthreads();
    float4 accP[MAM_MAXP];
#pragma unroll
    for (int p = 0; p < MAM_MAXP; ++p) accP[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = g; s < S; s += 16) {
        float4 accI = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int p = 0; p < MAM_MAXP; ++p)
            if (p < P) {
                const float4 v = h4[((long)p * S + s) * 16 + l];
                fma4(accI, Bt[p * S + s], v);
                fma4(accP[p], A[p * S + s], v);
            }
        reinterpret_cast<float4*>(h_intra)[(b * S + s) * 16 + l] = accI;
    }
    // inter sums: the wavefront's four groups by lane exchange, the four wavefronts through LDS
#pragma unroll
    for (int p = 0; p < MAM_MAXP; ++p)
        if (p < P) {
            float4 a = accP[p];
            a.x += __shfl_xor(a.x, 16); a.y += __shfl_xor(a.y, 16); a.z += __shfl_xor(a.z, 16); a.w += __shfl_xor(a.w, 16);
            a.x += __shfl_xor(a.x, 32); a.y += __shfl_xor(a.y, 32); a.z += __shfl_xor(a.z, 32); a.w += __shfl_xor(a.w, 32);
            if (lane < 16) reinterpret_cast<float4*>(red)[(wave * P + p) * 16 + l] = a;
        }
    __syncthreads();
    for (int i = tid; i < P * MAM_C; i += 256)
        h_inter[b * P * MAM_C + i] = red[i] + red[P * MAM_C + i] + red[2 * P * MAM_C + i] + red[3 * P * MAM_C + i];
}

// The same with the ray's rows REGISTER-RESIDENT between the two phases (P <= PR sub-exposures, S <= 16 NSR samples: 80 sixteen-byte loads
// per thread at the blurfactory shape, all issued in front of the first logit): h_local is read once instead of twice -- the kernel is
// HBM-bound, and a ray's 320 KiB do not fit the LDS but do fit the workgroup's register file (one workgroup of 256 threads per CU).
template <int PR, int NSR>
__global__ __launch_bounds__(256) void k_mam_local_fwd_r(const float* __restrict__ h, const float* __restrict__ u, int P, int S,
                                                         float* __restrict__ h_inter, float* __restrict__ h_intra,
                                                         float* __restrict__ alpha, float* __restrict__ beta) {
    extern __shared__ float lds[];
    float* A = lds;                         // [P][S] logits, then alpha
    float* Bt = A + P * S;                  // [P][S] beta
    float* rmax = Bt + P * S;               // [P] row max, [P] row sum
    float* rsum = rmax + MAM_MAXP;
    float* red = rsum + MAM_MAXP;           // [4 waves][P][64] partial inter sums
    const long b = blockIdx.x;
    const int tid = threadIdx.x, g = tid >> 4, l = tid & 15, wave = tid >> 6, lane = tid & 63;
    const float4* h4 = reinterpret_cast<const float4*>(h) + b * (long)P * S * 16;
    const float4 u4 = reinterpret_cast<const float4*>(u)[l];
    float4 hr[PR][NSR];
#pragma unroll
    for (int p = 0; p < PR; ++p)
#pragma unroll
        for (int j = 0; j < NSR; ++j) {
            const int s = g + 16 * j;
            hr[p][j] = (p < P && s < S) ? h4[((long)p * S + s) * 16 + l] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
    for (int j = 0; j < NSR; ++j)
#pragma unroll
        for (int p = 0; p < PR; ++p) {
            const float d = row_sum_dpp(dot4(hr[p][j], u4));
            if (l == 0 && p < P && g + 16 * j < S) A[p * S + g + 16 * j] = d;
        }
    __syncthreads();
    for (int p = wave; p < P; p += 4) {      // the softmax along the samples: one wavefront per sub-exposure
        float m = -INFINITY;
        for (int s = lane; s < S; s += 64) m = fmaxf(m, A[p * S + s]);
        m = wave_max(m);
        float t = 0.f;
        for (int s = lane; s < S; s += 64) t += __expf(A[p * S + s] - m);
        t = wave_sum_dpp(t);
        if (lane == 0) { rmax[p] = m; rsum[p] = t; }
    }
    __syncthreads();
    for (int s = tid; s < S; s += 256) {     // the softmax along the sub-exposures: one thread per sample
        float m = -INFINITY, t = 0.f;
        for (int p = 0; p < P; ++p) m = fmaxf(m, A[p * S + s]);
        for (int p = 0; p < P; ++p) t += __expf(A[p * S + s] - m);
        const float it = 1.f / t;
        for (int p = 0; p < P; ++p) {
            const float a = A[p * S + s];
            const float al = __expf(a - rmax[p]) / rsum[p], be = __expf(a - m) * it;
            A[p * S + s] = al;
            Bt[p * S + s] = be;
            alpha[(b * P + p) * S + s] = al;
            beta[(b * P + p) * S + s] = be;
        }
    }
    __syncthreads();
    float4 accP[PR];
#pragma unroll
    for (int p = 0; p < PR; ++p) accP[p] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < NSR; ++j) {
        const int s = g + 16 * j;
        if (s < S) {
            float4 accI = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int p = 0; p < PR; ++p)
                if (p < P) {
                    fma4(accI, Bt[p * S + s], hr[p][j]);
                    fma4(accP[p], A[p * S + s], hr[p][j]);
                }
            reinterpret_cast<float4*>(h_intra)[(b * S + s) * 16 + l] = accI;
        }
    }
#pragma unroll
    for (int p = 0; p < PR; ++p)
        if (p < P) {
            float4 a = accP[p];
            a.x += __shfl_xor(a.x, 16); a.y += __shfl_xor(a.y, 16); a.z += __shfl_xor(a.z, 16); a.w += __shfl_xor(a.w, 16);
            a.x += __shfl_xor(a.x, 32); a.y += __shfl_xor(a.y, 32); a.z += __shfl_xor(a.z, 32); a.w += __shfl_xor(a.w, 32);
            if (lane < 16) reinterpret_cast<float4*>(red)[(wave * P + p) * 16 + l] = a;
        }
    __syncthreads();
    for (int i = tid; i < P * MAM_C; i += 256)
        h_inter[b * P * MAM_C + i] = red[i] + red[P * MAM_C + i] + red[2 * P * MAM_C + i] + red[3 * P * MAM_C + i];
}

// Backward.  With gA[p,s] = d_inter[p] . h[p,s], gB[p,s] = d_intra[s] . h[p,s] the two softmax backwards need sum_s alpha gA = d_inter[p] .
// h_inter[p] and sum_p beta gB = d_intra[s] . h_intra[s]: dots of the SAVED outputs, so h_local is read once:
//      d logit = alpha (gA - cP[p]) + beta (gB - cI[s]);   d h = alpha d_inter[p] + beta d_intra[s] + d logit u;   d u = sum d logit h
// The pieces below are shared by k_mam_local_bwd and the fused k_local_consumers_bwd.
struct MamBwdLds {
    float *dP, *cP, *red;                   // [MAXP][64] d_inter of the ray, [MAXP] d_inter[p] . h_inter[p], [4][64] reduction scratch
    float* end;                             // first float past the three
    __device__ explicit MamBwdLds(float* lds) : dP(lds), cP(dP + MAM_MAXP * MAM_C), red(cP + MAM_MAXP), end(red + 4 * MAM_C) {}
};
constexpr int MAM_BWD_LDS_FLOATS = MAM_MAXP * MAM_C + MAM_MAXP + 4 * MAM_C;

// dP <- d_inter of ray b (a barrier has to follow), then cP[p] <- d_inter[p] . h_inter[p] (ends behind a barrier)
__device__ __forceinline__ void mam_bwd_stage_dP(const MamBwdLds& m, const float* d_inter, long b, int P) {
    for (int i = threadIdx.x; i < P * MAM_C; i += 256) m.dP[i] = d_inter[b * P * MAM_C + i];
}
__device__ __forceinline__ void mam_bwd_cP(const MamBwdLds& m, const float* h_inter, long b, int P) {
    const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
    for (int p = g; p < P; p += 16) {
        const float c = row_sum_dpp(dot4(reinterpret_cast<const float4*>(m.dP)[p * 16 + l],
                                         reinterpret_cast<const float4*>(h_inter)[(b * P + p) * 16 + l]));
        if (l == 0) m.cP[p] = c;
    }
    __syncthreads();
}
// d_intra[s] of the lane's four channels and cI[s] = d_intra[s] . h_intra[s]
__device__ __forceinline__ float4 mam_bwd_sample(const float* d_intra, const float* h_intra, long b, int S, int s, float& cI) {
    const int l = threadIdx.x & 15;
    const float4 dI = reinterpret_cast<const float4*>(d_intra)[(b * S + s) * 16 + l];
    cI = row_sum_dpp(dot4(dI, reinterpret_cast<const float4*>(h_intra)[(b * S + s) * 16 + l]));
    return dI;
}
// the MAM's share of d h[p,s] (the lane's four channels) and d logit[p,s] (the caller adds d logit h to its d u)
__device__ __forceinline__ float4 mam_bwd_row(float4 v, float4 dp, float4 dI, float4 u4, float al, float be, float cP, float cI, float& da) {
    const float gA = row_sum_dpp(dot4(dp, v)), gB = row_sum_dpp(dot4(dI, v));
    da = al * (gA - cP) + be * (gB - cI);
    float4 o;
    o.x = al * dp.x + be * dI.x + da * u4.x;
    o.y = al * dp.y + be * dI.y + da * u4.y;
    o.z = al * dp.z + be * dI.z + da * u4.z;
    o.w = al * dp.w + be * dI.w + da * u4.w;
    return o;
}
// running max |d h_local|; fmaxf drops a NaN (or inf - inf): record it as +inf like the scatter's maximum does, not a finite scale word
__device__ __forceinline__ float mam_absmax_row(float amax, float4 o) {
    amax = fmaxf(fmaxf(amax, fmaxf(fabsf(o.x), fabsf(o.y))), fmaxf(fabsf(o.z), fabsf(o.w)));
    const float nan_probe = (o.x + o.y) + (o.z + o.w);
    return nan_probe != nan_probe ? __builtin_huge_valf() : amax;
}
// d_u_partial[b] <- the workgroup's du: the wavefront's four groups by lane exchange, the four wavefronts through LDS (one barrier inside)
__device__ __forceinline__ void mam_bwd_fold_du(const MamBwdLds& m, float4 du, float* d_u_partial, long b) {
    const int tid = threadIdx.x, l = tid & 15, wave = tid >> 6, lane = tid & 63;
    du.x += __shfl_xor(du.x, 16); du.y += __shfl_xor(du.y, 16); du.z += __shfl_xor(du.z, 16); du.w += __shfl_xor(du.w, 16);
    du.x += __shfl_xor(du.x, 32); du.y += __shfl_xor(du.y, 32); du.z += __shfl_xor(du.z, 32); du.w += __shfl_xor(du.w, 32);
    if (lane < 16) reinterpret_cast<float4*>(m.red)[wave * 16 + l] = du;
    __syncthreads();
    if (tid < MAM_C) d_u_partial[b * MAM_C + tid] = m.red[tid] + m.red[MAM_C + tid] + m.red[2 * MAM_C + tid] + m.red[3 * MAM_C + tid];
}
// max |d h_local| of this ray -> the caller's word (guarded: one atomic per raising workgroup, not per ray)
__device__ __forceinline__ void mam_bwd_fold_absmax(const MamBwdLds& m, float amax, unsigned* absmax) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (!absmax) return;
    amax = wave_max(amax);
    __syncthreads();
    if (lane == 0) m.red[wave] = amax;
    __syncthreads();
    if (tid == 0) {
        const unsigned mb = __float_as_uint(fmaxf(fmaxf(m.red[0], m.red[1]), fmaxf(m.red[2], m.red[3])));
        if (mb > *reinterpret_cast<volatile unsigned*>(absmax)) atomicMax(absmax, mb);
    }
}

template <bool ACC>
__global__ __launch_bounds__(256) void k_mam_local_bwd(const float* __restrict__ h, const float* __restrict__ u,
                                                       const float* __restrict__ alpha, const float* __restrict__ beta,
                                                       const float* __restrict__ h_inter, const float* __restrict__ h_intra,
                                                       const float* __restrict__ d_inter, const float* __restrict__ d_intra, int P, int S,
                                                       float* __restrict__ d_h, float* __restrict__ d_u_partial, unsigned* __restrict__ absmax) {
    extern __shared__ float lds[];
    const MamBwdLds m(lds);
    const long b = blockIdx.x;
    const int tid = threadIdx.x, g = tid >> 4, l = tid & 15;
    const float4* h4 = reinterpret_cast<const float4*>(h) + b * (long)P * S * 16;
    float4* dh4 = reinterpret_cast<float4*>(d_h) + b * (long)P * S * 16;
    const float4 u4 = reinterpret_cast<const float4*>(u)[l];
    mam_bwd_stage_dP(m, d_inter, b, P);
    __syncthreads();
    mam_bwd_cP(m, h_inter, b, P);
    float4 du = make_float4(0.f, 0.f, 0.f, 0.f);
    float amax = 0.f;
    for (int s = g; s < S; s += 16) {
        float cI;
        const float4 dI = mam_bwd_sample(d_intra, h_intra, b, S, s, cI);
#pragma unroll
        for (int p = 0; p < MAM_MAXP; ++p)
            if (p < P) {
                const long at = ((long)p * S + s) * 16 + l;
                const float4 dp = reinterpret_cast<const float4*>(m.dP)[p * 16 + l];
                const float4 v = h4[at];
                float da;
                float4 o = mam_bwd_row(v, dp, dI, u4, alpha[(b * P + p) * S + s], beta[(b * P + p) * S + s], m.cP[p], cI, da);
                if (ACC) {                   // d h_local already holds another consumer's share (the feature integration's): add to it here
                    const float4 prev = dh4[at];  // instead of in a separate pass over 2 x 335 MB
                    o.x += prev.x; o.y += prev.y; o.z += prev.z; o.w += prev.w;
                }
                dh4[at] = o;
                amax = mam_absmax_row(amax, o);
                fma4(du, da, v);
            }
    }
    mam_bwd_fold_du(m, du, d_u_partial, b);
    mam_bwd_fold_absmax(m, amax, absmax);
}

// ---- h_local's two consumers in ONE backward pass ----------------------------------------------------------------------------------------
// k_awp_integrate_bwd_c64 (kernel_awp_integrate.hip) and k_mam_local_bwd above both read h_local [R P, S, 64] and produce a d h_local of
// that size; as two launches the second reads the first one's result back and adds to it (1.67 GB of traffic at the blurfactory shape).  Here
// the MAM backward's 16-lane group that owns row (p, s) also evaluates the integration's gradient of that row -- its formulas need rows
// s - 1 and s + 1 of the same sub-exposure, which the neighbouring groups of the workgroup load anyway (cache hits) -- and writes the sum:
// h_local is fetched from HBM once, d h_local written once.  The integration's d z_vals / d rays_d need per-ray sums of d dist: the rows'
// values go through LDS ([P][S]) and are folded after the tile loop.  The two shares are the two kernels' own functions (mam_bwd_row above,
// awp_bwd_row of awp_integrate.h), added in the order of the two-launch path; only Q is obtained differently: a group does not walk the
// samples in order, so it rebuilds row s's Q from row s - 1's exponentials instead of carrying it.
struct LocalBwdParams {
    const float *h, *u, *alpha, *beta, *h_inter, *h_intra, *d_inter, *d_intra;     // the MAM part (k_mam_local_bwd)
    const float *z, *rays_d, *d_int;                                                 // the integration part: z [R P, S], rays_d [R P, 3], d out [R P, 64]
    int P, S;
    float *d_h, *d_u_partial, *d_z, *d_rays_d;                                       // d_z, d_rays_d: may be null
    unsigned* absmax;
};

__global__ __launch_bounds__(256) void k_local_consumers_bwd(const LocalBwdParams q) {
    extern __shared__ float lds[];
    const int P = q.P, S = q.S;
    const MamBwdLds m(lds);
    float* nrm = m.end;                     // [MAXP] |rays_d| of the sub-exposures
    float* zl = nrm + MAM_MAXP;             // [P][S] z_vals of the ray's sub-exposures
    float* dd = zl + P * S;                 // [P][S] d dist of every row
    const long b = blockIdx.x;
    const int tid = threadIdx.x, g = tid >> 4, l = tid & 15, wave = tid >> 6, lane = tid & 63;
    const float4* h4 = reinterpret_cast<const float4*>(q.h) + b * (long)P * S * 16;
    float4* dh4 = reinterpret_cast<float4*>(q.d_h) + b * (long)P * S * 16;
    const float4 u4 = reinterpret_cast<const float4*>(q.u)[l];
    mam_bwd_stage_dP(m, q.d_inter, b, P);
    for (int i = tid; i < P * S; i += 256) zl[i] = q.z[b * P * S + i];
    if (tid < P) nrm[tid] = ray_norm(q.rays_d + (b * P + tid) * 3);
    __syncthreads();
    mam_bwd_cP(m, q.h_inter, b, P);
    float4 du = make_float4(0.f, 0.f, 0.f, 0.f);
    float amax = 0.f;
    for (int s = g; s < S; s += 16) {
        float cI;
        const float4 dI = mam_bwd_sample(q.d_intra, q.h_intra, b, S, s, cI);
        const bool last = s == S - 1;
#pragma unroll 2
        for (int p = 0; p < P; ++p) {
            const long at = ((long)p * S + s) * 16 + l;
            const float4 v = h4[at];
            const float4 vm = h4[s > 0 ? at - 16 : at], vn = h4[last ? at : at + 16];
            const float4 gi = reinterpret_cast<const float4*>(q.d_int)[(b * P + p) * 16 + l];
            const float4 dp = reinterpret_cast<const float4*>(m.dP)[p * 16 + l];
            float da;
            const float4 om4 = mam_bwd_row(v, dp, dI, u4, q.alpha[(b * P + p) * S + s], q.beta[(b * P + p) * S + s], m.cP[p], cI, da);
            float o[4] = {om4.x, om4.y, om4.z, om4.w};
            fma4(du, da, v);
            // ---- the integration's share (row s of sub-exposure p)
            const float* zz = zl + p * S;
            const float norm = nrm[p];
            const float dist = __fmul_rn(awp_dz(zz, s, last), norm), dist_m = s > 0 ? awp_dist(zz, s - 1, S, norm) : 0.f;
            const float dist_n = awp_dist(zz, s + 1, S, norm);
            const float fc[4] = {v.x, v.y, v.z, v.w}, fm[4] = {vm.x, vm.y, vm.z, vm.w}, fn[4] = {vn.x, vn.y, vn.z, vn.w}, gg[4] = {gi.x, gi.y, gi.z, gi.w};
            // awp_bwd_row's steps, written out: wrapped in a function of array arguments hipcc allocates 88 - 96 registers for this loop instead
            // of 79 (one occupancy step); the formulas themselves are awp_integrate.h's
            float Q[4], e[4], om[4], Qn[4], G[4], lsum = 0.f, localm = 1.f, local = 1.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                Q[k] = s > 0 ? awp_om(awp_e(fm[k], dist_m)) : 1.f;       // om of row s - 1 (never the last row)
                localm *= Q[k];
                e[k] = last ? 1.f : awp_e(fc[k], dist);
                om[k] = awp_om(e[k]);
                local *= om[k];
            }
            float exm = AwpRowGroup::excl_mul(localm), ex = AwpRowGroup::excl_mul(local);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                exm *= Q[k]; Q[k] = s > 0 ? exm : 1.f;                   // Q of this row: the cumulative product of row s - 1's om over the channels
                ex *= om[k]; Qn[k] = ex;
                const float en = s + 2 < S ? awp_e(fn[k], dist_n) : 1.f;
                const float an = s + 2 < S ? __fadd_rn(-en, 1.f) : 0.f;
                G[k] = last ? 0.f : gg[k] * an * fn[k] * Qn[k];
                lsum += G[k];
            }
            float sfx = AwpRowGroup::sum_right(lsum), ddist = 0.f;
#pragma unroll
            for (int k = 3; k >= 0; --k) {
                sfx += G[k];
                const float a = last ? 0.f : __fadd_rn(-e[k], 1.f);
                const float through = last ? 0.f : sfx * __builtin_amdgcn_rcpf(om[k]);
                const float ga = gg[k] * Q[k] * fc[k] - through;
                o[k] += last ? 0.f : gg[k] * Q[k] * a + ga * dist * e[k];       // the MAM's share + the integration's
                ddist += last ? 0.f : ga * fc[k] * e[k];
            }
            const float dds = AwpRowGroup::sum(ddist);
            if (l == 0) dd[p * S + s] = dds;
            const float4 o4 = make_float4(o[0], o[1], o[2], o[3]);
            dh4[at] = o4;
            amax = mam_absmax_row(amax, o4);
        }
    }
    mam_bwd_fold_du(m, du, q.d_u_partial, b);
    // d z[s] = (d dist[s - 1] - d dist[s]) |d|;  d rays_d = (sum_s d dist[s] (z[s + 1] - z[s])) d / |d|      (awp.py:61-63)
    if (q.d_z)
        for (int i = tid; i < P * S; i += 256) {
            const int p = i / S, sx = i - p * S;
            q.d_z[b * P * S + i] = ((sx > 0 ? dd[i - 1] : 0.f) - dd[i]) * nrm[p];
        }
    if (q.d_rays_d)
        for (int p = wave; p < P; p += 4) {
            float a = 0.f;
            for (int sx = lane; sx < S - 1; sx += 64) a = fmaf(dd[p * S + sx], zl[p * S + sx + 1] - zl[p * S + sx], a);
            a = wave_sum_dpp(a);
            if (lane < 3) {
                const float* d = q.rays_d + (b * P + p) * 3;
                q.d_rays_d[(b * P + p) * 3 + lane] = nrm[p] > 0.f ? a * d[lane] / nrm[p] : 0.f;
            }
        }
    mam_bwd_fold_absmax(m, amax, q.absmax);
}

}  // namespace evd

using namespace evd;

static int mam_check(const char* who, long R, int P, int S, int C) {
    EVD_REQUIRE(R >= 0 && P >= 1 && S >= 1, "%s: bad sizes", who);
    EVD_REQUIRE(C == MAM_C, "%s: %d channels (built: the embedding's %d)", who, C, MAM_C);
    EVD_REQUIRE(P <= MAM_MAXP && S <= MAM_MAXS, "%s: P = %d, S = %d (built: P <= %d, S <= %d)", who, P, S, MAM_MAXP, MAM_MAXS);
    return EVD_OK;
}

int evd_mam_local_forward(const float* h_local, const float* u, long R, int P, int S, int C, float* h_inter, float* h_intra, float* alpha,
                          float* beta, void* stream) {
    EVD_REQUIRE(h_local && u && h_inter && h_intra && alpha && beta, "evd_mam_local_forward: null argument");
    if (int e = mam_check("evd_mam_local_forward", R, P, S, C)) return e;
    if (R == 0) return EVD_OK;
    const size_t lds = sizeof(float) * ((size_t)2 * P * S + 2 * MAM_MAXP + (size_t)4 * P * MAM_C);
    constexpr size_t lds_max = sizeof(float) * ((size_t)2 * MAM_MAXP * MAM_MAXS + 2 * MAM_MAXP + (size_t)4 * MAM_MAXP * MAM_C);
    EVD_SET_MAX_LDS(k_mam_local_fwd, lds_max);
    if (P <= 10 && S <= 128) {
        EVD_SET_MAX_LDS((k_mam_local_fwd_r<10, 8>), lds_max);
        k_mam_local_fwd_r<10, 8><<<(unsigned)R, 256, lds, as_stream(stream)>>>(h_local, u, P, S, h_inter, h_intra, alpha, beta);
    } else
        k_mam_local_fwd<<<(unsigned)R, 256, lds, as_stream(stream)>>>(h_local, u, P, S, h_inter, h_intra, alpha, beta);
    EVD_HIP(hipGetLastError());
    return EVD_OK;
}

int evd_mam_local_backward(const float* h_local, const float* u, const float* alpha, const float* beta, const float* h_inter,
                           const float* h_intra, const float* d_inter, const float* d_intra, long R, int P, int S, int C, float* d_h_local,
                           float* d_u_partial, int accumulate, unsigned* d_h_absmax, void* stream) {
    EVD_REQUIRE(h_local && u && alpha && beta && h_inter && h_intra && d_inter && d_intra && d_h_local && d_u_partial,
                "evd_mam_local_backward: null argument");
    if (int e = mam_check("evd_mam_local_backward", R, P, S, C)) return e;
    if (R == 0) return EVD_OK;
    if (d_h_absmax) EVD_HIP(hipMemsetAsync(d_h_absmax, 0, sizeof(unsigned), as_stream(stream)));     // the kernel raises the word; the entry owns its start value
    const size_t lds = sizeof(float) * MAM_BWD_LDS_FLOATS;
    if (accumulate)
        k_mam_local_bwd<true><<<(unsigned)R, 256, lds, as_stream(stream)>>>(h_local, u, alpha, beta, h_inter, h_intra, d_inter, d_intra, P, S,
                                                                            d_h_local, d_u_partial, d_h_absmax);
    else
        k_mam_local_bwd<false><<<(unsigned)R, 256, lds, as_stream(stream)>>>(h_local, u, alpha, beta, h_inter, h_intra, d_inter, d_intra, P, S,
                                                                             d_h_local, d_u_partial, d_h_absmax);
    EVD_HIP(hipGetLastError());
    return EVD_OK;
}

int evd_awp_local_consumers_backward(const float* h_local, const float* u, const float* alpha, const float* beta, const float* h_inter,
                                     const float* h_intra, const float* d_inter, const float* d_intra, const float* z, const float* rays_d,
                                     const float* d_integrated, long R, int P, int S, int C, float* d_h_local, float* d_u_partial, float* d_z,
                                     float* d_rays_d, unsigned* d_h_absmax, void* stream) {
    EVD_REQUIRE(h_local && u && alpha && beta && h_inter && h_intra && d_inter && d_intra && z && rays_d && d_integrated && d_h_local && d_u_partial,
                "evd_awp_local_consumers_backward: null argument");
    if (int e = mam_check("evd_awp_local_consumers_backward", R, P, S, C)) return e;
    if (R == 0) return EVD_OK;
    if (d_h_absmax) EVD_HIP(hipMemsetAsync(d_h_absmax, 0, sizeof(unsigned), as_stream(stream)));
    LocalBwdParams q{};
    q.h = h_local; q.u = u; q.alpha = alpha; q.beta = beta; q.h_inter = h_inter; q.h_intra = h_intra; q.d_inter = d_inter; q.d_intra = d_intra;
    q.z = z; q.rays_d = rays_d; q.d_int = d_integrated; q.P = P; q.S = S;
    q.d_h = d_h_local; q.d_u_partial = d_u_partial; q.d_z = d_z; q.d_rays_d = d_rays_d; q.absmax = d_h_absmax;
    const size_t lds = sizeof(float) * (MAM_BWD_LDS_FLOATS + MAM_MAXP + (size_t)2 * P * S);
    EVD_SET_MAX_LDS(k_local_consumers_bwd, sizeof(float) * (MAM_BWD_LDS_FLOATS + MAM_MAXP + (size_t)2 * MAM_MAXP * MAM_MAXS));
    k_local_consumers_bwd<<<(unsigned)R, 256, lds, as_stream(stream)>>>(q);
    EVD_HIP(hipGetLastError());
    return EVD_OK;
}
