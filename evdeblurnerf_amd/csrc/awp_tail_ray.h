// The per-ray chains of the AWP tail that two kernels share (awp_tail.h): the weights into LDS and the forward of one ray (k_awp_tail_fwd,
// and k_awp_tail_bwd where it recomputes the forward), and the BatchNorm-to-output finish of one ray (k_awp_tail_finish, k_awp_tail_bwd0).
#pragma once

#include "awp_tail_tile.h"

namespace evd {

__device__ __forceinline__ void tail_stage_weights(const TailKParams& p, const TailLds& L) {
    const TailDims& d = p.d;
    auto copy = [&](float* dst, const float* src, int n) {           // n is a multiple of 4 here except for the odd-width layer 0
        if ((n & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
#pragma unroll 4
            for (int i = threadIdx.x; i < n / 4; i += AT_NT) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
        } else {
#pragma unroll 4
            for (int i = threadIdx.x; i < n; i += AT_NT) dst[i] = src[i];
        }
    };
    for (int l = 0; l < d.n_mot; ++l) {
        copy(L.mw(l), p.w[2 * l], tail_param_size(d, 2 * l));
        copy(L.mb(l), p.w[2 * l + 1], AT_CM);
    }
    const float* const* w = p.w + 2 * d.n_mot;
    copy(L.lin_w, w[TW_LIN_W], AT_CM * AT_WS); copy(L.lin_b, w[TW_LIN_B], AT_CM);
    copy(L.conva, w[TW_CONVA], AT_MID * AT_CM); copy(L.convb, w[TW_CONVB], AT_MID * AT_CM); copy(L.convc, w[TW_CONVC], AT_MID * AT_CM);
    copy(L.convn, w[TW_CONVN], AT_MID * AT_MID); copy(L.convl, w[TW_CONVL], AT_MID * AT_MID); copy(L.convd, w[TW_CONVD], AT_CM * AT_CM);
}

// The forward of one ray into LDS (both the forward kernel and the backward, which recomputes it).  On return (after the final
// barrier): x0, xs[], hi, li, kP, nP, q, aP, ls, kI, nI, aS, f, yb (= convd f, the BatchNorm's input).
__device__ __forceinline__ void tail_forward_ray(const TailKParams& p, const TailLds& L, long r) {
    const TailDims& d = p.d;
    const int tid = at_tid(), P = d.P, S = d.S;
    TileJobs jobs{0};
    // awp.py:89-95, 104-105: [integrated features | view_feature | direction encoding of the first sub-exposure's ray]
    for (int i = tid; i < P * AT_WS; i += AT_NT) {
        const int pp = i >> 6, k = i & 63;
        L.x0[pp * d.IN0 + k] = p.h[r * P * AT_WS + i];
        L.hi[i] = p.h_inter[r * P * AT_WS + i];
    }
    for (int i = tid; i < P * d.VC; i += AT_NT) {
        const int pp = i / d.VC, j = i - pp * d.VC;
        float v;
        if (j < d.VF) v = p.vf[r * d.VF + j];
        else {
            const int e = j - d.VF, axis = e % 3, blk = e / 3;          // blk 0: the direction; 1 + 2 k: sin(2^k d); 2 + 2 k: cos(2^k d)
            const float* rd = p.rays_d + r * P * 3;
            const float dn = rd[axis] / sqrtf(rd[0] * rd[0] + rd[1] * rd[1] + rd[2] * rd[2]);
            if (blk == 0) v = dn;
            else {
                const float arg = dn * (float)(1 << ((blk - 1) >> 1));
                v = ((blk - 1) & 1) ? cosf(arg) : sinf(arg);
            }
        }
        L.x0[pp * d.IN0 + AT_WS + j] = v;
    }
    __syncthreads();
    // awp.py:107-109 (layer 0) and mam.py:72-74 applied to the per-sample part's inter sums
    lin<1>(jobs, L.xs(0), AT_CM, L.x0, d.IN0, L.mw(0), L.mb(0), P, AT_CM, d.IN0);
    lin<0>(jobs, L.li, AT_CM, L.hi, AT_WS, L.lin_w, L.lin_b, P, AT_CM, AT_WS);
    {   // ... and to the intra sums [S, 64] -> ls [S, 32]: 16 x 16 tiles over (samples, channels), a wavefront per tile
        const TileLane t(tid);
        const float* Wg = p.w[2 * d.n_mot + TW_LIN_W];
        const int nst = (S + 15) >> 4;
        for (int tt = tid >> 6; tt < 2 * nst; tt += AT_NT / 64) {
            const int st = tt >> 1, ct = tt & 1;
            const int srow = min(16 * st + t.c, S - 1);
            const f32x4v acc = tile16_h_intra(p.h_intra + (r * S + srow) * AT_WS, Wg + (16 * ct + t.c) * AT_WS, tid);
            const float bias = L.lin_b[16 * ct + t.c];
            t.rows(S - 16 * st, [&](int i, int m) { L.ls[(16 * st + m) * AT_LS + 16 * ct + t.c] = acc[i] + bias; });
        }
    }
    __syncthreads();
    for (int l = 1; l < d.n_mot; ++l) {
        lin<1>(jobs, L.xs(l), AT_CM, L.xs(l - 1), AT_CM, L.mw(l), L.mb(l), P, AT_CM, AT_CM);
        if (l == 1) lin<0>(jobs, L.kP, AT_MID, L.li, AT_CM, L.conva, nullptr, P, AT_MID, AT_CM);            // mam.py:38
        __syncthreads();
    }
    if (d.n_mot == 1) {
        lin<0>(jobs, L.kP, AT_MID, L.li, AT_CM, L.conva, nullptr, P, AT_MID, AT_CM);
        __syncthreads();
    }
    const float* xg = L.xs(d.n_mot - 1);
    lin<0>(jobs, L.q, AT_MID, xg, AT_CM, L.convc, nullptr, P, AT_MID, AT_CM);                               // mam.py:41
    lin<0>(jobs, L.nP, AT_MID, L.kP, AT_MID, L.convn, nullptr, P, AT_MID, AT_MID);                          // mam.py:46
    each_sample(tid, S, [&](int s, int hf) {                                                                // mam.py:39: convb
        float x[AT_CM];
#pragma unroll
        for (int c = 0; c < AT_CM; ++c) x[c] = L.ls[s * AT_LS + c];
        float o[AT_O16] = {};
        rows_dot<AT_CM, AT_O16, AT_O16>(L.convb + hf * AT_O16 * AT_CM, x, o);
#pragma unroll
        for (int j = 0; j < AT_O16; ++j) L.kI[s * AT_LK + hf * AT_O16 + j] = o[j];
    });
    __syncthreads();
    mm<0, false>(jobs, L.aP, P, L.q, AT_MID, 1, L.kP, AT_MID, 1, nullptr, P, P, AT_MID);                   // mam.py:42: logits over the sub-exposures
    each_sample(tid, S, [&](int s, int hf) {                                                                // mam.py:47 (convl), :43 (logits over the samples)
        float x[AT_MID];
#pragma unroll
        for (int c = 0; c < AT_MID; ++c) x[c] = L.kI[s * AT_LK + c];
        float o[AT_O16] = {};
        rows_dot<AT_MID, AT_O16, AT_O16>(L.convl + hf * AT_O16 * AT_MID, x, o);
#pragma unroll
        for (int j = 0; j < AT_O16; ++j) L.nI[s * AT_LK + hf * AT_O16 + j] = o[j];
        p_dot16(L.aS + s, d.SA, L.q, AT_MID, hf, P, x);
    });
    __syncthreads();
    for (int row = tid >> 6; row < P; row += AT_NT / 64) softmax_row(L.aS + row * d.SA, S);          // mam.py:42-43: the softmaxes
    if (int row; small_softmax_row(tid, P, row)) softmax_small(L.aP + row * P, P);
    __syncthreads();
    mm<0, false>(jobs, L.f, AT_CM, L.aP, P, 1, L.nP, 1, AT_MID, nullptr, P, AT_MID, P);                     // mam.py:49
    if ((tid >> 6) == AT_NT / 64 - 1) {                                                               // mam.py:50 (:52: the concatenation)
        const f32x4v acc = tile16(zero4(), L.aS, d.SA, 1, P, L.nI, AT_LK, 1, AT_MID, S);
        const TileLane t(tid);
        t.rows(P, [&](int i, int m) { L.f[m * AT_CM + AT_MID + t.c] = acc[i]; });
    }
    __syncthreads();
    lin<0>(jobs, L.yb, AT_CM, L.f, AT_CM, L.convd, nullptr, P, AT_CM, AT_CM);                               // mam.py:53: convd[0]
    __syncthreads();
}

// mam.py:53 (BatchNorm, residual, leaky_relu) and awp.py:112-115 of one ray on 32 lanes (lane = channel; called by every lane of the
// workgroup, rays past the end compute on the last ray and write nothing); returns through LDS: sh_hm[32] the mean over P, sh_w[P] the
// sigmoids, tot their sum
template <bool KEEP>
__device__ __forceinline__ void finish_ray(const TailFinishParams& p, long r, int c, const float* stat, float* sh_hm, float* sh_w, float& tot,
                                           float (&zkeep)[AT_MAXP]) {
    const int P = p.P;
    const float mean = stat[c], rstd = stat[AT_CM + c], g = p.bn_w[c], b = p.bn_b[c];
    float acc = 0.f;
#pragma unroll
    for (int pp = 0; pp < AT_MAXP; ++pp)
        if (pp < P) {
            const long at = (r * P + pp) * AT_CM + c;
            const float z = p.xg[at] + ((p.y[at] - mean) * rstd * g + b);
            if (KEEP) zkeep[pp] = z;
            acc += z > 0.f ? z : 0.2f * z;
        }
    sh_hm[c] = acc / (float)P;
    __syncthreads();
    if (c < P) {
        float a = p.wl_b[c];
        for (int k = 0; k < AT_CM; ++k) a = fmaf(p.wl_w[c * AT_CM + k], sh_hm[k], a);
        sh_w[c] = 1.0f / (1.0f + expf(-a));
    }
    __syncthreads();
    tot = 0.f;
    for (int j = 0; j < P; ++j) tot += sh_w[j];
}

}  // namespace evd
