// The AWP tail's backward (awp_tail.h): k_awp_tail_bwd0, k_awp_tail_bwd, k_awp_tail_reduce and evd_awp_tail_backward.  k_awp_tail_bwd walks a
// ray's chain backwards in named phases over (p, L, jobs, part, r, tid): kernel parameters, the ray's LDS arrays, the tile-job counter (ONE
// sequence per ray through all phases), the workgroup's partial row of parameter gradients, the ray, the ray loop's at_tid().
#include "awp_tail_ray.h"

namespace evd {

// d out -> d z, and this workgroup's partial sums of d beta, d gamma (BatchNorm) and d w_linear
__global__ __launch_bounds__(AT_FT) void k_awp_tail_bwd0(TailFinishParams p) {
    __shared__ float stat[2 * AT_CM], hm[AT_FR][AT_CM], sw[AT_FR][AT_MAXP], dpre[AT_FR][AT_MAXP], red[AT_FR][2 * AT_CM];
    const int tid = threadIdx.x, P = p.P;
    if (tid < 2 * AT_CM) stat[tid] = p.stats[tid];
    __syncthreads();
    const int slot = tid >> 5, c = tid & 31;
    const long r = (long)blockIdx.x * AT_FR + slot;
    float dbeta = 0.f, dgamma = 0.f;
    for (int j = tid; j < AT_FR * AT_MAXP; j += AT_FT) (&dpre[0][0])[j] = 0.f;
    float tot, z[AT_MAXP];
    finish_ray<true>(p, r < p.R ? r : p.R - 1, c, stat, hm[slot], sw[slot], tot, z);
    if (r >= p.R) hm[slot][c] = 0.f;                           // (rays past the end add nothing to d w_linear)
    if (r < p.R) {
        // out_j = w_j / tot:  d w_j = (g_j - sum_k g_k out_k) / tot;  d pre_j = d w_j w_j (1 - w_j)
        float dot = 0.f;
        for (int j = 0; j < P; ++j) dot = fmaf(p.d_out[r * P + j], sw[slot][j] / tot, dot);
        if (c < P) {
            const float w = sw[slot][c];
            dpre[slot][c] = (p.d_out[r * P + c] - dot) / tot * w * (1.0f - w);
        }
    }
    __syncthreads();
    if (r < p.R) {
        float dhm = 0.f;
        for (int j = 0; j < P; ++j) dhm = fmaf(dpre[slot][j], p.wl_w[j * AT_CM + c], dhm);
        dhm /= (float)P;
        const float mean = stat[c], rstd = stat[AT_CM + c];
#pragma unroll
        for (int pp = 0; pp < AT_MAXP; ++pp)
            if (pp < P) {
                const long at = (r * P + pp) * AT_CM + c;
                const float dzv = z[pp] > 0.f ? dhm : 0.2f * dhm;
                p.dz[at] = dzv;
                dbeta += dzv;
                dgamma = fmaf(dzv, (p.y[at] - mean) * rstd, dgamma);
            }
    }
    red[slot][c] = dbeta;
    red[slot][AT_CM + c] = dgamma;
    __syncthreads();
    float* part = p.partB + (long)blockIdx.x * p.partB_stride;
    if (tid < 2 * AT_CM) {
        float a = 0.f;
        for (int s = 0; s < AT_FR; ++s) a += red[s][tid];
        part[tid] = a;
    }
    for (int i = tid; i < P * AT_CM + P; i += AT_FT) {          // d w_linear.weight[j][k] = sum_rays d pre_j hm_k;  .bias[j] = sum d pre_j
        float a = 0.f;
        if (i < P * AT_CM) {
            const int j = i / AT_CM, k = i - j * AT_CM;
            for (int s = 0; s < AT_FR; ++s) a = fmaf(dpre[s][j], hm[s][k], a);
        } else {
            for (int s = 0; s < AT_FR; ++s) a += dpre[s][i - P * AT_CM];
        }
        part[2 * AT_CM + i] = a;
    }
}

// the ray's forward state into LDS: the block the forward saved, or the forward once more
__device__ __forceinline__ void bwd_restore_ray(const TailKParams& p, const TailLds& L, long r, int tid) {
    if (p.saved) {
        const float4* src = reinterpret_cast<const float4*>(p.saved + r * L.ray_floats);
        float4* dst = reinterpret_cast<float4*>(L.x0);
        const int n4 = L.ray_floats / 4;
        for (int i0 = 0; i0 < n4; i0 += 8 * AT_NT) {         // eight 16-byte loads per thread in flight (the block is one trip at P = 10, S = 128)
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + tid + u * AT_NT;
                v[u] = src[i < n4 ? i : 0];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + tid + u * AT_NT;
                if (i < n4) dst[i] = v[u];
            }
        }
        __syncthreads();
    } else {
        tail_forward_ray(p, L, r);
    }
}

// BatchNorm backward (mam.py:24-27 in training: batch statistics; eval: the running estimates are constants), the residual, and convd
__device__ __forceinline__ void bwd_batchnorm(const TailKParams& p, const TailLds& L, const TailBwdStatic& st, TileJobs& jobs, float* part, long r, int tid) {
    const int P = p.d.P, wb = 2 * p.d.n_mot;
    for (int i = tid; i < P * AT_CM; i += AT_NT) {
        const int c = i & 31;
        const float dzv = p.dz[r * P * AT_CM + i];
        const float g = p.w[wb + TW_BN_W][c] * st.stat[AT_CM + c];
        const float yh = (L.yb[i] - st.stat[c]) * st.stat[AT_CM + c];
        L.yb[i] = p.training ? g * (dzv - st.sums[c] - yh * st.sums[AT_CM + c]) : g * dzv;        // d y
        L.dxa[i] = dzv;                                                                             // d x_global, the residual's share
    }
    __syncthreads();
    wacc(jobs, part + p.off[wb + TW_CONVD], L.yb, AT_CM, L.f, AT_CM, P, AT_CM, AT_CM);
    mm<0, false>(jobs, L.df, AT_CM, L.yb, AT_CM, 1, L.convd, 1, AT_CM, nullptr, P, AT_CM, AT_CM);      // d f = d y convd
    __syncthreads();
}

// attention over the sub-exposures (mam.py:42, 46, 49) and over the samples (:43, 47, 50): d f -> d q, d kP, d kI; d convn, d convl
__device__ __forceinline__ void bwd_attentions(const TailKParams& p, const TailLds& L, TileJobs& jobs, float* part, long r, int tid) {
    const TailDims& d = p.d;
    const int P = d.P, S = d.S, wb = 2 * d.n_mot;
    mm<0, false>(jobs, L.daP, P, L.df, AT_CM, 1, L.nP, AT_MID, 1, nullptr, P, P, AT_MID);              // d aP[p][p'] = d fP[p] . nP[p']
    mm<0, false>(jobs, L.dnP, AT_MID, L.aP, 1, P, L.df, 1, AT_CM, nullptr, P, AT_MID, P);              // d nP[p'][m] = sum_p aP[p][p'] d fP[p][m]
    each_sample(tid, S, [&](int s, int hf) {
        float x[AT_MID];
#pragma unroll
        for (int c = 0; c < AT_MID; ++c) x[c] = L.nI[s * AT_LK + c];
        p_dot16(L.daS + s, d.SA, L.df + AT_MID, AT_CM, hf, P, x);                                // d aS[p][s] = d fI[p] . nI[s]
    });
    __syncthreads();
    each_sample(tid, S, [&](int s, int hf) {                                                         // d nI[s][m] = sum_p aS[p][s] d fI[p][m]  (into nI's place)
        float acc[AT_O16] = {};
        p_acc<AT_O16>(L.aS + s, d.SA, L.df + AT_MID + hf * AT_O16, AT_CM, P, acc);
#pragma unroll
        for (int j = 0; j < AT_O16; ++j) L.nI[s * AT_LK + hf * AT_O16 + j] = acc[j];
    });
    for (int row = tid >> 6; row < P; row += AT_NT / 64) softmax_row_bwd(L.aS + row * d.SA, L.daS + row * d.SA, S);
    if (int row; small_softmax_row(tid, P, row)) softmax_small_bwd(L.aP + row * P, L.daP + row * P, P);
    __syncthreads();
    float* dnI = L.nI;
    // d q = d lgP kP + d lgS kI;  d kP = d lgP^T q + d nP convn;  d kI = d lgS^T q + d nI convl
    const int wave = tid >> 6;
    const TileLane t(tid);
    if (wave == 0) {
        f32x4v acc = tile16(zero4(), L.daS, d.SA, 1, P, L.kI, AT_LK, 1, AT_MID, S);
        acc = tile16(acc, L.daP, P, 1, P, L.kP, AT_MID, 1, AT_MID, P);
        t.rows(P, [&](int i, int m) { L.dq[m * AT_MID + t.c] = acc[i]; });
    }
    if (jobs.mine()) {                                                                                // d kP = d lgP^T q + d nP convn (one tile, one owner)
        f32x4v acc = tile16(zero4(), L.daP, 1, P, P, L.q, AT_MID, 1, AT_MID, P);
        acc = tile16(acc, L.dnP, AT_MID, 1, P, L.convn, AT_MID, 1, AT_MID, AT_MID);
        t.rows(P, [&](int i, int m) { L.dkP[m * AT_MID + t.c] = acc[i]; });
    }
    wacc(jobs, part + p.off[wb + TW_CONVN], L.dnP, AT_MID, L.kP, AT_MID, P, AT_MID, AT_MID);
    if (wave == 1) {                                                                                  // d convl[m'][m] = sum_s d nI[s][m'] kI[s][m]
        const f32x4v acc = tile16(zero4(), dnI, 1, AT_LK, AT_MID, L.kI, AT_LK, 1, AT_MID, S);
        t.rows(AT_MID, [&](int i, int m) { part[p.off[wb + TW_CONVL] + m * AT_MID + t.c] += acc[i]; });
    }
    each_sample(tid, S, [&](int s, int hf) {
        float acc[AT_O16] = {}, g[AT_MID];
        p_acc<AT_O16>(L.daS + s, d.SA, L.q + hf * AT_O16, AT_MID, P, acc);
#pragma unroll
        for (int m = 0; m < AT_MID; ++m) g[m] = dnI[s * AT_LK + m];
        cols_acc<AT_MID, AT_O16, 8>(L.convl + hf * AT_O16, AT_MID, g, acc);
#pragma unroll
        for (int j = 0; j < AT_O16; ++j) L.dkI[s * AT_LK + hf * AT_O16 + j] = acc[j];
    });
    __syncthreads();
}

// conva / convb / convc, and back through MAM.linear: d kP, d kI, d q -> d li, d ls, d x_global; d h_inter, d h_intra to HBM
__device__ __forceinline__ void bwd_convs_and_linear(const TailKParams& p, const TailLds& L, TileJobs& jobs, float* part, long r, int tid) {
    const TailDims& d = p.d;
    const int P = d.P, S = d.S, wb = 2 * d.n_mot, wave = tid >> 6;
    const long* off = p.off;
    const TileLane t(tid);
    wacc(jobs, part + off[wb + TW_CONVA], L.dkP, AT_MID, L.li, AT_CM, P, AT_MID, AT_CM);
    if (wave == 2 || wave == 3) {                                                                     // d convb[m][c] = sum_s d kI[s][m] ls[s][c]
        const int ct = wave - 2;
        const f32x4v acc = tile16(zero4(), L.dkI, 1, AT_LK, AT_MID, L.ls + 16 * ct, AT_LS, 1, 16, S);
        t.rows(AT_MID, [&](int i, int m) { part[off[wb + TW_CONVB] + m * AT_CM + 16 * ct + t.c] += acc[i]; });
    }
    wacc(jobs, part + off[wb + TW_CONVC], L.dq, AT_MID, L.xs(d.n_mot - 1), AT_CM, P, AT_MID, AT_CM);
    mm<0, false>(jobs, L.dli, AT_CM, L.dkP, AT_MID, 1, L.conva, 1, AT_CM, nullptr, P, AT_CM, AT_MID);
    mm<0, true>(jobs, L.dxa, AT_CM, L.dq, AT_MID, 1, L.convc, 1, AT_CM, nullptr, P, AT_CM, AT_MID);   // d x_global += d q convc
    each_sample(tid, S, [&](int s, int hf) {                                                          // d ls[s] = d kI[s] convb
        float acc[AT_O32] = {}, g[AT_MID];
#pragma unroll
        for (int m = 0; m < AT_MID; ++m) g[m] = L.dkI[s * AT_LK + m];
        cols_acc<AT_MID, AT_O32, 8>(L.convb + hf * AT_O32, AT_CM, g, acc);
#pragma unroll
        for (int j = 0; j < AT_O32; ++j) L.dls[s * AT_LS + hf * AT_O32 + j] = acc[j];
    });
    __syncthreads();
    {   // d MAM.linear.weight [32][64] += d ls^T h_intra + d li^T h_inter: eight 16 x 16 tiles, one per wavefront (AT_NT / 64 == 8)
        const int ct = wave & 1, kt = wave >> 1;
        float* dst = part + off[wb + TW_LIN_W] + 16 * ct * AT_WS + 16 * kt + t.c;
        float old[4];
        t.rows(16, [&](int i, int m) { old[i] = dst[m * AT_WS]; });
        f32x4v acc = tile16_samples(zero4(), L.dls + 16 * ct + t.c, AT_LS, p.h_intra + r * S * AT_WS + 16 * kt + t.c, AT_WS, S, tid);
        acc = tile16(acc, L.dli + 16 * ct, 1, AT_CM, 16, L.hi + 16 * kt, AT_WS, 1, 16, P);
        t.rows(16, [&](int i, int m) { dst[m * AT_WS] = old[i] + acc[i]; });
    }
    for (int n0 = 0; n0 < AT_CM; n0 += 16)                                                            // d MAM.linear.bias = the column sums of d li and d ls
        if (jobs.mine()) {
            f32x4v acc = tile16(zero4(), L.dli + n0, 1, AT_CM, 16, L.tmp + 63, 0, 0, 16, P);
            acc = tile16(acc, L.dls + n0, 1, AT_LS, 16, L.tmp + 63, 0, 0, 16, S);
            if (t.c == 0) t.rows(16, [&](int i, int m) { part[off[wb + TW_LIN_B] + n0 + m] += acc[i]; });
        }
    mm<0, false>(jobs, p.d_hi + r * P * AT_WS, AT_WS, L.dli, AT_CM, 1, L.lin_w, 1, AT_WS, nullptr, P, AT_WS, AT_CM);
    {   // d h_intra [S][64] = d ls MAM.linear.weight: tiles over (samples, k), K = 32
        const int nst = (S + 15) >> 4;
        for (int tt = wave; tt < 4 * nst; tt += AT_NT / 64) {
            const int st = tt >> 2, kt = tt & 3;
            const f32x4v acc = tile16(zero4(), L.dls + 16 * st * AT_LS, AT_LS, 1, min(16, S - 16 * st), L.lin_w + 16 * kt, AT_WS, 1, 16, AT_CM);
            t.rows(16, [&](int i, int m) {
                const int so = 16 * st + m;
                if (so < S) p.d_hs[(r * S + so) * AT_WS + 16 * kt + t.c] = acc[i];
            });
        }
    }
}

// the motion embedding backwards (awp.py:107-109) -> d [integrated features | view_feature | direction encoding] of every sub-exposure, [P][IN0]
__device__ __forceinline__ const float* bwd_motion_embedding(const TailKParams& p, const TailLds& L, TileJobs& jobs, float* part, long r, int tid) {
    const TailDims& d = p.d;
    const int P = d.P;
    float *dx = L.dxa, *dprev = L.dxb;
    for (int l = d.n_mot - 1; l >= 0; --l) {
        __syncthreads();
        for (int i = tid; i < P * AT_CM; i += AT_NT) dx[i] = L.xs(l)[i] > 0.f ? dx[i] : 0.f;
        __syncthreads();
        const int K = l == 0 ? d.IN0 : AT_CM;
        const float* xin = l == 0 ? L.x0 : L.xs(l - 1);
        wacc(jobs, part + p.off[2 * l], dx, AT_CM, xin, K, P, AT_CM, K);
        bacc(jobs, part + p.off[2 * l + 1], dx, AT_CM, P, AT_CM, L.tmp + 63);
        mm<0, false>(jobs, dprev, K, dx, AT_CM, 1, L.mw(l), 1, K, nullptr, P, K, AT_CM);
        float* t = dx; dx = dprev; dprev = t;
    }
    __syncthreads();
    return dx;
}

// dx [P][IN0] to HBM: d h, d view_feature (summed over P) and, through the direction encoding, d rays_d (awp.py:89-95)
__device__ __forceinline__ void bwd_inputs(const TailKParams& p, const TailLds& L, const float* dx, long r, int tid) {
    const TailDims& d = p.d;
    const int P = d.P;
    for (int i = tid; i < P * AT_WS; i += AT_NT) p.d_h[r * P * AT_WS + i] = dx[(i >> 6) * d.IN0 + (i & 63)];
    for (int j = tid; j < d.VC; j += AT_NT) {
        float a = 0.f;
        for (int pp = 0; pp < P; ++pp) a += dx[pp * d.IN0 + AT_WS + j];
        if (j < d.VF) p.d_vf[r * d.VF + j] = a;
        else L.tmp[j - d.VF] = a;
    }
    __syncthreads();
    if (tid < 3 * P) {
        float out = 0.f;
        if (tid < 3 && d.F >= 0) {                                 // awp.py:89-92: d (d / |d|) of the first sub-exposure's ray
            const float* rd = p.rays_d + r * P * 3;
            const float nrm = sqrtf(rd[0] * rd[0] + rd[1] * rd[1] + rd[2] * rd[2]);
            float mine = 0.f, dotv = 0.f;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float dn = rd[a] / nrm;
                float g = L.tmp[a];
                for (int k = 0; k < d.F; ++k) {
                    const float fr = (float)(1 << k), arg = dn * fr;
                    g = fmaf(L.tmp[3 + 6 * k + a], fr * cosf(arg), g);
                    g = fmaf(L.tmp[6 + 6 * k + a], -fr * sinf(arg), g);
                }
                mine = a == tid ? g : mine;
                dotv = fmaf(g, dn, dotv);
            }
            out = (mine - rd[tid] / nrm * dotv) / nrm;
        }
        p.d_rays[r * P * 3 + tid] = out;
    }
    __syncthreads();
}

__global__ __launch_bounds__(AT_NT) void k_awp_tail_bwd(TailKParams p) {
    extern __shared__ float lds[];
    __shared__ TailBwdStatic st;
    TailLds L;
    tail_lds_layout(lds, p.d, true, L);
    tail_stage_weights(p, L);
    const int tid0 = threadIdx.x;
    {   // d beta, d gamma over all rays (k_awp_tail_bwd0's partial rows)
        const int col = tid0 & 63, grp = tid0 >> 6;
        double a = 0.0;
        for (int i = grp; i < p.nblkB; i += AT_NT / 64) a += (double)p.partB[(long)i * p.partB_stride + col];
        st.redd[grp][col] = a;
        if (tid0 < 2 * AT_CM) st.stat[tid0] = p.stats[tid0];
    }
    float* part = p.partA + (long)blockIdx.x * p.partA_stride;
    if (tid0 == 0) L.tmp[63] = 1.0f;                        // the column of ones of the bias-gradient tiles
    for (long i = tid0; i < p.off[p.nw]; i += AT_NT) part[i] = 0.f;
    __syncthreads();
    if (tid0 < 2 * AT_CM) {
        double a = 0.0;
        for (int g = 0; g < AT_NT / 64; ++g) a += st.redd[g][tid0];
        st.sums[tid0] = (float)(a / ((double)p.R * p.d.P));
    }
    __syncthreads();
    for (long r = blockIdx.x; r < p.R; r += gridDim.x) {
        const int tid = at_tid();                           // (per ray: see at_tid)
        TileJobs jobs{0};
        bwd_restore_ray(p, L, r, tid);
        bwd_batchnorm(p, L, st, jobs, part, r, tid);
        bwd_attentions(p, L, jobs, part, r, tid);
        bwd_convs_and_linear(p, L, jobs, part, r, tid);
        const float* dx = bwd_motion_embedding(p, L, jobs, part, r, tid);
        bwd_inputs(p, L, dx, r, tid);
    }
}

// d_params[i] = sum over the partial rows; the BatchNorm and w_linear gradients come from k_awp_tail_bwd0's rows (d beta, d gamma, d W, d b).
// 64 parameters per workgroup, its four wavefronts each a quarter of the rows (fold_rows), folded through LDS.
__global__ __launch_bounds__(256) void k_awp_tail_reduce(TailReduceParams p) {
    __shared__ float fold[4][64];
    const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const long i = (long)blockIdx.x * 64 + col;
    float a = 0.f;
    if (i < p.total) {
        const bool tail = i < p.n_tail;
        const long j = i - p.n_tail;                                   // 0..31 d gamma, 32..63 d beta, then w_linear
        const long c = tail ? i : (j < AT_CM ? AT_CM + j : (j < 2 * AT_CM ? j - AT_CM : j));
        const float* src = tail ? p.partA : p.partB;
        const long stride = tail ? p.partA_stride : p.partB_stride;
        a = fold_rows(src, stride, c, tail ? p.nA : p.nB, grp);
    }
    fold[grp][col] = a;
    __syncthreads();
    if (grp == 0 && i < p.total) p.d_params[i] = (fold[0][col] + fold[1][col]) + (fold[2][col] + fold[3][col]);
}

}  // namespace evd

using namespace evd;

extern "C" int evd_awp_tail_backward(const evd_awp_tail_desc* d, const float* const* params, const float* h, const float* view_feature,
                                     const float* rays_d, const float* h_inter, const float* h_intra, long R, const float* saved_y,
                                     const float* saved_xg, const float* saved_stats, const float* saved_rays, const float* d_out, float* d_h,
                                     float* d_view_feature, float* d_rays_d, float* d_h_inter, float* d_h_intra, float* d_params, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    TailDims dims;
    size_t lds = 0;
    if (int e = tail_check("evd_awp_tail_backward", d, R, true, dims, lds)) return e;
    EVD_REQUIRE(params && h && rays_d && h_inter && h_intra && saved_y && saved_xg && saved_stats && d_out && d_h && d_rays_d && d_h_inter &&
                    d_h_intra && d_params && workspace,
                "evd_awp_tail_backward: null argument");
    EVD_REQUIRE(dims.VF == 0 || (view_feature && d_view_feature), "evd_awp_tail_backward: view_feature / d_view_feature missing (VF = %d)", dims.VF);
    for (int i = 0; i < evd_awp_tail_num_params(dims.n_mot); ++i) EVD_REQUIRE(params[i], "evd_awp_tail_backward: parameter %d missing", i);
    TailBwdWs ws;
    const size_t need = tail_bwd_layout(dims, R, workspace, &ws);
    const int grid = ws.grid, nblk = ws.nblk, strideB = tail_partB_stride(dims.P);
    if (workspace_bytes < need) return fail(EVD_E_WORKSPACE, "evd_awp_tail_backward: workspace %zu < %zu bytes", workspace_bytes, need);
    const long total = tail_param_total(dims);
    if (R == 0) {
        EVD_HIP(hipMemsetAsync(d_params, 0, sizeof(float) * (size_t)total, as_stream(stream)));
        return EVD_OK;
    }
    TailFinishParams f{};
    tail_fill_finish(f, dims, d, params, R, saved_y, saved_xg, saved_stats);
    f.nblk = nblk; f.d_out = d_out; f.dz = ws.dz; f.partB = ws.partB; f.partB_stride = strideB;
    k_awp_tail_bwd0<<<nblk, AT_FT, 0, as_stream(stream)>>>(f);
    EVD_HIP(hipGetLastError());
    TailKParams k{};
    tail_fill(k, dims, d, params, R, h, view_feature, rays_d, h_inter, h_intra, saved_y, saved_xg, saved_rays);
    k.dz = ws.dz; k.stats = saved_stats; k.partB = ws.partB; k.nblkB = nblk; k.partB_stride = strideB;
    k.partA_stride = tail_partA_stride(dims);
    k.d_h = d_h; k.d_vf = d_view_feature; k.d_rays = d_rays_d; k.d_hi = d_h_inter; k.d_hs = d_h_intra; k.partA = ws.partA;
    EVD_SET_MAX_LDS(k_awp_tail_bwd, AT_LDS_CU - AT_LDS_BWD_FIXED);
    k_awp_tail_bwd<<<grid, AT_NT, lds, as_stream(stream)>>>(k);
    EVD_HIP(hipGetLastError());
    TailReduceParams rp{};
    rp.partA = ws.partA; rp.partB = ws.partB; rp.nA = grid; rp.nB = nblk; rp.partB_stride = strideB; rp.P = dims.P; rp.total = total;
    rp.partA_stride = k.partA_stride;
    rp.n_tail = (int)k.off[2 * dims.n_mot + TW_BN_W];
    rp.d_params = d_params;
    k_awp_tail_reduce<<<(unsigned)((total + 63) / 64), 256, 0, as_stream(stream)>>>(rp);
    EVD_HIP(hipGetLastError());
    return EVD_OK;
}
