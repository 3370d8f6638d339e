// AdaptiveWeightProposal.feature_integration (networks/dpnerf/awp.py:49-77), the AWP consumer's compositing scan, and its backward (the
// autograd node behind it under training, awp.py:98-104).  The row formulas are in awp_integrate.h; here are the four kernels' load schedules.
// HBM-bound (reads N x S x C floats once).  General form: a wavefront owns one ray, a lane CPL consecutive channels; per sample row one
// inclusive product scan over the lanes (Q of the next row) and, backward, one suffix sum over the lanes.
#include "awp_integrate.h"
#include "evd_common.h"

namespace evd {

template <int CPL>
__global__ __launch_bounds__(256) void k_awp_integrate(const float* __restrict__ feat, const float* __restrict__ z,
                                                       const float* __restrict__ rays_d, long N, int S, int C, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long n = blockIdx.x * (long)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (n >= N) return;
    const float norm = ray_norm(rays_d + n * 3);
    const float* fr = feat + n * (long)S * C;
    const float* zz = z + n * (long)S;
    float acc[CPL], Q[CPL];
#pragma unroll
    for (int q = 0; q < CPL; ++q) { acc[q] = 0.f; Q[q] = 1.f; }
    constexpr int UN = CPL == 1 ? 8 : 4;                 // sample rows of loads in flight (a row is 256 bytes per wavefront)
    for (int s0 = 0; s0 < S; s0 += UN) {
        float f[UN][CPL], dist[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int s = min(s0 + u, S - 1);
#pragma unroll
            for (int q = 0; q < CPL; ++q) { const int c = lane * CPL + q; f[u][q] = c < C ? fr[(long)s * C + c] : 0.f; }
            dist[u] = awp_dist(zz, s, S, norm);
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int s = s0 + u;
            if (s < S) awp_fwd_row<AwpWaveGroup, CPL, true>(f[u], dist[u], s < S - 1, lane * CPL, C, acc, Q);
        }
    }
#pragma unroll
    for (int q = 0; q < CPL; ++q) { const int c = lane * CPL + q; if (c < C) out[n * C + c] = acc[q]; }
}

// Same decomposition as the forward; one row of lookahead (every row's exponential is evaluated once: as "the next row's" in the
// iteration before).
template <int CPL>
__global__ __launch_bounds__(256) void k_awp_integrate_bwd(const float* __restrict__ feat, const float* __restrict__ z, const float* __restrict__ rays_d,
                                                           const float* __restrict__ d_out, long N, int S, int C, float* __restrict__ d_feat,
                                                           float* __restrict__ d_z, float* __restrict__ d_rays_d) {
    const int lane = threadIdx.x & 63;
    const long n = blockIdx.x * (long)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (n >= N) return;
    const float* d = rays_d + n * 3;
    const float norm = ray_norm(d);
    const float* fr = feat + n * (long)S * C;
    const float* zz = z + n * (long)S;
    constexpr int PF = CPL == 1 ? 4 : 2;                 // rows per block; the NEXT block's rows are loaded while this one is processed
    float g[CPL], Q[CPL], cur[PF + 1][CPL], nxt[PF][CPL], ec[CPL];
    auto row = [&](int s, float (&dst)[CPL]) {
        const int sc = s < S ? s : S - 1;
#pragma unroll
        for (int q = 0; q < CPL; ++q) { const int c = lane * CPL + q; dst[q] = c < C ? fr[(long)sc * C + c] : 0.f; }
    };
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        const int c = lane * CPL + q;
        g[q] = c < C ? d_out[n * C + c] : 0.f;
        Q[q] = 1.f;
    }
#pragma unroll
    for (int u = 0; u <= PF; ++u) row(u, cur[u]);
    {
        const float dist0 = awp_dist(zz, 0, S, norm);
#pragma unroll
        for (int q = 0; q < CPL; ++q) ec[q] = S > 1 ? awp_e(cur[0][q], dist0) : 1.f;
    }
    float dnorm = 0.f, dz_prev = 0.f;                    // d z[s] carried from the previous interval (+ d dist[s-1] |d|)
    for (int s0 = 0; s0 < S; s0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) row(s0 + PF + 1 + u, nxt[u]);
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int s = s0 + u;
            if (s < S) {
                const bool last = s == S - 1;
                const float dz = awp_dz(zz, s, last);
                float df[CPL], Qn[CPL], en[CPL];
                float ddist = awp_bwd_row<AwpWaveGroup, CPL, true, false>(cur[u], ec, Q, cur[u + 1], g, __fmul_rn(dz, norm), awp_dist(zz, s + 1, S, norm), last,
                                                                          s + 2 < S, lane * CPL, C, df, Qn, en);
#pragma unroll
                for (int q = CPL - 1; q >= 0; --q) { const int c = lane * CPL + q; if (c < C) d_feat[(n * (long)S + s) * C + c] = df[q]; }
                if (d_z || d_rays_d) {
                    ddist = AwpWaveGroup::sum(ddist);
                    if (d_z && lane == 0) d_z[n * (long)S + s] = dz_prev - ddist * norm;
                    dz_prev = ddist * norm;
                    dnorm += ddist * dz;
                }
#pragma unroll
                for (int q = 0; q < CPL; ++q) { Q[q] = Qn[q]; ec[q] = en[q]; }
            }
        }
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            cur[0][q] = cur[PF][q];
#pragma unroll
            for (int u = 0; u < PF; ++u) cur[u + 1][q] = nxt[u][q];
        }
    }
    if (d_rays_d && lane < 3) d_rays_d[n * 3 + lane] = norm > 0.f ? dnorm * d[lane] / norm : 0.f;
}

// The same two scans for C = 64 (the AWP embedding's width, every shipped config): 16 lanes per ray with 4 consecutive channels each (one
// 16-byte load per sample row), FOUR rays per wavefront.  The 64-lane form above spends one wavefront instruction per (ray, sample,
// operation) on 64 channels and was bound by its instruction count (2.0 TB/s); here an instruction serves four rays and the cumulative
// product / suffix sum over the channels is a 4-step scan inside a DPP row.
__global__ __launch_bounds__(256) void k_awp_integrate_c64(const float* __restrict__ feat, const float* __restrict__ z,
                                                           const float* __restrict__ rays_d, long N, int S, float* __restrict__ out) {
    const int l16 = threadIdx.x & 15;
    const long n0 = blockIdx.x * 16L + (threadIdx.x >> 4);
    const long n = n0 < N ? n0 : N - 1;                   // (rays past the end compute on the last ray and write nothing: the DPP rows stay whole)
    const float norm = ray_norm(rays_d + n * 3);
    const float4* fr = reinterpret_cast<const float4*>(feat + n * (long)S * 64) + l16;
    const float* zz = z + n * (long)S;
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, Q[4] = {1.f, 1.f, 1.f, 1.f};
    constexpr int UN = 4;
    for (int s0 = 0; s0 < S; s0 += UN) {
        float4 f4[UN];
        float dist[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int s = min(s0 + u, S - 1);
            f4[u] = fr[(long)s * 16];
            dist[u] = awp_dist(zz, s, S, norm);
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int s = s0 + u;
            if (s < S) {
                const float f[4] = {f4[u].x, f4[u].y, f4[u].z, f4[u].w};
                awp_fwd_row<AwpRowGroup, 4, false>(f, dist[u], s < S - 1, 0, 64, acc, Q);
            }
        }
    }
    if (n0 < N) reinterpret_cast<float4*>(out + n * 64)[l16] = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

__global__ __launch_bounds__(256) void k_awp_integrate_bwd_c64(const float* __restrict__ feat, const float* __restrict__ z,
                                                               const float* __restrict__ rays_d, const float* __restrict__ d_out, long N, int S,
                                                               float* __restrict__ d_feat, float* __restrict__ d_z, float* __restrict__ d_rays_d) {
    const int l16 = threadIdx.x & 15;
    const long n0 = blockIdx.x * 16L + (threadIdx.x >> 4);
    const bool live = n0 < N;
    const long n = live ? n0 : N - 1;
    const float* d = rays_d + n * 3;
    const float norm = ray_norm(d);
    const float4* fr = reinterpret_cast<const float4*>(feat + n * (long)S * 64) + l16;
    float4* dfr = reinterpret_cast<float4*>(d_feat + n * (long)S * 64) + l16;
    const float* zz = z + n * (long)S;
    constexpr int PF = 4;                                 // rows per block; the NEXT block's rows are loaded while this one is processed
    float4 cur[PF + 1], nxt[PF];
    const float4 g4 = reinterpret_cast<const float4*>(d_out + n * 64)[l16];
    const float g[4] = {g4.x, g4.y, g4.z, g4.w};
    float Q[4] = {1.f, 1.f, 1.f, 1.f}, ec[4];
#pragma unroll
    for (int u = 0; u <= PF; ++u) cur[u] = fr[(long)min(u, S - 1) * 16];
    {
        const float dist0 = awp_dist(zz, 0, S, norm);
        const float f0[4] = {cur[0].x, cur[0].y, cur[0].z, cur[0].w};
#pragma unroll
        for (int q = 0; q < 4; ++q) ec[q] = S > 1 ? awp_e(f0[q], dist0) : 1.f;
    }
    float dnorm = 0.f, dz_prev = 0.f;
    for (int s0 = 0; s0 < S; s0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) nxt[u] = fr[(long)min(s0 + PF + 1 + u, S - 1) * 16];
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int s = s0 + u;
            if (s < S) {
                const float fc[4] = {cur[u].x, cur[u].y, cur[u].z, cur[u].w};
                const float fn[4] = {cur[u + 1].x, cur[u + 1].y, cur[u + 1].z, cur[u + 1].w};
                const bool last = s == S - 1;
                const float dz = awp_dz(zz, s, last);
                float df[4], Qn[4], en[4];
                float ddist = awp_bwd_row<AwpRowGroup, 4, false, true>(fc, ec, Q, fn, g, __fmul_rn(dz, norm), awp_dist(zz, s + 1, S, norm), last, s + 2 < S, 0, 64,
                                                                       df, Qn, en);
                if (live) dfr[(long)s * 16] = make_float4(df[0], df[1], df[2], df[3]);
                if (d_z || d_rays_d) {
                    ddist = AwpRowGroup::sum(ddist);
                    if (d_z && live && l16 == 0) d_z[n * (long)S + s] = dz_prev - ddist * norm;
                    dz_prev = ddist * norm;
                    dnorm += ddist * dz;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) { Q[q] = Qn[q]; ec[q] = en[q]; }
            }
        }
        cur[0] = cur[PF];
#pragma unroll
        for (int u = 0; u < PF; ++u) cur[u + 1] = nxt[u];
    }
    if (d_rays_d && live && l16 < 3) d_rays_d[n * 3 + l16] = norm > 0.f ? dnorm * d[l16] / norm : 0.f;
}

}  // namespace evd

using namespace evd;

extern "C" {

int evd_awp_feature_integration(const float* feat, const float* z, const float* rays_d, long N, int S, int C, float* out, void* stream) {
    EVD_REQUIRE(feat && z && rays_d && out && N >= 0 && S >= 1 && C >= 1, "evd_awp_feature_integration: bad arguments");
    EVD_REQUIRE(C <= 256, "evd_awp_feature_integration: %d channels (built: <= 256)", C);
    if (N == 0) return EVD_OK;
    hipStream_t st = as_stream(stream);
    if (C == 64) k_awp_integrate_c64<<<cdiv(N, 16), 256, 0, st>>>(feat, z, rays_d, N, S, out);
    else if (C <= 64) k_awp_integrate<1><<<cdiv(N, 4), 256, 0, st>>>(feat, z, rays_d, N, S, C, out);
    else if (C <= 128) k_awp_integrate<2><<<cdiv(N, 4), 256, 0, st>>>(feat, z, rays_d, N, S, C, out);
    else k_awp_integrate<4><<<cdiv(N, 4), 256, 0, st>>>(feat, z, rays_d, N, S, C, out);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_awp_feature_integration_bwd(const float* feat, const float* z, const float* rays_d, const float* d_out, long N, int S, int C,
                                    float* d_feat, float* d_z, float* d_rays_d, void* stream) {
    EVD_REQUIRE(feat && z && rays_d && d_out && d_feat && N >= 0 && S >= 1 && C >= 1, "evd_awp_feature_integration_bwd: bad arguments");
    EVD_REQUIRE(C <= 256, "evd_awp_feature_integration_bwd: %d channels (built: <= 256)", C);
    if (N == 0) return EVD_OK;
    hipStream_t st = as_stream(stream);
    if (C == 64) k_awp_integrate_bwd_c64<<<cdiv(N, 16), 256, 0, st>>>(feat, z, rays_d, d_out, N, S, d_feat, d_z, d_rays_d);
    else if (C <= 64) k_awp_integrate_bwd<1><<<cdiv(N, 4), 256, 0, st>>>(feat, z, rays_d, d_out, N, S, C, d_feat, d_z, d_rays_d);
    else if (C <= 128) k_awp_integrate_bwd<2><<<cdiv(N, 4), 256, 0, st>>>(feat, z, rays_d, d_out, N, S, C, d_feat, d_z, d_rays_d);
    else k_awp_integrate_bwd<4><<<cdiv(N, 4), 256, 0, st>>>(feat, z, rays_d, d_out, N, S, C, d_feat, d_z, d_rays_d);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // extern "C"
