// Inverse-CDF resampling of the hierarchical pass: sample_pdf (utils/rays.py:149-193) on bins = z_mid, weights[1:-1] + merge
// (renderer.py:205,234) + z_std (:250), one launch.  The z stratification that precedes it is in kernels_rays.hip, the compositing scan
// that produces its weights in kernels_composite.hip.
//
//   k_sample_pdf_merge   new samples, merged and sorted z, sort order, z_std and (in a c2f render) the positions of the new / merged samples
#include "ray_math.h"
#include "voxel.h"          // launch_sample_pdf_merge_pts
#include "wave_ops.h"

namespace evd {

// One wavefront per ray; cdf staged in LDS.  The normalising sum and the cdf prefix sums are accumulated in
// float64: for <= 2^29 dynamic range those sums are exact, hence independent of the scan order and bitwise equal
// to torch's CPU cumsum (double accumulator).
__global__ __launch_bounds__(256) void k_sample_pdf_merge(const float* __restrict__ z, const float* __restrict__ wts, long R, int S,
                                                          int N, int det, const float* __restrict__ u,
                                                          float* __restrict__ z_samples, float* __restrict__ z_merged,
                                                          int* __restrict__ order, float* __restrict__ z_std,
                                                          const float* __restrict__ rb, int rb_cols, float* __restrict__ pts_new,
                                                          float* __restrict__ pts_merged) {
    // rb (the ray batch: o at columns 0..2, d at 3..5) + pts_new / pts_merged: the positions o + d z of the new / the merged samples are
    // written here as well (renderer.py:206: ray_point, as k_points writes them) -- two launches less in a c2f render
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long r = blockIdx.x * (long)(blockDim.x >> 6) + wv;
    const int nb = S - 1;                       // bins (z_mid) = cdf entries
    const int per = 2 * S + N + 2;              // floats of LDS per wave: z[S], cdf[nb]+pad, zs[N]
    float* zs0 = smem_f + (long)wv * per;       // z of the coarse pass
    float* cdf = zs0 + S;                       // [nb]
    float* zsm = cdf + S;                       // new samples [N]
    if (r >= R) return;
    const float* zr = z + r * (long)S;
    const float* wr = wts + r * (long)S;
    float ro[3] = {0.f, 0.f, 0.f}, rd3[3] = {0.f, 0.f, 0.f};
    if (rb) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { ro[c] = rb[r * rb_cols + c]; rd3[c] = rb[r * rb_cols + 3 + c]; }
    }
    for (int i = lane; i < S; i += 64) zs0[i] = zr[i];
    // sum of (w + 1e-5) over weights[1:-1]
    double part = 0.0;
    for (int i = lane; i < nb - 1; i += 64) part += (double)__fadd_rn(wr[i + 1], 1e-5f);
    const float sum = (float)wave_sum(part);
    // cdf[0] = 0, cdf[k+1] = float(prefix_double(pdf))
    double carry = 0.0;
    for (int base = 0; base < nb - 1; base += 64) {
        const int i = base + lane;
        const double p = (i < nb - 1) ? (double)(__fadd_rn(wr[i + 1], 1e-5f) / sum) : 0.0;
        const double incl = wave_scan_add_d(p, lane);
        if (i < nb - 1) cdf[i + 1] = (float)(carry + incl);
        carry += __shfl(incl, 63, WAVE);
    }
    if (lane == 0) cdf[0] = 0.f;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    // invert the cdf
    double m1 = 0.0;
    for (int j = lane; j < N; j += 64) {
        const float uu = det ? linspace_at(0.f, 1.f, N, j) : u[r * (long)N + j];
        int lo = 0, hi = nb;                    // first index with cdf[idx] > uu  (searchsorted right=True)
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (cdf[mid] <= uu) lo = mid + 1; else hi = mid; }
        const int below = max(lo - 1, 0), above = min(lo, nb - 1);
        float denom = __fsub_rn(cdf[above], cdf[below]);
        if (denom < 1e-5f) denom = 1.f;
        const float t = __fsub_rn(uu, cdf[below]) / denom;
        const float b0 = __fmul_rn(.5f, __fadd_rn(zs0[below + 1], zs0[below]));   // z_mid on the fly (renderer.py:200)
        const float b1 = __fmul_rn(.5f, __fadd_rn(zs0[above + 1], zs0[above]));
        const float s = __fadd_rn(b0, __fmul_rn(t, __fsub_rn(b1, b0)));
        zsm[j] = s;
        if (z_samples) z_samples[r * (long)N + j] = s;
        if (pts_new) {
#pragma unroll
            for (int c = 0; c < 3; ++c) pts_new[(r * (long)N + j) * 3 + c] = ray_point(ro[c], rd3[c], s);
        }
        m1 += (double)s;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    if (z_std) {                                // torch.std(unbiased=False)
        const double mean = wave_sum(m1) / (double)N;
        double v = 0.0;
        for (int j = lane; j < N; j += 64) { const double dd = (double)zsm[j] - mean; v += dd * dd; }
        v = wave_sum(v);
        if (lane == 0) z_std[r] = (float)sqrt(v / (double)N);
    }
    if (z_merged || order) {
        // stable rank of every element of cat(z, z_samples): #smaller + #equal-with-lower-index
        const int St = S + N;
        for (int e = lane; e < St; e += 64) {
            const float v = e < S ? zs0[e] : zsm[e - S];
            int rank = 0;
            for (int k = 0; k < S; ++k) { const float o = zs0[k]; rank += (o < v) || (o == v && k < e); }
            for (int k = 0; k < N; ++k) { const float o = zsm[k]; rank += (o < v) || (o == v && (k + S) < e); }
            if (z_merged) z_merged[r * (long)St + rank] = v;
            if (order) order[r * (long)St + rank] = e;
            if (pts_merged) {
#pragma unroll
                for (int c = 0; c < 3; ++c) pts_merged[(r * (long)St + rank) * 3 + c] = ray_point(ro[c], rd3[c], v);
            }
        }
    }
}

// evd_sample_pdf_merge + the positions of the new and of the merged samples (internal: evd_c2f_render_rays)
int launch_sample_pdf_merge_pts(const float* z, const float* weights, long R, int S, int N, int det, const float* u,
                                float* z_samples, float* z_merged, int* order, float* z_std,
                                const float* rb, int rb_cols, float* pts_new, float* pts_merged, hipStream_t stream) {
    EVD_REQUIRE(z && weights && R >= 0 && S >= 3 && N >= 1, "evd_sample_pdf_merge: bad arguments");
    EVD_REQUIRE(rb || (!pts_new && !pts_merged), "evd_sample_pdf_merge: sample positions need the ray batch");
    EVD_REQUIRE(det || u, "evd_sample_pdf_merge: det == 0 needs the explicit u draw");
    if (R == 0) return EVD_OK;
    const size_t lds = 4 * sizeof(float) * (size_t)(2 * S + N + 2);
    EVD_REQUIRE(lds <= 64 * 1024, "evd_sample_pdf_merge: S + N too large for the LDS staging (%zu bytes)", lds);
    k_sample_pdf_merge<<<cdiv(R, 4), 256, lds, stream>>>(z, weights, R, S, N, det, u, z_samples, z_merged, order, z_std, rb, rb_cols, pts_new, pts_merged);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // namespace evd

extern "C" {

int evd_sample_pdf_merge(const float* z, const float* weights, long R, int S, int N, int det, const float* u,
                         float* z_samples, float* z_merged, int* order, float* z_std, void* stream) {
    return evd::launch_sample_pdf_merge_pts(z, weights, R, S, N, det, u, z_samples, z_merged, order, z_std, nullptr, 0, nullptr, nullptr, evd::as_stream(stream));
}

}  // extern "C"
