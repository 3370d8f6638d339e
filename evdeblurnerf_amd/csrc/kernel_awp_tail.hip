// The AWP tail's forward (awp_tail.h): k_awp_tail_fwd, k_awp_tail_finish, the four size queries and evd_awp_tail_forward.  float32 throughout:
// the per-sample products (MAM.linear / convb / convl on [S, 64 -> 32 -> 16 -> 16]) run one sample row per lane group with the row in registers
// and the weights as LDS broadcasts, or as 16 x 16 tiles on the exact-float32 matrix core like everything P-sized (awp_tail_tile.h).
#include "awp_tail_ray.h"

namespace evd {

__global__ __launch_bounds__(AT_NT) void k_awp_tail_fwd(TailKParams p) {
    extern __shared__ float lds[];
    TailLds L;
    tail_lds_layout(lds, p.d, false, L);
    tail_stage_weights(p, L);
    __syncthreads();
    const int tid = threadIdx.x, P = p.d.P;
    double s1 = 0.0, s2 = 0.0;                                   // lanes 0..31: the sums of this workgroup's y, y^2 of channel tid
    for (long r = blockIdx.x; r < p.R; r += gridDim.x) {
        tail_forward_ray(p, L, r);
        if (p.saved) {                                           // the ray's forward state for the backward: 55 KB instead of a second forward
            float4* dst = reinterpret_cast<float4*>(p.saved + r * L.ray_floats);
            const float4* src = reinterpret_cast<const float4*>(L.x0);
#pragma unroll 4
            for (int i = tid; i < L.ray_floats / 4; i += AT_NT) dst[i] = src[i];
        }
        const float* xg = L.xs(p.d.n_mot - 1);
        for (int i = tid; i < P * AT_CM; i += AT_NT) {
            p.y[r * P * AT_CM + i] = L.yb[i];
            p.xg[r * P * AT_CM + i] = xg[i];
        }
        if (tid < AT_CM) {
            float a = 0.f, b = 0.f;
            for (int pp = 0; pp < P; ++pp) {
                const float v = L.yb[pp * AT_CM + tid];
                a += v;
                b = fmaf(v, v, b);
            }
            s1 += (double)a;
            s2 += (double)b;
        }
        __syncthreads();
    }
    if (tid < AT_CM) {
        p.bn_part[(long)blockIdx.x * 2 * AT_CM + tid] = s1;
        p.bn_part[(long)blockIdx.x * 2 * AT_CM + AT_CM + tid] = s2;
    }
}

__global__ __launch_bounds__(AT_FT) void k_awp_tail_finish(TailFinishParams p) {
    __shared__ double red[4][2 * AT_CM];
    __shared__ float stat[2 * AT_CM], hm[AT_FR][AT_CM], sw[AT_FR][AT_MAXP];
    const int tid = threadIdx.x, col = tid & 63, grp = tid >> 6;
    if (p.training) {
        red[grp][col] = fold_rows(p.bn_part, 2 * AT_CM, col, p.nparts, grp);      // (every workgroup folds all the partial rows)
        __syncthreads();
        if (tid < AT_CM) {
            const double n = (double)p.R * p.P;
            const double s1 = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
            const double s2 = red[0][AT_CM + tid] + red[1][AT_CM + tid] + red[2][AT_CM + tid] + red[3][AT_CM + tid];
            const double mu = s1 / n;
            double var = s2 / n - mu * mu;
            var = var > 0.0 ? var : 0.0;
            stat[tid] = (float)mu;
            stat[AT_CM + tid] = 1.0f / sqrtf((float)var + p.eps);
            if (blockIdx.x == 0) {
                if (p.run_mean) {                                           // BatchNorm1d's running estimates (momentum blend, unbiased variance)
                    p.run_mean[tid] = (1.0f - p.momentum) * p.run_mean[tid] + p.momentum * (float)mu;
                    p.run_var[tid] = (1.0f - p.momentum) * p.run_var[tid] + p.momentum * (float)(var * (n > 1.0 ? n / (n - 1.0) : 1.0));
                }
                if (tid == 0 && p.num_batches) *p.num_batches += 1;
            }
        }
    } else if (tid < AT_CM) {
        stat[tid] = p.run_mean[tid];
        stat[AT_CM + tid] = 1.0f / sqrtf(p.run_var[tid] + p.eps);
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid < 2 * AT_CM) p.stats[tid] = stat[tid];
    const int slot = tid >> 5, c = tid & 31;
    const long r = (long)blockIdx.x * AT_FR + slot;
    float tot, unused[AT_MAXP];
    finish_ray<false>(p, r < p.R ? r : p.R - 1, c, stat, hm[slot], sw[slot], tot, unused);
    if (r < p.R && c < p.P) p.out[r * p.P + c] = sw[slot][c] / tot;
}

}  // namespace evd

using namespace evd;

extern "C" {

int evd_awp_tail_num_params(int n_mot) { return 2 * n_mot + TW_COUNT; }

long evd_awp_tail_param_count(const evd_awp_tail_desc* d) { return tail_desc_ok(d) ? tail_param_total(tail_dims(d)) : -1; }

long evd_awp_tail_saved_floats(const evd_awp_tail_desc* d) {
    if (!tail_desc_ok(d)) return -1;
    TailLds L;
    tail_lds_layout(nullptr, tail_dims(d), false, L);
    return L.ray_floats;
}

size_t evd_awp_tail_workspace_bytes(const evd_awp_tail_desc* d, long R, int backward) {
    if (!tail_desc_ok(d) || R < 0) return 0;
    TailFwdWs f;
    TailBwdWs b;
    return backward ? tail_bwd_layout(tail_dims(d), R, nullptr, &b) : tail_fwd_layout(R, nullptr, &f);
}

int evd_awp_tail_forward(const evd_awp_tail_desc* d, const float* const* params, const float* h, const float* view_feature,
                         const float* rays_d, const float* h_inter, const float* h_intra, long R, float* bn_running_mean,
                         float* bn_running_var, long long* bn_num_batches, float* out, float* saved_y, float* saved_xg, float* saved_stats,
                         float* saved_rays, void* workspace, size_t workspace_bytes, void* stream) {
    TailDims dims;
    size_t lds = 0;
    if (d && d->training) {          // a training-mode forward is followed by the backward: refuse here what that kernel's working set cannot hold
        if (int e = tail_check("evd_awp_tail_forward", d, R, true, dims, lds)) return e;
    }
    if (int e = tail_check("evd_awp_tail_forward", d, R, false, dims, lds)) return e;
    EVD_REQUIRE(params && h && rays_d && h_inter && h_intra && out && saved_y && saved_xg && saved_stats && workspace,
                "evd_awp_tail_forward: null argument");
    EVD_REQUIRE(dims.VF == 0 || view_feature, "evd_awp_tail_forward: view_feature missing (VF = %d)", dims.VF);
    EVD_REQUIRE(d->training || (bn_running_mean && bn_running_var), "evd_awp_tail_forward: eval mode needs the BatchNorm running estimates");
    EVD_REQUIRE(!bn_running_mean == !bn_running_var, "evd_awp_tail_forward: bn_running_mean and bn_running_var go together");
    for (int i = 0; i < evd_awp_tail_num_params(dims.n_mot); ++i) EVD_REQUIRE(params[i], "evd_awp_tail_forward: parameter %d missing", i);
    TailFwdWs ws;
    const size_t need = tail_fwd_layout(R, workspace, &ws);
    if (workspace_bytes < need) return fail(EVD_E_WORKSPACE, "evd_awp_tail_forward: workspace %zu < %zu bytes", workspace_bytes, need);
    if (R == 0) return EVD_OK;
    TailKParams k{};
    tail_fill(k, dims, d, params, R, h, view_feature, rays_d, h_inter, h_intra, saved_y, saved_xg, saved_rays);
    k.bn_part = ws.bn_part;
    EVD_SET_MAX_LDS(k_awp_tail_fwd, AT_LDS_CU);
    k_awp_tail_fwd<<<ws.grid, AT_NT, lds, as_stream(stream)>>>(k);
    EVD_HIP(hipGetLastError());
    TailFinishParams f{};
    tail_fill_finish(f, dims, d, params, R, saved_y, saved_xg, saved_stats);
    f.bn_part = ws.bn_part; f.nparts = ws.grid; f.run_mean = bn_running_mean; f.run_var = bn_running_var; f.num_batches = bn_num_batches; f.out = out;
    k_awp_tail_finish<<<tail_nblk(R), AT_FT, 0, as_stream(stream)>>>(f);
    EVD_HIP(hipGetLastError());
    return EVD_OK;
}

}  // extern "C"
