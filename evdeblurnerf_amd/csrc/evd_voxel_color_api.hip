// C-ABI entry points that train the per-RAY colour network of a composite_feature level (kernel_type PBE, reference
// networks/pdrf/voxnerf.py:231-239): the inference row function keeping its two hidden activations (voxel_color_rows.h), and the
// hand-written backward.  Float32 in every mode, as at inference.
//
// Backward, one launch + one fold.  A workgroup owns a run of consecutive rays and walks it four at a time (a wavefront per ray):
//   dgrad   d2 = g_color s (1 - s);  d h1 = (W2^T d2) [h1 > 0];  d h0 = (W1^T d h1) [h0 > 0];  d in = W0^T d h0 -- a lane per unit, the
//           three weight matrices resident in LDS (27 KiB; column walks, conflict-free); d map = the first G of d in, d viewdirs from the rest
//           through the encoding's derivative
//   wgrad   every thread owns 16 elements of d W1, up to 11 of d W0, one of d W2 and one bias element in registers and adds the four
//           rays' outer-product terms in ray order
// and leaves its sums as one block of the workspace (the parameter layout of evd_voxel.cnet).  k_color_rows_fold adds the blocks in
// workgroup order.  No atomics: the result depends on R alone, two calls give the same bits.
#include "voxel_net.h"
#include "voxel_color_rows.h"

using namespace evd;

namespace {

constexpr int CR_HD = 64, CR_G = 15, CR_NIN_MAX = CR_G + 3 * (1 + 2 * PE_LV), CR_K1 = CR_HD * CR_HD / 256, CR_K0 = (CR_HD * CR_NIN_MAX + 255) / 256;
constexpr int CR_MAX_BLOCKS = 256;
static_assert(CR_NIN_MAX <= 64, "a lane per input column");

inline int cr_nin(const evd_voxel* v) { return v->geo + 3 * (1 + 2 * v->multires_views); }
inline long cr_nparam(int nin) { return (long)CR_HD * nin + CR_HD + CR_HD * CR_HD + CR_HD + 3 * CR_HD + 3; }
// rays per workgroup (a multiple of 4) and the workgroup count for R rays
inline long cr_rays_per_block(long R) { return 4 * cdiv(cdiv(R, 4L), (long)CR_MAX_BLOCKS); }
inline int cr_blocks(long R) { return R > 0 ? (int)cdiv(R, cr_rays_per_block(R)) : 0; }
inline bool cr_built(const evd_voxel* v) { return v && v->composite_feature && !v->generic && v->hidden_dim == CR_HD && v->geo == CR_G && v->num_layers_color == 3; }

struct CrStore { float *h0, *h1, *color; };
inline size_t cr_store_layout(long R, void* store, CrStore* L) {
    float* p = (float*)store;
    L->h0 = p; L->h1 = p + R * CR_HD; L->color = p + 2 * R * CR_HD;
    return (size_t)(2 * R * CR_HD + 3 * R) * sizeof(float);
}

__global__ __launch_bounds__(256) void k_color_rows_bwd(const float* __restrict__ cnet, const float* __restrict__ g_color, const float* __restrict__ fm,
                                                        const float* __restrict__ viewdirs, int vd_stride, long R, int Lv, long rays_per_block,
                                                        const float* __restrict__ h0s, const float* __restrict__ h1s, const float* __restrict__ cols,
                                                        float* __restrict__ d_map, float* __restrict__ d_vd, float* __restrict__ partial) {
    __shared__ float W0[CR_HD * CR_NIN_MAX], W1[CR_HD * CR_HD], W2[3 * CR_HD];
    __shared__ float x[4][64], a0[4][CR_HD], a1[4][CR_HD], d2[4][4], dh1[4][CR_HD], dh0[4][CR_HD], dx[4][64];
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
    const int nin = CR_G + 3 * (1 + 2 * Lv), n0 = CR_HD * nin;
    const float *w0 = cnet, *w1 = w0 + n0 + CR_HD, *w2 = w1 + CR_HD * CR_HD + CR_HD;
    for (int e = t; e < n0; e += 256) W0[e] = w0[e];
    for (int e = t; e < CR_HD * CR_HD; e += 256) W1[e] = w1[e];
    for (int e = t; e < 3 * CR_HD; e += 256) W2[e] = w2[e];
    float g1[CR_K1], g0[CR_K0], g2 = 0.f, gb = 0.f;
    int j0[CR_K0], i0[CR_K0];
#pragma unroll
    for (int k = 0; k < CR_K1; ++k) g1[k] = 0.f;
#pragma unroll
    for (int k = 0; k < CR_K0; ++k) {
        const int e = min(t + 256 * k, n0 - 1);
        g0[k] = 0.f; j0[k] = e / nin; i0[k] = e - j0[k] * nin;
    }
    const long rbeg = blockIdx.x * rays_per_block, rend = min(R, rbeg + rays_per_block);
    for (long rb = rbeg; rb < rend; rb += 4) {
        const long r = rb + wv;
        const bool live = r < rend;
        __syncthreads();                                     // the weights are in place; the wgrad of the four rays before is done
        float xv = 0.f;
        if (live && lane < nin) xv = lane < CR_G ? fm[r * CR_G + lane] : color_rows_dir_enc(lane - CR_G, viewdirs[r * vd_stride + (lane - CR_G) % 3]);
        x[wv][lane] = xv;
        a0[wv][lane] = live ? h0s[r * CR_HD + lane] : 0.f;
        a1[wv][lane] = live ? h1s[r * CR_HD + lane] : 0.f;
        if (lane < 4) {
            float g = 0.f;
            if (live && lane < 3) { const float s = cols[r * 3 + lane]; g = g_color[r * 3 + lane] * s * (1.f - s); }
            d2[wv][lane] = g;
        }
        __syncthreads();
        {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) s = fmaf(W2[c * CR_HD + lane], d2[wv][c], s);
            dh1[wv][lane] = a1[wv][lane] > 0.f ? s : 0.f;
        }
        __syncthreads();
        {
            float s = 0.f;
            for (int j = 0; j < CR_HD; ++j) s = fmaf(W1[j * CR_HD + lane], dh1[wv][j], s);
            dh0[wv][lane] = a0[wv][lane] > 0.f ? s : 0.f;
        }
        __syncthreads();
        {
            float s = 0.f;
            if (lane < nin)
                for (int j = 0; j < CR_HD; ++j) s = fmaf(W0[j * nin + lane], dh0[wv][j], s);
            dx[wv][lane] = s;
            if (live && lane < CR_G) d_map[r * CR_G + lane] = s;
        }
        __syncthreads();
        if (d_vd && live && lane < 3) {                      // [x, sin(x f0), cos(x f0), ...]: d/dx = 1, f cos(x f), -f sin(x f)
            const float dv = viewdirs[r * vd_stride + lane];
            float g = dx[wv][CR_G + lane];
            for (int f = 0; f < Lv; ++f) {
                const float fr = (float)(1 << f);
                g = fmaf(dx[wv][CR_G + 3 + 6 * f + lane], cosf(dv * fr) * fr, g);
                g = fmaf(-dx[wv][CR_G + 6 + 6 * f + lane], sinf(dv * fr) * fr, g);
            }
            d_vd[r * 3 + lane] = g;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {                        // the four rays' terms, in ray order (a ray past the run's end holds zeros)
            const float hv = a0[q][lane];
#pragma unroll
            for (int k = 0; k < CR_K1; ++k) g1[k] = fmaf(dh1[q][wv + 4 * k], hv, g1[k]);
#pragma unroll
            for (int k = 0; k < CR_K0; ++k) g0[k] = fmaf(dh0[q][j0[k]], x[q][i0[k]], g0[k]);
            if (t < 3 * CR_HD) g2 = fmaf(d2[q][wv], a1[q][lane], g2);
            gb += t < CR_HD ? dh0[q][lane] : t < 2 * CR_HD ? dh1[q][lane] : t < 2 * CR_HD + 3 ? d2[q][t - 2 * CR_HD] : 0.f;
        }
    }
    float* P = partial + (long)blockIdx.x * (n0 + CR_HD + CR_HD * CR_HD + CR_HD + 3 * CR_HD + 3);
#pragma unroll
    for (int k = 0; k < CR_K0; ++k)
        if (t + 256 * k < n0) P[t + 256 * k] = g0[k];
    float* Pb0 = P + n0;
    float* P1 = Pb0 + CR_HD;
    float* Pb1 = P1 + CR_HD * CR_HD;
    float* P2 = Pb1 + CR_HD;
    float* Pb2 = P2 + 3 * CR_HD;
#pragma unroll
    for (int k = 0; k < CR_K1; ++k) P1[(wv + 4 * k) * CR_HD + lane] = g1[k];
    if (t < 3 * CR_HD) P2[t] = g2;
    if (t < CR_HD) Pb0[t] = gb; else if (t < 2 * CR_HD) Pb1[t - CR_HD] = gb; else if (t < 2 * CR_HD + 3) Pb2[t - 2 * CR_HD] = gb;
}

struct CrFoldDst { float* p[6]; long end[6]; };          // w0, b0, w1, b1, w2, b2 and the end of each in the block layout

__global__ __launch_bounds__(256) void k_color_rows_fold(const float* __restrict__ partial, int nblocks, long np, CrFoldDst dst, int accumulate) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= np) return;
    float s = 0.f;
    for (int b = 0; b < nblocks; ++b) s += partial[b * np + p];
    long beg = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (p < dst.end[k]) {
            if (dst.p[k]) dst.p[k][p - beg] = accumulate ? dst.p[k][p - beg] + s : s;
            return;
        }
        beg = dst.end[k];
    }
}

}  // namespace

extern "C" {

size_t evd_voxel_color_rows_store_bytes(const evd_voxel* v, long R) {
    CrStore L;
    return (!cr_built(v) || R < 0) ? 0 : cr_store_layout(R, nullptr, &L);
}

size_t evd_voxel_color_rows_backward_workspace_bytes(const evd_voxel* v, long R) {
    return (!cr_built(v) || R < 0) ? 0 : (size_t)cr_blocks(R) * cr_nparam(cr_nin(v)) * sizeof(float);
}

static int cr_check(const evd_voxel* v, const char* entry) {
    EVD_REQUIRE(v, "%s: null level", entry);
    EVD_REQUIRE(v->composite_feature, "%s: the per-ray colour network belongs to a composite_feature level (kernel_type PBE)", entry);
    EVD_REQUIRE(cr_built(v), "%s: built for the standard coarse level (hidden 64, geo 15, three colour layers), not hidden %d / geo %d / %d colour layers",
                entry, v->hidden_dim, v->geo, v->num_layers_color);
    return EVD_OK;
}

int evd_voxel_color_rows_train(const evd_voxel* v, const float* fmap, const float* viewdirs, int vd_stride, long R, float* color,
                               void* store, size_t store_bytes, void* stream) {
    if (const int rc = cr_check(v, "evd_voxel_color_rows_train")) return rc;
    EVD_REQUIRE(fmap && viewdirs && color && store && R >= 0 && vd_stride >= 3, "evd_voxel_color_rows_train: bad arguments");
    if (R == 0) return EVD_OK;
    CrStore L;
    const size_t need = cr_store_layout(R, store, &L);
    if (store_bytes < need) return fail(EVD_E_WORKSPACE, "evd_voxel_color_rows_train: store %zu < %zu bytes", store_bytes, need);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_color_rows<true>, dim3((unsigned)cdiv(R, 4L)), dim3(256), 0, st, (const float*)v->cnet.p, fmap, viewdirs, vd_stride, R, v->geo,
                       v->hidden_dim, v->multires_views, color, L.h0, L.h1);
    EVD_LAUNCH_CHECK();
    EVD_HIP(hipMemcpyAsync(L.color, color, (size_t)R * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    return EVD_OK;
}

int evd_voxel_color_rows_backward(const evd_voxel* v, const float* g_color, const float* fmap, const float* viewdirs, int vd_stride, long R,
                                  const void* store, size_t store_bytes, const evd_voxel_grads* grads, float* d_map, float* d_viewdirs,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = cr_check(v, "evd_voxel_color_rows_backward")) return rc;
    EVD_REQUIRE(g_color && fmap && viewdirs && store && grads && d_map && workspace && R >= 0 && vd_stride >= 3, "evd_voxel_color_rows_backward: bad arguments");
    if (R == 0) return EVD_OK;
    CrStore L;
    const size_t need = cr_store_layout(R, const_cast<void*>(store), &L);
    if (store_bytes < need) return fail(EVD_E_WORKSPACE, "evd_voxel_color_rows_backward: store %zu < %zu bytes", store_bytes, need);
    const size_t need_ws = evd_voxel_color_rows_backward_workspace_bytes(v, R);
    if (workspace_bytes < need_ws) return fail(EVD_E_WORKSPACE, "evd_voxel_color_rows_backward: workspace %zu < %zu bytes", workspace_bytes, need_ws);
    hipStream_t st = as_stream(stream);
    const int nin = cr_nin(v), nb = cr_blocks(R);
    const long np = cr_nparam(nin);
    float* partial = (float*)workspace;
    hipLaunchKernelGGL(k_color_rows_bwd, dim3((unsigned)nb), dim3(256), 0, st, (const float*)v->cnet.p, g_color, fmap, viewdirs, vd_stride, R,
                       v->multires_views, cr_rays_per_block(R), (const float*)L.h0, (const float*)L.h1, (const float*)L.color, d_map, d_viewdirs, partial);
    EVD_LAUNCH_CHECK();
    CrFoldDst dst;
    const long sizes[6] = {(long)CR_HD * nin, CR_HD, CR_HD * CR_HD, CR_HD, 3 * CR_HD, 3};
    long end = 0;
    for (int k = 0; k < 6; ++k) {
        dst.p[k] = (k & 1) ? grads->color_b[k >> 1] : grads->color_w[k >> 1];
        dst.end[k] = (end += sizes[k]);
    }
    hipLaunchKernelGGL(k_color_rows_fold, dim3((unsigned)cdiv(np, 256L)), dim3(256), 0, st, (const float*)partial, nb, np, dst, grads->accumulate ? 1 : 0);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // extern "C"
