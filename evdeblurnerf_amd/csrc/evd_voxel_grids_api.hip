// C-ABI entry points of a PDRF level's tri-plane grids as parameters (handle: voxel_net.h): reading and loading them, the scatter backward
// of the gather in its three forms (atomic, hybrid, deterministic) and the TV regulariser.
#include "mlp_device.h"
#include "voxel_net.h"

#include <cmath>

using namespace evd;

extern "C" {

int evd_voxel_grid_sizes(const evd_voxel* v, long* sizes) {
    EVD_REQUIRE(v && sizes, "evd_voxel_grid_sizes: null argument");
    for (int i = 0; i < 3; ++i) {
        sizes[i] = (long)(v->plane[i].bytes / sizeof(float));
        sizes[3 + i] = (long)(v->line[i].bytes / sizeof(float));
    }
    sizes[6] = (long)(v->basis.bytes / sizeof(float));
    return EVD_OK;
}

int evd_voxel_get_grids(const evd_voxel* v, float* const* plane, float* const* line, float* basis, void* stream) {
    EVD_REQUIRE(v && plane && line && basis, "evd_voxel_get_grids: null argument");
    hipStream_t st = as_stream(stream);
    for (int i = 0; i < 3; ++i) {
        EVD_HIP(hipMemcpyAsync(plane[i], v->plane[i].p, v->plane[i].bytes, hipMemcpyDeviceToDevice, st));
        EVD_HIP(hipMemcpyAsync(line[i], v->line[i].p, v->line[i].bytes, hipMemcpyDeviceToDevice, st));
    }
    EVD_HIP(hipMemcpyAsync(basis, v->basis.p, v->basis.bytes, hipMemcpyDeviceToDevice, st));
    return EVD_OK;
}

// the seven tensors of a level in ONE launch: every source value is read once and written twice, as the float32 copy the float32-grade modes
// and the backward gather, and as the float16 copy the half-precision modes gather (13 launches and a second read of 165 MB before)
struct GridLoadSeg { const float* src; float* dst; _Float16* dst_h; long n4, tail0, n; };
struct GridLoadSegs { GridLoadSeg s[7]; };
static __global__ __launch_bounds__(256) void k_load_grids(const GridLoadSegs segs) {
    const GridLoadSeg s = segs.s[blockIdx.y];
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < s.n4; i += stride) {
        const f32x4 v = reinterpret_cast<const f32x4*>(s.src)[i];
        reinterpret_cast<f32x4*>(s.dst)[i] = v;
        if (s.dst_h) {
            typedef _Float16 h4 __attribute__((ext_vector_type(4)));
            const h4 h = {f16_sat(v[0]), f16_sat(v[1]), f16_sat(v[2]), f16_sat(v[3])};
            reinterpret_cast<h4*>(s.dst_h)[i] = h;
        }
    }
    for (long i = s.tail0 + (long)blockIdx.x * 256 + threadIdx.x; i < s.n; i += stride) {
        s.dst[i] = s.src[i];
        if (s.dst_h) s.dst_h[i] = f16_sat(s.src[i]);
    }
}

int evd_voxel_load_grids(evd_voxel* v, const float* const* plane, const float* const* line, const float* basis, void* stream) {
    EVD_REQUIRE(v && plane && line && basis, "evd_voxel_load_grids: null argument");
    hipStream_t st = as_stream(stream);
    GridLoadSegs segs;
    long nmax = 0;
    auto seg = [&](int k, const float* src, DevBuf& dst, DevBuf* dst_h) {
        const long n = (long)(dst.bytes / sizeof(float));
        const bool vec = ((uintptr_t)src % 16) == 0;            // device allocations are 256-byte aligned; a caller's slice may not be
        segs.s[k] = GridLoadSeg{src, (float*)dst.p, dst_h ? (_Float16*)dst_h->p : nullptr, vec ? n / 4 : 0, vec ? (n / 4) * 4 : 0, n};
        nmax = n > nmax ? n : nmax;
    };
    for (int i = 0; i < 3; ++i) {
        EVD_REQUIRE(plane[i] && line[i], "evd_voxel_load_grids: missing grid %d", i);
        seg(i, plane[i], v->plane[i], &v->plane_h[i]);
        seg(3 + i, line[i], v->line[i], &v->line_h[i]);
    }
    seg(6, basis, v->basis, nullptr);
    const long bx = cdiv(nmax / 4 + 1, 256L) < 2048 ? cdiv(nmax / 4 + 1, 256L) : 2048;
    hipLaunchKernelGGL(k_load_grids, dim3((unsigned)bx, 7), dim3(256), 0, st, segs);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_voxel_grid_mirrors(const evd_voxel* v, float** plane_f32, float** line_f32, float** basis_f32, void** plane_f16, void** line_f16) {
    EVD_REQUIRE(v && plane_f32 && line_f32 && basis_f32 && plane_f16 && line_f16, "evd_voxel_grid_mirrors: null argument");
    for (int i = 0; i < 3; ++i) {
        plane_f32[i] = (float*)v->plane[i].p; line_f32[i] = (float*)v->line[i].p;
        plane_f16[i] = v->plane_h[i].p; line_f16[i] = v->line_h[i].p;
    }
    *basis_f32 = (float*)v->basis.p;
    return EVD_OK;
}

static GridGrads grid_grads(const evd_voxel_grid_grads* g) {
    GridGrads gg;
    for (int i = 0; i < 3; ++i) { gg.plane[i] = g->plane[i]; gg.line[i] = g->line[i]; }
    gg.basis = g->basis;
    return gg;
}

int evd_voxel_sample_bwd(const evd_voxel* v, const float* pts, long n, const float* d_out, int d_stride, int d_col,
                         const evd_voxel_grid_grads* g, float* d_pts, void* stream) {
    EVD_REQUIRE(v && pts && d_out && g && n >= 0 && d_stride >= d_col + v->app_dim, "evd_voxel_sample_bwd: bad arguments");
    EVD_REQUIRE(v->app_act == EVD_ACT_NONE, "evd_voxel_sample_bwd: only app_actfn none is built (all shipped configs)");
    if (n == 0) return EVD_OK;
    const GridGrads gg = grid_grads(g);
    return launch_voxel_sample_bwd(v->gp, pts, n, d_out, d_stride, d_col, gg, d_pts, as_stream(stream));
}

size_t evd_voxel_sample_bwd_workspace_bytes(const evd_voxel* v, long n) {
    if (!v || n <= 0) return 0;
    return voxel_scatter_hybrid_workspace_bytes(v->gp, n);
}

static int sample_bwd_ws(const evd_voxel* v, bool half_grids, const float* pts, long n, const float* d_out, int d_stride, int d_col,
                         const evd_voxel_grid_grads* g, float* d_pts, void* workspace, size_t workspace_bytes, void* stream);
int evd_voxel_sample_bwd_ws(const evd_voxel* v, const float* pts, long n, const float* d_out, int d_stride, int d_col,
                            const evd_voxel_grid_grads* g, float* d_pts, void* workspace, size_t workspace_bytes, void* stream) {
    return sample_bwd_ws(v, false, pts, n, d_out, d_stride, d_col, g, d_pts, workspace, workspace_bytes, stream);
}
int evd_voxel_sample_bwd_prec(const evd_voxel* v, int precision, const float* pts, long n, const float* d_out, int d_stride, int d_col,
                              const evd_voxel_grid_grads* g, float* d_pts, void* workspace, size_t workspace_bytes, void* stream) {
    EVD_REQUIRE(precision >= 0 && precision <= EVD_PREC_F16M, "evd_voxel_sample_bwd_prec: unknown precision %d", precision);
    return sample_bwd_ws(v, v && grids_half_for(v, precision), pts, n, d_out, d_stride, d_col, g, d_pts, workspace, workspace_bytes, stream);
}
static int sample_bwd_ws(const evd_voxel* v, bool half_grids, const float* pts, long n, const float* d_out, int d_stride, int d_col,
                         const evd_voxel_grid_grads* g, float* d_pts, void* workspace, size_t workspace_bytes, void* stream) {
    EVD_REQUIRE(v && pts && d_out && g && n >= 0 && d_stride >= d_col + v->app_dim, "evd_voxel_sample_bwd_ws: bad arguments");
    EVD_REQUIRE(v->app_act == EVD_ACT_NONE, "evd_voxel_sample_bwd_ws: only app_actfn none is built (all shipped configs)");
    if (n == 0) return EVD_OK;
    const GridGrads gg = grid_grads(g);
    if (workspace && workspace_bytes > 0 && voxel_scatter_hybrid_ok(v->gp, n))
        return launch_voxel_sample_bwd_hybrid(v->gp, pts, n, d_out, d_stride, d_col, gg, d_pts, workspace, workspace_bytes, as_stream(stream), half_grids);
    return launch_voxel_sample_bwd(v->gp, pts, n, d_out, d_stride, d_col, gg, d_pts, as_stream(stream));
}

// ---- the deterministic scatter (kernel_voxel_scatter_det.hip; run_nerf.py:50)
// the exponent k of the fixed-point scale 2^k (unit 2^-k): with frexpf(cmax) -> E (cmax < 2^E) and h = ceil(log2(4 n)), k = 62 - h - E; a cell
// receives at most 4 n terms of magnitude < 2^E, so its sum stays below 2^62.  k is clamped to 126 (k_scatter_lines' clamp: 2^k stays a
// finite float32; a batch whose maximum is that small is resolved to 2^-126).  0 where no scale exists (cmax not finite, not positive).
int evd_scatter_det_unit_exp(float cmax, long n) {
    if (!(cmax > 0.f) || !std::isfinite(cmax) || n < 1) return 0;
    int E;
    (void)frexpf(cmax, &E);
    int h = 0;
    while (h < 62 && (1L << h) < 4 * n) ++h;
    const int k = 62 - h - E;
    return k > 126 ? 126 : k;
}

// the region of the workspace behind its 256-byte alignment: the shadow, or (a batch without a scale) the hybrid form's scratch
static size_t det_region_bytes(const evd_voxel* v, long n) {
    const size_t a = voxel_scatter_det_region_bytes(v->gp), b = voxel_scatter_hybrid_ok(v->gp, n) ? voxel_scatter_hybrid_workspace_bytes(v->gp, n) : 0;
    return a > b ? a : b;
}

static const size_t DET_WS_SLACK = 256;        // alignment slack for an unaligned caller pointer: the region starts at ws_align_ptr(workspace)
size_t evd_voxel_sample_bwd_det_workspace_bytes(const evd_voxel* v, long n) {
    if (!v || n <= 0) return 0;
    return det_region_bytes(v, n) + DET_WS_SLACK;
}

int evd_voxel_sample_bwd_det(const evd_voxel* v, int precision, const float* pts, long n, const float* d_out, int d_stride, int d_col,
                             const evd_voxel_grid_grads* g, float* d_pts, void* workspace, size_t workspace_bytes, void* stream) {
    EVD_REQUIRE(v && pts && d_out && g && n >= 0 && d_stride >= d_col + v->app_dim, "evd_voxel_sample_bwd_det: bad arguments");
    EVD_REQUIRE(precision >= 0 && precision <= EVD_PREC_F16M, "evd_voxel_sample_bwd_det: unknown precision %d", precision);
    EVD_REQUIRE(v->app_act == EVD_ACT_NONE, "evd_voxel_sample_bwd_det: only app_actfn none is built (all shipped configs)");
    if (n == 0) return EVD_OK;
    const size_t need = evd_voxel_sample_bwd_det_workspace_bytes(v, n);
    if (!workspace || workspace_bytes < need) return fail(EVD_E_WORKSPACE, "evd_voxel_sample_bwd_det: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    const bool half = grids_half_for(v, precision);
    const GridGrads gg = grid_grads(g);
    char* region = (char*)ws_align_ptr(workspace);
    int rc = launch_voxel_scatter_det_scale(v->gp, half, pts, n, d_out, d_stride, d_col, gg, region, st);
    if (rc) return rc;
    // the one host read of this entry: the unit is a function of the batch's maximum, and a batch without one takes another path
    unsigned bits = 0;
    EVD_HIP(hipMemcpyAsync(&bits, region, sizeof(bits), hipMemcpyDeviceToHost, st));
    EVD_HIP(hipStreamSynchronize(st));
    float cmax;
    memcpy(&cmax, &bits, sizeof(cmax));
    if (!std::isfinite(cmax))          // a NaN / Inf contribution: no scale exists, the gradients show it as the default path does
        return sample_bwd_ws(v, half, pts, n, d_out, d_stride, d_col, g, d_pts, region, det_region_bytes(v, n), stream);
    return launch_voxel_scatter_det_add(v->gp, half, pts, n, d_out, d_stride, d_col, gg, d_pts, region, evd_scatter_det_unit_exp(cmax, n), st);
}

// the six TV terms of a level: planes at weight 1e-2, lines at 1e-3; g = the gradients they are added to (null: the loss only)
static TvJobs tv_jobs(const evd_voxel* v, const evd_voxel_grid_grads* g) {
    TvJobs jobs;
    jobs.n = 6;
    for (int i = 0; i < 3; ++i) {
        const int C = v->n_comp[i], Wp = v->grid[kMat0[i]], Hp = v->grid[kMat1[i]], Lp = v->grid[kVec[i]];
        jobs.j[i] = TvJob{(const float*)v->plane[i].p, g ? g->plane[i] : nullptr, Hp, Wp, C, 1e-2f, 0, 0};
        jobs.j[3 + i] = TvJob{(const float*)v->line[i].p, g ? g->line[i] : nullptr, Lp, 1, C, 1e-3f, 0, 0};
    }
    return jobs;
}

int evd_voxel_tv_loss_bwd(const evd_voxel* v, const float* d_loss, const evd_voxel_grid_grads* g, void* stream) {
    EVD_REQUIRE(v && g && d_loss, "evd_voxel_tv_loss_bwd: null argument");
    TvJobs jobs = tv_jobs(v, g);
    return launch_tv_bwd_level(jobs, d_loss, as_stream(stream));
}

int evd_voxel_tv_loss(const evd_voxel* v, float* out, void* stream) {
    EVD_REQUIRE(v && out, "evd_voxel_tv_loss: null argument");
    hipStream_t st = as_stream(stream);
    double* acc = (double*)v->tv_acc.p;
    TvShape s;
    TvJobs jobs = tv_jobs(v, nullptr);
    int rc = launch_tv_level(jobs, acc, &s, st);
    if (rc) return rc;
    return launch_tv_finish(acc, s, out, st);
}

}  // extern "C"
