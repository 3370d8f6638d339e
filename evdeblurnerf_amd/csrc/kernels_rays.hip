// Ray front end of the render path: everything between a camera pose and the network's inputs.  Elementwise / per-ray kernels, HBM- or
// launch-bound; the arithmetic they share is in ray_math.h.  The compositing scan is in kernels_composite.hip, the inverse-CDF resampling
// in kernels_sample_pdf.hip.
//
//   k_get_rays, k_get_rays_pix   camera rays of an image / of pixel coordinates      (utils/rays.py:8-36)
//   k_ndc                        NDC rays                                           (utils/rays.py:104-145)
//   k_rbk_warp                   the rigid blur kernel's sub-exposure rays           (networks/dpnerf/blurmodel.py:51-82)
//   k_ray_batch                  rays [R,3,2] -> ray_batch rows, and its backward    (networks/renderer.py:423-446)
//   k_sample_z                   z stratification (+ the sample positions)           (renderer.py:163-180)
//   k_ray_batch_z                k_ray_batch + k_sample_z in one launch
//   k_points                     pts = o + d z, and its backward                     (renderer.py:180,206)
//   k_embed                      positional embedding                                (networks/embedding.py:88-98)
#include "ray_math.h"
#include "voxel.h"          // launch_sample_z_pts
#include "wave_ops.h"

namespace evd {

// reference utils/rays.py:8-22
struct Pose34 { float m[12]; };
__global__ void k_get_rays(int H, int W, float k00, float k02, float k11, float k12, float halfpix, const Pose34 pose,
                           float* __restrict__ ro, float* __restrict__ rd) {
    const float* c2w = pose.m;
    const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (idx >= (long)H * W) return;
    const int j = idx / W, i = idx % W;
    const float d0 = ((float)i + (halfpix - k02)) / k00, d1 = -((float)j + (halfpix - k12)) / k11;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        rd[idx * 3 + r] = camera_ray_dir(d0, d1, c2w, r);
        ro[idx * 3 + r] = c2w[r * 4 + 3];
    }
}

// reference utils/rays.py:25-36
__global__ void k_get_rays_pix(const float* __restrict__ coords, float k00, float k02, float k11, float k12, float halfpix,
                               const float* __restrict__ c2ws, long n, float* __restrict__ ro, float* __restrict__ rd) {
    const long p = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (p >= n) return;
    const float* c2w = c2ws + p * 12;
    const float d0 = (coords[p * 2] + (halfpix - k02)) / k00, d1 = -(coords[p * 2 + 1] + (halfpix - k12)) / k11;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        rd[p * 3 + r] = camera_ray_dir(d0, d1, c2w, r);
        ro[p * 3 + r] = c2w[r * 4 + 3];
    }
}

__global__ void k_ndc(float cw, float ch, float near, float two_near, const float* __restrict__ o, const float* __restrict__ d,
                      long n, float* __restrict__ oo, float* __restrict__ od) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a[3] = {o[i * 3], o[i * 3 + 1], o[i * 3 + 2]}, b[3] = {d[i * 3], d[i * 3 + 1], d[i * 3 + 2]}, x[3], y[3];
    ndc_one(cw, ch, near, two_near, a, b, x, y);
#pragma unroll
    for (int c = 0; c < 3; ++c) { oo[i * 3 + c] = x[c]; od[i * 3 + c] = y[c]; }
}

// RigidBlurringModel.rbk_warp (networks/dpnerf/blurmodel.py:51-82; SE3Field.get_transform / warp, RigidBody.exp_se3 /
// exp_so3 of utils/rigid_warping.py:18-49,72-107): one thread per (ray, sub-exposure slot).  The reference runs ~40 small
// tensor ops per motion in a Python loop over the 9 motions.
__global__ void k_rbk_warp(const float* __restrict__ rays, const float* __restrict__ r, const float* __restrict__ v, long R, int M,
                           int use_origin, float* __restrict__ new_rays, float* __restrict__ transforms) {
    const int P = M + (use_origin ? 1 : 0);
    const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (idx >= R * P) return;
    const long n = idx / P;
    const int slot = idx % P, i = slot - (use_origin ? 1 : 0);
    float o[3], d[3], e[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { o[c] = rays[n * 6 + c * 2]; d[c] = rays[n * 6 + c * 2 + 1]; e[c] = __fadd_rn(o[c], d[c]); }
    float T[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    float wo[3] = {o[0], o[1], o[2]}, wd[3] = {d[0], d[1], d[2]};
    if (i >= 0) {
        const float rot[3] = {r[(n * 3 + 0) * M + i], r[(n * 3 + 1) * M + i], r[(n * 3 + 2) * M + i]};
        const float tr[3] = {v[(n * 3 + 0) * M + i], v[(n * 3 + 1) * M + i], v[(n * 3 + 2) * M + i]};
        const float theta = __fadd_rn(sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(rot[0], rot[0]), __fmul_rn(rot[1], rot[1])), __fmul_rn(rot[2], rot[2]))), 1.0e-10f);
        const float w[3] = {rot[0] / theta, rot[1] / theta, rot[2] / theta}, vv[3] = {tr[0] / theta, tr[1] / theta, tr[2] / theta};
        const float Wm[9] = {0.f, -w[2], w[1], w[2], 0.f, -w[0], -w[1], w[0], 0.f};
        float W2[9];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < 3; ++k) acc = __fadd_rn(acc, __fmul_rn(Wm[a * 3 + k], Wm[k * 3 + b]));
                W2[a * 3 + b] = acc;
            }
        const float st = sinf(theta), omc = __fsub_rn(1.0f, cosf(theta)), tms = __fsub_rn(theta, st);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float p = 0.f;
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const float eye = a == b ? 1.f : 0.f;
                T[a * 4 + b] = __fadd_rn(__fadd_rn(eye, __fmul_rn(st, Wm[a * 3 + b])), __fmul_rn(omc, W2[a * 3 + b]));
                const float g = __fadd_rn(__fadd_rn(__fmul_rn(theta, eye), __fmul_rn(omc, Wm[a * 3 + b])), __fmul_rn(tms, W2[a * 3 + b]));
                p = __fadd_rn(p, __fmul_rn(g, vv[b]));
            }
            T[a * 4 + 3] = p;
        }
        float we[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            wo[a] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[a * 4], o[0]), __fmul_rn(T[a * 4 + 1], o[1])), __fmul_rn(T[a * 4 + 2], o[2])), T[a * 4 + 3]);
            we[a] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[a * 4], e[0]), __fmul_rn(T[a * 4 + 1], e[1])), __fmul_rn(T[a * 4 + 2], e[2])), T[a * 4 + 3]);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) wd[a] = __fsub_rn(we[a], wo[a]);
    }
    float* out = new_rays + idx * 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) { out[c * 2] = wo[c]; out[c * 2 + 1] = wd[c]; }
    if (transforms) {
#pragma unroll
        for (int k = 0; k < 16; ++k) transforms[idx * 16 + k] = T[k];
    }
}

// reference networks/renderer.py:423-446: rays [R,3,2] -> ray_batch [R,ncol]
__global__ void k_ray_batch(const float* __restrict__ rays, long R, int ndc, int use_viewdirs, float cw, float ch,
                            float near, float far, float* __restrict__ rb) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= R) return;
    float o[3], d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { o[c] = rays[i * 6 + c * 2]; d[c] = rays[i * 6 + c * 2 + 1]; }
    pack_ray_row(o, d, ndc, use_viewdirs, cw, ch, near, far, rb + i * (use_viewdirs ? 11 : 8));
}

// Backward of k_ray_batch (training: the loss reaches the blur kernel's camera motion through the packed rays, renderer.py:303-308):
// d ray_batch [R,11] -> d rays [R,3,2].  One thread per ray; the forward's intermediate values are recomputed.  near / far columns carry
// no gradient.  With o' = o + t d, t = -(1 + o_z) / d_z, a = o'_z:   o_out = (cw o'_x / a, ch o'_y / a, 1 + 2 / a),
// d_out = (cw (d_x / d_z - o'_x / a), ch (d_y / d_z - o'_y / a), -2 / a),   viewdirs = d / |d|   (utils/rays.py:104-145, renderer.py:431).
__global__ void k_ray_batch_bwd(const float* __restrict__ rays, const float* __restrict__ g, long R, int ndc, float cw, float ch, float* __restrict__ d_rays) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= R) return;
    float o[3], d[3], go[3], gd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { o[c] = rays[i * 6 + c * 2]; d[c] = rays[i * 6 + c * 2 + 1]; }
    const float* gr = g + i * 11;
    const float goo[3] = {gr[0], gr[1], gr[2]}, gdo[3] = {gr[3], gr[4], gr[5]}, gv[3] = {gr[8], gr[9], gr[10]};
    if (ndc) {
        const float t = -(1.f + o[2]) / d[2];
        const float px = o[0] + t * d[0], py = o[1] + t * d[1], a = o[2] + t * d[2];
        const float ia = 1.f / a, idz = 1.f / d[2];
        const float g_ox = cw * (goo[0] - gdo[0]), g_oy = ch * (goo[1] - gdo[1]);            // d loss / d (o'_x / a), d (o'_y / a)
        const float gp[3] = {g_ox * ia, g_oy * ia, (2.f * (gdo[2] - goo[2]) - g_ox * px - g_oy * py) * ia * ia};   // d loss / d o'
        const float g_t = gp[0] * d[0] + gp[1] * d[1] + gp[2] * d[2];
        go[0] = gp[0]; go[1] = gp[1]; go[2] = gp[2] - g_t * idz;
        gd[0] = t * gp[0] + cw * gdo[0] * idz;
        gd[1] = t * gp[1] + ch * gdo[1] * idz;
        gd[2] = t * gp[2] - (cw * gdo[0] * d[0] + ch * gdo[1] * d[1]) * idz * idz + g_t * (1.f + o[2]) * idz * idz;
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) { go[c] = goo[c]; gd[c] = gdo[c]; }
    }
    const float n2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2], inr = 1.f / sqrtf(n2);
    const float dot = (gv[0] * d[0] + gv[1] * d[1] + gv[2] * d[2]) / n2;                    // (viewdirs . g) / |d|
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gd[c] += (gv[c] - d[c] * dot) * inr;
        d_rays[i * 6 + c * 2] = go[c];
        d_rays[i * 6 + c * 2 + 1] = gd[c];
    }
}

// reference networks/renderer.py:163-178
__global__ void k_sample_z(const float* __restrict__ rb, int nc, long R, int S, int lindisp, int perturb,
                           const float* __restrict__ t_rand, float* __restrict__ z, float* __restrict__ pts) {
    // pts (or null): the sample positions o + d z as k_points writes them (renderer.py:180), one launch less in a c2f render
    const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (idx >= R * S) return;
    const long r = idx / S;
    const float zi = stratified_z(rb[r * nc + 6], rb[r * nc + 7], S, idx % S, lindisp, perturb, t_rand, idx);
    z[idx] = zi;
    if (pts) {
#pragma unroll
        for (int c = 0; c < 3; ++c) pts[idx * 3 + c] = ray_point(rb[r * nc + c], rb[r * nc + 3 + c], zi);
    }
}

// k_ray_batch + k_sample_z in one launch (evd_nerf_render: near / far are the configuration's scalars, so z does not depend on the packed
// row): thread = (ray, sample); the sample-0 thread also packs the ray's row (always 11 columns).
__global__ void k_ray_batch_z(const float* __restrict__ rays, long R, int ndc, float cw, float ch, float near, float far, int S, int lindisp, int perturb,
                              const float* __restrict__ t_rand, float* __restrict__ rb, float* __restrict__ z) {
    const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (idx >= R * S) return;
    const long r = idx / S;
    const int i = idx % S;
    z[idx] = stratified_z(near, far, S, i, lindisp, perturb, t_rand, idx);
    if (i != 0) return;
    float o[3], d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { o[c] = rays[r * 6 + c * 2]; d[c] = rays[r * 6 + c * 2 + 1]; }
    pack_ray_row(o, d, ndc, 1, cw, ch, near, far, rb + r * 11);
}

__global__ void k_points(const float* __restrict__ rb, int nc, const float* __restrict__ z, long n, int S, float* __restrict__ pts) {
    const long s = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (s >= n) return;
    const float* r = rb + (s / S) * nc;
    const float zv = z[s];
#pragma unroll
    for (int c = 0; c < 3; ++c) pts[s * 3 + c] = ray_point(r[c], r[3 + c], zv);
}

// pts = o + d z under autograd: d pts [R,S,3] -> rows of d ray_batch (columns 0..2 += sum_s d pts, 3..5 += sum_s z d pts; the others are
// left alone): one wavefront per ray, shuffle reduction (S <= a few hundred)
__global__ __launch_bounds__(256) void k_points_bwd(const float* __restrict__ z, const float* __restrict__ d_pts, long R, int S, int accumulate,
                                                    float* __restrict__ d_rb) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= R) return;
    float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s = lane; s < S; s += 64) {
        const float zv = z[r * S + s];
        const float* p = d_pts + (r * S + s) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) { a[c] += p[c]; a[3 + c] += zv * p[c]; }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) a[q] = wave_sum(a[q]);
    if (lane < 11) {                 // overwrite mode: the whole row (zeros in the near / far / viewdirs columns), so the caller needs no fill
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < 6; ++q) v = lane == q ? a[q] : v;
        float* out = d_rb + r * 11 + lane;
        if (accumulate) { if (lane < 6) *out += v; }
        else *out = v;
    }
}

// reference networks/embedding.py:88-98
__global__ void k_embed(const float* __restrict__ x, long n, int dim, int L, float* __restrict__ out) {
    const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (idx >= n * dim) return;
    const long i = idx / dim;
    const int c = idx % dim;
    const int od = dim * (1 + 2 * L);
    const float v = x[idx];
    float* o = out + i * od;
    o[c] = v;
    float f = 1.f;
    for (int k = 0; k < L; ++k) {
        const float a = v * f;
        o[dim + 2 * k * dim + c] = sinf(a);
        o[dim + (2 * k + 1) * dim + c] = cosf(a);
        f *= 2.f;
    }
}

static void ndc_coeffs(int H, int W, float focal, float* cw, float* ch) {
    // Python doubles in the reference (utils/rays.py:135-140), rounded to float32 when they meet the tensor
    *cw = (float)(-1.0 / ((double)W / (2.0 * (double)focal)));
    *ch = (float)(-1.0 / ((double)H / (2.0 * (double)focal)));
}

// evd_sample_z + the sample positions (internal: evd_c2f_render_rays)
int launch_sample_z_pts(const evd_render_cfg* cfg, const float* ray_batch, int ncol, long R, const float* t_rand, float* z, float* pts, hipStream_t stream) {
    EVD_REQUIRE(cfg && R >= 0 && z && cfg->N_samples > 0, "evd_sample_z: bad arguments");
    EVD_REQUIRE(!(cfg->perturb > 0.f) || t_rand, "evd_sample_z: perturb > 0 needs the explicit t_rand draw");
    if (R == 0) return EVD_OK;
    EVD_REQUIRE(ray_batch && ncol >= 8, "evd_sample_z: the packed rays (near / far at columns 6, 7) are missing");
    k_sample_z<<<cdiv(R * cfg->N_samples, 256), 256, 0, stream>>>(ray_batch, ncol, R, cfg->N_samples, cfg->lindisp, cfg->perturb > 0.f, t_rand, z, pts);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // namespace evd

using namespace evd;

extern "C" {

int evd_get_rays(int H, int W, const float* K, const float* c2w, int add_halfpix, float* rays_o, float* rays_d, void* stream) {
    EVD_REQUIRE(H > 0 && W > 0 && K && c2w && rays_o && rays_d, "evd_get_rays: bad arguments");
    Pose34 pose;
    memcpy(pose.m, c2w, sizeof(pose.m));
    const long n = (long)H * W;
    k_get_rays<<<cdiv(n, 256), 256, 0, as_stream(stream)>>>(H, W, K[0], K[2], K[4], K[5], add_halfpix ? 0.5f : 0.f, pose, rays_o, rays_d);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_get_rays_pix(const float* coords, const float* K, const float* c2ws, long n, int add_halfpix, float* rays_o, float* rays_d, void* stream) {
    EVD_REQUIRE(n >= 0 && K && rays_o && rays_d, "evd_get_rays_pix: bad arguments");
    if (n == 0) return EVD_OK;
    EVD_REQUIRE(coords && c2ws, "evd_get_rays_pix: null coords or c2ws");
    k_get_rays_pix<<<cdiv(n, 256), 256, 0, as_stream(stream)>>>(coords, K[0], K[2], K[4], K[5], add_halfpix ? 0.5f : 0.f, c2ws, n, rays_o, rays_d);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_ndc_rays(int H, int W, float focal, float near, const float* rays_o, const float* rays_d, long n,
                 float* out_o, float* out_d, void* stream) {
    EVD_REQUIRE(n >= 0 && out_o && out_d, "evd_ndc_rays: bad arguments");
    if (n == 0) return EVD_OK;
    EVD_REQUIRE(rays_o && rays_d, "evd_ndc_rays: null rays_o or rays_d");
    float cw, ch;
    ndc_coeffs(H, W, focal, &cw, &ch);
    k_ndc<<<cdiv(n, 256), 256, 0, as_stream(stream)>>>(cw, ch, near, (float)(2.0 * (double)near), rays_o, rays_d, n, out_o, out_d);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_embed(const float* x, long n, int dim, int L, float* out, void* stream) {
    EVD_REQUIRE(n >= 0 && dim > 0 && L >= 0 && out, "evd_embed: bad arguments");
    if (n == 0) return EVD_OK;
    EVD_REQUIRE(x, "evd_embed: null x");
    k_embed<<<cdiv(n * dim, 256), 256, 0, as_stream(stream)>>>(x, n, dim, L, out);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_rbk_warp(const float* rays, const float* r, const float* v, long R, int M, int use_origin, float* new_rays, float* transforms,
                 void* stream) {
    EVD_REQUIRE(R >= 0 && M >= 1 && (R == 0 || (rays && r && v && new_rays)), "evd_rbk_warp: bad arguments");
    if (R == 0) return EVD_OK;
    const long n = R * (long)(M + (use_origin ? 1 : 0));
    k_rbk_warp<<<cdiv(n, 256), 256, 0, as_stream(stream)>>>(rays, r, v, R, M, use_origin, new_rays, transforms);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_ray_batch(const evd_render_cfg* cfg, const float* rays, long R, float* ray_batch, void* stream) {
    EVD_REQUIRE(cfg && R >= 0 && ray_batch, "evd_ray_batch: bad arguments");
    if (R == 0) return EVD_OK;
    EVD_REQUIRE(rays, "evd_ray_batch: null rays");
    float cw, ch;
    ndc_coeffs(cfg->H, cfg->W, cfg->focal, &cw, &ch);
    k_ray_batch<<<cdiv(R, 256), 256, 0, as_stream(stream)>>>(rays, R, cfg->ndc, cfg->use_viewdirs, cw, ch, cfg->near, cfg->far, ray_batch);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_ray_batch_bwd(const evd_render_cfg* cfg, const float* rays, const float* d_ray_batch, long R, float* d_rays, void* stream) {
    EVD_REQUIRE(cfg && rays && d_ray_batch && d_rays && R >= 0 && cfg->use_viewdirs, "evd_ray_batch_bwd: bad arguments (11-column batch)");
    if (R == 0) return EVD_OK;
    float cw, ch;
    ndc_coeffs(cfg->H, cfg->W, cfg->focal, &cw, &ch);
    k_ray_batch_bwd<<<cdiv(R, 256), 256, 0, as_stream(stream)>>>(rays, d_ray_batch, R, cfg->ndc, cw, ch, d_rays);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

// ray packing + z stratification of evd_nerf_render in one launch
int evd_ray_batch_z(const evd_render_cfg* cfg, const float* rays, long R, const float* t_rand, float* ray_batch, float* z, void* stream) {
    EVD_REQUIRE(cfg && R >= 0 && ray_batch && z && cfg->N_samples > 0 && cfg->use_viewdirs, "evd_ray_batch_z: bad arguments");
    EVD_REQUIRE(!(cfg->perturb > 0.f) || t_rand, "evd_nerf_render: perturb > 0 needs the explicit t_rand draw");
    if (R == 0) return EVD_OK;
    EVD_REQUIRE(rays, "evd_ray_batch_z: null rays");
    float cw, ch;
    ndc_coeffs(cfg->H, cfg->W, cfg->focal, &cw, &ch);
    k_ray_batch_z<<<cdiv(R * cfg->N_samples, 256), 256, 0, as_stream(stream)>>>(rays, R, cfg->ndc, cw, ch, cfg->near, cfg->far, cfg->N_samples, cfg->lindisp,
                                                                               cfg->perturb > 0.f, t_rand, ray_batch, z);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_sample_z(const evd_render_cfg* cfg, const float* ray_batch, int ncol, long R, const float* t_rand, float* z, void* stream) {
    return launch_sample_z_pts(cfg, ray_batch, ncol, R, t_rand, z, nullptr, as_stream(stream));
}
int evd_sample_z_pts(const evd_render_cfg* cfg, const float* ray_batch, int ncol, long R, const float* t_rand, float* z, float* pts, void* stream) {
    EVD_REQUIRE(pts, "evd_sample_z_pts: null pts");
    return launch_sample_z_pts(cfg, ray_batch, ncol, R, t_rand, z, pts, as_stream(stream));
}

int evd_points(const float* ray_batch, int ncol, const float* z, long R, int S, float* pts, void* stream) {
    EVD_REQUIRE(ray_batch && z && pts && ncol >= 6 && R >= 0 && S >= 1, "evd_points: bad arguments");
    if (R == 0) return EVD_OK;
    k_points<<<cdiv(R * (long)S, 256), 256, 0, as_stream(stream)>>>(ray_batch, ncol, z, R * (long)S, S, pts);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_points_bwd(const float* z, const float* d_pts, long R, int S, int accumulate, float* d_ray_batch, void* stream) {
    EVD_REQUIRE(z && d_pts && d_ray_batch && R >= 0 && S >= 1, "evd_points_bwd: bad arguments");
    if (R == 0) return EVD_OK;
    k_points_bwd<<<cdiv(R, 4), 256, 0, as_stream(stream)>>>(z, d_pts, R, S, accumulate, d_ray_batch);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // extern "C"
