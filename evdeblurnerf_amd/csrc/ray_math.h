// The per-ray arithmetic of the render front end, each formula once (device inlines only): camera ray direction, |d|, NDC, sample position,
// z stratification and the packed ray row.  Every step is an unfused __fmul_rn / __fadd_rn sequence in the operation order of the
// reference's elementwise tensor ops; the kernels that write the same quantity (kernels_rays.hip, kernels_sample_pdf.hip,
// kernels_loader.hip, kernels_events.hip, the compositing and AWP scans) agree bit for bit because they all call these.
#pragma once

#include "evd_common.h"

namespace evd {

// component r of the camera ray through (d0, d1, -1): d0 c2w[r,0] + d1 c2w[r,1] + (-1) c2w[r,2]  (utils/rays.py:16,32); c2w is a [3,4] pose
__device__ __forceinline__ float camera_ray_dir(float d0, float d1, const float* c2w, int r) {
    const float d2 = -1.f;
    return __fadd_rn(__fadd_rn(__fmul_rn(d0, c2w[r * 4]), __fmul_rn(d1, c2w[r * 4 + 1])), __fmul_rn(d2, c2w[r * 4 + 2]));
}

// |d| as torch.norm(rays_d, dim=-1) accumulates it
__device__ __forceinline__ float ray_norm(const float* d) {
    return sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(d[0], d[0]), __fmul_rn(d[1], d[1])), __fmul_rn(d[2], d[2])));
}

// reference utils/rays.py:104-145 (unfused mul/add like the reference's elementwise tensor ops)
__device__ __forceinline__ void ndc_one(float cw, float ch, float near, float two_near, const float o[3], const float d[3],
                                        float oo[3], float od[3]) {
    const float t = -__fadd_rn(near, o[2]) / d[2];
    const float ox = __fadd_rn(o[0], __fmul_rn(t, d[0])), oy = __fadd_rn(o[1], __fmul_rn(t, d[1])),
                oz = __fadd_rn(o[2], __fmul_rn(t, d[2]));
    const float ox_oz = ox / oz, oy_oz = oy / oz;
    const float o2 = __fadd_rn(1.f, two_near / oz);
    oo[0] = __fmul_rn(cw, ox_oz);
    oo[1] = __fmul_rn(ch, oy_oz);
    oo[2] = o2;
    od[0] = __fmul_rn(cw, __fsub_rn(d[0] / d[2], ox_oz));
    od[1] = __fmul_rn(ch, __fsub_rn(d[1] / d[2], oy_oz));
    od[2] = __fsub_rn(1.f, o2);
}

// one coordinate of the sample position o + d z  (renderer.py:180,206)
__device__ __forceinline__ float ray_point(float o, float d, float z) { return __fadd_rn(o, __fmul_rn(d, z)); }

// sample i of S between near and far, linear in depth or in disparity; with perturb, drawn between the midpoints to its neighbours by
// t_rand[idx]  (renderer.py:163-178)
__device__ __forceinline__ float stratified_z(float near, float far, int S, int i, int lindisp, int perturb, const float* t_rand, long idx) {
    auto zat = [&](int k) {
        const float t = linspace_at(0.f, 1.f, S, k);
        return lindisp ? 1.f / __fadd_rn(__fmul_rn(1.f / near, __fsub_rn(1.f, t)), __fmul_rn(1.f / far, t))
                       : __fadd_rn(__fmul_rn(near, __fsub_rn(1.f, t)), __fmul_rn(far, t));
    };
    float zi = zat(i);
    if (perturb) {
        const float upper = (i < S - 1) ? __fmul_rn(.5f, __fadd_rn(zat(i + 1), zi)) : zi;
        const float lower = (i > 0) ? __fmul_rn(.5f, __fadd_rn(zi, zat(i - 1))) : zi;
        zi = __fadd_rn(lower, __fmul_rn(__fsub_rn(upper, lower), t_rand[idx]));
    }
    return zi;
}

// one ray (o, d) -> its ray_batch row: o, d (through NDC if asked), near, far and, with use_viewdirs, d / |d| of the world-space direction
// in columns 8..10  (renderer.py:423-446).  o and d are overwritten.
__device__ __forceinline__ void pack_ray_row(float o[3], float d[3], int ndc, int use_viewdirs, float cw, float ch, float near, float far, float* out) {
    if (use_viewdirs) {
        const float nrm = ray_norm(d);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[8 + c] = d[c] / nrm;
    }
    if (ndc) {
        float x[3], y[3];
        ndc_one(cw, ch, 1.f, 2.f, o, d, x, y);   // get_ndc_rays(H, W, K[0][0], 1., ...) renderer.py:437
#pragma unroll
        for (int c = 0; c < 3; ++c) { o[c] = x[c]; d[c] = y[c]; }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { out[c] = o[c]; out[3 + c] = d[c]; }
    out[6] = near;
    out[7] = far;
}

}  // namespace evd
