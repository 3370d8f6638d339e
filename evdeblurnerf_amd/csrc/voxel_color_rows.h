// Colour network of a composite_feature level, per RAY (voxnerf.py:231-239): h = cat([feature_map, PE(dirs)]) -> Linear + ReLU
// (num_layers_color - 1 times) -> Linear -> sigmoid.  One row function for the inference pass (evd_voxel_render_api.hip) and the training
// forward (evd_voxel_color_api.hip): same float32 fma order, same bits.
#pragma once

#include "evd_common.h"

namespace evd {

// element c of the direction encoding of one component d (embedding.py:88-98: [x, sin(x f0), cos(x f0), sin(x f1), ...], 3 values each)
__device__ __forceinline__ float color_rows_dir_enc(int c, float d) {
    return c < 3 ? d : ((c - 3) / 3 % 2 == 0 ? sinf(d * (float)(1 << ((c - 3) / 6))) : cosf(d * (float)(1 << ((c - 3) / 6))));
}

// A wavefront per ray, a lane per hidden unit (HD <= 256: up to 4 units per lane); the weights are the reference's float32 [out, in]
// rows, read through the caches (7 k MACs per ray: nothing to optimise).  KEEP: the two hidden activations (after their ReLU) go to
// keep_h0 / keep_h1 [R, HD] for the backward.
template <bool KEEP>
static __global__ __launch_bounds__(256) void k_color_rows(const float* __restrict__ cnet, const float* __restrict__ fm, const float* __restrict__ viewdirs,
                                                           int vd_stride, long R, int G, int HD, int Lv, float* __restrict__ color,
                                                           float* __restrict__ keep_h0, float* __restrict__ keep_h1) {
    __shared__ float in[4][160], h0[4][256], h1[4][256];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + w;
    const int icv = 3 * (1 + 2 * Lv), nin = G + icv;
    const float *w0 = cnet, *b0 = w0 + (long)HD * nin, *w1 = b0 + HD, *b1 = w1 + (long)HD * HD, *w2 = b1 + HD, *b2 = w2 + 3L * HD;
    if (r < R) {
        for (int i = lane; i < nin; i += 64) {
            float x;
            if (i < G) x = fm[r * G + i];
            else {
                const int c = i - G;
                x = color_rows_dir_enc(c, viewdirs[r * vd_stride + c % 3]);
            }
            in[w][i] = x;
        }
    }
    __syncthreads();
    if (r < R)
        for (int j = lane; j < HD; j += 64) {
            float s = b0[j];
            for (int i = 0; i < nin; ++i) s = fmaf(w0[(long)j * nin + i], in[w][i], s);
            h0[w][j] = fmaxf(s, 0.f);
            if (KEEP) keep_h0[r * HD + j] = h0[w][j];
        }
    __syncthreads();
    if (r < R)
        for (int j = lane; j < HD; j += 64) {
            float s = b1[j];
            for (int i = 0; i < HD; ++i) s = fmaf(w1[(long)j * HD + i], h0[w][i], s);
            h1[w][j] = fmaxf(s, 0.f);
            if (KEEP) keep_h1[r * HD + j] = h1[w][j];
        }
    __syncthreads();
    if (r < R && lane < 3) {
        float s = b2[lane];
        for (int i = 0; i < HD; ++i) s = fmaf(w2[(long)lane * HD + i], h1[w][i], s);
        color[r * 3 + lane] = 1.f / (1.f + expf(-s));            // torch.sigmoid(h) voxnerf.py:239
    }
}

}  // namespace evd
