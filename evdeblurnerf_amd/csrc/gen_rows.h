// Per-layer kernels on float32 rows (kernel_gen_rows.hip), EVD_PREC_F16X3 training: one Linear + bias + ReLU forward layer, dgrad, wgrad with
// a fixed-order reduction (k_gen_wreduce), the two encodings and their backward.  Every product is an exact float32 one on the matrix cores
// (v_mfma_f32_32x32x2f32), the parameters are read in place from a float32 arena; no floating-point atomics, no host synchronisation.
// Used by the generic NeRF backward (nerf_train_generic.h), the generic PDRF level (voxel_generic.h) and the AWP sample embedding on
// float32 rows (awp_embed_generic.h).
#pragma once

#include "evd_common.h"

namespace evd {

constexpr int GEN_ENC = 64;             // row width of the encoding planes: 3 (1 + 2 L) <= 63 columns in the reference's order, zero padded
constexpr size_t GEN_WS_FLOATS = (size_t)8 << 20;       // wgrad partial sums: at least 102 sample ranges of the largest layer (256 x 319 + bias)

// The per-layer backward launches.  A failed launch sets rc and turns the later calls into no-ops; `who` names the entry in the messages.
struct GenChain {
    long nsamp;
    float* partial;             // GEN_WS_FLOATS floats
    int accumulate;
    hipStream_t st;
    const char* who;
    int rc = EVD_OK;
    // dW[:, c0 : c0 + K] (and db) of one layer from its gradient rows G [nsamp, M] and its input rows X [nsamp, K]
    void wgrad(const float* G, int ldg, int M, const float* X, int ldx, int K, float* dw, int ldw, int c0, float* db);
    // out[s, k] = sum_{m < Mv} G[s, m] Wm[m, c0 + k], k < K (written up to the next multiple of 32: zeros); M = 32, 64, 128 or 256 columns of G
    // are read, rows m >= Mv of Wm are not (Mv = 0: all M)
    void dgrad(int M, const float* G, int ldg, const float* Wm, int ldw, int c0, int K, float* out, int ldo, const float* mask, int ldm,
               const float* eg, const float* ew, int add, int Mv = 0);
};
// PE(pts), PE(dirs) as float32 rows of GEN_ENC columns from rows [nsamp, 8] = (pts xyz, 0, dirs xyz, 0); and d x [nsamp, 3] from d PE(x)
int launch_gen_encode(const float* in, long nsamp, int L, int Lv, float* ep, float* ed, hipStream_t st);
int launch_gen_encode_bwd(const float* enc, const float* denc, long nsamp, int L, float* dx, hipStream_t st);
// out[s, k] = src[s, k] (rows of lds floats; k < Wd, a multiple of 4), zero where mask (rows of Wd floats, a ReLU output) is given and <= 0:
// an output's own gradient placed in a gradient plane [nsamp, Wd] ahead of the dgrad that adds to it
int launch_gen_rows_in(const float* src, long lds, const float* mask, long nsamp, int Wd, float* out, hipStream_t st);

// The forward layer, built for the width of the AWP sample embedding (awp_embed_generic.h):
// out[s, m] = relu(bias[m] + sum_k X[s, k] Wm[m, k]), m < 64, k < K in ascending order; out2: a second copy of the rows, or null
constexpr int AWPG_W = 64;
struct GenLinear {
    const float* X; long ldx;       // [nsamp, K] rows of ldx floats (16-byte aligned rows)
    const float* Wm;                // [64, K] nn.Linear layout
    const float* bias;              // [64]
    float *out, *out2;              // [nsamp, 64]
    long nsamp;
};
int launch_gen_linear_relu(int K, const GenLinear& a, hipStream_t st);

}  // namespace evd
