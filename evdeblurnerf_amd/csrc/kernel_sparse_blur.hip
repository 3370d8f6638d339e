// BlurModel.forward (networks/pdrf/blurmodel.py:109-224, kernel_type DSK and PBE, with ViewEmbedding.forward in front) and its backward.
// The reference runs about 60 small tensor ops each way on R P rows; here the network and the rays are one forward launch (DSK's align, a
// mean over the batch, takes a second launch of one workgroup) and the backward is two launches.
//
// A float32 tile network (mfma_f32_tile.h holds the scheme and everything the family shares).  A workgroup takes tiles in grid-stride
// order; a tile is 16 rows = T = 16 / P whole rays with all their P points, so the softmax over a ray's points and the ray's shared columns
// never leave the tile.  The row is the N dimension of every product, dealt to the wavefronts round robin; the rows, the hidden layers and
// the backward's d pre-activations live in zero-padded LDS arrays, and the parameters are read in place in torch layout.  The backward
// keeps nothing from the forward: it recomputes the rows and the hidden layers, walks d out -> d hidden -> d row on the matrix core, and
// forms the weight gradients (sb_products; a bias gradient is the product with a column of ones) with the family's resident accumulators.
// k_sparse_blur_reduce sums their partials and forms the per-image sums of pattern_pos, pattern_trans and the embedding table in ray order.
// sinf / cosf / tanhf / expf are the accurate ones.
#include <algorithm>
#include <cstddef>

#include "evd_common.h"
#include "mfma_f32_tile.h"

namespace evd {

constexpr int SB_NT = MT_NT, SB_NW = MT_NW;
constexpr int SB_ROWS = MT_TR;        // rows of a tile
constexpr int SB_MAXIN = 127, SB_MAXW = 64, SB_MAXP = 16, SB_MAXH = 4, SB_MAXL = 4;
constexpr int SB_XS = 129;            // row: up to 127 values, zeros up to a multiple of 16, odd stride
constexpr int SB_HS = 65;             // hidden row / d pre-activation row
constexpr int SB_OS = 17;             // output row (3 or 5 values, padded to 16)
constexpr int SB_MAX_BLOCKS = 128;

struct SbK {
    evd_sparse_blur_params p;
    const long* ids;
    const float *x, *rays_x, *rays_y, *poses, *noise, *feats;
    long R;
    int pbe, P, T, Lin, Lsp, C, F, nh, Wd, sc, isglobal, trans_src, n_img, n_pat, poses_per_image;      // trans_src: 0 none, 1 the network, 2 pattern_trans
    int Ein, in_cnl, n_out, ng;                                                // ng: the row's gradient-bearing columns (all but the spatial ones)
    float hw, rhw, pi_hw, div_x, div_y, fx, fy, cx, cy, inv2R;
    // forward outputs
    float *new_rays, *weight, *img_embed, *align_terms;
    // backward
    const float *d_new_rays, *d_weight, *d_align, *d_img_embed;
    float *dxe, *dpp, *dpt, *d_feats, *partial;
    MtMats mats;                       // the weight-gradient products
};

struct SbSmem {
    float xs[SB_ROWS][SB_XS];
    float hs[SB_MAXH + 1][SB_ROWS][SB_HS];          // linears' layers, then linears1.0
    float dp[SB_MAXH + 1][SB_ROWS][SB_HS];
    float o[SB_ROWS][SB_OS];
    float one[SB_ROWS][SB_OS];                      // column 0: 1 for a row of the batch
    float pos[SB_ROWS][2], dpos[SB_ROWS][2];        // input_pos and the gradient that reaches it past the network
};
#define SB_OFF(field) ((int)(offsetof(SbSmem, field) / sizeof(float)))

// The weight-gradient products d Y^T X (weight and bias of each layer, linears1.0 with the short cut in two column parts) and the
// network tensors behind pl.ten.end, in the flat gradient's order
constexpr void sb_products(MtPlan& pl, int nh, int Wd, int in_cnl, int sc, int n_out) {
    const int layer = SB_ROWS * SB_HS;
    for (int l = 0; l <= nh; ++l) {                                  // linears, then linears1.0
        const int dy = SB_OFF(dp) + l * layer, hx = SB_OFF(hs) + (l - 1) * layer;
        if (l == 0) {
            pl.add_tensor(Wd, in_cnl, pl.add_mat(Wd, in_cnl, dy, SB_HS, SB_OFF(xs), SB_XS));
        } else if (l == nh && sc) {
            const MtMat wx = pl.add_mat(Wd, in_cnl, dy, SB_HS, SB_OFF(xs), SB_XS);
            pl.add_tensor(Wd, in_cnl + Wd, wx, 0, in_cnl, pl.add_mat(Wd, Wd, dy, SB_HS, hx, SB_HS));
        } else {
            pl.add_tensor(Wd, Wd, pl.add_mat(Wd, Wd, dy, SB_HS, hx, SB_HS));
        }
        pl.add_tensor(Wd, 1, pl.add_mat(Wd, 1, dy, SB_HS, SB_OFF(one), SB_OS));
    }
    pl.add_tensor(n_out, Wd, pl.add_mat(n_out, Wd, SB_OFF(o), SB_OS, SB_OFF(hs) + nh * layer, SB_HS));      // linears1.2
    pl.add_tensor(n_out, 1, pl.add_mat(n_out, 1, SB_OFF(o), SB_OS, SB_OFF(one), SB_OS));
}
constexpr int sb_max_tiles() {
    MtPlan pl{};
    sb_products(pl, SB_MAXH, SB_MAXW, SB_MAXIN, 1, 5);
    return pl.mats.n_tiles;
}
constexpr int SB_MAX_TILES = sb_max_tiles();                                  // weight-gradient tiles at the largest shape
constexpr int SB_TPW = (SB_MAX_TILES + SB_NW - 1) / SB_NW;                    // ... of one wavefront

// image id of a ray, -1 outside [0, n)
__device__ __forceinline__ long sb_id(const SbK& k, long ray, int n) {
    const long id = k.ids[ray];
    return id >= 0 && id < n ? id : -1;
}

// rows, hidden layers and outputs of the tile's 16 rows from ray0 on, left in s.xs / s.hs / s.o / s.pos / s.one
__device__ __forceinline__ void sb_network(const SbK& k, SbSmem& s, long ray0, bool write_embed) {
    const int tid = threadIdx.x, wv = tid >> 6;
    const int nx = 16 * ((k.in_cnl + 15) / 16), rows = k.T * k.P;
    if (tid < 2 * SB_ROWS) {                                        // canonical position and its embedding: one lane per (row, component)
        const int r = tid >> 1, c = tid & 1, pnt = r % k.P;
        const long ray = ray0 + r / k.P;
        const bool valid = r < rows && ray < k.R;
        float pt = 0.f;
        if (valid) {
            const long pi = k.isglobal ? 0 : sb_id(k, ray, k.n_pat);
            pt = pi >= 0 ? tanhf(k.p.pattern_pos[(pi * k.P + pnt) * 2 + c]) * k.hw : 0.f;
            if (k.noise) pt = pt + k.noise[(ray * k.P + pnt) * 2 + c] * k.rhw;
        }
        const float v = pt * k.pi_hw;
        s.pos[r][c] = pt;
        s.xs[r][c] = v;
        float freq = 1.f;
        for (int f = 0; f < k.Lin; ++f, freq *= 2.f) {
            s.xs[r][2 + 4 * f + c] = valid ? sinf(v * freq) : 0.f;
            s.xs[r][4 + 4 * f + c] = valid ? cosf(v * freq) : 0.f;
        }
        if (c == 0) s.one[r][0] = valid ? 1.f : 0.f;
    }
    for (int i = tid; i < SB_ROWS * nx; i += SB_NT) {               // the row's other columns: embedding row | feats | spatial embedding | zeros
        const int r = i / nx, c = i % nx, pnt = r % k.P;
        if (c < k.Ein) continue;
        const long ray = ray0 + r / k.P;
        float v = 0.f;
        if (r < rows && ray < k.R) {
            if (c < k.Ein + k.C) {
                const int e = c - k.Ein;
                if (k.x) {
                    v = k.x[ray * k.C + e];
                } else {
                    const long id = sb_id(k, ray, k.n_img);
                    v = id >= 0 ? k.p.table[id * k.C + e] : 0.f;
                }
                if (write_embed && pnt == 0) k.img_embed[ray * k.C + e] = v;
            } else if (c < k.ng) {
                v = k.feats ? k.feats[(ray * k.P + pnt) * k.F + (c - k.Ein - k.C)] : 0.f;
            } else if (c < k.in_cnl) {
                const int j = c - k.ng, q = j < 2 ? j : (j - 2) & 3, comp = q & 1;
                const float sp = comp == 0 ? k.rays_x[ray] / k.div_x - (float)M_PI : k.rays_y[ray] / k.div_y - (float)M_PI;
                if (j < 2) {
                    v = sp;
                } else {
                    const float a = sp * (float)(1 << ((j - 2) >> 2));
                    v = q < 2 ? sinf(a) : cosf(a);
                }
            }
        }
        s.xs[r][c] = v;
    }
    __syncthreads();
    const int mt = (k.Wd + 15) / 16;
    for (int l = 0; l < k.nh; ++l) {                                // linears: (16 units) x 16 rows per job
        const float* in = l == 0 ? &s.xs[0][0] : &s.hs[l - 1][0][0];
        const int K = l == 0 ? k.in_cnl : k.Wd, st = l == 0 ? SB_XS : SB_HS;
        for (int job = wv; job < mt; job += SB_NW) {
            const int m0 = job * 16;
            mt_f4 acc = mt_tile(mt_zero(), k.p.linears_w[l] + (long)m0 * K, K, 1, k.Wd - m0, K, in, st, 1);
            mt_store_relu(&s.hs[l][0][0], SB_HS, acc, k.p.linears_b[l], m0, k.Wd);
        }
        __syncthreads();
    }
    const int ldw = (k.sc ? k.in_cnl : 0) + k.Wd;                   // linears1.0 on [row, hidden] or on the hidden layer
    for (int job = wv; job < mt; job += SB_NW) {
        const int m0 = job * 16;
        const float* w = k.p.linears1_w[0] + (long)m0 * ldw;
        mt_f4 acc = mt_zero();
        if (k.sc) acc = mt_tile(acc, w, ldw, 1, k.Wd - m0, k.in_cnl, &s.xs[0][0], SB_XS, 1);
        acc = mt_tile(acc, w + (ldw - k.Wd), ldw, 1, k.Wd - m0, k.Wd, &s.hs[k.nh - 1][0][0], SB_HS, 1);
        mt_store_relu(&s.hs[k.nh][0][0], SB_HS, acc, k.p.linears1_b[0], m0, k.Wd);
    }
    __syncthreads();
    if (wv == 0) {                                                  // linears1.2: 3 or 5 outputs
        const mt_f4 acc = mt_tile(mt_zero(), k.p.linears1_w[1], k.Wd, 1, k.n_out, k.Wd, &s.hs[k.nh][0][0], SB_HS, 1);
        mt_each(acc, 0, k.n_out, [&](int m, int n, float v) { s.o[n][m] = v + k.p.linears1_b[1][m]; });
    }
    __syncthreads();
}

// One row past the network: delta_trans x 0.01 (t), new_rays_xy (n), and the row's pose (NULL outside the batch's images)
struct SbRow {
    float t[2], n[2];
    const float* pose;
    long pat;
};
__device__ __forceinline__ SbRow sb_row(const SbK& k, const SbSmem& s, int r, long ray, int pnt) {
    SbRow w;
    w.pat = k.isglobal ? 0 : sb_id(k, ray, k.n_pat);
    const int oq = k.n_out - 3;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        float raw = 0.f;
        if (k.trans_src == 1) raw = s.o[r][c];
        else if (k.trans_src == 2 && w.pat >= 0) raw = k.p.pattern_trans[(w.pat * k.P + pnt) * 2 + c];
        w.t[c] = raw * 0.01f;
        w.n[c] = s.o[r][oq + c] + s.pos[r][c];
        if (k.pbe && pnt == 0) w.t[c] = w.n[c] = 0.f;
    }
    const long pr = k.poses_per_image ? k.ids[ray] : ray;
    w.pose = k.poses_per_image && sb_id(k, ray, k.poses_per_image) < 0 ? nullptr : k.poses + pr * 12;
    return w;
}

// softmax over a ray's P logits (column ow of rows r0 ...), as torch: exp(z - max) / sum; weight q is sb_weight(.., q, mx, sum)
__device__ __forceinline__ void sb_softmax(const SbK& k, const SbSmem& s, int r0, float& mx, float& sum) {
    const int ow = k.n_out - 1;
    mx = s.o[r0][ow];
    sum = 0.f;
    for (int q = 1; q < k.P; ++q) mx = fmaxf(mx, s.o[r0 + q][ow]);
    for (int q = 0; q < k.P; ++q) sum += expf(s.o[r0 + q][ow] - mx);
}
__device__ __forceinline__ float sb_weight(const SbK& k, const SbSmem& s, int r0, int q, float mx, float sum) {
    return expf(s.o[r0 + q][k.n_out - 1] - mx) / sum;
}

__global__ __launch_bounds__(SB_NT) void k_sparse_blur_fwd(SbK k) {
    __shared__ SbSmem s;
    const int tid = threadIdx.x;
    const long tiles = (k.R + k.T - 1) / k.T;
    mt_zero_lds(s);
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long ray0 = tile * k.T;
        sb_network(k, s, ray0, true);
        if (tid < k.T * k.P) {                                      // one lane per row: the row's ray
            const int r = tid, pnt = r % k.P;
            const long ray = ray0 + r / k.P;
            if (ray < k.R) {
                const SbRow w = sb_row(k, s, r, ray, pnt);
                const float rx = (k.rays_x[ray] - k.cx + w.n[0]) / k.fx, ry = -(k.rays_y[ray] - k.cy + w.n[1]) / k.fy;
                const float dir[3] = {rx - w.t[0], ry - w.t[1], -1.f};
                float* out = k.new_rays + (ray * k.P + pnt) * 6;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    float p[4] = {0.f, 0.f, 0.f, 0.f};
                    if (w.pose) { p[0] = w.pose[j * 4]; p[1] = w.pose[j * 4 + 1]; p[2] = w.pose[j * 4 + 2]; p[3] = w.pose[j * 4 + 3]; }
                    out[j * 2] = w.t[0] * p[0] + w.t[1] * p[1] + p[3];
                    out[j * 2 + 1] = dir[0] * p[0] + dir[1] * p[1] + dir[2] * p[2];
                }
                if (pnt == 0) {
                    float mx, sum;
                    sb_softmax(k, s, r, mx, sum);
                    for (int q = 0; q < k.P; ++q) k.weight[ray * k.P + q] = sb_weight(k, s, r, q, mx, sum);
                    if (!k.pbe) {                                   // this ray's terms of align's two means
                        k.align_terms[ray * 2] = fabsf(w.n[0]) + fabsf(w.n[1]);
                        k.align_terms[ray * 2 + 1] = fabsf(w.t[0]) + fabsf(w.t[1]);
                    }
                }
            }
        }
        __syncthreads();
    }
}

// align = mean |new_rays_xy[:, 0]| + 10 mean |delta_trans[:, 0]| from the per-ray terms: one workgroup, a fixed order, float64 sums
__global__ __launch_bounds__(256) void k_sparse_blur_align(const float* terms, long R, float* align) {
    __shared__ double acc[2][256];
    double a = 0., b = 0.;
    for (long r = threadIdx.x; r < R; r += 256) { a += terms[r * 2]; b += terms[r * 2 + 1]; }
    acc[0][threadIdx.x] = a;
    acc[1][threadIdx.x] = b;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) { acc[0][threadIdx.x] += acc[0][threadIdx.x + h]; acc[1][threadIdx.x] += acc[1][threadIdx.x + h]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) align[0] = (float)((acc[0][0] + 10. * acc[1][0]) / (2. * (double)R));
}

__device__ __forceinline__ float sb_sign(float v) { return v > 0.f ? 1.f : v < 0.f ? -1.f : 0.f; }

// d hidden = A^T d next through the ReLU, one 16-unit tile: A[m][j] = w[m + j lda]
__device__ __forceinline__ void sb_back(const SbK& k, float (*dp)[SB_HS], const float (*h)[SB_HS], const float* w, int lda, int m0, int K, const float* dnext,
                                        int dstride) {
    const mt_f4 acc = mt_tile(mt_zero(), w + m0, 1, lda, k.Wd - m0, K, dnext, dstride, 1);
    mt_gate_relu(&dp[0][0], SB_HS, &h[0][0], SB_HS, acc, m0, k.Wd);
}

__global__ __launch_bounds__(SB_NT) void k_sparse_blur_bwd(SbK k) {
    __shared__ SbSmem s;
    const int tid = threadIdx.x, wv = tid >> 6;
    const long tiles = (k.R + k.T - 1) / k.T;
    mt_f4 wg[SB_TPW];
#pragma unroll
    for (int i = 0; i < SB_TPW; ++i) wg[i] = mt_zero();
    __shared__ int4 jobs[SB_MAX_TILES];
    mt_jobs(jobs, k.mats, 0, SB_MAX_TILES);
    mt_zero_lds(s);
    const int mt = (k.Wd + 15) / 16, oq = k.n_out - 3, ow = k.n_out - 1, ldw = (k.sc ? k.in_cnl : 0) + k.Wd;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long ray0 = tile * k.T;
        sb_network(k, s, ray0, false);
        // ---- the rays: d new_rays -> d outputs (in place of the outputs), d input_pos, d pattern_trans rows
        if (tid < SB_ROWS) {
            const int r = tid, pnt = r % k.P;
            const long ray = ray0 + r / k.P;
            const bool valid = r < k.T * k.P && ray < k.R;
            float gn[2] = {0.f, 0.f}, gt[2] = {0.f, 0.f}, mx = 0.f, sum = 1.f, dot = 0.f;
            if (valid) {
                const SbRow w = sb_row(k, s, r, ray, pnt);
                const float* g = k.d_new_rays + (ray * k.P + pnt) * 6;
                float go[2] = {0.f, 0.f}, gd[2] = {0.f, 0.f};
                if (w.pose) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        go[0] += g[j * 2] * w.pose[j * 4]; go[1] += g[j * 2] * w.pose[j * 4 + 1];
                        gd[0] += g[j * 2 + 1] * w.pose[j * 4]; gd[1] += g[j * 2 + 1] * w.pose[j * 4 + 1];
                    }
                }
                gt[0] = go[0] - gd[0]; gt[1] = go[1] - gd[1];
                gn[0] = gd[0] / k.fx; gn[1] = -gd[1] / k.fy;
                if (pnt == 0) {
                    if (k.pbe) {
                        gn[0] = gn[1] = gt[0] = gt[1] = 0.f;
                    } else if (k.d_align) {
                        const float ga = k.d_align[0] * k.inv2R;
#pragma unroll
                        for (int c = 0; c < 2; ++c) { gn[c] += ga * sb_sign(w.n[c]); gt[c] += ga * 10.f * sb_sign(w.t[c]); }
                    }
                    sb_softmax(k, s, r, mx, sum);                   // weight = softmax(z): d z = weight (d weight - sum d weight weight)
                    for (int q = 0; q < k.P; ++q) dot += k.d_weight[ray * k.P + q] * sb_weight(k, s, r, q, mx, sum);
                }
                if (k.trans_src == 2) { k.dpt[(ray * k.P + pnt) * 2] = gt[0] * 0.01f; k.dpt[(ray * k.P + pnt) * 2 + 1] = gt[1] * 0.01f; }
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (k.n_out == 5) s.o[r][c] = k.trans_src == 1 ? gt[c] * 0.01f : 0.f;
                s.o[r][oq + c] = gn[c];
                s.dpos[r][c] = gn[c];
            }
            if (!valid) s.o[r][ow] = 0.f;
            else if (pnt == 0)
                for (int q = 0; q < k.P; ++q) s.o[r + q][ow] = sb_weight(k, s, r, q, mx, sum) * (k.d_weight[ray * k.P + q] - dot);
        }
        __syncthreads();
        // ---- d hidden, layer by layer
        for (int job = wv; job < mt; job += SB_NW) sb_back(k, s.dp[k.nh], s.hs[k.nh], k.p.linears1_w[1], k.Wd, job * 16, k.n_out, &s.o[0][0], SB_OS);
        __syncthreads();
        for (int job = wv; job < mt; job += SB_NW)
            sb_back(k, s.dp[k.nh - 1], s.hs[k.nh - 1], k.p.linears1_w[0] + (ldw - k.Wd), ldw, job * 16, k.Wd, &s.dp[k.nh][0][0], SB_HS);
        __syncthreads();
        for (int l = k.nh - 1; l >= 1; --l) {
            for (int job = wv; job < mt; job += SB_NW) sb_back(k, s.dp[l - 1], s.hs[l - 1], k.p.linears_w[l], k.Wd, job * 16, k.Wd, &s.dp[l][0][0], SB_HS);
            __syncthreads();
        }
        // ---- weight gradients: d Y^T X over the tile's rows, both operands in LDS
        mt_accumulate<SB_TPW, true>(wg, jobs, reinterpret_cast<const float*>(&s), k.mats.n_tiles, 0);
        __syncthreads();
        // ---- d row = W0^T d pre0 (+ the short cut's part), in place of the row: its gradient-bearing columns only
        for (int job = wv; job < (k.ng + 15) / 16; job += SB_NW) {
            const int m0 = job * 16;
            mt_f4 acc = mt_tile(mt_zero(), k.p.linears_w[0] + m0, 1, k.in_cnl, k.ng - m0, k.Wd, &s.dp[0][0][0], SB_HS, 1);
            if (k.sc) acc = mt_tile(acc, k.p.linears1_w[0] + m0, 1, ldw, k.ng - m0, k.Wd, &s.dp[k.nh][0][0], SB_HS, 1);
            mt_each(acc, m0, k.ng, [&](int m, int n, float v) { s.xs[n][m] = v; });
        }
        __syncthreads();
        if (tid < 2 * SB_ROWS) {                                    // d pattern_pos rows: through the embedding, input_pos and tanh
            const int r = tid >> 1, c = tid & 1, pnt = r % k.P;
            const long ray = ray0 + r / k.P;
            if (r < k.T * k.P && ray < k.R) {
                const float v = s.pos[r][c] * k.pi_hw;
                float gv = s.xs[r][c], freq = 1.f;
                for (int f = 0; f < k.Lin; ++f, freq *= 2.f)
                    gv += freq * (cosf(v * freq) * s.xs[r][2 + 4 * f + c] - sinf(v * freq) * s.xs[r][4 + 4 * f + c]);
                const long pi = k.isglobal ? 0 : sb_id(k, ray, k.n_pat);
                const float th = pi >= 0 ? tanhf(k.p.pattern_pos[(pi * k.P + pnt) * 2 + c]) : 0.f;
                k.dpp[(ray * k.P + pnt) * 2 + c] = (gv * k.pi_hw + s.dpos[r][c]) * k.hw * (1.f - th * th);
            }
        }
        for (int i = tid; i < k.T * k.C; i += SB_NT) {              // d embedding row: the ray's points in point order (+ what arrives at img_embed)
            const int rl = i / k.C, c = i % k.C;
            const long ray = ray0 + rl;
            if (ray >= k.R) continue;
            float a = 0.f;
            for (int q = 0; q < k.P; ++q) a += s.xs[rl * k.P + q][k.Ein + c];
            k.dxe[ray * k.C + c] = a + (k.d_img_embed ? k.d_img_embed[ray * k.C + c] : 0.f);
        }
        if (k.d_feats) {
            for (int i = tid; i < k.T * k.P * k.F; i += SB_NT) {
                const int r = i / k.F, c = i % k.F;
                const long ray = ray0 + r / k.P;
                if (ray < k.R) k.d_feats[(ray * k.P + r % k.P) * k.F + c] = s.xs[r][k.Ein + k.C + c];
            }
        }
        __syncthreads();
    }
    mt_store_partials(wg, k.partial, k.mats.n_tiles, 0);
}

struct SbReduce {
    const float *partial, *dxe, *dpp, *dpt;
    const long* ids;
    float* grads;
    long R, pat_floats, trans_floats, table_floats;
    int C, P, isglobal, table_form, n_blocks;
    MtTensors ten;                      // the network tensors behind pattern_pos, pattern_trans and the table
};

// One thread per gradient element.  pattern_pos, pattern_trans, table: the rows of the image's rays in ray order (an image without rays
// gets zeros).  The network tensors: the workgroups' partial tiles in workgroup order.
__global__ __launch_bounds__(256) void k_sparse_blur_reduce(SbReduce k) {
    const long e = blockIdx.x * 256L + threadIdx.x;
    if (e >= k.ten.end) return;
    const long net0 = k.pat_floats + k.trans_floats + k.table_floats;
    if (e < k.pat_floats + k.trans_floats) {
        const float* rows = e < k.pat_floats ? k.dpp : k.dpt;
        const long l = e < k.pat_floats ? e : e - k.pat_floats;
        k.grads[e] = mt_rows_of_image_sum(k.ids, k.R, l / (k.P * 2), rows, k.P * 2, (int)(l % (k.P * 2)), k.isglobal);
    } else if (e < net0) {
        const long l = e - k.pat_floats - k.trans_floats;
        k.grads[e] = k.table_form ? mt_rows_of_image_sum(k.ids, k.R, l / k.C, k.dxe, k.C, (int)(l % k.C)) : 0.f;
    } else {
        k.grads[e] = mt_reduce_sum(k.ten, k.partial, k.n_blocks, e);
    }
}

struct SbPlan {
    SbK k;
    SbReduce r;
    int blocks;
};

// workspace of evd_sparse_blur_backward: d embedding rows | d pattern_pos rows | d pattern_trans rows | the workgroups' partial tiles
struct SbWs { float *dxe, *dpp, *dpt, *partial; };
static size_t sb_layout(const SbPlan& pl, void* workspace, SbWs* L) {
    const SbK& k = pl.k;
    FloatSlots ws(workspace);
    L->dxe = ws.take((size_t)k.R * k.C);
    L->dpp = ws.take(2 * (size_t)k.R * k.P);
    L->dpt = ws.take(2 * (size_t)k.R * k.P);
    L->partial = ws.take(mt_partial_floats(pl.blocks, k.mats.n_tiles));
    return ws.bytes();
}
// workspace of evd_sparse_blur_forward (DSK): the rays' terms of align's two means
static size_t sb_layout_fwd(const SbPlan& pl, void* workspace, float** align_terms) {
    FloatSlots ws(workspace);
    *align_terms = ws.take(2 * (size_t)pl.k.R);
    return ws.bytes();
}

static int sb_plan(const char* who, const evd_sparse_blur_desc* d, long R, SbPlan* out) {
    EVD_REQUIRE(d, "%s: null descriptor", who);
    EVD_REQUIRE(d->kernel_type == 0 || d->kernel_type == 1, "%s: kernel_type %d is neither 0 (DSK) nor 1 (PBE)", who, d->kernel_type);
    EVD_REQUIRE(d->num_wide >= 1 && d->num_wide <= SB_MAXW, "%s: num_wide %d outside 1..%d", who, d->num_wide, SB_MAXW);
    EVD_REQUIRE(d->num_hidden >= 1 && d->num_hidden <= SB_MAXH, "%s: num_hidden %d outside 1..%d", who, d->num_hidden, SB_MAXH);
    EVD_REQUIRE(d->num_pt >= 1 && d->num_pt <= SB_MAXP, "%s: num_pt %d outside 1..%d", who, d->num_pt, SB_MAXP);
    EVD_REQUIRE(d->in_embed >= 1 && d->in_embed <= SB_MAXL, "%s: in_embed %d outside 1..%d", who, d->in_embed, SB_MAXL);
    EVD_REQUIRE(d->spatial_embed >= 0 && d->spatial_embed <= SB_MAXL, "%s: spatial_embed %d outside 0..%d", who, d->spatial_embed, SB_MAXL);
    EVD_REQUIRE(d->embed_cnl >= 0 && d->embed_cnl <= (1 << 20) && d->feat_cnl >= 0 && d->feat_cnl <= (1 << 20), "%s: embed_cnl / feat_cnl out of range", who);
    SbK& k = out->k;
    memset(out, 0, sizeof(*out));
    k.Ein = 2 * (1 + 2 * d->in_embed);
    k.C = d->embed_cnl;
    k.F = d->feat_cnl;
    k.ng = k.Ein + k.C + k.F;
    k.in_cnl = k.ng + (d->spatial_embed ? 2 * (1 + 2 * d->spatial_embed) : 0);
    EVD_REQUIRE(k.in_cnl <= SB_MAXIN, "%s: row width %d (embedded position %d + embed_cnl %d + feat_cnl %d + spatial embedding %d) above %d", who, k.in_cnl,
                k.Ein, k.C, k.F, k.in_cnl - k.ng, SB_MAXIN);
    EVD_REQUIRE(R >= 0 && d->n_img >= 0 && d->n_pattern >= 0 && d->poses_per_image >= 0, "%s: negative size", who);
    EVD_REQUIRE(d->kernel_hwindow > 0.f && d->fx != 0.f && d->fy != 0.f && d->H > 0 && d->W > 0, "%s: kernel_hwindow, fx, fy, H, W must be non-zero", who);
    k.pbe = d->kernel_type;
    k.P = d->num_pt;
    k.T = SB_ROWS / k.P;
    k.Lin = d->in_embed;
    k.Lsp = d->spatial_embed;
    k.nh = d->num_hidden;
    k.Wd = d->num_wide;
    k.sc = d->short_cut ? 1 : 0;
    k.isglobal = d->isglobal ? 1 : 0;
    k.trans_src = d->optim_trans ? 2 : d->optim_spatialvariant_trans ? 1 : 0;
    k.n_out = d->optim_spatialvariant_trans ? 5 : 3;
    k.n_img = d->n_img;
    k.n_pat = d->n_pattern;
    k.poses_per_image = d->poses_per_image;
    k.hw = d->kernel_hwindow;
    k.rhw = d->random_hwindow;
    k.pi_hw = (float)(M_PI / (double)d->kernel_hwindow);
    k.div_x = (float)(d->W / 2.0 / M_PI);
    k.div_y = (float)(d->H / 2.0 / M_PI);
    k.fx = d->fx; k.fy = d->fy; k.cx = d->cx; k.cy = d->cy;
    k.inv2R = R > 0 ? (float)(1.0 / (2.0 * (double)R)) : 0.f;
    k.R = R;
    SbReduce& r = out->r;
    MtPlan mp{};
    mp.ten.end = (long)k.n_pat * k.P * 2 * (d->optim_trans ? 2 : 1) + (long)k.n_img * k.C;      // pattern_pos, pattern_trans, the table come first
    sb_products(mp, k.nh, k.Wd, k.in_cnl, k.sc, k.n_out);
    const int rc = mt_check(who, mp, SB_MAX_TILES);
    if (rc != EVD_OK) return rc;
    k.mats = mp.mats;
    r.ten = mp.ten;
    r.pat_floats = (long)k.n_pat * k.P * 2;
    r.trans_floats = d->optim_trans ? r.pat_floats : 0;
    r.table_floats = (long)k.n_img * k.C;
    r.C = k.C > 0 ? k.C : 1;
    r.P = k.P;
    r.isglobal = k.isglobal;
    r.R = R;
    out->blocks = (int)std::min<long>(cdiv(R, k.T), SB_MAX_BLOCKS);
    return EVD_OK;
}

// the inputs of a call with R > 0
static int sb_inputs(const char* who, const evd_sparse_blur_desc* d, const evd_sparse_blur_params* p, const long* ids, const float* x, const float* rays_x,
                     const float* rays_y, const float* poses, const float* noise, const float* feats, SbPlan* pl) {
    SbK& k = pl->k;
    EVD_REQUIRE(p && ids && rays_x && rays_y && poses, "%s: null parameters / ids / rays_x / rays_y / poses", who);
    EVD_REQUIRE(x ? true : (p->table != nullptr && d->n_img >= 1), "%s: needs the embedding table, or per-ray embedding rows", who);
    EVD_REQUIRE(p->pattern_pos && d->n_pattern >= 1, "%s: null pattern_pos", who);
    EVD_REQUIRE(!d->optim_trans || p->pattern_trans, "%s: optim_trans without pattern_trans", who);
    for (int l = 0; l < k.nh; ++l) EVD_REQUIRE(p->linears_w[l] && p->linears_b[l], "%s: null parameter tensor (linears)", who);
    EVD_REQUIRE(p->linears1_w[0] && p->linears1_b[0] && p->linears1_w[1] && p->linears1_b[1], "%s: null parameter tensor (linears1)", who);
    EVD_REQUIRE(!feats || k.F > 0, "%s: feats with feat_cnl 0", who);
    k.p = *p;
    k.ids = ids;
    k.x = x;
    k.rays_x = rays_x;
    k.rays_y = rays_y;
    k.poses = poses;
    k.noise = noise;
    k.feats = feats;
    return EVD_OK;
}

}  // namespace evd

using namespace evd;

extern "C" {

size_t evd_sparse_blur_workspace_bytes(const evd_sparse_blur_desc* d, long R) {
    SbPlan pl;
    if (R < 0 || sb_plan("evd_sparse_blur_workspace_bytes", d, R, &pl) != EVD_OK) return 0;
    SbWs L;
    return sb_layout(pl, nullptr, &L);
}

int evd_sparse_blur_forward(const evd_sparse_blur_desc* d, const evd_sparse_blur_params* p, const long* ids, const float* x, const float* rays_x,
                            const float* rays_y, const float* poses, const float* noise, const float* feats, long R, float* new_rays, float* weight,
                            float* align, float* img_embed, void* workspace, size_t workspace_bytes, void* stream) {
    SbPlan pl;
    int rc = sb_plan("evd_sparse_blur_forward", d, R, &pl);
    if (rc != EVD_OK) return rc;
    if (R == 0) return EVD_OK;
    rc = sb_inputs("evd_sparse_blur_forward", d, p, ids, x, rays_x, rays_y, poses, noise, feats, &pl);
    if (rc != EVD_OK) return rc;
    EVD_REQUIRE(new_rays && weight && img_embed && (align || pl.k.pbe), "evd_sparse_blur_forward: null output");
    if (!pl.k.pbe) {
        const size_t need = sb_layout_fwd(pl, workspace, &pl.k.align_terms);
        if (!workspace || workspace_bytes < need) return fail(EVD_E_WORKSPACE, "evd_sparse_blur_forward: workspace %zu < %zu bytes", workspace_bytes, need);
    }
    pl.k.new_rays = new_rays;
    pl.k.weight = weight;
    pl.k.img_embed = img_embed;
    k_sparse_blur_fwd<<<pl.blocks, SB_NT, 0, as_stream(stream)>>>(pl.k);
    EVD_LAUNCH_CHECK();
    if (!pl.k.pbe) {
        k_sparse_blur_align<<<1, 256, 0, as_stream(stream)>>>(pl.k.align_terms, R, align);
        EVD_LAUNCH_CHECK();
    }
    return EVD_OK;
}

int evd_sparse_blur_backward(const evd_sparse_blur_desc* d, const evd_sparse_blur_params* p, const long* ids, const float* x, const float* rays_x,
                             const float* rays_y, const float* poses, const float* noise, const float* feats, long R, const float* d_new_rays,
                             const float* d_weight, const float* d_align, const float* d_img_embed, float* grads, float* d_x, float* d_feats,
                             void* workspace, size_t workspace_bytes, void* stream) {
    SbPlan pl;
    int rc = sb_plan("evd_sparse_blur_backward", d, R, &pl);
    if (rc != EVD_OK) return rc;
    EVD_REQUIRE(grads, "evd_sparse_blur_backward: null gradient buffer");
    SbReduce& rk = pl.r;
    rk.grads = grads;
    rk.ids = ids;
    rk.table_form = x ? 0 : 1;
    if (R > 0) {
        rc = sb_inputs("evd_sparse_blur_backward", d, p, ids, x, rays_x, rays_y, poses, noise, feats, &pl);
        if (rc != EVD_OK) return rc;
        EVD_REQUIRE(d_new_rays && d_weight, "evd_sparse_blur_backward: null d new_rays / d weight");
        EVD_REQUIRE(!d_feats || pl.k.F > 0, "evd_sparse_blur_backward: d feats with feat_cnl 0");
        SbWs L;
        const size_t need = sb_layout(pl, workspace, &L);
        if (!workspace || workspace_bytes < need) return fail(EVD_E_WORKSPACE, "evd_sparse_blur_backward: workspace %zu < %zu bytes", workspace_bytes, need);
        SbK& k = pl.k;
        k.d_new_rays = d_new_rays;
        k.d_weight = d_weight;
        k.d_align = d_align;
        k.d_img_embed = d_img_embed;
        k.d_feats = d_feats;
        k.dxe = x && d_x ? d_x : L.dxe;
        k.dpp = L.dpp;
        k.dpt = L.dpt;
        k.partial = L.partial;
        k_sparse_blur_bwd<<<pl.blocks, SB_NT, 0, as_stream(stream)>>>(k);
        EVD_LAUNCH_CHECK();
        rk.partial = k.partial;
        rk.dxe = k.dxe;
        rk.dpp = k.dpp;
        rk.dpt = k.dpt;
        rk.n_blocks = pl.blocks;
    }
    if (rk.ten.end > 0) {
        k_sparse_blur_reduce<<<(unsigned)cdiv(rk.ten.end, 256), 256, 0, as_stream(stream)>>>(rk);
        EVD_LAUNCH_CHECK();
    }
    return EVD_OK;
}

}  // extern "C"
