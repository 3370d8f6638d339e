// RigidBlurringModel.forward (networks/dpnerf/blurmodel.py:129-173 with ViewEmbedding.forward, networks/embedding.py:31-32, and
// SE3Field / RigidBody of utils/rigid_warping.py) and its backward.  The reference runs one gather, six small linears and a Python loop
// over the motions of ~40 tensor ops each; autograd doubles that.  Here: one forward launch, two backward launches.
//
// A float32 tile network (mfma_f32_tile.h holds the scheme and everything the family shares): a workgroup takes tiles of 16 rays in
// grid-stride order, the ray is the N dimension of every product, dealt to the wavefronts round robin; operands that depend on the ray
// live in LDS, the parameters are read in place in torch layout.  r / v go through LDS to one lane per (ray, slot) for the SE(3) part
// (rigid_blur_se3.h).  The backward keeps nothing from the forward: it recomputes the hidden layers, then forms, per tile, d heads ->
// d hidden -> d x on the matrix core, and the six weight gradients [W | b] = d Y^T [X | 1] (rb_products) with the family's resident
// accumulators.  k_rigid_blur_reduce sums their partials and forms the table's gradient as the sum, in ray order, of the d x rows of
// each image.
#include <algorithm>
#include <cstddef>

#include "evd_common.h"
#include "mfma_f32_tile.h"
#include "rigid_blur_se3.h"

namespace evd {

constexpr int RB_NT = MT_NT, RB_NW = MT_NW;
constexpr int RB_TR = MT_TR;          // rays of a tile
constexpr int RB_MAXC = 128, RB_MAXW = 64, RB_MAXM = 15;
constexpr int RB_XS = 145;            // x row: C values, the constant one, zeros up to a multiple of 16 (<= 144), odd stride
constexpr int RB_HS = 81;             // hidden row: W values, the constant one, zeros up to 80
constexpr int RB_PS = 65;             // d pre-activation row
constexpr int RB_OS = 49;             // head row (3 M <= 45, padded to 48)
constexpr int RB_WS = 17;             // weight-head row (M + 1 <= 16)
constexpr int RB_MAX_BLOCKS = 64;

struct RbK {
    evd_rigid_blur_params p;
    const float* rays;
    const long* ids;
    const float* x;
    long R;
    int C, Wb[3], M, P, use_origin, n_img;
    float rv_window;
    // forward outputs
    float *new_rays, *weight, *img_embed;
    // backward
    const float *d_new_rays, *d_weight, *d_img_embed;
    float *d_rays, *dx, *partial;
    MtMats mats;                       // the six weight-gradient products
};

struct RbSmem {
    float xs[RB_TR][RB_XS];
    float hs[3][RB_TR][RB_HS];
    float orv[2][RB_TR][RB_OS];
    float ow[RB_TR][RB_WS];
    float dp[3][RB_TR][RB_PS];
    float dray[RB_TR][RB_MAXM + 1][6];
};
#define RB_OFF(field) ((int)(offsetof(RbSmem, field) / sizeof(float)))

// The six weight-gradient products [W | b] = d Y^T [X | 1] (branches, then heads) and the twelve tensors behind pl.ten.end, in the flat
// gradient's order: a bias is the column that the constant one behind X adds to its weight's product
constexpr void rb_products(MtPlan& pl, int C, int W_r, int W_v, int W_w, int M) {
    const int Wb[3] = {W_r, W_v, W_w};
    for (int b = 0; b < 3; ++b) {
        const MtMat m = pl.add_mat(Wb[b], C + 1, RB_OFF(dp) + b * RB_TR * RB_PS, RB_PS, RB_OFF(xs), RB_XS);
        pl.add_tensor(Wb[b], C, m);
        pl.add_tensor(Wb[b], 1, m, C);
    }
    for (int b = 0; b < 3; ++b) {
        const int rows = b == 2 ? M + 1 : 3 * M;
        const MtMat m = pl.add_mat(rows, Wb[b] + 1, b == 2 ? RB_OFF(ow) : RB_OFF(orv) + b * RB_TR * RB_OS, b == 2 ? RB_WS : RB_OS,
                                   RB_OFF(hs) + b * RB_TR * RB_HS, RB_HS);
        pl.add_tensor(rows, Wb[b], m);
        pl.add_tensor(rows, 1, m, Wb[b]);
    }
}
constexpr int rb_max_tiles() {
    MtPlan pl{};
    rb_products(pl, RB_MAXC, RB_MAXW, RB_MAXW, RB_MAXW, RB_MAXM);
    return pl.mats.n_tiles;
}
constexpr int RB_MAX_TILES = rb_max_tiles();                   // weight-gradient tiles at the largest shape
constexpr int RB_TPW = (RB_MAX_TILES + RB_NW - 1) / RB_NW;     // ... of one wavefront

__device__ __forceinline__ const float* rb_branch_w(const RbK& k, int b) { return b == 0 ? k.p.r_branch_w : b == 1 ? k.p.v_branch_w : k.p.w_branch_w; }
__device__ __forceinline__ const float* rb_branch_b(const RbK& k, int b) { return b == 0 ? k.p.r_branch_b : b == 1 ? k.p.v_branch_b : k.p.w_branch_b; }
__device__ __forceinline__ const float* rb_head_w(const RbK& k, int b) { return b == 0 ? k.p.r_linear_w : b == 1 ? k.p.v_linear_w : k.p.w_linear_w; }
__device__ __forceinline__ const float* rb_head_b(const RbK& k, int b) { return b == 0 ? k.p.r_linear_b : b == 1 ? k.p.v_linear_b : k.p.w_linear_b; }
__device__ __forceinline__ int rb_head_rows(const RbK& k, int b) { return b == 2 ? k.M + 1 : 3 * k.M; }

// the feature row of ray `ray` (NULL: the ray is outside the batch, or its image id outside the table)
__device__ __forceinline__ const float* rb_row(const RbK& k, long ray) {
    if (ray >= k.R) return nullptr;
    if (!k.ids) return k.x + ray * k.C;
    const long id = k.ids[ray];
    return id >= 0 && id < k.n_img ? k.p.table + id * k.C : nullptr;
}

// x tile, hidden layers and heads of the 16 rays from ray0 on, left in s.xs / s.hs / s.orv / s.ow
__device__ __forceinline__ void rb_networks(const RbK& k, RbSmem& s, long ray0, bool write_embed) {
    const int tid = threadIdx.x, wv = tid >> 6;
    const int nx = 16 * ((k.C + 1 + 15) / 16);
    for (int i = tid; i < RB_TR * nx; i += RB_NT) {
        const int r = i / nx, c = i % nx;
        const float* row = rb_row(k, ray0 + r);
        const bool valid = ray0 + r < k.R;
        float v = 0.f;
        if (c < k.C) {
            v = row ? row[c] : 0.f;
            if (write_embed && valid) k.img_embed[(ray0 + r) * k.C + c] = v;
        } else if (c == k.C) {
            v = valid ? 1.f : 0.f;
        }
        s.xs[r][c] = v;
    }
    for (int i = tid; i < 3 * RB_TR * 80; i += RB_NT) {            // the constant one behind each hidden row and the zeros behind it
        const int b = i / (RB_TR * 80), r = (i / 80) % RB_TR, c = i % 80;
        if (c >= k.Wb[b]) s.hs[b][r][c] = (c == k.Wb[b] && ray0 + r < k.R) ? 1.f : 0.f;
    }
    __syncthreads();
    for (int job = wv; job < 12; job += RB_NW) {                     // hidden = relu(W x + b): (branch, 16 units) x 16 rays
        const int b = job >> 2, m0 = (job & 3) * 16, Wd = k.Wb[b];
        if (m0 >= Wd) continue;
        const mt_f4 acc = mt_tile(mt_zero(), rb_branch_w(k, b) + (long)m0 * k.C, k.C, 1, Wd - m0, k.C, &s.xs[0][0], RB_XS, 1);
        mt_store_relu(&s.hs[b][0][0], RB_HS, acc, rb_branch_b(k, b), m0, Wd);
    }
    __syncthreads();
    for (int job = wv; job < 7; job += RB_NW) {                      // heads: r, v (3 M rows, x rv_window), weight logits (M + 1 rows)
        const int b = job < 3 ? 0 : job < 6 ? 1 : 2, m0 = (job - 3 * b) * 16, rows = rb_head_rows(k, b), Wd = k.Wb[b];
        if (m0 >= rows) continue;
        const mt_f4 acc = mt_tile(mt_zero(), rb_head_w(k, b) + (long)m0 * Wd, Wd, 1, rows - m0, Wd, &s.hs[b][0][0], RB_HS, 1);
        const float* bias = rb_head_b(k, b);
        mt_each(acc, m0, rows, [&](int m, int n, float v) {
            const float y = v + bias[m];
            if (b == 2) s.ow[n][m] = y;
            else s.orv[b][n][m] = y * k.rv_window;
        });
    }
    __syncthreads();
}

__global__ __launch_bounds__(RB_NT) void k_rigid_blur_fwd(RbK k) {
    __shared__ RbSmem s;
    const int tid = threadIdx.x;
    const long tiles = (k.R + RB_TR - 1) / RB_TR;
    mt_zero_lds(s);
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long ray0 = tile * RB_TR;
        rb_networks(k, s, ray0, true);
        for (int q = tid; q < RB_TR * k.P; q += RB_NT) {             // one lane per (ray, slot)
            const int r = q / k.P, slot = q % k.P, mo = slot - k.use_origin;
            const long ray = ray0 + r;
            if (ray >= k.R) continue;
            float o[3], d[3], yo[3], yd[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { o[c] = k.rays[ray * 6 + c * 2]; d[c] = k.rays[ray * 6 + c * 2 + 1]; yo[c] = o[c]; yd[c] = d[c]; }
            if (mo >= 0) {
                const float rho[3] = {s.orv[0][r][mo], s.orv[0][r][k.M + mo], s.orv[0][r][2 * k.M + mo]};
                const float tau[3] = {s.orv[1][r][mo], s.orv[1][r][k.M + mo], s.orv[1][r][2 * k.M + mo]};
                rb_warp(rho, tau, o, d, yo, yd);
            }
            float* out = k.new_rays + (ray * k.P + slot) * 6;
#pragma unroll
            for (int c = 0; c < 3; ++c) { out[c * 2] = yo[c]; out[c * 2 + 1] = yd[c]; }
        }
        if (tid < RB_TR && ray0 + tid < k.R) {                         // weight = sigmoid / (row sum + 1e-10)
            float sg[RB_MAXM + 1], sum = 0.f;
#pragma unroll
            for (int j = 0; j <= RB_MAXM; ++j)
                if (j <= k.M) { sg[j] = act(EVD_ACT_SIGMOID, s.ow[tid][j]); sum += sg[j]; }
            sum += 1.0e-10f;
#pragma unroll
            for (int j = 0; j <= RB_MAXM; ++j)
                if (j <= k.M) k.weight[(ray0 + tid) * (k.M + 1) + j] = sg[j] / sum;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(RB_NT) void k_rigid_blur_bwd(RbK k) {
    __shared__ RbSmem s;
    const int tid = threadIdx.x, wv = tid >> 6;
    const long tiles = (k.R + RB_TR - 1) / RB_TR;
    mt_f4 wg[RB_TPW];
#pragma unroll
    for (int i = 0; i < RB_TPW; ++i) wg[i] = mt_zero();
    __shared__ int4 jobs[RB_MAX_TILES];
    mt_jobs(jobs, k.mats, 0, RB_MAX_TILES);
    mt_zero_lds(s);
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long ray0 = tile * RB_TR;
        rb_networks(k, s, ray0, false);
        // ---- SE(3) part: d new_rays -> d r, d v (in place of r, v) and the slots' d rays
        for (int q = tid; q < RB_TR * k.P; q += RB_NT) {
            const int r = q / k.P, slot = q % k.P, mo = slot - k.use_origin;
            const long ray = ray0 + r;
            const bool valid = ray < k.R;
            float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f}, go[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f};
            if (valid) {
                const float* g = k.d_new_rays + (ray * k.P + slot) * 6;
#pragma unroll
                for (int c = 0; c < 3; ++c) { o[c] = k.rays[ray * 6 + c * 2]; d[c] = k.rays[ray * 6 + c * 2 + 1]; go[c] = g[c * 2]; gd[c] = g[c * 2 + 1]; }
            }
            float d_o[3] = {go[0], go[1], go[2]}, d_d[3] = {gd[0], gd[1], gd[2]};
            if (mo >= 0) {
                const float rho[3] = {s.orv[0][r][mo], s.orv[0][r][k.M + mo], s.orv[0][r][2 * k.M + mo]};
                const float tau[3] = {s.orv[1][r][mo], s.orv[1][r][k.M + mo], s.orv[1][r][2 * k.M + mo]};
                float drho[3] = {0.f, 0.f, 0.f}, dtau[3] = {0.f, 0.f, 0.f};
                if (valid) rb_warp_bwd(rho, tau, o, d, go, gd, drho, dtau, d_o, d_d);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    s.orv[0][r][c * k.M + mo] = drho[c] * k.rv_window;
                    s.orv[1][r][c * k.M + mo] = dtau[c] * k.rv_window;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) { s.dray[r][slot][c * 2] = d_o[c]; s.dray[r][slot][c * 2 + 1] = d_d[c]; }
        }
        // ---- weight = sigmoid(z) / (sum + 1e-10): d weight -> d z (in place of z)
        if (tid < RB_TR) {
            const bool valid = ray0 + tid < k.R;
            float sg[RB_MAXM + 1], gw[RB_MAXM + 1], sum = 0.f, gs = 0.f;
#pragma unroll
            for (int j = 0; j <= RB_MAXM; ++j)
                if (j <= k.M) {
                    sg[j] = act(EVD_ACT_SIGMOID, s.ow[tid][j]);
                    gw[j] = valid ? k.d_weight[(ray0 + tid) * (k.M + 1) + j] : 0.f;
                    sum += sg[j];
                    gs += gw[j] * sg[j];
                }
            sum += 1.0e-10f;
            const float back = gs / (sum * sum);
#pragma unroll
            for (int j = 0; j <= RB_MAXM; ++j)
                if (j <= k.M) s.ow[tid][j] = valid ? (gw[j] / sum - back) * (sg[j] * (1.f - sg[j])) : 0.f;
        }
        __syncthreads();
        if (k.d_rays) {                                                // a ray's slots summed in slot order
            for (int i = tid; i < RB_TR * 6; i += RB_NT) {
                const int r = i / 6, c = i % 6;
                if (ray0 + r >= k.R) continue;
                float a = 0.f;
                for (int sl = 0; sl < k.P; ++sl) a += s.dray[r][sl][c];
                k.d_rays[(ray0 + r) * 6 + c] = a;
            }
        }
        // ---- d hidden = head^T d out, through the ReLU
        for (int job = wv; job < 12; job += RB_NW) {
            const int b = job >> 2, m0 = (job & 3) * 16, Wd = k.Wb[b], rows = rb_head_rows(k, b);
            if (m0 >= Wd) continue;
            const float* dout = b == 2 ? &s.ow[0][0] : &s.orv[b][0][0];
            const mt_f4 acc = mt_tile(mt_zero(), rb_head_w(k, b) + m0, 1, Wd, Wd - m0, rows, dout, b == 2 ? RB_WS : RB_OS, 1);
            mt_gate_relu(&s.dp[b][0][0], RB_PS, &s.hs[b][0][0], RB_HS, acc, m0, Wd);
        }
        __syncthreads();
        // ---- d x = sum over the branches of W^T d pre (+ the gradient that arrives at img_embed)
        if (k.dx) {
            for (int job = wv; job < (k.C + 15) / 16; job += RB_NW) {
                const int m0 = job * 16;
                mt_f4 acc = mt_zero();
#pragma unroll
                for (int b = 0; b < 3; ++b) acc = mt_tile(acc, rb_branch_w(k, b) + m0, 1, k.C, k.C - m0, k.Wb[b], &s.dp[b][0][0], RB_PS, 1);
                mt_each(acc, m0, k.C, [&](int m, int n, float v) {
                    const long ray = ray0 + n;
                    if (ray < k.R) k.dx[ray * k.C + m] = v + (k.d_img_embed ? k.d_img_embed[ray * k.C + m] : 0.f);
                });
            }
        }
        // ---- weight gradients: d Y^T [X | 1] over the tile's rays, both operands in LDS
        mt_accumulate<RB_TPW, true>(wg, jobs, reinterpret_cast<const float*>(&s), k.mats.n_tiles, 0);
        __syncthreads();
    }
    mt_store_partials(wg, k.partial, k.mats.n_tiles, 0);
}

struct RbReduce {
    const float *partial, *dx;
    const long* ids;
    float* grads;
    long R, table_floats;
    int C, n_blocks;
    MtTensors ten;                      // the twelve network tensors behind the table
};

// One thread per gradient element.  Table: the d x rows of the image's rays in ray order (an image without rays gets zeros).  The
// twelve network tensors: the workgroups' partial tiles in workgroup order.
__global__ __launch_bounds__(256) void k_rigid_blur_reduce(RbReduce k) {
    const long e = blockIdx.x * 256L + threadIdx.x;
    if (e >= k.ten.end) return;
    if (e < k.table_floats)                          // (per-ray form: the table takes no part, its slot is zeros)
        k.grads[e] = k.ids ? mt_rows_of_image_sum(k.ids, k.R, e / k.C, k.dx, k.C, (int)(e % k.C)) : 0.f;
    else
        k.grads[e] = mt_reduce_sum(k.ten, k.partial, k.n_blocks, e);
}

struct RbPlan {
    RbK k;
    RbReduce r;
    int blocks;
};

static int rb_blocks(long R) { return (int)std::min<long>(cdiv(R, RB_TR), RB_MAX_BLOCKS); }

// workspace of evd_rigid_blur_backward: the d x rows (table form) | the workgroups' partial weight-gradient tiles
struct RbWs { float *dx, *partial; };
static size_t rb_layout(const RbPlan& pl, long R, void* workspace, RbWs* L) {
    FloatSlots ws(workspace);
    L->dx = ws.take((size_t)R * pl.k.C);
    L->partial = ws.take(mt_partial_floats(rb_blocks(R), pl.k.mats.n_tiles));
    return ws.bytes();
}

static int rb_plan(const char* who, const evd_rigid_blur_desc* d, const evd_rigid_blur_params* p, const float* rays, const long* ids, const float* x,
                   long R, RbPlan* out) {
    EVD_REQUIRE(d, "%s: null descriptor", who);
    EVD_REQUIRE(d->D_r == 1 && d->D_v == 1 && d->D_w == 1, "%s: branch depths (%d, %d, %d): only depth 1 is built (the reference feeds every branch layer the "
                "branch input, blurmodel.py:148-158)", who, d->D_r, d->D_v, d->D_w);
    EVD_REQUIRE(d->W_r >= 1 && d->W_r <= RB_MAXW && d->W_v >= 1 && d->W_v <= RB_MAXW && d->W_w >= 1 && d->W_w <= RB_MAXW,
                "%s: hidden widths (%d, %d, %d) outside 1..%d", who, d->W_r, d->W_v, d->W_w, RB_MAXW);
    EVD_REQUIRE(d->C >= 1 && d->C <= RB_MAXC, "%s: feature width %d outside 1..%d", who, d->C, RB_MAXC);
    EVD_REQUIRE(d->M >= 1 && d->M <= RB_MAXM, "%s: num_motion %d outside 1..%d", who, d->M, RB_MAXM);
    EVD_REQUIRE(R >= 0 && d->n_img >= 0, "%s: negative size", who);
    RbK& k = out->k;
    memset(out, 0, sizeof(*out));
    k.C = d->C;
    k.Wb[0] = d->W_r; k.Wb[1] = d->W_v; k.Wb[2] = d->W_w;
    k.M = d->M;
    k.use_origin = d->use_origin ? 1 : 0;
    k.P = k.M + k.use_origin;
    k.n_img = d->n_img;
    k.rv_window = d->rv_window;
    k.R = R;
    MtPlan mp{};
    mp.ten.end = (long)k.n_img * k.C;                                  // the table's gradient comes first
    rb_products(mp, k.C, k.Wb[0], k.Wb[1], k.Wb[2], k.M);
    const int rc = mt_check(who, mp, RB_MAX_TILES);
    if (rc != EVD_OK) return rc;
    k.mats = mp.mats;
    out->r.ten = mp.ten;
    out->r.table_floats = (long)k.n_img * k.C;
    out->r.C = k.C;
    out->r.R = R;
    out->blocks = rb_blocks(R);
    if (R == 0) return EVD_OK;
    EVD_REQUIRE(p && rays, "%s: null parameters / rays", who);
    EVD_REQUIRE(ids ? (p->table != nullptr && d->n_img >= 1) : x != nullptr, "%s: needs ids and the table, or per-ray feature rows", who);
    EVD_REQUIRE(p->r_branch_w && p->r_branch_b && p->v_branch_w && p->v_branch_b && p->w_branch_w && p->w_branch_b && p->r_linear_w && p->r_linear_b &&
                p->v_linear_w && p->v_linear_b && p->w_linear_w && p->w_linear_b, "%s: null parameter tensor", who);
    k.p = *p;
    k.rays = rays;
    k.ids = ids;
    k.x = x;
    return EVD_OK;
}

}  // namespace evd

using namespace evd;

extern "C" {

size_t evd_rigid_blur_workspace_bytes(const evd_rigid_blur_desc* d, long R) {
    RbPlan pl;
    if (rb_plan("evd_rigid_blur_workspace_bytes", d, nullptr, nullptr, nullptr, nullptr, R < 0 ? -1 : 0, &pl) != EVD_OK) return 0;
    RbWs L;
    return rb_layout(pl, R, nullptr, &L);
}

int evd_rigid_blur_forward(const evd_rigid_blur_desc* d, const evd_rigid_blur_params* p, const float* rays, const long* ids, const float* x, long R,
                           float* new_rays, float* weight, float* img_embed, void* stream) {
    RbPlan pl;
    int rc = rb_plan("evd_rigid_blur_forward", d, p, rays, ids, x, R, &pl);
    if (rc != EVD_OK) return rc;
    if (R == 0) return EVD_OK;
    EVD_REQUIRE(new_rays && weight && img_embed, "evd_rigid_blur_forward: null output");
    pl.k.new_rays = new_rays;
    pl.k.weight = weight;
    pl.k.img_embed = img_embed;
    k_rigid_blur_fwd<<<pl.blocks, RB_NT, 0, as_stream(stream)>>>(pl.k);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_rigid_blur_backward(const evd_rigid_blur_desc* d, const evd_rigid_blur_params* p, const float* rays, const long* ids, const float* x, long R,
                            const float* d_new_rays, const float* d_weight, const float* d_img_embed, float* grads, float* d_rays, float* d_x,
                            void* workspace, size_t workspace_bytes, void* stream) {
    RbPlan pl;
    int rc = rb_plan("evd_rigid_blur_backward", d, p, rays, ids, x, R, &pl);
    if (rc != EVD_OK) return rc;
    EVD_REQUIRE(grads, "evd_rigid_blur_backward: null gradient buffer");
    RbReduce& rk = pl.r;
    rk.grads = grads;
    rk.ids = ids;
    if (R > 0) {
        EVD_REQUIRE(d_new_rays && d_weight, "evd_rigid_blur_backward: null d new_rays / d weight");
        RbWs L;
        const size_t need = rb_layout(pl, R, workspace, &L);
        if (!workspace || workspace_bytes < need) return fail(EVD_E_WORKSPACE, "evd_rigid_blur_backward: workspace %zu < %zu bytes", workspace_bytes, need);
        pl.k.d_new_rays = d_new_rays;
        pl.k.d_weight = d_weight;
        pl.k.d_img_embed = d_img_embed;
        pl.k.d_rays = d_rays;
        pl.k.dx = ids ? L.dx : d_x;
        pl.k.partial = L.partial;
        k_rigid_blur_bwd<<<pl.blocks, RB_NT, 0, as_stream(stream)>>>(pl.k);
        EVD_LAUNCH_CHECK();
        rk.partial = L.partial;
        rk.dx = L.dx;
        rk.n_blocks = pl.blocks;
    }
    if (rk.ten.end > 0) {
        k_rigid_blur_reduce<<<(unsigned)cdiv(rk.ten.end, 256), 256, 0, as_stream(stream)>>>(rk);
        EVD_LAUNCH_CHECK();
    }
    return EVD_OK;
}

}  // extern "C"
