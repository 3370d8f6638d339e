// ViewEmbeddingMLP (networks/embedding.py:35-62) evaluated once per IMAGE: img_embed [n_img, E] -> D layers of relu(W h + b), the
// embedding row concatenated in FRONT of a skip layer's output (:59-60) -> feature table [n_img, W], and its backward.  The reference runs
// the module per ray (a gather, D addmm + relu + cat and their autograd on R rows); its input is a function of the image id only, so the
// blur kernel entries take the table this file produces as their `table` and gather from it themselves.
//
// A float32 tile network (mfma_f32_tile.h holds the scheme and everything the family shares): a workgroup takes tiles of 16 images, the
// image is the N dimension of every product, dealt to the wavefronts round robin; the embedding rows and the hidden rows live in LDS
// behind a constant one and zeros up to the tile, the parameters are read in place in torch layout.  A skip layer's input is never
// assembled: its product is the sum of the embedding columns' and the hidden columns' products.  The backward keeps nothing from the
// forward: it recomputes the hidden rows, runs d pre-activation down the layers (the embedding columns of layer 0 and of every skip layer
// add into one d img_embed accumulator in registers), and forms the weight gradients (ve_products; a bias is the column the constant
// one adds) with the family's resident accumulators.  A workgroup holds at most VE_CHUNK such tiles; a wider network spreads them over
// blockIdx.y, each of which recomputes the rows.  k_view_embed_reduce sums the partials.
#include <algorithm>

#include "evd_common.h"
#include "mfma_f32_tile.h"

namespace evd {

constexpr int VE_NT = MT_NT, VE_NW = MT_NW;
constexpr int VE_TR = MT_TR;          // images of a tile
constexpr int VE_MAXN = 4096, VE_MAXE = 128, VE_MAXW = 128, VE_MAXD = 8;
constexpr int VE_CHUNK = 64;          // weight-gradient tiles of one workgroup
constexpr int VE_TPW = VE_CHUNK / VE_NW;                         // ... of one wavefront
constexpr int VE_EJ = VE_MAXE / 16 / VE_NW;                      // d img_embed tiles of one wavefront
constexpr int VE_MAX_BLOCKS = 32;     // workgroups that share the image tiles
constexpr int VE_MAX_LDS = 4 * VE_TR * (VE_MAXD * (VE_MAXE + 17) + VE_MAXD * (VE_MAXW + 1)) + 16 * VE_CHUNK;

struct VeK {
    evd_view_embed_mlp_params p;
    int n_img, E, W, D;
    unsigned skip;                     // bit i: layer i + 1 reads [embedding row | output of layer i]
    int ES, HS, PS;                    // LDS row strides: embedding row, hidden row, d pre-activation row (odd)
    float* out;                        // forward: feature table
    const float* d_out;                // backward
    float *d_table, *partial;
    MtMats mats;                       // the weight-gradient products
};

__host__ __device__ inline int ve_pad16(int n) { return (n + 15) & ~15; }
// layer i reads the embedding columns in front of its hidden columns
__host__ __device__ constexpr bool ve_skip_in(unsigned skip, int i) { return i > 0 && ((skip >> (i - 1)) & 1u); }
__host__ __device__ inline int ve_in_width(int E, int W, unsigned skip, int i) { return i == 0 ? E : ve_skip_in(skip, i) ? E + W : W; }

__device__ __forceinline__ const float* ve_pick(const float* const (&a)[VE_MAXD], int i) {
    const float* r = a[0];
#pragma unroll
    for (int j = 1; j < VE_MAXD; ++j) r = i == j ? a[j] : r;
    return r;
}
// LDS, as float offsets: the embedding rows at 0, the outputs of layers 0 .. D - 2, the d pre-activations of layers 0 .. D - 1
__host__ __device__ constexpr int ve_hs_off(const VeK& k, int i) { return VE_TR * k.ES + i * VE_TR * k.HS; }
__host__ __device__ constexpr int ve_dp_off(const VeK& k, int i) { return ve_hs_off(k, k.D - 1) + i * VE_TR * k.PS; }
__device__ __forceinline__ float* ve_es(const VeK& k, float* s) { return s; }
__device__ __forceinline__ float* ve_hs(const VeK& k, float* s, int i) { return s + ve_hs_off(k, i); }
__device__ __forceinline__ float* ve_dp(const VeK& k, float* s, int i) { return s + ve_dp_off(k, i); }

// The weight-gradient products of the layers and their tensors w[0], b[0], ... in the flat gradient's order.  Layer 0: d pre^T [embedding
// row | 1].  Layer i > 0: d pre^T [hidden row | 1], behind the product with the embedding row where the layer reads it; its weight's
// columns come from both, its bias is the column of the constant one.
constexpr void ve_products(MtPlan& pl, const VeK& k) {
    for (int i = 0; i < k.D; ++i) {
        const int dy = ve_dp_off(k, i);
        if (i == 0) {
            const MtMat e = pl.add_mat(k.W, k.E + 1, dy, k.PS, 0, k.ES);
            pl.add_tensor(k.W, k.E, e);
            pl.add_tensor(k.W, 1, e, k.E);
        } else if (ve_skip_in(k.skip, i)) {
            const MtMat e = pl.add_mat(k.W, k.E, dy, k.PS, 0, k.ES), h = pl.add_mat(k.W, k.W + 1, dy, k.PS, ve_hs_off(k, i - 1), k.HS);
            pl.add_tensor(k.W, k.E + k.W, e, 0, k.E, h);
            pl.add_tensor(k.W, 1, h, k.W);
        } else {
            const MtMat h = pl.add_mat(k.W, k.W + 1, dy, k.PS, ve_hs_off(k, i - 1), k.HS);
            pl.add_tensor(k.W, k.W, h);
            pl.add_tensor(k.W, 1, h, k.W);
        }
    }
}
constexpr int ve_max_tiles() {
    VeK k{};
    k.E = VE_MAXE; k.W = VE_MAXW; k.D = VE_MAXD; k.skip = (1u << (VE_MAXD - 1)) - 1u;
    MtPlan pl{};
    ve_products(pl, k);
    return pl.mats.n_tiles;
}
constexpr int VE_MAX_TILES = ve_max_tiles();                     // weight-gradient tiles at the largest shape, over all blockIdx.y
static_assert(VE_CHUNK % VE_NW == 0, "a chunk is dealt evenly to the wavefronts");

// W_i h of units m0 .. m0 + 15 of layer i for the tile's 16 images (the bias is added by the caller)
__device__ __forceinline__ mt_f4 ve_pre(const VeK& k, float* s, int i, int m0) {
    const int kin = ve_in_width(k.E, k.W, k.skip, i);
    const float* w = ve_pick(k.p.w, i) + (long)m0 * kin;
    mt_f4 acc = mt_zero();
    if (i == 0 || ve_skip_in(k.skip, i)) acc = mt_tile(acc, w, kin, 1, k.W - m0, k.E, ve_es(k, s), k.ES, 1);
    if (i > 0) acc = mt_tile(acc, w + (kin - k.W), kin, 1, k.W - m0, k.W, ve_hs(k, s, i - 1), k.HS, 1);
    return acc;
}

// embedding rows of the 16 images from img0 on and the outputs of layers 0 .. D - 2, left in LDS
__device__ __forceinline__ void ve_hidden(const VeK& k, float* s, int img0) {
    const int tid = threadIdx.x, wv = tid >> 6;
    const int ne = k.ES - 1;
    float* es = ve_es(k, s);
    for (int i = tid; i < VE_TR * ne; i += VE_NT) {
        const int r = i / ne, c = i % ne;
        float v = 0.f;
        if (img0 + r < k.n_img) v = c < k.E ? k.p.table[(long)(img0 + r) * k.E + c] : c == k.E ? 1.f : 0.f;
        es[r * k.ES + c] = v;
    }
    for (int i = tid; i < (k.D - 1) * VE_TR; i += VE_NT)               // the constant one behind each hidden row (zeros follow it)
        ve_hs(k, s, i / VE_TR)[(i % VE_TR) * k.HS + k.W] = img0 + i % VE_TR < k.n_img ? 1.f : 0.f;
    __syncthreads();
    for (int l = 0; l + 1 < k.D; ++l) {
        const float* bias = ve_pick(k.p.b, l);
        float* h = ve_hs(k, s, l);
        for (int m0 = 16 * wv; m0 < k.W; m0 += 16 * VE_NW) mt_store_relu(h, k.HS, ve_pre(k, s, l, m0), bias, m0, k.W);
        __syncthreads();
    }
}

extern __shared__ float ve_smem[];

__global__ __launch_bounds__(VE_NT) void k_view_embed_fwd(VeK k) {
    float* s = ve_smem;
    const int wv = threadIdx.x >> 6, L = k.D - 1;
    const int tiles = (k.n_img + VE_TR - 1) / VE_TR;
    mt_zero_lds(s, VE_TR * (k.ES + L * k.HS));
    const float* bias = ve_pick(k.p.b, L);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int img0 = tile * VE_TR;
        ve_hidden(k, s, img0);
        for (int m0 = 16 * wv; m0 < k.W; m0 += 16 * VE_NW) {
            mt_each(ve_pre(k, s, L, m0), m0, k.W, [&](int m, int n, float v) {
                const int img = img0 + n;
                if (img < k.n_img) k.out[(long)img * k.W + m] = act(EVD_ACT_RELU, v + bias[m]);
            });
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(VE_NT) void k_view_embed_bwd(VeK k) {
    float* s = ve_smem;
    const int wv = threadIdx.x >> 6, L = k.D - 1;
    const int tiles = (k.n_img + VE_TR - 1) / VE_TR;
    const int floats = VE_TR * (k.ES + L * k.HS + k.D * k.PS);
    const int chunk0 = blockIdx.y * VE_CHUNK;
    mt_f4 wg[VE_TPW];
#pragma unroll
    for (int i = 0; i < VE_TPW; ++i) wg[i] = mt_zero();
    int4* jobs = reinterpret_cast<int4*>(s + floats);
    mt_jobs(jobs, k.mats, chunk0, VE_CHUNK);
    mt_zero_lds(s, floats);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int img0 = tile * VE_TR;
        ve_hidden(k, s, img0);
        // ---- the last layer's output decides where d feature_table passes
        {
            const float* bias = ve_pick(k.p.b, L);
            float* dp = ve_dp(k, s, L);
            for (int m0 = 16 * wv; m0 < k.W; m0 += 16 * VE_NW) {
                mt_each(ve_pre(k, s, L, m0), m0, k.W, [&](int m, int n, float v) {
                    const int img = img0 + n;
                    dp[n * k.PS + m] = (img < k.n_img && v + bias[m] > 0.f) ? k.d_out[(long)img * k.W + m] : 0.f;
                });
            }
        }
        __syncthreads();
        // ---- d input = W^T d pre: the hidden columns through the ReLU below, the embedding columns into d img_embed
        mt_f4 de[VE_EJ];
#pragma unroll
        for (int q = 0; q < VE_EJ; ++q) de[q] = mt_zero();
        for (int i = L; i >= 0; --i) {
            const int kin = ve_in_width(k.E, k.W, k.skip, i);
            const float* w = ve_pick(k.p.w, i);
            const float* dp = ve_dp(k, s, i);
            if (i == 0 || ve_skip_in(k.skip, i)) {
#pragma unroll
                for (int q = 0; q < VE_EJ; ++q) {
                    const int m0 = 16 * (wv + VE_NW * q);
                    if (m0 < k.E) de[q] = mt_tile(de[q], w + m0, 1, kin, k.E - m0, k.W, dp, k.PS, 1);
                }
            }
            if (i > 0) {
                const float* h = ve_hs(k, s, i - 1);
                float* dlow = ve_dp(k, s, i - 1);
                for (int m0 = 16 * wv; m0 < k.W; m0 += 16 * VE_NW) {
                    const mt_f4 acc = mt_tile(mt_zero(), w + (kin - k.W) + m0, 1, kin, k.W - m0, k.W, dp, k.PS, 1);
                    mt_gate_relu(dlow, k.PS, h, k.HS, acc, m0, k.W);
                }
                __syncthreads();
            }
        }
        if (blockIdx.y == 0) {
#pragma unroll
            for (int q = 0; q < VE_EJ; ++q)
                mt_each(de[q], 16 * (wv + VE_NW * q), k.E, [&](int m, int n, float v) {
                    if (img0 + n < k.n_img) k.d_table[(long)(img0 + n) * k.E + m] = v;
                });
        }
        // ---- weight gradients: d pre^T [input | 1] over the tile's images, both operands in LDS
        mt_accumulate<VE_TPW, false>(wg, jobs, s, k.mats.n_tiles, chunk0);
        __syncthreads();
    }
    mt_store_partials(wg, k.partial, k.mats.n_tiles, chunk0);
}

struct VeReduce {
    const float* partial;
    float* grads;                       // behind the table's gradient
    int n_blocks;
    MtTensors ten;                      // w[0], b[0], ... in it
};

// One thread per element of the weight and bias gradients: the workgroups' partial tiles in workgroup order.
__global__ __launch_bounds__(256) void k_view_embed_reduce(VeReduce k) {
    const long e = blockIdx.x * 256L + threadIdx.x;
    if (e < k.ten.end) k.grads[e] = mt_reduce_sum(k.ten, k.partial, k.n_blocks, e);
}

struct VePlan {
    VeK k;
    VeReduce r;
    int blocks, chunks;
    size_t lds_fwd, lds_bwd;
};

static int ve_plan(const char* who, const evd_view_embed_mlp_desc* d, VePlan* out) {
    EVD_REQUIRE(d, "%s: null descriptor", who);
    EVD_REQUIRE(d->D >= 1 && d->D <= VE_MAXD, "%s: D %d outside 1..%d", who, d->D, VE_MAXD);
    EVD_REQUIRE(d->W >= 1 && d->W <= VE_MAXW, "%s: W %d outside 1..%d", who, d->W, VE_MAXW);
    EVD_REQUIRE(d->embed_dim >= 1 && d->embed_dim <= VE_MAXE, "%s: embed_dim %d outside 1..%d", who, d->embed_dim, VE_MAXE);
    EVD_REQUIRE(d->n_img >= 1 && d->n_img <= VE_MAXN, "%s: n_img %d outside 1..%d", who, d->n_img, VE_MAXN);
    EVD_REQUIRE(!((d->skip_mask >> (d->D - 1)) & 1u), "%s: skip_mask names the last layer %d: its output would be embed_dim + W wide, not the W "
                "that out_channels promises (networks/embedding.py:44,59-60)", who, d->D - 1);
    VeK& k = out->k;
    memset(out, 0, sizeof(*out));
    k.n_img = d->n_img;
    k.E = d->embed_dim;
    k.W = d->W;
    k.D = d->D;
    k.skip = d->skip_mask & ((1u << (d->D - 1)) - 1u);                 // an index >= D never fires
    k.ES = ve_pad16(k.E + 1) + 1;
    k.HS = ve_pad16(k.W + 1) + 1;
    k.PS = ve_pad16(k.W) + 1;
    MtPlan mp{};
    ve_products(mp, k);
    const int rc = mt_check(who, mp, VE_MAX_TILES);
    if (rc != EVD_OK) return rc;
    k.mats = mp.mats;
    out->r.ten = mp.ten;
    out->blocks = (int)std::min<long>(cdiv(k.n_img, VE_TR), VE_MAX_BLOCKS);
    out->chunks = (int)cdiv(k.mats.n_tiles, VE_CHUNK);
    out->lds_fwd = sizeof(float) * VE_TR * (k.ES + (k.D - 1) * k.HS);
    out->lds_bwd = out->lds_fwd + sizeof(float) * VE_TR * k.D * k.PS + sizeof(int4) * VE_CHUNK;
    return EVD_OK;
}

static int ve_params(const char* who, const VePlan& pl, const evd_view_embed_mlp_params* p) {
    EVD_REQUIRE(p && p->table, "%s: null params / table", who);
    for (int i = 0; i < pl.k.D; ++i) EVD_REQUIRE(p->w[i] && p->b[i], "%s: null params w[%d] / b[%d]", who, i, i);
    return EVD_OK;
}

// workspace of evd_view_embed_mlp_backward: the workgroups' partial weight-gradient tiles
struct VeWs { float* partial; };
static const size_t VE_WS_SLACK = 256;     // alignment slack for an unaligned caller pointer
static size_t ve_layout(const VePlan& pl, void* workspace, VeWs* L) {
    Workspace ws(workspace);
    L->partial = ws.take<float>(mt_partial_floats(pl.blocks, pl.k.mats.n_tiles));
    return ws.used() + VE_WS_SLACK;
}

}  // namespace evd

using namespace evd;

extern "C" {

size_t evd_view_embed_mlp_workspace_bytes(const evd_view_embed_mlp_desc* d) {
    VePlan pl;
    VeWs L;
    if (ve_plan("evd_view_embed_mlp_workspace_bytes", d, &pl) != EVD_OK) return 0;
    return ve_layout(pl, nullptr, &L);
}

int evd_view_embed_mlp_forward(const evd_view_embed_mlp_desc* d, const evd_view_embed_mlp_params* p, float* feature_table, void* stream) {
    const char* who = "evd_view_embed_mlp_forward";
    VePlan pl;
    int rc = ve_plan(who, d, &pl);
    if (rc != EVD_OK) return rc;
    if ((rc = ve_params(who, pl, p)) != EVD_OK) return rc;
    EVD_REQUIRE(feature_table, "%s: null feature_table", who);
    pl.k.p = *p;
    pl.k.out = feature_table;
    EVD_SET_MAX_LDS(k_view_embed_fwd, VE_MAX_LDS);
    k_view_embed_fwd<<<pl.blocks, VE_NT, pl.lds_fwd, as_stream(stream)>>>(pl.k);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_view_embed_mlp_backward(const evd_view_embed_mlp_desc* d, const evd_view_embed_mlp_params* p, const float* d_feature_table, float* grads,
                                void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "evd_view_embed_mlp_backward";
    VePlan pl;
    int rc = ve_plan(who, d, &pl);
    if (rc != EVD_OK) return rc;
    if ((rc = ve_params(who, pl, p)) != EVD_OK) return rc;
    EVD_REQUIRE(d_feature_table && grads, "%s: null d_feature_table / grads", who);
    VeWs L;
    const size_t need = ve_layout(pl, workspace, &L);
    if (!workspace || workspace_bytes < need) return fail(EVD_E_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    const long table_floats = (long)pl.k.n_img * pl.k.E;
    pl.k.p = *p;
    pl.k.d_out = d_feature_table;
    pl.k.d_table = grads;
    pl.k.partial = L.partial;
    EVD_SET_MAX_LDS(k_view_embed_bwd, VE_MAX_LDS);
    k_view_embed_bwd<<<dim3(pl.blocks, pl.chunks), VE_NT, pl.lds_bwd, as_stream(stream)>>>(pl.k);
    EVD_LAUNCH_CHECK();
    VeReduce& rk = pl.r;
    rk.partial = L.partial;
    rk.grads = grads + table_floats;
    rk.n_blocks = pl.blocks;
    k_view_embed_reduce<<<(unsigned)cdiv(rk.ten.end, 256), 256, 0, as_stream(stream)>>>(rk);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // extern "C"
