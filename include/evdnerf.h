/*
 * evdnerf.h -- C ABI of libevdnerf.so: the MI355X (gfx950) renderer + blur/event-loss hot path of
 * EvDeblurNeRF, written as HIP kernels.  This is the drop-in boundary: the reference has no FFI
 * layer (it is pure PyTorch), so every entry point below replaces one Python function of the reference
 * (cited as file:line, paths relative to the reference checkout) and the Python mirror in
 * evdeblurnerf_amd/ binds them with ctypes (INTEGRATION.md shows the stub a maintainer would add).
 *
 * Conventions
 *   - every pointer marked "dev" is device memory (HBM) owned by the caller; tensors are float32,
 *     contiguous, row-major; "host" pointers are plain host memory read during the call only.
 *   - every entry returns 0 (EVD_OK) or a negative EVD_E* code; evd_last_error() gives the message
 *     of the last failure on the calling thread.
 *   - kernels are enqueued on the caller's HIP stream (void* = hipStream_t); no entry synchronises,
 *     allocates in the hot path, or keeps mutable state outside the handles it is given (the only process-wide data are
 *     write-once caches of device attributes).  Scratch memory comes from the caller
 *     (evd_*_workspace_bytes).  Opaque handles own only their packed parameters.
 *   - NULL output pointers mean "not wanted".
 */
#ifndef EVDNERF_H
#define EVDNERF_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EVD_OK 0
#define EVD_E_INVALID (-1)      /* bad argument / unsupported configuration */
#define EVD_E_HIP (-2)          /* a HIP runtime call failed */
#define EVD_E_WORKSPACE (-3)    /* workspace too small */
#define EVD_E_NODEVICE (-4)     /* no gfx950 device */

#define EVD_MAX_LAYERS 16

/* arithmetic of the per-sample MLP GEMMs (accumulation is always float32) */
#define EVD_PREC_F32 0      /* v_mfma_f32_32x32x2_f32: exact float32 products (bitwise an fmaf chain) */
#define EVD_PREC_F16X3 1    /* operands split hi+lo into two float16, 3 x v_mfma_f32_32x32x16_f16: ~2^-21 products */
#define EVD_PREC_BF16 2     /* v_mfma_f32_32x32x16_bf16: throughput mode, ~2^-8 operands */
#define EVD_PREC_F16 3      /* v_mfma_f32_32x32x16_f16, one product: bf16 speed, ~2^-11 operands, float16 range */
#define EVD_PREC_F16C 4     /* compensated float16: the float16 product + two block-scaled fp6 (e2m3) products of the operands' rounding
                             * residuals on v_mfma_scale_f32_32x32x64_f8f6f4: ~2^-15 operands at 1.4x the matrix-pipe time of EVD_PREC_F16.
                             * Built for the netdepth 8, netwidth 256, skips [4] NeRF network without feature rows; EVD_E_INVALID otherwise. */
#define EVD_NUM_PREC 5      /* arithmetic modes with weight streams of their own */
/* TRAINING entries only (evd_*_mlp_train / _backward / _train_store_bytes_prec, evd_voxel_sample_prec), round 4.  The reference trains in
 * float32 (run_nerf.py:593-601); both mixed modes below keep the single-product float16 mode's activation store and run ITS backward
 * (loss-scaled float16 operands, float32 accumulation), behind a forward that holds the float32 numbers:
 *   EVD_PREC_F16C (above) as a training mode: the compensated forward where a level / network has that kernel (PDRF fine level, 8 x 256
 *     NeRF), the split-float16 forward elsewhere (PDRF coarse level).  Forward ~2^-15; ReLU patterns differ from float32 in ~5e-6 of the
 *     units, which bounds the gradients at ~sqrt(5e-6) = a few 1e-3 of their norm whatever the batch size.
 *   EVD_PREC_F16M: the split-float16 (EVD_PREC_F16X3) forward everywhere: forward ~2^-21, float32's own ReLU patterns; gradients within
 *     the float16 backward's rounding (~1e-3).  Inference entries reject it (render in EVD_PREC_F16X3). */
#define EVD_PREC_F16M 5

/* activation codes: reference networks/nerf.py:31-33, networks/pdrf/voxnerf.py:28-30 */
#define EVD_ACT_NONE 0
#define EVD_ACT_RELU 1
#define EVD_ACT_SIGMOID 2
#define EVD_ACT_EXP 3
#define EVD_ACT_SIGMOID1 4
#define EVD_ACT_SOFTPLUS 5
#define EVD_ACT_TANH 6

const char* evd_last_error(void);
int evd_version(void);
/* test support (tests/test_gpu_dist.py; no reference counterpart): the number of delay kernels the side-stream test hook launched in this
 * process (EVD_TEST_SIDE_SPIN_US=N in the environment puts an N-microsecond spin in front of every backward launch on a handle's side
 * stream; 0 when the variable is unset -- the hook is then one branch per backward entry) */
long evd_debug_side_spin_count(void);
/* number of gfx950 devices visible; <0 on error */
int evd_device_count(void);

/* ---------------------------------------------------------------- rays (reference utils/rays.py) */
/* get_rays, utils/rays.py:8-22.  K host[9], c2w host[12] -> rays_o/rays_d dev [H,W,3].  add_halfpix: the reference's keyword
 * (:8-9; HALF_PIX = 0.5 added to the pixel index when non-zero). */
int evd_get_rays(int H, int W, const float* K, const float* c2w, int add_halfpix, float* rays_o, float* rays_d, void* stream);
/* get_rays_pix, utils/rays.py:25-36.  coords dev [n,2], c2ws dev [n,3,4], K host[9].  add_halfpix 0: the coordinates are already
 * sub-pixel positions (rectified event coordinates, data/loader_events.py:290-293 passes integer_coords).  n == 0 is a no-op; with
 * n > 0 a NULL coords or c2ws is refused (-1). */
int evd_get_rays_pix(const float* coords, const float* K, const float* c2ws, long n, int add_halfpix,
                     float* rays_o, float* rays_d, void* stream);
/* get_ndc_rays, utils/rays.py:104-145.  n == 0 is a no-op; with n > 0 a NULL rays_o or rays_d is refused (-1). */
int evd_ndc_rays(int H, int W, float focal, float near, const float* rays_o, const float* rays_d, long n,
                 float* out_o, float* out_d, void* stream);
/* RigidBlurringModel.rbk_warp, networks/dpnerf/blurmodel.py:51-82 (SE3Field / RigidBody of utils/rigid_warping.py): the
 * sub-exposure rays of the blur batch.  rays dev [R,3,2]; r, v dev [R,3,M] (the r_linear / v_linear outputs viewed as
 * [R,3,M], blurmodel.py:52-53) -> new_rays dev [R, M + use_origin, 3, 2] (slot 0 = the input ray when use_origin),
 * transforms dev [R, M + use_origin, 4, 4] or NULL. */
int evd_rbk_warp(const float* rays, const float* r, const float* v, long R, int M, int use_origin, float* new_rays, float* transforms,
                 void* stream);
/* RigidBlurringModel.forward, networks/dpnerf/blurmodel.py:129-173, with ViewEmbedding.forward (networks/embedding.py:31-32) in front and
 * rbk_warp (:51-82, utils/rigid_warping.py:18-49,72-110) behind it: the whole blur kernel network of a training iteration (the call site
 * is networks/renderer.py:303-304, the module is built at run_nerf.py:204-215).  The parameters are the reference module's own tensors,
 * float32 in torch layout ([out, in] weights), read in place: nothing is packed and no handle is kept.
 *   C = width of a ray's feature row; W_r, W_v, W_w = hidden widths of the three branches (1..64); D_* = branch depths, 1 only (the
 *   reference's loop feeds every branch layer the branch INPUT, :148-158, so a deeper branch is ill-formed or equal to its last layer);
 *   M = num_motion (1..15); n_img = rows of the embedding table (0 without one); C <= 128.  Anything else: EVD_E_INVALID. */
typedef struct {
    int C, W_r, W_v, W_w, D_r, D_v, D_w, M, use_origin, n_img;
    float rv_window;
} evd_rigid_blur_desc;
typedef struct {
    const float* table;                                                           /* view_embed_module.img_embed dev [n_img, C], or NULL */
    const float *r_branch_w, *r_branch_b, *v_branch_w, *v_branch_b, *w_branch_w, *w_branch_b;    /* *_branch.0: dev [W_*, C], [W_*] */
    const float *r_linear_w, *r_linear_b, *v_linear_w, *v_linear_b;               /* dev [3 M, W_r / W_v], [3 M] */
    const float *w_linear_w, *w_linear_b;                                         /* dev [M + 1, W_w], [M + 1] */
} evd_rigid_blur_params;
/* bytes of the backward's workspace for R rays (0 for an unsupported descriptor) */
size_t evd_rigid_blur_workspace_bytes(const evd_rigid_blur_desc* d, long R);
/* One launch.  rays dev [R,3,2]; a ray's feature row is table[ids[r]] (ids dev [R] int64: ViewEmbedding 'param', blurmodel.py:133-135) or,
 * with ids == NULL, x[r] (x dev [R, C]: what the caller's param_mlp / feats concatenation produced, :139-146).
 * -> new_rays dev [R, M + use_origin, 3, 2], weight dev [R, M + 1] (:163-164), img_embed dev [R, C] (the feature rows, bit for bit: :171). */
int evd_rigid_blur_forward(const evd_rigid_blur_desc* d, const evd_rigid_blur_params* p, const float* rays, const long* ids, const float* x, long R,
                           float* new_rays, float* weight, float* img_embed, void* stream);
/* torch.autograd of the above (the reference has no explicit backward): two launches, no float atomics, the same bits on every run.
 * d_new_rays dev [R, M + use_origin, 3, 2], d_weight dev [R, M + 1], d_img_embed dev [R, C] or NULL (what arrives at the img_embed output).
 * -> grads dev: one flat float32 buffer in evd_rigid_blur_params' order (table [n_img, C] -- zeros in the ids == NULL form --, then the
 * twelve network tensors), overwritten; d_rays dev [R,3,2] or NULL; d_x dev [R, C] or NULL (ids == NULL form only).  R = 0 writes zeros. */
int evd_rigid_blur_backward(const evd_rigid_blur_desc* d, const evd_rigid_blur_params* p, const float* rays, const long* ids, const float* x, long R,
                            const float* d_new_rays, const float* d_weight, const float* d_img_embed, float* grads, float* d_rays, float* d_x,
                            void* workspace, size_t workspace_bytes, void* stream);
/* BlurModel.forward, networks/pdrf/blurmodel.py:109-224 (kernel_type DSK and PBE: the sparse kernel of Deblur-NeRF / PDRF), with
 * ViewEmbedding.forward in front: canonical positions -> embedded rows -> linears / linears1 -> offsets, translations, softmax weights ->
 * the P rays of every pixel (the call site is networks/renderer.py:303-304, the module is built at run_nerf.py:184-203).  The parameters
 * are the reference module's own tensors, float32 in torch layout, read in place.
 *   kernel_type 0 = DSK, 1 = PBE (point 0 keeps the pixel's own ray, no align); num_pt = P (1..16); in_embed 1..4, spatial_embed 0..4 =
 *   frequencies of the two positional embeddings; embed_cnl = C, width of an image's embedding row; feat_cnl = F, width of a row's feats
 *   columns (PBE; 0 for DSK); row width 2 (1 + 2 in_embed) + C + F + (spatial_embed ? 2 (1 + 2 spatial_embed) : 0) <= 127; num_hidden
 *   1..4 layers of num_wide 1..64 units; n_img = rows of the embedding table (0 without one); n_pattern = rows of pattern_pos /
 *   pattern_trans (1 with isglobal); poses_per_image = n > 0: poses is [n, 3, 4] indexed by ids (the module's `poses` buffer), 0: [R, 3, 4];
 *   H, W = image size (spatial embedding); fx, fy, cx, cy = K[0][0], K[1][1], K[0][2], K[1][2].  Anything else: EVD_E_INVALID. */
typedef struct {
    int kernel_type, num_pt, in_embed, spatial_embed, embed_cnl, feat_cnl, num_hidden, num_wide, short_cut, isglobal, optim_trans,
        optim_spatialvariant_trans, n_img, n_pattern, poses_per_image, H, W;
    float kernel_hwindow, random_hwindow, fx, fy, cx, cy;
} evd_sparse_blur_desc;
typedef struct {
    const float *pattern_pos, *pattern_trans;                /* dev [n_pattern, P, 2]; pattern_trans NULL without optim_trans */
    const float* table;                                      /* img_embed.img_embed dev [n_img, C], or NULL */
    const float *linears_w[4], *linears_b[4];                /* linears.{0,2,..}: dev [num_wide, row width | num_wide], [num_wide] */
    const float *linears1_w[2], *linears1_b[2];              /* linears1.{0,2}: dev [num_wide, (row width +) num_wide], [3 | 5, num_wide] */
} evd_sparse_blur_params;
/* bytes of the workspace both calls take for R rays (0 for an unsupported descriptor) */
size_t evd_sparse_blur_workspace_bytes(const evd_sparse_blur_desc* d, long R);
/* One launch for the network and the rays; DSK's align is a mean over the batch, which a second launch of one workgroup sums from per-ray
 * terms.  ids dev [R] int64; a ray's embedding row is table[ids[r]] or, with x != NULL, x[r] (x dev [R, C]); rays_x, rays_y dev [R];
 * poses dev [R, 3, 4] (or [n, 3, 4]); noise dev [R, P, 2] standard normal or NULL (no perturbation); feats dev [R P, F] or NULL (zeros).
 * -> new_rays dev [R, P, 3, 2], weight dev [R, P], align dev [1] (DSK; NULL allowed for PBE), img_embed dev [R, C] (the rows, bit for bit). */
int evd_sparse_blur_forward(const evd_sparse_blur_desc* d, const evd_sparse_blur_params* p, const long* ids, const float* x, const float* rays_x,
                            const float* rays_y, const float* poses, const float* noise, const float* feats, long R, float* new_rays, float* weight,
                            float* align, float* img_embed, void* workspace, size_t workspace_bytes, void* stream);
/* torch.autograd of the above: two launches, no atomics, the same bits on every run.  d_new_rays dev [R, P, 3, 2], d_weight dev [R, P],
 * d_align dev [1] or NULL, d_img_embed dev [R, C] or NULL (what arrives at the img_embed output).
 * -> grads dev: one flat float32 buffer, overwritten: pattern_pos, pattern_trans (with optim_trans), table [n_img, C] (x == NULL form),
 * linears.{0,2,..}.{weight,bias}, linears1.{0,2}.{weight,bias}; d_x dev [R, C] or NULL (x != NULL form); d_feats dev [R P, F] or NULL.
 * R = 0 writes zeros.  No gradient goes to poses, pixel coordinates or the intrinsics. */
int evd_sparse_blur_backward(const evd_sparse_blur_desc* d, const evd_sparse_blur_params* p, const long* ids, const float* x, const float* rays_x,
                             const float* rays_y, const float* poses, const float* noise, const float* feats, long R, const float* d_new_rays,
                             const float* d_weight, const float* d_align, const float* d_img_embed, float* grads, float* d_x, float* d_feats,
                             void* workspace, size_t workspace_bytes, void* stream);
/* ViewEmbeddingMLP, networks/embedding.py:35-62 (built at run_nerf.py:171-175 for kernel_img_embed_type 'param_mlp'), evaluated once per
 * IMAGE instead of once per ray: the module's input is a function of the image id only, so its values form a table [n_img, W] that
 * evd_rigid_blur_* / evd_sparse_blur_* take as their `table` and gather from by ids.  Layer i is h = relu(w[i] h + b[i]); after a skip
 * index i the next layer reads cat([embedding row, h]) (embedding columns first, :59-60), so its weight is [W, embed_dim + W].  Float32,
 * the parameters are the module's own tensors in torch layout, read in place: nothing is packed and no handle is kept.
 *   n_img 1..4096, embed_dim 1..128, W 1..128, D 1..8 layers; skip_mask bit i = skip index i: any set within 0..D-2, a bit >= D is inert
 *   (the reference's default skips=[4] with D=4), bit D-1 is refused (the module would return embed_dim + W columns under an
 *   out_channels of W).  Anything else: EVD_E_INVALID naming the field. */
typedef struct {
    int n_img, embed_dim, W, D;
    unsigned skip_mask;
} evd_view_embed_mlp_desc;
typedef struct {
    const float* table;                                      /* img_embed dev [n_img, embed_dim] */
    const float *w[8], *b[8];                                /* view_embed_linears.{i}: dev [W, embed_dim | W | embed_dim + W], [W] */
} evd_view_embed_mlp_params;
/* networks/embedding.py:35-62: bytes of the backward's workspace (0 for an unsupported descriptor) */
size_t evd_view_embed_mlp_workspace_bytes(const evd_view_embed_mlp_desc* d);
/* networks/embedding.py:51-62 on every row of img_embed, one launch -> feature_table dev [n_img, W].  A row's value does not depend on
 * its position in the table. */
int evd_view_embed_mlp_forward(const evd_view_embed_mlp_desc* d, const evd_view_embed_mlp_params* p, float* feature_table, void* stream);
/* torch.autograd of networks/embedding.py:51-62: two launches (the hidden layers are recomputed), no atomics, the same bits on every run.
 * d_feature_table dev [n_img, W] -> grads dev: one flat float32 buffer in the params' order (table [n_img, embed_dim], then w[0], b[0],
 * ...), overwritten.  An image whose d_feature_table row is zero gets a zero table row and adds nothing to the other gradients. */
int evd_view_embed_mlp_backward(const evd_view_embed_mlp_desc* d, const evd_view_embed_mlp_params* p, const float* d_feature_table, float* grads,
                                void* workspace, size_t workspace_bytes, void* stream);
/* The NaN / Inf guard of render_rays, networks/renderer.py:259-263 (there: isnan().any() + isinf().any() per result key = two
 * host synchronisations per key).  Here one launch: ptrs host[n_keys] (device arrays), counts host[n_keys] (floats per array),
 * n_keys <= 16 -> flags dev [n_keys] (unsigned): bit 0 = the key contains a NaN, bit 1 = an Inf.  Nothing synchronises; the caller
 * reads the words when (if) it wants the answer. */
int evd_numerics_flags(const float* const* ptrs, const long* counts, int n_keys, unsigned* flags, void* stream);
/* Embedder.forward, networks/embedding.py:88-98.  x dev [n,dim] -> out dev [n, dim*(1+2L)].  n == 0 is a no-op; with n > 0 a NULL x is
 * refused (-1). */
int evd_embed(const float* x, long n, int dim, int L, float* out, void* stream);

/* ---------------------------------------------------------------- render configuration
 * arguments of NeRFAll.render / render_rays (networks/renderer.py:399-466, 129-264) */
typedef struct {
    int H, W;
    float focal;            /* K[0][0] */
    int ndc, use_viewdirs, lindisp, N_samples, N_importance, white_bkgd;
    float near, far, perturb;
    int is_train;           /* nn.Module.training: gates render_rmnearplane (nerf.py:107) */
    int precision;          /* EVD_PREC_* for the MLP GEMMs */
} evd_render_cfg;

/* NeRFAll.render ray packing, networks/renderer.py:423-446: rays dev [R,3,2] -> ray_batch dev [R,11]
 * = o(3) d(3) near far viewdir(3); viewdir = d/|d| before the NDC warp.  (8 columns when !use_viewdirs)  R == 0 is a no-op; with
 * R > 0 a NULL rays is refused (-1). */
int evd_ray_batch(const evd_render_cfg* cfg, const float* rays, long R, float* ray_batch, void* stream);
/* Backward of evd_ray_batch (the training branch of NeRFAll.forward, renderer.py:303-308: the loss reaches the blur kernel's warped
 * rays through the packing, viewdirs normalisation :431 and the NDC warp utils/rays.py:104-145; the reference gets it from autograd):
 * d_ray_batch dev [R,11] -> d_rays dev [R,3,2] (overwritten).  The near / far columns carry no gradient. */
int evd_ray_batch_bwd(const evd_render_cfg* cfg, const float* rays, const float* d_ray_batch, long R, float* d_rays, void* stream);
/* pts = rays_o + rays_d * z (renderer.py:180,206,235): ray_batch dev rows of ncol floats (o at 0..2, d at 3..5), z dev [R,S] -> pts dev [R,S,3];
 * its backward: d_pts dev [R,S,3] -> columns 0..2 (sum_s d_pts) and 3..5 (sum_s z d_pts) of d_ray_batch dev [R,11], of every row: accumulate == 0 overwrites
 * the WHOLE row (zeros in the other columns), != 0 adds into those six columns and leaves the others alone. */
int evd_points(const float* ray_batch, int ncol, const float* z, long R, int S, float* pts, void* stream);
int evd_points_bwd(const float* z, const float* d_pts, long R, int S, int accumulate, float* d_ray_batch, void* stream);
/* z stratification, networks/renderer.py:163-178.  t_rand dev [R,S] is the explicit torch.rand draw
 * (required when cfg->perturb > 0).  -> z dev [R,S] */
int evd_sample_z(const evd_render_cfg* cfg, const float* ray_batch, int ncol, long R, const float* t_rand,
                 float* z, void* stream);
/* The same, and the sample positions pts dev [R,S,3] = o + d z with the arithmetic of evd_points, in one launch (what evd_c2f_render_rays
 * runs; ncol >= 6). */
int evd_sample_z_pts(const evd_render_cfg* cfg, const float* ray_batch, int ncol, long R, const float* t_rand,
                     float* z, float* pts, void* stream);
/* evd_ray_batch + evd_sample_z in one launch (what evd_nerf_render runs; 11-column batch, near / far from cfg): rays dev [R,3,2] ->
 * ray_batch dev [R,11], z dev [R,S].  Both outputs carry the bits the two entries give. */
int evd_ray_batch_z(const evd_render_cfg* cfg, const float* rays, long R, const float* t_rand, float* ray_batch, float* z,
                    void* stream);

/* ---------------------------------------------------------------- NeRF backbone (networks/nerf.py) */
typedef struct evd_nerf evd_nerf;   /* opaque: packed MFMA-fragment weight streams on one device */

typedef struct {                    /* host float32 pointers, nn.Linear layout [out,in] (state_dict arrays) */
    int D, W, multires, multires_views, skip;
    int rgb_act, sigma_act;         /* EVD_ACT_* (nerf.py:34-35) */
    float rmnear;                   /* render_rmnearplane */
    const float *pts_w[EVD_MAX_LAYERS], *pts_b[EVD_MAX_LAYERS];
    const float *views_w, *views_b, *feature_w, *feature_b, *alpha_w, *alpha_b, *rgb_w, *rgb_b; /* rgb_b may be NULL */
    /* use_viewdirs=False networks (networks/nerf.py:41-44,158-160): views_w .. rgb_w NULL and output_linear given instead,
     * output_w [output_ch, W], output_b [output_ch], output_ch 4 or 5 (renderer.py:46: 5 with importance sampling; raw2outputs reads
     * channels 0..3 only).  Their ray batch has 8 columns (renderer.py:443-446).  Inference on the generic kernel (every mode but
     * EVD_PREC_F16C); no training entries.  In the reference this network only runs with extract_feature "before_linear" (kernel_use_awp):
     * nerf.py:159 asserts otherwise. */
    const float *output_w, *output_b;
    int output_ch;
} evd_nerf_desc;

int evd_nerf_create(const evd_nerf_desc* desc, evd_nerf** out);
void evd_nerf_destroy(evd_nerf* net);
/* Parameters live in one float32 arena, canonical order: pts_linears[l].weight, .bias for l < D, then views_linears.0,
 * feature_linear, alpha_linear, rgb_linear (weight, bias each; reference nn.Linear layouts, networks/nerf.py:14-44).
 * evd_nerf_param_blocks writes the arena offset of each of the 2 D + 8 tensors plus the total (up to `capacity` longs) and
 * returns 2 D + 8.  evd_nerf_load_params re-packs every weight stream of the network on the device from new values
 * (params: device float32 [evd_nerf_param_count]) -- what a training loop calls after optimizer.step() (run_nerf.py:601). */
long evd_nerf_param_count(const evd_nerf* net);
int evd_nerf_param_blocks(const evd_nerf* net, long* offsets, int capacity);
int evd_nerf_load_params(evd_nerf* net, const float* params, void* stream);
/* bytes of the packed weight stream for a precision (what one workgroup streams per sample tile); EVD_PREC_F16C: the inference
 * stream, in which feature_linear is folded into views_linears.0 (the training forward reads an unfolded stream of its own) */
size_t evd_nerf_stream_bytes(const evd_nerf* net, int precision);

/* NeRF.mlpforward + NeRF.eval, networks/nerf.py:46-72,131-162, fused with the point computation
 * pts = o + d z (renderer.py:180) and both positional encodings.  ray_batch dev [R,11] ([R,8] for a use_viewdirs=False network), z dev [R,S]
 * -> raw dev [R,S,4] = (rgb, alpha);  feature dev [R,S,W] optional: feature_kind 1 = "after_linear"
 * (nerf.py:149-150), 2 = "before_linear" (:141-142). */
int evd_nerf_mlp(const evd_nerf* net, int precision, const float* ray_batch, const float* z, long R, int S,
                 float* raw, float* feature, int feature_kind, void* stream);

/* Training variant of evd_nerf_mlp (the forward half of the autograd graph of NeRF.mlpforward, networks/nerf.py:46-72, that
 * run_nerf.py:593-601 differentiates): same raw, and every layer's activations are kept in `store` (device,
 * evd_nerf_train_store_bytes(R * S) bytes, fragment layout of csrc/nerf_mlp.h) for evd_nerf_mlp_backward.
 * Built for precision EVD_PREC_F16 / EVD_PREC_BF16 and EVD_PREC_F16X3 on the netdepth 8, netwidth 256, skips [4] network;
 * EVD_E_INVALID otherwise.  EVD_PREC_F16X3 is the float32-grade training mode (the reference trains in float32, run_nerf.py:593-601):
 * every stored fragment is a (hi, lo) float16 pair, every product of the forward, the dgrad and the wgrad kernels is the 3-MFMA
 * split product -- twice the store (evd_nerf_train_store_bytes_prec), gradients equal to float32 autograd to ~1e-5.
 * evd_nerf_train_store_bytes = the half-precision size (kept for existing callers).
 * Every other view-branch network (netdepth 1..EVD_MAX_LAYERS, netwidth 64 / 128 / 256, one skip index or none, multires 0..10,
 * multires_views 0..10) trains in EVD_PREC_F16X3 only, on the generic kernels (csrc/kernel_nerf_train_generic.hip, kernel_gen_rows.hip): the forward is
 * evd_nerf_mlp's generic kernel with stores (raw bit-equal to evd_nerf_mlp), the store holds float32 rows (sample position and
 * direction, every layer's output) and the backward's per-sample gradient rows, and the backward multiplies in exact float32 on the
 * matrix cores with no floating-point atomics (bit-reproducible).  The sizes depend on the network:
 * evd_nerf_train_store_bytes_net / evd_nerf_backward_workspace_bytes_net return, for the 8 x 256 / (10, 4) / skips [4] network, what
 * evd_nerf_train_store_bytes_prec / evd_nerf_backward_workspace_bytes return; for a network on the generic path its sizes in
 * EVD_PREC_F16X3 and 0 in every other precision (EVD_PREC_F32 included: no training path).  use_viewdirs=False networks: 0. */
size_t evd_nerf_train_store_bytes(long nsamp);
size_t evd_nerf_train_store_bytes_prec(int precision, long nsamp);
size_t evd_nerf_train_store_bytes_net(const evd_nerf* net, int precision, long nsamp);
int evd_nerf_mlp_train(const evd_nerf* net, int precision, const float* ray_batch, const float* z, long R, int S,
                       float* raw, void* store, size_t store_bytes, void* stream);

/* Gradients of the network parameters, device float32 in the reference's nn.Linear layouts ([out, in] weights, [out] biases;
 * the same fields as evd_nerf_desc).  NULL = not wanted.  accumulate == 0: every wanted block is overwritten; != 0: the gradients are
 * ADDED into it (a training loop's persistent .grad buffers, several backward calls per optimizer step: run_nerf.py:593-601 runs one
 * loss.backward() over three renders). */
typedef struct {
    float *pts_w[EVD_MAX_LAYERS], *pts_b[EVD_MAX_LAYERS];
    float *views_w, *views_b, *feature_w, *feature_b, *alpha_w, *alpha_b, *rgb_w, *rgb_b;
    int accumulate;
} evd_nerf_grads;

/* Backward of evd_nerf_mlp_train: d_raw dev [R,S,4] (d loss / d raw) -> parameter gradients, what torch autograd computes for
 * NeRF.mlpforward (networks/nerf.py:46-72) under loss.backward() (run_nerf.py:593-601).  `store` is the one the forward
 * filled (it is consumed: the gradient fragments are written into it).  Arithmetic: MFMA operands in the forward's half
 * precision under a power-of-two loss scale chosen from max |d_raw|, float32 accumulation; the scale is removed before the
 * gradients are written.  d_pts / d_dirs dev [R*S,3] (NULL = not wanted): d loss / d sample position through PE(pts) (both
 * pts_linears[0] and the skip layer) and / d view direction through PE(dirs), per sample -- they need the forward's positions
 * pts dev [R*S,3] (= o + d z) and viewdirs (rows of vd_stride floats per ray).  workspace: evd_nerf_backward_workspace_bytes().
 * A network on the generic path (see evd_nerf_mlp_train): store and workspace sized by the *_net queries, float32 arithmetic without a
 * loss scale, pts / viewdirs read from the store. */
size_t evd_nerf_backward_workspace_bytes(void);
size_t evd_nerf_backward_workspace_bytes_net(const evd_nerf* net, int precision);
int evd_nerf_mlp_backward(const evd_nerf* net, int precision, const float* d_raw, long R, int S, void* store, size_t store_bytes,
                          const evd_nerf_grads* grads, const float* pts, const float* viewdirs, int vd_stride, float* d_pts,
                          float* d_dirs, void* workspace, size_t workspace_bytes, void* stream);

/* Training forward and backward WITH the per-sample feature the AWP proposal reads as depth_feature in mode='nerf'
 * (networks/renderer.py:238-257; run_nerf.py:223 builds the proposal with input_ch = netwidth).  EVD_PREC_F16X3 only, and always the
 * generic kernels of evd_nerf_mlp_train (float32 rows in the store, exact float32 backward, no atomics) -- for EVERY view-branch network of
 * width 64 / 128 / 256, the 8 x 256 / (10, 4) / skips [4] one included; use_viewdirs=False networks and every other precision:
 * EVD_E_INVALID (the size queries: 0).  The plain entries above are untouched by these.
 *   evd_nerf_mlp_train_feature: raw bit-equal to evd_nerf_mlp_train's, for the 8 x 256 network too (the handle keeps a stream in the pipelined
 *     kernel's skip-layer order for it).  feature_kind 1 = "after_linear" (the
 *     feature_linear output, nerf.py:149-150), 2 = "before_linear" (the ReLU output of the last pts_linears layer, :141-142).  The feature
 *     is a plane of the store, not a copy: row s (s < R * S; the store pads the sample count to 32, those rows are not written) starts
 *     *feature_offset + s * *feature_stride FLOATS into the store and holds netwidth floats.  The backward leaves that plane as it is.
 *   evd_nerf_mlp_backward_feature: the gradients of sum(raw d_raw) + sum(feature d_feature).  d_feature dev rows of d_feature_stride
 *     floats ([R * S, netwidth]), or NULL: then exactly evd_nerf_mlp_backward on the generic path.  grads (accumulate included), d_pts,
 *     d_dirs as there; the sample positions and directions are read from the store.
 *   Sizes: evd_nerf_train_feature_store_bytes, evd_nerf_backward_feature_workspace_bytes. */
size_t evd_nerf_train_feature_store_bytes(const evd_nerf* net, int precision, long nsamp);
size_t evd_nerf_backward_feature_workspace_bytes(const evd_nerf* net, int precision);
int evd_nerf_mlp_train_feature(const evd_nerf* net, int precision, const float* ray_batch, const float* z, long R, int S, float* raw,
                               int feature_kind, void* store, size_t store_bytes, long* feature_offset, long* feature_stride, void* stream);
int evd_nerf_mlp_backward_feature(const evd_nerf* net, int precision, const float* d_raw, const float* d_feature, long d_feature_stride,
                                  int feature_kind, long R, int S, void* store, size_t store_bytes, const evd_nerf_grads* grads,
                                  float* d_pts, float* d_dirs, void* workspace, size_t workspace_bytes, void* stream);

/* raw2outputs: networks/nerf.py:74-129 (sigma_ch 3, rgb_ch0 0) and networks/pdrf/voxnerf.py:153-201
 * (sigma_ch 0, rgb_ch0 1).  raw dev [R,S,C], z dev [R,S], rays_d dev rows of rays_d_stride floats.
 * noise dev [R,S-1] optional (explicit randn*raw_noise_std draw).  rmnear_thresh <= 0 disables the
 * eval near-plane mask.  Outputs: out_map [R,n_rgb], density [R,S-1], acc [R], weights [R,S],
 * depth [R], fmap [R,F] = sum_s w feature[R,S,F]. */
int evd_raw2outputs(const float* raw, const float* z, const float* rays_d, int rays_d_stride, long R, int S, int C,
                    int sigma_ch, int rgb_ch0, int n_rgb, int rgb_act, int sigma_act, int white_bkgd,
                    float rmnear_thresh, const float* noise,
                    float* out_map, float* density, float* acc, float* weights, float* depth,
                    const float* feature, int F, float* fmap, void* stream);

/* Backward of evd_raw2outputs (first slice of the training path; torch autograd provides this in the reference):
 * g_map dev [R,3], g_depth dev [R], g_acc dev [R], g_weights dev [R,S] = dL/d(out_map, depth, acc, weights), any may be
 * NULL (= zero) -> d_raw dev [R,S,4] = dL/d raw.  z and rays_d are sampling inputs and get no gradient (sample_pdf is
 * detached in the reference, renderer.py:201).  Built for C = 4, n_rgb = 3, S <= 256. */
int evd_raw2outputs_bwd(const float* raw, const float* z, const float* rays_d, int rays_d_stride, long R, int S, int C,
                        int sigma_ch, int rgb_ch0, int n_rgb, int rgb_act, int sigma_act, int white_bkgd, float rmnear_thresh,
                        const float* noise, const float* g_map, const float* g_depth, const float* g_acc, const float* g_weights,
                        float* d_raw, void* stream);
/* The same with the gradient w.r.t. the ray directions, d_rays_d dev [R, >= 3] (row stride d_rays_d_stride) or NULL: alpha depends on
 * rays_d through dists * |rays_d| (nerf.py:104, voxnerf.py:179), which the blur batch's learnable ray warp differentiates
 * (run_nerf.py:593): dL/d rays_d = (sum_i dL/d density_i * density_i) * rays_d / |rays_d|^2. */
int evd_raw2outputs_bwd_rays(const float* raw, const float* z, const float* rays_d, int rays_d_stride, long R, int S, int C,
                             int sigma_ch, int rgb_ch0, int n_rgb, int rgb_act, int sigma_act, int white_bkgd, float rmnear_thresh,
                             const float* noise, const float* g_map, const float* g_depth, const float* g_acc, const float* g_weights,
                             float* d_raw, float* d_rays_d, int d_rays_d_stride, void* stream);
/* Backward of the FEATURE composite of a composite_feature level (kernel_type PBE, voxnerf.py:223-229): the map is
 * fmap[r,c] = sum_i w_i act(rows[r,i,c]) over the G geo channels, the density is channel sigma_ch of raw dev [R,S,C].
 * rows dev [R,S,G] are the geo rows BEFORE the activation rows_act (relu on the coarse level, none is legal).  g_fmap dev [R,G],
 * g_depth dev [R], g_acc dev [R], g_weights dev [R,S]: any may be NULL (= zero).  Writes d_raw dev [R,S,C] (channel sigma_ch = dL/d sigma,
 * every other channel zero), d_rows dev [R,S,G] (every element) and, where wanted, d_rays_d as evd_raw2outputs_bwd_rays does.
 * The forward quantities are recomputed; G in 1..128, S in 1..256. */
int evd_raw2outputs_feat_bwd(const float* raw, int C, int sigma_ch, const float* rows, int G, int rows_act, const float* z,
                             const float* rays_d, int rays_d_stride, const float* noise, int sigma_act, float rmnear_thresh, long R, int S,
                             const float* g_fmap, const float* g_depth, const float* g_acc, const float* g_weights,
                             float* d_raw, float* d_rows, float* d_rays_d, int d_rays_d_stride, void* stream);

/* sample_pdf, utils/rays.py:149-193, called as in renderer.py:200-201,230-231 with bins = z_mid and
 * weights[...,1:-1]: z dev [R,S], weights dev [R,S] -> z_samples dev [R,N].  det != 0 => u = linspace;
 * else u dev [R,N].  Also returns, fused: z_merged dev [R,S+N] = sort(cat(z, z_samples)) (renderer.py:205,234),
 * order dev int32 [R,S+N] (index into the concatenation, as torch.sort's second result), z_std dev [R]
 * (renderer.py:250). */
int evd_sample_pdf_merge(const float* z, const float* weights, long R, int S, int N, int det, const float* u,
                         float* z_samples, float* z_merged, int* order, float* z_std, void* stream);

typedef struct {        /* result dict of render_rays, networks/renderer.py:242-257; dev pointers or NULL */
    float *rgb, *depth, *acc;                   /* rgb_map [R,3], depth_map [R], acc_map [R] */
    float *z_vals, *weights;                    /* [R, N_samples+N_importance] */
    float *rgb0, *depth0, *acc0, *z_std;        /* coarse pass (N_importance > 0) */
    float *z_vals0, *weights0;                  /* [R, N_samples] */
    float *feature;                             /* per-sample feature of the last pass [R,S_final,F] */
    float *raw;                                 /* raw network output of the last pass [R,S_final,4] */
    int feature_kind;                           /* NeRF: 1 after_linear, 2 before_linear */
} evd_render_out;

size_t evd_nerf_render_workspace_bytes(const evd_render_cfg* cfg, long R);
/* NeRFAll.render_rays for mode='nerf' (networks/renderer.py:129-264, else-branch :218-240): ray_batch dev [R,11].
 * fine may be NULL iff N_importance == 0.  Explicit random draws (the reference calls torch.rand / randn
 * inside): t_rand dev [R,N_samples] and u dev [R,N_importance] when perturb > 0; noise0 dev [R,N_samples-1] /
 * noise1 dev [R,N_samples+N_importance-1] = randn * raw_noise_std (NULL = no density noise). */
int evd_nerf_render_rays(const evd_nerf* coarse, const evd_nerf* fine, const evd_render_cfg* cfg, const float* ray_batch,
                         long R, const float* t_rand, const float* u, const float* noise0, const float* noise1,
                         evd_render_out* out, void* workspace, size_t workspace_bytes, void* stream);
/* NeRFAll.render (networks/renderer.py:399-466) = evd_ray_batch + evd_nerf_render_rays: rays dev [R,3,2] */
int evd_nerf_render(const evd_nerf* coarse, const evd_nerf* fine, const evd_render_cfg* cfg, const float* rays, long R,
                    const float* t_rand, const float* u, const float* noise0, const float* noise1,
                    evd_render_out* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- PDRF backbone (networks/pdrf/voxnerf.py) */
typedef struct evd_voxel evd_voxel; /* opaque: channel-last tri-plane grids + packed MLPs on one device */

typedef struct {                    /* host float32 pointers */
    int num_layers, hidden_dim, geo_feat_dim, num_layers_color, input_ch, multires, multires_views;
    int app_dim, n_comp[3], grid[3], app_act, rgb_act, sigma_act, composite_feature;
    float aabb[6], rmnear;
    const float *sigma_w[EVD_MAX_LAYERS];
    const float *color_w[EVD_MAX_LAYERS], *color_b[EVD_MAX_LAYERS];
    const float *plane[3], *line[3], *basis;
} evd_voxel_desc;

/* Level shapes (reference options --coarse_hidden_dim, --fine_hidden_dim, --fine_geo_feat_dim, --kernel_feat_cnl,
 * --{coarse,fine}_num_layers[_color], --fine_app_dim; options.py:134-163): hidden_dim 64, 128 or 256 (also the colour network's hidden
 * width, voxnerf.py:73,78), geo_feat_dim 1..128, num_layers and num_layers_color 1..4, input_ch - 3 (1 + 2 multires) feature channels a
 * multiple of 16 in 16..64; anything else is EVD_E_INVALID.  The STANDARD levels -- 64/15/32 and 256/128/64 (hidden / geo / features)
 * with 2 + 3 layers -- have the pipelined, resident and compensated kernels and the training path.  Every other shape is a GENERIC
 * level: inference in every arithmetic mode (EVD_PREC_F16C is EVD_PREC_F16X3 there, float32 grids included, as on the standard coarse level) through
 * evd_voxel_mlp, evd_voxel_forward and the c2f render; no composite_feature, no training entries (EVD_E_INVALID). */
int evd_voxel_create(const evd_voxel_desc* desc, evd_voxel** out);
void evd_voxel_destroy(evd_voxel* v);
/* VoxelNeRFBase.sample / compute_appfeature, voxnerf.py:203-208,132-151.  pts dev [n,3] -> out dev [n,out_stride]
 * written at column out_col (so coarse and fine features can share one [n,64] buffer, renderer.py:195) */
int evd_voxel_sample(const evd_voxel* v, const float* pts, long n, float* out, int out_stride, int out_col, void* stream);
/* The same as the c2f renderer runs it in arithmetic mode `precision`: EVD_PREC_F16 / EVD_PREC_BF16 gather the float16 copies of the
 * grids (half the bytes; the level networks round their inputs to 2^-11 / 2^-8 anyway), the float32-grade modes the float32 grids.
 * What the training forward calls, so that it is the inference render's arithmetic. */
int evd_voxel_sample_prec(const evd_voxel* v, int precision, const float* pts, long n, float* out, int out_stride, int out_col, void* stream);
/* VoxelNeRFBase.forward, voxnerf.py:210-259.  pts dev [R,S,3], viewdirs dev rows of vd_stride floats,
 * fts dev [R,S,F] -> color [R,3], depth [R], acc [R], weights [R,S], feature [R,S,geo].
 * A level created with composite_feature != 0 (kernel_type PBE, voxnerf.py:223-239) composites its geo features first and runs the
 * colour network per ray: `feature` is then the COMPOSITED map [R,geo].  This entry is the inference pass (the workspace query includes its scratch); the two
 * per-ray steps train through evd_raw2outputs_feat_bwd and evd_voxel_color_rows_train / _backward below. */
int evd_voxel_forward(const evd_voxel* v, int precision, const float* pts, const float* viewdirs, int vd_stride, const float* fts, int F,
                      const float* z, const float* rays_d, int rays_d_stride, long R, int S, int is_train,
                      float* color, float* depth, float* acc, float* weights, float* feature,
                      void* workspace, size_t workspace_bytes, void* stream);
size_t evd_voxel_forward_workspace_bytes(const evd_voxel* v, long R, int S);
/* The per-sample part of VoxelNeRFBase.forward alone (voxnerf.py:210-221,240-254), inference: pts dev [R,S,3], viewdirs dev rows of
 * vd_stride floats (one per ray), fts dev rows of ft_stride floats -> raw dev [R,S,4] = (sigma, sigmoid(colour)) and feature dev
 * [R,S,geo] (NULL = not wanted), the per-sample geo rows.  Any level; the kernel evd_voxel_forward runs for the same arguments. */
int evd_voxel_mlp(const evd_voxel* v, int precision, const float* pts, const float* viewdirs, int vd_stride, const float* fts, int ft_stride,
                  long R, int S, float* raw, float* feature, void* stream);
size_t evd_c2f_render_workspace_bytes(const evd_voxel* coarse, const evd_voxel* fine, const evd_render_cfg* cfg, long R);
/* NeRFAll.render_rays for mode='c2f' (networks/renderer.py:182-217); arguments as evd_nerf_render_rays.
 * out->feature receives the fine level's per-sample geo features [R,S_final,geo_feat_dim] (what AWP consumes). */
int evd_c2f_render_rays(const evd_voxel* coarse, const evd_voxel* fine, const evd_render_cfg* cfg, const float* ray_batch, long R,
                        const float* t_rand, const float* u, const float* noise0, const float* noise1,
                        evd_render_out* out, void* workspace, size_t workspace_bytes, void* stream);
/* NeRFAll.render for mode='c2f' = evd_ray_batch + evd_c2f_render_rays */
int evd_c2f_render(const evd_voxel* coarse, const evd_voxel* fine, const evd_render_cfg* cfg, const float* rays, long R,
                   const float* t_rand, const float* u, const float* noise0, const float* noise1,
                   evd_render_out* out, void* workspace, size_t workspace_bytes, void* stream);
/* The coarse feature rows of the merged sample set, renderer.py:209-213: torch.cat([ft_comb0, ft_comb1], 1) gathered by the sort order
 * (`order` of evd_sample_pdf_merge): old dev [R,S,F], fresh dev [R,N,F], order dev int32 [R,S+N] -> out dev rows of out_stride floats
 * (columns 0..F-1 written).  evd_c2f_render_rays does this internally; the entry (and its backward: a permutation, d_out rows of
 * d_stride floats -> d_old dev [R,S,F], d_fresh dev [R,N,F], every row written once) serves the training path under autograd. */
int evd_merge_features(const float* old, const float* fresh, const int* order, long R, int S, int N, int F, float* out, int out_stride, void* stream);
int evd_merge_features_bwd(const float* d_out, int d_stride, const int* order, long R, int S, int N, int F, float* d_old, float* d_fresh, void* stream);
/* TV_loss_app, voxnerf.py:126-130 (TVLoss :306-324): sum over planes*1e-2 + lines*1e-3 -> out dev [1] (float) */
int evd_voxel_tv_loss(const evd_voxel* v, float* out, void* stream);

/* ---- training one PDRF level's sigma / colour networks -------------------------------------------------
 * Parameters live in one float32 arena, canonical order sigma_net.0.weight, sigma_net.1.weight, color_net.{0,1,2}.{weight,bias}
 * (reference nn.Linear layouts, voxnerf.py:60-84); evd_voxel_param_blocks writes the 8 offsets + the total and returns 8
 * (a generic level: sigma_net.0 .. num_layers-1, then color_net.l.{weight,bias}; num_layers + 2 num_layers_color blocks);
 * evd_voxel_load_params re-packs every weight stream of the level on the device (after optimizer.step()).
 * evd_voxel_mlp_train = the per-sample part of VoxelNeRFBase.forward (voxnerf.py:210-221,240-254): raw dev [R,S,4] =
 * (sigma, sigmoid(colour)), every layer's activations kept in `store` (evd_voxel_train_store_bytes); feature dev [R,S,geo]
 * (NULL = not wanted; the fine level, and a coarse level with composite_feature) = the per-sample geo features AWP consumes
 * (voxnerf.py:221) or, on a composite_feature level (kernel_type PBE), the rows BEFORE rgb_activate that evd_raw2outputs composites per
 * ray (voxnerf.py:223-229; f16x3 / f16 / bf16 -- in the half-precision modes the rounded values the store keeps), whose gradient
 * evd_voxel_mlp_backward takes back as d_feature (NULL = none).
 * evd_voxel_mlp_backward: d_raw, raw dev [R,S,4] -> parameter gradients (overwritten) and d_fts dev [R*S, d_fts_stride]
 * (columns 0 .. ft_dim-1 overwritten; NULL = not wanted), the gradient of the sampled features that evd_voxel_sample_bwd
 * scatters into the grids.  d_pts / d_dirs dev [R*S, 3] (NULL = not wanted; need the forward's pts / viewdirs): the gradient
 * that reaches the sample position through PE(pts) and the view direction through PE(dirs) (per sample: the caller sums over a
 * ray's samples) -- what carries the loss back to the rays, i.e. to the blur kernel's camera motion.  awp_store (NULL = none; fine
 * level): the store of the fused AWP embedding AFTER evd_awp_embed_backward ran on the same samples -- its d geo fragments are added
 * to the geo features' gradient without ever becoming a float32 [R*S,128] tensor (below).
 * Built for EVD_PREC_F16 / EVD_PREC_BF16 and the float32-grade EVD_PREC_F16X3 (as evd_nerf_mlp_train; awp_store is a half-precision
 * coupling: in f16x3 the AWP consumer's gradient comes back as d_feature rows), both shipped levels (64/15/32 and 256/128/64).
 * A level of any other shape evd_voxel_create accepts trains in EVD_PREC_F16X3 alone: the forward is the inference kernel of that mode
 * (raw bit-equal to evd_voxel_mlp) writing float32 rows to the store, the backward one exact-float32 wgrad and dgrad launch per layer
 * with a fixed summation order (two calls give the same bits); no awp_store there.  Its backward workspace is sized by
 * evd_voxel_backward_workspace_bytes_net (a standard level: evd_voxel_backward_workspace_bytes(); 0: NULL handle, or a precision the
 * level does not train in); evd_voxel_train_store_bytes_prec answers 0 for such a precision too. */
typedef struct { float *sigma_w[4], *color_w[4], *color_b[4]; int accumulate; /* sigma_net.l, color_net.l (unused layers NULL); as in evd_nerf_grads */ } evd_voxel_grads;
int evd_voxel_geo_feat_dim(const evd_voxel* v);
long evd_voxel_param_count(const evd_voxel* v);
int evd_voxel_param_blocks(const evd_voxel* v, long* offsets, int capacity);
int evd_voxel_load_params(evd_voxel* v, const float* params, void* stream);
size_t evd_voxel_train_store_bytes(const evd_voxel* v, long nsamp);         /* the f16 / bf16 size */
size_t evd_voxel_train_store_bytes_prec(const evd_voxel* v, int precision, long nsamp);   /* EVD_PREC_F16X3: (hi, lo) fragments, twice that */
size_t evd_voxel_backward_workspace_bytes(void);
size_t evd_voxel_backward_workspace_bytes_net(const evd_voxel* v, int precision);
int evd_voxel_mlp_train(const evd_voxel* v, int precision, const float* pts, const float* viewdirs, int vd_stride, const float* fts,
                        int ft_stride, long R, int S, float* raw, float* feature, void* store, size_t store_bytes, void* stream);
int evd_voxel_mlp_backward(const evd_voxel* v, int precision, const float* d_raw, const float* raw, const float* d_feature,
                           const void* awp_store, size_t awp_store_bytes, long R, int S, void* store, size_t store_bytes, const evd_voxel_grads* grads, float* d_fts, int d_fts_stride, const float* pts,
                           const float* viewdirs, int vd_stride, float* d_pts, float* d_dirs, void* workspace,
                           size_t workspace_bytes, void* stream);
/* The per-RAY colour network of a composite_feature level (voxnerf.py:231-239) for training, float32 in every mode as at inference.
 * evd_voxel_color_rows_train: fmap dev [R,geo] (the composited map), viewdirs dev rows of vd_stride floats -> color dev [R,3], the bits
 * evd_voxel_forward writes for the same map, and the two hidden activations kept in `store` (evd_voxel_color_rows_store_bytes).
 * evd_voxel_color_rows_backward: g_color dev [R,3] -> d_map dev [R,geo], d_viewdirs dev [R,3] through the direction encoding (NULL = not
 * wanted) and the gradients of color_net.l.{weight,bias} through grads->color_w / color_b (NULL pointer = skipped; sigma_w is not read);
 * grads->accumulate != 0 adds into the caller's buffers instead of writing.  Each workgroup sums its rays' terms in ray order and the
 * workgroups' partial sums (in `workspace`, evd_voxel_color_rows_backward_workspace_bytes) are folded in workgroup order: two calls give
 * the same bits.  Built for the standard coarse level (hidden 64, geo 15, three colour layers, multires_views 0..4); a 256/128
 * composite level is refused with EVD_E_INVALID. */
size_t evd_voxel_color_rows_store_bytes(const evd_voxel* v, long R);
size_t evd_voxel_color_rows_backward_workspace_bytes(const evd_voxel* v, long R);
int evd_voxel_color_rows_train(const evd_voxel* v, const float* fmap, const float* viewdirs, int vd_stride, long R, float* color,
                               void* store, size_t store_bytes, void* stream);
int evd_voxel_color_rows_backward(const evd_voxel* v, const float* g_color, const float* fmap, const float* viewdirs, int vd_stride, long R,
                                  const void* store, size_t store_bytes, const evd_voxel_grads* grads, float* d_map, float* d_viewdirs,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- training the PDRF grids (scatter-add into the tri-planes) -----------------------------------------
 * The library keeps planes / lines CHANNEL-LAST: plane[i] [grid[m1]][grid[m0]][C_i] (reference app_plane.i is [1,C,H,W],
 * voxnerf.py:112-113), line[i] [grid[vec]][C_i], basis [app_dim][sum C] (= basis_mat.weight).  Parameters and gradients of
 * the training path use THAT layout (a permute away from the state dict).
 * evd_voxel_grid_sizes: element counts, sizes[0..2] planes, [3..5] lines, [6] basis.
 * evd_voxel_get_grids / evd_voxel_load_grids: copy the grids out to / in from caller-owned device buffers (load also
 * refreshes the float16 copies the half-precision modes read) -- what a training loop calls after optimizer.step(). */
typedef struct { float *plane[3], *line[3], *basis; } evd_voxel_grid_grads;
int evd_voxel_grid_sizes(const evd_voxel* v, long* sizes);
int evd_voxel_get_grids(const evd_voxel* v, float* const* plane, float* const* line, float* basis, void* stream);
int evd_voxel_load_grids(evd_voxel* v, const float* const* plane, const float* const* line, const float* basis, void* stream);
/* Where the level keeps its grids: the seven float32 device arrays (plane_f32[0..2], line_f32[0..2], *basis_f32) evd_voxel_load_grids
 * writes, and the float16 copies of the planes and lines (plane_f16 / line_f16; the basis has none).  Order and element layout are
 * those of evd_voxel_get_grids / evd_voxel_load_grids.  A writer that stores a new grid value to BOTH (the float16 one through the
 * saturating conversion of evd_voxel_load_grids) has done what evd_voxel_load_grids does: the optimizer step's mirrors (evd_adam_step).
 * Host call, touches no device state; the pointers stay valid until evd_voxel_destroy. */
int evd_voxel_grid_mirrors(const evd_voxel* v, float** plane_f32, float** line_f32, float** basis_f32, void** plane_f16, void** line_f16);
/* Backward of evd_voxel_sample (VoxelNeRFBase.sample / compute_appfeature, voxnerf.py:132-151,203-208; app_actfn none):
 * d_out dev rows of d_stride floats, the app_dim gradient columns start at d_col -> gradients ADDED into g (caller zeroes;
 * NULL = not wanted) with float32 hardware atomics; like the reference's grid_sample backward (voxnerf.py:144) the summation
 * order is not deterministic.  d_pts dev [n,3] (NULL = not wanted) is OVERWRITTEN with d loss / d pts through the bilinear /
 * linear interpolation weights (ATen grid_sample backward semantics: taps outside the grid contribute nothing).
 * Arithmetic: d coef = d out . basis_mat is a split-float16 product (operands scaled by powers of two, hi + lo, ~2^-21 per product) in
 * EVERY precision mode, EVD_PREC_F32 included; the rest (weights, re-gathered values, the sums into the gradients) is float32. */
int evd_voxel_sample_bwd(const evd_voxel* v, const float* pts, long n, const float* d_out, int d_stride, int d_col,
                         const evd_voxel_grid_grads* g, float* d_pts, void* stream);
/* The same with caller scratch (evd_voxel_sample_bwd_workspace_bytes(v, n): 4 x (sum of n_comp) + 48 B per sample, 432 B at the
 * shipped (64, 16, 16), plus 512 B; n_comp in {16, 32, 64}, else the call is evd_voxel_sample_bwd): the HYBRID form -- the plane taps stay direct float atomics, the line taps (a third of the atomic
 * requests, onto a few hundred cells) are summed per 2048 samples in LDS slices of the line gradients (64-bit fixed point, exact
 * conversion of every float32 contribution above 2^-49 of the chunk's maximum) and added once: 24-27 % faster, same sums to float32
 * rounding of the summation order.  With workspace NULL / 0 bytes this IS evd_voxel_sample_bwd. */
size_t evd_voxel_sample_bwd_workspace_bytes(const evd_voxel* v, long n);
int evd_voxel_sample_bwd_ws(const evd_voxel* v, const float* pts, long n, const float* d_out, int d_stride, int d_col,
                            const evd_voxel_grid_grads* g, float* d_pts, void* workspace, size_t workspace_bytes, void* stream);
/* The same in the arithmetic mode `precision` of the forward gather (evd_voxel_sample_prec): where that forward interpolated the FLOAT16
 * copies of the grids (f16 / bf16 on every level, f16c on the fine level of a c2f pair), the backward's re-gather of the plane / line values
 * (d plane = d coef x line value, d line = d coef x plane value, d pts) reads the same copies -- the gradient of the function the forward
 * computed, at half the gather's loads and bytes; the other modes are evd_voxel_sample_bwd_ws. */
int evd_voxel_sample_bwd_prec(const evd_voxel* v, int precision, const float* pts, long n, const float* d_out, int d_stride, int d_col,
                              const evd_voxel_grid_grads* g, float* d_pts, void* workspace, size_t workspace_bytes, void* stream);
/* The DETERMINISTIC scatter (the reference asks for repeatable runs, seed_everything(args.seed, deterministic=True), run_nerf.py:50, and
 * names grid_sample's backward, voxnerf.py:144, as the operation that cannot repeat).  Arguments as evd_voxel_sample_bwd_prec: ADDS into
 * the gradients of g (NULL = not wanted), overwrites d_pts, reads the float16 grid copies where the forward of `precision` did; n == 0 is a
 * no-op; every n_comp evd_voxel_sample_bwd takes.  Every tap contribution w_tap x (d coef x other) is computed in float32 (d coef: one
 * float32 fmaf chain over app_dim per element, a function of the sample alone), converted with round-to-nearest to signed 64-bit fixed
 * point and added with an integer atomic to a shadow accumulator in the workspace; a finish kernel adds (float)(acc x unit) to each
 * gradient element once and leaves the accumulator zero (the entry zeroes the shadow itself: the workspace may hold anything).
 *   unit:  ONE per call.  cmax = the largest |contribution| of the batch (a first pass over the same arithmetic, atomicMax on the float's
 *          bits); frexpf(cmax) -> E (cmax < 2^E), h = ceil(log2(4 n)), unit = 2^(E - (62 - h)) = 2^-k with k = evd_scatter_det_unit_exp(cmax, n).
 *          A cell receives at most 4 n terms below 2^(62 - h) units: no overflow for any input; contributions more than 62 - h bits (>= 40
 *          for n <= 2^20) below the batch maximum are flushed.  k is clamped to 126, so that 2^k is a finite float32.
 *   guarantee:  the plane and line gradients are bit-identical from run to run AND under any permutation of the samples; d_pts is a fixed-order
 *          sum per sample (bit-identical per sample under permutation); the basis gradient is summed per workgroup (tile t on workgroup t mod
 *          min(tiles, 512)) and the workgroups' partials are folded in workgroup order: bit-identical from run to run for a given n, NOT
 *          permutation invariant.
 *   non-finite d_out or grids (cmax not finite):  no unit exists; the batch is scattered by evd_voxel_sample_bwd_prec into the same workspace,
 *          so a NaN / Inf reaches the gradients exactly as it does there.
 * The entry READS cmax ON THE HOST between its two passes: it synchronises the stream once per call (the exception to the conventions above;
 * it cannot be captured into a graph).  Workspace: 8 B per plane and line gradient element + 512 x app_dim x sum(n_comp) x 4 B of
 * workgroup partials (or the size of evd_voxel_sample_bwd_workspace_bytes where that is larger) + 512 B; NULL level -> 0. */
size_t evd_voxel_sample_bwd_det_workspace_bytes(const evd_voxel* v, long n);
int evd_voxel_sample_bwd_det(const evd_voxel* v, int precision, const float* pts, long n, const float* d_out, int d_stride, int d_col,
                             const evd_voxel_grid_grads* g, float* d_pts, void* workspace, size_t workspace_bytes, void* stream);
/* pure host function: the exponent k of the fixed-point scale 2^k above (k = 62 - ceil(log2(4 n)) - E, at most 126); 0 where cmax is
 * not finite or not positive or n < 1 */
int evd_scatter_det_unit_exp(float cmax, long n);
/* d_loss[0] * d TV_loss_app / d grid added into g (voxnerf.py:126-130, 306-324); d_loss is a DEVICE scalar (no host sync) */
int evd_voxel_tv_loss_bwd(const evd_voxel* v, const float* d_loss, const evd_voxel_grid_grads* g, void* stream);

/* ---------------------------------------------------------------- loss-side pixel ops */
/* RigidBlurringModel.rbk_weighted_sum, networks/dpnerf/blurmodel.py:112-127 (and renderer.py:299,332-354):
 * out[r,c] = sum_p ccw[r,p] x[r*P+p, c] */
int evd_weighted_sum(const float* x, const float* ccw, long R, int P, int C, float* out, void* stream);

typedef struct evd_crf evd_crf;     /* opaque: CRF MLP parameters (networks/tonemapping.py:7-93) */
typedef struct {
    int map_type;                   /* 0 none, 1 gamma, 2 learn */
    float gamma;
    int extra_features;
    const float *w[4], *b[4];       /* host: linear.{0,2,4,6}.{weight,bias} when map_type == 2 */
} evd_crf_desc;
int evd_crf_create(const evd_crf_desc* desc, evd_crf** out);
void evd_crf_destroy(evd_crf* crf);
/* Deterministic loss reductions (run_nerf.py:50).  With on != 0, evd_blur_loss_reduce, evd_blur_loss_bwd(_dev), evd_event_loss_reduce and
 * evd_event_loss_bwd(_dev) called with THIS handle launch forms without floating-point atomics: a bounded grid (<= 256 workgroups) walks the
 * batch, per-workgroup sums go to a buffer of the handle (allocated on the first enable, outside the iteration loop) and one wavefront adds them
 * in workgroup order and performs the call's single partial[k] += sum (d_params: overwritten, as before); d_w1 / d_w2 are the three channel
 * terms added in channel order.  Same bits for the same batch.  While on, the handle is NOT re-entrant for these entries (one launch's partials
 * live in the handle's buffer): one stream at a time.  With on == 0 (the default) every kernel, launch and bit is as before. */
int evd_crf_set_deterministic(evd_crf* crf, int on);
/* CRF.forward (+ rec601/rec709/avg luma of TonemappingTransform.encode_luma, tonemapping.py:120-139).
 * x dev [n,3]; feat dev NULL | [n,E] (feat_per_channel 0) | [n,3,E] (1).  luma < 0: out [n,3];
 * luma 0/1/2 = rec601/rec709/avg: out [n,1]. */
int evd_crf_forward(const evd_crf* crf, const float* x, const float* feat, int feat_per_channel, int skip_learn,
                    int luma, long n, float* out, void* stream);

/* Fused blur-loss reduction for one pixel batch (spec: run_nerf.py:443-497 + rbk_weighted_sum):
 *   rgb   = sum_p w1[r,p] rgb_p[r,p]       rgb1 = sum_p w1[r,p] rgb0_p[r,p]     awp = sum_p w2[r,p] rgb_p[r,p]
 *   partial[0..2] = sum_r |crf(rgb)-tgt|^2, |crf(rgb1)-tgt|^2, |crf(awp)-tgt|^2   (3 channels summed)
 *   partial[3..4] = sum_r |crf(rgb_p[r,0])-tgt0|^2, |crf(rgb0_p[r,0])-tgt0|^2     (pts0 / EDI prior terms)
 *   partial[5]    = 3 R  (element count)
 * rgb0_p, w2, tgt0 may be NULL (their partials stay 0).  Accumulates (atomicAdd) into partial dev [8]:
 * zero it once per step; ranks all-reduce the 8 floats (evdeblurnerf_amd/dist.py).  Optionally writes
 * the blended colours rgb/rgb1/awp dev [R,3]. */
int evd_blur_loss_reduce(const evd_crf* crf_rgb, int skip_learn, const float* rgb_p, const float* rgb0_p,
                         const float* w1, const float* w2, const float* tgt, const float* tgt0, long R, int P,
                         float* partial, float* out_rgb, float* out_rgb1, float* out_awp, void* stream);

/* Backward of evd_blur_loss_reduce (identity / gamma response on the image branch, as in every shipped config):
 * g_partial host[5] = dL/d partial[0..4] -> d_rgb_p, d_rgb0_p dev [R,P,3] (d_rgb0_p may be NULL), d_w1, d_w2 dev [R,P] or NULL. */
int evd_blur_loss_bwd(const evd_crf* crf_rgb, int skip_learn, const float* rgb_p, const float* rgb0_p, const float* w1, const float* w2,
                      const float* tgt, const float* tgt0, long R, int P, const float* g_partial, float* d_rgb_p, float* d_rgb0_p,
                      float* d_w1, float* d_w2, void* stream);
/* the same with dL/d partial read from DEVICE memory (g_partial_dev dev[>=5]): what an autograd node calls, no host copy in the backward */
int evd_blur_loss_bwd_dev(const evd_crf* crf_rgb, int skip_learn, const float* rgb_p, const float* rgb0_p, const float* w1, const float* w2,
                          const float* tgt, const float* tgt0, long R, int P, const float* g_partial_dev, float* d_rgb_p, float* d_rgb0_p,
                          float* d_w1, float* d_w2, void* stream);

/* Fused event-loss reduction (spec: run_nerf.py:518-570, utils/events.py:260-284):
 *   bii = thr_neg*cum_neg + thr_pos*cum_pos;  feat = (cum_neg, cum_pos) per event ("pos-neg") or scattered to the
 *   event's colour channel ("color-pos-neg", color_mask != NULL); luma = CRF_event(rgb) -> rec601 luma, or the
 *   masked channel when tonemap_only;  pred = log(l_end+1e-5) - log(l_start+1e-5);
 *   partial[0] += sum w (pred-bii)^2 (fine), partial[1] += same for the coarse pair, partial[2] += sum w.
 * start/end/start0/end0 dev [N,3] linear rgb; cum_neg/cum_pos dev [N]; color_mask dev uint8 [N,3] or NULL;
 * color_weight host[3] or NULL.  start0/end0 may be NULL. */
int evd_event_loss_reduce(const evd_crf* crf_ev, int skip_learn, int add_bii_feat, int tonemap_only,
                          const float* start, const float* end, const float* start0, const float* end0,
                          const float* cum_neg, const float* cum_pos, float thr_neg, float thr_pos,
                          const unsigned char* color_mask, const float* color_weight, long N,
                          float* partial, void* stream);

/* Backward of evd_event_loss_reduce: gradients of  g_fine * partial[0] + g_coarse * partial[1]  w.r.t. the colour inputs
 * (d_start, d_end, d_start0, d_end0 dev [N,3]; the *0 pair may be NULL) and w.r.t. the learnable event-CRF parameters
 * (d_params dev [evd_crf_param_count()] or NULL; layout: linear.0.weight as [16][8] rows zero-padded from 1 + extra_features,
 * linear.0.bias [16], linear.2.weight [16][16], linear.2.bias, linear.4.weight [16][16], linear.4.bias, linear.6.weight [16],
 * linear.6.bias [1]).  d_params is overwritten. */
int evd_crf_param_count(void);
/* a learn CRF's parameters to / from a HOST array of evd_crf_param_count() floats in that layout (the handle keeps them on the host:
 * they travel as a kernel argument); load is what a loop that trains the event-CRF calls after optimizer.step() */
int evd_crf_get_params(const evd_crf* crf, float* host_params);
int evd_crf_load_params(evd_crf* crf, const float* host_params);
int evd_event_loss_bwd(const evd_crf* crf_ev, int skip_learn, int add_bii_feat, int tonemap_only,
                       const float* start, const float* end, const float* start0, const float* end0,
                       const float* cum_neg, const float* cum_pos, float thr_neg, float thr_pos,
                       const unsigned char* color_mask, const float* color_weight, long N, float g_fine, float g_coarse,
                       float* d_start, float* d_end, float* d_start0, float* d_end0, float* d_params, void* stream);
/* the same with (g_fine, g_coarse) = g_partial_dev[0], [1] read from DEVICE memory */
int evd_event_loss_bwd_dev(const evd_crf* crf_ev, int skip_learn, int add_bii_feat, int tonemap_only,
                           const float* start, const float* end, const float* start0, const float* end0,
                           const float* cum_neg, const float* cum_pos, float thr_neg, float thr_pos,
                           const unsigned char* color_mask, const float* color_weight, long N, const float* g_partial_dev,
                           float* d_start, float* d_end, float* d_start0, float* d_end0, float* d_params, void* stream);

/* AdaptiveWeightProposal.feature_integration, networks/dpnerf/awp.py:49-77 (the compositing scan of the AWP consumer of
 * the path's per-sample features): feat dev [N,S,C] (N = rays x sub-exposures; every channel is its own density),
 * z dev [N,S], rays_d dev [N,3] -> out dev [N,C].  Restated as written: the last sample gets alpha 0 (awp.py:67) and the
 * cumprod of awp.py:69-73 runs along the channel axis of the previous sample's row. */
int evd_awp_feature_integration(const float* feat, const float* z, const float* rays_d, long N, int S, int C, float* out, void* stream);
/* Its backward (what torch.autograd does behind awp.py:98-104 during training, run_nerf.py:593-601): d out dev [N,C] -> d feat dev
 * [N,S,C]; d z dev [N,S] and d rays_d dev [N,3] where wanted (null: skipped; the distances are (z[s+1] - z[s]) |rays_d|, awp.py:61-63). */
int evd_awp_feature_integration_bwd(const float* feat, const float* z, const float* rays_d, const float* d_out, long N, int S, int C,
                                    float* d_feat, float* d_z, float* d_rays_d, void* stream);

/* MotionAggregationModule / CorrelationModule, the per-sample part (networks/dpnerf/mam.py:72-74: self.linear on x_local = h_local
 * [R P, S, 64]; :29-33: line_conv_att, softmax over the samples (dim -1) and over the sub-exposures (dim -2), the two weighted sums).
 * The linear map commutes with the softmax-weighted sums and a constant leaves a softmax unchanged, so with u = W^T v dev [64]
 * (W = MAM.linear.weight [32,64], v = Corr.line_conv_att.weight [32]):  logit = u . h_local;  alpha = softmax_s, beta = softmax_p;
 * h_inter dev [R,P,64] = sum_s alpha h_local, h_intra dev [R,S,64] = sum_p beta h_local -- the caller applies W, b to those
 * (curver_inter = W h_inter + b, curves_intra = W h_intra + b, mam.py:31-32).  alpha, beta dev [R,P,S] are kept for the backward.
 * C must be 64 (the embedding's width), P <= 16, S <= 512. */
int evd_mam_local_forward(const float* h_local, const float* u, long R, int P, int S, int C, float* h_inter, float* h_intra, float* alpha,
                          float* beta, void* stream);
/* Its backward (torch.autograd behind mam.py:29-33,72-74 in training, run_nerf.py:593-601): d h_inter dev [R,P,64], d h_intra dev
 * [R,S,64] -> d h_local dev [R P, S, 64] (accumulate = 0: written; != 0: ADDED to what is there -- h_local has a second consumer, the
 * feature integration, whose backward writes the buffer first) and d u as per-ray partials dev [R,64] (the caller sums them).
 * d_h_absmax (optional): dev word, set to 0 by this entry (on the stream) and raised to the float bits of max |d h_local| as written here (the loss scale the
 * embedding's backward needs: saves it a pass over the tensor). */
int evd_mam_local_backward(const float* h_local, const float* u, const float* alpha, const float* beta, const float* h_inter,
                           const float* h_intra, const float* d_inter, const float* d_intra, long R, int P, int S, int C, float* d_h_local,
                           float* d_u_partial, int accumulate, unsigned* d_h_absmax, void* stream);

/* The PER-RAY remainder of the adaptive weight proposal as kernels: networks/dpnerf/awp.py:89-95 (direction encoding of the first
 * sub-exposure's normalised ray direction, concatenated behind view_feature), :104-109 (motion_feature_embed_layer: n_mot x Linear + ReLU on
 * [integrated features | view_embedded]), networks/dpnerf/mam.py:35-53 (CorrelationModule.forward behind its per-sample part: conva /
 * convb / convc, the two softmax(bmm) attention maps over the P sub-exposures and the S samples, convn / convl, convd = Conv1d +
 * BatchNorm1d, residual, leaky_relu 0.2) and awp.py:112-115 (mean over P, w_linear, sigmoid, normalisation) -- in the reference ~100 small
 * launches each way.  Two launches forward (the BatchNorm statistics are over ALL rays: per-workgroup partial sums in the first, folded by
 * the second), three backward.  Inputs per ray: h dev [R,P,64] (evd_awp_feature_integration's output), view_feature dev [R,VF] (NULL when
 * VF = 0), rays_d dev [R P,3], h_inter dev [R,P,64] / h_intra dev [R,S,64] (evd_mam_local_forward's outputs; MAM.linear is applied here).
 * Built for W_sam 64, W_mot 32 (kernel_awp_sam_emb_width / kernel_awp_mot_emb_width of the shipped configs), n_mot <= 4, P <= 16,
 * dir_freqs 0..4 (get_embedder(ray_dir_freq): [d, sin(2^k d), cos(2^k d)...], 3 + 6 dir_freqs columns; -1: no direction columns), VF <= 64,
 * and S as far as the per-ray working set fits the 160 KiB LDS (S <= 128 for the backward at P = 10); EVD_E_INVALID otherwise.
 *
 * params: HOST array of evd_awp_tail_num_params(n_mot) DEVICE pointers, float32, nn.Module layouts ([out, in]):
 *   motion_feature_embed_layer.{l}.weight, .bias (l = 0..n_mot-1; layer 0 is [32, 64 + VF + 3 + 6 dir_freqs]),  MAM.linear.weight [32,64],
 *   .bias,  Corr.conva / convb / convc .weight [16,32],  Corr.convn / convl .weight [16,16],  Corr.convd.0.weight [32,32],
 *   Corr.convd.1.weight, .bias [32],  w_linear.weight [P,32], .bias [P].
 * d_params (backward): ONE flat dev float32 buffer of evd_awp_tail_param_count elements, the same tensors in the same order.
 * BatchNorm: training != 0 normalises with the batch statistics (biased variance) and, when bn_running_mean / _var are given, blends the
 * batch mean / UNBIASED variance into them with bn_momentum and adds 1 to *bn_num_batches (int64, may be NULL); training == 0 uses the
 * running estimates.  saved_y, saved_xg dev [R,P,32] and saved_stats dev [64] (mean, 1/sqrt(var + eps)) are kept for the backward;
 * saved_rays dev [R, evd_awp_tail_saved_floats(d)] (optional in both calls) takes every ray's forward state -- 55 KB per ray at P = 10,
 * S = 128 -- so that the backward does not run the forward a second time (measured: a third of its time).
 * workspace: evd_awp_tail_workspace_bytes(d, R, backward) bytes, any alignment; fewer -> EVD_E_WORKSPACE, nothing is written.  The size
 * queries return -1 (evd_awp_tail_param_count, _saved_floats) / 0 (_workspace_bytes) for a descriptor outside the ranges above. */
typedef struct {
    int P, S, VF, dir_freqs, n_mot, training;
    float bn_eps, bn_momentum;
} evd_awp_tail_desc;
int evd_awp_tail_num_params(int n_mot);
long evd_awp_tail_param_count(const evd_awp_tail_desc* d);
size_t evd_awp_tail_workspace_bytes(const evd_awp_tail_desc* d, long R, int backward);
long evd_awp_tail_saved_floats(const evd_awp_tail_desc* d);
int evd_awp_tail_forward(const evd_awp_tail_desc* d, const float* const* params, const float* h, const float* view_feature,
                         const float* rays_d, const float* h_inter, const float* h_intra, long R, float* bn_running_mean,
                         float* bn_running_var, long long* bn_num_batches, float* out, float* saved_y, float* saved_xg, float* saved_stats,
                         float* saved_rays, void* workspace, size_t workspace_bytes, void* stream);
/* d_out dev [R,P] -> d_h dev [R,P,64], d_view_feature dev [R,VF] (NULL when VF = 0), d_rays_d dev [R P,3] (rows other than a ray's first
 * are written as zeros), d_h_inter dev [R,P,64], d_h_intra dev [R,S,64], d_params (above); all written, not accumulated. */
int evd_awp_tail_backward(const evd_awp_tail_desc* d, const float* const* params, const float* h, const float* view_feature,
                          const float* rays_d, const float* h_inter, const float* h_intra, long R, const float* saved_y,
                          const float* saved_xg, const float* saved_stats, const float* saved_rays, const float* d_out, float* d_h,
                          float* d_view_feature,
                          float* d_rays_d, float* d_h_inter, float* d_h_intra, float* d_params, void* workspace, size_t workspace_bytes,
                          void* stream);

/* The backward of h_local's two consumers in one launch -- evd_awp_feature_integration_bwd (awp.py:49-77; feat = h_local, N = R P rows,
 * d_integrated dev [R P, 64] = d out) and evd_mam_local_backward (above) --: h_local is read once and d h_local dev [R P, S, 64] written
 * once with the SUM of both shares; d_z dev [R P, S] and d_rays_d dev [R P, 3] (the integration's; null = not wanted), d_u_partial dev
 * [R, 64], d_h_absmax as in evd_mam_local_backward.  C must be 64, P <= 16, S <= 512. */
int evd_awp_local_consumers_backward(const float* h_local, const float* u, const float* alpha, const float* beta, const float* h_inter,
                                     const float* h_intra, const float* d_inter, const float* d_intra, const float* z, const float* rays_d,
                                     const float* d_integrated, long R, int P, int S, int C, float* d_h_local, float* d_u_partial, float* d_z,
                                     float* d_rays_d, unsigned* d_h_absmax, void* stream);

/* AdaptiveWeightProposal.sample_feature_embed_layer (networks/dpnerf/awp.py:36-37: D_sam x nn.Linear; :98-100: each followed by ReLU)
 * fused into one MFMA kernel that reads the fine level's geo features WHERE THEY ALREADY ARE: the reference writes them as
 * depth_feature [R P, S, 128] float32 (renderer.py:253-256) and runs four torch Linear + ReLU passes over it (:314); here the
 * training forward of the fine level keeps the geo features as MFMA fragments for its own backward (evd_voxel_mlp_train's store),
 * evd_awp_embed_forward reads those fragments and writes only h_local dev [n, W_sam] float32 -- the tensor awp.py:102
 * (feature_integration) and :113 (the MAM) consume.  Built for input_ch 128, W_sam 64, D_sam 4 (fine_geo_feat_dim,
 * kernel_awp_sam_emb_width / _depth of the shipped configs; EVD_E_INVALID otherwise), EVD_PREC_F16 / EVD_PREC_BF16.
 *   weights[l] host [W_sam, in_l] / biases[l] host [W_sam]: sample_feature_embed_layer.l.{weight,bias}
 *   evd_awp_embed_load_params: flat dev float32 arena W0, b0, W1, b1, ... (evd_awp_embed_param_count elements) -> every stream
 *   evd_awp_embed_forward: geo features EITHER as geo_rows dev [n,128] float32 OR as (fine, fine_store) = the fine level and the
 *     store its evd_voxel_mlp_train filled for the same n = R*S samples.  store (NULL: inference) keeps the activations for
 *     evd_awp_embed_backward (evd_awp_embed_store_bytes).
 *   evd_awp_embed_backward: d_h_local dev [n, W_sam] (d_h_absmax: dev word holding the float bits of max |d_h_local| when the producer
 *     took it -- evd_mam_local_backward does --, NULL = a pass over d_h_local finds it) -> parameter gradients (overwritten; NULL = not wanted) and the geo features'
 *     gradient, left as fragments in `store` for evd_voxel_mlp_backward(awp_store = store) and, where wanted, written as
 *     d_geo_rows dev [n,128] float32 (NULL = not wanted). */
typedef struct evd_awp_embed evd_awp_embed;
typedef struct { float *w[4], *b[4]; } evd_awp_embed_grads;
int evd_awp_embed_create(const float* const* weights, const float* const* biases, int input_ch, int width, int depth, evd_awp_embed** out);
void evd_awp_embed_destroy(evd_awp_embed* a);
long evd_awp_embed_param_count(const evd_awp_embed* a);
int evd_awp_embed_load_params(evd_awp_embed* a, const float* params, void* stream);
size_t evd_awp_embed_store_bytes(const evd_awp_embed* a, long nsamp);
size_t evd_awp_embed_backward_workspace_bytes(void);
int evd_awp_embed_forward(const evd_awp_embed* a, int precision, const float* geo_rows, const evd_voxel* fine, const void* fine_store,
                          size_t fine_store_bytes, long nsamp, float* h_local, void* store, size_t store_bytes, void* stream);
int evd_awp_embed_backward(const evd_awp_embed* a, int precision, const float* d_h_local, long nsamp, void* store, size_t store_bytes,
                           const evd_awp_embed_grads* grads, float* d_geo_rows, const unsigned* d_h_absmax, void* workspace,
                           size_t workspace_bytes, void* stream);

/* The same sample embedding on FLOAT32 ROWS, for the inputs of mode='nerf': run_nerf.py:223 builds the proposal with input_ch = netwidth
 * and the renderer hands it the NeRF network's per-sample feature (renderer.py:238-257).  input_ch 64 / 128 / 256, W_sam 64, D_sam 1..8
 * (EVD_E_INVALID otherwise).  One launch per layer: out[s, m] = relu(b[m] + sum_k X[s, k] W[m, k]) in exact float32 on the matrix cores,
 * k ascending; every layer's output rows are kept in `store` (evd_awp_embed_f32_store_bytes; required).  The backward runs the per-layer
 * wgrad / dgrad launches of the generic NeRF training path (evd_nerf_mlp_backward): no atomics, the same bits on every call.
 *   rows dev [n, input_ch] float32, rows of rows_stride floats (a multiple of 4, 16-byte aligned -- e.g. the feature plane
 *     evd_nerf_mlp_train_feature leaves in its store); the backward reads the SAME rows again.
 *   evd_awp_embed_f32_load_params: flat dev float32 arena W0, b0, W1, b1, ... (evd_awp_embed_f32_param_count elements).
 *   evd_awp_embed_f32_backward: d_h_local dev [n, 64] -> parameter gradients in nn.Linear layout (overwritten; NULL = not wanted) and
 *     d_rows dev [n, input_ch] (NULL = not wanted).  workspace: evd_awp_embed_f32_backward_workspace_bytes(). */
typedef struct evd_awp_embed_f32 evd_awp_embed_f32;
typedef struct { float *w[8], *b[8]; } evd_awp_embed_f32_grads;
int evd_awp_embed_f32_create(const float* const* weights, const float* const* biases, int input_ch, int width, int depth, evd_awp_embed_f32** out);
void evd_awp_embed_f32_destroy(evd_awp_embed_f32* a);
long evd_awp_embed_f32_param_count(const evd_awp_embed_f32* a);
int evd_awp_embed_f32_load_params(evd_awp_embed_f32* a, const float* params, void* stream);
size_t evd_awp_embed_f32_store_bytes(const evd_awp_embed_f32* a, long nsamp);
size_t evd_awp_embed_f32_backward_workspace_bytes(void);
int evd_awp_embed_f32_forward(const evd_awp_embed_f32* a, const float* rows, long rows_stride, long nsamp, float* h_local, void* store,
                              size_t store_bytes, void* stream);
int evd_awp_embed_f32_backward(const evd_awp_embed_f32* a, const float* d_h_local, const float* rows, long rows_stride, long nsamp, void* store,
                               size_t store_bytes, const evd_awp_embed_f32_grads* grads, float* d_rows, void* workspace, size_t workspace_bytes,
                               void* stream);

/* EDI prior (utils/edi.py:73-95): bii dev [steps-1, npix], blurry dev [npix] -> sharp dev [npix] */
int evd_edi_deblur(const float* blurry, const float* bii, int steps, long npix, float* sharp, void* stream);
/* brightness_increment_image with bilinear sub-pixel splat (utils/edi.py:7-70, grey events):
 * x,y dev [n] float, p dev int8 [n] -> image dev [h,w] (overwritten) */
int evd_edi_bii_image(const float* x, const float* y, const signed char* p, long n, int w, int h,
                      float c_pos, float c_neg, float* image, void* stream);
/* The whole prior table, LLFFEventsDataset.compute_edi_prior (data/loader_events.py:99-131), on the resident event tables: per image the
 * event windows between `steps` boundary timestamps, the bilinear splat of every window and the double integral.
 *   events        dev float64 [N, 4] (coordinate id, timestamp, polarity, successor: the table of evd_event_filter + the successor column),
 *                 timestamps ascending
 *   id_to_coords  dev float64 [Ncoords, 2] (x, y)
 *   boundaries    dev float64 [n_img, steps]: np.linspace(start, end, steps) of every image, made on the host in float64 (:107)
 *   images        dev float32 [n_img, h, w, 3], the blurry images     prior_out  dev float32 [n_img, h, w, 3]
 *   windows_out   dev int64 [2, n_img, steps] or NULL: left[i, j] / right[i, j] = the lower / upper bound of boundary j in the timestamp
 *                 column (torch.searchsorted side left / right, :111-112)
 *   bad_id        dev int32 [1] or NULL: set to 1 when an event's coordinate id lies outside [0, Ncoords); such an event is skipped
 * Window j of image i holds the events left[i, j] <= e < right[i, j + 1] (:119-121): an event exactly on an interior boundary counts in
 * both neighbouring windows.  Taps as evd_edi_bii_image (utils/edi.py:7-41) on the float64 coordinates, with ONE deviation: a tap with
 * xf < 0 or yf < 0 is dropped (numpy's negative index wraps it to the opposite edge in the reference); the event's other taps land.
 * The tap weights are summed as 64-bit integers in units of 2^-40 (integer atomics: the table is bit-reproducible; a pixel takes 2^23 unit
 * taps per window and polarity before overflow; a stored weight is the float64 product rounded to the nearest unit: off by <= 2^-41).
 * bii = float(pos) c_pos - float(neg) c_neg and the double integral in float32 as evd_edi_deblur; one bii feeds the three channels.
 * steps odd, 3 <= steps <= 65.  Workspace: evd_edi_prior_workspace_bytes(c, steps, h, w) = the windows of c images + their accumulator
 * planes, c (steps - 1) h w 16 bytes (11.5 MB per image at 260 x 346, steps 9); c is capped at 16 images (the figure no longer grows
 * beyond).  The entry takes any workspace >= the figure for ONE image and works through the images in chunks of as many as fit
 * (<= 16); the result does not depend on the chunk.  No device-to-host read-back; asynchronous on `stream`. */
size_t evd_edi_prior_workspace_bytes(int n_img, int steps, int h, int w);
int evd_edi_prior(const double* events, long N, const double* id_to_coords, long n_coords, const double* boundaries, const float* images,
                  int n_img, int steps, int h, int w, float c_pos, float c_neg, float* prior_out, long long* windows_out, int* bad_id,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- event preprocessing
 * compute_successor, utils/events.py:72-120 (flat_xy = True): pixel_ids dev int32 [N] (y * w + x of every event, in stream
 * order), HW = number of pixels -> successor dev int64 [N] (index of the next event at the same pixel, or the event itself),
 * num_successors dev int32 [N], latest_seen dev int64 [HW] (the pixel's first event, -1 if none), first_seen dev int64 [HW]
 * (its last event).  Bit-identical to the reference loop.  Every id must lie in [0, HW) (events.compute_successor checks it): an id outside
 * is never used as an index into latest_seen / first_seen, but the outputs are then unspecified. */
size_t evd_compute_successor_workspace_bytes(long N);
int evd_compute_successor(const int* pixel_ids, long N, long HW, long long* successor, int* num_successors,
                          long long* latest_seen, long long* first_seen, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- event batch assembly (second half)
 * EventsDataset.sample_events, data/loader_events.py:259-304: for a batch of event ids the start / end event pair, the polarity sums
 * between them and the two rays of each pair -- the reference gathers on the device, round-trips the timestamps through
 * .cpu().numpy() for the pose interpolation (:280-283) and calls get_rays_pix twice (:292-295, utils/rays.py:25-36); here ONE launch on
 * resident tables.
 *   events        dev float64 [N, ncol], the reference's augmented table (:247): column 0 = coordinate id, ncol-3 = timestamp,
 *                 ncol-2 = polarity, ncol-1 = successor index (compute_successor)
 *   id_to_coords  dev float32 [Ncoords, 2] (x, y)             id_to_color_map  dev uint8 [Ncoords, 3] or NULL (colour events)
 *   poses         dev float32 [N, 3, 4]: c2w of EVERY event at its own timestamp (the reference's interpolate_poses -- scipy Slerp +
 *                 cubic spline on the CPU, out of scope -- evaluated once per dataset instead of once per batch; 48 bytes per event)
 *   events_ids    dev int64 [n]          hops  dev int64 [n] or NULL
 *   hops == NULL: the branch of every shipped config (event_accumulate_step_range [0, 0], :272-276): end = the successor,
 *                 pos / neg = its polarity where positive / where not.
 *   hops != NULL: gather_successor (utils/events.py:221-257): hops[i] + 1 successor steps, the polarities of the visited events summed
 *                 by sign; a step that leaves [0, N) gives successor -1 and zero sums (:252-255).  The random hop counts of :265-268 are
 *                 the caller's draw.
 *   add_halfpix   the reference passes integer_coords (:292)
 * outputs (dev): rays_start / rays_end float32 [n, 3, 2] (origin, direction in the last axis, :296-297), pos_cumsum / neg_cumsum
 * float32 [n], coords_ids int64 [n], color_map uint8 [n, 3] (NULL with id_to_color_map NULL), successor int64 [n] or NULL (the end event),
 * mismatch int32 [1] or NULL: set to 1 when an end event is not on its start event's coordinate id (the reference asserts, :284), when an
 * id / successor / coordinate id (column 0, checked against n_coords = Ncoords) lies outside its table -- such an event gives zero outputs
 * --, or (track form) when an event's timestamp is not finite. */
int evd_sample_events(const double* events, long N, int ncol, const float* id_to_coords, long n_coords, const unsigned char* id_to_color_map,
                      const float* poses, const long long* events_ids, const long long* hops, long n, const float* K, int add_halfpix,
                      float* rays_start, float* rays_end, float* pos_cumsum, float* neg_cumsum, long long* coords_ids,
                      unsigned char* color_map, long long* successor, int* mismatch, void* stream);

/* ---------------------------------------------------------------- camera trajectory on the device
 * LLFFEventsDataset.interpolate_poses, data/loader_events.py:133-148: the pose of an event camera at a timestamp = scipy Slerp of the
 * key rotations + a cubic (not-a-knot) spline of the key translations (utils/data.py:34-62 _get_slerp_interpolator, built at
 * loader_events.py:175-182, queries clipped to the key range), the LLFF column change [r1, -r0, r2, t] (:137), float32, translation
 * x bd_scale (:140), then recenter_poses with the image dataset's average pose (:142-143, utils/data.py:167-183: inv(c2w) @ pose in
 * float64, stored float32).  The reference evaluates it on the CPU for every batch (scipy, .cpu().numpy() round trip at :280-283).
 * Here the HOST prepares, once per dataset, what does not depend on the query (evdeblurnerf_amd/poses.py, plain numpy): the key
 * rotations as unit quaternions (scipy's from_matrix: orthogonalised, then the largest-diagonal branch), the rotation vectors
 * log(q_i^-1 q_i+1) between neighbours, and the spline as one cubic per interval in u = (t - t_i) / (t_i+1 - t_i); the device evaluates
 * one pose per timestamp in float64 with the reference's float32 roundings at the same places.
 * --spherify (utils/data.py:189-252) is not covered: no shipped config sets it, and the reference's event path returns float64 there. */
typedef struct evd_pose_track {
    int n_keys;                 /* M >= 4 key poses (scipy's cubic interp1d needs 4) */
    const double* key_t;        /* dev [M] strictly ascending timestamps */
    const double* key_quat;     /* dev [M, 4] unit quaternions (x, y, z, w) of the key rotations */
    const double* key_rotvec;   /* dev [M-1, 3] rotation vector of q_i^-1 * q_i+1 */
    const double* trans_coef;   /* dev [M-1, 4, 3] c0..c3 of the translation on interval i, polynomial in u */
    float bd_scale;             /* loader_events.py:140 (float32 product, like the reference's in-place multiply) */
    int recenter;               /* non-zero: left-multiply by recenter_inv (loader_events.py:142-143) */
    double recenter_inv[12];    /* rows 0..2 of inv(c2w 4x4), row-major [3, 4] */
} evd_pose_track;
/* interpolate_poses(t): t dev float64 [n] -> poses dev float32 [n, 3, 4] (rows 0..2 of the reference's [n, 4, 4]; the fourth row is
 * 0 0 0 1) */
int evd_interpolate_poses(const evd_pose_track* track, const double* t, long n, float* poses, void* stream);
/* evd_sample_events with the start / end poses evaluated from the track at the events' own timestamps (column ncol-3) inside the
 * same launch, i.e. EventsDataset.sample_events as the reference runs it (loader_events.py:280-283) without a per-event pose table.
 * All other arguments as evd_sample_events. */
int evd_sample_events_track(const double* events, long N, int ncol, const float* id_to_coords, long n_coords, const unsigned char* id_to_color_map,
                            const evd_pose_track* track, const long long* events_ids, const long long* hops, long n, const float* K,
                            int add_halfpix, float* rays_start, float* rays_end, float* pos_cumsum, float* neg_cumsum, long long* coords_ids,
                            unsigned char* color_map, long long* successor, int* mismatch, void* stream);

/* ---------------------------------------------------------------- once-per-dataset event tables (last clause)
 * What LLFFEventsDataset.load_event_data (data/loader_events.py:150-257) and load_events_h5 (utils/events.py:11-69) compute on the CPU
 * from the ARRAYS of events.h5 (reading the file stays with the caller).  Data-dependent sizes are returned in device words; outputs are
 * sized for the worst case.  Mirror: evdeblurnerf_amd.events.EventTables.from_arrays.
 *
 * evd_event_coord_ids -- utils/events.py:39-66 with optimize_ids=True (what load_event_data passes, :186-188): the pixels no event
 *   rounds to (np.round, clipped; :39-42), then np.unique(return_index, return_inverse) over the float64 rows [event (x, y) ; silent
 *   pixel (x, y)] viewed as 16 raw bytes (utils/misc.py:143-149 to_flattenvoid): the ids follow the BYTE order of the little-endian pairs.
 *   x, y dev float32 [N]  ->  ev_coord_ids dev int64 [N], noev_coord_ids dev int64 [h w] (the first counts[1] valid, raster order of the
 *   silent pixels), id_to_coords dev float64 [N + h w, 2] (the first counts[0] rows valid), counts dev int64 [2] = (Ncoords, Nsilent).
 * evd_event_filter -- loader_events.py:191 (events with tmin <= t <= tmax, order kept) and :203-206 (if the smallest kept polarity is 0,
 *   zeros become -1): coord_ids int64 [N], t / p float64 [N] -> events_out dev float64 [N, 3] (id, t, p; the first *count rows valid),
 *   count dev int64 [1], bad_polarity dev int32 [1] or NULL: set when the kept polarities are not {-1, 1} afterwards (the reference asserts).
 * evd_event_color_map -- loader_events.py:208-236: id_to_color_map dev uint8 [Ncoords, 3], one-hot r / g / b of the Bayer pattern
 *   (r g / g b).  inv_mapx == NULL: integer coordinates, the colour of the pixel itself (:215-218).  Else inv_mapx / inv_mapy dev
 *   float32 [h, w] (ev_map.npz): the colour of the LAST pixel in raster order whose map entry equals the coordinate BY VALUE, as the
 *   reference's dict lookup does (:229-232): -0.0 finds 0.0 and the other way round, a NaN entry finds nothing (id_to_coords must be the
 *   table evd_event_coord_ids wrote -- it is searched in its byte order); unmapped dev int32 [1] or NULL: set when a coordinate
 *   that is not a silent pixel's (noev_coord_ids [n_noev]) got no colour (the reference asserts, :231-234). */
size_t evd_event_coord_ids_workspace_bytes(long N, int h, int w);
int evd_event_coord_ids(const float* x, const float* y, long N, int h, int w, long long* ev_coord_ids, long long* noev_coord_ids, double* id_to_coords,
                        long long* counts, void* workspace, size_t workspace_bytes, void* stream);
size_t evd_event_filter_workspace_bytes(long N);
int evd_event_filter(const long long* coord_ids, const double* t, const double* p, long N, double tmin, double tmax, double* events_out, long long* count,
                     int* bad_polarity, void* workspace, size_t workspace_bytes, void* stream);
size_t evd_event_color_map_workspace_bytes(long n_coords);
int evd_event_color_map(const double* id_to_coords, long n_coords, int h, int w, const float* inv_mapx, const float* inv_mapy, const long long* noev_coord_ids,
                        long n_noev, unsigned char* id_to_color_map, int* unmapped, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- image batch assembly (first half)
 * LLFFDataset.__getitem__, data/loader.py:325-356: a batch of flat ray ids in [0, n_img * H * W) -> image id / pixel
 * (unravel_idx_from_rayid :118-123, C order), the image's pose, the pixel's colour (and the EDI prior's colour, set_pts0_prior :110-116),
 * the pixel-centre ray (get_rays_pix on the integer pixel with add_halfpix, utils/rays.py:25-36).  One launch on the resident dataset.
 *   ray_ids dev int64 [n]; images dev float32 [n_img, H, W, 3]; pts0_images the same shape or NULL; poses dev float32 [n_img, 3, 4];
 *   K host[9].
 * outputs (dev, the keys of the reference's dict): rays float32 [n, 3, 2] (origin, direction in the last axis), rays_x / rays_y
 * float32 [n] (pixel + 0.5), images_idx int64 [n], rgbsf float32 [n, 3], poses_out float32 [n, 3, 4], rgbsf_pts0 float32 [n, 3]
 * (NULL with pts0_images NULL), invalid int32 [1] or NULL: set to 1 when an id lies outside [0, n_img * H * W) (the reference raises
 * an IndexError; such a ray is written as zeros with images_idx -1). */
int evd_image_batch(const long long* ray_ids, long n, const float* images, const float* pts0_images, const float* poses, int n_img, int H,
                    int W, const float* K, float* rays, float* rays_x, float* rays_y, long long* images_idx, float* rgbsf, float* poses_out,
                    float* rgbsf_pts0, int* invalid, void* stream);

/* The same batch with its ray ids drawn in the launch (run_nerf.py:61-68): one kernel, nothing read back.  The generator is the
 * library's own, counter-based on (seed, epoch, batch): the same triple gives the same ids bit for bit; torch's streams are not reproduced.
 *   mode 0 "random"  BatchSampler(RandomSampler) with drop_last: row j of batch b is the value at position b N + j of a keyed bijection
 *                    of [0, n_img H W) -- a 6-round Feistel network over the next power of four, round function murmur3's 32-bit
 *                    finaliser of (half ^ key(seed, epoch, round)), cycle-walked into the range.  No id twice within the epoch's
 *                    floor(n_rays / N) batches; batch must lie inside the epoch.  chosen_images / live_counts / perm are not read.
 *   mode 1 "images"  data/sampler_image_batch.py: `same` distinct images, N / same distinct unused pixels of each.  The caller chooses
 *                    the images and keeps the counts (host int[same] each: image id, pixels it has left this epoch, >= N / same);
 *                    perm is dev int32 [n_img, H W], every row a permutation of [0, H W) (any; the identity to start), whose first
 *                    live_count entries are the unused pixels.  One wavefront per image removes N / same of them by partial
 *                    Fisher-Yates into the rows' dead tails; a new epoch only resets the caller's counts.  Rows s N / same .. of the batch
 *                    belong to chosen_images[s].  assemble 0 advances perm only (to replay an epoch's draws; outputs may be NULL).
 *   outputs as evd_image_batch, plus ray_ids dev int64 [N].  rgbsf_pts0 / poses_out may be NULL. */
int evd_image_batch_draw(int mode, int assemble, long N, unsigned long long seed, long epoch, long batch, const int* chosen_images,
                         const int* live_counts, int same, int* perm, const float* images, const float* pts0_images, const float* poses,
                         int n_img, int H, int W, const float* K, long long* ray_ids, float* rays, float* rays_x, float* rays_y,
                         long long* images_idx, float* rgbsf, float* poses_out, float* rgbsf_pts0, void* stream);

/* ---------------------------------------------------------------- test-set pass: image metrics, 8-bit frames
 * compute_img_metric(im1t, im2t, 'mse' | 'psnr' | 'ssim', margin, mask), utils/metrics.py:18-100 (called at run_nerf.py:685-687,704), for a
 * whole batch in one main launch plus a fixed-order finish launch: scikit-image 0.19.2's mean_squared_error, peak_signal_noise_ratio and
 * structural_similarity(multichannel=True) with the reference's arguments.
 *   pred, target  dev float32 [B, H, W, 3], values nominally in [0, 1]; mapped clamp(2 x - 1, -1, 1) in float32 (:48-49).  Everything after
 *                 the mapping is float64 (the reference keeps float32; its SSIM then loses 1e-8 .. 4e-7 to cancellation).
 *   mask          dev float32 [B, H, W, mask_ch], mask_ch 1 or 3, or NULL (mask_ch ignored)
 *   margin_h / w  rows / columns dropped on every side: int(H * margin) + 1 and int(W * margin) + 1 for margin > 0, else 0 (:67-71).  The
 *                 region (H - 2 margin_h) x (W - 2 margin_w) is a window into the frames (no copy); borders, the SSIM crop and every
 *                 count refer to it.  A region smaller than 7 in either dimension is rejected (scikit-image raises).
 *   out           dev float64 [3 B + 3]: mse [B], psnr [B], ssim [B], then the three means over the batch (summed image by image, :100)
 * mse = mean((x - y)^2) over the region and the channels.  psnr = 10 log10(data_range^2 / mse), data_range 1 if the mapped PREDICTION (the
 * first argument) has no negative value in the region, else 2: the reference's behaviour, kept; +inf for identical images; NaN inputs
 * give NaN.  ssim: uniform 7 x 7 window, K1 0.01, K2 0.03, data_range 2, sample covariance (49 / 48),
 * S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), the mean of S over the region shrunk by 3 and over the channels.
 * With a mask: x and y are multiplied by it before mse / psnr and the minimum (zeros count toward it), 10 log10(h w / sum(mask[..., 0]))
 * is subtracted from psnr AND from mse (:83-85), and ssim = sum(S mask) / sum(mask) over the whole region and the channels, S there with
 * scipy.ndimage.uniform_filter's default border (half-sample symmetric reflect) (:90-91).
 * ONE deviation: every image is multiplied by its own mask; the reference multiplies the whole batch by every earlier image's mask
 * inside its loop (:77-78), which is the same for a batch of one or identical binary masks.
 * No floating-point atomics: workgroup partials go to the workspace (evd_img_metrics_workspace_bytes(B, H, W): 40 bytes per tile of
 * EVD_IMG_METRICS_TILE_H x EVD_IMG_METRICS_TILE_W pixels, sized for margin 0) and are summed in a fixed order; two runs give the same
 * bits and an image's values do not depend on the rest of the batch.  No read-back; asynchronous on `stream`. */
#define EVD_IMG_METRICS_TILE_H 16
#define EVD_IMG_METRICS_TILE_W 32
size_t evd_img_metrics_workspace_bytes(int B, int H, int W);
int evd_img_metrics(const float* pred, const float* target, const float* mask, int mask_ch, int B, int H, int W, int margin_h, int margin_w,
                    double* out, void* workspace, size_t workspace_bytes, void* stream);
/* to8b, utils/misc.py:6: out[i] = (uint8)(255 * clip(x[i], 0, 1)), the product in float32, truncated; NaN -> 0.  x dev float32 [n],
 * out dev uint8 [n]. */
int evd_to8b(const float* x, long n, unsigned char* out, void* stream);

/* ---------------------------------------------------------------- test-set, video and render-only passes: 8-bit pictures of frame stacks
 * The arithmetic between render_path and the image / video / logger calls (run_nerf.py:374-389, 663-679, 726-732): depth pictures, error
 * maps and the video's normalised RGB, as uint8 on the device.  Two calls per picture kind, no host synchronisation between them:
 * evd_frame_range writes (lo, hi) pairs to device memory, evd_frame_map reads them there.
 *
 * A stack is n_frames contiguous frames of per_frame VALUES.  The value v of an element comes from a tagged source:
 *   EVD_FRAME_SRC_PLAIN    v = x[i]                                             x dev float32 [n_frames * per_frame], y ignored
 *   EVD_FRAME_SRC_INVERT   v = 1 - x[i]                                         (:374, :663)
 *   EVD_FRAME_SRC_SQERR    v = (((x0 - y0)^2 + (x1 - y1)^2) + (x2 - y2)^2) / 3  x, y dev float32 [n_frames * per_frame, 3]: per_frame counts
 *                                                                               PIXELS; np.mean(-1) of a float32 [..., 3] array (:670)
 * Every step is one correctly rounded float32 operation in NumPy's order (IEEE division, no contraction), so the bytes are defined bit for
 * bit.  The scope picks the slices a range belongs to: EVD_FRAME_SCOPE_ALL one (lo, hi) for the stack, EVD_FRAME_SCOPE_FRAME one per frame.
 *
 * evd_frame_range: range dev float32 [2] (ALL) or [2 n_frames] (FRAME), (min v, max v) per slice with fminf / fmaxf: a NaN value is
 *   skipped (a slice of nothing but NaN gives (+inf, -inf)).  Workgroup partials go to the workspace
 *   (evd_frame_workspace_bytes(n_frames, per_frame, scope); 0 for sizes the entries reject) and a finish launch folds them in a fixed
 *   order; no floating-point atomics.  The error is not stored.
 * evd_frame_map: y = subtract_lo ? (v - lo) / (hi - lo) : v / hi;  g = (uint8)(255 * clip(y, 0, 1)), truncated as evd_to8b does;
 *   out dev uint8 [n_frames * per_frame] receives g, or with lut (dev uint8 [256, 3]) out [n_frames * per_frame, 3] receives the three
 *   bytes lut[255 - g] (the table's rows in the order given; cv2.applyColorMap(255 - g, ...) with the caller's table).
 *   Two stated deviations where the reference's result is undefined: hi == 0 (hi == lo with subtract_lo) gives grey level 0 for the
 *   whole slice, and a NaN value gives grey level 0.
 * Memory bound: both read the sources once (4 or 24 bytes per value), the map writes 1 or 3 bytes.  16-byte loads and packed byte stores
 * where a slice's pointers allow it, element by element for its head and tail (and for the whole slice where they do not).
 * Asynchronous on `stream`; the sizes must satisfy 3 n_frames per_frame < 2^40. */
#define EVD_FRAME_SRC_PLAIN 0
#define EVD_FRAME_SRC_INVERT 1
#define EVD_FRAME_SRC_SQERR 2
#define EVD_FRAME_SCOPE_ALL 0
#define EVD_FRAME_SCOPE_FRAME 1
size_t evd_frame_workspace_bytes(int n_frames, long per_frame, int scope);
int evd_frame_range(const float* x, const float* y, int source, int scope, int n_frames, long per_frame, float* range, void* workspace,
                    size_t workspace_bytes, void* stream);
int evd_frame_map(const float* x, const float* y, int source, int scope, int n_frames, long per_frame, const float* range, int subtract_lo,
                  const unsigned char* lut, unsigned char* out, void* stream);
/* The bare table lookup, cv2.applyColorMap(g, table) with the caller's table: out[i, :] = lut[g[i], :].  g dev uint8 [n], lut dev uint8
 * [256, 3], out dev uint8 [n, 3]; n = 0: nothing launched. */
int evd_frame_colormap(const unsigned char* g, long n, const unsigned char* lut, unsigned char* out, void* stream);

/* LPIPS, the fourth metric of the test-set pass: compute_img_metric(im1t, im2t, 'lpips'), utils/metrics.py:92-95 (called at run_nerf.py:688),
 * i.e. networks/lpips/lpips.py LPIPS(net, version, lpips, spatial) in eval mode, float32 throughout.  Built: net = 'alex' and 'vgg' ('vgg16'),
 * version 0.1 and 0.0, with the linear heads (lpips=True) and the baseline without them (lpips=False), the spatial average (evd_lpips) and
 * the spatial map (evd_lpips_spatial).
 * The WEIGHTS ARE THE CALLER'S: torchvision's pretrained AlexNet / VGG-16 `features` (not part of the reference checkout; torchvision
 * downloads them) and the linear heads of the reference's weights/v0.1/{alex,vgg}.pth.  The library ships none and fetches nothing.
 * evd_lpips_desc / evd_lpips_create: the AlexNet backbone with heads (the reference's default LPIPS() call):
 *   conv_w[l], conv_b[l]  host float32, torchvision's features.{0,3,6,8,10}.{weight,bias}: [Cout, Cin, kh, kw] / [Cout] with
 *                         (Cout, Cin, k) = (64, 3, 11), (192, 64, 5), (384, 192, 3), (256, 384, 3), (256, 256, 3)
 *   lin[l]                host float32 [Cout of layer l]: lin{l}.model.1.weight (a 1 x 1 convolution without bias)
 *   shift, scale          the ScalingLayer's constants (lpips.py:245-252)
 * evd_lpips_net_desc / evd_lpips_create_net: any built backbone, with or without heads:
 *   net                   EVD_LPIPS_NET_ALEX (5 convolutions as above) or EVD_LPIPS_NET_VGG16: the 13 convolutions of features[0:30],
 *                         features.{0,2,5,7,10,12,14,17,19,21,24,26,28}.{weight,bias}, all 3 x 3 / pad 1, Cout = 64, 64, 128, 128, 256 x 3,
 *                         512 x 3, 512 x 3, a 2 x 2 / stride 2 floor pool in front of convolutions 2, 4, 7 and 10, taps after convolutions
 *                         1, 3, 6, 9 and 12 (relu1_2, 2_2, 3_3, 4_3, 5_3; 64, 128, 256, 512, 512 channels).  Entries past the backbone's
 *                         convolutions are not read.
 *   heads                 non-zero: lin[t] is the head of tap t (lpips=True); 0: the baseline, the plain channel sum of the squared
 *                         difference (lpips=False, lpips.py:219-223), lin is not read
 *   shift, scale          as above; version 0.0 (no scaling layer) is shift 0, scale 1, which are exact
 * Host pointers are read during a _create call only (as for every _create entry); the handle owns packed device copies ([K, Cout] with
 * K = (ky, kx, c), the layout of the implicit-GEMM kernel), remembers its backbone and is destroyed with evd_lpips_destroy.
 * evd_lpips:
 *   pred, target  dev float32 [B, H, W, 3] in (0, 1); the first convolution maps them on load, clamp(2 x - 1, -1, 1)
 *                 (utils/metrics.py:48-49), then (x - shift) / scale, and pads with zeros by predicate.  H, W >= evd_lpips_min_side(net):
 *                 the smallest side at which the backbone's last pool still has one output (EVD_LPIPS_MIN_SIDE for AlexNet's second
 *                 3 x 3 / stride 2 pool, EVD_LPIPS_VGG_MIN_SIDE for VGG's four 2 x 2 pools); 0 for an unknown backbone.
 *   out           dev float64 [6 B + 1]: the per-image values [B], their mean over the batch (summed image by image), then the per-layer
 *                 terms [B, 5]; value[b] = sum_l term[b, l], term[b, l] = mean over the layer's pixels of
 *                 sum_c lin_c (f0_c / (n0 + 1e-10) - f1_c / (n1 + 1e-10))^2 with n = sqrt(sum_c f_c^2); an all-zero feature vector gives 0.
 *   workspace     evd_lpips_model_workspace_bytes(m, B, H, W, 0) bytes (0 for a null handle and for sizes the entry rejects): two
 *                 activation buffers and the partials.  evd_lpips_workspace_bytes(B, H, W) is the same for an AlexNet handle.
 * evd_lpips_spatial (spatial=True): per tap the per-pixel distance d (the same float64 arithmetic) goes to a float64 map; every output pixel
 * reads the five maps bilinearly as nn.Upsample(size=(H, W), mode='bilinear', align_corners=False) does (lpips.py:134-136: source
 * coordinate (dst + 0.5) in / out - 0.5, clamped below at 0, the upper neighbour clamped to the last index), adds them in layer order in
 * float64 and rounds once.
 *   map           dev float32 [B, H, W]
 *   layer_maps    dev float32 [B, 5, H, W], the five upsampled maps, or null
 *   workspace     evd_lpips_model_workspace_bytes(m, B, H, W, 1) bytes: two activation buffers and the five maps
 * Predicted and target frames of the whole batch go through every layer in ONE launch (M = 2 B h w rows of the implicit GEMM on
 * v_mfma_f32_32x32x2_f32: exact float32 products).  The features are float32; the normalisation, the distance and every sum after it
 * are float64, workgroup partials summed in a fixed order without floating-point atomics: two runs give the same bits, an image's
 * value (and map) does not depend on the rest of the batch, and identical frames give exactly 0 (an all-zero map).  No allocation, no
 * host copy, no synchronisation; asynchronous on `stream`.
 * Not built: net = 'squeeze' (fire modules of 16, 32 and 48 channels, channel concatenation and ceil-mode pools fit neither the 64-column
 * tile nor the one-tap K tile), dropout in training mode, pnet_tune, any backward. */
#define EVD_LPIPS_MIN_SIDE 31
#define EVD_LPIPS_VGG_MIN_SIDE 16
#define EVD_LPIPS_LAYERS 5
#define EVD_LPIPS_MAX_CONVS 13
#define EVD_LPIPS_NET_ALEX 0
#define EVD_LPIPS_NET_VGG16 1
typedef struct evd_lpips_model evd_lpips_model;     /* opaque: backbone id, packed backbone weights, heads, scaling constants (a type
                                                      * cannot share the entry's name evd_lpips in C) */
typedef struct {
    const float *conv_w[EVD_LPIPS_LAYERS], *conv_b[EVD_LPIPS_LAYERS];
    const float* lin[EVD_LPIPS_LAYERS];
    float shift[3], scale[3];
} evd_lpips_desc;
typedef struct {
    int net, heads;
    const float *conv_w[EVD_LPIPS_MAX_CONVS], *conv_b[EVD_LPIPS_MAX_CONVS];
    const float* lin[EVD_LPIPS_LAYERS];
    float shift[3], scale[3];
} evd_lpips_net_desc;
int evd_lpips_create(const evd_lpips_desc* desc, evd_lpips_model** out);
int evd_lpips_create_net(const evd_lpips_net_desc* desc, evd_lpips_model** out);
void evd_lpips_destroy(evd_lpips_model* m);
int evd_lpips_min_side(int net);
size_t evd_lpips_workspace_bytes(int B, int H, int W);
size_t evd_lpips_model_workspace_bytes(const evd_lpips_model* m, int B, int H, int W, int spatial);
int evd_lpips(const evd_lpips_model* m, const float* pred, const float* target, int B, int H, int W, double* out, void* workspace, size_t workspace_bytes,
              void* stream);
int evd_lpips_spatial(const evd_lpips_model* m, const float* pred, const float* target, int B, int H, int W, float* map, float* layer_maps,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- optimizer step (run_nerf.py:593-613)
 * clip_grad_norm_ + torch.optim.Adam(amsgrad=False, maximize=False).step() over any number of float32 arrays in ONE launch, with the
 * hand-over to the library folded in: the new value of a parameter can be stored to a float32 and a float16 mirror in the same pass
 * (the grids of a PDRF level: evd_voxel_grid_mirrors), and the gradient just consumed can be cleared.
 *
 * A SEGMENT is one contiguous float32 array -- a parameter with its gradient and moments; `n` elements, 0 allowed; starts need only
 * 4-byte alignment (leaves are views at arbitrary element offsets of a flat tensor).  The 16-byte-aligned body of a segment moves as
 * 16-byte loads / stores where param, grad, exp_avg, exp_avg_sq and the mirrors share the parameter's phase within 16 bytes (the float16
 * mirror: within 8), head and tail -- and a segment whose arrays do not -- element by element.  The table lives in device memory
 * (uploaded by the first step), so there may be thousands of segments.
 * A GROUP is Adam's hyper-parameter set, passed by value per call (the learning rate changes every step).
 * Arithmetic per element, float32, IEEE division and square root, as torch/optim/adam.py _single_tensor_adam writes it:
 *   g = grad * clip_coef (flagged segments, max_norm > 0);  g += weight_decay * p;  m += (1 - beta1) (g - m);
 *   v = v beta2 + ((1 - beta2) g) g;  denom = sqrt(v) / sqrt(bc2) + eps;  p += (-(lr / bc1) m) / denom
 * with bc1 = 1 - beta1^t, bc2 = 1 - beta2^t, t = steps[i] + 1 evaluated on the host in float64 PER SEGMENT.
 * clip_coef = min(1, max_norm / (total_norm[0] + 1e-6)) is formed on the device from the scalar evd_grad_norm wrote
 * (torch.nn.utils.clip_grad_norm_'s float32 arithmetic; a non-finite norm propagates as it does there); the stored gradients are not scaled. */
typedef struct evd_adam evd_adam;
typedef struct {
    float* param;               /* dev [n] */
    float* exp_avg;             /* dev [n] */
    float* exp_avg_sq;          /* dev [n] */
    float* mirror_f32;          /* dev [n] or NULL: receives the new parameter value */
    void* mirror_f16;           /* dev [n] float16 or NULL: receives it rounded to nearest and saturated to +-65504 */
    long n;
    int group;                  /* index into the groups of evd_adam_step */
    int clip;                   /* counts towards evd_grad_norm and is scaled by the clip coefficient */
} evd_adam_segment;
typedef struct { double lr, beta1, beta2, eps, weight_decay; } evd_adam_group;
/* Host only: validates and copies the table (no device call; NULL param / exp_avg / exp_avg_sq with n > 0, n < 0, group outside
 * 0..ngroups-1 are EVD_E_INVALID).  nseg = 0 is allowed. */
int evd_adam_create(const evd_adam_segment* segments, int nseg, int ngroups, evd_adam** out);
void evd_adam_destroy(evd_adam* a);
/* Device scratch of evd_adam_step / evd_grad_norm: the per-call segment table (gradient pointers, step sizes) and the norm's partial sums */
size_t evd_adam_workspace_bytes(const evd_adam* a);
/* total_norm[0] (dev float32) = L2 norm over the flagged segments whose grads[i] is not NULL.  Float64 partial sums per workgroup and
 * one fixed-order finishing launch, no floating-point atomics: the same bits from call to call.  grads: HOST array of nseg device pointers. */
int evd_grad_norm(evd_adam* a, const float* const* grads, float* total_norm, void* workspace, size_t workspace_bytes, void* stream);
/* One step.  grads: HOST array of nseg device pointers; a NULL entry skips the segment (parameter, moments and step count untouched: torch's
 * `p.grad is None`).  steps: HOST array of nseg step counts BEFORE this step (the caller adds one to those it passed a gradient for).
 * groups: ngroups entries, as at creation.  max_norm > 0: clip with the DEVICE scalar total_norm (required then).  zero_grads: every
 * gradient consumed is overwritten with zeros in the same pass.  No host synchronisation and no pageable copy in the steady state: the
 * per-call table travels through pinned staging buffers the handle rotates.  nseg = 0 / all n = 0: EVD_OK, nothing launched. */
int evd_adam_step(evd_adam* a, const float* const* grads, const long* steps, const evd_adam_group* groups, int ngroups, float max_norm,
                  const float* total_norm, int zero_grads, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- measurement aid (no reference counterpart)
 * Sustained rate of back-to-back v_mfma_f32_32x32x16_bf16 issue on every SIMD of the current device, in dense
 * TFLOP/s, with constant (random_operands == 0) or random operands.  The chip clocks to its power budget, so the
 * second is the practical ceiling of any bf16/f16 MFMA kernel working on real data.  Synchronises the stream. */
int evd_probe_mfma_rate(int random_operands, int iters, double* tflops, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVDNERF_H */
