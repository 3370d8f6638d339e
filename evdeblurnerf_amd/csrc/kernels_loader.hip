// Image batch assembly on the device ("next" row f-3, first half): LLFFDataset.__getitem__, reference data/loader.py:325-356.
// The reference keeps images [n_img, H, W, 3] and poses [n_img, 3, 4] on the device and builds a batch with six indexing / stacking
// launches + get_rays_pix; here one thread per ray id does the unravel (:118-123, C order), the three gathers and the pixel-centre ray.
// Integer / gather work, a few hundred KB per batch: latency-bound, one launch is the whole optimisation.
//
// k_image_batch_draw is the same row assembly with the ray ids drawn in the launch (run_nerf.py:61-68): `random` evaluates a keyed
// bijection of [0, n_rays) at the batch's positions, `images` removes pixels from resident per-image permutations.  The library's own
// counter-based generator (mix64 / mix32 below); torch's generator streams are not reproduced.
#include "ray_math.h"

namespace evd {

// the destination arrays of a batch (the keys of the reference's dict); poses_out / rgb0 may be null
struct BatchRows {
    float *rays, *rays_x, *rays_y;
    long long* img_idx;
    float *rgb, *poses_out, *rgb0;
};

// row i of a batch from ray id `id`, which the caller has checked to lie in [0, n_img * H * W)
__device__ __forceinline__ void image_batch_row(long i, long long id, const float* __restrict__ images, const float* __restrict__ pts0,
                                                const float* __restrict__ poses, int H, int W, float k00, float hx, float k11, float hy,
                                                const BatchRows& o) {
    const long long hw = (long long)H * W;
    const long long im = id / hw, rem = id - im * hw;       // unravel_index(ray_id, (n_imgs, h, w)), loader.py:118-123
    const int y = (int)(rem / W), x = (int)(rem - (long long)y * W);
    const float* c2w = poses + im * 12;
    float p[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) p[k] = c2w[k];
    // get_rays_pix on the integer pixel (utils/rays.py:25-36): the int64 coordinate meets a float scalar -> float32 arithmetic
    const float d0 = ((float)x + hx) / k00, d1 = -((float)y + hy) / k11;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        o.rays[i * 6 + r * 2] = p[r * 4 + 3];
        o.rays[i * 6 + r * 2 + 1] = camera_ray_dir(d0, d1, p, r);
    }
    o.rays_x[i] = (float)x + 0.5f;                          // ray_x + HALF_PIX (:343-344)
    o.rays_y[i] = (float)y + 0.5f;
    o.img_idx[i] = im;
    const long long px = id * 3;                            // images[img_id, ray_y, ray_x] of a contiguous [n_img, H, W, 3] tensor
    o.rgb[i * 3] = images[px];
    o.rgb[i * 3 + 1] = images[px + 1];
    o.rgb[i * 3 + 2] = images[px + 2];
    if (o.poses_out) {
#pragma unroll
        for (int k = 0; k < 12; ++k) o.poses_out[i * 12 + k] = p[k];
    }
    if (o.rgb0) {
        o.rgb0[i * 3] = pts0[px];
        o.rgb0[i * 3 + 1] = pts0[px + 1];
        o.rgb0[i * 3 + 2] = pts0[px + 2];
    }
}

__global__ __launch_bounds__(256) void k_image_batch(const long long* __restrict__ ids, long n, const float* __restrict__ images,
                                                     const float* __restrict__ pts0, const float* __restrict__ poses, int n_img, int H, int W,
                                                     float k00, float hx, float k11, float hy, BatchRows o, int* __restrict__ invalid) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= n) return;
    const long long id = ids[i];
    const long long hw = (long long)H * W;
    if (id < 0 || id >= hw * n_img) {               // the reference's indexing raises; here zeros, image id -1 and the flag word
        if (invalid) atomicExch(invalid, 1);
        for (int k = 0; k < 6; ++k) o.rays[i * 6 + k] = 0.f;
        o.rays_x[i] = o.rays_y[i] = 0.f;
        o.img_idx[i] = -1;
        o.rgb[i * 3] = o.rgb[i * 3 + 1] = o.rgb[i * 3 + 2] = 0.f;
        if (o.poses_out) for (int k = 0; k < 12; ++k) o.poses_out[i * 12 + k] = 0.f;
        if (o.rgb0) o.rgb0[i * 3] = o.rgb0[i * 3 + 1] = o.rgb0[i * 3 + 2] = 0.f;
        return;
    }
    image_batch_row(i, id, images, pts0, poses, H, W, k00, hx, k11, hy, o);
}

// ------------------------------------------------------------------------------------------------ the draws
// splitmix64's finaliser and murmur3's: the two mixing hashes of the draw generator (host and device)
__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ unsigned mix32(unsigned h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

constexpr int kDrawRounds = 6;
constexpr int kDrawMaxSame = 64;

struct DrawArgs {
    int mode;                            // 0 random, 1 images
    int assemble;                        // 0: `images` only advances the permutations (seek replays an epoch with it)
    long N;
    // random: Feistel network on 2 * half_bits bits (the next power of four >= n_rays), cycle-walked into [0, n_rays)
    long long n_rays, first;             // first = batch * N, the batch's first position of the epoch's sequence
    int half_bits;
    unsigned key[kDrawRounds];           // one 32-bit key per round from (seed, epoch, round)
    // images: block s serves image img[s], whose permutation has live[s] pixels left; per = N / same pixels each
    int same, per;
    unsigned long long base;             // mix of (seed, epoch, batch)
    int img[kDrawMaxSame], live[kDrawMaxSame];
};

__device__ __forceinline__ unsigned long long feistel(unsigned long long v, int hb, const unsigned* key) {
    const unsigned mask = (1u << hb) - 1u;                  // hb <= 30: the entry refuses more than 2^60 rays
    unsigned l = (unsigned)(v >> hb) & mask, r = (unsigned)v & mask;
#pragma unroll
    for (int k = 0; k < kDrawRounds; ++k) {
        const unsigned t = l ^ (mix32(r ^ key[k]) & mask);
        l = r;
        r = t;
    }
    return ((unsigned long long)l << hb) | r;
}

// random: 256 lanes, one row each.  images: 64 lanes (one wavefront) per chosen image; lane 0 removes `per` pixels from the live head
// [0, live) of the image's permutation by partial Fisher-Yates (the picks end up in [live - per, live), still a permutation), then
// every lane assembles rows.
__global__ __launch_bounds__(256) void k_image_batch_draw(DrawArgs a, int* __restrict__ perm, const float* __restrict__ images,
                                                          const float* __restrict__ pts0, const float* __restrict__ poses, int H, int W,
                                                          float k00, float hx, float k11, float hy, long long* __restrict__ ray_ids,
                                                          BatchRows o) {
    if (a.mode == 0) {
        const long i = blockIdx.x * 256L + threadIdx.x;
        if (i >= a.N) return;
        unsigned long long v = feistel((unsigned long long)(a.first + i), a.half_bits, a.key);
        while (v >= (unsigned long long)a.n_rays) v = feistel(v, a.half_bits, a.key);      // a bijection of the domain: the walk returns
        ray_ids[i] = (long long)v;
        image_batch_row(i, (long long)v, images, pts0, poses, H, W, k00, hx, k11, hy, o);
        return;
    }
    const int s = blockIdx.x;
    const long long hw = (long long)H * W;
    const int im = a.img[s];
    int* p = perm + im * hw;
    const long row0 = (long)s * a.per;
    if (threadIdx.x == 0) {
        int live = a.live[s];
        const unsigned long long key = a.base ^ ((unsigned long long)(unsigned)im << 32);
        for (int k = 0; k < a.per; ++k, --live) {
            const unsigned r = (unsigned)(((mix64(key ^ (unsigned)k) >> 32) * (unsigned long long)live) >> 32);     // in [0, live)
            const int pick = p[r], last = p[live - 1];
            p[r] = last;
            p[live - 1] = pick;
            if (a.assemble) ray_ids[row0 + k] = im * hw + pick;
        }
    }
    if (!a.assemble) return;
    __syncthreads();
    for (long k = threadIdx.x; k < a.per; k += blockDim.x)
        image_batch_row(row0 + k, ray_ids[row0 + k], images, pts0, poses, H, W, k00, hx, k11, hy, o);
}

}  // namespace evd

using namespace evd;

extern "C" {

int evd_image_batch(const long long* ray_ids, long n, const float* images, const float* pts0_images, const float* poses, int n_img, int H,
                    int W, const float* K, float* rays, float* rays_x, float* rays_y, long long* images_idx, float* rgbsf, float* poses_out,
                    float* rgbsf_pts0, int* invalid, void* stream) {
    EVD_REQUIRE(n >= 0 && n_img > 0 && H > 0 && W > 0 && K, "evd_image_batch: bad arguments");
    EVD_REQUIRE(!rgbsf_pts0 || pts0_images, "evd_image_batch: rgbsf_pts0 wanted without pts0_images");
    hipStream_t st = as_stream(stream);
    if (invalid) EVD_HIP(hipMemsetAsync(invalid, 0, sizeof(int), st));
    if (n == 0) return EVD_OK;
    EVD_REQUIRE(ray_ids && images && poses && rays && rays_x && rays_y && images_idx && rgbsf, "evd_image_batch: null argument");
    // (halfpix - K[0][2]) is a Python double in the reference, rounded to float32 when it meets the tensor (utils/rays.py:28-29)
    const float hx = (float)(0.5 - (double)K[2]), hy = (float)(0.5 - (double)K[5]);
    const BatchRows o{rays, rays_x, rays_y, images_idx, rgbsf, poses_out, rgbsf_pts0};
    hipLaunchKernelGGL(k_image_batch, dim3((unsigned)cdiv(n, 256L)), dim3(256), 0, st, ray_ids, n, images, pts0_images, poses, n_img, H, W,
                       K[0], hx, K[4], hy, o, invalid);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_image_batch_draw(int mode, int assemble, long N, unsigned long long seed, long epoch, long batch, const int* chosen_images,
                         const int* live_counts, int same, int* perm, const float* images, const float* pts0_images, const float* poses,
                         int n_img, int H, int W, const float* K, long long* ray_ids, float* rays, float* rays_x, float* rays_y,
                         long long* images_idx, float* rgbsf, float* poses_out, float* rgbsf_pts0, void* stream) {
    EVD_REQUIRE(mode == 0 || mode == 1, "evd_image_batch_draw: mode %d is neither 0 (random) nor 1 (images)", mode);
    EVD_REQUIRE(N >= 1, "evd_image_batch_draw: N = %ld < 1", N);
    EVD_REQUIRE(n_img >= 1 && H > 0 && W > 0, "evd_image_batch_draw: n_img = %d, H = %d, W = %d (each must be >= 1)", n_img, H, W);
    EVD_REQUIRE(epoch >= 0 && batch >= 0, "evd_image_batch_draw: negative epoch or batch");
    EVD_REQUIRE(assemble || mode == 1, "evd_image_batch_draw: only the images mode has a state to advance without assembling");
    if (assemble) {
        EVD_REQUIRE(K && images && poses && ray_ids && rays && rays_x && rays_y && images_idx && rgbsf, "evd_image_batch_draw: null argument");
        EVD_REQUIRE(!rgbsf_pts0 || pts0_images, "evd_image_batch_draw: rgbsf_pts0 wanted without pts0_images");
    }
    const long long hw = (long long)H * W;
    DrawArgs a{};
    a.mode = mode;
    a.assemble = assemble;
    a.N = N;
    unsigned grid, block;
    if (mode == 0) {
        EVD_REQUIRE(hw <= (1ll << 60) / n_img, "evd_image_batch_draw: n_img * H * W beyond 2^60");
        a.n_rays = hw * n_img;
        EVD_REQUIRE(N <= a.n_rays && batch < a.n_rays / N, "evd_image_batch_draw: batch %ld outside the epoch of %lld batches of N = %ld", batch,
                    a.n_rays / N, N);
        a.first = (long long)batch * N;
        a.half_bits = 1;
        while (a.half_bits < 31 && (1ll << (2 * a.half_bits)) < a.n_rays) ++a.half_bits;
        const unsigned long long ke = mix64(mix64(seed) ^ (unsigned long long)epoch);
        for (int r = 0; r < kDrawRounds; ++r) a.key[r] = (unsigned)(mix64(ke ^ (0x72616E64ull + r)) >> 32);
        grid = (unsigned)cdiv(N, 256L);
        block = 256;
    } else {
        EVD_REQUIRE(same >= 1 && same <= kDrawMaxSame && same <= n_img, "evd_image_batch_draw: same_imgs_size = %d outside [1, min(n_img, %d)]", same,
                    kDrawMaxSame);
        EVD_REQUIRE(N % same == 0, "evd_image_batch_draw: N = %ld is not divisible by same_imgs_size = %d", N, same);
        EVD_REQUIRE(hw <= 0x7FFFFFFFll && N / same <= hw, "evd_image_batch_draw: H * W beyond int32 or fewer than N / same_imgs_size pixels per image");
        EVD_REQUIRE(chosen_images && live_counts && perm, "evd_image_batch_draw: null argument (chosen_images, live_counts, perm)");
        a.same = same;
        a.per = (int)(N / same);
        for (int s = 0; s < same; ++s) {
            EVD_REQUIRE(chosen_images[s] >= 0 && chosen_images[s] < n_img, "evd_image_batch_draw: chosen image %d outside [0, %d)", chosen_images[s], n_img);
            EVD_REQUIRE(live_counts[s] >= a.per && live_counts[s] <= hw, "evd_image_batch_draw: image %d has %d live pixels, %d wanted of %lld",
                        chosen_images[s], live_counts[s], a.per, hw);
            for (int t = 0; t < s; ++t) EVD_REQUIRE(chosen_images[t] != chosen_images[s], "evd_image_batch_draw: image %d chosen twice", chosen_images[s]);
            a.img[s] = chosen_images[s];
            a.live[s] = live_counts[s];
        }
        a.base = mix64(mix64(mix64(seed ^ 0x696D6167ull) ^ (unsigned long long)epoch) ^ (unsigned long long)batch);
        grid = (unsigned)same;
        block = 64;
    }
    // (halfpix - K[0][2]) rounded to float32 as in evd_image_batch
    const float hx = K ? (float)(0.5 - (double)K[2]) : 0.f, hy = K ? (float)(0.5 - (double)K[5]) : 0.f;
    const BatchRows o{rays, rays_x, rays_y, images_idx, rgbsf, poses_out, rgbsf_pts0};
    hipLaunchKernelGGL(k_image_batch_draw, dim3(grid), dim3(block), 0, as_stream(stream), a, perm, images, pts0_images, poses, H, W,
                       K ? K[0] : 1.f, hx, K ? K[4] : 1.f, hy, ray_ids, o);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // extern "C"
