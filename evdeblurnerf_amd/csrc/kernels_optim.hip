// Optimizer step of run_nerf.py:593-613 on the device: gradient norm, clip, Adam, the hand-over of the new grid values to a PDRF level
// (float32 + saturated float16 mirrors) and the clearing of the consumed gradients, all segments in ONE launch (include/evdnerf.h,
// "optimizer step").
//
// Work decomposition.  A segment's elements are indexed from the 16-byte boundary at or below its parameter pointer: virtual index
// j = i + phase, phase = (address of param mod 16) / 4.  A CHUNK is 2048 consecutive virtual indices of one segment = 512 groups of four,
// two groups per lane of a 256-lane workgroup; chunk_start[] is the prefix sum of the segments' chunk counts, and a workgroup strides
// through the global chunk numbers of a capped grid, finding a chunk's segment by bisection (a few cached loads per 8 KB of parameter).
// A group that lies wholly inside the segment moves as 16-byte loads / stores when the segment's arrays share the parameter's phase; the
// groups across the head and the tail, and every group of a segment whose arrays do not, go element by element.
#include "evd_common.h"

#include <cmath>

using namespace evd;

namespace {

constexpr int kMaxGroups = 16;
constexpr int kChunk = 2048;            // virtual elements per chunk
constexpr int kGroupsPerLane = kChunk / 4 / 256;
constexpr int kStepBlocks = 2048;       // grid cap of the step (256 CUs x 8 workgroups)
constexpr int kNormBlocks = 1024;       // grid cap of the norm = number of float64 partial sums
constexpr int kSlots = 4;               // pinned staging buffers in rotation

typedef float vf4 __attribute__((ext_vector_type(4)));
typedef _Float16 vh4 __attribute__((ext_vector_type(4)));
// The arrays' addresses come out of tables in memory, where the compiler cannot see that they are global: said here, so that it emits
// global_load / global_store instead of flat ones
#define EVD_GLOBAL __attribute__((address_space(1)))
typedef EVD_GLOBAL float gf32;
typedef EVD_GLOBAL const float gcf32;
typedef EVD_GLOBAL vf4 gvf4;
typedef EVD_GLOBAL const vf4 gcvf4;
typedef EVD_GLOBAL _Float16 gf16;
typedef EVD_GLOBAL vh4 gvh4;

struct SegStatic {
    float *p, *m, *v, *mf32;
    _Float16* mf16;
    long n;
    int group, clip, phase, pad;
};
struct SegDyn {                         // what changes from call to call
    const float* g;
    float step_size_neg;                // -(lr / bias_correction1)
    float bc2_sqrt;                     // sqrt(bias_correction2)
};
struct GroupArg { float om_beta1, beta2, om_beta2, eps, wd; };
struct GroupArgs { GroupArg g[kMaxGroups]; };

// largest s with chunk_start[s] <= c (segments without chunks share their successor's start and are never returned)
__device__ __forceinline__ int find_segment(const long* __restrict__ chunk_start, int nseg, long c) {
    int lo = 0, hi = nseg;              // invariant: chunk_start[lo] <= c < chunk_start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_start[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}

struct Hyper { float om_beta1, beta2, om_beta2, eps, wd, step_size_neg, bc2_sqrt, coef; bool clip; };

// torch/optim/adam.py _single_tensor_adam, one element (ATen's lerp, addcmul and addcdiv formulas; -ffp-contract=off: no fused multiply-add)
__device__ __forceinline__ void adam_element(const Hyper& h, float& p, float g, float& m, float& v) {
    if (h.clip) g = g * h.coef;
    if (h.wd != 0.f) g = g + h.wd * p;
    const float d = g - m;
    m = h.om_beta1 < 0.5f ? m + h.om_beta1 * d : g - d * (1.f - h.om_beta1);
    v = v * h.beta2 + (h.om_beta2 * g) * g;
    const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
    p = p + (h.step_size_neg * m) / denom;
}

__device__ __forceinline__ bool same_phase(const void* a, const void* p) { return (((uintptr_t)a ^ (uintptr_t)p) & 15) == 0; }

__global__ __launch_bounds__(256) void k_adam_step(const SegStatic* __restrict__ segs, const SegDyn* __restrict__ dyn, const long* __restrict__ chunk_start,
                                                   int nseg, long total_chunks, const GroupArgs groups, float max_norm,
                                                   const float* __restrict__ total_norm, int zero_grads) {
    float coef = 1.f;
    if (max_norm > 0.f) {               // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1), float32; NaN stays NaN
        coef = (1.f / (total_norm[0] + 1e-6f)) * max_norm;
        coef = coef > 1.f ? 1.f : coef;
    }
    for (long c = blockIdx.x; c < total_chunks; c += gridDim.x) {
        const int s = find_segment(chunk_start, nseg, c);
        const SegDyn dy = dyn[s];
        if (dy.g == nullptr) continue;  // p.grad is None: parameter, moments and step count stay as they are
        const SegStatic sg = segs[s];
        const GroupArg ga = groups.g[sg.group];
        const Hyper h = {ga.om_beta1, ga.beta2, ga.om_beta2, ga.eps, ga.wd, dy.step_size_neg, dy.bc2_sqrt, coef, max_norm > 0.f && sg.clip != 0};
        const bool vec = same_phase(dy.g, sg.p) && same_phase(sg.m, sg.p) && same_phase(sg.v, sg.p) && (!sg.mf32 || same_phase(sg.mf32, sg.p)) &&
                         (!sg.mf16 || ((uintptr_t)sg.mf16 & 7) == (((uintptr_t)sg.p & 15) >> 1));
        gf32 *P = (gf32*)sg.p, *M = (gf32*)sg.m, *V = (gf32*)sg.v, *F32 = (gf32*)sg.mf32, *G = (gf32*)dy.g;
        gf16* F16 = (gf16*)sg.mf16;
        const long q0 = (c - chunk_start[s]) * (kChunk / 4) + threadIdx.x;
#pragma unroll
        for (int k = 0; k < kGroupsPerLane; ++k) {
            const long i0 = (q0 + k * 256) * 4 - sg.phase;          // first element of this group of four
            if (i0 >= sg.n || i0 + 3 < 0) continue;
            if (vec && i0 >= 0 && i0 + 3 < sg.n) {
                vf4 p = *(gcvf4*)(P + i0), m = *(gcvf4*)(M + i0), v = *(gcvf4*)(V + i0);
                const vf4 g = *(gcvf4*)(G + i0);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float pe = p[e], me = m[e], ve = v[e];
                    adam_element(h, pe, g[e], me, ve);
                    p[e] = pe; m[e] = me; v[e] = ve;
                }
                *(gvf4*)(P + i0) = p;
                __builtin_nontemporal_store(m, (gvf4*)(M + i0));
                __builtin_nontemporal_store(v, (gvf4*)(V + i0));
                if (F32) __builtin_nontemporal_store(p, (gvf4*)(F32 + i0));
                if (F16) {
                    const vh4 hh = {f16_sat(p[0]), f16_sat(p[1]), f16_sat(p[2]), f16_sat(p[3])};
                    __builtin_nontemporal_store(hh, (gvh4*)(F16 + i0));
                }
                if (zero_grads) *(gvf4*)(G + i0) = vf4{0.f, 0.f, 0.f, 0.f};
            } else {
                for (int e = 0; e < 4; ++e) {
                    const long i = i0 + e;
                    if (i < 0 || i >= sg.n) continue;
                    float pe = P[i], me = M[i], ve = V[i];
                    adam_element(h, pe, G[i], me, ve);
                    P[i] = pe;
                    __builtin_nontemporal_store(me, M + i);
                    __builtin_nontemporal_store(ve, V + i);
                    if (F32) __builtin_nontemporal_store(pe, F32 + i);
                    if (F16) __builtin_nontemporal_store(f16_sat(pe), F16 + i);
                    if (zero_grads) G[i] = 0.f;
                }
            }
        }
    }
}

// fixed-order sum of the 256 lanes' float64 values (the same tree on every call); the result is valid in lane 0
__device__ __forceinline__ double block_sum(double x, double* lds) {
    lds[threadIdx.x] = x;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) lds[threadIdx.x] += lds[threadIdx.x + w];
        __syncthreads();
    }
    return lds[0];
}

__global__ __launch_bounds__(256) void k_grad_sumsq(const SegStatic* __restrict__ segs, const SegDyn* __restrict__ dyn, const long* __restrict__ chunk_start,
                                                    int nseg, long total_chunks, double* __restrict__ partial) {
    __shared__ double lds[256];
    double acc = 0.0;
    for (long c = blockIdx.x; c < total_chunks; c += gridDim.x) {
        const int s = find_segment(chunk_start, nseg, c);
        gcf32* g = (gcf32*)dyn[s].g;
        if (g == nullptr || segs[s].clip == 0) continue;
        const long n = segs[s].n;
        const int phase = segs[s].phase;
        const bool vec = same_phase(dyn[s].g, segs[s].p);
        const long q0 = (c - chunk_start[s]) * (kChunk / 4) + threadIdx.x;
#pragma unroll
        for (int k = 0; k < kGroupsPerLane; ++k) {
            const long i0 = (q0 + k * 256) * 4 - phase;
            if (i0 >= n || i0 + 3 < 0) continue;
            if (vec && i0 >= 0 && i0 + 3 < n) {
                const vf4 x = *(gcvf4*)(g + i0);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc += (double)x[e] * (double)x[e];
            } else {
                for (int e = 0; e < 4; ++e) {
                    const long i = i0 + e;
                    if (i >= 0 && i < n) acc += (double)g[i] * (double)g[i];
                }
            }
        }
    }
    const double t = block_sum(acc, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void k_grad_norm_finish(const double* __restrict__ partial, int nblocks, float* __restrict__ total_norm) {
    __shared__ double lds[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) acc += partial[i];
    const double t = block_sum(acc, lds);
    if (threadIdx.x == 0) total_norm[0] = (float)sqrt(t);
}

size_t dyn_offset() { return (size_t)kNormBlocks * sizeof(double); }

}  // namespace

struct evd_adam {
    std::vector<SegStatic> segs;
    std::vector<long> chunk_start;          // nseg + 1
    long total_chunks = 0;
    int ngroups = 0;
    // device copies of the two tables and the pinned staging buffers of the per-call table: made by the first call that launches
    DevBuf d_segs, d_chunks;
    bool on_device = false;
    SegDyn* stage[kSlots] = {};
    hipEvent_t staged[kSlots] = {};
    bool in_flight[kSlots] = {};
    int slot = 0;
    std::mutex mu;                          // one call at a time per handle (the staging rotation)
};

namespace {

int ensure_device(evd_adam* a) {
    if (a->on_device) return EVD_OK;
    int rc = a->d_segs.upload(a->segs.data(), a->segs.size() * sizeof(SegStatic));
    if (!rc) rc = a->d_chunks.upload(a->chunk_start.data(), a->chunk_start.size() * sizeof(long));
    if (rc) return rc;
    for (int k = 0; k < kSlots; ++k) {
        EVD_HIP(hipHostMalloc((void**)&a->stage[k], a->segs.size() * sizeof(SegDyn), hipHostMallocDefault));
        EVD_HIP(hipEventCreateWithFlags(&a->staged[k], hipEventDisableTiming));
    }
    a->on_device = true;
    return EVD_OK;
}

// the next pinned buffer of the rotation, free to be written: its last copy (kSlots calls ago) has long run; the wait is the rare exception
int next_stage(evd_adam* a, SegDyn** out, int* slot) {
    const int k = a->slot;
    a->slot = (k + 1) % kSlots;
    if (a->in_flight[k] && hipEventQuery(a->staged[k]) != hipSuccess) {
        (void)hipGetLastError();            // "not ready" is an answer, not an error for the next launch check to find
        EVD_HIP(hipEventSynchronize(a->staged[k]));
    }
    a->in_flight[k] = false;
    *out = a->stage[k];
    *slot = k;
    return EVD_OK;
}

int send_stage(evd_adam* a, int slot, void* workspace, hipStream_t st) {
    EVD_HIP(hipMemcpyAsync((char*)workspace + dyn_offset(), a->stage[slot], a->segs.size() * sizeof(SegDyn), hipMemcpyHostToDevice, st));
    EVD_HIP(hipEventRecord(a->staged[slot], st));
    a->in_flight[slot] = true;
    return EVD_OK;
}

}  // namespace

extern "C" {

int evd_adam_create(const evd_adam_segment* segments, int nseg, int ngroups, evd_adam** out) {
    EVD_REQUIRE(out && nseg >= 0 && (segments || nseg == 0), "evd_adam_create: null argument");
    EVD_REQUIRE(ngroups >= 1 && ngroups <= kMaxGroups, "evd_adam_create: %d groups (1..%d)", ngroups, kMaxGroups);
    for (int i = 0; i < nseg; ++i) {
        const evd_adam_segment& s = segments[i];
        EVD_REQUIRE(s.n >= 0, "evd_adam_create: segment %d has n = %ld < 0", i, s.n);
        EVD_REQUIRE(s.group >= 0 && s.group < ngroups, "evd_adam_create: segment %d names group %d of %d", i, s.group, ngroups);
        EVD_REQUIRE(s.n == 0 || (s.param && s.exp_avg && s.exp_avg_sq), "evd_adam_create: segment %d: null param / exp_avg / exp_avg_sq", i);
        EVD_REQUIRE(((uintptr_t)s.param | (uintptr_t)s.exp_avg | (uintptr_t)s.exp_avg_sq | (uintptr_t)s.mirror_f32) % 4 == 0 && (uintptr_t)s.mirror_f16 % 2 == 0,
                    "evd_adam_create: segment %d: misaligned array", i);
    }
    evd_adam* a = new evd_adam();
    a->ngroups = ngroups;
    a->segs.resize(nseg);
    a->chunk_start.assign(nseg + 1, 0);
    for (int i = 0; i < nseg; ++i) {
        const evd_adam_segment& s = segments[i];
        const int phase = (int)(((uintptr_t)s.param & 15) / 4);
        a->segs[i] = SegStatic{s.param, s.exp_avg, s.exp_avg_sq, s.mirror_f32, (_Float16*)s.mirror_f16, s.n, s.group, s.clip ? 1 : 0, phase, 0};
        a->chunk_start[i + 1] = a->chunk_start[i] + (s.n > 0 ? cdiv(s.n + phase, (long)kChunk) : 0);
    }
    a->total_chunks = a->chunk_start[nseg];
    *out = a;
    return EVD_OK;
}

void evd_adam_destroy(evd_adam* a) {
    if (!a) return;
    for (int k = 0; k < kSlots; ++k) {
        if (a->staged[k]) (void)hipEventDestroy(a->staged[k]);
        if (a->stage[k]) (void)hipHostFree(a->stage[k]);
    }
    a->d_segs.release();
    a->d_chunks.release();
    delete a;
}

size_t evd_adam_workspace_bytes(const evd_adam* a) {
    if (!a) return 0;
    return dyn_offset() + (a->segs.size() + 1) * sizeof(SegDyn);
}

int evd_grad_norm(evd_adam* a, const float* const* grads, float* total_norm, void* workspace, size_t workspace_bytes, void* stream) {
    EVD_REQUIRE(a && total_norm, "evd_grad_norm: null argument");
    const int nseg = (int)a->segs.size();
    EVD_REQUIRE(grads || nseg == 0, "evd_grad_norm: null gradient table");
    EVD_REQUIRE(workspace && workspace_bytes >= evd_adam_workspace_bytes(a), "evd_grad_norm: workspace of %zu bytes, %zu needed", workspace_bytes,
                evd_adam_workspace_bytes(a));
    for (int i = 0; i < nseg; ++i) EVD_REQUIRE((uintptr_t)grads[i] % 4 == 0, "evd_grad_norm: gradient %d is misaligned", i);
    hipStream_t st = as_stream(stream);
    std::lock_guard<std::mutex> lock(a->mu);
    int nb = 0;
    if (a->total_chunks > 0) {
        int rc = ensure_device(a);
        if (rc) return rc;
        SegDyn* host;
        int slot;
        rc = next_stage(a, &host, &slot);
        if (rc) return rc;
        for (int i = 0; i < nseg; ++i) host[i] = SegDyn{grads[i], 0.f, 1.f};
        rc = send_stage(a, slot, workspace, st);
        if (rc) return rc;
        nb = (int)(a->total_chunks < kNormBlocks ? a->total_chunks : kNormBlocks);
        hipLaunchKernelGGL(k_grad_sumsq, dim3(nb), dim3(256), 0, st, (const SegStatic*)a->d_segs.p, (const SegDyn*)((char*)workspace + dyn_offset()),
                           (const long*)a->d_chunks.p, nseg, a->total_chunks, (double*)workspace);
        EVD_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_grad_norm_finish, dim3(1), dim3(256), 0, st, (const double*)workspace, nb, total_norm);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int evd_adam_step(evd_adam* a, const float* const* grads, const long* steps, const evd_adam_group* groups, int ngroups, float max_norm,
                  const float* total_norm, int zero_grads, void* workspace, size_t workspace_bytes, void* stream) {
    EVD_REQUIRE(a, "evd_adam_step: null handle");
    const int nseg = (int)a->segs.size();
    EVD_REQUIRE(groups && ngroups == a->ngroups, "evd_adam_step: %d groups passed, the handle was created with %d", groups ? ngroups : 0, a->ngroups);
    EVD_REQUIRE((grads && steps) || nseg == 0, "evd_adam_step: null gradient / step table");
    EVD_REQUIRE(!(max_norm > 0.f) || total_norm, "evd_adam_step: max_norm > 0 needs the device scalar evd_grad_norm wrote");
    if (a->total_chunks == 0) return EVD_OK;
    EVD_REQUIRE(workspace && workspace_bytes >= evd_adam_workspace_bytes(a), "evd_adam_step: workspace of %zu bytes, %zu needed", workspace_bytes,
                evd_adam_workspace_bytes(a));
    for (int i = 0; i < nseg; ++i)
        EVD_REQUIRE((uintptr_t)grads[i] % 4 == 0 && steps[i] >= 0, "evd_adam_step: segment %d: misaligned gradient or negative step count", i);
    GroupArgs ga = {};
    for (int k = 0; k < ngroups; ++k)   // the scalars torch forms in float64 and hands to float32 tensor ops
        ga.g[k] = GroupArg{(float)(1.0 - groups[k].beta1), (float)groups[k].beta2, (float)(1.0 - groups[k].beta2), (float)groups[k].eps, (float)groups[k].weight_decay};
    hipStream_t st = as_stream(stream);
    std::lock_guard<std::mutex> lock(a->mu);
    int rc = ensure_device(a);
    if (rc) return rc;
    SegDyn* host;
    int slot;
    rc = next_stage(a, &host, &slot);
    if (rc) return rc;
    for (int i = 0; i < nseg; ++i) {
        const evd_adam_group& g = groups[a->segs[i].group];
        const double t = (double)(steps[i] + 1);
        const double bc1 = 1.0 - std::pow(g.beta1, t), bc2 = 1.0 - std::pow(g.beta2, t);
        host[i] = SegDyn{grads[i], (float)(-(g.lr / bc1)), (float)std::pow(bc2, 0.5)};
    }
    rc = send_stage(a, slot, workspace, st);
    if (rc) return rc;
    const int nb = (int)(a->total_chunks < kStepBlocks ? a->total_chunks : kStepBlocks);
    hipLaunchKernelGGL(k_adam_step, dim3(nb), dim3(256), 0, st, (const SegStatic*)a->d_segs.p, (const SegDyn*)((char*)workspace + dyn_offset()),
                       (const long*)a->d_chunks.p, nseg, a->total_chunks, ga, max_norm, total_norm, zero_grads ? 1 : 0);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // extern "C"
