// The line taps of the tri-plane scatter, and the hybrid scatter that evd_voxel_sample_bwd_ws / _prec run (reference: the backward of
// F.grid_sample in VoxelNeRFBase.compute_appfeature, networks/pdrf/voxnerf.py:132-151, under run_nerf.py:593-601).
//
// The direct kernel (kernel_voxel_sample_bwd.hip k_voxel_sample_bwd<false>) issues 576 float atomics per sample; they run at the L2's rate of one
// dword per clock and channel (~250 G adds/s).  In the hybrid form the plane taps stay direct float atomics (k_voxel_sample_bwd_w, or
// k_voxel_sample_bwd<true> for the shapes the wavefront-autonomous kernel is not built for); the line taps -- a third of the requests, onto
// <= 586 cells -- are left as one row of per-channel contributions per sample plus the tap records, and k_scatter_lines adds them through
// LDS with 64-bit fixed-point accumulators: 1.19 -> 0.90 ms at 2^19 fine-level samples, 1.50 -> 1.10 ms at 655 k coarse-level samples,
// same sums to 1.2e-6.  (A sort + LDS-tile form for the plane taps as well was twice as slow as the direct kernel, 2.99 against
// 1.43 ms: profiles/r02_scatter_*.)
#include "evd_common.h"
#include "voxel.h"

namespace evd {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int SC_NT = 512, SC_LCH = 2048, SC_LDS_MAX = 150 * 1024;

struct LineJob {
    float* grad;
    int C, Lp, coff, comp, c_lo, cg;        // channels [c_lo, c_lo + cg) of component comp
};
struct LineJobs { LineJob j[12]; };

// The line taps.  A workgroup keeps a cg-channel slice of a WHOLE line gradient (<= 586 cells) in LDS for SC_LCH samples and adds
// it to the gradient once.  The LDS accumulators are 64-bit FIXED POINT, not float: ds_add_f32 executes at ~0.4 lane-operations per
// clock and CU on this chip (100 M of them took 445 us here -- no faster than the global float atomics they were to replace), integer
// LDS atomics run 6 x faster.  The scale is a power of two chosen per workgroup from the largest contribution of its chunk
// (max |row| 2^k < 2^49, at most 2^13 terms per accumulator: no overflow), so a float32 contribution converts EXACTLY unless it is
// below 2^-49 of the chunk's maximum: the sums are more accurate than float32 atomics, and deterministic inside the workgroup.
// gmax (optional): the float bits of max |rows_l| over ALL samples, taken by the kernel that wrote the rows: the fixed-point scale is then that
// one instead of this chunk's own maximum, and the chunk's rows are read once (123 -> 89 us per 2^19 samples)
// Workgroup order (round 6): a job reads a 64-byte (16-channel) slice of every row of its chunk, i.e. HALF of each 128-byte line it pulls;
// the other half belongs to the next job of the same chunk.  With the jobs as the grid's y dimension the six jobs of a chunk ran a whole
// x sweep apart and every line came from HBM / the Infinity Cache twice (the kernel moved ~2 GB of rows per iteration at 3.0 TB/s while its LDS
// atomics, ablated, were worth 12 %).  Now the grid is one-dimensional and decoded so that ALL jobs of a chunk are neighbours in time ON ONE XCD
// (workgroup ids go round-robin over the 8 XCDs: id % 8): id = ((chunk / 8) nj + job) 8 + chunk % 8 -- the first job's miss fills that
// XCD's L2 for the others (and the four z-line jobs share their tap records the same way): 769 -> 684 us per iteration; the jobs of a chunk on
// consecutive ids, i.e. on different XCDs: 798 (profiles/r06_scatter_lines_order_ab.log).  Chunks of 4096 / 8192 samples (a quarter of the
// end-of-chunk atomics) change nothing (r06_scatter_lines_chunk_ab.log).
__global__ __launch_bounds__(SC_NT) void k_scatter_lines(const LineJobs jobs, const float* __restrict__ rows_l, const LTap* __restrict__ ltap, long n, int ctot,
                                                       const unsigned* __restrict__ gmax, int nj) {
    const int q = blockIdx.x >> 3, job = q % nj, chunk = (q / nj) * 8 + (blockIdx.x & 7);
    if ((long)chunk * SC_LCH >= n) return;
    const LineJob jb = jobs.j[job];
    if (!jb.grad) return;
    extern __shared__ __attribute__((aligned(16))) unsigned long long lacc[];       // [Lp][cg]
    __shared__ float wmax[SC_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cg = jb.cg, total = jb.Lp * cg;
    for (int o = tid; o < total; o += SC_NT) lacc[o] = 0ull;
    const long base = (long)chunk * SC_LCH, end = base + SC_LCH < n ? base + SC_LCH : n;
    // a lane owns 4 consecutive channels of a sample (one 16-byte load): cg / 4 lanes per sample
    const int lps = cg >> 2, spw = 64 / lps, c4 = (lane % lps) * 4, sub = lane / lps, step = (SC_NT / 64) * spw;
    const float* col = rows_l + jb.coff + jb.c_lo + c4;
    float m = gmax ? __uint_as_float(*gmax) : 0.f;
    for (long s = base + wave * spw + sub; s < (gmax ? base : end); s += step) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(col + s * ctot);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float a = fabsf(v[k]);
            m = a != a ? __builtin_huge_valf() : fmaxf(m, a);          // (fmaxf drops NaNs: they are recorded as +inf)
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) wmax[wave] = m;
    __syncthreads();
    m = 0.f;
#pragma unroll
    for (int w = 0; w < SC_NT / 64; ++w) m = fmaxf(m, wmax[w]);
    if (m > 3.0e38f) {                                  // a NaN / Inf contribution: no fixed-point scale exists -- add this chunk's taps
        for (long s = base + wave * spw + sub; s < end; s += step) {       // directly, so that the gradient shows it as the direct form would
            const LTap t = ltap[s * 3 + jb.comp];
            const f32x4 v = *reinterpret_cast<const f32x4*>(col + s * ctot);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (t.w0 != 0.f) unsafeAtomicAdd(jb.grad + (long)t.c0 * jb.C + jb.c_lo + c4 + k, t.w0 * v[k]);
                if (t.w1 != 0.f) unsafeAtomicAdd(jb.grad + (long)t.c1 * jb.C + jb.c_lo + c4 + k, t.w1 * v[k]);
            }
        }
        return;
    }
    if (!(m > 0.f)) return;                             // nothing to add
    int e;
    (void)frexpf(m, &e);                                // m = f 2^e, f in [0.5, 1)
    if (e < -77) e = -77;                               // 2^(49 - e) must stay a finite float32: a chunk whose maximum is below 2^-78 keeps the scale 2^126
                                                        // (its contributions are then resolved to 2^-126 instead of 2^-49 of the maximum: far below float32 atomics)
    const float up = ldexpf(1.f, 49 - e);               // |w v| up <= 2^49
    constexpr int UN = 4;
    for (long s0 = base + wave * spw + sub; s0 < end; s0 += UN * step) {
        LTap t[UN];
        f32x4 v[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const long s = s0 + u * step;
            if (s < end) {
                t[u] = ltap[s * 3 + jb.comp];
                v[u] = *reinterpret_cast<const f32x4*>(col + s * ctot);
            } else {
                t[u].c0 = t[u].c1 = 0; t[u].w0 = t[u].w1 = 0.f; v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            if (t[u].w0 != 0.f) {
#pragma unroll
                for (int k = 0; k < 4; ++k) atomicAdd(&lacc[t[u].c0 * cg + c4 + k], (unsigned long long)__float2ll_rn((t[u].w0 * v[u][k]) * up));
            }
            if (t[u].w1 != 0.f) {
#pragma unroll
                for (int k = 0; k < 4; ++k) atomicAdd(&lacc[t[u].c1 * cg + c4 + k], (unsigned long long)__float2ll_rn((t[u].w1 * v[u][k]) * up));
            }
        }
    }
    __syncthreads();
    const double down = ldexp(1.0, e - 49);
    for (int o = tid; o < total; o += SC_NT) {
        const long long a = (long long)lacc[o];
        if (a != 0) unsafeAtomicAdd(jb.grad + (long)(o / cg) * jb.C + jb.c_lo + (o % cg), (float)((double)a * down));
    }
}

static const int kM0[3] = {0, 0, 1}, kM1[3] = {1, 2, 2}, kV[3] = {2, 1, 0};

static int launch_lines(const GridParams& g, const GridGrads& gg, const float* rows_l, const LTap* ltap, long n, hipStream_t st, const unsigned* gmax = nullptr) {
    const int ctot = g.n_comp[0] + g.n_comp[1] + g.n_comp[2];
    LineJobs lj;
    int nj = 0, coff = 0;
    size_t llds = 0;
    for (int i = 0; i < 3; ++i) {
        const int C = g.n_comp[i], Lp = g.grid[kV[i]];
        int cg = 16;                                      // 64-bit accumulators: 16-channel slices (586 cells: 75 KB)
        while (cg > 4 && (size_t)Lp * cg * 8 > (size_t)SC_LDS_MAX / 2) cg /= 2;
        for (int c_lo = 0; c_lo < C && gg.line[i]; c_lo += cg) {
            if (nj >= 12) return fail(EVD_E_INVALID, "evd_voxel_sample_bwd: too many line channel groups");
            LineJob& j = lj.j[nj++];
            j.grad = gg.line[i]; j.C = C; j.Lp = Lp; j.coff = coff; j.comp = i; j.c_lo = c_lo; j.cg = cg;
            const size_t l = (size_t)Lp * cg * 8;
            llds = l > llds ? l : llds;
        }
        coff += C;
    }
    for (int k = nj; k < 12; ++k) lj.j[k].grad = nullptr;
    if (nj) {
        EVD_SET_MAX_LDS(k_scatter_lines, (size_t)SC_LDS_MAX);
        const long chunks8 = cdiv(cdiv(n, (long)SC_LCH), 8L) * 8;
        hipLaunchKernelGGL(k_scatter_lines, dim3((unsigned)(chunks8 * nj)), dim3(SC_NT), llds, st, lj, rows_l, ltap, n, ctot, gmax, nj);
        EVD_LAUNCH_CHECK();
    }
    return EVD_OK;
}

// The hybrid form needs channel counts k_scatter_lines' lane mapping handles and lines whose 16-channel slices fit LDS.  (The 16-bit bound
// on the plane sizes came with the removed sort form's tap records; it stays so that the shapes which take this path do not change.)
bool voxel_scatter_hybrid_ok(const GridParams& g, long n) {
    for (int i = 0; i < 3; ++i) {
        const int C = g.n_comp[i];
        if (C != 16 && C != 32 && C != 64) return false;
        const int Wp = g.grid[kM0[i]], Hp = g.grid[kM1[i]], Lp = g.grid[kV[i]];
        if (Wp > 65535 || Hp > 65535 || (size_t)Lp * 16 * 8 > (size_t)SC_LDS_MAX / 2) return false;      // a 16-channel slice of a whole line (64-bit accumulators) must fit half the LDS
    }
    return n > 0 && n < (1L << 31);
}

// rows_l [n, ctot] | ltap [n, 3] | the max |line row| word (k_scatter_lines' fixed-point scale)
struct HybridWs { float* rows_l; LTap* ltap; unsigned* lmax; };
static const size_t HYBRID_WS_SLACK = 256;      // alignment slack for an unaligned caller pointer
static size_t hybrid_layout(const GridParams& g, long n, void* workspace, HybridWs* L) {
    const size_t ctot = (size_t)(g.n_comp[0] + g.n_comp[1] + g.n_comp[2]);
    Workspace ws(workspace);
    L->rows_l = ws.take<float>((size_t)n * ctot); L->ltap = ws.take<LTap>((size_t)n * 3); L->lmax = ws.take<unsigned>(1);
    return ws.used() + HYBRID_WS_SLACK;
}
size_t voxel_scatter_hybrid_workspace_bytes(const GridParams& g, long n) { HybridWs L; return n <= 0 ? 0 : hybrid_layout(g, n, nullptr, &L); }

int launch_voxel_sample_bwd_hybrid(const GridParams& g, const float* pts, long n, const float* d_out, int d_stride, int d_col, const GridGrads& gg,
                                   float* d_pts, void* workspace, size_t workspace_bytes, hipStream_t st, bool half_grids) {
    HybridWs L;
    const size_t need = hybrid_layout(g, n, workspace, &L);
    if (workspace_bytes < need) return fail(EVD_E_WORKSPACE, "evd_voxel_sample_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    float* rows_l = L.rows_l; LTap* ltap = L.ltap;
    if (!voxel_sample_bwd_w_ok(g)) {
        int rc = launch_voxel_sample_bwd_planes(g, pts, n, d_out, d_stride, d_col, gg, d_pts, rows_l, ltap, st);
        if (rc) return rc;
        return launch_lines(g, gg, rows_l, ltap, n, st);
    }
    // max |line row| of the whole batch, taken by the main kernel: k_scatter_lines' scale without a pass of its own over the rows
    EVD_HIP(hipMemsetAsync(L.lmax, 0, sizeof(unsigned), st));
    int rc = launch_voxel_sample_bwd_w(g, pts, n, d_out, d_stride, d_col, gg, d_pts, rows_l, ltap, L.lmax, half_grids, st);
    if (rc) return rc;
    return launch_lines(g, gg, rows_l, ltap, n, st, L.lmax);
}

}  // namespace evd
