// PDRF backbone (reference networks/pdrf/voxnerf.py): the small row kernels around the tri-plane levels and the generic level network.
// The feature gather is in kernel_voxel_sample.hip, its backward in kernel_voxel_sample_bwd.hip / kernel_voxel_scatter.hip, the TV
// regulariser in kernel_voxel_tv.hip, the sample positions pts = o + d z (k_points) with the ray front end in kernels_rays.hip.
//
//   k_merge_features   the merged-sample feature rows of the c2f pass      (renderer.py:205-213), and its backward
//   k_f32_to_f16       the float16 copies of the grids
//   k_voxel_mlp        VoxelNeRFBase.forward, per-sample part             (voxnerf.py:210-221,240-254)
//                      sigma net + colour net on the same transposed-MFMA machinery as the NeRF backbone.
#include "voxel_taps.h"          // f16x4

namespace evd {

// merged-sample feature rows of the c2f pass (renderer.py:205-213): out[r, k, 0:F] = order[r, k] < S ? old[r, order] : fresh[r, order - S]
// -- the reference's gather of cat([ft_comb0, ft_comb1]) by the sort order, 16 bytes per lane
__global__ void k_merge_features(const float* __restrict__ old, const float* __restrict__ fresh, const int* __restrict__ order,
                                 long R, int S, int N, int F, float* __restrict__ out, int out_stride) {
    const int per = F / 4;
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long St = S + N;
    if (t >= R * St * per) return;
    const long smp = t / per;
    const int q = t % per;
    const long r = smp / St;
    const int o = order[smp];
    const float* src = o < S ? old + (r * S + o) * (long)F : fresh + (r * N + (o - S)) * (long)F;
    *reinterpret_cast<f32x4*>(out + smp * (long)out_stride + 4 * q) = *reinterpret_cast<const f32x4*>(src + 4 * q);
}

// its backward: the gather is a permutation of the rows of cat([old, fresh]), so every gradient row has exactly one destination
__global__ void k_merge_features_bwd(const float* __restrict__ d_out, int d_stride, const int* __restrict__ order, long R, int S, int N, int F,
                                     float* __restrict__ d_old, float* __restrict__ d_fresh) {
    const int per = F / 4;
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long St = S + N;
    if (t >= R * St * per) return;
    const long smp = t / per;
    const int q = t % per;
    const long r = smp / St;
    const int o = order[smp];
    float* dst = o < S ? d_old + (r * S + o) * (long)F : d_fresh + (r * N + (o - S)) * (long)F;
    *reinterpret_cast<f32x4*>(dst + 4 * q) = *reinterpret_cast<const f32x4*>(d_out + smp * (long)d_stride + 4 * q);
}

__global__ __launch_bounds__(256) void k_f32_to_f16(const float* __restrict__ x, long n4, _Float16* __restrict__ y) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256)
        *reinterpret_cast<f16x4*>(y + 4 * i) = __builtin_convertvector(*reinterpret_cast<const f32x4*>(x + 4 * i), f16x4);
}

// ------------------------------------------------------------------------------------------------
// HD hidden width, G geo_feat_dim, FT feature channels read per sample (32 coarse, 64 fine)
template <int PREC, int HD, int G, int FT>
__global__ __launch_bounds__(mlp_threads(PREC), is_half_prec(PREC) ? 2 : 1) void k_voxel_mlp(const VoxMlpParams p) {
    typedef Ops<PREC> O;
    typedef typename O::B B;
    constexpr int NT = mlp_threads(PREC);
    constexpr int T = HD / 32, KS = HD / 16, KF = FT / 16;
    constexpr int FPC = Stream<PREC>::FPC;
    constexpr bool kSmallGeo = (1 + G) <= 32;          // coarse level: [sigma, geo] fits one tile
    constexpr int GT = kSmallGeo ? 1 : G / 32;         // geo tiles
    constexpr int GK = kSmallGeo ? 1 : G / 16;         // geo k-steps fed to the colour net
    static_assert(kSmallGeo || G % 32 == 0, "geo_feat_dim must be < 32 or a multiple of 32");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5;
    const long s = (long)blockIdx.x * (NT / 2) + wave * 32 + n;
    const bool valid = s < p.nsamp;
    const long sc = valid ? s : p.nsamp - 1;
    float pts[3], vd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        pts[c] = p.pts[sc * 3 + c];
        vd[c] = p.viewdirs[(sc / p.S) * p.vd_stride + c];
    }
    // layer-0 input = cat([fts, PE(pts)])  (voxnerf.py:214): FT/16 natural k-steps + the PE arrangement
    B in0[KF + PE_KS], in_dir[PEV_KS];
    {
        const float* f = p.fts + sc * (long)p.ft_stride + 8 * h;
#pragma unroll
        for (int j = 0; j < KF; ++j) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(f + 16 * j), b = *reinterpret_cast<const f32x4*>(f + 16 * j + 4);
            const f32x8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
            in0[j] = O::make_b(v);
        }
        B pe[PE_KS];
        encode_b_rt<PREC, PE_KS>(pts, h, p.pe_l, pe);
#pragma unroll
        for (int j = 0; j < PE_KS; ++j) in0[KF + j] = pe[j];
        encode_b_rt<PREC, PEV_KS>(vd, h, p.pe_lv, in_dir);
    }
    const float* lbias = stage_bias<PREC>(smem, p.bias, p.nbias, tid);
    Stream<PREC> st;
    st.start(p.wstream, smem, p.nchunks, tid);
    const float* zero_bias = lbias;        // first 512 floats of the bias block are zeros (sigma net: bias=False)
    const float* cbias = lbias + 32 * 16;

    constexpr int F0 = T * (KF + PE_KS);
    B hid[KS];
    layer<PREC, KF + PE_KS, T, true, OUT_B, 0, false>(st, in0, hid, nullptr, zero_bias, lane, nullptr, HD);
    constexpr int OFF1 = F0 % FPC;
    float sig[16];
    B cin[GK + PEV_KS];
    float* frow = (p.feature && valid) ? p.feature + s * G : nullptr;
    if constexpr (kSmallGeo) {
        // one tile holds [sigma, geo_1..G]; it is both the sigma output and (k-step 0) the colour-net input
        B tmp[2];
        layer<PREC, KS, 1, false, OUT_BOTH, OFF1, false>(st, hid, tmp, sig, zero_bias, lane, nullptr, HD);
        cin[0] = tmp[0];
        if (frow) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                if (row >= 1 && row <= G) frow[row - 1] = sig[r];
            }
        }
    } else {
        layer<PREC, KS, 1, false, OUT_F32, OFF1, false>(st, hid, nullptr, sig, zero_bias, lane, nullptr, HD);
        constexpr int OFF1b = (F0 + KS) % FPC;
        layer<PREC, KS, GT, false, OUT_B, OFF1b, false>(st, hid, cin, nullptr, zero_bias, lane, frow, G);
    }
    constexpr int F1 = kSmallGeo ? KS : KS + GT * KS;
#pragma unroll
    for (int j = 0; j < PEV_KS; ++j) cin[GK + j] = in_dir[j];
    constexpr int OFF2 = (F0 + F1) % FPC;
    B c0[KS], c1[KS];
    layer<PREC, GK + PEV_KS, T, true, OUT_B, OFF2, false>(st, cin, c0, nullptr, cbias, lane, nullptr, HD);
    constexpr int F2 = T * (GK + PEV_KS);
    constexpr int OFF3 = (F0 + F1 + F2) % FPC;
    layer<PREC, KS, T, true, OUT_B, OFF3, false>(st, c0, c1, nullptr, cbias + 32 * T, lane, nullptr, HD);
    constexpr int OFF4 = (F0 + F1 + F2 + T * KS) % FPC;
    float col[16];
    layer<PREC, KS, 1, false, OUT_F32, OFF4, true>(st, c1, nullptr, col, cbias + 64 * T, lane, nullptr, HD);
    if (h == 0 && valid) {
        f32x4 o;
        o[0] = sig[0];
#pragma unroll
        for (int c = 0; c < 3; ++c) o[1 + c] = 1.f / (1.f + expf(-col[c]));      // torch.sigmoid(h) voxnerf.py:252
        *reinterpret_cast<f32x4*>(p.raw + s * 4) = o;
    }
}

template <int PREC, int HD, int G, int FT>
static int launch_vox(const VoxMlpParams& p, hipStream_t st) {
    constexpr int NT = mlp_threads(PREC);
    const long blocks = cdiv(p.nsamp, NT / 2);
    const size_t lds = MlpLds<PREC>::TOTAL;
    EVD_SET_MAX_LDS((&k_voxel_mlp<PREC, HD, G, FT>), lds);
    hipLaunchKernelGGL((k_voxel_mlp<PREC, HD, G, FT>), dim3((unsigned)blocks), dim3(NT), lds, st, p);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int voxel_mlp_dispatch(int prec, int HD, int G, int FT, const VoxMlpParams& p, hipStream_t st) {
#define EVD_CASE(P, H_, G_, F_) if (prec == P && HD == H_ && G == G_ && FT == F_) return launch_vox<P, H_, G_, F_>(p, st)
    EVD_CASE(EVD_PREC_BF16, 64, 15, 32);
    EVD_CASE(EVD_PREC_F16, 64, 15, 32);
    EVD_CASE(EVD_PREC_F16X3, 64, 15, 32);
    EVD_CASE(EVD_PREC_F32, 64, 15, 32);
    EVD_CASE(EVD_PREC_BF16, 256, 128, 64);
    EVD_CASE(EVD_PREC_F16, 256, 128, 64);
    EVD_CASE(EVD_PREC_F16X3, 256, 128, 64);
    EVD_CASE(EVD_PREC_F32, 256, 128, 64);
#undef EVD_CASE
    return fail(EVD_E_INVALID, "evd_voxel: no kernel for precision %d hidden %d geo %d features %d "
                "(built: coarse 64/15/32, fine 256/128/64)", prec, HD, G, FT);
}

int launch_merge_features(const float* old, const float* fresh, const int* order, long R, int S, int N, int F, float* out, int out_stride,
                          hipStream_t st) {
    const long n = R * (long)(S + N) * (F / 4);
    k_merge_features<<<cdiv(n, 256), 256, 0, st>>>(old, fresh, order, R, S, N, F, out, out_stride);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int launch_merge_features_bwd(const float* d_out, int d_stride, const int* order, long R, int S, int N, int F, float* d_old, float* d_fresh, hipStream_t st) {
    const long n = R * (long)(S + N) * (F / 4);
    k_merge_features_bwd<<<cdiv(n, 256), 256, 0, st>>>(d_out, d_stride, order, R, S, N, F, d_old, d_fresh);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

int launch_f32_to_f16(const float* x, long n, _Float16* y, hipStream_t st) {
    k_f32_to_f16<<<(unsigned)(cdiv(n / 4, 256) < 4096 ? cdiv(n / 4, 256) : 4096), 256, 0, st>>>(x, n / 4, y);
    EVD_LAUNCH_CHECK();
    return EVD_OK;
}

}  // namespace evd
