// Host side of the training backwards: the launch patterns that run_nerf_backward (nerf_train_kernel.h), run_voxel_backward
// (voxel_train_kernel.h) and run_awp_backward (awp_embed_kernel.h) share.  Included by nerf_train_kernel.h behind the kernels it
// launches and in front of run_nerf_backward; not a header to include on its own.
#pragma once

namespace evd {

// what a fused wgrad + dgrad step (k_wgrad_dgrad) of a PDRF level takes beyond the NeRF trunk's
struct FusedExtra {
    int mask_slot = -1;                 // ReLU pattern of the dgrad's output (-1: none)
    int RTr = 8;                        // row tiles the reduce reads (< 8: the kernel still lays every workgroup's set out as 8)
    int y_last_slot = -1;
    const char* ygen_wt = nullptr;
    float* rows = nullptr;              // the first rows_tiles tiles of d X as float32 rows of rows_stride floats
    int rows_stride = 0, rows_tiles = 0;
};

struct BwdChain : BwdPlanBase {
    long tile_bytes;
    hipStream_t st;                     // the caller's stream
    BwdChain(const BwdPlanBase& b, long tile_bytes_, hipStream_t st_) : BwdPlanBase(b), tile_bytes(tile_bytes_), st(st_) {}

    // workgroups of a wgrad launch or a fused step: one sample tile per iteration, grid-stride
    int tile_grid() const { return (int)(tiles < wgrad_blocks ? tiles : wgrad_blocks); }

    // *ws = the stream of a wgrad: the side stream, behind everything issued so far on the caller's stream (the producer of the
    // wgrad's operands), or without a side stream the caller's
    int fork(hipStream_t* ws) const {
        *ws = st;
        if (!side) return EVD_OK;
        EVD_HIP(hipEventRecord(ev, st));
        EVD_HIP(hipStreamWaitEvent(side, ev, 0));
        *ws = side;
        return test_side_spin(side);
    }
    // the caller's stream behind the wgrad launches in flight on the side stream: they use the partial scratch, read what a fused step
    // writes next, and the entry's caller relies on stream order
    int join() const {
        if (side && !test_skip_side_join()) {
            EVD_HIP(hipEventRecord(ev, side));
            EVD_HIP(hipStreamWaitEvent(st, ev, 0));
        }
        return EVD_OK;
    }

    DgradParams dgrad_params(const char* wt, int in_slot, int extra_slot, int mask_slot, int out_slot) const {
        DgradParams p;
        p.wstream = wt; p.store = store; p.tile_bytes = tile_bytes; p.in_slot = in_slot; p.extra_slot = extra_slot; p.mask_slot = mask_slot; p.out_slot = out_slot;
        return p;
    }
    WgradParams wgrad_params(bool bias, int y_slot, int x_slot) const {
        WgradParams p;
        p.store = store; p.tiles = tiles; p.tile_bytes = tile_bytes; p.y_slot = y_slot; p.x_slot = x_slot; p.bias = bias ? 1 : 0; p.partial = partial;
        return p;
    }
    // sum of the `nparts` workgroups' partial blocks -> dW (rows from `rowmap`, columns from `colmap`: offsets into maps) and db
    int reduce(int nparts, int RT, int CT, bool bias, int rowmap, int colmap, float* dW, int ld, float* db, long part_stride, hipStream_t ws) const {
        WreduceParams q;
        q.partial = partial; q.nparts = nparts; q.RT = RT; q.CT = CT; q.NC = CT + (bias ? 1 : 0);
        q.rowmap = maps + rowmap; q.colmap = maps + colmap; q.dW = dW; q.ld = ld; q.db = bias ? db : nullptr; q.maxbits = maxbits; q.accum = accumulate;
        q.part_stride = part_stride;
        hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)((long)RT * q.NC * 4)), dim3(256), 0, ws, q);
        EVD_LAUNCH_CHECK();
        return EVD_OK;
    }

    // wgrad + reduce of one parameter block, on the side stream when there is one.  Issued BEFORE the dgrad that reads the same two
    // arrays (incoming gradient, saved activation): the two are independent, run concurrently and share those reads in the Infinity Cache.
    template <class Launch>
    int wgrad(Launch launch, int blocks, int RT, int CT, bool bias, int y_slot, int x_slot, int rowmap, int colmap, float* dW, int ld, float* db) const {
        if (!dW) return EVD_OK;
        hipStream_t ws;
        int rc;
        if ((rc = fork(&ws))) return rc;
        if ((rc = launch(wgrad_params(bias, y_slot, x_slot), blocks, ws))) return rc;
        return reduce(blocks, RT, CT, bias, rowmap, colmap, dW, ld, db, 0, ws);
    }

    // wgrad(l) with dgrad(l) in one launch (k_wgrad_dgrad) on the caller's stream, then the reduce (none when dW is null: the dgrad alone)
    template <class Launch>
    int fused(Launch launch, int CT, bool bias, int y_slot, int x_slot, int rowmap, int colmap, float* dW, int ld, float* db, const char* wt, int out_slot,
              const FusedExtra& x = FusedExtra()) const {
        const int blocks = tile_grid();
        WgradFusedParams p;
        p.w = wgrad_params(bias, y_slot, x_slot);
        p.wt = wt; p.out_store = store; p.mask_slot = x.mask_slot; p.out_slot = out_slot; p.y_last_slot = x.y_last_slot; p.ygen_wt = x.ygen_wt;
        p.rows = x.rows; p.rows_stride = x.rows_stride; p.rows_tiles = x.rows_tiles; p.nsamp = nsamp; p.maxbits = maxbits;
        int rc;
        if ((rc = join())) return rc;
        if ((rc = launch(p, blocks, st))) return rc;
        if (!dW) return EVD_OK;
        return reduce(blocks, x.RTr, CT, bias, rowmap, colmap, dW, ld, db, x.RTr < 8 ? (long)8 * (CT + (bias ? 1 : 0)) * 1024 : 0, st);
    }

    // gradient of a positional encoding from its KS gradient fragments at `slot` (k_pe_bwd)
    template <int PREC, int L, int KS>
    int pe_bwd(int slot, const float* x, int x_stride, int per, float* dx, int accumulate_dx) const {
        hipLaunchKernelGGL((k_pe_bwd<PREC, L, KS>), dim3((unsigned)cdiv(tiles * 64, 256L)), dim3(256), 0, st, (const char*)store, tile_bytes, slot, nsamp, x, x_stride, per,
                           maxbits, dx, accumulate_dx);
        EVD_LAUNCH_CHECK();
        return EVD_OK;
    }
    // nfrag gradient fragments at `slot` -> float32 rows (k_frags_to_rows, defined with its kernel in voxel_train_kernel.h)
    template <int PREC> int frags_to_rows(int slot, int nfrag, float* rows, int stride) const;
};

}  // namespace evd
