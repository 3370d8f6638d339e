"""Decoders of the training kernels' activation stores: lane-linear 1 KiB MFMA B fragments (one per 32-sample tile and 16 channels) ->
[nsamp, channels] tensors in the hidden-channel arrangement.  The float64 backward tests read the kernel's own ReLU pattern out of a
store with these ("same pattern" comparisons).  Test infrastructure only."""
import torch

# fragment slots of the NeRF activation store (csrc/nerf_mlp.h, namespace astore)
PE, DIR, H0, F, HV, FWD_END = 0, 4, 6, 134, 150, 158
G_RGB, G_ALPHA, D_HV, D_F, D_H0, TILE_FRAGS = 158, 159, 160, 168, 184, 331
# fragment slots of the AWP embedding's store (csrc/awp_embed.h, namespace awpstore)
A_GEO, A_E0, A_D_E0, A_D_GEO, A_TILE_FRAGS = 0, 8, 24, 40, 48


def phi(kk):
    return 8 * ((kk & 7) >> 2) + 4 * (kk >> 3) + (kk & 3)


def _frags(v, tiles, nfrag, nsamp):
    """[tiles, nfrag, lane = n + 32 h, 8] values -> [nsamp, 16 nfrag], channel 16 j + phi(8 h + e)"""
    v = v.view(tiles, nfrag, 2, 32, 8)
    out = torch.zeros((tiles, 32, nfrag * 16), dtype=torch.float32, device=v.device)
    for h in range(2):
        for e in range(8):
            out[:, :, torch.arange(nfrag) * 16 + phi(8 * h + e)] = v[:, :, h, :, e].permute(0, 2, 1)
    return out.reshape(tiles * 32, nfrag * 16)[:nsamp]


def decode(store, nsamp, slot, nfrag, dtype):
    """fragments [slot, slot + nfrag) of every tile -> [nsamp, 16 * nfrag] in the hidden-channel arrangement (channel 16 j + phi(kk))"""
    tiles = store.numel() // (TILE_FRAGS * 1024)
    v = store.view(tiles, TILE_FRAGS, 64, 16)[:, slot:slot + nfrag].contiguous().view(dtype).float()   # [tiles, nfrag, lane, 8]
    return _frags(v, tiles, nfrag, nsamp)


def vdecode(store, nsamp, tile_frags, slot, nfrag, dtype):
    """... of a PDRF level's store (voxel_mlp_kernel.h VStore) with tile_frags fragments per tile"""
    tiles = store.numel() // (tile_frags * 1024)
    v = store.view(tiles, tile_frags, 64, 16)[:, slot:slot + nfrag].contiguous().view(dtype).float()
    return _frags(v, tiles, nfrag, nsamp)


def adecode(store, nsamp, slot, nfrag, dtype):
    """fragments [slot, slot + nfrag) of every tile of an awp store -> [nsamp, 16 nfrag], channel 16 j + phi(kk)"""
    tiles = (store.numel() - 256) // (A_TILE_FRAGS * 1024)
    v = store[:tiles * A_TILE_FRAGS * 1024].view(tiles, A_TILE_FRAGS, 64, 16)[:, slot:slot + nfrag].contiguous().view(dtype).float()
    return _frags(v, tiles, nfrag, nsamp)


def vstore_slots(HD, G, FT):
    """(HID, C0, C1, TILE_FRAGS) of VStore<HD, G, FT>: [fts | PE(pts)], hidden, geo, PE(dirs), c0, c1, then the gradient fragments"""
    KS, KF, GT = HD // 16, FT // 16, (G + 31) // 32
    HID = KF + 4
    C0 = HID + KS + 2 * GT + 2
    C1 = C0 + KS
    tile_frags = C1 + KS + 2 + KS + KS + (2 * GT + 2) + KS + (2 * ((FT + 31) // 32) + 4) + 3   # + d PE(dirs), d PE(pts) fragments, 3 bit-mask fragments
    return HID, C0, C1, tile_frags
