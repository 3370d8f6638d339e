"""The sparse blur kernel network in plain PyTorch: what evdeblurnerf_amd.blurmodel.SparseBlurKernel computes, as batched float32 tensor ops
under autograd -- the restatement tests/sparse_blur_ref.py run on the module's own parameters and device.  Same constructor, parameter
names and forward signature, so the two exchange state dicts.  tools/bench_sparse_blur.py and tools/bench_train_step.py --kernel dsk-torch
time it against the library's kernels."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import sparse_blur_ref as SR  # noqa: E402
from evdeblurnerf_amd.blurmodel import SparseBlurKernel  # noqa: E402


class TorchSparseBlur(SparseBlurKernel):
    def forward(self, H, W, K, rays, rays_info, feats=None, return_img_embed=False, noise=None, **kwargs):
        ids = rays_info["images_idx"].reshape(-1)
        cfg = dict(kernel_type=self.kernel_type, num_pt=self.num_pt, kernel_hwindow=self.kernel_hwindow, random_hwindow=self.random_hwindow,
                   in_embed=self.in_embed, spatial_embed=self.spatial_embed, num_hidden=self.num_hidden, feat_cnl=self.feat_cnl, short_cut=self.short_cut,
                   isglobal=self.isglobal, optim_trans=self.optim_trans, optim_spatialvariant_trans=self.optim_sv_trans)
        if self.random_hwindow > 0 and noise is None:
            noise = torch.randn((ids.shape[0], self.num_pt, 2), device=ids.device)
        poses = rays_info["poses"] if self.poses is None else self.poses[ids]
        K4 = (float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]))
        new_rays, weight, align, img_embed = SR.forward(dict(self.named_parameters()), cfg, H, W, K4, ids, rays_info["rays_x"].reshape(-1),
                                                        rays_info["rays_y"].reshape(-1), poses, noise, feats)
        return new_rays, weight, align, ({"img_embed": img_embed} if return_img_embed else {})
