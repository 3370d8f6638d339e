"""Image batch assembly on the device: the per-iteration part of the reference's ``LLFFDataset`` (data/loader.py) -- ``__getitem__``
(:325-356) and ``unravel_idx_from_rayid`` (:118-123) on the resident ``images`` / ``poses`` (/ ``pts0_images``, set_pts0_prior :110-116).
``ImageBatcher.sampler`` draws the ray ids of an iteration in the same launch (run_nerf.py:61-68, ``RaySampler``), and ``LLFFScene`` is the
once-per-dataset part (``__init__``, :27-99, 203-320; the scene box of utils/voxels.py:46-79) on the arrays a folder holds.
Reading the dataset from disk (images, poses_bounds.npy) stays with the caller: on-disk formats are out of scope."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L

HALF_PIX = 0.5          # utils/rays.py:5


class ImageBatcher:
    """images [n_img, H, W, 3] float32, poses [n_img, 3, 4] float32 (the train split of loader.py:60-63), K [3, 3].
    ``batcher[ray_ids]`` returns the reference's dict: rays [n, 3, 2], rays_x / rays_y [n, 1] (pixel + 0.5), images_idx [n, 1] int64,
    rgbsf [n, 3], poses [n, 3, 4] (+ rgbsf_pts0 [n, 3] once a prior is set) -- one kernel launch."""

    def __init__(self, images, poses, K, device="cuda"):
        dev = torch.device(device)
        self.device = dev
        self.images = torch.as_tensor(images, dtype=torch.float32, device=dev).contiguous()
        self.poses = torch.as_tensor(poses, dtype=torch.float32, device=dev)[:, :3, :4].contiguous()
        if self.images.dim() != 4 or self.images.shape[-1] != 3 or self.poses.shape[0] != self.images.shape[0]:
            raise L.EvdError("ImageBatcher: images [n_img, H, W, 3] and one [3, 4] pose per image")
        self.n_imgs, self.h, self.w = (int(v) for v in self.images.shape[:3])
        self.n_rays = self.n_imgs * self.h * self.w
        self.K = np.ascontiguousarray(np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float32).reshape(-1))
        self.pts0_images = None
        self._invalid = torch.zeros((1,), dtype=torch.int32, device=dev)

    def __len__(self):
        return self.n_rays

    def set_pts0_prior(self, pts0_images):
        """loader.py:110-116"""
        p = torch.as_tensor(pts0_images, dtype=torch.float32, device=self.device).contiguous()
        assert p.shape[0] == self.images.shape[0]
        if tuple(p.shape) != tuple(self.images.shape):
            raise L.EvdError("set_pts0_prior: the prior images must have the shape of the images")
        self.pts0_images = p

    def unravel_idx_from_rayid(self, ray_id):
        """loader.py:118-123 (C order): ray id -> (image id, y, x)"""
        if isinstance(ray_id, torch.Tensor):
            i = torch.div(ray_id, self.h * self.w, rounding_mode="floor")
            rem = ray_id - i * (self.h * self.w)
            y = torch.div(rem, self.w, rounding_mode="floor")
            return i, y, rem - y * self.w
        return np.unravel_index(ray_id, (self.n_imgs, self.h, self.w), order="C")

    def __getitem__(self, ray_ids, check=False):
        """loader.py:325-356.  check=True reads the device flag back and raises IndexError for an id outside [0, len(self))."""
        if isinstance(ray_ids, int):
            ray_ids = [ray_ids]
        ids = torch.as_tensor(ray_ids, device=self.device).to(torch.int64).contiguous().reshape(-1)
        n = ids.shape[0]
        rays, rx, ry, idx, rgb, poses, rgb0 = self._rows(n)
        L.check(L.lib().evd_image_batch(L.ptr(ids), n, L.ptr(self.images), L.ptr(self.pts0_images), L.ptr(self.poses), self.n_imgs, self.h, self.w,
                                        self.K.ctypes.data_as(C.POINTER(C.c_float)), L.ptr(rays), L.ptr(rx), L.ptr(ry), L.ptr(idx), L.ptr(rgb),
                                        L.ptr(poses), L.ptr(rgb0), L.ptr(self._invalid), L.stream_ptr()), "evd_image_batch")
        if check and int(self._invalid.item()):
            raise IndexError("ImageBatcher: a ray id outside [0, n_imgs * h * w)")
        return self._as_dict(rays, rx, ry, idx, rgb, poses, rgb0)

    def _rows(self, n):
        """the destination tensors of an n-ray batch (rgb0 None without a prior)"""
        f32 = dict(dtype=torch.float32, device=self.device)
        return (torch.empty((n, 3, 2), **f32), torch.empty((n, 1), **f32), torch.empty((n, 1), **f32), torch.empty((n, 1), dtype=torch.int64, device=self.device),
                torch.empty((n, 3), **f32), torch.empty((n, 3, 4), **f32), torch.empty((n, 3), **f32) if self.pts0_images is not None else None)

    @staticmethod
    def _as_dict(rays, rx, ry, idx, rgb, poses, rgb0):
        out = {"rays": rays, "rays_x": rx, "rays_y": ry, "images_idx": idx, "rgbsf": rgb, "poses": poses}
        if rgb0 is not None:
            out["rgbsf_pts0"] = rgb0
        return out

    def sampler(self, N_rand, mode="random", same_imgs_size=None, seed=0):
        """The ray draw of a training iteration (run_nerf.py:61-68) fused with the batch assembly -> RaySampler"""
        return RaySampler(self, N_rand, mode=mode, same_imgs_size=same_imgs_size, seed=seed)


# ------------------------------------------------------------------------------------------ per-iteration ray draws on the device
_M64 = (1 << 64) - 1


def _mix64(z):
    """splitmix64's finaliser: the mixing hash of the draw generator (csrc/kernels_loader.hip mix64)"""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


class RaySampler:
    """``next(sampler)`` -> the dict of ``ImageBatcher.__getitem__`` plus ``ray_ids`` [N] int64, drawn and assembled in one launch
    (``evd_image_batch_draw``); nothing is read back, the host knows the epoch ends by counting.  An endless iterator: ``epoch`` / ``batch``
    are the coordinates of the next draw, ``seek(epoch, batch)`` moves there.  The generator is the library's own, counter-based on
    (seed, epoch, batch): equal triples give equal ids bit for bit; torch's generator streams are not reproduced.

    mode "random": BatchSampler(RandomSampler(dataset), N_rand, drop_last=True) -- without replacement over an epoch of n_rays // N_rand
    batches, the tail dropped; no epoch permutation exists, the kernel evaluates a keyed bijection of [0, n_rays) at the batch's positions.
    mode "images": ImageBatchSampler (data/sampler_image_batch.py) -- ``same_imgs_size`` distinct images, uniform among those with at least
    N_rand // same_imgs_size unused pixels (chosen here, a few integers), that many distinct unused pixels of each (removed on the device
    from a resident int32 permutation per image, n_img * H * W * 4 bytes); the epoch ends when fewer images are eligible.  An epoch start
    only resets the host's counts: the permutations carry over, so the ids of an epoch depend on the draws before it and ``seek`` to an
    earlier position replays them from (0, 0) without assembling (one small launch per replayed batch)."""

    MODES = {"random": 0, "images": 1}

    def __init__(self, batcher, N_rand, mode="random", same_imgs_size=None, seed=0):
        if mode not in self.MODES:
            raise ValueError(f"RaySampler: unknown ray sampling mode {mode!r} (random | images)")
        self.batcher, self.mode, self.N, self.seed = batcher, mode, int(N_rand), int(seed) & _M64
        self.epoch = self.batch = 0
        hw = batcher.h * batcher.w
        if self.N < 1:
            raise L.EvdError("RaySampler: N_rand < 1")
        if mode == "random":
            if self.N > batcher.n_rays:
                raise L.EvdError(f"RaySampler: N_rand = {self.N} exceeds the {batcher.n_rays} rays of the dataset (drop_last leaves no batch)")
            self.n_batches = batcher.n_rays // self.N
            return
        self.same = int(same_imgs_size) if same_imgs_size is not None else 0
        if self.same < 1 or self.same > batcher.n_imgs:
            raise L.EvdError(f"RaySampler: same_imgs_size = {same_imgs_size} outside [1, n_imgs = {batcher.n_imgs}]")
        if self.N % self.same != 0:
            raise L.EvdError("RaySampler: N_rand must be divisible by same_imgs_size (sampler_image_batch.py:20)")
        self.per = self.N // self.same
        if self.per > hw:
            raise L.EvdError(f"RaySampler: {self.per} pixels per image wanted of {hw}")
        self._perm = None
        self._reset_images()

    def __iter__(self):
        return self

    # ---- images mode, host side: the counts and the image choice
    def _reset_images(self):
        b = self.batcher
        self._perm = torch.arange(b.h * b.w, dtype=torch.int32, device=b.device).repeat(b.n_imgs, 1).contiguous()
        self._live = [b.h * b.w] * b.n_imgs
        self.epoch = self.batch = 0

    def _choose_images(self):
        """``same`` distinct images, uniform among the eligible ones (:36-41, equal weights): a partial Fisher-Yates of the ascending list"""
        pool = [i for i, c in enumerate(self._live) if c >= self.per]
        key = _mix64(_mix64(_mix64(self.seed ^ 0x63686F6F) ^ self.epoch) ^ self.batch)
        for s in range(self.same):
            r = s + (((_mix64(key ^ s) >> 32) * (len(pool) - s)) >> 32)
            pool[s], pool[r] = pool[r], pool[s]
        return pool[:self.same]

    def _advance_images(self, chosen):
        for i in chosen:
            self._live[i] -= self.per
        if sum(c >= self.per for c in self._live) < self.same:          # (:59-62)
            self._live = [self.batcher.h * self.batcher.w] * self.batcher.n_imgs
            self.epoch, self.batch = self.epoch + 1, 0
        else:
            self.batch += 1

    def _launch(self, assemble):
        b, n = self.batcher, self.N
        chosen = chosen_c = live = None
        same, ids, rows = 0, None, (None,) * 7
        if self.mode == "images":
            chosen = self._choose_images()
            same = self.same
            live = (C.c_int * same)(*[self._live[i] for i in chosen])
            chosen_c = (C.c_int * same)(*chosen)
        if assemble:
            ids = torch.empty((n,), dtype=torch.int64, device=b.device)
            rows = b._rows(n)
        rays, rx, ry, idx, rgb, poses, rgb0 = rows
        L.check(L.lib().evd_image_batch_draw(self.MODES[self.mode], int(assemble), n, self.seed, self.epoch, self.batch, chosen_c if chosen else None, live, same,
                                             L.ptr(self._perm) if chosen else None, L.ptr(b.images), L.ptr(b.pts0_images), L.ptr(b.poses), b.n_imgs, b.h, b.w,
                                             b.K.ctypes.data_as(C.POINTER(C.c_float)), L.ptr(ids), L.ptr(rays), L.ptr(rx), L.ptr(ry), L.ptr(idx), L.ptr(rgb),
                                             L.ptr(poses), L.ptr(rgb0), L.stream_ptr()), "evd_image_batch_draw")
        if self.mode == "images":
            self._advance_images(chosen)
        else:
            self.batch += 1
            if self.batch == self.n_batches:
                self.epoch, self.batch = self.epoch + 1, 0
        if not assemble:
            return None
        out = b._as_dict(*rows)
        out["ray_ids"] = ids
        return out

    def __next__(self):
        return self._launch(True)

    def seek(self, epoch, batch):
        """The next draw becomes batch ``batch`` of epoch ``epoch``."""
        epoch, batch = int(epoch), int(batch)
        if epoch < 0 or batch < 0:
            raise L.EvdError("RaySampler.seek: negative epoch or batch")
        if self.mode == "random":
            if batch >= self.n_batches:
                raise L.EvdError(f"RaySampler.seek: batch {batch} outside the epoch of {self.n_batches} batches")
            self.epoch, self.batch = epoch, batch
            return
        if (epoch, batch) < (self.epoch, self.batch):
            self._reset_images()
        while (self.epoch, self.batch) < (epoch, batch):
            self._launch(False)
        if (self.epoch, self.batch) != (epoch, batch):
            raise L.EvdError(f"RaySampler.seek: epoch {epoch} ends before batch {batch}")


# ------------------------------------------------------------------------------------------ once-per-dataset pose preparation (host, numpy)
def load_poses(poses_bounds, factor, imgshape, bdsmin=None, bd_factor=.75, scale=None):
    """LLFFDataset.load_poses (data/loader.py:178-203) on the array of poses_bounds.npy [N, 17] (reading the file stays with the caller):
    image size and the focal of the down-scaled images into column 4, LLFF column change [r1, -r0, r2, t, hwf], float32, translations and
    bounds rescaled by 1 / (min bound x bd_factor) (or `scale`).  -> poses [N, 3, 5] float32, bds [N, 2] float32, sc.  A few dozen 3 x 5
    matrices: host arithmetic, as in the reference."""
    poses_arr = np.array(poses_bounds, dtype=np.float64, copy=True)
    poses = poses_arr[:, :-2].reshape([-1, 3, 5])
    if not _is_pure_rotation_matrix(poses[:, :3, :3]):
        raise L.EvdError("load_poses: poses_bounds does not hold rotation matrices (the reference asserts, loader.py:181)")
    bds = poses_arr[:, -2:]
    poses[:, :2, 4] = np.array(imgshape[:2]).reshape([1, 2])
    poses[:, 2, 4] = poses[:, 2, 4] * 1. / factor
    poses = np.concatenate([poses[..., 1:2], -poses[..., 0:1], poses[..., 2:]], -1).astype(np.float32)
    bds = bds.astype(np.float32)
    bdsmin = np.min(bds) if bdsmin is None else bdsmin
    sc = (1. if bd_factor is None else 1. / (bdsmin * bd_factor)) if scale is None else scale
    poses[:, :3, 3] *= sc
    bds *= sc
    return poses, bds, sc


def _is_pure_rotation_matrix(M):
    """utils/data.py:9-31: every det isclose to 1 (numpy's default tolerances) and M^T allclose to inv(M) with atol 5e-7"""
    M = np.asarray(M)
    if not np.all(np.isclose(np.linalg.det(M), 1.0)):
        return False
    return bool(np.allclose(np.transpose(M, (0, 2, 1)), np.linalg.inv(M), atol=5e-7))


def _normalize(x):
    return x / np.linalg.norm(x)


def poses_avg(poses):
    """utils/data.py poses_avg: centre = mean translation, z = normalised sum of the z axes, up = sum of the y axes -> the view matrix with
    the hwf column of pose 0 ([3, 5])"""
    hwf = poses[0, :3, -1:]
    center = poses[:, :3, 3].mean(0)
    vec2 = _normalize(_normalize(poses[:, :3, 2].sum(0)))          # (poses_avg normalises, viewmatrix normalises again: utils/data.py:119-134)
    up = poses[:, :3, 1].sum(0)
    vec0 = _normalize(np.cross(up, vec2))
    vec1 = _normalize(np.cross(vec2, vec0))
    return np.concatenate([np.stack([vec0, vec1, vec2, center], 1), hwf], 1)


def recenter_poses(poses, c2w=None, return_c2w=False):
    """utils/data.py:167-183: inv(average pose) @ poses on the [3, 4] part; c2w: a given average pose (the event loader re-applies the image
    dataset's, run_nerf.py:74-81) -> poses (same dtype), and the [4, 4] c2w with return_c2w"""
    poses_ = poses + 0
    bottom = np.reshape([0, 0, 0, 1.], [1, 4])
    if c2w is None:
        c2w = poses_avg(poses)
        c2w = np.concatenate([c2w[:3, :4], bottom], -2)
    bottom = np.tile(np.reshape(bottom, [1, 1, 4]), [poses.shape[0], 1, 1])
    p44 = np.concatenate([poses[:, :3, :4], bottom], -2)
    p44 = np.linalg.inv(c2w) @ p44
    poses_[:, :3, :4] = p44[:, :3, :4]
    return (poses_, c2w) if return_c2w else poses_


def image_batcher_from_llff_arrays(poses_bounds, images, K=None, factor=1, bd_factor=.75, recenter=True, recenter_partial=None, device="cuda"):
    """The pose side of LLFFDataset.__init__ (data/loader.py:50-63 through load_poses :178-203 and the recentring branch of
    recenter_spherify_poses :205-216) on arrays: -> (ImageBatcher over the recentred [N, 3, 4] poses, dict(poses [N, 3, 5], bds, sc,
    recenter_partial [4, 4] -- what EventTables / PoseTrack re-apply)).  K None: load_intrinsics (:133-137) from the poses' hwf column."""
    imgs = np.asarray(images)
    poses, bds, sc = load_poses(poses_bounds, factor, imgs.shape[1:], bd_factor=bd_factor)
    c2w = None
    if recenter:
        poses, c2w = (recenter_poses(poses, c2w=recenter_partial), recenter_partial) if recenter_partial is not None else recenter_poses(poses, return_c2w=True)
    if K is None:
        H, W_, focal = poses[0, :3, -1]
        K = np.array([[focal, 0, 0.5 * W_], [0, focal, 0.5 * H], [0, 0, 1]])
    return ImageBatcher(imgs, poses[:, :3, :4], K, device=device), {"poses": poses, "bds": bds, "sc": sc, "recenter_partial": c2w}


# ------------------------------------------------------------------------------------------ once-per-dataset scene setup (host, numpy)
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _look_along(z, up, pos):
    """camera frames [..., 3, 4] with the z axis along ``z``: x = up x z, y = z x x, all normalised; fourth column ``pos``"""
    z = _unit(z)
    x = _unit(np.cross(np.broadcast_to(up, z.shape), z))
    y = _unit(np.cross(z, x))
    return np.stack([x, y, z, np.broadcast_to(pos, z.shape)], -1)


def _with_hwf(frames, c2w):
    return np.concatenate([frames, np.broadcast_to(c2w[:3, 4:5], frames.shape[:-1] + (1,))], -1)


def render_path_spiral(c2w, up, rads, focal, zdelta, zrate, rots, N):
    """utils/data.py:139-151 for all N views at once: camera centres on the spiral (rads_x cos t, -rads_y sin t, -rads_z sin(t zrate)) of the
    frame ``c2w`` [3, 5], t over ``rots`` turns, each looking at the point ``focal`` in front of c2w -> [N, 3, 5] float64.  ``zdelta`` is
    taken and, as in the reference, unused."""
    A = np.asarray(c2w, np.float64)[:3, :4]
    t = np.linspace(0., 2. * np.pi * rots, N + 1)[:-1]
    local = np.stack([np.cos(t), -np.sin(t), -np.sin(t * zrate), np.ones_like(t)], -1) * np.append(np.asarray(rads, np.float64), 1.)
    centres = local @ A.T
    focus = A @ np.array([0., 0., -np.float64(focal), 1.])
    return _with_hwf(_look_along(centres - focus, np.asarray(up, np.float64), centres), np.asarray(c2w))


def render_path_epi(c2w, up, rads, N):
    """utils/data.py:154-164 for all N views at once: centres on the x axis of ``c2w`` from -rads to rads, all looking along its z axis.
    The reference scales the homogeneous coordinate with ``rads`` too (c = rads (t x_axis + origin)); kept. -> [N, 3, 5] float64"""
    A = np.asarray(c2w, np.float64)[:3, :4]
    t = np.linspace(-1, 1, N + 1)[:-1]
    centres = np.float64(rads) * (t[:, None] * A[:, 0] + A[:, 3])
    return _with_hwf(_look_along(np.broadcast_to(A[:, 2], centres.shape), np.asarray(up, np.float64), centres), np.asarray(c2w))


def llff_render_poses(poses, bds, path_epi=False, render_focuspoint_scale=1., render_radius_scale=1., n_views=120, n_rots=2):
    """The video path of recenter_spherify_poses (data/loader.py:228-263) from the prepared poses [N, 3, 5] float32 and bounds float32:
    the average pose, a focus depth between 0.9 x the closest and 5 x the furthest bound (weights .25 / .75 in inverse depth), radii = the
    90th percentile of |translation|.  The scalars are float32 like the arrays they come from; the path itself is float64, rounded once
    -> [n_views, 3, 5] float32."""
    f32 = np.float32
    poses, bds = np.asarray(poses, f32), np.asarray(bds, f32)
    c2w = poses_avg(poses)
    up = _unit(poses[:, :3, 1].sum(0))
    close_depth, inf_depth = bds.min() * f32(.9), bds.max() * f32(5.)
    focal = f32(1.) / (f32(.25) / close_depth + f32(.75) / inf_depth) * f32(render_focuspoint_scale)
    rads = np.percentile(np.abs(poses[:, :3, 3]), 90, 0).astype(f32)
    rads[:2] *= f32(render_radius_scale)
    if path_epi:
        return render_path_epi(c2w, up, rads[0] / f32(2), n_views).astype(f32)
    return render_path_spiral(c2w, up, rads, focal, close_depth * f32(.2), zrate=.5, rots=n_rots, N=n_views).astype(f32)


def _fma32(a, b, c):
    """a b + c on float32 arrays: the product is exact in float64, one rounding of the sum to float64 precedes the rounding to float32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def bbox3d_for_llff(poses, hwf, near=0.0, far=1.0, is_ndc=True):
    """get_bbox3d_for_llff (utils/voxels.py:46-79): the box of the points at ``near`` and ``far`` on the four image-corner rays of every
    pose [N, 3, 4] (pixel grid without the half pixel, utils/rays.py:52-101; normalised directions; moved to NDC with near plane 1 when
    ``is_ndc``), widened by (0.01, 0.01, 0.0001) -> (min, max), float32 triples.  All in float32 in the reference's operation order: the
    grid sizes of the tri-planes are truncations of this box.  The reference's matrix product and norm accumulate with fused
    multiply-adds, k ascending; ``_fma32`` restates that."""
    f32 = np.float32
    H, W, focal = int(hwf[0]), int(hwf[1]), f32(hwf[2])
    P = np.asarray(poses, f32)[:, :3, :4]
    cx, cy = np.array([0, W - 1, 0, W - 1], f32), np.array([0, 0, H - 1, H - 1], f32)
    dirs = np.stack([(cx - f32(W / 2)) / focal, -(cy - f32(H / 2)) / focal, -np.ones(4, f32)], -1)
    a, R = np.broadcast_arrays(dirs[None, :, None, :], P[:, None, :, :3])                     # [N, corner, row, k]
    d = _fma32(a[..., 2], R[..., 2], _fma32(a[..., 1], R[..., 1], a[..., 0] * R[..., 0]))
    d = d / np.sqrt(_fma32(d[..., 2], d[..., 2], _fma32(d[..., 1], d[..., 1], d[..., 0] * d[..., 0])))[..., None]
    o = np.broadcast_to(P[:, None, :, 3], d.shape)
    if is_ndc:                                                                               # get_ndc_rays, utils/rays.py:104-145, near = 1
        o = o + (-(f32(1.) + o[..., 2]) / d[..., 2])[..., None] * d
        ox_oz, oy_oz = o[..., 0] / o[..., 2], o[..., 1] / o[..., 2]
        sx, sy = f32(-1.) / (f32(W) / (f32(2.) * focal)), f32(-1.) / (f32(H) / (f32(2.) * focal))
        o2 = f32(1.) + f32(2.) / o[..., 2]
        d = np.stack([sx * (d[..., 0] / d[..., 2] - ox_oz), sy * (d[..., 1] / d[..., 2] - oy_oz), f32(1.) - o2], -1)
        o = np.stack([sx * ox_oz, sy * oy_oz, o2], -1)
    pts = np.concatenate([o + f32(near) * d, o + f32(far) * d], 0).reshape(-1, 3)
    margin = np.array([0.01, 0.01, 0.0001], f32)
    return np.minimum(pts.min(0), f32(100)) - margin, np.maximum(pts.max(0), f32(-100)) + margin


class LLFFScene:
    """What LLFFDataset.__init__ derives from the arrays of an LLFF folder (data/loader.py:44-90), once per dataset on the host:
    ``poses`` [N, 3, 5] / ``bds`` (scaled, recentred), ``scale``, ``recenter_partial`` [4, 4], ``K``, ``h``, ``w``, the hold-out split
    ``i_train`` / ``i_val`` / ``i_test`` with ``test_poses``, ``render_poses`` [120, 3, 4] float32, ``closest_bds`` / ``furthest_bds``,
    ``near`` / ``far`` and ``bounding_box`` (the args.bounding_box NeRFAll takes).  ``batcher()`` is the ImageBatcher of the train split,
    ``event_kwargs()`` what EventTables.from_arrays re-applies to the event trajectory.  Reading the folder (and datadownsample's
    cv2.resize) stays with the caller."""

    @classmethod
    def from_arrays(cls, poses_bounds, images, factor=1, bd_factor=.75, recenter=True, llffhold=8, llffhold_end=False, path_epi=False,
                    render_focuspoint_scale=1., render_radius_scale=1., no_ndc=False, all_poses_bounds=None, spherify=False, device="cuda"):
        """poses_bounds [N, 17] (poses_bounds.npy), images [N, H, W, 3] float32 at the size the factor gives.  all_poses_bounds [M, 17]:
        pose_transform_allknown -- the scale, the recentring pose and the min / max bounds come from the whole trajectory (:266-276)."""
        if spherify:
            raise NotImplementedError("spherify: no shipped config sets --spherify (spherify_poses, utils/data.py:189-253, is not built)")
        self = cls()
        self.images = np.asarray(images)
        if self.images.ndim != 4 or self.images.shape[0] != np.asarray(poses_bounds).shape[0]:
            raise L.EvdError("LLFFScene: images [N, H, W, 3], one per row of poses_bounds")
        self.device, self.factor = device, factor
        imgshape = self.images.shape[1:]
        # the transform of the trajectory the scale is taken from (get_pose_transform_data), then the images' poses under it
        ref_poses, ref_bds, self.scale = load_poses(poses_bounds if all_poses_bounds is None else all_poses_bounds, factor, imgshape, bd_factor=bd_factor)
        self.recenter_partial = recenter_poses(ref_poses, return_c2w=True)[1] if recenter else None
        self.poses, self.bds, _ = load_poses(poses_bounds, factor, imgshape, bd_factor=bd_factor, scale=self.scale)
        if recenter:
            self.poses = recenter_poses(self.poses, c2w=self.recenter_partial)
        self.render_poses = np.ascontiguousarray(llff_render_poses(self.poses, self.bds, path_epi, render_focuspoint_scale, render_radius_scale)[:, :3, :4])
        n = self.images.shape[0]
        self.i_test = np.arange(n)[-llffhold:] if llffhold_end else np.arange(n)[::llffhold]          # (:48-57)
        self.i_val = self.i_test
        self.i_train = np.setdiff1d(np.arange(n), self.i_test)
        if self.i_train.size == 0:
            raise L.EvdError(f"LLFFScene: llffhold = {llffhold} leaves no training view of {n}")
        self.test_poses = self.poses[self.i_test][:, :3, :4]
        H, W_, focal = self.poses[0, :3, -1]
        sh, sw = np.float32(imgshape[0]) / H, np.float32(imgshape[1]) / W_                              # load_intrinsics (:135-139, 315-317)
        self.K = np.array([[focal * sw, 0, np.float32(0.5) * W_ * sw], [0, focal * sh, np.float32(0.5) * H * sh], [0, 0, 1]], np.float64)
        self.h, self.w = int(imgshape[0]), int(imgshape[1])
        self.closest_bds, self.furthest_bds = float(self.bds.min()), float(self.bds.max())            # (:76-77)
        self.near, self.far = (ref_bds.min() * np.float32(.9), ref_bds.max() * np.float32(1.)) if no_ndc else (0., 1.)      # (:82-87)
        self.no_ndc = bool(no_ndc)
        self.bounding_box = bbox3d_for_llff(self.poses[:, :3, :4], self.poses[0, :3, -1], near=0, far=1, is_ndc=not no_ndc)        # (:89)
        return self

    def batcher(self):
        """the ImageBatcher over the train split (:59-63)"""
        return ImageBatcher(self.images[self.i_train], self.poses[self.i_train][:, :3, :4], self.K, device=self.device)

    def event_kwargs(self):
        """the transform EventTables.from_arrays / PoseTrack re-apply to the event trajectory (run_nerf.py:74-81)"""
        return {"bd_scale": float(self.scale), "recenter": self.recenter_partial is not None, "recenter_partial": self.recenter_partial}
