#!/usr/bin/env python
"""Time one training iteration's ray draw + batch assembly at the shipped shape: 30 images of 400 x 400, N_rand = 1024.

    python tools/bench_ray_draw.py [--reps 300] [--out profiles/ray_draw_bench.json]      on the GPU

Per mode, the two routes alternate draw by draw in one process after 20 warm-up draws of each; every draw is timed with a host clock
from the call to the end of a device synchronise (the draw's launch cost is part of what it removes), the median of --reps with quartiles:
  random   (a) new   next(batcher.sampler(N, "random"))             one launch, ids from the keyed bijection
           (b) old   ImageBatcher[perm[b N : (b + 1) N]] on a torch.randperm(n_rays) of the device; the randperm itself (once per
                     epoch in that route) is timed apart
  images   (a) new   next(batcher.sampler(N, "images", same))       one launch, partial Fisher-Yates on the resident permutations
           (b) old   the rule of data/sampler_image_batch.py restated in torch operations on the device (a [n_img, H, W] mask, its sums,
                     two multinomials, the mask update, the read-back that decides the epoch's end), then ImageBatcher[ids]
Informational: no speed is asserted anywhere.  Prints one JSON line; --out also writes it to a file."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_IMG, H, W, N_RAND = 30, 400, 400, 1024
SAMES = (8, 2)


class TorchImageRule:
    """data/sampler_image_batch.py:29-62 on the device"""

    def __init__(self, n_img, h, w, N, same, device):
        import torch
        self.t, self.n_img, self.h, self.w, self.same, self.per = torch, n_img, h, w, same, N // same
        self.mask = torch.ones((n_img, h, w), dtype=torch.bool, device=device)
        self.elig = (self.mask.sum(dim=(1, 2)) >= self.per)

    def draw(self):
        t = self.t
        img = t.multinomial(self.elig.float(), num_samples=self.same)
        pix = t.multinomial(self.mask[img].reshape(self.same, -1).float(), num_samples=self.per)
        ids = (img[:, None] * (self.h * self.w) + pix).reshape(-1)
        self.mask.view(-1)[ids] = False
        self.elig = self.mask.sum(dim=(1, 2)) >= self.per
        if int(self.elig.sum().item()) < self.same:
            self.mask.fill_(True)
            self.elig = self.mask.sum(dim=(1, 2)) >= self.per
        return ids


def stats(ms):
    q = np.percentile(ms, [25, 50, 75])
    return {"median": round(float(q[1]), 4), "p25": round(float(q[0]), 4), "p75": round(float(q[2]), 4), "min": round(float(np.min(ms)), 4),
            "max": round(float(np.max(ms)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from evdeblurnerf_amd.loader import ImageBatcher
    if not torch.cuda.is_available():
        raise SystemExit("bench_ray_draw: needs a GPU")
    if a.reps < 200:
        raise SystemExit("bench_ray_draw: at least 200 draws per route")
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    images = torch.rand((N_IMG, H, W, 3), device=dev, generator=g)
    poses = torch.randn((N_IMG, 3, 4), device=dev, generator=g)
    K = np.array([[433.0, 0, 200.0], [0, 433.0, 200.0], [0, 0, 1]], np.float32)
    b = ImageBatcher(images, poses, K)
    b.set_pts0_prior(images.flip(0).contiguous())

    def alternate(new, old):
        for _ in range(20):
            new(), old()
        torch.cuda.synchronize()
        ms = ([], [])
        for _ in range(a.reps):
            for fn, dst in ((new, ms[0]), (old, ms[1])):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                dst.append((time.perf_counter() - t0) * 1e3)
        return stats(ms[0]), stats(ms[1])

    res = {"reps": a.reps, "device": torch.cuda.get_device_name(0), "shape": {"n_img": N_IMG, "H": H, "W": W, "N_rand": N_RAND},
           "timing": "host clock, call to end of device synchronise, routes alternating draw by draw, ms"}
    # ---- random
    s = b.sampler(N_RAND, mode="random", seed=1)
    state = {"perm": torch.randperm(b.n_rays, device=dev), "k": 0}

    def old_random():
        k = state["k"]
        state["k"] = (k + 1) % s.n_batches
        return b[state["perm"][k * N_RAND:(k + 1) * N_RAND]]
    new_ms, old_ms = alternate(lambda: next(s), old_random)
    rp = []
    for _ in range(20):
        t0 = time.perf_counter()
        torch.randperm(b.n_rays, device=dev)
        torch.cuda.synchronize()
        rp.append((time.perf_counter() - t0) * 1e3)
    res["random"] = {"new_ms": new_ms, "old_ms": old_ms, "old_randperm_once_per_epoch_ms": stats(rp[5:]), "batches_per_epoch": s.n_batches}
    # ---- images
    res["images"] = {}
    for same in SAMES:
        s = b.sampler(N_RAND, mode="images", same_imgs_size=same, seed=1)
        rule = TorchImageRule(N_IMG, H, W, N_RAND, same, dev)
        new_ms, old_ms = alternate(lambda: next(s), lambda: b[rule.draw()])
        res["images"][f"same_imgs_size={same}"] = {"new_ms": new_ms, "old_ms": old_ms, "pixels_per_image": N_RAND // same,
                                                   "resident_permutation_bytes": N_IMG * H * W * 4}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
