"""Runs cases of tests/test_gpu_bwd_walk.py in a process of its own: EVD_BWD_OVERLAP, EVD_BWD_OVERLAP_VOXEL and EVD_AWP_BWD_FUSE are read
once per process, and with the side stream on EVD_BWD_OVERLAP is the number of persistent wgrad workgroups.

    python tests/bwd_walk_driver.py cases.json out.npz

cases.json: a list of {"name", "net" (nerf | fine | coarse | awp), "nsamp", "blocks", "sweep", "prec", "keep" (store the raw gradient
arrays), "null_layers" (NeRF: trunk layers whose gradient pointers are null)}.  Per case the network is built with the makers of
evdeblurnerf_amd.weights, the training forward and the backward run, and float64 autograd with the kernel's own ReLU pattern (f16x3: the
true pattern) is the reference.  out.npz: "<name>.<prec>/err/<tensor>" relative L2 errors, "/g/<tensor>" the raw gradients (keep),
"/repeat" 1 when a second backward on the same store gave the same bits in the per-sample outputs, "/finite" 1 when every output is
finite, "/sentinel/<tensor>" 1 when a buffer behind a null pointer kept its fill.  An f16x3 case that misses its bound as drawn: "/plain/"
those errors, "/one_tile/" the errors of its first 6144 samples at one tile per workgroup; only when these miss the bound too, "/ties" the
share of samples whose d raw was then zeroed for a ReLU tie and "/err/" the errors measured after that (run_cases)."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bwd_walk_ref as R  # noqa: E402
from store_decode import A_E0, H0, HV, adecode, decode, vdecode, vstore_slots  # noqa: E402

SENTINEL = 123.25


def _dev(a):
    return torch.tensor(a, device="cuda")


def _dt(prec):
    return torch.float16 if prec == "f16" else torch.bfloat16


def nerf_backward(net, prec, d_raw, store, pts, rb, null_layers=()):
    """evd_nerf_mlp_backward through the C ABI struct -> {key: gradient}, d_pts, d_dirs; the blocks of `null_layers` get null pointers
    (weight and bias) and keep SENTINEL"""
    from evdeblurnerf_amd import _lib as L
    n = d_raw.shape[0]
    blocks = net.param_blocks()
    flat = torch.zeros((net._nparam,), dtype=torch.float32, device="cuda")
    gs = L.NerfGrads()
    gs.accumulate = 0
    for key, shape, off in blocks:
        name, kind = key.rsplit(".", 1)
        field = "_w" if kind == "weight" else "_b"
        if name.startswith("pts_linears."):
            l = int(name.split(".")[1])
            if l in null_layers:
                flat[off:off + int(np.prod(shape))] = SENTINEL
                continue
            getattr(gs, "pts" + field)[l] = flat.data_ptr() + 4 * off
        else:
            head = {"views_linears.0": "views", "feature_linear": "feature", "alpha_linear": "alpha", "rgb_linear": "rgb"}[name]
            setattr(gs, head + field, flat.data_ptr() + 4 * off)
    nb = int(L.lib().evd_nerf_backward_workspace_bytes_net(net._h, L.PREC[prec]))
    ws = torch.empty((nb,), dtype=torch.uint8, device="cuda")
    d_pts, d_dirs = torch.empty((n, 3), device="cuda"), torch.empty((n, 3), device="cuda")
    vd = rb[:, 8:11]
    L.check(L.lib().evd_nerf_mlp_backward(net._h, L.PREC[prec], L.ptr(d_raw), n, 1, L.ptr(store), store.numel(), C.byref(gs), L.ptr(pts),
                                          C.c_void_p(vd.data_ptr()), 11, L.ptr(d_pts), L.ptr(d_dirs), L.ptr(ws), nb, L.stream_ptr()), "evd_nerf_mlp_backward")
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in net.unflatten(flat).items()}
    out["d_pts"], out["d_dirs"] = d_pts.cpu().numpy(), d_dirs.cpu().numpy()
    return out


def run_nerf(case, prec, sd, inp, null_layers=()):
    from evdeblurnerf_amd.nerf import NeRF
    net = NeRF(sd, precision=prec)
    rb, z, pts, d_raw = _dev(inp["rb"]), _dev(inp["z"]), _dev(inp["pts"]), _dev(inp["d_raw"])
    raw, store = net.mlpforward_train(rb, z)
    got = nerf_backward(net, prec, d_raw, store, pts, rb, null_layers)
    again = nerf_backward(net, prec, d_raw, store, pts, rb, null_layers)
    masks = None
    if prec != "f16x3":
        n = case.nsamp
        masks = {f"h{l}": (decode(store, n, H0 + 16 * l, 16, _dt(prec)) > 0).cpu().double() for l in range(8)}
        masks["hv"] = (decode(store, n, HV, 8, _dt(prec)) > 0).cpu().double()
    return got, again, masks


def run_level(case, prec, sd, inp):
    from evdeblurnerf_amd.voxnerf import VoxelNeRFRayFeatures, VoxelNeRFSampleFeatures
    fine = case.net == "fine"
    HD, G, FT, nvox, cls = (256, 128, 64, 48 ** 3, VoxelNeRFSampleFeatures) if fine else (64, 15, 32, 24 ** 3, VoxelNeRFRayFeatures)
    net = cls(sd, "", R.AABB, num_layers=2, hidden_dim=HD, geo_feat_dim=G, num_layers_color=3, input_ch=FT + 63, app_dim=32,
              app_n_comp=(64, 16, 16), n_voxels=nvox, precision=prec)
    pts, vd, fts, d_raw = _dev(inp["pts"]), _dev(inp["vd"]), _dev(inp["fts"]), _dev(inp["d_raw"])
    d_geo = _dev(inp["d_geo"]) if fine else None
    raw, store, _ = net.mlpforward_train(pts, vd, fts, prec, want_feature=fine)

    def backward():
        flat, d_fts, d_pts, d_dirs = net.mlp_backward_flat(d_raw, raw, store, prec, want_fts=True, pts=pts, viewdirs=vd, d_feature=d_geo)
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in net.unflatten(flat).items()}
        out["d_pts"], out["d_dirs"], out["d_fts"] = d_pts.cpu().numpy(), d_dirs.cpu().numpy(), d_fts.cpu().numpy()
        return out

    got, again = backward(), backward()
    HID, C0, C1, TF = vstore_slots(HD, G, FT)
    n, KS = case.nsamp, HD // 16
    masks = {k: (vdecode(store, n, TF, slot, KS, _dt(prec)) > 0).cpu().double() for k, slot in (("hid", HID), ("c0", C0), ("c1", C1))}
    return got, again, masks


def run_awp(case, prec, sd, inp):
    from evdeblurnerf_amd import _lib as L
    from evdeblurnerf_amd.awp import SampleFeatureEmbed
    ws = [sd[f"sample_feature_embed_layer.{l}.weight"] for l in range(4)]
    bs = [sd[f"sample_feature_embed_layer.{l}.bias"] for l in range(4)]
    emb = SampleFeatureEmbed(ws, bs, precision=prec)
    flat = torch.cat([torch.tensor(t).reshape(-1) for l in range(4) for t in (ws[l], bs[l])]).cuda().requires_grad_(True)
    x, d_h = _dev(inp["x"]).requires_grad_(True), _dev(inp["d_h"])
    h = emb(flat, x)
    store, n, lib = h.grad_fn.store, case.nsamp, L.lib()

    def backward():         # evd_awp_embed_backward as awp._SampleEmbed.backward calls it, on the same store
        gflat = torch.zeros((emb.nparam,), dtype=torch.float32, device="cuda")
        gs = L.AwpEmbedGrads()
        for l, (wo, bo) in enumerate(emb.offsets):
            gs.w[l], gs.b[l] = gflat.data_ptr() + 4 * wo, gflat.data_ptr() + 4 * bo
        d_rows = torch.empty((n, 128), dtype=torch.float32, device="cuda")
        nb = int(lib.evd_awp_embed_backward_workspace_bytes())
        wsp = torch.empty((nb,), dtype=torch.uint8, device="cuda")
        L.check(lib.evd_awp_embed_backward(emb._h, L.PREC[prec], L.ptr(d_h), n, L.ptr(store), store.numel(), C.byref(gs), L.ptr(d_rows), None,
                                           L.ptr(wsp), nb, L.stream_ptr()), "evd_awp_embed_backward")
        torch.cuda.synchronize()
        g, out = gflat.cpu().numpy(), {}
        for l, (wo, bo) in enumerate(emb.offsets):
            out[f"w{l}"], out[f"b{l}"] = g[wo:bo].reshape(ws[l].shape), g[bo:bo + 64]
        out["d_geo_rows"] = d_rows.cpu().numpy()
        return out

    got, again = backward(), backward()
    masks = [(adecode(store, n, A_E0 + 4 * l, 4, _dt(prec)) > 0).cpu().double() for l in range(4)]
    return got, again, masks


def _measure(case, prec, sd, inp, nulls=()):
    """one forward + two backwards + the float64 reference -> (gradients, those of the second backward, {tensor: relative L2}, seconds)"""
    t0 = time.time()
    if case.net == "nerf":
        got, again, masks = run_nerf(case, prec, sd, inp, nulls)
    elif case.net == "awp":
        got, again, masks = run_awp(case, prec, sd, inp)
    else:
        got, again, masks = run_level(case, prec, sd, inp)
    t1 = time.time()
    ref = R.reference_chunked(case, sd, inp, masks)
    skipped = [k for k in got if case.net == "nerf" and any(k.startswith(f"pts_linears.{l}.") for l in nulls)]
    return got, again, {k: R.rel_l2(g, ref[k]) for k, g in got.items() if k not in skipped}, (t1 - t0, time.time() - t1)


def _worst(errs, net, prec):
    """(tensor, error / bound) of the tensor closest to (or furthest beyond) its bound"""
    name = max(errs, key=lambda k: errs[k] / R.tol(net, prec, k))
    return name, errs[name] / R.tol(net, prec, name)


def run_cases(specs):
    """-> {key: array} (module docstring)"""
    out, sds = {}, {}
    for spec in specs:
        case = R.Case(spec["name"], spec["net"], spec["nsamp"], spec["blocks"], list(spec["sweep"]))
        prec, nulls = spec["prec"], tuple(spec.get("null_layers", ()))
        key = f"{case.name}.{prec}" + (".null" if nulls else "")
        sd = sds.setdefault(case.net, R.state_dict(case.net))
        inp = R.case_inputs(case)
        got, again, errs, secs = _measure(case, prec, sd, inp, nulls)
        note = ""
        if prec == "f16x3" and _worst(errs, case.net, prec)[1] >= 1.0:
            # The float32-grade mode is held to the TRUE ReLU pattern, and a unit whose pre-activation lies within rounding of zero is
            # decided by rounding.  The bound stays.  Where the same inputs can run at one tile per workgroup in this process (their first
            # 6144 samples: 192 tiles) and miss the bound there TOO, the cause is such a tie and not the walk: d raw is then zeroed on the
            # samples that hold a tie by the float64 reference alone (TAU, at most TIE_CAP of the samples: tests/nerf_generic_ref.py) and
            # the case is measured again.  In every other event the figures stay as drawn and the parent's bound fails the case.
            for k, v in errs.items():
                out[f"{key}/plain/{k}"] = np.float64(v)
            name, ratio = _worst(errs, case.net, prec)
            note = f"; as drawn {ratio:.1f} x the bound ({name})"
            if case.net == "nerf" and case.nsamp > 6144 and R.tiles_of(6144) <= case.blocks:
                one = R.Case(case.name, case.net, 6144, case.blocks, [])
                _, _, e1, _ = _measure(one, prec, sd, {k: v[:6144] for k, v in inp.items()})
                for k, v in e1.items():
                    out[f"{key}/one_tile/{k}"] = np.float64(v)
                name, ratio = _worst(e1, case.net, prec)
                note += f", first 6144 samples at one tile per workgroup {ratio:.1f} x ({name})"
                if ratio >= 1.0:
                    ties = R.nerf_tie_samples(sd, inp)
                    out[f"{key}/ties"] = np.float64(ties.mean())
                    assert ties.mean() <= R.TIE_CAP, (key, ties.mean())
                    inp = dict(inp, d_raw=np.where(ties[:, None, None], np.float32(0), inp["d_raw"]))
                    got, again, errs, secs = _measure(case, prec, sd, inp, nulls)
                    note += f": ReLU ties, {int(ties.sum())} samples with one taken out"
                else:
                    note += ": within the bound there, so no tie exclusion"
        if prec == "f16x3":
            rays = {k: v for k, v in errs.items() if not R.is_param(k)}
            note += "; per-sample gradients " + ", ".join(f"{k} {v:.2e}" for k, v in rays.items())
        for name, g in got.items():
            if name not in errs:
                out[f"{key}/sentinel/{name}"] = np.float64(bool((g == SENTINEL).all()))
                continue
            out[f"{key}/err/{name}"] = np.float64(errs[name])
            if spec.get("keep"):
                out[f"{key}/g/{name}"] = g
        per_sample = [k for k in got if not R.is_param(k)]
        out[f"{key}/repeat"] = np.float64(all(np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)) for k in per_sample))
        out[f"{key}/finite"] = np.float64(all(np.isfinite(g).all() for g in got.values()))
        name, ratio = _worst(errs, case.net, prec)
        print(f"[{key}] {case.nsamp} samples, {R.tiles_of(case.nsamp)} tiles, {case.blocks} workgroups at most: worst error / bound "
              f"{ratio:.3f} ({name}){note}; GPU {secs[0]:.2f} s, float64 reference {secs[1]:.2f} s", flush=True)
    return out


def main():
    with open(sys.argv[1]) as f:
        specs = json.load(f)
    np.savez(sys.argv[2], **run_cases(specs))


if __name__ == "__main__":
    main()
