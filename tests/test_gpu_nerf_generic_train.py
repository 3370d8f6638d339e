"""Training of mode='nerf' networks of any depth, width, skip and encoding (the generic path of evd_nerf_mlp_train / _backward,
EVD_PREC_F16X3) against the float64 restatement of tests/nerf_generic_ref.py, itself pinned to the reference's NeRF class by golden G40.

ReLU ties: a unit whose float64 pre-activation lies within TAU = 2e-6 of zero is decided by rounding in any float32-grade arithmetic, so
d raw is zero on the samples that have one (at most 10 % of a case, asserted on the CPU in tests/test_nerf_generic_ref.py); the forward is
compared on all samples.  Bounds: raw 2e-5 and parameter gradients 5e-6 relative L2 (tests/test_gpu_train_f32grade.py, the project's
bounds for this mode; float32 torch's own error on these cases is 5.8e-7), gradients that reach the rays 2e-4 (same file)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nerf_generic_ref as G
from evdeblurnerf_amd import weights as W
from test_gpu_train import rel_l2
from torch_restatement import nerf_composite

pytestmark = pytest.mark.gpu
DEV = "cuda"


def make_net(name, prec="f16x3"):
    from evdeblurnerf_amd.nerf import NeRF
    D, Wd, L, Lv, skip, _, _, _ = G.CASES[name]
    return NeRF(G.case_state_dict(name), D=D, W=Wd, multires=L, multires_views=Lv, skips=() if skip is None else (skip,),
                precision=prec)


def T(x):
    return torch.tensor(x, device=DEV)


@pytest.mark.parametrize("name", list(G.CASES))
def test_training_forward_is_the_inference_arithmetic(name):
    net = make_net(name)
    rb, z, _ = G.case_inputs(name)
    raw, store = net.mlpforward_train(T(rb), T(z))
    assert torch.equal(raw, net.mlpforward(T(rb), T(z))[0])
    ref = G.case_reference(name)[0]
    err = (raw.reshape(-1, 4).cpu().double() - ref).abs().max().item()
    print(f"[case {name}] max |raw - float64 restatement| = {err:.2e}")
    assert err < 2e-5


@pytest.mark.parametrize("name", list(G.CASES))
def test_parameter_gradients_match_float64_autograd(name):
    net = make_net(name)
    rb, z, _ = G.case_inputs(name)
    _, ref, d_raw, frac = G.case_reference(name)
    raw, store = net.mlpforward_train(T(rb), T(z))
    grads = net.mlp_backward(T(d_raw), store)
    assert set(grads) == set(ref)
    errs = {k: rel_l2(g.cpu().double(), ref[k]) for k, g in grads.items()}
    worst = max(errs, key=errs.get)
    print(f"[case {name}] worst relative L2 error of a parameter gradient vs float64 autograd (true ReLU, {100 * frac:.1f} % of the samples "
          f"zeroed as ties): {worst} {errs[worst]:.2e}")
    assert errs[worst] < 5e-6, {k: f"{v:.1e}" for k, v in errs.items()}


@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_gradients_reach_the_rays(name):
    net = make_net(name)
    sd = G.case_state_dict(name)
    rb_np, z_np, _ = G.case_inputs(name)
    d_raw = G.case_reference(name)[2]
    R, S = z_np.shape
    flat = net.flat_params(sd)
    rb = torch.tensor(rb_np, device=DEV, requires_grad=True)
    raw = net.mlp_train(flat, rb, T(z_np))
    (raw * T(d_raw)).sum().backward()
    rb64 = torch.tensor(rb_np, dtype=torch.float64, requires_grad=True)
    z64 = torch.tensor(z_np, dtype=torch.float64)
    # float32 sample positions, the derivative through the float64 expression (tests/test_gpu_train_f32grade.py:67-72)
    pts32 = torch.tensor(rb_np[:, None, 0:3] + rb_np[:, None, 3:6] * z_np[..., None], dtype=torch.float64)
    expr = rb64[:, None, 0:3] + rb64[:, None, 3:6] * z64[..., None]
    pts = (pts32 + (expr - expr.detach())).reshape(-1, 3)
    dirs = rb64[:, None, 8:11].expand(-1, S, -1).reshape(-1, 3)
    ref = G.case_net(name)
    (ref(pts, dirs) * torch.tensor(d_raw, dtype=torch.float64).reshape(-1, 4)).sum().backward()
    got = rb.grad.cpu().double()
    errs = {"rays_o": rel_l2(got[:, 0:3], rb64.grad[:, 0:3]), "rays_d": rel_l2(got[:, 3:6], rb64.grad[:, 3:6]),
            "viewdirs": rel_l2(got[:, 8:11], rb64.grad[:, 8:11]),
            "parameters": rel_l2(flat.grad.cpu().double(), torch.cat([ref.p[k.replace(".", "_")].grad.reshape(-1) for k, _, _ in net.param_blocks()]))}
    print(f"[case {name}] ray / parameter gradient relative L2 errors vs float64 autograd:", {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) < 2e-4, errs


@pytest.mark.parametrize("name", ["b", "d"])
def test_backward_repeats_bit_for_bit_and_accumulates(name):
    net = make_net(name)
    rb, z, _ = G.case_inputs(name)
    d_raw = T(G.case_reference(name)[2])
    runs = []
    for _ in range(2):
        raw, store = net.mlpforward_train(T(rb), T(z))
        pts = (T(rb)[:, None, 0:3] + T(rb)[:, None, 3:6] * T(z)[..., None]).contiguous()
        runs.append(net.mlp_backward_flat(d_raw, store, pts=pts, ray_batch=T(rb)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    flat = runs[0][0]
    assert flat.abs().max().item() > 0 and bool(torch.isfinite(flat).all())
    known = torch.randn(flat.shape, generator=torch.Generator().manual_seed(3)).to(DEV) * flat.abs().mean()
    buf = known.clone()
    raw, store = net.mlpforward_train(T(rb), T(z))
    assert net.mlp_backward_flat(d_raw, store, accumulate_into=buf) is None
    assert torch.equal(buf, known + flat)


def nerfall_args(N_importance, kernel_type=None):
    return SimpleNamespace(mode="nerf", netdepth=4, netwidth=64, netdepth_fine=6, netwidth_fine=128, multires=6, multires_views=2, use_viewdirs=True,
                           rgb_activate="sigmoid", sigma_activate="relu", N_importance=N_importance, kernel_type=kernel_type)


def nerfall_state_dict(seed):
    ic, icv = W.pe_dim(6), W.pe_dim(2)
    sd = dict(W.prefixed(W.make_nerf_state_dict(seed, 4, 64, input_ch=ic, input_ch_views=icv), "mlp_coarse"))
    sd.update(W.prefixed(W.make_nerf_state_dict(seed + 1, 6, 128, input_ch=ic, input_ch_views=icv), "mlp_fine"))
    return sd


# The coarse-only comparison through the composite: a ray's colour gradient reaches all its samples, so tie samples cannot be taken out
# through d raw as in the per-network tests; instead the colour weight of every RAY that carries a tie sample (float64 pre-activation
# within TAU of zero) is zero.  The same cap holds: at most 10 % of the samples (rays) may be taken out.
def coarse_reference(sd, rays_np, S, w_rgb, rb32):
    """float64: ray packing -> float32 sample positions (from the float32 ray batch rb32 the model packs) -> restated coarse network ->
    composite; returns (rgb, ray gradient, parameter gradients, w_rgb with the tie rays zeroed, fraction of rays zeroed)"""
    from evdeblurnerf_amd.renderer import NeRFAll
    K = W.synthetic_camera()
    rays64 = torch.tensor(rays_np, dtype=torch.float64, requires_grad=True)
    rb64 = NeRFAll.ray_batch_train(400, 400, K, rays64)
    z32 = torch.linspace(0., 1., S).numpy()[None].repeat(rays_np.shape[0], 0)
    z = torch.tensor(z32, dtype=torch.float64)
    pts32 = torch.tensor(rb32[:, None, 0:3] + rb32[:, None, 3:6] * z32[..., None], dtype=torch.float64)
    expr = rb64[:, None, 0:3] + rb64[:, None, 3:6] * z[..., None]
    pts = (pts32 + (expr - expr.detach())).reshape(-1, 3)
    dirs = rb64[:, None, 8:11].expand(-1, S, -1).reshape(-1, 3)
    net = G.GenericNerf(sd, 4, 64, 6, 2, 4, prefix="mlp_coarse.")
    pre = {}
    raw = net(pts, dirs, pre).reshape(-1, S, 4)
    tie_rays = G.tie_samples(pre).reshape(-1, S).any(-1).numpy()
    w_rgb = w_rgb.copy()
    w_rgb[tie_rays] = 0.0
    rgb, _ = nerf_composite(raw, z, rb64[:, 3:6])
    (rgb * torch.tensor(w_rgb, dtype=torch.float64)).sum().backward()
    grads = {"mlp_coarse." + k: net.p[k.replace(".", "_")].grad for k in (kk[len("mlp_coarse."):] for kk in sd if kk.startswith("mlp_coarse."))}
    return rgb.detach(), rays64.grad, grads, w_rgb, float(tie_rays.mean())


@pytest.mark.parametrize("in_place", [False, True])
def test_nerfall_coarse_pass_matches_float64(in_place):
    """NeRFAll in training mode, coarse pass only (no resampling to diverge): rgb within 2e-5, every parameter gradient and the ray gradient
    within 2e-4 of its norm.  Measured: 1.8e-4 on alpha_linear.bias, whose gradient is a cancelling sum of the compositing scan's float32
    d alpha (the sigma head of golden G18 measures 1.6e-4 on the pipelined path for the same reason)."""
    from evdeblurnerf_amd.renderer import NeRFAll
    sd = nerfall_state_dict(620)        # 1 ray of 32 carries a tie sample (seed 600: 4 rays, over the cap)
    R, S = 32, 24
    rays_np = W.synthetic_rays(5, R)
    w_rgb = np.random.RandomState(8).standard_normal((R, 3)).astype(np.float32)
    rb32 = NeRFAll.ray_batch_train(400, 400, W.synthetic_camera(), T(rays_np)).cpu().numpy()       # the packing the model itself runs
    rgb64, rays_g, grads64, w_rgb, frac = coarse_reference(sd, rays_np, S, w_rgb, rb32)
    assert frac <= G.TIE_CAP
    model = NeRFAll(nerfall_args(0), sd, precision="f16x3").enable_training(sd, grads_in_place=in_place).train()
    rays = torch.tensor(rays_np, device=DEV, requires_grad=True)
    rgb, _, _, _ = model(400, 400, W.synthetic_camera(), 1 << 20, rays=rays, ndc=True, near=0., far=1., N_samples=S, N_importance=0, perturb=0.,
                         raw_noise_std=0.)
    err = (rgb.detach().cpu().double() - rgb64).abs().max().item()
    (rgb * T(w_rgb)).sum().backward()
    errs = {k: rel_l2(v.grad.cpu().double(), grads64[k]) for k, v in model.named_parameters() if k in grads64}
    assert set(errs) == set(grads64)
    errs["rays"] = rel_l2(rays.grad.cpu().double(), rays_g)
    worst = max(errs, key=errs.get)
    print(f"[NeRFAll 4 x 64 coarse pass, grads_in_place={in_place}] rgb error {err:.2e}; worst gradient {worst} {errs[worst]:.2e}; {100 * frac:.1f} % of the "
          "rays zeroed as ties")
    assert err < 2e-5
    assert errs[worst] < 2e-4, {k: f"{v:.1e}" for k, v in errs.items()}


def _iteration(model, opt, rays, target, kw):
    rgb, rgb0, _, _ = model(400, 400, W.synthetic_camera(), 1 << 20, rays=rays, **kw)
    loss = ((rgb - target) ** 2).mean() + ((rgb0 - target) ** 2).mean()
    if not model._grads_in_place:
        opt.zero_grad()
    loss.backward()
    return loss


HIER_KW = dict(ndc=True, near=0., far=1., N_samples=24, N_importance=16, perturb=0., raw_noise_std=0.)


@pytest.mark.parametrize("in_place", [False, True])
def test_nerfall_hierarchical_training(in_place):
    """4 x 64 coarse + 6 x 128 fine (skip 4 live in the fine network), (6, 2): one iteration, every leaf gets a finite non-zero gradient, 30 Adam
    steps on a fixed batch lower the loss, the state dict round-trips to the same render; deterministic=True repeats bit for bit."""
    from evdeblurnerf_amd import optim as O
    from evdeblurnerf_amd.renderer import NeRFAll
    sd = nerfall_state_dict(620)
    R = 32
    rays = T(W.synthetic_rays(6, R))
    target = torch.full((R, 3), 0.3, device=DEV)

    def fresh():
        model = NeRFAll(nerfall_args(16), sd, precision="f16x3").enable_training(sd, grads_in_place=in_place, deterministic=True).train()
        assert set(k for k, _ in model.named_parameters()) == set(sd) == set(model.state_dict())
        return model, O.Adam(model.parameters(), lr=2e-3, model=model, zero_grads=in_place)

    model, opt = fresh()
    first = _iteration(model, opt, rays, target, HIER_KW)
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and p.grad.abs().max().item() > 0, k
    g1 = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    opt.step()
    p1 = {k: p.detach().clone() for k, p in model.named_parameters()}
    model2, opt2 = fresh()
    assert torch.equal(_iteration(model2, opt2, rays, target, HIER_KW), first)
    for k, p in model2.named_parameters():
        assert torch.equal(p.grad, g1[k]), k
    opt2.step()
    for k, p in model2.named_parameters():
        assert torch.equal(p.detach(), p1[k]), k
    for _ in range(29):
        loss = _iteration(model, opt, rays, target, HIER_KW)
        opt.step()
    print(f"[NeRFAll 4 x 64 + 6 x 128, grads_in_place={in_place}] loss {first.item():.4e} -> {loss.item():.4e} after 30 Adam steps")
    assert loss.item() < first.item()
    out = model.state_dict()
    fresh_model = NeRFAll(nerfall_args(16), {k: v.cpu().numpy() for k, v in out.items()}, precision="f16x3").eval()
    model.eval()
    kw = dict(ndc=True, near=0., far=1., use_viewdirs=True, N_samples=24, N_importance=16, perturb=0., raw_noise_std=0.)
    a = model.render(400, 400, W.synthetic_camera(), rays=rays, **kw)[0]
    b = fresh_model.render(400, 400, W.synthetic_camera(), rays=rays, **kw)[0]
    assert (a - b).abs().max().item() < 1e-6


def test_forward_train_reaches_a_blur_kernel():
    """forward_train with a kernelsnet in front: the loss gradient crosses both generic networks and the ray packing into the kernel's
    motion parameters"""
    from evdeblurnerf_amd.renderer import NeRFAll
    from test_gpu_train import _ToyRigidKernel
    sd = nerfall_state_dict(620)
    model = NeRFAll(nerfall_args(16, "RBK"), sd, precision="f16x3").train()
    kern = _ToyRigidKernel().cuda()
    model.kernelsnet, model.kernel_type = kern, "RBK"
    pc, pf = model.trainable_parameters(sd)
    R = 16
    rays = T(W.synthetic_rays(3, R))
    rgb, rgb0, _, tens = model.forward_train(400, 400, W.synthetic_camera(), rays, pc, pf, force_naive=False, N_samples=24, N_importance=16, perturb=0.)
    assert rgb.shape == (R, 3)
    (((rgb - 0.3) ** 2).mean() + ((rgb0 - 0.3) ** 2).mean()).backward()
    for p in list(kern.parameters()) + [pc, pf]:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and p.grad.abs().max().item() > 0


@pytest.mark.parametrize("prec,tol", [("f32", 1e-4), ("f16x3", 1e-4), ("f16", 2e-4), ("bf16", 3e-2)])
def test_width_128_inference(prec, tol):
    from evdeblurnerf_amd.nerf import NeRF
    D, Wd, L, Lv, skip = 5, 128, 10, 4, 2
    sd = W.make_nerf_state_dict(481, D, Wd, input_ch=W.pe_dim(L), input_ch_views=W.pe_dim(Lv), skips=(skip,))
    rb, z = G.make_inputs(50, 21, 6)
    net = NeRF(sd, D=D, W=Wd, multires=L, multires_views=Lv, skips=(skip,), precision=prec)
    raw = net.mlpforward(T(rb), T(z))[0]
    with torch.no_grad():
        ref = G.GenericNerf(sd, D, Wd, L, Lv, skip)(*G.positions(rb, z))
    err = (raw.reshape(-1, 4).cpu().double() - ref).abs().max().item()
    print(f"[{prec}, 5 x 128] max |raw - float64 restatement| = {err:.2e}")
    assert err < tol


def test_refusals():
    from evdeblurnerf_amd import _lib as L
    from evdeblurnerf_amd.nerf import NeRF
    rb, z, _ = G.case_inputs("a")
    for prec in ("f16", "bf16", "f16c", "f16m"):
        net = make_net("a", "f16x3")
        with pytest.raises(L.EvdError):
            net.mlpforward_train(T(rb), T(z), precision=prec)
        assert int(L.lib().evd_nerf_train_store_bytes_net(net.handle, L.PREC[prec], 64)) == 0
        assert int(L.lib().evd_nerf_backward_workspace_bytes_net(net.handle, L.PREC[prec])) == 0
        raw, store = net.mlpforward_train(T(rb), T(z))
        with pytest.raises(L.EvdError):
            net.mlp_backward_flat(torch.zeros_like(raw), store, precision=prec)
    sd = W.make_nerf_state_dict(31, 4, 64, use_viewdirs=False)
    nv = NeRF(sd, D=4, W=64, use_viewdirs=False, precision="f16x3")
    with pytest.raises(L.EvdError):
        nv.mlpforward_train(T(rb[:, :8]), T(z))
    assert int(L.lib().evd_nerf_train_store_bytes_net(nv.handle, L.PREC["f16x3"], 64)) == 0
    with pytest.raises(L.EvdError):
        NeRF(W.make_nerf_state_dict(32, 4, 96), D=4, W=96, precision="f16x3")
    w128 = NeRF(W.make_nerf_state_dict(33, 4, 128), D=4, W=128, precision="f16c")          # as at width 64: no f16c stream
    with pytest.raises(L.EvdError):
        w128.mlpforward(T(rb), T(z))
    # the standard network: the per-network queries return what the existing ones return, in every precision
    std = NeRF(W.make_nerf_state_dict(21), precision="f16x3")
    for prec in ("f32", "f16x3", "bf16", "f16", "f16c", "f16m"):
        assert int(L.lib().evd_nerf_train_store_bytes_net(std.handle, L.PREC[prec], 1000)) == int(L.lib().evd_nerf_train_store_bytes_prec(L.PREC[prec], 1000))
    assert int(L.lib().evd_nerf_backward_workspace_bytes_net(std.handle, L.PREC["f16"])) == int(L.lib().evd_nerf_backward_workspace_bytes())
    assert int(L.lib().evd_nerf_backward_workspace_bytes_net(std.handle, L.PREC["f32"])) == 0
