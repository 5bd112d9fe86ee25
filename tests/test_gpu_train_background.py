"""Training with a background, the dataset's alpha channel and an opacity term on the GPU
(include/nerfmi_train.h "training with a background"): the three _bg backwards with the
options off against the original entries (bit for bit), with the options on against a composition of
the stage entry points (rel-L2 <= 1e-6) and against float64 autograd of the oracle on kink-free rays
(the GPU within 2x the float32 oracle's distance + 1e-6, DESIGN.md §14's rule), and the Trainer surface.

Inputs and helpers are tests/test_gpu_train_hier.py's (the reference's seed-0 weights, o = 0.3 randn,
near 2, far 6, explicit t_rand / u_rand); alpha is uniform in [0, 1] with exact 0 and 1 mixed in, the
background one random colour per ray.  Every test runs under both MLP arithmetics where the entry point
allows (the occupancy-grid step is f16x3 only).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO
from oracle import nerf_oracle as O

sys.path.insert(0, os.path.join(REPO, "tests"))
import test_gpu_train_hier as H   # noqa: E402  (its helpers; its tests are collected from its own file)

pytestmark = pytest.mark.gpu
NEAR, FAR = H.NEAR, H.FAR
NAMES, APP_PROJ = H.NAMES, H.APP_PROJ
NAN = float("nan")
rel_l2 = H.rel_l2


@pytest.fixture(scope="module", autouse=True, params=["f16x3", "f32"])
def arith(request):
    from nerfmi import _lib as L
    prev = L.set_mlp_arith(request.param)
    yield request.param
    L.set_mlp_arith(prev)


def bg_case(B, seed):
    """alpha (B,) in [0, 1] with exact 0 and 1, and one background colour per ray, on the device."""
    g = torch.Generator().manual_seed(seed)
    alpha = torch.rand(B, generator=g)
    alpha[0::5] = 0.0
    alpha[1::5] = 1.0
    return alpha.cuda(), torch.rand(B, 3, generator=g).cuda()


def torch_head(rgb_map, acc, target, alpha, bg, aw, weight):
    """bg_loss_kernel's expressions in float32 torch on the device: (g_rgb, g_acc, colour mse, opacity mse,
    final)."""
    B = rgb_map.shape[0]
    k = torch.clamp(1.0 - acc, min=0.0)
    a = torch.ones_like(acc) if alpha is None else alpha
    b = torch.zeros_like(rgb_map) if bg is None else bg.expand(B, 3)
    tp = a[:, None] * target + (1.0 - a)[:, None] * b
    final = rgb_map + k[:, None] * b
    e = final - tp
    g_rgb = e * float(np.float32(weight * 2.0 / (3.0 * B)))
    ea = acc - a
    bgg = b * g_rgb
    dot = (bgg[:, 0] + bgg[:, 1]) + bgg[:, 2]                 # the kernel's order of the three terms
    g_acc = torch.where(k > 0, -dot, torch.zeros_like(acc)) + \
        float(np.float32(aw)) * (float(np.float32(weight * 2.0 / B)) * ea)
    return g_rgb.contiguous(), g_acc.contiguous(), (e.double() ** 2).sum() / (3 * B), (ea.double() ** 2).sum() / B, final


def acc_of(rgb, sigma, z):
    """The opacity of (B, n) rows by nerf_composite_bg."""
    L = H._lib()
    lib = L.load()
    B, n = z.shape
    rm, dm, acc = torch.empty(B, 3, device=z.device), torch.empty(B, device=z.device), torch.empty(B, device=z.device)
    L.check(lib.nerf_composite_bg(L.ptr(rgb), L.ptr(sigma), L.ptr(z), B, n, L.ptr(rm), L.ptr(dm), None, None, 0, NAN,
                                  L.ptr(acc), L.stream()), "nerf_composite_bg")
    return acc


def part_grads(packed, packedT, p, B, n, ds, dr, app, rows):
    """nerf_mlp_backward + nerf_param_grads of one sample set (H.stage_backward's second half)."""
    L = H._lib()
    lib, dev = L.load(), L.device()
    P, s = L.ptr, L.stream()
    M = B * n
    f16 = L.get_mlp_arith() == "f16x3"
    grad = torch.empty(L.tile_rows(M), L.GRAD_ROW, device=dev)
    L.check(lib.nerf_mlp_backward(P(packed), P(packedT), P(p["save"]), P(p["masks"]) if f16 else None, P(p["sigma"]),
                                  P(p["rgb"]), P(ds), P(dr), M, P(grad), s), "mlp_backward")
    gs, gptr = H._grad_set(dev)
    dapp = torch.full((rows, 32), NAN, device=dev) if rows else None
    wsz = lib.nerf_param_grads_workspace_bytes(M)
    ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
    L.check(lib.nerf_param_grads(P(p["save"]), P(grad), M, n, P(app), rows, P(packed), gptr, P(dapp), P(ws), wsz, s),
            "param_grads")
    return gs, dapp


def check_grads(gs, dapp, gs_ref, dapp_ref, rows, tol, what, exact=False):
    for i, name in enumerate(NAMES):
        if rows == 0 and name in APP_PROJ:
            continue
        got, ref = gs[i].cpu().numpy(), gs_ref[i].cpu().numpy()
        assert np.all(np.isfinite(got)), (what, name)
        if exact:
            assert np.array_equal(got.view(np.int32), ref.view(np.int32)), (what, name)
        else:
            assert rel_l2(got, ref) <= tol, (what, name, rel_l2(got, ref))
    if rows:
        if exact:
            assert torch.equal(dapp, dapp_ref), what
        else:
            assert rel_l2(dapp.cpu().numpy(), dapp_ref.cpu().numpy()) <= tol, what


# ------------------------------------------------------------------------------------ dense step
def dense_forward(packed, r, N, app, rows):
    L = H._lib()
    lib, dev = L.load(), L.device()
    B = r["o"].shape[0]
    t_vals, _ = H._tables(N, 1, dev)
    x = {k: v.to(dev).contiguous() for k, v in r.items()}
    need = lib.nerf_train_workspace_bytes(B, N)
    out = dict(ws=torch.empty(need, dtype=torch.uint8, device=dev), rgb_map=torch.empty(B, 3, device=dev),
               depth=torch.empty(B, device=dev), x=x)
    P = L.ptr
    L.check(lib.nerf_train_forward(P(packed), P(x["o"]), P(x["d"]), B, NEAR, FAR, N, P(t_vals), 1, P(x["t_rand"]), 0,
                                   P(app), rows, P(out["rgb_map"]), P(out["depth"]), None, None, P(out["ws"]), need,
                                   L.stream()), "nerf_train_forward")
    return out


def dense_backward(packed, packedT, fw, N, app, rows, bgo=None):
    """nerf_train_backward (bgo None) or nerf_train_backward_bg (bgo = (alpha, bg, aw)): (gradients, dapp,
    loss parts, rgb_final)."""
    L = H._lib()
    lib, dev = L.load(), L.device()
    B = fw["rgb_map"].shape[0]
    gs, gptr = H._grad_set(dev)
    dapp = torch.full((rows, 32), NAN, device=dev) if rows else None
    loss = torch.full((2,), NAN, device=dev)
    final = torch.full((B, 3), NAN, device=dev)
    P = L.ptr
    args = [P(packed), P(packedT), P(fw["rgb_map"]), P(fw["x"]["target"]), B, N, P(app), rows, gptr, P(dapp), P(loss),
            P(fw["ws"]), fw["ws"].numel()]
    if bgo is None:
        L.check(lib.nerf_train_backward(*args, L.stream()), "nerf_train_backward")
    else:
        alpha, bg, aw = bgo
        L.check(lib.nerf_train_backward_bg(*args, P(alpha), P(bg), 0 if bg is None else bg.shape[0], aw, P(final),
                                           L.stream()), "nerf_train_backward_bg")
    torch.cuda.synchronize()
    return gs, dapp, loss, final


def dense_stage(packed, r, N, app, rows):
    """The dense forward from the stage entry points: the sample set's rows and the composite."""
    L = H._lib()
    lib, dev = L.load(), L.device()
    P, s = L.ptr, L.stream()
    B = r["o"].shape[0]
    t_vals, _ = H._tables(N, 1, dev)
    x = {k: v.to(dev).contiguous() for k, v in r.items()}
    dn, z = torch.empty(B, 3, device=dev), torch.empty(B, N, device=dev)
    feat, encd = torch.empty(B, 256, device=dev), torch.empty(B, 32, device=dev)
    L.check(lib.nerf_normalize_dirs(P(x["d"]), B, P(dn), s), "normalize")
    L.check(lib.nerf_sample_stratified(P(x["o"]), P(dn), B, NEAR, FAR, N, P(t_vals), 1, P(x["t_rand"]), 0, P(z), None, s),
            "stratified")
    L.check(lib.nerf_ray_features_train(P(packed), P(dn), B, P(app), rows, P(feat), P(encd), s), "features")
    M = B * N
    c = dict(rgb=torch.empty(M, 3, device=dev), sigma=torch.empty(M, device=dev),
             save=torch.empty(L.tile_rows(M), L.SAVE_ROW, device=dev),
             masks=torch.empty(M, L.MASK_ROW, dtype=torch.int32, device=dev))
    L.check(lib.nerf_mlp_forward_train(P(packed), P(x["o"]), P(dn), P(z), B, N, P(feat), P(encd), P(c["rgb"]),
                                       P(c["sigma"]), P(c["save"]), P(c["masks"]), s), "mlp_forward_train")
    rgb_map, depth = torch.empty(B, 3, device=dev), torch.empty(B, device=dev)
    L.check(lib.nerf_composite(P(c["rgb"]), P(c["sigma"]), P(z), B, N, P(rgb_map), P(depth), None, s), "composite")
    return dict(c=c, z=z, dn=dn, rgb_map=rgb_map, x=x)


def dense_reference(packed, packedT, st, N, app, rows, alpha, bg, aw):
    L = H._lib()
    lib, dev = L.load(), L.device()
    P, s = L.ptr, L.stream()
    B = st["rgb_map"].shape[0]
    c = st["c"]
    acc = acc_of(c["rgb"], c["sigma"], st["z"])
    g_rgb, g_acc, l_rgb, l_acc, final = torch_head(st["rgb_map"], acc, st["x"]["target"], alpha, bg, aw, 1.0)
    ds, dr = torch.empty(B * N, device=dev), torch.empty(B * N, 3, device=dev)
    L.check(lib.nerf_composite_backward_grad_acc(P(c["rgb"]), P(c["sigma"]), P(st["z"]), P(g_rgb), None, B, N, P(ds),
                                                 P(dr), P(g_acc), NAN, s), "composite_backward_grad_acc")
    gs, dapp = part_grads(packed, packedT, c, B, N, ds, dr, app, rows)
    return gs, dapp, torch.stack([l_rgb, l_acc]), final


@pytest.mark.parametrize("B,N", [(37, 8), (5, 32)])
@pytest.mark.parametrize("rows_kind", ["none", "one", "per_ray"])
def test_dense_step(ref_state, app_vec, B, N, rows_kind):
    L = H._lib()
    dev = L.device()
    packed, packedT = H._packed(ref_state, dev)
    app, rows = H._app(app_vec, B, {"none": 0, "one": 1, "per_ray": B}[rows_kind], dev)
    r = H._rays(B, N, 1, seed=13 * N + B)
    fw = dense_forward(packed, r, N, app, rows)
    # options off: the original backward's bits
    gs0, dapp0, loss0, _ = dense_backward(packed, packedT, fw, N, app, rows)
    gs1, dapp1, loss1, final1 = dense_backward(packed, packedT, fw, N, app, rows, (None, None, 0.0))
    check_grads(gs1, dapp1, gs0, dapp0, rows, 0, "options off", exact=True)
    assert torch.equal(loss1[:1], loss0[:1]) and float(loss1[1]) == 0.0 and torch.equal(final1, fw["rgb_map"])
    st = dense_stage(packed, r, N, app, rows)
    assert torch.equal(st["rgb_map"], fw["rgb_map"])
    alpha, bg = bg_case(B, seed=B + N)
    for aw in (0.0, 0.1):
        for al, b in ((alpha, bg), (None, bg[:1].contiguous()), (alpha, None)):
            gs, dapp, loss, final = dense_backward(packed, packedT, fw, N, app, rows, (al, b, aw))
            gs_ref, dapp_ref, loss_ref, final_ref = dense_reference(packed, packedT, st, N, app, rows, al, b, aw)
            torch.cuda.synchronize()
            check_grads(gs, dapp, gs_ref, dapp_ref, rows, 1e-6, (aw, al is None, b is None))
            for k in range(2):
                assert abs(float(loss[k]) - float(loss_ref[k])) <= 1e-6 * float(loss_ref[k]), (aw, k)
            assert torch.equal(final, final_ref)
    # the opacity term alone changes the gradients
    a = dense_backward(packed, packedT, fw, N, app, rows, (alpha, bg, 0.0))[0]
    b_ = dense_backward(packed, packedT, fw, N, app, rows, (alpha, bg, 0.1))[0]
    i = NAMES.index("density_head.weight")
    assert rel_l2(a[i].cpu().numpy(), b_[i].cpu().numpy()) > 1e-3


# ----------------------------------------------------------------------------- hierarchical step
def hier_backward_bg(packed, packedT, fw, N, Nf, cw, app, rows, alpha, bg, aw):
    L = H._lib()
    lib, dev = L.load(), L.device()
    B = fw["rgb_map"].shape[0]
    gs, gptr = H._grad_set(dev)
    dapp = torch.full((rows, 32), NAN, device=dev) if rows else None
    loss = torch.full((4,), NAN, device=dev)
    final, cfinal = torch.full((B, 3), NAN, device=dev), torch.full((B, 3), NAN, device=dev)
    P = L.ptr
    L.check(lib.nerf_train_hier_backward_bg(P(packed), P(packedT), P(fw["rgb_map"]), P(fw["rgb_c"]), P(fw["x"]["target"]),
                                            B, N, Nf, cw, P(app), rows, gptr, P(dapp), P(loss), P(fw["ws"]),
                                            fw["ws"].numel(), P(alpha), P(bg), 0 if bg is None else bg.shape[0], aw,
                                            P(final), P(cfinal), L.stream()), "nerf_train_hier_backward_bg")
    torch.cuda.synchronize()
    return gs, dapp, loss, final, cfinal


def hier_reference(packed, packedT, st, N, Nf, cw, app, rows, alpha, bg, aw):
    """The step's gradients from the stage entry points: per part the opacity (nerf_composite_bg on the
    coarse rows and on the rows gathered through merged_src), the head in torch, the _acc composite
    backwards (the merged one on top of the coarse rows), the MLP backward and the weight gradients."""
    L = H._lib()
    lib, dev = L.load(), L.device()
    P, s = L.ptr, L.stream()
    B, T = st["rgb_map"].shape[0], N + Nf
    c, f, tgt = st["c"], st["f"], st["x"]["target"]
    idx = st["src"].long() & 0xFFFF
    rgb_all = torch.gather(torch.cat([c["rgb"].view(B, N, 3), f["rgb"].view(B, Nf, 3)], 1), 1,
                           idx[..., None].expand(B, T, 3)).contiguous()
    sigma_all = torch.gather(torch.cat([c["sigma"].view(B, N), f["sigma"].view(B, Nf)], 1), 1, idx).contiguous()
    acc_c, acc_f = acc_of(c["rgb"], c["sigma"], st["z"]), acc_of(rgb_all, sigma_all, st["z_all"])
    gc_rgb, gc_acc, lc_rgb, lc_acc, cfinal = torch_head(st["rgb_c"], acc_c, tgt, alpha, bg, aw, cw)
    gf_rgb, gf_acc, lf_rgb, lf_acc, final = torch_head(st["rgb_map"], acc_f, tgt, alpha, bg, aw, 1.0)
    ds_c, dr_c = torch.empty(B * N, device=dev), torch.empty(B * N, 3, device=dev)
    ds_f, dr_f = torch.empty(B * Nf, device=dev), torch.empty(B * Nf, 3, device=dev)
    L.check(lib.nerf_composite_backward_grad_acc(P(c["rgb"]), P(c["sigma"]), P(st["z"]), P(gc_rgb), None, B, N, P(ds_c),
                                                 P(dr_c), P(gc_acc), NAN, s), "composite_backward_grad_acc")
    L.check(lib.nerf_composite_merged_backward_acc(P(c["rgb"]), P(c["sigma"]), P(f["rgb"]), P(f["sigma"]), P(st["src"]),
                                                   P(st["z_all"]), P(gf_rgb), None, B, N, Nf, 1, P(ds_c), P(dr_c),
                                                   P(ds_f), P(dr_f), P(gf_acc), NAN, s),
            "composite_merged_backward_acc")
    g_c, dapp_c = part_grads(packed, packedT, c, B, N, ds_c, dr_c, app, rows)
    g_f, dapp_f = part_grads(packed, packedT, f, B, Nf, ds_f, dr_f, app, rows)
    gs = [a + b for a, b in zip(g_c, g_f)]
    dapp = dapp_c + dapp_f if rows else None
    return gs, dapp, torch.stack([lf_rgb, lc_rgb, lf_acc, lc_acc]), final, cfinal


@pytest.mark.parametrize("B,N,Nf", [(37, 8, 16), (5, 32, 32), (5, 32, 40)])
@pytest.mark.parametrize("rows_kind", ["none", "one", "per_ray"])
def test_hierarchical_step(ref_state, app_vec, B, N, Nf, rows_kind):
    L = H._lib()
    dev = L.device()
    packed, packedT = H._packed(ref_state, dev)
    app, rows = H._app(app_vec, B, {"none": 0, "one": 1, "per_ray": B}[rows_kind], dev)
    r = H._rays(B, N, Nf, seed=11 * N + Nf)
    fw = H.hier_forward(packed, r, N, Nf, app, rows)
    st = H.stage_forward(packed, r, N, Nf, app, rows)
    assert torch.equal(fw["rgb_map"], st["rgb_map"]) and torch.equal(fw["rgb_c"], st["rgb_c"])
    # options off: the original backward's bits
    gs0, dapp0, loss0 = H.hier_backward(packed, packedT, fw, N, Nf, 0.5, app, rows)
    gs1, dapp1, loss1, final1, cfinal1 = hier_backward_bg(packed, packedT, fw, N, Nf, 0.5, app, rows, None, None, 0.0)
    check_grads(gs1, dapp1, gs0, dapp0, rows, 0, "options off", exact=True)
    assert torch.equal(loss1[:2], loss0) and not bool(loss1[2:].any())
    assert torch.equal(final1, fw["rgb_map"]) and torch.equal(cfinal1, fw["rgb_c"])
    alpha, bg = bg_case(B, seed=B + N + Nf)
    for cw, aw in ((1.0, 0.0), (0.25, 0.1)):
        gs, dapp, loss, final, cfinal = hier_backward_bg(packed, packedT, fw, N, Nf, cw, app, rows, alpha, bg, aw)
        gs_ref, dapp_ref, loss_ref, final_ref, cfinal_ref = hier_reference(packed, packedT, st, N, Nf, cw, app, rows,
                                                                           alpha, bg, aw)
        torch.cuda.synchronize()
        check_grads(gs, dapp, gs_ref, dapp_ref, rows, 1e-6, (cw, aw))
        for k in range(4):
            assert abs(float(loss[k]) - float(loss_ref[k])) <= 1e-6 * float(loss_ref[k]), (cw, aw, k)
        assert torch.equal(final, final_ref) and torch.equal(cfinal, cfinal_ref)


# ------------------------------------------------------------------------ whole steps vs float64
def _oracle_step_bg(state, app, o, dn, z, z_all, target, alpha, bg, aw, cw, dtype):
    """total = fine part + cw coarse part (dense: z_all None, the coarse part alone with weight 1), each part
    mse(final, target') + aw mse(acc, alpha), by the oracle's _pass and torch autograd in `dtype`."""
    st = {k: v.to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    a = None if app is None else app.to(dtype).clone().requires_grad_(True)
    al, b, tg = alpha.to(dtype), bg.to(dtype), target.to(dtype)
    tp = al[:, None] * tg + (1.0 - al)[:, None] * b
    accs = []

    def part(zz):
        pts = (o[:, None, :] + dn[:, None, :] * zz[..., None]).to(dtype)          # formed in fp32
        rgb_map, _, w = O._pass(st, pts, dn.to(dtype), zz.to(dtype), a)
        acc = w.sum(1)[:, 0]
        accs.append(acc.detach())
        final = rgb_map + torch.clamp(1.0 - acc, min=0.0)[:, None] * b
        return F.mse_loss(final, tp) + aw * ((acc - al) ** 2).mean()

    total = part(z) if z_all is None else part(z_all) + cw * part(z)
    total.backward()
    grads = {k: v.grad.detach() for k, v in st.items() if v.grad is not None}
    if a is not None:
        grads["app"] = a.grad.detach().reshape(1, 32)
    return grads, accs


def _check_vs_float64(gs, dapp, g32, g64, with_app, what):
    got = {n: gs[i].cpu().numpy().reshape(-1) for i, n in enumerate(NAMES)}
    if with_app:
        got["app"] = dapp.cpu().numpy().reshape(-1)
    worst = 0.0
    for n in g64:
        if not with_app and n in APP_PROJ:
            continue
        e_gpu = rel_l2(got[n], g64[n].numpy().reshape(-1))
        e_cpu = rel_l2(g32[n].numpy().reshape(-1), g64[n].numpy().reshape(-1))
        worst = max(worst, e_gpu / (2 * e_cpu + 1e-6))
        print(f"{what} {n}: rel-L2 vs float64  gpu {e_gpu:.3g}  cpu fp32 {e_cpu:.3g}")
        assert e_gpu <= 2 * e_cpu + 1e-6, (n, e_gpu, e_cpu)
    print(f"{what}: at most {worst:.2f} of the bound")


@pytest.mark.parametrize("N,Nf,R,with_app", [(8, 16, 24, True), (32, 32, 16, False), (8, 0, 24, True), (32, 0, 16, True)])
def test_steps_match_float64_autograd(ref_state, app_vec, N, Nf, R, with_app):
    """Nf = 0: the dense step.  Rays whose samples clear every ReLU kink and keep acc 1e-3 below 1."""
    L = H._lib()
    lib, dev = L.load(), L.device()
    packed, packedT = H._packed(ref_state, dev)
    cw, aw = 0.5, 0.1
    K = 8 * R
    cand = H._rays(K, N, max(Nf, 1), seed=103 * N + Nf)
    app, rows = H._app(app_vec, K, 1 if with_app else 0, dev)
    app_cpu = app_vec if with_app else None
    dn = torch.empty(K, 3, device=dev)
    L.check(lib.nerf_normalize_dirs(L.ptr(cand["d"].to(dev).contiguous()), K, L.ptr(dn), L.stream()), "normalize")
    _, _, _, z = H.coarse_forward(packed, cand, N, app, rows)
    zs = [z.cpu()]
    if Nf:
        fw = H.hier_forward(packed, cand, N, Nf, app, rows)
        zs.append(fw["z_out"].cpu())
    torch.cuda.synchronize()
    dn = dn.cpu()
    keep = torch.nonzero(H._pre_activations_clear(ref_state, cand["o"], dn, zs, app_cpu))[:, 0][:R]
    assert keep.numel() == R
    r = H._take(cand, keep)
    alpha, bg = bg_case(R, seed=N + Nf)
    if Nf:
        fw = H.hier_forward(packed, r, N, Nf, app, rows)
        gs, dapp, loss, _, _ = hier_backward_bg(packed, packedT, fw, N, Nf, cw, app, rows, alpha, bg, aw)
        assert torch.equal(fw["z_out"].cpu(), zs[1][keep])
        z_all = zs[1][keep]
    else:
        fw = dense_forward(packed, r, N, app, rows)
        gs, dapp, loss, _ = dense_backward(packed, packedT, fw, N, app, rows, (alpha, bg, aw))
        z_all = None
    args = (ref_state, app_cpu, r["o"], dn[keep], zs[0][keep], z_all, r["target"], alpha.cpu(), bg.cpu(), aw, cw)
    g32, _ = _oracle_step_bg(*args, torch.float32)
    g64, accs = _oracle_step_bg(*args, torch.float64)
    assert all(bool(((1.0 - a).abs() >= 1e-3).all()) for a in accs)              # away from the kink of k
    _check_vs_float64(gs, dapp, g32, g64, with_app, f"({N},{Nf})")
    assert bool(torch.isfinite(loss).all()) and float(loss.min()) > 0


# --------------------------------------------------------------------------------- grid step
def _occ_calls(lib, L, packed, packedT, r, N, app, rows, grid, bgo):
    """nerf_train_occ_sample / _forward / _backward(_bg): (M_live, rgb_map, gradients, dapp, loss, final)."""
    dev = L.device()
    P, s = L.ptr, L.stream()
    B = r["o"].shape[0]
    t_vals, _ = H._tables(N, 1, dev)
    x = {k: v.to(dev).contiguous() for k, v in r.items()}
    ws = torch.empty(lib.nerf_train_occ_workspace_bytes(B, N), dtype=torch.uint8, device=dev)
    count = torch.full((1,), -7, dtype=torch.int32, device=dev)
    L.check(lib.nerf_train_occ_sample(P(x["o"]), P(x["d"]), B, NEAR, FAR, N, P(t_vals), 1, P(x["t_rand"]), 0, P(grid.bits),
                                      grid.resolution, grid.c_lo(), grid.c_inv(), P(count), P(ws), ws.numel(), s), "sample")
    m_live = int(count.item())
    rgb_map, depth = torch.empty(B, 3, device=dev), torch.empty(B, device=dev)
    L.check(lib.nerf_train_occ_forward(P(packed), P(x["o"]), B, N, m_live, P(app), rows, P(rgb_map), P(depth), None, None,
                                       P(ws), ws.numel(), s), "forward")
    gs, gptr = H._grad_set(dev)
    dapp = torch.full((max(rows, 1), 32), NAN, device=dev) if rows else None
    loss, final = torch.full((2,), NAN, device=dev), torch.full((B, 3), NAN, device=dev)
    args = [P(packed), P(packedT), P(rgb_map), P(x["target"]), B, N, m_live, P(app), rows, gptr, P(dapp), P(loss), P(ws),
            ws.numel()]
    if bgo is None:
        L.check(lib.nerf_train_occ_backward(*args, s), "backward")
    else:
        alpha, bg, aw = bgo
        L.check(lib.nerf_train_occ_backward_bg(*args, P(alpha), P(bg), 0 if bg is None else bg.shape[0], aw, P(final), s),
                "backward_bg")
    torch.cuda.synchronize()
    return m_live, rgb_map, gs, dapp, loss, final


@pytest.mark.parametrize("B,N", [(37, 8), (5, 32)])
def test_grid_step(ref_state, app_vec, arith, B, N):
    import nerfmi
    L = H._lib()
    lib, dev = L.load(), L.device()
    packed, packedT = H._packed(ref_state, dev)
    app, rows = H._app(app_vec, B, 1, dev)
    if arith != "f16x3":       # the grid step is f16x3 only: the _bg entry refuses like its original
        p_, gptr = L.ptr(packed), H._grad_set(dev)[1]
        rc = lib.nerf_train_occ_backward_bg(p_, p_, p_, p_, B, N, 0, L.ptr(app), rows, gptr, None, p_, p_, 1 << 30, None,
                                            None, 0, 0.0, None, L.stream())
        assert rc == 3 and b"f16x3 only" in lib.nerf_last_error()
        return
    r = H._rays(B, N, 1, seed=17 * N + B)
    G = 8
    ones = nerfmi.OccupancyGrid((-8.0,) * 3, (8.0,) * 3, G).from_mask(torch.ones(G, G, G, dtype=torch.bool))
    zeros = nerfmi.OccupancyGrid((-8.0,) * 3, (8.0,) * 3, G).from_mask(torch.zeros(G, G, G, dtype=torch.bool))
    alpha, bg = bg_case(B, seed=B + N)
    # options off: the original entry's bits
    m0, map0, gs0, dapp0, loss0, _ = _occ_calls(lib, L, packed, packedT, r, N, app, rows, ones, None)
    m1, map1, gs1, dapp1, loss1, final1 = _occ_calls(lib, L, packed, packedT, r, N, app, rows, ones, (None, None, 0.0))
    assert m0 == m1 == B * N and torch.equal(map0, map1)
    check_grads(gs1, dapp1, gs0, dapp0, rows, 0, "options off", exact=True)
    assert torch.equal(loss1[:1], loss0[:1]) and float(loss1[1]) == 0.0 and torch.equal(final1, map1)
    # all ones with the options on: the dense _bg step's forward bits, its losses and blended map, and its
    # gradients up to the summation order of the per-row route
    fw = dense_forward(packed, r, N, app, rows)
    assert torch.equal(fw["rgb_map"], map0)
    for aw in (0.0, 0.1):
        _, _, gs, dapp, loss, final = _occ_calls(lib, L, packed, packedT, r, N, app, rows, ones, (alpha, bg, aw))
        gs_d, dapp_d, loss_d, final_d = dense_backward(packed, packedT, fw, N, app, rows, (alpha, bg, aw))
        assert torch.equal(loss, loss_d) and torch.equal(final, final_d)
        # (d sigma and d rgb are the same bits; the weight gradients then run the per-row route: other
        # groupings and block exponents of split-f16 products of relative error 2^-21, so 1e-4 on a
        # tensor's rel-L2 has two orders of margin, while dropping the opacity term moves them by > 1e-3)
        check_grads(gs, dapp, gs_d, dapp_d, rows, 1e-4, ("all ones", aw))
    # all zeros: acc == 0, the blended map is the background, the losses follow, every gradient is zero
    m, map_z, gs, dapp, loss, final = _occ_calls(lib, L, packed, packedT, r, N, app, rows, zeros, (alpha, bg, 0.1))
    assert m == 0 and not bool(map_z.any()) and torch.equal(final, bg)
    tp = alpha[:, None] * r["target"].cuda() + (1.0 - alpha)[:, None] * bg
    assert abs(float(loss[0]) - float(((bg - tp).double() ** 2).mean())) <= 1e-6 * float(loss[0])
    assert abs(float(loss[1]) - float((alpha.double() ** 2).mean())) <= 1e-6 * float(loss[1])
    assert all(not bool(g.any()) for g in gs)


# ------------------------------------------------------------------------------------ Trainer
def _trainer(ref_state, N=16, **kw):
    return H._ref_trainer(ref_state, num_samples=N, **kw)


def test_random_backgrounds():
    """One colour per ray in [0, 1), repeated for the same (step seed, rank), different between steps and
    between ranks."""
    from nerfmi.train import random_background, step_seed
    B = 257
    a = random_background(B, step_seed(1, 0))
    assert a.shape == (B, 3) and float(a.min()) >= 0.0 and float(a.max()) < 1.0
    assert torch.equal(a, random_background(B, step_seed(1, 0)))
    assert not torch.equal(a, random_background(B, step_seed(2, 0)))
    assert not torch.equal(a, random_background(B, step_seed(1, 1)))
    assert len(torch.unique(a)) > B                                   # not one colour for the batch
    assert torch.equal(random_background(7, step_seed(1, 0)), a[:7])  # ray r's colour does not depend on B


@pytest.mark.parametrize("kind", ["dense", "hier", "grid"])
def test_trainer_step_is_the_c_calls_and_is_deterministic(ref_state, arith, kind):
    import nerfmi
    from nerfmi.train import random_background
    N, Nf, B, img, aw, cw = 16, 24, 64, 2, 0.1, 0.5
    r = H._rays(B, N, Nf, seed=5)
    alpha, _ = bg_case(B, seed=3)
    if kind == "grid" and arith != "f16x3":       # the grid step is f16x3 only: refused as without a background
        g8 = nerfmi.OccupancyGrid((-8.0,) * 3, (8.0,) * 3, 8).from_mask(torch.ones(8, 8, 8, dtype=torch.bool))
        tr = _trainer(ref_state, N=N, background="random", occupancy=g8)
        with pytest.raises(ValueError, match="f16x3"):
            tr.forward_backward(r["o"].cuda(), r["d"].cuda(), r["target"].cuda(), img, t_rand=r["t_rand"], alpha=alpha)
        return
    kw = {}
    if kind == "hier":
        kw = dict(hierarchical=True, n_importance=Nf, coarse_loss_weight=cw)

    def grid():
        return nerfmi.OccupancyGrid((-8.0,) * 3, (8.0,) * 3, 8).from_mask(torch.ones(8, 8, 8, dtype=torch.bool))

    runs = []
    for _ in range(2):
        if kind == "grid":
            kw = dict(occupancy=grid())
        tr = _trainer(ref_state, N=N, background="random", acc_weight=aw, **kw)
        dev = tr.dev
        extra = dict(u_rand=r["u_rand"]) if kind == "hier" else {}
        loss, final = tr.forward_backward(r["o"].to(dev), r["d"].to(dev), r["target"].to(dev), img, t_rand=r["t_rand"],
                                          seed=77, alpha=alpha, **extra)
        torch.cuda.synchronize()
        runs.append((tr.grad.detach().clone(), tr.loss_parts.detach().clone(), final.clone(), float(loss)))
    for a, b in zip(*runs):
        assert (a == b) if isinstance(a, float) else torch.equal(a, b)                 # two identical runs
    grad, parts, final, loss = runs[0]
    packed, packedT = H._packed(ref_state, dev)
    app = tr.appearance_embeddings[img].reshape(1, 32).clone()
    bg = random_background(B, 77)
    if kind == "hier":
        fw = H.hier_forward(packed, r, N, Nf, app, 1)
        gs, dapp, parts_c, final_c, _ = hier_backward_bg(packed, packedT, fw, N, Nf, cw, app, 1, alpha, bg, aw)
        want = (parts_c[0] + aw * parts_c[2]) + cw * (parts_c[1] + aw * parts_c[3])
    elif kind == "dense":
        fw = dense_forward(packed, r, N, app, 1)
        gs, dapp, parts_c, final_c = dense_backward(packed, packedT, fw, N, app, 1, (alpha, bg, aw))
        want = parts_c[0] + aw * parts_c[1]
    else:
        L = H._lib()
        _, _, gs, dapp, parts_c, final_c = _occ_calls(L.load(), L, packed, packedT, r, N, app, 1, grid(), (alpha, bg, aw))
        want = parts_c[0] + aw * parts_c[1]
    assert torch.equal(parts, parts_c) and torch.equal(final, final_c) and loss == float(want)
    for i, n in enumerate(NAMES):
        assert torch.equal(tr.view(grad, i).reshape(-1), gs[i]), n
    assert torch.equal(tr.view(grad, 24)[img], dapp[0])


def test_trainer_fixed_background_and_default(ref_state):
    """A fixed colour is one broadcast row; the default trainer has no loss_parts, takes no new path and ends
    on the same parameters before and after a background trainer ran; validation_background()."""
    N, B = 16, 64
    r = H._rays(B, N, 1, seed=9)
    alpha, _ = bg_case(B, seed=4)

    def two_steps(tr, **kw):
        dev = tr.dev
        for i in range(2):
            tr.step(r["o"].to(dev), r["d"].to(dev), r["target"].to(dev), i, t_rand=r["t_rand"], **kw)
        torch.cuda.synchronize()
        return tr.flat.detach().cpu().clone()

    first = _trainer(ref_state, N=N)
    assert not hasattr(first, "loss_parts") and first.validation_background() is None
    a = two_steps(first)
    white = _trainer(ref_state, N=N, background=(1.0, 1.0, 1.0))
    assert white.validation_background() == (1.0, 1.0, 1.0)
    assert _trainer(ref_state, N=N, background="random").validation_background() == (1.0, 1.0, 1.0)
    w = two_steps(white, alpha=alpha)
    assert white.loss_parts.shape == (2,) and float(white.loss_parts[0]) > 0
    second = _trainer(ref_state, N=N)
    assert torch.equal(two_steps(second), a) and not torch.equal(w, a)
    # the fixed colour equals the same colour given per ray through the C entry
    dev = white.dev
    tr = _trainer(ref_state, N=N, background=(0.25, 0.5, 1.0), acc_weight=0.1)
    loss, final = tr.forward_backward(r["o"].to(dev), r["d"].to(dev), r["target"].to(dev), 1, t_rand=r["t_rand"],
                                      alpha=alpha)
    packed, packedT = H._packed(ref_state, dev)
    app = tr.appearance_embeddings[1].reshape(1, 32).clone()
    fw = dense_forward(packed, r, N, app, 1)
    bg = torch.tensor([[0.25, 0.5, 1.0]], device=dev).expand(B, 3).contiguous()
    gs, dapp, parts, final_c = dense_backward(packed, packedT, fw, N, app, 1, (alpha, bg, 0.1))
    assert torch.equal(final, final_c) and torch.equal(tr.loss_parts, parts)
    for i, n in enumerate(NAMES):
        assert torch.equal(tr.view(tr.grad, i).reshape(-1), gs[i]), n
    with pytest.raises(ValueError, match="alpha"):
        tr.forward_backward(r["o"].to(dev), r["d"].to(dev), r["target"].to(dev), 1, t_rand=r["t_rand"], alpha=alpha[:5])
