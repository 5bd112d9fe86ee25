"""Training with the distortion loss on the GPU (include/nerfmi_train.h "distortion"): the
three _dist backwards with the weight at 0 against their _bg entries (bit for bit), with the weight on
against float64 autograd of tests/distortion_cases.py's truth on kink-free rays (the GPU within 2x the
float32 oracle's distance + 1e-6, DESIGN.md §14's rule) and against a composition of the stage entry points
(rel-L2 <= 1e-6, DESIGN.md §15's rule), launches of empty rays, the Trainer surface and the CLI.

Inputs and helpers are tests/test_gpu_train_hier.py's and tests/test_gpu_train_background.py's (the
reference's seed-0 weights, o = 0.3 randn, near 2, far 6, explicit t_rand / u_rand).  Every test runs under
both MLP arithmetics where the entry point allows (the occupancy-grid step is f16x3 only).
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO
from oracle import nerf_oracle as O

sys.path.insert(0, os.path.join(REPO, "tests"))
import degenerate_cases as D                    # noqa: E402
import distortion_cases as DC                   # noqa: E402
import occupancy_restated as R                  # noqa: E402
import test_gpu_train_background as TB          # noqa: E402  (helpers only; the tests are collected from their own files)
import test_gpu_train_background_grid as TG     # noqa: E402
import test_gpu_train_hier as H                 # noqa: E402

pytestmark = pytest.mark.gpu
NEAR, FAR, NAN = H.NEAR, H.FAR, float("nan")
NAMES, APP_PROJ = H.NAMES, H.APP_PROJ
rel_l2 = H.rel_l2
WEIGHTS = (0.01, 1.0)


@pytest.fixture(scope="module", autouse=True, params=["f16x3", "f32"])
def arith(request):
    from nerfmi import _lib as L
    prev = L.set_mlp_arith(request.param)
    yield request.param
    L.set_mlp_arith(prev)


def _rows(bg):
    return 0 if bg is None else bg.shape[0]


# ------------------------------------------------------------------------------ the C entries
def dense_dist(packed, packedT, fw, N, app, rows, alpha, bg, aw, dw, near=NEAR, far=FAR):
    """nerf_train_backward_dist on a TB.dense_forward: (gradients, dapp, 3 loss parts, rgb_final)."""
    L = H._lib()
    lib, dev = L.load(), L.device()
    B = fw["rgb_map"].shape[0]
    gs, gptr = H._grad_set(dev)
    dapp = torch.full((rows, 32), NAN, device=dev) if rows else None
    loss, final = torch.full((3,), NAN, device=dev), torch.full((B, 3), NAN, device=dev)
    P = L.ptr
    L.check(lib.nerf_train_backward_dist(P(packed), P(packedT), P(fw["rgb_map"]), P(fw["x"]["target"]), B, N, P(app), rows,
                                         gptr, P(dapp), P(loss), P(fw["ws"]), fw["ws"].numel(), P(alpha), P(bg), _rows(bg),
                                         aw, P(final), dw, near, far, L.stream()), "nerf_train_backward_dist")
    torch.cuda.synchronize()
    return gs, dapp, loss, final


def hier_dist(packed, packedT, fw, N, Nf, cw, app, rows, alpha, bg, aw, dw, near=NEAR, far=FAR):
    """nerf_train_hier_backward_dist on an H.hier_forward: (gradients, dapp, 6 loss parts, final, coarse final)."""
    L = H._lib()
    lib, dev = L.load(), L.device()
    B = fw["rgb_map"].shape[0]
    gs, gptr = H._grad_set(dev)
    dapp = torch.full((rows, 32), NAN, device=dev) if rows else None
    loss = torch.full((6,), NAN, device=dev)
    final, cfinal = torch.full((B, 3), NAN, device=dev), torch.full((B, 3), NAN, device=dev)
    P = L.ptr
    L.check(lib.nerf_train_hier_backward_dist(P(packed), P(packedT), P(fw["rgb_map"]), P(fw["rgb_c"]),
                                              P(fw["x"]["target"]), B, N, Nf, cw, P(app), rows, gptr, P(dapp), P(loss),
                                              P(fw["ws"]), fw["ws"].numel(), P(alpha), P(bg), _rows(bg), aw, P(final),
                                              P(cfinal), dw, near, far, L.stream()), "nerf_train_hier_backward_dist")
    torch.cuda.synchronize()
    return gs, dapp, loss, final, cfinal


def occ_dist(packed, packedT, r, N, app, rows, grid, alpha, bg, aw, dw, entry="dist"):
    """nerf_train_occ_sample / _forward / _backward_dist (entry "bg": _backward_bg): (M_live, rgb_map,
    gradients, dapp, loss parts, final)."""
    L = H._lib()
    lib, dev = L.load(), L.device()
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
    loss, final = torch.full((3 if entry == "dist" else 2,), NAN, device=dev), torch.full((B, 3), NAN, device=dev)
    args = [P(packed), P(packedT), P(rgb_map), P(x["target"]), B, N, m_live, P(app), rows, gptr, P(dapp), P(loss), P(ws),
            ws.numel(), P(alpha), P(bg), _rows(bg), aw, P(final)]
    if entry == "dist":
        L.check(lib.nerf_train_occ_backward_dist(*args, dw, NEAR, FAR, s), "backward_dist")
    else:
        L.check(lib.nerf_train_occ_backward_bg(*args, s), "backward_bg")
    torch.cuda.synchronize()
    return m_live, rgb_map, gs, dapp, loss, final


# ------------------------------------------------------------- the stage compositions (references)
def weights_of(rgb, sigma, z):
    """The weights of (B, n) rows by nerf_composite."""
    L = H._lib()
    B, n = z.shape
    rm, dm, w = torch.empty(B, 3, device=z.device), torch.empty(B, device=z.device), torch.empty(B, n, device=z.device)
    L.check(L.load().nerf_composite(L.ptr(rgb), L.ptr(sigma), L.ptr(z), B, n, L.ptr(rm), L.ptr(dm), L.ptr(w), L.stream()),
            "nerf_composite")
    return w


def distortion_of(w, z, scale):
    """nerf_distortion: (mean over the rays of l in float64, g_w)."""
    L = H._lib()
    B, T = z.shape
    loss, g = torch.empty(B, device=z.device), torch.empty(B, T, device=z.device)
    L.check(L.load().nerf_distortion(L.ptr(w), L.ptr(z), B, T, NEAR, FAR, scale, L.ptr(loss), L.ptr(g), L.stream()),
            "nerf_distortion")
    return loss.double().sum() / B, g


def dense_reference(packed, packedT, st, N, app, rows, alpha, bg, aw, dw):
    L = H._lib()
    lib, dev = L.load(), L.device()
    P, s = L.ptr, L.stream()
    B = st["rgb_map"].shape[0]
    c, z = st["c"], st["z"]
    acc = TB.acc_of(c["rgb"], c["sigma"], z)
    l_dist, g_w = distortion_of(weights_of(c["rgb"], c["sigma"], z), z, dw / B)
    g_rgb, g_acc, l_rgb, l_acc, final = TB.torch_head(st["rgb_map"], acc, st["x"]["target"], alpha, bg, aw, 1.0)
    ds, dr = torch.empty(B * N, device=dev), torch.empty(B * N, 3, device=dev)
    L.check(lib.nerf_composite_backward_grad_w(P(c["rgb"]), P(c["sigma"]), P(z), P(g_rgb), None, B, N, P(ds), P(dr),
                                               P(g_acc), NAN, P(g_w), s), "composite_backward_grad_w")
    gs, dapp = TB.part_grads(packed, packedT, c, B, N, ds, dr, app, rows)
    return gs, dapp, torch.stack([l_rgb, l_acc, l_dist]), final


def hier_reference(packed, packedT, st, N, Nf, cw, app, rows, alpha, bg, aw, dw):
    """TB.hier_reference with each part's distortion term: nerf_distortion on the part's weights (the merged
    ones in merged order), the _w composite backwards."""
    L = H._lib()
    lib, dev = L.load(), L.device()
    P, s = L.ptr, L.stream()
    B, T = st["rgb_map"].shape[0], N + Nf
    c, f, tgt = st["c"], st["f"], st["x"]["target"]
    idx = st["src"].long() & 0xFFFF
    rgb_all = torch.gather(torch.cat([c["rgb"].view(B, N, 3), f["rgb"].view(B, Nf, 3)], 1), 1,
                           idx[..., None].expand(B, T, 3)).contiguous()
    sigma_all = torch.gather(torch.cat([c["sigma"].view(B, N), f["sigma"].view(B, Nf)], 1), 1, idx).contiguous()
    acc_c, acc_f = TB.acc_of(c["rgb"], c["sigma"], st["z"]), TB.acc_of(rgb_all, sigma_all, st["z_all"])
    ld_c, gw_c = distortion_of(weights_of(c["rgb"], c["sigma"], st["z"]), st["z"], cw * dw / B)
    ld_f, gw_f = distortion_of(weights_of(rgb_all, sigma_all, st["z_all"]), st["z_all"], 1.0 * dw / B)
    gc_rgb, gc_acc, lc_rgb, lc_acc, cfinal = TB.torch_head(st["rgb_c"], acc_c, tgt, alpha, bg, aw, cw)
    gf_rgb, gf_acc, lf_rgb, lf_acc, final = TB.torch_head(st["rgb_map"], acc_f, tgt, alpha, bg, aw, 1.0)
    ds_c, dr_c = torch.empty(B * N, device=dev), torch.empty(B * N, 3, device=dev)
    ds_f, dr_f = torch.empty(B * Nf, device=dev), torch.empty(B * Nf, 3, device=dev)
    L.check(lib.nerf_composite_backward_grad_w(P(c["rgb"]), P(c["sigma"]), P(st["z"]), P(gc_rgb), None, B, N, P(ds_c),
                                               P(dr_c), P(gc_acc), NAN, P(gw_c), s), "composite_backward_grad_w")
    L.check(lib.nerf_composite_merged_backward_w(P(c["rgb"]), P(c["sigma"]), P(f["rgb"]), P(f["sigma"]), P(st["src"]),
                                                 P(st["z_all"]), P(gf_rgb), None, B, N, Nf, 1, P(ds_c), P(dr_c), P(ds_f),
                                                 P(dr_f), P(gf_acc), NAN, P(gw_f), s), "composite_merged_backward_w")
    g_c, dapp_c = TB.part_grads(packed, packedT, c, B, N, ds_c, dr_c, app, rows)
    g_f, dapp_f = TB.part_grads(packed, packedT, f, B, Nf, ds_f, dr_f, app, rows)
    gs = [a + b for a, b in zip(g_c, g_f)]
    dapp = dapp_c + dapp_f if rows else None
    return gs, dapp, torch.stack([lf_rgb, lc_rgb, lf_acc, lc_acc, ld_f, ld_c]), final, cfinal


def occ_reference(packed, packedT, r, N, app, mask, alpha, bg, aw, dw):
    """TG.occ_reference with the distortion term on the zero-filled dense rows."""
    L = H._lib()
    lib, dev = L.load(), L.device()
    P, s = L.ptr, L.stream()
    B = r["o"].shape[0]
    M = B * N
    x, dn, z, feat, encd = TG.staged(packed, r, N, app)
    live, _ = TG.live_of(x, dn, z, mask)
    idx, k = R.live_list(live)
    idx = idx.long().to(dev)
    ray = idx // N
    o1, d1, z1 = x["o"][ray].contiguous(), dn[ray].contiguous(), z.reshape(-1)[idx].contiguous()
    f1, e1 = feat[ray].contiguous(), encd[ray].contiguous()
    p = dict(save=torch.empty(L.tile_rows(k), L.SAVE_ROW, device=dev),
             masks=torch.empty(max(k, 1), L.MASK_ROW, dtype=torch.int32, device=dev),
             rgb=torch.empty(max(k, 1), 3, device=dev), sigma=torch.empty(max(k, 1), device=dev))
    L.check(lib.nerf_mlp_forward_train(P(packed), P(o1), P(d1), P(z1), k, 1, P(f1), P(e1), P(p["rgb"]), P(p["sigma"]),
                                       P(p["save"]), P(p["masks"]), s), "mlp_forward_train")
    rgb_d, sig_d = torch.zeros(M, 3, device=dev), torch.zeros(M, device=dev)
    rgb_d[idx], sig_d[idx] = p["rgb"][:k], p["sigma"][:k]
    rgb_map, depth = torch.empty(B, 3, device=dev), torch.empty(B, device=dev)
    L.check(lib.nerf_composite(P(rgb_d), P(sig_d), P(z), B, N, P(rgb_map), P(depth), None, s), "composite")
    acc = TB.acc_of(rgb_d, sig_d, z)
    l_dist, g_w = distortion_of(weights_of(rgb_d, sig_d, z), z, dw / B)
    g_rgb, g_acc, l_rgb, l_acc, final = TB.torch_head(rgb_map, acc, x["target"], alpha, bg, aw, 1.0)
    ds, dr = torch.empty(M, device=dev), torch.empty(M, 3, device=dev)
    L.check(lib.nerf_composite_backward_grad_w(P(rgb_d), P(sig_d), P(z), P(g_rgb), None, B, N, P(ds), P(dr), P(g_acc),
                                               NAN, P(g_w), s), "composite_backward_grad_w")
    gs, dapp = TB.part_grads(packed, packedT, p, k, 1, ds[idx].contiguous(), dr[idx].contiguous(), app, 1)
    torch.cuda.synchronize()
    return k, rgb_map, gs, dapp, torch.stack([l_rgb, l_acc, l_dist]), final, live


def close_parts(loss, ref, what):
    for k in range(ref.numel()):
        assert abs(float(loss[k]) - float(ref[k])) <= 1e-6 * abs(float(ref[k])) + 1e-30, (what, k, float(loss[k]), float(ref[k]))


# ----------------------------------------------------------- 1. weight 0: the _bg entries' bits
@pytest.mark.parametrize("B,N,Nf", [(37, 8, 16), (5, 32, 32)])
def test_weight_zero_is_the_bg_entry(ref_state, app_vec, arith, B, N, Nf):
    L = H._lib()
    dev = L.device()
    packed, packedT = H._packed(ref_state, dev)
    app, rows = H._app(app_vec, B, 1, dev)
    alpha, bg = TB.bg_case(B, seed=B + N)
    for al, b, aw in ((None, None, 0.0), (alpha, bg, 0.1)):
        # (far <= near is not looked at while the weight is 0)
        r = H._rays(B, N, 1, seed=13 * N + B)
        fw = TB.dense_forward(packed, r, N, app, rows)
        gs0, dapp0, loss0, final0 = TB.dense_backward(packed, packedT, fw, N, app, rows, (al, b, aw))
        gs1, dapp1, loss1, final1 = dense_dist(packed, packedT, fw, N, app, rows, al, b, aw, 0.0, near=6.0, far=2.0)
        TB.check_grads(gs1, dapp1, gs0, dapp0, rows, 0, "dense, weight 0", exact=True)
        assert torch.equal(loss1[:2], loss0) and float(loss1[2]) == 0.0 and torch.equal(final1, final0)
        r = H._rays(B, N, Nf, seed=11 * N + Nf)
        fw = H.hier_forward(packed, r, N, Nf, app, rows)
        gs0, dapp0, loss0, final0, cfinal0 = TB.hier_backward_bg(packed, packedT, fw, N, Nf, 0.5, app, rows, al, b, aw)
        gs1, dapp1, loss1, final1, cfinal1 = hier_dist(packed, packedT, fw, N, Nf, 0.5, app, rows, al, b, aw, 0.0)
        TB.check_grads(gs1, dapp1, gs0, dapp0, rows, 0, "hierarchical, weight 0", exact=True)
        assert torch.equal(loss1[:4], loss0) and not bool(loss1[4:].any())
        assert torch.equal(final1, final0) and torch.equal(cfinal1, cfinal0)
        if arith == "f16x3":
            grid, _ = TG.half_space()
            r = H._rays(B, N, 1, seed=17 * N + B + 4)
            m0, map0, gs0, dapp0, loss0, final0 = occ_dist(packed, packedT, r, N, app, rows, grid, al, b, aw, 0.0, "bg")
            m1, map1, gs1, dapp1, loss1, final1 = occ_dist(packed, packedT, r, N, app, rows, grid, al, b, aw, 0.0)
            assert m0 == m1 and torch.equal(map0, map1)
            TB.check_grads(gs1, dapp1, gs0, dapp0, rows, 0, "grid, weight 0", exact=True)
            assert torch.equal(loss1[:2], loss0) and float(loss1[2]) == 0.0 and torch.equal(final1, final0)


# --------------------------------------------------- 2. weight on: the stage composition
@pytest.mark.parametrize("dw", WEIGHTS)
@pytest.mark.parametrize("B,N", [(37, 8), (5, 32)])
def test_dense_step_equals_its_stage_composition(ref_state, app_vec, B, N, dw):
    L = H._lib()
    dev = L.device()
    packed, packedT = H._packed(ref_state, dev)
    app, rows = H._app(app_vec, B, 1, dev)
    r = H._rays(B, N, 1, seed=13 * N + B)
    fw = TB.dense_forward(packed, r, N, app, rows)
    st = TB.dense_stage(packed, r, N, app, rows)
    assert torch.equal(st["rgb_map"], fw["rgb_map"])
    alpha, bg = TB.bg_case(B, seed=B + N)
    # a per-ray background, alpha and an opacity weight: the three terms add; then every _bg option off
    for al, b, aw in ((alpha, bg, 0.1), (None, None, 0.0)):
        gs, dapp, loss, final = dense_dist(packed, packedT, fw, N, app, rows, al, b, aw, dw)
        gs_ref, dapp_ref, loss_ref, final_ref = dense_reference(packed, packedT, st, N, app, rows, al, b, aw, dw)
        torch.cuda.synchronize()
        TB.check_grads(gs, dapp, gs_ref, dapp_ref, rows, 1e-6, ("dense", dw, aw))
        close_parts(loss, loss_ref, ("dense", dw, aw))
        assert torch.equal(final, final_ref) and float(loss[2]) > 0
    # options off: the plain MSE's gradient plus the distortion term's; the term moves the gradients
    gs_mse, dapp_mse, loss_mse, _ = TB.dense_backward(packed, packedT, fw, N, app, rows)
    assert abs(float(loss[0]) - float(loss_mse[0])) <= 1e-6 * float(loss_mse[0])
    assert torch.equal(final, fw["rgb_map"])
    i = NAMES.index("density_head.weight")
    assert rel_l2(gs[i].cpu().numpy(), gs_mse[i].cpu().numpy()) > 1e-4 * dw


@pytest.mark.parametrize("dw", WEIGHTS)
@pytest.mark.parametrize("B,N,Nf", [(37, 8, 16), (5, 32, 32)])
def test_hierarchical_step_equals_its_stage_composition(ref_state, app_vec, B, N, Nf, dw):
    L = H._lib()
    dev = L.device()
    packed, packedT = H._packed(ref_state, dev)
    app, rows = H._app(app_vec, B, 1, dev)
    r = H._rays(B, N, Nf, seed=11 * N + Nf)
    fw = H.hier_forward(packed, r, N, Nf, app, rows)
    st = H.stage_forward(packed, r, N, Nf, app, rows)
    assert torch.equal(fw["rgb_map"], st["rgb_map"]) and torch.equal(fw["rgb_c"], st["rgb_c"])
    alpha, bg = TB.bg_case(B, seed=B + N + Nf)
    cw = 0.5
    for al, b, aw in ((alpha, bg, 0.1), (None, None, 0.0)):
        gs, dapp, loss, final, cfinal = hier_dist(packed, packedT, fw, N, Nf, cw, app, rows, al, b, aw, dw)
        gs_ref, dapp_ref, loss_ref, final_ref, cfinal_ref = hier_reference(packed, packedT, st, N, Nf, cw, app, rows, al, b,
                                                                           aw, dw)
        torch.cuda.synchronize()
        TB.check_grads(gs, dapp, gs_ref, dapp_ref, rows, 1e-6, ("hierarchical", dw, aw))
        close_parts(loss, loss_ref, ("hierarchical", dw, aw))
        assert torch.equal(final, final_ref) and torch.equal(cfinal, cfinal_ref)
        assert float(loss[4]) > 0 and float(loss[5]) > 0
    gs_mse, _, loss_mse = H.hier_backward(packed, packedT, fw, N, Nf, cw, app, rows)
    torch.cuda.synchronize()
    close_parts(loss[:2], loss_mse, "hierarchical, options off")
    i = NAMES.index("density_head.weight")
    assert rel_l2(gs[i].cpu().numpy(), gs_mse[i].cpu().numpy()) > 1e-4 * dw


@pytest.mark.parametrize("dw", WEIGHTS)
def test_grid_step_equals_its_stage_composition(ref_state, app_vec, arith, dw):
    L = H._lib()
    lib, dev = L.load(), L.device()
    B, N = 37, 8
    packed, packedT = H._packed(ref_state, dev)
    app, rows = H._app(app_vec, B, 1, dev)
    if arith != "f16x3":       # the grid step is f16x3 only: the _dist entry refuses like its original
        p_, gptr = L.ptr(packed), H._grad_set(dev)[1]
        rc = lib.nerf_train_occ_backward_dist(p_, p_, p_, p_, B, N, 0, L.ptr(app), rows, gptr, None, p_, p_, 1 << 30, None,
                                              None, 0, 0.0, None, dw, NEAR, FAR, L.stream())
        assert rc == 3 and b"f16x3 only" in lib.nerf_last_error()
        return
    r = H._rays(B, N, 1, seed=17 * N + B + 4)
    grid, mask = TG.half_space()
    alpha, bg = TB.bg_case(B, seed=B + N)
    for al, b, aw in ((alpha, bg, 0.1), (None, None, 0.0)):
        m_live, rgb_map, gs, dapp, loss, final = occ_dist(packed, packedT, r, N, app, rows, grid, al, b, aw, dw)
        k, map_ref, gs_ref, dapp_ref, loss_ref, final_ref, live = occ_reference(packed, packedT, r, N, app, mask, al, b, aw,
                                                                                dw)
        per_ray = live.sum(1)
        assert m_live == k and 0 < k < B * N and bool(((per_ray > 0) & (per_ray < N)).any())
        assert torch.equal(rgb_map, map_ref) and torch.equal(final, final_ref)
        TB.check_grads(gs, dapp, gs_ref, dapp_ref, rows, 1e-6, ("partial grid", dw, aw))
        close_parts(loss, loss_ref, ("partial grid", dw, aw))
        assert float(loss[2]) > 0


# ----------------------------------------------------- 3. weight on: float64 autograd of the truth
def _oracle_step(state, app, o, dn, z, z_all, live, target, alpha, bg, aw, cw, dw, dtype, exp32=None):
    """total = fine part + cw coarse part (dense and grid: z_all None, the coarse part alone with weight 1),
    each part mse(final, target') + aw mse(acc, alpha) + dw mean(l).  float64: DC.composite_distortion_f64 (the
    straight-through composite at the fp32 path's exp, `exp32`); float32: the oracle's composite and the
    same loss expression in fp32.  `live` (B,N) masks the dead samples' sigma and rgb to 0 (the grid step)."""
    st = {k: v.to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    a = None if app is None else app.to(dtype).clone().requires_grad_(True)
    B = o.shape[0]
    al = torch.ones(B, dtype=dtype) if alpha is None else alpha.to(dtype)
    b = torch.zeros(B, 3, dtype=dtype) if bg is None else bg.to(dtype)
    tp = al[:, None] * target.to(dtype) + (1.0 - al)[:, None] * b
    accs = []

    def part(zz, keep):
        n = zz.shape[1]
        pts = (o[:, None, :] + dn[:, None, :] * zz[..., None]).to(dtype)          # formed in fp32
        dexp = dn.to(dtype).unsqueeze(1).expand(-1, n, -1).reshape(-1, 3)
        rgb, sigma = O.nerf_forward(st, pts.reshape(-1, 3), dexp, O._expand_app(a, B, n))
        if keep is not None:
            rgb, sigma = rgb * keep.reshape(-1, 1).to(dtype), sigma * keep.reshape(-1, 1).to(dtype)
        rgb, sigma = rgb.reshape(B, n, 3), sigma.reshape(B, n, 1)
        if dtype == torch.float64:
            rgb_map, acc, l, _ = DC.composite_distortion_f64(rgb, sigma, zz, NEAR, FAR, exp32)
        else:
            rgb_map, _, w = O.composite(rgb, sigma, zz.to(dtype))
            acc, l = w.sum(1)[:, 0], DC.loss_autograd(w[..., 0], zz, NEAR, FAR)
            assert l.dtype == torch.float32
        accs.append(acc.detach())
        final = rgb_map + torch.clamp(1.0 - acc, min=0.0)[:, None] * b
        return F.mse_loss(final, tp) + aw * ((acc - al) ** 2).mean() + dw * l.mean()

    total = part(z, live) if z_all is None else part(z_all, None) + cw * part(z, None)
    total.backward()
    grads = {k: v.grad.detach() for k, v in st.items() if v.grad is not None}
    if a is not None:
        grads["app"] = a.grad.detach().reshape(1, 32)
    return grads, accs


def _check_vs_float64(gs, dapp, args, what):
    """DESIGN.md §14's rule per tensor: the GPU's rel-L2 distance from the float64 truth (at the kernels'
    exp) within 2x the float32 oracle's (from the truth at torch's exp) + 1e-6."""
    g32, _ = _oracle_step(*args, torch.float32)
    g64_cpu, accs = _oracle_step(*args, torch.float64, torch.exp)
    g64_gpu, _ = _oracle_step(*args, torch.float64, D.exp_rn)
    assert all(bool(((1.0 - a).abs() >= 1e-3).all()) for a in accs)              # away from the kink of k
    got = {n: gs[i].cpu().numpy().reshape(-1) for i, n in enumerate(NAMES)}
    got["app"] = dapp.cpu().numpy().reshape(-1)
    worst = 0.0
    for n in g64_gpu:
        e_gpu = rel_l2(got[n], g64_gpu[n].numpy().reshape(-1))
        e_cpu = rel_l2(g32[n].numpy().reshape(-1), g64_cpu[n].numpy().reshape(-1))
        worst = max(worst, e_gpu / (2 * e_cpu + 1e-6))
        assert e_gpu <= 2 * e_cpu + 1e-6, (what, n, e_gpu, e_cpu)
    print(f"{what}: at most {worst:.2f} of the bound 2 e_cpu + 1e-6")


def _kink_free(ref_state, app_vec, packed, B, N, Nf, seed, app, rows):
    """B rays of 16 B candidates whose samples (coarse, and merged when Nf) clear every ReLU kink (no float64
    pre-activation within 1e-5 of its layer's rms of zero: no ReLU branch can differ between the GPU, the
    fp32 CPU and float64 there, assert_branch_flips_bounded's case of zero flips), with dn, z and z_all."""
    L = H._lib()
    lib, dev = L.load(), L.device()
    K = 16 * B
    cand = H._rays(K, N, max(Nf, 1), seed=seed)
    dn = torch.empty(K, 3, device=dev)
    L.check(lib.nerf_normalize_dirs(L.ptr(cand["d"].to(dev).contiguous()), K, L.ptr(dn), L.stream()), "normalize")
    _, _, _, z = H.coarse_forward(packed, cand, N, app, rows)
    zs = [z.cpu()]
    if Nf:
        zs.append(H.hier_forward(packed, cand, N, Nf, app, rows)["z_out"].cpu())
    torch.cuda.synchronize()
    dn = dn.cpu()
    keep = torch.nonzero(H._pre_activations_clear(ref_state, cand["o"], dn, zs, app_vec))[:, 0][:B]
    assert keep.numel() == B, f"fewer than {B} of {K} rays clear the ReLU kinks"
    return H._take(cand, keep), dn[keep], zs[0][keep], (zs[1][keep] if Nf else None)


@pytest.mark.parametrize("dw", WEIGHTS)
@pytest.mark.parametrize("B,N,Nf", [(37, 8, 0), (5, 32, 0), (37, 8, 16), (5, 32, 32)])
def test_steps_match_float64_autograd(ref_state, app_vec, B, N, Nf, dw):
    """Nf = 0: the dense step.  dw = 0.01 with alpha, a per-ray background and acc_weight 0.1 (the three
    terms add); dw = 1 with every _bg option off (the plain MSE plus the distortion term)."""
    L = H._lib()
    dev = L.device()
    packed, packedT = H._packed(ref_state, dev)
    app, rows = H._app(app_vec, B, 1, dev)
    cw = 0.5
    r, dn, z, z_all = _kink_free(ref_state, app_vec, packed, B, N, Nf, 103 * N + Nf, app, rows)
    alpha, bg = TB.bg_case(B, seed=N + Nf)
    al, b, aw = (alpha, bg, 0.1) if dw < 1 else (None, None, 0.0)
    if Nf:
        fw = H.hier_forward(packed, r, N, Nf, app, rows)
        gs, dapp, loss, _, _ = hier_dist(packed, packedT, fw, N, Nf, cw, app, rows, al, b, aw, dw)
        assert torch.equal(fw["z_out"].cpu(), z_all)                 # the kept rays resample as they did
    else:
        fw = TB.dense_forward(packed, r, N, app, rows)
        gs, dapp, loss, _ = dense_dist(packed, packedT, fw, N, app, rows, al, b, aw, dw)
    cpu = lambda t: None if t is None else t.cpu()   # noqa: E731
    args = (ref_state, app_vec, r["o"], dn, z, z_all, None, r["target"], cpu(al), cpu(b), aw, cw, dw)
    _check_vs_float64(gs, dapp, args, f"({B},{N},{Nf}) dw={dw}")
    assert bool(torch.isfinite(loss).all())


@pytest.mark.parametrize("dw", WEIGHTS)
def test_grid_step_matches_float64_autograd(ref_state, app_vec, arith, dw):
    if arith != "f16x3":
        return                                                       # (refused: test_grid_step_equals_its_stage_composition)
    L = H._lib()
    dev = L.device()
    B, N = 37, 8
    packed, packedT = H._packed(ref_state, dev)
    app, rows = H._app(app_vec, B, 1, dev)
    grid, mask = TG.half_space()
    r, dn, z, _ = _kink_free(ref_state, app_vec, packed, B, N, 0, 107 * N, app, rows)
    live = R.classify(r["o"], dn, z, TG.LO, TG.HI, TG.G, mask)
    per_ray = live.sum(1)
    assert bool(((per_ray > 0) & (per_ray < N)).any()) and 0.1 < float(live.float().mean()) < 0.95
    alpha, bg = TB.bg_case(B, seed=N)
    al, b, aw = (alpha, bg, 0.1) if dw < 1 else (None, None, 0.0)
    m_live, _, gs, dapp, loss, _ = occ_dist(packed, packedT, r, N, app, rows, grid, al, b, aw, dw)
    assert m_live == int(live.sum())
    cpu = lambda t: None if t is None else t.cpu()   # noqa: E731
    args = (ref_state, app_vec, r["o"], dn, z, None, live, r["target"], cpu(al), cpu(b), aw, 1.0, dw)
    _check_vs_float64(gs, dapp, args, f"partial grid dw={dw}")
    assert bool(torch.isfinite(loss).all()) and float(loss[2]) > 0


# ------------------------------------------------------------------------ 4. empty rays only
def test_launch_of_empty_rays(ref_state, app_vec, arith):
    """37 rays (4 does not divide it) through a model whose density is 0 everywhere: the distortion loss is
    exactly 0 and the term adds exactly nothing to any gradient (the _bg entry's bits)."""
    L = H._lib()
    dev = L.device()
    B, N, Nf = 37, 8, 16
    st0 = {k: v.clone() for k, v in ref_state.items()}
    st0["density_head.weight"] = torch.zeros_like(st0["density_head.weight"])
    st0["density_head.bias"] = torch.full_like(st0["density_head.bias"], -1.0)
    packed, packedT = H._packed(st0, dev)
    app, rows = H._app(app_vec, B, 1, dev)
    alpha, bg = TB.bg_case(B, seed=5)
    r = H._rays(B, N, Nf, seed=3)
    fw = TB.dense_forward(packed, r, N, app, rows)
    assert not bool(fw["rgb_map"].any())
    gs0, dapp0, loss0, final0 = TB.dense_backward(packed, packedT, fw, N, app, rows, (alpha, bg, 0.1))
    gs1, dapp1, loss1, final1 = dense_dist(packed, packedT, fw, N, app, rows, alpha, bg, 0.1, 1.0)
    TB.check_grads(gs1, dapp1, gs0, dapp0, rows, 0, "empty rays, dense", exact=True)
    assert torch.equal(loss1[:2], loss0) and float(loss1[2]) == 0.0 and torch.equal(final1, final0)
    fw = H.hier_forward(packed, r, N, Nf, app, rows)
    gs0, dapp0, loss0, _, _ = TB.hier_backward_bg(packed, packedT, fw, N, Nf, 0.5, app, rows, alpha, bg, 0.1)
    gs1, dapp1, loss1, _, _ = hier_dist(packed, packedT, fw, N, Nf, 0.5, app, rows, alpha, bg, 0.1, 1.0)
    TB.check_grads(gs1, dapp1, gs0, dapp0, rows, 0, "empty rays, hierarchical", exact=True)
    assert torch.equal(loss1[:4], loss0) and not bool(loss1[4:].any())
    if arith == "f16x3":
        import nerfmi
        zeros = nerfmi.OccupancyGrid((-8.0,) * 3, (8.0,) * 3, 8).from_mask(torch.zeros(8, 8, 8, dtype=torch.bool))
        packed, packedT = H._packed(ref_state, dev)
        m, map_z, gs, _, loss, _ = occ_dist(packed, packedT, r, N, app, rows, zeros, alpha, bg, 0.1, 1.0)
        assert m == 0 and not bool(map_z.any()) and float(loss[2]) == 0.0 and all(not bool(g.any()) for g in gs)


# ------------------------------------------------------------------------------- 5. refusals
def test_refusals(ref_state, app_vec):
    L = H._lib()
    lib, dev = L.load(), L.device()
    B, N = 5, 8
    packed, packedT = H._packed(ref_state, dev)
    app, rows = H._app(app_vec, B, 1, dev)
    fw = TB.dense_forward(packed, H._rays(B, N, 1, seed=1), N, app, rows)
    for dw, near, far, word in ((-0.5, NEAR, FAR, "dist_weight"), (NAN, NEAR, FAR, "dist_weight"), (0.1, 6.0, 2.0, "far"),
                                (0.1, 2.0, 2.0, "far"), (0.1, 2.0, float("inf"), "far")):
        with pytest.raises(RuntimeError, match=word):
            dense_dist(packed, packedT, fw, N, app, rows, None, None, 0.0, dw, near=near, far=far)
    gs, _, loss, _ = dense_dist(packed, packedT, fw, N, app, rows, None, None, 0.0, 0.1)     # still usable after them
    assert bool(torch.isfinite(loss).all()) and all(bool(torch.isfinite(g).all()) for g in gs)


# ------------------------------------------------------------------------------------ 6. Trainer
def _trainer(ref_state, N=16, **kw):
    return H._ref_trainer(ref_state, num_samples=N, **kw)


@pytest.mark.parametrize("kind", ["dense", "hier", "grid"])
def test_trainer_step_is_the_c_calls_and_is_deterministic(ref_state, arith, kind):
    import nerfmi
    from nerfmi.train import random_background
    N, Nf, B, img, aw, cw, dw = 16, 24, 64, 2, 0.1, 0.5, 0.01
    if kind == "grid" and arith != "f16x3":
        return
    r = H._rays(B, N, Nf, seed=5)
    alpha, _ = TB.bg_case(B, seed=3)

    def grid():
        return nerfmi.OccupancyGrid((-8.0,) * 3, (8.0,) * 3, 8).from_mask(torch.ones(8, 8, 8, dtype=torch.bool))

    runs = []
    for _ in range(2):
        kw = dict(hierarchical=True, n_importance=Nf, coarse_loss_weight=cw) if kind == "hier" else {}
        if kind == "grid":
            kw = dict(occupancy=grid())
        tr = _trainer(ref_state, N=N, background="random", acc_weight=aw, distortion_weight=dw, **kw)
        dev = tr.dev
        extra = dict(u_rand=r["u_rand"]) if kind == "hier" else {}
        loss, final = tr.forward_backward(r["o"].to(dev), r["d"].to(dev), r["target"].to(dev), img, t_rand=r["t_rand"],
                                          seed=77, alpha=alpha, **extra)
        torch.cuda.synchronize()
        runs.append((tr.grad.detach().clone(), tr.loss_parts.detach().clone(), final.clone(), float(loss)))
    for a, b in zip(*runs):
        assert (a == b) if isinstance(a, float) else torch.equal(a, b)                 # two identical runs
    grad, parts, final, loss = runs[0]
    assert tr.near == NEAR and tr.far == FAR
    packed, packedT = H._packed(ref_state, dev)
    app = tr.appearance_embeddings[img].reshape(1, 32).clone()
    bg = random_background(B, 77)
    if kind == "hier":
        fw = H.hier_forward(packed, r, N, Nf, app, 1)
        gs, dapp, p, final_c, _ = hier_dist(packed, packedT, fw, N, Nf, cw, app, 1, alpha, bg, aw, dw)
        want = ((p[0] + aw * p[2]) + dw * p[4]) + cw * ((p[1] + aw * p[3]) + dw * p[5])
    elif kind == "dense":
        fw = TB.dense_forward(packed, r, N, app, 1)
        gs, dapp, p, final_c = dense_dist(packed, packedT, fw, N, app, 1, alpha, bg, aw, dw)
        want = (p[0] + aw * p[1]) + dw * p[2]
    else:
        _, _, gs, dapp, p, final_c = occ_dist(packed, packedT, r, N, app, 1, grid(), alpha, bg, aw, dw)
        want = (p[0] + aw * p[1]) + dw * p[2]
    assert parts.shape == (6 if kind == "hier" else 3,) and float(parts[-1]) > 0
    assert torch.equal(parts, p) and torch.equal(final, final_c) and loss == float(want)
    for i, n in enumerate(NAMES):
        assert torch.equal(tr.view(grad, i).reshape(-1), gs[i]), n
    assert torch.equal(tr.view(grad, 24)[img], dapp[0])


def test_trainer_distortion_alone_and_weight_zero(ref_state):
    """distortion_weight alone (no background, no opacity term): the _dist entry with every _bg option off, an
    alpha is still refused; distortion_weight=0 is a trainer built without the argument, bit for bit over three
    steps."""
    N, B = 16, 64
    r = H._rays(B, N, 1, seed=9)

    def three_steps(tr):
        dev = tr.dev
        for i in range(3):
            tr.step(r["o"].to(dev), r["d"].to(dev), r["target"].to(dev), i, t_rand=r["t_rand"])
        torch.cuda.synchronize()
        return tr.flat.detach().cpu().clone(), tr.exp_avg.detach().cpu().clone()

    first = _trainer(ref_state, N=N)
    a = three_steps(first)
    zero = _trainer(ref_state, N=N, distortion_weight=0.0)
    assert not hasattr(zero, "loss_parts") and zero.distortion_weight == 0.0
    z = three_steps(zero)
    assert torch.equal(z[0], a[0]) and torch.equal(z[1], a[1])
    tr = _trainer(ref_state, N=N, distortion_weight=0.5)
    dev = tr.dev
    loss, rgb_map = tr.forward_backward(r["o"].to(dev), r["d"].to(dev), r["target"].to(dev), 1, t_rand=r["t_rand"])
    packed, packedT = H._packed(ref_state, dev)
    app = tr.appearance_embeddings[1].reshape(1, 32).clone()
    fw = TB.dense_forward(packed, r, N, app, 1)
    gs, dapp, parts, final = dense_dist(packed, packedT, fw, N, app, 1, None, None, 0.0, 0.5)
    assert torch.equal(tr.loss_parts, parts) and torch.equal(rgb_map, fw["rgb_map"])
    assert float(loss) == float(parts[0] + 0.0 * parts[1] + 0.5 * parts[2])
    for i, n in enumerate(NAMES):
        assert torch.equal(tr.view(tr.grad, i).reshape(-1), gs[i]), n
    with pytest.raises(ValueError, match="alpha"):
        tr.forward_backward(r["o"].to(dev), r["d"].to(dev), r["target"].to(dev), 1, t_rand=r["t_rand"],
                            alpha=torch.ones(B))
    d = three_steps(tr)
    assert not torch.equal(d[0], a[0])


# ------------------------------------------------------------------------------------- 7. CLI
def test_cli_trains_with_the_distortion_loss(tmp_path, monkeypatch, capsys, arith):
    if arith != "f16x3":
        return                                                       # (the CLI trains under the default arithmetic)
    import run as cli
    monkeypatch.chdir(tmp_path)
    assert cli.main(["--mode", "train", "--random_init", "0", "--distortion_weight", "0.01", "--iterations", "3"]) == 0
    assert "distortion loss, weight 0.01" in capsys.readouterr().out
    ck = torch.load(tmp_path / "checkpoints" / "checkpoint_final.pt", weights_only=False)
    assert ck["iteration"] == 3 and np.isfinite(ck["loss"]) and ck["loss"] > 0      # (the colour part's loss)
