"""Training with a background under a partly occupied grid (nerf_train_occ_backward_bg; DESIGN.md §13 and
§15): rays whose dead samples leave acc < 1 beside live ones, the opacity gradient reaching the live rows
through the gather.  The whole step against the composition of the stage entry points that
tests/test_gpu_train_occupancy.py uses (the N = 1 forward of the live samples scattered into zero-filled
dense rows, nerf_composite_bg, the loss head in torch, nerf_composite_backward_grad_acc, a gather,
nerf_mlp_backward and nerf_param_grads over the live rows; rel-L2 <= 1e-6), and against float64 autograd
of the oracle with the dead samples' sigma and rgb masked to 0, on kink-free rays by DESIGN.md §14's rule
(the GPU within 2x the float32 oracle's distance + 1e-6).  f16x3 throughout (the gathered kernel's
arithmetic; tests/test_gpu_train_background.py holds the refusal under f32).

The grid: 16^3 cells over [-8, 8]^3 with the cells of x < 1 set, so rays heading towards +x lose their
far samples, rays heading away keep all of them, and some lose all.
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
import occupancy_restated as R          # noqa: E402
import test_gpu_train_background as TB  # noqa: E402  (its helpers; its tests are collected from its own file)
import test_gpu_train_hier as H         # noqa: E402

pytestmark = pytest.mark.gpu
NEAR, FAR, NAN = H.NEAR, H.FAR, float("nan")
NAMES = H.NAMES
G, LO, HI = 16, (-8.0,) * 3, (8.0,) * 3


@pytest.fixture(scope="module", autouse=True)
def f16x3():
    from nerfmi import _lib as L
    prev = L.set_mlp_arith("f16x3")
    yield
    L.set_mlp_arith(prev)


def half_space():
    """(grid, mask [iz, iy, ix]): the cells with ix < 9 (x < 1) set."""
    import nerfmi
    mask = np.zeros((G, G, G), bool)
    mask[:, :, :9] = True
    return nerfmi.OccupancyGrid(LO, HI, G).from_mask(torch.from_numpy(mask)), mask


def staged(packed, r, N, app):
    """dn, z, ray features and enc_d of the rays r through the stage entry points (one appearance row)."""
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
    L.check(lib.nerf_ray_features_train(P(packed), P(dn), B, P(app), 1, P(feat), P(encd), s), "features")
    torch.cuda.synchronize()
    return x, dn, z, feat, encd


def live_of(x, dn, z, mask):
    live = R.classify(x["o"].cpu(), dn.cpu(), z.cpu(), LO, HI, G, mask)
    per_ray = live.sum(1)
    return live, per_ray


def occ_reference(packed, packedT, r, N, app, mask, alpha, bg, aw):
    """The step from the stage entry points: (M_live, rgb_map, gradients, dapp, loss parts, final)."""
    L = H._lib()
    lib, dev = L.load(), L.device()
    P, s = L.ptr, L.stream()
    B = r["o"].shape[0]
    M = B * N
    x, dn, z, feat, encd = staged(packed, r, N, app)
    live, _ = live_of(x, dn, z, mask)
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
    g_rgb, g_acc, l_rgb, l_acc, final = TB.torch_head(rgb_map, acc, x["target"], alpha, bg, aw, 1.0)
    ds, dr = torch.empty(M, device=dev), torch.empty(M, 3, device=dev)
    L.check(lib.nerf_composite_backward_grad_acc(P(rgb_d), P(sig_d), P(z), P(g_rgb), None, B, N, P(ds), P(dr), P(g_acc),
                                                 NAN, s), "composite_backward_grad_acc")
    gs, dapp = TB.part_grads(packed, packedT, p, k, 1, ds[idx].contiguous(), dr[idx].contiguous(), app, 1)
    torch.cuda.synchronize()
    return k, rgb_map, gs, dapp, torch.stack([l_rgb, l_acc]), final, acc, live


@pytest.mark.parametrize("B,N", [(37, 8), (5, 32)])
def test_partial_grid_step_equals_its_stage_composition(ref_state, app_vec, B, N):
    L = H._lib()
    lib, dev = L.load(), L.device()
    packed, packedT = H._packed(ref_state, dev)
    app, rows = H._app(app_vec, B, 1, dev)
    r = H._rays(B, N, 1, seed=17 * N + B + 4)     # (seeds at which both shapes hold mixed, all-dead and all-live rays)
    grid, mask = half_space()
    alpha, bg = TB.bg_case(B, seed=B + N)
    for aw in (0.0, 0.1):
        m_live, rgb_map, gs, dapp, loss, final = TB._occ_calls(lib, L, packed, packedT, r, N, app, rows, grid, (alpha, bg, aw))
        k, map_ref, gs_ref, dapp_ref, loss_ref, final_ref, acc, live = occ_reference(packed, packedT, r, N, app, mask,
                                                                                     alpha, bg, aw)
        per_ray = live.sum(1)
        assert m_live == k and 0 < k < B * N
        assert bool(((per_ray > 0) & (per_ray < N)).any())           # rays with dead samples beside live ones
        assert bool((per_ray == 0).any()) and bool((per_ray == N).any())
        assert float(acc.max()) < 1.0 and float(acc.min()) >= 0.0
        assert torch.equal(rgb_map, map_ref) and torch.equal(final, final_ref)
        TB.check_grads(gs, dapp, gs_ref, dapp_ref, rows, 1e-6, ("partial grid", aw))
        for i in range(2):
            assert abs(float(loss[i]) - float(loss_ref[i])) <= 1e-6 * float(loss_ref[i]), (aw, i)
    # the opacity term reaches the live rows through the gather
    a = TB._occ_calls(lib, L, packed, packedT, r, N, app, rows, grid, (alpha, bg, 0.0))[2]
    i = NAMES.index("density_head.weight")
    assert TB.rel_l2(a[i].cpu().numpy(), gs[i].cpu().numpy()) > 1e-3


def _masked_oracle_step(state, app, o, dn, z, live, target, alpha, bg, aw, dtype):
    """mse(final, target') + aw mse(acc, alpha) with the dead samples' sigma and rgb replaced by 0 (a constant
    of the step), by the oracle's NeRF.forward and composite and torch autograd in `dtype`."""
    st = {k: v.to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    a = app.to(dtype).clone().requires_grad_(True)
    B, N = z.shape
    pts = (o[:, None, :] + dn[:, None, :] * z[..., None]).to(dtype)              # formed in fp32
    dexp = dn.to(dtype).unsqueeze(1).expand(-1, N, -1).reshape(-1, 3)
    rgb, sigma = O.nerf_forward(st, pts.reshape(-1, 3), dexp, a.reshape(1, 32).expand(B * N, -1))
    keep = live.reshape(-1, 1).to(dtype)
    rgb_map, _, w = O.composite((rgb * keep).reshape(B, N, 3), (sigma * keep).reshape(B, N, 1), z.to(dtype))
    acc = w.sum(1)[:, 0]
    al, b = alpha.to(dtype), bg.to(dtype)
    tp = al[:, None] * target.to(dtype) + (1.0 - al)[:, None] * b
    final = rgb_map + torch.clamp(1.0 - acc, min=0.0)[:, None] * b
    (F.mse_loss(final, tp) + aw * ((acc - al) ** 2).mean()).backward()
    grads = {k: v.grad.detach() for k, v in st.items() if v.grad is not None}
    grads["app"] = a.grad.detach().reshape(1, 32)
    return grads, acc.detach()


@pytest.mark.parametrize("N,R_", [(8, 24), (32, 16)])
def test_partial_grid_step_matches_float64_autograd(ref_state, app_vec, N, R_):
    L = H._lib()
    lib, dev = L.load(), L.device()
    packed, packedT = H._packed(ref_state, dev)
    aw = 0.1
    K = 8 * R_
    cand = H._rays(K, N, 1, seed=107 * N)
    app, rows = H._app(app_vec, K, 1, dev)
    grid, mask = half_space()
    x, dn, z, _, _ = staged(packed, cand, N, app)
    ok = H._pre_activations_clear(ref_state, cand["o"], dn.cpu(), [z.cpu()], app_vec)
    keep = torch.nonzero(ok)[:, 0][:R_]
    assert keep.numel() == R_
    r = H._take(cand, keep)
    dn, z = dn.cpu()[keep], z.cpu()[keep]
    live = R.classify(r["o"], dn, z, LO, HI, G, mask)
    per_ray = live.sum(1)
    assert bool(((per_ray > 0) & (per_ray < N)).any()) and 0.1 < float(live.float().mean()) < 0.95
    alpha, bg = TB.bg_case(R_, seed=N)
    m_live, _, gs, dapp, loss, _ = TB._occ_calls(lib, L, packed, packedT, r, N, app, rows, grid, (alpha, bg, aw))
    assert m_live == int(live.sum())
    args = (ref_state, app_vec, r["o"], dn, z, live, r["target"], alpha.cpu(), bg.cpu(), aw)
    g32, _ = _masked_oracle_step(*args, torch.float32)
    g64, acc = _masked_oracle_step(*args, torch.float64)
    assert bool(((1.0 - acc).abs() >= 1e-3).all())                               # away from the kink of k
    TB._check_vs_float64(gs, dapp, g32, g64, True, f"partial grid ({N})")
    assert bool(torch.isfinite(loss).all()) and float(loss.min()) > 0
