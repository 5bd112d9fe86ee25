"""Training with the hierarchical fine pass on the GPU (include/nerfmi_train.h "training with the
hierarchical fine pass"): the merged composite's backward against the dense kernel, the
forward against the existing entry points, the whole step against its composition from the stage
entry points and against a float64 autograd of the oracle, and the Trainer surface.

Every test runs under both MLP arithmetics.  Inputs: the reference's seed-0 weights, one appearance
row (and a no-appearance case), rays o = 0.3 randn, d a normalised randn, near 2, far 6 (the
positional encoding stays on its fast path), explicit t_rand / u_rand.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
NEAR, FAR = 2.0, 6.0
NAMES = list(O.STATE_KEYS)
APP_PROJ = ("appearance_projection.weight", "appearance_projection.bias")


@pytest.fixture(scope="module", autouse=True, params=["f16x3", "f32"])
def arith(request):
    from nerfmi import _lib as L
    prev = L.set_mlp_arith(request.param)
    yield request.param
    L.set_mlp_arith(prev)


def _lib():
    from nerfmi import _lib as L
    return L


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _tables(N, Nf, dev):
    from nerfmi.ray_utils import linspace_table
    return linspace_table(N, dev), linspace_table(Nf, dev, drop_last=True)


def _rays(B, N, Nf, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(B, 3, generator=g) * 0.3
    d = F.normalize(torch.randn(B, 3, generator=g), dim=-1)
    return dict(o=o, d=d, t_rand=torch.rand(B, N, generator=g), u_rand=torch.rand(B, Nf, generator=g),
                target=torch.rand(B, 3, generator=g))


def _take(r, idx):
    return {k: v[idx].contiguous() for k, v in r.items()}


def _packed(state, dev):
    L = _lib()
    lib = L.load()
    ts = [state[k].to(dev).float().contiguous() for k in O.STATE_KEYS]
    arr = (ctypes.c_void_p * 24)(*[t.data_ptr() for t in ts])
    packed = torch.empty(lib.nerf_packed_weights_floats(), device=dev)
    packedT = torch.empty(lib.nerf_packed_transposed_floats(), device=dev)
    L.check(lib.nerf_pack_weights(arr, L.ptr(packed), L.stream()), "pack")
    L.check(lib.nerf_pack_weights_transposed(arr, L.ptr(packedT), L.stream()), "packT")
    return packed, packedT


def _app(app, B, rows, dev):
    """(device rows, app_rows) for app_rows in {0, 1, B}: the row itself, or B scaled copies of it."""
    if rows == 0:
        return None, 0
    if rows == 1:
        return app.reshape(1, 32).to(dev).contiguous(), 1
    scale = 1.0 + 0.1 * torch.arange(B, dtype=torch.float32)[:, None]
    return (app.reshape(1, 32) * scale).to(dev).contiguous(), B


def _grad_set(dev):
    gs = [torch.full((n,), float("nan"), device=dev) for n in PARAM_SIZES]
    return gs, (ctypes.c_void_p * 24)(*[g.data_ptr() for g in gs])


PARAM_SIZES = [256 * 63, 256] + [256 * 256, 256] * 3 + [256 * 319, 256] + [256 * 256, 256] * 3 + \
    [256, 1, 128 * 283, 128, 128 * 32, 128, 3 * 128, 3]


def hier_forward(packed, r, N, Nf, app, rows, seed=0):
    """nerf_train_hier_forward on the rays r: every output, the workspace (for the backward)."""
    L = _lib()
    lib, dev = L.load(), L.device()
    B = r["o"].shape[0]
    t_vals, u_lin = _tables(N, Nf, dev)
    x = {k: v.to(dev).contiguous() for k, v in r.items()}
    need = lib.nerf_train_hier_workspace_bytes(B, N, Nf)
    assert need > 0
    out = dict(ws=torch.empty(need, dtype=torch.uint8, device=dev), rgb_map=torch.empty(B, 3, device=dev),
               depth=torch.empty(B, device=dev), weights=torch.empty(B, N + Nf, device=dev),
               z_out=torch.empty(B, N + Nf, device=dev), rgb_c=torch.empty(B, 3, device=dev),
               depth_c=torch.empty(B, device=dev), w_c=torch.empty(B, N, device=dev), x=x)
    P = L.ptr
    L.check(lib.nerf_train_hier_forward(P(packed), P(x["o"]), P(x["d"]), B, NEAR, FAR, N, Nf, P(t_vals), P(u_lin), 1,
                                        P(x["t_rand"]), P(x["u_rand"]), seed, P(app), rows, P(out["rgb_map"]),
                                        P(out["depth"]), P(out["weights"]), P(out["z_out"]), P(out["rgb_c"]),
                                        P(out["depth_c"]), P(out["w_c"]), P(out["ws"]), need, L.stream()),
            "nerf_train_hier_forward")
    return out


def hier_backward(packed, packedT, fw, N, Nf, cw, app, rows):
    """nerf_train_hier_backward on a hier_forward: (24 gradients, dapp or None, the 2 loss parts)."""
    L = _lib()
    lib, dev = L.load(), L.device()
    B = fw["rgb_map"].shape[0]
    gs, gptr = _grad_set(dev)
    dapp = torch.full((rows, 32), float("nan"), device=dev) if rows else None
    loss = torch.zeros(2, device=dev)
    P = L.ptr
    L.check(lib.nerf_train_hier_backward(P(packed), P(packedT), P(fw["rgb_map"]), P(fw["rgb_c"]), P(fw["x"]["target"]),
                                         B, N, Nf, cw, P(app), rows, gptr, P(dapp), P(loss), P(fw["ws"]),
                                         fw["ws"].numel(), L.stream()), "nerf_train_hier_backward")
    return gs, dapp, loss


def coarse_forward(packed, r, N, app, rows, seed=0):
    """nerf_train_forward on the same rays: (rgb_map, depth, weights, z)."""
    L = _lib()
    lib, dev = L.load(), L.device()
    B = r["o"].shape[0]
    t_vals, _ = _tables(N, 1, dev)
    o, d, t = (r[k].to(dev).contiguous() for k in ("o", "d", "t_rand"))
    need = lib.nerf_train_workspace_bytes(B, N)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rgb, depth = torch.empty(B, 3, device=dev), torch.empty(B, device=dev)
    w, z = torch.empty(B, N, device=dev), torch.empty(B, N, device=dev)
    P = L.ptr
    L.check(lib.nerf_train_forward(P(packed), P(o), P(d), B, NEAR, FAR, N, P(t_vals), 1, P(t), seed, P(app), rows,
                                   P(rgb), P(depth), P(w), P(z), P(ws), need, L.stream()), "nerf_train_forward")
    return rgb, depth, w, z


def stage_forward(packed, r, N, Nf, app, rows, seed=0):
    """The hierarchical forward composed from the stage entry points: both parts' forward with saves,
    the resample with its source map, a torch scatter into merged rows and nerf_composite."""
    L = _lib()
    lib, dev = L.load(), L.device()
    B = r["o"].shape[0]
    T = N + Nf
    P, s = L.ptr, L.stream()
    t_vals, u_lin = _tables(N, Nf, dev)
    x = {k: v.to(dev).contiguous() for k, v in r.items()}
    dn, z = torch.empty(B, 3, device=dev), torch.empty(B, N, device=dev)
    feat, encd = torch.empty(B, 256, device=dev), torch.empty(B, 32, device=dev)
    L.check(lib.nerf_normalize_dirs(P(x["d"]), B, P(dn), s), "normalize")
    L.check(lib.nerf_sample_stratified(P(x["o"]), P(dn), B, NEAR, FAR, N, P(t_vals), 1, P(x["t_rand"]), seed, P(z), None,
                                       s), "stratified")
    L.check(lib.nerf_ray_features_train(P(packed), P(dn), B, P(app), rows, P(feat), P(encd), s), "features")

    def part(zz, n):
        M = B * n
        p = dict(rgb=torch.empty(M, 3, device=dev), sigma=torch.empty(M, device=dev),
                 save=torch.empty(L.tile_rows(M), L.SAVE_ROW, device=dev),
                 masks=torch.empty(M, L.MASK_ROW, dtype=torch.int32, device=dev))
        L.check(lib.nerf_mlp_forward_train(P(packed), P(x["o"]), P(dn), P(zz), B, n, P(feat), P(encd), P(p["rgb"]),
                                           P(p["sigma"]), P(p["save"]), P(p["masks"]), s), "mlp_forward_train")
        return p

    c = part(z, N)
    rgb_c, depth_c, w_c = torch.empty(B, 3, device=dev), torch.empty(B, device=dev), torch.empty(B, N, device=dev)
    L.check(lib.nerf_composite(P(c["rgb"]), P(c["sigma"]), P(z), B, N, P(rgb_c), P(depth_c), P(w_c), s), "composite")
    z_all, z_fine = torch.empty(B, T, device=dev), torch.empty(B, Nf, device=dev)
    src = torch.empty(B, T, dtype=torch.int16, device=dev)
    L.check(lib.nerf_sample_importance_src(P(z), P(w_c), B, N, Nf, P(u_lin), P(x["u_rand"]), seed, P(z_all), P(z_fine),
                                           P(src), s), "importance_src")
    f = part(z_fine, Nf)
    idx = src.long() & 0xFFFF
    rgb_all = torch.gather(torch.cat([c["rgb"].view(B, N, 3), f["rgb"].view(B, Nf, 3)], 1), 1,
                           idx[..., None].expand(B, T, 3)).contiguous()
    sigma_all = torch.gather(torch.cat([c["sigma"].view(B, N), f["sigma"].view(B, Nf)], 1), 1, idx).contiguous()
    rgb_map, depth, w = torch.empty(B, 3, device=dev), torch.empty(B, device=dev), torch.empty(B, T, device=dev)
    L.check(lib.nerf_composite(P(rgb_all), P(sigma_all), P(z_all), B, T, P(rgb_map), P(depth), P(w), s), "composite")
    return dict(c=c, f=f, z=z, z_all=z_all, z_fine=z_fine, src=src, rgb_c=rgb_c, depth_c=depth_c, w_c=w_c,
                rgb_map=rgb_map, depth=depth, weights=w, x=x, dn=dn)


def stage_backward(packed, packedT, st, N, Nf, cw, app, rows, fine_only=False):
    """The step's gradients composed from the stage entry points: per part the composite backward (the
    dense one on the coarse rows, the merged one on top), nerf_mlp_backward and nerf_param_grads, then
    a torch add of the two parts.  fine_only: the fine part's gradients alone (the coarse rows' terms
    dropped).  Returns (24 gradients, dapp or None, the 2 loss parts)."""
    L = _lib()
    lib, dev = L.load(), L.device()
    P, s = L.ptr, L.stream()
    B = st["rgb_map"].shape[0]
    tgt = st["x"]["target"]
    # the library's g: its float scale times the float error
    scale_c, scale_f = float(np.float32(cw * (2.0 / (3.0 * B)))), float(np.float32(2.0 / (3.0 * B)))
    e_c, e_f = st["rgb_c"] - tgt, st["rgb_map"] - tgt
    g_c, g_f = (e_c * scale_c).contiguous(), (e_f * scale_f).contiguous()
    c, f = st["c"], st["f"]
    ds_c, dr_c = torch.empty(B * N, device=dev), torch.empty(B * N, 3, device=dev)
    ds_f, dr_f = torch.empty(B * Nf, device=dev), torch.empty(B * Nf, 3, device=dev)
    L.check(lib.nerf_composite_backward_grad(P(c["rgb"]), P(c["sigma"]), P(st["z"]), P(g_c), None, B, N, P(ds_c),
                                             P(dr_c), s), "composite_backward_grad")
    L.check(lib.nerf_composite_merged_backward(P(c["rgb"]), P(c["sigma"]), P(f["rgb"]), P(f["sigma"]), P(st["src"]),
                                               P(st["z_all"]), P(g_f), None, B, N, Nf, 1, P(ds_c), P(dr_c), P(ds_f),
                                               P(dr_f), s), "composite_merged_backward")
    f16 = L.get_mlp_arith() == "f16x3"
    sets = []
    for p, n, ds, dr in ((c, N, ds_c, dr_c), (f, Nf, ds_f, dr_f)):
        M = B * n
        grad = torch.empty(L.tile_rows(M), L.GRAD_ROW, device=dev)
        L.check(lib.nerf_mlp_backward(P(packed), P(packedT), P(p["save"]), P(p["masks"]) if f16 else None, P(p["sigma"]),
                                      P(p["rgb"]), P(ds), P(dr), M, P(grad), s), "mlp_backward")
        gs, gptr = _grad_set(dev)
        dapp = torch.full((rows, 32), float("nan"), device=dev) if rows else None
        wsz = lib.nerf_param_grads_workspace_bytes(M)
        ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
        L.check(lib.nerf_param_grads(P(p["save"]), P(grad), M, n, P(app), rows, P(packed), gptr, P(dapp), P(ws), wsz, s),
                "param_grads")
        sets.append((gs, dapp))
    if fine_only:
        gs, dapp = sets[1]
    else:
        gs = [a + b for a, b in zip(sets[0][0], sets[1][0])]
        dapp = sets[0][1] + sets[1][1] if rows else None
    loss = torch.stack([(e_f.double() ** 2).sum() / (3 * B), (e_c.double() ** 2).sum() / (3 * B)])
    return gs, dapp, loss


# ------------------------------------------------------------- 1. merged backward against the dense one
@pytest.mark.parametrize("B,N,Nf", [(37, 8, 16), (5, 32, 40), (3, 256, 1024)])
@pytest.mark.parametrize("with_depth", [False, True])
def test_merged_backward_equals_the_dense_kernel_on_merged_rows(B, N, Nf, with_depth):
    """composite_merged_backward_kernel keeps composite_backward_kernel's arithmetic AND its scan order
    (one wave per ray, 64 positions per chunk): on rows gathered through merged_src the two agree bit for
    bit.  The bound the interface promises (one float ulp plus 1e-12 of the tensor's largest entry, what a
    reordered double scan of T <= 1,280 factors could move) is asserted first, then the equality."""
    L = _lib()
    lib, dev = L.load(), L.device()
    P, s = L.ptr, L.stream()
    T = N + Nf
    g = torch.Generator().manual_seed(1000 * N + Nf)
    rgb_c, rgb_f = torch.rand(B, N, 3, generator=g).to(dev), torch.rand(B, Nf, 3, generator=g).to(dev)
    sig_c = F.relu(torch.randn(B, N, generator=g) * 3).to(dev)
    sig_f = F.relu(torch.randn(B, Nf, generator=g) * 3).to(dev)
    z = torch.sort(2 + 4 * torch.rand(B, N, generator=g), dim=-1).values.to(dev)
    w = torch.rand(B, N, generator=g).to(dev)
    u = torch.rand(B, Nf, generator=g).to(dev)
    g_map = torch.randn(B, 3, generator=g).to(dev)
    g_depth = torch.randn(B, generator=g).to(dev) if with_depth else None
    _, u_lin = _tables(N, Nf, dev)
    z_all, z_fine = torch.empty(B, T, device=dev), torch.empty(B, Nf, device=dev)
    src = torch.empty(B, T, dtype=torch.int16, device=dev)
    L.check(lib.nerf_sample_importance_src(P(z), P(w), B, N, Nf, P(u_lin), P(u), 0, P(z_all), P(z_fine), P(src), s),
            "importance_src")
    idx = src.long() & 0xFFFF
    assert torch.equal(torch.sort(idx, dim=1).values, torch.arange(T, device=dev).expand(B, T))   # a permutation per ray
    # the dense kernel on the merged rows, gathered back to cat[coarse, fine] order
    rgb_m = torch.gather(torch.cat([rgb_c, rgb_f], 1), 1, idx[..., None].expand(B, T, 3)).contiguous()
    sig_m = torch.gather(torch.cat([sig_c, sig_f], 1), 1, idx).contiguous()
    ds_m, dr_m = torch.empty(B, T, device=dev), torch.empty(B, T, 3, device=dev)
    L.check(lib.nerf_composite_backward_grad(P(rgb_m), P(sig_m), P(z_all), P(g_map), P(g_depth), B, T, P(ds_m), P(dr_m),
                                             s), "composite_backward_grad")
    ref_ds = torch.empty_like(ds_m).scatter_(1, idx, ds_m)
    ref_dr = torch.empty_like(dr_m).scatter_(1, idx[..., None].expand(B, T, 3), dr_m)

    def run(acc, ds_c, dr_c):
        ds_f, dr_f = torch.full((B, Nf), float("nan"), device=dev), torch.full((B, Nf, 3), float("nan"), device=dev)
        L.check(lib.nerf_composite_merged_backward(P(rgb_c), P(sig_c), P(rgb_f), P(sig_f), P(src), P(z_all), P(g_map),
                                                   P(g_depth), B, N, Nf, acc, P(ds_c), P(dr_c), P(ds_f), P(dr_f), s),
                "composite_merged_backward")
        return ds_f, dr_f

    ds_c, dr_c = torch.full((B, N), float("nan"), device=dev), torch.full((B, N, 3), float("nan"), device=dev)
    ds_f, dr_f = run(0, ds_c, dr_c)
    torch.cuda.synchronize()
    for got, ref, name in ((torch.cat([ds_c, ds_f], 1), ref_ds, "dsigma"), (torch.cat([dr_c, dr_f], 1), ref_dr, "drgb")):
        got64, ref64 = got.double().cpu(), ref.double().cpu()
        err = (got64 - ref64).abs()
        bound = 2.0 ** -23 * ref64.abs() + 1e-12 * ref64.abs().max()
        differ = int((got.cpu() != ref.cpu()).sum())
        print(f"{name} ({B},{N},{Nf}) depth={with_depth}: max err {float(err.max()):.3g}, {differ} elements differ")
        assert torch.isfinite(got64).all(), name
        assert bool((err <= bound).all()), (name, float((err - bound).max()))
        assert differ == 0, (name, differ)                  # the dense kernel's scan order: the same bits
    assert float(ref_ds.abs().max()) > 0 and float(ref_dr.abs().max()) > 0
    # accumulate_coarse: coarse rows = prefill + term in one float add, fine rows as before
    pre_s, pre_r = torch.randn(B, N, generator=g).to(dev), torch.randn(B, N, 3, generator=g).to(dev)
    acc_s, acc_r = pre_s.clone(), pre_r.clone()
    ds_f2, dr_f2 = run(1, acc_s, acc_r)
    torch.cuda.synchronize()
    assert torch.equal(acc_s, pre_s + ds_c) and torch.equal(acc_r, pre_r + dr_c)
    assert torch.equal(ds_f2, ds_f) and torch.equal(dr_f2, dr_f)


# ------------------------------------------------------------------------------- 2. forward reuse
@pytest.mark.parametrize("B,N,Nf", [(37, 8, 16), (5, 32, 32)])
@pytest.mark.parametrize("with_app", [True, False])
def test_forward_reuses_the_existing_stages_bit_for_bit(ref_state, app_vec, B, N, Nf, with_app):
    L = _lib()
    dev = L.device()
    packed, _ = _packed(ref_state, dev)
    app, rows = _app(app_vec, B, 1 if with_app else 0, dev)
    r = _rays(B, N, Nf, seed=7 * N + Nf)
    fw = hier_forward(packed, r, N, Nf, app, rows)
    rgb_c, depth_c, w_c, z = coarse_forward(packed, r, N, app, rows)
    st = stage_forward(packed, r, N, Nf, app, rows)
    torch.cuda.synchronize()
    # the coarse pass is nerf_train_forward's
    assert torch.equal(fw["rgb_c"], rgb_c) and torch.equal(fw["depth_c"], depth_c) and torch.equal(fw["w_c"], w_c)
    # z_all is the oracle's resample of the GPU's own coarse weights (F5: bit-exact given the same weights)
    z_ref, _ = O.sample_importance_h1(r["o"], r["d"], z.cpu(), w_c.cpu(), Nf, r["u_rand"])
    assert torch.equal(fw["z_out"].cpu(), z_ref)
    # the merged outputs are the stage composition's
    assert torch.equal(st["z"], z) and torch.equal(st["z_all"], fw["z_out"])
    for k in ("rgb_map", "depth", "weights"):
        assert torch.equal(fw[k], st[k]), k
    assert float(fw["weights"].sum()) > 0


# ------------------------------------------------------- 3. whole step against its stage composition
@pytest.mark.parametrize("B,N,Nf", [(37, 8, 16), (5, 32, 32), (5, 32, 40)])
@pytest.mark.parametrize("rows_kind", ["none", "one", "per_ray"])
def test_step_equals_its_stage_composition(ref_state, app_vec, B, N, Nf, rows_kind):
    """(5, 32, 40) sends the fine part down the non-fused ray-sum route.  Both sides run the same
    kernels on the same rows and may differ only in the order of the final two-term float sums."""
    L = _lib()
    dev = L.device()
    packed, packedT = _packed(ref_state, dev)
    app, rows = _app(app_vec, B, {"none": 0, "one": 1, "per_ray": B}[rows_kind], dev)
    r = _rays(B, N, Nf, seed=11 * N + Nf)
    fw = hier_forward(packed, r, N, Nf, app, rows)
    st = stage_forward(packed, r, N, Nf, app, rows)
    assert torch.equal(fw["rgb_map"], st["rgb_map"]) and torch.equal(fw["rgb_c"], st["rgb_c"])
    for cw in (1.0, 0.0, 0.25):
        gs, dapp, loss = hier_backward(packed, packedT, fw, N, Nf, cw, app, rows)
        gs_ref, dapp_ref, loss_ref = stage_backward(packed, packedT, st, N, Nf, cw, app, rows)
        torch.cuda.synchronize()
        for i, name in enumerate(NAMES):
            if rows == 0 and name in APP_PROJ:      # unused without appearance rows: not written
                continue
            got, ref = gs[i].cpu().numpy(), gs_ref[i].cpu().numpy()
            assert np.all(np.isfinite(got)), (cw, name)
            assert rel_l2(got, ref) <= 1e-6, (cw, name, rel_l2(got, ref))
        if rows:
            assert rel_l2(dapp.cpu().numpy(), dapp_ref.cpu().numpy()) <= 1e-6, cw
        for k in range(2):
            assert abs(float(loss[k]) - float(loss_ref[k])) <= 1e-6 * float(loss_ref[k]), (cw, k)
        if cw == 0.0:
            # the coarse rows still carry the merged composite's term: dropping them (a fine-only
            # composition) gives other gradients (coarse samples are N of the N + Nf composited ones)
            gs_fine, _, _ = stage_backward(packed, packedT, st, N, Nf, cw, app, rows, fine_only=True)
            i = NAMES.index("pts_linears.7.weight")
            assert rel_l2(gs[i].cpu().numpy(), gs_fine[i].cpu().numpy()) > 1e-2


# ---------------------------------------------------------------- 4. whole step against float64
def _pre_activations_clear(state, o, dn, zs, app, rel=1e-5):
    """Per ray: no float64 trunk pre-activation of any sample at the positions zs (a list of (K, n) z
    tensors; points formed in fp32) lies within rel x (its layer's rms) of zero."""
    K = o.shape[0]
    ok = torch.ones(K, dtype=torch.bool)
    st64 = {k: v.double() for k, v in state.items()}
    for z in zs:
        n = z.shape[1]
        pts = (o[:, None, :] + dn[:, None, :] * z[..., None]).reshape(-1, 3)
        dexp = dn[:, None, :].expand(K, n, 3).reshape(-1, 3)
        pres = []
        with torch.no_grad():
            O.nerf_forward(st64, pts.double(), dexp.double(), None if app is None else app.double(), keep=pres)
        for p_ in pres:
            ok &= ((p_.abs() / p_.pow(2).mean().sqrt()) > rel).reshape(K, -1).all(dim=1)
    return ok


def _oracle_step(state, app, o, dn, z, z_all, target, cw, dtype):
    """loss = mse(fine) + cw mse(coarse) by the oracle's _pass on the given (constant) positions and torch
    autograd in `dtype`: (gradients by name (+ "app"), fine mse, coarse mse)."""
    st = {k: v.to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    a = None if app is None else app.to(dtype).clone().requires_grad_(True)
    pts_c = (o[:, None, :] + dn[:, None, :] * z[..., None]).to(dtype)          # formed in fp32
    pts_a = (o[:, None, :] + dn[:, None, :] * z_all[..., None]).to(dtype)
    rgb_c, _, _ = O._pass(st, pts_c, dn.to(dtype), z.to(dtype), a)
    rgb_f, _, _ = O._pass(st, pts_a, dn.to(dtype), z_all.to(dtype), a)
    mse_f, mse_c = F.mse_loss(rgb_f, target.to(dtype)), F.mse_loss(rgb_c, target.to(dtype))
    (mse_f + cw * mse_c).backward()
    grads = {k: v.grad.detach() for k, v in st.items() if v.grad is not None}
    if a is not None:
        grads["app"] = a.grad.detach().reshape(1, 32)
    return grads, float(mse_f.detach()), float(mse_c.detach())


@pytest.mark.parametrize("N,Nf,R,with_app", [(8, 16, 24, True), (8, 16, 24, False), (32, 32, 16, True)])
def test_step_matches_float64_autograd(ref_state, app_vec, N, Nf, R, with_app):
    """The step on rays whose samples (the points the GPU itself uses, coarse and merged) are clear of
    every ReLU kink, against torch autograd of the oracle on those points as constants: per tensor the
    GPU is no further from float64 than twice the float32 oracle (+ 1e-6), and each loss part is within
    2e-5 relative of the float32 oracle's."""
    L = _lib()
    lib, dev = L.load(), L.device()
    packed, packedT = _packed(ref_state, dev)
    cw = 1.0
    K = 8 * R
    cand = _rays(K, N, Nf, seed=101 * N + Nf)
    app, rows = _app(app_vec, K, 1 if with_app else 0, dev)
    app_cpu = app_vec if with_app else None
    fw = hier_forward(packed, cand, N, Nf, app, rows)
    _, _, _, z = coarse_forward(packed, cand, N, app, rows)
    dn = torch.empty(K, 3, device=dev)
    L.check(lib.nerf_normalize_dirs(L.ptr(fw["x"]["d"]), K, L.ptr(dn), L.stream()), "normalize")
    torch.cuda.synchronize()
    z, z_all, dn = z.cpu(), fw["z_out"].cpu(), dn.cpu()
    ok = _pre_activations_clear(ref_state, cand["o"], dn, [z, z_all], app_cpu)
    print(f"({N},{Nf}): {int(ok.sum())} of {K} candidate rays clear the ReLU kinks")
    keep = torch.nonzero(ok)[:, 0][:R]
    assert keep.numel() == R, f"only {int(ok.sum())} of {K} rays clear the ReLU kinks"
    r = _take(cand, keep)
    fw = hier_forward(packed, r, N, Nf, app, rows)
    gs, dapp, loss = hier_backward(packed, packedT, fw, N, Nf, cw, app, rows)
    torch.cuda.synchronize()
    assert torch.equal(fw["z_out"].cpu(), z_all[keep])           # the kept rays resample as they did
    zk, zak, dnk = z[keep], z_all[keep], dn[keep]
    g32, f32_f, f32_c = _oracle_step(ref_state, app_cpu, r["o"], dnk, zk, zak, r["target"], cw, torch.float32)
    g64, _, _ = _oracle_step(ref_state, app_cpu, r["o"], dnk, zk, zak, r["target"], cw, torch.float64)
    got = {n: gs[i].cpu().numpy().reshape(-1) for i, n in enumerate(NAMES)}
    if with_app:
        got["app"] = dapp.cpu().numpy().reshape(-1)
    for n in g64:
        if not with_app and n in APP_PROJ:
            continue
        e_gpu = rel_l2(got[n], g64[n].numpy().reshape(-1))
        e_cpu = rel_l2(g32[n].numpy().reshape(-1), g64[n].numpy().reshape(-1))
        print(f"({N},{Nf}) {n}: rel-L2 vs float64  gpu {e_gpu:.3g}  cpu fp32 {e_cpu:.3g}")
        assert e_gpu <= 2 * e_cpu + 1e-6, (n, e_gpu, e_cpu)
    assert abs(float(loss[0]) - f32_f) <= 2e-5 * f32_f, (float(loss[0]), f32_f)
    assert abs(float(loss[1]) - f32_c) <= 2e-5 * f32_c, (float(loss[1]), f32_c)


# ------------------------------------------------------------------------------------ 5. Trainer
def _teacher(n_images, hw, seed=0):
    import nerfmi
    from nerfmi.dataset import SyntheticNeRFDataset
    cfg = nerfmi.Config()
    np.random.seed(seed)
    torch.manual_seed(seed)                         # (the dataset draws its appearance table from torch's RNG)
    ds = SyntheticNeRFDataset(cfg, n_images=n_images, H=hw, W=hw)
    torch.manual_seed(seed)
    return cfg, ds


def test_hierarchical_training_reduces_the_fine_loss_on_teacher_scene():
    """test_training_reduces_loss_on_teacher_scene's rule on the fine MSE: 40 steps of 1,024 rays at the
    headline 64 + 128 (Config.num_importance itself is 64, so n_importance is given)."""
    from nerfmi.train import Trainer
    cfg, ds = _teacher(4, 64)
    tr = Trainer(cfg, appearance_embeddings=ds.appearance_embeddings, hierarchical=True, n_importance=128)
    assert (cfg.num_samples, tr.n_importance) == (64, 128)
    fine, total = [], []
    for i in range(40):
        b = ds.get_rays(batch_size=1024)
        total.append(float(tr.step(b["rays_o"], b["rays_d"], b["rgb"], b["appearance_idx"], seed=i + 1)))
        fine.append(float(tr.loss_parts[0]))
        assert abs(total[-1] - (fine[-1] + float(tr.loss_parts[1]))) <= 1e-6 * total[-1]
    assert np.all(np.isfinite(fine)) and np.all(np.isfinite(total))
    assert np.mean(fine[-5:]) < 0.7 * np.mean(fine[:5]), fine


def test_hierarchical_training_is_deterministic():
    """Two trainers from one seed, 10 steps of 1,024 rays: parameters, both Adam moments and both loss
    parts are bit-identical (one fixed order for the sum of the two parts' gradients, no float atomics)."""
    from nerfmi.train import Trainer
    runs = []
    for _ in range(2):
        cfg, ds = _teacher(3, 64)
        tr = Trainer(cfg, appearance_embeddings=ds.appearance_embeddings, hierarchical=True, n_importance=128)
        parts = []
        for i in range(10):
            b = ds.get_rays(batch_size=1024)
            tr.step(b["rays_o"], b["rays_d"], b["rgb"], b["appearance_idx"], seed=i + 1)
            parts.append(tr.loss_parts.detach().cpu().clone())
        torch.cuda.synchronize()
        runs.append((tr.flat.detach().cpu().clone(), tr.exp_avg.detach().cpu().clone(),
                     tr.exp_avg_sq.detach().cpu().clone(), torch.stack(parts)))
    for a_, b_ in zip(*runs):
        assert torch.equal(a_, b_)
    assert float(runs[0][3].min()) > 0


def _ref_trainer(ref_state, num_samples=64, **kw):
    import nerfmi
    from nerfmi.train import Trainer
    cfg = nerfmi.Config()
    cfg.num_samples = num_samples
    torch.manual_seed(0)
    model = nerfmi.NeRF(cfg)
    model.load_state_dict(ref_state)
    torch.manual_seed(1)
    return Trainer(cfg, model=model, appearance_embeddings=torch.randn(4, 32), **kw)


def test_trainer_step_is_the_two_c_calls(ref_state):
    """Trainer(hierarchical=True).forward_backward equals nerf_train_hier_forward + _backward on the
    same inputs bit for bit: loss parts, rgb_map, every gradient and the appearance row's."""
    N, Nf, B, cw, img = 16, 24, 64, 0.5, 2
    tr = _ref_trainer(ref_state, num_samples=N, hierarchical=True, n_importance=Nf, coarse_loss_weight=cw)
    r = _rays(B, N, Nf, seed=5)
    dev = tr.dev
    loss, rgb_map = tr.forward_backward(r["o"].to(dev), r["d"].to(dev), r["target"].to(dev), img, t_rand=r["t_rand"],
                                        u_rand=r["u_rand"])
    torch.cuda.synchronize()
    packed, packedT = _packed(ref_state, dev)
    app = tr.appearance_embeddings[img].reshape(1, 32).clone()
    fw = hier_forward(packed, r, N, Nf, app, 1)
    gs, dapp, parts = hier_backward(packed, packedT, fw, N, Nf, cw, app, 1)
    torch.cuda.synchronize()
    assert torch.equal(rgb_map, fw["rgb_map"]) and torch.equal(tr.loss_parts, parts)
    assert float(loss) == float(parts[0] + cw * parts[1])
    for i, n in enumerate(NAMES):
        assert torch.equal(tr.view(tr.grad, i).reshape(-1), gs[i]), n
    table_grad = tr.view(tr.grad, 24)
    assert torch.equal(table_grad[img], dapp[0])
    assert float(table_grad.abs().sum()) == float(dapp.abs().sum())       # every other row zero


def test_default_trainer_is_unchanged_beside_a_hierarchical_one(ref_state):
    """hierarchical=False after a hierarchical trainer ran in the same process still takes the coarse
    step: two default trainers, one before and one after, end on the same parameters."""
    r = _rays(256, 64, 128, seed=9)

    def three_steps(tr):
        dev = tr.dev
        for i in range(3):
            tr.step(r["o"].to(dev), r["d"].to(dev), r["target"].to(dev), i % 4, t_rand=r["t_rand"])
        torch.cuda.synchronize()
        return tr.flat.detach().cpu().clone()

    first = _ref_trainer(ref_state)
    a = three_steps(first)
    hier = _ref_trainer(ref_state, hierarchical=True)
    dev = hier.dev
    hier.step(r["o"].to(dev), r["d"].to(dev), r["target"].to(dev), 0, t_rand=r["t_rand"], seed=3)
    second = _ref_trainer(ref_state)
    assert not second.hierarchical and not hasattr(second, "loss_parts")
    with pytest.raises(ValueError, match="u_rand"):
        second.forward_backward(r["o"], r["d"], r["target"], 0, t_rand=r["t_rand"], u_rand=r["u_rand"])
    assert torch.equal(three_steps(second), a)
    assert not torch.equal(hier.flat.detach().cpu(), a)
