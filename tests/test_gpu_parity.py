"""Parity of the HIP path (through the C ABI) with the oracle and the reference's golden outputs.

Tolerances (north star: 1e-4 relative fp32 on rgb/depth, bit-exact ray indices):
  * ray generation, normalisation, stratified z and pts: bit-exact (same IEEE operations);
  * rgb / depth / weights / sigma: |gpu - ref| <= 1e-4*|ref| + 1e-6 (the 1e-6 floor because
    random-init rgb is ~0.03 and accumulations of ~64-256 terms differ in order);
  * PE features: |gpu - ref| <= 2e-6 (sin/cos are 1-2 ulp functions on both sides);
  * fine z (inverse CDF) from the same coarse weights: bit-exact (the pdf normaliser is summed
    in torch's CPU order and the double prefix sums are exact); behind a GPU-computed coarse pass
    the weights already differ by ~1e-6 relative, so z there is held to 1e-5 relative.
"""
import os

import numpy as np
import pytest
import torch

from conftest import seeded_uniform
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-6


def close(gpu, ref, rtol=RTOL, atol=ATOL, what=""):
    gpu = gpu.detach().float().cpu().numpy() if torch.is_tensor(gpu) else np.asarray(gpu)
    ref = ref.detach().float().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref)
    assert gpu.shape == ref.shape, (what, gpu.shape, ref.shape)
    err = np.abs(gpu - ref)
    bad = err > atol + rtol * np.abs(ref)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} outside tol; max abs err {err.max():.3g}"


@pytest.fixture(scope="module")
def nerfmi_mod():
    import nerfmi
    return nerfmi


@pytest.fixture(scope="module", autouse=True, params=["f16x3", "f32"])
def arith(request, nerfmi_mod):
    """Every parity test runs under both MLP arithmetics (include/nerfmi.h, nerf_arith)."""
    prev = nerfmi_mod.set_mlp_arith(request.param)
    yield request.param
    nerfmi_mod.set_mlp_arith(prev)


@pytest.fixture(scope="module")
def model(nerfmi_mod, ref_state):
    m = nerfmi_mod.NeRF(nerfmi_mod.Config())
    m.load_state_dict(ref_state)
    return m.cuda().eval().requires_grad_(False)     # the inference kernels (autograd: test_gpu_autograd.py)


def crop(golden, scene, n=None):
    f1 = golden("f1_get_rays.npz")
    o, d = torch.from_numpy(f1[f"{scene}_o"]), torch.from_numpy(f1[f"{scene}_d"])
    return (o, d) if n is None else (o[:n], d[:n])


# ------------------------------------------------------------------------------------ rays
def test_get_rays_bit_exact(nerfmi_mod, golden, golden_meta):
    f1 = golden("f1_get_rays.npz")
    for scene in ("chair", "hotdog"):
        c2w = torch.from_numpy(f1[f"{scene}_c2w"]).cuda()
        o, d = nerfmi_mod.get_rays(800, 800, golden_meta["F1"]["focal"], c2w)
        assert o.shape == d.shape == (800, 800, 3) and o.stride()[:2] == (0, 0)
        assert np.array_equal(d[368:432, 368:432].reshape(-1, 3).cpu().numpy(), f1[f"{scene}_d"]), scene
        assert np.array_equal(o[368:432, 368:432].reshape(-1, 3).cpu().numpy(), f1[f"{scene}_o"]), scene
        _, d_ref = O.get_rays(800, 800, golden_meta["F1"]["focal"], c2w.cpu())
        assert torch.equal(d.cpu(), d_ref), f"{scene}: full frame not bit-exact"
    o, d = nerfmi_mod.get_rays(5, 7, 123.4, torch.from_numpy(f1["small_c2w"]))   # CPU in -> CPU out
    assert d.device.type == "cpu" and np.array_equal(d.numpy(), f1["small_d"])
    assert np.array_equal(o.contiguous().numpy(), f1["small_o"])


def test_stratified_bit_exact(nerfmi_mod, golden):
    o, d = crop(golden, "chair")
    dn = O.normalize(d)
    for n in (64, 32, 7, 1):
        z, pts = nerfmi_mod.sample_stratified(o.cuda(), dn.cuda(), 2.0, 6.0, n, perturb=False)
        z_ref, pts_ref = O.sample_stratified(o, dn, 2.0, 6.0, n)
        assert torch.equal(z.cpu(), z_ref) and torch.equal(pts.cpu(), pts_ref), n
    t_rand = torch.rand(o.shape[0], 64)
    z, pts = nerfmi_mod.sample_stratified(o.cuda(), dn.cuda(), 2.0, 6.0, 64, perturb=True, t_rand=t_rand)
    z_ref, pts_ref = O.sample_stratified(o, dn, 2.0, 6.0, 64, t_rand)
    assert torch.equal(z.cpu(), z_ref) and torch.equal(pts.cpu(), pts_ref)
    # in-kernel RNG: stays inside the strata and is seeded
    z1, _ = nerfmi_mod.sample_stratified(o.cuda(), dn.cuda(), 2.0, 6.0, 64, seed=3)
    z2, _ = nerfmi_mod.sample_stratified(o.cuda(), dn.cuda(), 2.0, 6.0, 64, seed=3)
    assert torch.equal(z1, z2)
    assert bool((z1[:, 1:] >= z1[:, :-1]).all()) and float(z1.min()) >= 2.0 and float(z1.max()) <= 6.0


def test_positional_encoding(nerfmi_mod):
    torch.manual_seed(4)
    x = torch.randn(4096, 3) * 3
    # values beyond the MLP kernels' fast sin/cos range (|x| > 16, csrc/pe_sin.h) and a few at +-1000, in
    # every coordinate and both signs: this module takes the library sinf / cosf whatever the size
    u = torch.rand(96)
    rows, sign = torch.arange(96), 1.0 - 2.0 * ((torch.arange(96) // 3) % 2)
    x[rows, rows % 3] = sign * (16 + 48 * u)
    x[torch.arange(96, 102), torch.arange(6) % 3] = torch.tensor([1000.0, 1000.0, 1000.0, -1000.0, -1000.0, -1000.0])
    for c in range(3):
        assert bool((x[:, c] == 1000.0).any()) and bool((x[:, c] == -1000.0).any())
        assert bool((x[:96, c] > 16).any()) and bool((x[:96, c] < -16).any())
    for levels, inc in ((10, True), (4, True), (6, False)):
        pe = nerfmi_mod.PositionalEncoding(levels, include_input=inc)
        got = pe(x.cuda())
        ref = O.positional_encoding(x, levels) if inc else O.positional_encoding(x, levels)[:, 3:]
        close(got, ref, rtol=0, atol=2e-6, what=f"PE L={levels}")


# ------------------------------------------------------------------------------------- MLP
def test_forward_matches_reference(nerfmi_mod, model, golden, app_vec):
    f2 = golden("f2_forward.npz")
    x, d = torch.from_numpy(f2["x"]), torch.from_numpy(f2["d"])
    cases = (("none", None, 1024), ("app2d", app_vec[None], 1024), ("app1d", app_vec, 1024),
             ("per_sample", torch.from_numpy(f2["app_per_sample"]), 512))
    with torch.no_grad():
        for name, a, n in cases:
            rgb, sigma = model(x[:n].cuda(), d[:n].cuda(), None if a is None else a.cuda())
            assert rgb.shape == (n, 3) and sigma.shape == (n, 1)
            close(rgb, f2[f"rgb_{name}"], what=f"rgb {name}")
            close(sigma, f2[f"sigma_{name}"], what=f"sigma {name}")


def test_forward_accuracy_vs_float64(model, ref_state, app_vec, arith):
    """Both arithmetics are fp32-accurate: max error against a float64 evaluation of the same
    weights stays within a small multiple of the fp32 CPU path's own error."""
    torch.manual_seed(12)
    x = torch.rand(8192, 3) * 6 - 3
    d = torch.nn.functional.normalize(torch.randn(8192, 3), dim=-1)
    st64 = {k: v.double() for k, v in ref_state.items()}
    with torch.no_grad():
        rgb, sigma = model(x.cuda(), d.cuda(), app_vec.cuda())
        rgb32, sigma32 = O.nerf_forward(ref_state, x, d, app_vec)
        rgb64, sigma64 = O.nerf_forward(st64, x.double(), d.double(), app_vec.double())
    e_gpu = (rgb.cpu().double() - rgb64).abs().max().item()
    e_cpu = (rgb32.double() - rgb64).abs().max().item()
    s_gpu = ((sigma.cpu().double() - sigma64).abs() / (sigma64.abs() + 1e-3)).max().item()
    s_cpu = ((sigma32.double() - sigma64).abs() / (sigma64.abs() + 1e-3)).max().item()
    print(f"{arith}: rgb max err vs f64 {e_gpu:.3g} (cpu f32 {e_cpu:.3g}); sigma {s_gpu:.3g} (cpu {s_cpu:.3g})")
    assert e_gpu <= 4 * e_cpu + 1e-7
    assert s_gpu <= 4 * s_cpu + 1e-6


def test_forward_ragged_and_position_independent(model, ref_state):
    torch.manual_seed(6)
    x = torch.randn(1000, 3) * 2          # not a multiple of 32 samples
    d = torch.nn.functional.normalize(torch.randn(1000, 3), dim=-1)
    with torch.no_grad():
        rgb, sigma = model(x.cuda(), d.cuda())
        perm = torch.randperm(1000)
        rgb_p, sigma_p = model(x[perm].cuda(), d[perm].cuda())
        one_rgb, one_sigma = model(x[:1].cuda(), d[:1].cuda())
    assert torch.equal(rgb[perm], rgb_p) and torch.equal(sigma[perm], sigma_p)
    assert torch.equal(one_rgb, rgb[:1]) and torch.equal(one_sigma, sigma[:1])
    rgb_o, sigma_o = O.nerf_forward(ref_state, x, d)
    close(rgb, rgb_o, what="rgb")
    close(sigma, sigma_o, what="sigma")
    # with gradients enabled the same call is differentiable (autograd.py, the training kernels)
    model.requires_grad_(True)
    try:
        rgb_g, sigma_g = model(x.cuda(), d.cuda())
    finally:
        model.requires_grad_(False)
    assert rgb_g.grad_fn is not None and sigma_g.grad_fn is not None
    close(rgb_g, rgb_o, what="rgb (differentiable path)")
    close(sigma_g, sigma_o, what="sigma (differentiable path)")


# ------------------------------------------------------------------------------- composite
def test_composite_kernel(ref_state):
    import ctypes
    from nerfmi import _lib
    lib = _lib.load()
    torch.manual_seed(8)

    def unaligned(t):   # the same values at a 4-byte offset from a 16-byte boundary (the scalar-load kernel)
        buf = torch.empty(t.numel() + 1, device="cuda")
        buf[1:] = t.reshape(-1).cuda()
        return buf[1:].view(t.shape)
    for B, N, odd in ((37, 64, False), (5, 192, False), (9, 1, False), (3, 100, False), (2, 1000, False),
                      (4, 2, False), (6, 7, False), (19, 17, False), (21, 64, True), (3, 192, True)):
        z = torch.sort(torch.rand(B, N) * 4 + 2, dim=-1).values
        sigma = torch.relu(torch.randn(B, N) * 3)
        rgb = torch.rand(B, N, 3)
        zc, sc, rc = (unaligned(t) if odd else t.cuda() for t in (z, sigma, rgb))
        rm = torch.empty(B, 3, device="cuda")
        dm = torch.empty(B, device="cuda")
        wm = unaligned(torch.zeros(B, N)) if odd else torch.empty(B, N, device="cuda")
        _lib.check(lib.nerf_composite(_lib.ptr(rc), _lib.ptr(sc), _lib.ptr(zc), B, N, _lib.ptr(rm), _lib.ptr(dm),
                                      _lib.ptr(wm), _lib.stream()), "composite")
        r_ref, d_ref, w_ref = O.composite(rgb, sigma[..., None], z)
        close(rm, r_ref, what=f"rgb B={B} N={N}")
        close(dm, d_ref[:, 0], what=f"depth B={B} N={N}")
        if N > 1:
            close(wm, w_ref[..., 0], what=f"weights B={B} N={N}")
        else:   # the reference's weights are empty at N=1; the kernel writes zeros
            assert w_ref.shape[1] == 0 and not wm.any()


# --------------------------------------------------------------------------- volume_render
def test_volume_render_coarse(nerfmi_mod, model, golden, app_vec):
    f3 = golden("f3_coarse.npz")
    o, d = crop(golden, "chair")
    rgb, depth, ex = nerfmi_mod.volume_render(model, o.cuda(), d.cuda(), 2.0, 6.0, 64, 64,
                                              appearance_embedding=app_vec.cuda(), perturb=False)
    assert rgb.shape == (4096, 3) and depth.shape == (4096, 1)
    assert ex["weights"].shape == (4096, 64, 1) and ex["z_vals"].shape == (4096, 64)
    close(rgb, f3["chair_rgb"], what="rgb")
    close(depth, f3["chair_depth"], what="depth")
    close(ex["weights"][:256, :, 0], f3["chair_weights256"], what="weights")
    assert np.array_equal(ex["z_vals"][0].cpu().numpy(), f3["z_row"])
    rgb, depth, _ = nerfmi_mod.volume_render(model, o[:1024].cuda(), d[:1024].cuda(), 2.0, 6.0, 64, 0, perturb=False)
    close(rgb, f3["chair_noapp_rgb"], what="rgb no app")
    close(depth, f3["chair_noapp_depth"], what="depth no app")
    rgb, depth, _ = nerfmi_mod.volume_render(model, o[:1024].cuda(), d[:1024].cuda(), 2.0, 6.0, 32, 0,
                                             appearance_embedding=app_vec.cuda(), perturb=False)
    close(rgb, f3["chair_n32_rgb"], what="rgb N=32")
    oh, dh = crop(golden, "hotdog", 1024)
    rgb, depth, _ = nerfmi_mod.volume_render(model, oh, dh, 2.0, 6.0, 64, 128, appearance_embedding=app_vec,
                                             perturb=False)                    # CPU tensors in -> CPU out
    assert rgb.device.type == "cpu"
    close(rgb, f3["hotdog_rgb"], what="hotdog rgb")
    close(depth, f3["hotdog_depth"], what="hotdog depth")


def test_volume_render_perturb(nerfmi_mod, model, golden, golden_meta, app_vec):
    f4 = golden("f4_perturb.npz")
    m = golden_meta["F4"]
    t_rand = seeded_uniform(m["seed"], m["t_rand_shape"], m["t_rand_sha256"])
    o, d = crop(golden, "chair", 1024)
    rgb, depth, ex = nerfmi_mod.volume_render(model, o.cuda(), d.cuda(), 2.0, 6.0, 64, 64,
                                              appearance_embedding=app_vec.cuda(), perturb=True, t_rand=t_rand)
    close(rgb, f4["rgb"], what="rgb")
    close(depth, f4["depth"], what="depth")
    assert np.array_equal(ex["z_vals"][:128].cpu().numpy(), f4["z128"])


def test_sample_importance(nerfmi_mod, golden, golden_meta):
    f5 = golden("f5_importance.npz")
    m = golden_meta["F5"]
    u = seeded_uniform(m["seed"], m["u_rand_shape"], m["u_rand_sha256"])
    o, d, z, w = (torch.from_numpy(f5[k]).cuda() for k in ("o", "d", "z", "w"))
    z_all, pts = nerfmi_mod.sample_importance(o, d, z, w, 128, u_rand=u)
    assert np.array_equal(z_all.cpu().numpy(), f5["z_all"])
    assert bool((z_all[:, 1:] >= z_all[:, :-1]).all())
    za = z_all.cpu()
    assert torch.equal(pts.cpu(), o.cpu()[:, None, :] + d.cpu()[:, None, :] * za[..., None])
    # weights as (B,N,1) are accepted too; the reference's raising input gives the H1 result
    u = seeded_uniform(12, (2, 128), m["u_bad_sha256"])
    w_bad = torch.from_numpy(f5["w_bad"]).cuda()[..., None]
    z_all, _ = nerfmi_mod.sample_importance(o[:2], d[:2], z[:2], w_bad, 128, u_rand=u)
    assert np.array_equal(z_all.cpu().numpy(), f5["z_bad_all"])


def test_sample_importance_shapes_vs_oracle(nerfmi_mod):
    torch.manual_seed(12)
    for B, N, Nf in ((33, 64, 128), (5, 7, 9), (7, 100, 64), (3, 256, 1024), (4, 1, 16), (2, 64, 1)):
        o = torch.randn(B, 3)
        d = torch.nn.functional.normalize(torch.randn(B, 3), dim=-1)
        z = torch.sort(torch.rand(B, N) * 4 + 2, dim=-1).values
        w = torch.rand(B, N) * (torch.rand(B, N) > 0.5)
        w[0] = 0                      # all-zero weights: a uniform pdf
        u = torch.rand(B, Nf)
        z_all, pts = nerfmi_mod.sample_importance(o.cuda(), d.cuda(), z.cuda(), w.cuda(), Nf, u_rand=u)
        z_ref, pts_ref = O.sample_importance_h1(o, d, z, w, Nf, u)
        assert torch.equal(z_all.cpu(), z_ref), (B, N, Nf)
        assert torch.equal(pts.cpu(), pts_ref), (B, N, Nf)


def test_sample_importance_merge_scatter(nerfmi_mod):
    """nerf_sample_importance_merge: z_all equals the resample alone, every coarse (rgb, sigma) sits at
    the merged slot of its z, and each fine sample's slot holds its z (ragged, N = 1, and the largest
    supported N and Nf)."""
    import ctypes
    from nerfmi import _lib
    lib = _lib.load()
    torch.manual_seed(13)
    for B, N, Nf in ((33, 64, 128), (5, 7, 9), (6, 64, 512), (3, 256, 1024), (4, 1, 16)):
        z = torch.sort(torch.rand(B, N) * 4 + 2, dim=-1).values
        w = torch.rand(B, N) * (torch.rand(B, N) > 0.5)
        u = torch.rand(B, Nf)
        u_lin = torch.linspace(0, 1, Nf + 1)[:-1].contiguous()
        rgb_c, sigma_c = torch.rand(B, N, 3), torch.rand(B, N)
        T = N + Nf
        zg, wg, ug, ul, rc, sc = (t.cuda() for t in (z, w, u, u_lin, rgb_c, sigma_c))
        z_all = torch.empty(B, T, device="cuda")
        rgb_all = torch.full((B, T, 3), float("nan"), device="cuda")
        sigma_all = torch.full((B, T), float("nan"), device="cuda")
        z_fine = torch.empty(B, Nf, device="cuda")
        slot = torch.empty(B, Nf, dtype=torch.int32, device="cuda")
        _lib.check(lib.nerf_sample_importance_merge(
            _lib.ptr(zg), _lib.ptr(wg), _lib.ptr(rc), _lib.ptr(sc), B, N, Nf, _lib.ptr(ul), _lib.ptr(ug),
            ctypes.c_uint64(0), _lib.ptr(z_all), _lib.ptr(rgb_all), _lib.ptr(sigma_all), _lib.ptr(z_fine),
            _lib.ptr(slot), _lib.stream()), "importance_merge")
        torch.cuda.synchronize()
        z_ref, _ = O.sample_importance_h1(torch.zeros(B, 3), torch.zeros(B, 3), z, w, Nf, u)
        assert torch.equal(z_all.cpu(), z_ref), (B, N, Nf)
        za, ra, sa, zf, sl = (t.cpu() for t in (z_all, rgb_all, sigma_all, z_fine, slot))
        rows = torch.arange(B)[:, None]
        assert torch.equal(za[rows, sl.long()], zf), (B, N, Nf)          # fine z at its slot
        fine = torch.zeros(B, T, dtype=torch.bool)
        fine[rows, sl.long()] = True
        assert int(fine.sum()) == B * Nf                                  # distinct slots
        assert torch.equal(torch.sort(za[~fine].reshape(B, N), dim=-1).values, z)   # the coarse z fill the rest
        # coarse slots carry the coarse evaluation of their z (ties between equal coarse z aside, the
        # k-th coarse slot in order holds coarse sample k)
        assert torch.equal(ra[~fine].reshape(B, N, 3), rgb_c), (B, N, Nf)
        assert torch.equal(sa[~fine].reshape(B, N), sigma_c), (B, N, Nf)


def test_hierarchical_h1(nerfmi_mod, model, golden, golden_meta, app_vec):
    f6 = golden("f6_hierarchical.npz")
    m = golden_meta["F6"]
    u = seeded_uniform(m["seed"], m["u_rand_shape"], m["u_rand_sha256"])
    o, d = crop(golden, "chair", 1024)
    rgb, depth, ex = nerfmi_mod.render_rays(model, o.cuda(), d.cuda(), 2.0, 6.0, 64, 128,
                                            appearance_embedding=app_vec.cuda(), perturb=False,
                                            hierarchical=True, u_rand=u)
    close(rgb, f6["rgb"], what="fine rgb")
    close(depth, f6["depth"], what="fine depth")
    close(ex["rgb_map_coarse"], f6["rgb_coarse"], what="coarse rgb")
    close(ex["z_vals"][:64], f6["z_all64"], rtol=1e-5, atol=0, what="z_all")
    close(ex["weights"][:64, :, 0], f6["weights64"], what="fine weights")
    # the staged path (per-stage entry points) runs the same kernels: identical bits
    timing = []
    rgb2, depth2, ex2 = nerfmi_mod.render_rays(model, o.cuda(), d.cuda(), 2.0, 6.0, 64, 128,
                                               appearance_embedding=app_vec.cuda(), perturb=False,
                                               hierarchical=True, u_rand=u, timing=timing)
    assert len(timing) == 2
    assert torch.equal(rgb, rgb2) and torch.equal(depth, depth2) and torch.equal(ex["z_vals"], ex2["z_vals"])


def test_edge_sizes(nerfmi_mod, model, ref_state, app_vec):
    torch.manual_seed(9)
    for B in (1, 3, 33):
        o = torch.randn(B, 3)
        d = torch.randn(B, 3)
        rgb, depth, ex = nerfmi_mod.volume_render(model, o.cuda(), d.cuda(), 2.0, 6.0, 64, 0, perturb=False)
        r_ref, d_ref, _ = O.volume_render(ref_state, o, d, 2.0, 6.0, 64)
        close(rgb, r_ref, what=f"B={B}")
        close(depth, d_ref, what=f"B={B}")
    o = torch.zeros(0, 3, device="cuda")
    rgb, depth, ex = nerfmi_mod.volume_render(model, o, o, 2.0, 6.0, 64, 128, hierarchical=True)
    assert rgb.shape == (0, 3) and depth.shape == (0, 1)
    # 2-D ray grids keep their shape (render.py:89-90)
    o = torch.randn(4, 5, 3)
    d = torch.randn(4, 5, 3)
    rgb, depth, _ = nerfmi_mod.volume_render(model, o.cuda(), d.cuda(), 2.0, 6.0, 16, 0, perturb=False)
    assert rgb.shape == (4, 5, 3) and depth.shape == (4, 5, 1)


def test_hierarchical_extreme_sizes(nerfmi_mod, model, ref_state, app_vec, golden):
    """The largest supported hierarchical pass (N = 256, Nf = 1024: 1,280 merged samples per ray) and
    ragged ones (samples per ray not a multiple of a wave's 32, one fine sample): the coarse maps
    against the oracle, and the fine maps with the fine samples held equal (the oracle's fine pass on
    the GPU's merged z, as in test_full_frame_properties)."""
    o, d = crop(golden, "chair", 24)
    torch.manual_seed(14)
    for N, Nf in ((256, 1024), (50, 70), (33, 1), (7, 200), (64, 195)):   # (64, 195): T > 256, T % 4 != 0
        u = torch.rand(o.shape[0], Nf)
        rgb, depth, ex = nerfmi_mod.render_rays(model, o.cuda(), d.cuda(), 2.0, 6.0, N, Nf,
                                                appearance_embedding=app_vec.cuda(), perturb=False,
                                                hierarchical=True, u_rand=u)
        r_ref, _, ex_ref = O.render_rays_h1(ref_state, o, d, 2.0, 6.0, N, Nf, app_vec, None, u)
        close(ex["rgb_map_coarse"], ex_ref["rgb_map_coarse"], what=f"coarse rgb N={N} Nf={Nf}")
        close(ex["depth_map_coarse"], ex_ref["depth_map_coarse"], what=f"coarse depth N={N} Nf={Nf}")
        z = ex["z_vals"].cpu()
        assert z.shape == (o.shape[0], N + Nf) and bool((z[:, 1:] >= z[:, :-1]).all())
        dn = O.normalize(d)
        pts = o[:, None, :] + dn[:, None, :] * z[..., None]
        r_fix, d_fix, _ = O._pass(ref_state, pts, dn, z, app_vec)
        close(rgb, r_fix, what=f"fine rgb, same z, N={N} Nf={Nf}")
        close(depth, d_fix, what=f"fine depth, same z, N={N} Nf={Nf}")


def test_render_unaligned_outputs(nerfmi_mod, model, ref_state, app_vec, golden):
    """nerf_render_rays with weights_out and z_out one float off 16-byte alignment (views into a larger
    caller buffer): the merged fine composite takes its scalar-store variants (composite.hip) at
    T = 192 (staged) and T = 259 (unstaged); maps, weights and merged z match the aligned call, and
    the fine maps the oracle's fine pass on the same z."""
    from nerfmi import _lib
    from nerfmi.models import app_rows
    from nerfmi.ray_utils import linspace_table
    from nerfmi.render import packed_for
    lib, dev = _lib.load(), _lib.device()
    o, d = crop(golden, "chair", 24)
    B = o.shape[0]
    torch.manual_seed(15)
    for N, Nf in ((64, 128), (64, 195)):
        T = N + Nf
        u = torch.rand(B, Nf)
        rgb_a, depth_a, ex = nerfmi_mod.render_rays(model, o.cuda(), d.cuda(), 2.0, 6.0, N, Nf,
                                                    appearance_embedding=app_vec.cuda(), perturb=False,
                                                    hierarchical=True, u_rand=u)
        oo, dd = o.reshape(-1, 3).cuda().contiguous(), d.reshape(-1, 3).cuda().contiguous()
        app, rows = app_rows(app_vec, B, dev)
        wbuf, zbuf = torch.zeros(B * T + 1, device=dev), torch.zeros(B * T + 1, device=dev)
        w, z = wbuf[1:], zbuf[1:]                        # 4 bytes past a 16-byte boundary
        assert w.data_ptr() % 16 != 0 and z.data_ptr() % 16 != 0
        rgb, depth = torch.empty(B, 3, device=dev), torch.empty(B, device=dev)
        crgb, cdepth = torch.empty(B, 3, device=dev), torch.empty(B, device=dev)
        ws = torch.empty(lib.nerf_render_workspace_bytes(B, N, Nf), dtype=torch.uint8, device=dev)
        P = _lib.ptr
        _lib.check(lib.nerf_render_rays(P(packed_for(model)), P(oo), P(dd), B, 2.0, 6.0, N, Nf, P(linspace_table(N, dev)),
                                        P(linspace_table(Nf, dev, drop_last=True)), 0, None, P(u.cuda().contiguous()), 0,
                                        0, P(app), rows, P(rgb), P(depth), P(w), P(z), P(crgb), P(cdepth), P(ws),
                                        ws.numel(), _lib.stream()), "nerf_render_rays")
        torch.cuda.synchronize()
        close(rgb, rgb_a.reshape(B, 3), rtol=1e-6, what=f"rgb T={T}")
        close(depth, depth_a.reshape(B), rtol=1e-6, what=f"depth T={T}")
        close(w.reshape(B, T), ex["weights"].reshape(B, T), rtol=1e-6, what=f"weights T={T}")
        assert torch.equal(z.reshape(B, T).cpu(), ex["z_vals"].cpu()), T
        dn = O.normalize(d)
        zc = z.reshape(B, T).cpu()
        r_fix, d_fix, _ = O._pass(ref_state, o[:, None, :] + dn[:, None, :] * zc[..., None], dn, zc, app_vec)
        close(rgb, r_fix, what=f"fine rgb vs oracle, same z, T={T}")
        close(depth.reshape(B, 1), d_fix, what=f"fine depth vs oracle, same z, T={T}")


def test_render_chunked_matches_one_launch(nerfmi_mod, tmp_path):
    """A call past the launch-size limit runs as ray chunks (capi.hip, nerf_render_chunk_rays): with the
    limit lowered to 2^16 samples in a child process (NERFMI_MAX_LAUNCH_SAMPLES), a 3,000-ray 64 + 128
    H1 render with per-ray appearance rows, a ray offset and in-kernel draws runs as 6 chunks of 512
    rays (nerf_render_rays) and as 3 + 6 chunk launches stage by stage (nerf_mlp_forward): every output
    equals the one-launch render of this process bit for bit."""
    import subprocess
    import sys
    from conftest import REPO
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import render_chunked
    ref = render_chunked.render()
    out = tmp_path / "chunked.pt"
    env = dict(os.environ, NERFMI_MAX_LAUNCH_SAMPLES=str(1 << 16))
    from nerfmi import _lib
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "render_chunked.py"), str(out), _lib.get_mlp_arith()],
                       env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = torch.load(out, weights_only=True)
    assert set(got) == set(ref)
    for k in ref:
        assert torch.equal(got[k], ref[k]), k


def test_full_frame_properties(nerfmi_mod, model, ref_state, app_vec, golden_meta, arith):
    """800x800 hierarchical 64+128 (the bench workload): size-independent properties on every ray,
    and accuracy on 4096 rays sampled across the frame.

    The fine pass is ill-conditioned in the coarse weights: the inverse CDF moves a fine sample by
    ~4x the relative change of the weights, and the 2^9 positional-encoding frequency turns that
    into phase, so two fp32 evaluations in different summation orders (the oracle's and the GPU's)
    differ end to end on a few rays per thousand by more than either differs from the exact
    result's neighbourhood.  Parity is therefore asserted (a) at 1e-4 for every ray with the fine
    samples held equal (the oracle's fine pass on the GPU's z), and (b) end to end against a
    float64 render of the same rays: the GPU's error is no worse than the fp32 CPU oracle's own
    in max, p99.9 and median (conftest.check_no_worse_than_cpu)."""
    from conftest import check_no_worse_than_cpu, render_h1_f64
    from nerfmi import cameras
    c2w = cameras.frame_c2w("chair").cuda()
    o, d = nerfmi_mod.get_rays(800, 800, golden_meta["F1"]["focal"], c2w)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    torch.manual_seed(10)
    u = torch.rand(o.shape[0], 128)
    rgb, depth, ex = nerfmi_mod.render_rays(model, o, d, 2.0, 6.0, 64, 128, appearance_embedding=app_vec.cuda(),
                                            perturb=False, hierarchical=True, u_rand=u)
    assert torch.isfinite(rgb).all() and torch.isfinite(depth).all()
    assert float(rgb.min()) >= 0 and float(rgb.max()) <= 1
    z = ex["z_vals"]
    assert bool((z[:, 1:] >= z[:, :-1]).all())
    wsum = ex["weights"][..., 0].sum(-1)
    assert float(wsum.max()) <= 1 + 1e-5
    assert float(depth.min()) >= 2.0 - 1e-4 and float(depth.max()) <= 6.0 + 1e-4
    idx = torch.randperm(o.shape[0])[:4096]
    oc, dc = o[idx].cpu(), d[idx].cpu()
    # (a) fine samples held equal
    dn = O.normalize(dc)
    zg = z[idx].cpu()
    pts = oc[:, None, :] + dn[:, None, :] * zg[..., None]
    r_fix, d_fix, _ = O._pass(ref_state, pts, dn, zg, app_vec)
    close(rgb[idx], r_fix, what="fine rgb, same z")
    close(depth[idx], d_fix, what="fine depth, same z")
    # (b) end to end, referenced to float64
    r_ref, d_ref, ex_ref = O.render_rays_h1(ref_state, oc, dc, 2.0, 6.0, 64, 128, app_vec, None, u[idx])
    close(ex["rgb_map_coarse"][idx], ex_ref["rgb_map_coarse"], what="coarse rgb")
    r64, d64 = render_h1_f64(ref_state, oc, dc, app_vec, u[idx])
    check_no_worse_than_cpu(rgb[idx].cpu(), r_ref, r64, f"full frame {arith} rgb")
    check_no_worse_than_cpu(depth[idx].cpu(), d_ref, d64, f"full frame {arith} depth")
    psnr = -10 * torch.log10(((rgb[idx].cpu() - r_ref) ** 2).mean())
    assert float(psnr) > 80, float(psnr)


def test_coarse_reuse_is_bit_identical(nerfmi_mod, model, golden, app_vec):
    """The fine pass evaluates only the Nf new samples and reuses the coarse evaluations; that must
    give exactly the bits of re-evaluating all N+Nf merged samples (the reference's formulation)."""
    o, d = crop(golden, "hotdog")
    torch.manual_seed(14)
    u = torch.rand(o.shape[0], 128)
    t = torch.rand(o.shape[0], 64)
    kw = dict(appearance_embedding=app_vec.cuda(), perturb=True, hierarchical=True, t_rand=t, u_rand=u)
    a = nerfmi_mod.render_rays(model, o.cuda(), d.cuda(), 2.0, 6.0, 64, 128, **kw)                  # C, reuse
    b = nerfmi_mod.render_rays(model, o.cuda(), d.cuda(), 2.0, 6.0, 64, 128, staged=True, **kw)     # staged, reuse
    c = nerfmi_mod.render_rays(model, o.cuda(), d.cuda(), 2.0, 6.0, 64, 128, staged=True, reuse_coarse=False, **kw)
    for x in (b, c):
        assert torch.equal(a[0], x[0]) and torch.equal(a[1], x[1])
        assert torch.equal(a[2]["weights"], x[2]["weights"]) and torch.equal(a[2]["z_vals"], x[2]["z_vals"])
    # in-kernel RNG path (no explicit uniforms): C and staged agree too
    kw = dict(appearance_embedding=app_vec.cuda(), perturb=True, hierarchical=True, seed=5)
    a = nerfmi_mod.render_rays(model, o.cuda(), d.cuda(), 2.0, 6.0, 64, 128, **kw)
    c = nerfmi_mod.render_rays(model, o.cuda(), d.cuda(), 2.0, 6.0, 64, 128, staged=True, reuse_coarse=False, **kw)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_render_path_frames_single_rank(nerfmi_mod, model, app_vec):
    """frames.render_path_frames on one rank equals rendering each frame directly (ray order,
    row-shard ray generation, reassembly)."""
    from nerfmi import cameras, frames
    poses = [cameras.frame_c2w("hotdog", "circle", k, 120) for k in (0, 7)]
    H, W, f = 40, 56, cameras.synthetic_focal(56)
    rgb, depth = frames.render_path_frames(model, poses, H, W, f, 2.0, 6.0, 64, 0, appearance_embedding=app_vec,
                                           perturb=False)
    assert rgb.shape == (2, H, W, 3) and depth.shape == (2, H, W)
    for k, c2w in enumerate(poses):
        o, d = nerfmi_mod.get_rays(H, W, f, c2w.cuda())
        r, dd, _ = nerfmi_mod.render_rays(model, o.reshape(-1, 3), d.reshape(-1, 3), 2.0, 6.0, 64, 0,
                                          appearance_embedding=app_vec, perturb=False)
        assert torch.equal(rgb[k].reshape(-1, 3), r) and torch.equal(depth[k].reshape(-1), dd[:, 0])
        o2, d2 = nerfmi_mod.get_rays(H, W, f, c2w.cuda(), rows=(5, 9))
        assert torch.equal(d2, d[5:14])
