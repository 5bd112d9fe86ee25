"""Sampling and compositing on opaque, empty and tied rays: the regime of a trained scene, which the
parity tests' mild inputs (random-init density 0.0015-0.025, sigma = relu(3 randn), weights =
rand * (rand > 0.5)) never reach.  Inputs: tests/degenerate_cases.py (tests/test_degenerate_cases_cpu.py
shows on the CPU that they reach the regime).

  * composite forward: against the fp32 oracle at the suite's tolerance, plus what the arithmetic
    gives exactly (w = 0 where sigma = 0; empty rays exactly 0; w >= 0 on sorted rays), through the
    vector and the scalar kernel, across 64-sample rounds with the carried product at 0 or denormal;
  * composite backward (both entry points): truth = float64 autograd through the straight-through
    composite (degenerate_cases.composite_f64_st), baseline = torch fp32 autograd through the oracle on
    the CPU, each measured at its own rounding of exp (the kernels' is correctly rounded, torch's CPU
    exp is a 1-ulp function, and on the fog profile one ulp of exp is 1e-3 of alpha); per ray, errors
    scaled by the ray's largest true gradient (+1e-8, the existing tests' atol: a per-tensor scale
    would be swamped by the empty rays' ~1e10 depth gradients), and the GPU's scaled error no worse
    than the baseline's in max, p99.9 and median up to the project's 1.5
    (conftest.check_no_worse_than_cpu's rule);
  * importance + merge: bit-equal to the oracle under ties (lower_bound for coarse, upper_bound for
    fine), exact cdf hits, u = 0 and the largest u, and unsorted z (the full-rank fallback), with
    NaN-prefilled outputs so an unwritten slot shows;
  * the H1 render of a sharp scene (degenerate_cases.sharp_state) end to end under both MLP
    arithmetics: no worse than the fp32 CPU oracle against float64, exact zeros, staged == fused,
    unaligned outputs.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import degenerate_cases as D
from conftest import check_no_worse_than_cpu
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-6
B_COMP = 67
_CACHE = {}


def close(gpu, ref, rtol=RTOL, atol=ATOL, what=""):
    gpu = gpu.detach().float().cpu().numpy() if torch.is_tensor(gpu) else np.asarray(gpu)
    ref = ref.detach().float().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref)
    assert gpu.shape == ref.shape, (what, gpu.shape, ref.shape)
    err = np.abs(gpu - ref)
    bad = err > atol + rtol * np.abs(ref)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} outside tol; max abs err {err.max():.3g}"


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _L():
    from nerfmi import _lib as L
    return L


def unaligned(t):
    """The same values 4 bytes past a 16-byte boundary (the scalar-load kernels)."""
    buf = torch.empty(t.numel() + 1, device="cuda", dtype=t.dtype)
    buf[1:] = t.reshape(-1).cuda()
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % 16 == 4
    return out


def profiles(N):
    """ray_profiles at (67, N) and the fp32 oracle's composite of them, computed once."""
    def make():
        z, sigma, rgb = D.ray_profiles(B_COMP, N, torch.Generator().manual_seed(N))
        return z, sigma, rgb, O.composite(rgb, sigma[..., None], z)
    return cached(("profiles", N), make)


# ------------------------------------------------------------------------------ composite forward
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset4"])
@pytest.mark.parametrize("N", [2, 5, 64, 65, 100, 192, 259])
def test_composite_forward(N, offset):
    L = _L()
    lib, P = L.load(), L.ptr
    B = B_COMP
    z, sigma, rgb, (r_ref, d_ref, w_ref) = profiles(N)
    zc, sc, rc = (unaligned(t) if offset else t.cuda() for t in (z, sigma, rgb))
    rm = torch.full((B, 3), float("nan"), device="cuda")
    dm = torch.full((B,), float("nan"), device="cuda")
    wm = unaligned(torch.full((B, N), float("nan"))) if offset else torch.full((B, N), float("nan"), device="cuda")
    L.check(lib.nerf_composite(P(rc), P(sc), P(zc), B, N, P(rm), P(dm), P(wm), L.stream()), "composite")
    torch.cuda.synchronize()
    rm, dm, wm = rm.cpu(), dm.cpu(), wm.cpu()
    close(rm, r_ref, what=f"rgb N={N}")
    close(dm, d_ref[:, 0], what=f"depth N={N}")
    close(wm, w_ref[..., 0], what=f"weights N={N}")
    # exact consequences of the arithmetic
    assert not wm[sigma == 0].any(), "a weight where sigma is 0"
    empty = (sigma == 0).all(-1)
    assert int(empty.sum()) >= 8
    assert not rm[empty].any() and not dm[empty].any(), "an empty ray with a non-zero map"
    assert bool((wm[D.sorted_rays(B)] >= 0).all())
    # the maps without the optional weights output take the same kernel: same bits
    rm2, dm2 = torch.empty(B, 3, device="cuda"), torch.empty(B, device="cuda")
    L.check(lib.nerf_composite(P(rc), P(sc), P(zc), B, N, P(rm2), P(dm2), None, L.stream()), "composite")
    assert torch.equal(rm2.cpu(), rm) and torch.equal(dm2.cpu(), dm)


# ----------------------------------------------------------------------------- composite backward
def scaled_error(got, truth):
    """|got - truth| per value, each ray's scaled by its largest |truth| + 1e-8."""
    B = truth.shape[0]
    t = truth.reshape(B, -1).double()
    sc = t.abs().max(-1, keepdim=True).values + 1e-8
    return ((got.reshape(B, -1).double() - t).abs() / sc).flatten().numpy()


def no_worse_per_ray(got, truth_got, base, truth_base, what, factor=1.5):
    """conftest.check_no_worse_than_cpu's rule on the per-ray scaled errors, each evaluation against
    the truth at its own rounding of exp (degenerate_cases.composite_f64_st)."""
    eg, eb = scaled_error(got, truth_got), scaled_error(base, truth_base)
    sg = (eg.max(), np.quantile(eg, 0.999), np.median(eg))
    sb = (eb.max(), np.quantile(eb, 0.999), np.median(eb))
    print(f"{what}: per-ray scaled err vs truth max/p99.9/median  gpu {sg[0]:.3g} {sg[1]:.3g} {sg[2]:.3g}   "
          f"cpu fp32 autograd {sb[0]:.3g} {sb[1]:.3g} {sb[2]:.3g}   ratio "
          f"{sg[0] / (sb[0] + 1e-300):.2f} {sg[1] / (sb[1] + 1e-300):.2f} {sg[2] / (sb[2] + 1e-300):.2f}")
    for a, b, name in zip(sg, sb, ("max", "p99.9", "median")):
        assert a <= factor * b + 1e-9, (what, name, a, b)


def backward_refs(N, kind):
    """For ray_profiles at N and the loss
      kind "rgb" | "depth" | "both": sum(rgb_map * g_rgb) [+] sum(depth_map * g_depth)
      kind "mse": mean((rgb_map - target)^2)            (train.py:87)
    (drgb, dsigma, rgb_map, weights) three times: the truth for the kernels (float64 autograd through
    composite_f64_st at the kernels' correctly rounded exp), the truth for torch's CPU path (the same
    at torch's exp) and the baseline, fp32 autograd through the oracle; and the upstream tensors."""
    def make():
        z, sigma, rgb, _ = profiles(N)
        g = torch.Generator().manual_seed(1000 + N)
        grm, gdm, target = torch.randn(B_COMP, 3, generator=g), torch.randn(B_COMP, 1, generator=g), torch.rand(B_COMP, 3, generator=g)
        out = []
        for fn, dt in ((lambda r, s, zz: D.composite_f64_st(r, s, zz, D.exp_rn), torch.float64),
                       (D.composite_f64_st, torch.float64), (O.composite, torch.float32)):
            r, s = rgb.to(dt).clone().requires_grad_(True), sigma[..., None].to(dt).clone().requires_grad_(True)
            rm, dm, w = fn(r, s, z)
            if kind == "mse":
                loss = F.mse_loss(rm, target.to(dt))
            else:
                loss = (rm * grm.to(dt)).sum() * (kind != "depth") + (dm * gdm.to(dt)).sum() * (kind != "rgb")
            loss.backward()
            assert torch.isfinite(r.grad).all() and torch.isfinite(s.grad).all()
            out.append((r.grad.detach(), s.grad.detach()[..., 0], rm.detach(), w.detach()[..., 0]))
        return out[0], out[1], out[2], (grm, gdm, target)
    return cached(("bwd", N, kind), make)


def check_backward(N, what, dr, ds, truth, truth_cpu, base):
    dr, ds = dr.cpu(), ds.cpu()
    assert torch.isfinite(dr).all() and torch.isfinite(ds).all(), what
    no_worse_per_ray(ds, truth[1], base[1], truth_cpu[1], f"{what} dsigma N={N}")
    no_worse_per_ray(dr, truth[0], base[0], truth_cpu[0], f"{what} drgb N={N}")
    np.testing.assert_allclose(dr.numpy(), truth[0].numpy(), rtol=1e-4, atol=1e-8, err_msg=f"{what} drgb = w g")
    assert not dr[base[3] == 0].any(), f"{what}: drgb where the weight is 0"


@pytest.mark.parametrize("kind", ["rgb", "depth", "both"])
@pytest.mark.parametrize("N", [2, 5, 64, 65, 100, 259])
def test_composite_backward_grad(N, kind):
    L = _L()
    lib, P = L.load(), L.ptr
    B = B_COMP
    z, sigma, rgb, _ = profiles(N)
    truth, truth_cpu, base, (grm, gdm, _) = backward_refs(N, kind)
    rg, sg, zg = rgb.cuda().contiguous(), sigma.cuda().contiguous(), z.cuda().contiguous()
    ds = torch.full((B, N), float("nan"), device="cuda")
    dr = torch.full((B, N, 3), float("nan"), device="cuda")
    a = grm.cuda() if kind != "depth" else None
    b = gdm[:, 0].contiguous().cuda() if kind != "rgb" else None
    L.check(lib.nerf_composite_backward_grad(P(rg), P(sg), P(zg), P(a), P(b), B, N, P(ds), P(dr), L.stream()),
            "composite_backward_grad")
    torch.cuda.synchronize()
    check_backward(N, f"backward_grad[{kind}]", dr, ds, truth, truth_cpu, base)


@pytest.mark.parametrize("N", [2, 5, 64, 65, 100, 259])
def test_composite_backward_mse(N):
    """nerf_composite_backward: g = scale (rgb_map - target) from the GPU's own forward map, and sq_err."""
    L = _L()
    lib, P = L.load(), L.ptr
    B = B_COMP
    z, sigma, rgb, _ = profiles(N)
    truth, truth_cpu, base, (_, _, target) = backward_refs(N, "mse")
    rg, sg, zg, tg = (t.cuda().contiguous() for t in (rgb, sigma, z, target))
    rgb_map, depth = torch.empty(B, 3, device="cuda"), torch.empty(B, device="cuda")
    L.check(lib.nerf_composite(P(rg), P(sg), P(zg), B, N, P(rgb_map), P(depth), None, L.stream()), "composite")
    ds = torch.full((B, N), float("nan"), device="cuda")
    dr = torch.full((B, N, 3), float("nan"), device="cuda")
    sq = torch.full((B,), float("nan"), device="cuda")
    L.check(lib.nerf_composite_backward(P(rg), P(sg), P(zg), P(rgb_map), P(tg), B, N, 2.0 / (3 * B), P(ds), P(dr),
                                        P(sq), L.stream()), "composite_backward")
    torch.cuda.synchronize()
    np.testing.assert_allclose(sq.cpu().numpy(), ((truth[2] - target.double()) ** 2).sum(-1).numpy(), rtol=1e-5, atol=1e-7)
    check_backward(N, "backward[mse]", dr, ds, truth, truth_cpu, base)


# ------------------------------------------------------------------------------- importance, merge
IMPORTANCE_SHAPES = ((33, 64, 128), (5, 7, 9), (7, 100, 64), (3, 256, 1024), (4, 1, 16), (2, 64, 1))


def importance_case(case, B, N, Nf):
    gen = torch.Generator().manual_seed(50 + N + Nf)
    z = torch.sort(torch.rand(B, N, generator=gen) * 4 + 2, dim=-1).values
    if case == "exact":
        z, w, u = D.exact_hit_case(N, Nf, B)
    elif case == "peaked":
        w, u = D.peaked_weights(B, N, gen), torch.rand(B, Nf, generator=gen)
    elif case == "edge":
        w, u = D.peaked_weights(B, N, gen), D.edge_uniforms(B, Nf, gen)
        w[B // 2:] = torch.rand(B - B // 2, N, generator=gen)        # broad pdfs too: u over every bin
    else:
        z, _ = D.unsorted_z(z)
        w, u = D.peaked_weights(B, N, gen), D.edge_uniforms(B, Nf, gen)
    o = torch.randn(B, 3, generator=gen)
    d = F.normalize(torch.randn(B, 3, generator=gen), dim=-1)
    return o, d, z, w, u


def check_importance(nerfmi, case, B, N, Nf):
    L = _L()
    lib, P = L.load(), L.ptr
    o, d, z, w, u = importance_case(case, B, N, Nf)
    T = N + Nf
    z_ref, pts_ref = O.sample_importance_h1(o, d, z, w, Nf, u)
    zf_ref = D.fine_samples(z, w, Nf, u)[0]
    assert torch.equal(z_ref, torch.sort(torch.cat([z, zf_ref], -1), -1).values)
    # nerf_sample_importance
    z_all, pts = nerfmi.sample_importance(o.cuda(), d.cuda(), z.cuda(), w.cuda(), Nf, u_rand=u)
    assert torch.equal(z_all.cpu(), z_ref), (case, B, N, Nf)
    assert torch.equal(pts.cpu(), pts_ref), (case, B, N, Nf)
    # nerf_sample_importance_merge
    gen = torch.Generator().manual_seed(60)
    rgb_c, sigma_c = torch.rand(B, N, 3, generator=gen), torch.rand(B, N, generator=gen)
    u_lin = torch.linspace(0, 1, Nf + 1)[:-1].contiguous()
    zg, wg, ug, ul, rc, sc = (t.cuda().contiguous() for t in (z, w, u, u_lin, rgb_c, sigma_c))
    nan = float("nan")
    z_all = torch.full((B, T), nan, device="cuda")
    rgb_all = torch.full((B, T, 3), nan, device="cuda")
    sigma_all = torch.full((B, T), nan, device="cuda")
    z_fine = torch.full((B, Nf), nan, device="cuda")
    slot = torch.full((B, Nf), -1, dtype=torch.int32, device="cuda")
    L.check(lib.nerf_sample_importance_merge(
        P(zg), P(wg), P(rc), P(sc), B, N, Nf, P(ul), P(ug), ctypes.c_uint64(0), P(z_all), P(rgb_all), P(sigma_all),
        P(z_fine), P(slot), L.stream()), "importance_merge")
    torch.cuda.synchronize()
    za, ra, sa, zf, sl = (t.cpu() for t in (z_all, rgb_all, sigma_all, z_fine, slot))
    assert torch.equal(za, z_ref), (case, B, N, Nf)                       # no NaN left: every slot written
    assert torch.equal(zf, zf_ref), (case, B, N, Nf)
    assert int(sl.min()) >= 0 and int(sl.max()) < T
    rows = torch.arange(B)[:, None]
    fine = torch.zeros(B, T, dtype=torch.bool)
    fine[rows, sl.long()] = True
    assert int(fine.sum()) == B * Nf, "two fine samples share a slot"
    assert torch.equal(za[rows, sl.long()], zf), "a fine sample's slot does not hold its z"
    order = torch.sort(z, dim=-1, stable=True).indices                   # coarse samples, stable by z
    assert torch.equal(za[~fine].reshape(B, N), torch.gather(z, 1, order))
    assert torch.equal(ra[~fine].reshape(B, N, 3), rgb_c[rows, order]), "coarse rgb not at its merged slot"
    assert torch.equal(sa[~fine].reshape(B, N), torch.gather(sigma_c, 1, order)), "coarse sigma not at its merged slot"
    assert torch.isnan(ra[fine]).all() and torch.isnan(sa[fine]).all()   # fine slots are left to the fine MLP
    return z, zf


@pytest.fixture(scope="module")
def nerfmi_mod():
    import nerfmi
    return nerfmi


@pytest.mark.parametrize("case", ["peaked", "edge", "unsorted"])
@pytest.mark.parametrize("B,N,Nf", IMPORTANCE_SHAPES)
def test_importance_merge(nerfmi_mod, case, B, N, Nf):
    z, zf = check_importance(nerfmi_mod, case, B, N, Nf)
    if case == "peaked" and N > 1 and Nf > 1:           # the ties are there (the GPU's own fine z)
        assert bool((zf[:, :, None] == z[:, None, :]).any()) and bool((zf[:, 1:] == zf[:, :-1]).any())
    if case == "unsorted" and N > 1:
        assert not bool((z[:, 1:] >= z[:, :-1]).all())


@pytest.mark.parametrize("B,N,Nf", [(8, 4, 4), (8, 64, 128), (8, 64, 32)])
def test_importance_merge_exact_hits(nerfmi_mod, B, N, Nf):
    z, zf = check_importance(nerfmi_mod, "exact", B, N, Nf)
    step = max(Nf // N, 1)
    assert bool((zf[:, ::step, None] == z[:, None, :]).any(-1).all())     # fine z bit-equal to coarse z


# --------------------------------------------------------------------------- sharp scene, end to end
@pytest.fixture(scope="module", params=["f16x3", "f32"])
def arith(request):
    """The MLP arithmetic in force (include/nerfmi.h, nerf_arith): the sharp-scene tests run under both."""
    L = _L()
    prev = L.set_mlp_arith(request.param)
    yield request.param
    L.set_mlp_arith(prev)


def model_of(state):
    import nerfmi
    m = nerfmi.NeRF(nerfmi.Config())
    m.load_state_dict(state)
    return m.cuda().eval().requires_grad_(False)


def gpu_sigma(model, o, d, z, app):
    """sigma (B,n) of the render path's own MLP launch on samples z of rays (o, d): the per-stage entry
    points the staged render uses (nerf_normalize_dirs, nerf_mlp_forward), so the same bits."""
    from nerfmi.models import app_rows, run_mlp
    from nerfmi.render import packed_for
    L = _L()
    lib, dev = L.load(), L.device()
    B, n = z.shape
    og, dg = o.to(dev).contiguous(), d.to(dev).contiguous()
    dn = torch.empty_like(dg)
    L.check(lib.nerf_normalize_dirs(L.ptr(dg), B, L.ptr(dn), L.stream()), "nerf_normalize_dirs")
    a, rows = app_rows(app, B, dev)
    _, sigma = run_mlp(packed_for(model), og, dn, z.to(dev).contiguous(), B, n, a, rows, (B, n), torch.device("cpu"))
    return sigma[..., 0]


def sharp_refs(ref_state, golden, app_vec, N):
    """The sharp scene's rays and the oracle's coarse render of them in fp32 and in float64."""
    def make():
        o, d = D.sharp_rays(golden)
        st = D.sharp_state(ref_state)
        r32, d32, ex32 = O.volume_render(st, o, d, 2.0, 6.0, N, app_vec)
        st64 = {k: v.double() for k, v in st.items()}
        r64, d64, _ = O.volume_render(st64, o.double(), d.double(), 2.0, 6.0, N, app_vec.double())
        return o, d, st, st64, (r32, d32, ex32["z_vals"]), (r64, d64)
    return cached(("sharp", N), make)


SHARP_SHAPES = [(64, 128), (64, 195), (7, 5)]   # merged composite: staged vector | T = 259, unstaged scalar | T = 12


def sharp_render(nerfmi_mod, ref_state, golden, app_vec, arith, N, Nf):
    """The fused H1 render of the sharp scene on the GPU, once per (arithmetic, shape)."""
    def make():
        o, d, st, _, _, _ = sharp_refs(ref_state, golden, app_vec, N)
        model = model_of(st)
        u = torch.rand(o.shape[0], Nf, generator=torch.Generator().manual_seed(31))
        rgb, depth, ex = nerfmi_mod.render_rays(model, o.cuda(), d.cuda(), 2.0, 6.0, N, Nf,
                                                appearance_embedding=app_vec.cuda(), perturb=False,
                                                hierarchical=True, u_rand=u)
        out = dict(rgb=rgb.cpu(), depth=depth.cpu(), z=ex["z_vals"].cpu(), w=ex["weights"][..., 0].cpu(),
                   crgb=ex["rgb_map_coarse"].cpu(), cdepth=ex["depth_map_coarse"].cpu())
        for k, t in out.items():
            assert torch.isfinite(t).all(), k
        return model, u, out
    return cached(("render", arith, N, Nf), make)


@pytest.mark.parametrize("N,Nf", SHARP_SHAPES)
def test_sharp_scene_accuracy(nerfmi_mod, ref_state, golden, app_vec, arith, N, Nf):
    """Coarse maps against the oracle's float64 coarse render, and fine maps with the fine samples held
    equal: the oracle's pass over the GPU's own merged z in float64 (the truth) and in fp32 (the
    baseline).  Each map no worse than the fp32 CPU oracle in max, p99.9 and median up to 1.5
    (conftest.check_no_worse_than_cpu).  K = 1e5 on the density head turns fp32 rounding (of the sample
    points and of the MLP's raw density, ~2e-9 on 0.02) into errors of 1e-4 and more in the maps on
    both sides alike, so the 1e-4 tolerance is not the criterion here.  float64 means what it does in
    conftest.render_h1_f64: the same expressions from the same fp32 inputs (o, d, z), the sample
    points included."""
    o, d, st, st64, (r32, d32, _), (r64, d64) = sharp_refs(ref_state, golden, app_vec, N)
    _, _, g = sharp_render(nerfmi_mod, ref_state, golden, app_vec, arith, N, Nf)
    z = g["z"]
    dn, dn64 = O.normalize(d), O.normalize(d.double())
    with torch.no_grad():
        rf32, df32, _ = O._pass(st, o[:, None, :] + dn[:, None, :] * z[..., None], dn, z, app_vec)
        rf64, df64, _ = O._pass(st64, o.double()[:, None, :] + dn64[:, None, :] * z.double()[..., None], dn64,
                                z.double(), app_vec.double())
    failures = []
    for got, cpu, f64, what in ((g["crgb"], r32, r64, "coarse rgb"), (g["cdepth"], d32, d64, "coarse depth"),
                                (g["rgb"], rf32, rf64, "fine rgb, same z"), (g["depth"], df32, df64, "fine depth, same z")):
        try:
            check_no_worse_than_cpu(got, cpu, f64, f"sharp {arith} N={N} Nf={Nf} {what}")
        except AssertionError as e:
            failures.append(e.args[0])
    assert not failures, failures


@pytest.mark.parametrize("N,Nf", SHARP_SHAPES)
def test_sharp_scene_exact(nerfmi_mod, ref_state, golden, app_vec, arith, N, Nf):
    """What holds exactly on the sharp scene: ascending merged z, weight 0 where the model's sigma is 0,
    empty rays rendering exactly 0 in both passes, the staged path bit-identical to the fused call, and
    nerf_render_rays with weights_out / z_out one float off alignment matching the aligned call."""
    o, d, st, _, (_, _, zc), _ = sharp_refs(ref_state, golden, app_vec, N)
    model, u, g = sharp_render(nerfmi_mod, ref_state, golden, app_vec, arith, N, Nf)
    B, T = o.shape[0], N + Nf
    rgb, depth, z, w, crgb, cdepth = (g[k] for k in ("rgb", "depth", "z", "w", "crgb", "cdepth"))
    assert z.shape == (B, T) and bool((z[:, 1:] >= z[:, :-1]).all())
    # zeros: a sample the model gives sigma 0 has weight 0; a ray of such samples renders exactly 0
    sg_f = gpu_sigma(model, o, d, z, app_vec)
    sg_c = gpu_sigma(model, o, d, zc, app_vec)
    assert 0.3 < float((sg_f == 0).float().mean()) < 0.995, "the scene lost its empty space or its surfaces"
    assert not w[sg_f == 0].any(), "a fine weight where the model's sigma is 0"
    empty_c, empty_f = (sg_c == 0).all(-1), (sg_f == 0).all(-1)
    print(f"sharp {arith} N={N} Nf={Nf}: {int(empty_c.sum())} / {int(empty_f.sum())} rays empty in the coarse / fine pass, "
          f"{int((w.max(-1).values > 0.99).sum())} opaque")
    assert int(empty_c.sum()) >= 0.2 * B and int(empty_f.sum()) >= 0.1 * B
    assert not crgb[empty_c].any() and not cdepth[empty_c].any(), "coarse map of an empty ray"
    assert not rgb[empty_f].any() and not depth[empty_f].any(), "fine map of an empty ray"
    # the staged path runs the same kernels: identical bits
    timing = []
    kw = dict(appearance_embedding=app_vec.cuda(), perturb=False, hierarchical=True, u_rand=u)
    rgb2, depth2, ex2 = nerfmi_mod.render_rays(model, o.cuda(), d.cuda(), 2.0, 6.0, N, Nf, timing=timing, **kw)
    assert len(timing) == 2
    assert torch.equal(rgb2.cpu(), rgb) and torch.equal(depth2.cpu(), depth)
    assert torch.equal(ex2["z_vals"].cpu(), z) and torch.equal(ex2["weights"][..., 0].cpu(), w)
    assert torch.equal(ex2["rgb_map_coarse"].cpu(), crgb) and torch.equal(ex2["depth_map_coarse"].cpu(), cdepth)
    # nerf_render_rays with weights_out and z_out one float off 16-byte alignment
    from nerfmi.models import app_rows
    from nerfmi.ray_utils import linspace_table
    from nerfmi.render import packed_for
    L = _L()
    lib, dev, P = L.load(), L.device(), L.ptr
    oo, dd = o.cuda().contiguous(), d.cuda().contiguous()
    app, rows = app_rows(app_vec, B, dev)
    wbuf, zbuf = torch.full((B * T + 1,), float("nan"), device=dev), torch.full((B * T + 1,), float("nan"), device=dev)
    wu, zu = wbuf[1:], zbuf[1:]
    assert wu.data_ptr() % 16 != 0 and zu.data_ptr() % 16 != 0
    rgb3, depth3 = torch.empty(B, 3, device=dev), torch.empty(B, device=dev)
    crgb3, cdepth3 = torch.empty(B, 3, device=dev), torch.empty(B, device=dev)
    ws = torch.empty(lib.nerf_render_workspace_bytes(B, N, Nf), dtype=torch.uint8, device=dev)
    L.check(lib.nerf_render_rays(P(packed_for(model)), P(oo), P(dd), B, 2.0, 6.0, N, Nf, P(linspace_table(N, dev)),
                                 P(linspace_table(Nf, dev, drop_last=True)), 0, None, P(u.cuda().contiguous()), 0,
                                 0, P(app), rows, P(rgb3), P(depth3), P(wu), P(zu), P(crgb3), P(cdepth3), P(ws),
                                 ws.numel(), L.stream()), "nerf_render_rays")
    torch.cuda.synchronize()
    close(rgb3, rgb, rtol=1e-6, what=f"unaligned rgb T={T}")
    close(depth3, depth[:, 0], rtol=1e-6, what=f"unaligned depth T={T}")
    close(wu.reshape(B, T), w, rtol=1e-6, what=f"unaligned weights T={T}")
    assert torch.equal(zu.reshape(B, T).cpu(), z), T
