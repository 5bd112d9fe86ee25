"""The generators of tests/degenerate_cases.py reach the regime they name — on the CPU, with the
oracle alone.  A GPU test on these inputs (tests/test_gpu_degenerate_rays.py) means what it says only
if the inputs really hold ties, exact cdf hits, unsorted rows, underflowing transmittance and a
scene with empty, opaque and partial rays; this file asserts that they do.
"""
import pytest
import torch

import degenerate_cases as D
from oracle import nerf_oracle as O

IMPORTANCE_SHAPES = ((33, 64, 128), (5, 7, 9), (7, 100, 64), (3, 256, 1024), (4, 1, 16), (2, 64, 1))
EXACT_SHAPES = ((4, 4), (64, 128), (64, 32))
COMPOSITE_N = (2, 5, 64, 65, 100, 192, 259)


def sorted_z(B, N, gen):
    return torch.sort(torch.rand(B, N, generator=gen) * 4 + 2, dim=-1).values


def test_fine_samples_is_the_oracles_resample():
    gen = torch.Generator().manual_seed(1)
    z, w, u = sorted_z(9, 64, gen), D.peaked_weights(9, 64, gen), torch.rand(9, 128, generator=gen)
    zf, _, _, _ = D.fine_samples(z, w, 128, u)
    z_all, _ = O.sample_importance_h1(torch.zeros(9, 3), torch.zeros(9, 3), z, w, 128, u)
    assert torch.equal(z_all, torch.sort(torch.cat([z, zf], -1), -1).values)


@pytest.mark.parametrize("B,N,Nf", [(64, 64, 128), (64, 7, 9)] + [s for s in IMPORTANCE_SHAPES if s[1] > 1 and s[2] > 1])
def test_peaked_weights_give_ties(B, N, Nf):
    gen = torch.Generator().manual_seed(21)
    z, w = sorted_z(B, N, gen), D.peaked_weights(B, N, gen)
    u = torch.rand(B, Nf, generator=gen)
    assert float(w[0, 0]) >= 0.1 and int((w[0] > 0).sum()) == 1
    assert float(w[1, N - 1]) >= 0.1
    if B > 3:
        assert not w[2].any() and bool((w[3] == 1e-12).all())
    zf, _, _, _ = D.fine_samples(z, w, Nf, u)
    hits = int((zf[:, :, None] == z[:, None, :]).any(-1).sum())
    pairs = int((zf[:, 1:] == zf[:, :-1]).sum())
    desc = int((zf[:, 1:] < zf[:, :-1]).sum())
    print(f"({B},{N},{Nf}): {hits} fine samples equal a coarse z, {pairs} equal neighbouring fine pairs, {desc} descending")
    assert hits >= 1 and pairs >= 1 and desc == 0
    z_all, pts = O.sample_importance_h1(torch.zeros(B, 3), torch.ones(B, 3), z, w, Nf, u)
    assert torch.isfinite(z_all).all() and torch.isfinite(pts).all()


@pytest.mark.parametrize("N,Nf", EXACT_SHAPES)
def test_exact_hits(N, Nf):
    z, w, u = D.exact_hit_case(N, Nf)
    zf, cdf, uu, inds = D.fine_samples(z, w, Nf, u)
    assert torch.equal(cdf, (torch.arange(N + 1, dtype=torch.float32) / N).expand(8, N + 1))
    # Nf | N: every u_j is a cdf entry.  N | Nf: u_j = j/Nf is cdf[k] at j = k Nf/N (every entry below
    # the last is hit) and lies strictly inside a bin otherwise.
    hit = torch.gather(cdf, 1, inds) == uu
    step = max(Nf // N, 1)
    assert bool(hit[:, ::step].all()) and int(hit.sum()) == 8 * min(N, Nf)
    assert bool((zf[:, ::step, None] == z[:, None, :]).any(-1).all())     # those fine z are coarse z, bit for bit
    z_all, _ = O.sample_importance_h1(torch.zeros(8, 3), torch.zeros(8, 3), z, w, Nf, u)
    assert torch.isfinite(z_all).all()
    if (N, Nf) == (4, 4):
        assert z_all[0].tolist() == [2, 2, 3, 3, 4, 4, 5, 5]


@pytest.mark.parametrize("B,N,Nf", IMPORTANCE_SHAPES)
def test_edge_uniforms_and_unsorted_rows(B, N, Nf):
    u = D.edge_uniforms(B, Nf)
    assert bool((u == 0).any()) and bool((u == D.U_MAX).any()) and float(u.max()) == D.U_MAX < 1.0
    assert float(u[0, 0]) == 0.0 and float(u[1, -1]) == D.U_MAX
    assert bool(((u > 0) & (u < D.U_MAX)).any()) or Nf == 1
    gen = torch.Generator().manual_seed(22)
    z, changed = D.unsorted_z(sorted_z(B, N, gen))
    asc = (z[:, 1:] >= z[:, :-1]).all(-1)
    assert torch.equal(~asc, changed)
    assert bool(changed.any()) == (N > 1) and bool((~changed).any())
    w = D.peaked_weights(B, N, gen)
    z_all, _ = O.sample_importance_h1(torch.zeros(B, 3), torch.zeros(B, 3), z, w, Nf, u)
    assert torch.isfinite(z_all).all()


def test_last_uniform_reaches_the_last_cdf_entry():
    """u_rand = U_MAX in the last column: u rounds to 1.0 and searchsorted returns N or N + 1, the
    indices the H1 clamp exists for."""
    gen = torch.Generator().manual_seed(23)
    z, w = sorted_z(33, 64, gen), D.peaked_weights(33, 64, gen)
    _, cdf, uu, inds = D.fine_samples(z, w, 128, D.edge_uniforms(33, 128))
    assert bool((uu[1::2, -1] == 1.0).all()) and bool((inds[1::2, -1] >= 64).all())


@pytest.mark.parametrize("N", COMPOSITE_N)
def test_ray_profiles(N):
    B = 67
    z, sigma, rgb = D.ray_profiles(B, N, torch.Generator().manual_seed(N))
    prof = [D.profile_of(b) for b in range(B)]
    assert sorted(set(prof)) == list(range(D.N_PROFILES))
    asc = (z[:, 1:] >= z[:, :-1]).all(-1)
    assert torch.equal(asc, D.sorted_rays(B))
    for b in range(B):
        if prof[b] == 8:
            assert bool((z[b] == z[b, 0]).all())
        if prof[b] == 9:
            q = D.start_of(b, N) % (N - 1)
            assert float(z[b, q + 1]) < float(z[b, q]) and float(sigma[b, q:q + 2].max()) <= 5
        if prof[b] == 7 and D.start_of(b, N) + 1 < N:
            s0 = D.start_of(b, N)
            assert bool((z[b, s0:s0 + 4] == z[b, s0]).all())
    assert torch.isfinite(z).all() and torch.isfinite(sigma).all() and bool((sigma >= 0).all())
    # the fp32 oracle on them, and its transmittance
    rm, dm, w = O.composite(rgb, sigma[..., None], z)
    assert torch.isfinite(rm).all() and torch.isfinite(dm).all() and torch.isfinite(w).all()
    dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full((B, 1), 1e-3)], -1)
    alpha = 1.0 - torch.exp(-sigma * dist)
    T = torch.cumprod(torch.cat([torch.ones(B, 1), 1.0 - alpha + 1e-10], -1), -1)     # T[:, s]: before sample s
    empty = [b for b in range(B) if prof[b] == 0]
    assert not rm[empty].any() and not dm[empty].any()
    walls = [b for b in range(B) if prof[b] in (1, 6)]
    for b in walls:
        s0 = D.start_of(b, N)
        assert float(T[b, s0]) == 1.0
        assert float(T[b, min(s0 + 6, N)]) == 0.0 or s0 + 6 > N, (b, s0)
    if N >= 64:
        assert bool((alpha[walls] == 1.0).any())
        tiny = torch.finfo(torch.float32).tiny
        assert bool(((T[walls] > 0) & (T[walls] < tiny)).any())          # through the denormals
        # the double-precision product crosses a 64-sample round boundary at 0 or denormal
        assert any(D.start_of(b, N) < 60 and float(T[b, 64]) == 0.0 for b in walls)
    # autograd through the fp32 oracle and through the straight-through float64 truth: finite
    for fn, dt in ((O.composite, torch.float32), (D.composite_f64_st, torch.float64)):
        r, s = rgb.to(dt).clone().requires_grad_(True), sigma[..., None].to(dt).clone().requires_grad_(True)
        a, b_, _ = fn(r, s, z)
        (a.sum() + b_.sum()).backward()
        assert torch.isfinite(r.grad).all() and torch.isfinite(s.grad).all(), dt
        if N == 64 and dt == torch.float32:
            assert float(s.grad[empty].abs().max()) > 1e6          # the empty rays' depth gradients
    # the straight-through truth is the fp32 function in value
    r64, d64, w64 = D.composite_f64_st(rgb.double(), sigma[..., None].double(), z)
    assert float((d64 - dm.double()).abs().max()) < 5e-6 and float((r64 - rm.double()).abs().max()) < 2e-6


BG_N = (2, 5, 64, 65, 100, 259)
DEAD_RAY = 1e-11       # a saturated ray none of whose gradients reaches this is dead: see below


def bg_losses(N, gate=None, bd=6.0):
    """ray_profiles at (67, N) with a background colour per ray and bd, and d sigma of
    sum(colour g) + sum(depth gd) + sum(acc ga) by the truth (at torch's exp) and by the fp32 baseline:
    (z, sigma, acc32, (values, d sigma) of the truth, the same of the baseline)."""
    B = 67
    z, sigma, rgb = D.ray_profiles(B, N, torch.Generator().manual_seed(N))
    g = torch.Generator().manual_seed(1000 + N)
    grm, gdm, ga = torch.randn(B, 3, generator=g), torch.randn(B, 1, generator=g), torch.randn(B, 1, generator=g)
    bg = torch.rand(B, 3, generator=g)
    out = []
    for fn, dt in ((D.composite_f64_st_bg, torch.float64), (D.composite_f32_bg, torch.float32)):
        r, s = rgb.to(dt).clone().requires_grad_(True), sigma[..., None].to(dt).clone().requires_grad_(True)
        _, dm, _, acc, col = fn(r, s, z, bg.to(dt), bd, gate=gate)
        ((col * grm.to(dt)).sum() + (dm * gdm.to(dt)).sum() + (acc * ga.to(dt)).sum()).backward()
        assert torch.isfinite(r.grad).all() and torch.isfinite(s.grad).all(), (N, dt)
        out.append(((col.detach().double(), dm.detach().double(), acc.detach().double()), s.grad[..., 0].double()))
    return z, sigma, D.acc32_of(sigma, z), out[0], out[1]


@pytest.mark.parametrize("N", BG_N)
def test_background_truth(N):
    """composite_f64_st_bg / composite_f32_bg on ray_profiles: finite gradients, the empty and the
    saturated rays are there (acc32 exactly 0 and exactly 1, none above 1, the same gate at both roundings
    of exp), the truth is the fp32 function in value, and what the gate does on a saturated ray.

    The gate on a ray with acc32 == 1: d acc / d sigma_s = dist_s e_s T_end / f_s, about 0 there, so taking
    the other branch (k = 1 - acc with its gradient) moves d sigma by less than 1e-6 of the ray's largest
    gradient on every saturated ray that has a gradient to speak of: 25 to 35 rays from N = 5 on, most of
    them with a change that is not exactly 0.  It does NOT hold on the rays that are opaque from sample 0
    (or tied at it): every e_s T_s underflows together, no d sigma of the ray exceeds 1.2e-12, and the
    gate's 1e-12 is of the size of the ray's own gradients, an order-1 effect (at N = 2, 13 of the 21
    saturated rays move by 0.26 to 290 times their largest gradient).  Those rays are asserted dead
    (gradient and change both below 1e-11), and at N = 2 that the effect is of order 1 on them.  So a
    comparison on a ray's own scale does see the gate there: tests/test_gpu_degenerate_train.py holds the
    saturated rays to the truth that way, and runs whole steps on saturated rays alone."""
    z, sigma, acc32, (val, ds), (val32, _) = bg_losses(N)
    assert int((acc32 == 0).sum()) >= 8 and int((acc32 == 1).sum()) >= 20 and not bool((acc32 > 1).any())
    assert torch.equal(acc32 < 1, D.acc32_of(sigma, z, D.exp_rn) < 1)
    for a, b, tol in zip(val, val32, (2e-6, 5e-6, 2e-6)):        # colour, depth, acc
        assert float((a - b).abs().max()) < tol
    sat = acc32 == 1
    _, _, _, (_, ds_open), _ = bg_losses(N, gate=torch.ones(67, dtype=torch.bool))
    change, largest = (ds - ds_open).abs().max(-1).values[sat], ds.abs().max(-1).values[sat]
    assert torch.equal(ds[~sat], ds_open[~sat])                  # k > 0 there under either rule
    dead = largest < DEAD_RAY
    print(f"N={N}: {int(sat.sum())} saturated rays, {int(dead.sum())} of them dead; gate changes d sigma by at most "
          f"{float((change / largest)[~dead].max()):.3g} of a live ray's largest gradient, {float(change.max()):.3g} absolute")
    assert bool((change[~dead] < 1e-6 * largest[~dead]).all())
    assert bool((change[dead] < DEAD_RAY).all())
    if N >= 5:       # measured: 25 to 35 live rays, 22 to 34 of them with a change that is not exactly 0
        assert int((~dead).sum()) >= 20 and int((change[~dead] > 0).sum()) >= 15
    else:            # N = 2: 16 dead rays, 13 with a gradient, all 13 moved by at least a quarter of it
        assert int(((largest > 0) & (change >= 0.1 * largest))[dead].sum()) >= 10


def test_sharp_state_scene(ref_state, golden, app_vec):
    o, d = D.sharp_rays(golden)
    assert o.shape == (256, 3)
    st = D.sharp_state(ref_state)
    rgb, depth, ex = O.volume_render(st, o, d, 2.0, 6.0, 64, app_vec)
    w = ex["weights"][..., 0]
    assert torch.isfinite(rgb).all() and torch.isfinite(depth).all() and torch.isfinite(w).all()
    empty = w.sum(-1) == 0
    opaque = w.max(-1).values > 0.99
    partial = ~empty & ~opaque
    first = (w > 0).float().argmax(-1)[~empty]
    n_first = len(set(first.tolist()))
    print(f"sharp_state: {int(empty.sum())} empty, {int(opaque.sum())} opaque, {int(partial.sum())} partial rays; "
          f"{n_first} distinct first-hit indices")
    for m in (empty, opaque, partial):
        assert int(m.sum()) >= 0.2 * 256
    assert n_first >= 10
    assert not rgb[empty].any() and not depth[empty].any()
    # and the hierarchical oracle on it, at the sizes of the GPU test
    for N, Nf in ((64, 128), (7, 5)):
        u = torch.rand(256, Nf, generator=torch.Generator().manual_seed(31))
        r, dd, exh = O.render_rays_h1(st, o, d, 2.0, 6.0, N, Nf, app_vec, None, u)
        assert torch.isfinite(r).all() and torch.isfinite(dd).all() and torch.isfinite(exh["weights"]).all()
        assert bool((exh["z_vals"][:, 1:] >= exh["z_vals"][:, :-1]).all())
