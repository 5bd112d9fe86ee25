"""The training-side kernels on opaque, empty and tied rays: the regime of a trained scene
(tests/degenerate_cases.py), where a background matters (acc == 0: the colour is the background;
acc == 1: k == 0) and where the fine pass matters (coarse weights a near-delta, merged rows full of ties).

  * nerf_composite_backward_grad_acc (g_acc and the background depth bd) on ray_profiles against the
    float64 straight-through truth with an opacity and a background (degenerate_cases.composite_f64_st_bg),
    by test_gpu_degenerate_rays.py's criterion: per-ray scaled errors no worse than fp32 torch autograd's
    in max, p99.9 and median up to 1.5;
  * nerf_composite_merged_backward / _acc on merged rows built the way the step builds them, from peaked
    coarse weights and edge uniforms (hundreds of tied pairs) and from unsorted coarse z (the full-rank
    fallback's src): bit-equal to the dense kernel on the gathered rows, and those rows held to the truth;
  * whole steps (dense and hierarchical, with and without the _bg options) on the sharp scene
    (degenerate_cases.sharp_state): equal to their stage composition, finite, deterministic, and what
    holds exactly on empty rays (the blended colour is the background; a batch of empty rays has every
    parameter gradient exactly 0 and the losses of its definitions);
  * the MLP data-gradient chain and the weight gradients behind such a scene against float64
    (test_gpu_accuracy.test_gradients_vs_float64's rule), with the sparse upstream the composite backward
    produces there.

Every output is prefilled with NaN so an unwritten slot shows.  Helpers: test_gpu_degenerate_rays (R),
test_gpu_train_hier (H), test_gpu_train_background (TB), test_gpu_accuracy (A).
"""
import os
import sys

import pytest
import torch

from conftest import REPO
from oracle import nerf_oracle as O

sys.path.insert(0, os.path.join(REPO, "tests"))
import degenerate_cases as D              # noqa: E402
import test_gpu_accuracy as A             # noqa: E402  (helpers only; the tests are collected from their own files)
import test_gpu_degenerate_rays as R      # noqa: E402
import test_gpu_train_background as TB    # noqa: E402
import test_gpu_train_hier as H           # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
B_COMP = R.B_COMP
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(scope="module", params=["f16x3", "f32"])
def arith(request):
    """The MLP arithmetic in force: the sharp-scene tests run under both."""
    L = H._lib()
    prev = L.set_mlp_arith(request.param)
    yield request.param
    L.set_mlp_arith(prev)


def backward_acc(z, sigma, rgb, g_rgb, g_depth, g_acc, bd):
    """nerf_composite_backward_grad_acc on device tensors (nullable gradients), outputs prefilled with NaN."""
    L = H._lib()
    lib, P = L.load(), L.ptr
    B, N = z.shape
    ds, dr = torch.full((B, N), NAN, device="cuda"), torch.full((B, N, 3), NAN, device="cuda")
    L.check(lib.nerf_composite_backward_grad_acc(P(rgb), P(sigma), P(z), P(g_rgb), P(g_depth), B, N, P(ds), P(dr),
                                                 P(g_acc), bd, L.stream()), "composite_backward_grad_acc")
    torch.cuda.synchronize()
    return ds, dr


def dev(t):
    return None if t is None else t.cuda().contiguous()


# --------------------------------------------- 2. nerf_composite_backward_grad_acc against the truth
KINDS = {          # (grad_map, grad_depth, g_acc, bd)
    "acc": (False, False, True, None),
    "bd": (False, True, False, 6.0),
    "all": (True, True, True, 6.0),
    "all_nan_bd": (True, True, True, None),
}


def truth_refs(z, sigma, rgb, ups, use, bd):
    """(drgb, dsigma, rgb_map, weights) of sum(rgb_map grm) + sum(depth gdm) + sum(acc ga) (the terms in
    `use`) three times: the truth at the kernels' exp, the truth at torch's exp, the fp32 baseline
    (test_gpu_degenerate_rays.backward_refs' triple)."""
    grm, gdm, ga = ups
    B = z.shape[0]
    out = []
    for fn, dt in ((lambda r, s: D.composite_f64_st_bg(r, s, z, None, bd, D.exp_rn), torch.float64),
                   (lambda r, s: D.composite_f64_st_bg(r, s, z, None, bd), torch.float64),
                   (lambda r, s: D.composite_f32_bg(r, s, z, None, bd), torch.float32)):
        r, s = rgb.to(dt).clone().requires_grad_(True), sigma[..., None].to(dt).clone().requires_grad_(True)
        rm, dm, w, acc, _ = fn(r, s)
        loss = (rm * grm.to(dt)).sum() * use[0] + (dm * gdm.to(dt).reshape(B, 1)).sum() * use[1] + \
            (acc * ga.to(dt).reshape(B, 1)).sum() * use[2]
        loss.backward()
        assert torch.isfinite(r.grad).all() and torch.isfinite(s.grad).all()
        out.append((r.grad.detach(), s.grad.detach()[..., 0], rm.detach(), w.detach()[..., 0]))
    return out


def acc_refs(N, kind):
    def make():
        z, sigma, rgb, _ = R.profiles(N)
        g = torch.Generator().manual_seed(2000 + N)
        ups = torch.randn(B_COMP, 3, generator=g), torch.randn(B_COMP, generator=g), torch.randn(B_COMP, generator=g)
        return truth_refs(z, sigma, rgb, ups, KINDS[kind][:3], KINDS[kind][3]), ups
    return cached(("acc", N, kind), make)


# A saturated ray's d sigma against the truth on the ray's own scale.  The kernel evaluates the truth's
# expressions in double from the same fp32 alpha, factor and dist, and differs from it by the fp32 value of
# e = exp(-sigma dist) in the last factor (2^-24 relative) and the one rounding of d sigma (2^-24): 2^-23 of
# an element, so of the ray's largest; 8x that is allowed.  Both sides form d alpha_s = dw_s T_s - (sum_{t>s}
# dw_t w_t) / f_s in double, a difference of terms of size G = max |dw| that cancels to ~0 on these rays, each
# in its own order over N terms: N 2^-53 G apiece, times dist e <= 4, so N 2^-50 G absolute, with G bounded by
# |g_acc| + 6 |g_depth| + sum |g_rgb| (|z - bd|, |z - mean| <= 6, rgb <= 1).  Below fp32's smallest normal
# number a value has no relative precision: 1e-37.
SAT_RTOL, SAT_ATOL = 2.0 ** -20, 1e-37


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("N", [2, 5, 64, 65, 100, 259])
def test_composite_backward_grad_acc(N, kind):
    """Measured (MI355X): d sigma per-ray scaled error 1.3e-7 to 3.9e-7 in max over the 24 cases, against the
    fp32 baseline's 6.1e-7 to 3.7; ratios at most 0.60 in max, 0.59 in p99.9 and 1.02 in median.

    On the saturated rays that criterion is weak: with g_acc alone their true gradient is ~0 and fp32
    autograd's is its cancellation noise (errors of order 1 on the 1e-8 the scale adds), and the gate of k
    shows only through that 1e-8, on the rays opaque from sample 0 at N = 2 and 5, whose every gradient is
    below 1e-11 and where the gate is an order-1 effect (test_degenerate_cases_cpu.test_background_truth).
    So the saturated rays are also held to the truth directly, each on the scale of its OWN largest
    gradient: SAT_RTOL of it, plus SAT_ATOL.  Measured: at most 0.41 of that bound; dmean = bd where
    k == 0 exceeds it 56 and 42 times at N = 2, 22 and 6.9 times at N = 5 (kinds "bd", "all"), 1.2 times at
    N = 64 (a partial ray cannot see that edit, k > 0 there either way)."""
    z, sigma, rgb, _ = R.profiles(N)
    (truth, truth_cpu, base), (grm, gdm, ga) = acc_refs(N, kind)
    use_map, use_depth, use_acc, bd = KINDS[kind]
    ds, dr = backward_acc(dev(z), dev(sigma), dev(rgb), dev(grm) if use_map else None, dev(gdm) if use_depth else None,
                          dev(ga) if use_acc else None, NAN if bd is None else bd)
    sat = D.acc32_of(sigma, z, D.exp_rn) == 1
    assert int(sat.sum()) >= 20
    err = (ds.cpu().double() - truth[1])[sat].abs().max(-1).values
    largest = truth[1][sat].abs().max(-1).values
    G = (ga.abs() * use_acc + 6.0 * gdm.abs() * use_depth + grm.abs().sum(-1) * use_map)[sat].double()
    tol = SAT_RTOL * largest + N * 2.0 ** -50 * G + SAT_ATOL
    print(f"backward_grad_acc[{kind}] N={N}: {int(sat.sum())} saturated rays, largest true |d sigma| per ray "
          f"{float(largest.min()):.3g} to {float(largest.max()):.3g}, error at most {float((err / tol).max()):.3g} of "
          f"the bound, {float(err.max()):.3g} absolute")
    assert bool((err <= tol).all()), float((err / tol).max())
    R.check_backward(N, f"backward_grad_acc[{kind}]", dr, ds, truth, truth_cpu, base)
    if kind == "acc":
        # an empty ray: T == 1, e == 1, the suffix 0, so d sigma_s = g_acc dist_s, the double product rounded once
        empty = torch.tensor([D.profile_of(b) == 0 for b in range(B_COMP)])
        assert int(empty.sum()) >= 8 and not bool(sigma[empty].any())
        dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full((B_COMP, 1), 1e-3)], -1)
        want = ga[empty, None].double() * dist[empty].double()
        assert bool(((ds.cpu()[empty].double() - want).abs() <= 2.0 ** -24 * want.abs()).all())
        assert not bool(dr.cpu().any())                      # no grad_map: drgb = w 0


# ------------------------------------------------- 3. merged backwards on tied and unsorted rows
MERGED = [(37, 8, 16), (5, 7, 10), (7, 64, 65), (3, 256, 1024)]   # staged vector | scalar | T = 129 | unstaged
FINE_SIGMA = (0.0, 1e-3, 50.0, 300.0, 1e4, 3e38)


def merged_rows(B, N, Nf, unsorted):
    """Merged rows the way the step builds them: z_all and src from nerf_sample_importance_src on peaked
    coarse weights and edge uniforms; coarse (sigma, rgb) from ray_profiles, fine sigma a seeded choice of
    ray_profiles' values per sample, fine rgb random.  Everything on the CPU but z_all / src / idx."""
    L = H._lib()
    lib, P, s = L.load(), L.ptr, L.stream()
    T = N + Nf
    gen = torch.Generator().manual_seed(300 + N + Nf)
    z = torch.sort(torch.rand(B, N, generator=gen) * 4 + 2, dim=-1).values
    if unsorted:
        z, changed = D.unsorted_z(z)
        assert bool(changed.any())
    w, u = D.peaked_weights(B, N, gen), D.edge_uniforms(B, Nf, gen)
    _, sig_c, rgb_c = D.ray_profiles(B, N, gen)
    sig_f = torch.tensor(FINE_SIGMA)[torch.randint(0, len(FINE_SIGMA), (B, Nf), generator=gen)]
    rgb_f = torch.rand(B, Nf, 3, generator=gen)
    desc = z[:, 1:] < z[:, :-1]
    if unsorted:       # ray_profiles' rule for a descending pair: sigma <= 5 on both of its samples
        assert bool(desc.any())
        pair = torch.cat([desc, torch.zeros(B, 1, dtype=torch.bool)], 1) | torch.cat([torch.zeros(B, 1, dtype=torch.bool), desc], 1)
        sig_c = torch.where(pair, sig_c.clamp_max(5.0), sig_c)
        sig_f[changed] = sig_f[changed].clamp_max(5.0)
    else:
        assert not bool(desc.any())
    _, u_lin = H._tables(N, Nf, L.device())
    zg, wg, ug = dev(z), dev(w), dev(u)
    z_all, z_fine = torch.full((B, T), NAN, device="cuda"), torch.full((B, Nf), NAN, device="cuda")
    src = torch.full((B, T), -1, dtype=torch.int16, device="cuda")
    L.check(lib.nerf_sample_importance_src(P(zg), P(wg), B, N, Nf, P(u_lin), P(ug), 0, P(z_all), P(z_fine), P(src), s),
            "importance_src")
    torch.cuda.synchronize()
    idx = src.long() & 0xFFFF
    # a permutation of the ray's cat indices (the merged kernel indexes LDS with it), an ascending merged row
    assert torch.equal(torch.sort(idx, dim=1).values, torch.arange(T, device="cuda").expand(B, T))
    za = z_all.cpu()
    assert torch.isfinite(za).all() and bool((za[:, 1:] >= za[:, :-1]).all())
    ties = int((za[:, 1:] == za[:, :-1]).sum())
    print(f"({B},{N},{Nf}) unsorted={unsorted}: {ties} tied adjacent pairs in z_all")
    if not unsorted:
        assert ties >= B, ties
    return dict(z_all=z_all, src=src, idx=idx, rgb_c=rgb_c, sig_c=sig_c, rgb_f=rgb_f, sig_f=sig_f, gen=gen)


@pytest.mark.parametrize("unsorted", [False, True], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("B,N,Nf", MERGED)
def test_merged_backwards_on_tied_rows(B, N, Nf, unsorted):
    L = H._lib()
    lib, P, s = L.load(), L.ptr, L.stream()
    T = N + Nf
    m = merged_rows(B, N, Nf, unsorted)
    gen, idx, z_all = m["gen"], m["idx"], m["z_all"]
    rgb_c, sig_c, rgb_f, sig_f = (dev(m[k]) for k in ("rgb_c", "sig_c", "rgb_f", "sig_f"))
    ups = torch.randn(B, 3, generator=gen), torch.randn(B, generator=gen), torch.randn(B, generator=gen)
    g_map, g_depth, g_acc = (dev(t) for t in ups)
    pre_s, pre_r = dev(torch.randn(B, N, generator=gen)), dev(torch.randn(B, N, 3, generator=gen))
    rgb_m = torch.gather(torch.cat([rgb_c, rgb_f], 1), 1, idx[..., None].expand(B, T, 3)).contiguous()
    sig_m = torch.gather(torch.cat([sig_c, sig_f], 1), 1, idx).contiguous()

    def merged(ga, bd, accumulate):
        ds_c = pre_s.clone() if accumulate else torch.full((B, N), NAN, device="cuda")
        dr_c = pre_r.clone() if accumulate else torch.full((B, N, 3), NAN, device="cuda")
        ds_f, dr_f = torch.full((B, Nf), NAN, device="cuda"), torch.full((B, Nf, 3), NAN, device="cuda")
        args = [P(rgb_c), P(sig_c), P(rgb_f), P(sig_f), P(m["src"]), P(z_all), P(g_map), P(g_depth), B, N, Nf, accumulate,
                P(ds_c), P(dr_c), P(ds_f), P(dr_f)]
        if ga is None:
            L.check(lib.nerf_composite_merged_backward(*args, s), "composite_merged_backward")
        else:
            L.check(lib.nerf_composite_merged_backward_acc(*args, P(ga), bd, s), "composite_merged_backward_acc")
        torch.cuda.synchronize()
        return ds_c, dr_c, ds_f, dr_f

    for what, ga, bd in (("plain", None, NAN), ("acc", g_acc, NAN), ("acc+bd", g_acc, 5.5)):
        # the dense kernel on the gathered rows, scattered back to cat[coarse, fine] order
        if ga is None:
            ds_m, dr_m = torch.full((B, T), NAN, device="cuda"), torch.full((B, T, 3), NAN, device="cuda")
            L.check(lib.nerf_composite_backward_grad(P(rgb_m), P(sig_m), P(z_all), P(g_map), P(g_depth), B, T, P(ds_m),
                                                     P(dr_m), s), "composite_backward_grad")
            torch.cuda.synchronize()
        else:
            ds_m, dr_m = backward_acc(z_all, sig_m, rgb_m, g_map, g_depth, ga, bd)
        assert torch.isfinite(ds_m).all() and torch.isfinite(dr_m).all(), what
        ref_ds = torch.full_like(ds_m, NAN).scatter_(1, idx, ds_m)
        ref_dr = torch.full_like(dr_m, NAN).scatter_(1, idx[..., None].expand(B, T, 3), dr_m)
        ds_c, dr_c, ds_f, dr_f = merged(ga, bd, 0)
        assert torch.equal(torch.cat([ds_c, ds_f], 1), ref_ds), (what, "dsigma")
        assert torch.equal(torch.cat([dr_c, dr_f], 1), ref_dr), (what, "drgb")
        # accumulate: coarse rows = prefill + term in one float add, fine rows as before
        as_c, ar_c, as_f, ar_f = merged(ga, bd, 1)
        assert torch.equal(as_c, pre_s + ds_c) and torch.equal(ar_c, pre_r + dr_c), what
        assert torch.equal(as_f, ds_f) and torch.equal(ar_f, dr_f), what
        if not unsorted:
            # the tied rows against float64: the criterion of section 2 on the dense kernel's (= the merged one's) output
            use = (True, True, ga is not None)
            truth, truth_cpu, base = truth_refs(z_all.cpu(), sig_m.cpu(), rgb_m.cpu(), ups, use, None if bd != bd else bd)
            R.check_backward(T, f"merged rows ({B},{N},{Nf}) [{what}]", dr_m, ds_m, truth, truth_cpu, base)
    assert float(ref_ds.abs().max()) > 0 and float(ref_dr.abs().max()) > 0


# ------------------------------------------------------------- 4. whole steps on a sharp scene
SHARP = [(32, 40), (64, 128)]
def options(alpha, bg):
    """no alpha, one colour | alpha, no background | alpha with exact 0 and 1, one colour per ray"""
    return {"bg1": (None, bg[:1].contiguous()), "alpha": (alpha, None), "alpha+bg": (alpha, bg)}


def sharp_case(ref_state, golden, app_vec, arith, N, Nf):
    """The sharp scene's 256 rays with seeded t_rand / u_rand / target, the packed sharp model, and the
    stage forwards of the dense and the hierarchical step, once per (arithmetic, shape); the regime is
    asserted on the GPU's own forward."""
    def make():
        L = H._lib()
        d_ = L.device()
        o, d = D.sharp_rays(golden)
        B = o.shape[0]
        g = torch.Generator().manual_seed(N)
        r = dict(o=o, d=d, t_rand=torch.rand(B, N, generator=g), u_rand=torch.rand(B, Nf, generator=g),
                 target=torch.rand(B, 3, generator=g))
        packed, packedT = H._packed(D.sharp_state(ref_state), d_)
        app, rows = H._app(app_vec, B, 1, d_)
        st = H.stage_forward(packed, r, N, Nf, app, rows)
        T = N + Nf
        c, f, idx = st["c"], st["f"], st["src"].long() & 0xFFFF
        rgb_all = torch.gather(torch.cat([c["rgb"].view(B, N, 3), f["rgb"].view(B, Nf, 3)], 1), 1,
                               idx[..., None].expand(B, T, 3)).contiguous()
        sigma_all = torch.gather(torch.cat([c["sigma"].view(B, N), f["sigma"].view(B, Nf)], 1), 1, idx).contiguous()
        acc_c, acc_f = TB.acc_of(c["rgb"], c["sigma"], st["z"]), TB.acc_of(rgb_all, sigma_all, st["z_all"])
        torch.cuda.synchronize()
        za = st["z_all"].cpu()
        ties = int((za[:, 1:] == za[:, :-1]).sum())
        counts = [(int((a == 0).sum()), int((a >= 1).sum()), int(((a > 1e-3) & (a < 1 - 1e-3)).sum())) for a in (acc_c, acc_f)]
        print(f"sharp {arith} ({N},{Nf}): coarse acc == 0 / >= 1 / partial {counts[0]}, merged {counts[1]}, {ties} tied pairs in "
              f"the merged z, {float((c['sigma'] == 0).float().mean()):.3f} of the coarse sigma exactly 0")
        assert min(counts[0]) >= 20 and min(counts[1]) >= 20 and ties >= 100, (counts, ties)
        alpha, bg = TB.bg_case(B, seed=N + Nf)
        return dict(r=r, packed=packed, packedT=packedT, app=app, rows=rows, st=st, acc_c=acc_c, acc_f=acc_f, alpha=alpha,
                    bg=bg, B=B)
    return cached(("sharp", arith, N, Nf), make)


def close_parts(loss, ref, what):
    for k in range(len(ref)):
        assert abs(float(loss[k]) - float(ref[k])) <= 1e-6 * float(ref[k]), (what, k, float(loss[k]), float(ref[k]))


def same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        if x is not None:
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, i)


@pytest.mark.parametrize("N,Nf", SHARP)
def test_sharp_dense_step(ref_state, golden, app_vec, arith, N, Nf):
    """nerf_train_backward and nerf_train_backward_bg against dense_reference (the stage entry points and
    the head in torch, whose torch.where(k > 0, ...) is the kernel's rule on the saturated rays)."""
    S = sharp_case(ref_state, golden, app_vec, arith, N, Nf)
    packed, packedT, app, rows, r, B = (S[k] for k in ("packed", "packedT", "app", "rows", "r", "B"))
    fw = TB.dense_forward(packed, r, N, app, rows)
    st = TB.dense_stage(packed, r, N, app, rows)
    assert torch.equal(st["rgb_map"], fw["rgb_map"]) and torch.equal(st["c"]["sigma"], S["st"]["c"]["sigma"])
    empty = S["acc_c"] == 0
    assert not bool(fw["rgb_map"][empty].any())
    # the original entry, and the _bg entry with the options off: its bits
    gs0, dapp0, loss0, _ = TB.dense_backward(packed, packedT, fw, N, app, rows)
    gs1, dapp1, loss1, final1 = TB.dense_backward(packed, packedT, fw, N, app, rows, (None, None, 0.0))
    TB.check_grads(gs1, dapp1, gs0, dapp0, rows, 0, "options off", exact=True)
    assert torch.equal(loss1[:1], loss0[:1]) and float(loss1[1]) == 0.0 and torch.equal(final1, fw["rgb_map"])
    gs_ref, dapp_ref, loss_ref, _ = TB.dense_reference(packed, packedT, st, N, app, rows, None, None, 0.0)
    TB.check_grads(gs0, dapp0, gs_ref, dapp_ref, rows, 1e-6, "nerf_train_backward")
    assert torch.isfinite(dapp0).all()
    close_parts(loss0[:1], loss_ref[:1], "nerf_train_backward")
    for name, (al, b) in options(S["alpha"], S["bg"]).items():
        for aw in (0.0, 0.1):
            gs, dapp, loss, final = TB.dense_backward(packed, packedT, fw, N, app, rows, (al, b, aw))
            gs_ref, dapp_ref, loss_ref, final_ref = TB.dense_reference(packed, packedT, st, N, app, rows, al, b, aw)
            torch.cuda.synchronize()
            TB.check_grads(gs, dapp, gs_ref, dapp_ref, rows, 1e-6, (name, aw))
            assert torch.isfinite(dapp).all() and torch.isfinite(loss).all() and torch.isfinite(final).all()
            close_parts(loss, loss_ref, (name, aw))
            assert torch.equal(final.view(torch.int32), final_ref.view(torch.int32)), (name, aw)
            want = torch.zeros(B, 3, device=final.device) if b is None else b.expand(B, 3)
            assert torch.equal(final[empty], want[empty]), (name, aw, "an empty ray's colour is the background")
    # the same step twice, forward included: the same bits (alpha, a colour per ray, acc_weight 0.1)
    bgo = (S["alpha"], S["bg"], 0.1)
    first = TB.dense_backward(packed, packedT, fw, N, app, rows, bgo)
    again = TB.dense_backward(packed, packedT, TB.dense_forward(packed, r, N, app, rows), N, app, rows, bgo)
    same_bits(list(again[0]) + list(again[1:]), list(first[0]) + list(first[1:]), "determinism")


@pytest.mark.parametrize("N,Nf", SHARP)
def test_sharp_hierarchical_step(ref_state, golden, app_vec, arith, N, Nf):
    """nerf_train_hier_backward and its _bg form against hier_reference, coarse_weight in {0, 1}."""
    S = sharp_case(ref_state, golden, app_vec, arith, N, Nf)
    packed, packedT, app, rows, r, st, B = (S[k] for k in ("packed", "packedT", "app", "rows", "r", "st", "B"))
    fw = H.hier_forward(packed, r, N, Nf, app, rows)
    assert torch.equal(fw["rgb_map"], st["rgb_map"]) and torch.equal(fw["rgb_c"], st["rgb_c"])
    assert torch.equal(fw["z_out"], st["z_all"])
    empty_c, empty_f = S["acc_c"] == 0, S["acc_f"] == 0
    assert int(empty_f.sum()) >= 20
    for cw in (0.0, 1.0):
        gs0, dapp0, loss0 = H.hier_backward(packed, packedT, fw, N, Nf, cw, app, rows)
        gs1, dapp1, loss1, final1, cfinal1 = TB.hier_backward_bg(packed, packedT, fw, N, Nf, cw, app, rows, None, None, 0.0)
        TB.check_grads(gs1, dapp1, gs0, dapp0, rows, 0, "options off", exact=True)
        assert torch.equal(loss1[:2], loss0) and not bool(loss1[2:].any())
        assert torch.equal(final1, fw["rgb_map"]) and torch.equal(cfinal1, fw["rgb_c"])
        gs_ref, dapp_ref, loss_ref, _, _ = TB.hier_reference(packed, packedT, st, N, Nf, cw, app, rows, None, None, 0.0)
        TB.check_grads(gs0, dapp0, gs_ref, dapp_ref, rows, 1e-6, ("nerf_train_hier_backward", cw))
        assert torch.isfinite(dapp0).all()
        close_parts(loss0, loss_ref[:2], ("nerf_train_hier_backward", cw))
        for name, (al, b) in options(S["alpha"], S["bg"]).items():
            for aw in (0.0, 0.1):
                gs, dapp, loss, final, cfinal = TB.hier_backward_bg(packed, packedT, fw, N, Nf, cw, app, rows, al, b, aw)
                gs_ref, dapp_ref, loss_ref, final_ref, cfinal_ref = TB.hier_reference(packed, packedT, st, N, Nf, cw, app,
                                                                                      rows, al, b, aw)
                torch.cuda.synchronize()
                what = (name, cw, aw)
                TB.check_grads(gs, dapp, gs_ref, dapp_ref, rows, 1e-6, what)
                assert torch.isfinite(dapp).all() and torch.isfinite(loss).all(), what
                close_parts(loss, loss_ref, what)
                assert torch.equal(final.view(torch.int32), final_ref.view(torch.int32)), what
                assert torch.equal(cfinal.view(torch.int32), cfinal_ref.view(torch.int32)), what
                want = torch.zeros(B, 3, device=final.device) if b is None else b.expand(B, 3)
                assert torch.equal(final[empty_f], want[empty_f]) and torch.equal(cfinal[empty_c], want[empty_c]), what
    # the same step twice, forward included: the same bits (coarse_weight 1, alpha, a colour per ray, acc_weight 0.1)
    first = TB.hier_backward_bg(packed, packedT, fw, N, Nf, 1.0, app, rows, S["alpha"], S["bg"], 0.1)
    again = TB.hier_backward_bg(packed, packedT, H.hier_forward(packed, r, N, Nf, app, rows), N, Nf, 1.0, app, rows,
                                S["alpha"], S["bg"], 0.1)
    same_bits(list(again[0]) + list(again[1:]), list(first[0]) + list(first[1:]), "determinism")


@pytest.mark.parametrize("N,Nf", SHARP)
def test_batch_of_empty_rays(ref_state, golden, app_vec, arith, N, Nf):
    """The rays the forward found empty (in both passes), gathered into a launch of their own with a ray
    count that 4 does not divide: drgb = w g = 0 and d v_s = d sigma_s [sigma_s > 0] = 0, so every
    parameter gradient and dapp are exactly 0, the colour loss is mean((bg - target')^2) and the opacity
    loss mean(alpha^2)."""
    S = sharp_case(ref_state, golden, app_vec, arith, N, Nf)
    packed, packedT, app, rows = (S[k] for k in ("packed", "packedT", "app", "rows"))
    keep = torch.nonzero((S["acc_c"] == 0) & (S["acc_f"] == 0))[:, 0].cpu()
    if keep.numel() % 4 == 0:
        keep = keep[:-1]
    E = keep.numel()
    assert E >= 20 and E % 4 != 0
    r = H._take(S["r"], keep)
    alpha, bg = S["alpha"][keep.cuda()].contiguous(), S["bg"][keep.cuda()].contiguous()
    tp = alpha[:, None] * r["target"].cuda() + (1.0 - alpha)[:, None] * bg
    l_rgb, l_acc = float(((bg - tp).double() ** 2).mean()), float((alpha.double() ** 2).mean())
    assert l_rgb > 0 and l_acc > 0
    fw_d = TB.dense_forward(packed, r, N, app, rows)
    fw_h = H.hier_forward(packed, r, N, Nf, app, rows)
    torch.cuda.synchronize()
    # the same samples give the same (empty) rays in the smaller launch
    assert not bool(fw_d["rgb_map"].any()) and not bool(fw_h["rgb_map"].any()) and not bool(fw_h["rgb_c"].any())
    assert not bool(fw_h["weights"].any()) and not bool(fw_h["w_c"].any())
    for aw in (0.0, 0.1):
        gs, dapp, loss, final = TB.dense_backward(packed, packedT, fw_d, N, app, rows, (alpha, bg, aw))
        assert all(not bool(g.view(torch.int32).bitwise_and(0x7FFFFFFF).any()) for g in gs), ("dense", aw)
        assert not bool(dapp.any()) and torch.equal(final, bg)
        close_parts(loss, (l_rgb, l_acc), ("dense", aw))
        gs, dapp, loss, final, cfinal = TB.hier_backward_bg(packed, packedT, fw_h, N, Nf, 1.0, app, rows, alpha, bg, aw)
        assert all(not bool(g.view(torch.int32).bitwise_and(0x7FFFFFFF).any()) for g in gs), ("hier", aw)
        assert not bool(dapp.any()) and torch.equal(final, bg) and torch.equal(cfinal, bg)
        close_parts(loss, (l_rgb, l_rgb, l_acc, l_acc), ("hier", aw))


@pytest.mark.parametrize("N,Nf", SHARP)
def test_batch_of_saturated_rays(ref_state, golden, app_vec, arith, N, Nf):
    """The rays the forward found saturated (acc >= 1, k == 0), gathered into a launch of their own: where
    the head's rule "g_acc takes -(bg . g_rgb) only where k > 0" shows.  In the whole batch the partial rays
    carry every gradient and the rule moves no tensor by more than ~1e-8; here what reaches the trunk is
    d sigma [sigma > 0], small on these rays (d density_head.bias 6e-9 to 4e-7), and a g_acc that passed
    -(bg . g_rgb) at k == 0 moves it by the order of a ray's own gradient on many rays (the rays
    test_degenerate_cases_cpu.test_background_truth calls dead are of this kind).  Measured: the step and the
    composition agree bit for bit; kb >= 0 for kb > 0 in bg_loss_kernel puts pts_linears.0.weight 4.8e-5
    (32 samples) and 8.4e-5 (64) apart in rel-L2, under both arithmetics.  The step against
    dense_reference / hier_reference, whose head is torch.where(k > 0, ...), at check_grads' 1e-6."""
    S = sharp_case(ref_state, golden, app_vec, arith, N, Nf)
    packed, packedT, app, rows = (S[k] for k in ("packed", "packedT", "app", "rows"))
    for kind, mask in (("dense", S["acc_c"] >= 1), ("hier", (S["acc_c"] >= 1) & (S["acc_f"] >= 1))):
        keep = torch.nonzero(mask)[:, 0].cpu()
        E = keep.numel()
        assert E >= 20, (kind, E)
        r = H._take(S["r"], keep)
        alpha, bg = S["alpha"][keep.cuda()].contiguous(), S["bg"][keep.cuda()].contiguous()
        assert bool(((alpha > 0) & (alpha < 1)).any()) and bool((alpha == 0).any()) and bool((alpha == 1).any())
        if kind == "dense":
            fw = TB.dense_forward(packed, r, N, app, rows)
            st = TB.dense_stage(packed, r, N, app, rows)
            acc = [TB.acc_of(st["c"]["rgb"], st["c"]["sigma"], st["z"])]
        else:
            fw = H.hier_forward(packed, r, N, Nf, app, rows)
            st = H.stage_forward(packed, r, N, Nf, app, rows)
            c, f, idx, T = st["c"], st["f"], st["src"].long() & 0xFFFF, N + Nf
            rgb_all = torch.gather(torch.cat([c["rgb"].view(E, N, 3), f["rgb"].view(E, Nf, 3)], 1), 1,
                                   idx[..., None].expand(E, T, 3)).contiguous()
            sigma_all = torch.gather(torch.cat([c["sigma"].view(E, N), f["sigma"].view(E, Nf)], 1), 1, idx).contiguous()
            acc = [TB.acc_of(c["rgb"], c["sigma"], st["z"]), TB.acc_of(rgb_all, sigma_all, st["z_all"])]
            assert torch.equal(fw["rgb_c"], st["rgb_c"])
        torch.cuda.synchronize()
        assert torch.equal(fw["rgb_map"], st["rgb_map"])
        assert all(bool((a >= 1).all()) for a in acc), (kind, "the same samples saturate in the smaller launch")
        i_w, i_b = H.NAMES.index("density_head.weight"), H.NAMES.index("density_head.bias")
        for name, (al, b) in options(alpha, bg).items():
            for aw in (0.0, 0.1):
                what = (kind, name, aw)
                if kind == "dense":
                    gs, dapp, loss, final = TB.dense_backward(packed, packedT, fw, N, app, rows, (al, b, aw))
                    gs_ref, dapp_ref, loss_ref, final_ref = TB.dense_reference(packed, packedT, st, N, app, rows, al, b, aw)
                else:
                    gs, dapp, loss, final, _ = TB.hier_backward_bg(packed, packedT, fw, N, Nf, 1.0, app, rows, al, b, aw)
                    gs_ref, dapp_ref, loss_ref, final_ref, _ = TB.hier_reference(packed, packedT, st, N, Nf, 1.0, app, rows,
                                                                                  al, b, aw)
                torch.cuda.synchronize()
                print(f"saturated {kind} {arith} ({N},{Nf}) {name} aw={aw}: {E} rays, |d density_head.weight| "
                      f"{float(gs_ref[i_w].norm()):.3g}, d density_head.bias {float(gs_ref[i_b]):.3g}, rel-L2 step vs "
                      f"composition {H.rel_l2(gs[i_w].cpu().numpy(), gs_ref[i_w].cpu().numpy()):.3g}")
                assert float(gs_ref[i_w].norm()) > 0, what
                TB.check_grads(gs, dapp, gs_ref, dapp_ref, rows, 1e-6, what)
                assert torch.isfinite(dapp).all() and torch.isfinite(loss).all(), what
                close_parts(loss, loss_ref, what)
                # k == 0: the blended colour is the composite's own
                assert torch.equal(final.view(torch.int32), final_ref.view(torch.int32)) and torch.equal(final, fw["rgb_map"]), what


# -------------------------------------- 5. the MLP backward and weight gradients behind such a scene
def test_gradients_behind_a_sharp_scene_vs_float64(ref_state, golden, app_vec, arith):
    """test_gpu_accuracy.test_gradients_vs_float64 (its kink-proof own-mask references, its flip bound and
    its per-tensor bound 2 e_cpu + 1e-6) with the sharp model, the 256 x 32 coarse sample points of the
    sharp scene and, as the upstream, the (drgb, dsigma) nerf_composite_backward_grad_acc gives on those
    rows for the background loss (alpha with exact 0 and 1, one colour per ray, acc_weight 0.1).

    That upstream is sparse where the data-gradient kernel reads it: drgb = w g is exactly 0 on every
    sample without weight, and d sigma reaches the trunk as d sigma [sigma > 0] (the density ReLU),
    exactly 0 on every empty sample.  d sigma itself is NOT mostly zero: on an empty ray it is
    (g . rgb_s + g_acc) dist_s, the gradient of adding density there; it is zero only on the empty rays whose
    alpha is exactly 0 (no error, no gradient) and far behind a wall.  So "at least 30 % of the upstream's
    d sigma rows are exactly zero" is false of the rows as produced (9.8 %) and true of the gated ones
    (97.9 %): both figures are printed, the 30 % is asserted on the gated rows, the all-zero 32-row block on
    the raw ones."""
    import nerfmi
    N, Nf = SHARP[0]
    S = sharp_case(ref_state, golden, app_vec, arith, N, Nf)
    stg, r, B = S["st"], S["r"], S["B"]
    c = stg["c"]
    g_rgb, g_acc, _, _, _ = TB.torch_head(stg["rgb_c"], S["acc_c"], stg["x"]["target"], S["alpha"], S["bg"], 0.1, 1.0)
    ds, dr = backward_acc(stg["z"], c["sigma"].view(B, N), c["rgb"].view(B, N, 3), g_rgb, None, g_acc, NAN)
    assert torch.isfinite(ds).all() and torch.isfinite(dr).all()
    M = B * N
    g_sig, g_col = ds.reshape(M, 1).cpu(), dr.reshape(M, 3).cpu()
    z, dn = stg["z"].cpu(), stg["dn"].cpu()
    x = (r["o"][:, None, :] + dn[:, None, :] * z[..., None]).reshape(M, 3).contiguous()
    d = dn[:, None, :].expand(B, N, 3).reshape(M, 3).contiguous()
    st, app = D.sharp_state(ref_state), app_vec
    model = nerfmi.NeRF(nerfmi.Config())
    model.load_state_dict(st)
    model = model.cuda()
    rgb, sigma = model(x.cuda(), d.cuda(), app.cuda())
    ((rgb * g_col.cuda()).sum() + (sigma * g_sig.cuda()).sum()).backward()
    with torch.no_grad():
        m_gpu = A.gpu_relu_masks(model, x.cuda(), d.cuda(), app)
    # the upstream really is the sparse one
    live = sigma.detach().cpu().reshape(M, 1) > 0
    raw0, gated0 = float((g_sig == 0).float().mean()), float(((g_sig * live) == 0).float().mean())
    zero_row = (g_sig[:, 0] == 0) & (g_col == 0).all(-1)
    blocks0 = int(zero_row.reshape(M // 32, 32).all(-1).sum())
    print(f"sharp upstream {arith}: d sigma rows exactly 0: {raw0:.3f} raw, {gated0:.3f} behind the density ReLU; drgb rows "
          f"exactly 0: {float((g_col == 0).all(-1).float().mean()):.3f}; {blocks0} of {M // 32} 32-row blocks all zero; "
          f"largest |d sigma| {float(g_sig.abs().max()):.3g}")
    assert gated0 >= 0.3 and blocks0 >= 1
    assert 0.3 < float((~live).float().mean()) < 0.995 and float(g_sig.abs().max()) > 0

    def ref_grads(dtype, masks=None, record=None, pres=None):
        sd = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in st.items()}   # fresh leaves

        def relu(pre, i):
            if record is not None:
                record.append(pre.detach() > 0)
            if pres is not None:
                pres.append(pre.detach())
            return torch.relu(pre) if masks is None else pre * masks[i].to(dtype)
        with torch.enable_grad():
            r_, s_ = O.nerf_forward(sd, x.to(dtype), d.to(dtype), app.to(dtype), relu=relu)
            ((r_ * g_col.to(dtype)).sum() + (s_ * g_sig.to(dtype)).sum()).backward()
        return {k: v.grad.double() for k, v in sd.items()}

    m_cpu, pre64 = [], []
    g32 = ref_grads(torch.float32, record=m_cpu)
    g64_cpu, g64_gpu = ref_grads(torch.float64, masks=m_cpu, pres=pre64), ref_grads(torch.float64, masks=m_gpu)
    flips = sum(int((a != b).sum()) for a, b in zip(m_cpu, m_gpu))
    near = sum(int((p.abs() <= 1e-4 * p.pow(2).mean().sqrt()).sum()) for p in pre64)
    assert flips <= 4 * near + 8, (arith, "ReLU branches differ between the GPU and the CPU", flips, near)

    def rel(a, b):
        return float((a - b).norm() / (b.norm() + 1e-300))

    worst, failures = [], []
    for k, p in model.named_parameters():
        assert torch.isfinite(p.grad).all(), k
        e_gpu, e_cpu = rel(p.grad.cpu().double(), g64_gpu[k]), rel(g32[k], g64_cpu[k])
        bound = 2.0 * e_cpu + 1e-6
        worst.append((e_gpu / bound, k, e_gpu, e_cpu))
        if e_gpu > bound:
            failures.append((k, e_gpu, e_cpu, bound))
    worst.sort(reverse=True)
    print(f"sharp/{arith}: {flips} ReLU branches differ between the GPU and the CPU ({near} float64 pre-activations "
          f"within 1e-4 rms of a kink); worst gradient tensors "
          f"(ratio to the bound, key, gpu rel-L2, cpu rel-L2): {worst[:3]}")
    assert not failures, (arith, failures)
