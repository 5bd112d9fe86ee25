"""The distortion loss as a stage on the GPU (include/nerfmi_train.h "distortion"):
nerf_distortion (csrc/distortion.hip) against the float64 O(T^2) definition of tests/distortion_cases.py,
and the per-sample upstream gradient of the composite backward (the _w kernels of csrc/composite_bwd.hip).

Bound of the stage, per output against float64: 2^-23 |ref| + T 2^-48 S with S = scale inv max z sum w of
the ray: one float rounding (2^-24) with a margin of 2, plus the double sums' cancellation.  Inputs: the
fp32 weights of degenerate_cases.ray_profiles(67, T) (walls, shells, empty rays, fog, tied z), sorted rays
only, at T on both sides of the 64-sample chunk boundary, tails, and long rays at (3, 1280), (2, 4096).
"""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests"))
import degenerate_cases as D    # noqa: E402
import distortion_cases as DC   # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
NEAR, FAR = 2.0, 6.0
STAGE = [(67, 2), (67, 5), (67, 64), (67, 65), (67, 100), (67, 259), (3, 1280), (2, 4096)]
SHAPES = [(37, 8), (5, 32), (3, 256), (6, 7)]
MERGED = [(37, 8, 16), (3, 256, 1024), (5, 7, 10)]


def _L():
    from nerfmi import _lib
    return _lib


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc):
    assert rc == 0, _L().load().nerf_last_error()


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def distortion(w, z, scale=1.0, want_loss=True, want_grad=True, near=NEAR, far=FAR):
    """nerf_distortion on device tensors: (loss_rays or None, g_w or None), outputs pre-filled with NaN."""
    B, T = w.shape
    loss = torch.full((B,), NAN, device="cuda") if want_loss else None
    g = torch.full((B, T), NAN, device="cuda") if want_grad else None
    ok(_L().load().nerf_distortion(P(w), P(z), B, T, near, far, scale, P(loss), P(g), S()))
    torch.cuda.synchronize()
    return loss, g


def stage_case(B, T):
    """Sorted rays of the profiles; the long shapes take the fog, tied-z and shell rays of an 8-ray batch
    (weight on every sample, on a run of equal z, and in one lump)."""
    if B == 67:
        w, z, keep = DC.profile_weights(67, T)
        assert int(keep.sum()) == 66
        return w[keep].contiguous(), z[keep].contiguous()
    w, z, _ = DC.profile_weights(8, T)
    rows = [5, 7, 3][:B]
    return w[rows].contiguous(), z[rows].contiguous()


@pytest.mark.parametrize("B,T", STAGE)
def test_stage_matches_the_definition(B, T):
    w, z = stage_case(B, T)
    l_ref, g_ref = DC.definition(w, z, NEAR, FAR)
    for scale in (1.0, 0.37 / 4096):
        loss, g = distortion(w.cuda(), z.cuda(), scale)
        b_l = DC.bound(l_ref, T, DC.ray_scale(w, z, NEAR, FAR))
        b_g = DC.bound(scale * g_ref, T, DC.ray_scale(w, z, NEAR, FAR, scale))
        e_l, e_g = (loss.double().cpu() - l_ref).abs(), (g.double().cpu() - scale * g_ref).abs()
        tiny = torch.finfo(torch.float64).tiny
        print(f"({B},{T}) scale {scale:.3g}: worst ratio to the bound  l {float((e_l / b_l.clamp_min(tiny)).max()):.3f}"
              f"  g_w {float((e_g / b_g.clamp_min(tiny)).max()):.3f}")
        assert bool((e_l <= b_l).all()), (scale, float((e_l / b_l.clamp_min(tiny)).max()))
        assert bool((e_g <= b_g).all()), (scale, float((e_g / b_g.clamp_min(tiny)).max()))
    # the empty rays (profile 0) are among them: exact zeros
    empty = ~w.bool().any(-1)
    assert bool(empty.any()) or B < 67
    assert not bool(loss.cpu()[empty].any()) and not bool(g.cpu()[empty].any())


def test_zero_weights_and_one_sample():
    z = torch.sort(torch.rand(7, 130) * 4 + 2, dim=-1).values.cuda()
    loss, g = distortion(torch.zeros(7, 130, device="cuda"), z)          # 7 rays: a partly filled block
    assert not bool(loss.any()) and not bool(g.any())
    loss, g = distortion(torch.rand(7, 1).cuda(), z[:, :1].contiguous())
    assert not bool(loss.any()) and not bool(g.any())                     # T = 1: l = 0, no gradient


@pytest.mark.parametrize("T", [2, 65, 259])
def test_descending_rays_stay_finite(T):
    w, z, keep = DC.profile_weights(67, T)
    w, z = w[~keep].contiguous(), z[~keep].contiguous()                   # the profile-9 rays
    assert w.shape[0] >= 1 and bool(torch.isfinite(w).all())
    loss, g = distortion(w.cuda(), z.cuda())
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(g).all())


@pytest.mark.parametrize("B,T", [(67, 65), (3, 1280)])
def test_deterministic_and_loss_alone(B, T):
    w, z = (t.cuda() for t in stage_case(B, T))
    l1, g1 = distortion(w, z, 0.25)
    l2, g2 = distortion(w, z, 0.25)
    assert same_bits(l1, l2) and same_bits(g1, g2)
    l3, none = distortion(w, z, 0.25, want_grad=False)
    assert none is None and same_bits(l3, l1)
    none, g3 = distortion(w, z, 0.25, want_loss=False)
    assert none is None and same_bits(g3, g1)


def test_python_stage():
    import nerfmi
    w, z = stage_case(67, 100)
    l_ref, g_ref = DC.definition(w, z, NEAR, FAR)
    loss = nerfmi.distortion_loss(w[..., None], z, NEAR, FAR)             # the (B,T,1) extras['weights'] shape
    l2, g = nerfmi.distortion_loss(w.cuda(), z.cuda(), NEAR, FAR, return_grad=True)
    assert loss.is_cuda and loss.shape == (66,) and g.shape == (66, 100) and same_bits(loss, l2)
    assert not loss.requires_grad and not g.requires_grad
    S_ = DC.ray_scale(w, z, NEAR, FAR)
    assert bool(((loss.double().cpu() - l_ref).abs() <= DC.bound(l_ref, 100, S_)).all())
    assert bool(((g.double().cpu() - g_ref).abs() <= DC.bound(g_ref, 100, S_)).all())


# ------------------------------------------------------------------- the _w composite backward
def stage_inputs(B, N, seed=0):
    """tests/test_gpu_background.py's: degenerate profiles, then random sigma."""
    g = torch.Generator().manual_seed(1000 * N + B + seed)
    z, sigma, rgb = D.ray_profiles(B, N, g)
    half = (B + 1) // 2
    sigma[half:] = F.relu(torch.randn(B - half, N, generator=g)) * 0.5
    z[half:] = torch.sort(torch.rand(B - half, N, generator=g) * 4 + 2, dim=-1).values
    return z.contiguous(), sigma.contiguous(), rgb.contiguous()


def backward_w(z, sigma, rgb, g_rgb, g_depth, g_acc, bd, g_w, entry="w"):
    lib = _L().load()
    B, N = z.shape
    ds, dr = torch.full((B, N), NAN, device="cuda"), torch.full((B, N, 3), NAN, device="cuda")
    head = (P(rgb), P(sigma), P(z), P(g_rgb), P(g_depth), B, N, P(ds), P(dr), P(g_acc), bd)
    if entry == "w":
        ok(lib.nerf_composite_backward_grad_w(*head, P(g_w), S()))
    else:
        ok(lib.nerf_composite_backward_grad_acc(*head, S()))
    torch.cuda.synchronize()
    return ds, dr


@pytest.mark.parametrize("B,N", SHAPES)
def test_w_backward_without_g_w_is_the_acc_kernel(B, N):
    z, sigma, rgb = (t.cuda() for t in stage_inputs(B, N, seed=1))
    g = torch.Generator().manual_seed(7 + N)
    g_rgb, g_depth = torch.randn(B, 3, generator=g).cuda(), torch.randn(B, generator=g).cuda() * 1e-3
    g_acc = torch.randn(B, generator=g).cuda()
    for bd in (NAN, 6.0):
        for ga in (None, g_acc):
            ref = backward_w(z, sigma, rgb, g_rgb, g_depth, ga, bd, None, entry="acc")
            for gw in (None, torch.zeros(B, N, device="cuda")):       # null: the _acc launch; zeros: the _w kernel
                got = backward_w(z, sigma, rgb, g_rgb, g_depth, ga, bd, gw)
                assert same_bits(got[0], ref[0]) and same_bits(got[1], ref[1]), (bd, ga is None, gw is None)


@pytest.mark.parametrize("B,N", SHAPES)
def test_constant_g_w_is_g_acc(B, N):
    """g_acc null and g_w[r, :] = c_r: the bits of g_acc = c_r with g_w null (both are one double add to dw)."""
    z, sigma, rgb = (t.cuda() for t in stage_inputs(B, N, seed=2))
    g = torch.Generator().manual_seed(11 + N)
    g_rgb, g_depth = torch.randn(B, 3, generator=g).cuda(), torch.randn(B, generator=g).cuda() * 1e-3
    c = torch.randn(B, generator=g).cuda()
    for bd in (NAN, 6.0):
        ref = backward_w(z, sigma, rgb, g_rgb, g_depth, c, bd, None)
        got = backward_w(z, sigma, rgb, g_rgb, g_depth, None, bd, c[:, None].expand(B, N).contiguous())
        assert same_bits(got[0], ref[0]) and same_bits(got[1], ref[1]), bd
        assert not same_bits(ref[0], backward_w(z, sigma, rgb, g_rgb, g_depth, None, bd, None)[0])


def restated(rgb, sigma, z, bd, dtype):
    """render.py:56-80 in `dtype` with autograd: (rgb_map, depth, acc, weights)."""
    zz = z.to(dtype)
    dists = torch.cat([zz[..., 1:] - zz[..., :-1], torch.full_like(zz[..., :1], 1e-3)], -1)
    alpha = 1.0 - torch.exp(-sigma * dists)
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10], 1), 1)[:, :-1]
    w = alpha * trans
    acc = w.sum(-1)
    swz = (w * zz).sum(-1)
    depth = swz / (acc + 1e-10) if bd != bd else swz + torch.clamp(1.0 - acc, min=0.0) * bd
    return (w[..., None] * rgb).sum(1), depth, acc, w


def rel_l2(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("bd", [NAN, 6.0])
def test_w_backward_matches_float64_autograd(B, N, bd):
    """d(sigma, rgb) for random upstream gradients of the colour, the depth, the opacity and every weight:
    the GPU is within 2x the float32 torch-CPU restatement's distance from float64, + 1e-6 (DESIGN.md §15's
    rule)."""
    R = max(B, 8)
    g = torch.Generator().manual_seed(31 * N + B)
    z = torch.sort(torch.rand(R, N, generator=g) * 4 + 2, dim=-1).values
    sigma, rgb = F.relu(torch.randn(R, N, generator=g)) * 0.5, torch.rand(R, N, 3, generator=g)
    g_rgb, g_depth, g_acc = torch.randn(R, 3, generator=g), torch.randn(R, generator=g), torch.randn(R, generator=g)
    g_w = torch.randn(R, N, generator=g)
    outs = {}
    for dt in (torch.float32, torch.float64):
        s_, c_ = sigma.to(dt).clone().requires_grad_(True), rgb.to(dt).clone().requires_grad_(True)
        colour, depth, acc, w = restated(c_, s_, z, bd, dt)
        if dt == torch.float64:
            assert bool(((1.0 - acc).abs() >= 1e-3).all()), "inputs must keep acc away from the kink"
        ((colour * g_rgb.to(dt)).sum() + (depth * g_depth.to(dt)).sum() + (acc * g_acc.to(dt)).sum() +
         (w * g_w.to(dt)).sum()).backward()
        outs[dt] = (s_.grad, c_.grad)
    ds, dr = backward_w(z.cuda(), sigma.cuda(), rgb.cuda(), g_rgb.cuda(), g_depth.cuda(), g_acc.cuda(), bd, g_w.cuda())
    for got, i, name in ((ds, 0, "dsigma"), (dr, 1, "drgb")):
        e_gpu, e_cpu = rel_l2(got, outs[torch.float64][i]), rel_l2(outs[torch.float32][i], outs[torch.float64][i])
        print(f"({B},{N}) bd={bd} {name}: rel-L2 vs float64  gpu {e_gpu:.3g}  cpu fp32 {e_cpu:.3g}")
        assert e_gpu <= 2 * e_cpu + 1e-6, (name, e_gpu, e_cpu)


@pytest.mark.parametrize("B,N,Nf", MERGED)
def test_merged_backward_w(B, N, Nf):
    """nerf_composite_merged_backward_w: with g_w null the merged _acc entry's bits (accumulate mode
    included); with g_w on (merged order), the dense _w kernel's bits on the rows gathered through
    merged_src."""
    from nerfmi.ray_utils import linspace_table
    lib = _L().load()
    T = N + Nf
    g = torch.Generator().manual_seed(1000 * N + Nf)
    rgb_c, rgb_f = torch.rand(B, N, 3, generator=g).cuda(), torch.rand(B, Nf, 3, generator=g).cuda()
    sig_c = (F.relu(torch.randn(B, N, generator=g)) * 0.5).cuda()
    sig_f = (F.relu(torch.randn(B, Nf, generator=g)) * 0.5).cuda()
    z = torch.sort(2 + 4 * torch.rand(B, N, generator=g), dim=-1).values.cuda()
    w, u = torch.rand(B, N, generator=g).cuda(), torch.rand(B, Nf, generator=g).cuda()
    g_map, g_depth = torch.randn(B, 3, generator=g).cuda(), torch.randn(B, generator=g).cuda()
    g_acc, g_w = torch.randn(B, generator=g).cuda(), torch.randn(B, T, generator=g).cuda()
    pre_s, pre_r = torch.randn(B, N, generator=g).cuda(), torch.randn(B, N, 3, generator=g).cuda()
    u_lin = linspace_table(Nf, z.device, drop_last=True)
    z_all, z_fine = torch.empty(B, T, device="cuda"), torch.empty(B, Nf, device="cuda")
    src = torch.empty(B, T, dtype=torch.int16, device="cuda")
    ok(lib.nerf_sample_importance_src(P(z), P(w), B, N, Nf, P(u_lin), P(u), 0, P(z_all), P(z_fine), P(src), S()))
    idx = src.long() & 0xFFFF

    def merged(entry_w, accumulate, ga, bd, gw):
        ds_c = pre_s.clone() if accumulate else torch.full((B, N), NAN, device="cuda")
        dr_c = pre_r.clone() if accumulate else torch.full((B, N, 3), NAN, device="cuda")
        ds_f, dr_f = torch.full((B, Nf), NAN, device="cuda"), torch.full((B, Nf, 3), NAN, device="cuda")
        args = [P(rgb_c), P(sig_c), P(rgb_f), P(sig_f), P(src), P(z_all), P(g_map), P(g_depth), B, N, Nf, accumulate,
                P(ds_c), P(dr_c), P(ds_f), P(dr_f), P(ga), bd]
        if entry_w:
            ok(lib.nerf_composite_merged_backward_w(*args, P(gw), S()))
        else:
            ok(lib.nerf_composite_merged_backward_acc(*args, S()))
        torch.cuda.synchronize()
        return ds_c, dr_c, ds_f, dr_f

    for accumulate in (0, 1):
        ref = merged(False, accumulate, g_acc, 5.5, None)
        for gw in (None, torch.zeros(B, T, device="cuda")):
            for a, b in zip(merged(True, accumulate, g_acc, 5.5, gw), ref):
                assert same_bits(a, b), accumulate
    # g_w on: the dense _w kernel on the gathered rows, scattered back
    rgb_m = torch.gather(torch.cat([rgb_c, rgb_f], 1), 1, idx[..., None].expand(B, T, 3)).contiguous()
    sig_m = torch.gather(torch.cat([sig_c, sig_f], 1), 1, idx).contiguous()
    for bd in (NAN, 5.5):
        ds_m, dr_m = backward_w(z_all, sig_m, rgb_m, g_map, g_depth, g_acc, bd, g_w)
        ref_ds = torch.empty_like(ds_m).scatter_(1, idx, ds_m)
        ref_dr = torch.empty_like(dr_m).scatter_(1, idx[..., None].expand(B, T, 3), dr_m)
        ds_c, dr_c, ds_f, dr_f = merged(True, 0, g_acc, bd, g_w)
        assert torch.equal(torch.cat([ds_c, ds_f], 1), ref_ds) and torch.equal(torch.cat([dr_c, dr_f], 1), ref_dr)
        assert not torch.equal(merged(True, 0, g_acc, bd, None)[0], ds_c)      # g_w reaches the coarse rows
