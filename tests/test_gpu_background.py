"""The opacity map and the background blend on the GPU (include/nerfmi.h "opacity map and background",
DESIGN.md §15): the composite stage forward and backward, the render entry points, volume_render.

Definitions under test, per ray: acc = (float) sum w (the composite's own double sum, rounded once),
k = max(0, 1 - acc), colour = rgb_map + k bg (product rounded, then the sum), and with a background depth
bd, depth = (float) sum w z + k bd.  The exact statements (options off, bg = 0, empty and opaque-first
rays, the blend itself) are asserted bit for bit; the float64 comparisons hold the composite to
tests/test_gpu_parity.py's bound, 1e-4 |ref| + 1e-6, on rays that keep acc 1e-3 away from the kink of k.

Inputs of the stage tests: the rays of tests/degenerate_cases.py (opaque, empty, tied z) in the first
half of a batch, ray 1 made opaque at its first sample, and random sigma in the second half.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests"))
import degenerate_cases as D   # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-6         # tests/test_gpu_parity.py's bound on the composite
NAN = float("nan")
SHAPES = [(37, 8), (5, 32), (3, 256), (6, 7)]            # (6, 7): the scalar-load kernel (N % 4 != 0)
MERGED = [(37, 8, 16), (3, 256, 1024), (5, 7, 10)]       # staged, unstaged (T > 256), staged scalar-load


def _L():
    from nerfmi import _lib
    return _lib


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc):
    assert rc == 0, _L().load().nerf_last_error()


def close(gpu, ref, what):
    gpu, ref = gpu.detach().double().cpu(), ref.detach().double().cpu()
    err = (gpu - ref).abs()
    bad = err > ATOL + RTOL * ref.abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} outside tol; max abs err {float(err.max()):.3g}"


def stage_inputs(B, N, seed=0):
    """z (B,N), sigma (B,N), rgb (B,N,3) on the CPU: degenerate profiles, then random sigma; ray 0 is
    empty (profile 0) and ray 1 opaque at its first sample."""
    g = torch.Generator().manual_seed(1000 * N + B + seed)
    z, sigma, rgb = D.ray_profiles(B, N, g)
    half = (B + 1) // 2
    sigma[half:] = F.relu(torch.randn(B - half, N, generator=g)) * 0.5
    z[half:] = torch.sort(torch.rand(B - half, N, generator=g) * 4 + 2, dim=-1).values
    z[1] = torch.linspace(2.0, 6.0, N)
    sigma[1] = 0.0
    sigma[1, 0] = 3e38
    assert not bool(sigma[0].any())
    return z.contiguous(), sigma.contiguous(), rgb.contiguous()


def composite(z, sigma, rgb, bg=None, bd=NAN, want_acc=True, plain=False):
    """nerf_composite (plain) or nerf_composite_bg on device tensors: (rgb_map, depth, weights, acc)."""
    lib = _L().load()
    B, N = z.shape
    rm, dm = torch.full((B, 3), NAN, device="cuda"), torch.full((B,), NAN, device="cuda")
    wm = torch.full((B, N), NAN, device="cuda")
    acc = torch.full((B,), NAN, device="cuda") if want_acc else None
    if plain:
        ok(lib.nerf_composite(P(rgb), P(sigma), P(z), B, N, P(rm), P(dm), P(wm), S()))
    else:
        rows = 0 if bg is None else bg.shape[0]
        ok(lib.nerf_composite_bg(P(rgb), P(sigma), P(z), B, N, P(rm), P(dm), P(wm), P(bg), rows, bd, P(acc), S()))
    torch.cuda.synchronize()
    return rm, dm, wm, acc


def oracle64(z, sigma, rgb):
    """The float64 restatement of render.py:56-80 at the kernels' fp32 alpha (degenerate_cases):
    (rgb_map, sum w z, acc) in float64."""
    rm, _, w = D.composite_f64_st(rgb.double(), sigma.double()[..., None], z, exp32=D.exp_rn)
    w = w[..., 0]
    return rm, (w * z.double()).sum(-1), w.sum(-1)


# ------------------------------------------------------------------------------- forward stage
@pytest.mark.parametrize("B,N", SHAPES)
def test_composite_bg_forward_stage(B, N):
    z, sigma, rgb = stage_inputs(B, N)
    zc, sc, rc = z.cuda(), sigma.cuda(), rgb.cuda()
    g = torch.Generator().manual_seed(N)
    bg_b = torch.rand(B, 3, generator=g).cuda()
    bg_1 = torch.tensor([[0.25, 0.5, 1.0]], device="cuda")
    bd = 6.0
    p_rgb, p_depth, p_w, _ = composite(zc, sc, rc, plain=True)
    # options off but the opacity output: every other output is nerf_composite's
    o_rgb, o_depth, o_w, acc = composite(zc, sc, rc)
    assert torch.equal(o_rgb, p_rgb) and torch.equal(o_depth, p_depth) and torch.equal(o_w, p_w)
    # ... and with everything off (the plain launch)
    q_rgb, q_depth, q_w, _ = composite(zc, sc, rc, want_acc=False)
    assert torch.equal(q_rgb, p_rgb) and torch.equal(q_depth, p_depth) and torch.equal(q_w, p_w)
    # acc against the stored weights: each <= 1 and rounded once, plus the final rounding
    assert float(o_w.max()) <= 1.0
    assert bool(((acc.double() - o_w.double().sum(-1)).abs() <= N * 2.0 ** -24).all())
    assert float(acc[0]) == 0.0 and float(acc[1]) == 1.0          # the empty ray, the opaque-first ray
    for bg in (bg_1, bg_b):
        z_rgb, _, z_w, z_acc = composite(zc, sc, rc, bg=torch.zeros_like(bg))
        assert torch.equal(z_rgb, p_rgb) and torch.equal(z_w, p_w) and torch.equal(z_acc, acc)    # bg = 0
        b_rgb, b_depth, b_w, b_acc = composite(zc, sc, rc, bg=bg, bd=bd)
        assert torch.equal(b_w, p_w) and torch.equal(b_acc, acc)
        # the blend, operation for operation: the product rounded, then the sum
        k = torch.clamp(1.0 - acc, min=0.0)
        assert torch.equal(b_rgb, p_rgb + k[:, None] * bg.expand(B, 3))
        empty = acc == 0
        assert bool(empty[0]) and torch.equal(b_rgb[empty], bg.expand(B, 3)[empty])               # colour == bg
        assert bool((b_depth[empty] == bd).all())                                                 # depth == bd
        opaque = acc >= 1
        assert bool(opaque[1]) and torch.equal(b_rgb[opaque], p_rgb[opaque])
        # float64, away from the kink of k
        r64, s64, a64 = oracle64(z, sigma, rgb)
        keep = (1.0 - a64).abs() >= 1e-3
        assert int(keep.sum()) >= max(2, B // 3), int(keep.sum())
        k64 = torch.clamp(1.0 - a64, min=0.0)
        close(b_rgb.cpu()[keep], (r64 + k64[:, None] * bg.expand(B, 3).double().cpu())[keep], f"colour ({B},{N})")
        close(b_depth.cpu()[keep], (s64 + k64 * bd)[keep], f"depth ({B},{N})")
        close(acc.cpu()[keep], a64[keep], f"acc ({B},{N})")


def test_composite_bg_argument_errors():
    lib = _L().load()
    t = torch.zeros(16, device="cuda")
    for rows in (2, -1, 5):
        assert lib.nerf_composite_bg(P(t), P(t), P(t), 4, 1, P(t), P(t), None, P(t), rows, NAN, None, S()) == 1
        assert b"bg_rows" in lib.nerf_last_error()
    assert lib.nerf_composite_bg(P(t), P(t), P(t), 4, 1, P(t), P(t), None, None, 1, NAN, None, S()) == 1
    assert b"null bg" in lib.nerf_last_error()
    assert lib.nerf_composite_bg(None, None, None, 0, 4, None, None, None, None, 0, NAN, None, S()) == 0


# ------------------------------------------------------------------------------ backward stage
def restated(rgb, sigma, z, bg, bd, dtype):
    """render.py:56-80 + the definitions in `dtype` with autograd: (colour, depth, acc)."""
    rgb, sigma = rgb.to(dtype), sigma.to(dtype)
    zz = z.to(dtype)
    dists = torch.cat([zz[..., 1:] - zz[..., :-1], torch.full_like(zz[..., :1], 1e-3)], -1)
    alpha = 1.0 - torch.exp(-sigma * dists)
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10], 1), 1)[:, :-1]
    w = alpha * trans
    acc = w.sum(-1)
    k = torch.clamp(1.0 - acc, min=0.0)
    colour = (w[..., None] * rgb).sum(1) + (k[:, None] * bg.to(dtype) if bg is not None else 0.0)
    swz = (w * zz).sum(-1)
    depth = swz / (acc + 1e-10) if bd != bd else swz + k * bd
    return colour, depth, acc


def rel_l2(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def smooth_inputs(B, N, seed):
    """Random rays with acc well below 1 (the kink of k) and sorted z."""
    g = torch.Generator().manual_seed(seed)
    z = torch.sort(torch.rand(B, N, generator=g) * 4 + 2, dim=-1).values
    sigma = F.relu(torch.randn(B, N, generator=g)) * 0.5
    rgb = torch.rand(B, N, 3, generator=g)
    grads = torch.randn(B, 3, generator=g), torch.randn(B, generator=g), torch.randn(B, generator=g)
    return z, sigma, rgb, grads, torch.rand(B, 3, generator=g)


def backward_acc(z, sigma, rgb, g_rgb, g_depth, g_acc, bd):
    lib = _L().load()
    B, N = z.shape
    ds, dr = torch.full((B, N), NAN, device="cuda"), torch.full((B, N, 3), NAN, device="cuda")
    ok(lib.nerf_composite_backward_grad_acc(P(rgb), P(sigma), P(z), P(g_rgb), P(g_depth), B, N, P(ds), P(dr), P(g_acc),
                                            bd, S()))
    torch.cuda.synchronize()
    return ds, dr


@pytest.mark.parametrize("B,N", SHAPES)
def test_backward_with_g_acc_off_is_the_existing_kernel(B, N):
    lib = _L().load()
    z, sigma, rgb = (t.cuda() for t in stage_inputs(B, N, seed=1))
    g = torch.Generator().manual_seed(7 + N)
    g_rgb, g_depth = torch.randn(B, 3, generator=g).cuda(), torch.randn(B, generator=g).cuda() * 1e-3
    for gd in (None, g_depth):
        ds0, dr0 = torch.full((B, N), NAN, device="cuda"), torch.full((B, N, 3), NAN, device="cuda")
        ok(lib.nerf_composite_backward_grad(P(rgb), P(sigma), P(z), P(g_rgb), P(gd), B, N, P(ds0), P(dr0), S()))
        torch.cuda.synchronize()
        for ga in (None, torch.zeros(B, device="cuda")):
            ds, dr = backward_acc(z, sigma, rgb, g_rgb, gd, ga, NAN)
            assert torch.equal(ds.view(torch.int32), ds0.view(torch.int32)), (gd is None, ga is None)
            assert torch.equal(dr.view(torch.int32), dr0.view(torch.int32))


@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("bd", [NAN, 6.0])
def test_backward_with_g_acc_matches_float64_autograd(B, N, bd):
    """d(sigma, rgb) for random upstream gradients of the colour, the depth and the opacity, on rays away
    from the kink of k: the GPU is within 2x the float32 torch-CPU restatement's distance from float64,
    + 1e-6 (DESIGN.md §14's rule)."""
    R = max(B, 8)
    z, sigma, rgb, (g_rgb, g_depth, g_acc), bg = smooth_inputs(R, N, seed=31 * N + B)
    outs = {}
    for dt in (torch.float32, torch.float64):
        s_, c_ = sigma.to(dt).clone().requires_grad_(True), rgb.to(dt).clone().requires_grad_(True)
        colour, depth, acc = restated(c_, s_, z, bg, bd, dt)
        if dt == torch.float64:
            assert bool(((1.0 - acc).abs() >= 1e-3).all()), "inputs must keep acc away from the kink"
        ((colour * g_rgb.to(dt)).sum() + (depth * g_depth.to(dt)).sum() + (acc * g_acc.to(dt)).sum()).backward()
        outs[dt] = (s_.grad, c_.grad)
    # the blend's own path to acc, as the caller of the stage entry forms it: -(bg . g_rgb) where k > 0
    ga = (g_acc - (bg * g_rgb).sum(-1)).cuda().contiguous()
    ds, dr = backward_acc(z.cuda(), sigma.cuda(), rgb.cuda(), g_rgb.cuda(), g_depth.cuda(), ga, bd)
    for got, i, name in ((ds, 0, "dsigma"), (dr, 1, "drgb")):
        e_gpu, e_cpu = rel_l2(got, outs[torch.float64][i]), rel_l2(outs[torch.float32][i], outs[torch.float64][i])
        print(f"({B},{N}) bd={bd} {name}: rel-L2 vs float64  gpu {e_gpu:.3g}  cpu fp32 {e_cpu:.3g}")
        assert e_gpu <= 2 * e_cpu + 1e-6, (name, e_gpu, e_cpu)


@pytest.mark.parametrize("B,N,Nf", MERGED)
def test_merged_backward_acc(B, N, Nf):
    """nerf_composite_merged_backward_acc: with g_acc off the existing merged kernel's bits (accumulate mode
    included); with g_acc and bd on, the dense _acc kernel's bits on the rows gathered through merged_src."""
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
    g_acc = torch.randn(B, generator=g).cuda()
    pre_s, pre_r = torch.randn(B, N, generator=g).cuda(), torch.randn(B, N, 3, generator=g).cuda()
    u_lin = linspace_table(Nf, z.device, drop_last=True)
    z_all, z_fine = torch.empty(B, T, device="cuda"), torch.empty(B, Nf, device="cuda")
    src = torch.empty(B, T, dtype=torch.int16, device="cuda")
    ok(lib.nerf_sample_importance_src(P(z), P(w), B, N, Nf, P(u_lin), P(u), 0, P(z_all), P(z_fine), P(src), S()))
    idx = src.long() & 0xFFFF

    def merged(entry_acc, accumulate, ga, bd):
        ds_c = pre_s.clone() if accumulate else torch.full((B, N), NAN, device="cuda")
        dr_c = pre_r.clone() if accumulate else torch.full((B, N, 3), NAN, device="cuda")
        ds_f, dr_f = torch.full((B, Nf), NAN, device="cuda"), torch.full((B, Nf, 3), NAN, device="cuda")
        args = [P(rgb_c), P(sig_c), P(rgb_f), P(sig_f), P(src), P(z_all), P(g_map), P(g_depth), B, N, Nf, accumulate,
                P(ds_c), P(dr_c), P(ds_f), P(dr_f)]
        if entry_acc:
            ok(lib.nerf_composite_merged_backward_acc(*args, P(ga), bd, S()))
        else:
            ok(lib.nerf_composite_merged_backward(*args, S()))
        torch.cuda.synchronize()
        return ds_c, dr_c, ds_f, dr_f

    for accumulate in (0, 1):
        ref = merged(False, accumulate, None, NAN)
        for ga in (None, torch.zeros(B, device="cuda")):
            for a, b in zip(merged(True, accumulate, ga, NAN), ref):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), accumulate
    # g_acc and bd on: the dense kernel on the gathered rows, scattered back
    rgb_m = torch.gather(torch.cat([rgb_c, rgb_f], 1), 1, idx[..., None].expand(B, T, 3)).contiguous()
    sig_m = torch.gather(torch.cat([sig_c, sig_f], 1), 1, idx).contiguous()
    for bd in (NAN, 5.5):
        ds_m, dr_m = backward_acc(z_all, sig_m, rgb_m, g_map, g_depth, g_acc, bd)
        ref_ds = torch.empty_like(ds_m).scatter_(1, idx, ds_m)
        ref_dr = torch.empty_like(dr_m).scatter_(1, idx[..., None].expand(B, T, 3), dr_m)
        ds_c, dr_c, ds_f, dr_f = merged(True, 0, g_acc, bd)
        assert torch.equal(torch.cat([ds_c, ds_f], 1), ref_ds) and torch.equal(torch.cat([dr_c, dr_f], 1), ref_dr)
        no_acc = merged(True, 0, None, bd)
        assert not torch.equal(no_acc[0], ds_c)                     # g_acc reaches the coarse rows


# ------------------------------------------------------------------------------ render entries
@pytest.fixture(scope="module", params=["f16x3", "f32"])
def arith(request):
    L = _L()
    prev = L.set_mlp_arith(request.param)
    yield request.param
    L.set_mlp_arith(prev)


@pytest.fixture(scope="module")
def model(ref_state):
    import nerfmi
    m = nerfmi.NeRF(nerfmi.Config())
    m.load_state_dict(ref_state)
    return m.cuda().eval().requires_grad_(False)


def render_inputs(B, N, Nf, seed=3):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(B, 3, generator=g) * 0.3
    d = F.normalize(torch.randn(B, 3, generator=g), dim=-1)
    return dict(o=o.cuda(), d=d.cuda(), t_rand=torch.rand(B, N, generator=g).cuda(),
                u_rand=torch.rand(B, max(Nf, 1), generator=g).cuda(), bg=torch.rand(B, 3, generator=g).cuda())


def grid(kind):
    import nerfmi
    if kind is None:
        return None
    G = 8
    m = torch.ones(G, G, G, dtype=torch.bool) if kind == "ones" else torch.zeros(G, G, G, dtype=torch.bool)
    return nerfmi.OccupancyGrid((-8.0,) * 3, (8.0,) * 3, G).from_mask(m)


def render_entry(model, r, N, Nf, occ, bg_args):
    """nerf_render_rays(_occ)(_bg) on the inputs r: bg_args None = the original entry, else (bg, bd,
    want_acc).  Returns a dict of every output."""
    from nerfmi.ray_utils import linspace_table
    from nerfmi.render import packed_for
    L = _L()
    lib = L.load()
    B, T, dev = r["o"].shape[0], N + Nf, r["o"].device
    out = dict(rgb=torch.full((B, 3), NAN, device=dev), depth=torch.full((B,), NAN, device=dev),
               w=torch.full((B, T), NAN, device=dev), z=torch.full((B, T), NAN, device=dev),
               crgb=torch.full((B, 3), NAN, device=dev), cdepth=torch.full((B,), NAN, device=dev))
    args = [P(packed_for(model)), P(r["o"]), P(r["d"]), B, 2.0, 6.0, N, Nf, P(linspace_table(N, dev)),
            P(linspace_table(Nf, dev, drop_last=True)) if Nf else None, 1, P(r["t_rand"]), P(r["u_rand"]) if Nf else None,
            0, 0, None, 0]
    name, sizer = "nerf_render_rays", lib.nerf_render_workspace_bytes
    if occ is not None:
        args += [P(occ.bits), occ.resolution, occ.c_lo(), occ.c_inv()]
        name, sizer = "nerf_render_rays_occ", lib.nerf_render_occ_workspace_bytes
    ws = torch.empty(sizer(B, N, Nf), dtype=torch.uint8, device=dev)
    args += [P(out["rgb"]), P(out["depth"]), P(out["w"]), P(out["z"]), P(out["crgb"]) if Nf else None,
             P(out["cdepth"]) if Nf else None, P(ws), ws.numel()]
    if bg_args is not None:
        bg, bd, want = bg_args
        out["acc"] = torch.full((B,), NAN, device=dev) if want else None
        out["cacc"] = torch.full((B,), NAN, device=dev) if (want and Nf) else None
        args += [P(bg), 0 if bg is None else bg.shape[0], bd, P(out["acc"]), P(out["cacc"])]
        name += "_bg"
    ok(getattr(lib, name)(*args, S()))
    torch.cuda.synchronize()
    return out


RENDER_CASES = [(48, 32, 40, k) for k in (None, "ones", "zeros")] + [(48, 32, 0, k) for k in (None, "zeros")] + \
    [(B, N, Nf, None) for B, N, Nf in MERGED]


@pytest.mark.parametrize("B,N,Nf,occ_kind", RENDER_CASES)
def test_render_entries(arith, model, B, N, Nf, occ_kind):
    """(48, 32, 40) plain, with an all-ones and with an all-zero grid; the coarse-only entry; the merged
    composite's three other forms (staged at T = 24, unstaged at T = 1,280, scalar loads at T = 17)."""
    r = render_inputs(B, N, Nf)
    occ = grid(occ_kind)
    bd = 6.0
    plain = render_entry(model, r, N, Nf, occ, None)
    off = render_entry(model, r, N, Nf, occ, (None, NAN, False))
    keys = ("rgb", "depth", "w", "z") + (("crgb", "cdepth") if Nf else ())
    for k in keys:
        assert torch.equal(off[k].view(torch.int32), plain[k].view(torch.int32)), k     # options off: the original
    only_acc = render_entry(model, r, N, Nf, occ, (None, NAN, True))
    for k in keys:
        assert torch.equal(only_acc[k].view(torch.int32), plain[k].view(torch.int32)), k
    acc = only_acc["acc"]
    assert bool(((acc.double() - plain["w"].double().sum(-1)).abs() <= (N + Nf) * 2.0 ** -24).all())
    for bg in (r["bg"], r["bg"][:1].contiguous()):
        zero = render_entry(model, r, N, Nf, occ, (torch.zeros_like(bg), NAN, True))
        assert torch.equal(zero["rgb"], plain["rgb"])                                   # bg = 0: rgb_map's bits
        got = render_entry(model, r, N, Nf, occ, (bg, bd, True))
        assert torch.equal(got["w"], plain["w"]) and torch.equal(got["z"], plain["z"])
        assert torch.equal(got["acc"], acc)
        bgb = bg.expand(B, 3)
        k = torch.clamp(1.0 - acc, min=0.0)
        assert torch.equal(got["rgb"], plain["rgb"] + k[:, None] * bgb)                 # the blend, operation for operation
        swz = (plain["w"].double() * plain["z"].double()).sum(-1)
        close(got["depth"], swz + k.double() * bd, f"depth ({B},{N},{Nf}) {occ_kind}")
        if Nf:                                                                          # the coarse maps: the same blend
            kc = torch.clamp(1.0 - got["cacc"], min=0.0)
            assert torch.equal(got["crgb"], plain["crgb"] + kc[:, None] * bgb)
        if occ_kind == "zeros":                                                         # every sample dead
            assert not bool(acc.any()) and torch.equal(got["rgb"], bgb.contiguous())
            assert bool((got["depth"] == bd).all())
            if Nf:
                assert not bool(got["cacc"].any()) and torch.equal(got["crgb"], bgb.contiguous())
                assert bool((got["cdepth"] == bd).all())
        else:
            assert float(acc.max()) > 0.0


def test_render_bg_argument_errors(model):
    r = render_inputs(8, 8, 0)
    lib = _L().load()
    for bad in ((r["bg"][:3].contiguous(), NAN, True),):
        with pytest.raises(AssertionError):
            render_entry(model, r, 8, 0, None, bad)
        assert b"bg_rows" in lib.nerf_last_error()


def _volume(model, r, N, Nf, **kw):
    import nerfmi
    with torch.no_grad():
        return nerfmi.volume_render(model, r["o"], r["d"], 2.0, 6.0, N, Nf, perturb=True, hierarchical=bool(Nf), seed=11,
                                    **kw)


@pytest.mark.parametrize("Nf", [0, 40])
def test_volume_render_options(arith, model, Nf):
    B, N = 48, 32
    r = render_inputs(B, N, Nf)
    rgb0, depth0, ex0 = _volume(model, r, N, Nf)
    assert "acc_map" not in ex0
    rgb1, depth1, ex1 = _volume(model, r, N, Nf, return_acc=True)
    assert torch.equal(rgb1, rgb0) and torch.equal(depth1, depth0)                      # return_acc alone: bit-identical
    assert ex1["acc_map"].shape == (B, 1) and ("acc_map_coarse" in ex1) == bool(Nf)
    assert torch.equal(ex1["weights"], ex0["weights"])
    k = torch.clamp(1.0 - ex1["acc_map"], min=0.0)
    for bg, bgb in (((0.25, 0.5, 1.0), torch.tensor([[0.25, 0.5, 1.0]], device="cuda").expand(B, 3)), (r["bg"], r["bg"])):
        rgb2, depth2, ex2 = _volume(model, r, N, Nf, background=bg, background_depth=6.0)
        assert torch.equal(ex2["acc_map"], ex1["acc_map"])
        assert torch.equal(rgb2, rgb0 + k * bgb)
        rgb3, depth3, _ = _volume(model, r, N, Nf, background=bg, background_color=(1.0, 0.0, 0.0))
        assert torch.equal(rgb3, rgb2) and torch.equal(depth3, depth0)                  # background_color stays ignored
    occ = grid("zeros")
    rgb4, depth4, ex4 = _volume(model, r, N, Nf, background=(0.25, 0.5, 1.0), background_depth=6.0, occupancy=occ)
    assert bool((rgb4 == torch.tensor([0.25, 0.5, 1.0], device="cuda")).all()) and bool((depth4 == 6.0).all())
    assert not bool(ex4["acc_map"].any())
    with pytest.raises(ValueError, match="staged"):
        _volume(model, r, N, Nf, return_acc=True, staged=True)


def test_volume_render_background_under_gradients(ref_state):
    """The coarse differentiable path with a background, a background depth and a differentiable acc_map
    (nerf_composite_bg forward, nerf_composite_backward_grad_acc backward).  The reference side runs the
    differentiable per-sample model call on the same points and composites with torch autograd of the
    restated definitions in float32 on the device.  Both sides evaluate the same points with the same MLP
    kernels; they differ in the composite (float32 torch against the kernels' double scans: 2^-24 per
    operation over 16 samples, up to 1e-5 where 1 - exp(-x) cancels at small x) and in the grouping of the
    weight-gradient sums (per ray against per sample), so a parameter tensor's rel-L2 distance is held to
    1e-4, an order above that and four below the distance of 1 and more that leaving out the opacity and
    background paths gives."""
    import nerfmi
    m = nerfmi.NeRF(nerfmi.Config())
    m.load_state_dict(ref_state)
    m = m.cuda()
    B, N, bd = 24, 16, 6.0
    r = render_inputs(B, N, 0, seed=5)
    bg = r["bg"]

    def loss_of(colour, depth, acc):
        return (colour ** 2).sum() + 0.1 * depth.sum() + 0.5 * ((acc - 0.5) ** 2).sum()

    def grads():
        out = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
        m.zero_grad()
        return out

    rgb, depth, ex = nerfmi.volume_render(m, r["o"], r["d"], 2.0, 6.0, N, 0, perturb=True, t_rand=r["t_rand"],
                                          background=bg, background_depth=bd)
    acc = ex["acc_map"]
    assert rgb.requires_grad and depth.requires_grad and acc.requires_grad
    with torch.no_grad():
        rgb_p, depth_p, ex_p = nerfmi.volume_render(m, r["o"], r["d"], 2.0, 6.0, N, 0, perturb=True, t_rand=r["t_rand"],
                                                    background=bg, background_depth=bd)
    close(rgb.detach(), rgb_p, "colour, training forward vs inference")
    close(acc.detach(), ex_p["acc_map"], "acc, training forward vs inference")
    loss_of(rgb, depth[:, 0], acc[:, 0]).backward()
    got = grads()
    z = ex["z_vals"].detach()
    dn = torch.empty_like(r["d"])                       # the kernels' own normalisation: the same points, bit for bit
    ok(_L().load().nerf_normalize_dirs(P(r["d"]), B, P(dn), S()))
    pts = (r["o"][:, None, :] + dn[:, None, :] * z[..., None]).reshape(-1, 3)
    rgb_s, sig_s = m(pts, dn[:, None, :].expand(B, N, 3).reshape(-1, 3))
    colour, depth_r, acc_r = restated(rgb_s.reshape(B, N, 3), sig_s.reshape(B, N), z, bg, bd, torch.float32)
    close(rgb.detach(), colour.detach(), "colour vs the restatement")
    loss_of(colour, depth_r, acc_r).backward()
    ref = grads()
    rgb2, depth2, _ = nerfmi.volume_render(m, r["o"], r["d"], 2.0, 6.0, N, 0, perturb=True, t_rand=r["t_rand"])
    ((rgb2 ** 2).sum() + 0.1 * depth2.sum()).backward()
    plain = grads()
    for n in ("density_head.weight", "pts_linears.0.weight", "pts_linears.7.weight", "rgb_linear.weight"):
        print(f"{n}: rel-L2 vs torch autograd of the restatement {rel_l2(got[n], ref[n]):.3g}, "
              f"vs the plain render's {rel_l2(got[n], plain[n]):.3g}")
        assert rel_l2(got[n], ref[n]) <= 1e-4, n
    assert rel_l2(got["density_head.weight"], plain["density_head.weight"]) > 1e-2


def test_chunked_render_with_background_equals_one_launch(arith, tmp_path):
    """nerf_render_rays_bg past the launch-size limit (lowered to 4,096 samples in a child process): 300
    rays at 32 + 40 with one background colour per ray run as 3 chunks of 102 rays; every output equals
    this process's one-launch render bit for bit."""
    import background_chunked
    ref = background_chunked.render(arith=arith)
    out = tmp_path / "chunked.pt"
    env = dict(os.environ, NERFMI_MAX_LAUNCH_SAMPLES="4096")
    p = subprocess.run([sys.executable, os.path.join(REPO, "tests", "background_chunked.py"), str(out), arith], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = torch.load(out, weights_only=True)
    assert set(got) == set(ref)
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
