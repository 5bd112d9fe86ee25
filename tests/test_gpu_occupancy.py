"""Occupancy-grid sample skipping on the GPU (include/nerfmi.h "occupancy grid"; csrc/occupancy.hip,
the gathered entry of csrc/mlp16s.hip, nerf_render_rays_occ) against the restated contract
(tests/occupancy_restated.py) and the masked composition of the existing entry points.

The main criterion is bit-identity: rendering with a grid equals nerf_mlp_forward on all samples,
sigma masked by the restated rule, then nerf_composite.  Every test that launches a new kernel
poisons the kernel's output buffers first.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from oracle import nerf_oracle as O

sys.path.insert(0, os.path.join(REPO, "tests"))
import occupancy_restated as R   # noqa: E402

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-6
LO, HI = (-1.5, -1.3, -1.7), (1.6, 1.9, 1.4)       # not symmetric about the camera axis
F3 = ctypes.c_float * 3


@pytest.fixture(scope="module")
def nerfmi_mod():
    import nerfmi
    return nerfmi


@pytest.fixture(scope="module")
def lib(nerfmi_mod):
    from nerfmi import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def model(nerfmi_mod, ref_state):
    m = nerfmi_mod.NeRF(nerfmi_mod.Config())
    m.load_state_dict(ref_state)
    return m.cuda().eval().requires_grad_(False)


@pytest.fixture(params=["f16x3", "f32"])
def arith(request, nerfmi_mod):
    prev = nerfmi_mod.set_mlp_arith(request.param)
    yield request.param
    nerfmi_mod.set_mlp_arith(prev)


@pytest.fixture(scope="module")
def f1_rays(golden):
    f1 = golden("f1_get_rays.npz")
    return torch.from_numpy(f1["chair_o"]).contiguous(), torch.from_numpy(f1["chair_d"]).contiguous()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc, lib):
    assert rc == 0, lib.nerf_last_error()


def c_grid(G):
    return F3(*[float(np.float32(v)) for v in LO]), F3(*[float(v) for v in R.inv_of(LO, HI, G)])


def masks_for(G):
    return {"sphere": R.sphere_mask(G), "checker": R.checker_mask(G),
            "single": R.single_cell_mask(G, (G // 2, G // 2 - 1 if G > 1 else 0, G // 2)),
            "ones": np.ones((G, G, G), bool), "zeros": np.zeros((G, G, G), bool)}


def bits_of(mask):
    return torch.from_numpy(R.pack_bits(mask).view(np.int32).copy()).cuda()


def grid_of(nerfmi_mod, mask, lo=LO, hi=HI):
    G = mask.shape[0]
    return nerfmi_mod.OccupancyGrid(lo, hi, G).from_mask(torch.from_numpy(mask))


def staged_inputs(lib, model, o, d, N, app=None, near=2.0, far=6.0):
    """dn, z (perturb=False), ray features and the packed weights through the per-stage entry points."""
    from nerfmi.render import packed_for
    from nerfmi.ray_utils import linspace_table
    B = o.shape[0]
    dn = torch.empty_like(d)
    ok(lib.nerf_normalize_dirs(P(d), B, P(dn), S()), lib)
    z = torch.empty(B, N, device="cuda")
    ok(lib.nerf_sample_stratified(P(o), P(dn), B, near, far, N, P(linspace_table(N, o.device)), 0, None, 0, P(z),
                                  None, S()), lib)
    packed = packed_for(model)
    feat = torch.empty(B, 256, device="cuda")
    ok(lib.nerf_ray_features(P(packed), P(dn), B, P(app), 0 if app is None else 1, P(feat), S()), lib)
    return packed, dn, z, feat


def mlp_all(lib, packed, o, dn, z, feat):
    B, N = z.shape
    rgb = torch.full((B * N, 3), float("nan"), device="cuda")
    sigma = torch.full((B * N,), float("nan"), device="cuda")
    ok(lib.nerf_mlp_forward(P(packed), P(o), P(dn), P(z), B, N, P(feat), P(rgb), P(sigma), None, 0, S()), lib)
    return rgb, sigma


def composite(lib, rgb, sigma, z):
    B, N = z.shape
    rgb_map = torch.full((B, 3), float("nan"), device="cuda")
    depth = torch.full((B, 1), float("nan"), device="cuda")
    w = torch.full((B, N), float("nan"), device="cuda")
    ok(lib.nerf_composite(P(rgb), P(sigma), P(z), B, N, P(rgb_map), P(depth), P(w), S()), lib)
    return rgb_map, depth, w


def close(gpu, ref, what):
    gpu, ref = gpu.detach().float().cpu().numpy(), ref.detach().float().cpu().numpy()
    assert gpu.shape == ref.shape, (what, gpu.shape, ref.shape)
    err = np.abs(gpu - ref)
    bad = err > ATOL + RTOL * np.abs(ref)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} outside tol; max abs err {err.max():.3g}"


# --------------------------------------------------------------------------------- 1. classify
def classify_rays(n):
    """37 rays: 31 random ones and the six axis rays from the origin, z from 0 to 4, so that the samples
    leave the box through every face."""
    g = torch.Generator().manual_seed(11)
    o = torch.cat([torch.rand(31, 3, generator=g) * 2 - 1, torch.zeros(6, 3)])
    d = torch.cat([torch.nn.functional.normalize(torch.randn(31, 3, generator=g), dim=-1),
                   torch.eye(3), -torch.eye(3)])
    z = (torch.linspace(0.0, 4.0, n).expand(37, n) + torch.rand(37, 1, generator=g) * 0.1).contiguous()
    return o.contiguous(), d.contiguous(), z


@pytest.mark.parametrize("G", [5, 32])
@pytest.mark.parametrize("n", [7, 64])
def test_classify_matches_the_restated_rule(lib, n, G):
    o, d, z = classify_rays(n)
    B = o.shape[0]
    t = R.cell_coords(o, d, z, LO, HI, G)
    for c in range(3):                       # every out-of-box branch is taken by some sample
        assert bool((t[..., c] < 0).any()) and bool((t[..., c] >= G).any()), c
    og, dg, zg = o.cuda(), d.cuda(), z.cuda()
    lo, inv = c_grid(G)
    ws = torch.empty(lib.nerf_occupancy_classify_workspace_bytes(B, n), dtype=torch.uint8, device="cuda")
    for name, m in masks_for(G).items():
        want = R.classify(o, d, z, LO, HI, G, m)
        idx, cnt = R.live_list(want)
        bits = bits_of(m)
        for with_mask in (True, False):
            live = torch.full((B * n,), -1, dtype=torch.int32, device="cuda")
            count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
            mask = torch.full((B, n), 0xCD, dtype=torch.uint8, device="cuda") if with_mask else None
            ws.fill_(0xEE)
            ok(lib.nerf_occupancy_classify(P(og), P(dg), P(zg), B, n, P(bits), G, lo, inv, P(live), P(count),
                                           P(mask), P(ws), ws.numel(), S()), lib)
            assert int(count.item()) == cnt, (name, n, G)
            got = live[:cnt].cpu()
            assert torch.equal(got, idx), (name, n, G)
            assert bool((got[1:] > got[:-1]).all()), "ascending"
            assert bool((live[cnt:] == -1).all()), "nothing written past the count"
            if with_mask:
                assert torch.equal(mask.cpu().bool(), want), (name, n, G)
        if name == "ones":
            assert 0 < cnt < B * n
        if name == "zeros":
            assert cnt == 0


# ------------------------------------------------------------------------------ 2. gathered MLP
@pytest.fixture(scope="module")
def mlp_case(lib, model, f1_rays, nerfmi_mod):
    """100 F1 rays x 64 samples and 37 x 7, evaluated once by nerf_mlp_forward (f16x3)."""
    prev = nerfmi_mod.set_mlp_arith("f16x3")
    out = {}
    for B, N in ((100, 64), (37, 7)):
        o, d = f1_rays[0][:B].cuda(), f1_rays[1][:B].cuda()
        packed, dn, z, feat = staged_inputs(lib, model, o, d, N)
        rgb, sigma = mlp_all(lib, packed, o, dn, z, feat)
        out[(B, N)] = (packed, o, dn, z, feat, rgb, sigma)
    torch.cuda.synchronize()
    nerfmi_mod.set_mlp_arith(prev)
    return out


@pytest.mark.parametrize("B,N,k", [(100, 64, 0), (100, 64, 1), (100, 64, 127), (100, 64, 128), (100, 64, 129),
                                   (100, 64, 3001), (100, 64, 6400), (37, 7, 129)])
def test_gathered_mlp_rows_equal_the_plain_forward(lib, nerfmi_mod, mlp_case, B, N, k):
    prev = nerfmi_mod.set_mlp_arith("f16x3")
    try:
        packed, o, dn, z, feat, rgb_all, sigma_all = mlp_case[(B, N)]
        M = B * N
        g = torch.Generator().manual_seed(100 + k)
        if k == M:
            idx = torch.arange(M)
        else:                                    # sample 0 stays outside the list: the list's tail names it
            idx = (torch.randperm(M - 1, generator=g)[:k] + 1).sort().values
        live = torch.zeros(M, dtype=torch.int32, device="cuda")
        live[:k] = idx.to(torch.int32).cuda()
        count = torch.tensor([k], dtype=torch.int32, device="cuda")
        rgb = torch.full((M, 3), 12345.0, device="cuda")
        sigma = torch.full((M,), 12345.0, device="cuda")
        ok(lib.nerf_mlp_forward_live(P(packed), P(o), P(dn), P(z), B, N, P(feat), P(live), P(count), P(rgb), P(sigma),
                                     S()), lib)
        sel = torch.zeros(M, dtype=torch.bool)
        sel[idx] = True
        sel = sel.cuda()
        assert torch.equal(rgb[sel], rgb_all[sel]) and torch.equal(sigma[sel], sigma_all[sel])
        assert bool((rgb[~sel] == 12345.0).all()) and bool((sigma[~sel] == 12345.0).all())
    finally:
        nerfmi_mod.set_mlp_arith(prev)


def test_gathered_mlp_is_f16x3_only(lib, nerfmi_mod, mlp_case):
    packed, o, dn, z, feat, _, _ = mlp_case[(37, 7)]
    prev = nerfmi_mod.set_mlp_arith("f32")
    try:
        live = torch.zeros(37 * 7, dtype=torch.int32, device="cuda")
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        buf = torch.zeros(37 * 7, 3, device="cuda")
        rc = lib.nerf_mlp_forward_live(P(packed), P(o), P(dn), P(z), 37, 7, P(feat), P(live), P(count), P(buf),
                                       P(buf), S())
        assert rc == 3 and b"f16x3" in lib.nerf_last_error()
    finally:
        nerfmi_mod.set_mlp_arith(prev)


# ------------------------------------------------------------------------------ 3. pack / dilate
@pytest.mark.parametrize("G", [5, 33])
@pytest.mark.parametrize("s", [1, 2])
def test_pack_and_dilate_match_the_restatement(lib, nerfmi_mod, G, s):
    L = s * G
    g = torch.Generator().manual_seed(5 * G + s)
    lat = torch.rand(L, L, L, generator=g)
    thr = 0.97 if s == 1 else 0.995
    want = R.threshold_mask(lat.numpy(), G, s, thr)
    assert 0 < want.sum() < want.size // 4
    words = lib.nerf_occupancy_words(G)
    bits = torch.full((words,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ok(lib.nerf_occupancy_pack(P(lat.cuda().contiguous()), G, s, thr, P(bits), S()), lib)
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), R.pack_bits(want)), "pack"
    cur = bits
    for step in (1, 2):
        out = torch.full((words,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        ok(lib.nerf_occupancy_dilate(P(cur), G, P(out), S()), lib)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), R.pack_bits(R.dilate(want, step))), step
        cur = out
    for dil in (0, 1, 2):                      # the Python surface
        grid = nerfmi_mod.OccupancyGrid(LO, HI, G).from_density(lat, threshold=thr, supersample=s, dilate=dil)
        exp = R.dilate(want, dil)
        assert np.array_equal(grid.bits.cpu().numpy().view(np.uint32), R.pack_bits(exp)), dil
        assert np.array_equal(grid.to_mask().cpu().numpy(), exp) and grid.fraction() == exp.sum() / G ** 3
    # a threshold that equals a probe: strictly greater
    lat2 = torch.zeros(L, L, L)
    lat2[0, 0, 0] = 1.0
    assert nerfmi_mod.OccupancyGrid(LO, HI, G).from_density(lat2, 1.0, s, 0).fraction() == 0.0
    assert nerfmi_mod.OccupancyGrid(LO, HI, G).from_density(lat2, 0.5, s, 0).fraction() == 1 / G ** 3


# -------------------------------------------------------------------------------- 4. from_model
def test_from_model_matches_the_oracle_density(nerfmi_mod, model, ref_state):
    """Bits equal the oracle's sigma > thr on probe_points(), except at probes within the parity
    tolerance of the threshold, of which there may be at most 1 % (the oracle alone: 1 of 512, the
    median probe itself)."""
    G = 8
    pts = nerfmi_mod.OccupancyGrid(LO, HI, G).probe_points()
    assert pts.shape == (G, G, G, 3) and pts.dtype == torch.float32
    x = pts.reshape(-1, 3).cpu()
    with torch.no_grad():
        _, sig = O.nerf_forward(ref_state, x, torch.tensor([[1.0, 0.0, 0.0]]).expand(x.shape[0], 3))
    sig = sig.reshape(-1)
    thr = float(sig[sig > 0].median())
    ambiguous = (sig - thr).abs() <= 1e-4 * thr + 1e-6
    print(f"threshold {thr:.6g}; {int(ambiguous.sum())} of {sig.numel()} probes within tolerance of it")
    assert int(ambiguous.sum()) <= sig.numel() // 100
    grid = nerfmi_mod.OccupancyGrid.from_model(model, LO, HI, resolution=G, threshold=thr, supersample=1, dilate=0)
    got = grid.to_mask().cpu().reshape(-1)
    want = sig > thr
    assert 0 < int(want.sum()) < want.numel()
    assert torch.equal(got[~ambiguous], want[~ambiguous])
    # slabs do not change the result
    g2 = nerfmi_mod.OccupancyGrid.from_model(model, LO, HI, resolution=G, threshold=thr, dilate=0, slab_samples=100)
    assert torch.equal(g2.bits, grid.bits)


# ------------------------------------------------------------------------- 5-8. render with a grid
RENDER_G = 32


@pytest.fixture(scope="module")
def render_mask():
    return R.sphere_mask(RENDER_G, 0.3)


@pytest.fixture(scope="module")
def oracle_coarse(ref_state, f1_rays, app_vec):
    """Oracle z, pts, rgb and sigma of the coarse cases, computed once: (B, N) -> tensors (CPU)."""
    out = {}
    for B, N in ((4096, 64), (37, 7)):
        o, d = f1_rays[0][:B], f1_rays[1][:B]
        dn = O.normalize(d)
        z, pts = O.sample_stratified(o, dn, 2.0, 6.0, N)
        with torch.no_grad():
            rgb, sigma = O.nerf_forward(ref_state, pts.reshape(-1, 3),
                                        dn.unsqueeze(1).expand(-1, N, -1).reshape(-1, 3),
                                        app_vec.unsqueeze(0).expand(B * N, -1))
        out[(B, N)] = (dn, z.contiguous(), rgb.reshape(B, N, 3), sigma.reshape(B, N, 1))
    return out


@pytest.mark.parametrize("B,N", [(4096, 64), (37, 7)])
def test_render_coarse_is_the_masked_composition(lib, nerfmi_mod, model, f1_rays, app_vec, render_mask, oracle_coarse,
                                                 arith, B, N):
    o, d = f1_rays[0][:B].cuda(), f1_rays[1][:B].cuda()
    app = app_vec.cuda().reshape(1, 32).contiguous()
    packed, dn, z, feat = staged_inputs(lib, model, o, d, N, app)
    dn_o, z_o, rgb_o, sigma_o = oracle_coarse[(B, N)]
    assert torch.equal(dn.cpu(), dn_o) and torch.equal(z.cpu(), z_o)        # no sample is ambiguous
    live = R.classify(o.cpu(), dn_o, z_o, LO, HI, RENDER_G, render_mask)
    share = float(live.float().mean())
    print(f"live share {share:.3f}")
    if B == 4096:
        assert 0.02 < share < 0.9
    rgb_s, sigma_s = mlp_all(lib, packed, o, dn, z, feat)
    sigma_m = torch.where(live.reshape(-1).cuda(), sigma_s, torch.zeros_like(sigma_s))
    want = composite(lib, rgb_s, sigma_m, z)
    grid = grid_of(nerfmi_mod, render_mask)
    with torch.no_grad():
        rgb, depth, ex = nerfmi_mod.volume_render(model, o, d, 2.0, 6.0, N, 0, appearance_embedding=app_vec.cuda(),
                                                  perturb=False, occupancy=grid)
    assert torch.equal(rgb, want[0]) and torch.equal(depth, want[1])
    assert torch.equal(ex["weights"].squeeze(-1), want[2]) and torch.equal(ex["z_vals"], z)
    assert bool((ex["weights"].squeeze(-1)[~live.cuda()] == 0).all())
    # against the oracle's composite of its own sigma, masked by the restated rule
    sig_masked = torch.where(live.unsqueeze(-1), sigma_o, torch.zeros_like(sigma_o))
    rgb_ref, depth_ref, w_ref = O.composite(rgb_o, sig_masked, z_o)
    close(rgb, rgb_ref, "rgb")
    close(depth, depth_ref, "depth")
    close(ex["weights"], w_ref, "weights")


@pytest.mark.parametrize("B,N,Nf", [(1024, 64, 128), (37, 5, 3)])
def test_render_hierarchical_is_the_masked_composition(lib, nerfmi_mod, model, f1_rays, app_vec, render_mask, arith,
                                                       B, N, Nf):
    """The composed side evaluates all N + Nf merged samples (reuse_coarse=False semantics, pinned
    bit-identical to the reuse path by tests/test_gpu_parity.py)."""
    from nerfmi.ray_utils import linspace_table
    o, d = f1_rays[0][:B].cuda(), f1_rays[1][:B].cuda()
    packed, dn, z, feat = staged_inputs(lib, model, o, d, N, app_vec.cuda().reshape(1, 32).contiguous())
    u = torch.rand(B, Nf, generator=torch.Generator().manual_seed(21)).cuda()
    T = N + Nf
    # coarse
    live_c = R.classify(o.cpu(), dn.cpu(), z.cpu(), LO, HI, RENDER_G, render_mask)
    rgb_c, sigma_c = mlp_all(lib, packed, o, dn, z, feat)
    sigma_c = torch.where(live_c.reshape(-1).cuda(), sigma_c, torch.zeros_like(sigma_c))
    crgb, cdepth, wc = composite(lib, rgb_c, sigma_c, z)
    # fine: resample from the masked coarse weights, evaluate and mask all merged samples
    z_all = torch.full((B, T), float("nan"), device="cuda")
    ok(lib.nerf_sample_importance(P(o), P(dn), P(z), P(wc), B, N, Nf, P(linspace_table(Nf, o.device, drop_last=True)),
                                  P(u), 0, P(z_all), None, S()), lib)
    live_f = R.classify(o.cpu(), dn.cpu(), z_all.cpu(), LO, HI, RENDER_G, render_mask)
    rgb_a, sigma_a = mlp_all(lib, packed, o, dn, z_all, feat)
    sigma_a = torch.where(live_f.reshape(-1).cuda(), sigma_a, torch.zeros_like(sigma_a))
    want = composite(lib, rgb_a, sigma_a, z_all)
    grid = grid_of(nerfmi_mod, render_mask)
    with torch.no_grad():
        rgb, depth, ex = nerfmi_mod.volume_render(model, o, d, 2.0, 6.0, N, Nf, appearance_embedding=app_vec.cuda(),
                                                  perturb=False, hierarchical=True, u_rand=u, occupancy=grid)
    assert torch.equal(ex["z_vals"], z_all)
    assert torch.equal(ex["rgb_map_coarse"], crgb) and torch.equal(ex["depth_map_coarse"], cdepth)
    assert torch.equal(rgb, want[0]) and torch.equal(depth, want[1])
    assert torch.equal(ex["weights"].squeeze(-1), want[2])
    assert bool((ex["weights"].squeeze(-1)[~live_f.cuda()] == 0).all())
    if B == 1024:
        assert 0.02 < float(live_f.float().mean()) < 0.95


@pytest.mark.parametrize("B,N,Nf", [(1024, 64, 128), (37, 7, 0), (37, 5, 3)])
def test_all_ones_grid_is_the_plain_render_and_all_zeros_is_empty(nerfmi_mod, model, f1_rays, app_vec, arith, B, N, Nf):
    o, d = f1_rays[0][:B].cuda(), f1_rays[1][:B].cuda()
    u = torch.rand(B, max(Nf, 1), generator=torch.Generator().manual_seed(22)).cuda()
    kw = dict(appearance_embedding=app_vec.cuda(), perturb=False, hierarchical=Nf > 0, u_rand=u if Nf else None)
    box = ((-8.0, -8.0, -8.0), (8.0, 8.0, 8.0))          # contains every sample of the 2..6 segment
    ones = grid_of(nerfmi_mod, np.ones((4, 4, 4), bool), *box)
    zeros = grid_of(nerfmi_mod, np.zeros((4, 4, 4), bool), *box)
    with torch.no_grad():
        plain = nerfmi_mod.volume_render(model, o, d, 2.0, 6.0, N, Nf, **kw)
        full = nerfmi_mod.volume_render(model, o, d, 2.0, 6.0, N, Nf, occupancy=ones, **kw)
        empty = nerfmi_mod.volume_render(model, o, d, 2.0, 6.0, N, Nf, occupancy=zeros, **kw)
    assert torch.equal(full[0], plain[0]) and torch.equal(full[1], plain[1])
    assert set(full[2]) == set(plain[2])
    for k in plain[2]:
        assert torch.equal(full[2][k], plain[2][k]), k
    assert float(plain[0].abs().max()) > 0
    assert bool((empty[0] == 0).all()) and bool((empty[1] == 0).all()) and bool((empty[2]["weights"] == 0).all())
    if Nf == 0:
        assert torch.equal(empty[2]["z_vals"], plain[2]["z_vals"])
    for t in (empty[0], empty[1], empty[2]["weights"], empty[2]["z_vals"]):
        assert bool(torch.isfinite(t).all())


def test_grid_on_the_wrong_device_or_dtype_is_refused(nerfmi_mod, model, f1_rays):
    o, d = f1_rays[0][:8].cuda(), f1_rays[1][:8].cuda()
    cpu_grid = nerfmi_mod.OccupancyGrid(LO, HI, 4, device="cpu")
    with torch.no_grad():
        with pytest.raises(ValueError, match="grid is on"):
            nerfmi_mod.volume_render(model, o, d, 2.0, 6.0, 8, 0, occupancy=cpu_grid)
        g = nerfmi_mod.OccupancyGrid(LO, HI, 4)
        g.bits = g.bits.to(torch.int64)
        with pytest.raises(ValueError, match="int32"):
            nerfmi_mod.volume_render(model, o, d, 2.0, 6.0, 8, 0, occupancy=g)


# ----------------------------------------------------------------------------------- 9. chunked
def test_chunked_call_equals_the_one_launch_call(nerfmi_mod, tmp_path):
    """With NERFMI_MAX_LAUNCH_SAMPLES = 2^16 in a child process (the hook is read once), a 3,000-ray
    64 + 128 render with a grid runs as 6 chunks of 512 rays: every output equals this process's
    one-launch render bit for bit."""
    import subprocess
    import occupancy_chunked
    ref = occupancy_chunked.render()
    out = tmp_path / "chunked.pt"
    env = dict(os.environ, NERFMI_MAX_LAUNCH_SAMPLES=str(1 << 16))
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "occupancy_chunked.py"), str(out)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = torch.load(out, weights_only=True)
    assert set(got) == set(ref)
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
    assert float(ref["rgb"].abs().max()) > 0 and bool((ref["weights"] == 0).any())


# --------------------------------------------------------------------------------------- 10. CLI
def test_run_cli_with_an_occupancy_grid(tmp_path, capsys):
    from PIL import Image
    import run as cli
    out = str(tmp_path / "occ")
    rc = cli.main(["--mode", "render", "--scene", "chair", "--random_init", "0", "--occupancy", "16", "--quality",
                   "preview", "--width", "40", "--height", "24", "--frames", "1", "--output_dir", out, "--save_depth"])
    assert rc == 0
    assert "Occupancy grid 16^3" in capsys.readouterr().out
    assert np.array(Image.open(os.path.join(out, "rgb_000.png"))).shape == (24, 40, 3)
    dep = np.load(os.path.join(out, "raw", "depth_000.npy"))
    assert dep.shape == (24, 40) and np.isfinite(dep).all()
