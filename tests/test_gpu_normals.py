"""Density-gradient normals on the GPU (include/nerfmi_train.h "position gradient and normals",
DESIGN.md §17): the position-gradient kernel against float64 on its own ReLU branches, its independence
of the launch's size, the normals composite against its formula, and the normal map of volume_render,
the chunked pass and the CLI.

The float64 references are kink-proof in the way of tests/test_gpu_accuracy.py::test_gradients_vs_float64:
each fp32 evaluation is compared with float64 on the piecewise-linear branch that evaluation took (the
GPU's ReLU masks from its saved activations, the fp32 CPU autograd's from its own pre-activations)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

M_POINTS = 2085          # 65 blocks of 32 + 5: a ragged tail over many waves
_CACHE = {}


@pytest.fixture(scope="module", autouse=True, params=["f16x3", "f32"])
def arith(request):
    from nerfmi import _lib as L
    prev = L.set_mlp_arith(request.param)
    yield request.param
    L.set_mlp_arith(prev)


def model_of(state):
    import nerfmi
    m = nerfmi.NeRF(nerfmi.Config())
    m.load_state_dict(state)
    return m.cuda().eval().requires_grad_(False)


def points():
    g = torch.Generator().manual_seed(31)
    x = torch.rand(M_POINTS, 3, generator=g) * 3 - 1.5
    d = torch.nn.functional.normalize(torch.randn(M_POINTS, 3, generator=g), dim=-1)
    g_rgb, g_sig = torch.randn(M_POINTS, 3, generator=g), torch.randn(M_POINTS, 1, generator=g)
    return x, d, g_rgb, g_sig


def half_empty_state(ref_state):
    """ref_state with density_head.bias lowered by the median density pre-activation of the test's points
    (fp32 CPU oracle): half of them then have sigma = 0."""
    if "half" not in _CACHE:
        x, d, _, _ = points()
        pres = []

        def relu(pre, i):
            if i == 8:
                pres.append(pre.detach())
            return torch.relu(pre)
        with torch.no_grad():
            O.nerf_forward(ref_state, x, d, None, relu=relu)
        st = {k: v.clone() for k, v in ref_state.items()}
        st["density_head.bias"] = st["density_head.bias"] - pres[0].median()
        _CACHE["half"] = st
    return _CACHE["half"]


def gpu_position_grad(model, x, d, app, g_sig, g_rgb, guard=64):
    """The staged C calls on points x (one "ray" per point, z = 0): ray features, forward with saves,
    data-gradient chain for the given upstream (g_sig (M), g_rgb (M,3)), position gradient.  Returns sigma,
    dx (M,3), the ten ReLU masks the forward took (from its saved activations) and the guard floats behind
    dx (filled with a sentinel before the launch)."""
    from nerfmi import _lib
    from nerfmi.autograd import packed_pair
    from nerfmi.normals import packed_input_for
    lib, s, P = _lib.load(), _lib.stream(), _lib.ptr
    packed, packedT = packed_pair(model)
    packed_in = packed_input_for(model)
    M, dev = x.shape[0], x.device
    appd, rows = (None, 0) if app is None else (app.reshape(1, 32).to(dev).contiguous(), 1)
    feat, encd = torch.empty(M, 256, device=dev), torch.empty(M, 32, device=dev)
    z = torch.zeros(M, 1, device=dev)
    rgb, sigma = torch.empty(M, 3, device=dev), torch.empty(M, device=dev)
    MT = _lib.tile_rows(M)
    save = torch.empty(MT, _lib.SAVE_ROW, device=dev)
    grad = torch.empty(MT, _lib.GRAD_ROW, device=dev)
    masks = torch.empty(M, _lib.MASK_ROW, dtype=torch.int32, device=dev)
    dx = torch.full((M * 3 + guard,), 12345.0, device=dev)
    dsig, drgb = g_sig.reshape(M).to(dev).contiguous(), g_rgb.reshape(M, 3).to(dev).contiguous()
    _lib.check(lib.nerf_ray_features_train(P(packed), P(d), M, P(appd), rows, P(feat), P(encd), s), "features")
    _lib.check(lib.nerf_mlp_forward_train(P(packed), P(x), P(d), P(z), M, 1, P(feat), P(encd), P(rgb), P(sigma),
                                          P(save), P(masks), s), "mlp_forward_train")
    _lib.check(lib.nerf_mlp_backward(P(packed), P(packedT), P(save), P(masks), P(sigma), P(rgb), P(dsig), P(drgb), M,
                                     P(grad), s), "mlp_backward")
    _lib.check(lib.nerf_mlp_position_grad(P(packed_in), P(save), P(grad), M, P(dx), s), "position_grad")
    rows_ = _lib.untile(save, M).cpu()
    h_at = [l * 256 if l < 4 else 1024 + 64 + (l - 4) * 256 for l in range(8)]        # layout.h save_h
    m = [rows_[:, a:a + 256] > 0 for a in h_at]
    m.append((sigma.cpu() > 0).reshape(M, 1))
    m.append(rows_[:, 2144:2144 + 128] > 0)                                           # kSaveRDir
    return sigma.cpu(), dx[:M * 3].reshape(M, 3).cpu(), m, dx[M * 3:].cpu()


def ref_position_grad(st, x, d, app, g_sig, g_rgb, dtype, masks=None, record=None, pres=None):
    """d/dx of sum(rgb g_rgb) + sum(sigma g_sig) by torch autograd of the oracle, in `dtype`, on the given
    ReLU branches (masks) or on its own (recorded into `record`; pre-activations into `pres`)."""
    sd = {k: v.to(dtype) for k, v in st.items()}
    xg = x.to(dtype).clone().requires_grad_(True)

    def relu(pre, i):
        if record is not None:
            record.append(pre.detach() > 0)
        if pres is not None:
            pres.append(pre.detach())
        return torch.relu(pre) if masks is None else pre * masks[i].to(dtype)
    with torch.enable_grad():
        r, s = O.nerf_forward(sd, xg, d.to(dtype), None if app is None else app.to(dtype), relu=relu)
        ((r * g_rgb.to(dtype)).sum() + (s * g_sig.to(dtype)).sum()).backward()
    return xg.grad.double()


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-300))


def cpu_refs(key, st, x, d, app, g_sig, g_rgb):
    """The fp32 CPU autograd, its ReLU branches, float64 on those branches and the float64
    pre-activations: independent of the GPU's arithmetic, computed once per (weights, upstream)."""
    if key not in _CACHE:
        m_cpu, pre64 = [], []
        g32 = ref_position_grad(st, x, d, app, g_sig, g_rgb, torch.float32, record=m_cpu)
        g64 = ref_position_grad(st, x, d, app, g_sig, g_rgb, torch.float64, masks=m_cpu, pres=pre64)
        near = sum(int((p.abs() <= 1e-4 * p.pow(2).mean().sqrt()).sum()) for p in pre64)
        _CACHE[key] = (g32, g64, m_cpu, near)
    return _CACHE[key]


@pytest.mark.parametrize("upstream", ["density", "random"])
@pytest.mark.parametrize("which", ["seed0", "half_empty"])
def test_position_gradient_vs_float64(which, upstream, ref_state, app_vec, arith):
    """dx of 2,085 points against float64 autograd on the GPU's own ReLU branches: rel-L2 within 2 x the
    fp32 CPU autograd's own (against float64 on ITS branches) + 1e-6, the bound of every other gradient here.
    Upstreams: the density's (dsigma = 1, drgb = 0: nerfmi.density_gradient, which must return the staged
    calls' bits) and a random (g_rgb, g_sigma).  With the density's, every point of sigma = 0 has dx == 0
    exactly.  The half-empty weights put the density head's kink in the middle of the points."""
    import nerfmi
    st = ref_state if which == "seed0" else half_empty_state(ref_state)
    model = model_of(st)
    x, d, g_rgb, g_sig = points()
    if upstream == "density":
        app = None
        d = torch.zeros_like(d)
        d[:, 2] = 1.0
        g_rgb, g_sig = torch.zeros_like(g_rgb), torch.ones_like(g_sig)
    else:
        app = app_vec
    with torch.no_grad():
        sigma, dx, m_gpu, guard = gpu_position_grad(model, x.cuda(), d.cuda(), app, g_sig, g_rgb)
    assert torch.isfinite(dx).all()
    assert (guard == 12345.0).all(), "floats behind dx[M-1] were written"
    if upstream == "density":
        s2, dx2 = nerfmi.density_gradient(model, x.cuda())
        assert torch.equal(s2.cpu(), sigma) and torch.equal(dx2.cpu(), dx)
        empty = sigma == 0
        assert (dx[empty] == 0).all(), "a point of sigma = 0 has a non-zero density gradient"
        if which == "half_empty":
            share = float(empty.float().mean())
            print(f"{which}/{arith}: {share:.3f} of the points have sigma = 0")
            assert 0.25 <= share <= 0.75, share
    g32, g64_cpu, m_cpu, near = cpu_refs((which, upstream), st, x, d, app, g_sig, g_rgb)
    g64_gpu = ref_position_grad(st, x, d, app, g_sig, g_rgb, torch.float64, masks=m_gpu)
    flips = sum(int((a != b).sum()) for a, b in zip(m_cpu, m_gpu))
    assert flips <= 4 * near + 8, (which, arith, "ReLU branches differ between the GPU and the CPU", flips, near)
    e_gpu, e_cpu = rel(dx.double(), g64_gpu), rel(g32, g64_cpu)
    bound = 2.0 * e_cpu + 1e-6
    print(f"{which}/{upstream}/{arith}: dx rel-L2 vs float64 gpu {e_gpu:.3g}, cpu fp32 {e_cpu:.3g}, bound {bound:.3g}; "
          f"{flips} ReLU branches differ ({near} float64 pre-activations within 1e-4 rms of a kink)")
    assert e_gpu <= bound, (which, upstream, arith, e_gpu, e_cpu, bound)


def test_position_independence_and_tails(ref_state, arith):
    """The first 1, 31, 32 and 33 points as launches of their own equal the rows of the 2,085-point launch
    bit for bit (a row depends on its own sample only), and no launch writes behind dx[M-1]."""
    model = model_of(ref_state)
    x, _, _, _ = points()
    x = x.cuda()
    d = torch.zeros_like(x)
    d[:, 2] = 1.0
    ones, zeros = torch.ones(M_POINTS), torch.zeros(M_POINTS, 3)
    with torch.no_grad():
        sigma, dx, _, guard = gpu_position_grad(model, x, d, None, ones, zeros)
        assert (guard == 12345.0).all()
        assert dx.abs().max() > 0
        for m in (1, 31, 32, 33):
            s_m, dx_m, _, guard = gpu_position_grad(model, x[:m].contiguous(), d[:m].contiguous(), None, ones[:m],
                                                    zeros[:m])
            assert torch.equal(s_m, sigma[:m]), m
            assert torch.equal(dx_m, dx[:m]), m
            assert (guard == 12345.0).all(), m


def normals_formula(dx, w, dtype):
    g = dx.to(dtype)
    n = -g / torch.sqrt((g * g).sum(-1, keepdim=True) + 1e-30)
    return (w.to(dtype).unsqueeze(-1) * n).sum(1)


def check_normals_bound(gpu, cpu32, f64_gpu, f64_cpu, what):
    """The largest error of the GPU against float64 is no worse than 4 x the fp32 torch evaluation's own
    + 1e-7 (components are at most 1 in magnitude: absolute errors)."""
    e_gpu = float((gpu.double() - f64_gpu).abs().max())
    e_cpu = float((cpu32.double() - f64_cpu).abs().max())
    print(f"{what}: max abs err vs float64 gpu {e_gpu:.3g}, fp32 torch {e_cpu:.3g}")
    assert e_gpu <= 4.0 * e_cpu + 1e-7, (what, e_gpu, e_cpu)


@pytest.mark.parametrize("B,T", [(37, 1), (37, 16), (37, 24), (3, 4096)])
def test_composite_normals(B, T, arith):
    """nerf_composite_normals against n = -g / sqrt(g.g + 1e-30), sum w n in float64: random gradients with
    rows of exact zeros (n = 0) and rows of norm 1e-25 (g.g underflows in fp32), random weights with zeros."""
    from nerfmi.normals import composite_normals
    g = torch.Generator().manual_seed(100 + T)
    dx = torch.randn(B, T, 3, generator=g) * torch.exp(3 * torch.randn(B, T, 1, generator=g))
    kind = torch.rand(B, T, generator=g)
    dx[kind < 0.15] = 0.0
    tiny = (kind >= 0.15) & (kind < 0.3)
    dx[tiny] = torch.nn.functional.normalize(dx[tiny], dim=-1) * 1e-25
    w = torch.rand(B, T, generator=g) / max(T // 4, 1)
    w[torch.rand(B, T, generator=g) < 0.3] = 0.0
    got = composite_normals(dx.cuda(), w.cuda()).cpu()
    assert got.shape == (B, 3) and torch.isfinite(got).all()
    f64 = normals_formula(dx, w, torch.float64)
    check_normals_bound(got, normals_formula(dx, w, torch.float32), f64, f64, f"composite normals B={B} T={T}")
    # a ray's result does not depend on the launch: the first ray alone
    one = composite_normals(dx[:1].cuda(), w[:1].cuda()).cpu()
    assert torch.equal(one, got[:1])


def render_inputs(B=37):
    g = torch.Generator().manual_seed(5)
    o = torch.randn(B, 3, generator=g) * 0.2
    d = torch.randn(B, 3, generator=g)
    u = torch.rand(B, 8, generator=g)
    return o, d, u


def dense_state(ref_state):
    """The density head x 40: opacities around 0.8 on the test's rays instead of a few per cent."""
    st = {k: v.clone() for k, v in ref_state.items()}
    st["density_head.weight"] *= 40.0
    st["density_head.bias"] *= 40.0
    return st


def rebuilt_normal_map(model, o, d, ex):
    """nerf_composite_normals(density_gradient(o + dn z), weights) from a render's extras."""
    import nerfmi
    from nerfmi import _lib
    from nerfmi.normals import composite_normals
    lib = _lib.load()
    B = o.shape[0]
    dn = torch.empty_like(d)
    _lib.check(lib.nerf_normalize_dirs(_lib.ptr(d), B, _lib.ptr(dn), _lib.stream()), "nerf_normalize_dirs")
    z = ex["z_vals"]
    pts = o[:, None, :] + dn[:, None, :] * z[..., None]          # separate roundings, as the forward's
    _, grad = nerfmi.density_gradient(model, pts)
    return composite_normals(grad, ex["weights"].reshape(B, -1)), pts, dn


@pytest.mark.parametrize("hier", [False, True])
def test_volume_render_normals(hier, ref_state, app_vec, arith):
    """volume_render(return_normals=True) at 37 rays, N = 16 (+ Nf = 8 hierarchical), perturb=False:
    (a) every other output is bit for bit the call's without the argument; (b) normal_map is
    nerf_composite_normals(density_gradient(o + dn z), weights) of the returned extras, bit for bit, also
    (d) with an occupancy grid that kills about half the samples; (c) against the float64 oracle on the
    GPU's own branches, with the density head x 40 so the rays are mostly opaque: no worse than 4 x the
    fp32 CPU evaluation (on its branches) + 1e-7."""
    import nerfmi
    st = dense_state(ref_state)
    model = model_of(st)
    o, d, u = render_inputs()
    o, d = o.cuda(), d.cuda()
    kw = dict(appearance_embedding=app_vec.cuda(), perturb=False, hierarchical=hier, u_rand=u if hier else None,
              return_acc=True)
    with torch.no_grad():
        rgb0, dep0, ex0 = nerfmi.volume_render(model, o, d, 2.0, 6.0, 16, 8, **kw)
        rgb1, dep1, ex1 = nerfmi.volume_render(model, o, d, 2.0, 6.0, 16, 8, return_normals=True, **kw)
        # (a)
        assert torch.equal(rgb0, rgb1) and torch.equal(dep0, dep1)
        assert set(ex1) == set(ex0) | {"normal_map"}
        for k in ex0:
            assert torch.equal(ex0[k], ex1[k]), k
        T = 24 if hier else 16
        assert ex1["z_vals"].shape == (37, T) and ex1["normal_map"].shape == (37, 3)
        # (b)
        nm = ex1["normal_map"]
        rebuilt, pts, dn = rebuilt_normal_map(model, o, d, ex1)
        assert torch.equal(nm, rebuilt)
        assert torch.isfinite(nm).all() and nm.abs().max() > 0
        acc = ex1["acc_map"].reshape(-1)
        assert (nm.norm(dim=-1) <= acc * (1 + 1e-5) + 1e-6).all(), "a normal longer than the ray's opacity"
        # a leading shape, and a background that the normal map ignores
        _, _, ex2 = nerfmi.volume_render(model, o[:36].reshape(4, 9, 3), d[:36].reshape(4, 9, 3), 2.0, 6.0, 16, 8,
                                         appearance_embedding=app_vec.cuda(), perturb=False, hierarchical=hier,
                                         u_rand=u[:36] if hier else None, return_normals=True,
                                         background=(1.0, 0.5, 0.25))
        assert ex2["normal_map"].shape == (4, 9, 3)
        assert torch.equal(ex2["normal_map"].reshape(36, 3), nm[:36])
        # (d)
        gm = torch.Generator().manual_seed(9)
        grid = nerfmi.OccupancyGrid((-7.0,) * 3, (7.0,) * 3, 8).from_mask(torch.rand(8, 8, 8, generator=gm) < 0.5)
        _, _, ex3 = nerfmi.volume_render(model, o, d, 2.0, 6.0, 16, 8, occupancy=grid, return_normals=True, **kw)
        dead = float((ex3["weights"] == 0).float().mean()), float((ex1["weights"] == 0).float().mean())
        assert dead[0] > dead[1] + 0.1, dead
        rebuilt3, _, _ = rebuilt_normal_map(model, o, d, ex3)
        assert torch.equal(ex3["normal_map"], rebuilt3)
        assert not torch.equal(ex3["normal_map"], nm)
    # (c) the oracle on the GPU's points and z, in float64 on the GPU's branches / in fp32 and float64 on the CPU's
    B = 37
    z = ex1["z_vals"].cpu()
    p = pts.reshape(-1, 3).cpu()
    dd = torch.zeros_like(p)                     # sigma and its gradient do not depend on the direction
    dd[:, 2] = 1.0
    with torch.no_grad():
        _, _, m_gpu, _ = gpu_position_grad(model, p.cuda(), dd.cuda(), None, torch.ones(B * T), torch.zeros(B * T, 3))

    def oracle_map(dtype, masks=None, record=None):
        sd = {k: v.to(dtype) for k, v in st.items()}
        xg = p.to(dtype).clone().requires_grad_(True)

        def relu(pre, i):
            if record is not None:
                record.append(pre.detach() > 0)
            return torch.relu(pre) if masks is None else pre * masks[i].to(dtype)
        with torch.enable_grad():
            r, s = O.nerf_forward(sd, xg, dd.to(dtype), None, relu=relu)
            s.sum().backward()
        _, _, w = O.composite(r.detach().reshape(B, T, 3), s.detach().reshape(B, T, 1), z.to(dtype))
        return normals_formula(xg.grad.reshape(B, T, 3), w[..., 0], dtype), w[..., 0].sum(1)

    m_cpu = []
    n32, _ = oracle_map(torch.float32, record=m_cpu)
    n64_cpu, _ = oracle_map(torch.float64, masks=m_cpu)
    n64_gpu, acc64 = oracle_map(torch.float64, masks=m_gpu)
    print(f"hier={hier}/{arith}: oracle opacities {float(acc64.min()):.3f}..{float(acc64.max()):.3f}")
    assert (acc64 > 0.5).all() and (acc64 < 0.99).all(), (float(acc64.min()), float(acc64.max()))
    check_normals_bound(nm.cpu(), n32, n64_gpu, n64_cpu, f"normal map hier={hier}/{arith}")


def test_normals_chunked_matches_one_pass(tmp_path, arith):
    """With NERFMI_MAX_LAUNCH_SAMPLES = 4096 in a child process (the hook is read once), the normals pass
    of a 600-ray 16 + 8 render runs as 4 chunks of 170 rays: the child's normal_map equals this process's
    one-chunk result bit for bit."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import normals_chunked
    from nerfmi import _lib
    ref = normals_chunked.render()
    out = tmp_path / "chunked.pt"
    env = dict(os.environ, NERFMI_MAX_LAUNCH_SAMPLES="4096")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "normals_chunked.py"), str(out), _lib.get_mlp_arith()],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = torch.load(out, weights_only=True)
    assert set(got) == set(ref)
    assert ref["normal_map"].abs().max() > 0
    for k in ref:
        assert torch.equal(got[k], ref[k]), k


def test_cli_save_normals(tmp_path, arith):
    """run.py --mode render --save_normals writes normal_###.png of the frame's size beside the depth, on
    both render branches (whole frame and --chunk) alike; without the flag no such file appears."""
    from PIL import Image
    import run as cli
    base = ["--mode", "render", "--scene", "chair", "--random_init", "0", "--frames", "2", "--width", "16", "--height",
            "16"]
    a, b, c = (str(tmp_path / n) for n in "abc")
    assert cli.main(base + ["--output_dir", a, "--save_normals", "--quality", "preview"]) == 0
    assert cli.main(base + ["--output_dir", b, "--save_normals", "--quality", "preview", "--chunk", "100"]) == 0
    assert cli.main(base + ["--output_dir", c, "--quality", "preview"]) == 0
    for i in range(2):
        img = np.array(Image.open(os.path.join(a, f"normal_{i:03d}.png")))
        assert img.shape == (16, 16, 3) and img.dtype == np.uint8
        assert len(np.unique(img.reshape(-1, 3), axis=0)) > 1, "the normal map is one colour"
        assert np.array_equal(img, np.array(Image.open(os.path.join(b, f"normal_{i:03d}.png"))))
        assert os.path.exists(os.path.join(c, f"rgb_{i:03d}.png"))
    assert not [f for f in os.listdir(c) if f.startswith("normal_")]
