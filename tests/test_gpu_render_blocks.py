"""The render MLP's persistent block loop (csrc/mlp16s.hip): a workgroup per CU runs sample blocks of
128 in rounds, so results must not depend on how many blocks a launch has, on which round, workgroup or
lane a sample lands in, or on what the launch before left behind.

G = the device's CU count; one block is 128 samples."""
import pytest
import torch

from oracle import nerf_oracle as O
from test_gpu_parity import close

pytestmark = pytest.mark.gpu

BLOCK = 128


@pytest.fixture(scope="module")
def nerfmi_mod():
    import nerfmi
    return nerfmi


@pytest.fixture(scope="module", autouse=True, params=["f16x3", "f32"])
def arith(request, nerfmi_mod):
    prev = nerfmi_mod.set_mlp_arith(request.param)
    yield request.param
    nerfmi_mod.set_mlp_arith(prev)


@pytest.fixture(scope="module")
def model(nerfmi_mod, ref_state):
    m = nerfmi_mod.NeRF(nerfmi_mod.Config())
    m.load_state_dict(ref_state)
    return m.cuda().eval().requires_grad_(False)


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def points(cus):
    """Sample positions and directions for the largest case, shared by the tests (never modified)."""
    n = BLOCK * (3 * cus + 1) + 37
    torch.manual_seed(21)
    x = torch.randn(n, 3) * 2
    d = torch.nn.functional.normalize(torch.randn(n, 3), dim=-1)
    return x, d


@pytest.fixture(scope="module")
def oracle_subset(points, ref_state):
    """The oracle's forward on a fixed 4,096-sample subset of `points`, computed once."""
    x, d = points
    torch.manual_seed(22)
    idx = torch.randperm(x.shape[0])[:4096].sort().values
    rgb, sigma = O.nerf_forward(ref_state, x[idx], d[idx])
    return idx, rgb, sigma


def forward(model, x, d):
    with torch.no_grad():
        rgb, sigma = model(x.cuda(), d.cuda())
    return rgb, sigma


def block_counts(G):
    return (1, 100, BLOCK * G - 5, BLOCK * G, BLOCK * G + 1, BLOCK * (3 * G + 1) + 37)


@pytest.mark.parametrize("case", range(6))
def test_block_counts_around_the_grid(model, points, oracle_subset, ref_state, cus, case):
    """Fewer blocks than workgroups, exactly one each, one workgroup with two, several rounds with a
    ragged tail."""
    M = block_counts(cus)[case]
    x, d = points[0][:M], points[1][:M]
    rgb, sigma = forward(model, x, d)
    assert rgb.shape == (M, 3) and sigma.shape == (M, 1)
    assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(sigma).all())
    if M <= 4096:   # the whole case is its subset
        rgb_o, sigma_o = O.nerf_forward(ref_state, x, d)
        close(rgb, rgb_o, what=f"rgb M={M}")
        close(sigma, sigma_o, what=f"sigma M={M}")
    else:
        idx, rgb_o, sigma_o = oracle_subset
        keep = idx < M
        close(rgb[idx[keep].cuda()], rgb_o[keep], what=f"rgb M={M}")
        close(sigma[idx[keep].cuda()], sigma_o[keep], what=f"sigma M={M}")
    rgb_r, sigma_r = forward(model, x.flip(0), d.flip(0))
    assert torch.equal(rgb_r.flip(0), rgb) and torch.equal(sigma_r.flip(0), sigma), M


def test_position_independence_across_rounds(model, points, cus):
    """Every sample changes round, workgroup and lane under a rotation by 128 G + 32."""
    M = BLOCK * 2 * cus + 64
    x, d = points[0][:M], points[1][:M]
    rgb, sigma = forward(model, x, d)
    k = BLOCK * cus + 32
    rgb_r, sigma_r = forward(model, x.roll(-k, 0), d.roll(-k, 0))
    assert torch.equal(rgb_r.roll(k, 0), rgb) and torch.equal(sigma_r.roll(k, 0), sigma)
    one_rgb, one_sigma = forward(model, x[:1], d[:1])
    assert torch.equal(one_rgb, rgb[:1]) and torch.equal(one_sigma, sigma[:1])


@pytest.mark.parametrize("N,Nf", [(64, 128), (32, 32), (7, 5)])
def test_render_waves_on_and_off_ray_boundaries(nerfmi_mod, model, ref_state, app_vec, cus, N, Nf):
    """Hierarchical, perturbed render of 2 G + 3 rays: N % 32 == 0 takes the per-ray feature DMA, N = 7
    the global-read path.  Against the oracle, and bit for bit against two calls split at ray G + 1."""
    from nerfmi import cameras
    B = 2 * cus + 3
    o, d = nerfmi_mod.get_rays(800, 800, cameras.synthetic_focal(800), cameras.frame_c2w("chair").cuda())
    first = 392 * 800 + 100
    o = o.reshape(-1, 3)[first:first + B].cpu()
    d = d.reshape(-1, 3)[first:first + B].cpu()
    torch.manual_seed(23)
    t, u = torch.rand(B, N), torch.rand(B, Nf)

    def render(lo, hi):
        with torch.no_grad():
            rgb, depth, _ = nerfmi_mod.render_rays(model, o[lo:hi].cuda(), d[lo:hi].cuda(), 2.0, 6.0, N, Nf,
                                                   appearance_embedding=app_vec.cuda(), perturb=True,
                                                   hierarchical=True, t_rand=t[lo:hi], u_rand=u[lo:hi])
        return rgb, depth

    rgb, depth = render(0, B)
    r_ref, d_ref, _ = O.render_rays_h1(ref_state, o, d, 2.0, 6.0, N, Nf, app_vec, t, u)
    close(rgb, r_ref, what=f"rgb N={N} Nf={Nf}")
    close(depth, d_ref, what=f"depth N={N} Nf={Nf}")
    split = cus + 1
    (rgb_a, depth_a), (rgb_b, depth_b) = render(0, split), render(split, B)
    assert torch.equal(torch.cat([rgb_a, rgb_b]), rgb) and torch.equal(torch.cat([depth_a, depth_b]), depth)


def test_back_to_back_launches_leave_no_state(model, points):
    """Two identical calls on one stream with nothing between them."""
    x, d = points[0].cuda(), points[1].cuda()
    with torch.no_grad():
        rgb1, sigma1 = model(x, d)
        rgb2, sigma2 = model(x, d)
    assert torch.equal(rgb1, rgb2) and torch.equal(sigma1, sigma2)
