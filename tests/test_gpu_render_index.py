"""The render MLP's sample and ray indices (csrc/mlp16s_body.h: the 32-bit block loop, the sample -> ray
division by a multiply-high, csrc/sample_index.h) at the smallest shapes where they can go wrong.

Every case checks the kernel's outputs two ways: against the CPU oracle at the suite's 1e-4, and bit
for bit against the same samples evaluated by one launch per ray, where every ray is ray 0 of its
launch and every sample sits in the first block (position independence, as
test_gpu_parity.py::test_forward_ragged_and_position_independent states it).  The cases:
  * N in {1, 7, 33} with 40 rays: a wave's 32 samples span rays, the per-sample feature rows;
  * N = 32 and 64 with M = R N not a multiple of the 128-sample block, and M < 128: the tail clamp;
  * 520 rays x 64 = 33,280 samples, 260 blocks: on 256 compute units the first workgroups run two
    blocks and the rest one;
  * a hierarchical render (the fine pass writes through out_slot), at 64 + 128 and at 33 + 40;
  * a render with an occupancy grid whose live list skips whole rays and splits others mid-wave.
The kernel under test is the split-f16 one: the module runs under f16x3."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
import occupancy_restated as R
from test_gpu_occupancy import HI, LO, close, grid_of, mlp_all, staged_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nerfmi_mod():
    import nerfmi
    return nerfmi


@pytest.fixture(scope="module", autouse=True)
def f16x3(nerfmi_mod):
    prev = nerfmi_mod.set_mlp_arith("f16x3")
    yield
    nerfmi_mod.set_mlp_arith(prev)


@pytest.fixture(scope="module")
def lib(nerfmi_mod):
    from nerfmi import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def model(nerfmi_mod, ref_state):
    m = nerfmi_mod.NeRF(nerfmi_mod.Config())
    m.load_state_dict(ref_state)
    return m.cuda().eval().requires_grad_(False)


@pytest.fixture(scope="module")
def rays(golden):
    f1 = golden("f1_get_rays.npz")
    return torch.from_numpy(f1["chair_o"]).contiguous(), torch.from_numpy(f1["chair_d"]).contiguous()


# (rays, samples per ray)
MLP_CASES = [(40, 1), (40, 7), (40, 33),          # waves span rays
             (5, 32), (3, 64), (3, 32), (1, 64),  # M = 160, 192 (tails of 32 and 64), 96 and 64 (< 128)
             (520, 64)]                            # 260 blocks: two for the first workgroups


@pytest.mark.parametrize("B,N", MLP_CASES)
def test_mlp_rows_by_position_and_against_the_oracle(lib, model, ref_state, rays, B, N):
    o, d = rays[0][:B].cuda(), rays[1][:B].cuda()
    packed, dn, z, feat = staged_inputs(lib, model, o, d, N)
    rgb, sigma = mlp_all(lib, packed, o, dn, z, feat)
    # one launch per ray
    one = [mlp_all(lib, packed, o[r:r + 1], dn[r:r + 1], z[r:r + 1], feat[r:r + 1]) for r in range(B)]
    rgb_1, sigma_1 = torch.cat([a for a, _ in one]), torch.cat([b for _, b in one])
    assert not bool(torch.isnan(rgb).any()) and not bool(torch.isnan(sigma).any())   # (mlp_all poisons with NaN)
    assert torch.equal(rgb, rgb_1) and torch.equal(sigma, sigma_1)
    # the oracle on its own samples (bit-equal to the GPU's)
    dn_o = O.normalize(rays[1][:B])
    z_o, pts = O.sample_stratified(rays[0][:B], dn_o, 2.0, 6.0, N)
    assert torch.equal(dn.cpu(), dn_o) and torch.equal(z.cpu(), z_o)
    with torch.no_grad():
        rgb_o, sigma_o = O.nerf_forward(ref_state, pts.reshape(-1, 3), dn_o.unsqueeze(1).expand(-1, N, -1).reshape(-1, 3))
    close(rgb, rgb_o, "rgb")
    close(sigma.reshape(-1, 1), sigma_o, "sigma")


@pytest.mark.parametrize("N,Nf", [(64, 128), (33, 40)])
def test_hierarchical_render_by_position_and_against_the_oracle(nerfmi_mod, model, ref_state, rays, app_vec, N, Nf):
    B = 24
    o, d = rays[0][:B].cuda(), rays[1][:B].cuda()
    u = torch.rand(B, Nf, generator=torch.Generator().manual_seed(31))

    def render(sl):
        with torch.no_grad():
            return nerfmi_mod.render_rays(model, o[sl], d[sl], 2.0, 6.0, N, Nf, appearance_embedding=app_vec.cuda(),
                                          perturb=False, hierarchical=True, u_rand=u[sl])[:2]
    rgb, depth = render(slice(0, B))
    one = [render(slice(r, r + 1)) for r in range(B)]
    assert torch.equal(rgb, torch.cat([a for a, _ in one])) and torch.equal(depth, torch.cat([b for _, b in one]))
    rgb_o, depth_o, _ = O.render_rays_h1(ref_state, rays[0][:B], rays[1][:B], 2.0, 6.0, N, Nf, app_vec, None, u)
    close(rgb, rgb_o, "rgb")
    close(depth, depth_o, "depth")


def test_occupancy_render_by_position_and_against_the_oracle(nerfmi_mod, model, ref_state, rays, app_vec):
    """48 rays x 33 samples through the gathered kernel.  Every fourth ray starts far outside the grid's
    box, so the live list skips it whole; the others leave the box part of the way, so a wave's 32
    list entries start and end inside rays."""
    B, N, G = 48, 33, 32
    o, d = rays[0][:B].clone(), rays[1][:B].clone()
    o[::4] += 100.0
    mask = R.sphere_mask(G, 0.3)
    dn = O.normalize(d)
    z, pts = O.sample_stratified(o, dn, 2.0, 6.0, N)
    live = R.classify(o, dn, z, LO, HI, G, mask)
    per_ray = live.sum(1)
    assert bool((per_ray[::4] == 0).all()) and bool(((per_ray > 0) & (per_ray < N)).any())
    starts = (torch.cumsum(per_ray, 0) - per_ray)[per_ray > 0]
    assert bool((starts % 32 != 0).any()) and int(per_ray.sum()) > 128      # rays split mid-wave, several blocks
    grid = grid_of(nerfmi_mod, mask)

    def render(sl):
        with torch.no_grad():
            rgb, depth, ex = nerfmi_mod.volume_render(model, o[sl].cuda(), d[sl].cuda(), 2.0, 6.0, N, 0,
                                                      appearance_embedding=app_vec.cuda(), perturb=False,
                                                      occupancy=grid)
        return rgb, depth, ex["weights"]
    got = render(slice(0, B))
    one = [render(slice(r, r + 1)) for r in range(B)]
    for k, name in enumerate(("rgb", "depth", "weights")):
        assert torch.equal(got[k], torch.cat([t[k] for t in one])), name
    with torch.no_grad():
        rgb_s, sigma_s = O.nerf_forward(ref_state, pts.reshape(-1, 3), dn.unsqueeze(1).expand(-1, N, -1).reshape(-1, 3),
                                        app_vec.unsqueeze(0).expand(B * N, -1))
    sigma_m = torch.where(live.unsqueeze(-1), sigma_s.reshape(B, N, 1), torch.zeros(B, N, 1))
    rgb_o, depth_o, w_o = O.composite(rgb_s.reshape(B, N, 3), sigma_m, z)
    close(got[0], rgb_o, "rgb")
    close(got[1], depth_o, "depth")
    close(got[2], w_o, "weights")
    assert bool((got[2].squeeze(-1).cpu()[~live] == 0).all())
