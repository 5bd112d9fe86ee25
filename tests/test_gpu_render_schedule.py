"""The render MLP's schedule (csrc/mlp16s.hip: half-quarter side work, the weight DMA's piece
assignment) leaves its results alone: the kernel is deterministic over more blocks than workgroups,
its two entries agree bit for bit, and a small hierarchical render still matches the oracle.

f16x3 only: the f32 kernel (csrc/mlp.hip) has no part in it.  Sizes: 128 (2 G + 1) + 37 samples
(G = the device's CU count) give every workgroup of the persistent grid two or three 128-sample
blocks, so the block loop's wrap of the weight stream runs, and a ragged last block.
"""
import ctypes
import os
import sys

import pytest
import torch

from conftest import REPO
from oracle import nerf_oracle as O

sys.path.insert(0, os.path.join(REPO, "tests"))
from test_gpu_parity import close   # noqa: E402

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
def model(nerfmi_mod, ref_state):
    m = nerfmi_mod.NeRF(nerfmi_mod.Config())
    m.load_state_dict(ref_state)
    return m.cuda().eval().requires_grad_(False)


@pytest.fixture(scope="module")
def samples():
    """(x, d) of 128 (2 G + 1) + 37 samples, on the device."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m = 128 * (2 * cus + 1) + 37
    g = torch.Generator().manual_seed(81)
    x = torch.rand(m, 3, generator=g) * 4 - 2
    d = torch.nn.functional.normalize(torch.randn(m, 3, generator=g), dim=-1)
    return x.cuda(), d.cuda()


def test_repeated_forward_is_bit_identical(model, samples):
    """Eight identical calls: a ring slot published before one of its pieces has landed would show
    as values that differ from call to call."""
    x, d = samples
    with torch.no_grad():
        first = model(x, d)
        for k in range(7):
            rgb, sigma = model(x, d)
            assert torch.equal(rgb, first[0]) and torch.equal(sigma, first[1]), f"call {k + 2} differs"
    assert bool(torch.isfinite(first[0]).all()) and bool(torch.isfinite(first[1]).all())


def test_plain_entry_equals_the_gathered_entry(nerfmi_mod, model, samples):
    """nerf_mlp_forward against nerf_mlp_forward_live with the identity list, on the same samples
    (each a ray of one sample at z = 0 from the sample's position): the two kernels share their text."""
    from nerfmi import _lib
    from nerfmi.render import packed_for
    lib = _lib.load()
    x, d = samples
    m = x.shape[0]
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    S = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    packed = packed_for(model)
    z = torch.zeros(m, 1, device="cuda")
    feat = torch.empty(m, 256, device="cuda")
    assert lib.nerf_ray_features(P(packed), P(d), m, None, 0, P(feat), S) == 0, lib.nerf_last_error()
    rgb = torch.full((m, 3), float("nan"), device="cuda")
    sigma = torch.full((m,), float("nan"), device="cuda")
    assert lib.nerf_mlp_forward(P(packed), P(x), P(d), P(z), m, 1, P(feat), P(rgb), P(sigma), None, 0, S) == 0, \
        lib.nerf_last_error()
    live = torch.arange(m, dtype=torch.int32, device="cuda")
    count = torch.tensor([m], dtype=torch.int32, device="cuda")
    rgb_l = torch.full((m, 3), float("nan"), device="cuda")
    sigma_l = torch.full((m,), float("nan"), device="cuda")
    assert lib.nerf_mlp_forward_live(P(packed), P(x), P(d), P(z), m, 1, P(feat), P(live), P(count), P(rgb_l),
                                     P(sigma_l), S) == 0, lib.nerf_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(sigma).all())
    assert torch.equal(rgb, rgb_l) and torch.equal(sigma, sigma_l)
    # and the module's call on the same samples runs the plain entry: the same bits
    with torch.no_grad():
        rgb_m, sigma_m = model(x, d)
    assert torch.equal(rgb_m, rgb) and torch.equal(sigma_m.reshape(-1), sigma)


@pytest.mark.parametrize("n,nf", [(64, 128), (7, 5)])
def test_small_perturbed_hierarchical_render(nerfmi_mod, model, ref_state, app_vec, golden, n, nf):
    f1 = golden("f1_get_rays.npz")
    o, d = torch.from_numpy(f1["chair_o"])[:3], torch.from_numpy(f1["chair_d"])[:3]
    g = torch.Generator().manual_seed(1000 * n + nf)
    t = torch.rand(3, n, generator=g)
    u = torch.rand(3, nf, generator=g)
    rgb, depth, ex = nerfmi_mod.render_rays(model, o.cuda(), d.cuda(), 2.0, 6.0, n, nf,
                                            appearance_embedding=app_vec.cuda(), perturb=True, hierarchical=True,
                                            t_rand=t, u_rand=u)
    r_ref, d_ref, ex_ref = O.render_rays_h1(ref_state, o, d, 2.0, 6.0, n, nf, app_vec, t, u)
    close(ex["rgb_map_coarse"], ex_ref["rgb_map_coarse"], what=f"coarse rgb ({n}, {nf})")
    close(rgb, r_ref, what=f"fine rgb ({n}, {nf})")
    close(depth, d_ref, what=f"fine depth ({n}, {nf})")
