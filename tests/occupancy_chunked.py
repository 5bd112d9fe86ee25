"""Child of tests/test_gpu_occupancy.py::test_chunked_call_equals_the_one_launch_call: renders the
test's batch with an occupancy grid in this process, whose NERFMI_MAX_LAUNCH_SAMPLES (set by the
parent) makes nerf_render_rays_occ split the call into ray chunks, and saves the outputs."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def render(out_path=None):
    import nerfmi
    import occupancy_restated as R
    torch.manual_seed(0)
    model = nerfmi.NeRF(nerfmi.Config()).cuda().eval()
    g = torch.Generator().manual_seed(7)
    B = 3000
    o = torch.randn(B, 3, generator=g) * 0.2
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1)
    app = torch.randn(B, 32, generator=g)                  # one appearance row per ray
    grid = nerfmi.OccupancyGrid((-4.5, -4.3, -4.7), (4.6, 4.9, 4.4), 16).from_mask(torch.from_numpy(R.checker_mask(16)))
    with torch.no_grad():
        rgb, depth, ex = nerfmi.render_rays(model, o.cuda(), d.cuda(), 2.0, 6.0, 64, 128, appearance_embedding=app.cuda(),
                                            perturb=True, hierarchical=True, seed=1234, ray_offset=5, occupancy=grid)
    outs = {"rgb": rgb.cpu(), "depth": depth.cpu(), "weights": ex["weights"].cpu(), "z": ex["z_vals"].cpu(),
            "rgb_c": ex["rgb_map_coarse"].cpu()}
    if out_path:
        torch.save(outs, out_path)
    return outs


if __name__ == "__main__":
    render(sys.argv[1])
