"""Child of tests/test_gpu_background.py::test_chunked_render_with_background_equals_one_launch: renders
the test's batch in this process, whose NERFMI_MAX_LAUNCH_SAMPLES (set by the parent) makes
nerf_render_rays_bg and nerf_render_rays_occ_bg split the call into ray chunks, and saves the outputs
for the parent."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def render(out_path=None, arith=None):
    import nerfmi
    if arith:
        nerfmi.set_mlp_arith(arith)
    torch.manual_seed(0)
    model = nerfmi.NeRF(nerfmi.Config()).cuda().eval().requires_grad_(False)
    g = torch.Generator().manual_seed(7)
    B = 300
    o = torch.randn(B, 3, generator=g) * 0.2
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1)
    bg = torch.rand(B, 3, generator=g)                     # one background colour per ray
    grid = nerfmi.OccupancyGrid((-8.0,) * 3, (8.0,) * 3, 8)
    mask = torch.zeros(8, 8, 8, dtype=torch.bool)
    mask[:, :, :5] = True
    grid.from_mask(mask)
    outs = {}
    with torch.no_grad():
        for name, occ in (("plain", None), ("grid", grid)):
            kw = {} if occ is None else {"occupancy": occ}
            rgb, depth, ex = nerfmi.render_rays(model, o.cuda(), d.cuda(), 2.0, 6.0, 32, 40, perturb=True,
                                                hierarchical=True, seed=1234, ray_offset=5, background=bg.cuda(),
                                                background_depth=6.0, **kw)
            for k, v in (("rgb", rgb), ("depth", depth), ("acc", ex["acc_map"]), ("acc_c", ex["acc_map_coarse"]),
                         ("rgb_c", ex["rgb_map_coarse"]), ("depth_c", ex["depth_map_coarse"]),
                         ("weights", ex["weights"])):
                outs[f"{k}_{name}"] = v.cpu()
    if out_path:
        torch.save(outs, out_path)
    return outs


if __name__ == "__main__":
    render(sys.argv[1], sys.argv[2])
