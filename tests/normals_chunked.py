"""Child of tests/test_gpu_normals.py::test_normals_chunked_matches_one_pass: renders the test's batch
with return_normals=True in this process, whose NERFMI_MAX_LAUNCH_SAMPLES (set by the parent) makes
nerf_render_normals run its pass in several ray chunks, and saves the outputs for the parent."""
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
    model = nerfmi.NeRF(nerfmi.Config())
    with torch.no_grad():                                   # a denser scene: weights well above zero
        model.density_head.weight *= 40.0
        model.density_head.bias *= 40.0
    model = model.cuda().eval()
    g = torch.Generator().manual_seed(17)
    B = 600
    o = torch.randn(B, 3, generator=g) * 0.2
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1)
    with torch.no_grad():
        rgb, depth, ex = nerfmi.render_rays(model, o.cuda(), d.cuda(), 2.0, 6.0, 16, 8, perturb=True, hierarchical=True,
                                            seed=4321, return_normals=True)
    outs = {"rgb": rgb.cpu(), "depth": depth.cpu(), "weights": ex["weights"].cpu(), "z": ex["z_vals"].cpu(),
            "normal_map": ex["normal_map"].cpu()}
    if out_path:
        torch.save(outs, out_path)
    return outs


if __name__ == "__main__":
    render(sys.argv[1], sys.argv[2])
