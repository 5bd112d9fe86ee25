"""Time the 800x800 frame of bench.py (same pose, weights and appearance row) with and without an
occupancy grid.  Recorded, not a gate: DESIGN.md §12's table is filled from the output.

    python scripts/bench_occupancy.py [--runs 9] [--out profiles/occupancy/occupancy_800.json]

Modes: coarse (64 samples) and hierarchical (64 + 128).  Grids at G = 128: all ones over [-8, 8]^3
(every sample live: the overhead of the path itself), and over [-1.5, 1.5]^3 all ones, centred
spheres whose live share of the coarse samples is bisected towards 25 % and 5 %, and the from_model
grid of the bench model.  Per mode the plain frame and every grid are measured in the
same process, interleaved round by round (plain, grid 1, grid 2, ... per round): one frame between
two HIP events, the MLP launches' own events through nerf_profile_mlp_*; after 2 warm-up rounds
the median, min and max over `runs` rounds are kept.  Per grid:
  ms          the frame
  mlp_ms      the MLP launches of the frame (2 in the hierarchical mode)
  other_ms    ms - mlp_ms: everything else; its excess over the plain frame's is the classify +
              zero-fill cost (classify_ms)
  live_share  live samples / all samples of the frame, from nerf_occupancy_classify's count on the
              frame's own z (the merged N + Nf samples in the hierarchical mode)
Needs a HIP device.
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
H = W = 800
N_COARSE, N_FINE = 64, 128
G = 128
BOUND = 1.5


def sphere_grid(nerfmi, radius):
    c = (torch.arange(G, device="cuda", dtype=torch.float32) + 0.5) / G * (2 * BOUND) - BOUND
    z, y, x = torch.meshgrid(c, c, c, indexing="ij")
    return nerfmi.OccupancyGrid((-BOUND,) * 3, (BOUND,) * 3, G).from_mask(x * x + y * y + z * z < radius * radius)


def live_share(grid, o, dn, z):
    from nerfmi import _lib
    lib = _lib.load()
    B, n = z.shape
    live = torch.empty(B * n, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.nerf_occupancy_classify_workspace_bytes(B, n), dtype=torch.uint8, device="cuda")
    _lib.check(lib.nerf_occupancy_classify(_lib.ptr(o), _lib.ptr(dn), _lib.ptr(z), B, n, _lib.ptr(grid.bits),
                                           grid.resolution, grid.c_lo(), grid.c_inv(), _lib.ptr(live),
                                           _lib.ptr(count), None, _lib.ptr(ws), ws.numel(), _lib.stream()),
               "nerf_occupancy_classify")
    return int(count.item()) / (B * n)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "occupancy", "occupancy_800.json"))
    args = ap.parse_args(argv)
    import nerfmi
    from nerfmi import _lib, cameras, frames
    from nerfmi.ray_utils import rays_on_device

    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    model = nerfmi.NeRF(nerfmi.Config()).to(dev).eval().requires_grad_(False)
    torch.manual_seed(1)
    app = torch.randn(100, 32)[0].to(dev)
    focal = cameras.synthetic_focal(W)
    pose = cameras.frame_c2w("chair", "circle", frame=0, num_frames=120)
    o, d = rays_on_device(H, W, focal, pose, (0, H), dev)
    o = o.contiguous()
    dn = torch.nn.functional.normalize(d, dim=-1)
    z_c, _ = nerfmi.sample_stratified(o, dn, 2.0, 6.0, N_COARSE, perturb=False)

    def bisect(target):
        lo_r, hi_r = 0.0, BOUND * 3 ** 0.5
        for _ in range(14):
            mid = 0.5 * (lo_r + hi_r)
            if live_share(sphere_grid(nerfmi, mid), o, dn, z_c) < target:
                lo_r = mid
            else:
                hi_r = mid
        return 0.5 * (lo_r + hi_r)

    ones = nerfmi.OccupancyGrid((-BOUND,) * 3, (BOUND,) * 3, G).from_mask(torch.ones(G, G, G, dtype=torch.bool))
    r25, r5 = bisect(0.25), bisect(0.05)
    with torch.no_grad():
        learned = nerfmi.OccupancyGrid.from_model(model, (-BOUND,) * 3, (BOUND,) * 3, resolution=G)
    # every sample of the 2..6 segment lies in [-8, 8]^3: all samples live, the pure overhead of the path
    whole = nerfmi.OccupancyGrid((-8.0,) * 3, (8.0,) * 3, G).from_mask(torch.ones(G, G, G, dtype=torch.bool))
    grids = [("plain", None, None), ("all ones [-8,8]^3", whole, None), ("all ones", ones, None),
             (f"sphere r={r25:.3f}", sphere_grid(nerfmi, r25), r25), (f"sphere r={r5:.3f}", sphere_grid(nerfmi, r5), r5),
             ("from_model", learned, None)]

    @torch.no_grad()
    def frame(grid, hier, seed):
        return frames.render_path_frames(model, [pose], H, W, focal, 2.0, 6.0, N_COARSE, N_FINE if hier else 0,
                                         appearance_embedding=app, perturb=True, hierarchical=hier, seed=seed,
                                         occupancy=grid)

    result = {"size": [H, W], "samples": [N_COARSE, N_FINE], "grid_resolution": G, "box": [-BOUND, BOUND],
              "runs": args.runs, "warmup_rounds": 2, "device": torch.cuda.get_device_name(0),
              "mlp_arith": nerfmi.get_mlp_arith(),
              "timing": "per round every variant renders one frame between two HIP events, the plain frame and the "
                        "grids interleaved; MLP launches by nerf_profile_mlp_*; median [min, max] over `runs` rounds",
              "modes": {}}
    for mode, hier in (("coarse", False), ("hierarchical", True)):
        ms = {name: [] for name, _, _ in grids}
        mlp = {name: [] for name, _, _ in grids}
        for rnd in range(args.runs + 2):
            for name, grid, _ in grids:
                _lib.profile_mlp_begin(16)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                frame(grid, hier, rnd)
                b.record()
                b.synchronize()
                launches = _lib.profile_mlp_end(16)
                if rnd >= 2:
                    ms[name].append(a.elapsed_time(b))
                    mlp[name].append(sum(t for t, _ in launches))
        rows = []
        plain_ms, plain_mlp = statistics.median(ms["plain"]), statistics.median(mlp["plain"])
        for name, grid, radius in grids:
            m, k = statistics.median(ms[name]), statistics.median(mlp[name])
            row = {"name": name, "ms": m, "ms_min": min(ms[name]), "ms_max": max(ms[name]), "mlp_ms": k,
                   "mlp_ms_min": min(mlp[name]), "mlp_ms_max": max(mlp[name]), "other_ms": m - k}
            if grid is not None:
                with torch.no_grad():
                    _, _, ex = nerfmi.render_rays(model, o, d, 2.0, 6.0, N_COARSE, N_FINE if hier else 0,
                                                  appearance_embedding=app, perturb=True, hierarchical=hier,
                                                  seed=args.runs + 1, occupancy=grid)
                share = live_share(grid, o, dn, ex["z_vals"].contiguous())
                row.update(live_share=share, cells_set=grid.fraction(), sphere_radius=radius,
                           classify_ms=(m - k) - (plain_ms - plain_mlp), frame_vs_plain=m / plain_ms,
                           mlp_vs_plain=k / plain_mlp, mlp_vs_share_times_plain=k / (share * plain_mlp) if share else None)
            rows.append(row)
            print(f"{mode:12s} {name:18s} {m:8.2f} ms [{row['ms_min']:.2f}, {row['ms_max']:.2f}]  mlp {k:8.2f}  "
                  f"other {m - k:6.2f}" + (f"  live {row['live_share']:.4f}  mlp/(share*plain) "
                                           f"{row['mlp_vs_share_times_plain'] or float('nan'):.3f}" if grid is not None else ""),
                  flush=True)
        result["modes"][mode] = rows
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
