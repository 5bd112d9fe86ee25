"""Time bench_train.py's training step (4,096 rays x 64 samples, fwd + bwd + Adam, one GPU) dense and
with an occupancy grid.  Recorded, not a gate: DESIGN.md §13's table is filled from the output.

    python scripts/bench_train_occupancy.py [--runs 9] [--out profiles/occupancy/train_occupancy.json]

Variants, measured in one process and interleaved round by round (dense, grid 1, grid 2, ... per
round): the dense step; the step under an all-ones grid over [-8, 8]^3, which contains every sample
(the overhead of the path itself and of the per-row weight-gradient route); the step under centred
spheres at G = 128 over [-1.5, 1.5]^3 whose live share of the batch's samples is bisected towards
25 % and 5 % (§12's table).  Every variant has its own Trainer from the same seed and steps on the
same batches.  Per round a variant runs `--steps` whole steps (forward_backward, all_reduce,
optimizer_step) between two host clock reads with the device idle at both: step_ms is wall time per
step, the host wait of the grid path included; after 2 warm-up rounds the median, min and max over
`runs` rounds are kept.  Per variant also:
  live_share     live samples / all samples (Trainer.live_fraction, the last timed step's)
  phases_ms      HIP events inside one step: sample_wait (sample + classify + the packings + the host
                 wait; dense: none), forward (to the end of the composite), backward (composite
                 backward, gather, data gradients, weight gradients)
  kernels_ms     the stage entry points on the step's own live list: mlp_forward, mlp_backward,
                 param_grads (the N = 1 per-row route over M_live rows; dense: Trainer.profile_step)
  vs_dense       step_ms / the dense step_ms of the same run; vs_share_times_dense divides that by
                 the live share
Needs a HIP device.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
BATCH = 4096
G = 128
BOUND = 1.5


def sphere_grid(nerfmi, radius):
    c = (torch.arange(G, device="cuda", dtype=torch.float32) + 0.5) / G * (2 * BOUND) - BOUND
    z, y, x = torch.meshgrid(c, c, c, indexing="ij")
    return nerfmi.OccupancyGrid((-BOUND,) * 3, (BOUND,) * 3, G).from_mask(x * x + y * y + z * z < radius * radius)


def stage_kernels(tr, grid, b, seed):
    """Event-timed gathered forward, data gradients and weight gradients of one step through the stage
    entry points, on the live list nerf_occupancy_classify builds from the step's own samples."""
    from nerfmi import _lib
    from nerfmi.ray_utils import linspace_table
    lib, P, s, dev = tr.lib, _lib.ptr, _lib.stream(), tr.dev
    ck = _lib.check
    N = tr.config.num_samples
    o, d = b["rays_o"].reshape(-1, 3).to(dev).contiguous(), b["rays_d"].reshape(-1, 3).to(dev).contiguous()
    tgt = b["rgb"].reshape(-1, 3).to(dev).contiguous()
    B = o.shape[0]
    M = B * N
    dn, z = torch.empty(B, 3, device=dev), torch.empty(B, N, device=dev)
    feat, encd = torch.empty(B, 256, device=dev), torch.empty(B, 32, device=dev)
    app = tr.appearance_embeddings[int(b["appearance_idx"])].reshape(1, 32)
    ck(lib.nerf_pack_weights(tr.param_ptrs, P(tr.packed), s), "pack")
    ck(lib.nerf_pack_weights_transposed(tr.param_ptrs, P(tr.packedT), s), "packT")
    ck(lib.nerf_normalize_dirs(P(d), B, P(dn), s), "normalize")
    ck(lib.nerf_sample_stratified(P(o), P(dn), B, tr.near, tr.far, N, P(linspace_table(N, dev)), 1, None, seed, P(z),
                                  None, s), "stratified")
    ck(lib.nerf_ray_features_train(P(tr.packed), P(dn), B, P(app), 1, P(feat), P(encd), s), "features")
    live = torch.empty(M, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    cws = torch.empty(lib.nerf_occupancy_classify_workspace_bytes(B, N), dtype=torch.uint8, device=dev)
    ck(lib.nerf_occupancy_classify(P(o), P(dn), P(z), B, N, P(grid.bits), grid.resolution, grid.c_lo(), grid.c_inv(),
                                   P(live), P(count), None, P(cws), cws.numel(), s), "classify")
    k = int(count.item())
    rgb, sigma = torch.zeros(M, 3, device=dev), torch.zeros(M, device=dev)
    rgb_l, sig_l = torch.empty(max(k, 1), 3, device=dev), torch.empty(max(k, 1), device=dev)
    save = torch.empty(_lib.tile_rows(k), _lib.SAVE_ROW, device=dev)
    grad = torch.empty(_lib.tile_rows(k), _lib.GRAD_ROW, device=dev)
    masks = torch.empty(max(k, 1), _lib.MASK_ROW, dtype=torch.int32, device=dev)
    rgb_map, depth = torch.empty(B, 3, device=dev), torch.empty(B, device=dev)
    dsig, drgb, sq = torch.empty(M, device=dev), torch.empty(M, 3, device=dev), torch.empty(B, device=dev)
    grads = [torch.empty_like(tr.view(tr.grad, i)) for i in range(24)]
    gptr = (ctypes.c_void_p * 24)(*[g.data_ptr() for g in grads])
    wsz = lib.nerf_param_grads_workspace_bytes(k)
    ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    cur = torch.cuda.current_stream()
    for _ in range(2):          # the second pass is kept: the first pays the library's one-time set-up
        ev[0].record(cur)
        ck(lib.nerf_mlp_forward_train_live(P(tr.packed), P(o), P(dn), P(z), B, N, P(feat), P(encd), P(live), k, P(rgb),
                                           P(sigma), P(rgb_l), P(sig_l), P(save), P(masks), s), "forward_train_live")
        ev[1].record(cur)
        ck(lib.nerf_composite(P(rgb), P(sigma), P(z), B, N, P(rgb_map), P(depth), None, s), "composite")
        ck(lib.nerf_composite_backward(P(rgb), P(sigma), P(z), P(rgb_map), P(tgt), B, N, 2.0 / (3 * B), P(dsig), P(drgb),
                                       P(sq), s), "composite_backward")
        idx = live[:k].long()
        dsig_l, drgb_l = dsig[idx].contiguous(), drgb[idx].contiguous()
        ev[2].record(cur)
        ck(lib.nerf_mlp_backward(P(tr.packed), P(tr.packedT), P(save), P(masks), P(sig_l), P(rgb_l), P(dsig_l), P(drgb_l),
                                 k, P(grad), s), "mlp_backward")
        ev[3].record(cur)
        ck(lib.nerf_param_grads(P(save), P(grad), k, 1, P(app), 1, P(tr.packed), gptr, P(tr.dapp), P(ws), wsz, s),
           "param_grads")
        ev[4].record(cur)
    torch.cuda.synchronize()
    return {"rows": k, "mlp_forward": ev[0].elapsed_time(ev[1]), "mlp_backward": ev[2].elapsed_time(ev[3]),
            "param_grads": ev[3].elapsed_time(ev[4])}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--steps", type=int, default=4, help="steps per variant and round")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "occupancy", "train_occupancy.json"))
    args = ap.parse_args(argv)
    import nerfmi
    from nerfmi.dataset import SyntheticNeRFDataset
    from nerfmi.train import Trainer

    cfg = nerfmi.Config()
    np.random.seed(100)
    ds = SyntheticNeRFDataset(cfg, n_images=100)
    rounds = args.runs + 2
    batches = [ds.get_rays(batch_size=BATCH) for _ in range(rounds * args.steps + 1)]
    table = ds.appearance_embeddings.detach().clone()

    def trainer(grid):
        torch.manual_seed(0)
        return Trainer(cfg, appearance_embeddings=table.clone(), occupancy=grid)

    def share_of(grid):
        tr = trainer(grid)
        b = batches[0]
        tr.forward_backward(b["rays_o"], b["rays_d"], b["rgb"], b["appearance_idx"], seed=1)
        return tr.live_fraction

    def bisect(target):
        lo_r, hi_r = 0.0, BOUND * 3 ** 0.5
        for _ in range(12):
            mid = 0.5 * (lo_r + hi_r)
            if share_of(sphere_grid(nerfmi, mid)) < target:
                lo_r = mid
            else:
                hi_r = mid
        return 0.5 * (lo_r + hi_r)

    whole = nerfmi.OccupancyGrid((-8.0,) * 3, (8.0,) * 3, G).from_mask(torch.ones(G, G, G, dtype=torch.bool))
    r25, r5 = bisect(0.25), bisect(0.05)
    variants = [("dense", None, None), ("all ones [-8,8]^3", whole, None),
                (f"sphere r={r25:.3f}", sphere_grid(nerfmi, r25), r25), (f"sphere r={r5:.3f}", sphere_grid(nerfmi, r5), r5)]
    trainers = {name: trainer(grid) for name, grid, _ in variants}
    stream = torch.cuda.current_stream()

    def step(tr, b, marks=None):
        if marks is not None:
            marks[0].record(stream)
        tr.forward_backward(b["rays_o"], b["rays_d"], b["rgb"], b["appearance_idx"], seed=tr.steps + 1, _marks=marks)
        if marks is not None:
            marks[2].record(stream)
        tr.all_reduce()
        tr.optimizer_step()

    ms = {name: [] for name, _, _ in variants}
    for rnd in range(rounds):
        for name, _, _ in variants:
            tr = trainers[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                step(tr, batches[rnd * args.steps + i])
            torch.cuda.synchronize()
            if rnd >= 2:
                ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    result = {"batch": [BATCH, cfg.num_samples], "grid_resolution": G, "box": [-BOUND, BOUND], "runs": args.runs,
              "steps_per_round": args.steps, "warmup_rounds": 2, "device": torch.cuda.get_device_name(0),
              "mlp_arith": nerfmi.get_mlp_arith(),
              "timing": "per round every variant runs steps_per_round whole steps (forward_backward, all_reduce, "
                        "optimizer_step) between two host clock reads with the device idle, the dense step and the "
                        "grids interleaved; median [min, max] ms per step over `runs` rounds; phases by HIP events "
                        "inside one further step; kernels through the stage entry points",
              "variants": []}
    dense_ms = statistics.median(ms["dense"])
    last = batches[-1]
    for name, grid, radius in variants:
        tr = trainers[name]
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        step(tr, last, marks)
        torch.cuda.synchronize()
        m = statistics.median(ms[name])
        row = {"name": name, "step_ms": m, "step_ms_min": min(ms[name]), "step_ms_max": max(ms[name]),
               "vs_dense": m / dense_ms}
        if grid is None:
            kt = tr.profile_step(last["rays_o"], last["rays_d"], last["rgb"], last["appearance_idx"])
            row.update(live_share=1.0, sphere_radius=None,
                       phases_ms={"sample_wait": 0.0, "forward": marks[0].elapsed_time(marks[1]),
                                  "backward": marks[1].elapsed_time(marks[2])},
                       kernels_ms={"rows": BATCH * cfg.num_samples, "mlp_forward": kt["mlp_forward_ms"],
                                   "mlp_backward": kt["mlp_backward_ms"], "param_grads": kt["param_grads_ms"]})
        else:
            share = tr.live_fraction
            row.update(live_share=share, sphere_radius=radius, cells_set=grid.fraction(),
                       vs_share_times_dense=m / (share * dense_ms) if share else None,
                       phases_ms={"sample_wait": marks[0].elapsed_time(marks[5]),
                                  "forward": marks[5].elapsed_time(marks[1]),
                                  "backward": marks[1].elapsed_time(marks[2])},
                       kernels_ms=stage_kernels(tr, grid, last, tr.steps + 1))
        result["variants"].append(row)
        k = row["kernels_ms"]
        print(f"{name:20s} {m:7.3f} ms [{row['step_ms_min']:.3f}, {row['step_ms_max']:.3f}]  live {row['live_share']:.4f}  "
              f"x dense {row['vs_dense']:.3f}  phases {row['phases_ms']['sample_wait']:.3f} / "
              f"{row['phases_ms']['forward']:.3f} / {row['phases_ms']['backward']:.3f}  kernels fwd {k['mlp_forward']:.3f} "
              f"bwd {k['mlp_backward']:.3f} wgrad {k['param_grads']:.3f} ({k['rows']} rows)", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
