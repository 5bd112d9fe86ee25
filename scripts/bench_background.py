"""Time the opacity map and background options against the unchanged paths.  Recorded,
not a gate: §15's table is filled from the output.

    python scripts/bench_background.py [--rounds 9] [--out profiles/background/background.json]

One process, every variant of a group interleaved round by round after 2 warm-up rounds; the judge of a
variant is the unchanged path of the same group in the same run.

  render    the 800 x 800 frame at 64 + 128 (hierarchical, in-kernel draws, one appearance row): plain
            nerf_render_rays, against nerf_render_rays_bg with a background colour, a background depth and
            both opacity outputs.  One frame per round and variant, between two HIP events.
  train     the 4,096-ray step at 64 samples (dense) and at 64 + 128 (hierarchical), forward_backward +
            all_reduce + Adam: the default Trainer against Trainer(background="random", acc_weight=0.01)
            with a per-ray alpha.  `--steps` steps per round and variant between two HIP events; ms per step.

Reported per variant: median [min, max] over the rounds, and whether the variant's median lies within the
judge's own min-max spread.  Needs a HIP device.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
BATCH, N_COARSE, N_FINE, SIDE = 4096, 64, 128, 800


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9, help="timed rounds per variant (after 2 warm-up rounds)")
    ap.add_argument("--steps", type=int, default=4, help="training steps per round and variant")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "background", "background.json"))
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    import nerfmi
    from nerfmi import cameras
    from nerfmi.dataset import SyntheticNeRFDataset
    from nerfmi.train import Trainer

    stream = torch.cuda.current_stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    groups = {}
    # ---------------------------------------------------------------- render
    torch.manual_seed(0)
    model = nerfmi.NeRF(nerfmi.Config()).cuda().eval().requires_grad_(False)
    torch.manual_seed(1)
    app = torch.randn(100, 32)[0].cuda()
    o, d = nerfmi.get_rays(SIDE, SIDE, cameras.synthetic_focal(SIDE), cameras.frame_c2w("chair").cuda())
    o, d = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()

    def frame(**kw):
        with torch.no_grad():
            nerfmi.render_rays(model, o, d, 2.0, 6.0, N_COARSE, N_FINE, appearance_embedding=app, perturb=True,
                               hierarchical=True, seed=3, **kw)

    groups["render 800^2 64+128"] = (1, [
        ("plain", lambda: frame()),
        ("background + depth + acc", lambda: frame(background=(1.0, 1.0, 1.0), background_depth=6.0, return_acc=True)),
    ])
    # ----------------------------------------------------------------- train
    np.random.seed(100)
    cfg = nerfmi.Config()
    cfg.num_samples = N_COARSE
    ds = SyntheticNeRFDataset(cfg, n_images=100)
    n_batches = (args.rounds + 2) * args.steps
    batches = [ds.get_rays(batch_size=BATCH) for _ in range(n_batches)]
    g = torch.Generator().manual_seed(5)
    alphas = [torch.rand(BATCH, generator=g).cuda() for _ in range(n_batches)]
    table = ds.appearance_embeddings.detach().clone()

    def trainer(**kw):
        torch.manual_seed(0)
        c = nerfmi.Config()
        c.num_samples = N_COARSE
        return Trainer(c, appearance_embeddings=table.clone(), **kw)

    cursor = {}

    def steps_of(tr, name, with_alpha):
        def run():
            at = cursor.get(name, 0)
            for i in range(args.steps):
                b = batches[(at + i) % n_batches]
                kw = {"alpha": alphas[(at + i) % n_batches]} if with_alpha else {}
                tr.step(b["rays_o"], b["rays_d"], b["rgb"], b["appearance_idx"], seed=tr.steps + 1, **kw)
            cursor[name] = at + args.steps
        return run

    bgk = dict(background="random", acc_weight=0.01)
    hk = dict(hierarchical=True, n_importance=N_FINE)
    groups["train dense 4096 x 64"] = (args.steps, [
        ("default", steps_of(trainer(), "d0", False)),
        ("background=random", steps_of(trainer(**bgk), "d1", True)),
    ])
    groups["train hierarchical 4096 x (64 + 128)"] = (args.steps, [
        ("default", steps_of(trainer(**hk), "h0", False)),
        ("background=random", steps_of(trainer(**hk, **bgk), "h1", True)),
    ])
    result = {"device": torch.cuda.get_device_name(0), "mlp_arith": nerfmi.get_mlp_arith(), "rounds": args.rounds,
              "steps_per_round": args.steps,
              "timing": "two HIP events around one frame / `steps_per_round` whole steps; the variants of a group "
                        "alternate round by round in one process after 2 warm-up rounds; ms per frame / per step",
              "groups": []}
    for gname, (per, variants) in groups.items():
        times = {name: [] for name, _ in variants}
        for rnd in range(args.rounds + 2):
            for name, fn in variants:
                ms = timed(fn) / per
                if rnd >= 2:
                    times[name].append(ms)
        judge = times[variants[0][0]]
        rows = []
        for name, _ in variants:
            t = sorted(times[name])
            med = statistics.median(t)
            rows.append({"name": name, "ms": med, "ms_min": t[0], "ms_max": t[-1],
                         "median_within_judge_spread": bool(min(judge) <= med <= max(judge))})
            print(f"{gname:40s} {name:28s} {med:9.3f} ms [{t[0]:.3f}, {t[-1]:.3f}]"
                  f"  within the judge's spread: {rows[-1]['median_within_judge_spread']}", flush=True)
        result["groups"].append({"name": gname, "variants": rows, "ratio": rows[1]["ms"] / rows[0]["ms"]})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
