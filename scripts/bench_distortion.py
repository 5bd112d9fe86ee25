"""Time the distortion loss against the unchanged training steps.  Recorded, not a gate:
§16's table is filled from the output.

    python scripts/bench_distortion.py [--rounds 9] [--out profiles/distortion/distortion.json]

One process, the two variants of a group interleaved round by round after 2 warm-up rounds; the judge of
a variant is the unchanged path of the same group in the same run.

  train     the 4,096-ray step at 64 samples (dense) and at 64 + 128 (hierarchical), forward_backward +
            all_reduce + Adam: the default Trainer against Trainer(distortion_weight=0.01).  `--steps` steps
            per round and variant between two HIP events; ms per step.

Reported per variant: median [min, max] over the rounds, and whether the variant's median lies within the
judge's own min-max spread (if not, by how much it leaves it).

For information only, no assertion: `--quality_steps` hierarchical steps of 1,024 rays on the
teacher-rendered synthetic scene from one seed, with and without the weight, then the colour PSNR of the
last 10 steps and the mean distortion loss of the fine weights on one fixed batch of the scene's rays.
Needs a HIP device.
"""
import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
BATCH, N_COARSE, N_FINE = 4096, 64, 128
WEIGHT = 0.01


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9, help="timed rounds per variant (after 2 warm-up rounds)")
    ap.add_argument("--steps", type=int, default=4, help="training steps per round and variant")
    ap.add_argument("--quality_steps", type=int, default=200, help="steps of the before-and-after record (0: skip)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "distortion", "distortion.json"))
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    import nerfmi
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

    np.random.seed(100)
    cfg = nerfmi.Config()
    cfg.num_samples = N_COARSE
    ds = SyntheticNeRFDataset(cfg, n_images=100)
    n_batches = (args.rounds + 2) * args.steps
    batches = [ds.get_rays(batch_size=BATCH) for _ in range(n_batches)]
    table = ds.appearance_embeddings.detach().clone()

    def trainer(**kw):
        torch.manual_seed(0)
        c = nerfmi.Config()
        c.num_samples = N_COARSE
        return Trainer(c, appearance_embeddings=table.clone(), near=ds.near, far=ds.far, **kw)

    cursor = {}

    def steps_of(tr, name):
        def run():
            at = cursor.get(name, 0)
            for i in range(args.steps):
                b = batches[(at + i) % n_batches]
                tr.step(b["rays_o"], b["rays_d"], b["rgb"], b["appearance_idx"], seed=tr.steps + 1)
            cursor[name] = at + args.steps
        return run

    dk = dict(distortion_weight=WEIGHT)
    hk = dict(hierarchical=True, n_importance=N_FINE)
    groups = {
        "train dense 4096 x 64": (args.steps, [("default", steps_of(trainer(), "d0")),
                                               ("distortion_weight=0.01", steps_of(trainer(**dk), "d1"))]),
        "train hierarchical 4096 x (64 + 128)": (args.steps, [("default", steps_of(trainer(**hk), "h0")),
                                                              ("distortion_weight=0.01", steps_of(trainer(**hk, **dk), "h1"))]),
    }
    result = {"device": torch.cuda.get_device_name(0), "mlp_arith": nerfmi.get_mlp_arith(), "rounds": args.rounds,
              "steps_per_round": args.steps, "distortion_weight": WEIGHT,
              "timing": "two HIP events around `steps_per_round` whole steps; the variants of a group alternate round "
                        "by round in one process after 2 warm-up rounds; ms per step",
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
            outside = max(0.0, med - max(judge), min(judge) - med)
            rows.append({"name": name, "ms": med, "ms_min": t[0], "ms_max": t[-1],
                         "median_within_judge_spread": bool(outside == 0.0), "ms_outside_judge_spread": outside})
            print(f"{gname:40s} {name:24s} {med:9.3f} ms [{t[0]:.3f}, {t[-1]:.3f}]"
                  f"  outside the judge's spread by {outside:.3f} ms", flush=True)
        result["groups"].append({"name": gname, "variants": rows, "ratio": rows[1]["ms"] / rows[0]["ms"]})

    # ------------------------------------------------ for information: depth-smear before and after
    if args.quality_steps > 0:
        record = []
        for dw in (0.0, WEIGHT):
            np.random.seed(7)
            torch.manual_seed(7)
            qds = SyntheticNeRFDataset(cfg, n_images=8, H=64, W=64)
            fixed = qds.get_rays(batch_size=1024)
            torch.manual_seed(0)
            c = nerfmi.Config()
            c.num_samples = N_COARSE
            tr = Trainer(c, appearance_embeddings=qds.appearance_embeddings, near=qds.near, far=qds.far,
                         **(dict(distortion_weight=dw) if dw else {}), **hk)
            colour = []
            for i in range(args.quality_steps):
                b = qds.get_rays(batch_size=1024)
                tr.step(b["rays_o"], b["rays_d"], b["rgb"], b["appearance_idx"], seed=i + 1)
                colour.append(float(tr.loss_parts[0]))
            with torch.no_grad():
                app = tr.appearance_embeddings[int(fixed["appearance_idx"])]
                _, _, extras = nerfmi.volume_render(tr.model, fixed["rays_o"].cuda(), fixed["rays_d"].cuda(), tr.near, tr.far,
                                                    N_COARSE, N_FINE, appearance_embedding=app, perturb=False,
                                                    hierarchical=True)
                ell = nerfmi.distortion_loss(extras["weights"], extras["z_vals"], tr.near, tr.far)
            mse = statistics.mean(colour[-10:])
            record.append({"distortion_weight": dw, "steps": args.quality_steps,
                           "colour_psnr_last10": -10.0 * math.log10(mse), "mean_distortion_fixed_batch": float(ell.mean())})
            print(f"distortion_weight {dw:g}: colour PSNR (last 10 steps) {record[-1]['colour_psnr_last10']:.2f} dB, "
                  f"mean l on the fixed batch {record[-1]['mean_distortion_fixed_batch']:.4e}", flush=True)
        result["for_information"] = {"what": "hierarchical 64 + 128 steps of 1,024 rays on the teacher-rendered synthetic "
                                             "scene (8 images of 64 x 64) from one seed; no assertion", "runs": record}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
