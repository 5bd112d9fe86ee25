"""Time the hierarchical training step (4,096 rays x (64 coarse + 128 fine), fwd + bwd + Adam, one GPU)
against the coarse step on the same number of samples in one part (4,096 x 192).  Recorded, not a gate:
DESIGN.md §14's table is filled from the output.

    python scripts/bench_train_hier.py [--steps 60] [--out profiles/hier/train_hier.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/bench_train_hier.py --trace-steps 10
    python scripts/rocpd_summary.py DIR/run_results.db --csv stats.csv
    python scripts/bench_train_hier.py --kernel-stats stats.csv --trace-steps 10 --out profiles/hier/kernel_split.json

Timed run: two Trainers from the same seed on the same batches, the hierarchical one and the coarse one at
num_samples = 192 (the same MLP work in one sample set, the existing step), alternating in rounds of
`--round` steps after 2 warm-up rounds.  Every step (forward_backward, all_reduce, optimizer_step) sits
between two HIP events on the stream; a third event marks the end of the forward.  Reported per variant:
the median, min, max and the 10th / 90th percentile of the step in ms over `--steps` steps, rays/s from the
median, the forward / backward split, and the ratio of the medians.

Trace run (--trace-steps K, under rocprofv3, profiler overhead included so no end-to-end number is taken
from it): 2 warm-up steps and K hierarchical steps, nothing else.  --kernel-stats groups the resulting
per-kernel totals into forward, composite and resample, data gradients, weight gradients and the rest,
per step.  Needs a HIP device (except --kernel-stats).
"""
import argparse
import csv
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
BATCH, N_COARSE, N_FINE = 4096, 64, 128

# kernel-name fragments -> phase (first match wins)
SETUP = "dataset set-up (not the step)"       # the teacher scene's render, once per run
PHASES = [
    (SETUP, ("mlp16s_kernel", "get_rays_kernel", "normalize_kernel")),
    ("composite and resample", ("composite_merged_backward_kernel", "composite_backward_kernel", "composite_kernel",
                                "importance_kernel", "loss_kernel", "stratified")),
    ("sum of the two parts", ("add_segments_kernel",)),
    ("data gradients", ("mlp_backward",)),
    ("forward", ("mlp16_kernel", "mlp_kernel", "ray_feature")),
    ("weight gradients", ("wgrad", "ray_sums", "app_grad", "reduce")),
    ("packing and Adam", ("pack", "adam", "scale16", "scaleT16", "stats")),
]


def phase_of(name):
    for phase, frags in PHASES:
        if any(f in name for f in frags):
            return phase
    return "other"


def kernel_split(path, steps, warmup=2):
    """Per-step kernel time by phase from a rocpd_summary.py CSV of a --trace-steps run (its 2 warm-up
    steps ran the same kernels: totals are divided by steps + warmup)."""
    phases, kernels = {}, []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "nerf::" not in row["Name"]:
                continue
            ms = float(row["TotalDurationNs"]) / 1e6 / (steps + warmup)
            ph = phase_of(row["Name"])
            phases[ph] = phases.get(ph, 0.0) + ms
            kernels.append({"kernel": row["Name"].split("(")[0], "phase": ph, "calls_per_step":
                            int(row["Calls"]) / (steps + warmup), "ms_per_step": ms})
    in_step = sum(ms for ph, ms in phases.items() if ph != SETUP)
    return {"steps": steps, "warmup": warmup, "phases_ms_per_step": phases, "kernel_ms_per_step": in_step,
            "note": "kernel time summed over both of param_grads' streams, which overlap: more than the step's wall time",
            "kernels": kernels}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60, help="timed steps per variant (at least 50)")
    ap.add_argument("--round", type=int, default=10, help="steps a variant runs before the other takes over")
    ap.add_argument("--trace-steps", type=int, default=0, help="hierarchical steps only, for a kernel trace")
    ap.add_argument("--kernel-stats", default=None, help="a rocpd_summary.py CSV of a --trace-steps run to group")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hier", "train_hier.json"))
    args = ap.parse_args(argv)
    if args.kernel_stats:
        result = kernel_split(args.kernel_stats, args.trace_steps or 10)
        for ph, ms in sorted(result["phases_ms_per_step"].items(), key=lambda kv: -kv[1]):
            print(f"{ph:24s} {ms:8.3f} ms / step")
        return write(args.out, result)
    if not args.trace_steps and args.steps < 50:
        ap.error("--steps: at least 50 timed steps")
    import numpy as np
    import torch
    import nerfmi
    from nerfmi.dataset import SyntheticNeRFDataset
    from nerfmi.train import Trainer

    def config(n):
        cfg = nerfmi.Config()
        cfg.num_samples = n
        return cfg

    np.random.seed(100)
    ds = SyntheticNeRFDataset(config(N_COARSE), n_images=100)
    rounds = 2 + -(-args.steps // args.round)
    n_batches = (args.trace_steps + 2) if args.trace_steps else rounds * args.round
    batches = [ds.get_rays(batch_size=BATCH) for _ in range(n_batches)]
    table = ds.appearance_embeddings.detach().clone()

    def trainer(hier):
        torch.manual_seed(0)
        if hier:
            return Trainer(config(N_COARSE), appearance_embeddings=table.clone(), hierarchical=True, n_importance=N_FINE)
        return Trainer(config(N_COARSE + N_FINE), appearance_embeddings=table.clone())

    stream = torch.cuda.current_stream()

    def step(tr, b, marks=None):
        if marks is not None:
            marks[0].record(stream)
        tr.forward_backward(b["rays_o"], b["rays_d"], b["rgb"], b["appearance_idx"], seed=tr.steps + 1, _marks=marks)
        tr.all_reduce()
        tr.optimizer_step()
        if marks is not None:
            marks[2].record(stream)

    if args.trace_steps:
        tr = trainer(True)
        for b in batches:
            step(tr, b)
        torch.cuda.synchronize()
        print(f"traced {args.trace_steps} hierarchical steps after 2 warm-up steps; fine mse {float(tr.loss_parts[0]):.5f}")
        return 0
    variants = [("hierarchical 64 + 128", trainer(True)), ("coarse 192", trainer(False))]
    times = {name: [] for name, _ in variants}
    for rnd in range(rounds):
        for name, tr in variants:
            marks = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.round)]
            for i in range(args.round):
                step(tr, batches[rnd * args.round + i], marks[i])
            torch.cuda.synchronize()
            if rnd >= 2:
                times[name] += [(m[0].elapsed_time(m[2]), m[0].elapsed_time(m[1]), m[1].elapsed_time(m[2])) for m in marks]
    result = {"batch": [BATCH, N_COARSE, N_FINE], "device": torch.cuda.get_device_name(0), "mlp_arith": nerfmi.get_mlp_arith(),
              "timing": "per step two HIP events around forward_backward + all_reduce + optimizer_step and one at the end "
                        "of the forward; the two variants alternate in rounds of `round` steps after 2 warm-up rounds, in "
                        "one process on the same batches; ms per step",
              "round": args.round, "variants": []}
    for name, tr in variants:
        t = sorted(x[0] for x in times[name])[:]
        med = statistics.median(t)
        q = statistics.quantiles(t, n=10)
        row = {"name": name, "steps": len(t), "step_ms": med, "step_ms_min": t[0], "step_ms_max": t[-1], "step_ms_p10": q[0],
               "step_ms_p90": q[-1], "rays_per_s": BATCH / med * 1e3,
               "forward_ms": statistics.median(x[1] for x in times[name]),
               "backward_adam_ms": statistics.median(x[2] for x in times[name])}
        result["variants"].append(row)
        print(f"{name:24s} {med:7.3f} ms [{t[0]:.3f}, {t[-1]:.3f}] p10 {q[0]:.3f} p90 {q[-1]:.3f}  {row['rays_per_s'] / 1e6:.3f} M rays/s  "
              f"forward {row['forward_ms']:.3f}  backward + Adam {row['backward_adam_ms']:.3f}  ({len(t)} steps)", flush=True)
    result["hier_over_coarse192"] = result["variants"][0]["step_ms"] / result["variants"][1]["step_ms"]
    print(f"hierarchical / coarse 192: {result['hier_over_coarse192']:.3f}")
    return write(args.out, result)


def write(path, result):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
