"""Time the post effects (nerfmi.PostProcessor) and the Gaussian blur alone on one device-resident
800x800 frame.  Recorded, not a gate: DESIGN.md's effects table is filled from the output.

    python scripts/bench_effects.py [--size 800] [--runs 30] [--inner 10] [--out profiles/effects/effects_800.json]

Per entry: every shape is warmed up first; one run is `inner` back-to-back calls on device tensors
between two HIP events (so a call's launches queue behind the previous call's and the figure is
the steady-state time per call, not one call's enqueue latency); the result is the median over
`runs` runs, with min and max.  The noise of Film Grain and Hologram is on the device beforehand
(a host draw of 1.9 M normals would be all one measured).  `bytes` is what the algorithm has to
move (inputs read once, the output written once), computed from the shapes; GB/s is bytes over the
median, against the 8 TB/s HBM peak.  Needs a HIP device: there is no CPU path to time.
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
FRAME_MS = 291.37          # the 800x800 hierarchical frame itself (BENCH_r06.json, ms_per_step)
HBM_GBS = 8000.0


def timed(fn, runs, inner):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return statistics.median(ms), min(ms), max(ms)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "effects", "effects_800.json"))
    args = ap.parse_args(argv)
    if args.runs < 20:
        ap.error("--runs must be at least 20")
    import nerfmi
    from nerfmi.post_processor import depth_percentile, gaussian_blur
    S = args.size
    P = S * S
    g = torch.Generator(device="cuda").manual_seed(0)
    img = torch.randint(0, 256, (S, S, 3), generator=g, device="cuda", dtype=torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(S, device="cuda"), torch.arange(S, device="cuda"), indexing="ij")
    depth = (0.2 + 0.6 * xx / S + 0.1 * torch.rand(S, S, generator=g, device="cuda")).float().contiguous()
    depth[S // 4: 3 * S // 4, S // 3: 2 * S // 3] = 0.05
    grain = torch.randn(S, S, 3, generator=g, device="cuda") * 50
    flicker = torch.randn(S, S, 3, generator=g, device="cuda") * 0.03
    spans = [(S // 5, 3), (S // 2, 5), (S - 2, 4)]

    def effect(name, **params):
        pp = nerfmi.PostProcessor()
        pp.current_effect = name
        pp.params.update(params)
        return pp

    fog, toon, vig, cross, post = (effect(n) for n in ("Fog", "Toon Shader", "Vignette", "Cross Processing",
                                                        "Posterize"))
    fg, holo, sk = effect("Film Grain"), effect("Hologram"), effect("Pencil Sketch")
    img_b, depth_b, noise_b = 3 * P, 4 * P, 12 * P
    entries = [        # name, callable, algorithmic bytes (image in + out, + depth, + noise)
        ("Fog (depth)", lambda: fog.apply_effect(img, depth), 2 * img_b + depth_b),
        ("Toon Shader (depth)", lambda: toon.apply_effect(img, depth), 2 * img_b + depth_b),
        ("Vignette", lambda: vig.apply_effect(img), 2 * img_b),
        ("Cross Processing", lambda: cross.apply_effect(img), 2 * img_b),
        ("Posterize", lambda: post.apply_effect(img), 2 * img_b),
        ("Film Grain", lambda: fg._effect_film_grain(img, noise=grain), 2 * img_b + noise_b),
        ("Hologram (no depth)", lambda: holo._effect_hologram(img, None, noise=flicker, spans=spans),
         2 * img_b + noise_b),
        ("Hologram (depth)", lambda: holo._effect_hologram(img, depth, noise=flicker, spans=spans),
         2 * img_b + noise_b + depth_b),
        ("Pencil Sketch (no depth)", lambda: sk.apply_effect(img), 2 * img_b),
        ("Pencil Sketch (depth)", lambda: sk.apply_effect(img, depth), 2 * img_b + depth_b),
        ("depth_percentile q=70", lambda: depth_percentile(depth, 70), depth_b),
    ]
    for size in (3, 15, 51):
        e = effect("Bloom", bloom_size=size)
        entries.append((f"Bloom size {size}", lambda e=e: e.apply_effect(img), 2 * img_b))
    for k in (3, 15, 21, 51, 63):
        entries.append((f"blur k={k} (3 channels)", lambda k=k: gaussian_blur(img, k), 2 * img_b))
    gray = img[:, :, 0].contiguous()
    entries.append(("blur k=21 (1 channel)", lambda: gaussian_blur(gray, 21), 2 * P))

    rows = []
    for name, fn, nbytes in entries:
        med, lo, hi = timed(fn, args.runs, args.inner)
        rows.append({"name": name, "ms": med, "ms_min": lo, "ms_max": hi, "bytes": nbytes,
                     "gb_per_s": nbytes / med / 1e6, "frac_of_hbm_peak": nbytes / med / 1e6 / HBM_GBS,
                     "frac_of_frame": med / FRAME_MS})
        print(f"{name:28s} {med:8.4f} ms  [{lo:.4f}, {hi:.4f}]  {nbytes / 1e6:7.2f} MB  {nbytes / med / 1e6:8.1f} GB/s  "
              f"{100 * med / FRAME_MS:6.3f} % of the frame", flush=True)
    result = {"size": [S, S], "runs": args.runs, "calls_per_run": args.inner, "warmup_calls": 3,
              "timing": "HIP events around `calls_per_run` back-to-back PostProcessor calls on device tensors; "
                        "median over `runs`",
              "device": torch.cuda.get_device_name(0), "frame_ms": FRAME_MS, "hbm_peak_gb_per_s": HBM_GBS,
              "effects": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
