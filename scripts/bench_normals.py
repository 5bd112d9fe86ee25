"""What the normal map costs: on bench.py's 800 x 800 frame, at 64 and at 64 + 128
samples a ray, in one process and interleaved round by round:

  plain     frames.render_path_frames of the frame (bench.py's step)
  normals   the same with return_normals=True
  phases    one chunk of the normals pass (the 2^18 samples nerf_render_normals runs at a time) through the
            staged C calls, HIP events between them: ray features + forward with saves, data-gradient chain,
            position gradient, composite

Each figure is the median with [min, max] over the rounds.  The judge is the plain frame of the same run;
the position-gradient kernel's time stands beside nerf_mlp_backward's on the same M.  Writes one JSON
file (default profiles/normals/normals_800.json) and prints it.  Needs the GPU: there is no fallback.

    python scripts/bench_normals.py [--rounds 7] [--warmup 2] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

H = W = 800
N_COARSE, N_FINE = 64, 128
CHUNK_SAMPLES = 1 << 18


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def frame_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


class Phases:
    """One chunk of the normals pass on the frame's first rays, stage by stage."""

    def __init__(self, model, o, d, T):
        from nerfmi import _lib
        from nerfmi.autograd import packed_pair
        from nerfmi.normals import packed_input_for
        self.lib, self.L = _lib.load(), _lib
        dev = o.device
        self.T = T
        self.B = B = CHUNK_SAMPLES // T
        self.M = M = B * T
        self.packed, self.packedT = packed_pair(model)
        self.packed_in = packed_input_for(model)
        self.o = o[:B].contiguous()
        self.dn = torch.nn.functional.normalize(d[:B], dim=-1).contiguous()
        self.z = torch.linspace(2.0, 6.0, T, device=dev).repeat(B, 1).contiguous()
        self.w = torch.full((B, T), 1.0 / T, device=dev)
        MT = _lib.tile_rows(M)
        self.feat, self.encd = torch.empty(B, 256, device=dev), torch.empty(B, 32, device=dev)
        self.rgb, self.sigma = torch.empty(M, 3, device=dev), torch.empty(M, device=dev)
        self.save, self.grad = torch.empty(MT, _lib.SAVE_ROW, device=dev), torch.empty(MT, _lib.GRAD_ROW, device=dev)
        self.masks = torch.empty(M, _lib.MASK_ROW, dtype=torch.int32, device=dev)
        self.dsig, self.drgb = torch.ones(M, device=dev), torch.zeros(M, 3, device=dev)
        self.dx, self.nm = torch.empty(M, 3, device=dev), torch.empty(B, 3, device=dev)

    def run(self):
        lib, L, P, s = self.lib, self.L, self.L.ptr, self.L.stream()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        L.check(lib.nerf_ray_features_train(P(self.packed), P(self.dn), self.B, None, 0, P(self.feat), P(self.encd), s),
                "nerf_ray_features_train")
        L.check(lib.nerf_mlp_forward_train(P(self.packed), P(self.o), P(self.dn), P(self.z), self.B, self.T,
                                           P(self.feat), P(self.encd), P(self.rgb), P(self.sigma), P(self.save),
                                           P(self.masks), s), "nerf_mlp_forward_train")
        ev[1].record()
        L.check(lib.nerf_mlp_backward(P(self.packed), P(self.packedT), P(self.save), P(self.masks), P(self.sigma),
                                      P(self.rgb), P(self.dsig), P(self.drgb), self.M, P(self.grad), s),
                "nerf_mlp_backward")
        ev[2].record()
        L.check(lib.nerf_mlp_position_grad(P(self.packed_in), P(self.save), P(self.grad), self.M, P(self.dx), s),
                "nerf_mlp_position_grad")
        ev[3].record()
        L.check(lib.nerf_composite_normals(P(self.dx), P(self.w), self.B, self.T, P(self.nm), s),
                "nerf_composite_normals")
        ev[4].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "normals", "normals_800.json"))
    args = ap.parse_args()
    import nerfmi
    from nerfmi import _lib, cameras, frames
    dev = _lib.device()
    torch.manual_seed(0)
    model = nerfmi.NeRF(nerfmi.Config()).to(dev).eval().requires_grad_(False)
    torch.manual_seed(1)
    app = torch.randn(100, 32)[0].to(dev)
    focal = cameras.synthetic_focal(W)
    pose = cameras.frame_c2w("chair", "circle", frame=0, num_frames=120)
    o, d = nerfmi.get_rays(H, W, focal, pose.to(dev))
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    names = ("forward_with_saves", "data_gradient_chain", "position_gradient", "composite_normals")
    result = {"frame": [H, W], "arith": _lib.get_mlp_arith(), "rounds": args.rounds, "chunk_samples": CHUNK_SAMPLES,
              "device": torch.cuda.get_device_name(dev), "cases": {}}
    for nf in (0, N_FINE):
        T = N_COARSE + nf

        @torch.no_grad()
        def frame(i, normals):
            return frames.render_path_frames(model, [pose], H, W, focal, 2.0, 6.0, N_COARSE, nf, appearance_embedding=app,
                                             perturb=True, hierarchical=bool(nf), seed=i,
                                             **({"return_normals": True} if normals else {}))
        ph = Phases(model, o, d, T)
        for i in range(args.warmup):
            frame(i, False), frame(i, True), ph.run()
        plain, withn, phases = [], [], []
        for i in range(args.rounds):
            plain.append(frame_ms(lambda: frame(100 + i, False)))
            withn.append(frame_ms(lambda: frame(100 + i, True)))
            phases.append(ph.run())
        chunks = -(-(H * W) // ph.B)
        case = {"samples_per_ray": T, "plain_frame_ms": summary(plain), "normals_frame_ms": summary(withn),
                "normals_over_plain": statistics.median(withn) / statistics.median(plain),
                "chunk": {"rays": ph.B, "samples": ph.M, "chunks_per_frame": chunks,
                          "phase_ms": {n: summary([p[k] for p in phases]) for k, n in enumerate(names)}}}
        pm = case["chunk"]["phase_ms"]
        case["chunk"]["position_gradient_over_data_gradient_chain"] = (pm["position_gradient"]["median"] /
                                                                       pm["data_gradient_chain"]["median"])
        result["cases"][f"{N_COARSE}+{nf}"] = case
        del ph
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
