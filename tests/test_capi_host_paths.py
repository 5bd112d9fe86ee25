"""The host layer of libnerfmi.so pinned against recordings (CPU, no launch): the exact workspace
sizes of every carve, and the (return code, nerf_last_error()) of every argument check of the render
and training entry points that exist with and without an occupancy grid.

Both tables are recorded results (tests/golden/host_workspace_bytes.json, host_error_parity.json):
    NERFMI_LIB=<the build to record from> python tests/test_capi_host_paths.py
rewrites them.  Every call below passes fake non-null pointers, so each one must fail a check or hit
its empty-batch return before anything is launched: a call that would pass every check is left out
(see the notes in error_cases), and the test refuses a recording that holds a HIP error."""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden")

RENDER_SHAPES = [(1, 1, 0), (37, 7, 0), (37, 7, 5), (256, 64, 128), (640000, 64, 128), (1 << 25, 64, 128)]
TRAIN_SHAPES = [(1, 1), (37, 7), (100, 40), (256, 64), (4096, 64)]
CLASSIFY_SHAPES = [(1, 1), (37, 7), (1000, 7)]


def workspace_sizes(lib):
    out = {}
    for B, N, Nf in RENDER_SHAPES:
        out[f"nerf_render_workspace_bytes({B},{N},{Nf})"] = lib.nerf_render_workspace_bytes(B, N, Nf)
        out[f"nerf_render_occ_workspace_bytes({B},{N},{Nf})"] = lib.nerf_render_occ_workspace_bytes(B, N, Nf)
    for B, N in TRAIN_SHAPES:
        out[f"nerf_train_workspace_bytes({B},{N})"] = lib.nerf_train_workspace_bytes(B, N)
        out[f"nerf_train_occ_workspace_bytes({B},{N})"] = lib.nerf_train_occ_workspace_bytes(B, N)
        out[f"nerf_param_grads_workspace_bytes({B * N})"] = lib.nerf_param_grads_workspace_bytes(B * N)
    for B, n in CLASSIFY_SHAPES:
        out[f"nerf_occupancy_classify_workspace_bytes({B},{n})"] = lib.nerf_occupancy_classify_workspace_bytes(B, n)
    return out


P = 0x1000            # a fake device pointer: never dereferenced by a check
B, N, NF = 4, 8, 5
F32, F16X3 = 0, 1


def error_cases(lib):
    """{case name: [return code, message]}.  One valid call per entry point, one argument made bad at
    a time.  The valid call itself is never made, and as a second guard every mutated call but the
    ones a host table refuses also carries a workspace one byte short (nerf_param_grads: no workspace
    at all), so a mutation that slipped past its check would end at the workspace check, not at a
    launch.  (The composite stage's entry points take no workspace: there the refused check, or the
    empty batch's return in front of the launch, is the only end.)  Left out because they pass every check: null for the optional pointers (t_rand, u_rand,
    weights_out, z_out, coarse_*, dapp); N = 4097 for nerf_mlp_forward_live (no upper bound on N);
    the f32 setting for the entries that run under both arithmetics; B == 0 for nerf_train_occ_sample
    (it then clears the caller's live count on the device); nerf_param_grads with a workspace one
    byte short (it still holds both streams' partial buffers)."""
    lo = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
    inv = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    grads = (ctypes.c_void_p * 24)(*([P] * 24))
    grads_hole = (ctypes.c_void_p * 24)(*([P] * 3 + [0] + [P] * 20))
    out = {}

    def run(entry, order, base, name, **change):
        args = dict(base, **change)
        rc = getattr(lib, entry)(*[args[k] for k in order])
        out[f"{entry}: {name}"] = [rc, lib.nerf_last_error().decode() if rc else ""]

    def sweep(entry, order, base, required, changes, f32_only=False):
        for p in required:
            run(entry, order, base, f"{p} null", **{p: None})
        for name, change in changes:
            run(entry, order, base, name, **change)
        if f32_only:
            prev = lib.nerf_set_mlp_arith(F32)
            try:
                run(entry, order, base, "under f32")
            finally:
                lib.nerf_set_mlp_arith(prev)

    shape = [("B = -1", dict(B=-1)), ("N = 0", dict(N=0)), ("N = 4097", dict(N=4097)), ("B = 0", dict(B=0))]
    grid = [("G = 0", dict(G=0)), ("G = 1025", dict(G=1025))]
    live = [("M_live = -1", dict(M_live=-1)), ("M_live = B*N + 1", dict(M_live=B * N + 1))]
    many = ("2^32 samples", dict(B=1 << 20, N=4096))

    # ---- the single-call render, without and with a grid
    order = ["packed", "rays_o", "rays_d", "B", "near", "far", "N", "Nf", "t_vals", "u_lin", "perturb", "t_rand",
             "u_rand", "seed", "ray0", "app", "app_rows", "rgb_map", "depth_map", "weights_out", "z_out", "coarse_rgb",
             "coarse_depth", "workspace", "ws_bytes", "stream"]
    base = dict(packed=P, rays_o=P, rays_d=P, B=B, near=2.0, far=6.0, N=N, Nf=NF, t_vals=P, u_lin=P, perturb=1,
                t_rand=P, u_rand=P, seed=7, ray0=0, app=P, app_rows=1, rgb_map=P, depth_map=P, weights_out=P, z_out=P,
                coarse_rgb=P, coarse_depth=P, workspace=P, stream=None)
    required = ["packed", "rays_o", "rays_d", "t_vals", "u_lin", "app", "rgb_map", "depth_map", "workspace"]
    changes = shape + [("ray0 = -1", dict(ray0=-1)), ("Nf = -1", dict(Nf=-1)), ("Nf = 1025", dict(Nf=1025)),
                       ("N = 257 with Nf", dict(N=257)), ("app_rows = 2", dict(app_rows=2)),
                       ("workspace one byte short", {})]
    sweep("nerf_render_rays", order, dict(base, ws_bytes=lib.nerf_render_workspace_bytes(B, N, NF) - 1), required,
          changes)
    i = order.index("rgb_map")
    order = order[:i] + ["bits", "G", "lo", "inv"] + order[i:]
    base = dict(base, bits=P, G=16, lo=lo, inv=inv, ws_bytes=lib.nerf_render_occ_workspace_bytes(B, N, NF) - 1)
    sweep("nerf_render_rays_occ", order, base, required + ["bits", "lo", "inv"], changes + grid)

    # ---- the dense training step
    order = ["packed", "rays_o", "rays_d", "B", "near", "far", "N", "t_vals", "perturb", "t_rand", "seed", "app",
             "app_rows", "rgb_map", "depth_map", "weights_out", "z_out", "workspace", "ws_bytes", "stream"]
    ws_bytes = lib.nerf_train_workspace_bytes(B, N)
    base = dict(packed=P, rays_o=P, rays_d=P, B=B, near=2.0, far=6.0, N=N, t_vals=P, perturb=1, t_rand=P, seed=7, app=P,
                app_rows=1, rgb_map=P, depth_map=P, weights_out=P, z_out=P, workspace=0x100000, ws_bytes=ws_bytes - 1,
                stream=None)
    sweep("nerf_train_forward", order, base,
          ["packed", "rays_o", "rays_d", "t_vals", "app", "rgb_map", "depth_map", "workspace"],
          shape + [("app_rows = 2", dict(app_rows=2)), many, ("workspace one byte short", {})])
    order = ["packed", "packedT", "rgb_map", "target", "B", "N", "app", "app_rows", "grads", "dapp", "loss", "workspace",
             "ws_bytes", "stream"]
    base = dict(packed=P, packedT=P, rgb_map=P, target=P, B=B, N=N, app=P, app_rows=1, grads=grads, dapp=P, loss=P,
                workspace=0x100000, ws_bytes=ws_bytes - 1, stream=None)
    backward_ptrs = ["packed", "packedT", "rgb_map", "target", "app", "grads", "loss", "workspace"]
    sweep("nerf_train_backward", order, base, backward_ptrs,
          shape + [("app_rows = 2", dict(app_rows=2)), ("gradient 3 null", dict(grads=grads_hole)),
                   ("workspace one byte short", {}), ("no forward wrote the workspace", dict(ws_bytes=ws_bytes))])

    # ---- the training step with a grid
    ws_bytes = lib.nerf_train_occ_workspace_bytes(B, N)
    order = ["rays_o", "rays_d", "B", "near", "far", "N", "t_vals", "perturb", "t_rand", "seed", "bits", "G", "lo",
             "inv", "live_count", "workspace", "ws_bytes", "stream"]
    base = dict(rays_o=P, rays_d=P, B=B, near=2.0, far=6.0, N=N, t_vals=P, perturb=1, t_rand=P, seed=7, bits=P, G=16,
                lo=lo, inv=inv, live_count=P, workspace=0x200000, ws_bytes=ws_bytes - 1, stream=None)
    sweep("nerf_train_occ_sample", order, base,
          ["rays_o", "rays_d", "t_vals", "bits", "lo", "inv", "live_count", "workspace"],
          shape[:3] + grid + [many, ("workspace one byte short", {})])
    order = ["packed", "rays_o", "B", "N", "M_live", "app", "app_rows", "rgb_map", "depth_map", "weights_out", "z_out",
             "workspace", "ws_bytes", "stream"]
    base = dict(packed=P, rays_o=P, B=B, N=N, M_live=5, app=P, app_rows=1, rgb_map=P, depth_map=P, weights_out=P,
                z_out=P, workspace=0x200000, ws_bytes=ws_bytes - 1, stream=None)
    occ_step = shape[:3] + [("B = 0", dict(B=0, M_live=0))] + live + [("app_rows = -1", dict(app_rows=-1)), ("app_rows = 2", dict(app_rows=2)), many,
                               ("workspace one byte short", {})]
    sweep("nerf_train_occ_forward", order, base, ["packed", "rays_o", "app", "rgb_map", "depth_map", "workspace"],
          occ_step, f32_only=True)
    order = ["packed", "packedT", "rgb_map", "target", "B", "N", "M_live", "app", "app_rows", "grads", "dapp", "loss",
             "workspace", "ws_bytes", "stream"]
    base = dict(packed=P, packedT=P, rgb_map=P, target=P, B=B, N=N, M_live=5, app=P, app_rows=1, grads=grads, dapp=P,
                loss=P, workspace=0x200000, ws_bytes=ws_bytes - 1, stream=None)
    sweep("nerf_train_occ_backward", order, base, backward_ptrs,
          occ_step + [("gradient 3 null", dict(grads=grads_hole)),
                      ("no forward with this M_live wrote the workspace", dict(ws_bytes=ws_bytes))], f32_only=True)

    # ---- the stage entry points
    order = ["save", "grad", "M", "N", "app", "app_rows", "packed", "grads", "dapp", "workspace", "ws_bytes", "stream"]
    base = dict(save=P, grad=P, M=B * N, N=N, app=P, app_rows=1, packed=P, grads=grads, dapp=P, workspace=P, ws_bytes=0,
                stream=None)
    sweep("nerf_param_grads", order, base, ["save", "grad", "app", "packed", "grads", "workspace"],
          [("M = -1", dict(M=-1)), ("N = 0", dict(N=0)), ("N = 4097", dict(N=4097)), ("app_rows = 2", dict(app_rows=2)),
           ("gradient 3 null", dict(grads=grads_hole)), ("M = 0", dict(M=0)), ("no workspace", {})])
    order = ["packed", "origins", "dirs", "z_vals", "R", "N", "ray_feat", "live", "live_count", "rgb", "sigma", "stream"]
    base = dict(packed=P, origins=P, dirs=P, z_vals=P, R=B, N=N, ray_feat=P, live=P, live_count=P, rgb=P, sigma=P,
                stream=None)
    sweep("nerf_mlp_forward_live", order, base,
          ["packed", "origins", "dirs", "z_vals", "ray_feat", "live", "live_count", "rgb", "sigma"],
          [("R = -1", dict(R=-1)), ("N = 0", dict(N=0)), ("R = 0", dict(R=0)), ("2^34 samples", dict(R=1 << 22, N=4096))],
          f32_only=True)
    order = ["packed", "origins", "dirs", "z_vals", "R", "N", "ray_feat", "enc_d", "live", "M_live", "rgb", "sigma",
             "rgb_live", "sigma_live", "save", "masks", "stream"]
    base = dict(packed=P, origins=P, dirs=P, z_vals=P, R=B, N=N, ray_feat=P, enc_d=P, live=P, M_live=5, rgb=P, sigma=P,
                rgb_live=P, sigma_live=P, save=P, masks=P, stream=None)
    sweep("nerf_mlp_forward_train_live", order, base,
          ["packed", "origins", "dirs", "z_vals", "ray_feat", "enc_d", "live", "rgb", "sigma", "rgb_live", "sigma_live",
           "save", "masks"],
          [("R = -1", dict(R=-1)), ("N = 0", dict(N=0)), ("N = 4097", dict(N=4097)), ("R = 0", dict(R=0, M_live=0)),
           ("2^32 samples", dict(R=1 << 20, N=4096))] + live, f32_only=True)

    # ---- the composite stage (no workspace: a refused check or the empty batch is all that ends a call)
    bg = [("bg_rows = 2", dict(bg_rows=2)), ("bg null with bg_rows = 1", dict(bg=None))]
    order = ["rgb", "sigma", "z_vals", "B", "N", "rgb_map", "depth_map", "weights", "stream"]
    base = dict(rgb=P, sigma=P, z_vals=P, B=B, N=N, rgb_map=P, depth_map=P, weights=P, stream=None)
    required = ["rgb", "sigma", "z_vals", "rgb_map", "depth_map"]
    sweep("nerf_composite", order, base, required, shape)
    order = order[:-1] + ["bg", "bg_rows", "bd", "acc_map", "stream"]
    sweep("nerf_composite_bg", order, dict(base, bg=P, bg_rows=1, bd=6.0, acc_map=P), required, shape + bg)
    order = ["rgb", "sigma", "z_vals", "rgb_map", "target", "B", "N", "scale", "dsigma", "drgb", "sq_err", "stream"]
    base = dict(rgb=P, sigma=P, z_vals=P, rgb_map=P, target=P, B=B, N=N, scale=0.5, dsigma=P, drgb=P, sq_err=P,
                stream=None)
    sweep("nerf_composite_backward", order, base,
          ["rgb", "sigma", "z_vals", "rgb_map", "target", "dsigma", "drgb", "sq_err"], shape)
    order = ["rgb", "sigma", "z_vals", "grad_rgb_map", "grad_depth_map", "B", "N", "dsigma", "drgb", "stream"]
    base = dict(rgb=P, sigma=P, z_vals=P, grad_rgb_map=P, grad_depth_map=P, B=B, N=N, dsigma=P, drgb=P, stream=None)
    required = ["rgb", "sigma", "z_vals", "dsigma", "drgb"]
    sweep("nerf_composite_backward_grad", order, base, required, shape)
    sweep("nerf_composite_backward_grad_acc", order[:-1] + ["g_acc", "bd", "stream"], dict(base, g_acc=P, bd=6.0),
          required, shape)
    order = ["rgb_c", "sigma_c", "rgb_f", "sigma_f", "src", "z_all", "grad_rgb_map", "grad_depth_map", "B", "N", "Nf",
             "accumulate", "dsigma_c", "drgb_c", "dsigma_f", "drgb_f", "stream"]
    base = dict(rgb_c=P, sigma_c=P, rgb_f=P, sigma_f=P, src=P, z_all=P, grad_rgb_map=P, grad_depth_map=P, B=B, N=N,
                Nf=NF, accumulate=1, dsigma_c=P, drgb_c=P, dsigma_f=P, drgb_f=P, stream=None)
    required = ["rgb_c", "sigma_c", "rgb_f", "sigma_f", "src", "z_all", "dsigma_c", "drgb_c", "dsigma_f", "drgb_f"]
    merged = [("B = -1", dict(B=-1)), ("N = 0", dict(N=0)), ("N = 257", dict(N=257)), ("Nf = 0", dict(Nf=0)),
              ("Nf = 1025", dict(Nf=1025)), ("B = 0", dict(B=0))]
    sweep("nerf_composite_merged_backward", order, base, required, merged)
    sweep("nerf_composite_merged_backward_acc", order[:-1] + ["g_acc", "bd", "stream"], dict(base, g_acc=P, bd=6.0),
          required, merged)

    # ---- the backward steps with a background
    bg_loss = bg + [("acc_weight = -1", dict(acc_weight=-1.0)), ("acc_weight NaN", dict(acc_weight=float("nan")))]
    bg_tail = ["alpha", "bg", "bg_rows", "acc_weight", "rgb_final", "stream"]
    bg_args = dict(alpha=P, bg=P, bg_rows=1, acc_weight=0.5, rgb_final=P)
    step = ["packed", "packedT", "rgb_map", "target", "B", "N", "app", "app_rows", "grads", "dapp", "loss", "workspace",
            "ws_bytes"]
    ws_bytes = lib.nerf_train_workspace_bytes(B, N)
    base = dict(packed=P, packedT=P, rgb_map=P, target=P, B=B, N=N, app=P, app_rows=1, grads=grads, dapp=P, loss=P,
                workspace=0x300000, ws_bytes=ws_bytes - 1, stream=None, **bg_args)
    sweep("nerf_train_backward_bg", step + bg_tail, base, backward_ptrs,
          shape + bg_loss + [("app_rows = 2", dict(app_rows=2)), ("gradient 3 null", dict(grads=grads_hole)),
                             ("workspace one byte short", {}),
                             ("no forward wrote the workspace", dict(ws_bytes=ws_bytes))])
    ws_bytes = lib.nerf_train_occ_workspace_bytes(B, N)
    i = step.index("app")
    base = dict(base, M_live=5, workspace=0x400000, ws_bytes=ws_bytes - 1)
    sweep("nerf_train_occ_backward_bg", step[:i] + ["M_live"] + step[i:] + bg_tail, base, backward_ptrs,
          occ_step + bg_loss + [("gradient 3 null", dict(grads=grads_hole)),
                                ("no forward with this M_live wrote the workspace", dict(ws_bytes=ws_bytes))],
          f32_only=True)
    ws_bytes = lib.nerf_train_hier_workspace_bytes(B, N, NF)
    order = ["packed", "packedT", "rgb_map", "coarse_rgb", "target", "B", "N", "Nf", "coarse_weight", "app", "app_rows",
             "grads", "dapp", "loss", "workspace", "ws_bytes"] + bg_tail[:-1] + ["coarse_final", "stream"]
    base = dict(base, coarse_rgb=P, Nf=NF, coarse_weight=0.1, coarse_final=P, workspace=0x500000, ws_bytes=ws_bytes - 1)
    sweep("nerf_train_hier_backward_bg", order, base, backward_ptrs + ["coarse_rgb"],
          [("B = -1", dict(B=-1)), ("N = 1", dict(N=1)), ("N = 257", dict(N=257)), ("Nf = 0", dict(Nf=0)),
           ("Nf = 1025", dict(Nf=1025)), ("B = 0", dict(B=0)), ("2^31 coarse samples", dict(B=1 << 23, N=256)),
           ("app_rows = 2", dict(app_rows=2)), ("coarse_weight = -1", dict(coarse_weight=-1.0)),
           ("gradient 3 null", dict(grads=grads_hole)), ("workspace one byte short", {}),
           ("no forward wrote the workspace", dict(ws_bytes=ws_bytes))] + bg_loss)

    # ---- the hierarchical step itself
    hier_shape = [("B = -1", dict(B=-1)), ("N = 1", dict(N=1)), ("N = 257", dict(N=257)), ("Nf = 0", dict(Nf=0)),
                  ("Nf = 1025", dict(Nf=1025)), ("B = 0", dict(B=0)), ("2^31 coarse samples", dict(B=1 << 23, N=256)),
                  ("app_rows = 2", dict(app_rows=2))]
    hier_step = hier_shape + [("coarse_weight = -1", dict(coarse_weight=-1.0)),
                              ("gradient 3 null", dict(grads=grads_hole)), ("workspace one byte short", {}),
                              ("no forward wrote the workspace", dict(ws_bytes=ws_bytes))]
    order = ["packed", "rays_o", "rays_d", "B", "near", "far", "N", "Nf", "t_vals", "u_lin", "perturb", "t_rand",
             "u_rand", "seed", "app", "app_rows", "rgb_map", "depth_map", "weights_out", "z_out", "coarse_rgb",
             "coarse_depth", "coarse_weights", "workspace", "ws_bytes", "stream"]
    fwd = dict(packed=P, rays_o=P, rays_d=P, B=B, near=2.0, far=6.0, N=N, Nf=NF, t_vals=P, u_lin=P, perturb=1, t_rand=P,
               u_rand=P, seed=7, app=P, app_rows=1, rgb_map=P, depth_map=P, weights_out=P, z_out=P, coarse_rgb=P,
               coarse_depth=P, coarse_weights=P, workspace=0x600000, ws_bytes=ws_bytes - 1, stream=None)
    sweep("nerf_train_hier_forward", order, fwd,
          ["packed", "rays_o", "rays_d", "t_vals", "u_lin", "app", "rgb_map", "depth_map", "coarse_rgb", "coarse_depth",
           "workspace"], hier_shape + [("workspace one byte short", {})])
    hier = ["packed", "packedT", "rgb_map", "coarse_rgb", "target", "B", "N", "Nf", "coarse_weight", "app", "app_rows",
            "grads", "dapp", "loss", "workspace", "ws_bytes"]
    base = dict(base, workspace=0x700000)
    sweep("nerf_train_hier_backward", hier + ["stream"], base, backward_ptrs + ["coarse_rgb"], hier_step)

    # ---- the backward steps with the distortion term
    dist_loss = bg_loss + [("dist_weight = -1", dict(dist_weight=-1.0)), ("dist_weight NaN", dict(dist_weight=float("nan"))),
                           ("far <= near", dict(near=6.0, far=2.0)), ("far infinite", dict(far=float("inf")))]
    dist_tail = ["dist_weight", "near", "far", "stream"]
    base = dict(base, dist_weight=0.01, near=2.0, far=6.0, workspace=0x800000)
    sweep("nerf_train_hier_backward_dist", hier + bg_tail[:-1] + ["coarse_final"] + dist_tail, base,
          backward_ptrs + ["coarse_rgb"], hier_step + dist_loss)
    ws_bytes = lib.nerf_train_workspace_bytes(B, N)
    base = dict(base, workspace=0x900000, ws_bytes=ws_bytes - 1)
    sweep("nerf_train_backward_dist", step + bg_tail[:-1] + dist_tail, base, backward_ptrs,
          shape + dist_loss + [("app_rows = 2", dict(app_rows=2)), ("gradient 3 null", dict(grads=grads_hole)),
                               ("workspace one byte short", {}),
                               ("no forward wrote the workspace", dict(ws_bytes=ws_bytes))])
    ws_bytes = lib.nerf_train_occ_workspace_bytes(B, N)
    base = dict(base, workspace=0xA00000, ws_bytes=ws_bytes - 1)
    sweep("nerf_train_occ_backward_dist", step[:i] + ["M_live"] + step[i:] + bg_tail[:-1] + dist_tail, base,
          backward_ptrs, occ_step + dist_loss + [("gradient 3 null", dict(grads=grads_hole)),
                                                 ("no forward with this M_live wrote the workspace",
                                                  dict(ws_bytes=ws_bytes))], f32_only=True)

    # ---- the distortion stage (no workspace either)
    order = ["rgb", "sigma", "z_vals", "grad_rgb_map", "grad_depth_map", "B", "N", "dsigma", "drgb", "g_acc", "bd", "g_w",
             "stream"]
    sweep("nerf_composite_backward_grad_w", order,
          dict(rgb=P, sigma=P, z_vals=P, grad_rgb_map=P, grad_depth_map=P, B=B, N=N, dsigma=P, drgb=P, g_acc=P, bd=6.0,
               g_w=P, stream=None), ["rgb", "sigma", "z_vals", "dsigma", "drgb"], shape)
    order = ["rgb_c", "sigma_c", "rgb_f", "sigma_f", "src", "z_all", "grad_rgb_map", "grad_depth_map", "B", "N", "Nf",
             "accumulate", "dsigma_c", "drgb_c", "dsigma_f", "drgb_f", "g_acc", "bd", "g_w", "stream"]
    sweep("nerf_composite_merged_backward_w", order,
          dict(rgb_c=P, sigma_c=P, rgb_f=P, sigma_f=P, src=P, z_all=P, grad_rgb_map=P, grad_depth_map=P, B=B, N=N, Nf=NF,
               accumulate=1, dsigma_c=P, drgb_c=P, dsigma_f=P, drgb_f=P, g_acc=P, bd=6.0, g_w=P, stream=None),
          ["rgb_c", "sigma_c", "rgb_f", "sigma_f", "src", "z_all", "dsigma_c", "drgb_c", "dsigma_f", "drgb_f"], merged)
    order = ["weights", "z_vals", "B", "T", "near", "far", "scale", "loss_rays", "g_w", "stream"]
    sweep("nerf_distortion", order,
          dict(weights=P, z_vals=P, B=B, T=N, near=2.0, far=6.0, scale=1.0, loss_rays=P, g_w=P, stream=None),
          ["weights", "z_vals"],
          [("B = -1", dict(B=-1)), ("T = 0", dict(T=0)), ("T = 4097", dict(T=4097)), ("B = 0", dict(B=0)),
           ("far <= near", dict(near=6.0, far=2.0)), ("far infinite", dict(far=float("inf"))),
           ("scale NaN", dict(scale=float("nan"))), ("scale infinite", dict(scale=float("inf")))])
    order = ["z_vals", "weights", "B", "N", "Nf", "u_lin", "u_rand", "seed", "z_all", "z_fine", "merged_src", "stream"]
    sweep("nerf_sample_importance_src", order,
          dict(z_vals=P, weights=P, B=B, N=N, Nf=NF, u_lin=P, u_rand=P, seed=7, z_all=P, z_fine=P, merged_src=P,
               stream=None), ["z_vals", "weights", "u_lin", "z_all", "z_fine", "merged_src"], merged)
    return out


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def test_workspace_sizes_are_pinned():
    from nerfmi import _lib
    got = workspace_sizes(_lib.load())
    want = _golden("host_workspace_bytes.json")
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], k
    big = "nerf_render_workspace_bytes(%d,64,128)" % (1 << 25)
    assert 0 < want["nerf_render_workspace_bytes(640000,64,128)"] < want[big]      # past the chunk limit: one chunk's


def test_error_parity_with_the_recording():
    from nerfmi import _lib
    lib = _lib.load()
    arith = lib.nerf_get_mlp_arith()
    got = error_cases(lib)
    assert lib.nerf_get_mlp_arith() == arith
    want = _golden("host_error_parity.json")
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], k
    # the recording itself: no call reached a launch, and only the empty batches succeed
    for k, (rc, msg) in want.items():
        assert rc != 2, k
        assert (rc == 0) == k.endswith((": B = 0", ": R = 0", ": M = 0")), k
    assert len(want) >= 497


if __name__ == "__main__":
    from nerfmi import _lib
    lib = _lib.load()
    for name, table in (("host_workspace_bytes.json", workspace_sizes(lib)), ("host_error_parity.json", error_cases(lib))):
        with open(os.path.join(GOLDEN, name), "w") as f:
            json.dump(table, f, indent=1)
            f.write("\n")
        print(name, len(table), "entries from", _lib.LIB_PATH)
