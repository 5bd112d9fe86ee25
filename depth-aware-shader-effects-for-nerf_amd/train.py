"""Training loop of the reference (src/train.py:13-207) on the nerfmi HIP kernels.

One iteration (train.py:77-92) is: volume_render(perturb=True) over a batch of rays of one image
→ F.mse_loss against the pixels → loss.backward() → Adam.step().  Here that is four C-ABI
calls (include/nerfmi_train.h) and one RCCL all-reduce:

  nerf_train_forward    normalise, stratified samples, fused PE→MLP forward on MFMA saving every
                        activation, composite (csrc/train_api.hip, csrc/mlp.hip, csrc/mlp16.hip)
  nerf_train_backward   loss, composite backward (reverse scan), MLP data-gradient chain on MFMA
                        with transposed weight fragments, every weight gradient as an MFMA
                        reduction over the batch, appearance-row gradient
  all_reduce            data parallel: the flat gradient buffer averaged over ranks (one RCCL
                        collective of 2.4 MB + the appearance table)
  nerf_adam             torch.optim.Adam's update on the flat parameter buffer (one launch)

Parameters, gradients and Adam moments live in flat device buffers; the NeRF module's parameters
are views into the parameter buffer, so the model, its state_dict and checkpoints always see the
trained values.  The reference's quirks are kept: the first 5 iterations
use min(64, batch_size) rays (train.py:26,56-57), StepLR steps only when i % step_size == 0
(train.py:95-96), n_importance is ignored by the coarse-only volume_render (render.py:83-86),
and one image's rays form each batch (dataset.py:249-277).

Not a reference feature: ``Trainer(hierarchical=True)`` / ``train_nerf(hierarchical=True)`` run the H1
fine pass in every step and train on mse(fine) + coarse_loss_weight * mse(coarse)
(nerf_train_hier_forward / nerf_train_hier_backward).  Nor are ``background=`` and
``acc_weight=``: the target is blended with a background colour through the dataset's alpha channel, the
prediction is composited over the same colour, and the ray's opacity is pulled towards alpha (the _bg
backwards of include/nerfmi_train.h).  The reference's ``background_color`` stays ignored.
"""
import ctypes
import math
import os
import time

import numpy as np
import torch

from . import _lib
from .models import NeRF, STATE_KEYS, state_tensors
from .ray_utils import linspace_table

_APP_DIM = 32


class Trainer:
    """Flat-buffer NeRF (+ appearance table) trainer: one object per rank.

    ``group``: a torch.distributed process group for data parallelism (gradients averaged over
    it before the optimizer step, as DDP would); None trains on this process alone.

    ``occupancy``: an OccupancyGrid on this process's device.  Every step then classifies its
    samples against the grid and runs the MLP forward, backward and weight gradients on the live
    ones only (include/nerfmi_train.h "training with an occupancy grid"): a dead
    sample has sigma = 0 as a constant of the step.  f16x3 arithmetic only.  The step costs one host
    wait (the live count), placed behind the weight packings.

    ``occupancy_refresh``: None keeps the grid's bits as given.  A dict (missing keys take
    OCCUPANCY_REFRESH_DEFAULTS) makes the trainer keep the grid current while the model changes: for
    the first ``warmup`` optimizer steps the grid is all ones over its box, and after optimizer
    step k >= warmup with k == warmup or k % every == 0 the bits are replaced by
    OccupancyGrid.from_model(self.model, box, resolution, threshold, supersample, dilate).  The
    rebuild is deterministic, so data-parallel ranks (identical weights) rebuild identical bits and
    nothing is communicated.

    ``hierarchical``: every step also runs the H1 fine pass (``n_importance`` resampled positions per
    ray, default config.num_importance; one network for both passes, as in the hierarchical render)
    and trains on loss = mse(fine) + ``coarse_loss_weight`` * mse(coarse) (include/nerfmi_train.h
    "training with the hierarchical fine pass").  forward_backward then returns that
    loss with the fine (merged) rgb_map and leaves the two device floats (fine, coarse) on
    ``self.loss_parts``.  Not combined with ``occupancy``.

    ``background``: None (default: the step makes the calls it always made), three floats, or "random"
    (one colour per ray from the library's counter RNG, keyed by the step's seed, which carries the rank).
    A step then takes the batch's ``alpha`` (B,), None = ones, trains on
    mse(rgb_map + k bg, alpha target + (1 - alpha) bg) + ``acc_weight`` * mse(acc, alpha) with acc the
    ray's opacity and k = max(0, 1 - acc), returns the blended map, and leaves the parts on
    ``self.loss_parts``: (colour, opacity), or with ``hierarchical`` (fine colour, coarse colour, fine
    opacity, coarse opacity).  ``acc_weight`` > 0 works without a background too (black); a trainer with
    neither refuses an ``alpha`` (ValueError), so ``loss_parts`` is allocated once, by configuration.  The
    forwards are unchanged; it works dense, with ``occupancy`` and with
    ``hierarchical``.

    ``distortion_weight``: 0 (default: the step makes the calls it makes without the argument) or a finite
    weight > 0 of mip-NeRF 360's distortion loss on the ray weights over the trainer's near / far (the
    _dist backwards of include/nerfmi_train.h): total = (colour + ``acc_weight`` * opacity)
    + ``distortion_weight`` * distortion per part.  ``self.loss_parts`` is then (colour, opacity,
    distortion), or with ``hierarchical`` (fine colour, coarse colour, fine opacity, coarse opacity, fine
    distortion, coarse distortion).  It works dense, with ``occupancy`` and with ``hierarchical``, with or
    without a background."""

    def __init__(self, config, model=None, appearance_embeddings=None, n_images=None, group=None,
                 lr=None, betas=(0.9, 0.999), eps=1e-8, near=None, far=None, occupancy=None,
                 occupancy_refresh=None, hierarchical=False, n_importance=None, coarse_loss_weight=1.0,
                 background=None, acc_weight=0.0, distortion_weight=0.0):
        _check_occupancy_args(occupancy, occupancy_refresh)
        self.background, self.acc_weight = _check_background_args(background, acc_weight)
        self.distortion_weight = _check_distortion_weight(distortion_weight)
        self.hierarchical, self.n_importance, self.coarse_loss_weight = _check_hierarchical_args(
            config, hierarchical, n_importance, coarse_loss_weight, occupancy)
        self.config = config
        # the sampling interval: the dataset's near/far (train.py:79 passes dataset.near/far), the
        # config's when no dataset is given
        self.near = float(config.near if near is None else near)
        self.far = float(config.far if far is None else far)
        self.dev = _lib.device()
        self.lib = _lib.load()
        self.group = group
        model = model if model is not None else NeRF(config)
        self.model = model.to(self.dev)
        named = dict(self.model.named_parameters())
        # 24 parameter slots in STATE_KEYS order; a use_appearance=False model has no
        # appearance_projection (models.py:99-103): its slots stay zero and are not parameters
        self.present = [k in named for k in STATE_KEYS]
        tensors = state_tensors(named, self.dev)
        self.shapes = [tuple(t.shape) for t in tensors]
        self.sizes = [t.numel() for t in tensors]
        if config.use_appearance:
            if appearance_embeddings is None:
                appearance_embeddings = torch.randn(n_images or 100, config.appearance_dim)
            self.n_images = appearance_embeddings.shape[0]
            self.sizes.append(appearance_embeddings.numel())
            self.shapes.append(tuple(appearance_embeddings.shape))
        else:
            self.n_images = 0
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).tolist()
        total = self.offsets[-1]
        self.flat = torch.empty(total, device=self.dev)
        self.grad = torch.zeros(total, device=self.dev)
        self.exp_avg = torch.zeros(total, device=self.dev)
        self.exp_avg_sq = torch.zeros(total, device=self.dev)
        with torch.no_grad():
            for i, t in enumerate(tensors):
                self.view(self.flat, i).copy_(t.detach())
            if self.n_images:
                self.view(self.flat, len(tensors)).copy_(appearance_embeddings.detach())
            # the module's parameters become views of the flat buffer
            for i, k in enumerate(STATE_KEYS):
                if not self.present[i]:
                    continue
                mod_name, pname = k.rsplit(".", 1)
                mod = self.model.get_submodule(mod_name)
                setattr(mod, pname, torch.nn.Parameter(self.view(self.flat, i), requires_grad=False))
        self.appearance_embeddings = self.view(self.flat, len(tensors)) if self.n_images else None
        if isinstance(appearance_embeddings, torch.nn.Parameter):
            # the caller's table (dataset.appearance_embeddings, an nn.Parameter as dataset.py:81-83)
            # becomes a view of the flat buffer, so every optimizer step updates it in place as
            # the reference's Adam does (train.py:36-39)
            appearance_embeddings.data = self.appearance_embeddings
        # Adam's parameter numbering (model.parameters() order, then the appearance table)
        self.param_slots = [i for i in range(24) if self.present[i]] + ([24] if self.n_images else [])
        self.rank = 0
        if group is not None:
            import torch.distributed as dist
            self.rank = dist.get_rank(group)
        # every rank starts from rank 0's weights and table, as DDP's constructor does
        broadcast_state([self.flat], group)
        self.param_ptrs = (ctypes.c_void_p * 24)(*[self.view(self.flat, i).data_ptr() for i in range(24)])
        self.grad_ptrs = (ctypes.c_void_p * 24)(*[self.view(self.grad, i).data_ptr() for i in range(24)])
        self.app_grad = self.view(self.grad, 24) if self.n_images else None
        self.packed = torch.empty(self.lib.nerf_packed_weights_floats(), device=self.dev)
        self.packedT = torch.empty(self.lib.nerf_packed_transposed_floats(), device=self.dev)
        self.dapp = torch.empty(1, _APP_DIM, device=self.dev)
        self.lr = config.learning_rate if lr is None else lr
        self.initial_lr = self.lr
        self.betas, self.eps = betas, eps
        self.steps = 0
        self._ws = None
        self._tvals = {}
        self._side = None          # side stream for the transposed packing (forward_backward)
        self._bg_row = None        # the fixed background colour as a (1,3) device tensor
        # The backward's form, decided once: the suffix of the C entries the steps call, which fixes the loss
        # terms (colour; "_bg": and opacity; "_dist": and distortion).  Term k of part p (0 fine or the only
        # one, 1 coarse) of P parts is loss float k * P + p; a plain dense trainer has the one float and no
        # loss_parts.
        self.loss_form = "_dist" if self.distortion_weight > 0.0 else "_bg" if self._bg_configured() else ""
        terms = {"": 1, "_bg": 2, "_dist": 3}[self.loss_form]
        self._term_weights = (self.acc_weight, self.distortion_weight)[:terms - 1]   # of the terms behind the colour
        self._parts = 2 if self.hierarchical else 1
        self._ws_hier = None
        self._loss = torch.zeros(terms * self._parts, device=self.dev)
        if terms * self._parts > 1:
            self.loss_parts = self._loss
        self.occupancy = occupancy
        self.occupancy_refresh = None
        self.live_fraction = None  # share of the last step's samples the grid marked live
        if occupancy is not None:
            if occupancy.device != self.dev:
                raise ValueError(f"Trainer: the occupancy grid is on {occupancy.device}, the trainer on {self.dev}")
            if occupancy_refresh is not None:
                self.occupancy_refresh = dict(OCCUPANCY_REFRESH_DEFAULTS, **occupancy_refresh)
                if self.occupancy_refresh["warmup"] > 0:
                    G = occupancy.resolution
                    occupancy.from_mask(torch.ones(G, G, G, dtype=torch.bool))
                else:
                    self._rebuild_occupancy()
            self._live_dev = torch.zeros(1, dtype=torch.int32, device=self.dev)
            self._live_host = torch.zeros(1, dtype=torch.int32).pin_memory()
            self._live_ev = torch.cuda.Event()
            self._ws_occ = None

    def view(self, buf, i):
        return buf[self.offsets[i]: self.offsets[i + 1]].view(self.shapes[i])

    def _workspace(self, B, N):
        need = self.lib.nerf_train_workspace_bytes(B, N)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
        return self._ws

    # ------------------------------------------------- what the step variants and profile_step share
    def _batch(self, rays_o, rays_d, target):
        """(o, d, target) as contiguous float32 (B,3) tensors on the device."""
        return tuple(t.reshape(-1, 3).to(self.dev, torch.float32).contiguous() for t in (rays_o, rays_d, target))

    def _t_vals(self, N):
        if N not in self._tvals:
            self._tvals[N] = linspace_table(N, self.dev)
        return self._tvals[N]

    def _app_row(self, app_idx):
        """(app, rows): the batch's image's appearance row and 1, or (None, 0)."""
        if self.n_images and app_idx is not None:
            return self.appearance_embeddings[int(app_idx)].reshape(1, _APP_DIM), 1
        return None, 0

    def _maps(self, B):
        return torch.empty(B, 3, device=self.dev), torch.empty(B, device=self.dev)

    def _pack_transposed_aside(self, main):
        """The transposed weights are read only by the backward: they are packed on a side stream while
        the forward runs (forked after everything queued so far, so after the previous step's backward
        read them; the caller waits for self._join before this step's backward)."""
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.dev)
            self._fork, self._join = torch.cuda.Event(), torch.cuda.Event()
        self._fork.record(main)
        self._side.wait_event(self._fork)
        _lib.check(self.lib.nerf_pack_weights_transposed(self.param_ptrs, _lib.ptr(self.packedT),
                                                         self._side.cuda_stream), "nerf_pack_weights_transposed")
        if self.app_grad is not None:    # the table's gradient is one row this step: zeroed beside the forward
            with torch.cuda.stream(self._side):
                self.app_grad.zero_()
        self._join.record(self._side)

    def _bg_configured(self):
        return self.background is not None or self.acc_weight > 0.0

    def _bg_args(self, B, seed, alpha):
        """The step's (alpha, bg, bg_rows, rgb_final) tensors for the _bg and _dist entries: every option
        off for a trainer with only a distortion weight, and no rgb_final for the plain form (which passes
        none of them).  An alpha is refused without a background or an opacity term."""
        if not self._bg_configured():
            if alpha is not None:
                raise ValueError("Trainer: alpha belongs to a trainer with background= or acc_weight > 0")
            return None, None, 0, torch.empty(B, 3, device=self.dev) if self.loss_form else None
        if alpha is not None:
            alpha = alpha.reshape(-1).to(self.dev, torch.float32).contiguous()
            if alpha.shape[0] != B:
                raise ValueError(f"Trainer: alpha has {alpha.shape[0]} values for {B} rays")
        bg, rows = None, 0
        if self.background == "random":
            bg, rows = random_background(B, seed, self.dev), B
        elif self.background is not None:
            if self._bg_row is None:
                self._bg_row = torch.tensor([self.background], dtype=torch.float32, device=self.dev)
            bg, rows = self._bg_row, 1
        return alpha, bg, rows, torch.empty(B, 3, device=self.dev)

    def validation_background(self):
        """The fixed colour a validation render composites over: the trainer's, white for "random"."""
        if self.background is None:
            return None
        return (1.0, 1.0, 1.0) if self.background == "random" else self.background

    def _zero_unused_projection(self, rows):
        if rows == 0:   # appearance_projection unused: its gradient is zero, as torch leaves it (None → no update)
            self.view(self.grad, 20).zero_()
            self.view(self.grad, 21).zero_()

    def _pack_for_step(self, main, B, app_idx):
        """The step variants' prologue: both weight packings (the transposed one aside), the output maps
        and the appearance row.  (rgb_map, depth, app, rows)"""
        _lib.check(self.lib.nerf_pack_weights(self.param_ptrs, _lib.ptr(self.packed), _lib.stream()),
                   "nerf_pack_weights")
        self._pack_transposed_aside(main)
        return self._maps(B) + self._app_row(app_idx)

    def _backward(self, main, entry, args, ws, app_idx, rgb_map, bgo):
        """The step variants' epilogue: the join with the transposed packing, then the C entry `entry` in
        the trainer's form (`args`: what it takes between packedT and the gradient pointers, ending in app,
        rows): the _bg form with `bgo` (_bg_args) and the opacity weight behind ws_bytes, the _dist form
        with the distortion weight, near and far behind those.  (loss, the map the loss was taken on)"""
        P, rows = _lib.ptr, args[-1]
        # d app of the batch's image goes straight into its row of the table's gradient
        dapp = self.app_grad[int(app_idx)] if rows else None
        main.wait_event(self._join)
        al, bg, bg_rows, out = bgo
        tail = ()
        if self.loss_form:
            tail = (P(al), P(bg), bg_rows, self.acc_weight, P(out)) + (None,) * (self._parts - 1)   # (no coarse_final)
        if self.loss_form == "_dist":
            tail += (self.distortion_weight, self.near, self.far)
        lp, n, entry = self._loss, self._parts, entry + self.loss_form
        _lib.check(getattr(self.lib, entry)(P(self.packed), P(self.packedT), *args, self.grad_ptrs, P(dapp), P(lp),
                                            P(ws), ws.numel(), *tail, _lib.stream()), entry)
        self._zero_unused_projection(rows)
        # per part ((colour + acc_weight opacity) + distortion_weight distortion), then fine + weight coarse
        total = [lp[p] for p in range(n)]
        for k, weight in enumerate(self._term_weights, 1):
            total = [t + weight * lp[k * n + p] for p, t in enumerate(total)]
        loss = total[0] + self.coarse_loss_weight * total[1] if n == 2 else total[0]
        return loss, (rgb_map if out is None else out)

    # ------------------------------------------------------------------------------ one step
    def forward_backward(self, rays_o, rays_d, target, app_idx=None, *, t_rand=None, u_rand=None, seed=None,
                         alpha=None, _marks=None):
        """Loss (device scalar) and gradients in self.grad for one batch (train.py:77-90).
        rays (B,3) and target (B,3) on the device; app_idx: the batch's image (appearance row).
        t_rand (B,N) = the torch.rand draw of ray_utils.py:80; else the in-kernel RNG on `seed`.
        u_rand (B,n_importance): the fine pass's draws (hierarchical trainers only).
        alpha (B,): the target pixels' alpha channel (trainers with a background; None = ones); with a
        background the returned map is the blended one."""
        lib, s, P = self.lib, _lib.stream(), _lib.ptr
        N = self.config.num_samples
        o, d, tgt = self._batch(rays_o, rays_d, target)
        B = o.shape[0]
        if t_rand is not None:
            t_rand = t_rand.to(self.dev, torch.float32).contiguous()
            assert t_rand.shape == (B, N)
        if seed is None:
            seed = step_seed(self.steps + 1, self.rank)
        bgo = self._bg_args(B, seed, alpha)
        if self.hierarchical:
            return self._forward_backward_hier(o, d, tgt, app_idx, t_rand, u_rand, seed, _marks, bgo)
        if u_rand is not None:
            raise ValueError("Trainer: u_rand belongs to the fine pass; construct the trainer with hierarchical=True")
        if self.occupancy is not None:
            return self._forward_backward_occ(o, d, tgt, app_idx, t_rand, seed, _marks, bgo)
        main = torch.cuda.current_stream(self.dev)
        rgb_map, depth, app, rows = self._pack_for_step(main, B, app_idx)
        t_vals = self._t_vals(N)
        ws = self._workspace(B, N)
        _lib.check(lib.nerf_train_forward(P(self.packed), P(o), P(d), B, self.near, self.far, N,
                                          P(t_vals), 1, P(t_rand), int(seed), P(app), rows, P(rgb_map),
                                          P(depth), None, None, P(ws), ws.numel(), s),
                   "nerf_train_forward")
        if _marks is not None:
            _marks[1].record(torch.cuda.current_stream())
        return self._backward(main, "nerf_train_backward", (P(rgb_map), P(tgt), B, N, P(app), rows), ws, app_idx,
                              rgb_map, bgo)

    def _forward_backward_hier(self, o, d, tgt, app_idx, t_rand, u_rand, seed, _marks, bgo):
        """forward_backward with the fine pass: nerf_train_hier_forward + nerf_train_hier_backward on one
        workspace that carries both sample sets' saves."""
        lib, s, P = self.lib, _lib.stream(), _lib.ptr
        N, Nf = self.config.num_samples, self.n_importance
        B = o.shape[0]
        if u_rand is not None:
            u_rand = u_rand.to(self.dev, torch.float32).contiguous()
            assert u_rand.shape == (B, Nf)
        main = torch.cuda.current_stream(self.dev)
        rgb_map, depth, app, rows = self._pack_for_step(main, B, app_idx)
        t_vals = self._t_vals(N)
        u_lin = linspace_table(Nf, self.dev, drop_last=True)        # ray_utils.py:115
        need = lib.nerf_train_hier_workspace_bytes(B, N, Nf)
        if B and need == 0:
            raise ValueError(f"Trainer: the hierarchical step takes num_samples in 2..256 and n_importance in "
                             f"1..1024, got {N} + {Nf}")
        if self._ws_hier is None or self._ws_hier.numel() < need:
            self._ws_hier = torch.empty(need, dtype=torch.uint8, device=self.dev)
        ws = self._ws_hier
        rgb_c, depth_c = self._maps(B)
        _lib.check(lib.nerf_train_hier_forward(P(self.packed), P(o), P(d), B, self.near, self.far, N, Nf, P(t_vals),
                                               P(u_lin), 1, P(t_rand), P(u_rand), int(seed), P(app), rows,
                                               P(rgb_map), P(depth), None, None, P(rgb_c), P(depth_c), None, P(ws),
                                               ws.numel(), s), "nerf_train_hier_forward")
        if _marks is not None:
            _marks[1].record(main)
        return self._backward(main, "nerf_train_hier_backward",
                              (P(rgb_map), P(rgb_c), P(tgt), B, N, Nf, self.coarse_loss_weight, P(app), rows), ws, app_idx,
                              rgb_map, bgo)

    def _forward_backward_occ(self, o, d, tgt, app_idx, t_rand, seed, _marks, bgo):
        """forward_backward on the live samples of self.occupancy: sample + classify, the live count
        to pinned host memory behind an event, the two weight packings (which cover that copy), the
        wait, then the gathered forward and the compact backward."""
        lib, s, P = self.lib, _lib.stream(), _lib.ptr
        g = self.occupancy
        if _lib.get_mlp_arith() != "f16x3":
            raise ValueError("Trainer: training with an occupancy grid runs under the f16x3 arithmetic only")
        if g.device != self.dev:
            raise ValueError(f"Trainer: the occupancy grid is on {g.device}, the trainer on {self.dev}")
        N = self.config.num_samples
        B = o.shape[0]
        t_vals = self._t_vals(N)
        need = lib.nerf_train_occ_workspace_bytes(B, N)
        if self._ws_occ is None or self._ws_occ.numel() < need:
            self._ws_occ = torch.empty(need, dtype=torch.uint8, device=self.dev)
        ws = self._ws_occ
        main = torch.cuda.current_stream(self.dev)
        _lib.check(lib.nerf_train_occ_sample(P(o), P(d), B, self.near, self.far, N, P(t_vals), 1, P(t_rand),
                                             int(seed), P(g.bits), g.resolution, g.c_lo(), g.c_inv(),
                                             P(self._live_dev), P(ws), ws.numel(), s), "nerf_train_occ_sample")
        self._live_host.copy_(self._live_dev, non_blocking=True)
        self._live_ev.record(main)
        rgb_map, depth, app, rows = self._pack_for_step(main, B, app_idx)
        self._live_ev.synchronize()                      # the step's one host wait
        m_live = int(self._live_host[0])
        self.live_fraction = m_live / max(1, B * N)
        if _marks is not None and len(_marks) > 5:       # (scripts/bench_train_occupancy.py: end of sample + wait)
            _marks[5].record(main)
        _lib.check(lib.nerf_train_occ_forward(P(self.packed), P(o), B, N, m_live, P(app), rows, P(rgb_map), P(depth),
                                              None, None, P(ws), ws.numel(), s), "nerf_train_occ_forward")
        if _marks is not None:
            _marks[1].record(main)
        return self._backward(main, "nerf_train_occ_backward", (P(rgb_map), P(tgt), B, N, m_live, P(app), rows), ws,
                              app_idx, rgb_map, bgo)

    def _rebuild_occupancy(self):
        from .occupancy import OccupancyGrid
        g, r = self.occupancy, self.occupancy_refresh
        new = OccupancyGrid.from_model(self.model, g.lo, g.hi, resolution=g.resolution, threshold=r["threshold"],
                                       supersample=r["supersample"], dilate=r["dilate"])
        g.bits = new.bits

    def profile_step(self, rays_o, rays_d, target, app_idx=None, seed=12345):
        """Event-timed phases of one training step through the stage entry points (no parameter
        update): {phase: ms} for the forward MLP, the MLP data-gradient chain, the weight
        gradients and the whole forward+backward."""
        lib, s, P = self.lib, _lib.stream(), _lib.ptr
        cur = torch.cuda.current_stream()
        N = self.config.num_samples
        o, d, tgt = self._batch(rays_o, rays_d, target)
        B = o.shape[0]
        M = B * N
        dev = self.dev
        dn, z = torch.empty(B, 3, device=dev), torch.empty(B, N, device=dev)
        feat, encd = torch.empty(B, 256, device=dev), torch.empty(B, 32, device=dev)
        rgb, sigma = torch.empty(M, 3, device=dev), torch.empty(M, device=dev)
        MT = _lib.tile_rows(M)                                       # tile-major save/grad rows
        save, grad = torch.empty(MT, _lib.SAVE_ROW, device=dev), torch.empty(MT, _lib.GRAD_ROW, device=dev)
        masks = torch.empty(M, _lib.MASK_ROW, dtype=torch.int32, device=dev)
        rgb_map, depth = self._maps(B)
        dsig, drgb, sq = torch.empty(M, device=dev), torch.empty(M, 3, device=dev), torch.empty(B, device=dev)
        grads = [torch.empty_like(self.view(self.grad, i)) for i in range(24)]
        gptr = (ctypes.c_void_p * 24)(*[g.data_ptr() for g in grads])
        wsz = self.lib.nerf_param_grads_workspace_bytes(M)
        ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
        app, rows = self._app_row(app_idx)
        t_vals = self._t_vals(N)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        ck = _lib.check
        ev[0].record(cur)
        ck(lib.nerf_pack_weights(self.param_ptrs, P(self.packed), s), "pack")
        ck(lib.nerf_pack_weights_transposed(self.param_ptrs, P(self.packedT), s), "packT")
        ev[1].record(cur)
        ck(lib.nerf_normalize_dirs(P(d), B, P(dn), s), "normalize")
        ck(lib.nerf_sample_stratified(P(o), P(dn), B, self.near, self.far, N,
                                      P(t_vals), 1, None, seed, P(z), None, s), "stratified")
        ck(lib.nerf_ray_features_train(P(self.packed), P(dn), B, P(app), rows, P(feat), P(encd), s), "features")
        ev[2].record(cur)
        ck(lib.nerf_mlp_forward_train(P(self.packed), P(o), P(dn), P(z), B, N, P(feat), P(encd), P(rgb), P(sigma),
                                      P(save), P(masks), s), "mlp_forward_train")
        ev[3].record(cur)
        ck(lib.nerf_composite(P(rgb), P(sigma), P(z), B, N, P(rgb_map), P(depth), None, s), "composite")
        ck(lib.nerf_composite_backward(P(rgb), P(sigma), P(z), P(rgb_map), P(tgt), B, N, 2.0 / (3 * B), P(dsig),
                                       P(drgb), P(sq), s), "composite_backward")
        ev[4].record(cur)
        mk = masks if _lib.get_mlp_arith() == "f16x3" else None    # the f16x3 forward wrote them
        ck(lib.nerf_mlp_backward(P(self.packed), P(self.packedT), P(save), P(mk), P(sigma), P(rgb), P(dsig), P(drgb),
                                 M, P(grad), s), "mlp_backward")
        ev[5].record(cur)
        ck(lib.nerf_param_grads(P(save), P(grad), M, N, P(app), rows, P(self.packed), gptr, P(self.dapp), P(ws),
                                wsz, s), "param_grads")
        ev[6].record(cur)
        torch.cuda.synchronize()
        return {"pack_ms": ev[0].elapsed_time(ev[1]), "rays_ms": ev[1].elapsed_time(ev[2]),
                "mlp_forward_ms": ev[2].elapsed_time(ev[3]), "composite_fwd_bwd_ms": ev[3].elapsed_time(ev[4]),
                "mlp_backward_ms": ev[4].elapsed_time(ev[5]), "param_grads_ms": ev[5].elapsed_time(ev[6]),
                "total_ms": ev[0].elapsed_time(ev[6])}

    def all_reduce(self):
        """Average the gradients over the data-parallel group (one RCCL all-reduce)."""
        average_gradients(self.grad, self.group)

    def optimizer_step(self):
        """torch.optim.Adam.step() on every parameter (train.py:91), one launch."""
        self.steps += 1
        _lib.check(self.lib.nerf_adam(_lib.ptr(self.flat), _lib.ptr(self.grad), _lib.ptr(self.exp_avg),
                                      _lib.ptr(self.exp_avg_sq), self.flat.numel(), float(self.lr),
                                      float(self.betas[0]), float(self.betas[1]), float(self.eps), self.steps,
                                      _lib.stream()), "nerf_adam")
        self.model._packed = None          # the module's cached inference packing is stale now
        r = self.occupancy_refresh
        if r is not None and self.steps >= r["warmup"] and (self.steps == r["warmup"] or self.steps % r["every"] == 0):
            self._rebuild_occupancy()

    def step(self, rays_o, rays_d, target, app_idx=None, *, t_rand=None, u_rand=None, seed=None, alpha=None):
        loss, rgb = self.forward_backward(rays_o, rays_d, target, app_idx, t_rand=t_rand, u_rand=u_rand, seed=seed,
                                          alpha=alpha)
        self.all_reduce()
        self.optimizer_step()
        return loss

    # ---------------------------------------------------------------------- checkpoints
    def optimizer_state_dict(self):
        """torch.optim.Adam.state_dict() layout (train.py:116,178): per-parameter step/exp_avg/exp_avg_sq,
        parameters numbered model.parameters() order then the appearance table."""
        n = len(self.param_slots)
        state = {}
        if self.steps:
            for i, slot in enumerate(self.param_slots):
                state[i] = {"step": torch.tensor(float(self.steps)),
                            "exp_avg": self.view(self.exp_avg, slot).detach().cpu().clone(),
                            "exp_avg_sq": self.view(self.exp_avg_sq, slot).detach().cpu().clone()}
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": 0, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": False, "initial_lr": self.initial_lr, "params": list(range(n))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd):
        st = sd["state"]
        if len(sd["param_groups"][0]["params"]) != len(self.param_slots):
            raise ValueError(f"optimizer state has {len(sd['param_groups'][0]['params'])} parameters, "
                             f"this trainer {len(self.param_slots)}")
        for i, e in st.items():
            slot = self.param_slots[int(i)]
            self.view(self.exp_avg, slot).copy_(e["exp_avg"])
            self.view(self.exp_avg_sq, slot).copy_(e["exp_avg_sq"])
            self.steps = int(float(e["step"]))
        self.lr = sd["param_groups"][0]["lr"]
        broadcast_state([self.exp_avg, self.exp_avg_sq], self.group)

    def checkpoint(self, loss, psnr, iteration):
        """The dict train.py:114-125 saves."""
        ck = {"model_state_dict": {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()},
              "optimizer_state_dict": self.optimizer_state_dict(), "loss": loss, "psnr": psnr,
              "iteration": iteration}
        if self.n_images:
            ck["appearance_embeddings"] = self.appearance_embeddings.detach().cpu().clone()
        if self.occupancy is not None:
            ck["occupancy"] = self.occupancy.state_dict()
        return ck


# occupancy_refresh defaults (hyper-parameters, not gates): all ones for the first 256 steps, then a
# rebuild every 256 steps at one probe per cell, sigma > 0.01, one dilation
OCCUPANCY_REFRESH_DEFAULTS = {"every": 256, "warmup": 256, "threshold": 0.01, "dilate": 1, "supersample": 1}


def _check_occupancy_args(occupancy, occupancy_refresh):
    """ValueError for anything but an OccupancyGrid / a dict of the refresh keys (no device needed)."""
    from .occupancy import OccupancyGrid
    if occupancy is None:
        if occupancy_refresh is not None:
            raise ValueError("Trainer: occupancy_refresh needs an occupancy grid")
        return
    if not isinstance(occupancy, OccupancyGrid):
        raise ValueError(f"Trainer: occupancy must be an OccupancyGrid, got {type(occupancy).__name__}")
    if occupancy_refresh is None:
        return
    if not isinstance(occupancy_refresh, dict) or set(occupancy_refresh) - set(OCCUPANCY_REFRESH_DEFAULTS):
        raise ValueError(f"Trainer: occupancy_refresh must be a dict with keys among "
                         f"{sorted(OCCUPANCY_REFRESH_DEFAULTS)}, got {occupancy_refresh!r}")
    r = dict(OCCUPANCY_REFRESH_DEFAULTS, **occupancy_refresh)
    if int(r["every"]) < 1 or int(r["warmup"]) < 0 or int(r["dilate"]) < 0 or int(r["supersample"]) < 1:
        raise ValueError(f"Trainer: occupancy_refresh={occupancy_refresh!r}: every >= 1, warmup >= 0, dilate >= 0, "
                         f"supersample >= 1")


def _check_hierarchical_args(config, hierarchical, n_importance, coarse_loss_weight, occupancy):
    """(hierarchical, n_importance, coarse_loss_weight) checked; ValueError otherwise (no device needed)."""
    hierarchical = bool(hierarchical)
    if not hierarchical:
        if n_importance is not None:
            raise ValueError("Trainer: n_importance needs hierarchical=True")
        if float(coarse_loss_weight) != 1.0:
            raise ValueError("Trainer: coarse_loss_weight needs hierarchical=True")
        return False, None, 1.0
    if occupancy is not None:
        raise ValueError("Trainer: hierarchical=True is not combined with occupancy= (the hierarchical step "
                         "runs on every sample)")
    nf = config.num_importance if n_importance is None else n_importance
    if isinstance(nf, bool) or not isinstance(nf, (int, np.integer)) or not 1 <= int(nf) <= 1024:
        raise ValueError(f"Trainer: n_importance must be an integer in 1..1024, got {nf!r}")
    if not 2 <= int(config.num_samples) <= 256:
        raise ValueError(f"Trainer: hierarchical=True takes config.num_samples in 2..256, got {config.num_samples}")
    cw = float(coarse_loss_weight)
    if not (cw >= 0.0 and math.isfinite(cw)):
        raise ValueError(f"Trainer: coarse_loss_weight must be finite and >= 0, got {coarse_loss_weight!r}")
    return True, int(nf), cw


def _check_background_args(background, acc_weight):
    """(background, acc_weight) checked: None, "random" or a tuple of three finite floats, and a finite
    float >= 0; ValueError otherwise (no device needed)."""
    aw = float(acc_weight)
    if not (aw >= 0.0 and math.isfinite(aw)):
        raise ValueError(f"Trainer: acc_weight must be finite and >= 0, got {acc_weight!r}")
    if background is None or (isinstance(background, str) and background == "random"):
        return background, aw
    try:
        bg = tuple(float(v) for v in background)
    except (TypeError, ValueError):
        bg = ()
    if isinstance(background, str) or len(bg) != 3 or not all(math.isfinite(v) for v in bg):
        raise ValueError(f'Trainer: background must be None, "random" or three finite floats, got {background!r}')
    return bg, aw


def _check_distortion_weight(distortion_weight):
    """The distortion loss's weight checked as acc_weight is: a finite float >= 0; ValueError otherwise."""
    dw = float(distortion_weight)
    if not (dw >= 0.0 and math.isfinite(dw)):
        raise ValueError(f"Trainer: distortion_weight must be finite and >= 0, got {distortion_weight!r}")
    return dw


_BACKGROUND_KEY = 0xBAC6C0105EED        # the random backgrounds' stream: the step's seed ^ this


def random_background(B, seed, dev=None):
    """(B,3) uniform colours of a step: value c of ray r is draw 3 r + c of the library's counter
    generator (include/nerfmi.h, nerf_rng_uniforms) keyed by seed ^ _BACKGROUND_KEY, so the same
    (step seed, rank) repeats them and different steps or ranks differ."""
    dev = _lib.device() if dev is None else dev
    out = torch.empty(B, 3, device=dev)
    _lib.check(_lib.load().nerf_rng_uniforms((int(seed) ^ _BACKGROUND_KEY) & ((1 << 64) - 1), 0, 3 * B,
                                             _lib.ptr(out), _lib.stream()), "nerf_rng_uniforms")
    return out


def step_seed(key, rank):
    """Key of a step's in-kernel jitter stream: distinct per step and per data-parallel rank (the
    reference draws torch.rand per call, ray_utils.py:80; ranks must not share draws)."""
    return (int(key) & ((1 << 40) - 1)) | (int(rank) << 40)


def broadcast_state(tensors, group):
    """Rank 0's copy of each tensor on every rank of `group` (a no-op alone)."""
    if group is None:
        return
    import torch.distributed as dist
    src = dist.get_global_rank(group, 0)
    for t in tensors:
        dist.broadcast(t, src=src, group=group)


def average_gradients(flat_grad, group):
    """Data-parallel gradient sync: one all-reduce of the whole flat gradient buffer (2.4 MB of
    NeRF weights + the appearance table), then / world — the mean-loss gradient of the union of
    the ranks' batches.  One large collective suits xGMI's per-link ring bandwidth better than
    per-tensor buckets."""
    if group is None:
        return
    import torch.distributed as dist
    world = dist.get_world_size(group)
    dist.all_reduce(flat_grad, group=group)     # (world 1 included: the collective runs whenever a group exists)
    if world > 1:
        flat_grad.div_(world)


def train_nerf(config, dataset, save_dir="checkpoints", group=None, num_iterations=None, log_every=10,
               checkpoint_every=1000, seed=None, plots=True, return_metrics=False, occupancy=None,
               occupancy_refresh=None, hierarchical=False, n_importance=None, coarse_loss_weight=1.0,
               background=None, acc_weight=0.0, distortion_weight=0.0, trainer_cls=None):
    """src/train.py:13-207 on nerfmi: returns the trained model, as the reference does
    (train.py:207; run.py:347 assigns it).  ``return_metrics=True`` returns (model, losses, psnrs)
    instead; the per-iteration losses and PSNRs are also left on ``train_nerf.losses`` /
    ``train_nerf.psnrs``.  The dataset's appearance table (an nn.Parameter, dataset.py:81-83) is
    trained in place (train.py:36-39).  Every ``checkpoint_every`` iterations rank 0 writes
    checkpoint_{i:06d}.pt and the validation render render_{i:06d}.png of train.py:127-173.
    Under data parallelism every rank draws its own batch (its own image, its own jitter
    stream) and the gradients are averaged; rank 0 writes.  ``occupancy`` / ``occupancy_refresh``
    go to the Trainer (training on the live samples of an occupancy grid); the final and periodic
    checkpoints then carry the grid's state_dict under "occupancy".  ``hierarchical`` /
    ``n_importance`` / ``coarse_loss_weight`` go to the Trainer too (coarse + fine loss): the logged
    loss and PSNR are then the fine pass's, and the validation render is hierarchical.  ``background`` /
    ``acc_weight`` go to the Trainer as well: with a background or an opacity weight set every step gets the
    batch's alpha channel (``batch["alpha"]``; None, the custom format, means ones), the logged loss and PSNR are the
    colour term's, and the validation render composites over the trainer's colour (white for "random").
    ``distortion_weight`` > 0 goes to the Trainer too (the distortion loss on the ray weights); the logged loss
    and PSNR stay the colour term's.  ``trainer_cls`` (tests): the class constructed instead of Trainer."""
    import torch.distributed as dist
    _check_occupancy_args(occupancy, occupancy_refresh)
    _check_background_args(background, acc_weight)
    dist_kwargs = {"distortion_weight": distortion_weight} if _check_distortion_weight(distortion_weight) > 0.0 else {}
    _check_hierarchical_args(config, hierarchical, n_importance, coarse_loss_weight, occupancy)
    rank = dist.get_rank(group) if group is not None else 0
    if rank == 0:
        os.makedirs(save_dir, exist_ok=True)
    initial_batch_size = min(64, config.batch_size)                    # train.py:26
    bg_kwargs = {}
    if background is not None or float(acc_weight) != 0.0:
        bg_kwargs = dict(background=background, acc_weight=acc_weight)
    trainer = (trainer_cls or Trainer)(
        config, appearance_embeddings=getattr(dataset, "appearance_embeddings", None), n_images=len(dataset),
        group=group, near=getattr(dataset, "near", None), far=getattr(dataset, "far", None), occupancy=occupancy,
        occupancy_refresh=occupancy_refresh, hierarchical=hierarchical, n_importance=n_importance,
        coarse_loss_weight=coarse_loss_weight, **bg_kwargs, **dist_kwargs)
    iters = config.num_iterations if num_iterations is None else num_iterations
    losses, psnrs = [], []
    train_nerf.losses, train_nerf.psnrs = losses, psnrs
    start = time.time()
    loss_v = psnr_v = float("nan")
    for i in range(1, iters + 1):
        batch = dataset.get_rays(batch_size=initial_batch_size) if i <= 5 else dataset.get_rays()
        app_idx = batch["appearance_idx"] if config.use_appearance else None
        step_kwargs = {"alpha": batch.get("alpha")} if bg_kwargs else {}
        loss = trainer.step(batch["rays_o"], batch["rays_d"], batch["rgb"], app_idx,
                            seed=None if seed is None else step_seed(seed * 1_000_003 + i, trainer.rank),
                            **step_kwargs)
        if i % config.scheduler_step_size == 0:                          # StepLR, train.py:95-96
            trainer.lr *= config.scheduler_gamma
        # the fine MSE; with a background or an opacity term the (fine) colour term
        loss_v = float(trainer.loss_parts[0]) if (trainer.hierarchical or trainer.loss_form) else float(loss)
        psnr_v = -10.0 * math.log10(loss_v) if loss_v > 0 else float("inf")
        losses.append(loss_v)
        psnrs.append(psnr_v)
        if rank == 0 and log_every and i % log_every == 0:
            print(f"iter {i}: Loss: {loss_v:.5f}, PSNR: {psnr_v:.2f}")
        if rank == 0 and checkpoint_every and i % checkpoint_every == 0:
            torch.save(trainer.checkpoint(loss_v, psnr_v, i), os.path.join(save_dir, f"checkpoint_{i:06d}.pt"))
            if plots:
                validation_render(trainer.model, dataset, config, i, save_dir, hierarchical=trainer.hierarchical,
                                  n_importance=trainer.n_importance,
                                  **({"background": trainer.validation_background()} if background is not None else {}))
    if rank == 0:
        torch.save(trainer.checkpoint(loss_v, psnr_v, iters), os.path.join(save_dir, "checkpoint_final.pt"))
        if plots:
            _plot_curves(losses, psnrs, os.path.join(save_dir, "training_curves.png"))
        print(f"Training completed in {time.time() - start:.2f}s")
    if return_metrics:
        return trainer.model, losses, psnrs
    return trainer.model


@torch.no_grad()
def validation_render(model, dataset, config, iteration, save_dir, hierarchical=False, n_importance=None,
                      background=None):
    """The sample render of train.py:127-173: the first 1000 rays of the last image, coarse
    volume_render with perturb=False (``hierarchical``: the H1 fine pass with n_importance samples, as
    a hierarchical trainer trained it; ``background``: three floats the render is composited over), RGB
    and viridis depth side by side in render_{iteration:06d}.png.  Returns (rgb (1000,3), depth (1000,1))."""
    from .render import volume_render
    val = dataset.get_rays(idx=len(dataset) - 1)
    o, d = val["rays_o"][:1000], val["rays_d"][:1000]
    app = None
    if config.use_appearance:
        app = dataset.appearance_embeddings[val["appearance_idx"]]
    rgb, depth, _ = volume_render(model, o, d, near=dataset.near, far=dataset.far, n_samples=config.num_samples,
                                  n_importance=config.num_importance if n_importance is None else n_importance,
                                  appearance_embedding=app, perturb=False, hierarchical=hierarchical,
                                  **({} if background is None else {"background": background}))
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    rgb_viz = rgb.reshape(-1, 3).cpu().numpy()
    n = int(np.sqrt(rgb_viz.shape[0]))
    plt.figure(figsize=(10, 5))
    plt.subplot(1, 2, 1)
    plt.imshow(np.clip(rgb_viz[:n * n].reshape(n, n, 3), 0, 1))
    plt.title(f"RGB - Iteration {iteration}")
    plt.axis("off")
    plt.subplot(1, 2, 2)
    plt.imshow(depth.reshape(-1).cpu().numpy()[:n * n].reshape(n, n), cmap="viridis")
    plt.title(f"Depth - Iteration {iteration}")
    plt.colorbar()
    plt.axis("off")
    plt.savefig(os.path.join(save_dir, f"render_{iteration:06d}.png"))
    plt.close()
    return rgb, depth


def _plot_curves(losses, psnrs, path):
    """training_curves.png of train.py:189-204."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    plt.figure(figsize=(10, 5))
    plt.subplot(1, 2, 1)
    plt.plot(losses)
    plt.title("Training Loss")
    plt.xlabel("Iteration")
    plt.ylabel("Loss")
    plt.subplot(1, 2, 2)
    plt.plot(psnrs)
    plt.title("Training PSNR")
    plt.xlabel("Iteration")
    plt.ylabel("PSNR (dB)")
    plt.savefig(path)
    plt.close()
