"""`render_rays` with the reference's signature and result keys (morpheus.py:558-794).

`HotPathRenderer` plays the role of the `self` that MorpheuS.render_rays closes over: it owns
`model` (scene_representation), `config` (the YAML dict), `occupancy_grid` (anything with a
nerfacc-style `.sampling(rays_o, rays_d, ...) -> (ray_indices, t_starts, t_ends)`) and
`num_frames`.  A maintainer wires it into morpheus.py by delegating MorpheuS.render_rays to
`HotPathRenderer.render_rays`.

What the renderer takes from its sampler is one `occgrid.PackedSamples` record per call: the sampler's own `sample_packed(...)`
where it has one (the grids, `UniformSampler`, `PresetSampler`), else the three tensors of `.sampling` with the ranges they
imply (`HotPathRenderer._sampler_record`).  It reads nothing else of the sampler and writes nothing to it.  `_render_rays` is
four stages that hand values on: sample, place, query and composite, training terms.

Covered: the eval outputs (image, depth, sdf, weights, weights_sum, normal, deform, normal_raw) and
the deterministic training extras (loss_orient, loss_code, sdf_loss, fs_loss, normal_image).  The
randomised regularisers of morpheus.py:714-783 (normal perturbation / smoothness) reuse the same
model entry points and are implemented here on top of them.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import chunking, ops, resample
from .model import safe_normalize, scene_representation
from .occgrid import PackedSamples, PackedSampling, check_prune_args


class UniformSampler(PackedSampling):
    """Benchmark sampler of SURVEY 8(d) behind nerfacc's `.sampling` call shape: S equal bins per
    ray inside the AABB with one stratified jitter per ray (csrc/sampler.hip; the box clip is csrc/march.h's).  `jitter` pins
    the per-ray draws (PackedSampling.fixed_jitter); the record's `xyz` are the kernel's own midpoints o + d (ts+te)/2 (the same
    arithmetic as morpheus.py:647)."""

    def __init__(self, n_samples: int, bound: float, jitter: Optional[torch.Tensor] = None):
        self.n_samples, self.bound = n_samples, float(bound)
        self._init_sampling_state()
        self.fixed_jitter = jitter

    def sampling(self, rays_o, rays_d, sigma_fn=None, render_step_size=None, alpha_thre=0, stratified=True,
                 cone_angle=0.0, early_stop_eps=0, alpha_fn=None):
        """With a sigma_fn / alpha_fn the samples are pruned by visibility as occgrid.OccupancyGrid.sampling prunes them (there
        is no occupancy field here: alpha_thre is taken as given)."""
        return self.sample_packed(rays_o, rays_d, sigma_fn=sigma_fn, alpha_fn=alpha_fn, alpha_thre=alpha_thre,
                                  early_stop_eps=early_stop_eps, stratified=stratified, cone_angle=cone_angle)[:3]

    def _marcher(self, rays_o, rays_d, sigma_fn, alpha_fn, alpha_thre, early_stop_eps, render_step_size=None, cone_angle=0.0):
        if cone_angle != 0.0:
            raise NotImplementedError("cone marching (cone_angle != 0) is not implemented")
        check_prune_args(sigma_fn, alpha_fn, alpha_thre, early_stop_eps)

        def march(u, capacity):
            if capacity is not None:
                raise NotImplementedError("UniformSampler: every ray has n_samples samples; sample_capacity does not apply")
            if u is None:          # not stratified: the middle of every bin
                u = torch.full((rays_o.shape[0],), 0.5, device=rays_o.device)
            ri, ts, te, xyz, rs, rc = ops.sample_uniform(rays_o, rays_d, u, self.n_samples, self.bound, with_xyz=True)
            return (ri, ts, te, rs, rc), xyz

        return march, float          # no occupancy field: alpha_thre as given


class PresetSampler:
    """Feeds fixed packed samples (parity runs treat samples as inputs)."""

    def __init__(self, ray_indices, t_starts, t_ends):
        self.samples = (ray_indices, t_starts, t_ends)
        self._long = ray_indices.long()      # for the ranges of every call: the samples are fixed, the ray count is the call's

    def sampling(self, rays_o, rays_d, **kw):
        return self.samples

    def sample_packed(self, rays_o, rays_d, **kw) -> PackedSamples:
        return PackedSamples(*self.samples, *ops.packed_info(self._long, rays_o.shape[0]))


class FrameLayout(NamedTuple):
    """How the rays of one render_rays call map to frames, for every pass that needs a time per point"""
    single_frame: bool                  # every ray is one frame's and the render warps: the time travels as an expanded scalar
    ray_slots: Optional[Tuple[torch.Tensor, torch.Tensor]]   # several frames, one per batch row: (t_rows [B], slot per ray int32 [N])
    one_t: bool                         # every ray carries rays_t[0], canonical render or not


def frame_layout(prefix, frame_batched: bool, cano: bool, rays_t) -> FrameLayout:
    """`prefix`: the leading shape of the ray tensors; with frame_batched each row of [B, n] is ONE frame (how the reference's
    dataset builds every batch).  rays_t: [B * n, 1].  `one_t` deliberately ignores `cano`: the smoothness loss
    takes its normals at the rays' own times even in a canonical render (morpheus.py:548-553 warps always).  The per-row slots
    are what lets the model apply per-frame deform codes without a device->host sync."""
    rows = bool(frame_batched) and len(prefix) == 2
    one_t = rows and prefix[0] == 1
    ray_slots = None
    if rows and not one_t and not cano:
        ray_slots = (rays_t.view(*prefix)[:, 0].contiguous(),
                     torch.arange(prefix[0], device=rays_t.device, dtype=torch.int32).repeat_interleave(prefix[1]))
    return FrameLayout(one_t and not cano, ray_slots, one_t)


class _RayIndex:
    """the samples' ray indices as int64 (torch gathers) and int32 (the HIP kernels; the marcher and the uniform sampler already
    produce int32): each form is made once, and only if something asks for it"""
    __slots__ = ("given", "_long", "_i32")

    def __init__(self, given: torch.Tensor):
        self.given, self._long, self._i32 = given, None, None

    def long(self):
        if self._long is None:
            self._long = self.given.long()
        return self._long

    def i32(self):
        if self._i32 is None:
            self._i32 = self.given if self.given.dtype == torch.int32 else self.given.to(torch.int32)
        return self._i32


class _Rays(NamedTuple):
    """the flattened rays of one render_rays call"""
    o: torch.Tensor                     # [N, 3]
    d: torch.Tensor                     # [N, 3]
    t: torch.Tensor                     # [N, 1]
    prefix: tuple                       # the leading shape they came with
    cano: bool
    layout: FrameLayout


class _Placed(NamedTuple):
    """the samples of one render where the field is queried"""
    rec: PackedSamples
    idx: _RayIndex
    xyz: torch.Tensor                   # [M, 3]
    time_step: torch.Tensor             # [M, 1]
    frame_slots: Optional[Tuple[torch.Tensor, torch.Tensor]]   # (t_rows [B], slot per sample int32 [M]) with FrameLayout.ray_slots
    valid: Optional[torch.Tensor]       # fixed-capacity sampling: bool [M], the entries that are samples


class HotPathRenderer:
    def __init__(self, model: scene_representation, config: dict, occupancy_grid, num_frames: int,
                 frame_batched: bool = True):
        self.model, self.config, self.occupancy_grid, self.num_frames = model, config, occupancy_grid, num_frames
        # frame_batched: each row of the [B, N, .] ray tensors is ONE frame (how the reference's dataset
        # builds every batch) -> per-frame deform-code bias without a host sync.
        self.frame_batched = frame_batched
        # Opt-in visibility pruning: None (off, the reference's call), or dict(alpha_thre=..., early_stop_eps=...).  When set,
        # render_rays (and so eval_step) hands the sampler a sigma_fn of its own -- a density-only pass of the model under no_grad
        # -- and queries, composites and differentiates the samples that pass leaves visible only (_density_fn).
        self.prune: Optional[dict] = None
        # Opt-in importance resampling: None (off, the call as it is without it), or dict(n_importance=, det=False, jitter=None,
        # eps=1e-5).  When set, one density-only pass (_density_fn; the pruning pass's own when `prune` is set too) weighs the
        # sampler's intervals and resample.refine_samples cuts them at n_importance draws per ray; the render then carries
        # on with the refined samples as if the sampler had returned them.  config['render']['n_importance'] seeds it (absent
        # from the shipped configs).
        n_imp = int((config.get("render") or {}).get("n_importance", 0) or 0)
        self.importance: Optional[dict] = dict(n_importance=n_imp) if n_imp > 0 else None

    # -- helpers of morpheus.py:518-556
    def _const(self, key, build, device):
        """small device constants built once per device (a torch.tensor(list, device=...) is a host->device copy: a sync
        point of the eager step and illegal inside a captured HIP graph)"""
        c = self.__dict__.setdefault("_consts", {})
        k = (key, str(device))
        if k not in c:
            c[k] = build().to(device)
        return c[k]

    def get_ortho_normal_dir(self, normals, phi=None):
        """morpheus.py:518-528; `phi` injects the random angle (parity tests)."""
        n = torch.nn.functional.normalize(normals, dim=-1)
        # n[..., [1, 0, 2]] * (1, -1, 0) without host-built index / constant tensors (each is a host->device copy: a sync in the
        # eager step, illegal inside a captured HIP graph); the same three values
        u = torch.nn.functional.normalize(torch.stack([n[..., 1], -n[..., 0], n[..., 2] * 0.0], -1), dim=-1)
        v = torch.cross(n, u, dim=-1)
        if phi is None:
            phi = self._ortho_angle(normals)
        return torch.cos(phi) * u + torch.sin(phi) * v

    @staticmethod
    def _ortho_angle(normals):
        """the random angle of get_ortho_normal_dir (morpheus.py:525): one uniform draw per normal, times 2 pi"""
        # (fp32(2 pi) == 2 fp32(pi): one product gives the bits of the reference's `rand() * 2.0 * np.pi`)
        return torch.rand(list(normals.shape[:-1]) + [1], device=normals.device) * (2.0 * np.pi)

    def get_normal_smoothness_loss(self, rays_o, rays_d, rays_t, depth, offsets=None, phi=None, ray_slots=None,
                                   single_frame=None):
        """morpheus.py:530-556: normals at npts = trunc*100+1 points around the rendered depth of every ray vs normals at
        points displaced by smoothness_std along a random direction orthogonal to the normal.  The reference drops the
        points outside the 1.1 sphere with a boolean index (a device->host sync and a data-dependent shape); here they
        stay in the batch and leave the mean through a 0/1 weight -- the same value, no sync.
        `offsets` [npts] / `phi` [npts*N, 1] inject the two random draws (parity tests); `ray_slots` = (t_rows, slot per
        ray) for multi-frame batches; `single_frame`: every ray carries rays_t[0] (one batch row = one frame).  With neither,
        the points take their own ray's time, as the reference does (per-ray rays_t)."""
        trunc = self.config["train"]["trunc"]
        npts = int(trunc * 100 + 1)
        if offsets is None:
            off = self._const(("smooth_offsets", trunc, npts), lambda: torch.linspace(-0.5 * trunc, 0.5 * trunc, npts), depth.device)
            off = torch.add(off, torch.rand_like(off), alpha=0.01)
        else:
            off = offsets
        # pts = (depth + off[:, None])[..., None] * rays_d[None] + rays_o[None] and the 1.1-sphere test in one launch each way
        pts, keep = ops.smooth_points(depth, off.to(depth), rays_o, rays_d)
        n_rays = rays_t.shape[0]
        if ray_slots is not None:
            tt, fs = rays_t[None].repeat(npts, 1, 1).view(-1, 1), (ray_slots[0], ray_slots[1].repeat(npts))
        elif single_frame:         # one frame: the time is an expanded scalar (model._slots sees a single slot)
            tt, fs = rays_t[:1].expand(npts * n_rays, 1), None
        else:                      # rays of several times without a row structure: per-sample times (model._slots)
            tt, fs = rays_t[None].repeat(npts, 1, 1).view(-1, 1), None
        n1, _ = self.model.normal(pts, t=tt, frame_slots=fs)
        # pts + get_ortho_normal_dir(n1) * smoothness_std, then sum(square(n1 - n2) * keep) / max(3 sum(keep), 1): one launch each
        pts_p = ops.ortho_perturb(pts, n1, self._ortho_angle(n1) if phi is None else phi, self.config["train"]["smoothness_std"])
        n2, _ = self.model.normal(pts_p, t=tt, frame_slots=fs)
        return ops.masked_mean("sqdiff", n1, n2, row_weight=keep)

    # -- forward-only consumer (f-4)
    def eval_step(self, data, cano=False, optimize_pose=False, max_chunk=300 * 300):
        """MorpheuS.eval_step (morpheus.py:1238-1269; the same loop is in visualizer.py:69-91): a whole view rendered in
        chunks of <= max_chunk rays, forward only (callers wrap it in no_grad), RGB and depth images re-assembled."""
        rays_o, rays_d, rays_t, rays_id = data["rays_o"], data["rays_d"], data["rays_t"], data["rays_id"]
        B, N = rays_o.shape[:2]
        H, W = data["H"], data["W"]
        shading = data["shading"] if "shading" in data else "albedo"
        ambient_ratio = data["ambient_ratio"] if "ambient_ratio" in data else 1.0
        scale_factor = int(N // max_chunk + 1)
        if N > max_chunk:
            max_chunk = N // scale_factor + 1
        pred_rgb, pred_depth = [], []
        for i in range(0, N, max_chunk):
            out = self.render_rays(rays_o[:, i:i + max_chunk], rays_d[:, i:i + max_chunk], rays_t[:, i:i + max_chunk],
                                   rays_id[:, i:i + max_chunk], H, W, perturb=True, ambient_ratio=ambient_ratio,
                                   shading=shading, cano=cano, optimize_pose=optimize_pose)
            pred_rgb.append(out["image"])
            pred_depth.append(out["depth"])
        return torch.cat(pred_rgb, dim=1).reshape(B, H, W, 3), torch.cat(pred_depth, dim=1).reshape(B, H, W)

    def _density_fn(self, rays_o, rays_d, rays_t, cano, single_frame, ray_slots=None):
        """the sigma_fn of a pruned render (self.prune): density of the marched samples without colour, normals or autograd --
        the warp nets and the sdf net.  Runs inside the step's operand scope (an evaluation render prepares its weight operands
        once for this pass and the main one) and in row chunks when the call is large (chunking.rows_under_cap of a warp + one
        field query per row: nothing is parked without autograd, the chunks bound the pass's transient buffers the same way).
        ray_slots = (t_rows [B], slot per ray [N]) for a batch of several frames, as the main pass has them."""
        model = self.model
        o, d = rays_o.detach(), rays_d.detach()

        def sigma_fn(t_starts, t_ends, ray_indices):
            with torch.no_grad():
                x = ops.sample_positions_nograd(o, d, ray_indices, t_starts, t_ends)
                M = x.shape[0]
                slot = None
                if single_frame:       # a batch row is one frame: a single row travels as an expanded scalar, as in the main pass
                    t = rays_t[:1].expand(M, 1)
                elif ray_slots is not None:
                    t, slot = rays_t[ray_indices.long()], ray_slots[1][ray_indices.long()].contiguous()
                else:
                    t = rays_t[ray_indices.long()]
                rows = chunking.rows_under_cap(chunking.query_bytes_per_row(not cano, 1), device=x.device, rows=M)
                out = []
                for a_ in range(0, M, rows):
                    fs = None if slot is None else (ray_slots[0], slot[a_:a_ + rows])
                    out.append(model.density(x[a_:a_ + rows], t=t[a_:a_ + rows], cano=cano, return_color=False,
                                             frame_slots=fs)["sigma"].reshape(-1))
                return out[0] if len(out) == 1 else torch.cat(out)

        return sigma_fn

    _IMPORTANCE_KEYS = ("n_importance", "det", "jitter", "eps")

    def _importance_args(self) -> Optional[dict]:
        """self.importance checked: None when resampling is off (None, or n_importance = 0), else the dict with its defaults"""
        if not self.importance:
            return None
        unknown = set(self.importance) - set(self._IMPORTANCE_KEYS)
        if unknown:
            raise ValueError(f"HotPathRenderer.importance: unknown keys {sorted(unknown)} ({', '.join(self._IMPORTANCE_KEYS)})")
        args = dict(n_importance=0, det=False, jitter=None, eps=1e-5)
        args.update(self.importance)
        if int(args["n_importance"]) < 0:
            raise ValueError(f"HotPathRenderer.importance: n_importance = {args['n_importance']}")
        return args if int(args["n_importance"]) > 0 else None

    _PRUNE_KEYS = ("alpha_thre", "early_stop_eps")

    def _prune_args(self) -> Optional[dict]:
        """self.prune checked: None when pruning is off, else the two thresholds as floats (an absent one is 0)"""
        if not self.prune:
            return None
        unknown = set(self.prune) - set(self._PRUNE_KEYS)
        if unknown:
            raise ValueError(f"HotPathRenderer.prune: unknown keys {sorted(unknown)} ({', '.join(self._PRUNE_KEYS)})")
        return {k: float(self.prune.get(k, 0.0)) for k in self._PRUNE_KEYS}

    # -- the hot path
    def render_rays(self, rays_o, rays_d, rays_t, rays_id, H, W, perturb=True, bg_color=None, ambient_ratio=1.0,
                    light_d=None, shading="albedo", real_view=True, cano=False, rays_depth=None, rays_mask=None,
                    optimize_pose=False):
        with self.model.operand_scope():      # weight operands prepared once for every field query of this call
            return self._render_rays(rays_o, rays_d, rays_t, rays_id, H, W, perturb, bg_color, ambient_ratio, light_d,
                                     shading, real_view, cano, rays_depth, rays_mask, optimize_pose)

    def _render_rays(self, rays_o, rays_d, rays_t, rays_id, H, W, perturb, bg_color, ambient_ratio, light_d, shading,
                     real_view, cano, rays_depth, rays_mask, optimize_pose):
        """the stages in turn: sample, place, query and composite, training terms.  The order of torch's random draws is part of
        the contract (the golden tests inject them in call order): the sampler's jitter, light_d, the perturbation draws, the
        smoothness loss's offsets and angles."""
        prefix = rays_o.shape[:-1]
        rays_o = rays_o.contiguous().view(-1, 3)
        rays_d = rays_d.contiguous().view(-1, 3)
        rays_t = rays_t.contiguous().view(-1, 1)
        rays_id = rays_id.contiguous().view(-1, 1)
        if not cano and optimize_pose:
            rows = tuple(prefix) if (self.frame_batched and len(prefix) == 2) else None
            rays_o, rays_d = self.model.pose_optimisation(rays_o, rays_d, rays_id, rows=rows)
        if rays_depth is not None:
            rays_depth = rays_depth.contiguous().view(-1, 1)
        if rays_mask is not None:
            rays_mask = rays_mask.contiguous().view(-1, 1)
        rays = _Rays(rays_o, rays_d, rays_t, prefix, cano, frame_layout(prefix, self.frame_batched, cano, rays_t))

        rec = self._sample(rays)
        # per-sample light directions are only read by the shaded modes (model.py:515-531), and not at ambient_ratio = 1
        # (real-view steps), where the lambertian factor is exactly 1
        lit = shading != "albedo" and (ambient_ratio != 1 or shading in ("textureless", "normal"))
        if light_d is None and lit:
            light_d = safe_normalize(rays_o + torch.randn(3, device=rays_o.device))      # morpheus.py:641
        at = self._place(rays, rec)
        if rec.ray_indices.shape[0] == 0:
            # the reference falls into a NameError here; return the white image it intended
            return dict(image=torch.ones([*prefix, 3], device=rays_o.device), depth=torch.zeros([*prefix], device=rays_o.device),
                        sdf=None, weights=None, weights_sum=None, normal=None, deform=None, normal_raw=None)
        results, sigmas, chunk_rows = self._query_and_composite(rays, at, light_d if lit else None, shading, ambient_ratio,
                                                                real_view, bg_color)
        if self.model.training:
            self._training_terms(results, rays, at, sigmas, chunk_rows, real_view, rays_depth, rays_mask)
        return results

    def _sampler_record(self, rays_o, rays_d, **kw) -> PackedSamples:
        """the sampler's samples as a record: its own `sample_packed`, or -- anything with a nerfacc-style `.sampling` -- the
        three tensors it returns (int32 or int64 indices, as given) and the ranges they imply.  The one place that looks at what
        the sampler has."""
        sample_packed = getattr(self.occupancy_grid, "sample_packed", None)
        if sample_packed is not None:
            return sample_packed(rays_o, rays_d, **kw)
        ri, ts, te = self.occupancy_grid.sampling(rays_o, rays_d, **kw)
        return PackedSamples(ri, ts, te, *ops.packed_info(ri.long(), rays_o.shape[0]))

    @torch.no_grad()
    def _sample(self, rays: _Rays) -> PackedSamples:
        """Stage 1: the sampler's record; with `prune` the sampler is handed a density pass of the model to prune by, with
        `importance` the samples are then refined (resample.refine_samples) by the densities of one pass -- the pruning pass's
        own where there was one: the survivors take theirs through the record's src_index, so a render has one density pass."""
        importance, prune = self._importance_args(), self._prune_args()
        density = sigma_fn = None
        seen = []
        if prune or importance:
            density = self._density_fn(rays.o, rays.d, rays.t, rays.cano, rays.layout.single_frame, rays.layout.ray_slots)
        if prune:
            sigma_fn = density
            if importance:          # the resampling below weighs the survivors with the densities of this pass

                def sigma_fn(t_starts, t_ends, ray_indices):
                    seen.append(density(t_starts, t_ends, ray_indices))
                    return seen[0]

        prune = prune or dict(alpha_thre=0, early_stop_eps=0)
        rec = self._sampler_record(rays.o, rays.d, sigma_fn=sigma_fn, render_step_size=self.config["render"]["step_size"],
                                   alpha_thre=prune["alpha_thre"], stratified=True, cone_angle=0.0,
                                   early_stop_eps=prune["early_stop_eps"])
        if importance and rec.ray_indices.shape[0] > 0:
            if not seen:
                sigma = density(rec.t_starts, rec.t_ends, rec.ray_indices)
            else:
                sigma = seen[0] if rec.src_index is None else seen[0].index_select(0, rec.src_index.long())
            rec = resample.refine_samples(rec, int(importance["n_importance"]), sigmas=sigma, det=bool(importance["det"]),
                                          jitter=importance["jitter"], eps=float(importance["eps"]))
        return rec

    def _place(self, rays: _Rays, rec: PackedSamples) -> _Placed:
        """Stage 2: where and when the field is queried.  The positions are the sampler's own midpoints unless the rays carry a
        gradient (pose optimisation); the time of a sample is its ray's."""
        M = rec.ray_indices.shape[0]
        idx = _RayIndex(rec.ray_indices)
        # fixed-capacity sampling (occgrid.PackedSampling.sample_capacity): only the first n_valid packed entries are samples
        valid = None if rec.n_valid is None else (torch.arange(M, device=rays.o.device) < rec.n_valid)
        xyz = rec.xyz
        if xyz is None or rays.o.requires_grad or rays.d.requires_grad:
            # xyz = o[ri] + d[ri] * (ts + te) / 2 (morpheus.py:644-647) as one launch; its backward is a per-ray segment sum
            xyz = ops.sample_positions(rays.o, rays.d, idx.i32(), rec.t_starts, rec.t_ends, rec.ray_start, rec.ray_cnt)
        # a batch row is one frame: with a single row every sample shares rays_t[0] -- no gather needed, and the
        # model recognises the expanded scalar as a single deform-code slot by itself.  Several frames: slot per ray row.
        time_step = rays.t[:1].expand(M, 1) if rays.layout.single_frame else rays.t[idx.long()]
        frame_slots = None
        if rays.layout.ray_slots is not None:
            t_rows, slot_ray = rays.layout.ray_slots
            frame_slots = (t_rows, slot_ray[idx.long()].contiguous())
        return _Placed(rec, idx, xyz, time_step, frame_slots, valid)

    def _query_and_composite(self, rays: _Rays, at: _Placed, light_d, shading, ambient_ratio, real_view, bg_color):
        """Stage 3: the main field query (in row chunks when it would park too much), the compositor, the background blend
        -> (the result dict, the densities, the chunk length the query used).  light_d: None when the shading reads none."""
        model, cfg, rec, cano, prefix = self.model, self.config, at.rec, rays.cano, rays.prefix
        M_samples = rec.ray_indices.shape[0]
        t_light = None if light_d is None else light_d[at.idx.long()]
        # a bound on what the call parks (chunking.py): the main query and the perturbed-normal query of the regulariser in row
        # chunks when their estimate passes MORPHEUS_MAX_PARK_GB -- chunks but the last re-made in backward
        tr_ = cfg["train"]
        with_normals = shading != "albedo"
        perturb_query = model.training and tr_["normal_smooth_3d"] > 0 and with_normals
        row_bytes = chunking.query_bytes_per_row(not cano, 1 + (6 if with_normals else 0)) + \
            (chunking.query_bytes_per_row((not tr_["topo_none"]) and not cano, 6) if perturb_query else 0)
        chunk_rows = chunking.rows_under_cap(row_bytes, device=rays.o.device, rows=M_samples) if torch.is_grad_enabled() else M_samples
        t_rows, slot_rows = at.frame_slots if at.frame_slots is not None else (None, None)

        def main_query(x_, t_, l_, s_):
            return model(x_, t_, l_, ratio=ambient_ratio, shading=shading, cano=cano,
                         frame_slots=None if s_ is None else (t_rows, s_))

        sdf, sigmas, rgbs, normals, deform, normal_raw = chunking.chunked_query(main_query, (at.xyz, at.time_step, t_light, slot_rows),
                                                                                 chunk_rows, model=model)

        weights, opacity, depth, rgb_acc = ops.composite(sigmas, rec.t_starts.contiguous(), rec.t_ends.contiguous(), rgbs,
                                                         rec.ray_start, rec.ray_cnt, padded=at.valid is not None)
        opacity, depth = opacity[:, None], depth[:, None]
        if bg_color is None:
            if cfg["model"]["bg_radius"] > 0 and cano and (not real_view):
                bg_color = model.background(rays.d, rays.t)
            else:
                bg_color = 1
        if isinstance(bg_color, (int, float)) and rgb_acc.is_cuda:
            # a constant background (the reference's white, `bg_color = 1`): one cached [N, 3] constant, the same blend launch
            n_rays_ = rgb_acc.shape[0]
            bg_color = self._const(("bg", float(bg_color), n_rays_), lambda: torch.full((n_rays_, 3), float(bg_color)), rgb_acc.device)
        elif (torch.is_tensor(bg_color) and bg_color.is_cuda and not bg_color.requires_grad and bg_color.numel() == 3
              and bg_color.shape != rgb_acc.shape):
            bg_color = bg_color.reshape(1, 3).to(rgb_acc.dtype).expand(rgb_acc.shape[0], 3).contiguous()     # one colour for every ray
        if torch.is_tensor(bg_color) and bg_color.shape == rgb_acc.shape and bg_color.is_cuda:
            image = ops.bg_blend(rgb_acc, opacity, bg_color).view(*prefix, 3)       # the same three rounded operations, one launch
        else:
            image = (rgb_acc + (1 - opacity) * bg_color).view(*prefix, 3)
        results = dict(image=image, depth=depth.view(*prefix), sdf=sdf, weights=weights, weights_sum=opacity, normal=normals,
                       deform=deform, normal_raw=normal_raw)
        if at.valid is not None:
            results.update(valid=at.valid, n_valid=rec.n_valid)      # for the caller's own per-sample means (trainstep.sample_mean)
        return results, sigmas, chunk_rows

    def _training_terms(self, results, rays: _Rays, at: _Placed, sigmas, chunk_rows, real_view, rays_depth, rays_mask):
        """Stage 4: the regularisers and losses of a training render, added to `results`.  The means over two per-sample tensors
        [M, ...] (the reference's `(a - b).abs().mean()`) are ops.masked_mean("absdiff", ..., n_valid=) -- padding entries
        excluded, one launch each way."""
        model, tr, rec, cano = self.model, self.config["train"], at.rec, rays.cano
        xyzs, time_step, frame_slots, n_valid = at.xyz, at.time_step, at.frame_slots, rec.n_valid
        sdf, weights, normals, deform = results["sdf"], results["weights"], results["normal"], results["deform"]
        padded = at.valid is not None
        if tr["ori_weight"] > 0 and normals is not None and (not real_view):
            t_dirs = safe_normalize(rays.d[at.idx.long()])
            lo = weights.detach() * (normals * t_dirs).sum(-1).clamp(min=0) ** 2
            results["loss_orient"] = lo.sum(-1).mean()
        if tr["normal_smooth_3d"] > 0 and normals is not None:
            if tr["normal_dir"]:
                xyzs_p = ops.ortho_perturb(xyzs, normals, self._ortho_angle(normals), tr["smoothness_std"])
            else:
                xyzs_p = torch.add(xyzs, torch.randn_like(xyzs), alpha=tr["smoothness_std"])

            def perturbed_normals(x_, t_, s_):
                if tr["topo_none"]:
                    return model.normal(x_, topo=None, cano=cano)[:1]
                fs_ = None if s_ is None else (frame_slots[0], s_)
                return model.normal(x_, topo=model.get_topo(x_, t=t_, frame_slots=fs_), cano=cano)[:1]

            slot_rows = None if frame_slots is None else frame_slots[1]
            normals_p, = chunking.chunked_query(perturbed_normals, (xyzs_p, time_step, slot_rows), chunk_rows, model=model)
            results["loss_normal_perturb"] = ops.masked_mean("absdiff", normals, normals_p, n_valid=n_valid)
            if tr["normal_smooth_3d_t"] > 0:
                tt = time_step + torch.rand_like(time_step) * 1 / self.num_frames
                normals_pt, _ = model.normal(xyzs, topo=model.get_topo(xyzs, t=tt), cano=cano)
                results["loss_normal_perturb_t"] = ops.masked_mean("absdiff", normals, normals_pt, n_valid=n_valid)
            if tr["deform_smooth"] > 0 and not cano:
                deform_p, _, _ = model.warp(xyzs_p, t=time_step, frame_slots=frame_slots)
                results["loss_deform_perturb"] = ops.masked_mean("absdiff", deform, deform_p, n_valid=n_valid)
        if (tr["deform_smooth_t"] > 0 or tr["topo_smooth_t"] > 0) and not cano:
            tt = time_step + torch.rand_like(time_step) * 1 / self.num_frames
            deform_pt, topo_pt, _ = model.warp(xyzs, t=tt)
            topo_now = model.get_topo(xyzs, t=time_step, frame_slots=frame_slots)   # the reference reads an undefined `topo` here
            results["loss_deform_perturb_t"] = ops.masked_mean("absdiff", deform, deform_pt, n_valid=n_valid)
            results["loss_topo_perturb_t"] = ops.masked_mean("absdiff", topo_now, topo_pt, n_valid=n_valid)
        if tr["code_reg"] > 0 and not cano:
            # the three code samples (t0, t0 - 1/F, t0 + 1/F: morpheus.py:783-787) from ONE launch each way: the offsets are a
            # cached device constant (t0 + (-d) is t0 - d bit for bit), the rows come apart with unbind (one stack backward)
            d = 1.0 / self.num_frames
            offs = self._const(("code_reg_offsets", d), lambda: torch.tensor([[0.0], [-d], [d]]), time_step.device)
            code, cp, cn = model.get_deform_code(time_step[:1] + offs).unbind(0)
            # square(2 code - cp - cn).mean() with the chain's rounding ((2 code - cp) - cn): the difference and the mean in one launch
            results["loss_code"] = ops.masked_mean("sqdiff", (2 * code - cp)[None], cn[None])
        if tr["normal_smooth_2d"] > 0 and normals is not None and (not real_view):
            # accumulate_along_rays(weights, (normals+1)/2) with the LIVE weights (morpheus.py:775): the density
            # gradient of the normal image is part of the normal_smooth_2d loss
            _, _, _, nimg = ops.composite(sigmas, rec.t_starts.contiguous(), rec.t_ends.contiguous(), (normals + 1) / 2,
                                          rec.ray_start, rec.ray_cnt, padded=padded)
            results["normal_image"] = nimg
        if tr["normal_smoothness"] > 0:
            results["normal_reg"] = self.get_normal_smoothness_loss(rays.o, rays.d, rays.t, results["depth"].reshape(1, -1),
                                                                    ray_slots=rays.layout.ray_slots, single_frame=rays.layout.one_t)
        if rays_depth is not None:
            # get_sdf_loss (utils.py:91-113, morpheus.py:789) on the packed samples: one launch each way
            fs_loss, sdf_loss = ops.sdf_losses(sdf, rec.t_starts, rec.t_ends, at.idx.i32(), rays_depth, rays_mask, tr["trunc"], n_valid)
            results["sdf_loss"], results["fs_loss"] = sdf_loss, fs_loss
