"""`OccGridEstimator` -- nerfacc's occupancy estimator in full on HIP kernels (csrc/estimator.hip): levels, any axis-aligned
box, a non-cubic grid, cone steps, near / far planes and per-ray t_min / t_max, `mark_invisible_cells`, and an update that
never reads the device from the host.

    import morpheus_amd.volrend as nerfacc
    estimator = nerfacc.OccGridEstimator(aabb, resolution=128, levels=4).to("cuda")
    ray_indices, t_starts, t_ends = estimator.sampling(rays_o, rays_d, sigma_fn=sigma_fn, cone_angle=0.004)

nerfacc is third-party, un-vendored and not on any machine this project uses.  The class name, the buffers (`resolution` int32
[3], `aabbs` [levels,6], `occs` [levels * cells_per_lvl], `binaries` bool [levels,Rx,Ry,Rz]), the signatures and defaults of
`sampling`, `update_every_n_steps` and `mark_invisible_cells`, and the update rule are nerfacc 0.5.x's as RECALLED from its public
source: recalled, agreement unverified.

Two interval placements, chosen by the attribute `traversal` (not a buffer: `state_dict()` does not carry it):
  * "lattice" (the default): this build's fixed-lattice definition (csrc/march.h, the one march behind both classes), extended by
    levels, planes and cone steps: every ray walks t0 + k * step from clip entry to clip exit and keeps the steps whose midpoint
    lies in an occupied cell -- tests/estimator_oracle.py restates it in fp32;
  * "dda": the grid is walked cell by cell (mh_est_traverse_slots), empty cells are jumped to their exit and stepping starts
    again at the entry of the next occupied cell, so where a sample lies inside an occupied region depends on where the ray
    entered the REGION, not the clip box.  The rule is this build's statement of nerfacc's traverse_grids as recalled, agreement
    unverified, with one deliberate departure: a run of occupied cells starts its samples at max(its entry, the end of the ray's
    last sample), where the recalled rule restarts at the entry and lets two samples overlap behind an empty gap shorter than
    half a step -- `resample` and the compositor assume t_starts[k] >= t_ends[k-1] inside a ray.  tests/traverse_oracle.py
    restates it in fp32.
include/morpheus_hip.h states both and the kernels equal the restatements bit for bit.  `sampling`'s signature is nerfacc's and
stays so: `sampling_as(traversal, ...)` is `sampling` with the placement of that one call given.

`occgrid.OccupancyGrid` stays what the reference's own call uses.  Differences from it:
  * without a density function (`sigma_fn` / `alpha_fn`) `alpha_thre` and `early_stop_eps` are IGNORED, as nerfacc does --
    `OccupancyGrid.sampling` raises ValueError there; nerfacc's default early_stop_eps = 1e-4 would otherwise make the most
    common call raise;
  * the pruning threshold and the update's threshold use the mean of the NON-NEGATIVE occs (invisible cells hold -1);
  * post-warm-up updates draw the occupied quarter WITH replacement from a compacted list instead of a top-k over random keys.
With `levels=1`, a centred cubic box and default planes `sampling` returns `OccupancyGrid.sampling`'s samples bit for bit, and
the two classes load each other's `state_dict()`.

`sample_packed` is `occgrid.PackedSampling`'s: the same `PackedSamples` record as `OccupancyGrid` gives, remembered as `last`
(which `packed`, `src_index` and `n_valid` read), and `overflow`, `sample_capacity` and `fixed_jitter` with the same meaning, so
`HotPathRenderer(model, cfg, estimator, ...)` and the graph-captured step take this class unchanged.
There is no CPU path: CPU tensors raise MorpheusHipError, as everywhere in the package.
"""
from __future__ import annotations

import math
from typing import Callable, Optional

import numpy as np
import torch

from . import ops
from ._lib import MorpheusHipError
from .occgrid import PackedSampling

__all__ = ["OccGridEstimator", "level_aabbs"]

MAX_LEVELS = 16
TRAVERSALS = ("lattice", "dda")


def _traversal(value) -> str:
    if value not in TRAVERSALS:
        raise ValueError(f"OccGridEstimator: traversal is one of {TRAVERSALS}, got {value!r}")
    return value


def level_aabbs(roi_aabb, levels: int) -> np.ndarray:
    """float32 [levels, 6]: level l is the root box scaled by 2^l about its centre, formed in float64 and rounded once"""
    box = np.asarray(torch.as_tensor(roi_aabb, dtype=torch.float64).reshape(-1).tolist(), dtype=np.float64)
    if box.shape != (6,) or not np.isfinite(box).all() or not (box[3:] > box[:3]).all():
        raise ValueError(f"OccGridEstimator: roi_aabb is (x0, y0, z0, x1, y1, z1) with finite lo < hi on every axis, got {box.tolist()}")
    centre, half = (box[:3] + box[3:]) / 2.0, (box[3:] - box[:3]) / 2.0
    rows = [np.concatenate([centre - half * 2.0 ** l, centre + half * 2.0 ** l]) for l in range(levels)]
    out = np.stack(rows).astype(np.float32)
    if not (out[:, 3:] > out[:, :3]).all():
        raise ValueError(f"OccGridEstimator: roi_aabb {box.tolist()} is empty once rounded to float32")
    return out


class OccGridEstimator(PackedSampling, torch.nn.Module):
    def __init__(self, roi_aabb, resolution=128, levels: int = 1):
        super().__init__()
        if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not (1 <= levels <= MAX_LEVELS):
            raise ValueError(f"OccGridEstimator: levels is an int in [1, {MAX_LEVELS}], got {levels!r}")
        res = [int(resolution)] * 3 if isinstance(resolution, (int, np.integer)) else [int(r) for r in torch.as_tensor(resolution).reshape(-1).tolist()]
        if len(res) != 3 or min(res) < 1:
            raise ValueError(f"OccGridEstimator: resolution is a positive int or three of them, got {resolution!r}")
        self.levels = int(levels)
        self.cells_per_lvl = res[0] * res[1] * res[2]
        if self.levels * self.cells_per_lvl >= 2 ** 31:
            raise ValueError("OccGridEstimator: levels * cells_per_lvl must stay under 2^31")
        aabbs = level_aabbs(roi_aabb, self.levels)
        self.register_buffer("resolution", torch.tensor(res, dtype=torch.int32))
        self.register_buffer("aabbs", torch.from_numpy(aabbs))
        self.register_buffer("occs", torch.zeros(self.levels * self.cells_per_lvl))
        self.register_buffer("binaries", torch.zeros([self.levels] + res, dtype=torch.bool))
        self._res = tuple(res)
        self._set_diagonal(aabbs)
        self.thre: Optional[torch.Tensor] = None     # device scalar: the threshold of the last update
        self._traversal = "lattice"
        self._init_sampling_state()

    @property
    def traversal(self) -> str:
        """the interval placement of `sampling`: "lattice" (the default) or "dda"; any other value raises ValueError"""
        return self._traversal

    @traversal.setter
    def traversal(self, value):
        self._traversal = _traversal(value)

    def _set_diagonal(self, aabbs):
        # the slot-row bound needs the coarsest diagonal on the HOST: kept from construction / loading, never read back
        c = np.asarray(aabbs, dtype=np.float64)[-1]
        self._diagonal = float(math.sqrt(float(((c[3:] - c[:3]) ** 2).sum())))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        a = state_dict.get(prefix + "aabbs")
        if a is not None and tuple(a.shape) == tuple(self.aabbs.shape):
            self._set_diagonal(a.detach().cpu().numpy())

    # -- sampling --------------------------------------------------------------------------------
    def sampling(self, rays_o, rays_d, sigma_fn=None, alpha_fn=None, near_plane=0.0, far_plane=1e10, t_min=None, t_max=None,
                 render_step_size=1e-3, early_stop_eps=1e-4, alpha_thre=0.0, stratified=False, cone_angle=0.0):
        """nerfacc's OccGridEstimator.sampling (signature and defaults recalled, agreement unverified) -> (ray_indices int32,
        t_starts, t_ends): the first three fields of `sample_packed`'s record, which `self.last` keeps.
        sigma_fn / alpha_fn: fn(t_starts, t_ends, ray_indices) -> [M] densities / opacities of the marched samples; the samples
        with transmittance under early_stop_eps or opacity under min(alpha_thre, mean of the non-negative occs) are dropped
        (ops.visibility_prune) and the record's `src_index` holds the marched position of every returned sample.
        Without a density function the two thresholds are ignored, as nerfacc does -- `OccupancyGrid.sampling` raises there.
        t_min / t_max: float32 [n_rays] on the device.  `sample_capacity` set: fixed-length results and no host read.
        The placement is `self.traversal`; everything else here works alike on both."""
        return self.sample_packed(rays_o, rays_d, sigma_fn=sigma_fn, alpha_fn=alpha_fn, alpha_thre=alpha_thre,
                                  early_stop_eps=early_stop_eps, stratified=stratified, near_plane=near_plane, far_plane=far_plane,
                                  t_min=t_min, t_max=t_max, render_step_size=render_step_size, cone_angle=cone_angle)[:3]

    def _marcher(self, rays_o, rays_d, sigma_fn, alpha_fn, alpha_thre, early_stop_eps, near_plane=0.0, far_plane=1e10, t_min=None,
                 t_max=None, render_step_size=1e-3, cone_angle=0.0):
        if sigma_fn is not None and alpha_fn is not None:
            raise ValueError("sampling: give sigma_fn or alpha_fn, not both")
        if not (0.0 <= alpha_thre <= 1.0) or not (0.0 <= early_stop_eps <= 1.0):
            raise ValueError(f"sampling: alpha_thre ({alpha_thre}) and early_stop_eps ({early_stop_eps}) lie in [0, 1]")
        if not (render_step_size > 0) or not (cone_angle >= 0):
            raise ValueError(f"sampling: render_step_size ({render_step_size}) > 0 and cone_angle ({cone_angle}) >= 0")
        if not rays_o.is_cuda or not self.occs.is_cuda:
            raise MorpheusHipError("OccGridEstimator.sampling runs on an MI355X only (rays on %s, estimator on %s); there is "
                                   "no CPU path" % (rays_o.device, self.occs.device))

        rays = ops.est_traverse_rays if self._traversal == "dda" else ops.est_march_rays

        def march(u, capacity):
            return rays(rays_o, rays_d, u, float(render_step_size), self.aabbs, self.binaries.view(torch.uint8), self._diagonal,
                        float(cone_angle), float(near_plane), float(far_plane), t_min, t_max, capacity=capacity), None

        return march, lambda cap: ops.est_threshold(self.occs, cap)

    def sampling_as(self, traversal: str, rays_o, rays_d, **kw):
        """`sampling(rays_o, rays_d, **kw)` with the placement `traversal` for this one call; the attribute is left as it was"""
        keep, self._traversal = self._traversal, _traversal(traversal)
        try:
            return self.sampling(rays_o, rays_d, **kw)
        finally:
            self._traversal = keep

    # -- occupancy update -------------------------------------------------------------------------
    def make_draws(self, warmup: bool):
        """the random numbers of one update, drawn by torch on the device: u_point [L,n,3] in [0,1); post-warm-up also uniform
        int32 [L,k] in [0, cells_per_lvl) and u_occ [L,k] in [0,1), k = cells_per_lvl // 4, n = 2 k (warm-up: n = cells_per_lvl)"""
        L, cells, dev = self.levels, self.cells_per_lvl, self.occs.device
        k = cells // 4
        if warmup:
            return dict(u_point=torch.rand(L, cells, 3, device=dev))
        return dict(u_point=torch.rand(L, 2 * k, 3, device=dev), uniform=torch.randint(cells, (L, k), device=dev, dtype=torch.int32),
                    u_occ=torch.rand(L, k, device=dev))

    @torch.no_grad()
    def select_cells(self, warmup: bool, draws=None):
        """-> ids int32 [L,n] (-1: padding), points [L,n,3]: the cells of one update and the point to evaluate in each"""
        binary = self.binaries.view(torch.uint8)
        draws = self.make_draws(warmup) if draws is None else draws
        if warmup:
            return ops.est_select(self.aabbs, binary, True, draws["u_point"])
        occ_list, occ_cnt = ops.est_occupied_list(binary)
        return ops.est_select(self.aabbs, binary, False, draws["u_point"], draws["uniform"], draws["u_occ"], occ_list, occ_cnt)

    @torch.no_grad()
    def update_every_n_steps(self, step: int, occ_eval_fn: Callable, occ_thre: float = 1e-2, ema_decay: float = 0.95,
                             warmup_steps: int = 256, n: int = 16, draws=None):
        """nerfacc's update (recalled, agreement unverified), without a device->host read: every n-th step evaluate occ_eval_fn
        ([P,3] points -> [P] or [P,1]) at one jittered point per selected cell of every level -- all cells during warm-up,
        afterwards cells_per_lvl // 4 uniform draws and as many among the occupied cells (fewer occupied cells: each once, the
        rest padding) -- then occs = max(occs * ema_decay, occ) where evaluated (invisible cells, occs < 0, stay), `self.thre` =
        min(mean of the non-negative occs, occ_thre), binaries = occs > thre.  draws: make_draws' dict, to fix the random numbers."""
        if step % n != 0:
            return
        if not self.occs.is_cuda:
            raise MorpheusHipError("OccGridEstimator.update_every_n_steps runs on an MI355X only; there is no CPU path")
        if not (ema_decay >= 0):
            raise ValueError(f"update_every_n_steps: ema_decay ({ema_decay}) >= 0")
        ids, pts = self.select_cells(step < warmup_steps, draws)
        if ids.shape[1] > 0:
            ops.est_ema(ids, occ_eval_fn(pts.view(-1, 3)), self.occs, float(ema_decay))
        if self.thre is None or self.thre.device != self.occs.device:
            self.thre = torch.zeros((), device=self.occs.device)
        ops.est_threshold(self.occs, float(occ_thre), self.thre, self.binaries.view(torch.uint8))

    @torch.no_grad()
    def mark_invisible_cells(self, K, c2w, width: int, height: int, near_plane: float = 0.0):
        """nerfacc's mark_invisible_cells (recalled, agreement unverified): occs = 0 for the cells some camera sees at a depth
        >= near_plane and no camera sees nearer, -1 for the others, which no update touches again.  K [3,3] or [C,3,3], c2w
        [C,3,4] or [C,4,4], OpenCV convention (x right, y down, z forward)."""
        if not self.occs.is_cuda or not c2w.is_cuda or not K.is_cuda:
            raise MorpheusHipError("OccGridEstimator.mark_invisible_cells runs on an MI355X only; there is no CPU path")
        if c2w.dim() != 3 or tuple(c2w.shape[1:]) not in ((3, 4), (4, 4)):
            raise ValueError(f"mark_invisible_cells: c2w [C,3,4] or [C,4,4], got {tuple(c2w.shape)}")
        C = c2w.shape[0]
        if tuple(K.shape) not in ((3, 3), (C, 3, 3)):
            raise ValueError(f"mark_invisible_cells: K [3,3] or [{C},3,3], got {tuple(K.shape)}")
        K = K.float().expand(C, 3, 3).contiguous()
        ops.est_mark_invisible(K, c2w[:, :3, :4].float().contiguous(), int(width), int(height), float(near_plane), self.aabbs,
                               self.binaries.view(torch.uint8), self.occs)

    def set_binary(self, binary: torch.Tensor):
        """Install the binary grids directly (tests / loading an external estimator)."""
        self.binaries.copy_(binary.to(torch.bool).view_as(self.binaries))
