"""`OccupancyGrid` -- stands where nerfacc's `OccGridEstimator` stands in the reference
(morpheus.py:196-202 construction, :628-638 sampling, :905-913 update, :341,355 checkpoint key 'estimator').

nerfacc is third-party, un-vendored and version un-pinned in the reference (docs/INSTALL.md:21), so the semantics
here follow its published 0.5.x behaviour as summarised in SURVEY.md C.9 and are otherwise defined by this build:
  * binary grid resolution^3 over the AABB; `occs` float EMA-max field;
  * update_every_n_steps(step, occ_eval_fn, occ_thre=1e-2, ema_decay=0.95, warmup_steps=256, n=16): every n-th step
    evaluate occ_eval_fn at one jittered point per selected cell (all cells during warm-up, afterwards a quarter
    uniformly at random plus a quarter of the occupied ones), occs = max(occs*decay, new),
    binaries = occs > min(mean(occs), occ_thre);
  * sampling(...): fixed-step marching of the occupied cells with one stratified near-plane jitter per ray
    (csrc/sampler.hip:march_wave_kernel, the march of csrc/march.h).  With a sigma_fn or alpha_fn the marched samples are then
    pruned by visibility (csrc/visibility.hip: T >= early_stop_eps and alpha >= min(alpha_thre, mean(occs)), include/morpheus_hip.h; recalled
    from nerfacc 0.5.x, NOT verified).  The reference passes sigma_fn=None, alpha_thre=0, early_stop_eps=0: no pruning,
    the marcher's samples as they are.  Cone marching (cone_angle != 0) is not implemented.
`sampling` returns nerfacc's three tensors; `sample_packed` (PackedSampling) returns everything a consumer of the samples needs
as one PackedSamples record -- the three tensors, the rays' ranges, the fixed-capacity count, the pruning's source positions,
midpoints where the kernel made them -- and `sampling` is its first three fields.
The heavy part of an update is occ_eval_fn = model.density on up to resolution^3 points, which runs on the HIP kernels.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional

import torch

from . import ops


def check_prune_args(sigma_fn, alpha_fn, alpha_thre, early_stop_eps):
    """the argument rules of visibility pruning shared by every sampler with nerfacc's `.sampling` call shape"""
    if sigma_fn is not None and alpha_fn is not None:
        raise ValueError("sampling: give sigma_fn or alpha_fn, not both")
    if sigma_fn is None and alpha_fn is None and (alpha_thre > 0 or early_stop_eps > 0):
        raise ValueError("sampling: alpha_thre / early_stop_eps prune by visibility and a density function is required "
                         "(sigma_fn or alpha_fn); nerfacc silently ignores the thresholds without one")
    if not (0.0 <= alpha_thre <= 1.0) or not (0.0 <= early_stop_eps <= 1.0):
        raise ValueError(f"sampling: alpha_thre ({alpha_thre}) and early_stop_eps ({early_stop_eps}) lie in [0, 1]")


class PackedSamples(NamedTuple):
    """The packed samples of one sampling call, as every consumer takes them: rec[:3] is nerfacc's (ray_indices, t_starts,
    t_ends).  A plain tuple of tensors built on the host -- no launch, no device read, nothing registered on a module."""
    ray_indices: torch.Tensor
    t_starts: torch.Tensor
    t_ends: torch.Tensor
    ray_start: torch.Tensor                       # int32 [N]: where every ray's samples begin
    ray_cnt: torch.Tensor                         # int32 [N]
    n_valid: Optional[torch.Tensor] = None        # fixed-capacity sampling: int32 0-dim device count of the entries that are samples
    src_index: Optional[torch.Tensor] = None      # pruned sampling: int32 [M], the position every sample had before (None: nothing was pruned)
    xyz: Optional[torch.Tensor] = None            # [M, 3] midpoints o + d (ts + te) / 2 where the sampler's kernel already produced them


class PackedSampling:
    """What `OccupancyGrid`, `estimator.OccGridEstimator` and `render.UniformSampler` share: `sample_packed`, the one path from
    `sampling`'s arguments to a PackedSamples record; the class keeps its own argument rules, its march and its threshold
    (`_marcher`).  State, with the same meaning in every class:
      last      the record of the last call; `packed` = (ray_start, ray_cnt), `src_index` and `n_valid` read it
      fixed_jitter  parity runs pin the per-ray jitter (a float: one value for every ray, chunk-invariant; a tensor: per ray)
      sample_capacity  None = off: ragged packed samples sized by one device->host sync, as nerfacc does.  With a capacity the
                packed arrays always have that length, the first `n_valid` (a device int) entries are the samples and the rest is
                padding no ray owns: constant shapes and no sync, so a whole training step can be captured in a HIP graph
                (trainstep.GraphedRealViewStep).  `overflow` (device int, sticky) is set when a batch had more samples than the
                capacity -- its tail rays were truncated -- and is the caller's cue to raise the capacity."""

    def _init_sampling_state(self):
        self.last: Optional[PackedSamples] = None
        self.fixed_jitter: Optional[torch.Tensor] = None
        self.sample_capacity: Optional[int] = None
        self.overflow: Optional[torch.Tensor] = None

    packed = property(lambda self: None if self.last is None else (self.last.ray_start, self.last.ray_cnt))
    src_index = property(lambda self: None if self.last is None else self.last.src_index)
    n_valid = property(lambda self: None if self.last is None else self.last.n_valid)

    @torch.no_grad()
    def sample_packed(self, rays_o, rays_d, sigma_fn=None, alpha_fn=None, alpha_thre=0.0, early_stop_eps=0.0, stratified=False,
                      **how) -> PackedSamples:
        """`sampling`'s arguments (`how`: the class's own, by keyword) -> the record, which `last` remembers: the jitter choice,
        the march, the optional visibility pruning.  self._marcher(rays_o, rays_d, sigma_fn, alpha_fn, alpha_thre, early_stop_eps,
        **how) checks the arguments by the class's rules and gives march(u, capacity) -> (the ragged five results or, with a
        capacity, the fixed-capacity seven of ops.march_rays / ops.march_rays_capped, the midpoints or None) and
        threshold(alpha_thre) -> the pruning threshold, a float or a device scalar."""
        march, threshold = self._marcher(rays_o, rays_d, sigma_fn, alpha_fn, alpha_thre, early_stop_eps, **how)
        n, dev = rays_o.shape[0], rays_o.device
        if isinstance(self.fixed_jitter, float):
            u = torch.full((n,), self.fixed_jitter, device=dev)
        elif self.fixed_jitter is not None:
            u = self.fixed_jitter
        elif stratified:
            u = torch.rand(n, device=dev)
        else:
            u = None
        capped = self.sample_capacity is not None
        out, xyz = march(u, int(self.sample_capacity) if capped else None)
        ri, ts, te, rs, rc = out[:5]
        n_valid = src = None
        if capped:
            n_valid = out[5]
            if self.overflow is None:
                self.overflow = torch.zeros((), dtype=torch.int32, device=dev)
            self.overflow.copy_(torch.maximum(self.overflow, out[6]))
        fn = sigma_fn if sigma_fn is not None else alpha_fn
        if fn is not None and ts.shape[0] > 0:
            thre = threshold(float(alpha_thre)) if alpha_thre > 0 else None      # formed on the device
            out = ops.visibility_prune(fn(ts, te, ri), ts, te, rs, rc, float(early_stop_eps), thre, alpha_form=sigma_fn is None,
                                       padded=capped)
            ri, ts, te, rs, rc, src = out[:6]
            if capped:
                n_valid = out[6]
            if xyz is not None:
                xyz = xyz.index_select(0, src.long())
        self.last = PackedSamples(ri, ts, te, rs, rc, n_valid, src, xyz)
        return self.last


class OccupancyGrid(PackedSampling, torch.nn.Module):
    def __init__(self, roi_aabb, resolution: int = 128):
        super().__init__()
        aabb = torch.as_tensor(roi_aabb, dtype=torch.float32).reshape(-1)
        assert aabb.numel() == 6
        b = float(aabb[3])
        assert torch.allclose(aabb[:3], -aabb[3:]) and torch.allclose(aabb[3:], aabb[3:4].expand(3)), \
            "the marcher assumes the reference's cubic AABB [-bound, bound]^3 (morpheus.py:113-127)"
        self.bound = b
        R = int(resolution)
        # buffer names / shapes / dtypes of nerfacc 0.5.x's OccGridEstimator with levels = 1 (as recalled from its public
        # source; the package is not in the reference tree): resolution int32 [3], aabbs [1,6], occs [R^3],
        # binaries bool [1,R,R,R] -- so that the reference's checkpoint entry 'estimator' (morpheus.py:341,355) loads
        self.register_buffer("resolution", torch.tensor([R, R, R], dtype=torch.int32))
        self.register_buffer("aabbs", aabb[None].clone())
        self.register_buffer("occs", torch.zeros(R ** 3))
        self.register_buffer("binaries", torch.zeros(1, R, R, R, dtype=torch.bool))
        self._R = R
        self._init_sampling_state()

    # -- sampling --------------------------------------------------------------------------------
    def sampling(self, rays_o, rays_d, sigma_fn=None, render_step_size=1e-3, alpha_thre=0.0, stratified=False,
                 cone_angle=0.0, early_stop_eps=0.0, alpha_fn=None):
        """nerfacc's OccGridEstimator.sampling -> (ray_indices, t_starts, t_ends): the first three fields of `sample_packed`'s
        record, which `self.last` keeps.  sigma_fn / alpha_fn: called as fn(t_starts, t_ends, ray_indices) -> [M] densities /
        opacities of the marched samples (not called when there is none); the samples with transmittance under early_stop_eps
        or opacity under min(alpha_thre, mean(occs)) are dropped (ops.visibility_prune), the record's `src_index` then holds the
        marched position of every returned sample.  The defaults are the reference's call (no pruning); nerfacc's own default
        early_stop_eps is 1e-4.  nerfacc silently ignores alpha_thre / early_stop_eps when neither function is given; here that
        is a ValueError."""
        return self.sample_packed(rays_o, rays_d, sigma_fn=sigma_fn, alpha_fn=alpha_fn, alpha_thre=alpha_thre,
                                  early_stop_eps=early_stop_eps, stratified=stratified, render_step_size=render_step_size,
                                  cone_angle=cone_angle)[:3]

    def _marcher(self, rays_o, rays_d, sigma_fn, alpha_fn, alpha_thre, early_stop_eps, render_step_size=1e-3, cone_angle=0.0):
        if cone_angle != 0.0:
            raise NotImplementedError("cone marching (cone_angle != 0) is not used by the reference's call "
                                      "(morpheus.py:629-638) and is not implemented")
        check_prune_args(sigma_fn, alpha_fn, alpha_thre, early_stop_eps)
        # a bool tensor is one byte per cell holding 0/1: the marcher reads it as uint8 without a copy
        binary, step = self.binaries[0].view(torch.uint8), float(render_step_size)

        def march(u, capacity):
            if capacity is None:
                return ops.march_rays(rays_o, rays_d, u, step, self.bound, binary), None
            return ops.march_rays_capped(rays_o, rays_d, u, step, self.bound, binary, capacity), None

        # nerfacc's rule: the opacity threshold never exceeds the grid's mean occupancy value
        return march, lambda cap: torch.clamp(self.occs.mean(), max=cap)

    # -- occupancy update -------------------------------------------------------------------------
    def _cell_points(self, idx: torch.Tensor) -> torch.Tensor:
        R = self._R
        ijk = torch.stack([idx // (R * R), (idx // R) % R, idx % R], -1).float()
        x = (ijk + torch.rand_like(ijk)) / R                       # [0,1]^3, one jittered point per cell
        return x * (2 * self.bound) - self.bound

    @torch.no_grad()
    def update_every_n_steps(self, step: int, occ_eval_fn: Callable, occ_thre: float = 1e-2, ema_decay: float = 0.95,
                             warmup_steps: int = 256, n: int = 16):
        if step % n != 0:
            return
        R3, dev = self._R ** 3, self.occs.device
        if step < warmup_steps:
            idx = torch.arange(R3, device=dev)
        else:
            # a quarter of the cells uniformly at random plus up to a quarter drawn among the occupied ones -- without the
            # device->host sync of a nonzero(): every cell gets a random key, unoccupied cells key 0, and the k largest keys
            # are k occupied cells drawn without replacement (fewer occupied cells than k: the zero-key remainder re-evaluates
            # unoccupied cells, which only refreshes them).  Fixed shapes: k + k points every refresh.
            k = R3 // 4
            uni = torch.randint(R3, (k,), device=dev)
            keys = torch.rand(R3, device=dev) * self.binaries.reshape(-1)
            occ_idx = torch.topk(keys, k, sorted=False).indices
            idx = torch.cat([uni, occ_idx])
        occ = occ_eval_fn(self._cell_points(idx)).reshape(-1).float()
        # EMA-max update.  `idx` may name a cell more than once (two uniform draws, or a uniform and an occupied draw): the
        # cell then takes the LARGEST of its evaluations -- a scatter-max, deterministic -- where an indexed assignment
        # would keep whichever duplicate the hardware wrote last.
        new = torch.maximum(self.occs[idx] * ema_decay, occ)
        self.occs.scatter_reduce_(0, idx, new, reduce="amax", include_self=False)
        thre = torch.clamp(self.occs.mean(), max=occ_thre)
        self.binaries.copy_((self.occs > thre).view_as(self.binaries))

    def set_binary(self, binary: torch.Tensor):
        """Install a binary grid directly (tests / loading an external estimator)."""
        self.binaries.copy_(binary.to(torch.bool).view_as(self.binaries))
