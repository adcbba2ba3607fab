"""nerfacc's volume-rendering functions on HIP kernels (csrc/volrend.hip), forward and backward.

    import morpheus_amd.volrend as nerfacc

lets a render loop written against nerfacc 0.5.x -- the reference's own `render_rays` (morpheus.py:675-685, :775), or a fork of
it with one more accumulated channel, another background rule or an alpha-based field -- run on an MI355X with nothing from
nerfacc installed.  `HotPathRenderer` does not go through here: it keeps the fused compositor (ops.composite), which does the
reference's four calls in one launch.  `OccGridEstimator` (morpheus_amd/estimator.py), the other half of such a loop, is exported
here too, so that `nerfacc.OccGridEstimator` resolves.

nerfacc is third-party, un-vendored and does not build on ROCm, so it is not on the machine this module was written on.  Names,
argument names, argument order, defaults and result shapes below are nerfacc 0.5.x's AS RECALLED from its public documentation;
neither they nor the numbers are verified against it (tools/check_against_nerfacc.py compares where nerfacc is installed).

Definitions, per ray over its samples in order, sd_i = sigma_i (t_ends_i - t_starts_i):
    density form   alpha_i = 1 - exp(-sd_i), computed as -expm1(-sd_i);   T_i = exp(-sum_{j<i} sd_j)
    alpha form     T_i = prod_{j<i} (1 - alpha_j)                          (alphas are taken as <= 1)
    both           w_i = T_i alpha_i
    accumulate     out[r, c] = sum_{i in r} w_i values[i, c]; a ray without samples gives exactly 0

Two input layouts, as in nerfacc:
    packed   1-D sample arrays with `packed_info` ([n_rays, 2] (start, count), what pack_info returns) or with `ray_indices`
             (int32 or int64) + `n_rays`.  `ray_indices` must be NON-DECREASING -- the precondition of nerfacc's own packed
             functions; it is not checked.  `ray_indices` without `n_rays` raises ValueError.  Every call that is given
             `ray_indices` finds the ray boundaries again (one small launch, no host synchronisation); a loop that makes several
             calls can pass `packed_info=pack_info(ray_indices, n_rays)` instead, with bit-identical results.
    dense    2-D [n_rays, n_samples] arrays with neither index: n_rays rays of equal count; outputs keep the 2-D shape and
             `values` is [n_rays, n_samples, D].

`prefix_trans` is multiplied onto `trans` (and onto the weights) in plain torch behind the kernel, so autograd carries it.

Gradients go to `sigmas`, `alphas`, `weights` and `values`.  `t_starts` / `t_ends` that require a gradient raise
NotImplementedError (the reference samples under no_grad, and the kernel forms sigma * dt itself).  All outputs are
differentiable and any subset of their gradients may be absent.

Where this differs from nerfacc, knowingly: the gradient of the alpha form is the product with the sample's own factor LEFT OUT,
    dL/dalpha_i = g_w_i T_i - sum_{j>i} (g_w_j alpha_j + g_T_j) prod_{k<j, k != i} (1 - alpha_k),
finite and correct at alpha_i == 1 exactly.  nerfacc divides T_j by (1 - alpha_i) and returns inf / NaN there (as recalled).
Non-finite sigma follows the compositor: +inf takes the remaining transmittance with exact zeros behind it, a NaN poisons its own
ray only (forward; the backward is unspecified there).

There is no CPU path: CPU tensors and a missing library raise MorpheusHipError, as everywhere in the package.  Empty inputs return
correctly shaped zeros without a launch.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Tuple

import torch
from torch import Tensor

from . import ops
from ._lib import MorpheusHipError, ptr, require_gpu
from .estimator import OccGridEstimator      # the other half of a nerfacc render loop: `nerfacc.OccGridEstimator` resolves
from .ops import _timed

__all__ = ["pack_info", "render_transmittance_from_density", "render_transmittance_from_alpha", "render_weight_from_density",
           "render_weight_from_alpha", "accumulate_along_rays", "render_visibility_from_density", "render_visibility_from_alpha",
           "rendering", "MorpheusHipError", "OccGridEstimator"]

MAX_CHANNELS = 256


# ------------------------------------------------------------------------------------------------------------ ray layout
def _ray_ranges(ray_indices: Tensor, n_rays: int) -> Tuple[Tensor, Tensor]:
    """(ray_start, ray_cnt) int32 [n_rays] of non-decreasing ray_indices: mh_pack_info, one launch, no host synchronisation"""
    require_gpu(ray_indices)
    if ray_indices.dtype not in (torch.int32, torch.int64) or ray_indices.dim() != 1:
        raise ValueError(f"ray_indices: a 1-D int32 or int64 tensor expected, got {ray_indices.dtype} {tuple(ray_indices.shape)}")
    n_rays, dev = int(n_rays), ray_indices.device
    if n_rays < 0:
        raise ValueError(f"n_rays = {n_rays}")
    M = ray_indices.shape[0]
    if M == 0 or n_rays == 0:
        return torch.zeros(n_rays, dtype=torch.int32, device=dev), torch.zeros(n_rays, dtype=torch.int32, device=dev)
    idx = ray_indices.detach().contiguous()
    rs, rc = torch.empty(n_rays, dtype=torch.int32, device=dev), torch.empty(n_rays, dtype=torch.int32, device=dev)
    _timed("mh_pack_info", ptr(idx), 1 if idx.dtype == torch.int64 else 0, M, n_rays, ptr(rs), ptr(rc))
    return rs, rc


def pack_info(ray_indices: Tensor, n_rays: Optional[int] = None) -> Tensor:
    """-> packed_info int64 [n_rays, 2]: (start, count) of every ray's samples in the packed arrays, the rays without samples
    included.  ray_indices: int32 or int64, non-decreasing (not checked).  nerfacc takes max + 1 for a missing n_rays, which
    costs a host read; here n_rays is required."""
    if n_rays is None:
        raise ValueError("pack_info: ray_indices without n_rays (the ray count cannot be read off the indices without a host read)")
    rs, rc = _ray_ranges(ray_indices, n_rays)
    return torch.stack((rs, rc), dim=1).long()


class _Layout:
    """what the kernels need to know of a call's rays: ray_start / ray_cnt int32 [N], the shape the per-sample results take, and
    whether some packed entries may belong to no ray (a caller's packed_info: such entries read as 0)"""

    def __init__(self, like: Tensor, packed_info, ray_indices, n_rays, what: str):
        require_gpu(like, packed_info, ray_indices)
        self.shape, dev = tuple(like.shape), like.device
        self.M = like.numel()
        if like.dim() == 2 and packed_info is None and ray_indices is None:
            self.N, S = self.shape
            self.rs = torch.arange(self.N, dtype=torch.int32, device=dev) * S
            self.rc = torch.full((self.N,), S, dtype=torch.int32, device=dev)
            self.dense, self.gaps = True, False
            return
        if like.dim() != 1:
            raise ValueError(f"{what}: 1-D packed arrays with packed_info or ray_indices + n_rays, or 2-D [n_rays, n_samples] arrays "
                             f"with neither, got shape {self.shape}")
        self.dense = False
        if packed_info is not None:
            if packed_info.dim() != 2 or packed_info.shape[1] != 2 or packed_info.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"{what}: packed_info is an integer [n_rays, 2] tensor of (start, count), got "
                                 f"{packed_info.dtype} {tuple(packed_info.shape)}")
            self.N = packed_info.shape[0]
            self.rs = packed_info[:, 0].to(torch.int32).contiguous()
            self.rc = packed_info[:, 1].to(torch.int32).contiguous()
            self.gaps = True
        elif ray_indices is not None:
            if n_rays is None:
                raise ValueError(f"{what}: ray_indices without n_rays")
            if ray_indices.shape != like.shape:
                raise ValueError(f"{what}: one ray index per sample, got {tuple(ray_indices.shape)} for {self.shape}")
            self.N = int(n_rays)
            self.rs, self.rc = _ray_ranges(ray_indices, self.N)
            self.gaps = False
        else:
            raise ValueError(f"{what}: 1-D packed arrays need packed_info or ray_indices + n_rays")


def _f32(t: Tensor, what: str) -> Tensor:
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: float32 expected, got {t.dtype}")
    return t


def _no_grad_t(t_starts, t_ends):
    if t_starts.requires_grad or t_ends.requires_grad:
        raise NotImplementedError("gradients to t_starts / t_ends are not implemented (the reference samples under no_grad; the "
                                  "kernel forms sigma * (t_ends - t_starts) itself)")


# ------------------------------------------------------------------------------------------------------------ weights
class _RayWeights(torch.autograd.Function):
    """(weights, trans, alphas) of the density form, (weights, trans) of the alpha form; any subset of the incoming gradients may
    be absent (NULL pointers, as _Composite).  The density form's backward reads the saved transmittance; the alpha form's
    recomputes its scan (it needs the product without the zero factors, which no output holds)."""

    @staticmethod
    def forward(ctx, values, t_starts, t_ends, rs, rc, gaps, alpha_form, with_weights):
        ctx.set_materialize_grads(False)
        v = values.detach().reshape(-1).contiguous()
        ts = None if alpha_form else t_starts.detach().reshape(-1).contiguous()
        te = None if alpha_form else t_ends.detach().reshape(-1).contiguous()
        new = torch.zeros_like if gaps else torch.empty_like
        weights, trans = (new(v) if with_weights else None), new(v)      # the transmittance-only calls write no weights
        alphas = None if alpha_form else new(v)
        _timed("mh_ray_weights_fwd", ptr(v), ptr(ts), ptr(te), 1 if alpha_form else 0, ptr(rs), ptr(rc), rs.shape[0], ptr(weights),
               ptr(trans), ptr(alphas))
        ctx.alpha_form, ctx.gaps, ctx.shape = alpha_form, gaps, values.shape
        ctx.save_for_backward(v, ts, te, rs, rc, trans)
        shape = values.shape
        weights = None if weights is None else weights.view(shape)
        if alpha_form:
            return weights, trans.view(shape)
        return weights, trans.view(shape), alphas.view(shape)

    @staticmethod
    def backward(ctx, g_w, g_T, g_a=None):
        v, ts, te, rs, rc, trans = ctx.saved_tensors
        c = lambda t: None if t is None else t.reshape(-1).contiguous()
        d = torch.zeros_like(v) if ctx.gaps else torch.empty_like(v)
        _timed("mh_ray_weights_bwd", ptr(v), ptr(ts), ptr(te), 1 if ctx.alpha_form else 0, ptr(rs), ptr(rc), rs.shape[0], ptr(trans),
               ptr(c(g_w)), ptr(c(g_T)), ptr(c(g_a)), ptr(d))
        return d.view(ctx.shape), None, None, None, None, None, None, None


def _weights(values, t_starts, t_ends, packed_info, ray_indices, n_rays, prefix_trans, alpha_form: bool, what: str, with_weights=True):
    """-> (weights-or-None, trans, alphas-or-None) in the layout of `values`, prefix_trans applied"""
    require_gpu(values, t_starts, t_ends, prefix_trans)
    _f32(values, what)
    if not alpha_form:
        _no_grad_t(t_starts, t_ends)
        if _f32(t_starts, what).shape != values.shape or _f32(t_ends, what).shape != values.shape:
            raise ValueError(f"{what}: t_starts, t_ends and sigmas of one shape, got {tuple(t_starts.shape)}, {tuple(t_ends.shape)}, "
                             f"{tuple(values.shape)}")
    lay = _Layout(values, packed_info, ray_indices, n_rays, what)
    if lay.M == 0 or lay.N == 0:
        z = values * 0.0                                 # correctly shaped zeros, no launch; stays in the graph
        outs = (z if with_weights else None, z.clone(), None if alpha_form else z.clone())
    else:
        outs = _RayWeights.apply(values, t_starts, t_ends, lay.rs, lay.rc, lay.gaps, alpha_form, with_weights)
        outs = tuple(outs) + ((None,) if alpha_form else ())
    weights, trans, alphas = outs
    if prefix_trans is not None:                         # one value per sample, as in nerfacc; plain torch: autograd carries it
        if prefix_trans.shape != values.shape:
            raise ValueError(f"{what}: prefix_trans of shape {tuple(values.shape)} expected, got {tuple(prefix_trans.shape)}")
        trans = trans * prefix_trans
        if with_weights:
            weights = trans * (values if alpha_form else alphas)
    return weights, trans, alphas


def render_transmittance_from_density(t_starts: Tensor, t_ends: Tensor, sigmas: Tensor, packed_info: Optional[Tensor] = None,
                                      ray_indices: Optional[Tensor] = None, n_rays: Optional[int] = None,
                                      prefix_trans: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """-> (trans, alphas): T_i = exp(-sum_{j<i} sigma_j dt_j), alpha_i = 1 - exp(-sigma_i dt_i)"""
    _, trans, alphas = _weights(sigmas, t_starts, t_ends, packed_info, ray_indices, n_rays, prefix_trans, False,
                                "render_transmittance_from_density", with_weights=False)
    return trans, alphas


def render_transmittance_from_alpha(alphas: Tensor, packed_info: Optional[Tensor] = None, ray_indices: Optional[Tensor] = None,
                                    n_rays: Optional[int] = None, prefix_trans: Optional[Tensor] = None) -> Tensor:
    """-> trans: T_i = prod_{j<i} (1 - alpha_j)"""
    return _weights(alphas, None, None, packed_info, ray_indices, n_rays, prefix_trans, True, "render_transmittance_from_alpha",
                    with_weights=False)[1]


def render_weight_from_density(t_starts: Tensor, t_ends: Tensor, sigmas: Tensor, packed_info: Optional[Tensor] = None,
                               ray_indices: Optional[Tensor] = None, n_rays: Optional[int] = None,
                               prefix_trans: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (weights, trans, alphas): w_i = T_i alpha_i (morpheus.py:675)"""
    return _weights(sigmas, t_starts, t_ends, packed_info, ray_indices, n_rays, prefix_trans, False, "render_weight_from_density")


def render_weight_from_alpha(alphas: Tensor, packed_info: Optional[Tensor] = None, ray_indices: Optional[Tensor] = None,
                             n_rays: Optional[int] = None, prefix_trans: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """-> (weights, trans): w_i = alpha_i prod_{j<i} (1 - alpha_j)"""
    return _weights(alphas, None, None, packed_info, ray_indices, n_rays, prefix_trans, True, "render_weight_from_alpha")[:2]


# ------------------------------------------------------------------------------------------------------------ accumulate
class _Accumulate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, values, rs, rc, gaps, D):
        w = weights.detach().reshape(-1).contiguous()
        v = None if values is None else values.detach().reshape(-1, D).contiguous()
        N = rs.shape[0]
        out = torch.empty(N, D, device=w.device)
        _timed("mh_accumulate_fwd", ptr(w), ptr(v), D, ptr(rs), ptr(rc), N, ptr(out))
        ctx.D, ctx.gaps, ctx.w_shape, ctx.v_shape = D, gaps, weights.shape, None if values is None else values.shape
        ctx.save_for_backward(w, v, rs, rc)
        return out

    @staticmethod
    def backward(ctx, g):
        w, v, rs, rc = ctx.saved_tensors
        new = torch.zeros_like if ctx.gaps else torch.empty_like
        d_w = new(w) if ctx.needs_input_grad[0] else None
        d_v = new(v) if v is not None and ctx.needs_input_grad[1] else None
        if d_w is not None or d_v is not None:
            _timed("mh_accumulate_bwd", ptr(w), ptr(v), ctx.D, ptr(rs), ptr(rc), rs.shape[0], ptr(g.contiguous()), ptr(d_w), ptr(d_v))
        return (None if d_w is None else d_w.view(ctx.w_shape), None if d_v is None else d_v.view(ctx.v_shape), None, None, None,
                None)


def _accumulate(weights, values, lay: _Layout):
    if values is not None:
        _f32(values, "accumulate_along_rays")
        if values.dim() != weights.dim() + 1 or values.shape[:-1] != weights.shape:
            raise ValueError(f"accumulate_along_rays: values of shape {tuple(weights.shape)} + (D,) expected, got {tuple(values.shape)}")
    D = 1 if values is None else values.shape[-1]
    if not 1 <= D <= MAX_CHANNELS:
        raise ValueError(f"accumulate_along_rays: 1 to {MAX_CHANNELS} channels, got {D}")
    if lay.N == 0 or lay.M == 0:
        z = torch.zeros(lay.N, D, device=weights.device)
        return z + 0.0 * weights.sum() if weights.requires_grad else z      # zeros without a launch
    return _Accumulate.apply(weights, values, lay.rs, lay.rc, lay.gaps, D)


def accumulate_along_rays(weights: Tensor, values: Optional[Tensor] = None, ray_indices: Optional[Tensor] = None,
                          n_rays: Optional[int] = None) -> Tensor:
    """-> [n_rays, D]: sum_{i in ray} weights_i values[i, :]; values None: the sum of the weights, [n_rays, 1].
    Packed: weights [M], values [M, D], ray_indices [M] + n_rays.  Dense: weights [n_rays, n_samples], values
    [n_rays, n_samples, D], no indices.  1 <= D <= 256.  A ray without samples gives exactly 0."""
    require_gpu(weights, values, ray_indices)
    _f32(weights, "accumulate_along_rays")
    return _accumulate(weights, values, _Layout(weights, None, ray_indices, n_rays, "accumulate_along_rays"))


# ------------------------------------------------------------------------------------------------------------ visibility
def _visibility(values, t_starts, t_ends, packed_info, ray_indices, n_rays, early_stop_eps, alpha_thre, prefix_trans, alpha_form, what):
    if prefix_trans is not None:
        raise NotImplementedError(f"{what}: prefix_trans is not supported (ops.visibility_mask carries no prefix)")
    require_gpu(values, t_starts, t_ends)
    lay = _Layout(values, packed_info, ray_indices, n_rays, what)
    if lay.M == 0:
        return torch.zeros(lay.shape, dtype=torch.bool, device=values.device)
    flat = lambda t: None if t is None else t.detach().reshape(-1)
    ts, te = (flat(values), flat(values)) if alpha_form else (flat(t_starts), flat(t_ends))      # the alpha form reads neither
    keep, _ = ops.visibility_mask(flat(values), ts, te, lay.rs, lay.rc, float(early_stop_eps), float(alpha_thre), alpha_form,
                                  padded=lay.gaps)
    return keep.bool().view(lay.shape)


def render_visibility_from_density(t_starts: Tensor, t_ends: Tensor, sigmas: Tensor, packed_info: Optional[Tensor] = None,
                                   ray_indices: Optional[Tensor] = None, n_rays: Optional[int] = None, early_stop_eps: float = 1e-4,
                                   alpha_thre: float = 0.0, prefix_trans: Optional[Tensor] = None) -> Tensor:
    """-> bool mask: (T_i >= early_stop_eps) & (alpha_i >= alpha_thre); ops.visibility_mask's rules (negative densities count as 0)"""
    return _visibility(sigmas, t_starts, t_ends, packed_info, ray_indices, n_rays, early_stop_eps, alpha_thre, prefix_trans, False,
                       "render_visibility_from_density")


def render_visibility_from_alpha(alphas: Tensor, packed_info: Optional[Tensor] = None, ray_indices: Optional[Tensor] = None,
                                 n_rays: Optional[int] = None, early_stop_eps: float = 1e-4, alpha_thre: float = 0.0,
                                 prefix_trans: Optional[Tensor] = None) -> Tensor:
    """-> bool mask: (T_i >= early_stop_eps) & (alpha_i >= alpha_thre); ops.visibility_mask's rules (alphas clamped to [0, 1])"""
    return _visibility(alphas, None, None, packed_info, ray_indices, n_rays, early_stop_eps, alpha_thre, prefix_trans, True,
                       "render_visibility_from_alpha")


# ------------------------------------------------------------------------------------------------------------ rendering
def rendering(t_starts: Tensor, t_ends: Tensor, ray_indices: Optional[Tensor] = None, n_rays: Optional[int] = None,
              rgb_sigma_fn: Optional[Callable] = None, rgb_alpha_fn: Optional[Callable] = None,
              render_bkgd: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Dict]:
    """nerfacc's rendering(): query the field, composite -> (colors [n_rays, 3], opacities [n_rays, 1], depths [n_rays, 1], extras).
    Exactly one of rgb_sigma_fn / rgb_alpha_fn, called as fn(t_starts, t_ends, ray_indices) -> (rgbs, sigmas or alphas).
    depths = sum w (t_starts + t_ends) / 2 divided by the opacity (clamped from below at float32's eps); render_bkgd is blended
    as colors + render_bkgd (1 - opacities).  extras: weights, trans, rgbs and alphas, and sigmas in the density form."""
    if (rgb_sigma_fn is None) == (rgb_alpha_fn is None):
        raise ValueError("rendering: exactly one of rgb_sigma_fn and rgb_alpha_fn")
    if ray_indices is not None and n_rays is None:
        raise ValueError("rendering: ray_indices without n_rays")
    idx = None if ray_indices is None else ray_indices.long()
    if rgb_sigma_fn is not None:
        rgbs, sigmas = rgb_sigma_fn(t_starts, t_ends, idx)
        if t_starts.shape[0] != 0 and sigmas.shape != t_starts.shape:
            raise ValueError(f"rendering: sigmas of shape {tuple(t_starts.shape)} expected, got {tuple(sigmas.shape)}")
        weights, trans, alphas = render_weight_from_density(t_starts, t_ends, sigmas, ray_indices=ray_indices, n_rays=n_rays)
        extras = {"weights": weights, "alphas": alphas, "trans": trans, "sigmas": sigmas, "rgbs": rgbs}
    else:
        rgbs, alphas = rgb_alpha_fn(t_starts, t_ends, idx)
        if t_starts.shape[0] != 0 and alphas.shape != t_starts.shape:
            raise ValueError(f"rendering: alphas of shape {tuple(t_starts.shape)} expected, got {tuple(alphas.shape)}")
        weights, trans = render_weight_from_alpha(alphas, ray_indices=ray_indices, n_rays=n_rays)
        extras = {"weights": weights, "trans": trans, "alphas": alphas, "rgbs": rgbs}
    colors = accumulate_along_rays(weights, rgbs, ray_indices, n_rays)
    opacities = accumulate_along_rays(weights, None, ray_indices, n_rays)
    depths = accumulate_along_rays(weights, (t_starts + t_ends)[..., None] / 2.0, ray_indices, n_rays)
    depths = depths / opacities.clamp_min(torch.finfo(rgbs.dtype).eps)
    if render_bkgd is not None:
        colors = colors + render_bkgd * (1.0 - opacities)
    return colors, opacities, depths, extras
