"""Importance resampling: NeRF's `sample_pdf` as the reference ships it (utils.py:10-44) and the form a renderer uses on packed
ragged samples -- the coarse intervals cut at n inverse-CDF draws per ray (csrc/resample.hip states every operation).

Everything here runs under no_grad: the reference samples under no_grad (morpheus.py:627) and there is no backward kernel;
gradients reach the field through a later query AT the refined samples, not through their positions.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops, volrend
from .occgrid import PackedSamples


@torch.no_grad()
def sample_pdf(bins, weights, n_samples: int, det: bool = False, u: Optional[torch.Tensor] = None):
    """utils.sample_pdf: bins [..., T] (old z values), weights [..., T - 1] (bin weights) -> [..., n_samples] new z values.
    `u` [..., n_samples] injects the draws; otherwise they are torch.rand's, or for `det` the reference's linspace grid
    (built on the host and copied, as the reference builds it, so that the grid has the reference's bits)."""
    n = int(n_samples)
    lead = tuple(bins.shape[:-1])
    T = bins.shape[-1]
    if tuple(weights.shape) != lead + (T - 1,):
        raise ValueError(f"sample_pdf: bins [..., T] and weights [..., T - 1] expected, got {tuple(bins.shape)}, {tuple(weights.shape)}")
    if u is None:
        if det:
            u = torch.linspace(0. + 0.5 / n, 1. - 0.5 / n, steps=n).to(weights.device).expand(lead + (n,))
        else:
            u = torch.rand(lead + (n,), device=weights.device)
    elif tuple(u.shape) != lead + (n,):
        raise ValueError(f"sample_pdf: u {list(lead + (n,))} expected, got {tuple(u.shape)}")
    out = ops.sample_pdf(bins.reshape(-1, T), weights.reshape(-1, T - 1), u.reshape(-1, n))
    return out.view(lead + (n,))


def _ray_indices(ray_start, ray_cnt, M: int, n_valid):
    """ray index of every packed position from (ray_start, ray_cnt), padding (positions no ray owns) as ray 0; no host read"""
    ends = torch.cumsum(ray_cnt, 0, dtype=torch.int32)
    pos = torch.arange(M, device=ray_cnt.device, dtype=torch.int32)
    ri = torch.searchsorted(ends, pos, right=True).clamp_(max=max(ray_cnt.shape[0] - 1, 0)).to(torch.int32)
    return ri if n_valid is None else torch.where(pos < n_valid, ri, torch.zeros_like(ri))


@torch.no_grad()
def importance_sampling(ray_start, ray_cnt, t_starts, t_ends, n_importance: int, weights=None, sigmas=None, det: bool = False,
                        jitter=None, eps: float = 1e-5, n_valid=None, with_xyz: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """`refine_samples` on loose arrays: the packed samples (ray_start, ray_cnt int32 [N]; t_starts, t_ends [M]; n_valid as the
    record's) -> (ray_indices, t_starts, t_ends, ray_start, ray_cnt[, xyz][, n_valid]): xyz with with_xyz, the new n_valid last
    when one was given."""
    rec = refine_samples(PackedSamples(None, t_starts, t_ends, ray_start, ray_cnt, n_valid), n_importance, weights, sigmas, det,
                         jitter, eps, with_xyz)
    return rec[:5] + ((rec.xyz,) if with_xyz is not None else ()) + ((rec.n_valid,) if n_valid is not None else ())


@torch.no_grad()
def refine_samples(rec: PackedSamples, n_importance: int, weights=None, sigmas=None, det: bool = False, jitter=None,
                   eps: float = 1e-5, with_xyz: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> PackedSamples:
    """The record's samples (its ray_indices are not read: the ranges say the same) cut at n_importance draws per ray from the
    piecewise-constant pdf (w_i + eps) / sum over each ray's own intervals -> the record of the refined samples.
    weights [M], or sigmas [M] (densities: they go through the compositor's weights kernel, volrend.render_weight_from_density,
    first) -- one of the two.  det: the draws sit at (k + 0.5) / n, the reference's det=True grid; else at (k + jitter[r, k]) / n,
    jitter fp32 [N, n] in [0, 1) (None: torch.rand).  rec.n_valid (int32 0-dim, device): the inputs have a fixed capacity and only
    their first n_valid entries are samples (occgrid.PackedSampling.sample_capacity); the outputs then have length M + n N, the
    result carries the new n_valid and nothing is read by the host.  with_xyz = (rays_o, rays_d): also the midpoints' positions.
    A ray without samples keeps none; n_importance = 0 returns the input's samples."""
    if (weights is None) == (sigmas is None):
        raise ValueError("importance_sampling: give weights or sigmas, one of the two")
    if det and jitter is not None:
        raise ValueError("importance_sampling: det=True places the draws at (k + 0.5) / n; a jitter cannot be given with it")
    n = int(n_importance)
    if n < 0:
        raise ValueError(f"importance_sampling: n_importance = {n}")
    ray_start, ray_cnt, t_starts, t_ends, n_valid = rec.ray_start, rec.ray_cnt, rec.t_starts, rec.t_ends, rec.n_valid
    ops.require_gpu(ray_start, ray_cnt, t_starts, t_ends, weights, sigmas, jitter, n_valid)
    N, M = ray_start.shape[0], t_starts.shape[0]
    if n == 0:
        ri = _ray_indices(ray_start, ray_cnt, M, n_valid)
        xyz = None
        if with_xyz is not None:
            xyz = ops.sample_positions_nograd(with_xyz[0].detach(), with_xyz[1].detach(), ri, t_starts, t_ends)
        return PackedSamples(ri, t_starts, t_ends, ray_start, ray_cnt, n_valid, None, xyz)
    if weights is None:
        weights = volrend.render_weight_from_density(t_starts, t_ends, sigmas.detach().reshape(-1).float(),
                                                     packed_info=torch.stack((ray_start, ray_cnt), dim=1))[0]
    if not det and jitter is None:
        jitter = torch.rand(N, n, device=t_starts.device)
    o, d = with_xyz if with_xyz is not None else (None, None)
    out = ops.resample_packed(weights, t_starts, t_ends, ray_start, ray_cnt, n, None if det else jitter, eps,
                              padded=n_valid is not None, rays_o=o, rays_d=d)
    return PackedSamples(*out[:5], n_valid=out[6] if n_valid is not None else None, xyz=out[5])
