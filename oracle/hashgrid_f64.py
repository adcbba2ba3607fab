"""ORACLE -- TEST INFRASTRUCTURE ONLY (never imported by morpheus_amd/).

The multires hash grid of external/encoders/gridencoder/src/gridencoder.cu evaluated in FLOAT64 (vectorised torch, with a
backward): the yardstick of the counted parity gate and of the double runs of the training steps.  oracle/make_golden.py runs the imported reference model in double with this
encoder standing where the CUDA-only one stands, so that the fixture holds, next to the reference's own fp32 result, the value
both fp32 implementations (the reference's and the HIP path's) are rounding towards -- the gate's allowance is then derived from
how far the REFERENCE's fp32 result is from it, not fitted to the HIP path's.

Same reading of the .cu as oracle/hashgrid.c (index / hash / clamp / weights: gridencoder.cu:45-79, :132-184), restated a
third time here only in that the arithmetic type is double; integer index maths is exact in either.  Level resolutions stay
the kernel's float32 table (gridencoder.cu:133) -- they are integers.

Backward (_GridEncodeF64): the table gradient is autograd's scatter through the value computation (grad_emb[row] += w * grad);
the input gradient is the KERNEL's rule (gridencoder.cu:206-246), not autograd's: per axis, the sum over the 4 corner pairs of
w * (right - left) * res, with the border clamp of the position ignored (autograd through the clamp would give zero slope in the
half-texel band at every face of the box, where the kernel, oracle/hashgrid.c and oracle/hashgrid_np.py all keep the slope of the
border cell), and zero for points with any u outside [0, 1].  A double yardstick with autograd's slope would differ from every fp32
implementation by a convention, not by round-off.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .hashgrid import effective_levels, level_resolutions

_P1, _P2 = 2654435761, 805459861
_M32 = (1 << 32) - 1


def _level_geometry(u, res):
    """cell [M,3] (long) and fractional position f [M,3] of one level (gridencoder.cu:148-152, align_corners = False)."""
    pos = (u * res - 0.5).clamp(0, res - 1)                          # :148
    g = torch.floor(pos)
    return g.long(), pos - g


def _rows(c, res, T, hashed):
    """Row within the level table of integer corner coordinates c = [cx, cy, cz] (gridencoder.cu:61-79)."""
    if hashed:
        idx = ((c[0] * 1) & _M32) ^ ((c[1] * _P1) & _M32) ^ ((c[2] * _P2) & _M32)
    else:
        idx = c[0] + c[1] * res + c[2] * res * res
    return idx % T


def _encode(u, emb, offsets, res_tab, n_levels):
    """u [M,3] float64 -> [M, L*C] float64 (levels >= n_levels and out-of-range points zero)."""
    M, C = u.shape[0], emb.shape[1]
    L = len(offsets) - 1
    inside = ((u >= 0) & (u <= 1)).all(-1, keepdim=True)             # gridencoder.cu:105-130
    out = torch.zeros(M, L * C, dtype=torch.float64)
    for l in range(n_levels):
        res = int(res_tab[l])
        T = int(offsets[l + 1]) - int(offsets[l])
        g, f = _level_geometry(u, res)
        acc = torch.zeros(M, C, dtype=torch.float64)
        hashed = res ** 3 > T                                        # :61-79: the running stride outgrew the table
        for corner in range(8):
            w = torch.ones(M, dtype=torch.float64)
            c = []
            for d in range(3):
                if (corner >> d) & 1:
                    w = w * f[:, d]
                    c.append(torch.clamp(g[:, d] + 1, max=res - 1))  # :182
                else:
                    w = w * (1 - f[:, d])
                    c.append(g[:, d])
            row = int(offsets[l]) + _rows(c, res, T, hashed)
            acc = acc + w[:, None] * emb[row]
        out[:, l * C:(l + 1) * C] = acc
    return torch.where(inside, out, torch.zeros_like(out))


def grid_dy_du_f64(u, emb, offsets, res_tab, n_levels):
    """[M, L, 3, C] float64 derivative of the features w.r.t. u by the kernel's rule (gridencoder.cu:206-246): per axis gd, the
    sum over the 4 corner pairs of the other two axes of w * (right - left) * res, the clamp of the position ignored; zero for
    points with any u outside [0, 1] and for levels >= n_levels."""
    M, C = u.shape[0], emb.shape[1]
    L = len(offsets) - 1
    out = torch.zeros(M, L, 3, C, dtype=torch.float64)
    inside = ((u >= 0) & (u <= 1)).all(-1)[:, None]
    for l in range(n_levels):
        res = int(res_tab[l])
        T = int(offsets[l + 1]) - int(offsets[l])
        hashed = res ** 3 > T
        g, f = _level_geometry(u, res)
        hi = torch.clamp(g + 1, max=res - 1)
        for gd in range(3):
            others = [d for d in range(3) if d != gd]
            acc = torch.zeros(M, C, dtype=torch.float64)
            for k in range(4):
                w = torch.full((M,), float(res), dtype=torch.float64)
                c = [None, None, None]
                for nd, d in enumerate(others):
                    up = (k >> nd) & 1
                    w = w * (f[:, d] if up else 1 - f[:, d])
                    c[d] = hi[:, d] if up else g[:, d]
                c[gd] = g[:, gd]
                left = emb[int(offsets[l]) + _rows(c, res, T, hashed)]
                c[gd] = hi[:, gd]
                right = emb[int(offsets[l]) + _rows(c, res, T, hashed)]
                acc = acc + w[:, None] * (right - left)
            out[:, l, gd] = torch.where(inside, acc, torch.zeros_like(acc))
    return out


def _corner_terms(x, offsets, res_tab, bound, n_levels):
    """Yields (level, rows [m] int64 numpy, w [m] float64 numpy, keep [m] int64 numpy: index of the point) for the 8 corners of every
    level < n_levels, corner 7 first, over the points inside the box only -- the terms of the scatter grad_emb[row] += w * grad."""
    u = (x.detach().double() + bound) / (2 * bound)
    keep = torch.nonzero(((u >= 0) & (u <= 1)).all(-1))[:, 0]
    u = u[keep]
    keep = keep.numpy()
    for l in range(n_levels):
        res = int(res_tab[l])
        T = int(offsets[l + 1]) - int(offsets[l])
        hashed = res ** 3 > T
        g, f = _level_geometry(u, res)
        for corner in range(7, -1, -1):
            w = torch.ones(u.shape[0], dtype=torch.float64)
            c = []
            for d in range(3):
                if (corner >> d) & 1:
                    w = w * f[:, d]
                    c.append(torch.clamp(g[:, d] + 1, max=res - 1))
                else:
                    w = w * (1 - f[:, d])
                    c.append(g[:, d])
            yield l, (int(offsets[l]) + _rows(c, res, T, hashed)).numpy(), w.numpy(), keep


def grid_table_grad_f64(x, grad, offsets, res_tab, bound, n_levels):
    """x [M,3] (world units, any float type), grad [M, L*C] -> float64 [rows, C]: the table gradient of grid_encode_f64 without its
    value graph, one pass of the scatter grad_emb[row] += w * grad.  The same bits as the autograd route (_GridEncodeF64): a
    corner's terms are summed in point order from zero, as index_put_(accumulate) does, and the eight corner sums of a level are
    added in the order autograd's engine runs their nodes (last built first); points outside the box add nothing there either."""
    L = len(offsets) - 1
    C = grad.shape[1] // L
    gd = grad.detach().double().numpy().reshape(grad.shape[0], L, C)
    out = np.zeros((int(offsets[-1]), C), dtype=np.float64)
    first = [True] * L
    for l, rows, w, keep in _corner_terms(x, offsets, res_tab, bound, n_levels):
        lo, hi = int(offsets[l]), int(offsets[l + 1])
        for ch in range(C):
            s = np.bincount(rows - lo, weights=w * gd[keep, l, ch], minlength=hi - lo)
            out[lo:hi, ch] = s if first[l] else out[lo:hi, ch] + s
        first[l] = False
    return torch.from_numpy(out)


def grid_term_counts(x, offsets, res_tab, bound, n_levels):
    """int64 [rows]: how many (point, corner) terms of the scatter land on each table row -- hash collisions and corners merged by
    the border clamp counted once each, zero-weight corners included; points outside the box and levels >= n_levels count nothing."""
    out = np.zeros(int(offsets[-1]), dtype=np.int64)
    for l, rows, _, _ in _corner_terms(x, offsets, res_tab, bound, n_levels):
        out += np.bincount(rows, minlength=out.shape[0])
    return torch.from_numpy(out)


class _GridEncodeF64(torch.autograd.Function):
    """Values of _encode; table gradient = autograd's scatter through _encode; input gradient = the kernel's rule."""

    @staticmethod
    def forward(ctx, u, emb, offsets, res_tab, n_levels):
        ctx.save_for_backward(u, emb)
        ctx.geom = (offsets, res_tab, n_levels)
        return _encode(u, emb, offsets, res_tab, n_levels)

    @staticmethod
    def backward(ctx, grad):
        u, emb = ctx.saved_tensors
        offsets, res_tab, n_levels = ctx.geom
        g_u = g_emb = None
        if ctx.needs_input_grad[0]:
            L, C = len(offsets) - 1, emb.shape[1]
            dy = grid_dy_du_f64(u.detach(), emb.detach(), offsets, res_tab, n_levels)
            g_u = torch.einsum("mldc,mlc->md", dy, grad.reshape(-1, L, C))
        if ctx.needs_input_grad[1]:
            with torch.enable_grad():
                e = emb.detach().requires_grad_(True)
                g_emb, = torch.autograd.grad(_encode(u.detach(), e, offsets, res_tab, n_levels), e, grad)
        return g_u, g_emb, None, None, None


def grid_encode_f64(x: torch.Tensor, emb: torch.Tensor, offsets, res_tab, bound: float, max_level=None) -> torch.Tensor:
    """x [M,3] float64 in world units -> [M, L*C] float64 (levels >= the effective count are zero, grid.py:42,53)."""
    assert x.dtype == torch.float64 and emb.dtype == torch.float64
    n_levels = effective_levels(max_level, len(offsets) - 1)
    u = (x + bound) / (2 * bound)                                    # grid.py:157 (autograd supplies the 1 / (2 bound))
    if not (torch.is_grad_enabled() and (u.requires_grad or emb.requires_grad)):
        return _encode(u, emb, offsets, res_tab, n_levels)
    return _GridEncodeF64.apply(u, emb, list(offsets), res_tab, n_levels)


class OracleGridEncoderF64(nn.Module):
    """Constructor / forward surface of the reference GridEncoder (grid.py:103-169), float64."""

    def __init__(self, input_dim=3, num_levels=16, level_dim=2, per_level_scale=2, base_resolution=16, log2_hashmap_size=19,
                 desired_resolution=None, gridtype="hash", align_corners=False, interpolation="linear"):
        super().__init__()
        assert input_dim == 3 and gridtype == "hash" and not align_corners and interpolation == "linear"
        if desired_resolution is not None:
            per_level_scale = np.exp2(np.log2(desired_resolution / base_resolution) / (num_levels - 1))
        self.input_dim, self.num_levels, self.level_dim = input_dim, num_levels, level_dim
        self.output_dim = num_levels * level_dim
        offs, total = [], 0
        for i in range(num_levels):
            res = int(np.ceil(base_resolution * per_level_scale ** i))
            n = int(np.ceil(min(2 ** log2_hashmap_size, res ** input_dim) / 8) * 8)
            offs.append(total)
            total += n
        offs.append(total)
        self.register_buffer("offsets", torch.from_numpy(np.asarray(offs, dtype=np.int32)))
        self._res = level_resolutions(num_levels, per_level_scale, base_resolution)
        self.embeddings = nn.Parameter(torch.zeros(total, level_dim, dtype=torch.float64))
        # round 5: the double run of a TRAINING step (oracle/make_golden.py:gen_round5, virt24) lets autograd through the table;
        # the forward-only yardsticks keep the detached form (identical values)
        self.differentiable = False

    def forward(self, inputs, bound=1, max_level=None):
        lead = list(inputs.shape[:-1])
        emb = self.embeddings if self.differentiable else self.embeddings.detach()
        out = grid_encode_f64(inputs.reshape(-1, 3).double(), emb.double(), self.offsets.tolist(), self._res, float(bound), max_level)
        return out.view(lead + [self.output_dim])
