"""torch.autograd wrappers over the C ABI (include/morpheus_hip.h).

Each Function allocates its outputs/workspaces as torch tensors (the reference's ownership model,
external/encoders/gridencoder/grid.py:50,56,84,87), hands raw device pointers plus torch's CURRENT
stream to libmorpheus_hip.so and returns.  There is no CPU or PyTorch fallback: a CPU tensor or a
missing library raises MorpheusHipError.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check, launch, ptr, require_gpu, stream
from .packing import field_joint_packer, field_packer, warp_joint_packer, warp_packer



class KernelTimer:
    """Optional per-C-ABI-call timing with events recorded on the launch stream (torch's current
    stream, which is the one handed to the library).  Used by bench.py for the roofline numbers.
    Events come from a pool that is recycled at reset(): creating two fresh events per call costs the host 20-50 us,
    which a short step (cfg2: 5 ms of GPU work, ~12 timed calls) would feel."""

    def __init__(self):
        self.enabled = False
        self.records = {}
        self._pool, self._used = [], 0

    def reset(self, enabled: bool):
        self.enabled, self.records, self._used = enabled, {}, 0

    def _event(self):
        if self._used == len(self._pool):
            self._pool.append(torch.cuda.Event(enable_timing=True))
        e = self._pool[self._used]
        self._used += 1
        return e

    @staticmethod
    def _stream():
        """the current stream as a torch Stream object, one object per raw handle (Event.record() without a stream argument
        resolves torch.cuda.current_stream() through three Python layers: 5.4 us against 1.5 -- twice per timed call)"""
        raw = stream()
        s = _STREAM_OBJECTS.get(raw)
        if s is None:
            s = _STREAM_OBJECTS[raw] = torch.cuda.current_stream()
        return s

    def start(self):
        if not self.enabled:
            return None
        e = self._event()
        e.record(self._stream())
        return e

    def stop(self, name: str, e0):
        if e0 is None:
            return
        e1 = self._event()
        e1.record(self._stream())
        self.records.setdefault(name, []).append((e0, e1))

    def summary(self):
        """name -> (calls, total_ms); call after torch.cuda.synchronize()."""
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v)) for k, v in self.records.items()}


_STREAM_OBJECTS: dict = {}
TIMER = KernelTimer()


def _timed(name: str, *args, key: Optional[str] = None):
    """launch(name, *args), timed under `key` (default: the entry point's own name) while TIMER is enabled"""
    if not TIMER.enabled:
        return launch(name, *args)
    e = TIMER.start()
    launch(name, *args)
    TIMER.stop(key or name, e)


_I32_CACHE = {}


def _i32arr(a):
    """host int32 array + its ctypes pointer for the C ABI's *_host arguments.  The arrays the hot path passes are static
    geometry (level tables, tile offsets, layer lists): lists / tuples and read-only numpy arrays are converted once and cached
    by value -- a training step makes ~150 of these calls."""
    # one key form for every source kind: (length, values...) of Python ints -- a list [3, 1, 2, 3] and the array [1, 2, 3] must
    # not meet in one entry
    if type(a) is tuple or type(a) is list:
        # fast path: the tuple of the values themselves (hash-equal to the canonical key's tail for Python and numpy ints alike);
        # the element types are checked once, when the entry is made
        k2 = ("seq", tuple(a))
        hit = _I32_CACHE.get(k2)
        if hit is not None:
            return hit
        if all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in a):
            key = (len(a),) + tuple(int(v) for v in a)
            hit = _I32_CACHE.get(key)
            if hit is None:
                arr = np.ascontiguousarray(a, dtype=np.int32)
                arr.setflags(write=False)
                hit = _I32_CACHE[key] = (arr, arr.ctypes.data_as(ctypes.c_void_p))
            _I32_CACHE[k2] = hit
            return hit
        key = None
    elif isinstance(a, np.ndarray) and a.dtype == np.int32 and a.ndim == 1 and a.size <= 64:
        key = (a.size,) + tuple(a.tolist())
    else:
        key = None
    if key is not None:
        hit = _I32_CACHE.get(key)
        if hit is None:
            arr = np.ascontiguousarray(a, dtype=np.int32)
            arr.setflags(write=False)
            hit = _I32_CACHE[key] = (arr, arr.ctypes.data_as(ctypes.c_void_p))
        return hit
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------------------------ hash grid
def _scratch(n: int, device, dtype=torch.float32) -> torch.Tensor:
    """An uninitialised 1-D scratch buffer of n elements for the kernels' parked tiles / per-point rows, allocated in SIZE CLASSES
    (eight per octave: n rounded up by at most 12.5 %).  The packed sample count of a training step changes from step to step, and
    so did the byte counts of its ~40 large allocations: the caching allocator can split a cached block but cannot grow one, so
    every step whose batch was a little larger than any before it opened new segments beside the cached ones -- the 180 x 180
    virtual-view step allocates 104 GB at its peak and had 245 GB RESERVED (profiles/r06_park_alloc.txt).  With size classes a
    step's requests find the previous step's blocks."""
    n = int(n)
    if n >= (1 << 18):
        q = 1 << (n.bit_length() - 4)
        return torch.empty((n + q - 1) // q * q, dtype=dtype, device=device)[:n]
    return torch.empty(n, dtype=dtype, device=device)


def level_resolutions(L: int, per_level_scale: float, base: int) -> np.ndarray:
    """res_l = (uint32)ceil(exp2f(l*S)*H) in float32, S = (float)log2(per_level_scale)
    (gridencoder.cu:133, grid.py:39).  Host-computed so no device libm is involved."""
    S = np.float32(np.log2(per_level_scale))
    l = np.arange(L, dtype=np.float32)
    return np.ceil(np.exp2(l * S).astype(np.float32) * np.float32(base)).astype(np.int32)


def effective_levels(max_level, L: int) -> int:
    """grid.py:42."""
    return L if max_level is None else max(min(int(math.ceil(max_level * L)), L), 1)


def _bin_points(lib, x, bound):
    """Counting-sort the points into 16^3 bricks (shared by every table evaluated at x)."""
    M, dev = x.shape[0], x.device
    ws = torch.empty(lib.mh_grid_bin_workspace_ints(), dtype=torch.int32, device=dev)
    perm = _scratch(M, dev, torch.int32)
    bstart = torch.empty(lib.mh_grid_bin_index_ints(), dtype=torch.int32, device=dev)
    _timed("mh_grid_bin_points", ptr(x), M, bound, ptr(ws), ptr(perm), ptr(bstart))
    return perm, bstart


# ---- arithmetic mode of the MLP kernels (MORPHEUS_MLP, or set_mlp_mode() at run time) -------------------------------------
# Values, parked tiles, accumulation and results are fp32 in every mode; what differs is how a product reaches the matrix cores.
#   "b3"  (default) bf16 x 3: every fp32 operand is cut EXACTLY into three bf16 slices (all 24 significand bits), the six
#         significant cross products go through v_mfma_f32_32x32x16_bf16 with fp32 accumulation (csrc/mlp_b3.hip): warp nets
#         forward / backward-data / weight gradients and the field forward.  fp32-faithful: what is dropped is below 2^-24 of a
#         product, less than the rounding of an fp32 multiply-add.
#   "f32" the native fp32 MFMA (v_mfma_f32_32x32x2_f32) everywhere (csrc/mlp.hip): the reference's arithmetic instruction for
#         instruction, and the slowest (the fp32 MFMA runs at the vector-ALU rate on gfx950).
# (A third form, two fp16 slices at power-of-two scales -- 22-bit operands, NOT fp32-faithful -- existed in rounds 3-5 and was
# deleted in round 6: git history, csrc/mlp_h2.hip.)
# The field nets' fused backward (mh_field_bwd_fused) follows the b3 mode too; the f32 mode runs it on the native fp32 MFMA; see
# FIELD_BWD below.
MLP_MODES = ("b3", "f32")
MODE_DTYPE = {"f32": "f32", "b3": "f32 (exact 3 x bf16 operand split, 6 slice products per MAC on the bf16 MFMA pipe, fp32 accumulate)"}
_mode = os.environ.get("MORPHEUS_MLP", "b3")
if _mode not in MLP_MODES:
    raise ValueError(f"MORPHEUS_MLP={_mode!r}: expected one of {MLP_MODES}")


def mlp_mode() -> str:
    return _mode


def set_mlp_mode(mode: str) -> str:
    """Select the PROCESS DEFAULT arithmetic of the MLP kernels, for operand packs prepared from now on by models that do not
    carry a mode of their own (`scene_representation.mlp_mode`).  A pack keeps the arithmetic it was prepared with (see
    _warp_mode): changing the default between a forward and its backward, or inside a model.operand_scope(), does not mix
    arithmetic forms.  -> the previous default."""
    global _mode
    if mode not in MLP_MODES:
        raise ValueError(f"mlp mode {mode!r}: expected one of {MLP_MODES}")
    prev, _mode = _mode, mode
    return prev


def _warp_mode(mode: Optional[str] = None) -> str:
    """operand-pack tag of the MLP nets: "b3" / "" (native fp32 MFMA).  `mode`: an explicit choice (a model's own
    `mlp_mode`); None = the process default (MORPHEUS_MLP / set_mlp_mode).  The tag is fixed when a pack is prepared and travels
    with it (MLPOperands.mode -> every forward's ctx): a forward and its backward always use the same arithmetic, and two models
    of one process may differ."""
    mode = _mode if mode is None else mode
    if mode not in MLP_MODES:
        raise ValueError(f"mlp mode {mode!r}: expected one of {MLP_MODES}")
    return "" if mode == "f32" else mode


def _grid_fwd(lib, x, embs, o_p, r_p, L, n_levels, bound, group):
    """One forward launch per table at the same points -> (list of [M, L*2], binning or None).
    Calls of at least mh_grid_stage_min_points() points (2^20 unless tuned) are binned into bricks FIRST and run the
    brick-staged forward (rows read from LDS instead of eight gathers per point and level; same bits); the binning is handed
    back for the caller's backward, which would otherwise make it itself.  That includes the large finite-difference-tap calls
    of a whole-view step (group = 6; same-box A/B against the gather-sharing grouped kernel: 72 x 72 view 0.66 -> 0.49 ms of
    forward per step, 180 x 180 3.7 -> 2.2 ms); smaller calls keep the grouped kernel."""
    M = x.shape[0]
    outs = []
    binned = None
    if L == 16 and M >= lib.mh_grid_stage_min_points(-1):     # (whatever `group`: a staged brick shares a cell's rows among all its points)
        binned = _bin_points(lib, x, bound)
    for emb in embs:
        out = _scratch(M * L * 2, x.device).view(M, L * 2)
        if binned is not None:
            _timed("mh_grid_encode_fwd_binned", ptr(x), ptr(emb), o_p, r_p, ptr(binned[0]), ptr(binned[1]), ptr(out), M, L,
                   n_levels, float(bound))
        else:
            _timed("mh_grid_encode_fwd", ptr(x), ptr(emb), o_p, r_p, ptr(out), M, L, n_levels, float(bound), int(group))
        outs.append(out)
    return outs, binned


def _grid_bwd(lib, x, embs, grads, o_p, r_p, L, n_levels, bound, need_dx, gmax_ptrs=None, sums=None, g_x_into=None, binned=None):
    """Embedding (and position) gradients of several tables evaluated at the same points: ONE brick binning shared by all
    tables.  gmax_ptrs[k]: device address of max|grads[k]| as float bits when its producer reduced it on the fly
    (mh_field_bwd_data), else None -> the kernel reduces it itself.
    sums[k]: device ADDRESS of a running table-gradient sum this call adds into (the brick kernel's last pass adds to the
    table), or None -> a fresh zero-filled table.  g_x_into: a [M,3] gradient of the same points that the tables' d/dx is added
    to in the kernel (brick path only), or None.
    -> (g_x or None, [g_emb; None where the gradient went into sums[k]])."""
    M = x.shape[0]
    g_x_total, g_embs = g_x_into, []          # binned: the forward's binning of the same points, when it made one
    brick = M > 0 and L == 16          # the brick kernel's level table is sized for the shipped 16-level geometry
    for k, (emb, grad) in enumerate(zip(embs, grads)):
        if grad is None:
            g_embs.append(None)
            continue
        grad = grad.contiguous()
        into = None if sums is None else sums[k]
        g_emb = torch.zeros_like(emb) if into is None else None
        g_emb_p = ptr(g_emb) if into is None else ctypes.c_void_p(into)
        if brick:
            if binned is None:
                binned = _bin_points(lib, x, bound)
            acc_dx = need_dx and g_x_total is not None
            g_x = g_x_total if acc_dx else (torch.empty_like(x) if need_dx else None)
            emb_acc = torch.empty(emb.numel(), dtype=torch.int64, device=emb.device)     # the kernel's fixed-point table sum
            _timed("mh_grid_encode_bwd_binned", ptr(grad), ptr(x), ptr(emb), o_p, r_p, ptr(binned[0]), ptr(binned[1]), g_emb_p,
                   ptr(emb_acc), ptr(g_x), int(acc_dx), M, L, n_levels, bound, None if gmax_ptrs is None else gmax_ptrs[k])
            g_x_total = g_x
        else:
            g_x = torch.empty_like(x) if need_dx else None
            _timed("mh_grid_encode_bwd", ptr(grad), ptr(x), ptr(emb), o_p, r_p, g_emb_p, ptr(g_x), M, L, n_levels, bound)
            if need_dx:
                g_x_total = g_x if g_x_total is None else g_x_total + g_x
        g_embs.append(g_emb)
    return (g_x_total if need_dx else None), g_embs


class _GridEncode(torch.autograd.Function):
    """grid.py:25-96 (_grid_encode) on the HIP kernels, for one or several tables evaluated at the
    same points (sdf + colour encoders share x: one index computation pattern, one binning).
    No dy_dx tensor is materialised; backward recomputes corner weights."""

    @staticmethod
    def forward(ctx, x, offsets_np, res_np, n_levels, bound, group, *embs):
        ctx.set_materialize_grads(False)      # unused outputs hand backward None, not a zero-filled tensor (one launch each)
        require_gpu(x, *embs)
        lib = _lib.load()
        x = x.detach().contiguous().float()
        L = len(res_np)
        o_np, o_p = _i32arr(offsets_np)
        r_np, r_p = _i32arr(res_np)
        saved = [emb.detach().contiguous() for emb in embs]
        outs, ctx.binned = _grid_fwd(lib, x, saved, o_p, r_p, L, n_levels, bound, group)
        ctx.save_for_backward(x, *saved)
        ctx.meta = (o_np, r_np, n_levels, float(bound), L)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        lib = _lib.load()
        x, *embs = ctx.saved_tensors
        o_np, r_np, n_levels, bound, L = ctx.meta
        o_p, r_p = o_np.ctypes.data_as(ctypes.c_void_p), r_np.ctypes.data_as(ctypes.c_void_p)
        g_x, g_embs = _grid_bwd(lib, x, embs, grads, o_p, r_p, L, n_levels, bound, ctx.needs_input_grad[0], binned=ctx.binned)
        return (g_x, None, None, None, None, None, *g_embs)


def grid_encode(x, emb, offsets_np, res_np, bound, max_level=None, group: int = 1):
    """x [..,3] in world units -> [.., L*2] (grid.py:152-169).  group: every `group` consecutive points are neighbours
    (6 = finite-difference taps, point-major): a gather-sharing hint, results do not depend on it."""
    L = len(res_np)
    lead = list(x.shape[:-1])
    (out,) = _GridEncode.apply(x.reshape(-1, 3), offsets_np, res_np, effective_levels(max_level, L), bound, group, emb)
    return out.view(lead + [L * 2])


def grid_encode_multi(x, embs, offsets_np, res_np, bound, max_level=None):
    """Several tables with identical level geometry at the same points -> tuple of [M, L*2]."""
    L = len(res_np)
    return _GridEncode.apply(x.reshape(-1, 3), offsets_np, res_np, effective_levels(max_level, L), bound, 1, *embs)


# ---- the grid encoder in full (csrc/hashgrid_general.hip): every channel count, grid type, alignment and interpolation ----------
GRID_TYPES = {"hash": 0, "tiled": 1}          # grid.py:13-16
GRID_INTERPS = {"linear": 0, "smoothstep": 1}  # grid.py:18-21
GRID_CHANNELS = (1, 2, 4, 8)


def _grid_switch(table: dict, value, what: str) -> int:
    if value in table:
        return table[value]
    if isinstance(value, (int, np.integer)) and not isinstance(value, bool) and int(value) in table.values():
        return int(value)
    raise ValueError(f"{what} {value!r}: expected one of {tuple(table)}")


def _grid_table(emb, offsets_np, C: int):
    """the checks every general-grid call makes on its table: [rows, C] fp32 on the GPU with the rows the offsets describe"""
    require_gpu(emb)
    if C not in GRID_CHANNELS:
        raise ValueError(f"level_dim {C}: the HIP grid encoder has C in {GRID_CHANNELS}")
    if emb.dtype != torch.float32 or emb.dim() != 2 or emb.shape[1] != C or emb.shape[0] != int(offsets_np[-1]):
        raise ValueError(f"embeddings {tuple(emb.shape)} {emb.dtype}: expected fp32 [{int(offsets_np[-1])}, {C}]")


class _GridEncodeGeneral(torch.autograd.Function):
    """grid.py:25-96 on mh_grid_general_fwd / _bwd.  Saves x and emb; cells and weights are recomputed in the backward (no dy_dx
    tensor), the position gradient is computed only when x asks for one."""

    @staticmethod
    def forward(ctx, x, emb, offsets_np, res_np, n_levels, bound, C, gridtype, align, interp):
        require_gpu(x)
        _lib.load()
        x = x.detach().contiguous().float()
        emb = emb.detach().contiguous()
        L = len(res_np)
        o_np, o_p = _i32arr(offsets_np)
        r_np, r_p = _i32arr(res_np)
        M = x.shape[0]
        out = torch.empty(M, L * C, dtype=torch.float32, device=x.device)
        _timed("mh_grid_general_fwd", ptr(x), ptr(emb), o_p, r_p, ptr(out), M, L, n_levels, C, gridtype, align, interp, float(bound))
        ctx.save_for_backward(x, emb)
        ctx.meta = (o_np, r_np, n_levels, float(bound), L, C, gridtype, align, interp)
        return out

    @staticmethod
    def backward(ctx, grad):
        x, emb = ctx.saved_tensors
        o_np, r_np, n_levels, bound, L, C, gridtype, align, interp = ctx.meta
        o_p, r_p = o_np.ctypes.data_as(ctypes.c_void_p), r_np.ctypes.data_as(ctypes.c_void_p)
        grad = grad.contiguous().float()
        M = x.shape[0]
        g_emb = torch.zeros_like(emb)
        g_x = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        emb_acc = torch.empty(emb.numel() + 1, dtype=torch.int64, device=emb.device)       # fixed-point table sum + max |grad|
        _timed("mh_grid_general_bwd", ptr(grad), ptr(x), ptr(emb), o_p, r_p, ptr(g_emb), ptr(emb_acc), ptr(g_x), M, L, n_levels, C,
               gridtype, align, interp, bound)
        return (g_x, g_emb if ctx.needs_input_grad[1] else None, None, None, None, None, None, None, None, None)


def grid_encode_general(x, emb, offsets_np, res_np, bound, max_level=None, C: int = 2, gridtype="hash", align_corners=False,
                        interp="linear"):
    """x [..,3] in world units -> [.., L*C] for any configuration of the reference operator (D = 3): C in {1, 2, 4, 8},
    gridtype 'hash' / 'tiled', align_corners, interp 'linear' / 'smoothstep' (names or the reference's ids, grid.py:13-21).
    Level-major, channel-minor; levels >= the effective count (grid.py:42) are zero."""
    L = len(res_np)
    C = int(C)
    _grid_table(emb, offsets_np, C)
    lead = list(x.shape[:-1])
    out = _GridEncodeGeneral.apply(x.reshape(-1, 3), emb, offsets_np, res_np, effective_levels(max_level, L), float(bound), C,
                                   _grid_switch(GRID_TYPES, gridtype, "gridtype"), int(bool(align_corners)),
                                   _grid_switch(GRID_INTERPS, interp, "interpolation"))
    return out.view(lead + [L * C])


def _grid_grad_target(emb, grad, offsets_np, C):
    _grid_table(emb, offsets_np, C)
    require_gpu(grad)
    if grad.dtype != torch.float32 or grad.shape != emb.shape or not grad.is_contiguous():
        raise ValueError(f"gradient buffer {tuple(grad.shape)} {grad.dtype}: expected contiguous fp32 {tuple(emb.shape)}")


@torch.no_grad()
def grid_grad_tv(x, emb, grad, offsets_np, res_np, weight: float, bound: float = 1.0, C: int = 2, gridtype="hash",
                 align_corners=False, normalized: bool = False):
    """Total-variation gradient of the table (kernel_grad_tv, gridencoder.cu:526-631) at the points x [..,3], ADDED to `grad`
    ([rows, C], contiguous; may be a view into a flat gradient bucket) in place.  normalized: x holds u in [0,1] already."""
    C = int(C)
    _grid_grad_target(emb, grad, offsets_np, C)
    require_gpu(x)
    x = x.detach().reshape(-1, 3).contiguous().float()
    emb = emb.detach().contiguous()
    _, o_p = _i32arr(offsets_np)
    _, r_p = _i32arr(res_np)
    acc = torch.empty(emb.numel(), dtype=torch.int64, device=emb.device)
    _timed("mh_grid_grad_tv", ptr(x), ptr(emb), o_p, r_p, ptr(grad), ptr(acc), float(weight), x.shape[0], len(res_np), C,
           _grid_switch(GRID_TYPES, gridtype, "gridtype"), int(bool(align_corners)), int(bool(normalized)), float(bound))
    return grad


@torch.no_grad()
def grid_grad_wd(emb, grad, offsets_np, weight: float, C: int = 2):
    """Level-wise mean weight decay (kernel_grad_wd, gridencoder.cu:671-703): grad[i] += 2 weight emb[i] / rows(level of i), in place."""
    C = int(C)
    _grid_grad_target(emb, grad, offsets_np, C)
    _, o_p = _i32arr(offsets_np)
    _timed("mh_grid_grad_wd", ptr(emb.detach().contiguous()), o_p, ptr(grad), float(weight), len(offsets_np) - 1, C)
    return grad


# ------------------------------------------------------------------------------------ compositor
class _Composite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sigma, t_starts, t_ends, rgb, ray_start, ray_cnt, padded=False):
        ctx.set_materialize_grads(False)      # unused outputs hand backward None, not a zero-filled tensor (one launch each)
        require_gpu(sigma, t_starts, t_ends, rgb, ray_start, ray_cnt)
        sigma, t_starts, t_ends = sigma.detach().contiguous(), t_starts.contiguous(), t_ends.contiguous()
        rgbc = rgb.detach().contiguous()
        N, M = ray_start.shape[0], sigma.shape[0]
        dev = sigma.device
        # padded: the packed arrays are longer than the rays' samples (fixed-capacity sampling); entries no ray owns are
        # never visited by the kernels (one wavefront per ray) and must read as weight 0 / gradient 0
        ctx.padded = bool(padded)
        weights = torch.zeros(M, device=dev) if padded else torch.empty(M, device=dev)
        opacity, depth = torch.empty(N, device=dev), torch.empty(N, device=dev)
        color = torch.empty(N, 3, device=dev)
        _timed("mh_composite_fwd", ptr(sigma), ptr(t_starts), ptr(t_ends), ptr(rgbc), ptr(ray_start), ptr(ray_cnt), ptr(weights),
               ptr(opacity), ptr(depth), ptr(color), N)
        ctx.save_for_backward(sigma, t_starts, t_ends, rgbc, ray_start, ray_cnt, weights)
        return weights, opacity, depth, color

    @staticmethod
    def backward(ctx, g_w, g_o, g_d, g_c):
        sigma, ts, te, rgb, ray_start, ray_cnt, weights = ctx.saved_tensors
        N = ray_start.shape[0]
        c = lambda t: None if t is None else t.contiguous()
        d_sigma = torch.zeros_like(sigma) if ctx.padded else torch.empty_like(sigma)
        d_rgb = torch.zeros_like(rgb) if ctx.padded else torch.empty_like(rgb)
        _timed("mh_composite_bwd", ptr(sigma), ptr(ts), ptr(te), ptr(rgb), ptr(ray_start), ptr(ray_cnt), ptr(weights), ptr(c(g_w)),
               ptr(c(g_o)), ptr(c(g_d)), ptr(c(g_c)), ptr(d_sigma), ptr(d_rgb), N)
        return d_sigma, None, None, d_rgb, None, None, None


def composite(sigma, t_starts, t_ends, rgb, ray_start, ray_cnt, padded: bool = False):
    """-> weights [M], opacity [N], depth [N], color [N,3]  (morpheus.py:675-685).  padded: see _Composite.forward."""
    return _Composite.apply(sigma, t_starts, t_ends, rgb, ray_start, ray_cnt, padded)


def packed_info(ray_indices: torch.Tensor, n_rays: int):
    """(ray_start, ray_cnt) int32 from sorted packed ray indices (no host sync)."""
    cnt = torch.bincount(ray_indices, minlength=n_rays)
    start = torch.cumsum(cnt, 0) - cnt
    return start.to(torch.int32), cnt.to(torch.int32)


# ------------------------------------------------------------------------------------ sampler / rays
def generate_rays(fx, fy, cx, cy, c2w, H, W, device):
    c2w = np.ascontiguousarray(np.asarray(c2w, dtype=np.float32).reshape(4, 4))
    o = torch.empty(H * W, 3, device=device)
    d = torch.empty(H * W, 3, device=device)
    require_gpu(o)
    _timed("mh_generate_rays", float(fx), float(fy), float(cx), float(cy), c2w.ctypes.data_as(ctypes.c_void_p), H, W, ptr(o),
           ptr(d))
    return o, d


def _intrinsics4(K):
    """fx, fy, cx, cy of a 3x3 intrinsic matrix as Python floats (rounded to fp32 at the C boundary, as torch casts the
    reference's float64 entries when they meet its fp32 pixel grid)"""
    return float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])


def _frame_pix(frame_idx, pix, n_views, HW):
    """checked (frame_idx int64 [B] | None, pix int32 [N] | None, N) of the device-pose ray kernels"""
    if frame_idx is not None:
        require_gpu(frame_idx)
        if frame_idx.dtype != torch.int64 or frame_idx.shape != (n_views,):
            raise ValueError(f"frame indices must be int64 [{n_views}], got {frame_idx.dtype} {tuple(frame_idx.shape)}")
        frame_idx = frame_idx.contiguous()
    if pix is None:
        return frame_idx, None, HW
    require_gpu(pix)
    if pix.dtype != torch.int32 or pix.dim() != 1:
        raise ValueError(f"pix must be int32 [N], got {pix.dtype} {tuple(pix.shape)}")
    return frame_idx, pix.contiguous(), pix.shape[0]


def generate_rays_dev(K, poses_dev, H: int, W: int, pix=None, frame_idx=None, num_frames: int = 0):
    """Rays of B camera poses that live on the device (`mh_generate_rays_dev`): fp32 [B,4,4] -> rays_o, rays_d [B,N,3] with the
    arithmetic of `generate_rays`, bit for bit.  `pix`: int32 [N] pixel indices (j*W+i) on the device, shared by the poses and
    clamped into the image; None = all H*W pixels.  With `frame_idx` (int64 [B] on the device, clamped into [0, num_frames))
    -> rays_o, rays_d, rays_t [B,N,1] = f / num_frames, rays_id int64 [B,N,1]."""
    require_gpu(poses_dev)
    if poses_dev.dtype != torch.float32 or poses_dev.dim() != 3 or poses_dev.shape[1:] != (4, 4):
        raise ValueError(f"poses must be float32 [B,4,4], got {poses_dev.dtype} {tuple(poses_dev.shape)}")
    poses_dev, dev, B = poses_dev.contiguous(), poses_dev.device, poses_dev.shape[0]
    frame_idx, pix, N = _frame_pix(frame_idx, pix, B, H * W)
    o, d = torch.empty(B, N, 3, device=dev), torch.empty(B, N, 3, device=dev)
    t = i = None
    if frame_idx is not None:
        t, i = torch.empty(B, N, 1, device=dev), torch.empty(B, N, 1, dtype=torch.int64, device=dev)
    _timed("mh_generate_rays_dev", *_intrinsics4(K), ptr(poses_dev), B, H, W, ptr(pix), N, ptr(frame_idx), int(num_frames),
           ptr(o), ptr(d), ptr(t), ptr(i))
    return (o, d) if frame_idx is None else (o, d, t, i)


def dataset_sample(K, poses, rgb, depth, mask, theta, phi, radius, depth_scale: float, frame_idx, pix=None):
    """One real-view batch in one launch (`mh_dataset_sample`, datasets/dataset.py:398-433) from device-resident frames: rgb uint8
    [F,H,W,3], depth uint16 / float32 [F,H,W], mask uint8 [F,H,W], poses fp32 [F,4,4], theta / phi / radius fp32 [F].
    frame_idx int64 [B], pix int32 [N] | None (the whole frame); both on the device, clamped by the kernel.
    -> dict(rays_o, rays_d [B,N,3], rays_t [B,N,1], rays_id int64 [B,N,1], image [B,3,N], depth [B,N], mask int64 [B,N],
            pose [B,4,4], theta, phi, radius [B])"""
    require_gpu(poses, rgb, depth, mask, theta, phi, radius, frame_idx)
    F, H, W = rgb.shape[:3]
    if rgb.dtype != torch.uint8 or rgb.shape != (F, H, W, 3) or mask.dtype != torch.uint8 or mask.shape != (F, H, W):
        raise ValueError("rgb must be uint8 [F,H,W,3] and mask uint8 [F,H,W]")
    if depth.dtype not in (torch.uint16, torch.float32) or depth.shape != (F, H, W):
        raise ValueError("depth must be uint16 or float32 [F,H,W]")
    if poses.dtype != torch.float32 or poses.shape != (F, 4, 4):
        raise ValueError("poses must be float32 [F,4,4]")
    for v in (theta, phi, radius):
        if v.dtype != torch.float32 or v.shape != (F,):
            raise ValueError("theta, phi and radius must be float32 [F]")
    dev, B = rgb.device, frame_idx.shape[0]
    frame_idx, pix, N = _frame_pix(frame_idx, pix, B, H * W)
    f32 = dict(device=dev, dtype=torch.float32)
    out = dict(rays_o=torch.empty(B, N, 3, **f32), rays_d=torch.empty(B, N, 3, **f32), rays_t=torch.empty(B, N, 1, **f32),
               rays_id=torch.empty(B, N, 1, dtype=torch.int64, device=dev), image=torch.empty(B, 3, N, **f32),
               depth=torch.empty(B, N, **f32), mask=torch.empty(B, N, dtype=torch.int64, device=dev),
               pose=torch.empty(B, 4, 4, **f32), theta=torch.empty(B, **f32), phi=torch.empty(B, **f32),
               radius=torch.empty(B, **f32))
    _timed("mh_dataset_sample", *_intrinsics4(K), ptr(poses), ptr(rgb), ptr(depth), int(depth.dtype == torch.float32),
           float(depth_scale), ptr(mask), ptr(theta), ptr(phi), ptr(radius), F, H, W, ptr(frame_idx), B, ptr(pix), N,
           *(ptr(out[k]) for k in ("rays_o", "rays_d", "rays_t", "rays_id", "image", "depth", "mask", "pose", "theta", "phi",
                                   "radius")))
    return out


VIRTUAL_ANGLES, VIRTUAL_SPHERE, VIRTUAL_POLAR = 0, 1, 2


def dataset_virtual_pose(mode: int, a, b, c, frame_idx, radius, theta, phi, radius_factor: float, bounds):
    """Look-at poses, view labels and deltas of B virtual views in one launch (`mh_dataset_virtual_pose`).  mode / a, b, c: see
    include/morpheus_hip.h; `bounds`: the six label thresholds (front/2, pi - front/2, pi + front/2, 2 pi - front/2, overhead,
    pi - overhead) as float64 Python numbers.  -> dict(pose [B,4,4], dir int64 [B], polar, azimuth, radius [B], deg [B,2])"""
    require_gpu(a, b, c, frame_idx, radius, theta, phi)
    B, dev, F = a.shape[0], a.device, radius.shape[0]
    for v in (a, b) + ((c,) if c is not None else ()):
        if v.dtype != torch.float32 or v.shape != (B,):
            raise ValueError(f"draws must be float32 [{B}], got {v.dtype} {tuple(v.shape)}")
    if mode == VIRTUAL_SPHERE and c is None:
        raise ValueError("the sphere branch takes three normal draws")
    frame_idx, _, _ = _frame_pix(frame_idx, None, B, 0)
    a, b, c = a.contiguous(), b.contiguous(), None if c is None else c.contiguous()
    f32 = dict(device=dev, dtype=torch.float32)
    out = dict(pose=torch.empty(B, 4, 4, **f32), dir=torch.empty(B, dtype=torch.int64, device=dev), polar=torch.empty(B, **f32),
               azimuth=torch.empty(B, **f32), radius=torch.empty(B, **f32), deg=torch.empty(B, 2, **f32))
    _timed("mh_dataset_virtual_pose", int(mode), ptr(a), ptr(b), ptr(c), ptr(frame_idx), B, ptr(radius), ptr(theta), ptr(phi), F, float(radius_factor), *(float(x) for x in bounds),
           *(ptr(out[k]) for k in ("pose", "dir", "polar", "azimuth", "radius", "deg")))
    return out


def prep_frames(rgb, depth, mask, origin, inv_affine, rotated, table_inside, table_padded, size_h: int, size_w: int):
    """Rotate, cut and mark the padding of every frame of a raw sequence in one launch (`mh_prep_frames`, the reference's
    preprocess/preprocess.py:rotate_and_crop_frames and its write expressions): rgb uint8 [F,H,W,3], depth uint16 [F,H,W], mask
    uint8 [F,H,W]; origin int32 [F,2] (top, left); inv_affine float64 [F,6]; rotated uint8 [F]; the two depth tables uint16
    [65536]; all on the device.  -> dict(rgb uint8 [F,h,w,3], depth uint16 [F,h,w], mask uint8 [F,h,w], padding uint8 [F,h,w])"""
    require_gpu(rgb, depth, mask, origin, inv_affine, rotated, table_inside, table_padded)
    F, H, W = rgb.shape[:3]
    if rgb.dtype != torch.uint8 or rgb.shape != (F, H, W, 3) or mask.dtype != torch.uint8 or mask.shape != (F, H, W):
        raise ValueError("rgb must be uint8 [F,H,W,3] and mask uint8 [F,H,W]")
    if depth.dtype != torch.uint16 or depth.shape != (F, H, W):
        raise ValueError("depth must be uint16 [F,H,W]")
    if origin.dtype != torch.int32 or origin.shape != (F, 2):
        raise ValueError(f"origin must be int32 [{F},2], got {origin.dtype} {tuple(origin.shape)}")
    if inv_affine.dtype != torch.float64 or inv_affine.shape != (F, 6):
        raise ValueError(f"inv_affine must be float64 [{F},6], got {inv_affine.dtype} {tuple(inv_affine.shape)}")
    if rotated.dtype != torch.uint8 or rotated.shape != (F,):
        raise ValueError(f"rotated must be uint8 [{F}], got {rotated.dtype} {tuple(rotated.shape)}")
    for t in (table_inside, table_padded):
        if t.dtype != torch.uint16 or t.shape != (65536,):
            raise ValueError("the depth tables must be uint16 [65536]")
    h, w = int(size_h), int(size_w)
    if h <= 0 or w <= 0 or F * h * w >= 2 ** 31 or H * W >= 2 ** 31:
        raise ValueError(f"window {h} x {w} of {F} frames {H} x {W}: sizes must be positive, F h w and H W below 2^31")
    dev = rgb.device
    u8 = dict(device=dev, dtype=torch.uint8)
    out = dict(rgb=torch.empty(F, h, w, 3, **u8), depth=torch.empty(F, h, w, device=dev, dtype=torch.uint16),
               mask=torch.empty(F, h, w, **u8), padding=torch.empty(F, h, w, **u8))
    rgb, depth, mask, origin, inv_affine, rotated, table_inside, table_padded = (
        t.contiguous() for t in (rgb, depth, mask, origin, inv_affine, rotated, table_inside, table_padded))
    _timed("mh_prep_frames", ptr(rgb), ptr(depth), ptr(mask), F, H, W, ptr(origin), ptr(inv_affine), ptr(rotated),
           ptr(table_inside), ptr(table_padded), h, w, *(ptr(out[k]) for k in ("rgb", "depth", "mask", "padding")))
    return out


def sample_uniform(rays_o, rays_d, jitter, S: int, bound: float, with_xyz: bool = False):
    """-> ray_idx int32 [N*S], t_starts, t_ends, xyz|None, ray_start, ray_cnt (no_grad, like morpheus.py:628)."""
    require_gpu(rays_o, rays_d, jitter)
    o, d, j = rays_o.detach().contiguous(), rays_d.detach().contiguous(), _ray_jitter(jitter, rays_o.shape[0])
    N, dev = o.shape[0], o.device
    ri = torch.empty(N * S, dtype=torch.int32, device=dev)
    ts, te = torch.empty(N * S, device=dev), torch.empty(N * S, device=dev)
    xyz = torch.empty(N * S, 3, device=dev) if with_xyz else None
    rs, rc = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    _timed("mh_sample_uniform", ptr(o), ptr(d), ptr(j), N, S, float(bound), ptr(ri), ptr(ts), ptr(te), ptr(xyz), ptr(rs), ptr(rc))
    return ri, ts, te, xyz, rs, rc


def rays_sample_uniform(fx, fy, cx, cy, c2w, H: int, W: int, pix, jitter, S: int, bound: float, with_xyz: bool = False):
    """Ray generation + uniform sampler in one launch (`mh_rays_sample_uniform`).  `pix`: int32 [N] pixel indices
    (j*W+i) on the device, the draw of datasets/dataset.py:412-423; None = the whole image.
    -> rays_o, rays_d [N,3], then the `sample_uniform` tuple."""
    require_gpu(jitter)
    c2w = np.ascontiguousarray(np.asarray(c2w, dtype=np.float32).reshape(4, 4))
    j, dev = jitter.contiguous(), jitter.device
    N = j.shape[0]
    if pix is not None:
        require_gpu(pix)
        if pix.dtype != torch.int32 or pix.shape != (N,):
            raise ValueError("pix must be int32 [N], one pixel index per jitter value")
        pix = pix.contiguous()
    elif N > H * W:
        raise ValueError("whole-image mode renders at most H*W rays")
    o, d = torch.empty(N, 3, device=dev), torch.empty(N, 3, device=dev)
    ri = torch.empty(N * S, dtype=torch.int32, device=dev)
    ts, te = torch.empty(N * S, device=dev), torch.empty(N * S, device=dev)
    xyz = torch.empty(N * S, 3, device=dev) if with_xyz else None
    rs, rc = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    _timed("mh_rays_sample_uniform", float(fx), float(fy), float(cx), float(cy), c2w.ctypes.data_as(ctypes.c_void_p), H, W,
           ptr(pix), ptr(j), N, S, float(bound), ptr(o), ptr(d), ptr(ri), ptr(ts), ptr(te), ptr(xyz), ptr(rs), ptr(rc))
    return o, d, ri, ts, te, xyz, rs, rc


def _ray_jitter(jitter, n_rays: int):
    """the per-ray near-plane jitter as the marcher reads it: float32 [n_rays], one value per ray -- the kernels index it by ray
    without a length of their own, so a buffer sized for another batch (a graphed step's static jitter met by an eager render)
    must not get through"""
    if jitter is None:
        return None
    if jitter.numel() != n_rays or jitter.dtype != torch.float32:
        raise ValueError(f"per-ray jitter: expected float32 [{n_rays}], got {jitter.dtype} {tuple(jitter.shape)}")
    return jitter.reshape(-1).contiguous()


# ---- the march: slot rows, a scan of the counts, pack (csrc/march.h behind both slots entries) ---------------------------
def _march_slots(entry, head, N: int, tail, cap: int, dev, call=None):
    """One launch of a slots entry (mh_march_slots / mh_est_march_slots / mh_est_traverse_slots: the arguments are head, N, tail,
    cap and the four outputs) -> (cnt_ovf int32 [N + 1] = [ray_cnt | slot-row overflow flag], rows fp32 [2, N, cap])."""
    cnt_ovf = torch.zeros(N + 1, dtype=torch.int32, device=dev)
    rows = torch.empty(2, N, cap, device=dev)
    (call or _timed)(entry, *head, N, *tail, cap, ptr(cnt_ovf), ptr(rows[0]), ptr(rows[1]), cnt_ovf.data_ptr() + 4 * N)
    return cnt_ovf, rows


def _march_ragged(who: str, entry, head, N: int, tail, cap: int, dev):
    """The ragged result (ray_idx int32 [M], t_starts [M], t_ends [M], ray_start [N], ray_cnt [N]).  One host sync: M = total
    sample count sizes the packed arrays (nerfacc synchronises at the same point); the same read brings the overflow flag, and
    a batch with a ray that overflows its slot row is marched again with a slot row twice as long."""
    if N == 0:
        e = torch.empty(0, device=dev)
        z = torch.empty(0, dtype=torch.int32, device=dev)
        return z, e, e.clone(), z.clone(), z.clone()
    while True:
        cnt_ovf, rows = _march_slots(entry, head, N, tail, cap, dev)
        cnt = cnt_ovf[:N]
        csum = torch.cumsum(cnt_ovf, 0, dtype=torch.int32)              # last element = M + overflow flag
        start = (csum[:N] - cnt).contiguous()
        M, tot = csum[N - 1:].tolist()                                  # the one device->host sync
        if tot == M:                                                    # no overflow
            break
        if cap > (1 << 20):
            raise _lib.MorpheusHipError(f"{who}: a ray takes more than 2^20 steps inside the box (step size / direction scale?)")
        cap *= 2
    ri = torch.empty(M, dtype=torch.int32, device=dev)
    ts, te = torch.empty(M, device=dev), torch.empty(M, device=dev)
    if M > 0:
        _timed("mh_march_pack", ptr(start), ptr(cnt), ptr(rows[0]), ptr(rows[1]), N, cap, ptr(ri), ptr(ts), ptr(te))
    return ri, ts, te, start, cnt.contiguous()


def capped_ranges(cnt: torch.Tensor, slot_overflow: torch.Tensor, capacity: int):
    """The fixed-capacity bookkeeping, on whatever device `cnt` lives (no host read): per-ray counts int32 [N], N > 0, the slot-row
    overflow flag (0-dim) and the packed length -> (start [N], cnt_c [N], n_valid 0-dim, overflow int32 0-dim).
    start is the exclusive scan of cnt clamped to capacity and cnt_c = min(cnt, capacity - start), so start + cnt_c never passes
    capacity, a ray behind the cut has start = capacity, cnt_c = 0, and start stays the exclusive scan of cnt_c.
    n_valid = min(total, capacity); overflow != 0: more samples than capacity, or a ray overflowed its slot row."""
    csum = torch.cumsum(cnt, 0, dtype=torch.int32)
    start = (csum - cnt).clamp_(max=capacity)
    total = csum[-1]
    cnt_c = torch.minimum(cnt, capacity - start)
    n_valid = total.clamp(max=capacity)
    overflow = ((total > capacity) | (slot_overflow != 0)).to(torch.int32)
    return start, cnt_c, n_valid, overflow


def _march_capped(entry, head, N: int, tail, cap: int, dev, capacity: int):
    """The fixed-capacity seven-tuple (ray_idx int32 [capacity], t_starts, t_ends [capacity], ray_start [N], ray_cnt [N], n_valid
    int32 0-dim, overflow int32 0-dim): constant shapes and no device->host sync, so that a training step can be captured in a
    HIP graph.  The first n_valid entries are the packed samples (identical to the ragged ones); the rest is padding (ray 0,
    t = 0) that no ray owns (capped_ranges).  overflow != 0: the caller re-captures with a larger capacity."""
    assert N > 0 and capacity > 0
    cnt_ovf, rows = _march_slots(entry, head, N, tail, cap, dev)
    start, cnt_c, n_valid, overflow = capped_ranges(cnt_ovf[:N], cnt_ovf[N], capacity)
    ri = torch.zeros(capacity, dtype=torch.int32, device=dev)
    ts, te = torch.zeros(capacity, device=dev), torch.zeros(capacity, device=dev)
    _timed("mh_march_pack", ptr(start), ptr(cnt_c), ptr(rows[0]), ptr(rows[1]), N, cap, ptr(ri), ptr(ts), ptr(te))
    return ri, ts, te, start, cnt_c, n_valid, overflow


def _grid_march_args(rays_o, rays_d, jitter, step: float, bound: float, binary: torch.Tensor):
    """-> (head, N, tail, cap, device, keep): mh_march_slots' arguments before N and between N and cap, the slot-row length
    mh_march_cap gives, and the contiguous tensors the pointers in `head` name, which the caller holds while it launches"""
    require_gpu(rays_o, rays_d, jitter, binary)
    lib = _lib.load()
    o, d = rays_o.detach().contiguous(), rays_d.detach().contiguous()
    j = _ray_jitter(jitter, rays_o.shape[0])
    assert binary.dtype == torch.uint8 and binary.is_contiguous() and binary.dim() == 3
    head, tail = (ptr(o), ptr(d), ptr(j)), (float(step), float(bound), binary.shape[0], ptr(binary))
    return head, o.shape[0], tail, int(lib.mh_march_cap(float(step), float(bound))), o.device, (o, d, j)


def march_rays(rays_o, rays_d, jitter, step: float, bound: float, binary: torch.Tensor):
    """Occupancy-grid marcher -> (ray_idx int32 [M], t_starts [M], t_ends [M], ray_start [N], ray_cnt [N]).
    Single pass, one wavefront per ray (mh_march_slots + mh_march_pack); one host sync and the doubling retry of an overflowing
    slot row (directions much shorter than unit length) as _march_ragged states them."""
    head, N, tail, cap, dev, _keep = _grid_march_args(rays_o, rays_d, jitter, step, bound, binary)
    return _march_ragged("march_rays", "mh_march_slots", head, N, tail, cap, dev)


def march_count(rays_o, rays_d, jitter, step: float, bound: float, binary: torch.Tensor) -> torch.Tensor:
    """Total number of samples the marcher would emit for these rays, as a 0-dim int32 DEVICE tensor (no host sync): lets a
    caller size / pick a fixed-capacity buffer ahead of the step (trainstep.GraphedRealViewStep).
    One march at the slot-row length mh_march_cap gives and no retry: the overflow flag is not read, so for a batch with a ray
    that overflows its slot row (directions much shorter than unit length -- march_rays marches such a batch again) the result
    is a LOWER BOUND of march_rays' total, each overflowing ray counted at the slot-row length at most."""
    head, N, tail, cap, dev, _keep = _grid_march_args(rays_o, rays_d, jitter, step, bound, binary)
    if N == 0:
        return torch.zeros((), dtype=torch.int32, device=dev)
    cnt_ovf, _rows = _march_slots("mh_march_slots", head, N, tail, cap, dev, call=launch)
    return cnt_ovf[:N].sum(dtype=torch.int32)


def march_rays_capped(rays_o, rays_d, jitter, step: float, bound: float, binary: torch.Tensor, capacity: int):
    """The same marcher with a FIXED packed length and no device->host sync (_march_capped): -> (ray_idx int32 [capacity],
    t_starts, t_ends [capacity], ray_start [N], ray_cnt [N], n_valid int32 0-dim, overflow int32 0-dim)."""
    head, N, tail, cap, dev, _keep = _grid_march_args(rays_o, rays_d, jitter, step, bound, binary)
    return _march_capped("mh_march_slots", head, N, tail, cap, dev, capacity)


# ------------------------------------------------------------------------------------ occupancy estimator (csrc/estimator.hip)
def _est_grid(aabbs, binary):
    """(L, Rx, Ry, Rz) of a level grid: aabbs fp32 [L,6] and binary uint8 [L,Rx,Ry,Rz], both contiguous on the device"""
    require_gpu(aabbs, binary)
    if binary.dtype != torch.uint8 or binary.dim() != 4 or not binary.is_contiguous():
        raise ValueError(f"estimator grid: binary uint8 [L,Rx,Ry,Rz] contiguous expected, got {binary.dtype} {tuple(binary.shape)}")
    L = binary.shape[0]
    if aabbs.dtype != torch.float32 or tuple(aabbs.shape) != (L, 6) or not aabbs.is_contiguous():
        raise ValueError(f"estimator grid: aabbs float32 [{L},6] contiguous expected, got {aabbs.dtype} {tuple(aabbs.shape)}")
    return (L,) + tuple(int(r) for r in binary.shape[1:])


def _est_slots_rays(who: str, entry: str, rays_o, rays_d, jitter, step, aabbs, binary, diagonal, cone_angle, near_plane, far_plane,
                    t_min, t_max, capacity):
    """the estimator's two placements behind one argument list: `entry` fills the slot rows, mh_march_pack packs them"""
    require_gpu(rays_o, rays_d, jitter, t_min, t_max)
    lib = _lib.load()
    L, Rx, Ry, Rz = _est_grid(aabbs, binary)
    o, d = rays_o.detach().contiguous(), rays_d.detach().contiguous()
    N, dev = o.shape[0], o.device
    j = _ray_jitter(jitter, N)
    tmn, tmx = _ray_jitter(t_min, N), _ray_jitter(t_max, N)
    step, cone, near, far = float(step), float(cone_angle), float(near_plane), float(far_plane)
    cap = int(lib.mh_est_march_cap(step, float(diagonal), near, far))
    if cap <= 0:
        raise ValueError(f"{who}: step {step}, diagonal {diagonal}, planes [{near}, {far}] give no slot row")
    head = (ptr(o), ptr(d), ptr(j), ptr(tmn), ptr(tmx))
    tail = (step, cone, near, far, ptr(aabbs), L, Rx, Ry, Rz, ptr(binary))
    if capacity is not None:
        return _march_capped(entry, head, N, tail, cap, dev, capacity)
    return _march_ragged(who, entry, head, N, tail, cap, dev)


def est_march_rays(rays_o, rays_d, jitter, step: float, aabbs, binary, diagonal: float, cone_angle: float = 0.0,
                   near_plane: float = 0.0, far_plane: float = 1e10, t_min=None, t_max=None, capacity: Optional[int] = None):
    """The estimator's marcher (mh_est_march_slots + mh_march_pack; the definition is in include/morpheus_hip.h).
    capacity None: march_rays' ragged result (ray_idx, t_starts, t_ends, ray_start, ray_cnt), one host read of M and the
    doubling retry of an overflowing slot row.  With a capacity: march_rays_capped's seven results, no host read.
    diagonal: of the coarsest box, a HOST number (the caller keeps it from construction)."""
    return _est_slots_rays("est_march_rays", "mh_est_march_slots", rays_o, rays_d, jitter, step, aabbs, binary, diagonal, cone_angle,
                           near_plane, far_plane, t_min, t_max, capacity)


def est_traverse_rays(rays_o, rays_d, jitter, step: float, aabbs, binary, diagonal: float, cone_angle: float = 0.0,
                      near_plane: float = 0.0, far_plane: float = 1e10, t_min=None, t_max=None, capacity: Optional[int] = None):
    """The estimator's cell-by-cell traversal (mh_est_traverse_slots + mh_march_pack; the definition is in
    include/morpheus_hip.h): est_march_rays' arguments and results, the samples placed run by run from the entry of every
    occupied stretch of cells instead of on the lattice from the clip entry."""
    return _est_slots_rays("est_traverse_rays", "mh_est_traverse_slots", rays_o, rays_d, jitter, step, aabbs, binary, diagonal,
                           cone_angle, near_plane, far_plane, t_min, t_max, capacity)


def est_occupied_list(binary):
    """-> (occ_list int32 [L, cells]: each level's occupied cells in index order, the rest of a row unspecified; occ_cnt int32
    [L]) -- count, a cumsum of the chunk counts on the device, pack.  No host read."""
    require_gpu(binary)
    lib = _lib.load()
    assert binary.dtype == torch.uint8 and binary.dim() == 4 and binary.is_contiguous()
    L, dev = binary.shape[0], binary.device
    cells = int(binary[0].numel())
    n_chunks = -(-cells // int(lib.mh_est_occ_chunk()))
    chunk_cnt = torch.zeros(L, n_chunks, dtype=torch.int32, device=dev)
    _timed("mh_est_occ_count", ptr(binary), L, cells, ptr(chunk_cnt))
    csum = torch.cumsum(chunk_cnt, 1, dtype=torch.int32)
    start = (csum - chunk_cnt).contiguous()
    occ_list = torch.empty(L, cells, dtype=torch.int32, device=dev)
    _timed("mh_est_occ_pack", ptr(binary), L, cells, ptr(start), ptr(occ_list))
    return occ_list, csum[:, -1].contiguous()


def est_select(aabbs, binary, warmup: bool, u_point, uniform=None, u_occ=None, occ_list=None, occ_cnt=None):
    """The cells of one update and the point to evaluate in each (mh_est_select, one launch) -> ids int32 [L,n] (-1: padding),
    points fp32 [L,n,3]; n = cells in warm-up, else 2 (cells // 4)."""
    L, Rx, Ry, Rz = _est_grid(aabbs, binary)
    cells = Rx * Ry * Rz
    k = cells // 4
    n = cells if warmup else 2 * k
    dev = binary.device
    require_gpu(u_point, uniform, u_occ, occ_list, occ_cnt)

    def want(t, shape, dtype, what):
        if t is None or tuple(t.shape) != shape or t.dtype != dtype:
            raise ValueError(f"est_select: {what} {dtype} {list(shape)} expected, got "
                             f"{None if t is None else (t.dtype, tuple(t.shape))}")
        return t.contiguous()

    u_point = want(u_point, (L, n, 3), torch.float32, "u_point")
    if not warmup:
        uniform, u_occ = want(uniform, (L, k), torch.int32, "uniform"), want(u_occ, (L, k), torch.float32, "u_occ")
        occ_list, occ_cnt = want(occ_list, (L, cells), torch.int32, "occ_list"), want(occ_cnt, (L,), torch.int32, "occ_cnt")
    ids = torch.empty(L, n, dtype=torch.int32, device=dev)
    pts = torch.empty(L, n, 3, device=dev)
    if n > 0:
        _timed("mh_est_select", 1 if warmup else 0, L, Rx, Ry, Rz, n, ptr(uniform), ptr(u_occ), ptr(u_point), ptr(occ_list),
               ptr(occ_cnt), ptr(aabbs), ptr(ids), ptr(pts))
    return ids, pts


def est_ema(ids, occ, occs, decay: float):
    """EMA-max of `occs` [L * cells] in place from the evaluations occ [L,n] of the cells ids [L,n] (mh_est_ema)."""
    require_gpu(ids, occ, occs)
    L, n = ids.shape
    occ = occ.detach().reshape(-1).float().contiguous()
    if occ.shape[0] != L * n or ids.dtype != torch.int32 or occs.dtype != torch.float32 or occs.numel() % L:
        raise ValueError(f"est_ema: one evaluation per selected cell ({L * n}) expected, got {tuple(occ.shape)}")
    if n > 0:
        _timed("mh_est_ema", ptr(ids.contiguous()), ptr(occ), L, n, occs.numel() // L, ptr(occs.clone()), float(decay), ptr(occs))


def est_threshold(occs, cap: float, thre=None, binaries=None):
    """thre (fp32 0-dim, device; made when None) = min(mean(occs[occs >= 0]), cap); binaries (uint8 view, optional) = occs > thre."""
    require_gpu(occs, thre, binaries)
    lib = _lib.load()
    if thre is None:
        thre = torch.empty((), device=occs.device)
    part = torch.empty(2 * int(lib.mh_est_max_partials()), dtype=torch.float64, device=occs.device)
    _timed("mh_est_threshold", ptr(occs), occs.numel(), float(cap), ptr(part), ptr(thre), ptr(binaries))
    return thre


def est_mark_invisible(K, c2w, width: int, height: int, near_plane: float, aabbs, binary, occs):
    """occs [L * cells] <- 0 where visible, -1 elsewhere (mh_est_mark_invisible); K [C,3,3], c2w [C,3,4], fp32 on the device."""
    L, Rx, Ry, Rz = _est_grid(aabbs, binary)
    require_gpu(K, c2w, occs)
    K, c2w = K.detach().float().contiguous(), c2w.detach().float().contiguous()
    C = c2w.shape[0]
    if tuple(K.shape) != (C, 3, 3) or tuple(c2w.shape) != (C, 3, 4) or occs.numel() != L * Rx * Ry * Rz:
        raise ValueError(f"est_mark_invisible: K [{C},3,3] and c2w [{C},3,4] expected, got {tuple(K.shape)}, {tuple(c2w.shape)}")
    _timed("mh_est_mark_invisible", ptr(K), ptr(c2w), C, float(width), float(height), float(near_plane), ptr(aabbs), L, Rx, Ry, Rz,
           ptr(occs))


# ------------------------------------------------------------------------------------ visibility pruning (csrc/visibility.hip)
def visibility_mask(values, t_starts, t_ends, ray_start, ray_cnt, early_stop_eps: float = 0.0, alpha_thre=None,
                    alpha_form: bool = False, padded: bool = False):
    """-> keep uint8 [M], kept_cnt int32 [N] (mh_visibility_mask, include/morpheus_hip.h).  values: sigma [M] (alpha_form: the
    opacities themselves); alpha_thre: None, a float, or a float32 DEVICE scalar (no host read).  padded: the packed arrays are
    longer than the rays' samples (fixed-capacity sampling); the entries no ray owns read as keep = 0."""
    require_gpu(values, t_starts, t_ends, ray_start, ray_cnt)
    v = values.detach().reshape(-1).float().contiguous()
    ts, te = t_starts.contiguous(), t_ends.contiguous()
    rs, rc = ray_start.contiguous(), ray_cnt.contiguous()
    M, N, dev = ts.shape[0], rs.shape[0], ts.device
    if v.shape[0] != M or te.shape[0] != M or rc.shape[0] != N or rs.dtype != torch.int32 or rc.dtype != torch.int32:
        raise ValueError(f"visibility_mask: one value per packed sample ({M}) and int32 ray_start / ray_cnt of one length, got "
                         f"{tuple(values.shape)}, {rs.dtype} [{N}], {rc.dtype} [{rc.shape[0]}]")
    if alpha_thre is not None and not torch.is_tensor(alpha_thre):
        alpha_thre = torch.full((), float(alpha_thre), device=dev) if float(alpha_thre) > 0 else None
    if alpha_thre is not None:
        require_gpu(alpha_thre)
        alpha_thre = alpha_thre.detach().reshape(()).float().contiguous()
    keep = torch.zeros(M, dtype=torch.uint8, device=dev) if padded else torch.empty(M, dtype=torch.uint8, device=dev)
    kept = torch.zeros(N, dtype=torch.int32, device=dev)
    _timed("mh_visibility_mask", ptr(v), 1 if alpha_form else 0, ptr(ts), ptr(te), ptr(rs), ptr(rc), N, M, float(early_stop_eps),
           ptr(alpha_thre), ptr(keep), ptr(kept))
    return keep, kept


def visibility_pack(keep, kept_cnt, t_starts, t_ends, ray_start, ray_cnt, padded: bool = False):
    """Order-preserving compaction of the packed samples by `keep` (mh_visibility_pack) -> (ray_idx int32 [M'], t_starts [M'],
    t_ends [M'], ray_start [N], ray_cnt [N], src_index int32 [M']) -- src_index: the packed position each kept sample had, for
    gathering what was computed on the unpruned set.  Ragged (padded=False): M' = the kept total, ONE device->host read, where
    the marcher has one too.  padded=True: M' = M (the marcher's capacity), a seventh result n_valid (int32 0-dim, device)
    counts the kept samples, the rest is the marcher's padding (ray 0, t = 0) that no ray owns; no host synchronisation."""
    require_gpu(keep, kept_cnt, t_starts, t_ends, ray_start, ray_cnt)
    ts, te = t_starts.contiguous(), t_ends.contiguous()
    rs, rc, kc = ray_start.contiguous(), ray_cnt.contiguous(), kept_cnt.contiguous()
    M, N, dev = ts.shape[0], rs.shape[0], ts.device
    if keep.dtype != torch.uint8 or keep.shape != (M,) or kc.shape != (N,) or kc.dtype != torch.int32:
        raise ValueError("visibility_pack: keep uint8 [M] and kept_cnt int32 [N] of visibility_mask expected")
    keep = keep.contiguous()
    new = lambda n, dt: torch.zeros(n, dtype=dt, device=dev) if padded else torch.empty(n, dtype=dt, device=dev)
    if N == 0 or M == 0:
        out = (new(M, torch.int32), new(M, torch.float32), new(M, torch.float32), kc.clone(), kc.clone(), new(M, torch.int32))
        return out + (torch.zeros((), dtype=torch.int32, device=dev),) if padded else out
    csum = torch.cumsum(kc, 0, dtype=torch.int32)
    start = (csum - kc).contiguous()
    M_out = M if padded else int(csum[N - 1])                           # ragged: the one device->host sync
    ri, src = new(M_out, torch.int32), new(M_out, torch.int32)
    ots, ote = new(M_out, torch.float32), new(M_out, torch.float32)
    _timed("mh_visibility_pack", ptr(keep), ptr(ts), ptr(te), ptr(rs), ptr(rc), ptr(start), N, M, M_out, ptr(ri), ptr(ots), ptr(ote),
           ptr(src))
    out = (ri, ots, ote, start, kc, src)
    return out + (csum[N - 1],) if padded else out


def visibility_prune(values, t_starts, t_ends, ray_start, ray_cnt, early_stop_eps: float = 0.0, alpha_thre=None,
                     alpha_form: bool = False, padded: bool = False):
    """visibility_mask + visibility_pack: the packed samples a density (alpha_form: opacity) pass leaves visible
    -> (ray_idx, t_starts, t_ends, ray_start, ray_cnt, src_index[, n_valid])."""
    keep, kept = visibility_mask(values, t_starts, t_ends, ray_start, ray_cnt, early_stop_eps, alpha_thre, alpha_form, padded)
    return visibility_pack(keep, kept, t_starts, t_ends, ray_start, ray_cnt, padded)


# ------------------------------------------------------------------------------------ importance resampling (csrc/resample.hip)
def sample_pdf(bins, weights, u):
    """The reference's utils.sample_pdf with the draws given (mh_sample_pdf): bins fp32 [B,T], weights fp32 [B,T-1], u fp32 [B,n]
    -> samples fp32 [B,n] in the order of u."""
    require_gpu(bins, weights, u)
    lib = _lib.load()
    b, w, uu = (t.detach().contiguous() for t in (bins, weights, u))
    if b.dim() != 2 or w.dim() != 2 or uu.dim() != 2 or any(t.dtype != torch.float32 for t in (b, w, uu)):
        raise ValueError(f"sample_pdf: float32 bins [B,T], weights [B,T-1] and u [B,n] expected, got {tuple(bins.shape)}, "
                         f"{tuple(weights.shape)}, {tuple(u.shape)}")
    B, T = b.shape
    n = uu.shape[1]
    if T < 2 or n < 1 or tuple(w.shape) != (B, T - 1) or uu.shape[0] != B:
        raise ValueError(f"sample_pdf: T >= 2, n >= 1, weights [B,T-1] and u [B,n] expected, got bins {tuple(b.shape)}, weights "
                         f"{tuple(w.shape)}, u {tuple(uu.shape)}")
    out = torch.empty(B, n, device=b.device)
    scratch = torch.empty(B * T, device=b.device) if T - 1 > int(lib.mh_resample_stage()) else None
    if B > 0:
        _timed("mh_sample_pdf", ptr(b), ptr(w), ptr(uu), B, T, n, ptr(scratch), ptr(out))
    return out


def resample_packed(weights, t_starts, t_ends, ray_start, ray_cnt, n: int, jitter=None, eps: float = 1e-5, padded: bool = False,
                    rays_o=None, rays_d=None):
    """The packed samples cut at n inverse-CDF draws per ray (mh_resample_ranges + mh_resample_packed, include/morpheus_hip.h)
    -> (ray_idx int32 [M'], t_starts [M'], t_ends [M'], ray_start [N], ray_cnt [N], xyz [M',3] | None[, n_valid]).
    jitter: fp32 [N,n] in [0,1), None = 0.5 (the reference's det grid).  xyz: the midpoints' positions, with rays_o / rays_d.
    Ragged (padded=False): M' = the new total, ONE device->host read, where the marcher has one too.  padded=True: the inputs
    have the marcher's fixed capacity M, M' = M + n N, a seventh result n_valid (int32 0-dim, device) counts the samples, the rest
    is the marcher's padding (ray 0, t = 0); no host synchronisation."""
    require_gpu(weights, t_starts, t_ends, ray_start, ray_cnt, jitter, rays_o, rays_d)
    lib = _lib.load()
    w = weights.detach().reshape(-1).float().contiguous()
    ts, te = t_starts.detach().contiguous(), t_ends.detach().contiguous()
    rs, rc = ray_start.contiguous(), ray_cnt.contiguous()
    M, N, dev, n = ts.shape[0], rs.shape[0], ts.device, int(n)
    if n < 1:
        raise ValueError(f"resample_packed: n = {n} draws (at least one)")
    if w.shape[0] != M or te.shape[0] != M or rc.shape[0] != N or rs.dtype != torch.int32 or rc.dtype != torch.int32 or \
            ts.dtype != torch.float32 or te.dtype != torch.float32:
        raise ValueError(f"resample_packed: one weight per packed sample ({M}), float32 t_starts / t_ends and int32 ray_start / "
                         f"ray_cnt of one length, got {tuple(weights.shape)}, {rs.dtype} [{N}], {rc.dtype} [{rc.shape[0]}]")
    if jitter is not None:
        if jitter.dtype != torch.float32 or tuple(jitter.shape) != (N, n):
            raise ValueError(f"resample_packed: jitter float32 [{N},{n}] expected, got {jitter.dtype} {tuple(jitter.shape)}")
        jitter = jitter.detach().contiguous()
    if (rays_o is None) != (rays_d is None):
        raise ValueError("resample_packed: rays_o and rays_d together (the midpoints' positions), or neither")
    limit = M + n * N
    if limit > 0x7fffffff:
        raise ValueError(f"resample_packed: {M} + {n} x {N} output samples do not fit int32 positions")
    new_rs, new_rc = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    total = torch.empty((), dtype=torch.int32, device=dev)
    _timed("mh_resample_ranges", ptr(rs), ptr(rc), N, M, n, limit, ptr(new_rs), ptr(new_rc), ptr(total))
    M_out = limit if padded else int(total)                           # ragged: the one device->host sync
    new = (lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev)) if padded else \
        (lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device=dev))
    ri, ots, ote = new(M_out, dtype=torch.int32), new(M_out), new(M_out)
    xyz = None
    if rays_o is not None:
        o, d = rays_o.detach().float().contiguous(), rays_d.detach().float().contiguous()
        if tuple(o.shape) != (N, 3) or tuple(d.shape) != (N, 3):
            raise ValueError(f"resample_packed: rays_o / rays_d [{N},3] expected, got {tuple(o.shape)}, {tuple(d.shape)}")
        xyz = new(M_out, 3)
    else:
        o = d = None
    if N > 0 and M > 0 and M_out > 0:
        long_rays = M > int(lib.mh_resample_stage())                  # only then can a ray be longer than the LDS staging
        s_cdf = torch.empty(M + N, device=dev) if long_rays else None
        s_cnt = torch.empty(M, dtype=torch.int32, device=dev) if long_rays else None
        _timed("mh_resample_packed", ptr(w), ptr(ts), ptr(te), ptr(rs), ptr(rc), ptr(new_rs), N, M, n, ptr(jitter), float(eps),
               ptr(s_cdf), ptr(s_cnt), M_out, ptr(o), ptr(d), ptr(ri), ptr(ots), ptr(ote), ptr(xyz))
    out = (ri, ots, ote, new_rs, new_rc, xyz)
    return out + (total,) if padded else out


# ------------------------------------------------------------------------------------ field-query glue (csrc/normal.hip)
class _FdTaps(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, topo, eps, bound):
        ctx.set_materialize_grads(False)      # unused outputs hand backward None, not a zero-filled tensor (one launch each)
        require_gpu(x, topo)
        xc = x.detach().contiguous().float()
        M, dev = xc.shape[0], xc.device
        tc = None if topo is None else topo.detach().contiguous().float()
        C = 0 if tc is None else tc.shape[1]
        taps = _scratch(6 * M * 3, dev).view(6 * M, 3)
        topo6 = torch.empty(6 * M, C, device=dev) if tc is not None else torch.empty(0, device=dev)
        launch("mh_fd_taps", ptr(xc), ptr(tc), C, float(eps), float(bound), M, ptr(taps), ptr(topo6 if tc is not None else None))
        ctx.save_for_backward(xc)
        ctx.meta = (float(eps), float(bound), C, topo is not None)
        if not ctx.needs_input_grad[0]:
            ctx.mark_non_differentiable(taps)       # taps of positions without gradient: the field skips its d/dx stage
        if topo is None or not ctx.needs_input_grad[1]:
            ctx.mark_non_differentiable(topo6)
        return taps, topo6

    @staticmethod
    def backward(ctx, g_taps, g_topo6):
        (xc,) = ctx.saved_tensors
        eps, bound, C, has_topo = ctx.meta
        M, dev = xc.shape[0], xc.device
        want_x = ctx.needs_input_grad[0] and g_taps is not None
        want_t = has_topo and ctx.needs_input_grad[1] and g_topo6 is not None
        g_x = torch.empty(M, 3, device=dev) if want_x else None
        g_t = torch.empty(M, C, device=dev) if want_t else None
        if want_x or want_t:
            launch("mh_fd_taps_bwd", ptr(xc), ptr(g_taps.contiguous() if want_x else None),
                   ptr(g_topo6.contiguous() if want_t else None), C, eps, bound, M, ptr(g_x), ptr(g_t))
        return g_x, g_t, None, None


def fd_taps(x, topo, eps: float, bound: float):
    """-> taps [6M,3] (point-major: +x,-x,+y,-y,+z,-z, clamped to the box), topo6 [6M,C] or None  (model.py:367-376)."""
    taps, topo6 = _FdTaps.apply(x, topo, eps, bound)
    return taps, (None if topo is None else topo6)


class _FdNormal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sdf6, eps):
        ctx.set_materialize_grads(False)      # unused outputs hand backward None, not a zero-filled tensor (one launch each)
        require_gpu(sdf6)
        s = sdf6.detach().contiguous().float()
        M, dev = s.shape[0], s.device
        normal, raw = torch.empty(M, 3, device=dev), torch.empty(M, 3, device=dev)
        launch("mh_fd_normal_fwd", ptr(s), float(eps), M, ptr(normal), ptr(raw))
        ctx.save_for_backward(s)
        ctx.eps = float(eps)
        return normal, raw

    @staticmethod
    def backward(ctx, g_n, g_r):
        (s,) = ctx.saved_tensors
        g = torch.empty_like(s)
        c = lambda t: None if t is None else t.contiguous()
        launch("mh_fd_normal_bwd", ptr(s), ptr(c(g_n)), ptr(c(g_r)), ctx.eps, s.shape[0], ptr(g))
        return g, None


def fd_normal(sdf6, eps: float):
    """sdf6 [M,6] -> (normal [M,3] = nan_to_num(safe_normalize(raw)), raw [M,3])   (model.py:377-398)."""
    return _FdNormal.apply(sdf6, eps)


class _MultiCode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, v0, v1, v2):
        ctx.set_materialize_grads(False)      # unused outputs hand backward None, not a zero-filled tensor (one launch each)
        require_gpu(t, v0, v1, v2)
        tc = t.detach().reshape(-1).contiguous().float()
        vs = [v.detach().contiguous() for v in (v0, v1, v2)]           # [1, C, size, 1]: contiguous == [C, size]
        C, sizes, F = vs[0].shape[1], [v.shape[2] for v in vs], tc.shape[0]
        out = torch.empty(F, 3 * C, device=tc.device)
        launch("mh_multicode_fwd", ptr(tc), ptr(vs[0]), ptr(vs[1]), ptr(vs[2]), sizes[0], sizes[1], sizes[2], C, F, ptr(out))
        ctx.save_for_backward(tc)
        ctx.meta = (C, sizes, [tuple(v.shape) for v in vs])
        return out

    @staticmethod
    def backward(ctx, g_out):
        (tc,) = ctx.saved_tensors
        C, sizes, shapes = ctx.meta
        flat = torch.zeros(C * sum(sizes), device=tc.device)
        gs, o = [], 0
        for sz in sizes:
            gs.append(flat[o:o + C * sz])
            o += C * sz
        launch("mh_multicode_bwd", ptr(tc), ptr(g_out.contiguous()), ptr(gs[0]), ptr(gs[1]), ptr(gs[2]), sizes[0], sizes[1],
               sizes[2], C, tc.shape[0])
        return (None, *[g.view(sh) for g, sh in zip(gs, shapes)])


def multicode_sample(t, volumes):
    """t [F] or [F,1] in [0,1] (clamped) -> [F, 3*C]: deform_code.py:20-38 for the three-level code grid, one launch."""
    assert len(volumes) == 3
    return _MultiCode.apply(t, *volumes)


class _SdfLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred_sdf, ts, te, ray_idx, rays_depth, rays_mask, trunc, n_valid=None):
        ctx.set_materialize_grads(False)      # unused outputs hand backward None, not a zero-filled tensor (one launch each)
        require_gpu(pred_sdf, ts, te, ray_idx, rays_depth, rays_mask, n_valid)
        p = pred_sdf.detach().contiguous().float()
        dep = rays_depth.detach().reshape(-1).contiguous().float()
        msk = None if rays_mask is None else rays_mask.detach().reshape(-1).contiguous().float()
        sums = torch.empty(3, device=p.device)
        nv = None if n_valid is None else n_valid.detach().reshape(1).to(torch.int32).contiguous()
        launch("mh_sdf_losses_fwd", ptr(p), ptr(ts), ptr(te), ptr(ray_idx), ptr(dep), ptr(msk), float(trunc), p.shape[0], ptr(nv),
               ptr(sums))
        ctx.save_for_backward(p, ts, te, ray_idx, dep, msk, sums, nv)
        ctx.trunc = float(trunc)
        return sums[0] / sums[2], sums[1] / sums[2]

    @staticmethod
    def backward(ctx, g_fs, g_sl):
        p, ts, te, ray_idx, dep, msk, sums, nv = ctx.saved_tensors
        g = torch.empty_like(p)
        c = lambda t: None if t is None else t.reshape(1).contiguous().float()
        launch("mh_sdf_losses_bwd", ptr(p), ptr(ts), ptr(te), ptr(ray_idx), ptr(dep), ptr(msk), ctx.trunc, p.shape[0], ptr(nv),
               ptr(sums), ptr(c(g_fs)), ptr(c(g_sl)), ptr(g))
        return g, None, None, None, None, None, None, None


def sdf_losses(pred_sdf, t_starts, t_ends, ray_idx, rays_depth, rays_mask, trunc: float, n_valid=None):
    """-> (fs_loss, sdf_loss) of utils.py:91-113 on packed samples; rays_depth / rays_mask are PER RAY ([N] or [N,1], mask may
    be None) and read through ray_idx (int32 [M]); the sample depth is (t_starts + t_ends) / 2.  n_valid: 0-dim device int
    tensor -- only the first n_valid packed entries are samples (march_rays_capped) -- or None."""
    return _SdfLosses.apply(pred_sdf, t_starts.contiguous(), t_ends.contiguous(), ray_idx.contiguous(), rays_depth, rays_mask,
                            trunc, n_valid)


class _SamplePositions(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rays_o, rays_d, ray_idx, ts, te, ray_start, ray_cnt):
        ctx.set_materialize_grads(False)      # unused outputs hand backward None, not a zero-filled tensor (one launch each)
        require_gpu(rays_o, rays_d, ray_idx, ts, te)
        o, d = rays_o.detach().contiguous().float(), rays_d.detach().contiguous().float()
        M = ts.shape[0]
        xyz = torch.empty(M, 3, device=o.device)
        launch("mh_sample_positions", ptr(o), ptr(d), ptr(ray_idx), ptr(ts), ptr(te), M, ptr(xyz))
        ctx.save_for_backward(ts, te, ray_start, ray_cnt)
        ctx.n = o.shape[0]
        return xyz

    @staticmethod
    def backward(ctx, g_xyz):
        ts, te, ray_start, ray_cnt = ctx.saved_tensors
        g_o, g_d = torch.empty(ctx.n, 3, device=ts.device), torch.empty(ctx.n, 3, device=ts.device)
        launch("mh_sample_positions_bwd", ptr(g_xyz.contiguous()), ptr(ts), ptr(te), ptr(ray_start), ptr(ray_cnt), ctx.n, ptr(g_o),
               ptr(g_d))
        return g_o, g_d, None, None, None, None, None


def sample_positions(rays_o, rays_d, ray_idx, t_starts, t_ends, ray_start, ray_cnt):
    """xyz [M,3] = rays_o[ri] + rays_d[ri] * (t_starts + t_ends) / 2 (morpheus.py:644-647) for packed, ray-major samples;
    backward is a per-ray segment sum (no sort, no atomics).  ray_idx int32 [M]; ray_start / ray_cnt int32 [N]."""
    return _SamplePositions.apply(rays_o, rays_d, ray_idx.contiguous(), t_starts.contiguous(), t_ends.contiguous(),
                                  ray_start.contiguous(), ray_cnt.contiguous())


def sample_positions_nograd(rays_o, rays_d, ray_idx, t_starts, t_ends):
    """sample_positions' forward alone (mh_sample_positions), for passes that carry no gradient and know no segment table: the
    density pass of a pruned render is handed nerfacc's (t_starts, t_ends, ray_indices) only."""
    require_gpu(rays_o, rays_d, ray_idx, t_starts, t_ends)
    o, d = rays_o.detach().contiguous().float(), rays_d.detach().contiguous().float()
    ri, ts, te = ray_idx.contiguous(), t_starts.contiguous(), t_ends.contiguous()
    if ri.dtype != torch.int32:
        ri = ri.to(torch.int32)
    M = ts.shape[0]
    xyz = torch.empty(M, 3, device=o.device)
    launch("mh_sample_positions", ptr(o), ptr(d), ptr(ri), ptr(ts), ptr(te), M, ptr(xyz))
    return xyz


# ------------------------------------------------------------------------------------ fused MLPs
# A/B and test switch: 0 = dPre4 of the warp nets is parked by backward-data and read by the weight gradients (the round-5 form)
REGEN_DPRE4 = os.environ.get("MORPHEUS_REGEN_DPRE4", "1") != "0"


# `arith` of the MLP entry points (include/morpheus_hip.h: MH_ARITH_F32, MH_ARITH_B3), by "is it the b3 form?"
_ARITH = {False: 0, True: 1}


# A/B and test switch: False = every field query returns its own gradient tensors and autograd adds them up (the round-3 form).
# The in-place sums are keyed on autograd's graph-task id (torch >= 2.1); without it the per-query form is used.
_GRAPH_TASK_ID = getattr(torch._C, "_current_graph_task_id", None)
ACCUMULATE_IN_PLACE = _GRAPH_TASK_ID is not None and os.environ.get("MORPHEUS_ACCUMULATE_IN_PLACE", "1") != "0"


class _QueryAccumulator:
    """Running gradient sums of ONE backward pass, shared by the field queries that were given the same prepared operands
    (`MLPOperands.acc`; a real-view training step issues six: render, finite-difference taps, regularisers, point loss).

    Each query's backward produces (a) the raw weight / bias / beta gradient [24 929], (b) a full table gradient [419 640, 2] per
    hash table.  Handed to autograd one tensor per query, that is a zero fill per table and an add per tensor per extra query
    (about 30 launches of 0.1 - 3.4 MB per step).  Instead the queries ADD INTO ONE TENSOR EACH inside their own kernels
    (mh_field_bwd_fused's reduction launch with accumulate = 1; the brick kernel's last pass adds into the table) and return None
    for token, beta and tables; `_PackOperands.backward` -- the node behind the token every query takes, which autograd runs only
    after ALL of them have run, None gradients included -- hands the finished sums to beta and the tables (its extra inputs) and
    maps the raw sum to the parameters.  Gradients that reach beta or a table along other paths are added by autograd as usual:
    the sums are complete when they are handed over, nothing is modified afterwards.

    A query joins only if it uses the very beta tensor and table parameters the operands were prepared with; any other query gets
    its own tensors as before.  State is keyed on the autograd graph task: a new backward pass starts empty, whatever the last
    one left behind."""

    def __init__(self, beta=None, tables=()):
        self.bound = beta is not None
        self.keep = (beta, tuple(tables))            # the ids below stay theirs for as long as the accumulator lives
        self.ids = (id(beta),) + tuple(id(t) for t in tables)
        self.task = None
        self.reset()

    def reset(self):
        self.raw = None                              # [raw_len + 1] running sum: weight / bias gradients, then d(loss)/d(beta)
        self.tab = [None] * (len(self.ids) - 1)      # running table-gradient sums
        self.gmax = None                             # pool of zeroed int32 pairs (max |feature gradient| words of the queries)
        self.gmax_used = 0

    def enter(self) -> bool:
        task = _GRAPH_TASK_ID()
        if task != self.task:
            self.reset()
            self.task = task
        return task >= 0           # -1: not inside a backward pass (a Function's backward called by hand): nobody would collect

    def joins(self, ids) -> bool:
        """ids = (id(beta), id(emb_s), id(emb_c) or id(None)) of a query: same beta, same tables (a colourless query: its one)"""
        return self.bound and ids[0] == self.ids[0] and ids[1] == self.ids[1] and (ids[2] == id(None) or ids[2:] == self.ids[2:])

    def gmax_words(self, dev):
        if self.gmax is None or self.gmax_used + 2 > self.gmax.numel():
            self.gmax, self.gmax_used = torch.zeros(64, dtype=torch.int32, device=dev), 0
        w = self.gmax[self.gmax_used:self.gmax_used + 2]
        self.gmax_used += 2
        return w

    def collect(self):
        """-> (raw or None, [table sums or None]) of the running backward pass; the accumulator is empty afterwards"""
        if _GRAPH_TASK_ID is None or self.task != _GRAPH_TASK_ID():
            self.reset()
        out = (self.raw, self.tab)
        self.reset()
        return out


class _PackOperands(torch.autograd.Function):
    """Natural (effective) weights + biases of the nets of one JointPacker -> the kernels' operands, ONCE per step:

        fwd pack  [A fragments | bias packs]         (non-differentiable: the kernels read them)
        bwd pack  [transposed A fragments]           (non-differentiable)
        token     [raw_len] uninitialised carrier    (differentiable)

    Every MLP call of the step takes the token as an input and returns `mh_warp_wgrad`'s raw tile-order gradient
    (dW tiles | db tiles) as the token's gradient; autograd sums the calls' contributions (ONE add of one flat tensor per
    extra call instead of one per parameter per call) and this Function's backward maps the sum to the natural layout
    with one gather.  `zero_bias0`: the first-layer bias of the warp nets reaches its parameter through the per-frame
    bias0 (model.warp), so its slot in the raw gradient is dropped here."""

    @staticmethod
    def forward(ctx, jp, zero_bias0, b3, n_w, acc, notify, *params):
        ctx.set_materialize_grads(False)      # unused outputs hand backward None, not a zero-filled tensor (one launch each)
        ctx.notify = notify                   # callables run when this node's backward runs (model: the step cache went stale)
        # behind the n_w weights / biases: the tensors whose gradients the queries sum in `acc` (field nets: beta, the hash tables)
        params, extras = params[:n_w], params[n_w:]
        ctx.acc, ctx.n_extra = acc, len(extras)
        require_gpu(*params)
        weights, biases, o = [], [], 0
        for pk in jp.packers:
            weights.append([p.detach() for p in params[o:o + len(pk.specs)]])
            o += len(pk.specs)
        for pk in jp.packers:
            biases.append([p.detach() for p in params[o:o + len(pk.specs)]])
            o += len(pk.specs)
        assert o == len(params) == n_w
        flat = jp.flat(weights, biases)
        m = jp.on(flat.device)
        if b3:       # the four operand gathers as one (packing.JointPacker.all_index): sections are views of one buffer
            sect = jp.all_index()[1]
            gathered = flat[m["all"]]
            take = lambda k: gathered[sect[k][0]:sect[k][0] + sect[k][1]]
            fpack, bpack = take("fwd"), take("bwd")
        else:
            fpack, bpack = flat[m["fwd"]], flat[m["bwd"]]
        if b3:
            # bf16x3 forward fragments (csrc/mlp_b3.hip): the same weights gathered in the 32x32x16 fragment order, then cut
            # into [hi | mid | lo] bf16 planes per layer by one launch
            w3 = torch.zeros((jp.fwd3_total_f4 + jp.bwd3_total_f4) * 4, device=flat.device)
            for key, layers, base in (("fwd3", jp.b3_layers, 0), ("bwd3", jp.b3T_layers, jp.fwd3_total_f4)):
                if key == "bwd3" and not jp.sliced_bwd_for(b3):
                    continue
                src = take(key)
                so, sp = _i32arr([l[0] for l in layers])
                no, np_ = _i32arr([l[1] for l in layers])
                do, dp = _i32arr([l[2] + base for l in layers])
                launch("mh_b3_slice", ptr(src), ptr(w3), len(layers), sp, np_, dp)
        else:
            w3 = fpack.new_empty(0)
        token = fpack.new_empty(jp.raw_len)
        ctx.jp, ctx.zero_bias0 = jp, zero_bias0
        ctx.mark_non_differentiable(fpack, bpack, w3)
        return fpack, bpack, w3, token

    @staticmethod
    def backward(ctx, _gf, _gb, _g3, g_token):
        for f in ctx.notify:
            f()
        n = ctx.jp.raw_len
        raw, tabs = ctx.acc.collect() if ctx.acc is not None else (None, [])
        g_extra = [None] * ctx.n_extra
        if raw is not None:                   # the joined queries' sum: [weights, biases | d beta]
            g_token = raw[:n] if g_token is None else g_token + raw[:n]
            g_extra = [raw[n].reshape(())] + list(tabs)
        if g_token is None:
            return (None,) * (6 + sum(2 * len(pk.specs) for pk in ctx.jp.packers)) + tuple(g_extra)
        nat_w, nat_b = ctx.jp.unpack_grads(g_token, zero_bias0=ctx.zero_bias0)
        flat = [g for net in nat_w for g in net] + [g for net in nat_b for g in net]
        return (None, None, None, None, None, None, *flat, *g_extra)


class MLPOperands:
    """Prepared operands of the warp nets (deform_net + topo_net) or of the field nets (sdf_net + color_net)."""

    def __init__(self, jp, fpack, bpack, w3, token, mode="", acc=None, notify=None):
        self.jp, self.fpack, self.bpack, self.token = jp, fpack, bpack, token
        self.notify = notify                               # list the pack node calls through when its backward runs
        self.acc = acc                                     # running gradient sums of the queries that share these operands
        self.mode = mode if w3.numel() else ""             # "b3": the sliced kernels the operands are cut for
        # slices per net (float32 storage, 4 floats per float4 unit), or None when the fp32-MFMA kernels serve
        self.w3 = [w3[4 * o:4 * (o + n)] for o, n in jp.w3] if w3.numel() else None
        self.wT3 = [w3[4 * (jp.fwd3_total_f4 + o):4 * (jp.fwd3_total_f4 + o + n)] for o, n in jp.wT3] if w3.numel() else None
        self.w = [jp.take(fpack, sl) for sl in jp.w]
        self.b = [jp.take(fpack, sl) for sl in jp.b]
        self.wT = [jp.take(bpack, sl) for sl in jp.wT]


def prepare_warp_operands(params_d: Sequence[torch.Tensor], params_t: Sequence[torch.Tensor], mode: Optional[str] = None) -> MLPOperands:
    """params_{d,t}: W0x [128,39], W1..W4 [128,128], W5 [n_out,128], b0 (its gradient travels through bias0), b1..b5.
    mode: the arithmetic the pack is cut for ("b3" / "f32"; None = the process default)."""
    jp = warp_joint_packer()
    flat = list(params_d[:6]) + list(params_t[:6]) + list(params_d[6:]) + list(params_t[6:])
    mode = _warp_mode(mode)
    notify = []
    return MLPOperands(jp, *_PackOperands.apply(jp, True, mode, len(flat), None, notify, *flat), mode=mode, notify=notify)


def prepare_field_operands(params: Sequence[torch.Tensor], mode: Optional[str] = None, beta=None, tables=()) -> MLPOperands:
    """params: Ws0 [64,73], Ws1, Ws2 [33,64], Wc0, Wc1, Wc2 [3,64], bs0, bs1, bs2, bc0, bc1, bc2 (natural, effective).
    beta (0-dim) and tables (the sdf and the colour hash table): when given, the field queries that are handed THESE tensors sum
    their beta / table / weight gradients in place and the pack hands the sums over once (_QueryAccumulator)."""
    jp = field_joint_packer()
    mode = _warp_mode(mode)    # the field FORWARD follows the mode; the fused backward picks its pack per pass (_field_wT)
    notify = []
    if beta is None:
        return MLPOperands(jp, *_PackOperands.apply(jp, False, mode, len(params), None, notify, *params), mode=mode, notify=notify)
    if len(tables) != 2:
        raise ValueError("prepare_field_operands: tables = (sdf table, colour table)")
    acc = _QueryAccumulator(beta, tables)
    return MLPOperands(jp, *_PackOperands.apply(jp, False, mode, len(params), acc, notify, *params, beta, *tables), mode=mode, acc=acc,
                       notify=notify)


class _WarpMLP(torch.autograd.Function):
    """deform_net + topo_net on [freq(x), per-slot code bias]  (model.py:412-437).

    bias0_{d,t} [n_slots,128] = code_slot @ W0[:,39:].T + b0, built by the caller in torch so that autograd carries the
    gradient on to the deform code, W0's code columns and b0.  `token` / `opnd`: see _PackOperands / MLPOperands.
    """

    @staticmethod
    def forward(ctx, x, slot, bias0_d, bias0_t, token, n_bands, opnd, slots_are_identity=False, elide=False):
        ctx.set_materialize_grads(False)      # unused outputs hand backward None, not a zero-filled tensor (one launch each)
        require_gpu(x, bias0_d, bias0_t)
        lib = _lib.load()
        bd, bt = opnd.b
        x = x.detach().contiguous().float()
        M, dev = x.shape[0], x.device
        need_grad = any(ctx.needs_input_grad)
        acts = _scratch(lib.mh_warp_acts_floats(M), dev) if need_grad else None
        deform, topo = torch.empty(M, 3, device=dev), torch.empty(M, 2, device=dev)
        b0d, b0t = bias0_d.detach().contiguous(), bias0_t.detach().contiguous()
        slot_c = None if slot is None else slot.contiguous()
        # Eliding (include/morpheus_hip.h): decided ONCE, here, and carried to the backward, which asks no switch again -- whoever
        # wrote the scratch without its all-zero lines is bound to read it by the words.  Several slots: the backward reads dPre0's
        # rows straight out of the scratch (per_pt_d / per_pt_t), so such a call elides nothing.
        level = 0
        if elide and need_grad and opnd.w3 is not None and opnd.wT3 is not None and bias0_d.shape[0] == 1:
            level = lib.mh_warp_elides(M)
        ctx.elided, ctx.elided_fwd = level >= 1, level >= 2
        ctx.b3, ctx.mode = opnd.w3 is not None, opnd.mode         # (the sliced packs w3 / wT3 are cut together)
        wd, wt = opnd.w3 if ctx.b3 else opnd.w
        wdT, wtT = opnd.wT3 if ctx.b3 else opnd.wT
        _timed("mh_warp_fwd", ptr(x), ptr(slot_c), ptr(b0d), ptr(b0t), ptr(wd), ptr(wt), ptr(bd), ptr(bt), n_bands, ptr(deform),
               ptr(topo), ptr(acts), M, _ARITH[ctx.b3], int(ctx.elided_fwd))
        ctx.save_for_backward(x, slot_c, wdT, wtT, acts)
        ctx.n_bands, ctx.n_slots, ctx.jp = n_bands, bias0_d.shape[0], opnd.jp
        # the caller SAYS when slot[i] == i (model._slots' one-slot-per-sample case); n_slots == M alone does not imply it
        # (B frames == M samples, or torch.unique's sorted inverse)
        ctx.identity = bool(slots_are_identity) and bias0_d.shape[0] == M
        return deform, topo

    @staticmethod
    def backward(ctx, g_deform, g_topo):
        lib = _lib.load()
        x, slot, wdT, wtT, acts = ctx.saved_tensors
        M, dev = x.shape[0], x.device
        n_tiles = lib.mh_mlp_tiles(M)
        dpre = _scratch(lib.mh_warp_dpre_floats(M), dev)
        g_x = torch.empty(M, 3, device=dev) if ctx.needs_input_grad[0] else None   # NULL -> the kernel skips the W0^T stage
        c = lambda t: None if t is None else t.contiguous()
        gd, gt = c(g_deform), c(g_topo)
        # b3, large batches: dPre4 (16 KB of a tile's 172) is not parked, the layer-4 weight-gradient launches make it again from
        # the incoming gradient, the ReLU sign words and the T5 slices -- the same bits (include/morpheus_hip.h: mh_warp_bwd_data)
        regen = bool(ctx.b3 and REGEN_DPRE4 and lib.mh_warp_regen_dpre4(M))
        _timed("mh_warp_bwd_data", ptr(x), ptr(gd), ptr(gt), ptr(wdT), ptr(wtT), ctx.n_bands, ptr(acts), ptr(dpre), ptr(g_x), M,
               _ARITH[ctx.b3], int(regen), int(ctx.elided))
        ws = torch.empty(max(lib.mh_warp_wgrad_workspace_floats(M), 1), device=dev)
        raw_len = ctx.jp.raw_len                                  # == mh_warp_raw_floats(): dW tiles | db tiles, tile-row order
        raw = torch.empty(raw_len, device=dev) if M > 0 else torch.zeros(raw_len, device=dev)      # (an empty call writes nothing)
        b3_only = (ptr(gd), ptr(gt), ptr(wdT), ptr(wtT)) if ctx.b3 else (None,) * 4     # what regenerating dPre4 reads
        _timed("mh_warp_wgrad", ptr(acts), ptr(dpre), *b3_only, _ARITH[ctx.b3], int(regen), int(ctx.elided), ptr(ws), ptr(raw), M,
               key="mh_mlp_wgrad[warp]")
        # per-slot first-layer bias gradient: sum of dPre0 over the points of each slot
        if ctx.n_slots == 1:
            (od, ot) = ctx.jp.bias0_raw
            g_b0d, g_b0t = raw[od:od + 128][None], raw[ot:ot + 128][None]
        else:
            # rows 0:128 and 672:800 of a dPre tile: dPre0 of deform_net and of topo_net (csrc/mlp_dev.h: "warp dpre")
            dp = dpre.view(n_tiles, lib.mh_warp_dpre_floats(1) // (lib.mh_mlp_tiles(1) * 32), 32)
            per_pt_d = dp[:, 0:128, :].permute(0, 2, 1).reshape(-1, 128)[:M]
            per_pt_t = dp[:, 672:800, :].permute(0, 2, 1).reshape(-1, 128)[:M]
            if ctx.identity:              # one slot per sample, slot[i] == i: the per-point rows ARE the answer
                g_b0d, g_b0t = per_pt_d, per_pt_t
            else:
                idx = slot.long()
                g_b0d = torch.zeros(ctx.n_slots, 128, device=dev).index_add_(0, idx, per_pt_d)
                g_b0t = torch.zeros(ctx.n_slots, 128, device=dev).index_add_(0, idx, per_pt_t)
        return (g_x, None, g_b0d, g_b0t, raw, None, None, None, None)


def warp_mlp(x, slot, bias0_d, bias0_t, n_bands, opnd: MLPOperands, slots_are_identity: bool = False, elide: bool = False):
    """slots_are_identity: slot[i] == i for every sample (bias0 rows are per sample): the first-layer bias gradient is then
    the per-point dPre0 rows themselves; any other slot map goes through index_add_.
    elide: the call MAY leave all-zero parked lines unwritten where that pays (b3, one slot, a batch of the per-layer weight-gradient
    path, both switches on: mh_warp_elides) -- same outputs and gradients; without it every line of the scratch is written."""
    return _WarpMLP.apply(x, slot, bias0_d, bias0_t, opnd.token, n_bands, opnd, slots_are_identity, elide)


def _field_fwd(lib, xc, fs, fc, tp, beta_c, n_bands, with_color, opnd, need_grad):
    """-> sdf, sigma, albedo|None, acts|None (parked activations for backward)."""
    b3 = opnd.w3 is not None
    w, b = (opnd.w3 if b3 else opnd.w)[0], opnd.b[0]
    M, dev = xc.shape[0], xc.device
    acts = _scratch(lib.mh_field_acts_floats(M), dev) if need_grad else None
    sdf, sigma = torch.empty(M, device=dev), torch.empty(M, device=dev)
    albedo = torch.empty(M, 3, device=dev) if with_color else None
    _timed("mh_field_fwd", ptr(xc), ptr(fs), ptr(fc), ptr(tp), ptr(w), ptr(b), ptr(beta_c), n_bands, int(bool(with_color)),
           ptr(sdf), ptr(sigma), ptr(albedo), ptr(acts), M, _ARITH[b3])
    return sdf, sigma, albedo, acts


# Arithmetic of the fused field backward in the b3 mode: the bf16 pipe like every other MLP kernel of the mode (arith = MH_ARITH_B3),
# both passes -- colour + sdf (cfg3's: 2.13 -> 1.78 ms) and sdf-only (the finite-difference taps, 12 of every 13 points of a
# training step: virtual-view 72 x 72 2.56 -> 1.88 ms).  Same-box A/Bs: profiles/r04_ab_field_bwd_b3.txt.  The colour + sdf pass
# only won once the weight gradient of the sdf net's geo rows had moved into the colour launch: before, the sliced sdf launch
# spilled 91 registers beside its 192 accumulators and measured equal to the fp32 form.
# MORPHEUS_FIELD_BWD = "f32" keeps the native fp32 MFMA form (what the f32 mode always uses), "sdf" the
# sliced form for the sdf-only pass alone (A/B).
# The colour + sdf pass of "b3" runs the PAIR form of the two launches (two waves per SIMD, csrc/mlp.hip field_pair_*_kernel;
# bit-identical outputs; same-box A/B in profiles/r07_field_bwd_pair.txt).  "b3w1" keeps the one-wave kernels for that pass too
# (A/B, and what the pair form's tests compare with); the sdf-only pass runs the one-wave kernels either way.
FIELD_BWD = os.environ.get("MORPHEUS_FIELD_BWD", "b3")
if FIELD_BWD not in ("b3", "b3w1", "sdf", "f32"):
    raise ValueError(f"MORPHEUS_FIELD_BWD={FIELD_BWD!r}: expected 'b3', 'b3w1', 'sdf' or 'f32'")
_PAIR_NEVER = 1 << 62         # mh_field_bwd_pair_min_points: no call is that large
_pair_min_default = None      # the library's own threshold, read before the first call changes it


def _field_wT(opnd, with_color: bool):
    """-> (transposed weight operand of the fused field backward, is it the bf16x3 pack?)"""
    sliced = FIELD_BWD in ("b3", "b3w1") or (FIELD_BWD == "sdf" and not with_color)
    if sliced and opnd.mode == "b3" and opnd.wT3 is not None:
        return opnd.wT3[0], True
    return opnd.wT[0], False


def _field_bwd(lib, xc, wT, beta_c, acts, sdf, albedo, g_sdf, g_sigma, g_albedo, n_bands, with_color, has_topo, has_fc,
               need_dx, jp, raw_into=None, gmax=None, b3=False):
    """mh_field_bwd_fused: backward-data and weight gradients of the field nets in one pass per net (the pre-activation
    gradients stay on the chip).  raw_into: device ADDRESS of a running [raw_len + 1] sum this call adds its weight / bias /
    beta gradients to (the reduction launch adds instead of writing), or None -> a fresh tensor.  gmax: 2 zeroed int32 words.
    -> g_xc|None, g_fs, g_fc|None, g_tp|None, raw|None (tile-order weight gradient followed by d(loss)/d(beta); None when it
    went into raw_into), gmax (int32[2]: max|g_fs|, max|g_fc| as float bits, reduced on the fly by the kernel for the hash-grid
    backward's fixed point)."""
    M, dev = xc.shape[0], xc.device
    if not with_color:
        g_albedo = None
    g_xc = torch.empty(M, 3, device=dev) if need_dx else None
    g_fs = _scratch(M * 32, dev).view(M, 32)
    g_fc = _scratch(M * 32, dev).view(M, 32) if (with_color and has_fc) else None
    g_tp = torch.empty(M, 2, device=dev) if has_topo else None
    if gmax is None:
        gmax = torch.zeros(2, dtype=torch.int32, device=dev)
    dgeo = _scratch(lib.mh_field_dgeo_floats(M), dev) if with_color else None
    ws = torch.empty(lib.mh_field_bwd_fused_workspace_floats(M), device=dev)
    raw = None
    if raw_into is None:      # an empty query returns MH_OK without writing: the gradient must then be zeros, not heap contents
        raw = torch.empty(jp.raw_len + 1, device=dev) if M > 0 else torch.zeros(jp.raw_len + 1, device=dev)
    c = lambda t: None if t is None else t.contiguous()
    if b3 and with_color:     # the form of the two launches follows FIELD_BWD at call time (a host-side choice, made at the launch)
        global _pair_min_default
        if _pair_min_default is None:
            _pair_min_default = lib.mh_field_bwd_pair_min_points(-1)
        want = _PAIR_NEVER if FIELD_BWD == "b3w1" else _pair_min_default
        if lib.mh_field_bwd_pair_min_points(-1) != want:
            lib.mh_field_bwd_pair_min_points(want)
    _timed("mh_field_bwd_fused", ptr(xc), ptr(sdf), ptr(albedo if with_color else None), ptr(c(g_sdf)), ptr(c(g_sigma)),
           ptr(c(g_albedo)), ptr(wT), ptr(beta_c), n_bands, int(with_color), ptr(acts), ptr(dgeo), ptr(ws),
           ptr(raw) if raw_into is None else ctypes.c_void_p(raw_into), int(raw_into is not None), ptr(g_xc), ptr(g_fs), ptr(g_fc),
           ptr(g_tp), ptr(gmax), M, _ARITH[bool(b3)])
    return g_xc, g_fs, g_fc, g_tp, raw, gmax


class _FieldMLP(torch.autograd.Function):
    """sdf_net (+Laplace density) and color_net on [freq(xc), hash, topo] / [hash_c, geo] with the hash features GIVEN
    (model.py:273-307, density.py:22-31).  The model itself goes through _FieldQuery (hash grids + nets in one node).

    beta: 0-dim device tensor = |beta_param| + 1e-4 (stays on the device: no host sync).  `token` / `opnd`: the
    prepared operands of prepare_field_operands.
    """

    @staticmethod
    def forward(ctx, xc, feat_s, feat_c, topo, beta, token, n_bands, with_color, opnd):
        ctx.set_materialize_grads(False)      # unused outputs hand backward None, not a zero-filled tensor (one launch each)
        require_gpu(xc, feat_s, feat_c, topo, beta)
        lib = _lib.load()
        xc = xc.detach().contiguous().float()
        fs = feat_s.detach().contiguous()
        fc = None if feat_c is None else feat_c.detach().contiguous()
        tp = None if topo is None else topo.detach().contiguous()
        beta_c = beta.detach().reshape(1).contiguous().float()
        sdf, sigma, albedo, acts = _field_fwd(lib, xc, fs, fc, tp, beta_c, n_bands, with_color, opnd, any(ctx.needs_input_grad))
        wT_sel, ctx.bwd_b3 = _field_wT(opnd, bool(with_color))
        ctx.save_for_backward(xc, wT_sel, beta_c, acts, sdf, albedo)
        ctx.cfg = (n_bands, bool(with_color), topo is not None, feat_c is not None)
        ctx.jp = opnd.jp
        if albedo is None:
            albedo = torch.empty(0, device=xc.device)        # (an empty allocation: no fill is dispatched)
            ctx.mark_non_differentiable(albedo)
        return sdf, sigma, albedo

    @staticmethod
    def backward(ctx, g_sdf, g_sigma, g_albedo):
        lib = _lib.load()
        xc, wT, beta_c, acts, sdf, albedo = ctx.saved_tensors
        n_bands, with_color, has_topo, has_fc = ctx.cfg
        g_xc, g_fs, g_fc, g_tp, raw, _ = _field_bwd(lib, xc, wT, beta_c, acts, sdf, albedo, g_sdf, g_sigma, g_albedo,
                                                    n_bands, with_color, has_topo, has_fc, ctx.needs_input_grad[0], ctx.jp,
                                                    b3=ctx.bwd_b3)
        n = ctx.jp.raw_len
        return (g_xc, g_fs, g_fc, g_tp, raw[n].reshape(()), raw[:n], None, None, None)


def field_mlp(xc, feat_s, feat_c, topo, beta, n_bands, with_color, opnd: MLPOperands):
    """-> sdf [M], sigma [M], albedo [M,3] (empty when with_color is False)."""
    return _FieldMLP.apply(xc, feat_s, feat_c, topo, beta, opnd.token, n_bands, with_color, opnd)


class _FieldQuery(torch.autograd.Function):
    """get_sigma_albedo (model.py:273-307) as ONE autograd node: hash-grid encode of the sdf (and colour) table at xc ->
    sdf_net + Laplace density (+ color_net).  Backward runs the field backward, then the brick backward of the tables with
    max|feature gradient| handed over directly (the field backward-data kernel reduces it on the fly; the brick kernel's
    fixed-point accumulation needs it) -- the features and their gradients never surface as autograd tensors."""

    @staticmethod
    def forward(ctx, xc, topo, beta, token, emb_s, emb_c, offsets_np, res_np, n_levels, bound, group, n_bands, opnd):
        ctx.set_materialize_grads(False)      # unused outputs hand backward None, not a zero-filled tensor (one launch each)
        with_color = emb_c is not None
        require_gpu(xc, topo, beta, emb_s, emb_c)
        lib = _lib.load()
        xc = xc.detach().contiguous().float()
        L = len(res_np)
        o_np, o_p = _i32arr(offsets_np)
        r_np, r_p = _i32arr(res_np)
        embs = [emb_s.detach().contiguous()] + ([emb_c.detach().contiguous()] if with_color else [])
        feats, ctx.binned = _grid_fwd(lib, xc, embs, o_p, r_p, L, n_levels, bound, group)
        tp = None if topo is None else topo.detach().contiguous()
        beta_c = beta.detach().reshape(1).contiguous().float()
        sdf, sigma, albedo, acts = _field_fwd(lib, xc, feats[0], feats[1] if with_color else None, tp, beta_c, n_bands,
                                              with_color, opnd, any(ctx.needs_input_grad))
        wT_sel, ctx.bwd_b3 = _field_wT(opnd, bool(with_color))
        ctx.save_for_backward(xc, wT_sel, beta_c, acts, sdf, albedo, *embs)
        ctx.cfg = (n_bands, with_color, topo is not None, o_np, r_np, n_levels, float(bound), L)
        ctx.jp, ctx.acc = opnd.jp, opnd.acc
        ctx.ids = (id(beta), id(emb_s), id(emb_c))       # identities of the shared inputs (see _QueryAccumulator.joins)
        if albedo is None:
            albedo = torch.empty(0, device=xc.device)        # (an empty allocation: no fill is dispatched)
            ctx.mark_non_differentiable(albedo)
        return sdf, sigma, albedo

    @staticmethod
    def backward(ctx, g_sdf, g_sigma, g_albedo):
        lib = _lib.load()
        xc, wT, beta_c, acts, sdf, albedo, *embs = ctx.saved_tensors
        n_bands, with_color, has_topo, o_np, r_np, n_levels, bound, L = ctx.cfg
        need_dx = ctx.needs_input_grad[0]
        acc, n = ctx.acc, ctx.jp.raw_len
        # joined: this query's weight / beta / table gradients go into the pass's running sums (handed over by _PackOperands.backward)
        joined = (ACCUMULATE_IN_PLACE and acc is not None and xc.shape[0] > 0 and ctx.needs_input_grad[3] and acc.joins(ctx.ids)
                  and acc.enter())
        g_xc, g_fs, g_fc, g_tp, raw, gmax = _field_bwd(
            lib, xc, wT, beta_c, acts, sdf, albedo, g_sdf, g_sigma, g_albedo, n_bands, with_color, has_topo, with_color, need_dx, ctx.jp,
            raw_into=acc.raw.data_ptr() if joined and acc.raw is not None else None, gmax=acc.gmax_words(xc.device) if joined else None,
            b3=ctx.bwd_b3)
        o_p, r_p = o_np.ctypes.data_as(ctypes.c_void_p), r_np.ctypes.data_as(ctypes.c_void_p)
        grads = [g_fs] + ([g_fc] if with_color else [])
        gptrs = [gmax.data_ptr(), gmax.data_ptr() + 4][:len(grads)]
        sums = [acc.tab[k].data_ptr() if acc.tab[k] is not None else None for k in range(len(grads))] if joined else None
        g_x, g_embs = _grid_bwd(lib, xc, embs, grads, o_p, r_p, L, n_levels, bound, need_dx, gptrs, sums=sums, g_x_into=g_xc,
                                binned=ctx.binned)
        if joined:
            if raw is not None:
                acc.raw = raw
            for k, g in enumerate(g_embs):
                if g is not None:
                    acc.tab[k] = g
            return (g_x, g_tp) + (None,) * 11
        return (g_x, g_tp, raw[n].reshape(()), raw[:n], g_embs[0], g_embs[1] if with_color else None, None, None, None, None, None, None, None)


def field_query(xc, topo, beta, emb_s, emb_c, offsets_np, res_np, bound, max_level, group, n_bands, opnd: MLPOperands):
    """-> sdf [M], sigma [M], albedo [M,3] (empty when emb_c is None: the sdf-only pass of the finite-difference taps)."""
    n_levels = effective_levels(max_level, len(res_np))
    return _FieldQuery.apply(xc, topo, beta, opnd.token, emb_s, emb_c, offsets_np, res_np, n_levels, float(bound), int(group),
                             n_bands, opnd)


class _WeightNormAll(torch.autograd.Function):
    """W_l = g_l * v_l / ||v_l||_row for a list of weight-normed layers (decoders.py:51-52), one launch forward and one
    backward (csrc/wnorm.hip) instead of norm / divide / multiply and their autograd graph per layer."""

    @staticmethod
    def forward(ctx, n, *vg):
        ctx.set_materialize_grads(False)      # unused outputs hand backward None, not a zero-filled tensor (one launch each)
        vs, gs = vg[:n], vg[n:]
        require_gpu(*vg)
        vs_c = [v.detach().contiguous() for v in vs]
        gs_c = [g.detach().contiguous() for g in gs]
        ws = [torch.empty_like(v) for v in vs_c]
        PA, IA = ctypes.c_void_p * n, ctypes.c_int32 * n
        rows, cols = IA(*[v.shape[0] for v in vs_c]), IA(*[v.shape[1] for v in vs_c])
        launch("mh_weight_norm_fwd", n, PA(*[ptr(v) for v in vs_c]), PA(*[ptr(g) for g in gs_c]), PA(*[ptr(w) for w in ws]), rows,
               cols)
        ctx.save_for_backward(*vs_c, *gs_c)
        ctx.n = n
        return tuple(ws)

    @staticmethod
    def backward(ctx, *gw):
        n = ctx.n
        saved = ctx.saved_tensors
        vs, gs = saved[:n], saved[n:]
        gw_c = [None if g is None else g.contiguous() for g in gw]
        dvs = [torch.empty_like(v) for v in vs]
        dgs = [torch.empty_like(g) for g in gs]
        PA, IA = ctypes.c_void_p * n, ctypes.c_int32 * n
        rows, cols = IA(*[v.shape[0] for v in vs]), IA(*[v.shape[1] for v in vs])
        launch("mh_weight_norm_bwd", n, PA(*[ptr(v) for v in vs]), PA(*[ptr(g) for g in gs]), PA(*[ptr(g) for g in gw_c]),
               PA(*[ptr(t) for t in dvs]), PA(*[ptr(t) for t in dgs]), rows, cols)
        return (None, *dvs, *dgs)


def weight_norm_all(vs: Sequence[torch.Tensor], gs: Sequence[torch.Tensor]):
    """Effective weights of weight-normed layers: vs[l] [out,in], gs[l] [out,1] -> list of [out,in]."""
    assert len(vs) == len(gs) and all(v.dim() == 2 for v in vs)
    return list(_WeightNormAll.apply(len(vs), *vs, *gs))


# ------------------------------------------------------------------------------------------ caller-side glue, one launch each
MEAN_KINDS = {"identity": 0, "square": 1, "abs": 2, "entropy": 3, "eikonal": 4, "absdiff": 5, "sqdiff": 6}


class _MaskedMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, a, b, w_row, n_valid):
        ctx.set_materialize_grads(False)
        require_gpu(a, b, w_row, n_valid)
        lib = _lib.load()
        a_c = a.detach().contiguous().float()
        b_c = None if b is None else b.detach().contiguous().float()
        assert a_c.dim() >= 1 and (b_c is None or b_c.shape == a_c.shape)
        M = a_c.shape[0]
        C = max(math.prod(a_c.shape[1:]), 1)          # from the trailing shape: an empty [0, 3] tensor still has C = 3
        w_c = None if w_row is None else w_row.detach().reshape(-1).contiguous().float()
        assert w_c is None or w_c.numel() == M
        nv = None if n_valid is None else n_valid.detach().reshape(1).to(torch.int32).contiguous()
        ws = torch.empty(lib.mh_masked_mean_workspace_floats(), device=a_c.device)
        out = torch.empty(2, device=a_c.device)
        launch("mh_masked_mean_fwd", kind, ptr(a_c), ptr(b_c), ptr(w_c), M, C, ptr(nv), ptr(ws), ptr(out))
        ctx.save_for_backward(a_c, b_c, w_c, nv, out)
        ctx.kind, ctx.shape = kind, a.shape
        return out[0]

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None, None
        a_c, b_c, w_c, nv, out = ctx.saved_tensors
        M = a_c.shape[0]
        C = max(math.prod(a_c.shape[1:]), 1)
        want_a, want_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2] and b_c is not None
        g_a = torch.empty_like(a_c) if want_a else None
        g_b = torch.empty_like(b_c) if want_b else None
        if (want_a or want_b) and a_c.numel():        # (an empty gradient has no address to hand over: nothing to launch)
            launch("mh_masked_mean_bwd", ctx.kind, ptr(a_c), ptr(b_c), ptr(w_c), M, C, ptr(nv), ptr(out),
                   ptr(g.reshape(1).contiguous().float()), ptr(g_a), ptr(g_b))
        return None, g_a, g_b, None, None


def masked_mean(kind: str, a, b=None, *, n_valid=None, row_weight=None):
    """Mean over the samples of f(a[, b]) for a per-sample tensor [M, ...] (include/morpheus_hip.h: mh_masked_mean_*): the
    reference's `f(a).mean()` when every row counts; with n_valid (0-dim device int tensor, fixed-capacity sampling) the rows behind
    it are left out; with row_weight [M] the value is sum(f * w) / max(per_row * sum(w), 1) (morpheus.py:556).  kind: see
    MEAN_KINDS ("eikonal": a is [M,3], f = (|row| - 1)^2; "absdiff" / "sqdiff": f(a - b))."""
    return _MaskedMean.apply(MEAN_KINDS[kind], a, b, row_weight, n_valid)


class _OrthoPerturb(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, normals, phi, scale):
        ctx.set_materialize_grads(False)
        require_gpu(x, normals, phi)
        x_c, n_c = x.detach().contiguous().float(), normals.detach().contiguous().float()
        p_c = phi.detach().reshape(-1).contiguous().float()
        M = x_c.shape[0]
        assert x_c.shape == (M, 3) and n_c.shape == (M, 3) and p_c.numel() == M
        out = torch.empty_like(x_c)
        launch("mh_ortho_perturb_fwd", ptr(x_c), ptr(n_c), ptr(p_c), float(scale), M, ptr(out))
        ctx.save_for_backward(n_c, p_c)
        ctx.scale = float(scale)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        n_c, p_c = ctx.saved_tensors
        g_n = None
        if ctx.needs_input_grad[1]:
            g_c = g.contiguous().float()
            g_n = torch.empty_like(n_c)
            launch("mh_ortho_perturb_bwd", ptr(n_c), ptr(p_c), ptr(g_c), ctx.scale, n_c.shape[0], ptr(g_n))
        return (g if ctx.needs_input_grad[0] else None), g_n, None, None


def ortho_perturb(x, normals, phi, scale: float):
    """x + scale * get_ortho_normal_dir(normals)  (morpheus.py:518-528 applied at :549 / :766) in one launch; phi [M] or [M,1] is the
    caller's uniform draw times 2 pi.  Gradients reach x (identity) and the normals."""
    return _OrthoPerturb.apply(x, normals, phi, scale)


class _SmoothPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, off, rays_o, rays_d):
        ctx.set_materialize_grads(False)
        require_gpu(depth, off, rays_o, rays_d)
        d_c, f_c = depth.detach().reshape(-1).contiguous().float(), off.detach().reshape(-1).contiguous().float()
        o_c, r_c = rays_o.detach().contiguous().float(), rays_d.detach().contiguous().float()
        N, K = d_c.shape[0], f_c.shape[0]
        assert o_c.shape == (N, 3) and r_c.shape == (N, 3)
        pts, keep = torch.empty(K * N, 3, device=d_c.device), torch.empty(K * N, device=d_c.device)
        launch("mh_smooth_points_fwd", ptr(d_c), ptr(f_c), ptr(o_c), ptr(r_c), N, K, ptr(pts), ptr(keep))
        ctx.save_for_backward(d_c, f_c, r_c)
        ctx.depth_shape = depth.shape
        ctx.mark_non_differentiable(keep)
        return pts, keep

    @staticmethod
    def backward(ctx, g, _gk):
        if g is None:
            return None, None, None, None
        d_c, f_c, r_c = ctx.saved_tensors
        N, K = d_c.shape[0], f_c.shape[0]
        need_depth, _, need_o, need_d = ctx.needs_input_grad
        g_depth = torch.empty(N, device=g.device) if need_depth else None
        g_o = torch.empty(N, 3, device=g.device) if need_o else None
        g_d = torch.empty(N, 3, device=g.device) if need_d else None
        if need_depth or need_o or need_d:
            launch("mh_smooth_points_bwd", ptr(g.contiguous().float()), ptr(d_c), ptr(f_c), ptr(r_c), N, K, ptr(g_depth), ptr(g_o),
                   ptr(g_d))
        return (None if g_depth is None else g_depth.view(ctx.depth_shape)), None, g_o, g_d


def smooth_points(depth, off, rays_o, rays_d):
    """-> pts [K*N,3] = (depth[n] + off[k]) * rays_d[n] + rays_o[n] (point k*N + n), keep [K*N] = (|pts| < 1.1) as 0 / 1: the points
    of get_normal_smoothness_loss (morpheus.py:530-547) in one launch each way; gradients to depth, rays_o, rays_d."""
    return _SmoothPoints.apply(depth, off, rays_o, rays_d)


class _BgBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, opacity, bg):
        ctx.set_materialize_grads(False)
        require_gpu(color, opacity, bg)
        c_c, o_c, b_c = color.detach().contiguous().float(), opacity.detach().reshape(-1).contiguous().float(), bg.detach().contiguous().float()
        N = c_c.shape[0]
        assert c_c.shape == (N, 3) and b_c.shape == (N, 3) and o_c.shape[0] == N
        image = torch.empty_like(c_c)
        launch("mh_bg_blend_fwd", ptr(c_c), ptr(o_c), ptr(b_c), N, ptr(image))
        ctx.save_for_backward(o_c, b_c)
        ctx.opacity_shape = opacity.shape
        return image

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None
        o_c, b_c = ctx.saved_tensors
        N = o_c.shape[0]
        need_c, need_o, need_b = ctx.needs_input_grad
        g_c = g.contiguous().float()
        g_o = torch.empty(N, device=g.device) if need_o else None
        g_b = torch.empty(N, 3, device=g.device) if need_b else None
        if need_o or need_b:
            launch("mh_bg_blend_bwd", ptr(g_c), ptr(o_c), ptr(b_c), N, ptr(g_o), ptr(g_b))
        return (g_c if need_c else None), (None if g_o is None else g_o.view(ctx.opacity_shape)), g_b


def bg_blend(color, opacity, bg):
    """color + (1 - opacity) * bg for a per-ray background [N,3] (morpheus.py:686-694) in one launch each way, the chain's rounding."""
    return _BgBlend.apply(color, opacity, bg)


class _PoseApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rays_o, rays_d, pose, frame_of_row, n_per_row):
        ctx.set_materialize_grads(False)
        require_gpu(rays_o, rays_d, pose, frame_of_row)
        o_c, d_c = rays_o.detach().contiguous().float(), rays_d.detach().contiguous().float()
        p_c = pose.detach().contiguous().float()
        f_c = frame_of_row.detach().reshape(-1).long().contiguous()
        B = f_c.numel()
        assert o_c.shape == (B * n_per_row, 3) and d_c.shape == o_c.shape and p_c.dim() == 2 and p_c.shape[1] == 6
        o_out, d_out = torch.empty_like(o_c), torch.empty_like(d_c)
        launch("mh_pose_apply_fwd", ptr(o_c), ptr(d_c), ptr(p_c), ptr(f_c), B, n_per_row, ptr(o_out), ptr(d_out))
        ctx.save_for_backward(d_c, p_c, f_c)
        ctx.n_per_row = n_per_row
        return o_out, d_out

    @staticmethod
    def backward(ctx, g_o, g_d):
        d_c, p_c, f_c = ctx.saved_tensors
        if (g_o is None and g_d is None) or not ctx.needs_input_grad[2]:
            return None, None, None, None, None
        lib = _lib.load()
        B = f_c.numel()
        g_o = None if g_o is None else g_o.contiguous().float()
        g_d = None if g_d is None else g_d.contiguous().float()
        ws = torch.empty(max(lib.mh_pose_bwd_workspace_floats(B, ctx.n_per_row), 1), device=d_c.device)
        g_pose = torch.empty_like(p_c)
        launch("mh_pose_apply_bwd", ptr(d_c), ptr(p_c), ptr(f_c), B, ctx.n_per_row, p_c.shape[0], ptr(g_o), ptr(g_d), ptr(ws),
               ptr(g_pose))
        return None, None, g_pose, None, None


def pose_apply(rays_o, rays_d, pose, frame_of_row, n_per_row: int):
    """(rays_o + t_f, R_f rays_d) for a batch of B rows of n_per_row rays, one frame per row (include/morpheus_hip.h:
    mh_pose_apply_*; models/pose.py:4-64 + model.py:335-346): pose [n_frames, 6], frame_of_row [B] frame ids.  The rays are data
    (no gradient); the gradient reaches `pose`."""
    return _PoseApply.apply(rays_o, rays_d, pose, frame_of_row, int(n_per_row))


class _RenderLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred_rgb, pred_depth, opacity, image, depth, mask, bg, rays_o, rays_d, w_rgb, w_mask, w_depth):
        ctx.set_materialize_grads(False)
        require_gpu(pred_rgb, pred_depth, opacity, image, depth, mask, bg, rays_o, rays_d)
        c = lambda t, *shape: t.detach().reshape(*shape).contiguous().float()
        N = pred_depth.numel()
        pr, pd, op = c(pred_rgb, N, 3), c(pred_depth, N), c(opacity, N)
        im, dp, mk, bgc = c(image, 3, N), c(depth, N), c(mask, N), c(bg, N, 3)
        ro, rd = c(rays_o, N, 3), c(rays_d, N, 3)
        gt_rgb, valid, out = torch.empty(3, N, device=pr.device), torch.empty(N, device=pr.device), torch.empty(4, device=pr.device)
        launch("mh_render_loss_fwd", ptr(pr), ptr(pd), ptr(op), ptr(im), ptr(dp), ptr(mk), ptr(bgc), ptr(ro), ptr(rd), N, w_rgb,
               w_mask, w_depth, ptr(gt_rgb), ptr(valid), ptr(out))
        ctx.save_for_backward(pr, pd, op, gt_rgb, dp, mk, valid)
        ctx.w = (float(w_rgb), float(w_mask), float(w_depth))
        ctx.shapes = (pred_rgb.shape, pred_depth.shape, opacity.shape)
        terms = out[1:]
        ctx.mark_non_differentiable(terms, gt_rgb, valid)     # the three terms are VALUES for logging: the gradient travels through out[0] only
        return out[0], terms, gt_rgb, valid

    @staticmethod
    def backward(ctx, g, _g_terms, _g_gt, _g_valid):
        if g is None:
            return (None,) * 12
        pr, pd, op, gt_rgb, dp, mk, valid = ctx.saved_tensors
        N = pd.numel()
        need = ctx.needs_input_grad
        g_rgb = torch.empty_like(pr) if need[0] else None
        g_dep = torch.empty_like(pd) if need[1] else None
        g_op = torch.empty_like(op) if need[2] else None
        if need[0] or need[1] or need[2]:
            launch("mh_render_loss_bwd", ptr(pr), ptr(pd), ptr(op), ptr(gt_rgb), ptr(dp), ptr(mk), ptr(valid), N, *ctx.w,
                   ptr(g.reshape(1).contiguous().float()), ptr(g_rgb), ptr(g_dep), ptr(g_op))
        s = ctx.shapes
        return (None if g_rgb is None else g_rgb.view(s[0]), None if g_dep is None else g_dep.view(s[1]),
                None if g_op is None else g_op.view(s[2]), None, None, None, None, None, None, None, None, None)


def real_view_render_loss(pred_rgb, pred_depth, opacity, image, depth, mask, bg, rays_o, rays_d, w_rgb, w_mask, w_depth):
    """get_gt_from_data + get_real_view_render_loss (morpheus.py:930-983) in one launch each way (include/morpheus_hip.h:
    mh_render_loss_*).  pred_rgb [..., 3] per ray (the renderer's `image`), pred_depth / opacity per ray; image: the dataset's
    [B,3,H,W] batch (B = 1: channel-major [3,N]); bg [N,3].  -> (weighted loss, the three terms [rgb, mask, depth] (detached
    values), gt_rgb [3,N], valid-depth mask [N])."""
    return _RenderLoss.apply(pred_rgb, pred_depth, opacity, image, depth, mask, bg, rays_o, rays_d, float(w_rgb), float(w_mask),
                             float(w_depth))


class _WeightedSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, *terms):
        ctx.set_materialize_grads(False)
        stacked = torch.stack([t.detach().reshape(()) for t in terms])
        ctx.save_for_backward(weights)
        ctx.n = len(terms)
        return (stacked * weights).sum()

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * (ctx.n + 1)
        (weights,) = ctx.saved_tensors
        gs = (weights * g).unbind(0)
        return (None, *[gs[k] if ctx.needs_input_grad[k + 1] else None for k in range(ctx.n)])


_WEIGHT_CACHE: dict = {}


def weighted_sum(pairs):
    """sum_k w_k * term_k for 0-dim device tensors term_k and host floats w_k: three launches forward (stack, multiply, add) and
    one backward, whatever the number of terms -- the reference's `loss = loss + w * term` chains (morpheus.py:946-1145) cost two
    launches per term each way.  The weight vector is built once per distinct tuple of weights (no host->device copy per step:
    that would be a sync in the eager step and illegal inside a captured graph)."""
    pairs = [(float(w), t) for w, t in pairs]
    if not pairs:
        return 0
    dev = pairs[0][1].device
    key = (tuple(w for w, _ in pairs), str(dev))
    wt = _WEIGHT_CACHE.get(key)
    if wt is None:
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("weighted_sum: a new set of loss weights inside a captured graph (run the step once eagerly first)")
        if len(_WEIGHT_CACHE) >= 64:        # weights that change every step do not belong here (multiply the term instead)
            _WEIGHT_CACHE.clear()
        wt = _WEIGHT_CACHE[key] = torch.tensor(key[0], dtype=torch.float32, device=dev)
    return _WeightedSum.apply(wt, *[t for _, t in pairs])


# ------------------------------------------------------------------------------------ frequency / spherical-harmonics encoders
def _encoder_rows(x, D: Optional[int], what: str):
    """the [B, D] fp32 contiguous rows of a device tensor (any dtype an autocast caller may hand over); D None: any width"""
    require_gpu(x)
    if x.dim() != 2 or (D is not None and x.shape[1] != D):
        raise _lib.MorpheusHipError(f"{what}: expected [B, {'D' if D is None else D}] rows, got {tuple(x.shape)}")
    return x.detach().contiguous().float()


class _FreqEncode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, degree, n_keep):
        ctx.set_materialize_grads(False)
        x_c = _encoder_rows(x, None, "freq_encode")
        B, D = x_c.shape
        out = torch.empty(B, D + 2 * D * degree, device=x_c.device)
        _timed("mh_freq_encode_fwd", ptr(x_c), B, D, degree, n_keep, ptr(out))
        ctx.save_for_backward(x_c)              # the forward's output is not an operand of the backward
        ctx.args = (degree, n_keep, x.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None
        (x_c,) = ctx.saved_tensors
        degree, n_keep, dtype = ctx.args
        B, D = x_c.shape
        g_x = torch.empty_like(x_c)
        _timed("mh_freq_encode_bwd", ptr(x_c), ptr(g.contiguous().float()), B, D, degree, n_keep, ptr(g_x))
        return g_x.to(dtype), None, None


def freq_encode(x, degree: int, n_keep: Optional[int] = None):
    """x [B, D] (1 <= D <= 8) -> [B, D + 2 D degree] fp32: x, then per band f < degree a block of D sines and a block of D cosines of
    2^f x (freqencoder.cu:28-58); the blocks of the bands f >= n_keep (default: degree) are zero, as FreqEncoder_torch's max_level
    leaves them (encodings.py:35-57).  One launch each way; the backward recomputes sine and cosine from x and runs only when x
    needs a gradient.  Under autocast: fp32 in, fp32 out (the reference's custom_fwd(cast_inputs=torch.float32))."""
    degree = int(degree)
    n_keep = degree if n_keep is None else int(n_keep)
    return _FreqEncode.apply(x, degree, n_keep)


class _SHEncode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, degree):
        ctx.set_materialize_grads(False)
        x_c = _encoder_rows(x, 3, "sh_encode")
        B = x_c.shape[0]
        out = torch.empty(B, degree * degree, device=x_c.device)
        _timed("mh_sh_encode_fwd", ptr(x_c), B, degree, ptr(out))
        ctx.save_for_backward(x_c)              # no dy_dx [B, 3 degree^2] is kept: the backward evaluates the derivative polynomials
        ctx.args = (degree, x.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None or not ctx.needs_input_grad[0]:
            return None, None
        (x_c,) = ctx.saved_tensors
        degree, dtype = ctx.args
        g_x = torch.empty_like(x_c)
        _timed("mh_sh_encode_bwd", ptr(x_c), ptr(g.contiguous().float()), x_c.shape[0], degree, ptr(g_x))
        return g_x.to(dtype), None


def sh_encode(x, degree: int):
    """x [B, 3] -> [B, degree^2] fp32 (1 <= degree <= 8): the real spherical harmonics in the reference's convention, polynomials
    evaluated as they stand (shencoder.cu:28-120; include/morpheus_hip.h states them).  One launch each way, the backward only when x
    needs a gradient."""
    return _SHEncode.apply(x, int(degree))


# ------------------------------------------------------------------------------------------ HIP-graph hygiene
def graph_memset_nodes(graph: "torch.cuda.CUDAGraph"):
    """(nodes, memset nodes, smallest memset in bytes) of a captured, not yet instantiated graph (`CUDAGraph(keep_graph=True)`)."""
    lib = _lib.load()
    n, m, b = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    check(lib.mh_graph_count_memset_nodes(ctypes.c_void_p(graph.raw_cuda_graph()), ctypes.byref(n), ctypes.byref(m), ctypes.byref(b)),
          "mh_graph_count_memset_nodes")
    return n.value, m.value, b.value


def graph_replace_memset_nodes(graph: "torch.cuda.CUDAGraph") -> int:
    """Every memset node of the captured graph becomes a fill-kernel node with the same edges (csrc/graph.hip: small memset
    nodes replay wrongly on ROCm 7.2, and PyTorch's multi-block reductions memset their semaphores).  Call between the end of
    the capture and the first replay, on a graph made with `torch.cuda.CUDAGraph(keep_graph=True)`.  -> nodes replaced."""
    lib = _lib.load()
    n = ctypes.c_int64()
    check(lib.mh_graph_replace_memset_nodes(ctypes.c_void_p(graph.raw_cuda_graph()), ctypes.byref(n)), "mh_graph_replace_memset_nodes")
    return n.value
