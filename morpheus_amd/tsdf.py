"""TSDF fusion on the device: run_tsdf_fusion / back_proj_frame (tools/vis.py:251-361) without Open3D.

The reference fuses the dataset's RGB-D frames into the background mesh of its visualiser (reconstruct_bg_mesh,
visualizer.py:110-125) with Open3D's ScalableTSDFVolume on the host.  Here the frames are integrated into a dense box of
voxels by the HIP kernels of csrc/tsdf.hip (mh_tsdf_touch + mh_tsdf_integrate per frame, no host synchronisation between
frames), the surface comes from the masked marching cubes of csrc/mesh.hip (cells with an unobserved corner give nothing) and
the vertex colours from mh_tsdf_vertex_colors.  Conventions: include/morpheus_hip.h (TSDF fusion).

Two stores share the kernels' per-voxel arithmetic.  TSDFVolume is dense inside the box: 20 bytes per voxel and one byte per
8^3 block; a box that does not fit (2^31 voxels or more, or more bytes than the cap) is refused before anything is allocated
(volume_bytes / memory_cap_bytes).  SparseTSDFVolume (csrc/tsdf_sparse.hip) holds only the blocks a frame reached, in a pool of
capacity_blocks slots behind an index volume of 4 bytes per block (sparse_bytes): the same block rule, the same bytes per
voxel, a logical box of up to 32768 voxels a side.  run_tsdf_fusion(store="sparse") sizes the pool from the frames.  The
default stays dense: the sparse store is asked for, never fallen back to.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import MorpheusHipError, launch, ptr, require_gpu
from .geometry import gpu_device, host_ptr, intrinsics, memory_cap_bytes, pose_pair   # memory_cap_bytes: also tsdf's public name
from .mesh import _count_then_emit, marching_cubes_masked, write_ply

BLOCK = 8
BYTES_PER_VOXEL = 20                 # tsdf, weight and three colour planes, fp32
PIXEL_CENTERS = ("integer", "half")
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
STORES = ("dense", "sparse")
SPARSE_MAX_SIDE_BLOCKS = 4096        # blocks per side of the sparse store's logical box (mh_tsdf_sparse_max_side_blocks)
BYTES_PER_SLOT = BLOCK ** 3 * BYTES_PER_VOXEL                       # 10 240: one block's five fp32 planes


def volume_bytes(dims: Sequence[int]) -> int:
    """device bytes of a dense volume of dims = (nx, ny, nz) voxels: 20 per voxel + 1 per 8^3 block"""
    n = int(dims[0]) * int(dims[1]) * int(dims[2])
    return n * BYTES_PER_VOXEL + n // BLOCK ** 3


def _block_dims(dims):
    nx, ny, nz = (int(d) for d in dims)
    if min(nx, ny, nz) < BLOCK or any(d % BLOCK for d in (nx, ny, nz)):
        raise MorpheusHipError(f"TSDF box: dims must be positive multiples of the block side {BLOCK}, got {(nx, ny, nz)}")
    return nx, ny, nz


def _extent(origin, dims, voxel_length) -> str:
    """the box as the refusals of check_box and check_sparse_box name it"""
    lo = [float(o) for o in origin]
    hi = [o + d * float(voxel_length) for o, d in zip(lo, dims)]
    return (f"box [{lo[0]:.3f}, {hi[0]:.3f}] x [{lo[1]:.3f}, {hi[1]:.3f}] x [{lo[2]:.3f}, {hi[2]:.3f}] at voxel_length "
            f"{float(voxel_length):g} is {dims[0]} x {dims[1]} x {dims[2]}")


def check_box(origin, dims, voxel_length: float, cap_bytes: float) -> None:
    """Raises MorpheusHipError when the dense box cannot be held: more than 2^31 - 1 voxels (the kernels' index range) or more
    bytes than cap_bytes."""
    nx, ny, nz = _block_dims(dims)
    n, need = nx * ny * nz, volume_bytes((nx, ny, nz))
    if n >= 2 ** 31 or need > cap_bytes:
        why = "more than 2^31 - 1 voxels" if n >= 2 ** 31 else f"{need / 1e9:.2f} GB of dense storage, over the cap of {cap_bytes / 1e9:.2f} GB"
        raise MorpheusHipError(
            f"TSDF {_extent(origin, (nx, ny, nz), voxel_length)} = {n} voxels: {why}.  Pass a tighter box with bounds=(min, max), or a "
            f"larger voxel_length (storage falls with its cube); max_gb= raises the cap.  run_tsdf_fusion(store=\"sparse\") and "
            f"SparseTSDFVolume hold only the blocks that the frames reach.")


def sparse_bytes(dims: Sequence[int], capacity_blocks: int) -> int:
    """device bytes of a block-sparse volume over a logical box of dims voxels with a pool of capacity_blocks slots: 10 240 per
    slot (five fp32 planes of 512 voxels) + 4 per slot (its block id) + 4 per block of the box (the index volume) + 8 (the
    slot counter and the overflow flag)"""
    blocks = (int(dims[0]) // BLOCK) * (int(dims[1]) // BLOCK) * (int(dims[2]) // BLOCK)
    return int(capacity_blocks) * (BYTES_PER_SLOT + 4) + 4 * blocks + 8


def _capacity(capacity_blocks) -> int:
    if isinstance(capacity_blocks, bool) or not isinstance(capacity_blocks, (int, np.integer)) or not 1 <= capacity_blocks < 2 ** 31:
        raise MorpheusHipError(f"capacity_blocks must be an integer in [1, 2^31), got {capacity_blocks!r}")
    return int(capacity_blocks)


def check_sparse_box(origin, dims, voxel_length: float, capacity_blocks: int, cap_bytes: float) -> None:
    """Raises MorpheusHipError when the block-sparse store cannot hold the logical box: a side over 32768 voxels, 2^31 blocks or
    more, or more bytes (sparse_bytes) than cap_bytes."""
    nx, ny, nz = _block_dims(dims)
    capacity = _capacity(capacity_blocks)
    blocks = (nx // BLOCK) * (ny // BLOCK) * (nz // BLOCK)
    need = sparse_bytes((nx, ny, nz), capacity)
    side = max(nx, ny, nz) > SPARSE_MAX_SIDE_BLOCKS * BLOCK
    if side or blocks >= 2 ** 31 or need > cap_bytes:
        why = (f"a side over {SPARSE_MAX_SIDE_BLOCKS * BLOCK} voxels" if side else "more than 2^31 - 1 blocks" if blocks >= 2 ** 31 else
               f"{need / 1e9:.2f} GB ({need} bytes: {BYTES_PER_SLOT + 4} per slot, 4 per block), over the cap of {cap_bytes / 1e9:.2f} GB")
        raise MorpheusHipError(
            f"sparse TSDF {_extent(origin, (nx, ny, nz), voxel_length)} voxels = {blocks} blocks with capacity_blocks = {capacity}: {why}.  Pass a "
            f"tighter box with bounds=(min, max), a larger voxel_length or a smaller capacity_blocks; max_gb= raises the cap.")


def box_from_bounds(lo, hi, voxel_length: float, margin: float):
    """-> (origin float64 [3], dims (nx, ny, nz)): the box [lo - margin, hi + margin] grown to whole 8^3 blocks"""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise MorpheusHipError(f"TSDF bounds must be finite with max >= min, got {lo.tolist()} .. {hi.tolist()}")
    origin = lo - margin
    side = BLOCK * float(voxel_length)
    blocks = np.maximum(np.ceil((hi + margin - origin) / side), 1).astype(np.int64)
    return origin, tuple(int(b) * BLOCK for b in blocks)


def _tensor(a, device):
    return a.to(device) if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a), device=device)


def rgb8(rgb, gray_scale: bool = False, intensity_scale: float = 1.0, alpha: float = 0.0, device=None) -> torch.Tensor:
    """The colour preparation of run_tsdf_fusion / back_proj_frame (tools/vis.py:269-282, 325-332) -> uint8 [H,W,3] on `device`.
    rgb: uint8 is taken as RGB8; floating point in [0, 1] is scaled by 255 and truncated (clamped to [0, 255] first).
    gray_scale: the channel mean in all three channels.  Otherwise intensity_scale < 1: rgb * intensity_scale; otherwise
    alpha > 0: rgb * alpha + (1 - alpha) (a blend toward white).  The input is not modified (the reference scales it in place)."""
    t = _tensor(rgb, device)
    if t.dim() != 3 or t.shape[-1] != 3:
        raise MorpheusHipError(f"rgb must be [H,W,3], got {tuple(t.shape)}")
    if t.dtype == torch.uint8:
        if not (gray_scale or intensity_scale < 1.0 or alpha > 0.0):
            return t.contiguous()
        t = t.to(torch.float32) / 255.0
    elif not t.is_floating_point():
        raise MorpheusHipError(f"rgb must be uint8 or floating point, got {t.dtype}")
    if gray_scale:
        t = t.mean(dim=-1, keepdim=True).expand(-1, -1, 3)
    elif intensity_scale < 1.0:
        t = t * intensity_scale
    elif alpha > 0.0:
        t = t * alpha + (1 - alpha)
    return (t * 255).clamp(0, 255).to(torch.uint8).contiguous()


def mask8(mask, device=None) -> Optional[torch.Tensor]:
    """mask [H,W] or [H,W,C] (channel 0) -> uint8 [H,W], 1 where mask > 0 (the reference zeroes depth where mask <= 0)"""
    if mask is None:
        return None
    t = _tensor(mask, device)
    if t.dim() == 3:
        t = t[:, :, 0]
    elif t.dim() != 2:
        raise MorpheusHipError(f"mask must be [H,W] or [H,W,C], got {tuple(t.shape)}")
    return (t > 0).to(torch.uint8).contiguous()


def _intrinsics(K, pixel_centers: str):
    if pixel_centers not in PIXEL_CENTERS:
        raise MorpheusHipError(f"pixel_centers must be one of {PIXEL_CENTERS}, got {pixel_centers!r}")
    fx, fy, cx, cy = intrinsics(K)
    if pixel_centers == "integer":                                 # Open3D's convention: the same kernels, shifted principal point
        cx, cy = cx + 0.5, cy + 0.5
    return fx, fy, cx, cy


_pose = pose_pair                    # OpenCV camera-to-world -> (c2w, w2c) float32 [3,4]; the name itself, not a call per frame


def _depth32(depth, device) -> torch.Tensor:
    t = _tensor(depth, device)
    if t.dim() != 2:
        raise MorpheusHipError(f"depth must be [H,W], got {tuple(t.shape)}")
    return t.to(torch.float32).contiguous()


def _frame(device, depth, color, K, c2w, mask, stride, pixel_centers):
    """what both stores' integrate() hand the kernels: (depth fp32, rgb uint8, mask uint8 or None, H, W, (fx, fy, cx, cy), c2w
    [3,4], w2c [3,4])"""
    intr = _intrinsics(K, pixel_centers)
    if int(stride) < 1:
        raise MorpheusHipError(f"stride must be >= 1, got {stride}")
    d = _depth32(depth, device)
    c = rgb8(color, device=device)
    m = mask8(mask, device)
    H, W = d.shape
    if c.shape[:2] != (H, W) or (m is not None and m.shape != (H, W)):
        raise MorpheusHipError(f"depth {tuple(d.shape)}, color {tuple(c.shape)} and mask "
                               f"{None if m is None else tuple(m.shape)} must share H and W")
    require_gpu(d, c, m)
    c2w_h, w2c_h = _pose(c2w)
    return d, c, m, H, W, intr, c2w_h, w2c_h


_NO_POOL = object()                  # _Volume's capacity_blocks for the dense store


class _Volume:
    """What the two stores share: the constructor's checks, the box as the kernels take it (_box), and extract_mesh around the
    store's own index-space surface (_index_mesh) and vertex_colors.  A store checks its own box and allocates."""

    def __init__(self, voxel_length: float, sdf_trunc: float, origin, dims, device, capacity_blocks=_NO_POOL):
        if not (voxel_length > 0 and sdf_trunc > 0):
            raise MorpheusHipError(f"voxel_length and sdf_trunc must be positive, got {voxel_length}, {sdf_trunc}")
        if capacity_blocks is not _NO_POOL:                        # refused after the lengths and before the device
            self.capacity = _capacity(capacity_blocks)
        self.device = gpu_device(type(self).__name__, device)
        self.voxel_length, self.sdf_trunc = float(voxel_length), float(sdf_trunc)
        self.origin = np.asarray(origin, np.float64).reshape(3).astype(np.float32)
        self.dims = tuple(int(d) for d in dims)
        self.blocks = tuple(d // BLOCK for d in self.dims)
        self.frames = 0

    def _box(self):
        return (float(self.origin[0]), float(self.origin[1]), float(self.origin[2]), self.voxel_length, self.sdf_trunc) + self.blocks

    def extract_mesh(self) -> dict:
        """-> dict(vertices [V,3] fp32 world space, triangles [T,3] int64, colors [V,3] fp32 in [0, 1]): the zero set over the
        cells whose eight corners were all observed; the two stores give the same vertex and triangle sets (the sparse one
        ordered by block).  One host synchronisation (to size the outputs)."""
        iv, tri = self._index_mesh()
        colors = self.vertex_colors(iv)
        vertices = torch.from_numpy(self.origin).to(self.device) + (iv + 0.5) * self.voxel_length   # voxel samples sit at centres
        return {"vertices": vertices.contiguous(), "triangles": tri, "colors": colors}


class TSDFVolume(_Volume):
    """A dense truncated signed distance volume on the device.  origin: world position of the box's corner; dims = (nx, ny,
    nz) voxels, multiples of 8.  Attributes: tsdf, weight [nx,ny,nz] fp32, color [3,nx,ny,nz] fp32 in [0, 255], active
    [nx/8,ny/8,nz/8] uint8."""

    def __init__(self, voxel_length: float, sdf_trunc: float, origin, dims, device="cuda", max_gb: Optional[float] = None):
        super().__init__(voxel_length, sdf_trunc, origin, dims, device)
        check_box(self.origin, self.dims, voxel_length, memory_cap_bytes(self.device, max_gb))
        nx, ny, nz = self.dims
        self.tsdf = torch.zeros(nx, ny, nz, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(nx, ny, nz, dtype=torch.float32, device=self.device)
        self.color = torch.zeros(3, nx, ny, nz, dtype=torch.float32, device=self.device)
        self.active = torch.zeros(self.blocks, dtype=torch.uint8, device=self.device)

    def integrate(self, depth, color, K, c2w, mask=None, *, depth_scale: float = 1.0, depth_trunc: float = 10.0,
                  stride: int = 4, pixel_centers: str = "half") -> None:
        """One frame: depth [H,W], color [H,W,3] (uint8 RGB8, or floating point in [0, 1]), K [3,3], c2w the OpenCV
        camera-to-world pose, mask [H,W] (pixels with mask <= 0 are not used).  Two launches, no host synchronisation."""
        d, c, m, H, W, (fx, fy, cx, cy), c2w_h, w2c_h = _frame(self.device, depth, color, K, c2w, mask, stride, pixel_centers)
        box = self._box()
        launch("mh_tsdf_touch", ptr(d), ptr(m), H, W, fx, fy, cx, cy, host_ptr(c2w_h), float(depth_scale), float(depth_trunc),
               int(stride), *box, ptr(self.active))
        launch("mh_tsdf_integrate", ptr(d), ptr(c), ptr(m), H, W, fx, fy, cx, cy, host_ptr(w2c_h), float(depth_scale),
               float(depth_trunc), *box, ptr(self.active), ptr(self.tsdf), ptr(self.weight), ptr(self.color))
        self.frames += 1

    def vertex_colors(self, index_vertices: torch.Tensor) -> torch.Tensor:
        """colours in [0, 1] of marching-cubes vertices given in the volume's index space"""
        require_gpu(index_vertices)
        V = index_vertices.shape[0]
        out = torch.empty(V, 3, dtype=torch.float32, device=self.device)
        launch("mh_tsdf_vertex_colors", ptr(index_vertices), V, ptr(self.color), *self.dims, ptr(out))
        return out

    def _index_mesh(self):
        return marching_cubes_masked(self.tsdf, self.weight, 0.0)


class SparseTSDFVolume(_Volume):
    """A truncated signed distance volume that stores only the 8^3 blocks a frame reached (include/morpheus_hip.h, the pooled
    block-sparse store).  origin, dims: the LOGICAL box, as TSDFVolume's but with up to 32768 voxels a side and no limit on the
    voxel count; capacity_blocks: the slots of the pool, fixed at construction (10 240 bytes each).  The block rule and every
    voxel's bytes are TSDFVolume's.  Attributes: slot [nbx,nby,nbz] int32 (-1: no storage), slot_block [capacity] int32, counters
    [2] int32 (slots wanted, overflow flag), tsdf, weight [capacity,512] fp32, color [3,capacity,512] fp32.
    When the frames reach more blocks than the pool has slots, the blocks beyond it stay without storage, nothing is written
    outside the pool, and the first call that reads the device anyway (check, allocated_blocks, to_dense, extract_mesh) raises."""

    def __init__(self, voxel_length: float, sdf_trunc: float, origin, dims, capacity_blocks: int, device="cuda",
                 max_gb: Optional[float] = None):
        super().__init__(voxel_length, sdf_trunc, origin, dims, device, capacity_blocks)
        check_sparse_box(self.origin, self.dims, voxel_length, self.capacity, memory_cap_bytes(self.device, max_gb))
        self.max_gb = max_gb
        n, device = BLOCK ** 3, self.device
        self.slot = torch.full(self.blocks, -1, dtype=torch.int32, device=device)
        self.slot_block = torch.zeros(self.capacity, dtype=torch.int32, device=device)
        self.counters = torch.zeros(2, dtype=torch.int32, device=device)
        self.tsdf = torch.zeros(self.capacity, n, dtype=torch.float32, device=device)
        self.weight = torch.zeros(self.capacity, n, dtype=torch.float32, device=device)
        self.color = torch.zeros(3, self.capacity, n, dtype=torch.float32, device=device)

    def integrate(self, depth, color, K, c2w, mask=None, *, depth_scale: float = 1.0, depth_trunc: float = 10.0,
                  stride: int = 4, pixel_centers: str = "half") -> None:
        """One frame, as TSDFVolume.integrate.  Two launches, no host synchronisation."""
        d, c, m, H, W, (fx, fy, cx, cy), c2w_h, w2c_h = _frame(self.device, depth, color, K, c2w, mask, stride, pixel_centers)
        launch("mh_tsdf_sparse_touch", ptr(d), ptr(m), H, W, fx, fy, cx, cy, host_ptr(c2w_h), float(depth_scale),
               float(depth_trunc), int(stride), *self._box(), self.capacity, ptr(self.slot), ptr(self.slot_block), ptr(self.counters))
        launch("mh_tsdf_sparse_integrate", ptr(d), ptr(c), ptr(m), H, W, fx, fy, cx, cy, host_ptr(w2c_h), float(depth_scale),
               float(depth_trunc), *self._box(), self.capacity, ptr(self.slot_block), ptr(self.counters), ptr(self.tsdf),
               ptr(self.weight), ptr(self.color))
        self.frames += 1

    def _checked(self, wanted: int, overflow: int) -> int:
        if overflow or wanted > self.capacity:
            raise MorpheusHipError(
                f"SparseTSDFVolume: the pool of capacity_blocks = {self.capacity} slots is full: the frames so far reached {wanted} "
                f"blocks, and those beyond the pool were left without storage, so the volume is incomplete.  Build it again with "
                f"capacity_blocks >= {wanted}; run_tsdf_fusion(store=\"sparse\") without capacity_blocks sizes the pool from the "
                f"frames (the union of the blocks their touch passes reach).")
        return wanted

    def check(self) -> int:
        """-> the number of allocated blocks; raises when the pool overflowed.  One host read."""
        return self._checked(*self.counters.tolist())

    def allocated_blocks(self) -> torch.Tensor:
        """-> int64 [n]: the linear ids (bx*nby + by)*nbz + bz of the blocks with storage, ascending.  One host read."""
        return self.slot_block[:self.check()].sort().values.long()

    def to_dense(self) -> "TSDFVolume":
        """-> a TSDFVolume over the same box with the same bytes (active = the allocated blocks); refused with the dense store's
        own error when the box does not fit it."""
        vol = TSDFVolume(self.voxel_length, self.sdf_trunc, self.origin, self.dims, device=self.device, max_gb=self.max_gb)
        self.check()
        launch("mh_tsdf_sparse_to_dense", *self.blocks, self.capacity, ptr(self.slot_block), ptr(self.counters), ptr(self.tsdf),
               ptr(self.weight), ptr(self.color), ptr(vol.tsdf), ptr(vol.weight), ptr(vol.color), ptr(vol.active))
        vol.frames = self.frames
        return vol

    @classmethod
    def from_dense(cls, dense: "TSDFVolume", keep=None, capacity_blocks: Optional[int] = None, block_order=None,
                   max_gb: Optional[float] = None) -> "SparseTSDFVolume":
        """The blocks of `dense` where keep [nbx,nby,nbz] != 0 (default: dense.active) as a sparse volume over the same box.
        capacity_blocks: default the number of kept blocks (one host read), at least 1.  block_order: a permutation of the
        nbx*nby*nbz block ids, the order in which blocks are handed their slots (no result depends on it)."""
        keep = dense.active if keep is None else _tensor(keep, dense.device)
        if tuple(keep.shape) != dense.blocks:
            raise MorpheusHipError(f"from_dense: keep must be {dense.blocks}, one entry per block, got {tuple(keep.shape)}")
        keep = (keep != 0).to(torch.uint8).contiguous()
        if capacity_blocks is None:
            capacity_blocks = max(int(keep.sum(dtype=torch.int64)), 1)
        order = None
        if block_order is not None:
            order = _tensor(block_order, dense.device).to(torch.int32).contiguous()
            if order.dim() != 1 or order.numel() != keep.numel():
                raise MorpheusHipError(f"from_dense: block_order must list all {keep.numel()} block ids, got {tuple(order.shape)}")
        vol = cls(dense.voxel_length, dense.sdf_trunc, dense.origin, dense.dims, capacity_blocks, device=dense.device, max_gb=max_gb)
        require_gpu(dense.tsdf, dense.weight, dense.color, keep, order)
        launch("mh_tsdf_sparse_from_dense", ptr(dense.tsdf), ptr(dense.weight), ptr(dense.color), ptr(keep), ptr(order), *vol.blocks,
               vol.capacity, ptr(vol.slot), ptr(vol.slot_block), ptr(vol.counters), ptr(vol.tsdf), ptr(vol.weight), ptr(vol.color))
        vol.frames = dense.frames
        return vol

    def vertex_colors(self, index_vertices: torch.Tensor) -> torch.Tensor:
        """colours in [0, 1] of marching-cubes vertices given in the logical box's index space"""
        require_gpu(index_vertices)
        V = index_vertices.shape[0]
        out = torch.empty(V, 3, dtype=torch.float32, device=self.device)
        launch("mh_tsdf_sparse_vertex_colors", ptr(index_vertices), V, ptr(self.color), ptr(self.slot), *self.blocks, self.capacity,
               ptr(out))
        return out

    def marching_cubes(self, isovalue: float = 0.0):
        """-> (vertices fp32 [V,3] in the logical box's index space, triangles int64 [T,3]): the masked marching cubes over the
        allocated blocks, in ascending block id whatever the slot order.  One host read (sizes, slot counter, overflow flag)."""
        wbytes = _lib.load().mh_mc_sparse_workspace_bytes(self.capacity)
        live = self.counters[0].clamp(max=self.capacity)
        ids = torch.where(torch.arange(self.capacity, device=self.device) < live, self.slot_block, INT32_MAX)
        sorted_blocks = ids.sort().values.to(torch.int32).contiguous()
        args = (ptr(self.tsdf), ptr(self.weight), ptr(self.slot), ptr(sorted_blocks), ptr(self.counters), *self.blocks, self.capacity,
                float(isovalue))

        def check(V, T, wanted, overflow):                         # the pool's overflow first: it explains any count
            self._checked(wanted, overflow)
            if V >= 2 ** 31 or T >= 2 ** 31:
                raise MorpheusHipError(f"SparseTSDFVolume: {V} vertices / {T} triangles do not fit int32 indices")

        return _count_then_emit("mh_mc_count_sparse", "mh_mc_emit_sparse", args, args, wbytes, self.device, self.counters, check)

    def _index_mesh(self):
        return self.marching_cubes(0.0)


def _frames(c2w_list, depth_list, mask_list, device):
    """per frame -> (depth fp32 [H,W], mask uint8 [H,W] or None, H, W, c2w [3,4] host float32), checked to be on the device"""
    for f, (c2w, depth) in enumerate(zip(c2w_list, depth_list)):
        d = _depth32(depth, device)
        m = mask8(None if mask_list is None else mask_list[f], device)
        require_gpu(d, m)
        yield d, m, d.shape[0], d.shape[1], _pose(c2w)[0]


def count_touched_blocks(K, c2w_list, depth_list, mask_list, origin, dims, voxel_length, sdf_trunc, *, depth_scale=1.0,
                         depth_trunc=10.0, stride=4, pixel_centers="integer", device="cuda") -> int:
    """-> the number of blocks of the logical box that the touch passes of all frames reach: what a SparseTSDFVolume fed the same
    frames allocates.  One launch per frame into one byte per block, and ONE host read."""
    fx, fy, cx, cy = _intrinsics(K, pixel_centers)
    device = torch.device(device)
    blocks = tuple(int(d) // BLOCK for d in dims)
    o = np.asarray(origin, np.float64).reshape(3).astype(np.float32)
    active = torch.zeros(blocks, dtype=torch.uint8, device=device)
    for d, m, H, W, c2w_h in _frames(c2w_list, depth_list, mask_list, device):
        launch("mh_tsdf_sparse_mark", ptr(d), ptr(m), H, W, fx, fy, cx, cy, host_ptr(c2w_h), float(depth_scale),
               float(depth_trunc), int(stride), float(o[0]), float(o[1]), float(o[2]), float(voxel_length), float(sdf_trunc), *blocks,
               ptr(active))
    return int(active.sum(dtype=torch.int64))


def frame_bounds(K, c2w_list, depth_list, mask_list=None, *, depth_scale=1.0, depth_trunc=10.0, stride=4,
                 pixel_centers="integer", device="cuda"):
    """-> (min float32 [3], max float32 [3]) of the usable back-projected pixels of all frames, or None without one.  One
    launch per frame and ONE host read for the sequence."""
    fx, fy, cx, cy = _intrinsics(K, pixel_centers)
    device = torch.device(device)
    acc = torch.tensor([INT32_MAX] * 3 + [INT32_MIN] * 3, dtype=torch.int32, device=device)
    for d, m, H, W, c2w_h in _frames(c2w_list, depth_list, mask_list, device):
        launch("mh_tsdf_bounds", ptr(d), ptr(m), H, W, fx, fy, cx, cy, host_ptr(c2w_h), float(depth_scale),
               float(depth_trunc), int(stride), ptr(acc))
    return decode_bounds(acc.cpu().numpy())


def decode_bounds(words: np.ndarray):
    """the six ordered int32 words of mh_tsdf_bounds -> (min [3], max [3]) float32, or None when no pixel was usable"""
    words = np.asarray(words, np.int32)
    if words[0] == INT32_MAX:
        return None
    bits = np.where(words >= 0, words, words ^ np.int32(0x7fffffff)).astype(np.int32)
    vals = bits.view(np.float32)
    return vals[:3].copy(), vals[3:].copy()


def _empty_mesh(device):
    return {"vertices": torch.zeros(0, 3, dtype=torch.float32, device=device),
            "triangles": torch.zeros(0, 3, dtype=torch.int64, device=device),
            "colors": torch.zeros(0, 3, dtype=torch.float32, device=device)}


def run_tsdf_fusion(K, H, W, c2w_list, depth_list, rgb_list, mask_list=None, skip=None, save_path=None, depth_scale=1.0,
                    depth_trunc=10.0, sdf_trunc=0.04, voxel_length=0.02, gray_scale=False, *, bounds=None,
                    pixel_centers: str = "integer", stride: int = 4, max_gb: Optional[float] = None, device="cuda",
                    intensity_scale: float = 1.0, alpha: float = 0.0, return_volume: bool = False, store: str = "dense",
                    capacity_blocks: Optional[int] = None):
    """run_tsdf_fusion (tools/vis.py:315-361) on the device -> dict(vertices, triangles, colors), what meshrender, mesheval and
    mesh.write_ply take; written as a PLY to save_path when that is given.
    K [3,3]; c2w_list: OpenCV camera-to-world poses; depth_list [H,W]; rgb_list [H,W,3] in [0, 1] (or uint8); mask_list [H,W] or
    [H,W,C]: numpy arrays or tensors, none of them modified (the reference scales rgb and zeroes depth in place).  `skip` is
    accepted and ignored, as in the reference.  pixel_centers: "integer" reads K as Open3D does (pixel centres at integers),
    "half" as the rest of this library does.  bounds = (min [3], max [3]) fixes the box (grown by sdf_trunc and to whole
    blocks); without it the box is sized from the frames' own back-projected pixels (one more launch per frame and one host
    read).  A box over max_gb (default: min(0.4 of the device, 0.85 of what is free)) is refused before anything is allocated.
    store: "dense" (TSDFVolume, the default) or "sparse" (SparseTSDFVolume: only the blocks the frames reach are stored, so a
    box the dense store refuses can be fused); never chosen automatically.  capacity_blocks (sparse only): the slots of the
    pool; without it the pool is sized exactly, by one touch pass over all frames and one more host read.
    No host synchronisation inside the frame loop."""
    n = len(c2w_list)
    if len(depth_list) != n or len(rgb_list) != n or (mask_list is not None and len(mask_list) != n):
        raise MorpheusHipError(f"run_tsdf_fusion: {n} poses, {len(depth_list)} depth maps, {len(rgb_list)} images"
                               + ("" if mask_list is None else f", {len(mask_list)} masks"))
    if not (voxel_length > 0 and sdf_trunc > 0 and depth_scale > 0 and depth_trunc > 0) or int(stride) < 1:
        raise MorpheusHipError("run_tsdf_fusion: voxel_length, sdf_trunc, depth_scale and depth_trunc must be positive, stride >= 1")
    _intrinsics(K, pixel_centers)
    if store not in STORES:
        raise MorpheusHipError(f"run_tsdf_fusion: store must be one of {STORES}, got {store!r}")
    if capacity_blocks is not None:
        if store != "sparse":
            raise MorpheusHipError("run_tsdf_fusion: capacity_blocks sizes the pool of store=\"sparse\"; the dense store has none")
        _capacity(capacity_blocks)
    H, W = int(H), int(W)
    for f in range(n):
        if tuple(depth_list[f].shape) != (H, W):
            raise MorpheusHipError(f"run_tsdf_fusion: depth {f} is {tuple(depth_list[f].shape)}, expected {(H, W)}")
    device = gpu_device("run_tsdf_fusion", device)
    if bounds is None:
        found = frame_bounds(K, c2w_list, depth_list, mask_list, depth_scale=depth_scale, depth_trunc=depth_trunc, stride=stride,
                             pixel_centers=pixel_centers, device=device) if n else None
        if found is None:                                          # no frame, or no usable pixel: an empty mesh
            mesh = _empty_mesh(device)
            if save_path is not None:
                _save(save_path, mesh)
            return (mesh, None) if return_volume else mesh
        bounds = found
    origin, dims = box_from_bounds(bounds[0], bounds[1], voxel_length, sdf_trunc)
    if store == "sparse":
        if capacity_blocks is None:
            check_sparse_box(origin, dims, voxel_length, 1, memory_cap_bytes(device, max_gb))
            capacity_blocks = max(1, count_touched_blocks(K, c2w_list, depth_list, mask_list, origin, dims, voxel_length, sdf_trunc,
                                                          depth_scale=depth_scale, depth_trunc=depth_trunc, stride=stride,
                                                          pixel_centers=pixel_centers, device=device))
        vol = SparseTSDFVolume(voxel_length, sdf_trunc, origin, dims, capacity_blocks, device=device, max_gb=max_gb)
    else:
        vol = TSDFVolume(voxel_length, sdf_trunc, origin, dims, device=device, max_gb=max_gb)
    for f in range(n):
        c = rgb8(rgb_list[f], gray_scale, intensity_scale, alpha, device=device)
        vol.integrate(depth_list[f], c, K, c2w_list[f], None if mask_list is None else mask_list[f], depth_scale=depth_scale,
                      depth_trunc=depth_trunc, stride=stride, pixel_centers=pixel_centers)
    mesh = vol.extract_mesh()
    if save_path is not None:
        _save(save_path, mesh)
    return (mesh, vol) if return_volume else mesh


def back_proj_frame(K, H, W, c2w, depth, rgb, save_path=None, mask=None, depth_scale=1.0, depth_trunc=10.0, sdf_trunc=0.04,
                    voxel_length=0.02, gray_scale=False, intensity_scale=1.0, alpha=0.0, **kwargs):
    """back_proj_frame (tools/vis.py:251-312): run_tsdf_fusion of one frame, with its colour options (gray_scale, else
    intensity_scale < 1, else alpha > 0).  store= and capacity_blocks= go through.  The point-cloud form (save_as_pcd) is not
    provided."""
    if kwargs.pop("save_as_pcd", False):
        raise MorpheusHipError("back_proj_frame: save_as_pcd (Open3D's extract_point_cloud) is not provided")
    return run_tsdf_fusion(K, H, W, [c2w], [depth], [rgb], None if mask is None else [mask], save_path=save_path,
                           depth_scale=depth_scale, depth_trunc=depth_trunc, sdf_trunc=sdf_trunc, voxel_length=voxel_length,
                           gray_scale=gray_scale, intensity_scale=intensity_scale, alpha=alpha, **kwargs)


def _save(path, mesh) -> None:
    d = os.path.dirname(os.fspath(path))
    if d:
        os.makedirs(d, exist_ok=True)
    write_ply(path, mesh["vertices"], mesh["triangles"], mesh["colors"])
