"""The bottom layer of the mesh tool chain, what mesh, tsdf, meshrender, mesheval and poseinit all need: host arrays and their pointers for
the C ABI, camera poses and intrinsics, the checks on mesh and point arrays, mh_icp_transform, the memory cap, the device refusal.
Every pose goes through ONE sequence of numpy operations (world_to_camera): the kernels get the same bytes whichever module asks.

Import order, at module level only (no import of the package inside a function body):
    geometry <- mesh <- tsdf
    geometry <- meshrender <- mesheval          (meshrender and mesheval may also import mesh)
    geometry <- meshrender <- mesheval <- poseinit
geometry itself imports only _lib and chunking.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from ._lib import MorpheusHipError, launch, ptr, require_gpu
from .chunking import DEFAULT_FRACTION, available_bytes


def host_array(a, dtype=None) -> np.ndarray:
    """tensor or array-like -> contiguous host array of `dtype` (its own when None); no copy when it already is one"""
    a = np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=dtype)
    return a if a.flags.c_contiguous else np.ascontiguousarray(a)


def host_ptr(a: np.ndarray):
    """the c_void_p of a contiguous host array, as the C ABI takes poses and intrinsics; the caller keeps `a` alive"""
    return a.ctypes.data_as(ctypes.c_void_p)


def cv2gl(c2w) -> np.ndarray:
    """OpenGL <-> OpenCV camera-to-world (tools/vis.py:cv2gl): columns 1 and 2 negated.  Its own inverse."""
    c2w = np.array(c2w, dtype=np.float64)
    c2w[:3, 1:3] *= -1
    return c2w


def world_to_camera(c2w, convention: str = "opengl", dtype=np.float32) -> np.ndarray:
    """c2w [4,4] or [3,4] host pose in `convention`, tensor or array -> row-major `dtype` [3,4] world -> OpenCV camera: assigned
    into a float64 identity, an OpenGL pose's columns 1 and 2 negated (cv2gl), numpy.linalg.inv, rows [:3], cast once."""
    if convention not in ("opengl", "opencv"):
        raise MorpheusHipError(f"convention must be 'opengl' or 'opencv', got {convention!r}")
    c = c2w.detach().cpu().numpy() if isinstance(c2w, torch.Tensor) else np.asarray(c2w)
    if c.shape not in ((4, 4), (3, 4)):
        raise MorpheusHipError(f"c2w must be [4,4] or [3,4], got {c.shape}")
    m = np.eye(4, dtype=np.float64)
    m[:3] = c[:3]
    if convention == "opengl":
        m = cv2gl(m)
    return np.ascontiguousarray(np.linalg.inv(m)[:3].astype(dtype))


def pose_pair(c2w):
    """OpenCV camera-to-world [4,4] or [3,4] -> (c2w, w2c) float32 [3,4] host arrays: world_to_camera(c2w, "opencv") and the pose
    it inverted.  The same sequence written out a second time, not a call of it: a fusion runs this once or twice per frame and
    its host time is its wall time, where one more Python call per frame (0.25 us) shows."""
    c = c2w.detach().cpu().numpy() if isinstance(c2w, torch.Tensor) else np.asarray(c2w)
    if c.shape not in ((4, 4), (3, 4)):
        raise MorpheusHipError(f"c2w must be [4,4] or [3,4], got {c.shape}")
    m = np.eye(4, dtype=np.float64)
    m[:3] = c[:3]
    return np.ascontiguousarray(m[:3].astype(np.float32)), np.ascontiguousarray(np.linalg.inv(m)[:3].astype(np.float32))


def intrinsics(K):
    """K, tensor or array -> (fx, fy, cx, cy) as Python floats.  Its shape is the caller's to check (only cull_mesh does)."""
    K = K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else np.asarray(K)
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def mesh_arrays(vertices, triangles, colors=None, normals=None):
    """Checks the arrays of a mesh on the device -> the triangles as the int32 the C ABI takes"""
    require_gpu(vertices, triangles, colors, normals)
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32 or not vertices.is_contiguous():
        raise MorpheusHipError(f"vertices: contiguous float32 [V,3], got {vertices.dtype} {tuple(vertices.shape)}")
    if triangles.dim() != 2 or triangles.shape[1] != 3 or triangles.dtype not in (torch.int32, torch.int64) \
            or not triangles.is_contiguous():
        raise MorpheusHipError(f"triangles: contiguous int32 / int64 [T,3], got {triangles.dtype} {tuple(triangles.shape)}")
    for name, a in (("colors", colors), ("normals", normals)):
        if a is not None and (a.shape != vertices.shape or a.dtype != torch.float32 or not a.is_contiguous()):
            raise MorpheusHipError(f"{name}: contiguous float32 [V,3] like vertices, got {a.dtype} {tuple(a.shape)}")
    # the C ABI takes the int32 indices mh_mc_emit writes; extract_mesh hands out int64 (a device-side cast, no wait)
    return triangles if triangles.dtype == torch.int32 else triangles.to(torch.int32)


def require_points(name, a):
    require_gpu(a)
    if a.dim() != 2 or a.shape[1] != 3 or a.dtype != torch.float32 or not a.is_contiguous():
        raise MorpheusHipError(f"{name}: contiguous float32 [N,3], got {a.dtype} {tuple(a.shape)}")
    return a


def transform_points(points: torch.Tensor, T) -> torch.Tensor:
    """T [4,4] or [3,4] host float64 applied to fp32 points: computed in float64, rounded once."""
    require_points("points", points)
    Th = host_array(np.asarray(T, dtype=np.float64)[:3])
    out = torch.empty_like(points)
    launch("mh_icp_transform", ptr(points), points.shape[0], host_ptr(Th), ptr(out))
    return out


def gpu_device(what: str, device) -> torch.device:
    """torch.device(device), refused in `what`'s name when it is not a GPU"""
    device = torch.device(device)
    if device.type != "cuda":
        raise MorpheusHipError(f"{what} runs on an MI355X only (device is {device}); there is no CPU path")
    return device


def memory_cap_bytes(device=None, max_gb: Optional[float] = None) -> float:
    """max_gb in GB when given; else the rule of chunking.py for parked bytes: min(0.4 of the device, 0.85 of what is free)"""
    if max_gb is not None:
        return float(max_gb) * 1e9
    idx = torch.cuda.current_device() if device is None or getattr(device, "index", None) is None else device.index
    total = float(torch.cuda.get_device_properties(idx).total_memory)
    return min(DEFAULT_FRACTION * total, 0.85 * available_bytes(device))
