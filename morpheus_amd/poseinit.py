"""Pose initialisation on the device: preprocess/pose_init/registrate.py of the reference (intermediate/transformations.npy and
radius.txt, what create_camera.py turns into cameras_sphere.npz) without the external program it calls.

The reference back-projects every frame's masked depth (mask2camera), centres the cloud, writes it as an .obj and runs
`Fast-Robust-ICP/build/FRICP <target> <source> <record> 3` ("Robust ICP") through os.system, first (or previous) frame against the
current one.  Here the clouds stay on the device: mh_depth_points_* is mask2camera as a count -> scan -> emit compaction,
robust_icp is a Welsch-weighted, graduated point-to-point ICP on mesheval.nearest (exact brute force), mh_icp_transform,
mh_icp_wsums and kabsch_update, and mh_knn_d2 gives the point spacing that ends its schedule (csrc/poseinit.hip; conventions in
include/morpheus_hip.h, restated in numpy by tests/poseinit_oracle.py).  init_poses is registrate.py's main loop, init_poses_from_dir
reads and writes its files.

Known differences from the reference: robust_icp is FRICP's method 3 as its paper describes it and as remembered -- the
binary was never available, so agreement with FRICP is UNVERIFIED (as Open3D's ICP in mesheval.icp_align); Anderson acceleration,
which changes FRICP's iteration count and not its fixed point, is not built.  The clouds are fp32 on the device (the reference's are
float64 on the host, written to the .obj with repr's digits): transformations and radius agree to fp32 rounding of the points.  No
.obj files are written, and visualization.py's merged cloud is not produced.

Import order: geometry <- meshrender <- mesheval <- poseinit.
"""
from __future__ import annotations

import math
import os
from glob import glob
from typing import Callable, Optional

import numpy as np
import torch

from . import _lib
from ._lib import MorpheusHipError, launch, ptr, require_gpu
from .geometry import gpu_device, host_array, intrinsics, require_points, transform_points
from .mesheval import kabsch_update, nearest

NU_END_K = 1.0 / (3.0 * math.sqrt(3.0))


# ---- masked back-projection ----------------------------------------------------------------------------------------------

def depth_points(depth: torch.Tensor, mask: torch.Tensor, K, return_pixels: bool = False):
    """mask2camera (registrate.py:42-54): depth [H,W] float32 in metres and mask [H,W] uint8 on the device, K [3,3] (or larger;
    fx, fy, cx, cy are read from it) -> points float32 [n,3] of the pixels with mask != 0 and depth > 0, in row-major pixel order
    (numpy.nonzero's).  x = depth * (u - cx) / fx in float64 from the fp32 depth, rounded once; pixel coordinates are integers, as
    there.  With return_pixels also the pixel index v*W + u of every point, int32 [n].  One host synchronisation (the count)."""
    if depth.dim() != 2 or depth.dtype != torch.float32 or not depth.is_contiguous():
        raise MorpheusHipError(f"depth: contiguous float32 [H,W], got {depth.dtype} {tuple(depth.shape)}")
    if mask.shape != depth.shape or mask.dtype != torch.uint8 or not mask.is_contiguous():
        raise MorpheusHipError(f"mask: contiguous uint8 {tuple(depth.shape)} like depth, got {mask.dtype} {tuple(mask.shape)}")
    require_gpu(depth, mask)
    H, W = depth.shape
    if H > 16384 or W > 16384:
        raise MorpheusHipError(f"depth_points: at most 16384 x 16384 pixels, got {H} x {W}")
    fx, fy, cx, cy = intrinsics(K)
    dev = depth.device
    tile = _lib.load().mh_depth_points_tile()
    tiles = (H * W + tile - 1) // tile
    counts = torch.empty(tiles, dtype=torch.int64, device=dev)
    launch("mh_depth_points_count", ptr(depth), ptr(mask), H, W, ptr(counts))
    starts = torch.zeros(tiles + 1, dtype=torch.int64, device=dev)
    starts[1:] = torch.cumsum(counts, 0)                           # exclusive prefix sum: integer, exact in any order
    n = int(starts[tiles])                                         # the host waits here
    points = torch.empty(n, 3, dtype=torch.float32, device=dev)
    pixels = torch.empty(n, dtype=torch.int32, device=dev) if return_pixels else None
    launch("mh_depth_points_emit", ptr(depth), ptr(mask), H, W, fx, fy, cx, cy, ptr(starts), n, ptr(points), ptr(pixels))
    return (points, pixels) if return_pixels else points


# ---- point spacing -------------------------------------------------------------------------------------------------------

def knn_d2(points: torch.Tensor, k: int) -> torch.Tensor:
    """-> float32 [N,k]: for every point the k smallest d2 = (dx*dx + dy*dy) + dz*dz (rounded fp32 operators, as nearest) to the
    OTHER points, ascending; the point itself is left out by index, so a duplicate counts with 0.  k in [1, 8]; +inf where fewer
    than k other points have a finite d2.  Exact brute force.  No host synchronisation."""
    k = int(k)
    if not 1 <= k <= 8:
        raise MorpheusHipError(f"knn_d2: k must be in [1, 8], got {k}")
    require_points("points", points)
    out = torch.empty(points.shape[0], k, dtype=torch.float32, device=points.device)
    launch("mh_knn_d2", ptr(points), points.shape[0], k, ptr(out))
    return out


def knn_median(points: torch.Tensor, k: int = 7) -> float:
    """The point spacing FRICP ends its schedule on: per point the median of the distances to its k - 1 nearest other points (the
    k nearest of a search that finds the point itself first; for 6 of them the mean of the 3rd and 4th), then the median over
    the points.  Distances are sqrt(d2) in float64 and both medians numpy's, in float64.  k in [2, 9].  One host synchronisation.
    nan for an empty cloud, +inf when the points have fewer than about k / 2 neighbours."""
    k = int(k)
    if not 2 <= k <= 9:
        raise MorpheusHipError(f"knn_median: k must be in [2, 9] (k - 1 neighbours of mh_knn_d2's [1, 8]), got {k}")
    d2 = knn_d2(points, k - 1)
    if d2.shape[0] == 0:
        return math.nan
    with np.errstate(invalid="ignore"):
        return float(np.median(np.median(np.sqrt(d2.cpu().numpy().astype(np.float64)), axis=1)))      # the host waits here


# ---- robust rigid registration -------------------------------------------------------------------------------------------

def icp_wsums(moved: torch.Tensor, target: torch.Tensor, idx: torch.Tensor, d2: torch.Tensor, inv_2nu2: float) -> torch.Tensor:
    """-> float64 [19] on the device: with w = exp(-d2 * inv_2nu2) in float64 per correspondence (idx >= 0): sum w, sum w d2,
    sum w p, sum w q, sum w p q^T, sum (1 - w), the number of correspondences -- in mesheval.icp_sums' order, so that
    kabsch_update takes [:17] as it is, and with inv_2nu2 = 0 [:17] are icp_sums' bytes."""
    require_points("moved", moved)
    require_points("target", target)
    require_gpu(idx, d2)
    N = moved.shape[0]
    if idx.shape != (N,) or idx.dtype != torch.int32 or d2.shape != (N,) or d2.dtype != torch.float32:
        raise MorpheusHipError("icp_wsums: idx int32 [N] and d2 float32 [N] as nearest returns them")
    inv_2nu2 = float(inv_2nu2)
    if not (0.0 <= inv_2nu2 < math.inf):
        raise MorpheusHipError(f"icp_wsums: inv_2nu2 must be finite and >= 0, got {inv_2nu2}")
    lib = _lib.load()
    sums = torch.zeros(19, dtype=torch.float64, device=moved.device)
    ws = torch.empty(lib.mh_icp_wsums_workspace_bytes(), dtype=torch.uint8, device=moved.device)
    launch("mh_icp_wsums", ptr(moved), N, ptr(target), target.shape[0], ptr(idx), ptr(d2), inv_2nu2, ptr(ws), ptr(sums))
    return sums


def _diagonal(points: torch.Tensor) -> float:
    """the bounding box's diagonal in float64 (nan for a cloud with a NaN coordinate)"""
    return float((points.amax(0).double() - points.amin(0).double()).norm())


def robust_icp(source: torch.Tensor, target: torch.Tensor, *, init=None, nu_begin_k: float = 3.0, nu_end_k: float = NU_END_K,
               nu_alpha: float = 0.5, knn: int = 7, max_icp: int = 100, stop: float = 1e-5) -> dict:
    """Robust point-to-point ICP with the Welsch function and graduated non-convexity -- method 3 ("Robust ICP") of Fast-Robust-ICP
    (Zhang, Yao, Deng: Fast and Robust Iterative Closest Point, TPAMI 2021) as remembered, WITHOUT its Anderson acceleration, which
    changes the iteration count and not the fixed point.  Agreement with the FRICP binary is UNVERIFIED: it was never available.
    -> dict(transformation float64 [4,4] numpy, iterations, stages, nu, energy, weight_sum, converged).  T maps source onto
    target, as in icp_align.  The definition:
      scale = the larger bounding-box diagonal of the two clouds; T = init, or the identity.
      correspondences = nearest(T source, target), no distance bound.
      nu_end = nu_end_k * knn_median(target, knn); nu = max(nu_begin_k * median of the first correspondence distances, nu_end).
      A stage is at most max_icp iterations of { sums = icp_wsums at 1 / (2 nu^2); T_new = kabsch_update(sums[:17]) @ T; new
      correspondences } and ends when ||T_new - T||_F < stop, the translation column divided by scale.  After a stage
      nu = max(nu * nu_alpha, nu_end); the stage that ran at nu_end is the last.
    converged: the last stage ended on `stop`.  energy = sum (1 - w) and weight_sum = sum w at nu_end over the final correspondences
    (one more evaluation).  Degenerate input returns the current T with converged False: sum w == 0 or not finite, fewer than 3
    correspondences, or a nu that is not positive and finite (a target without distinct neighbours); empty clouds return the
    identity.  One host synchronisation per iteration."""
    require_points("source", source)
    require_points("target", target)
    if not (0.0 < nu_alpha < 1.0):
        raise MorpheusHipError(f"robust_icp: nu_alpha must be in (0, 1), got {nu_alpha}")
    T = np.eye(4) if init is None else np.array(host_array(init, np.float64), dtype=np.float64)
    if T.shape != (4, 4):
        raise MorpheusHipError(f"robust_icp: init must be [4,4], got {T.shape}")
    out = {"transformation": T, "iterations": 0, "stages": 0, "nu": math.nan, "energy": math.nan, "weight_sum": 0.0,
           "converged": False}
    if source.shape[0] == 0 or target.shape[0] == 0:
        out["transformation"] = np.eye(4)
        return out
    scale = max(_diagonal(source), _diagonal(target))
    nu_end = nu_end_k * knn_median(target, knn)

    def correspond():
        moved = transform_points(source, T)
        return (moved,) + nearest(moved, target)

    moved, idx, d2 = correspond()
    first = np.sqrt(d2[idx >= 0].cpu().numpy().astype(np.float64))
    nu = max(nu_begin_k * float(np.median(first)), nu_end) if first.size else math.nan
    out["nu"] = nu
    if not (0.0 < nu < math.inf and 0.0 < nu_end and 0.0 < scale < math.inf):
        return out
    iterations = stages = 0
    while True:
        stages += 1
        converged = False
        for _ in range(int(max_icp)):
            s = icp_wsums(moved, target, idx, d2, 1.0 / (2.0 * nu * nu)).cpu().numpy()      # the host waits here
            if not (0.0 < s[0] < math.inf) or s[18] < 3:
                out.update(transformation=T, iterations=iterations, stages=stages, nu=nu)
                return out
            T_new = kabsch_update(s[:17]) @ T
            iterations += 1
            delta = T_new - T
            delta[:3, 3] /= scale
            T = T_new
            moved, idx, d2 = correspond()
            if np.linalg.norm(delta) < stop:
                converged = True
                break
        if nu == nu_end:
            break
        nu = max(nu * nu_alpha, nu_end)
    s = icp_wsums(moved, target, idx, d2, 1.0 / (2.0 * nu * nu)).cpu().numpy()
    return {"transformation": T, "iterations": iterations, "stages": stages, "nu": nu, "energy": float(s[17]),
            "weight_sum": float(s[0]), "converged": converged}


# ---- registrate.py's main loop -------------------------------------------------------------------------------------------

def mask_rule(mask_png) -> np.ndarray:
    """mask_read (registrate.py:24-38) on the decoded image -> uint8 [H,W] of 0 / 1: the values / 255, the mean of the first three
    channels of a colour image, > 0.5."""
    m = np.array(mask_png, dtype=int) / 255
    if m.ndim == 3:
        m = np.sum(m[..., :3], 2) / 3.
    elif m.ndim != 2:
        raise MorpheusHipError(f"mask: [H,W] or [H,W,C], got {m.shape}")
    return (m > 0.5).astype(np.uint8)


def depth_rule(raw, depth_scale: float = 1000.0) -> np.ndarray:
    """depth_read (registrate.py:9-20) on the decoded image -> float32 [H,W] metres: the fp32 quotient; 0 stays 0 and means no
    depth (the reference marks it -1 and masks it out)."""
    raw = np.array(raw, dtype=int)
    if raw.ndim != 2:
        raise MorpheusHipError(f"depth: [H,W], got {raw.shape}")
    return np.ascontiguousarray(raw.astype(np.float32) / np.float32(depth_scale))


def _default_register(source, target):
    return robust_icp(source, target)["transformation"]


def init_poses(depths, masks, K, *, depth_scale: float = 1000.0, rigid_registrate: int = 1,
               register: Optional[Callable] = None, device="cuda") -> dict:
    """registrate.py's main loop (lines 110-178) -> dict(transformations float64 [N,4,4] numpy, radius float).
    depths: N raw depth images (integers, [H,W]); depth = raw.astype(float32) / depth_scale, 0 = no depth.  masks: N mask images
    ([H,W] or [H,W,C], 0..255; mask_rule).  K: [3,3] (fx, fy, cx, cy).  Every frame's cloud (depth_points) is centred on its float64
    mean (transformation_coarse).  rigid_registrate 0: the translation only; 1: `register` first cloud -> current cloud, T_i =
    coarse_i @ fine_i; 2: previous -> current with the reference's running product (fine_i is multiplied onto frames i.. and frame
    i's coarse onto the product; the world points then use that matrix's rotation and translation, as there).  World points are
    (xyz_coarse - t) R in float64; radius = 1.2 x the largest point norm not above numpy's 95th percentile of all frames' norms.
    register(source, target) -> [4,4] gets the centred fp32 clouds on the device; it defaults to robust_icp's transformation.  A
    frame without a masked depth pixel raises (the reference takes the mean of nothing).  The norms are gathered on the host."""
    if rigid_registrate not in (0, 1, 2):
        raise MorpheusHipError(f"init_poses: rigid_registrate must be 0, 1 or 2, got {rigid_registrate}")
    if len(depths) != len(masks):
        raise MorpheusHipError(f"init_poses: {len(depths)} depth images and {len(masks)} masks")
    dev = gpu_device("init_poses", device)
    register = _default_register if register is None else register
    total = len(depths)
    transformations = np.repeat(np.eye(4)[None, ...], total, axis=0)
    norms = []
    first = previous = None
    for i in range(total):
        depth, mask = depth_rule(depths[i], depth_scale), mask_rule(masks[i])
        if depth.shape != mask.shape:
            raise MorpheusHipError(f"init_poses: frame {i}: depth {depth.shape} and mask {mask.shape}")
        xyz = depth_points(torch.from_numpy(depth).to(dev), torch.from_numpy(mask).to(dev), K)
        if xyz.shape[0] == 0:
            raise MorpheusHipError(f"init_poses: frame {i} has no masked pixel with depth")
        xyz64 = xyz.double()
        mean = xyz64.mean(0)
        world = xyz64 - mean                                       # xyz_coarse, float64 as there
        coarse = np.eye(4)
        coarse[:3, 3] = mean.cpu().numpy()
        if rigid_registrate != 2 or i == 0:
            transformations[i] = coarse
        if rigid_registrate:
            shift = np.eye(4)
            shift[:3, 3] = -coarse[:3, 3]
            cloud = transform_points(xyz, shift)                   # the centred cloud in fp32: x - mean in float64, rounded once
            if i == 0:
                first = cloud
            else:
                fine = np.array(host_array(register(first if rigid_registrate == 1 else previous, cloud), np.float64))
                if fine.shape != (4, 4):
                    raise MorpheusHipError(f"init_poses: register must return [4,4], got {fine.shape}")
                if rigid_registrate == 1:
                    transformations[i] = coarse @ fine
                    rot, trans = fine[:3, :3], fine[:3, 3]
                else:
                    transformations[i:] = fine[None] @ transformations[i:]
                    transformations[i] = coarse @ transformations[i]
                    rot, trans = transformations[i, :3, :3], transformations[i, :3, 3]
                world = (world - torch.from_numpy(np.ascontiguousarray(trans)).to(dev)) @ torch.from_numpy(np.ascontiguousarray(rot)).to(dev)
            previous = cloud
        norms.append(world.norm(dim=1).cpu().numpy())
    radius = math.nan
    if total:
        whole = np.concatenate(norms)
        radius = float(whole[whole <= np.percentile(whole, 95)].max() * 1.2)
    return {"transformations": transformations, "radius": radius}


def _images(data_path, sub):
    files = sorted(glob(os.path.join(data_path, sub, "*.jpg")))
    return files or sorted(glob(os.path.join(data_path, sub, "*.png")))


def init_poses_from_dir(data_path, *, depth_scale: float = 1000.0, rigid_registrate: int = 1, register: Optional[Callable] = None,
                        device="cuda") -> dict:
    """registrate.py as a whole: reads data_path/intrinsics.txt, depth/* and mask/* (.jpg, else .png, sorted, with PIL), runs
    init_poses and writes intermediate/transformations.npy (float64 [N,16]) and intermediate/radius.txt (%.8f), the files the
    reference's create_camera.py reads.  No .obj point clouds are written.  -> init_poses' dict."""
    from PIL import Image
    data_path = os.fspath(data_path)
    K = np.loadtxt(os.path.join(data_path, "intrinsics.txt"))
    depth_files, mask_files = _images(data_path, "depth"), _images(data_path, "mask")
    if len(depth_files) != len(mask_files):
        raise MorpheusHipError(f"{data_path}: {len(depth_files)} depth images and {len(mask_files)} masks")
    if not depth_files:
        raise MorpheusHipError(f"{data_path}: no depth/*.jpg or depth/*.png")
    out = init_poses([np.array(Image.open(f), dtype=int) for f in depth_files], [np.array(Image.open(f), dtype=int) for f in mask_files],
                     K, depth_scale=depth_scale, rigid_registrate=rigid_registrate, register=register, device=device)
    os.makedirs(os.path.join(data_path, "intermediate"), exist_ok=True)
    np.savetxt(os.path.join(data_path, "intermediate", "radius.txt"), np.array([out["radius"]]), fmt="%.8f")
    np.save(os.path.join(data_path, "intermediate", "transformations.npy"), out["transformations"].reshape(-1, 16))
    return out
