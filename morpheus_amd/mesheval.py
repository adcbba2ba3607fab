"""Mesh evaluation on the device: tools/culling.py of the reference (eval_mesh -> cull_meshes -> eval_mesh_3d -> metric_3d.txt,
and eval_depthL1 on depths.npz) without pyrender, trimesh, open3d or cv2.

The reference culls each exported mesh against its frame's camera (a pyrender depth map of both windings), samples 50 000
points on the culled mesh and on the ground-truth mesh with trimesh, aligns the two with Open3D's point-to-point ICP, and
scores accuracy / completion with a CPU KD-tree.  Here the depth map is morpheus_amd.meshrender's, and the HIP kernels of
csrc/mesheval.hip do the rest: mh_nn_search is the exact brute-force nearest-neighbour search every score and every ICP
iteration rests on; mh_cull_*, mh_mesh_area_weights / mh_sample_surface and mh_icp_* are the small kernels around it
(conventions in include/morpheus_hip.h, restated in numpy by tests/mesheval_oracle.py).  The reference subdivides every mesh to
0.01 edges before it culls (trimesh.remesh.subdivide_to_size); subdivide_to_size does that on the device (csrc/subdivide.hip,
mh_subdiv_*, tests/subdivide_oracle.py), and cull_mesh / eval_mesh run it with subdivide=True -- the reference's behaviour; the
default, False, culls the triangles as they are given.

Known differences from the reference's scores: with subdivide=True the subdivided mesh is trimesh's as a surface and
as a set of triangles, not in vertex order or in which midpoints are shared (no consumer depends on either); the ICP parameters
and stopping rule follow Open3D's documented defaults and were never compared with Open3D; sample_surface is seeded, where the
reference draws from numpy's global generator.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import MorpheusHipError, launch, ptr, require_gpu
from .geometry import (host_array, host_ptr, memory_cap_bytes, mesh_arrays, require_points, transform_points,  # noqa: F401
                       world_to_camera)                            # transform_points: also mesheval's public name
from .mesh import load_mesh
from .meshrender import mesh_sequence, render_mesh


# ---- nearest neighbour ---------------------------------------------------------------------------------------------------

def nearest(query: torch.Tensor, ref: torch.Tensor, max_dist: Optional[float] = None, segments: int = 0):
    """-> (idx int32 [Nq], d2 float32 [Nq]): for each query the reference point of least d2 = (dx*dx + dy*dy) + dz*dz (rounded
    fp32 operators), the lowest index among equals; candidates with a NaN or infinite d2, or with d2 > float32(max_dist)^2,
    are ignored; idx = -1 and d2 = +inf where none is left.  Exact brute force.  `segments` (how many runs the reference set
    is cut into; 0: chosen from the sizes) never changes the result.  No host synchronisation."""
    require_points("query", query)
    require_points("ref", ref)
    if segments > 4096:
        raise MorpheusHipError(f"nearest: at most 4096 segments, got {segments}")
    max_d2 = math.inf
    if max_dist is not None:
        m = np.float32(max_dist)
        if not m >= 0:
            raise MorpheusHipError(f"nearest: max_dist must be >= 0, got {max_dist}")
        with np.errstate(over="ignore"):
            max_d2 = float(m * m)
    Nq, Nr = query.shape[0], ref.shape[0]
    dev = query.device
    idx = torch.empty(Nq, dtype=torch.int32, device=dev)
    d2 = torch.empty(Nq, dtype=torch.float32, device=dev)
    ws = torch.empty(Nq, dtype=torch.int64, device=dev)
    launch("mh_nn_search", ptr(query), Nq, ptr(ref), Nr, max_d2, int(segments), ptr(ws), ptr(idx), ptr(d2))
    return idx, d2


# ---- culling -------------------------------------------------------------------------------------------------------------

def world_to_camera_f64(c2w) -> np.ndarray:
    """OpenGL camera-to-world [4,4] or [3,4] host pose -> float64 [3,4] world -> OpenCV camera (columns 1 and 2 negated, then
    numpy.linalg.inv, as cull_from_one_pose does)."""
    return world_to_camera(c2w, "opengl", np.float64)


def _depth_map(name, d, H, W, device):
    if d is None:
        return None
    if not isinstance(d, torch.Tensor):
        d = torch.from_numpy(host_array(d, np.float32)).to(device)
    require_gpu(d)
    if tuple(d.shape) != (H, W) or d.dtype != torch.float32 or not d.is_contiguous():
        raise MorpheusHipError(f"{name}: contiguous float32 [{H},{W}], got {d.dtype} {tuple(d.shape)}")
    return d


def cull_mesh(vertices: torch.Tensor, triangles: torch.Tensor, colors: Optional[torch.Tensor] = None, *, c2w, K, H: int,
              W: int, depth_gt=None, eps: float = 0.005, remove_missing_depth: bool = True, rendered_depth=None,
              return_masks: bool = False, subdivide: bool = False, max_edge: float = 0.01, max_iter: int = 10) -> dict:
    """cull_one_mesh / cull_from_one_pose (tools/culling.py:17-49, 86-131): keep the triangles that the camera of pose c2w
    (OpenGL, as the dataset stores it) observes -- a vertex in the frustum and no further than eps behind the rendered depth
    -- unless all three vertices fall on pixels without ground-truth depth.
    -> dict(vertices [V',3], triangles int64 [T',3] re-indexed, colors [V',3] or None), order preserved, unreferenced
    vertices removed; with return_masks also frustum / observed / invalid (bool [V]) and keep (bool [T]).
    rendered_depth defaults to render_mesh's double-sided depth map from the same camera (near = 0.01 as the reference's
    pyrender camera; its zfar = 10 is not restated: the scene box is [-1, 1]^3).  depth_gt: [H,W] float32, needed when
    remove_missing_depth.  subdivide=True is the reference's behaviour: the mesh is first subdivided to max_edge (subdivide_to_size;
    0.01 and 10 rounds there), so that what is kept or dropped is a piece no longer than that; the depth map is still rendered
    from the mesh as given ("we don't need subdivided mesh to render depth"), the masks, the kept set and the interpolated
    colours are those of the subdivided mesh, and return_masks refers to its arrays.  The default culls the triangles as they
    are given.  One host synchronisation (to size the outputs), one more with subdivide."""
    tri = mesh_arrays(vertices, triangles, colors)
    H, W = int(H), int(W)
    dev = vertices.device
    Kh = host_array(K)
    if Kh.shape != (3, 3):
        raise MorpheusHipError(f"K must be [3,3], got {Kh.shape}")
    if remove_missing_depth and depth_gt is None:
        raise MorpheusHipError("cull_mesh: remove_missing_depth needs depth_gt")
    if rendered_depth is None:
        rendered_depth = render_mesh(vertices, tri, c2w=c2w, K=Kh, H=H, W=W, convention="opengl", mode="color",
                                     near=0.01)["depth"]
    rendered_depth = _depth_map("rendered_depth", rendered_depth, H, W, dev)
    depth_gt = _depth_map("depth_gt", depth_gt, H, W, dev) if remove_missing_depth else None
    if subdivide:
        fine = _subdivide(vertices, tri, colors, max_edge, max_iter, None, False)
        if fine is not None:
            vertices, tri, colors, _ = fine
    w2c, Kd = world_to_camera_f64(c2w), host_array(Kh, np.float64)
    V, T = vertices.shape[0], tri.shape[0]
    frustum, observed, invalid = (torch.zeros(V, dtype=torch.uint8, device=dev) for _ in range(3))
    keep = torch.zeros(T, dtype=torch.uint8, device=dev)
    launch("mh_cull_vertices", ptr(vertices), V, host_ptr(w2c), host_ptr(Kd), H, W, ptr(rendered_depth), ptr(depth_gt), float(eps),
           ptr(frustum), ptr(observed), ptr(invalid))
    launch("mh_cull_triangles", ptr(tri), T, V, ptr(observed), ptr(invalid), ptr(keep))
    keep = keep.bool()
    kept = tri[keep].long()                                        # the host waits here
    used = torch.zeros(V, dtype=torch.bool, device=dev)
    used[kept.reshape(-1)] = True
    remap = torch.cumsum(used, 0) - 1
    out = {"vertices": vertices[used].contiguous(), "triangles": remap[kept].contiguous(),
           "colors": None if colors is None else colors[used].contiguous()}
    if return_masks:
        out.update(frustum=frustum.bool(), observed=observed.bool(), invalid=invalid.bool(), keep=keep)
    return out


# ---- subdivision ---------------------------------------------------------------------------------------------------------

def _subdivide(vertices, tri, colors, max_edge, max_iter, max_gb, want_index, hand_on_bytes=0):
    """subdivide_to_size on checked arrays (tri int32) -> (vertices, tri int32, colors, index int32 or None), or None when no
    triangle is split.  hand_on_bytes: what the caller allocates per output triangle on top (counted under the cap)."""
    m = np.float32(max_edge)
    if not (m > 0 and np.isfinite(m)):
        raise MorpheusHipError(f"subdivide_to_size: max_edge must be finite and positive in float32, got {max_edge}")
    max_iter = int(max_iter)
    if not 0 <= max_iter <= 10:
        raise MorpheusHipError(f"subdivide_to_size: max_iter must be in [0, 10], got {max_iter}")
    V, T = vertices.shape[0], tri.shape[0]
    if T == 0:
        return None
    dev = vertices.device
    depth = torch.empty(T, dtype=torch.int32, device=dev)
    counts = torch.empty(2, T, dtype=torch.int64, device=dev)
    launch("mh_subdiv_count", ptr(vertices), V, ptr(tri), T, float(m), max_iter, ptr(depth), ptr(counts[0]), ptr(counts[1]))
    starts = torch.zeros(2, T + 1, dtype=torch.int64, device=dev)
    starts[:, 1:] = torch.cumsum(counts, 1)                       # exclusive prefix sums: integer, exact in any order
    n_new, n_tri, deepest = (int(x) for x in torch.stack([starts[0, T], starts[1, T], depth.max().long()]).cpu())   # the host waits here
    if deepest > max_iter:
        long = depth > max_iter
        e = vertices[tri[long].long()].double()
        longest = float(torch.stack([(e[:, 1] - e[:, 0]).norm(dim=1), (e[:, 2] - e[:, 1]).norm(dim=1),
                                     (e[:, 0] - e[:, 2]).norm(dim=1)]).max())
        raise MorpheusHipError(
            f"subdivide_to_size: {int(long.sum())} of {T} triangles still have an edge above max_edge = {float(m):g} after max_iter = "
            f"{max_iter} halvings (longest edge {longest:g}); pass a larger max_edge (trimesh raises here too)")
    if n_new == 0 and n_tri == T:
        return None
    if V + n_new >= 2 ** 31 or n_tri >= 2 ** 31:
        raise MorpheusHipError(f"subdivide_to_size: {V + n_new} vertices and {n_tri} triangles at max_edge = {float(m):g} do not fit "
                               f"int32 indices; pass a larger max_edge")
    need = (V + n_new) * 12 * (1 if colors is None else 2) + n_tri * (12 + (4 if want_index else 0) + hand_on_bytes)
    cap = memory_cap_bytes(dev, max_gb)
    if need > cap:
        raise MorpheusHipError(
            f"subdivide_to_size: {V} vertices / {T} triangles become {V + n_new} vertices / {n_tri} triangles at max_edge = "
            f"{float(m):g}: {need / 1e9:.3f} GB, over the cap of {cap / 1e9:.3f} GB.  Pass a larger max_edge (the counts fall with "
            f"its square); max_gb= raises the cap.")
    out_v = torch.empty(V + n_new, 3, dtype=torch.float32, device=dev)
    out_c = None if colors is None else torch.empty(V + n_new, 3, dtype=torch.float32, device=dev)
    out_t = torch.empty(n_tri, 3, dtype=torch.int32, device=dev)
    index = torch.empty(n_tri, dtype=torch.int32, device=dev) if want_index else None
    launch("mh_subdiv_emit", ptr(vertices), ptr(colors), V, ptr(tri), T, ptr(depth), ptr(starts[0]), ptr(starts[1]), n_new, n_tri,
           ptr(out_v), ptr(out_c), ptr(out_t), ptr(index))
    return out_v, out_t, out_c, index


def subdivide_to_size(vertices: torch.Tensor, triangles: torch.Tensor, colors: Optional[torch.Tensor] = None, *,
                      max_edge: float = 0.01, max_iter: int = 10, max_gb: Optional[float] = None,
                      return_index: bool = False) -> dict:
    """trimesh.remesh.subdivide_to_size(vertices, triangles, max_edge, max_iter) as cull_one_mesh runs it (tools/culling.py:
    93-96): every triangle with an edge longer than max_edge is split into four at its edge midpoints, and so are its children.
    The children's edges are the parent's halved, so a triangle ends as 4^d pieces, d the smallest depth at which its longest
    edge * 2^-d <= max_edge (float64, no square root; include/morpheus_hip.h).  -> dict(vertices [V',3], triangles int64 [T',3],
    colors [V',3] or None -- interpolated like the positions), with return_index also index int64 [T'], the input triangle of
    every output triangle.  The V input vertices come first, unchanged; new vertices are not shared between input triangles (on a
    shared edge of equal depth they are the same bytes); trimesh's vertex order is not reproduced.  When no triangle needs
    splitting the result is the input.  A triangle with an index outside [0, V) or with a NaN edge passes through.
    One host synchronisation (the two totals and the largest depth).  Raises when a triangle is still too long after max_iter
    halvings (an infinite coordinate included), when the result does not fit int32 indices, and -- before anything is allocated
    -- when it would exceed max_gb (default: min(0.4 of the device, 0.85 of what is free))."""
    tri = mesh_arrays(vertices, triangles, colors)
    res = _subdivide(vertices, tri, colors, max_edge, max_iter, max_gb, return_index, hand_on_bytes=24 + (8 if return_index else 0))
    if res is None:
        out = {"vertices": vertices, "triangles": triangles if triangles.dtype == torch.int64 else triangles.long(), "colors": colors}
        if return_index:
            out["index"] = torch.arange(tri.shape[0], dtype=torch.int64, device=vertices.device)
        return out
    out = {"vertices": res[0], "triangles": res[1].long(), "colors": res[2]}
    if return_index:
        out["index"] = res[3].long()
    return out


# ---- surface sampling ----------------------------------------------------------------------------------------------------

def area_weights(vertices: torch.Tensor, triangles: torch.Tensor):
    """-> (areas float32 [T], cum int64 [T]): the triangles' areas and the inclusive prefix sum of their fixed-point values
    (grid q = G * 2^-40, G the power of two strictly above the largest area): integer, so exact in any order."""
    tri = mesh_arrays(vertices, triangles)
    V, T = vertices.shape[0], tri.shape[0]
    areas = torch.empty(T, dtype=torch.float32, device=vertices.device)
    qarea = torch.empty(T + 1, dtype=torch.int64, device=vertices.device)
    launch("mh_mesh_area_weights", ptr(vertices), V, ptr(tri), T, ptr(areas), ptr(qarea))
    return areas, torch.cumsum(qarea[:T], 0)


def sample_surface(vertices: torch.Tensor, triangles: torch.Tensor, count: int, *, seed: int = 0,
                   uniforms: Optional[torch.Tensor] = None):
    """trimesh.sample.sample_surface, reproducible: faces chosen by area, points uniform inside them.
    -> (points float32 [count,3], face int32 [count]).  uniforms [count,3] float32 in [0, 1) (column 0 picks the face, 1 and 2
    the barycentrics) default to a torch.Generator seeded with `seed` on the device.  One host synchronisation (an empty mesh
    or one of zero total area raises)."""
    tri = mesh_arrays(vertices, triangles)
    count = int(count)
    dev = vertices.device
    V, T = vertices.shape[0], tri.shape[0]
    if T == 0 or V == 0:
        raise MorpheusHipError("sample_surface: the mesh is empty")
    if uniforms is None:
        g = torch.Generator(device=dev)
        g.manual_seed(int(seed))
        uniforms = torch.rand(count, 3, generator=g, dtype=torch.float32, device=dev)
    require_points("uniforms", uniforms)
    if uniforms.shape[0] != count:
        raise MorpheusHipError(f"uniforms: [{count},3], got {tuple(uniforms.shape)}")
    _, cum = area_weights(vertices, tri)
    if int(cum[-1].item()) <= 0:
        raise MorpheusHipError("sample_surface: the mesh has zero total area")
    points = torch.empty(count, 3, dtype=torch.float32, device=dev)
    face = torch.empty(count, dtype=torch.int32, device=dev)
    launch("mh_sample_surface", ptr(vertices), V, ptr(tri), T, ptr(cum), ptr(uniforms), count, ptr(points), ptr(face))
    return points, face


# ---- rigid alignment -----------------------------------------------------------------------------------------------------

def icp_sums(moved: torch.Tensor, target: torch.Tensor, idx: torch.Tensor, d2: torch.Tensor) -> torch.Tensor:
    """-> float64 [17] on the device: n, sum d2, sum p, sum q, sum p q^T over the correspondences with idx >= 0, in a fixed
    order (the same bytes run to run)."""
    require_points("moved", moved)
    require_points("target", target)
    require_gpu(idx, d2)
    N = moved.shape[0]
    if idx.shape != (N,) or idx.dtype != torch.int32 or d2.shape != (N,) or d2.dtype != torch.float32:
        raise MorpheusHipError("icp_sums: idx int32 [N] and d2 float32 [N] as nearest returns them")
    lib = _lib.load()
    sums = torch.zeros(17, dtype=torch.float64, device=moved.device)
    ws = torch.empty(lib.mh_icp_workspace_bytes(), dtype=torch.uint8, device=moved.device)
    launch("mh_icp_sums", ptr(moved), N, ptr(target), target.shape[0], ptr(idx), ptr(d2), ptr(ws), ptr(sums))
    return sums


def kabsch_update(sums: np.ndarray) -> np.ndarray:
    """The rigid motion [4,4] (no scale) that best maps the p onto the q in the least-squares sense, from the 17 sums."""
    n = sums[0]
    mp, mq = sums[2:5] / n, sums[5:8] / n
    Hm = sums[8:17].reshape(3, 3) - n * np.outer(mp, mq)
    U, _, Vt = np.linalg.svd(Hm)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    out = np.eye(4)
    out[:3, :3] = R
    out[:3, 3] = mq - R @ mp
    return out


def icp_align(source: torch.Tensor, target: torch.Tensor, threshold: float = 0.1, max_iteration: int = 30,
              relative_fitness: float = 1e-6, relative_rmse: float = 1e-6) -> dict:
    """get_align_transformation (tools/culling.py:148-166): point-to-point ICP from the identity.
    -> dict(transformation float64 [4,4] numpy, fitness, inlier_rmse, iterations).  The parameters and the stopping rule
    (both |delta fitness| and |delta rmse| below their thresholds, or max_iteration) are what Open3D's registration_icp is
    understood to use; agreement with Open3D is unverified.  One host synchronisation per iteration."""
    require_points("source", source)
    require_points("target", target)
    Ns = source.shape[0]
    T = np.eye(4)

    def evaluate():
        moved = transform_points(source, T)
        idx, d2 = nearest(moved, target, max_dist=threshold)
        s = icp_sums(moved, target, idx, d2).cpu().numpy()         # the host waits here
        n = s[0]
        return s, (n / Ns if Ns else 0.0), (math.sqrt(s[1] / n) if n > 0 else 0.0)

    if Ns == 0 or target.shape[0] == 0:
        return {"transformation": T, "fitness": 0.0, "inlier_rmse": 0.0, "iterations": 0}
    s, fitness, rmse = evaluate()
    if s[0] == 0:
        return {"transformation": np.eye(4), "fitness": 0.0, "inlier_rmse": 0.0, "iterations": 0}
    it = 0
    while it < max_iteration:
        T = kabsch_update(s) @ T
        it += 1
        s_new, f_new, r_new = evaluate()
        done = abs(f_new - fitness) < relative_fitness and abs(r_new - rmse) < relative_rmse
        s, fitness, rmse = s_new, f_new, r_new
        if done or s[0] == 0:
            break
    return {"transformation": T, "fitness": float(fitness), "inlier_rmse": float(rmse), "iterations": it}


# ---- the scores ----------------------------------------------------------------------------------------------------------

def mesh_metrics(rec, gt, align: bool = True, num_points: int = 50000, seed: int = 0, dist_th: float = 0.05,
                 device="cuda", uniforms_rec=None, uniforms_gt=None) -> dict:
    """calc_3d_metric (tools/culling.py:189-221) -> {'acc': mean distance rec -> gt in cm, 'comp': mean distance gt -> rec in
    cm, 'comp ratio': % of gt points closer than dist_th to rec}.  rec / gt: mesh dicts (vertices, triangles) on the device or
    paths of PLYs in read_ply's layout; a gt with triangles None is a point cloud and is used as it is.  align: icp_align
    between the two vertex sets first, applied to rec.  Both surfaces are sampled with num_points points (seeds `seed` and
    `seed + 1`, or the injected uniforms).  Distances are sqrt(d2) in float64, the means in float64."""
    rec, gt = load_mesh(rec, device), load_mesh(gt, device)
    rv = rec["vertices"]
    if align:
        rv = transform_points(rv, icp_align(rv, gt["vertices"])["transformation"])
    def count(u):                                                  # injected uniforms bring their own count
        return num_points if u is None else u.shape[0]

    rec_pts = sample_surface(rv, rec["triangles"], count(uniforms_rec), seed=seed, uniforms=uniforms_rec)[0]
    if gt.get("triangles") is None:
        gt_pts = require_points("gt vertices", gt["vertices"])
    else:
        gt_pts = sample_surface(gt["vertices"], gt["triangles"], count(uniforms_gt), seed=seed + 1, uniforms=uniforms_gt)[0]
    d_acc = nearest(rec_pts, gt_pts)[1].double().sqrt()
    d_comp = nearest(gt_pts, rec_pts)[1].double().sqrt()
    return {"acc": float(d_acc.mean()) * 100, "comp": float(d_comp.mean()) * 100,
            "comp ratio": float((d_comp < dist_th).double().mean()) * 100}


def eval_mesh(meshes_or_dir, gt_meshes, poses, K, H: int, W: int, depths_gt, save_file: Optional[str] = None, epoch: int = 0,
              mesh_epoch: Optional[int] = None, align: bool = True, num_points: int = 50000, seed: int = 0, eps: float = 0.005,
              remove_missing_depth: bool = True, device="cuda", subdivide: bool = False, max_edge: float = 0.01) -> dict:
    """The loop of eval_mesh + eval_mesh_3d (tools/culling.py:223-235, 262-275): mesh i is culled from poses[i] against
    depths_gt[i] and scored against gt_meshes[i]; nothing is written in between.  meshes_or_dir as in render_all_meshes
    (`mesh_epoch` selects a directory's files); gt_meshes: mesh dicts or PLY paths by frame.  Appends the reference's line
    "Ep_{epoch}:\\t Acc:{}\\t Comp:{}" to save_file.  subdivide, max_edge: handed to cull_mesh; subdivide=True is what the reference
    does (every mesh subdivided to 0.01 edges before it is culled), the default culls the exported triangles as they are.
    -> {"acc": [...], "comp": [...], "comp ratio": [...], "frames": [...]}."""
    out = {"acc": [], "comp": [], "comp ratio": [], "frames": []}
    for i, mesh in mesh_sequence(meshes_or_dir, device, mesh_epoch):
        culled = cull_mesh(mesh["vertices"], mesh["triangles"], mesh.get("colors"), c2w=poses[i], K=K, H=H, W=W,
                           depth_gt=depths_gt[i], eps=eps, remove_missing_depth=remove_missing_depth, subdivide=subdivide,
                           max_edge=max_edge)
        m = mesh_metrics(culled, gt_meshes[i], align=align, num_points=num_points, seed=seed, device=device)
        for k in ("acc", "comp", "comp ratio"):
            out[k].append(m[k])
        out["frames"].append(i)
    if save_file is not None:
        with open(save_file, "a") as fh:
            print("Ep_{}:\t Acc:{}\t Comp:{}".format(epoch, np.array(out["acc"]).mean(), np.array(out["comp"]).mean()), file=fh)
    return out


def eval_depth_l1(depths, depths_gt, masks, save_dir: Optional[str] = None) -> np.ndarray:
    """eval_depthL1 (tools/culling.py:237-260): per frame the mean of |gt - pred| over the pixels with gt > 0, mask > 0 and an
    error in (0, 1]; 0 for a frame without such a pixel (the reference takes the mean of nothing there: nan).  depths: what render_all_meshes returns ({"depth_{i}": [H,W]}) or the path of a depths.npz; depths_gt
    [F,H,W]; masks [F,H,W] or [F,H,W,C] (channel 0).  Writes depthL1_scores.txt and depthL1_score_mean.txt (%.5f) under
    save_dir; the reference's colour-mapped error images need cv2 and are not written.  Host arithmetic, as there."""
    if isinstance(depths, (str, os.PathLike)):
        depths = np.load(os.fspath(depths))
    errors = []
    for i in range(len(depths_gt)):
        pred = np.asarray(depths[f"depth_{i}"])
        gt = depths_gt[i].cpu().numpy() if isinstance(depths_gt[i], torch.Tensor) else np.asarray(depths_gt[i])
        mask = masks[i].cpu().numpy() if isinstance(masks[i], torch.Tensor) else np.asarray(masks[i])
        if mask.ndim == 3:
            mask = mask[..., 0]
        err = np.abs(gt - pred)
        counted = (gt > 0) & (mask > 0) & (err > 0) & (err <= 1.0)
        errors.append(err[counted].mean() if counted.any() else 0.0)
    errors = np.array(errors)
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        np.savetxt(os.path.join(save_dir, "depthL1_scores.txt"), errors, fmt="%.5f")
        np.savetxt(os.path.join(save_dir, "depthL1_score_mean.txt"), np.array([errors.mean()]), fmt="%.5f")
    return errors
