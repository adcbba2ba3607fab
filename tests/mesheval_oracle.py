"""Numpy restatement of the mesh-evaluation conventions of include/morpheus_hip.h (mh_nn_*, mh_cull_*, mh_mesh_area_weights,
mh_sample_surface, mh_icp_*), written from the header text.  fp32 arrays and numpy's fp32 operators round every operation as
the header says; float64 where the header says float64.  Slow and plain on purpose.
"""
from __future__ import annotations

import math

import numpy as np

F = np.float32


# ---- nearest neighbour ---------------------------------------------------------------------------------------------------

def pair_d2(q, r):
    """q [Nq,3], r [Nr,3] fp32 -> d2 [Nq,Nr] fp32 = (dx*dx + dy*dy) + dz*dz."""
    with np.errstate(all="ignore"):
        dx = q[:, None, 0] - r[None, :, 0]
        dy = q[:, None, 1] - r[None, :, 1]
        dz = q[:, None, 2] - r[None, :, 2]
        return (dx * dx + dy * dy) + dz * dz


def nearest(query, ref, max_dist=None, chunk=256):
    """-> (idx int32 [Nq], d2 fp32 [Nq])."""
    query, ref = np.ascontiguousarray(query, F), np.ascontiguousarray(ref, F)
    Nq, Nr = query.shape[0], ref.shape[0]
    idx = np.full(Nq, -1, np.int32)
    best = np.full(Nq, np.inf, F)
    if Nr == 0 or Nq == 0:
        return idx, best
    max_d2 = F(np.inf)
    if max_dist is not None:
        with np.errstate(over="ignore"):
            max_d2 = F(max_dist) * F(max_dist)
    for a in range(0, Nq, chunk):
        d2 = pair_d2(query[a:a + chunk], ref)
        with np.errstate(invalid="ignore"):
            admissible = (d2 < F(np.inf)) & (d2 <= max_d2)         # NaN fails both
        d2 = np.where(admissible, d2, F(np.inf))
        j = np.argmin(d2, axis=1)                                  # the first occurrence: lowest index among equals
        m = d2[np.arange(d2.shape[0]), j]
        won = m < F(np.inf)
        idx[a:a + chunk] = np.where(won, j, -1)
        best[a:a + chunk] = m
    return idx, best


# ---- culling -------------------------------------------------------------------------------------------------------------

def cv2gl(c2w):
    c = np.array(c2w, dtype=np.float64)
    c[:3, 1:3] *= -1
    return c


def world_to_camera_f64(c2w):
    m = np.eye(4)
    m[:3] = np.asarray(c2w, np.float64)[:3]
    return np.linalg.inv(cv2gl(m))[:3]


def cull_vertices(vertices, w2c, K, H, W, rendered_depth, depth_gt, eps):
    """-> frustum, observed, invalid (bool [V]).  w2c float64 [3,4], K float64 [3,3]; depth maps fp32 [H,W]."""
    v = np.asarray(vertices, F).astype(np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    R, t = np.asarray(w2c, np.float64)[:, :3], np.asarray(w2c, np.float64)[:, 3]
    K = np.asarray(K, np.float64)
    with np.errstate(all="ignore"):
        cam = [((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + t[r] for r in range(3)]
        uvz = [(K[r, 0] * cam[0] + K[r, 1] * cam[1]) + K[r, 2] * cam[2] for r in range(3)]
        pz = uvz[2] + 1e-8
        px, py = uvz[0] / pz, uvz[1] / pz
        frustum = (0 <= px) & (px <= W - 1) & (0 <= py) & (py <= H - 1) & (pz > 0)
    u = np.where(frustum, px, 0.0).astype(np.int64)                # truncation; read only inside the frustum
    w = np.where(frustum, py, 0.0).astype(np.int64)
    limit = (np.asarray(rendered_depth, F)[w, u] + F(eps)).astype(np.float64)      # the sum in fp32
    with np.errstate(invalid="ignore"):
        observed = frustum & (pz < limit)
    if depth_gt is None:
        invalid = np.zeros_like(frustum)
    else:
        invalid = frustum & (np.asarray(depth_gt, F)[w, u] <= 0)
    return frustum, observed, invalid


def cull_triangles(triangles, V, observed, invalid):
    tri = np.asarray(triangles, np.int64)
    ok = ((tri >= 0) & (tri < V)).all(axis=1)
    safe = np.where(ok[:, None], tri, 0)
    return ok & observed[safe].any(axis=1) & ~invalid[safe].all(axis=1)


def compact(vertices, triangles, colors, keep):
    """Kept triangles and the vertices they reference, order preserved, re-indexed."""
    kept = np.asarray(triangles, np.int64)[keep]
    used = np.zeros(vertices.shape[0], bool)
    used[kept.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return vertices[used], remap[kept], None if colors is None else colors[used]


def cull_mesh(vertices, triangles, colors, c2w, K, H, W, rendered_depth, depth_gt=None, eps=0.005, remove_missing_depth=True):
    fr, ob, inv = cull_vertices(vertices, world_to_camera_f64(c2w), K, H, W, rendered_depth,
                                depth_gt if remove_missing_depth else None, eps)
    keep = cull_triangles(triangles, vertices.shape[0], ob, inv)
    v, t, c = compact(vertices, triangles, colors, keep)
    return {"vertices": v, "triangles": t, "colors": c, "frustum": fr, "observed": ob, "invalid": inv, "keep": keep}


# ---- surface sampling ----------------------------------------------------------------------------------------------------

def triangle_areas(vertices, triangles):
    v = np.asarray(vertices, F)
    tri = np.asarray(triangles, np.int64)
    ok = ((tri >= 0) & (tri < v.shape[0])).all(axis=1)
    safe = np.where(ok[:, None], tri, 0)
    a, b, c = v[safe[:, 0]], v[safe[:, 1]], v[safe[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        area = np.sqrt((nx * nx + ny * ny) + nz * nz) * F(0.5)
        area = np.where(ok & (area < F(np.inf)), area, F(0.0)).astype(F)
    return area


def area_weights(vertices, triangles):
    """-> (areas fp32 [T], qarea int64 [T], cum int64 [T])."""
    area = triangle_areas(vertices, triangles)
    m = area.max() if area.size else F(0)
    E = int(np.array(m, F).view(np.uint32) >> 23)
    q = np.rint(area.astype(np.float64) * math.ldexp(1.0, 166 - E)).astype(np.int64)
    return area, q, np.cumsum(q)


def sample_surface(vertices, triangles, uniforms):
    """-> (points fp32 [count,3], face int32 [count]) for injected uniforms fp32 [count,3]."""
    v = np.asarray(vertices, F)
    tri = np.asarray(triangles, np.int64)
    u = np.asarray(uniforms, F)
    _, _, cum = area_weights(v, tri)
    total = int(cum[-1])
    assert total > 0
    u0 = u[:, 0].astype(np.float64)
    with np.errstate(invalid="ignore"):
        target = np.where(u0 >= 1, total - 1, np.where(u0 >= 0, u0 * float(total), 0.0)).astype(np.int64)
    target = np.minimum(target, total - 1)
    face = np.searchsorted(cum, target, side="right")             # the first f with cum[f] > target
    r1, r2 = u[:, 1].copy(), u[:, 2].copy()
    flip = (r1 + r2) > F(1)
    r1 = np.where(flip, F(1) - r1, r1)
    r2 = np.where(flip, F(1) - r2, r2)
    v0, v1, v2 = v[tri[face, 0]], v[tri[face, 1]], v[tri[face, 2]]
    pts = (v0 + r1[:, None] * (v1 - v0)) + r2[:, None] * (v2 - v0)
    return pts.astype(F), face.astype(np.int32)


# ---- rigid alignment -----------------------------------------------------------------------------------------------------

def transform_points(points, T):
    p = np.asarray(points, F).astype(np.float64)
    T = np.asarray(T, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([(((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(F) for r in range(3)], axis=1)


def icp_terms(moved, target, idx, d2):
    """The [n_corr, 17] float64 terms whose column sums are the 17 numbers."""
    sel = idx >= 0
    p = np.asarray(moved, F)[sel].astype(np.float64)
    q = np.asarray(target, F)[idx[sel]].astype(np.float64)
    pq = (p[:, :, None] * q[:, None, :]).reshape(-1, 9)
    return np.concatenate([np.ones((p.shape[0], 1)), d2[sel].astype(np.float64)[:, None], p, q, pq], axis=1)


def icp_sums(moved, target, idx, d2):
    return icp_terms(moved, target, idx, d2).sum(axis=0)


def kabsch_update(sums):
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


def icp_align(source, target, threshold=0.1, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    source, target = np.asarray(source, F), np.asarray(target, F)
    Ns = source.shape[0]
    T = np.eye(4)

    def evaluate():
        moved = transform_points(source, T)
        idx, d2 = nearest(moved, target, max_dist=threshold)
        s = icp_sums(moved, target, idx, d2)
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

def point_metrics(rec_pts, gt_pts, dist_th=0.05):
    d_acc = np.sqrt(nearest(rec_pts, gt_pts)[1].astype(np.float64))
    d_comp = np.sqrt(nearest(gt_pts, rec_pts)[1].astype(np.float64))
    return {"acc": d_acc.mean() * 100, "comp": d_comp.mean() * 100, "comp ratio": (d_comp < dist_th).mean() * 100,
            "d_comp": d_comp}


def mesh_metrics(rec, gt, uniforms_rec, uniforms_gt, align=True, dist_th=0.05):
    rv = np.asarray(rec["vertices"], F)
    if align:
        rv = transform_points(rv, icp_align(rv, gt["vertices"])["transformation"])
    rec_pts = sample_surface(rv, rec["triangles"], uniforms_rec)[0]
    gt_pts = gt["vertices"] if gt.get("triangles") is None else sample_surface(gt["vertices"], gt["triangles"], uniforms_gt)[0]
    return point_metrics(rec_pts, gt_pts, dist_th)


def depth_l1(depths, depths_gt, masks):
    out = []
    for i in range(len(depths_gt)):
        gt, mask = np.asarray(depths_gt[i]), np.asarray(masks[i])
        if mask.ndim == 3:
            mask = mask[..., 0]
        err = np.abs(gt - np.asarray(depths[f"depth_{i}"]))
        counted = (gt > 0) & (mask > 0) & (err > 0) & (err <= 1.0)
        out.append(err[counted].mean() if counted.any() else 0.0)
    return np.array(out)


# ---- motions for the tests (meshes and cameras: tests/raster_oracle.py) ---------------------------------------------------

def mixed_area_mesh(icosphere):
    """From an icosphere builder (tests/raster_oracle.py): a sphere whose faces span areas of 10^4 : 1 (a cap scaled down by
    100), plus zero-area faces."""
    v, t = icosphere(2, 0.5)
    v = v.copy()
    small = v[:, 2] > 0.3
    v[small] = (v[small] * F(0.01) + np.array((0, 0, 0.8), F)).astype(F)
    t = t[small[t].all(axis=1) | (~small[t]).all(axis=1)]
    return v, np.concatenate([t, np.array([(0, 0, 1), (3, 3, 3)]), t[:5][:, [0, 0, 2]]])


def rigid(rx, ry, rz, t):
    """[4,4] float64: rotations about x, y, z (radians, applied in that order), then translation t."""
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    m = np.eye(4)
    m[:3, :3] = Rz @ Ry @ Rx
    m[:3, 3] = t
    return m
