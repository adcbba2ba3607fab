"""Writes tests/golden/eval3d.npz: closed-form inputs and what the reference's own evaluation functions return for them.

    python tools/make_eval_golden.py /path/to/reference

The one file of the mesh evaluation that reads the reference's tree (as oracle/make_golden.py does for the field); no test,
smoke() or benchmark does.  tools/culling.py there imports cv2, trimesh, pyrender, open3d and imageio at module level; the
functions pinned here (cull_from_one_pose, accuracy, completion, completion_ratio, eval_depthL1) are plain numpy / scipy, so
those names are stubbed with empty modules and the module is loaded as it is.  Numeric arrays only.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesheval_oracle as mo  # noqa: E402
import raster_oracle as ro  # noqa: E402

F = np.float32
BAND = 1e-12
SCORE_BAND = 2.0 ** -21


def load_reference(ref_root):
    for name in ("cv2", "imageio", "trimesh", "pyrender", "open3d", "tqdm"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["tqdm"].tqdm = lambda it, *a, **k: it
    sys.modules["cv2"].applyColorMap = lambda img, cmap: img
    sys.modules["cv2"].COLORMAP_JET = 2
    sys.modules["imageio"].imwrite = lambda *a, **k: None
    spec = importlib.util.spec_from_file_location("ref_culling", os.path.join(ref_root, "tools", "culling.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sphere_points(rng, n, radius, centre=(0, 0, 0)):
    p = rng.standard_normal((n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    return (p * radius + np.asarray(centre)).astype(F)


def torus_points(rng, n, R=0.45, r=0.15):
    a, b = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    return np.stack([(R + r * np.cos(b)) * np.cos(a), (R + r * np.cos(b)) * np.sin(a), r * np.sin(b)], 1).astype(F)


def sphere_depth(c2w_gl, K, H, W, radius):
    """The analytic front depth (camera-space z) of the sphere |x| = radius at every pixel (u, v) = (column, row), the pixel
    (u, v) standing for the ray through (u, v, 1) K^-T as cull_from_one_pose's projection has it; 0 where the ray misses."""
    w2c = mo.world_to_camera_f64(c2w_gl)
    centre = w2c[:, 3]                                             # the sphere's centre (the origin) in camera space
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1)
    a = (d * d).sum(-1)
    b = d @ centre
    disc = b * b - a * (centre @ centre - radius * radius)
    z = np.where(disc > 0, (b - np.sqrt(np.maximum(disc, 0))) / a, 0.0)
    return np.where(z > 0, z, 0.0).astype(F)


def near_boundary(vertices, w2c, K, H, W, depth, eps):
    """Vertices within BAND (relative) of a decision boundary of the cull masks, from the oracle's own float64 values."""
    v = vertices.astype(np.float64)
    cam = v @ w2c[:, :3].T + w2c[:, 3]
    uvz = cam @ K.T
    pz = uvz[:, 2] + 1e-8
    px, py = uvz[:, 0] / pz, uvz[:, 1] / pz
    fr, _, _ = mo.cull_vertices(vertices, w2c, K, H, W, depth, None, eps)
    u = np.where(fr, px, 0).astype(np.int64)
    w = np.where(fr, py, 0).astype(np.int64)
    limit = (depth[w, u] + F(eps)).astype(np.float64)

    def close(a, b):
        return np.abs(a - b) <= BAND * np.maximum(np.abs(a), np.abs(b)) + 1e-300

    edge = close(px, 0) | close(px, W - 1) | close(py, 0) | close(py, H - 1) | close(pz, 0)
    pixel = fr & (close(px, np.rint(px)) | close(py, np.rint(py)))
    return edge | pixel | (fr & close(pz, limit))


def main(ref_root, out_path):
    ref = load_reference(ref_root)
    rng = np.random.default_rng(20240607)
    out = {}

    # culling: points on a sphere of radius 0.5, a pinhole camera at distance 1.6, the sphere's analytic depth map, holes in a
    # checker of 8-pixel squares punched into depth_gt
    H, W = 120, 160
    K = np.array([[131.25, 0, 80.0], [0, 131.25, 60.0], [0, 0, 1]])
    c2w = ro.look_at((0.5, 0.4, 1.466), (0, 0, 0))
    c2w[:3, 3] *= 1.6 / np.linalg.norm(c2w[:3, 3])
    verts = sphere_points(rng, 20000, 0.5)
    depth = sphere_depth(c2w, K, H, W, 0.5)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth_gt = np.where(((ii // 8) + (jj // 8)) % 2 == 0, depth, F(0)).astype(F)
    obs, inv = ref.cull_from_one_pose(verts.astype(np.float64), c2w.copy(), K, H, W, depth, eps=0.005, depth_gt=depth_gt,
                                      remove_missing_depth=True)
    obs2, inv2 = ref.cull_from_one_pose(verts.astype(np.float64), c2w.copy(), K, H, W, depth, eps=0.005, depth_gt=depth_gt,
                                        remove_missing_depth=False)
    band = near_boundary(verts, mo.world_to_camera_f64(c2w), K, H, W, depth, 0.005)
    assert band.mean() <= 1e-4, f"{band.sum()} of {band.size} vertices sit on a decision boundary"
    assert 0.1 < obs.mean() < 0.6 and 0.05 < inv.mean() < 0.6 and not inv2.any(), (obs.mean(), inv.mean())
    out.update(cull_vertices=verts, cull_c2w=c2w, cull_K=K, cull_HW=np.array([H, W]), cull_depth=depth, cull_depth_gt=depth_gt,
               cull_eps=np.array(0.005), cull_obs=obs, cull_inv=inv, cull_obs_keep_depth=obs2)

    # scores: a sphere and a torus against a larger, shifted sphere and a thinner torus (distances on both sides of dist_th)
    gt = np.concatenate([sphere_points(rng, 3000, 0.5), torus_points(rng, 3000)])
    rec = np.concatenate([sphere_points(rng, 3000, 0.53, (0.02, -0.01, 0.03)), torus_points(rng, 2000, 0.47, 0.12)])
    acc, comp, ratio = ref.accuracy(gt, rec), ref.completion(gt, rec), ref.completion_ratio(gt, rec, dist_th=0.05)
    from scipy.spatial import cKDTree
    d = cKDTree(rec.astype(np.float64)).query(gt.astype(np.float64))[0]
    assert not ((d > 0.05 * (1 - SCORE_BAND)) & (d < 0.05 * (1 + SCORE_BAND))).any()
    assert 0.05 < ratio < 0.999, ratio
    out.update(score_gt=gt, score_rec=rec, score_acc=np.array(acc), score_comp=np.array(comp), score_ratio=np.array(ratio),
               score_dist_th=np.array(0.05))

    # depth L1: three small frames, masks with a channel axis, gt holes, errors above 1 and exact zeros
    Fr, h, w = 3, 24, 32
    d_gt = rng.uniform(0.5, 2.0, (Fr, h, w)).astype(F)
    d_gt[rng.uniform(size=d_gt.shape) < 0.2] = 0
    d_pred = (d_gt + rng.normal(0, 0.05, d_gt.shape)).astype(F)
    d_pred[rng.uniform(size=d_gt.shape) < 0.05] += F(1.5)
    same = rng.uniform(size=d_gt.shape) < 0.05
    d_pred[same] = d_gt[same]
    masks = (rng.uniform(size=(Fr, h, w, 3)) < 0.8).astype(F)
    dataset = types.SimpleNamespace(num_frames=Fr, depths=d_gt, masks=masks)
    captured = []
    real_savetxt = np.savetxt
    np.savetxt = lambda path, arr, **k: captured.append(np.array(arr, np.float64))
    try:
        with tempfile.TemporaryDirectory() as tmp:
            ddir = os.path.join(tmp, "depth")
            os.makedirs(ddir)
            np.savez(os.path.join(ddir, "depths.npz"), **{f"depth_{i}": d_pred[i] for i in range(Fr)})
            ref.eval_depthL1(ddir, dataset)
    finally:
        np.savetxt = real_savetxt
    out.update(l1_pred=d_pred, l1_gt=d_gt, l1_masks=masks, l1_scores=captured[0])

    np.savez_compressed(out_path, **out)
    size = os.path.getsize(out_path)
    assert size < 1 << 20, size
    print(out_path, size, "bytes;", {k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "eval3d.npz"))
