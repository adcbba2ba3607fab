"""CPU (no GPU): the numpy restatement of the mesh evaluation (tests/mesheval_oracle.py, written from include/morpheus_hip.h)
held to tests/golden/eval3d.npz -- what the reference's own cull_from_one_pose, accuracy / completion / completion_ratio and
eval_depthL1 return for closed-form inputs (tools/make_eval_golden.py) -- and to properties that need no table; argument
validation of the new entry points."""
import os

import numpy as np
import pytest

from tests import mesheval_oracle as eo
from tests import raster_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SCORE_TOL = 2.0 ** -21         # twice the bound on a distance from five rounded fp32 operations (8 * 2^-24 on d2, half on sqrt)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "eval3d.npz")))


@pytest.fixture(scope="module")
def lib():
    from morpheus_amd import _lib, build
    build.build()
    return _lib.load()


def _decision_band(g, rel=1e-12):
    """Vertices within `rel` of a decision boundary of the masks (|pz - (depth + eps)|, the frustum edges, a pixel boundary of
    px / py), where the reference's BLAS matmul and the elementwise form may round differently."""
    H, W = (int(x) for x in g["cull_HW"])
    w2c, K = eo.world_to_camera_f64(g["cull_c2w"]), g["cull_K"]
    cam = g["cull_vertices"].astype(np.float64) @ w2c[:, :3].T + w2c[:, 3]
    uvz = cam @ K.T
    pz = uvz[:, 2] + 1e-8
    px, py = uvz[:, 0] / pz, uvz[:, 1] / pz
    inside = (px > -1) & (px < W) & (py > -1) & (py < H)
    u = np.clip(px, 0, W - 1).astype(np.int64)
    v = np.clip(py, 0, H - 1).astype(np.int64)
    limit = (g["cull_depth"][v, u] + F(g["cull_eps"])).astype(np.float64)

    def close(a, b):
        return np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b)) + 1e-300

    edge = close(px, 0) | close(px, W - 1) | close(py, 0) | close(py, H - 1) | close(pz, 0)
    return edge | (inside & (close(px, np.rint(px)) | close(py, np.rint(py)) | close(pz, limit)))


def test_cull_masks_equal_the_reference(gold):
    g = gold
    H, W = (int(x) for x in g["cull_HW"])
    w2c = eo.world_to_camera_f64(g["cull_c2w"])
    band = _decision_band(g)
    assert band.mean() <= 1e-4, int(band.sum())                     # the cap: at most 0.01 % of the vertices excluded
    fr, obs, inv = eo.cull_vertices(g["cull_vertices"], w2c, g["cull_K"], H, W, g["cull_depth"], g["cull_depth_gt"],
                                    float(g["cull_eps"]))
    print(f"excluded {int(band.sum())} of {band.size}; observed {int(obs.sum())}, invalid {int(inv.sum())}, "
          f"differing obs {int((obs != g['cull_obs'])[~band].sum())} inv {int((inv != g['cull_inv'])[~band].sum())}")
    assert np.array_equal(obs[~band], g["cull_obs"][~band])
    assert np.array_equal(inv[~band], g["cull_inv"][~band])
    assert obs.sum() > 2000 and inv.sum() > 1000 and (fr & ~obs).sum() > 2000
    _, obs2, inv2 = eo.cull_vertices(g["cull_vertices"], w2c, g["cull_K"], H, W, g["cull_depth"], None, float(g["cull_eps"]))
    assert np.array_equal(obs2[~band], g["cull_obs_keep_depth"][~band]) and not inv2.any()


def test_cull_nan_vertices_index_nothing():
    v = np.array([(np.nan, 0, 0), (0, 0, np.inf), (0, 0, 0), (0, 0, 5.0)], F)
    c2w = ro.look_at((0, -2.0, 0), up=(0, 0, 1))
    K = np.array([[50.0, 0, 16], [0, 50.0, 12], [0, 0, 1]])
    depth = np.full((24, 32), 2.0, F)
    fr, obs, inv = eo.cull_vertices(v, eo.world_to_camera_f64(c2w), K, 24, 32, depth, np.zeros((24, 32), F), 0.005)
    assert fr.tolist() == [False, False, True, False] and obs.tolist() == [False, False, True, False]
    assert inv.tolist() == [False, False, True, False]
    keep = eo.cull_triangles(np.array([(0, 1, 2), (2, 2, 3), (0, 1, 3), (2, 3, 7)]), 4, obs, np.zeros(4, bool))
    assert keep.tolist() == [True, True, False, False]              # an index outside [0, V) drops the triangle


def test_scores_equal_the_reference(gold):
    g = gold
    m = eo.point_metrics(g["score_rec"], g["score_gt"], float(g["score_dist_th"]))
    acc, comp = m["acc"] / 100, m["comp"] / 100
    print(f"acc {acc!r} vs {float(g['score_acc'])!r}; comp {comp!r} vs {float(g['score_comp'])!r}; "
          f"rel {abs(acc / g['score_acc'] - 1):.3g} {abs(comp / g['score_comp'] - 1):.3g}; ratio {m['comp ratio']}")
    assert abs(acc - g["score_acc"]) <= SCORE_TOL * g["score_acc"]
    assert abs(comp - g["score_comp"]) <= SCORE_TOL * g["score_comp"]
    # the reference's ratio is the float32 mean of a 0 / 1 array: the same count over the same length, rounded to fp32
    assert F(m["comp ratio"] / 100) == g["score_ratio"]
    assert 5 < m["comp ratio"] < 99.9


def test_depth_l1_equals_the_reference(gold):
    g = gold
    got = eo.depth_l1({f"depth_{i}": g["l1_pred"][i] for i in range(3)}, g["l1_gt"], g["l1_masks"])
    assert np.all(np.abs(got - g["l1_scores"]) <= 1e-12 * np.abs(g["l1_scores"])), (got, g["l1_scores"])
    assert np.all(got > 0.01)


def test_sampling_counts_planes_and_determinism():
    v, t = eo.mixed_area_mesh(ro.icosphere)
    area, q, cum = eo.area_weights(v, t)
    pos = area[area > 0]
    assert pos.max() / pos.min() > 1e4 and (q == 0).sum() >= 7
    assert np.all(np.abs(q * (2.0 ** -40) * 2.0 ** (int(area.max().view(np.uint32) >> 23) - 126) - area) <= 2.0 ** -40)
    n = 200000
    rng = np.random.default_rng(3)
    u = np.stack([(np.arange(n) + 0.5) / n, rng.random(n), rng.random(n)], 1).astype(F)
    pts, face = eo.sample_surface(v, t, u)
    counts = np.bincount(face, minlength=len(t))
    expected = n * q.astype(np.float64) / float(cum[-1])
    # a lattice of n points meets an interval of length L in floor(L) or ceil(L) points, +-1 for its ends and one more for the
    # rounding of (k + 1/2)/n to fp32 (2^-25 relative, below 1/n here only up to n = 2^24: n = 2 * 10^5 leaves room)
    assert np.all(np.abs(counts - expected) <= 1.0 + 1e-9), float(np.abs(counts - expected).max())
    assert np.all(counts[q == 0] == 0)
    a, b, c = (v[t[face, k]].astype(np.float64) for k in range(3))
    p = pts.astype(np.float64)
    nrm = np.cross(b - a, c - a)
    scale = np.linalg.norm(np.stack([a, b, c]), axis=(0, 2)).max()
    dist = np.abs(((p - a) * nrm).sum(1)) / np.linalg.norm(nrm, axis=1)
    assert dist.max() <= 8 * 2.0 ** -24 * scale, dist.max()
    # barycentrics in float64 from the two edge vectors
    e1, e2, w = b - a, c - a, p - a
    d11, d12, d22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    w1, w2 = (w * e1).sum(1), (w * e2).sum(1)
    det = d11 * d22 - d12 * d12
    r1, r2 = (d22 * w1 - d12 * w2) / det, (d11 * w2 - d12 * w1) / det
    big = area[face] > 1e-3                                          # on the small cap the edges are 10^-3: fp32 round-off / edge
    tol = np.where(big, 1e-5, 2e-3)
    assert np.all(r1 >= -tol) and np.all(r2 >= -tol) and np.all(r1 + r2 <= 1 + tol)
    pts2, face2 = eo.sample_surface(v, t, u)
    assert np.array_equal(pts, pts2) and np.array_equal(face, face2)


def test_sampling_edge_uniforms():
    v, t = ro.icosphere(1, 0.5)
    u = np.array([(0, 0, 0), (np.nextafter(F(1), F(0)), 0.9, 0.9), (1.0, 0.5, 0.5), (-0.5, 1, 0), (np.nan, 0.2, 0.3)], F)
    pts, face = eo.sample_surface(v, t, u)
    assert face.tolist() == [0, len(t) - 1, len(t) - 1, 0, 0]
    assert np.array_equal(pts[0], v[t[0, 0]]) and np.isfinite(pts).all()


def test_icp_recovers_a_known_motion():
    rng = np.random.default_rng(11)
    # a cloud filling a cube (mean spacing 0.09): on a smooth closed surface point-to-point ICP slides along the surface and
    # meets its stopping rule short of the motion, which says nothing about the arithmetic checked here
    target = rng.uniform(-0.5, 0.5, (1500, 3)).astype(F)
    motion = eo.rigid(np.radians(3.0), np.radians(-2.0), np.radians(4.0), (0.02, -0.01, 0.005))
    sub = np.sort(rng.choice(len(target), 300, replace=False))
    source = eo.transform_points(target[sub], motion)
    res = eo.icp_align(source, target, threshold=0.1)
    err = np.abs(res["transformation"] @ motion - np.eye(4)).max()
    print(f"iterations {res['iterations']} fitness {res['fitness']} rmse {res['inlier_rmse']:.3g} |T M - I| {err:.3g}")
    assert res["fitness"] == 1.0 and res["iterations"] < 30
    # the source points are the target's, moved and rounded to fp32 once (2^-24 relative of coordinates <= 0.55): at the
    # solution every correspondence is exact up to that rounding, and 300 points over a unit cube determine the motion
    # to the same order
    assert err <= 1e-6 and res["inlier_rmse"] <= 1e-6
    none = eo.icp_align(source + F(10), target, threshold=0.1)
    assert np.array_equal(none["transformation"], np.eye(4)) and none["fitness"] == 0 and none["iterations"] == 0


def test_nearest_rules():
    ref = np.array([(0, 0, 0), (1, 0, 0), (1, 0, 0), (np.nan, 0, 0), (np.inf, 0, 0), (3e38, 3e38, 0)], F)
    q = np.array([(0.9, 0, 0), (0, 0, 0), (np.nan, 0, 0), (0.4, 0, 0), (-3e38, -3e38, 0)], F)
    idx, d2 = eo.nearest(q, ref)
    assert idx.tolist() == [1, 0, -1, 0, -1]                         # the last query overflows every d2
    assert d2[1] == 0 and np.isinf(d2[2]) and np.isinf(d2[4]) and d2[0] == (F(0.9) - F(1)) * (F(0.9) - F(1))
    idx, d2 = eo.nearest(q, ref, max_dist=0.3)
    assert idx.tolist() == [1, 0, -1, -1, -1] and np.isinf(d2[3])
    idx, _ = eo.nearest(q, ref[:0])
    assert idx.tolist() == [-1] * 5 and eo.nearest(q[:0], ref)[0].shape == (0,)


def test_nearest_equals_the_kd_tree():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(5)
    ref = rng.uniform(-1, 1, (20000, 3)).astype(F)
    q = rng.uniform(-1, 1, (4096, 3)).astype(F)
    idx, d2 = eo.nearest(q, ref)
    dist, kd = spatial.cKDTree(ref.astype(np.float64)).query(q.astype(np.float64), k=2)
    clear = dist[:, 1] - dist[:, 0] > SCORE_TOL * dist[:, 1]
    assert clear.mean() > 0.99
    assert np.array_equal(idx[clear], kd[clear, 0])
    rel = np.abs(np.sqrt(d2.astype(np.float64)) - dist[:, 0]) / dist[:, 0]
    print(f"clear {int(clear.sum())} of {len(q)}; worst relative distance error {rel.max():.3g}")
    assert rel.max() <= SCORE_TOL / 2


def test_argument_validation_without_gpu(lib):
    """status codes, never exceptions or launches: 1 for bad arguments, 0 for empty inputs"""
    inf = float("inf")
    assert lib.mh_nn_workspace_bytes(10) == 80 and lib.mh_nn_workspace_bytes(-1) == -1 and lib.mh_nn_workspace_bytes(1 << 31) == -1
    assert lib.mh_nn_tile_points() >= 64 and lib.mh_icp_workspace_bytes() > 0
    assert lib.mh_nn_search(None, 0, None, 5, inf, 0, None, None, None, None) == 0
    assert lib.mh_nn_search(None, 5, None, 5, inf, 0, None, None, None, None) == 1
    assert lib.mh_nn_search(None, 0, None, 0, float("nan"), 0, None, None, None, None) == 1
    assert lib.mh_nn_search(None, 0, None, 0, -1.0, 0, None, None, None, None) == 1
    assert lib.mh_nn_search(None, 0, None, 0, inf, 5000, None, None, None, None) == 1
    assert lib.mh_nn_search(None, -1, None, 0, inf, 0, None, None, None, None) == 1
    import ctypes
    w2c = (ctypes.c_double * 12)()
    K = (ctypes.c_double * 9)()
    assert lib.mh_cull_vertices(None, 0, w2c, K, 4, 4, None, None, 0.005, None, None, None, None) == 0
    assert lib.mh_cull_vertices(None, 3, w2c, K, 4, 4, None, None, 0.005, None, None, None, None) == 1
    assert lib.mh_cull_vertices(None, 0, None, K, 4, 4, None, None, 0.005, None, None, None, None) == 1
    assert lib.mh_cull_vertices(None, 0, w2c, K, 0, 4, None, None, 0.005, None, None, None, None) == 1
    assert lib.mh_cull_vertices(None, 0, w2c, K, 4, 20000, None, None, 0.005, None, None, None, None) == 1
    assert lib.mh_cull_triangles(None, 0, 5, None, None, None, None) == 0
    assert lib.mh_cull_triangles(None, 2, 5, None, None, None, None) == 1
    assert lib.mh_mesh_area_weights(None, 5, None, 0, None, None, None) == 0
    assert lib.mh_mesh_area_weights(None, 5, None, 2, None, None, None) == 1
    assert lib.mh_sample_surface(None, 5, None, 2, None, None, 0, None, None, None) == 0
    assert lib.mh_sample_surface(None, 5, None, 2, None, None, 3, None, None, None) == 1
    assert lib.mh_sample_surface(None, 5, None, -1, None, None, 0, None, None, None) == 1
    assert lib.mh_icp_transform(None, 0, w2c, None, None) == 0
    assert lib.mh_icp_transform(None, 0, None, None, None) == 1
    assert lib.mh_icp_transform(None, 4, w2c, None, None) == 1
    assert lib.mh_icp_sums(None, 0, None, 0, None, None, None, None, None) == 0
    assert lib.mh_icp_sums(None, 4, None, 0, None, None, None, None, None) == 1


def test_module_refuses_cpu_tensors_and_bad_shapes(lib):
    import torch
    from morpheus_amd import mesheval
    from morpheus_amd._lib import MorpheusHipError
    p = torch.zeros(4, 3)
    with pytest.raises(MorpheusHipError):
        mesheval.nearest(p, p)
    with pytest.raises(MorpheusHipError):
        mesheval.sample_surface(p, torch.zeros(2, 3, dtype=torch.int64), 10)
    with pytest.raises(MorpheusHipError):
        mesheval.icp_align(p, p)
    with pytest.raises(MorpheusHipError):
        mesheval.cull_mesh(p, torch.zeros(2, 3, dtype=torch.int64), c2w=np.eye(4), K=np.eye(3), H=4, W=4,
                           depth_gt=torch.zeros(4, 4))
    # eval_depth_l1 is host arithmetic: the fixture's stacks give the golden scores
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "eval3d.npz")))
    got = mesheval.eval_depth_l1({f"depth_{i}": g["l1_pred"][i] for i in range(3)}, g["l1_gt"], g["l1_masks"])
    assert np.all(np.abs(got - g["l1_scores"]) <= 1e-12 * g["l1_scores"])
