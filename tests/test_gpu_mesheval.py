"""GPU: the mesh evaluation (csrc/mesheval.hip, morpheus_amd.mesheval) against the numpy restatement tests/mesheval_oracle.py --
nearest neighbours, cull masks, compacted meshes, sampled points and cumulative areas bit for bit; the ICP sums to float64
round-off; the scores to 2^-21 relative; determinism; model -> mesh -> cull -> scores end to end."""
import os

import numpy as np
import pytest
import torch

from tests import mc_oracle as mo
from tests import mesheval_oracle as eo
from tests import raster_oracle as ro

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SCORE_TOL = 2.0 ** -21


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _nearest_same(q, r, max_dist=None, segments=0):
    from morpheus_amd import mesheval
    idx, d2 = mesheval.nearest(_dev(q, F), _dev(r, F), max_dist=max_dist, segments=segments)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (len(q),)
    oi, od = eo.nearest(q, r, max_dist=max_dist)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    assert np.array_equal(idx, oi), (int((idx != oi).sum()), len(q), len(r), segments)
    assert np.array_equal(_bits(d2), _bits(od))
    return idx, d2


def test_nearest_bit_identical_around_every_boundary():
    from morpheus_amd import _lib
    tile = _lib.load().mh_nn_tile_points()
    rng = np.random.default_rng(1)
    pool_q = rng.uniform(-1, 1, (2 * 256 + 1, 3)).astype(F)
    pool_r = rng.uniform(-1, 1, (3 * tile + 5, 3)).astype(F)
    # queries: one, a wavefront, a workgroup (-1, =, +1); references: one, four (the inner loop's step), a tile, several tiles
    for nq in (1, 63, 64, 65, 255, 256, 257, 513):
        for nr in (1, 3, 4, 5, tile - 1, tile, tile + 1):
            _nearest_same(pool_q[:nq], pool_r[:nr])
    # segments: lengths one less / equal / one more than a tile, a last segment shorter than the others, more segments than tiles
    for nr in (2 * tile - 2, 2 * tile, 2 * tile + 2, 3 * tile + 5):
        for seg in (1, 2, 3, 7, 64):
            _nearest_same(pool_q[:130], pool_r[:nr], segments=seg)
    _nearest_same(pool_q[:70], pool_r[:9], segments=4096)          # more segments than points


def test_nearest_large_once():
    rng = np.random.default_rng(2)
    q = rng.uniform(-1, 1, (50000, 3)).astype(F)
    r = rng.uniform(-1, 1, (20000, 3)).astype(F)
    idx, d2 = _nearest_same(q, r)
    assert (idx >= 0).all() and d2.max() < 0.1


def test_nearest_rules():
    rng = np.random.default_rng(3)
    r = rng.uniform(-1, 1, (3000, 3)).astype(F)
    r[1500:] = r[:1500]                                             # every point twice: the lower index wins
    q = np.concatenate([rng.uniform(-1, 1, (200, 3)).astype(F), r[700:900]])       # 200 queries that are reference points
    idx, d2 = _nearest_same(q, r)
    assert (idx < 1500).all() and (d2[200:] == 0).all() and np.array_equal(idx[200:], np.arange(700, 900))
    _nearest_same(q, r, segments=5)
    # max_dist cutting some and all candidates
    idx, d2 = _nearest_same(q[:200], r, max_dist=0.08)
    assert 0 < (idx < 0).sum() < 200 and np.isinf(d2[idx < 0]).all()
    idx, _ = _nearest_same(q[:200] + F(5), r, max_dist=0.08)
    assert (idx < 0).all()
    idx, _ = _nearest_same(q, r, max_dist=0.0)                      # only exact hits survive
    assert (idx[200:] >= 0).all()
    # NaN and infinite coordinates on either side; overflowing distances
    r2, q2 = r.copy(), q.copy()
    r2[::7, 0] = np.nan
    r2[3::11, 1] = np.inf
    r2[5::13] = F(3e38)
    q2[::5, 2] = np.nan
    q2[1::9, 0] = -np.inf
    q2[2::17] = F(-3e38)
    idx, _ = _nearest_same(q2, r2)
    assert (idx[::5] == -1).all() and (idx[1::9] == -1).all() and (idx >= 0).sum() > 100
    _nearest_same(q2, r2, max_dist=0.1, segments=3)
    # empty sides
    idx, d2 = _nearest_same(q, r[:0])
    assert (idx == -1).all() and np.isinf(d2).all()
    _nearest_same(q[:0], r)


def test_nearest_same_bytes_and_permutation():
    from morpheus_amd import mesheval
    g = torch.Generator(device=DEV)
    g.manual_seed(4)
    q = torch.rand(20000, 3, generator=g, device=DEV) * 2 - 1
    r = torch.rand(30000, 3, generator=g, device=DEV) * 2 - 1       # distinct points: ties have probability ~0, checked below
    a = mesheval.nearest(q, r)
    b = mesheval.nearest(q, r)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = mesheval.nearest(q, r, segments=1)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    perm = torch.randperm(r.shape[0], generator=g, device=DEV)
    p = mesheval.nearest(q, r[perm].contiguous())
    assert torch.equal(p[1], a[1])
    back = perm[p[0].long()].to(torch.int32)
    moved = back != a[0]
    if bool(moved.any()):                                           # a tie in d2 between two reference points: both are minimal
        qq, rr = q[moved].cpu().numpy(), r.cpu().numpy()
        for k, (i, j) in enumerate(zip(back[moved].cpu().numpy(), a[0][moved].cpu().numpy())):
            assert _bits(eo.pair_d2(qq[k:k + 1], rr[i:i + 1])) == _bits(eo.pair_d2(qq[k:k + 1], rr[j:j + 1]))
    print(f"winner changed for {int(moved.sum())} of {q.shape[0]} queries")


# ---- culling -------------------------------------------------------------------------------------------------------------

def _torus_mesh():
    shape = (48, 52, 30)
    v, t = mo.marching_cubes(mo.torus(shape, (23.6, 25.2, 14.3), 14.5, 6.2))
    return ro.to_unit_box(v, shape), t


def _cull_same(v, t, c2w, K, H, W, colors=None, depth_gt=None, remove_missing_depth=True):
    from morpheus_amd import meshrender, mesheval
    vd, td, cd = _dev(v, F), _dev(t, np.int64), _dev(colors, F)
    depth = meshrender.render_mesh(vd, td, c2w=c2w, K=K, H=H, W=W, convention="opengl", mode="color")["depth"]
    out = mesheval.cull_mesh(vd, td, cd, c2w=c2w, K=K, H=H, W=W, depth_gt=_dev(depth_gt, F),
                             remove_missing_depth=remove_missing_depth, return_masks=True)
    out2 = mesheval.cull_mesh(vd, td, cd, c2w=c2w, K=K, H=H, W=W, depth_gt=_dev(depth_gt, F),
                              remove_missing_depth=remove_missing_depth, rendered_depth=depth)
    ref = eo.cull_mesh(v, t, colors, c2w, K, H, W, depth.cpu().numpy(), depth_gt, 0.005, remove_missing_depth)
    for k in ("frustum", "observed", "invalid", "keep"):
        assert out[k].dtype == torch.bool
        assert np.array_equal(out[k].cpu().numpy(), ref[k]), k
    assert out["triangles"].dtype == torch.int64
    for k in ("vertices", "triangles", "colors"):
        if ref[k] is None:
            assert out[k] is None
        else:
            assert np.array_equal(out[k].cpu().numpy(), ref[k]), k
            assert torch.equal(out[k], out2[k])
    print(f"V {len(v)} T {len(t)}: frustum {int(ref['frustum'].sum())} observed {int(ref['observed'].sum())} "
          f"invalid {int(ref['invalid'].sum())} kept {int(ref['keep'].sum())} -> V' {len(ref['vertices'])}")
    return ref


def _holes(H, W, value=2.0):
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.where(((ii // 16) + (jj // 16)) % 2 == 0, F(value), F(0)).astype(F)


def test_cull_mesh_bit_identical():
    H, W = 240, 320
    K = np.array([[300.0, 0.7, 158.3], [0, 295.0, 121.9], [0, 0, 1]])            # a full 3 x 3 K, skew included
    rng = np.random.default_rng(6)
    for v, t, c2w in ((*ro.icosphere(4, 0.6), ro.look_at((1.9, 1.2, 0.9))),
                      (*_torus_mesh(), ro.look_at((0.3, -2.2, 1.6), target=(-0.05, 0, -0.4)))):
        colors = rng.random(v.shape).astype(F)
        ref = _cull_same(v, t, c2w, K, H, W, colors, _holes(H, W))
        assert 0 < ref["keep"].sum() < len(t) and ref["invalid"].sum() > 0 and len(ref["vertices"]) < len(v)
        ref2 = _cull_same(v, t, c2w, K, H, W, None, None, remove_missing_depth=False)
        assert not ref2["invalid"].any() and ref2["keep"].sum() > ref["keep"].sum()
    # the camera inside the mesh: every vertex in the frustum is a back face seen from inside
    v, t = ro.icosphere(3, 0.9)
    ref = _cull_same(v, t, ro.look_at((0.1, -0.05, 0.1), target=(1, 0.3, 0.2)), K, H, W, None, _holes(H, W))
    assert ref["keep"].sum() > 0
    # a mesh wholly outside the frustum: an empty result, no error
    v, t = ro.icosphere(2, 0.3)
    ref = _cull_same(v, t, ro.look_at((2.0, 0, 0), target=(4.0, 0, 0)), K, H, W, rng.random(v.shape).astype(F), _holes(H, W))
    assert ref["keep"].sum() == 0 and ref["vertices"].shape == (0, 3) and ref["triangles"].shape == (0, 3)


def test_cull_mesh_on_the_reference_fixture():
    from morpheus_amd import mesheval
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "eval3d.npz")))
    H, W = (int(x) for x in g["cull_HW"])
    v = g["cull_vertices"]
    t = np.arange(3 * (len(v) // 3)).reshape(-1, 3)                 # any triangles: the vertex masks are what is compared
    out = mesheval.cull_mesh(_dev(v), _dev(t), c2w=g["cull_c2w"], K=g["cull_K"], H=H, W=W, depth_gt=_dev(g["cull_depth_gt"]),
                             rendered_depth=_dev(g["cull_depth"]), eps=float(g["cull_eps"]), return_masks=True)
    fr, obs, inv = eo.cull_vertices(v, eo.world_to_camera_f64(g["cull_c2w"]), g["cull_K"], H, W, g["cull_depth"],
                                    g["cull_depth_gt"], float(g["cull_eps"]))
    assert np.array_equal(out["observed"].cpu().numpy(), obs) and np.array_equal(out["invalid"].cpu().numpy(), inv)
    assert np.array_equal(out["frustum"].cpu().numpy(), fr)


# ---- sampling ------------------------------------------------------------------------------------------------------------

def test_sample_surface_bit_identical():
    from morpheus_amd import mesheval
    rng = np.random.default_rng(8)
    for v, t in (eo.mixed_area_mesh(ro.icosphere), _torus_mesh()):
        n = 100003
        u = rng.random((n, 3)).astype(F)
        u[:4] = [(0, 0, 0), (np.nextafter(F(1), F(0)), 0.9, 0.9), (1.0, 0.5, 0.5), (np.nan, 0.25, 0.5)]
        areas, cum = mesheval.area_weights(_dev(v, F), _dev(t, np.int64))
        oa, _, ocum = eo.area_weights(v, t)
        assert np.array_equal(_bits(areas.cpu().numpy()), _bits(oa))
        assert cum.dtype == torch.int64 and np.array_equal(cum.cpu().numpy(), ocum)
        pts, face = mesheval.sample_surface(_dev(v, F), _dev(t, np.int64), n, uniforms=_dev(u))
        opts, oface = eo.sample_surface(v, t, u)
        assert face.dtype == torch.int32 and np.array_equal(face.cpu().numpy(), oface)
        assert np.array_equal(_bits(pts.cpu().numpy()), _bits(opts))
    a = mesheval.sample_surface(_dev(v, F), _dev(t, np.int64), 5000, seed=3)
    b = mesheval.sample_surface(_dev(v, F), _dev(t, np.int64), 5000, seed=3)
    c = mesheval.sample_surface(_dev(v, F), _dev(t, np.int64), 5000, seed=4)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])
    from morpheus_amd._lib import MorpheusHipError
    with pytest.raises(MorpheusHipError):
        mesheval.sample_surface(_dev(v, F), _dev(t[:0], np.int64), 10)
    with pytest.raises(MorpheusHipError):
        mesheval.sample_surface(_dev(v, F), _dev(np.array([(0, 0, 1), (2, 2, 2)]), np.int64), 10)      # zero total area


# ---- alignment -----------------------------------------------------------------------------------------------------------

def _icp_clouds():
    rng = np.random.default_rng(11)
    target = rng.uniform(-0.5, 0.5, (6000, 3)).astype(F)
    motion = eo.rigid(np.radians(1.5), np.radians(-1.0), np.radians(2.0), (0.01, -0.005, 0.004))
    source = eo.transform_points(target[np.sort(rng.choice(len(target), 2500, replace=False))], motion)
    source[::50] += F(3.0)                                          # some points without a correspondence
    return source, target, motion


def test_icp_sums_and_transform():
    from morpheus_amd import mesheval
    source, target, motion = _icp_clouds()
    T0 = eo.rigid(0.01, 0.02, -0.01, (0.003, 0.001, -0.002))
    moved = mesheval.transform_points(_dev(source), T0)
    assert np.array_equal(_bits(moved.cpu().numpy()), _bits(eo.transform_points(source, T0)))
    idx, d2 = mesheval.nearest(moved, _dev(target), max_dist=0.1)
    sums = mesheval.icp_sums(moved, _dev(target), idx, d2)
    sums2 = mesheval.icp_sums(moved, _dev(target), idx, d2)
    assert sums.dtype == torch.float64 and torch.equal(sums, sums2)
    terms = eo.icp_terms(moved.cpu().numpy(), target, idx.cpu().numpy(), d2.cpu().numpy())
    want, scale = terms.sum(axis=0), np.abs(terms).sum(axis=0)
    got = sums.cpu().numpy()
    print("relative to sum |terms|:", np.abs(got - want) / scale)
    assert got[0] == want[0] == (idx >= 0).sum().item() and 0 < got[0] < len(source)
    assert np.all(np.abs(got - want) <= 1e-12 * scale)


def test_icp_align_equals_the_oracle():
    from morpheus_amd import mesheval
    source, target, motion = _icp_clouds()
    res = mesheval.icp_align(_dev(source), _dev(target), threshold=0.1)
    ref = eo.icp_align(source, target, threshold=0.1)
    diff = np.abs(res["transformation"] - ref["transformation"]).max()
    print(f"iterations {res['iterations']} / {ref['iterations']}, fitness {res['fitness']}, rmse {res['inlier_rmse']:.3g}, "
          f"|T - T_oracle| {diff:.3g}, |T M - I| {np.abs(res['transformation'] @ motion - np.eye(4)).max():.3g}")
    assert res["transformation"].dtype == np.float64 and res["transformation"].shape == (4, 4)
    assert res["iterations"] == ref["iterations"] and diff <= 1e-9
    assert abs(res["fitness"] - ref["fitness"]) <= 1e-12 and abs(res["inlier_rmse"] - ref["inlier_rmse"]) <= 1e-9
    assert np.abs(res["transformation"] @ motion - np.eye(4)).max() <= 1e-6
    again = mesheval.icp_align(_dev(source), _dev(target), threshold=0.1)
    assert again["transformation"].tobytes() == res["transformation"].tobytes() and again["iterations"] == res["iterations"]
    none = mesheval.icp_align(_dev(source + F(10)), _dev(target))
    assert np.array_equal(none["transformation"], np.eye(4)) and none["fitness"] == 0.0


# ---- end to end ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    from morpheus_amd import harness
    return harness.build_model("b", DEV)


def _close_scores(got, want, band_points, n_gt):
    for k in ("acc", "comp"):
        assert abs(got[k] - want[k]) <= SCORE_TOL * want[k], (k, got[k], want[k])
    assert abs(got["comp ratio"] - want["comp ratio"]) <= 100.0 * band_points / n_gt + 1e-9, (got["comp ratio"], want["comp ratio"])


def test_model_to_scores_end_to_end(model, tmp_path):
    from morpheus_amd import mesh, meshrender, mesheval
    H, W = 120, 160
    K = np.array([[150.0, 0, 80.0], [0, 150.0, 60.0], [0, 0, 1]])
    c2w = ro.look_at((2.2, 0.8, 0.7))
    m = mesh.extract_mesh(model, resolution=128, S=128, t=25 / 200)
    depth_gt = torch.full((H, W), 2.0, device=DEV)
    depth_gt[:, :40] = 0
    culled = mesheval.cull_mesh(m["vertices"], m["triangles"], m["colors"], c2w=c2w, K=K, H=H, W=W, depth_gt=depth_gt)
    assert 0 < culled["triangles"].shape[0] < m["triangles"].shape[0]
    motion = eo.rigid(np.radians(1.0), np.radians(-0.8), np.radians(1.2), (0.01, -0.006, 0.004))
    gt = {"vertices": mesheval.transform_points(culled["vertices"], motion), "triangles": culled["triangles"]}
    n = 20000
    rng = np.random.default_rng(21)
    ur, ug = rng.random((n, 3)).astype(F), rng.random((n, 3)).astype(F)
    host = lambda d: {k: None if x is None else x.cpu().numpy() for k, x in d.items()}      # noqa: E731
    scores = {}
    for align in (False, True):
        got = mesheval.mesh_metrics(culled, gt, align=align, uniforms_rec=_dev(ur), uniforms_gt=_dev(ug))
        want = eo.mesh_metrics(host(culled), host(gt), ur, ug, align=align)
        d = want["d_comp"]
        band = int(((d > 0.05 * (1 - SCORE_TOL)) & (d < 0.05 * (1 + SCORE_TOL))).sum())
        print(f"align={align}: {got} oracle acc {want['acc']!r} comp {want['comp']!r} ratio {want['comp ratio']!r} band {band}")
        _close_scores(got, want, band, n)
        scores[align] = got
    assert scores[True]["acc"] < scores[False]["acc"] and scores[True]["comp"] < scores[False]["comp"]
    # a ground-truth point cloud is used as it is; PLY paths are read
    cloud = mesheval.mesh_metrics(culled, {"vertices": gt["vertices"], "triangles": None}, align=False, uniforms_rec=_dev(ur))
    assert cloud["acc"] > 0 and np.isfinite(cloud["comp"])
    mesh.write_ply(str(tmp_path / "rec.ply"), culled["vertices"], culled["triangles"], culled["colors"])
    mesh.write_ply(str(tmp_path / "gt.ply"), gt["vertices"], gt["triangles"])
    files = mesheval.mesh_metrics(str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), align=False, uniforms_rec=_dev(ur),
                                  uniforms_gt=_dev(ug))
    assert files == scores[False]

    # eval_mesh over three frames from mesh dicts: one line in the reference's format
    poses = [ro.look_at((2.2 * np.cos(a), 2.2 * np.sin(a), 0.7)) for a in (0.0, 0.7, 1.4)]
    meshes = [mesh.extract_mesh(model, resolution=64, S=64, t=f / 200) for f in (0, 25, 50)]
    gts = [{"vertices": mesheval.transform_points(x["vertices"], motion), "triangles": x["triangles"]} for x in meshes]
    dgt = [torch.full((H, W), 2.0, device=DEV)] * 3
    save = tmp_path / "metric_3d.txt"
    out = mesheval.eval_mesh(meshes, gts, poses, K, H, W, dgt, save_file=str(save), epoch=7, num_points=5000)
    assert out["frames"] == [0, 1, 2] and len(out["acc"]) == 3 and np.isfinite(out["acc"] + out["comp"]).all()
    line = save.read_text()
    assert line == "Ep_7:\t Acc:{}\t Comp:{}\n".format(np.array(out["acc"]).mean(), np.array(out["comp"]).mean())

    # eval_depth_l1: render_all_meshes' output against itself and against the fixture's stacks
    depths = meshrender.render_all_meshes(meshes, poses, K, H, W, scale=1)
    stack = np.stack([depths[f"depth_{i}"] for i in range(3)])
    assert (stack > 0).any()
    same = mesheval.eval_depth_l1(depths, stack, np.ones_like(stack))
    assert same.tolist() == [0.0, 0.0, 0.0]                        # no pixel has an error in (0, 1]
    shifted = mesheval.eval_depth_l1(depths, np.where(stack > 0, stack + F(0.25), 0), np.ones_like(stack), save_dir=str(tmp_path))
    assert np.all(np.abs(shifted - 0.25) < 1e-6) and not np.isnan(shifted).any()
    assert (tmp_path / "depthL1_scores.txt").read_text().split() == ["0.25000"] * 3
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "eval3d.npz")))
    np.savez(str(tmp_path / "depths.npz"), **{f"depth_{i}": g["l1_pred"][i] for i in range(3)})
    got = mesheval.eval_depth_l1(str(tmp_path / "depths.npz"), g["l1_gt"], g["l1_masks"])
    assert np.all(np.abs(got - g["l1_scores"]) <= 1e-12 * g["l1_scores"])
