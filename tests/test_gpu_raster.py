"""GPU: the HIP rasteriser (csrc/raster.hip, morpheus_amd.meshrender) against the numpy restatement tests/raster_oracle.py --
depth, tri_id, the clipped count and the fixed-point vertex-normal sums bit for bit; the float outputs by the error rule
(HIP's error against float64 <= 3 x the numpy-fp32 restatement's own, floor 2^-22); shared edges; the ray generator's
conventions; determinism; model -> mesh -> depths.npz end to end."""
import os

import numpy as np
import pytest
import torch

from tests import mc_oracle as mo
from tests import raster_oracle as ro

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FLOOR = 2.0 ** -22


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _render(v, t, c2w, K, H, W, colors=None, normals=None, **kw):
    from morpheus_amd import meshrender
    out = meshrender.render_mesh(_dev(v, np.float32), _dev(t, np.int64), _dev(colors), _dev(normals), c2w=c2w, fx=K[0], fy=K[1],
                                 cx=K[2], cy=K[3], H=H, W=W, **kw)
    assert out["depth"].dtype == torch.float32 and out["depth"].shape == (H, W)
    assert out["tri_id"].dtype == torch.int32 and out["tri_id"].shape == (H, W)
    assert out["image"].dtype == torch.float32 and out["image"].shape == (H, W, 3)
    assert out["clipped"].dtype == torch.int64 and out["clipped"].dim() == 0
    return {k: x.cpu().numpy() for k, x in out.items()}


def _same_as_oracle(v, t, c2w, K, H, W, near=0.01, convention="opengl", **kw):
    out = _render(v, t, c2w, K, H, W, near=near, convention=convention, mode="color", **kw)
    keys, clipped = ro.rasterize(v, t, ro.world_to_camera(c2w, convention), *K, H, W, near)
    depth, tri_id = ro.decode(keys)
    covered = int((tri_id >= 0).sum())
    print(f"{H}x{W} T={len(t)} covered={covered} clipped={clipped}")
    assert np.array_equal(out["tri_id"], tri_id), int((out["tri_id"] != tri_id).sum())
    assert np.array_equal(out["depth"].view(np.uint32), depth.view(np.uint32))
    assert int(out["clipped"]) == clipped
    assert np.array_equal(out["image"][tri_id < 0], np.ones((H * W - covered, 3), np.float32))
    return out, covered, clipped


def _mc_mesh(vol, shape):
    v, t = mo.marching_cubes(vol)
    return ro.to_unit_box(v, shape), t


def _centre_K(H, W, f):
    return (float(f), float(f), W / 2.0, H / 2.0)


@pytest.mark.parametrize("H,W", [(1, 1), (37, 53), (768, 1024)])
def test_icosphere_bit_identical(H, W):
    v, t = ro.icosphere(3, 0.8)
    _, covered, clipped = _same_as_oracle(v, t, ro.look_at((1.9, 1.2, 0.9)), _centre_K(H, W, 0.9 * max(H, W)), H, W)
    assert covered > 0 and clipped == 0


def test_marching_cubes_meshes_bit_identical():
    H, W = 768, 1024
    shape = (48, 52, 30)
    v, t = _mc_mesh(mo.torus(shape, (23.6, 25.2, 14.3), 14.5, 6.2), shape)
    _, covered, _ = _same_as_oracle(v, t, ro.look_at((0.3, -2.2, 1.6), target=(-0.05, 0, -0.4)), _centre_K(H, W, 900.0), H, W)
    assert covered > 100000
    shape = (40, 36, 44)
    v, t = _mc_mesh(mo.gaussians(shape, np.random.default_rng(5)), shape)
    _, covered, _ = _same_as_oracle(v, t, ro.look_at((2.1, 1.4, 0.8)), (700.0, 690.0, 500.3, 390.8), H, W)
    assert covered > 50000


def test_noise_mesh_bit_identical():
    """white noise: slivers, degenerate and sub-pixel triangles, NaN corners"""
    rng = np.random.default_rng(7)
    shape = (23, 19, 27)
    vol = rng.normal(size=shape).astype(np.float32)
    vol[rng.random(shape) < 0.02] = np.nan
    v, t = _mc_mesh(vol, shape)
    assert len(t) > 5000
    _same_as_oracle(v, t, ro.look_at((1.7, -1.9, 1.1)), _centre_K(240, 320, 330.0), 240, 320)
    _same_as_oracle(v, t, ro.look_at((0.2, 0.1, 0.05), target=(1, 0.3, 0.2)), _centre_K(240, 320, 150.0), 240, 320)   # inside it


def test_camera_inside_a_large_sphere_sees_back_faces():
    v, t = ro.icosphere(3, 3.0)
    H, W = 240, 320
    out, covered, clipped = _same_as_oracle(v, t, ro.look_at((0.4, -0.3, 0.2), target=(3, 1, 0.5)), _centre_K(H, W, 200.0), H, W)
    assert covered == H * W and clipped > 0                   # the half of the sphere behind the camera is dropped and counted


def test_mesh_partly_behind_near():
    v, t = ro.icosphere(3, 0.8)
    H, W = 200, 260
    c2w = ro.look_at((0.9, 0.2, 0.1), target=(0, 0, 0))       # 0.12 outside the surface; near = 0.5 cuts into the sphere
    out, covered, clipped = _same_as_oracle(v, t, c2w, _centre_K(H, W, 180.0), H, W, near=0.5)
    assert clipped > 0 and covered > 0
    _, _, clipped_far = _same_as_oracle(v, t, c2w, _centre_K(H, W, 180.0), H, W, near=0.05)
    assert clipped_far == 0


def test_full_screen_quad_takes_the_large_triangle_path():
    H, W = 768, 1024
    v = np.array([(-9, -7, 2), (9, -7, 2.5), (9, 7, 3), (-9, 7, 2.5)], np.float32)
    t = np.array([(0, 1, 2), (0, 2, 3)], np.int64)
    c2w = ro.cv2gl_pose(np.eye(4))
    out, covered, _ = _same_as_oracle(v, t, c2w, _centre_K(H, W, 600.0), H, W)
    assert covered == H * W
    for small_area in (1, 1 << 30):                            # everything queued / everything per lane: the same bytes
        again = _render(v, t, c2w, _centre_K(H, W, 600.0), H, W, mode="color", small_area=small_area)
        assert np.array_equal(again["depth"].view(np.uint32), out["depth"].view(np.uint32))
        assert np.array_equal(again["tri_id"], out["tri_id"])


def test_small_area_does_not_change_the_result():
    v, t = ro.icosphere(3, 0.8)
    H, W = 300, 400
    c2w, K = ro.look_at((1.9, 1.2, 0.9)), _centre_K(300, 400, 380.0)
    base = _render(v, t, c2w, K, H, W, mode="color")
    for small_area in (1, 16, 100000):
        out = _render(v, t, c2w, K, H, W, mode="color", small_area=small_area)
        assert np.array_equal(out["depth"].view(np.uint32), base["depth"].view(np.uint32))
        assert np.array_equal(out["tri_id"], base["tri_id"])


def test_empty_mesh_gives_the_background():
    out = _render(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), ro.look_at((1, 1, 1)), _centre_K(9, 11, 10.0), 9, 11,
                  background=(0.25, 0.5, 0.75))
    assert (out["depth"] == 0).all() and (out["tri_id"] == -1).all() and int(out["clipped"]) == 0
    assert np.array_equal(out["image"], np.broadcast_to(np.array([0.25, 0.5, 0.75], np.float32), (9, 11, 3)))
    v, _ = ro.icosphere(1)
    out = _render(v, np.zeros((0, 3), np.int64), ro.look_at((1, 1, 1)), _centre_K(9, 11, 10.0), 9, 11)
    assert (out["tri_id"] == -1).all() and (out["image"] == 1).all()


def test_opengl_and_opencv_poses_give_the_same_bytes():
    v, t = ro.icosphere(3, 0.8)
    H, W = 120, 160
    gl = ro.look_at((1.9, 1.2, 0.9))
    a = _render(v, t, gl, _centre_K(H, W, 150.0), H, W, convention="opengl")
    b = _render(v, t, ro.cv2gl_pose(gl), _centre_K(H, W, 150.0), H, W, convention="opencv")
    for k in ("depth", "tri_id", "image", "clipped"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["tri_id"] >= 0).sum() > 1000


def _meshes_for_normals():
    yield ro.icosphere(3, 0.8)
    shape = (48, 52, 30)
    yield _mc_mesh(mo.torus(shape, (23.6, 25.2, 14.3), 14.5, 6.2), shape)
    shape = (40, 36, 44)
    yield _mc_mesh(mo.gaussians(shape, np.random.default_rng(5)), shape)
    rng = np.random.default_rng(7)
    yield _mc_mesh(rng.normal(size=(23, 19, 27)).astype(np.float32), (23, 19, 27))
    v, t = ro.icosphere(2, 1e-12)                              # tiny: the grid follows the mesh's scale
    yield v, t


def test_vertex_normal_sums_bit_identical():
    from morpheus_amd import meshrender
    for v, t in _meshes_for_normals():
        nrm, acc = meshrender.vertex_normal_sums(_dev(v), _dev(t))
        acc = acc.cpu().numpy()
        sums, bits, want = ro.vertex_normal_sums(v, t)
        assert np.array_equal(acc[:-1].reshape(-1, 3), sums)
        assert int(acc[-1]) == int(bits)
        # normalised normals: the error rule against float64 normalisation of the same sums
        f64 = ro._normalize(sums.astype(np.float64), np.float64)
        err_hip = np.abs(nrm.cpu().numpy().astype(np.float64) - f64).max()
        err_np = np.abs(want.astype(np.float64) - f64).max()
        print(f"V={len(v)} normals: HIP {err_hip:.3e} numpy-fp32 {err_np:.3e}")
        assert err_hip <= max(3 * err_np, FLOOR)
        perm = np.random.default_rng(1).permutation(len(t))
        nrm2, acc2 = meshrender.vertex_normal_sums(_dev(v), _dev(t[perm]))
        assert torch.equal(acc2.cpu(), torch.from_numpy(acc)) and torch.equal(nrm2, nrm)
    # a vertex without triangles, and no triangles at all
    v, t = ro.icosphere(1)
    lone = np.concatenate([v, [[5, 5, 5]]]).astype(np.float32)
    assert np.array_equal(meshrender.vertex_normals(_dev(lone), _dev(t))[-1].cpu().numpy(), [0, 0, 1])
    none = meshrender.vertex_normals(_dev(v), _dev(np.zeros((0, 3), np.int64)))
    assert np.array_equal(none.cpu().numpy(), np.broadcast_to(np.array([0, 0, 1], np.float32), v.shape))


@pytest.mark.parametrize("mode", ["color", "normal", "shaded"])
@pytest.mark.parametrize("with_colors", [True, False])
def test_image_within_three_times_the_fp32_restatement(mode, with_colors):
    shape = (40, 36, 44)
    v, t = _mc_mesh(mo.gaussians(shape, np.random.default_rng(5)), shape)
    H, W = 300, 400
    c2w, K = ro.look_at((2.1, 1.4, 0.8)), (310.0, 305.0, 201.3, 148.8)
    colors = np.random.default_rng(2).random((len(v), 3)).astype(np.float32) if with_colors else None
    _, _, normals = ro.vertex_normal_sums(v, t)
    bg = (0.1, 0.2, 0.3)
    out = _render(v, t, c2w, K, H, W, colors=colors, normals=normals, mode=mode, ambient=0.25, background=bg)
    w2c = ro.world_to_camera(c2w)
    keys, _ = ro.rasterize(v, t, w2c, *K, H, W)
    assert np.array_equal(out["tri_id"], ro.decode(keys)[1])
    args = dict(colors=colors, normals=normals, mode=mode, ambient=0.25, background=bg)
    img32 = ro.resolve(keys, v, t, w2c, *K, dtype=np.float32, **args)
    img64 = ro.resolve(keys, v, t, w2c, *K, dtype=np.float64, **args)
    err_hip = np.abs(out["image"].astype(np.float64) - img64).max()
    err_np = np.abs(img32.astype(np.float64) - img64).max()
    print(f"{mode} colors={with_colors}: HIP {err_hip:.3e} numpy-fp32 {err_np:.3e} "
          f"bit-identical pixels {np.mean(out['image'] == img32):.4f}")
    assert err_hip <= max(3 * err_np, FLOOR)
    assert np.array_equal(out["image"][out["tri_id"] < 0], np.broadcast_to(np.array(bg, np.float32), ((out["tri_id"] < 0).sum(), 3)))
    if mode == "shaded" and not with_colors:
        lit = out["image"][out["tri_id"] >= 0]
        assert lit.max() <= 0.7 * (1 + 1e-6) and lit.min() >= 0.7 * 0.25 * (1 - 1e-6)


@pytest.mark.parametrize("mode", ["color", "normal", "shaded"])
def test_noise_mesh_image_is_finite_and_within_the_rule(mode):
    """white noise: slivers whose barycentric sub-areas cancel or underflow get the centroid's attributes, never NaN"""
    rng = np.random.default_rng(7)
    shape = (23, 19, 27)
    vol = rng.normal(size=shape).astype(np.float32)
    vol[rng.random(shape) < 0.02] = np.nan
    v, t = _mc_mesh(vol, shape)
    H, W = 240, 320
    c2w, K = ro.look_at((1.7, -1.9, 1.1)), _centre_K(H, W, 330.0)
    colors = np.random.default_rng(3).random((len(v), 3)).astype(np.float32)
    _, _, normals = ro.vertex_normal_sums(v, t)
    out = _render(v, t, c2w, K, H, W, colors=colors, normals=normals, mode=mode)
    assert (out["tri_id"] >= 0).sum() > 20000
    assert np.isfinite(out["image"]).all()
    w2c = ro.world_to_camera(c2w)
    keys, _ = ro.rasterize(v, t, w2c, *K, H, W)
    assert np.array_equal(out["tri_id"], ro.decode(keys)[1])
    args = dict(colors=colors, normals=normals, mode=mode)
    img32 = ro.resolve(keys, v, t, w2c, *K, dtype=np.float32, **args)
    img64 = ro.resolve(keys, v, t, w2c, *K, dtype=np.float64, **args)
    assert np.isfinite(img32).all() and np.isfinite(img64).all()
    err_hip = np.abs(out["image"].astype(np.float64) - img64).max()
    err_np = np.abs(img32.astype(np.float64) - img64).max()
    print(f"noise {mode}: HIP {err_hip:.3e} numpy-fp32 {err_np:.3e} bit-identical pixels {np.mean(out['image'] == img32):.4f}")
    assert err_hip <= max(3 * err_np, FLOOR)


def test_sliver_barycentrics_fall_back_to_the_centroid():
    """a triangle 2e-12 across seen through fx = 1e12 covers pixels, its plane gives z = 1, but its sub-areas against n
    (~1e-47) underflow to 0: l = 0 / 0, so the pixel gets the centroid's attributes (1/3 of each vertex), not NaN"""
    e = np.float32(1e-12)
    v = np.array([(-e, -e, 1), (e, -e, 1), (0, e, 1)], np.float32)
    t = np.array([(0, 1, 2)], np.int64)
    colors = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1)], np.float32)
    K, c2w = (1e12, 1e12, 2.0, 2.0), np.eye(4)
    out = _render(v, t, c2w, K, 4, 4, colors=colors, convention="opencv", mode="color")
    w2c = ro.world_to_camera(c2w, "opencv")
    keys, _ = ro.rasterize(v, t, w2c, *K, 4, 4)
    depth, tri_id = ro.decode(keys)
    assert np.array_equal(out["tri_id"], tri_id) and np.array_equal(out["depth"].view(np.uint32), depth.view(np.uint32))
    hit = tri_id >= 0
    assert hit.sum() >= 2 and (depth[hit] == 1).all()
    third = np.float32(1.0) / np.float32(3.0)
    assert np.array_equal(out["image"][hit], np.full((hit.sum(), 3), third, np.float32))
    assert np.array_equal(out["image"], ro.resolve(keys, v, t, w2c, *K, colors=colors, mode="color"))


def test_default_normals_are_the_vertex_normals():
    from morpheus_amd import meshrender
    v, t = ro.icosphere(3, 0.8)
    c2w, K = ro.look_at((1.9, 1.2, 0.9)), _centre_K(90, 120, 110.0)
    nrm = meshrender.vertex_normals(_dev(v), _dev(t)).cpu().numpy()
    a = _render(v, t, c2w, K, 90, 120, mode="normal")
    b = _render(v, t, c2w, K, 90, 120, mode="normal", normals=nrm)
    assert np.array_equal(a["image"], b["image"])
    hit = a["tri_id"] >= 0
    n_cam = a["image"][hit] * 2 - 1
    assert hit.sum() > 1000 and np.abs(np.linalg.norm(n_cam, axis=1) - 1).max() < 1e-5
    assert (n_cam[:, 2] < 0.1).all() and n_cam[:, 2].mean() < -0.5     # outward normals of the visible half face the camera


def test_shared_edges_cover_once():
    v, A, B, w2c, K = ro.split_plane()
    c2w = np.eye(4)
    cov = {}
    for name, tri in (("A", A), ("B", B), ("AB", np.concatenate([A, B]))):
        out = _render(v, tri, c2w, K, 32, 32, convention="opencv", mode="color")
        keys, _ = ro.rasterize(v, tri, w2c, *K, 32, 32)
        assert np.array_equal(out["tri_id"], ro.decode(keys)[1])
        cov[name] = out["tri_id"] >= 0
    assert not (cov["A"] & cov["B"]).any()
    assert np.array_equal(cov["A"] | cov["B"], cov["AB"])
    assert cov["AB"][5:27, 5:27].all()
    for ta in A:
        for tb in B:
            a = _render(v, ta[None], c2w, K, 32, 32, convention="opencv", mode="color")["tri_id"] >= 0
            b = _render(v, tb[None], c2w, K, 32, 32, convention="opencv", mode="color")["tri_id"] >= 0
            assert not (a & b).any()


@pytest.fixture(scope="module")
def model():
    from morpheus_amd import harness
    return harness.build_model("b", DEV)


@pytest.fixture(scope="module")
def model_mesh(model):
    from morpheus_amd import mesh
    out = mesh.extract_mesh(model, resolution=96, S=96, t=25 / 200)
    assert out["triangles"].shape[0] > 100
    return out


def test_depth_agrees_with_the_ray_generator(model_mesh):
    """rays of ops.generate_rays (unnormalised d, camera z = -1: the ray parameter is camera depth) intersected in float64
    with triangle tri_id[j, i] give depth[j, i] within 3 x the error that the numpy-fp32 restatement's depth of THIS view has
    against the same float64 intersections (floor 2^-22), over pixels with |n^ . d^| >= 0.05; at most 2 % of the hits may be
    excluded that way, as in tests/test_raster_host.py."""
    from morpheus_amd import meshrender, ops
    H = W = 72
    K = (80.0, 80.0, 36.0, 36.0)
    c2w = ro.look_at((0.4, -2.4, 0.7))
    out = meshrender.render_mesh(model_mesh["vertices"], model_mesh["triangles"], c2w=c2w, fx=K[0], fy=K[1], cx=K[2], cy=K[3],
                                 H=H, W=W, mode="color")
    o, d = ops.generate_rays(*K, c2w, H, W, DEV)
    o, d = o.cpu().numpy().astype(np.float64), d.cpu().numpy().astype(np.float64)
    tri_id, depth = out["tri_id"].cpu().numpy().reshape(-1), out["depth"].cpu().numpy().reshape(-1)
    hit = np.flatnonzero(tri_id >= 0)
    assert hit.size > 200, hit.size
    v = model_mesh["vertices"].cpu().numpy().astype(np.float64)
    tr = model_mesh["triangles"].cpu().numpy()[tri_id[hit]]
    a, b, c = v[tr[:, 0]], v[tr[:, 1]], v[tr[:, 2]]
    n = np.cross(b - a, c - a)
    s = ((a - o[hit]) * n).sum(1) / (d[hit] * n).sum(1)
    cosine = np.abs((d[hit] * n).sum(1)) / np.linalg.norm(n, axis=1) / np.linalg.norm(d[hit], axis=1)
    keep = cosine >= 0.05
    rel = np.abs(depth[hit] - s) / s
    # the restatement's own error on the same inputs: its fp32 depth of this mesh and view against the same yardstick
    vn, tn = model_mesh["vertices"].cpu().numpy(), model_mesh["triangles"].cpu().numpy()
    keys, _ = ro.rasterize(vn, tn, ro.world_to_camera(c2w), *K, H, W)
    np_depth, np_tri = (x.reshape(-1) for x in ro.decode(keys))
    assert np.array_equal(np_tri, tri_id)
    own = (np.abs(np_depth[hit] - s) / s)[keep].max()
    bound = max(3 * own, FLOOR)
    print(f"hits {hit.size} kept {keep.sum()} excluded share {1 - keep.mean():.4f} worst rel {rel[keep].max():.3e} "
          f"numpy-fp32 {own:.3e} bound {bound:.3e}")
    assert 1 - keep.mean() <= 0.02
    # the hit point lies inside the triangle (up to the snapping at its edges): the ray parameter is not just any plane's
    P = o[hit] + s[:, None] * d[hit]
    wa = (np.cross(b - P, c - P) * n).sum(1)
    wb = (np.cross(c - P, a - P) * n).sum(1)
    wc = (np.cross(a - P, b - P) * n).sum(1)
    lam = np.stack([wa, wb, wc], 1) / (wa + wb + wc)[:, None]
    assert lam.min() > -0.02, lam.min()
    assert rel[keep].max() <= bound


def test_deterministic_and_independent_of_triangle_order(model_mesh):
    from morpheus_amd import meshrender
    v, t, c = model_mesh["vertices"], model_mesh["triangles"], model_mesh["colors"]
    cam = dict(c2w=ro.look_at((0.4, -2.4, 0.7)), fx=300.0, fy=300.0, cx=160.0, cy=120.0, H=240, W=320)
    a = meshrender.render_mesh(v, t, c, **cam)
    b = meshrender.render_mesh(v, t, c, **cam)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert int((a["tri_id"] >= 0).sum()) > 2000
    perm = torch.randperm(t.shape[0], generator=torch.Generator().manual_seed(3)).to(DEV)
    p = meshrender.render_mesh(v, t[perm].contiguous(), c, **cam)
    assert torch.equal(p["depth"].view(torch.int32), a["depth"].view(torch.int32))
    assert torch.equal(p["clipped"], a["clipped"])
    hit = a["tri_id"] >= 0
    assert torch.equal(p["tri_id"] >= 0, hit)
    back = perm[p["tri_id"][hit].long()]
    moved = back != a["tri_id"][hit].long()
    # where the winner changed, two triangles tie in depth at that pixel: the other one's plane gives the same depth bits
    if bool(moved.any()):
        vn, tn = v.cpu().numpy(), t.cpu().numpy()
        w2c = ro.world_to_camera(cam["c2w"])
        jj, ii = (x[moved.cpu().numpy()] for x in np.nonzero(hit.cpu().numpy()))
        for tri, j, i in zip(back[moved].cpu().numpy(), jj, ii):
            keys, _ = ro.rasterize(vn, tn[tri][None], w2c, 300.0, 300.0, 160.0, 120.0, 240, 320)
            assert ro.decode(keys)[0][j, i].view(np.uint32) == a["depth"][j, i].cpu().numpy().view(np.uint32)
    print(f"winner changed at {int(moved.sum())} of {int(hit.sum())} pixels")


def test_render_all_meshes_end_to_end(model, tmp_path):
    from PIL import Image
    from morpheus_amd import mesh, meshrender
    H = W = 48
    K = np.array([[60.0, 0, 24.0], [0, 60.0, 24.0], [0, 0, 1]])
    frames = [0, 25, 50]
    poses = [ro.look_at((2.4 * np.cos(a), 2.4 * np.sin(a), 0.6)) for a in (0.0, 0.7, 1.4)]
    meshes = []
    for i, f in enumerate(frames):
        m = mesh.export_mesh(model, str(tmp_path / "mesh" / f"mesh_0007_{i:04d}.ply"), resolution=96, S=96, t=f / 200)
        meshes.append(m)
    res = meshrender.render_all_meshes(meshes, poses, K, H, W, save_images_dir=str(tmp_path / "img"),
                                       save_depths_dir=str(tmp_path / "dep"), scale=2, keep_results=True)
    assert np.array_equal(K, np.array([[60.0, 0, 24.0], [0, 60.0, 24.0], [0, 0, 1]]))       # the caller's K is not scaled
    npz = np.load(str(tmp_path / "dep" / "depths.npz"))
    assert sorted(npz.files) == ["depth_0", "depth_1", "depth_2"]
    for i, m in enumerate(meshes):
        one = meshrender.render_mesh(m["vertices"], m["triangles"], m["colors"], c2w=poses[i], fx=120.0, fy=120.0, cx=48.0,
                                     cy=48.0, H=96, W=96)
        assert npz[f"depth_{i}"].shape == (96, 96) and (npz[f"depth_{i}"] > 0).sum() > 200
        assert np.array_equal(npz[f"depth_{i}"].view(np.uint32), one["depth"].cpu().numpy().view(np.uint32))
        assert torch.equal(res[i]["depth"], one["depth"]) and torch.equal(res[i]["image"], one["image"])
        png = Image.open(str(tmp_path / "img" / f"{i:04d}.png"))
        assert png.size == (96, 96) and png.mode == "RGB"
        want = (one["image"].clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
        assert np.array_equal(np.asarray(png), want)
    # the same call fed from the PLY files: the same depth bytes (positions and indices survive the file; colours are bytes)
    res2 = meshrender.render_all_meshes(str(tmp_path / "mesh"), poses, K, H, W, save_depths_dir=str(tmp_path / "dep2"), scale=2)
    npz2 = np.load(str(tmp_path / "dep2" / "depths.npz"))
    assert sorted(res2) == ["depth_0", "depth_1", "depth_2"]           # by default: the host depths, nothing kept on the device
    for i in range(3):
        assert np.array_equal(npz2[f"depth_{i}"].view(np.uint32), npz[f"depth_{i}"].view(np.uint32))
        assert isinstance(res2[f"depth_{i}"], np.ndarray) and np.array_equal(res2[f"depth_{i}"], npz2[f"depth_{i}"])
    assert not os.path.exists(str(tmp_path / "dep2" / "0000.png"))


def test_render_all_meshes_selects_the_epoch(tmp_path):
    """every epoch's meshes share one directory (mesh_{epoch}_{frame}.ply): `epoch` picks the files, a directory of several
    epochs is refused without it, and an epoch that is not there is an error"""
    from morpheus_amd import mesh, meshrender
    from morpheus_amd._lib import MorpheusHipError
    H = W = 40
    K = np.array([[50.0, 0, 20.0], [0, 50.0, 20.0], [0, 0, 1]])
    poses = [ro.look_at((2.4, 0.3 * i, 0.5)) for i in range(2)]
    radius = {3: 0.4, 12: 0.8}                                 # two epochs of different meshes
    d = tmp_path / "mesh_all"
    d.mkdir()
    for epoch, r in radius.items():
        v, t = ro.icosphere(2, r)
        for i in range(2):
            mesh.write_ply(str(d / f"mesh_{epoch:04d}_{i:04d}.ply"), v, t)
    (d / "notes.ply").write_bytes(b"not a mesh of the run")       # a name that is not mesh_EPOCH_FRAME.ply is left alone
    with pytest.raises(MorpheusHipError, match="epochs"):
        meshrender.render_all_meshes(str(d), poses, K, H, W, scale=1)
    with pytest.raises(MorpheusHipError):
        meshrender.render_all_meshes(str(d), poses, K, H, W, scale=1, epoch=5)
    with pytest.raises(MorpheusHipError):
        meshrender.render_all_meshes([], poses, K, H, W, scale=1, epoch=3)
    got = {}
    for epoch, r in radius.items():
        out = meshrender.render_all_meshes(str(d), poses, K, H, W, scale=1, epoch=epoch, save_depths_dir=str(tmp_path / f"dep{epoch}"))
        assert sorted(out) == ["depth_0", "depth_1"]
        v, t = ro.icosphere(2, r)
        for i in range(2):
            one = meshrender.render_mesh(_dev(v), _dev(t), c2w=poses[i], fx=50.0, fy=50.0, cx=20.0, cy=20.0, H=H, W=W)
            assert np.array_equal(out[f"depth_{i}"].view(np.uint32), one["depth"].cpu().numpy().view(np.uint32))
            on_disk = np.load(str(tmp_path / f"dep{epoch}" / "depths.npz"))[f"depth_{i}"]
            assert np.array_equal(on_disk.view(np.uint32), out[f"depth_{i}"].view(np.uint32))
        got[epoch] = (out["depth_0"] > 0).sum()
    assert got[12] > 2 * got[3] > 0                            # the larger sphere of epoch 12, not whichever file sorts last
