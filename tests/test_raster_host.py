"""CPU (no GPU): the numpy restatement of the rasteriser (tests/raster_oracle.py) against a float64 ray caster that shares
nothing with it, its shared-edge rule and its fixed-point normals; the argument checks of the mh_raster_* /
mh_mesh_vertex_normals entry points without a device; read_ply as the inverse of write_ply; the refusal of CPU tensors."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import mc_oracle as mo
from tests import raster_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 80, 96                                                 # a 96 x 80 image


@pytest.fixture(scope="module")
def lib():
    from morpheus_amd import _lib, build
    build.build()
    return _lib.load()


def _icosphere_case():
    v, t = ro.icosphere(3, 0.8)                               # 1 280 triangles, silhouette inside the image
    return v, t, ro.world_to_camera(ro.look_at((1.9, 1.2, 0.9))), 170.0


def _torus_case():
    shape = (18, 19, 11)
    v, t = mo.marching_cubes(mo.torus(shape, (8.3, 9.1, 5.15), 5.2, 2.6))
    return ro.to_unit_box(v, shape), t, ro.world_to_camera(ro.look_at((0.3, -2.2, 1.6), target=(-0.05, 0, -0.4))), 420.0


@pytest.mark.parametrize("case", [_icosphere_case, _torus_case])
def test_oracle_matches_the_float64_ray_caster(case):
    """tri_id of the int64 rasteriser == the nearest hit of the float64 Moeller-Trumbore caster at every covered pixel whose
    centre is at least 1/128 px from every projected edge (the 8-bit snapping moves an edge by at most 2^-9 px per
    coordinate); at most 2 % of the covered pixels may be excluded that way (measured here: 1.6 % icosphere, 1.4 % torus).

    Depth: the oracle's fp32 ray-plane depth against the float64 intersection with the same triangle, over covered pixels with
    |n^ . d^| >= 0.05 (excluded: 0.013 % icosphere, 0.13 % torus; cap 2 %).  Worst relative error measured: 4.7e-7 (icosphere),
    2.1e-7 (torus).  raster_oracle.OWN_FP32_DEPTH_ERROR = 4.7e-7 is the oracle's own fp32 error that tests/test_gpu_raster.py uses."""
    v, t, w2c, f = case()
    assert t.shape[0] >= 1000
    cx, cy = W / 2, H / 2
    keys, clipped = ro.rasterize(v, t, w2c, f, f, cx, cy, H, W)
    depth, tri_id = ro.decode(keys)
    best, z, _ = ro.ray_cast(v, t, w2c, f, f, cx, cy, H, W)
    edge = ro.edge_distance_px(v, t, w2c, f, f, cx, cy, H, W)
    covered = (tri_id >= 0) | (best >= 0)
    excluded = covered & (edge < 1 / 128)
    share = excluded.sum() / covered.sum()
    differ = covered & ~excluded & (tri_id != best)
    print(f"covered {covered.sum()} excluded {excluded.sum()} ({share:.4f}) differing {differ.sum()} clipped {clipped}")
    assert clipped == 0 and covered.sum() > 4000
    assert share <= 0.02, share
    assert not differ.any(), np.argwhere(differ)[:10]

    cam = ro.to_camera(w2c, v, np.float64)
    jj, ii = np.nonzero(tri_id >= 0)
    tr = t[tri_id[jj, ii]]
    a, b, c = cam[tr[:, 0]], cam[tr[:, 1]], cam[tr[:, 2]]
    n = np.cross(b - a, c - a)
    dx, dy = ro.pixel_dirs(f, f, cx, cy, ii, jj, np.float64)
    d = np.stack([dx, dy, np.ones_like(dx)], 1)
    z64 = (n * a).sum(1) / (n * d).sum(1)
    cosine = np.abs((n * d).sum(1)) / np.linalg.norm(n, axis=1) / np.linalg.norm(d, axis=1)
    keep = cosine >= 0.05
    rel = np.abs(depth[jj, ii] - z64) / z64
    print(f"depth: worst rel {rel[keep].max():.3e} over kept pixels, excluded share {1 - keep.mean():.5f}")
    assert 1 - keep.mean() <= 0.02
    assert rel[keep].max() <= ro.OWN_FP32_DEPTH_ERROR


def test_oracle_shared_edges_cover_once():
    v, A, B, w2c, K = ro.split_plane()
    cov = {}
    for name, tri in (("A", A), ("B", B), ("AB", np.concatenate([A, B]))):
        keys, _ = ro.rasterize(v, tri, w2c, *K, 32, 32)
        cov[name] = ro.decode(keys)[1] >= 0
    assert not (cov["A"] & cov["B"]).any()
    assert np.array_equal(cov["A"] | cov["B"], cov["AB"])
    # the square [4.5, 27.5]^2: each centre on its border belongs to it or not by the edge's rule, the inside always does
    assert cov["AB"][5:27, 5:27].all() and cov["AB"].sum() in range(22 * 22, 24 * 24 + 1)
    # centres on the cutting edges (column 16 and the diagonals run through pixel centres) are covered exactly once
    for tri_a in A:
        for tri_b in B:
            ka, _ = ro.rasterize(v, tri_a[None], w2c, *K, 32, 32)
            kb, _ = ro.rasterize(v, tri_b[None], w2c, *K, 32, 32)
            assert not ((ka != ro.EMPTY) & (kb != ro.EMPTY)).any()


def test_oracle_vertex_normals():
    v, t = ro.icosphere(2, 0.7, (0.1, -0.2, 0.05))
    sums, bits, nrm = ro.vertex_normal_sums(v, t)
    want = ro.vertex_normals_f64(v, t)
    assert np.abs(nrm - want).max() < 1e-6
    outward = v.astype(np.float64) - np.array([0.1, -0.2, 0.05])
    assert ((nrm * outward).sum(1) > 0.69).all()
    perm = np.random.default_rng(0).permutation(len(t))
    sums2, bits2, _ = ro.vertex_normal_sums(v, t[perm])
    assert np.array_equal(sums, sums2) and bits == bits2
    assert np.abs(sums).max() < 6 << 40                        # valence <= 6, each |k| <= 2^40
    lone = np.concatenate([v, [[5, 5, 5]]]).astype(np.float32)  # a vertex no triangle uses
    assert np.array_equal(ro.vertex_normal_sums(lone, t)[2][-1], [0, 0, 1])


@pytest.mark.parametrize("with_colors", [False, True])
def test_read_ply_inverts_write_ply(tmp_path, with_colors):
    from morpheus_amd.mesh import read_ply, write_ply
    rng = np.random.default_rng(11)
    v = rng.normal(size=(13, 3)).astype(np.float32)
    t = rng.integers(0, 13, size=(9, 3))
    c = (rng.integers(0, 256, size=(13, 3)) / 255.0).astype(np.float32) if with_colors else None
    path = str(tmp_path / "m.ply")
    write_ply(path, torch.from_numpy(v), torch.from_numpy(t), None if c is None else torch.from_numpy(c))
    rv, rt, rc = read_ply(path)
    assert rv.dtype == np.float32 and rt.dtype == np.int64
    assert np.array_equal(rv, v) and np.array_equal(rt, t)
    if with_colors:
        assert rc.dtype == np.float32 and np.array_equal(rc, c)
    else:
        assert rc is None
    hdr, verts, faces = mo.read_ply(path)                       # and the two readers agree
    assert np.array_equal(faces, rt) and np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), rv)


def test_read_ply_refuses_other_files(tmp_path):
    from morpheus_amd._lib import MorpheusHipError
    from morpheus_amd.mesh import read_ply
    p = tmp_path / "x.ply"
    p.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(MorpheusHipError):
        read_ply(str(p))
    p.write_bytes(b"not a ply at all")
    with pytest.raises(MorpheusHipError):
        read_ply(str(p))


def test_raster_argument_validation_without_gpu(lib):
    """status codes, no launch: null pointers, sizes outside [1, 16384], near <= 0, bad modes, counts outside [0, 2^31)"""
    fake = 256                                                # never dereferenced: the checks come first
    w2c = np.eye(4, dtype=np.float32)[:3].copy()
    wp = w2c.ctypes.data_as(ctypes.c_void_p)
    K = (50.0, 50.0, 8.0, 8.0)

    def depth(v=fake, V=3, t=fake, T=1, w=wp, k=K, H=16, W=16, near=0.01, ws=fake, clipped=fake):
        return lib.mh_raster_depth(v, V, t, T, w, *k, H, W, near, 0, ws, clipped, None)

    def resolve(v=fake, V=3, t=fake, T=1, col=None, nrm=fake, w=wp, k=K, H=16, W=16, mode=2, ws=fake, d=fake, tid=fake, img=fake):
        return lib.mh_raster_resolve(v, V, t, T, col, nrm, w, *k, H, W, mode, 0.3, 1.0, 1.0, 1.0, ws, d, tid, img, None)

    for bad in (dict(v=None), dict(t=None), dict(w=None), dict(ws=None), dict(clipped=None), dict(H=0), dict(W=0), dict(H=-4),
                dict(H=16385), dict(W=16385), dict(near=0.0), dict(near=-1.0), dict(near=float("nan")), dict(near=float("inf")),
                dict(V=-1), dict(T=-1), dict(T=1 << 31), dict(V=1 << 31), dict(k=(0.0, 50.0, 8.0, 8.0)),
                dict(k=(50.0, -1.0, 8.0, 8.0)), dict(k=(float("nan"), 50.0, 8.0, 8.0))):
        assert depth(**bad) == 1, bad
    for bad in (dict(v=None), dict(t=None), dict(w=None), dict(ws=None), dict(d=None), dict(tid=None), dict(img=None),
                dict(nrm=None), dict(nrm=None, mode=1), dict(mode=3), dict(mode=-1), dict(H=0), dict(W=16385), dict(T=-1),
                dict(V=1 << 31), dict(k=(50.0, 0.0, 8.0, 8.0))):
        assert resolve(**bad) == 1, bad
    vn = lib.mh_mesh_vertex_normals
    assert vn(fake, 3, fake, 1, None, fake, None) == 1
    assert vn(None, 3, fake, 1, fake, fake, None) == 1
    assert vn(fake, 3, None, 1, fake, fake, None) == 1
    assert vn(fake, 3, fake, 1, fake, None, None) == 1
    assert vn(fake, -1, fake, 1, fake, fake, None) == 1
    assert vn(fake, 3, fake, 1 << 31, fake, fake, None) == 1
    wb = lib.mh_raster_workspace_bytes
    for H_, W_, T_ in [(0, 4, 1), (4, 0, 1), (-1, 4, 1), (16385, 4, 1), (4, 16385, 1), (4, 4, -1), (4, 4, 1 << 31)]:
        assert wb(H_, W_, T_) == -1, (H_, W_, T_)
    assert wb(1, 1, 0) > 0
    assert wb(16384, 16384, 0) >= 8 * 16384 * 16384
    assert wb(768, 1024, 500000) >= 8 * 768 * 1024 + 4 * 500000 > wb(768, 1024, 0) >= 8 * 768 * 1024


def test_render_mesh_refuses_cpu_tensors_and_bad_input():
    from morpheus_amd import meshrender
    from morpheus_amd._lib import MorpheusHipError
    v, t = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    cam = dict(c2w=np.eye(4), H=8, W=8, fx=10.0, fy=10.0, cx=4.0, cy=4.0)
    with pytest.raises(MorpheusHipError):
        meshrender.render_mesh(v, t, **cam)
    with pytest.raises(MorpheusHipError):
        meshrender.vertex_normals(v, t)
    with pytest.raises(MorpheusHipError):
        meshrender.render_mesh(v, t, mode="phong", **cam)
    with pytest.raises(MorpheusHipError):
        meshrender.world_to_camera(np.eye(4), "blender")
    assert np.array_equal(meshrender.world_to_camera(ro.look_at((1, 2, 3))), ro.world_to_camera(ro.look_at((1, 2, 3))))
    cv = meshrender.cv2gl(ro.look_at((1, 2, 3)))
    assert np.array_equal(meshrender.world_to_camera(cv, "opencv"), ro.world_to_camera(ro.look_at((1, 2, 3))))
