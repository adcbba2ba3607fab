"""CPU (no GPU): the marching-cubes restatement (tests/mc_oracle.py) against geometry that does not depend on its table --
closed manifolds of the right topology, exact planes, face consistency on saddle-rich and noise fields -- plus the PLY
writer, the argument checks of the mh_mc_* entry points and the refusal of CPU tensors."""
import importlib.util
import itertools
import math
import os

import numpy as np
import pytest
import torch

from tests import mc_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from morpheus_amd import _lib, build
    build.build()
    return _lib.load()


def _closed_manifold(v, t):
    _, uses = mo.edge_uses(t)
    assert uses.size and (uses == 2).all(), np.unique(uses, return_counts=True)
    assert np.unique(t).size == v.shape[0]                     # every vertex is used


def _on_box_face(v, a, b, shape):
    pa, pb = v[a], v[b]
    hi = np.asarray(shape, np.float32) - 1
    return ((pa == 0) & (pb == 0) | (pa == hi) & (pb == hi)).any(-1)


def test_table_file_is_the_generator_output():
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert open(mo.TABLE_PATH).read() == gen.render()
    assert [int(w) for w in mo.TABLE] == gen.packed_table()
    counts = mo.TABLE >> np.uint64(60)
    assert counts[0] == 0 and counts[255] == 0 and counts.max() == 5


@pytest.mark.parametrize("n,center,r", [(32, (15.2, 15.6, 15.4), 12.3), (64, (31.7, 30.9, 32.4), 24.6),
                                        (96, (47.3, 48.1, 46.6), 40.2)])
def test_sphere_is_a_closed_sphere(n, center, r):
    v, t = mo.marching_cubes(mo.sphere((n, n, n), center, r))
    _closed_manifold(v, t)
    assert mo.euler(v, t) == 2
    vol = mo.signed_volume(v, t)
    assert vol > 0 and abs(vol / (4 / 3 * math.pi * r ** 3) - 1) < 0.01, vol
    assert np.abs(np.linalg.norm(v - np.asarray(center), axis=1) - r).max() < 0.05


def test_torus_is_closed_with_genus_one():
    v, t = mo.marching_cubes(mo.torus((48, 52, 30), (23.6, 25.2, 14.3), 14.5, 6.2))
    _closed_manifold(v, t)
    assert mo.euler(v, t) == 0
    assert mo.signed_volume(v, t) > 0


def _box_section_area(shape, n, d):
    """area of {x : n.x = d} inside [0, shape-1]^3 (a convex polygon through the box edges' crossings)"""
    hi = np.asarray(shape, np.float64) - 1
    corners = np.array(list(itertools.product(*[(0.0, h) for h in hi])))
    pts = []
    for a, b in itertools.combinations(range(8), 2):
        if (corners[a] != corners[b]).sum() != 1:
            continue
        fa, fb = corners[a] @ n - d, corners[b] @ n - d
        if (fa < 0) != (fb < 0):
            pts.append(corners[a] + fa / (fa - fb) * (corners[b] - corners[a]))
    pts = np.array(pts)
    c = pts.mean(0)
    u = pts[0] - c
    u /= np.linalg.norm(u)
    w = np.cross(n, u)
    order = np.argsort(np.arctan2((pts - c) @ w, (pts - c) @ u))
    p = pts[order]
    return 0.5 * np.linalg.norm(np.cross(p - c, np.roll(p, -1, 0) - c).sum(0))


@pytest.mark.parametrize("seed", range(4))
def test_random_plane_is_the_exact_section(seed):
    rng = np.random.default_rng(seed)
    shape = tuple(int(s) for s in rng.integers(33, 61, 3))
    normal = rng.normal(size=3)
    center = rng.uniform(0.35, 0.65, 3) * (np.asarray(shape) - 1)
    n = normal / np.linalg.norm(normal)
    d = float(center @ n)
    vol, _ = mo.plane(shape, normal, d)
    v, t = mo.marching_cubes(vol)
    assert np.abs(v.astype(np.float64) @ n - d).max() < 1e-5
    assert abs(mo.area(v, t) / _box_section_area(shape, n, d) - 1) < 1e-4
    assert mo.euler(v, t) == 1
    edges, uses = mo.edge_uses(t)
    assert set(np.unique(uses)) <= {1, 2}
    border = edges[uses == 1]
    assert border.size and _on_box_face(v, border[:, 0], border[:, 1], shape).all()


def _interior_edges_used_twice(v, t, shape):
    edges, uses = mo.edge_uses(t)
    assert uses.max() <= 2
    inner = ~_on_box_face(v, edges[:, 0], edges[:, 1], shape)
    assert (uses[inner] == 2).all(), int((uses[inner] != 2).sum())


@pytest.mark.parametrize("seed", range(3))
def test_saddle_field_faces_are_consistent(seed):
    rng = np.random.default_rng(100 + seed)
    shape = (40, 36, 44)
    v, t = mo.marching_cubes(mo.gaussians(shape, rng))
    assert t.shape[0] > 1000
    _interior_edges_used_twice(v, t, shape)


def test_noise_faces_are_consistent():
    """white noise: ambiguous faces everywhere, NaN corners (outside) included"""
    rng = np.random.default_rng(7)
    shape = (23, 19, 27)
    vol = rng.normal(size=shape).astype(np.float32)
    vol[rng.random(shape) < 0.02] = np.nan
    v, t = mo.marching_cubes(vol)
    _interior_edges_used_twice(v, t, shape)


def test_all_outside_is_empty():
    v, t = mo.marching_cubes(np.ones((5, 6, 7), np.float32))
    assert v.shape == (0, 3) and t.shape == (0, 3)


@pytest.mark.parametrize("with_colors", [False, True])
def test_write_ply_round_trip(tmp_path, with_colors):
    from morpheus_amd.mesh import write_ply
    rng = np.random.default_rng(3)
    v = rng.normal(size=(11, 3)).astype(np.float32)
    t = rng.integers(0, 11, size=(7, 3))
    c = rng.uniform(-0.2, 1.2, size=(11, 3)).astype(np.float32) if with_colors else None
    path = str(tmp_path / "m.ply")
    write_ply(path, torch.from_numpy(v), torch.from_numpy(t), None if c is None else torch.from_numpy(c))
    header, verts, faces = mo.read_ply(path)
    want = ["ply", "format binary_little_endian 1.0", "element vertex 11",
            "property float x", "property float y", "property float z"]
    if with_colors:
        want += ["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
    want += ["element face 7", "property list uchar int vertex_indices", "end_header"]
    assert header == want
    assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), v)
    assert np.array_equal(faces, t)
    if with_colors:
        rgb = np.stack([verts["red"], verts["green"], verts["blue"]], 1)
        assert np.array_equal(rgb, np.rint(np.clip(c.astype(np.float64), 0, 1) * 255).astype(np.uint8))
        assert (verts["alpha"] == 255).all()


def test_mc_argument_validation_without_gpu(lib):
    """status codes, no launch: null pointers, sides < 2, 2^31 points or more"""
    fake = 256                                               # never dereferenced: the checks come first
    assert lib.mh_mc_count(None, 4, 4, 4, 0.0, fake, fake, None) == 1
    assert lib.mh_mc_count(fake, 4, 4, 4, 0.0, None, fake, None) == 1
    assert lib.mh_mc_count(fake, 4, 4, 4, 0.0, fake, None, None) == 1
    assert lib.mh_mc_emit(fake, 4, 4, 4, 0.0, fake, None, fake, None) == 1
    assert lib.mh_mc_emit(fake, 4, 4, 4, 0.0, fake, fake, None, None) == 1
    assert lib.mh_mc_emit(None, 4, 4, 4, 0.0, fake, fake, fake, None) == 1
    for shape in [(1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (-3, 4, 4), (2048, 1024, 1024), (1291, 1291, 1291)]:
        assert lib.mh_mc_count(fake, *shape, 0.0, fake, fake, None) == 1, shape
        assert lib.mh_mc_emit(fake, *shape, 0.0, fake, fake, fake, None) == 1, shape
        assert lib.mh_mc_workspace_bytes(*shape) == -1, shape
    small = lib.mh_mc_workspace_bytes(2, 2, 2)
    assert small > 0
    big = lib.mh_mc_workspace_bytes(2047, 1024, 1024)          # the largest side product below 2^31 of this form
    assert big >= 5 * 2047 * 1024 * 1024 and big > lib.mh_mc_workspace_bytes(256, 256, 256) > small
    assert "overflow" in lib.mh_status_string(3).decode()


def test_marching_cubes_refuses_cpu_tensors():
    from morpheus_amd import mesh
    from morpheus_amd._lib import MorpheusHipError
    with pytest.raises(MorpheusHipError):
        mesh.marching_cubes(torch.zeros(4, 4, 4))
