"""CPU (no GPU): the numpy restatement of the subdivision (tests/subdivide_oracle.py, written from include/morpheus_hip.h) held to
trimesh's algorithm -- a recursive midpoint split in float64, restated here -- and its two index maps to their ranges; the new
source is in the build with its flag, the entry points are bound from the header and validate their arguments without a device."""
import numpy as np
import pytest

from tests import subdivide_oracle as so

F = np.float32
SEED, COUNT = 20240607, 3000


@pytest.fixture(scope="module")
def lib():
    from morpheus_amd import _lib, build
    build.build()
    return _lib.load()


def test_closed_form_depth_equals_the_recursive_split():
    rng = np.random.default_rng(SEED)
    max_edge = 0.01
    scale = np.exp(rng.uniform(np.log(0.01), np.log(0.3), COUNT))
    centre = rng.uniform(-1, 1, (COUNT, 1, 3))
    corners = (centre + scale[:, None, None] * rng.uniform(-0.5, 0.5, (COUNT, 3, 3))).astype(F)
    v = corners.reshape(-1, 3)
    tri = np.arange(3 * COUNT).reshape(-1, 3)
    depth = so.depths(v, tri, max_edge, 10)
    parent, leaf_depth = so.recursive_leaf_depths(corners[:, 0], corners[:, 1], corners[:, 2], max_edge, 10)
    c64 = corners.astype(np.float64)
    longest = np.sqrt(np.max(((c64 - np.roll(c64, 1, axis=1)) ** 2).sum(2), axis=1))
    at_leaf = longest * 2.0 ** -depth.astype(np.float64)
    # within 10^-6 relative of the threshold at its own level, or at the parent level from above: the float64 midpoints of the
    # recursion and the closed form may round to different sides there
    band = (np.abs(at_leaf - max_edge) <= 1e-6 * max_edge) | ((2 * at_leaf > max_edge) & (2 * at_leaf - max_edge <= 1e-6 * max_edge)
                                                               & (depth > 0))
    assert band.mean() <= 0.01, int(band.sum())
    n_leaves = np.bincount(parent, minlength=COUNT)
    lo = np.full(COUNT, 99)
    hi = np.full(COUNT, -1)
    np.minimum.at(lo, parent, leaf_depth)
    np.maximum.at(hi, parent, leaf_depth)
    bad = ((n_leaves != 4 ** depth.astype(np.int64)) | (lo != depth) | (hi != depth)) & ~band
    print(f"{COUNT} triangles, depths {np.bincount(depth).tolist()}, left out {int(band.sum())}, disagreeing {int(bad.sum())}")
    assert not bad.any(), np.nonzero(bad)[0][:10]
    assert depth.min() == 0 and depth.max() >= 4                     # the cases cover unsplit triangles and deep ones
    nv, nt = so.counts(depth, 10)
    assert np.array_equal(nt[~band], n_leaves[~band])


def test_index_maps_are_bijections_for_every_n():
    for n in range(1, 1025):
        L = (n + 1) * (n + 2) // 2
        # rows of the lattice: row j holds n - j + 1 points from row_q(j); the rows tile [0, L) in order
        j = np.arange(n + 1)
        start = so.row_q(j, n)
        assert start[0] == 0 and np.array_equal(np.diff(start), n + 1 - j[:-1]) and start[-1] + 1 == L
        # rows of the triangles: row j holds 2(n - j) - 1 triangles from row_tri(j); the rows tile [0, n*n)
        jt = np.arange(n)
        tstart = so.row_tri(jt, n)
        assert tstart[0] == 0 and np.array_equal(np.diff(tstart), 2 * (n - jt[:-1]) - 1) and tstart[-1] + 1 == n * n
        # the decoders at both ends of every row
        for q, want_i in ((start, np.zeros(n + 1, np.int64)), (start + n - j, n - j)):
            gi, gj = so.decode_q(q, n)
            assert np.array_equal(gi, want_i) and np.array_equal(gj, j)
        for l, want_s in ((tstart, np.zeros(n, np.int64)), (tstart + 2 * (n - jt) - 2, 2 * (n - jt) - 2)):
            gj, gs = so.decode_tri(l, n)
            assert np.array_equal(gj, jt) and np.array_equal(gs, want_s)
        if n & (n - 1) and n not in (3, 5, 7, 100, 777, 1023):
            continue
        # every index, both ways, for the n that are used (powers of two) and a few that are not
        i, jj = so.lattice(n)
        assert len(i) == L and i.min() == 0 and jj.min() == 0 and (i + jj).max() == n
        assert np.array_equal(so.row_q(jj, n) + i, np.arange(L))
        assert len(np.unique(i * (n + 1) + jj)) == L                 # L distinct points
        gi, gj = so.decode_q(np.arange(L), n)
        assert np.array_equal(gi, i) and np.array_equal(gj, jj)
        tj, ts = so.local_triangles(n)
        assert len(tj) == n * n and np.array_equal(so.row_tri(tj, n) + ts, np.arange(n * n))
        assert ts.min() == 0 and np.all(ts <= 2 * (n - tj) - 2) and len(np.unique(tj * 2 * n + ts)) == n * n
        gj, gs = so.decode_tri(np.arange(n * n), n)
        assert np.array_equal(gj, tj) and np.array_equal(gs, ts)
        tq = so.triangle_lattice_indices(n)
        assert tq.min() == 0 and tq.max() == L - 1 and len(np.unique(tq)) == L      # every lattice point is used


def test_oracle_mesh_properties():
    """one triangle of depth 3 by hand: 42 new vertices, 64 triangles of the parent's winding whose areas add up"""
    m = 0.01
    v = np.array([(0, 0, 0), (0.03, 0, 0), (0, 0.03, 0), (5, 5, 5)], F)
    out = so.subdivide(v, np.array([(0, 1, 2), (0, 1, 9)]), max_edge=m)
    assert out["depth"].tolist() == [3, 0] and out["vertices"].shape == (4 + 45 - 3, 3) and out["triangles"].shape == (65, 3)
    assert out["triangles"][64].tolist() == [0, 1, 9] and out["index"].tolist() == [0] * 64 + [1]
    p = out["vertices"].astype(np.float64)[out["triangles"][:64]]
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert np.all(nrm[:, 2] > 0) and abs(nrm[:, 2].sum() / 2 - 0.03 * 0.03 / 2) < 1e-9
    assert np.array_equal(out["vertices"][:4], v)
    same = so.subdivide(v[:3] * F(0.1), np.array([(0, 1, 2)]), max_edge=m)
    assert same["depth"].tolist() == [0] and same["vertices"].shape == (3, 3) and same["triangles"].tolist() == [[0, 1, 2]]


def test_source_is_built_with_its_flag_and_exported(lib):
    from morpheus_amd import _lib, build
    assert "subdivide.hip" in build.SOURCES and build.FILE_FLAGS["subdivide.hip"] == ["-ffp-contract=off"]
    assert "mh_subdiv_count" in _lib.EXPORTS and "mh_subdiv_emit" in _lib.EXPORTS
    assert lib.mh_abi_version() == 10


def test_argument_validation_without_gpu(lib):
    """status codes, never exceptions or launches: 1 for bad arguments, 3 for totals past int32, 0 for an empty mesh"""
    count = lambda T, max_edge, max_iter, V=5: lib.mh_subdiv_count(None, V, None, T, max_edge, max_iter, None, None, None, None)  # noqa: E731
    assert count(0, 0.01, 10) == 0
    assert count(2, 0.01, 10) == 1                                   # null pointers
    for bad in (0.0, -0.01, float("nan"), float("inf")):
        assert count(0, bad, 10) == 1
    assert count(0, 0.01, -1) == 1 and count(0, 0.01, 11) == 1 and count(0, 0.01, 0) == 0
    assert count(-1, 0.01, 10) == 1 and count(0, 0.01, 10, V=1 << 31) == 1
    emit = lambda V, T, n_new, n_tri: lib.mh_subdiv_emit(None, None, V, None, T, None, None, None, n_new, n_tri, None, None, None,  # noqa: E731
                                                         None, None)
    assert emit(5, 0, 0, 0) == 0
    assert emit(5, 2, 0, 2) == 1                                     # null pointers
    assert emit(5, 2, -1, 2) == 1 and emit(5, 2, 0, 1) == 1          # fewer output triangles than input ones
    assert emit(5, 2, (1 << 31) - 5, 2) == 3 and emit(5, 2, 0, 1 << 31) == 3 and emit(5, 0, 1 << 31, 0) == 3


def test_module_refuses_cpu_tensors_and_bad_thresholds(lib):
    import torch
    from morpheus_amd import mesheval
    from morpheus_amd._lib import MorpheusHipError
    v, t = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(MorpheusHipError):
        mesheval.subdivide_to_size(v, t)
    with pytest.raises(MorpheusHipError):
        mesheval.cull_mesh(v, t, c2w=np.eye(4), K=np.eye(3), H=4, W=4, depth_gt=torch.zeros(4, 4), subdivide=True)
