"""CPU (no GPU): the numpy restatement of the pooled block-sparse TSDF store (tests/tsdf_sparse_oracle.py) against the dense
restatement (tests/tsdf_oracle.py) on a box both hold, and on a logical box of 2^32 voxels against the analytic surfaces of the
synthetic scene; the canonical mesh order; the host logic of morpheus_amd.tsdf for the sparse store; the new entry points.

The large box is the CPU proof that the inputs tests/test_gpu_tsdf_sparse.py gives the kernels are sound before a GPU sees them.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from tests import tsdf_oracle as to
from tests import tsdf_sparse_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ("mh_tsdf_sparse_group_slots", "mh_tsdf_sparse_max_side_blocks", "mh_tsdf_sparse_mark", "mh_tsdf_sparse_touch",
               "mh_tsdf_sparse_integrate", "mh_tsdf_sparse_to_dense", "mh_tsdf_sparse_from_dense", "mh_mc_sparse_workspace_bytes",
               "mh_mc_count_sparse", "mh_mc_emit_sparse", "mh_tsdf_sparse_vertex_colors")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@functools.lru_cache(maxsize=None)
def surface_bound_voxels():
    """the bound of tests/test_tsdf_host.py::test_fused_scene_lies_on_the_analytic_surfaces on an fp32 mesh of the scene: 3 x the
    float64 restatement's own largest distance to the analytic surfaces, floor 2^-22 (in voxels)"""
    d64 = to.surface_distance(to.extract_mesh(to.fuse_scene(np.float64))[0]) / to.VOXEL
    assert d64.max() < 1.0
    return 3 * float(d64.max()) + 2.0 ** -22


@pytest.mark.parametrize("stride,pixel_centers", [(4, "half"), (1, "integer")])
def test_small_box_is_the_dense_restatement(stride, pixel_centers):
    dense = to.fuse_scene(F, stride=stride, pixel_centers=pixel_centers)
    sparse = so.fuse_scene(F, stride=stride, pixel_centers=pixel_centers)
    got = sparse.to_dense()
    assert np.array_equal(got["active"], dense.active) and 0 < len(sparse.blocks) == int(dense.active.sum()) < dense.active.size
    for k in ("weight", "tsdf", "color"):
        assert np.array_equal(_bits(got[k]), _bits(getattr(dense, k))), k
    # everything outside the allocated blocks is zero in the dense restatement too: the two are one rule
    off = ~np.repeat(np.repeat(np.repeat(dense.active.astype(bool), 8, 0), 8, 1), 8, 2)
    assert (dense.weight[off] == 0).all() and (dense.tsdf[off] == 0).all() and (dense.color[:, off] == 0).all()
    assert np.array_equal(sparse.allocated(), np.flatnonzero(dense.active.reshape(-1)))


def test_large_box_runs_and_lies_on_the_analytic_surfaces():
    s = to.scene()
    assert np.prod(so.LARGE_DIMS, dtype=np.int64) == 2 ** 32
    vol = so.SparseVolume(to.VOXEL, to.TRUNC, so.large_origin(), so.LARGE_DIMS, F)
    union = set()
    for f in range(len(s["c2w"])):
        intr, (c2w, _) = to.host_intrinsics(s["K"]), to.host_pose(s["c2w"][f])
        union.update(vol.touched(s["depth"][f], s["mask"][f], intr, c2w).tolist())
        vol.add_frame(s["depth"][f], s["rgb"][f], s["K"], s["c2w"][f], s["mask"][f])
    assert len(vol.blocks) == len(union) and set(vol.blocks) == union
    verts, tris, colors, iv = vol.extract_mesh()
    dist = to.surface_distance(verts) / to.VOXEL
    print(f"sparse restatement, {so.LARGE_DIMS} box: {len(vol.blocks)} blocks, V {len(verts)} T {len(tris)}, distance to the analytic "
          f"surfaces in voxels max {dist.max():.6f} mean {dist.mean():.6f} (bound {surface_bound_voxels():.6f})")
    assert len(tris) > 3000 and colors.min() >= 0 and colors.max() <= 1
    assert iv.min() >= 8 * min(so.LARGE_SHIFT) - 8 and dist.max() <= surface_bound_voxels()


def test_canonical_order():
    verts, tris, colors, _ = to.extract_mesh(to.fuse_scene(F, frames=range(3)))
    assert len(tris) > 500
    cv, ct, cc = so.canonical(verts, tris, colors)
    assert cv.shape == verts.shape and ct.shape == tris.shape and (ct[:, 0] == ct.min(1)).all()
    assert (np.lexsort((cv[:, 2], cv[:, 1], cv[:, 0])) == np.arange(len(cv))).all()
    # the same surface: every canonical triangle is one of the input's, corner for corner up to a rotation
    key = lambda v, t: sorted(min(tuple(np.roll(v[tri], -r, 0).reshape(-1).tolist()) for r in range(3)) for tri in t)
    assert key(cv, ct) == key(verts, tris)
    rng = np.random.default_rng(5)
    pv, pt = rng.permutation(len(verts)), rng.permutation(len(tris))
    inv = np.empty(len(pv), np.int64)
    inv[pv] = np.arange(len(pv))
    rot = np.stack([np.roll(t, int(r)) for t, r in zip(inv[tris][pt], rng.integers(0, 3, len(tris)))])
    pv2, pt2, pc2 = so.canonical(verts[pv], rot, colors[pv])
    assert np.array_equal(_bits(pv2), _bits(cv)) and np.array_equal(pt2, ct) and np.array_equal(_bits(pc2.astype(F)), _bits(cc.astype(F)))
    flipped = tris.copy()
    flipped[7] = flipped[7, ::-1]
    assert not np.array_equal(so.canonical(verts, flipped)[1], ct)
    with pytest.raises(AssertionError, match="share"):
        so.canonical(np.concatenate([verts, verts[:1]]), tris)
    e = so.canonical(np.zeros((0, 3), F), np.zeros((0, 3), np.int64))
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3) and e[2] is None


def test_sparse_host_logic_without_a_device():
    from morpheus_amd import tsdf
    E = tsdf.MorpheusHipError
    assert tsdf.sparse_bytes((64, 64, 48), 100) == 100 * 10240 + 100 * 4 + 8 * 8 * 6 * 4 + 8
    assert tsdf.sparse_bytes(so.LARGE_DIMS, 200) == 200 * 10244 + 4 * 2 ** 23 + 8
    assert tsdf.sparse_bytes(so.LARGE_DIMS, 200) < 40e6 and tsdf.volume_bytes(so.LARGE_DIMS) > 85e9
    tsdf.check_sparse_box((0, 0, 0), so.LARGE_DIMS, 0.02, 200, 1e9)            # the box the dense store refuses
    with pytest.raises(E, match=r"2\^31 - 1 voxels.*store=\"sparse\""):
        tsdf.check_box((0, 0, 0), so.LARGE_DIMS, 0.02, 1e15)
    # the refusal names the box, the capacity and the bytes, before anything is allocated
    with pytest.raises(E, match=r"2048 x 2048 x 1024 voxels = 8388608 blocks with capacity_blocks = 200000: 2\.08 GB \(2082354440 "
                                r"bytes.*cap of 1\.00 GB.*smaller capacity_blocks"):
        tsdf.check_sparse_box((-1, -1, -1), so.LARGE_DIMS, 0.02, 200000, 1e9)
    side = tsdf.SPARSE_MAX_SIDE_BLOCKS * 8
    assert side >= 2048 and side < 2 ** 24                                      # (float)i exact
    tsdf.check_sparse_box((0, 0, 0), (side, 8, 8), 0.02, 1, 1e9)
    with pytest.raises(E, match=f"a side over {side} voxels"):
        tsdf.check_sparse_box((0, 0, 0), (side + 8, 8, 8), 0.02, 1, 1e15)
    with pytest.raises(E, match=r"2\^31 - 1 blocks"):
        tsdf.check_sparse_box((0, 0, 0), (side, side, 1024), 0.02, 1, 1e15)
    with pytest.raises(E, match="multiples of the block side 8"):
        tsdf.check_sparse_box((0, 0, 0), (60, 64, 64), 0.02, 1, 1e9)
    for bad in (0, -3, 2.5, None, True, 2 ** 31):
        with pytest.raises(E, match="capacity_blocks must be an integer"):
            tsdf.check_sparse_box((0, 0, 0), (8, 8, 8), 0.02, bad, 1e9)
    with pytest.raises(E, match="capacity_blocks must be an integer"):
        tsdf.SparseTSDFVolume(0.02, 0.04, (0, 0, 0), (8, 8, 8), 0, device="cpu")
    with pytest.raises(E, match="no CPU path"):
        tsdf.SparseTSDFVolume(0.02, 0.04, (0, 0, 0), (8, 8, 8), 4, device="cpu")
    with pytest.raises(E, match="must be positive"):
        tsdf.SparseTSDFVolume(0.0, 0.04, (0, 0, 0), (8, 8, 8), 4, device="cpu")
    # store= / capacity_blocks= are checked before any device work
    K = np.array([[10.0, 0, 3.5], [0, 10.0, 2.5], [0, 0, 1]])
    d, rgb = np.ones((5, 7), F), np.zeros((5, 7, 3), F)
    args = (K, 5, 7, [np.eye(4)], [d], [rgb])
    with pytest.raises(E, match=r"store must be one of \('dense', 'sparse'\)"):
        tsdf.run_tsdf_fusion(*args, store="auto")
    with pytest.raises(E, match="the dense store has none"):
        tsdf.run_tsdf_fusion(*args, capacity_blocks=10)
    with pytest.raises(E, match="capacity_blocks must be an integer"):
        tsdf.run_tsdf_fusion(*args, store="sparse", capacity_blocks=0)
    with pytest.raises(E, match="store must be one of"):
        tsdf.back_proj_frame(K, 5, 7, np.eye(4), d, rgb, store="hash")
    with pytest.raises(E, match="no CPU path"):
        tsdf.run_tsdf_fusion(*args, store="sparse", capacity_blocks=10, device="cpu")
    with pytest.raises(TypeError):
        tsdf.run_tsdf_fusion(*args, None, None, None, 1.0, 10.0, 0.04, 0.02, False, "sparse")      # keyword-only


def test_sparse_entry_points_are_declared_and_exported():
    from morpheus_amd import _lib, build, tsdf
    build.build()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "morpheus_hip.h")).read()
    raw = ctypes.CDLL(_lib.SO)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTS and hasattr(raw, name), name
    assert hdr.count("#define MH_ABI_VERSION 10 ") == 1 and lib.mh_abi_version() == 10
    assert "tsdf_sparse.hip" in build.SOURCES and build.FILE_FLAGS["tsdf_sparse.hip"] == ["-ffp-contract=off"]
    P, I32, I64, Fl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    assert list(lib.mh_tsdf_sparse_integrate.argtypes) == [P, P, P, I32, I32, Fl, Fl, Fl, Fl, P, Fl, Fl, Fl, Fl, Fl, Fl, Fl, I32, I32,
                                                           I32, I32, P, P, P, P, P, P]
    assert list(lib.mh_mc_count_sparse.argtypes) == [P, P, P, P, P, I32, I32, I32, I32, Fl, P, P, P]
    assert lib.mh_mc_sparse_workspace_bytes.restype is I64 and lib.mh_tsdf_sparse_group_slots.restype is I32
    # host-only queries and bad arguments: a status, never a launch (no device here)
    assert lib.mh_tsdf_sparse_group_slots() >= 1 and lib.mh_tsdf_sparse_max_side_blocks() == tsdf.SPARSE_MAX_SIDE_BLOCKS
    assert lib.mh_mc_sparse_workspace_bytes(0) == -1 and lib.mh_mc_sparse_workspace_bytes(10) >= 10 * 512 * 5
    w = np.eye(4, dtype=np.float32)[:3].copy()
    wp = w.ctypes.data_as(ctypes.c_void_p)
    one = ctypes.c_void_p(64)                                       # a non-null pointer that is never followed: the checks come first
    frame = (4, 4, 1.0, 1.0, 2.0, 2.0, wp, 1.0, 10.0)
    box = (0.0, 0.0, 0.0, 0.02, 0.04)
    assert lib.mh_tsdf_sparse_touch(one, None, *frame, 4, *box, 256, 256, 128, 0, one, one, one, None) == 1       # capacity 0
    assert lib.mh_tsdf_sparse_touch(one, None, *frame, 4, *box, 4097, 1, 1, 8, one, one, one, None) == 1          # a side too long
    assert lib.mh_tsdf_sparse_touch(one, None, *frame, 4, *box, 2048, 2048, 512, 8, one, one, one, None) == 1     # 2^31 blocks
    assert lib.mh_tsdf_sparse_touch(one, None, *frame, 4, *box, 256, 256, 128, 8, None, one, one, None) == 1      # no index volume
    assert lib.mh_tsdf_sparse_touch(one, None, *frame, 0, *box, 256, 256, 128, 8, one, one, one, None) == 1       # stride 0
    assert lib.mh_tsdf_sparse_mark(one, None, *frame, 4, *box, 4097, 1, 1, one, None) == 1
    assert lib.mh_tsdf_sparse_mark(one, None, *frame, 4, *box, 256, 256, 128, None, None) == 1
    assert lib.mh_tsdf_touch(one, None, *frame, 4, *box, 256, 256, 128, one, None) == 1       # the dense touch still refuses the box
    assert lib.mh_tsdf_sparse_integrate(one, None, None, *frame, *box, 1, 1, 1, 8, one, one, one, one, one, None) == 1      # no rgb
    assert lib.mh_tsdf_sparse_integrate(one, one, None, *frame, *box, 1, 1, 1, 8, one, None, one, one, one, None) == 1      # no counters
    assert lib.mh_tsdf_sparse_to_dense(256, 256, 128, 8, one, one, one, one, one, one, one, one, one, None) == 1   # no dense box
    assert lib.mh_tsdf_sparse_to_dense(8, 8, 8, 0, one, one, one, one, one, one, one, one, one, None) == 1
    assert lib.mh_tsdf_sparse_from_dense(one, one, one, None, None, 256, 256, 128, 8, one, one, one, one, one, one, None) == 1
    assert lib.mh_tsdf_sparse_from_dense(None, one, one, None, None, 8, 8, 8, 8, one, one, one, one, one, one, None) == 1
    assert lib.mh_mc_count_sparse(one, one, one, one, one, 8, 8, 8, 0, 0.0, one, one, None) == 1
    assert lib.mh_mc_count_sparse(one, one, one, None, one, 8, 8, 8, 4, 0.0, one, one, None) == 1
    assert lib.mh_mc_emit_sparse(one, one, one, one, one, 8, 8, 8, 4, 0.0, one, None, one, None) == 1
    assert lib.mh_tsdf_sparse_vertex_colors(None, 0, None, None, 8, 8, 8, 4, None, None) == 0                      # empty: fine
    assert lib.mh_tsdf_sparse_vertex_colors(None, 5, None, None, 8, 8, 8, 4, None, None) == 1
    assert lib.mh_tsdf_sparse_vertex_colors(None, 0, None, None, 8, 8, 8, 0, None, None) == 1
