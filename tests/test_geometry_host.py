"""Host: morpheus_amd.geometry, the bottom layer of the mesh tool chain.  The layering of the five modules, read from their
source with ast; the camera functions against the three independent numpy restatements the oracles keep (raster_oracle,
mesheval_oracle, tsdf_oracle), byte for byte."""
import ast
import os

import numpy as np
import pytest
import torch

from morpheus_amd import geometry, mesheval, meshrender, tsdf
from morpheus_amd._lib import MorpheusHipError
from tests import mesheval_oracle as eo
from tests import raster_oracle as ro
from tests import tsdf_oracle as to

PKG = os.path.dirname(os.path.abspath(geometry.__file__))
# module -> the modules of the chain it may import: geometry <- mesh <- tsdf, geometry <- meshrender <- mesheval (+ mesh)
MAY_IMPORT = {"geometry": set(), "mesh": {"geometry"}, "tsdf": {"geometry", "mesh"}, "meshrender": {"geometry", "mesh"},
              "mesheval": {"geometry", "mesh", "meshrender"}}
MUST_IMPORT = {"geometry": set(), "mesh": {"geometry"}, "tsdf": {"geometry", "mesh"}, "meshrender": {"geometry"},
               "mesheval": {"geometry", "meshrender"}}


def _package_imports(node):
    """the morpheus_amd modules an import statement names (relative, or absolute through the package's name)"""
    if isinstance(node, ast.ImportFrom) and (node.level > 0 or (node.module or "").split(".")[0] == "morpheus_amd"):
        path = (node.module or "").split(".") if node.level > 0 else node.module.split(".")[1:]
        return {path[0]} if path and path[0] else {a.name for a in node.names}
    if isinstance(node, ast.Import):
        return {a.name.split(".")[1] for a in node.names if a.name.startswith("morpheus_amd.")}
    return set()


def _parsed(name):
    with open(os.path.join(PKG, name + ".py")) as fh:
        return ast.parse(fh.read())


@pytest.mark.parametrize("name", sorted(MAY_IMPORT))
def test_layering(name):
    tree = _parsed(name)
    inside = [(fn.name, n.lineno) for fn in ast.walk(tree) if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef))
              for n in ast.walk(fn) if isinstance(n, (ast.Import, ast.ImportFrom)) and _package_imports(n)]
    assert not inside, f"{name}.py imports from the package inside a function body: {inside}"
    imported = set().union(*(_package_imports(n) for n in ast.walk(tree)))       # none inside a function: all at module level
    assert imported & set(MAY_IMPORT) <= MAY_IMPORT[name], (name, imported)
    assert MUST_IMPORT[name] <= imported, (name, imported)
    if name == "geometry":
        assert imported == {"_lib", "chunking"}, imported


def _rigid_poses(n, seed=0):
    rng = np.random.default_rng(seed)
    poses = []
    for _ in range(n):
        q, r = np.linalg.qr(rng.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = q, rng.uniform(-3, 3, 3)
        poses.append(m)
    return poses


def _same(got, want, dtype):
    assert isinstance(got, np.ndarray) and got.dtype == dtype and got.shape == (3, 4) and got.flags.c_contiguous
    assert np.array_equal(got, want)
    return True


def test_cameras_same_bytes_as_the_oracles():
    checked = 0
    for m in _rigid_poses(200):
        forms = [(m, m), (m[:3].astype(np.float32),) * 2, (torch.from_numpy(m).float(), m.astype(np.float32)),
                 (torch.from_numpy(m.copy()), m)]
        for given, as_array in forms:
            for convention in ("opengl", "opencv"):
                want = ro.world_to_camera(as_array, convention)
                _same(geometry.world_to_camera(given, convention), want, np.float32)
                _same(meshrender.world_to_camera(given, convention), want, np.float32)
            want64 = eo.world_to_camera_f64(as_array)
            _same(geometry.world_to_camera(given, "opengl", np.float64), want64, np.float64)
            _same(mesheval.world_to_camera_f64(given), want64, np.float64)
            for got, want in zip(geometry.pose_pair(given), to.host_pose(as_array)):
                checked += _same(got, want, np.float32)
            assert np.array_equal(geometry.pose_pair(given)[1], geometry.world_to_camera(given, "opencv"))
            assert np.array_equal(geometry.cv2gl(geometry.cv2gl(as_array)), np.asarray(as_array, np.float64))
    assert checked == 200 * 4 * 2
    assert tsdf._pose is geometry.pose_pair
    assert np.array_equal(meshrender.cv2gl(m), eo.cv2gl(m)) and not np.array_equal(meshrender.cv2gl(m), m)


def test_pose_errors_and_intrinsics():
    for bad in (np.eye(3), np.zeros((4, 3)), torch.zeros(2, 4, 4)):
        for fn in (geometry.world_to_camera, geometry.pose_pair, meshrender.world_to_camera, mesheval.world_to_camera_f64):
            with pytest.raises(MorpheusHipError, match=r"c2w must be \[4,4\] or \[3,4\]"):
                fn(bad)
    for fn in (geometry.world_to_camera, meshrender.world_to_camera):
        with pytest.raises(MorpheusHipError, match="convention must be 'opengl' or 'opencv', got 'blender'"):
            fn(np.eye(4), "blender")
    K = np.array([[10.0, 0, 3.5], [0, 11.0, 2.5], [0, 0, 1]])
    for given in (K, K.astype(np.float32), torch.from_numpy(K), torch.from_numpy(K).float(), K.tolist()):
        got = geometry.intrinsics(given)
        assert got == (10.0, 11.0, 3.5, 2.5) and all(type(x) is float for x in got)
    assert tsdf._intrinsics(torch.from_numpy(K), "integer") == (10.0, 11.0, 4.0, 3.0)
    a = geometry.host_array(torch.arange(6).reshape(2, 3).t(), np.float64)
    assert a.flags.c_contiguous and a.dtype == np.float64 and a.shape == (3, 2)
    assert geometry.host_ptr(a).value == a.ctypes.data
    assert geometry.host_array(a, np.float64) is a
