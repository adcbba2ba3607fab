"""GPU: marching cubes on the HIP kernels (csrc/mesh.hip) against the numpy restatement tests/mc_oracle.py bit for bit, a
512^3 sphere checked on the device, and mesh export from a model (morpheus_amd.mesh) against the reference's loop."""
import math

import numpy as np
import pytest
import torch

from tests import mc_oracle as mo

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _gpu_mc(vol, iso=0.0):
    from morpheus_amd import mesh
    v, t = mesh.marching_cubes(torch.from_numpy(np.ascontiguousarray(vol)).to(DEV), iso)
    assert v.dtype == torch.float32 and t.dtype == torch.int64
    return v.cpu().numpy(), t.cpu().numpy()


def _same_as_oracle(vol, iso=0.0):
    v, t = _gpu_mc(vol, iso)
    ov, ot = mo.marching_cubes(vol, iso)
    assert v.shape == ov.shape and t.shape == ot.shape, (v.shape, ov.shape, t.shape, ot.shape)
    assert np.array_equal(v.view(np.uint32), ov.view(np.uint32))          # bit for bit (NaN-free by construction)
    assert np.array_equal(t, ot)
    return v, t


@pytest.mark.parametrize("shape,iso,seed", [((37, 41, 29), 0.0, 0), ((2, 3, 2), 0.0, 1), ((33, 2, 65), 0.25, 2),
                                            ((17, 130, 19), -0.5, 3)])
def test_noise_volume_bit_identical(shape, iso, seed):
    rng = np.random.default_rng(seed)
    vol = rng.normal(size=shape).astype(np.float32)
    r = rng.random(shape)
    vol[r < 0.05] = np.float32(iso)                         # exactly on the isovalue: outside
    vol[(r >= 0.05) & (r < 0.07)] = np.nan
    vol[(r >= 0.07) & (r < 0.08)] = np.inf
    vol[(r >= 0.08) & (r < 0.09)] = -np.inf
    v, t = _same_as_oracle(vol, iso)
    assert t.shape[0] > 0 or min(shape) == 2


def test_shapes_bit_identical():
    _same_as_oracle(mo.sphere((40, 44, 38), (19.3, 21.7, 18.6), 13.1))
    _same_as_oracle(mo.torus((48, 52, 30), (23.6, 25.2, 14.3), 14.5, 6.2))
    _same_as_oracle(mo.plane((45, 39, 51), (0.3, -0.8, 0.5), 7.0)[0])
    _same_as_oracle(mo.gaussians((40, 36, 44), np.random.default_rng(5)))


def test_all_positive_volume_is_empty():
    v, t = _gpu_mc(np.full((9, 10, 11), 2.0, np.float32))
    assert v.shape == (0, 3) and t.shape == (0, 3)


def test_deterministic():
    from morpheus_amd import mesh
    vol = torch.from_numpy(mo.gaussians((64, 64, 64), np.random.default_rng(9))).to(DEV)
    v1, t1 = mesh.marching_cubes(vol)
    v2, t2 = mesh.marching_cubes(vol)
    assert torch.equal(v1, v2) and torch.equal(t1, t2)


def test_sphere_512_closed_on_device():
    from morpheus_amd import mesh
    n, r = 512, 231.7
    c = torch.tensor([255.3, 256.6, 254.9], dtype=torch.float64, device=DEV)
    ax = torch.arange(n, dtype=torch.float64, device=DEV)
    vol = torch.empty(n, n, n, dtype=torch.float32, device=DEV)
    for i in range(0, n, 64):                                # in slabs: float64 coordinates of 512^3 points are 3 GB
        x = ax[i:i + 64].view(-1, 1, 1) - c[0]
        vol[i:i + 64] = (torch.sqrt(x * x + (ax.view(1, -1, 1) - c[1]) ** 2 + (ax.view(1, 1, -1) - c[2]) ** 2) - r).float()
    v, t = mesh.marching_cubes(vol)
    del vol
    V, T = v.shape[0], t.shape[0]
    e = torch.cat([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]).sort(1).values
    keys, uses = torch.unique(e[:, 0] * V + e[:, 1], return_counts=True)
    assert bool((uses == 2).all())
    assert torch.unique(t).numel() == V
    assert V - keys.numel() + T == 2
    vd = v.double()
    a, b, cc = vd[t[:, 0]], vd[t[:, 1]], vd[t[:, 2]]
    vol_signed = float((a * torch.cross(b, cc, dim=1)).sum() / 6.0)
    assert abs(vol_signed / (4 / 3 * math.pi * r ** 3) - 1) < 1e-3, vol_signed


def _reference_sdf(model, resolution, S, t, cano):
    """morpheus.py:385-395 with each sub-grid kept on the device"""
    sdf = torch.zeros(resolution, resolution, resolution, device=DEV)
    X = torch.linspace(-1, 1, resolution).split(S)
    with torch.no_grad():
        for xi, xs in enumerate(X):
            for yi, ys in enumerate(X):
                for zi, zs in enumerate(X):
                    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                    pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                    val = model.density(pts.to(DEV), t=t, cano=cano)
                    sdf[xi * S: xi * S + len(xs), yi * S: yi * S + len(ys), zi * S: zi * S + len(zs)] = \
                        val["sdf"].reshape(len(xs), len(ys), len(zs))
    return sdf


@pytest.fixture(scope="module")
def model():
    from morpheus_amd import harness
    return harness.build_model("b", DEV)


@pytest.mark.parametrize("t,cano", [(None, False), (25 / 200, False), (25 / 200, True)])
def test_extract_mesh_matches_reference_loop(model, t, cano):
    from morpheus_amd import mesh
    res, S = 96, 32
    out = mesh.extract_mesh(model, resolution=res, S=S, t=t, cano=cano)
    sdf = _reference_sdf(model, res, S, t, cano)
    assert torch.equal(out["sdf"], sdf)
    ov, ot = mo.marching_cubes(sdf.cpu().numpy(), 0.0)
    assert ot.shape[0] > 100, ot.shape                      # the field has a surface in the box
    want_v = torch.from_numpy(ov).to(DEV) / (res - 1.0) * 2 - 1
    assert torch.equal(out["vertices"], want_v)
    assert np.array_equal(out["triangles"].cpu().numpy(), ot)
    with torch.no_grad():
        albedo = model.density(out["vertices"], t=t, cano=cano)["albedo"]
    assert out["colors"].shape == (ov.shape[0], 3) and torch.equal(out["colors"], albedo)


def test_export_mesh_writes_what_extract_mesh_returns(model, tmp_path):
    from morpheus_amd import mesh
    path = str(tmp_path / "sub" / "mesh_0000.ply")
    got = mesh.export_mesh(model, path, resolution=64, S=64, t=0.3)
    want = mesh.extract_mesh(model, resolution=64, S=64, t=0.3)
    assert torch.equal(got["vertices"], want["vertices"]) and torch.equal(got["triangles"], want["triangles"])
    header, verts, faces = mo.read_ply(path)
    assert header[2] == f"element vertex {want['vertices'].shape[0]}"
    xyz = np.stack([verts["x"], verts["y"], verts["z"]], 1)
    assert np.array_equal(xyz, want["vertices"].cpu().numpy())
    assert np.array_equal(faces, want["triangles"].cpu().numpy())
    rgb = np.stack([verts["red"], verts["green"], verts["blue"]], 1)
    c = want["colors"].cpu().numpy().astype(np.float64)
    assert np.array_equal(rgb, np.rint(np.clip(c, 0, 1) * 255).astype(np.uint8))
