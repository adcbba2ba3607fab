"""GPU: the pooled block-sparse TSDF store (csrc/tsdf_sparse.hip, morpheus_amd.tsdf.SparseTSDFVolume) against the dense store's
restatement tests/tsdf_oracle.py bit for bit after every frame, against tests/tsdf_sparse_oracle.py on a logical box of 2^32
voxels that the dense store refuses, its marching cubes against the masked pair of csrc/mesh.hip in canonical order, the
overflow path, the frame loop under graph capture and run_tsdf_fusion(store="sparse")."""
import functools

import numpy as np
import pytest
import torch

from tests import raster_oracle as ro
from tests import tsdf_oracle as to
from tests import tsdf_sparse_oracle as so

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F = np.float32


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(gpu: torch.Tensor, want: np.ndarray, what):
    w = torch.from_numpy(np.ascontiguousarray(want)).to(DEV)
    assert gpu.shape == w.shape and gpu.dtype == w.dtype, (what, gpu.shape, w.shape, gpu.dtype, w.dtype)
    assert torch.equal(_bits(gpu), _bits(w)), (what, int((_bits(gpu) != _bits(w)).sum()))


def _extra_frames(h, w):
    """a camera inside the box and one that sees none of it (looking away from far outside)"""
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    depth_in = (0.25 + 0.1 * np.sin(ii / 17.0) * np.cos(jj / 13.0)).astype(F)
    rgb = np.stack([ii % 256, jj % 256, (ii + jj) % 256], -1).astype(np.uint8)
    inside = ro.cv2gl_pose(ro.look_at((0.3, 0.25, 0.1), (0.0, 0.0, -0.1)))
    away = ro.cv2gl_pose(ro.look_at((5.0, 5.0, 5.0), (10.0, 10.0, 10.0)))
    return [(inside, depth_in, rgb, None), (away, np.full((h, w), 1.0, F), rgb, None)]


def _frames(pixel_centers):
    s = to.scene()
    K = s["K"].copy()
    if pixel_centers == "integer":
        K[:2, 2] -= 0.5
    frames = [(s["c2w"][f], s["depth"][f], s["rgb"][f], s["mask"][f]) for f in range(len(s["c2w"]))]
    frames[3:3] = _extra_frames(to.H, to.W)
    return K, frames


@functools.lru_cache(maxsize=1)
def _dense_reference(stride, pixel_centers, dims):
    """the dense restatement after every frame: [(active, weight, tsdf, color)], shared by the capacities of one configuration"""
    K, frames = _frames(pixel_centers)
    want = to.Volume(to.VOXEL, to.TRUNC, to.SCENE_ORIGIN, dims, F)
    out = []
    for c2w, depth, rgb, mask in frames:
        want.add_frame(depth, rgb, K, c2w, mask, stride=stride, pixel_centers=pixel_centers)
        out.append((want.active.copy(), want.weight.copy(), want.tsdf.copy(), want.color.copy()))
    return out


def _check_index(vol):
    """slot_block restricted to the counter is a bijection onto the blocks with a slot; -> the number of allocated blocks"""
    n, overflow = vol.counters.tolist()
    assert not overflow and 0 <= n <= vol.capacity
    slot = vol.slot.reshape(-1)
    have = torch.nonzero(slot >= 0).flatten()
    sb = vol.slot_block[:n].long()
    assert int((slot < -1).sum()) == 0 and have.numel() == n
    assert torch.equal(sb.sort().values, have) and torch.equal(slot[sb].long(), torch.arange(n, device=DEV))
    return n


@pytest.mark.parametrize("capacity", ["exact", "larger"])
@pytest.mark.parametrize("stride,pixel_centers,dims", [(4, "half", (64, 64, 48)), (1, "integer", (64, 64, 48)),
                                                       (4, "integer", (64, 64, 64)), (1, "half", (64, 64, 64))])
def test_volume_after_each_frame_equals_the_dense_one(stride, pixel_centers, dims, capacity):
    from morpheus_amd import _lib, tsdf
    group = _lib.load().mh_tsdf_sparse_group_slots()
    ref = _dense_reference(stride, pixel_centers, dims)
    cap = int(ref[-1][0].sum())                                     # exactly what the frames reach
    if capacity == "larger":
        cap += 1 if (cap + 1) % group else 2
        assert group > 1 and cap % group != 0                       # the last workgroup of integrate is a partial one
    K, frames = _frames(pixel_centers)
    vol = tsdf.SparseTSDFVolume(to.VOXEL, to.TRUNC, to.SCENE_ORIGIN, dims, cap, device=DEV)
    for f, (c2w, depth, rgb, mask) in enumerate(frames):
        vol.integrate(depth, rgb, K, c2w, mask, stride=stride, pixel_centers=pixel_centers)
        d = vol.to_dense()
        for k, want in zip(("active", "weight", "tsdf", "color"), ref[f]):
            _same(getattr(d, k), want, (k, f))
        assert _check_index(vol) == int(ref[f][0].sum())
    assert torch.equal(vol.allocated_blocks(), torch.nonzero(d.active.reshape(-1)).flatten())
    assert 0.2 < float(d.active.float().mean()) < 0.9 and float(d.weight.max()) >= 4


@functools.lru_cache(maxsize=None)
def _surface_bound():
    """world units: the rule of tests/test_tsdf_host.py (3 x the float64 restatement's own distance to the analytic surfaces,
    floor 2^-22 voxels)"""
    d64 = to.surface_distance(to.extract_mesh(to.fuse_scene(np.float64))[0])
    assert d64.max() < to.VOXEL
    return 3 * float(d64.max()) + 2.0 ** -22 * to.VOXEL


def _fuse(vol, stride=4):
    s = to.scene()
    for f in range(len(s["c2w"])):
        vol.integrate(s["depth"][f], s["rgb"][f], s["K"], s["c2w"][f], s["mask"][f], stride=stride)
    return vol


def test_the_box_the_dense_store_refuses():
    from morpheus_amd import tsdf
    origin = so.large_origin()
    with pytest.raises(tsdf.MorpheusHipError, match=r"2\^31 - 1 voxels"):
        tsdf.TSDFVolume(to.VOXEL, to.TRUNC, origin, so.LARGE_DIMS, device=DEV, max_gb=1e6)
    want = so.fuse_scene(F, origin=origin, dims=so.LARGE_DIMS)
    ids = want.allocated()
    vol = _fuse(tsdf.SparseTSDFVolume(to.VOXEL, to.TRUNC, origin, so.LARGE_DIMS, len(ids), device=DEV))
    assert _check_index(vol) == len(ids)
    _same(vol.allocated_blocks(), ids, "allocated blocks")
    with pytest.raises(tsdf.MorpheusHipError, match=r"2\^31 - 1 voxels"):
        vol.to_dense()
    rows = np.array([want.blocks[b] for b in ids.tolist()])
    slots = vol.slot.reshape(-1)[torch.from_numpy(ids).to(DEV)].long()
    _same(vol.weight[slots], want.weight[rows].reshape(-1, 512), "weight")
    _same(vol.tsdf[slots], want.tsdf[rows].reshape(-1, 512), "tsdf")
    _same(vol.color[:, slots], want.color[rows].transpose(1, 0, 2, 3, 4).reshape(3, -1, 512), "color")
    m = vol.extract_mesh()
    dist = to.surface_distance(m["vertices"].cpu().numpy())
    print(f"sparse store, {so.LARGE_DIMS} box: {len(ids)} blocks ({tsdf.sparse_bytes(so.LARGE_DIMS, len(ids)) / 1e6:.1f} MB), V "
          f"{m['vertices'].shape[0]} T {m['triangles'].shape[0]}, distance to the analytic surfaces in voxels max "
          f"{dist.max() / to.VOXEL:.6f} (bound {_surface_bound() / to.VOXEL:.6f})")
    assert m["triangles"].shape[0] > 3000 and dist.max() <= _surface_bound()
    assert int(m["triangles"].max()) < m["vertices"].shape[0] and float(m["colors"].min()) >= 0 and float(m["colors"].max()) <= 1


def _noise_volume(dims, rng):
    """a dense volume of noise with scattered unobserved points, NaN weights included (the generator of tests/test_gpu_tsdf.py)"""
    from morpheus_amd import tsdf
    vol = tsdf.TSDFVolume(1.0, 2.0, (0.0, 0.0, 0.0), dims, device=DEV)
    w = (rng.random(dims) > 0.15).astype(F) * 3
    w[rng.random(dims) < 0.02] = np.nan
    vol.tsdf.copy_(torch.from_numpy(rng.normal(size=dims).astype(F)))
    vol.weight.copy_(torch.from_numpy(w))
    vol.color.copy_(torch.from_numpy((rng.random((3,) + dims) * 255).astype(F)))
    return vol


def _canonical(mesh_or_tuple):
    v, t, c = (mesh_or_tuple[k] for k in ("vertices", "triangles", "colors")) if isinstance(mesh_or_tuple, dict) else mesh_or_tuple
    return so.canonical(v.cpu().numpy(), t.cpu().numpy(), c.cpu().numpy())


def _assert_canonical_equal(a, b, what):
    for x, y, k in zip(a, b, ("vertices", "triangles", "colors")):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape)
        same = np.array_equal(x.view(np.int32), y.view(np.int32)) if x.dtype == np.float32 else np.array_equal(x, y)
        assert same, (what, k)


@pytest.mark.parametrize("keep_kind", ["all", "one", "some"])
@pytest.mark.parametrize("dims", [(8, 8, 8), (16, 8, 24), (32, 32, 32)])
def test_sparse_marching_cubes_against_the_masked_pair(dims, keep_kind):
    from morpheus_amd import mesh, tsdf
    rng = np.random.default_rng(17 + sum(dims))
    dense = _noise_volume(dims, rng)
    nb = dense.blocks
    n = int(np.prod(nb))
    keep = np.ones(nb, np.uint8)
    if keep_kind == "one":
        keep[:] = 0
        keep.reshape(-1)[n // 2] = 1
    elif keep_kind == "some":
        keep = (rng.random(nb) < 0.6).astype(np.uint8)
        keep.reshape(-1)[n - 1] = 1
    k8 = torch.from_numpy(np.repeat(np.repeat(np.repeat(keep, 8, 0), 8, 1), 8, 2)).to(DEV).bool()
    # the masked pair over the dense volume with the dropped blocks unobserved
    v, t = mesh.marching_cubes_masked(dense.tsdf, torch.where(k8, dense.weight, torch.zeros_like(dense.weight)))
    want = _canonical((v, t, dense.vertex_colors(v)))
    vol = tsdf.SparseTSDFVolume.from_dense(dense, keep)
    assert _check_index(vol) == int(keep.sum()) == vol.capacity
    iv, tri = vol.marching_cubes()
    assert (len(tri) > 0) == (len(want[1]) > 0) and (keep_kind != "all" or len(tri) > 100)
    _assert_canonical_equal(_canonical((iv, tri, vol.vertex_colors(iv))), want, (dims, keep_kind))
    m1, m2 = vol.extract_mesh(), vol.extract_mesh()
    other = tsdf.SparseTSDFVolume.from_dense(dense, keep, capacity_blocks=int(keep.sum()) + 3,
                                             block_order=torch.from_numpy(rng.permutation(n)))
    back = tsdf.SparseTSDFVolume.from_dense(dense, keep, block_order=torch.arange(n - 1, -1, -1))
    m3, m4 = other.extract_mesh(), back.extract_mesh()
    for k in ("vertices", "triangles", "colors"):
        # two runs, and two other assignments of slots: the same bytes without canonicalising
        assert torch.equal(_bits(m1[k]), _bits(m2[k])) and torch.equal(_bits(m1[k]), _bits(m3[k])) and torch.equal(_bits(m1[k]), _bits(m4[k])), k
    # and the round trip: to_dense gives the kept blocks' bytes back
    d = vol.to_dense()
    _same(d.active, keep, "active")
    assert torch.equal(_bits(d.tsdf), _bits(torch.where(k8, dense.tsdf, torch.zeros_like(dense.tsdf))))
    assert torch.equal(_bits(d.weight), _bits(torch.where(k8, dense.weight, torch.zeros_like(dense.weight))))
    assert torch.equal(_bits(d.color), _bits(torch.where(k8[None], dense.color, torch.zeros_like(dense.color))))


@functools.lru_cache(maxsize=None)
def _dense_scene_mesh():
    from morpheus_amd import tsdf
    vol = _fuse(tsdf.TSDFVolume(to.VOXEL, to.TRUNC, to.SCENE_ORIGIN, to.SCENE_DIMS, device=DEV))
    return int(vol.active.sum()), _canonical(vol.extract_mesh())


def test_fused_scene_mesh_equals_the_dense_one():
    from morpheus_amd import tsdf
    needed, want = _dense_scene_mesh()
    vol = _fuse(tsdf.SparseTSDFVolume(to.VOXEL, to.TRUNC, to.SCENE_ORIGIN, to.SCENE_DIMS, needed, device=DEV))
    assert vol.check() == needed and len(want[1]) > 3000
    _assert_canonical_equal(_canonical(vol.extract_mesh()), want, "scene")


def test_overflow_is_reported_and_later_volumes_are_sound():
    from morpheus_amd import tsdf
    needed, want = _dense_scene_mesh()
    small = _fuse(tsdf.SparseTSDFVolume(to.VOXEL, to.TRUNC, to.SCENE_ORIGIN, to.SCENE_DIMS, needed // 2, device=DEV))
    torch.cuda.synchronize()                                        # the frame loop completed
    for call in (small.check, small.allocated_blocks, small.to_dense, small.extract_mesh):
        with pytest.raises(tsdf.MorpheusHipError, match=f"capacity_blocks = {needed // 2} slots is full.*reached {needed} blocks.*"
                                                        f"capacity_blocks >= {needed}"):
            call()
    wanted, overflow = small.counters.tolist()
    slot = small.slot.reshape(-1)
    assert overflow == 1 and wanted == needed and int((slot >= 0).sum()) == needed // 2 and int(slot.max()) == needed // 2 - 1
    vol = _fuse(tsdf.SparseTSDFVolume(to.VOXEL, to.TRUNC, to.SCENE_ORIGIN, to.SCENE_DIMS, needed, device=DEV))
    _assert_canonical_equal(_canonical(vol.extract_mesh()), want, "after an overflow")


def test_sparse_frame_loop_runs_under_graph_capture():
    """No host synchronisation per frame: the loop is captured into a HIP graph on one stream and the replay leaves the bytes of
    the dense restatement."""
    from morpheus_amd import tsdf
    s = to.scene()
    n = 4
    depth = [torch.from_numpy(s["depth"][f]).to(DEV) for f in range(n)]
    rgb = [torch.from_numpy(s["rgb"][f]).to(DEV) for f in range(n)]
    mask = [None if s["mask"][f] is None else torch.from_numpy(s["mask"][f]).to(DEV) for f in range(n)]
    want = to.fuse_scene(F, frames=range(n))
    vol = tsdf.SparseTSDFVolume(to.VOXEL, to.TRUNC, to.SCENE_ORIGIN, to.SCENE_DIMS, int(want.active.sum()) + 5, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for f in range(n):
            vol.integrate(depth[f], rgb[f], s["K"], s["c2w"][f], mask[f])
    torch.cuda.synchronize()
    assert vol.counters.tolist() == [0, 0] and float(vol.weight.max()) == 0       # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert _check_index(vol) == int(want.active.sum())
    d = vol.to_dense()
    for k in ("active", "weight", "tsdf", "color"):
        _same(getattr(d, k), getattr(want, k), k)
    assert float(d.weight.max()) >= 3
    del g


def test_run_tsdf_fusion_sparse(tmp_path):
    from morpheus_amd import mesh as pmesh, tsdf
    s = to.scene()
    lo, hi = np.array(to.SCENE_ORIGIN) + to.TRUNC, np.array(to.SCENE_ORIGIN) + np.array(to.SCENE_DIMS) * to.VOXEL - to.TRUNC
    args = (s["K"], to.H, to.W, s["c2w"], s["depth"], s["rgb"], s["mask"])
    kw = dict(voxel_length=to.VOXEL, sdf_trunc=to.TRUNC, pixel_centers="half", device=DEV)
    dense = tsdf.run_tsdf_fusion(*args, bounds=(lo, hi), **kw)
    sparse, vol = tsdf.run_tsdf_fusion(*args, bounds=(lo, hi), store="sparse", return_volume=True, **kw)
    assert isinstance(vol, tsdf.SparseTSDFVolume) and vol.check() == vol.capacity                   # sized exactly
    assert sparse["triangles"].shape[0] > 3000
    _assert_canonical_equal(_canonical(sparse), _canonical(dense), "run_tsdf_fusion")
    # the box sized from the frames, through back_proj_frame
    one = tsdf.back_proj_frame(s["K"], to.H, to.W, s["c2w"][0], s["depth"][0], s["rgb"][0], **kw)
    one_s = tsdf.back_proj_frame(s["K"], to.H, to.W, s["c2w"][0], s["depth"][0], s["rgb"][0], store="sparse", **kw)
    assert one["vertices"].shape[0] > 500
    _assert_canonical_equal(_canonical(one_s), _canonical(one), "back_proj_frame")
    # the large box: refused densely, fused sparsely, written and read back
    origin = so.large_origin()
    big = (origin + to.TRUNC, origin + np.array(so.LARGE_DIMS) * to.VOXEL - to.TRUNC - 0.5 * to.VOXEL)
    assert tsdf.box_from_bounds(big[0], big[1], to.VOXEL, to.TRUNC)[1] == so.LARGE_DIMS
    with pytest.raises(tsdf.MorpheusHipError, match=r"2\^31 - 1 voxels.*store=\"sparse\""):
        tsdf.run_tsdf_fusion(*args, bounds=big, **kw)
    path = tmp_path / "bg" / "room.ply"
    m, vol = tsdf.run_tsdf_fusion(*args, bounds=big, store="sparse", save_path=str(path), return_volume=True, **kw)
    assert vol.dims == so.LARGE_DIMS and vol.check() == vol.capacity and m["triangles"].shape[0] > 3000
    assert to.surface_distance(m["vertices"].cpu().numpy()).max() <= _surface_bound()
    pv, pt, pc = pmesh.read_ply(str(path))
    assert np.array_equal(pv, m["vertices"].cpu().numpy()) and np.array_equal(pt, m["triangles"].cpu().numpy())
    assert np.abs(pc - m["colors"].cpu().numpy()).max() <= 0.5 / 255 + 1e-7
    # a pool too small is reported by the call itself (extract_mesh reads the flag)
    with pytest.raises(tsdf.MorpheusHipError, match="slots is full"):
        tsdf.run_tsdf_fusion(*args, bounds=(lo, hi), store="sparse", capacity_blocks=10, **kw)
