"""GPU: TSDF fusion on the HIP kernels (csrc/tsdf.hip) and the masked marching cubes (csrc/mesh.hip) against the numpy
restatement tests/tsdf_oracle.py bit for bit; depth maps of this project's rasteriser fused and rendered back; the multi-mesh
render_mesh_from_view; the frame loop under graph capture (a host synchronisation there is an error)."""
import numpy as np
import pytest
import torch

from tests import mc_oracle as mo
from tests import raster_oracle as ro
from tests import tsdf_oracle as to

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


@pytest.mark.parametrize("stride,pixel_centers,dims", [(4, "half", (64, 64, 48)), (1, "integer", (64, 64, 48)),
                                                       (4, "integer", (64, 64, 64)), (1, "half", (64, 64, 64))])
def test_volume_after_each_frame_bit_identical(stride, pixel_centers, dims):
    from morpheus_amd import _lib, tsdf
    group = _lib.load().mh_tsdf_group_blocks()
    assert (48 // 8) % group != 0 and (64 // 8) % group == 0        # box sizes on and off the workgroup's block count
    s = to.scene()
    K = s["K"].copy()
    if pixel_centers == "integer":
        K[:2, 2] -= 0.5
    frames = [(s["c2w"][f], s["depth"][f], s["rgb"][f], s["mask"][f]) for f in range(len(s["c2w"]))]
    frames[3:3] = _extra_frames(to.H, to.W)
    want = to.Volume(to.VOXEL, to.TRUNC, to.SCENE_ORIGIN, dims, F)
    vol = tsdf.TSDFVolume(to.VOXEL, to.TRUNC, to.SCENE_ORIGIN, dims, device=DEV)
    for f, (c2w, depth, rgb, mask) in enumerate(frames):
        want.add_frame(depth, rgb, K, c2w, mask, stride=stride, pixel_centers=pixel_centers)
        vol.integrate(depth, rgb, K, c2w, mask, stride=stride, pixel_centers=pixel_centers)
        _same(vol.active, want.active, ("active", f))
        _same(vol.weight, want.weight, ("weight", f))
        _same(vol.tsdf, want.tsdf, ("tsdf", f))
        _same(vol.color, want.color, ("color", f))
    assert 0.2 < float(vol.active.float().mean()) < 0.9 and float(vol.weight.max()) >= 4


def _fused(stride=4):
    from morpheus_amd import tsdf
    s = to.scene()
    vol = tsdf.TSDFVolume(to.VOXEL, to.TRUNC, to.SCENE_ORIGIN, to.SCENE_DIMS, device=DEV)
    for f in range(len(s["c2w"])):
        vol.integrate(s["depth"][f], s["rgb"][f], s["K"], s["c2w"][f], s["mask"][f], stride=stride)
    return vol


def test_masked_marching_cubes_and_colours_bit_identical():
    from morpheus_amd import mesh
    vol = _fused()
    tsdf_h, weight_h, color_h = vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.color.cpu().numpy()
    ov, ot = to.masked_marching_cubes(tsdf_h, weight_h)
    v, t = mesh.marching_cubes_masked(vol.tsdf, vol.weight)
    _same(v, ov, "vertices")
    _same(t, ot, "triangles")
    assert len(ot) > 3000
    _same(vol.vertex_colors(v), to.vertex_colors(ov, color_h), "colors")
    m1, m2 = vol.extract_mesh(), vol.extract_mesh()
    for k in ("vertices", "triangles", "colors"):
        assert torch.equal(m1[k], m2[k]), k                         # two runs, the same bytes
    world, _, colors, _ = to.extract_mesh(to.fuse_scene(F))
    _same(m1["vertices"], world, "world vertices")
    _same(m1["colors"], colors, "world colours")
    # noise volumes with scattered unobserved points, NaN weights included
    rng = np.random.default_rng(11)
    for shape in ((37, 41, 29), (2, 3, 2), (33, 2, 65)):
        f = rng.normal(size=shape).astype(F)
        w = (rng.random(shape) > 0.15).astype(F) * 3
        w[rng.random(shape) < 0.02] = np.nan
        ov, ot = to.masked_marching_cubes(f, w)
        v, t = mesh.marching_cubes_masked(torch.from_numpy(f).to(DEV), torch.from_numpy(w).to(DEV))
        _same(v, ov, shape)
        _same(t, ot, shape)


def test_all_weights_positive_equals_the_unmasked_pair():
    from morpheus_amd import mesh
    for vol in (mo.gaussians((64, 64, 64), np.random.default_rng(9)), mo.torus((48, 52, 30), (23.6, 25.2, 14.3), 14.5, 6.2)):
        x = torch.from_numpy(vol).to(DEV)
        v0, t0 = mesh.marching_cubes(x)
        v1, t1 = mesh.marching_cubes_masked(x, torch.full_like(x, 2.0))
        assert len(t0) > 0 and torch.equal(_bits(v0), _bits(v1)) and torch.equal(t0, t1)
    e = mesh.marching_cubes_masked(x, torch.zeros_like(x))
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3)


def test_rasterised_depth_fused_and_rendered_back():
    """This project's rasteriser -> run_tsdf_fusion -> mesh -> rasteriser.  Bound: the rule of tests/test_tsdf_host.py (3 x the
    float64 restatement's own distance to the analytic surfaces on this scene, measured here again), plus the spacing of the
    surface samples for the distance to the source mesh."""
    from morpheus_amd import mesheval, meshrender, tsdf
    s = to.scene()
    verts, tris = s["mesh"]
    d64 = to.extract_mesh(to.fuse_scene(np.float64))[0]
    bound = 3 * float(to.surface_distance(d64).max())               # world units
    assert bound < 3 * to.VOXEL
    V, T = torch.from_numpy(verts).to(DEV), torch.from_numpy(tris).to(DEV)
    col = torch.from_numpy(to.scene_color(verts).astype(F) / 255).to(DEV)
    K = s["K"]
    depths, rgbs = [], []
    for c2w in s["c2w"]:
        out = meshrender.render_mesh(V, T, col, c2w=c2w, K=K, H=to.H, W=to.W, convention="opencv", mode="color")
        depths.append(out["depth"])
        rgbs.append(out["image"])
    lo, hi = np.array(to.SCENE_ORIGIN) + to.TRUNC, np.array(to.SCENE_ORIGIN) + np.array(to.SCENE_DIMS) * to.VOXEL - to.TRUNC
    before = [d.clone() for d in depths]
    mesh = tsdf.run_tsdf_fusion(K, to.H, to.W, s["c2w"], depths, rgbs, bounds=(lo, hi), voxel_length=to.VOXEL, sdf_trunc=to.TRUNC,
                                pixel_centers="half", device=DEV)
    assert all(torch.equal(a, b) for a, b in zip(before, depths))   # inputs left as they were
    assert mesh["vertices"].shape[0] > 3000
    n_samples = 400000
    pts, _ = mesheval.sample_surface(V, T, n_samples, seed=0)
    spacing = float(np.sqrt(mo.area(verts, tris) / n_samples))
    _, d2 = mesheval.nearest(mesh["vertices"], pts)
    dist = d2.sqrt()
    print(f"fused from rasterised depth: V {mesh['vertices'].shape[0]}, distance to the source mesh in voxels: max "
          f"{float(dist.max()) / to.VOXEL:.4f} mean {float(dist.mean()) / to.VOXEL:.4f} (bound {bound / to.VOXEL:.4f} + spacing "
          f"{spacing / to.VOXEL:.4f})")
    assert float(dist.max()) <= bound + spacing
    c = mesh["colors"]
    assert float(c.min()) >= 0 and float(c.max()) <= 1
    for f in (0, to.MASKED_FRAME, to.N_CAMERAS - 1):
        back = meshrender.render_mesh(mesh["vertices"], mesh["triangles"], c, c2w=s["c2w"][f], K=K, H=to.H, W=to.W,
                                      convention="opencv", mode="color")
        both = (back["depth"] > 0) & (depths[f] > 0)
        err = (back["depth"] - depths[f]).abs()[both]
        out_share = float((err > bound).float().mean())
        print(f"frame {f} rendered back: {int(both.sum())} pixels covered by both, depth error max {float(err.max()):.5f} median "
              f"{float(err.median()):.5f}, share beyond the bound (silhouettes) {out_share:.4f}")
        # the box's ground square fills about half of an arc camera's image (tests/test_tsdf_host.py measures 0.50 - 0.56)
        assert float(both.float().mean()) > 0.4 and out_share <= 0.02


def test_render_mesh_from_view_back_proj_frame_and_ply(tmp_path):
    from morpheus_amd import mesh as pmesh, meshrender, mesheval, tsdf
    s = to.scene()
    K = s["K"]
    sv, st = ro.icosphere(2, 0.2)
    fg = {"vertices": torch.from_numpy(sv).to(DEV), "triangles": torch.from_numpy(st).to(DEV),
          "colors": torch.rand(len(sv), 3, device=DEV), "transform": np.array([[0, -1, 0, 0.1], [1, 0, 0, -0.05], [0, 0, 1, 0.2],
                                                                             [0, 0, 0, 1.0]])}
    path = tmp_path / "bg" / "bg.ply"
    bg = tsdf.back_proj_frame(K, to.H, to.W, s["c2w"][0], s["depth"][0], s["rgb"][0].astype(F) / 255, save_path=str(path),
                              voxel_length=to.VOXEL, sdf_trunc=to.TRUNC, pixel_centers="half", device=DEV)
    one = tsdf.run_tsdf_fusion(K, to.H, to.W, [s["c2w"][0]], [s["depth"][0]], [s["rgb"][0].astype(F) / 255],
                               voxel_length=to.VOXEL, sdf_trunc=to.TRUNC, pixel_centers="half", device=DEV)
    assert bg["vertices"].shape[0] > 500
    for k in ("vertices", "triangles", "colors"):
        assert torch.equal(bg[k], one[k]), k
    pv, pt, pc = pmesh.read_ply(str(path))
    assert np.array_equal(pv, bg["vertices"].cpu().numpy()) and np.array_equal(pt, bg["triangles"].cpu().numpy())
    assert np.abs(pc - bg["colors"].cpu().numpy()).max() <= 0.5 / 255 + 1e-7
    # the scene by hand
    moved = mesheval.transform_points(fg["vertices"], fg["transform"])
    hv = torch.cat([moved, bg["vertices"]])
    ht = torch.cat([fg["triangles"], bg["triangles"] + len(sv)])
    hc = torch.cat([fg["colors"], bg["colors"]])
    c2w = s["c2w"][1]
    for mode, native, colors in (("color", "color", hc), ("gray", "shaded", None), ("normal", "normal", None)):
        got = meshrender.render_mesh_from_view([fg, bg], c2w, K, to.H, to.W, mode=mode, return_result=True)
        want = meshrender.render_mesh(hv, ht, colors, c2w=c2w, K=K, H=to.H, W=to.W, convention="opencv", mode=native)
        for k in ("depth", "tri_id", "image"):
            assert torch.equal(got[k], want[k]), (mode, k)
        assert int((got["tri_id"] >= 0).sum()) > 1000 and int(((got["tri_id"] >= 0) & (got["tri_id"] < len(st))).sum()) > 50
    img = meshrender.render_mesh_from_view([fg, bg], c2w, K, to.H, to.W, mode="color")
    assert img.shape == (to.H, to.W, 3) and img.dtype == torch.float32
    with pytest.raises(tsdf.MorpheusHipError, match="mode"):
        meshrender.render_mesh_from_view([fg], c2w, K, to.H, to.W, mode="depth")
    # empty inputs: no frames, no usable pixel
    e = tsdf.run_tsdf_fusion(K, to.H, to.W, [], [], [], device=DEV)
    assert e["vertices"].shape == (0, 3) and e["triangles"].shape == (0, 3)
    e = tsdf.run_tsdf_fusion(K, to.H, to.W, [s["c2w"][0]], [np.zeros((to.H, to.W), F)], [s["rgb"][0]], device=DEV)
    assert e["vertices"].shape == (0, 3)
    # the box is sized from the frames, and refused when it does not fit
    with pytest.raises(tsdf.MorpheusHipError, match="bounds="):
        tsdf.run_tsdf_fusion(K, to.H, to.W, s["c2w"], s["depth"], s["rgb"], voxel_length=to.VOXEL, max_gb=0.001, device=DEV)
    lo, hi = tsdf.frame_bounds(K, s["c2w"][:1], s["depth"][:1], pixel_centers="half", stride=1, device=DEV)
    want = to.Volume(to.VOXEL, to.TRUNC, (0, 0, 0), (8, 8, 8)).back_project(s["depth"][0], None, to.host_intrinsics(K),
                                                                           to.host_pose(s["c2w"][0])[0], 1.0, 10.0, 1)
    assert np.array_equal(lo, want.min(0)) and np.array_equal(hi, want.max(0))


def test_frame_loop_runs_under_graph_capture():
    """No host synchronisation per frame: the loop is captured into a HIP graph (a synchronising call inside a capture is an
    error) and the replay leaves the bytes of the eager run."""
    from morpheus_amd import tsdf
    s = to.scene()
    n = 4
    depth = [torch.from_numpy(s["depth"][f]).to(DEV) for f in range(n)]
    rgb = [torch.from_numpy(s["rgb"][f]).to(DEV) for f in range(n)]
    mask = [None if s["mask"][f] is None else torch.from_numpy(s["mask"][f]).to(DEV) for f in range(n)]
    eager = tsdf.TSDFVolume(to.VOXEL, to.TRUNC, to.SCENE_ORIGIN, to.SCENE_DIMS, device=DEV)
    vol = tsdf.TSDFVolume(to.VOXEL, to.TRUNC, to.SCENE_ORIGIN, to.SCENE_DIMS, device=DEV)

    def loop(v):
        for f in range(n):
            v.integrate(depth[f], rgb[f], s["K"], s["c2w"][f], mask[f])

    loop(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loop(vol)
    torch.cuda.synchronize()
    assert float(vol.weight.max()) == 0                             # captured, not run
    g.replay()
    torch.cuda.synchronize()
    for k in ("active", "tsdf", "weight", "color"):
        assert torch.equal(_bits(getattr(vol, k)), _bits(getattr(eager, k))), k
    assert float(vol.weight.max()) >= 3
    del g
