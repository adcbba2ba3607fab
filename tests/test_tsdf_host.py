"""CPU (no GPU): the numpy restatement of the TSDF fusion (tests/tsdf_oracle.py) against closed forms and against geometry that
does not depend on its conventions, the masked marching cubes of the restatement against tests/mc_oracle.py, and the host
logic of morpheus_amd.tsdf.

Figures of test_fused_scene_lies_on_the_analytic_surfaces (run with -s to print them; recorded in profiles/r10_tsdf_fusion.txt):
the synthetic scene (icosphere r = 0.3 on the plane z = -0.3, 12 cameras on a circle turned 0.37 rad off the box's axes and one
above, 160 x 120, f = 140, voxel_length 0.02, sdf_trunc 0.04, 64 x 64 x 48 box, stride 4, 51 % of the blocks active) gives 7 730
vertices / 14 352 triangles whose distance to the analytic surfaces is, in voxels, max 0.399023 / mean 0.061815 in float64 and in
fp32 alike; no cell changes its sign pattern between the two dtypes, 2 voxels read another pixel in fp32 (each within 1e-4
pixels of a pixel boundary), and off those the fp32 vertices lie within 8.94e-06 voxels of the float64 ones.  Rendered back by the
numpy rasteriser, frames 0, 1 (the masked one) and 12 (from above) give their depth maps back within 3 x 0.399 voxels = 0.0239
on all but 0.55 %, 0.44 % and 0.44 % of the pixels both cover (cap: 2 %).
Two properties of the conventions shaped the scene (both are the reference's defaults, sdf_trunc = 2 voxels, at work): a surface
seen only at more than ~60 degrees from its normal keeps its first interior voxel behind -sdf_trunc, i.e. unobserved, and the
masked marching cubes leaves a hole there -- with 6 arc cameras and none above, the sphere's top and the face toward the masked
camera had such holes and 2.4 - 3.0 % of the pixels were beyond the bound; and the ground must be tessellated, since the ray
caster and the rasteriser drop a triangle with a vertex behind the camera whole.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import mc_oracle as mo
from tests import raster_oracle as ro
from tests import tsdf_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ("mh_mc_masked_workspace_bytes", "mh_mc_count_masked", "mh_mc_emit_masked", "mh_tsdf_group_blocks",
               "mh_tsdf_bounds", "mh_tsdf_touch", "mh_tsdf_integrate", "mh_tsdf_vertex_colors")


def _plane_frame(h=48, w=64, f=60.0, depth=1.0):
    """a camera at the origin looking down +z (OpenCV: the identity pose) at the fronto-parallel plane z = depth"""
    K = np.array([[f, 0, w / 2.0], [0, f, h / 2.0], [0, 0, 1.0]])
    return K, np.eye(4), np.full((h, w), depth, F), np.full((h, w, 3), 200, np.uint8)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fronto_parallel_plane_closed_form(dtype):
    K, c2w, depth, rgb = _plane_frame()
    vl, trunc = 0.02, 0.04
    # the optical axis passes through voxel centres: x = y = 0 is the centre of voxel 8 of 16 when the origin is -8.5 voxels
    vol = to.Volume(vl, trunc, (-8.5 * vl, -8.5 * vl, 0.5), (16, 16, 48), dtype)
    vol.add_frame(depth, rgb, K, c2w, stride=1)
    z = vol.origin[2].astype(np.float64) + (np.arange(48) + 0.5) * np.float64(F(vl))
    axis_t, axis_w = vol.tsdf[8, 8], vol.weight[8, 8]
    want = np.minimum(1.0, (1.0 - z) / np.float64(F(trunc)))
    seen = (1.0 - z) > -np.float64(F(trunc))
    active = np.repeat(vol.active[1, 1].astype(bool), 8)
    assert active.any() and not active.all()                       # untouched blocks exist on the axis
    assert np.array_equal(axis_w > 0, seen & active)               # behind -sdf_trunc and in untouched blocks: weight 0
    tol = 0.0 if dtype is np.float64 else 4e-6
    # on the axis the pixel is the principal one up to half a pixel: m = sqrt(1 + 2 (0.5 / f)^2)
    m = np.sqrt(1.0 + 2 * (0.5 / 60.0) ** 2)
    want_m = np.minimum(1.0, (1.0 - z) * m / np.float64(F(trunc)))
    assert np.abs(axis_t[axis_w > 0] - want_m[axis_w > 0]).max() <= max(tol, 1e-12)
    assert np.abs(want_m - want).max() < 1e-3                      # and that is min(1, (d - z) / trunc) to the ray's obliqueness
    assert (vol.weight[~np.repeat(np.repeat(np.repeat(vol.active.astype(bool), 8, 0), 8, 1), 8, 2)] == 0).all()
    assert set(np.unique(vol.weight)) <= {0.0, 1.0}
    before = vol.tsdf.copy(), vol.color.copy()
    vol.add_frame(depth, rgb, K, c2w, stride=1)
    assert set(np.unique(vol.weight)) <= {0.0, 2.0}                # w counts frames
    assert np.abs(vol.tsdf - before[0]).max() <= tol and np.abs(vol.color - before[1]).max() <= 200 * tol
    assert set(np.unique(vol.color[:, vol.weight > 0])) == {200.0} or dtype is np.float32


def test_masked_marching_cubes_of_the_restatement():
    rng = np.random.default_rng(3)
    for vol in (mo.sphere((24, 26, 22), (11.3, 12.7, 10.6), 7.1), mo.torus((32, 34, 20), (15.6, 16.2, 9.3), 9.5, 4.2),
                mo.gaussians((20, 24, 22), rng, k=20)):
        ov, ot = mo.marching_cubes(vol)
        v, t = to.masked_marching_cubes(vol, np.ones_like(vol))
        assert np.array_equal(v.view(np.uint32), ov.view(np.uint32)) and np.array_equal(t, ot)
        # a half-space (and a few scattered points) unobserved
        weight = np.ones_like(vol)
        weight[vol.shape[0] // 2:] = 0
        weight[rng.random(vol.shape) < 0.01] = 0
        v, t = to.masked_marching_cubes(vol, weight)
        assert 0 < len(t) < len(ot)
        # no vertex on an edge with an unobserved end
        p0 = np.floor(v).astype(np.int64)
        axis = np.argmax(v - np.floor(v) > 0, 1)
        p1 = p0.copy()
        frac = (v - np.floor(v)).max(1) > 0
        p1[np.arange(len(v)), axis] += frac
        assert (weight[p0[:, 0], p0[:, 1], p0[:, 2]] > 0).all() and (weight[p1[:, 0], p1[:, 1], p1[:, 2]] > 0).all()
        assert np.unique(t).size == len(v)                         # a cell without all corners owns no vertex: none is unused
        # the surviving triangles are the unmasked ones of the valid cells: as coordinate triples a sub-sequence of the
        # unmasked list, as many as the table gives the valid cells
        key = lambda vv, tt: [tuple(vv[tri].reshape(-1).tolist()) for tri in tt]
        full, part = key(ov, ot), key(v, t)
        it = iter(full)
        assert all(any(k == x for x in it) for k in part)
        inside = vol < 0
        nx, ny, nz = vol.shape
        cube = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
        for c, (dx, dy, dz) in enumerate(mo.CORNER):
            cube |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
        ntri = (mo.TABLE[cube] >> np.uint64(60)).astype(np.int64)
        assert len(t) == int(ntri[to.valid_cells(weight)].sum())


def test_fused_scene_lies_on_the_analytic_surfaces():
    """Geometric truth, independent of the conventions: every vertex of the mesh fused from the synthetic frames against the
    closed-form surfaces the frames were cast from.  fp32 gate: DESIGN 4 (3 x the float64 restatement's own figure, floor
    2^-22 relative); the float64 figure is only held to one voxel (more means a convention error, not round-off)."""
    out = {}
    for dt in (np.float64, np.float32):
        pix = []
        vol = to.fuse_scene(dt, on_frame=lambda f, v: pix.append((v.last_pixel.copy(), [np.asarray(x, np.float64) for x in v.last_u])))
        verts, tris, colors, iv = to.extract_mesh(vol)
        dist = to.surface_distance(verts) / to.VOXEL
        out[dt] = dict(vol=vol, verts=verts, tris=tris, iv=iv, pix=pix, max=float(dist.max()), mean=float(dist.mean()))
        print(f"tsdf scene {dt.__name__}: V {len(verts)} T {len(tris)} distance to the analytic surfaces in voxels: max "
              f"{dist.max():.6f} mean {dist.mean():.6f}; active blocks {vol.active.mean():.3f}")
        assert len(verts) > 3000 and colors.min() >= 0 and colors.max() <= 1
    d64, d32 = out[np.float64], out[np.float32]
    assert d64["max"] < 1.0, d64                                    # sanity bound of the conventions
    floor = 2.0 ** -22
    assert d32["max"] <= 3 * d64["max"] + floor and d32["mean"] <= 3 * d64["mean"] + floor
    # companion gate: same triangle set, vertices within 1e-3 voxels -- but for the voxels whose projection lies within round-off
    # of a pixel boundary, where the two dtypes read different depth pixels (counted, and shown to be exactly that)
    sign_diff = int(((d64["vol"].tsdf < 0) != (d32["vol"].tsdf < 0))[(d64["vol"].weight > 0)].sum())
    flipped = np.zeros(d64["vol"].dims, bool)
    for (p64, uv), (p32, _) in zip(d64["pix"], d32["pix"]):
        diff = p64 != p32
        if diff.any():
            with np.errstate(all="ignore"):
                gap = np.minimum(np.abs(uv[0] - np.round(uv[0])), np.abs(uv[1] - np.round(uv[1])))[diff]
            assert gap.max() < 1e-4, gap.max()                      # a pixel boundary within fp32 round-off of the projection
        flipped |= diff
    print(f"tsdf scene: cells whose sign differs between the dtypes {sign_diff}; voxels that read another pixel in fp32 "
          f"{int(flipped.sum())}")
    assert sign_diff == 0
    assert np.array_equal(d64["tris"], d32["tris"])
    p0 = np.floor(d64["iv"]).astype(np.int64)
    p1 = np.ceil(d64["iv"]).astype(np.int64)
    clean = ~(flipped[p0[:, 0], p0[:, 1], p0[:, 2]] | flipped[p1[:, 0], p1[:, 1], p1[:, 2]])
    delta = np.abs(d64["verts"].astype(np.float64) - d32["verts"])[clean].max() / to.VOXEL
    print(f"tsdf scene: fp32 vertices against float64 on the {int(clean.sum())} of {len(clean)} vertices off such voxels: "
          f"{delta:.2e} voxels")
    assert clean.mean() > 0.98 and delta <= 1e-3
    # the restatement alone, rendered back (numpy rasteriser of tests/raster_oracle.py): the fused mesh gives each training
    # camera its depth map back within the same bound, but for the pixels at silhouettes -- at most 2 % of those both cover
    s = to.scene()
    K = s["K"]
    bound = 3 * d64["max"] * to.VOXEL
    for f in (0, to.MASKED_FRAME, to.N_CAMERAS - 1):
        keys, _ = ro.rasterize(d32["verts"], d32["tris"], to.host_pose(s["c2w"][f])[1], K[0, 0], K[1, 1], K[0, 2], K[1, 2], to.H, to.W)
        depth, _ = ro.decode(keys)
        both = (depth > 0) & (s["depth"][f] > 0) & (s["depth"][f] <= 10.0)
        err = np.abs(depth - s["depth"][f])[both]
        share = float((err > bound).mean())
        print(f"tsdf scene: frame {f} rendered back: {int(both.sum())} pixels covered by both, depth error median {np.median(err):.5f}, "
              f"share beyond {bound:.4f} (silhouettes) {share:.4f}")
        assert both.mean() > 0.4 and share <= 0.02               # the box's ground square fills about half of an arc camera's image


def test_bounds_words_decode_and_box():
    from morpheus_amd import tsdf
    vals = np.array([-1.5, 0.0, 2.25, -0.0, 3.0, 1e-3], F)
    bits = vals.view(np.int32)
    words = np.where(bits >= 0, bits, bits ^ np.int32(0x7fffffff))
    assert words[0] < words[3] < words[1] < words[5]                # ordered like the values, -0 below +0
    lo, hi = tsdf.decode_bounds(words)
    assert np.array_equal(lo, vals[:3]) and np.array_equal(hi.view(np.uint32), vals[3:].view(np.uint32))
    assert tsdf.decode_bounds(np.array([2 ** 31 - 1] * 3 + [-2 ** 31] * 3, np.int64).astype(np.int32)) is None
    origin, dims = tsdf.box_from_bounds((0, 0, 0), (1.0, 0.1, 0.33), 0.02, 0.04)
    assert np.allclose(origin, -0.04) and dims == (56, 16, 24)      # ceil(1.08 / 0.16) = 7 blocks, 2, 3
    assert all(o + d * 0.02 >= h + 0.04 for o, d, h in zip(origin, dims, (1.0, 0.1, 0.33)))
    with pytest.raises(tsdf.MorpheusHipError, match="finite"):
        tsdf.box_from_bounds((0, 0, 0), (np.nan, 1, 1), 0.02, 0.04)


def test_host_logic_without_a_device():
    from morpheus_amd import tsdf
    E = tsdf.MorpheusHipError
    # the memory refusal names the box, the voxel count and the two ways out, before anything is allocated
    assert tsdf.volume_bytes((512, 512, 512)) == 512 ** 3 * 20 + 64 ** 3
    tsdf.check_box((0, 0, 0), (64, 64, 64), 0.02, 1e9)
    with pytest.raises(E, match=r"512 x 512 x 512 = 134217728 voxels.*2\.68 GB.*cap of 1\.00 GB.*bounds=.*larger voxel_length"):
        tsdf.check_box((-5.12, -5.12, -5.12), (512, 512, 512), 0.02, 1e9)
    with pytest.raises(E, match=r"2\^31 - 1 voxels"):
        tsdf.check_box((0, 0, 0), (2048, 2048, 512), 0.02, 1e15)
    with pytest.raises(E, match="multiples of the block side 8"):
        tsdf.check_box((0, 0, 0), (60, 64, 64), 0.02, 1e9)
    # colour preparation: truncation, gray_scale, intensity_scale, alpha; inputs left as they were
    rng = np.random.default_rng(0)
    rgb = rng.random((5, 7, 3)).astype(np.float32)
    keep = rgb.copy()
    assert np.array_equal(tsdf.rgb8(rgb).numpy(), (keep * 255).astype(np.uint8))
    gray = tsdf.rgb8(rgb, gray_scale=True).numpy()
    assert np.array_equal(gray[..., 0], gray[..., 1]) and np.array_equal(gray[..., 0], gray[..., 2])
    assert np.abs(gray[..., 0].astype(np.float64) - np.floor(keep.astype(np.float64).mean(-1) * 255)).max() <= 1
    assert np.array_equal(tsdf.rgb8(rgb, intensity_scale=0.5).numpy(), ((keep * 0.5) * 255).astype(np.uint8))
    assert np.array_equal(tsdf.rgb8(rgb, alpha=0.25).numpy(), ((keep * 0.25 + 0.75) * 255).astype(np.uint8))
    u8 = (keep * 255).astype(np.uint8)
    assert np.array_equal(tsdf.rgb8(u8).numpy(), u8)
    assert np.array_equal(rgb, keep)
    mask = rng.normal(size=(5, 7, 2))
    assert np.array_equal(tsdf.mask8(mask).numpy(), (mask[:, :, 0] > 0).astype(np.uint8)) and tsdf.mask8(None) is None
    # argument checks come before any device work
    K = np.array([[10.0, 0, 3.5], [0, 10.0, 2.5], [0, 0, 1]])
    d = np.ones((5, 7), np.float32)
    args = (K, 5, 7, [np.eye(4)], [d], [rgb])
    with pytest.raises(E, match="1 poses, 2 depth maps"):
        tsdf.run_tsdf_fusion(K, 5, 7, [np.eye(4)], [d, d], [rgb])
    with pytest.raises(E, match="pixel_centers"):
        tsdf.run_tsdf_fusion(*args, pixel_centers="centre")
    with pytest.raises(E, match="must be positive"):
        tsdf.run_tsdf_fusion(*args, voxel_length=0.0)
    with pytest.raises(E, match=r"expected \(6, 7\)"):
        tsdf.run_tsdf_fusion(K, 6, 7, [np.eye(4)], [d], [rgb])
    with pytest.raises(E, match="no CPU path"):
        tsdf.run_tsdf_fusion(*args, device="cpu")
    with pytest.raises(E, match="no CPU path"):
        tsdf.TSDFVolume(0.02, 0.04, (0, 0, 0), (8, 8, 8), device="cpu")
    with pytest.raises(E, match="save_as_pcd"):
        tsdf.back_proj_frame(K, 5, 7, np.eye(4), d, rgb, save_as_pcd=True)
    assert np.array_equal(rgb, keep) and (d == 1).all()
    assert tsdf._intrinsics(K, "integer") == (10.0, 10.0, 4.0, 3.0) and tsdf._intrinsics(K, "half") == (10.0, 10.0, 3.5, 2.5)


def test_new_entry_points_are_declared_and_exported():
    import ctypes
    from morpheus_amd import _lib, build
    build.build()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "morpheus_hip.h")).read()
    raw = ctypes.CDLL(_lib.SO)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTS and hasattr(raw, name), name
    assert hdr.count("#define MH_ABI_VERSION 10 ") == 1 and lib.mh_abi_version() == 10
    P, I32, I64, Fl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    assert list(lib.mh_tsdf_integrate.argtypes) == [P, P, P, I32, I32, Fl, Fl, Fl, Fl, P, Fl, Fl, Fl, Fl, Fl, Fl, Fl, I32, I32, I32,
                                                    P, P, P, P, P]
    assert list(lib.mh_mc_count_masked.argtypes) == [P, P, I32, I32, I32, Fl, P, P, P] and lib.mh_tsdf_group_blocks.restype is I32
    # bad arguments: a status, never a launch (no device here)
    assert lib.mh_tsdf_group_blocks() >= 1
    assert lib.mh_mc_masked_workspace_bytes(1, 8, 8) == -1
    assert lib.mh_mc_masked_workspace_bytes(16, 16, 16) == lib.mh_mc_workspace_bytes(16, 16, 16) + 4096
    assert lib.mh_mc_count_masked(None, None, 8, 8, 8, 0.0, None, None, None) == 1
    assert lib.mh_mc_emit_masked(None, 8, 8, 8, 0.0, None, None, None, None) == 1
    w = np.eye(4, dtype=np.float32)[:3].copy()
    wp = w.ctypes.data_as(ctypes.c_void_p)
    one = ctypes.c_void_p(64)                                       # a non-null pointer that is never followed: the checks come first
    frame = (4, 4, 1.0, 1.0, 2.0, 2.0, wp, 1.0, 10.0)
    assert lib.mh_tsdf_bounds(None, None, *frame, 4, one, None) == 1                        # no depth
    assert lib.mh_tsdf_bounds(one, None, *frame, 0, one, None) == 1                         # stride 0
    assert lib.mh_tsdf_bounds(one, None, 4, 4, 0.0, 1.0, 2.0, 2.0, wp, 1.0, 10.0, 4, one, None) == 1     # fx = 0
    box = (0.0, 0.0, 0.0, 0.02, 0.04)
    assert lib.mh_tsdf_touch(one, None, *frame, 4, *box, 0, 1, 1, one, None) == 1           # no blocks
    assert lib.mh_tsdf_touch(one, None, *frame, 4, 0.0, 0.0, 0.0, 0.0, 0.04, 1, 1, 1, one, None) == 1    # voxel_length 0
    assert lib.mh_tsdf_touch(one, None, *frame, 4, *box, 256, 256, 64, one, None) == 1      # 2^31 voxels
    assert lib.mh_tsdf_integrate(one, None, None, *frame, *box, 1, 1, 1, one, one, one, one, None) == 1   # no rgb
    assert lib.mh_tsdf_integrate(one, one, None, 4, 20000, 1.0, 1.0, 2.0, 2.0, wp, 1.0, 10.0, *box, 1, 1, 1, one, one, one, one,
                                 None) == 1                                                  # W out of range
    assert lib.mh_tsdf_vertex_colors(None, 0, None, 8, 8, 8, None, None) == 0               # empty: fine
    assert lib.mh_tsdf_vertex_colors(None, 5, None, 8, 8, 8, None, None) == 1
    assert lib.mh_tsdf_vertex_colors(None, -1, None, 8, 8, 8, None, None) == 1
