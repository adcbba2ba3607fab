"""CPU (no GPU): the host side of morpheus_amd.preprocess and the restatement tests/preprocess_oracle.py against the reference's own
results (tests/golden/preprocess.npz, recorded by tools/make_preprocess_golden.py from preprocess/preprocess.py:DataProcessor and
preprocess/pose_init/create_camera.py).

Everything recorded is a chain of rounded operators that the CPU here runs as the reference's CPU did, so every comparison with the
golden is BIT FOR BIT: the four planes of both runs, the crop centres, the virtual poses, both r / theta / phi tables, K_virt, the
polar chains on generic poses and the cameras of the pose initialisation.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import preprocess_oracle as P


@pytest.fixture(scope="module")
def g():
    return P.load_golden()


def inputs(g):
    return {k[3:]: g[k] for k in g if k.startswith("in_")}


def run_scale(radius):
    return float(np.float32(1.0) / np.float32(radius))


def test_golden_holds_the_cases_the_definition_turns_on(g):
    i = inputs(g)
    assert os.path.getsize(P.GOLDEN) < 100_000
    assert all(np.issubdtype(v.dtype, np.number) for v in g.values())
    for k, v in P.make_inputs().items():      # the shared definition of the inputs is what the golden was recorded from
        assert np.array_equal(i[k], v) and i[k].dtype == v.dtype, k
    assert i["rgb"].shape == (P.F, P.H, P.W, 3) and i["rgb"].min() == 0 and i["rgb"].max() == 255
    assert set(np.unique(i["mask"])) == {0, 128, 254, 255}
    for tag, h, w, radius in P.RUNS:
        centres = g[tag + "centres"]
        assert centres.tolist() == [[int(x), int(y)] for x, y in P.TARGETS]      # int() towards zero: (-1.5, -0.5) -> (-1, 0)
        origin = P.window_origins(centres, h, w)
        assert tuple(P.window_kind(t, l, h, w, P.H, P.W) for t, l in origin) == P.KINDS
        assert g[tag + "rgb"].shape == (P.F, h, w, 3) and g[tag + "depth"].dtype == np.uint16
        assert set(np.unique(g[tag + "padding"])) == {0, 255}
        assert not g[tag + "padding"][0].any() and not g[tag + "padding"][1].any() and g[tag + "padding"][3].any()
    for kind, (py, px, h, w) in P.EXCLUDED.items():
        top, left = P.window_origins([(px, py)], h, w)[0]
        assert P.window_kind(top, left, h, w, P.H, P.W) == kind
        assert P.crop_centres(g["ex_" + kind + "_pose"][None], i["K"][:1]).tolist() == [[px, py]]


@pytest.mark.parametrize("run", range(len(P.RUNS)))
def test_oracle_equals_the_reference_on_every_recorded_array(g, run):
    tag, h, w, radius = P.RUNS[run]
    i = inputs(g)
    centres = P.crop_centres(i["poses"], i["K"])
    assert centres.dtype == np.int64 and np.array_equal(centres, g[tag + "centres"])
    tin, tpad = P.depth_tables(P.DEPTH_SCALE, run_scale(radius))
    o = P.prep_frames(i["rgb"], i["depth"], i["mask"], P.window_origins(centres, h, w), np.zeros((P.F, 6)), np.zeros(P.F, np.uint8),
                      tin, tpad, h, w)
    for k in ("rgb", "depth", "mask", "padding"):
        assert o[k].dtype == g[tag + k].dtype and np.array_equal(o[k], g[tag + k]), k
    vv = P.virtual_views(i["poses"], i["K"], h, w)
    assert vv["poses_virt"].dtype == torch.float32 and np.array_equal(vv["poses_virt"].numpy(), g[tag + "poses_virt"])
    assert np.array_equal(torch.stack([vv["radius"], vv["theta"], vv["phi"]], -1).numpy(), g[tag + "rtp"])
    assert np.array_equal(torch.stack([vv["raw_radius"], vv["raw_theta"], vv["raw_phi"]], -1).numpy(), g[tag + "raw_rtp"])
    assert np.array_equal(vv["K_virt"], g[tag + "K_virt"])


def test_oracle_polar_chains_and_cameras_equal_the_reference(g):
    tp = torch.from_numpy(g["pol_poses"])
    assert np.array_equal(tp.numpy(), P.make_polar_poses())
    for virtual, tag in ((True, "pol_virt"), (False, "pol_raw")):
        assert np.array_equal(torch.stack(P.polar_from_c2w(tp, virtual), -1).numpy(), g[tag]), tag
    r, th, ph = (torch.from_numpy(g["pol_virt"][:, k].copy()) for k in range(3))
    assert np.array_equal(P.c2w_from_polar(r, th, ph, tp[:, :3, 0]).numpy(), g["pol_c2w"])
    ci = P.make_camera_inputs()
    for tag, ref in (("cam0_", None), ("cam1_", ci["ref_points"])):
        cams = P.cameras_from_pose_init(ci["transformations"], float(g[tag + "radius"]), ci["K"], ref)
        for k in range(len(ci["transformations"])):
            assert np.array_equal(cams[f"world_mat_{k}"], g[tag + "world_mats"][k]) and np.array_equal(cams[f"scale_mat_{k}"], g[tag + "scale_mats"][k])


@pytest.mark.parametrize("run", range(len(P.RUNS)))
def test_host_functions_equal_the_reference(g, run):
    from morpheus_amd import preprocess as pp
    tag, h, w, radius = P.RUNS[run]
    i = inputs(g)
    poses, K = torch.from_numpy(i["poses"]), torch.from_numpy(i["K"])
    centres = pp.crop_centres(poses, K)
    assert centres.dtype == np.int64 and np.array_equal(centres, g[tag + "centres"])
    assert np.array_equal(pp.window_origins(centres, h, w), P.window_origins(g[tag + "centres"], h, w))
    vv = pp.virtual_views(poses, K, h, w)
    assert torch.equal(vv["poses_virt"], torch.from_numpy(g[tag + "poses_virt"]))
    assert torch.equal(torch.stack([vv["radius"], vv["theta"], vv["phi"]], -1), torch.from_numpy(g[tag + "rtp"]))
    assert torch.equal(torch.stack([vv["raw_radius"], vv["raw_theta"], vv["raw_phi"]], -1), torch.from_numpy(g[tag + "raw_rtp"]))
    assert vv["K_virt"].dtype == np.float64 and np.array_equal(vv["K_virt"], g[tag + "K_virt"])


def test_host_polar_chains_and_cameras_equal_the_reference(g, tmp_path):
    from morpheus_amd import preprocess as pp
    tp = torch.from_numpy(g["pol_poses"])
    for virtual, tag in ((True, "pol_virt"), (False, "pol_raw")):
        got = torch.stack(pp.polar_from_c2w(tp, virtual), -1)
        assert got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(g[tag])), tag
    r, th, ph = (torch.from_numpy(g["pol_virt"][:, k].copy()) for k in range(3))
    assert torch.equal(pp.c2w_from_polar(r, th, ph, tp[:, :3, 0]), torch.from_numpy(g["pol_c2w"]))
    ci = P.make_camera_inputs()
    for tag, ref in (("cam0_", None), ("cam1_", ci["ref_points"])):
        cams = pp.cameras_from_pose_init(ci["transformations"].reshape(-1, 16), float(g[tag + "radius"]), ci["K"], ref)
        assert len(cams) == 12
        for k in range(6):
            assert cams[f"world_mat_{k}"].dtype == np.float32 and np.array_equal(cams[f"world_mat_{k}"], g[tag + "world_mats"][k])
            assert cams[f"scale_mat_{k}"].dtype == np.float32 and np.array_equal(cams[f"scale_mat_{k}"], g[tag + "scale_mats"][k])
    pp.write_cameras(tmp_path / "cameras_sphere.npz", cams)
    with np.load(tmp_path / "cameras_sphere.npz") as z:
        assert sorted(z.files) == sorted(cams) and all(np.array_equal(z[k], cams[k]) for k in cams)


def test_projection_matrix_recomposes(g, tmp_path):
    """load_K_Rt_from_P is an RQ decomposition, not cv2's: K [R|t] must give P back up to scale.  P is scaled to unit Frobenius
    norm and so is the recomposition; the measured round-trip error over these twelve cameras (focal lengths ~500, translations
    ~1) is 4.5e-16 at most, a handful of float64 roundings of entries below 1; the bound is 64 x 2^-53 = 7.2e-15 for the chain of a
    QR, a solve and two 3 x 3 products.  K is upper triangular with a positive diagonal and K[2,2] = 1, R a rotation up to its
    fp32 storage.  camera_params then gives the OpenGL pose, flipped by the alignment, and the depth scale 1 / radius."""
    from morpheus_amd import preprocess as pp
    ci = P.make_camera_inputs()
    worst = 0.0
    for tag in ("cam0_", "cam1_"):
        for wm, sm in zip(g[tag + "world_mats"], g[tag + "scale_mats"]):
            Pm = (wm @ sm)[:3, :4].astype(np.float64)
            K4, pose = pp.load_K_Rt_from_P(Pm)
            assert K4.shape == (4, 4) and K4.dtype == np.float64 and pose.shape == (4, 4) and pose.dtype == np.float32
            K = K4[:3, :3]
            assert np.array_equal(np.tril(K, -1), np.zeros((3, 3))) and (np.diag(K) > 0).all() and K[2, 2] == 1.0
            # recompose in float64 from the float64 factors (the fp32 pose would put 2^-24 into it)
            q, r = np.linalg.qr(np.flipud(Pm[:, :3]).T)
            R64 = np.flipud(q.T) * np.where(np.diag(np.fliplr(np.flipud(r.T))) < 0, -1.0, 1.0)[:, None]
            assert np.abs(R64.T - pose[:3, :3]).max() <= 2.0 ** -24
            c = -np.linalg.solve(Pm[:, :3], Pm[:, 3])
            assert np.abs(c - pose[:3, 3]).max() <= 2.0 ** -24 * max(1.0, np.abs(c).max())
            back = K @ np.concatenate([R64, -(R64 @ c)[:, None]], 1)
            err = np.abs(back / np.linalg.norm(back) - Pm / np.linalg.norm(Pm)).max()
            worst = max(worst, err)
            assert err <= 64 * 2.0 ** -53, err
    print("worst round-trip error", worst)
    cams = pp.cameras_from_pose_init(ci["transformations"], float(g["cam0_radius"]), ci["K"])
    poses, intrinsics, scales, scale_mats = pp.camera_params(cams, 6)
    assert poses.dtype == torch.float32 and poses.shape == (6, 4, 4) and intrinsics.dtype == torch.float64 and scales.shape == (6, 1)
    assert scales.dtype == torch.float32 and float(scales[0]) == run_scale(g["cam0_radius"]) and len(scale_mats) == 6
    radius = float(np.float32(g["cam0_radius"]))
    for k in range(6):
        c2w = np.linalg.inv(ci["transformations"][k])          # OpenCV camera-to-world, world units
        want = c2w.copy()
        want[:3, 3] /= radius                                  # the unit sphere's units
        want[:3, 1:3] *= -1                                    # OpenGL
        want = np.diag([1.0, -1.0, -1.0, 1.0]) @ want          # aligned
        assert np.abs(poses[k].numpy() - want).max() < 1e-5
        assert np.abs(intrinsics[k].numpy()[:3, :3] - ci["K"]).max() < 1e-3
    unaligned = pp.camera_params(cams, 6, align=False)[0]
    assert torch.equal(unaligned[:, 1:3], -poses[:, 1:3]) and torch.equal(unaligned[:, 0], poses[:, 0])


def test_depth_tables_are_the_two_numpy_products():
    from morpheus_amd import preprocess as pp
    raw = np.arange(65536).astype(np.uint16)
    for depth_scale, scale in ((1000.0, 1.0), (1000.0, run_scale(1.25)), (5000.0, 1.7)):
        tin, tpad = pp.depth_tables(depth_scale, scale)
        d = (raw / depth_scale).astype(np.float32)
        d *= np.array([scale], dtype=np.float32)
        assert d.dtype == np.float32 and (d * 1000).dtype == np.float32
        assert tin.dtype == np.uint16 and np.array_equal(tin, (d * 1000).astype(np.uint16))
        assert tpad.dtype == np.uint16 and np.array_equal(tpad, (d.astype(np.float64) * 1000).astype(np.uint16))
        assert (tin != tpad).any() and tin[0] == 0 and tpad[0] == 0
        o = P.depth_tables(depth_scale, scale)
        assert np.array_equal(o[0], tin) and np.array_equal(o[1], tpad)
    tin, tpad = pp.depth_tables(1000.0, 1.0)
    assert int((tin != raw).sum()) == 739 and int((tpad != raw).sum()) == 32501 and int((tin != tpad).sum()) == 31762
    tin, tpad = pp.depth_tables(1000.0, 2.0)                   # this build's rule: saturation
    assert tin[40000] == 65535 and tpad[65535] == 65535 and tin[100] in (199, 200)
    # the bytes survive x / 255.0 * 255. truncated
    b = np.arange(256)
    assert np.array_equal((b / 255.0 * 255.).astype(np.uint8), b)


def test_affine_maps():
    from morpheus_amd import preprocess as pp
    for deg in P.ANGLES:
        M = pp.rotation_matrix((7, 4), deg)
        assert M.dtype == np.float64 and np.array_equal(M, P.rotation_matrix((7, 4), deg))
        a = pp.invert_affine(M)
        assert np.array_equal(a, P.invert_affine(M))
        full = np.vstack([M, [0, 0, 1]]) @ np.vstack([a.reshape(2, 3), [0, 0, 1]])
        assert np.abs(full - np.eye(3)).max() < 1e-14
        assert np.abs(M @ np.array([7.0, 4.0, 1.0]) - (7.0, 4.0)).max() < 1e-14      # the centre stays
    a = pp.invert_affine(pp.rotation_matrix((7, 4), 0.0))
    assert np.array_equal(a, [1, 0, 0, 0, 1, 0])               # exactly the identity
    M90 = pp.rotation_matrix((0, 0), 90.0)                     # a positive angle turns counter-clockwise on the screen (y down)
    assert np.abs(M90 @ np.array([1.0, 0.0, 1.0]) - (0.0, -1.0)).max() < 1e-15


def result_from_oracle(g, run):
    """a PreprocessResult as `preprocess` returns it, with the frames made by the oracle on the CPU"""
    from morpheus_amd import preprocess as pp
    tag, h, w, radius = P.RUNS[run]
    i = inputs(g)
    poses, K = torch.from_numpy(i["poses"]), torch.from_numpy(i["K"])
    centres = pp.crop_centres(poses, K)
    origin = pp.window_origins(centres, h, w)
    tin, tpad = pp.depth_tables(P.DEPTH_SCALE, run_scale(radius))
    o = P.prep_frames(i["rgb"], i["depth"], i["mask"], origin, np.zeros((P.F, 6)), np.zeros(P.F, np.uint8), tin, tpad, h, w)
    return pp.PreprocessResult(**{k: torch.from_numpy(v) for k, v in o.items()}, crop_centres=centres, origin=origin, table_inside=tin,
                               table_padded=tpad, size_h=h, size_w=w, **pp.virtual_views(poses, K, h, w))


def test_write_dir_is_read_back_by_the_dataset(g, tmp_path):
    from PIL import Image
    from morpheus_amd.dataset import DeviceDataset
    tag, h, w, radius = P.RUNS[1]
    res = result_from_oracle(g, 1)
    res.write_dir(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["K_virt.txt", "color_virt", "crop_centre_list.txt", "depth_raw_crop", "mask_virt", "padding_mask",
                                            "poses_virt", "r_theta_phi.txt", "raw_r_theta_phi.txt"]
    assert sorted(os.listdir(tmp_path / "depth_raw_crop")) == ["%06d.png" % k for k in range(P.F)]
    assert sorted(os.listdir(tmp_path / "poses_virt")) == ["%06d.txt" % k for k in range(P.F)]
    ds = DeviceDataset.from_dir({"data": {"data_dir": str(tmp_path), "depth_scale": 1000.0}}, device="cpu")
    assert (ds.num_frames, ds.H, ds.W) == (P.F, h, w)
    assert np.array_equal(ds.rgb_dev.numpy(), g[tag + "rgb"]) and np.array_equal(ds.depth_dev.numpy(), g[tag + "depth"])
    assert ds.depth_dev.dtype == torch.uint16 and np.array_equal(ds.mask_dev.numpy(), g[tag + "mask"])
    assert np.array_equal(ds.poses.numpy(), g[tag + "poses_virt"]) and np.array_equal(ds.intrinsics.numpy(), g[tag + "K_virt"])
    for k, name in enumerate(("radius", "theta", "phi")):
        assert np.array_equal(getattr(ds, name).numpy(), g[tag + "rtp"][:, k]), name
    pad = np.stack([np.asarray(Image.open(tmp_path / "padding_mask" / ("%06d.png" % k))) for k in range(P.F)])
    assert pad.dtype == np.uint8 and np.array_equal(pad, g[tag + "padding"])
    assert np.array_equal(np.loadtxt(tmp_path / "raw_r_theta_phi.txt").astype(np.float32), g[tag + "raw_rtp"])
    assert np.array_equal(np.loadtxt(tmp_path / "crop_centre_list.txt"), g[tag + "centres"])


def write_raw_dir(root, g, radius=1.25, mask_rgb=False):
    """the raw layout the reference's Database reads: rgb/, depth/, mask/ as .png and cameras_sphere.npz whose world_mat @ scale_mat
    decomposes into the golden's intrinsics and (after the OpenGL flip and the alignment) the golden's poses"""
    from PIL import Image
    i = inputs(g)
    for sub in ("rgb", "depth", "mask"):
        os.makedirs(os.path.join(root, sub))
    cams = {}
    for f in range(P.F):
        Image.fromarray(i["rgb"][f], "RGB").save(os.path.join(root, "rgb", f"{f:04d}.png"))
        Image.fromarray(i["depth"][f]).save(os.path.join(root, "depth", f"{f:04d}.png"))
        m = i["mask"][f]
        m = np.stack([255 - m, m // 2, m], -1) if mask_rgb else m      # the blue plane is the mask
        Image.fromarray(m).save(os.path.join(root, "mask", f"{f:04d}.png"))
        c2w = np.diag([1.0, -1.0, -1.0, 1.0]) @ i["poses"][f].astype(np.float64)      # undo the alignment
        c2w[:3, 1:3] *= -1                                                            # OpenCV axes
        c2w[:3, 3] *= radius                                                          # world units
        K4 = i["K"][f]
        cams[f"world_mat_{f}"] = (K4 @ np.linalg.inv(c2w)).astype(np.float32)
        cams[f"scale_mat_{f}"] = np.diag([radius, radius, radius, 1.0]).astype(np.float32)
    np.savez(os.path.join(root, "cameras_sphere.npz"), **cams)
    return {"data": {"data_dir": str(root), "render_cameras_name": "cameras_sphere.npz", "depth_scale": 1000.0}}


def test_raw_directory_reader_and_argument_rules(g, tmp_path):
    from morpheus_amd import preprocess as pp
    from morpheus_amd._lib import MorpheusHipError
    i = inputs(g)
    cfg = write_raw_dir(tmp_path / "a", g, mask_rgb=True)
    rgb, depth, mask = pp.read_raw_dir(cfg["data"]["data_dir"])
    assert rgb.dtype == np.uint8 and depth.dtype == np.uint16 and mask.dtype == np.uint8
    assert np.array_equal(rgb, i["rgb"]) and np.array_equal(depth, i["depth"]) and np.array_equal(mask, i["mask"])
    cfg = write_raw_dir(tmp_path / "b", g)
    assert np.array_equal(pp.read_raw_dir(cfg["data"]["data_dir"])[2], i["mask"])
    with np.load(tmp_path / "b" / "cameras_sphere.npz") as z:
        poses, K, scales, _ = pp.camera_params(z, P.F)
    # the decomposition is not bit-exact, the centres it leads to are: the targets sit half a pixel inside
    assert np.abs(poses.numpy() - i["poses"]).max() < 1e-5 and np.abs(K.numpy() - i["K"]).max() < 1e-4
    assert np.array_equal(pp.crop_centres(poses, K), g["s7_centres"]) and float(scales[0]) == run_scale(1.25)
    pre = {"size_h": 7, "size_w": 7, "rot_degree": 0}
    full = {"data": dict(cfg["data"], **pre)}
    with pytest.raises(MorpheusHipError, match="no CPU path"):      # everything on the host runs, the frames need the device
        pp.preprocess_dir(full, device="cpu")
    cams = (torch.from_numpy(i["poses"]), torch.from_numpy(i["K"]), torch.tensor([[1.0]] * 5 + [[0.8]] * 5))
    with pytest.raises(ValueError, match="one positive depth scale"):
        pp.preprocess(i["rgb"], i["depth"], i["mask"], cams, full, device="cpu")
    with pytest.raises(ValueError, match="poses and intrinsics"):
        pp.preprocess(i["rgb"][:4], i["depth"][:4], i["mask"][:4], (cams[0], cams[1], cams[2][:5]), full, device="cpu")
    with pytest.raises(FileNotFoundError, match="rgb"):
        pp.read_raw_dir(str(tmp_path))
    from morpheus_amd.dataset import DeviceDataset
    with pytest.raises(MorpheusHipError, match="no CPU path"):
        DeviceDataset.from_raw(cfg, device="cpu", pre=pre)
    with pytest.raises(KeyError, match="size_h"):
        DeviceDataset.from_raw(cfg, device="cpu")


def test_library_takes_bad_preprocess_arguments_without_a_launch():
    import ctypes
    from morpheus_amd import _lib, build
    build.build()
    lib = _lib.load()
    hdr = open(os.path.join(os.path.dirname(build.HEADER), "morpheus_hip.h")).read()
    assert len(re.findall(r"\bmh_prep_frames\s*\(", hdr)) == 1 and "mh_prep_frames" in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(_lib.SO), "mh_prep_frames")
    N = [None]
    assert lib.mh_prep_frames(*N * 3, 0, 12, 16, *N * 5, 8, 8, *N * 4, None) == 0                  # no frames: nothing to do
    assert lib.mh_prep_frames(*N * 3, 2, 12, 16, *N * 5, 8, 8, *N * 4, None) == 1                  # null pointers
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    p += (-p) % 8
    ok = [p] * 3 + [2, 12, 16] + [p] * 5 + [8, 8] + [p] * 4
    for at, bad in ((3, -1), (4, 0), (5, -3), (11, 0), (12, -8), (3, 2 ** 31 - 1), (4, 2 ** 30), (13, p + 2), (14, p + 4), (15, p + 1),
                    (16, p + 3), (7, p + 4), (0, None), (10, None), (16, None)):
        args = list(ok)
        args[at] = bad
        assert lib.mh_prep_frames(*args, None) == 1, (at, bad)
    assert lib.mh_abi_version() == 10


def test_preprocess_source_is_built_without_contraction():
    from morpheus_amd import build
    assert "preprocess.hip" in build.SOURCES and build.FILE_FLAGS["preprocess.hip"] == ["-ffp-contract=off"]
    assert "dataset.hip" in build.SOURCES and build.FILE_FLAGS["dataset.hip"] == ["-ffp-contract=off"]
