"""Record tests/golden/preprocess.npz from the reference's own DataProcessor and create_camera.py (build container only: needs the
reference tree).

    python tools/make_preprocess_golden.py <reference tree>

preprocess/preprocess.py is loaded by file path.  cv2 and imageio are not installed, so both are stubbed: cv2.getRotationMatrix2D
follows [[c, s, (1 - c) cx - s cy], [-s, c, s cx + (1 - c) cy]], cv2.warpAffine ASSERTS an identity matrix (the golden is recorded at
rot_degree = 0) and returns a copy, imageio.imwrite keeps what it is handed.  A DataProcessor is filled without reading a sequence
from disk, from tests/preprocess_oracle.make_inputs (F = 10 frames of 12 x 16, translation-only cameras) and run twice
(preprocess_oracle.RUNS): window 8 x 8 with depth scale 1 and window 7 x 7 (an odd size, for `// 2`) with depth scale 1 / 1.25.
Its own text files go to a temporary directory.  The ten frames fall on every kind of window the reference can run
(preprocess_oracle.KINDS; asserted for both sizes), and the reference is shown to RAISE on the three kinds it cannot run
(preprocess_oracle.EXCLUDED: a window crossing two different sides, one wholly outside, one larger than the frame).

Recorded, numeric arrays only:
  in_*            the frames, poses and intrinsics
  <run>centres    crop_centre_list.txt;  <run>rgb / depth / mask / padding: what the four imwrite lines were handed
  <run>poses_virt, <run>rtp, <run>raw_rtp, <run>K_virt
  pol_*           get_polar_from_c2w (both forms) and get_c2w_from_polar on preprocess_oracle.make_polar_poses
  cam0_*, cam1_*  create_camera.py through runpy on a temporary directory, without and with intermediate/ref.xyz
Finally tests/preprocess_oracle.py is checked against all of it, bit for bit.
"""
import importlib.util
import os
import runpy
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import preprocess_oracle as P  # noqa: E402

WRITTEN = {}


def load_module(ref):
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR, cv2.INTER_NEAREST = 1, 0

    def get_rotation_matrix(center, angle, scale):
        assert scale == 1.0
        return P.rotation_matrix(center, angle)

    def warp_affine(img, M, size, flags=None):
        assert np.array_equal(np.asarray(M)[:, :2], np.eye(2)) and not np.asarray(M)[:, 2].any(), "the golden is recorded unrotated"
        assert tuple(size) == (img.shape[1], img.shape[0])
        return img.copy()
    cv2.getRotationMatrix2D, cv2.warpAffine = get_rotation_matrix, warp_affine
    imageio = types.ModuleType("imageio")
    imageio.imwrite = lambda path, arr: WRITTEN.__setitem__(os.path.join(os.path.basename(os.path.dirname(path)), os.path.basename(path)), np.array(arr))
    sys.modules["cv2"], sys.modules["imageio"] = cv2, imageio
    sys.path.insert(0, ref)                                   # `from utils import ...`
    spec = importlib.util.spec_from_file_location("reference_preprocess", os.path.join(ref, "preprocess", "preprocess.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.path.remove(ref)
    return mod


def make_processor(mod, inp, tmp, size_h, size_w, radius, frames=None):
    sel = slice(None) if frames is None else frames
    dp = object.__new__(mod.DataProcessor)
    dp.cfg = {"data": {"data_dir": tmp, "size_h": size_h, "size_w": size_w, "rot_degree": 0, "depth_scale": P.DEPTH_SCALE}}
    dp.align, dp.data_dir = True, tmp
    dp.size_h, dp.size_w, dp.rot_degree = size_h, size_w, 0
    dp.align_mat = dp.get_align_mat()
    dp.images = np.stack(list(inp["rgb"][sel])) / 255.0
    dp.n_images = len(dp.images)
    dp.depths = (np.stack(list(inp["depth"][sel])) / P.DEPTH_SCALE).astype(np.float32)
    dp.masks = np.stack(list(inp["mask"][sel])) / 255.0
    dp.poses = torch.from_numpy(inp["poses"][sel].copy())
    dp.intrinsics = torch.from_numpy(inp["K"][sel].copy())
    scale_mat = np.diag([radius, radius, radius, 1.0]).astype(np.float32)
    dp.scales = torch.stack([torch.from_numpy(np.array([1.0 / scale_mat[0, 0]])) for _ in range(dp.n_images)])
    assert dp.scales.dtype == torch.float32
    dp.scale_depth()
    assert dp.depths.dtype == np.float32
    dp.H, dp.W = dp.depths.shape[1:3]
    # rotate_and_crop_frames mixes the torch pose with numpy: np.linalg.inv(Tensor) comes back as a Tensor, and with the numpy 2 /
    # torch pair of the build container `K @ x_c` (ndarray @ Tensor) raises a TypeError.  The frame's pose is handed over as the
    # fp32 numpy array it wraps, so that the chain the reference means runs: fp32 inverse, float64 projection.
    get_frame = dp.get_frame

    def get_frame_numpy_pose(idx):
        ret = get_frame(idx)
        ret["c2w"] = ret["c2w"].numpy()
        return ret
    dp.get_frame = get_frame_numpy_pose
    return dp


def pose_for(px, py, K):
    """a translation-only camera whose world centre projects half a pixel inside (px, py)"""
    Z = 2.0
    X, Y = (px + 0.5 - K[0, 2]) * Z / K[0, 0], (py + 0.5 - K[1, 2]) * Z / K[1, 1]
    return np.array([[1.0, 0, 0, -X], [0, -1.0, 0, -Y], [0, 0, -1.0, -Z], [0, 0, 0, 1.0]], dtype=np.float32)


def run_cameras(ref, out):
    ci = P.make_camera_inputs()
    for tag, with_ref in (("cam0_", False), ("cam1_", True)):
        with tempfile.TemporaryDirectory() as tmp:
            os.makedirs(os.path.join(tmp, "depth"))
            os.makedirs(os.path.join(tmp, "intermediate"))
            np.savetxt(os.path.join(tmp, "intrinsics.txt"), ci["K"])
            for i in range(len(ci["transformations"])):
                open(os.path.join(tmp, "depth", f"{i:04d}.png"), "wb").close()
            np.save(os.path.join(tmp, "intermediate", "transformations.npy"), ci["transformations"].reshape(-1, 16))
            np.savetxt(os.path.join(tmp, "intermediate", "radius.txt"), np.array([ci["radius"]]), fmt="%.8f")
            if with_ref:
                np.savetxt(os.path.join(tmp, "intermediate", "ref.xyz"), ci["ref_points"])
            argv = sys.argv
            sys.argv = ["create_camera.py", "--data_path", tmp + os.sep]
            try:
                runpy.run_path(os.path.join(ref, "preprocess", "pose_init", "create_camera.py"), run_name="__main__")
            finally:
                sys.argv = argv
            with np.load(os.path.join(tmp, "cameras_sphere.npz")) as z:
                cams = {k: z[k] for k in z.files}
            radius = float(np.loadtxt(os.path.join(tmp, "intermediate", "radius.txt.bk" if with_ref else "radius.txt")))
            ref_pts = np.loadtxt(os.path.join(tmp, "intermediate", "ref.xyz")) if with_ref else None
        n = len(ci["transformations"])
        out[tag + "world_mats"] = np.stack([cams[f"world_mat_{i}"] for i in range(n)])
        out[tag + "scale_mats"] = np.stack([cams[f"scale_mat_{i}"] for i in range(n)])
        out[tag + "radius"] = np.float64(radius)
        orc = P.cameras_from_pose_init(ci["transformations"], radius, ci["K"], ref_pts)
        assert set(orc) == set(cams)
        for k in cams:
            assert cams[k].dtype == orc[k].dtype == np.float32 and np.array_equal(cams[k], orc[k]), (tag, k)
        print(f"{tag}: {n} cameras, scale {cams['scale_mat_0'][0, 0]}")


def main(ref):
    mod = load_module(ref)
    inp = P.make_inputs()
    out = {"in_" + k: v for k, v in inp.items()}
    for tag, size_h, size_w, radius in P.RUNS:
        WRITTEN.clear()
        with tempfile.TemporaryDirectory() as tmp:
            dp = make_processor(mod, inp, tmp, size_h, size_w, radius)
            dp.preprocess()
            centres = np.loadtxt(os.path.join(tmp, "crop_centre_list.txt")).astype(np.int64)
            rtp, raw_rtp = (np.loadtxt(os.path.join(tmp, k)) for k in ("r_theta_phi.txt", "raw_r_theta_phi.txt"))
            K_virt = np.loadtxt(os.path.join(tmp, "K_virt.txt"))
        origin = P.window_origins(centres, size_h, size_w)
        kinds = tuple(P.window_kind(t, l, size_h, size_w, P.H, P.W) for t, l in origin)
        assert kinds == P.KINDS, kinds                       # the reference returned for each of the ten
        assert centres.tolist() == [[int(x), int(y)] for x, y in P.TARGETS], centres
        planes = {k: np.stack([WRITTEN[os.path.join(sub, f"{i:06d}.png")] for i in range(P.F)])
                  for k, sub in (("rgb", "color_virt"), ("depth", "depth_raw_crop"), ("mask", "mask_virt"), ("padding", "padding_mask"))}
        assert planes["depth"].dtype == np.uint16 and all(planes[k].dtype == np.uint8 for k in ("rgb", "mask", "padding"))
        out.update({tag + k: v for k, v in planes.items()})
        out.update({tag + "centres": centres, tag + "poses_virt": dp.poses_virt.numpy(), tag + "K_virt": K_virt,
                    tag + "rtp": torch.stack([dp.radius, dp.theta, dp.phi], -1).numpy(),
                    tag + "raw_rtp": torch.stack([dp.raw_radius, dp.raw_theta, dp.raw_phi], -1).numpy()})
        assert np.array_equal(rtp.astype(np.float32), out[tag + "rtp"]) and np.array_equal(raw_rtp.astype(np.float32), out[tag + "raw_rtp"])
        # ---- the oracle against the reference
        scale = float(np.float32(1.0) / np.float32(radius))
        tin, tpad = P.depth_tables(P.DEPTH_SCALE, scale)
        assert np.array_equal(P.crop_centres(inp["poses"], inp["K"]), centres)
        orc = P.prep_frames(inp["rgb"], inp["depth"], inp["mask"], origin, np.zeros((P.F, 6)), np.zeros(P.F, np.uint8), tin, tpad, size_h, size_w)
        for k in planes:
            assert orc[k].dtype == planes[k].dtype and np.array_equal(orc[k], planes[k]), (tag, k)
        vv = P.virtual_views(inp["poses"], inp["K"], size_h, size_w)
        assert np.array_equal(vv["poses_virt"].numpy(), out[tag + "poses_virt"]) and np.array_equal(vv["K_virt"], K_virt)
        assert np.array_equal(torch.stack([vv["radius"], vv["theta"], vv["phi"]], -1).numpy(), out[tag + "rtp"])
        assert np.array_equal(torch.stack([vv["raw_radius"], vv["raw_theta"], vv["raw_phi"]], -1).numpy(), out[tag + "raw_rtp"])
        # both write products occur and both change values
        ins = np.array([k == "inside" for k in kinds])
        for sel, what in ((ins, "fp32"), (~ins, "float64")):
            o = origin[sel]
            moved = 0
            for f, (t, l) in zip(np.nonzero(sel)[0], o):
                on = planes["padding"][f] == 0
                Y, X = np.nonzero(on)
                moved += int((planes["depth"][f][on] != inp["depth"][f][Y + t, X + l]).sum())
            assert moved > 0, what
            print(f"{tag}{what} product: {int(sel.sum())} frames, {moved} depth values rewritten")

    # ---- the kinds the reference cannot run
    for kind, (py, px, size_h, size_w) in P.EXCLUDED.items():
        top, left = P.window_origins([(px, py)], size_h, size_w)[0]
        assert P.window_kind(top, left, size_h, size_w, P.H, P.W) == kind
        one = dict(inp)
        one["poses"] = inp["poses"].copy()
        one["poses"][0] = pose_for(px, py, inp["K"][0])
        with tempfile.TemporaryDirectory() as tmp:
            dp = make_processor(mod, one, tmp, size_h, size_w, 1.0, frames=slice(0, 1))
            try:
                dp.rotate_and_crop_frames()
            except ValueError as e:
                assert "broadcast" in str(e), e
                print(f"{kind}: the reference raises ({e})")
            else:
                raise AssertionError(f"{kind}: the reference returned")
        assert P.crop_centres(one["poses"][:1], one["K"][:1]).tolist() == [[px, py]]
        out["ex_" + kind + "_pose"] = one["poses"][0]

    # ---- the polar chains on generic poses
    poses = P.make_polar_poses()
    dp = object.__new__(mod.DataProcessor)
    tp = torch.from_numpy(poses)
    for virtual, tag in ((True, "pol_virt"), (False, "pol_raw")):
        r, th, ph = dp.get_polar_from_c2w(tp, virtual=virtual)
        out[tag] = torch.stack([r, th, ph], -1).numpy()
        assert np.array_equal(torch.stack(P.polar_from_c2w(tp, virtual), -1).numpy(), out[tag]), tag
    r, th, ph = (torch.from_numpy(out["pol_virt"][:, k].copy()) for k in range(3))
    x_axis = dp.get_x_vector_from_c2w(tp)
    out["pol_c2w"] = dp.get_c2w_from_polar(radius=r, x_axis=x_axis, theta=th, phi=ph).numpy()
    assert np.array_equal(P.c2w_from_polar(r, th, ph, x_axis).numpy(), out["pol_c2w"])
    out["pol_poses"] = poses
    assert (out["pol_virt"][:, 2] > 180).any() and (out["pol_virt"][:, 2] < 180).any()

    run_cameras(ref, out)
    path = os.path.join(ROOT, "tests", "golden", "preprocess.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
