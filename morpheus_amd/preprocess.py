"""Preprocessing of a raw RGB-D sequence on the device: cameras, virtual views, rotated and cropped frames.

Stands where the reference's preprocess/pose_init/create_camera.py and preprocess/preprocess.py (`Database`, `DataProcessor`) stand,
between `morpheus_amd.poseinit` (intermediate/transformations.npy, radius.txt) and `morpheus_amd.dataset.DeviceDataset`:

    cameras_from_pose_init / write_cameras   the registration result -> cameras_sphere.npz
    camera_params, load_K_Rt_from_P          cameras_sphere.npz -> poses (OpenGL, aligned), intrinsics, scales
    virtual_views, crop_centres              the virtual cameras and the projected world centre of every frame
    preprocess / preprocess_dir              the frames: ONE launch of csrc/preprocess.hip (`ops.prep_frames`) for the sequence
    PreprocessResult.write_dir               the reference's directory layout, with PIL and numpy

The small per-frame camera chains stay on the host in the reference's own torch fp32 / numpy operators and equal it bit for bit on
the CPU (tests/golden/preprocess.npz).  The frames are rewritten on the device; what the kernel computes, and that its rotation is
this build's own definition (agreement with cv2 unverified), is the header comment of csrc/preprocess.hip.  `load_K_Rt_from_P`
replaces cv2.decomposeProjectionMatrix by an RQ decomposition and is judged by recomposition, not against cv2.
Nothing here needs cv2 or imageio.
"""
from __future__ import annotations

import math
import os
from glob import glob

import numpy as np
import torch

from . import ops


# -------------------------------------------------------------------------------------------------------------------- cameras
def load_K_Rt_from_P(P):
    """P [3,4] = K [R|t] -> (intrinsics [4,4] float64 with K / K[2,2], pose [4,4] float32 = camera-to-world).  K is upper
    triangular with a positive diagonal (an RQ decomposition with its signs fixed), R orthogonal, the pose's translation the
    camera centre -M^-1 p4."""
    P = np.asarray(P, dtype=np.float64)[:3, :4]
    M = P[:, :3]
    q, r = np.linalg.qr(np.flipud(M).T)
    K, R = np.fliplr(np.flipud(r.T)), np.flipud(q.T)          # M = K R
    sign = np.where(np.diag(K) < 0, -1.0, 1.0)
    K, R = K * sign[None, :], R * sign[:, None]
    intrinsics = np.eye(4)
    intrinsics[:3, :3] = K / K[2, 2]
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = R.T
    pose[:3, 3] = -np.linalg.solve(M, P[:, 3])
    return intrinsics, pose


def camera_params(camera_dict, n: int, align: bool = True):
    """`Database.get_camera_params`: world_mat_i / scale_mat_i of cameras_sphere.npz -> (poses fp32 [n,4,4] camera-to-world in
    OpenGL axes, flipped by diag(1, -1, -1, 1) when `align`; intrinsics float64 [n,4,4]; scales fp32 [n,1] = 1 / scale_mat[0,0];
    the scale matrices)"""
    align_mat = torch.eye(4)
    align_mat[1, 1] = align_mat[2, 2] = -1.0
    poses, intrinsics, scales, scale_mats = [], [], [], []
    for i in range(n):
        world_mat, scale_mat = (np.asarray(camera_dict[f"{k}_mat_{i}"]).astype(np.float32) for k in ("world", "scale"))
        K, pose = load_K_Rt_from_P((world_mat @ scale_mat)[:3, :4])
        pose = torch.from_numpy(pose)
        pose[:3, 1] *= -1
        pose[:3, 2] *= -1
        poses.append(align_mat @ pose if align else pose)
        intrinsics.append(torch.from_numpy(K))
        scales.append(torch.from_numpy(np.array([np.float32(1.0) / scale_mat[0, 0]], dtype=np.float32)))
        scale_mats.append(scale_mat)
    return torch.stack(poses), torch.stack(intrinsics), torch.stack(scales), scale_mats


def cameras_from_pose_init(transformations, radius, K, ref_points=None, object_scale: float = 1.05):
    """create_camera.py: world-to-camera transformations [n,4,4] (or [n,16]) and the radius of `poseinit.init_poses`, the 3 x 3
    matrix of intrinsics.txt -> {"world_mat_i": fp32(K4 @ w2c_i), "scale_mat_i": fp32(diag(r, r, r, 1))}.  With reference points
    [m,3] the radius is multiplied by their largest norm times `object_scale`."""
    K = np.asarray(K, dtype=np.float64)
    intrinsic = np.diag([K[0, 0], K[1, 1], 1.0, 1.0]).astype(np.float32)
    intrinsic[0, 2], intrinsic[1, 2] = K[0, 2], K[1, 2]
    radius = np.float64(radius)
    if ref_points is not None:
        radius = radius * (np.linalg.norm(np.asarray(ref_points), ord=2, axis=-1, keepdims=False).max() * object_scale)
    T = np.asarray(transformations).reshape(-1, 4, 4)
    cams = {f"world_mat_{i}": (intrinsic @ T[i]).astype(np.float32) for i in range(len(T))}
    scale_mat = np.diag([radius, radius, radius, 1.0]).astype(np.float32)
    cams.update({f"scale_mat_{i}": scale_mat for i in range(len(T))})
    return cams


def write_cameras(path, cameras) -> None:
    """cameras_sphere.npz as create_camera.py writes it"""
    np.savez(path, **cameras)


# -------------------------------------------------------------------------------------------------------------- virtual views
def _safe_normalize(x, eps=1e-20):
    return x / torch.sqrt(torch.clamp(torch.sum(x * x, -1, keepdim=True), min=eps))


def polar_from_c2w(poses, virtual: bool):
    """`get_polar_from_c2w`: camera-to-world fp32 [n,4,4] -> (radius, theta, phi) fp32 [n], angles in degrees, phi in [0, 360).
    virtual: the camera that looks along the real one's z axis through the origin's plane (r = centre . z, angles of z); otherwise
    the angles of the camera centre itself.  Frame by frame on 0-dim fp32 tensors, as the reference runs it."""
    radius, thetas, phis = [], [], []
    for c2w in torch.as_tensor(poses):
        centre, z_dir = c2w[:3, 3], c2w[:3, 2]
        if virtual:
            r = (centre * z_dir).sum()
            theta, phi = torch.acos(z_dir[1]), torch.atan2(z_dir[0], z_dir[2])
        else:
            r = torch.sqrt(torch.sum(centre ** 2))
            unit = centre / r
            theta, phi = torch.acos(unit[1]), torch.atan2(unit[0], unit[2])
        if phi < 0.0:
            phi += 2 * np.pi
        radius.append(r * 1.0)
        thetas.append(theta * 180.0 / np.pi)
        phis.append(phi * 180.0 / np.pi)
    return torch.tensor(radius), torch.tensor(thetas), torch.tensor(phis)


def c2w_from_polar(radius, theta, phi, x_axis):
    """`get_c2w_from_polar` with an x axis, OpenGL, keep_chirality: radius, theta, phi fp32 [n] (degrees), x_axis fp32 [n,3] ->
    fp32 [n,4,4] with columns (x_axis, normalize(forward x x_axis), forward = normalize(centre), centre)"""
    theta, phi = theta / 180 * np.pi, phi / 180 * np.pi
    centres = torch.stack([radius * torch.sin(theta) * torch.sin(phi), radius * torch.cos(theta),
                           radius * torch.sin(theta) * torch.cos(phi)], dim=-1)
    forward = _safe_normalize(centres - 0)
    up = _safe_normalize(torch.cross(forward, x_axis, dim=-1))
    poses = torch.eye(4, dtype=torch.float).unsqueeze(0).repeat(forward.shape[0], 1, 1)
    poses[:, :3, :3] = torch.stack((x_axis, up, forward), dim=-1)
    poses[:, :3, 3] = centres
    return poses


def virtual_views(poses, intrinsics, size_h: int, size_w: int) -> dict:
    """`get_virtual_views`: poses fp32 [n,4,4], intrinsics float64 [n,4,4] -> radius / theta / phi (virtual), raw_radius / raw_theta
    / raw_phi (the real centres), poses_virt fp32 [n,4,4] and K_virt float64 [3,3] (frame 0's focal lengths, the window's centre)"""
    poses = torch.as_tensor(poses)
    radius, theta, phi = polar_from_c2w(poses, virtual=True)
    raw_radius, raw_theta, raw_phi = polar_from_c2w(poses, virtual=False)
    x_axis = torch.stack([c2w[:3, 0] for c2w in poses], dim=0)
    intrinsics = torch.as_tensor(intrinsics)
    K_virt = np.array([[float(intrinsics[0, 0, 0]), 0.0, size_w / 2], [0.0, float(intrinsics[0, 1, 1]), size_h / 2], [0.0, 0.0, 1.0]])
    return dict(radius=radius, theta=theta, phi=phi, raw_radius=raw_radius, raw_theta=raw_theta, raw_phi=raw_phi,
                poses_virt=c2w_from_polar(radius, theta, phi, x_axis), K_virt=K_virt)


def crop_centres(poses, K) -> np.ndarray:
    """Where the world centre falls in every frame -> int64 [n,2] = (px, py).  The reference's chain: OpenGL -> OpenCV axes, the
    inverse in fp32, the projection K (R 0 + t) in float64, int(px / pz) truncating towards zero."""
    out = []
    for c2w, Kf in zip(torch.as_tensor(poses).numpy().astype(np.float32), torch.as_tensor(K).numpy().astype(np.float64)):
        c2w = c2w.copy()
        c2w[:, 1] *= -1
        c2w[:, 2] *= -1
        w2c = np.linalg.inv(c2w)
        x_c = w2c[:3, :3] @ np.zeros((3,)) + w2c[:3, -1]
        px, py, pz = Kf[:3, :3] @ x_c
        out.append((int(px / pz), int(py / pz)))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def window_origins(centres, size_h: int, size_w: int) -> np.ndarray:
    """(px, py) [n,2] -> (top, left) int64 [n,2] = (py - size_h // 2 + 1, px - size_w // 2 + 1)"""
    c = np.asarray(centres, dtype=np.int64).reshape(-1, 2)
    return np.stack([c[:, 1] - size_h // 2 + 1, c[:, 0] - size_w // 2 + 1], -1)


# --------------------------------------------------------------------------------------------------------------------- frames
def depth_tables(depth_scale: float, scale: float):
    """What the reference writes for every raw 16-bit depth -> (table_inside, table_padded) uint16 [65536], in its own expressions:
    d = fp32(raw / depth_scale), d *= scale in fp32, then `(d * 1000).astype(uint16)` with the product in fp32 (a window inside the
    frame: a slice of the fp32 array) or in float64 (every other window: np.zeros((h, w))).  The 1000 is the reference's constant,
    not depth_scale.  A value that does not fit 16 bits saturates (this build's rule)."""
    raw = np.arange(65536).astype(np.uint16)
    d = (raw / depth_scale).astype(np.float32)
    d *= np.array([scale], dtype=np.float32)
    inside, padded = d * 1000, d.astype(np.float64) * 1000
    return np.clip(inside, 0, 65535).astype(np.uint16), np.clip(padded, 0, 65535).astype(np.uint16)


def rotation_matrix(centre, rot_degree: float) -> np.ndarray:
    """The forward 2 x 3 map of a rotation by `rot_degree` about `centre` = (cx, cy), float64:
    [[c, s, (1 - c) cx - s cy], [-s, c, s cx + (1 - c) cy]]"""
    c, s = math.cos(rot_degree * math.pi / 180.0), math.sin(rot_degree * math.pi / 180.0)
    cx, cy = float(centre[0]), float(centre[1])
    return np.array([[c, s, (1 - c) * cx - s * cy], [-s, c, s * cx + (1 - c) * cy]], dtype=np.float64)


def invert_affine(M) -> np.ndarray:
    """2 x 3 map -> the six numbers of its inverse (a0 a1 a2 / a3 a4 a5), float64"""
    M = np.asarray(M, dtype=np.float64)
    det = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    i00, i01, i10, i11 = M[1, 1] / det, -M[0, 1] / det, -M[1, 0] / det, M[0, 0] / det
    return np.array([i00, i01, -(i00 * M[0, 2] + i01 * M[1, 2]), i10, i11, -(i10 * M[0, 2] + i11 * M[1, 2])], dtype=np.float64)


class PreprocessResult:
    """What `preprocess` made.  On the device, DeviceDataset's storage layout: rgb uint8 [F,h,w,3], depth uint16 [F,h,w], mask and
    padding uint8 [F,h,w].  On the host: poses_virt fp32 [F,4,4], K_virt float64 [3,3], radius / theta / phi and raw_radius /
    raw_theta / raw_phi fp32 [F], crop_centres int64 [F,2] (px, py), origin int64 [F,2] (top, left), inv_affine float64 [F,6],
    table_inside / table_padded uint16 [65536]."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def write_dir(self, data_dir) -> None:
        """The reference's layout under `data_dir`: color_virt/, depth_raw_crop/, mask_virt/, padding_mask/ as %06d.png,
        poses_virt/%06d.txt, K_virt.txt, r_theta_phi.txt, raw_r_theta_phi.txt, crop_centre_list.txt"""
        from PIL import Image
        planes = {"color_virt": self.rgb, "depth_raw_crop": self.depth, "mask_virt": self.mask, "padding_mask": self.padding}
        for sub in list(planes) + ["poses_virt"]:
            os.makedirs(os.path.join(data_dir, sub), exist_ok=True)
        for sub, frames in planes.items():
            for i, frame in enumerate(frames.cpu().numpy()):
                Image.fromarray(frame).save(os.path.join(data_dir, sub, "{:06d}.png".format(i)))
        for i, c2w in enumerate(self.poses_virt):
            np.savetxt(os.path.join(data_dir, "poses_virt", "{:06d}.txt".format(i)), c2w.cpu().numpy())
        np.savetxt(os.path.join(data_dir, "K_virt.txt"), self.K_virt)
        np.savetxt(os.path.join(data_dir, "r_theta_phi.txt"), torch.stack([self.radius, self.theta, self.phi], dim=-1).numpy())
        np.savetxt(os.path.join(data_dir, "raw_r_theta_phi.txt"),
                   torch.stack([self.raw_radius, self.raw_theta, self.raw_phi], dim=-1).numpy())
        np.savetxt(os.path.join(data_dir, "crop_centre_list.txt"), self.crop_centres)


def preprocess(rgb, depth, mask, cameras, config, device="cuda") -> PreprocessResult:
    """`DataProcessor.preprocess` without its files.  rgb uint8 [F,H,W,3], depth uint16 [F,H,W] (raw), mask uint8 [F,H,W] (numpy or
    torch, any device); `cameras`: the world_mat_i / scale_mat_i mapping of cameras_sphere.npz, or (poses, intrinsics, scales) as
    `camera_params` returns them; config["data"] holds size_h, size_w, rot_degree (0 when absent) and depth_scale."""
    d = config["data"]
    size_h, size_w, rot_degree = int(d["size_h"]), int(d["size_w"]), float(d.get("rot_degree", 0.0))
    rgb, depth, mask = (v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v)) for v in (rgb, depth, mask))
    F = rgb.shape[0]
    if isinstance(cameras, (tuple, list)):
        poses, intrinsics, scales = cameras
    else:
        poses, intrinsics, scales, _ = camera_params(cameras, F)
    poses, intrinsics = torch.as_tensor(poses).to(torch.float32), torch.as_tensor(intrinsics).to(torch.float64)
    scales = np.unique(torch.as_tensor(scales).to(torch.float32).numpy().reshape(-1))
    if len(poses) != F or len(intrinsics) != F:
        raise ValueError(f"{F} frames need {F} poses and intrinsics, got {len(poses)} and {len(intrinsics)}")
    if len(scales) != 1 or not np.isfinite(scales[0]) or scales[0] <= 0:
        raise ValueError(f"the frames must share one positive depth scale (create_camera.py writes one scale_mat), got {scales}")
    views = virtual_views(poses, intrinsics, size_h, size_w)
    centres = crop_centres(poses, intrinsics)
    origin = window_origins(centres, size_h, size_w)
    if np.abs(origin).max() >= 2 ** 31:
        raise ValueError("a window origin does not fit 32 bits")
    inv = np.stack([invert_affine(rotation_matrix(c, rot_degree)) for c in centres])
    if not np.isfinite(inv).all():
        raise ValueError("rot_degree gives a non-finite affine map")
    table_inside, table_padded = depth_tables(float(d["depth_scale"]), float(scales[0]))
    dev = torch.device(device)
    out = ops.prep_frames(rgb.to(dev), depth.to(dev), mask.to(dev), torch.from_numpy(origin.astype(np.int32)).to(dev),
                          torch.from_numpy(inv).to(dev), torch.full((F,), int(rot_degree != 0.0), dtype=torch.uint8, device=dev),
                          torch.from_numpy(table_inside).to(dev), torch.from_numpy(table_padded).to(dev), size_h, size_w)
    return PreprocessResult(rgb=out["rgb"], depth=out["depth"], mask=out["mask"], padding=out["padding"], crop_centres=centres,
                            origin=origin, inv_affine=inv, table_inside=table_inside, table_padded=table_padded, size_h=size_h,
                            size_w=size_w, rot_degree=rot_degree, scale=float(scales[0]), **views)


def read_raw_dir(data_dir):
    """rgb/ (.jpg, else .png), depth/ and mask/ (the first as many as there are rgb frames) under `data_dir` with PIL -> (rgb uint8
    [F,H,W,3], depth uint16 [F,H,W], mask uint8 [F,H,W]).  A mask image with colour channels gives the channel cv2's BGR decode
    puts first: the BLUE plane of an RGB decode."""
    from PIL import Image

    def listed(sub):
        return sorted(glob(os.path.join(data_dir, sub, "*.jpg"))) or sorted(glob(os.path.join(data_dir, sub, "*.png")))

    def read(path, what):
        with Image.open(path) as im:
            if what == "rgb":
                return np.asarray(im.convert("RGB"), dtype=np.uint8)
            if what == "mask":
                if im.mode != "L":
                    return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8)[..., 2])
                return np.asarray(im, dtype=np.uint8)
            a = np.asarray(im)
            if a.ndim != 2 or a.min() < 0 or a.max() > 65535:
                raise ValueError(f"{path}: expected one channel of 16-bit depth, got shape {a.shape}")
            return a.astype(np.uint16)

    names = listed("rgb")
    if not names:
        raise FileNotFoundError(f"no rgb/*.jpg or rgb/*.png under {data_dir}")
    n = len(names)
    rgb = np.stack([read(p, "rgb") for p in names])
    depth = np.stack([read(p, "depth") for p in listed("depth")[:n]])
    mask = np.stack([read(p, "mask") for p in listed("mask")[:n]])
    if depth.shape != rgb.shape[:3] or mask.shape != rgb.shape[:3]:
        raise ValueError(f"rgb {rgb.shape[:3]}, depth {depth.shape} and mask {mask.shape} do not agree")
    return rgb, depth, mask


def preprocess_dir(config, device="cuda") -> PreprocessResult:
    """Read the raw sequence and data.render_cameras_name under data.data_dir and run `preprocess`; nothing is written
    (`.write_dir(data_dir)` does that)."""
    root = config["data"]["data_dir"]
    rgb, depth, mask = read_raw_dir(root)
    with np.load(os.path.join(root, config["data"]["render_cameras_name"])) as z:
        cameras = {k: z[k] for k in z.files}
    return preprocess(rgb, depth, mask, cameras, config, device)
