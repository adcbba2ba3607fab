"""Device-resident dataset: real-view batches and virtual views from csrc/dataset.hip.

`DeviceDataset` stands where the reference's `datasets/dataset.py:DeformDataset` stands and keeps its attribute names.  The frames
stay on the device in their file precision -- rgb uint8 [F,H,W,3], depth uint16 (or fp32) [F,H,W], mask uint8 [F,H,W]: 6 bytes
a pixel against the reference's 60 -- and no table of rays is built: a real-view batch is ONE launch that forms the rays from
the frame's device pose and gathers colour, depth and mask (`ops.dataset_sample`); a virtual view is two (`ops.dataset_virtual_pose`
for pose, label and deltas, `ops.generate_rays_dev` for the rays), and the pose never visits the host.  With the indices drawn
on the device a call makes no device-to-host transfer.

What is the reference's bit for bit and what is judged in float64 instead: the header comment of csrc/dataset.hip.
The image decode stays on the host and happens once (`from_dir`, PIL and numpy; `from_raw` reads a RAW sequence and cuts its frames
on the device through morpheus_amd.preprocess, with no files in between).  Resized known views
(`data.known_view_scale != 1.0`) are not implemented.  Sampling needs the frames on an MI355X: there is no CPU path.
"""
from __future__ import annotations

import copy
import numbers
import os
import random
from glob import glob
from typing import Optional

import numpy as np
import torch

from . import ops
from ._lib import MorpheusHipError


def remove_outlier(poses, theta, phi, radius, num_frames: int, thresh: float = 2.0):
    """The reference's translation-outlier rule (BaseDataset.remove_outlier), torch on the CPU.

    The step lengths between consecutive camera centres are turned into z-scores.  Every step whose |z| exceeds `thresh` is a
    suspect.  For a suspect step into frame k, the step is measured again on the REPAIRED sequence; if its z-score (signed,
    against the original mean and deviation) still exceeds `thresh`, frame k takes the pose, theta, phi and radius of frame
    k - 1, and if the step from the repaired frame k into frame k + 1 is an outlier too the walk goes on to k + 1.
    -> (new poses, the repaired frames); theta, phi and radius are rewritten IN PLACE."""
    trans = poses[:, :3, 3]
    step = (trans[1:] - trans[:-1]).square().sum(-1).sqrt()
    mean, std = torch.mean(step), torch.std(step)
    suspects = torch.where(torch.abs((step - mean) / std) > thresh)[0]
    trans_new, pose_new, repaired = trans.clone(), poses.clone(), []
    for i in suspects.tolist():
        k = i + 1
        while k <= num_frames - 1:
            d = (trans_new[k] - trans_new[k - 1]).square().sum(-1).sqrt()
            if not bool((d - mean) / std > thresh):
                break
            repaired.append(k)
            trans_new[k] = trans_new[k - 1].clone()
            pose_new[k] = pose_new[k - 1].clone()
            for v in (theta, phi, radius):
                v[k] = v[k - 1].clone()
            if k > num_frames - 2:
                break
            d_next = (trans_new[k + 1] - trans_new[k]).square().sum(-1).sqrt()
            if not bool((d_next - mean) / std > thresh):
                break
            k += 1
    return pose_new, repaired


def _label_bounds(front: float, overhead: float):
    """the six thresholds of the reference's get_view_direction as its float64 expressions (the kernel compares at fp32)"""
    return (front / 2, np.pi - front / 2, np.pi + front / 2, 2 * np.pi - front / 2, overhead, np.pi - overhead)


def view_direction(thetas, phis, overhead: float, front: float):
    """The six-way view label of angles in radians on the host (datasets/utils.py:70-91): 0 front, 1 left side, 2 back, 3 right
    side by phi % 2 pi, then 4 top / 5 bottom by theta.  The device form is csrc/dataset.hip:virtual_pose_kernel."""
    lo, back, left, wrap, over, bottom = _label_bounds(front, overhead)
    res = torch.zeros(thetas.shape[0], dtype=torch.long)
    phis = phis % (2 * np.pi)
    res[(phis >= left) & (phis < wrap)] = 1
    res[(phis >= back) & (phis < left)] = 2
    res[(phis >= lo) & (phis < back)] = 3
    res[thetas <= over] = 4
    res[thetas >= bottom] = 5
    return res


class DeviceDataset:
    def __init__(self, config, rgb, depth, mask, poses, intrinsics, radius, theta, phi, device="cuda", is_train: bool = True):
        """From arrays (numpy or torch): rgb uint8 [F,H,W,3], depth uint16 or float32 [F,H,W] (raw values: metres are
        depth / data.depth_scale), mask uint8 [F,H,W], poses [P,4,4] camera-to-world, intrinsics [3,3], radius / theta / phi [P].
        The arrays are moved to `device`; poses, theta, phi and radius are also kept on the CPU under the reference's names.
        P may exceed F (`from_dir` with a `test_id` subset): as in the reference, frame k then goes with row k of the tables;
        the host copies keep every row, the device copies the first F."""
        if config["data"].get("known_view_scale", 1.0) != 1.0:
            raise NotImplementedError("data.known_view_scale != 1.0: the reference resizes the known views with cv2's resize "
                                      "(INTER_LINEAR / INTER_NEAREST), which is not restated here; every shipped config has 1.0")
        self.cfg, self.data_dir, self.is_train = config, config["data"].get("data_dir"), is_train
        self.device = torch.device(device)
        rgb, depth, mask = (torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v) for v in (rgb, depth, mask))
        if rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[-1] != 3:
            raise ValueError(f"rgb must be uint8 [F,H,W,3], got {rgb.dtype} {tuple(rgb.shape)}")
        self.num_frames, self.H, self.W = (int(s) for s in rgb.shape[:3])
        if depth.dtype not in (torch.uint16, torch.float32) or depth.shape != rgb.shape[:3]:
            raise ValueError(f"depth must be uint16 or float32 {tuple(rgb.shape[:3])}, got {depth.dtype} {tuple(depth.shape)}")
        if mask.dtype != torch.uint8 or mask.shape != rgb.shape[:3]:
            raise ValueError(f"mask must be uint8 {tuple(rgb.shape[:3])}, got {mask.dtype} {tuple(mask.shape)}")
        self.intrinsics = torch.as_tensor(np.asarray(intrinsics, dtype=np.float64)).reshape(3, 3).clone()
        self.radius, self.theta, self.phi = (torch.as_tensor(np.asarray(v)).to(torch.float32).reshape(-1).clone()
                                             for v in (radius, theta, phi))
        poses = torch.as_tensor(np.asarray(poses)).to(torch.float32).reshape(-1, 4, 4).clone()
        if len(poses) < self.num_frames or any(len(v) != len(poses) for v in (self.radius, self.theta, self.phi)):
            raise ValueError("poses, radius, theta and phi need one row per frame")
        self.outliers = []
        if config["data"].get("outlier_remove", False):
            poses, self.outliers = remove_outlier(poses, self.theta, self.phi, self.radius, self.num_frames)
        self.poses = poses
        self.bounding_box = torch.tensor([-1.01, -1.01, -1.01, 1.01, 1.01, 1.01]).to(torch.float32)
        self.bound = self.bounding_box.abs().max()
        self.depth_scale = float(config["data"]["depth_scale"])
        dev = self.device
        self.rgb_dev, self.depth_dev, self.mask_dev = (v.contiguous().to(dev) for v in (rgb, depth, mask))
        self.poses_dev, self.radius_dev, self.theta_dev, self.phi_dev = (v.contiguous().to(dev) for v in
                                                                         (v[:self.num_frames] for v in
                                                                          (self.poses, self.radius, self.theta, self.phi)))
        self._intri = self.scale_intrinsics(self.intrinsics, 1.0)      # known_view_scale is 1.0 here
        self._host = {}

    # ------------------------------------------------------------------------------------------------------------ loading
    @classmethod
    def from_dir(cls, config, device="cuda", test_id=None, is_train: bool = True):
        """Read the reference's directory layout under data.data_dir with PIL and numpy: color_virt/*.png (RGB),
        depth_raw_crop/*.png (16 bit), mask_virt/*.png, poses_virt/*.txt, K_virt.txt, r_theta_phi.txt.  `test_id` picks frames of
        the three image lists, as the reference does; poses and r_theta_phi keep every row."""
        from PIL import Image
        root = config["data"]["data_dir"]

        def listed(sub):
            paths = sorted(glob(os.path.join(root, sub, "*.png")))
            return paths if test_id is None else [paths[i] for i in test_id]

        def read(path, what):
            with Image.open(path) as im:
                if what == "rgb":
                    return np.asarray(im.convert("RGB"), dtype=np.uint8)
                a = np.asarray(im)
                if a.ndim != 2:
                    raise ValueError(f"{path}: expected one channel, got shape {a.shape}")
                if what == "depth":
                    if a.min() < 0 or a.max() > 65535:
                        raise ValueError(f"{path}: depth values outside 16 bits")
                    return a.astype(np.uint16)
                if a.dtype != np.uint8:
                    raise ValueError(f"{path}: expected an 8-bit mask, got {a.dtype}")
                return a

        rgb = np.stack([read(p, "rgb") for p in listed("color_virt")])
        depth = np.stack([read(p, "depth") for p in listed("depth_raw_crop")])
        mask = np.stack([read(p, "mask") for p in listed("mask_virt")])
        K = np.loadtxt(os.path.join(root, "K_virt.txt"))
        rtp = np.loadtxt(os.path.join(root, "r_theta_phi.txt")).reshape(-1, 3)
        poses = np.stack([np.loadtxt(p) for p in sorted(glob(os.path.join(root, "poses_virt", "*.txt")))])
        return cls(config, rgb, depth, mask, poses, K, rtp[:, 0], rtp[:, 1], rtp[:, 2], device=device, is_train=is_train)

    @classmethod
    def from_raw(cls, config, device="cuda", pre=None, is_train: bool = True):
        """From a RAW sequence under data.data_dir (rgb/, depth/, mask/ and data.render_cameras_name): `preprocess.preprocess_dir`
        forms the virtual cameras and cuts the frames on the device, and the device tensors go to the constructor as they are --
        no files in between, no host round trip.  The preprocessing keys (size_h, size_w, rot_degree, depth_scale) are read from
        config["data"]; `pre` overrides them, for a training YAML that lacks them or whose depth_scale describes the CUT frames
        (the reference writes those with its constant 1000) rather than the raw ones.  The dataset itself keeps `config`."""
        from . import preprocess
        r = preprocess.preprocess_dir({**config, "data": {**config["data"], **(pre or {})}}, device)
        ds = cls(config, r.rgb, r.depth, r.mask, r.poses_virt, r.K_virt, r.radius, r.theta, r.phi, device=device, is_train=is_train)
        ds.preprocessed = r
        return ds

    # ------------------------------------------------------------------------------- the reference's host-side attributes
    def _host_view(self, name, make):
        if name not in self._host:
            self._host[name] = make()
        return self._host[name]

    @property
    def depths(self):
        """float64 [F,H,W] in metres on the host, made on first use (eval_depth_l1 reads it)"""
        return self._host_view("depths", lambda: self.depth_dev.cpu().numpy().astype(np.float64) / self.depth_scale)

    @property
    def masks(self):
        """float64 [F,H,W] = byte / 255 on the host, made on first use"""
        return self._host_view("masks", lambda: self.mask_dev.cpu().numpy().astype(np.float64) / 255.0)

    @property
    def resident_bytes(self) -> int:
        return sum(v.numel() * v.element_size() for v in (self.rgb_dev, self.depth_dev, self.mask_dev, self.poses_dev,
                                                          self.radius_dev, self.theta_dev, self.phi_dev))

    def get_radius(self, t):
        return self.radius[t]

    def scale_intrinsics(self, intrinsics, scale):
        intrinsics = copy.deepcopy(intrinsics)
        intrinsics[..., :2, :3] *= scale
        return intrinsics

    def get_c2w_from_cam_center(self, cam_centers, targets=0, camera_convention="OpenGL"):
        """Host look-at towards `targets` (OpenGL, keep_chirality), in the dtype of `cam_centers`: for callers of the reference's
        name.  The training path forms its poses on the device."""
        if camera_convention != "OpenGL":
            raise NotImplementedError("only the OpenGL convention is used by the reference's callers")

        def unit(x):
            return x / torch.sqrt(torch.clamp(torch.sum(x * x, -1, keepdim=True), min=1e-20))
        forward = unit(cam_centers - targets)
        up = torch.tensor([0.0, 1.0, 0.0], dtype=forward.dtype).expand_as(forward)
        right = unit(torch.linalg.cross(up, forward, dim=-1))
        up = unit(torch.linalg.cross(forward, right, dim=-1))
        poses = torch.eye(4, dtype=forward.dtype).unsqueeze(0).repeat(forward.shape[0], 1, 1)
        poses[:, :3, :3] = torch.stack((right, up, forward), dim=-1)
        poses[:, :3, 3] = cam_centers
        return poses

    def get_c2w_from_polar(self, t=None, radius=None, theta=torch.tensor([60.0]), phi=torch.tensor([0.0]), return_dirs=True,
                           angle_overhead=30, angle_front=60, radius_scale=None):
        """Host poses and view labels from polar angles in degrees -> ([B,4,4], int64 [B] | None), for callers of the
        reference's name (morpheus.py:449)."""
        if t is not None:
            radius = self.get_radius(t)
        if radius_scale is not None:
            radius = radius_scale * radius
        theta, phi = theta / 180 * np.pi, phi / 180 * np.pi
        centres = torch.stack([radius * torch.sin(theta) * torch.sin(phi), radius * torch.cos(theta),
                               radius * torch.sin(theta) * torch.cos(phi)], dim=-1)
        dirs = view_direction(theta, phi, angle_overhead / 180 * np.pi, angle_front / 180 * np.pi) if return_dirs else None
        return self.get_c2w_from_cam_center(centres), dirs

    # --------------------------------------------------------------------------------------------------------- real views
    def _frames(self, idx, bs, what="idx"):
        """frame indices -> int64 [B] on the device; indices handed in on the CPU are checked here, device ones are clamped
        by the kernels"""
        if idx is None:
            return torch.randint(0, self.num_frames, (bs,), device=self.device)
        if isinstance(idx, numbers.Integral):
            idx = torch.tensor([int(idx)])
        idx = torch.as_tensor(idx)
        if idx.dim() == 0:
            idx = idx.reshape(1)
        if idx.dim() != 1 or idx.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"{what} must be an int or a one-dimensional integer tensor")
        if not idx.is_cuda and idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.num_frames):
            raise IndexError(f"{what} outside [0, {self.num_frames})")
        return idx.to(device=self.device, dtype=torch.int64)

    def sample_real_view_rays(self, idx=None, bs=1, ray_num: Optional[int] = None, index=None):
        """The reference's batch (dataset.py:398-433), tensors on the device.  `idx`: frames (integer, sequence or tensor; None: `bs`
        frames drawn on the device).  `ray_num` pixels, one draw shared by the batch: `index` (int32 pixel indices j*W+i) or,
        without it, drawn on the device.  Without `ray_num` and `index`: whole frames."""
        frames = self._frames(idx, bs)
        B, HW = frames.shape[0], self.H * self.W
        if index is not None:
            index = torch.as_tensor(index)
            if index.dim() != 1 or index.dtype != torch.int32:
                raise ValueError("index must be a one-dimensional int32 tensor")
            if ray_num is not None and index.shape[0] != ray_num:
                raise ValueError(f"index holds {index.shape[0]} pixels, ray_num is {ray_num}")
            if not index.is_cuda and index.numel() and (int(index.min()) < 0 or int(index.max()) >= HW):
                raise IndexError(f"index outside [0, {HW})")
            index = index.to(self.device)
        elif ray_num is not None:
            index = torch.randint(0, HW, (ray_num,), device=self.device, dtype=torch.int32)
        if not self.rgb_dev.is_cuda:      # after the argument checks; with the frames on the CPU nothing above touched a GPU
            raise MorpheusHipError(f"DeviceDataset: the frames are on {self.rgb_dev.device}; sampling runs on an MI355X only, "
                                   "there is no CPU path")
        intri = self._intri.clone()
        o = ops.dataset_sample(intri, self.poses_dev, self.rgb_dev, self.depth_dev, self.mask_dev, self.theta_dev, self.phi_dev,
                               self.radius_dev, self.depth_scale, frames, index)
        if index is None:
            H, W, tail = self.H, self.W, (self.H, self.W)
        else:
            H, W, tail = index.shape[0], 1, (index.shape[0], 1)
        return {"rays_o": o["rays_o"], "rays_d": o["rays_d"], "rays_t": o["rays_t"], "rays_id": o["rays_id"], "H": H, "W": W,
                "image": o["image"].view(B, 3, *tail), "depth": o["depth"].view(B, *tail), "mask": o["mask"].view(B, *tail),
                "intri": intri, "pose": o["pose"], "theta": o["theta"], "phi": o["phi"], "radius": o["radius"]}

    # ------------------------------------------------------------------------------------------------------ virtual views
    def get_virtual_view_rays(self, bs=1, t=None, is_train=True, scale=None, phis=0, draws=None):
        """The reference's virtual view (dataset.py:503-578) on the device, plus `pose` [B,4,4] and `deg` [B,2] (theta, phi in
        degrees).  `draws` injects the random numbers: {"thetas", "phis"} fp32 [B] in radians (the theta/phi box) or {"normals"}
        fp32 [B,3] (the uniform sphere: column k is the k-th normal draw); without it they are drawn on the device, and the
        choice of the branch (random.random() < data.uniform_sphere_rate) stays a host decision.  In the sphere branch every
        view is scaled by its own frame's radius (the reference's expression broadcasts only for bs = 1, where both agree)."""
        d, dev = self.cfg["data"], self.device
        frames = self._frames(t, bs, "t")
        B = frames.shape[0]
        if not self.radius_dev.is_cuda:
            raise MorpheusHipError(f"DeviceDataset: the tables are on {self.radius_dev.device}; virtual views run on an MI355X "
                                   "only, there is no CPU path")
        f32 = dict(device=dev, dtype=torch.float32)
        if is_train:
            front, overhead = float(np.deg2rad(d["angle_front"])), float(np.deg2rad(d["angle_overhead"]))
            factor = d["novel_view_scale_factor"]
            if draws is None:
                if random.random() < d["uniform_sphere_rate"]:
                    draws = {"normals": torch.randn(B, 3, **f32)}
                else:
                    tr, pr = np.deg2rad(d["theta_range"]), np.deg2rad(d["phi_range"])
                    draws = {"thetas": torch.rand(B, **f32) * float(tr[1] - tr[0]) + float(tr[0]),
                             "phis": torch.rand(B, **f32) * float(pr[1] - pr[0]) + float(pr[0])}
            if "normals" in draws:
                n = torch.as_tensor(draws["normals"]).to(**f32)
                if n.shape != (B, 3):
                    raise ValueError(f"draws['normals'] must be [{B}, 3]")
                mode, (a, b, c) = ops.VIRTUAL_SPHERE, n.t().contiguous().unbind(0)
            else:
                mode, c = ops.VIRTUAL_ANGLES, None
                a, b = (torch.as_tensor(draws[k]).to(**f32).reshape(-1) for k in ("thetas", "phis"))
        else:
            if B != 1:
                raise ValueError("is_train=False renders one view of one frame")
            front, overhead = d["angle_front"] / 180 * np.pi, d["angle_overhead"] / 180 * np.pi
            factor, mode, c = 1.0, ops.VIRTUAL_POLAR, None
            a, b = torch.tensor([d["default_polar"]], **f32), torch.tensor([phis * 360], **f32)
        v = ops.dataset_virtual_pose(mode, a, b, c, frames, self.radius_dev, self.theta_dev, self.phi_dev, factor,
                                     _label_bounds(front, overhead))
        if scale is not None:
            H, W, intri = int(scale * self.H), int(scale * self.W), self.scale_intrinsics(self.intrinsics, scale=scale)
        elif self.is_train:
            s = d["novel_view_scale"]
            H, W, intri = int(s * self.H), int(s * self.W), self.scale_intrinsics(self.intrinsics, scale=s)
        else:
            H, W, intri = self.H, self.W, self.intrinsics
        rays_o, rays_d, rays_t, rays_id = ops.generate_rays_dev(intri, v["pose"], H, W, None, frames, self.num_frames)
        return {"H": H, "W": W, "rays_o": rays_o, "rays_d": rays_d, "rays_t": rays_t, "rays_id": rays_id, "dir": v["dir"],
                "polar": v["polar"], "azimuth": v["azimuth"], "radius": v["radius"], "pose": v["pose"], "deg": v["deg"]}
