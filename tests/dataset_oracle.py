"""Restatement of the reference's dataset stage (datasets/dataset.py:DeformDataset) -- test infrastructure, torch on the CPU.

What morpheus_amd.dataset / csrc/dataset.hip must reproduce, stated once:
  * real views (`real_view`): the ray of pixel (i, j) of frame f, rays_t = f / F (fp32 quotient of the two fp32 values), rays_id = f,
    image = fp32(u8 / 255.0 in float64), depth = fp32(u16 / depth_scale in float64), mask = 1 where the byte is 255 else 0 --
    all fp32 operator chains, equal to the reference BIT FOR BIT (tests/golden/dataset.npz, tools/make_dataset_golden.py);
  * virtual views (`virtual_view`): from fp32 angles in radians, bit for bit: the label (thresholds rounded to fp32, phi % 2 pi
    in fp32), the degree values (/ pi * 180), the deltas and the `> 180 -> -360` wrap.  The look-at pose is stated in FLOAT64 from
    the fp32 inputs (the fp32 radius product, the fp32 angles or the three normal draws): the reference's fp32 pose and the
    kernel's are both judged against it.  In the sphere branch the fp32 angles are not inputs: `sphere_angles` restates the
    reference's fp32 chain (normalize with its fused sum, acos, the C library's atan2f), and they equal the golden bit for bit.
The golden's inputs and the configuration it was recorded with are defined here (`make_inputs`, `CONFIG`) so that the tool and
the tests share them.
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset.npz")
F, H, W = 5, 6, 8
CONFIG = {"data": {"data_dir": "unused", "depth_scale": 1000.0, "known_view_scale": 1.0, "novel_view_scale": 0.5,
                   "novel_view_scale_factor": 1.25, "theta_range": [45, 105], "phi_range": [-180, 180], "angle_overhead": 30,
                   "angle_front": 60, "default_polar": 80.0, "uniform_sphere_rate": 0.5, "outlier_remove": False}}
F32, F64 = torch.float32, torch.float64
ANGLES, SPHERE, POLAR = 0, 1, 2
REAL_KEYS = ("rays_o", "rays_d", "rays_t", "rays_id", "image", "depth", "mask", "pose", "theta", "phi", "radius")
VIRTUAL_CASES = ("box", "sphere0", "sphere1", "sphere2", "polar0", "polar1")


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def look_at_np(centres):
    """float64 numpy look-at (OpenGL, towards the origin, keep_chirality) -> [B,4,4]"""
    def unit(x):
        return x / np.sqrt(np.maximum((x * x).sum(-1, keepdims=True), 1e-20))
    fwd = unit(centres)
    right = unit(np.cross(np.broadcast_to(np.array([0.0, 1.0, 0.0]), fwd.shape), fwd))
    up = unit(np.cross(fwd, right))
    P = np.tile(np.eye(4), (len(centres), 1, 1))
    P[:, :3, :3] = np.stack([right, up, fwd], -1)
    P[:, :3, 3] = centres
    return P


def make_inputs():
    """the golden's frames: F = 5 of 6 x 8 (H != W); rgb with 0 and 255, depth with 0 and 65535, masks with 0, 128, 254, 255;
    generic look-at poses with a roll, so that no rotation is axis-aligned"""
    rng = np.random.default_rng(20240518)
    rgb = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    rgb[0, 0, 0], rgb[4, H - 1, W - 1] = (0, 255, 1), (255, 0, 254)
    depth = rng.integers(300, 4000, (F, H, W)).astype(np.uint16)
    depth[1, 2, 3], depth[2, 0, 0], depth[2, H - 1, W - 1], depth[3, 1, 1] = 0, 65535, 1, 65534
    mask = rng.choice(np.array([0, 128, 254, 255], dtype=np.uint8), (F, H, W))
    mask[3, 0, :4] = (0, 128, 254, 255)
    radius = rng.uniform(1.5, 2.5, F)
    theta = rng.uniform(50.0, 100.0, F)
    phi = rng.uniform(0.0, 40.0, F)
    th, ph = np.deg2rad(theta), np.deg2rad(phi)
    centres = np.stack([radius * np.sin(th) * np.sin(ph), radius * np.cos(th), radius * np.sin(th) * np.cos(ph)], -1)
    poses = look_at_np(centres)
    for f in range(F):                      # a roll about the viewing axis
        a = 0.2 + 0.3 * f
        roll = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        poses[f, :3, :3] = poses[f, :3, :3] @ roll
    K = np.array([[9.3, 0.0, 4.1], [0.0, 9.7, 2.9], [0.0, 0.0, 1.0]])
    return dict(rgb=rgb, depth=depth, mask=mask, poses=poses.astype(np.float32), K=K, radius=radius.astype(np.float32),
                theta=theta.astype(np.float32), phi=phi.astype(np.float32))


def outlier_sequence():
    """20 poses on a gentle arc with frames 4 and 5 thrown far off (two consecutive translation outliers) -> poses, r/theta/phi"""
    n = 20
    c = np.stack([np.linspace(-0.4, 0.4, n), 0.3 + 0.02 * np.arange(n) ** 1.5, 2.0 - 0.01 * np.arange(n)], -1)
    c[4] += (3.0, -2.0, 1.5)
    c[5] += (3.1, -2.1, 1.4)
    poses = look_at_np(c).astype(np.float32)
    rtp = np.stack([np.linspace(1.9, 2.1, n), np.linspace(60, 90, n), np.linspace(0, 35, n)], -1).astype(np.float32)
    return poses, rtp


def scaled_K(K, scale):
    K = torch.as_tensor(np.asarray(K, dtype=np.float64)).clone()
    if scale is not None:
        K[:2, :3] *= scale
    return K


def rays(K, pose32, Hh, Ww, index=None):
    """fp32 rays of the pixels `index` (None: all) for poses [B,4,4] -> rays_o, rays_d [B,N,3]"""
    K = torch.as_tensor(np.asarray(K)).to(F32)          # the float64 entries meet an fp32 grid: they are used at fp32
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    pose32 = torch.as_tensor(pose32).to(F32)
    p = torch.arange(Hh * Ww) if index is None else torch.as_tensor(index).long()
    j, i = (p // Ww).to(F32), (p % Ww).to(F32)
    d0, d1, d2 = ((i + 0.5) - cx) / fx, -(((j + 0.5) - cy) / fy), -torch.ones_like(i)
    R = pose32[:, None, :3, :3]                          # [B,1,3,3]
    rays_d = (d0[None, :, None] * R[..., 0] + d1[None, :, None] * R[..., 1]) + d2[None, :, None] * R[..., 2]
    rays_o = pose32[:, None, :3, 3].expand(-1, p.shape[0], -1).contiguous()
    return rays_o, rays_d


def real_view(inp, idx, index=None, depth_scale=CONFIG["data"]["depth_scale"]):
    """the reference's sample_real_view_rays for frames `idx` and the pixel draw `index` (None: whole frames)"""
    idx = torch.as_tensor(idx).long().reshape(-1)
    B, nF = len(idx), inp["rgb"].shape[0]
    Hh, Ww = inp["rgb"].shape[1:3]
    pose = torch.as_tensor(inp["poses"]).to(F32)[idx]
    rays_o, rays_d = rays(inp["K"], pose, Hh, Ww, index)
    N = rays_o.shape[1]
    image = torch.from_numpy(inp["rgb"].astype(np.float64) / 255.0).permute(0, 3, 1, 2).to(F32)[idx].reshape(B, 3, -1)
    depth = torch.from_numpy(inp["depth"].astype(np.float64) / depth_scale).to(F32)[idx].reshape(B, -1)
    mask = torch.from_numpy((inp["mask"] == 255)).to(torch.int64)[idx].reshape(B, -1)
    if index is None:
        tail, Ho, Wo = (Hh, Ww), Hh, Ww
    else:
        sel = torch.as_tensor(index).long()
        image, depth, mask, tail, Ho, Wo = image[..., sel], depth[..., sel], mask[..., sel], (N, 1), N, 1
    return {"rays_o": rays_o, "rays_d": rays_d, "rays_t": (idx.to(F32) / torch.tensor(float(nF), dtype=F32))[:, None, None].repeat(1, N, 1),
            "rays_id": idx[:, None, None].repeat(1, N, 1), "H": Ho, "W": Wo, "image": image.reshape(B, 3, *tail),
            "depth": depth.reshape(B, *tail), "mask": mask.reshape(B, *tail), "intri": scaled_K(inp["K"], 1.0), "pose": pose,
            "theta": torch.as_tensor(inp["theta"])[idx], "phi": torch.as_tensor(inp["phi"])[idx],
            "radius": torch.as_tensor(inp["radius"])[idx]}


def label_bounds(front, overhead):
    """the six thresholds as float64, rounded to fp32 where they are compared"""
    b = (front / 2, np.pi - front / 2, np.pi + front / 2, 2 * np.pi - front / 2, overhead, np.pi - overhead)
    return [torch.tensor(float(x), dtype=F64).to(F32) for x in b]


def view_label(th, ph, front, overhead):
    lo, back, left, wrap, over, bottom = label_bounds(front, overhead)
    m = torch.remainder(ph, torch.tensor(2 * np.pi, dtype=F64).to(F32))
    res = torch.zeros(th.shape[0], dtype=torch.long)
    res[(m >= left) & (m < wrap)] = 1
    res[(m >= back) & (m < left)] = 2
    res[(m >= lo) & (m < back)] = 3
    res[th <= over] = 4
    res[th >= bottom] = 5
    return res


f32 = np.float32
_ATANHI = [f32(x) for x in (4.6364760399e-01, 7.8539812565e-01, 9.8279368877e-01, 1.5707962513e+00)]
_ATANLO = [f32(x) for x in (5.0121582440e-09, 3.7748947079e-08, 3.4473217170e-08, 7.5497894159e-08)]
_AT = [f32(x) for x in (3.3333334327e-01, -2.0000000298e-01, 1.4285714924e-01, -1.1111110449e-01, 9.0908870101e-02, -7.6918758452e-02,
                        6.6610731184e-02, -5.8335702866e-02, 4.9768779427e-02, -3.6531571299e-02, 1.6285819933e-02)]


def _word(x):
    return int(np.array(x, f32).view(np.int32))


def libm_atanf(x):
    """fdlibm's s_atanf.c on one np.float32: every operator rounds to fp32"""
    x = f32(x)
    hx = _word(x)
    ix = hx & 0x7fffffff
    if ix >= 0x4c800000:
        if ix > 0x7f800000:
            return x + x
        return _ATANHI[3] + _ATANLO[3] if hx > 0 else -_ATANHI[3] - _ATANLO[3]
    if ix < 0x3ee00000:
        if ix < 0x31000000:
            return x
        k = -1
    else:
        x = abs(x)
        if ix < 0x3f980000:
            if ix < 0x3f300000:
                k, x = 0, (f32(2) * x - f32(1)) / (f32(2) + x)
            else:
                k, x = 1, (x - f32(1)) / (x + f32(1))
        elif ix < 0x401c0000:
            k, x = 2, (x - f32(1.5)) / (f32(1) + f32(1.5) * x)
        else:
            k, x = 3, f32(-1) / x
    z = x * x
    w = z * z
    A = _AT
    s1 = z * (A[0] + w * (A[2] + w * (A[4] + w * (A[6] + w * (A[8] + w * A[10])))))
    s2 = w * (A[1] + w * (A[3] + w * (A[5] + w * (A[7] + w * A[9]))))
    if k < 0:
        return x - x * (s1 + s2)
    r = _ATANHI[k] - ((x * (s1 + s2) - _ATANLO[k]) - x)
    return -r if hx < 0 else r


def libm_atan2f(y, x):
    """fdlibm's e_atan2f.c for finite arguments, on np.float32: the C library's atan2f, which torch's CPU atan2 runs on strided
    columns"""
    y, x = f32(y), f32(x)
    tiny, pi_o_2, pi, pi_lo = f32(1.0e-30), f32(1.5707963705e+00), f32(3.1415927410e+00), f32(-8.7422776573e-08)
    hx, hy = _word(x), _word(y)
    ix, iy = hx & 0x7fffffff, hy & 0x7fffffff
    if ix > 0x7f800000 or iy > 0x7f800000:
        return x + y
    if hx == 0x3f800000:
        return libm_atanf(y)
    m = (1 if hy < 0 else 0) | (2 if hx < 0 else 0)
    if iy == 0:
        return y if m < 2 else (pi + tiny if m == 2 else -pi - tiny)
    if ix == 0:
        return -pi_o_2 - tiny if hy < 0 else pi_o_2 + tiny
    k = (iy - ix) >> 23
    if k > 60:
        z = pi_o_2 + f32(0.5) * pi_lo
    elif hx < 0 and k < -60:
        z = f32(0)
    else:
        z = libm_atanf(abs(y / x))
    return (z, -z, pi - (z - pi_lo), (z - pi_lo) - pi)[m]


def sphere_angles(a, b, c):
    """theta, phi (fp32 radians) of the uniform-sphere branch from the three normal draws, as the reference's CPU forms them in fp32:
    norm = sqrt(fma(z, z, fma(y, y, x * x))) (torch's reduction fuses each `acc + v * v`; the fp32 products are exact in float64,
    so the fused sum is stated there and rounded), unit = v / max(norm, 1e-12), theta = the float64 acos(unit_y) rounded once (the
    reference's vector acos is within one fp32 step of it), phi = libm_atan2f(unit_x, unit_z), plus fp32 2 pi where negative."""
    v = np.stack([np.asarray(a, f32).reshape(-1), np.abs(np.asarray(b, f32).reshape(-1)), np.asarray(c, f32).reshape(-1)], -1)
    d = v.astype(np.float64)
    s = (v[:, 0] * v[:, 0]).astype(f32)
    s = (d[:, 1] * d[:, 1] + s.astype(np.float64)).astype(f32)
    s = (d[:, 2] * d[:, 2] + s.astype(np.float64)).astype(f32)
    u = v / np.maximum(np.sqrt(s), f32(1e-12))[:, None]
    th = np.arccos(u[:, 1].astype(np.float64)).astype(f32)
    ph = np.array([libm_atan2f(y, x) for y, x in zip(u[:, 0], u[:, 2])], f32).reshape(-1)
    ph = np.where(ph < 0, ph + f32(2 * np.pi), ph).astype(f32)
    return torch.from_numpy(th), torch.from_numpy(ph)


def virtual_view(inp, cfg, mode, a, b, c, t, ds_is_train=True, scale=None):
    """-> dict(H, W, K, pose64 [B,4,4] float64, dir, deg [B,2], polar, azimuth, radius, th, ph (the fp32 radians), rays_t, rays_id)"""
    d = cfg["data"]
    t = torch.as_tensor(t).long().reshape(-1)
    nF = inp["rgb"].shape[0]
    Hh, Ww = inp["rgb"].shape[1:3]
    a, b = torch.as_tensor(a).to(F32).reshape(-1), torch.as_tensor(b).to(F32).reshape(-1)
    pi_f, twopi_f = torch.tensor(np.pi, dtype=F64).to(F32), torch.tensor(2 * np.pi, dtype=F64).to(F32)
    r_tab, th_tab, ph_tab = (torch.as_tensor(inp[k]).to(F32) for k in ("radius", "theta", "phi"))
    if mode == POLAR:
        front, overhead = d["angle_front"] / 180 * np.pi, d["angle_overhead"] / 180 * np.pi
        rad = r_tab[t]
        th_deg, ph_deg = a, b
        th, ph = a / 180 * pi_f, b / 180 * pi_f
    else:
        front, overhead = float(np.deg2rad(d["angle_front"])), float(np.deg2rad(d["angle_overhead"]))
        rad = r_tab[t] * torch.tensor(float(d["novel_view_scale_factor"]), dtype=F64).to(F32)
    if mode == SPHERE:
        v = torch.stack([a.double(), torch.as_tensor(b).double().abs(), torch.as_tensor(c).to(F32).reshape(-1).double()], -1)
        u = v / torch.clamp(v.square().sum(-1, keepdim=True).sqrt(), min=1e-12)
        th, ph = sphere_angles(a, b, c)
        centres = rad.double()[:, None] * u
    else:
        if mode == ANGLES:
            th, ph = a, torch.where(b < 0, b + twopi_f, b)
        t64, p64 = th.double(), ph.double()
        centres = torch.stack([rad.double() * torch.sin(t64) * torch.sin(p64), rad.double() * torch.cos(t64),
                               rad.double() * torch.sin(t64) * torch.cos(p64)], -1)
    if mode != POLAR:
        th_deg, ph_deg = th / pi_f * 180, ph / pi_f * 180
    pose64 = torch.from_numpy(look_at_np(centres.numpy()))
    az = ph_deg - ph_tab[t]
    az = torch.where(az > 180, az - 360, az)
    if scale is not None:
        Ho, Wo, K = int(scale * Hh), int(scale * Ww), scaled_K(inp["K"], scale)
    elif ds_is_train:
        s = d["novel_view_scale"]
        Ho, Wo, K = int(s * Hh), int(s * Ww), scaled_K(inp["K"], s)
    else:
        Ho, Wo, K = Hh, Ww, scaled_K(inp["K"], None)
    N = Ho * Wo
    return {"H": Ho, "W": Wo, "K": K, "pose64": pose64, "dir": view_label(th, ph, front, overhead),
            "deg": torch.stack([th_deg, ph_deg], -1), "polar": th_deg - th_tab[t], "azimuth": az, "radius": rad - r_tab[t],
            "th": th, "ph": ph, "rays_t": (t.to(F32) / torch.tensor(float(nF), dtype=F32))[:, None, None].repeat(1, N, 1),
            "rays_id": t[:, None, None].repeat(1, N, 1)}
