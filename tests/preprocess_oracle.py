"""Restatement of the reference's preprocessing stage (preprocess/preprocess.py:Database, DataProcessor and
preprocess/pose_init/create_camera.py) -- test infrastructure, numpy float64 and torch fp32 on the CPU.

What morpheus_amd.preprocess / csrc/preprocess.hip must reproduce, stated once:
  * the virtual cameras (`polar_from_c2w`, `c2w_from_polar`, `virtual_views`): the reference's chains of torch fp32 operators, frame
    by frame where it goes frame by frame (a 0-dim acos is another program than a vectorised one), bit for bit;
  * the crop centres (`crop_centres`): OpenGL -> OpenCV, the fp32 inverse, the float64 projection of the world centre, int() towards
    zero; the window origin `top, left = py - size_h // 2 + 1, px - size_w // 2 + 1`;
  * the frames (`prep_frames`).  Output pixel (y, x) of frame f looks at canvas pixel (Y, X) = (top + y, left + x); outside
    [0,H) x [0,W) rgb, depth and mask are 0 and padding is 255, inside padding is 0 -- for every window, also the three kinds the
    reference raises on (`window_kind`: "two_sides", "outside", "larger").  depth = table_inside[raw] when the frame's window
    passes `top >= 0 and left >= 0 and top + h < H and left + w < W`, else table_padded[raw] (`depth_tables`: the reference's fp32
    and float64 write products).  Unrotated frames copy rgb and mask bytes.  Rotated frames, this build's own definition
    (agreement with cv2 unverified): M = [[c, s, (1 - c) cx - s cy], [-s, c, s cx + (1 - c) cy]] (`rotation_matrix`), its inverse
    (`invert_affine`), then in float64, each operator rounded on its own and in THIS order:
        u = (a0 X + a1 Y) + a2            v = (a3 X + a4 Y) + a5
        nearest (depth, mask): column floor(u + 0.5), row floor(v + 0.5), 0 outside the image
        bilinear (rgb): fu = floor(u), fv = floor(v), ax = u - fu, ay = v - fv, taps byte / 255.0 (0 outside the image)
            val = ((p00 ((1 - ax)(1 - ay)) + p01 (ax (1 - ay))) + p10 ((1 - ax) ay)) + p11 (ax ay);  byte = (val * 255.).astype(uint8)
  * the cameras of the pose initialisation (`cameras_from_pose_init`): world_mat = fp32(intrinsic4x4 fp32 @ w2c), scale_mat =
    fp32(diag(r, r, r, 1)), r scaled by the largest reference-point norm times object_scale when reference points are given.
The golden's inputs (`make_inputs`, `make_polar_poses`, `make_camera_inputs`) are defined here so that tools/make_preprocess_golden.py
and the tests share them.
"""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preprocess.npz")
F, H, W = 10, 12, 16
DEPTH_SCALE = 1000.0
RUNS = (("s8_", 8, 8, 1.0), ("s7_", 7, 7, 1.25))      # tag, size_h, size_w, radius of the scale matrix (depth scale = 1 / radius)
# where the world centre projects to, (x, y) in pixels: half a pixel inside the truncated value, the negative ones too, so
# that int() towards zero and floor() differ there
TARGETS = ((8.5, 5.5), (8.5, 7.5), (11.5, 5.5), (8.5, 1.5), (1.5, 5.5), (-1.5, -0.5), (8.5, 9.5), (14.5, 5.5), (14.5, 9.5), (11.5, 1.5))
KINDS = ("inside", "touch_bottom", "touch_right", "top_neg", "left_neg", "both_neg", "beyond_bottom", "beyond_right", "beyond_both",
         "top_neg_touch_right")
EXCLUDED = {"two_sides": (1, 14, 8, 8), "outside": (5, 14 + 8, 8, 8), "larger": (5, 8, 14, 18)}      # py, px, size_h, size_w
ANGLES = (0.0, 90.0, 180.0, 37.5, -10.0)


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------------------------ windows
def window_origins(centres, size_h, size_w):
    """(px, py) int [n,2] -> (top, left) int64 [n,2]"""
    c = np.asarray(centres, dtype=np.int64).reshape(-1, 2)
    return np.stack([c[:, 1] - size_h // 2 + 1, c[:, 0] - size_w // 2 + 1], -1)


def is_inside(top, left, h, w, Hh, Ww):
    return bool(top >= 0 and left >= 0 and top + h < Hh and left + w < Ww)


def window_kind(top, left, h, w, Hh, Ww):
    """which of the reference's branches a window takes; "two_sides", "outside" and "larger" are the kinds it raises on"""
    if h > Hh or w > Ww:
        return "larger"
    if top >= Hh or left >= Ww or top + h <= 0 or left + w <= 0:
        return "outside"
    if is_inside(top, left, h, w, Hh, Ww):
        return "inside"
    lo_t, lo_l, hi_b, hi_r = top < 0, left < 0, top + h > Hh, left + w > Ww
    if (lo_t and hi_r) or (lo_l and hi_b):
        return "two_sides"
    if lo_t or lo_l:
        name = "both_neg" if lo_t and lo_l else ("top_neg" if lo_t else "left_neg")
        if lo_t and not lo_l and left + w == Ww:
            name += "_touch_right"
        if lo_l and not lo_t and top + h == Hh:
            name += "_touch_bottom"
        return name
    if hi_b or hi_r:
        return "beyond_both" if hi_b and hi_r else ("beyond_bottom" if hi_b else "beyond_right")
    if top + h == Hh and left + w == Ww:
        return "touch_both"
    return "touch_bottom" if top + h == Hh else "touch_right"


# ------------------------------------------------------------------------------------------------------------------- inputs
def make_inputs():
    """The golden's sequence: F = 10 frames of 12 x 16.  rgb with 0 and 255, masks of 0 / 128 / 254 / 255, translation-only
    cameras (OpenGL, aligned) whose world centre projects to TARGETS, and a depth in which both write products change values:
    with depth_scale 1000 and scale 1 the fp32 product moves 739 of the 65536 raw values and the float64 product 32501; every
    frame carries raw values of each set."""
    rng = np.random.default_rng(20250117)
    rgb = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    rgb[0, 0, 0], rgb[F - 1, H - 1, W - 1] = (0, 255, 1), (255, 0, 254)
    mask = rng.choice(np.array([0, 128, 254, 255], dtype=np.uint8), (F, H, W))
    depth = rng.integers(300, 4000, (F, H, W)).astype(np.uint16)
    tin, tpad = depth_tables(DEPTH_SCALE, 1.0)
    raw = np.arange(65536)
    moved32 = raw[(tin != raw) & (raw > 300) & (raw < 60000)]
    moved64 = raw[(tpad != raw) & (tin == raw) & (raw > 300) & (raw < 60000)]
    for f in range(F):
        where = rng.permutation(H * W)[:64]
        vals = np.concatenate([rng.choice(moved32, 32), rng.choice(moved64, 32)])
        depth[f].reshape(-1)[where] = vals.astype(np.uint16)
    depth[1, 2, 3], depth[2, 5, 8], depth[3, 6, 9] = 0, 65535, 1
    K = np.eye(4)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 9.3, 9.7, 7.6, 5.4
    poses = np.zeros((F, 4, 4))
    for f, (tx, ty) in enumerate(TARGETS):
        Z = 2.0 + 0.1 * f
        X, Y = (tx - K[0, 2]) * Z / K[0, 0], (ty - K[1, 2]) * Z / K[1, 1]
        poses[f] = np.array([[1.0, 0, 0, -X], [0, -1.0, 0, -Y], [0, 0, -1.0, -Z], [0, 0, 0, 1.0]])
    return dict(rgb=rgb, depth=depth, mask=mask, poses=poses.astype(np.float32), K=np.tile(K, (F, 1, 1)))


def make_polar_poses():
    """8 generic camera-to-world matrices (look-at with a roll, fp32) for the polar chains; half of them with the camera's z axis
    pointing to negative x, where atan2 is negative and 2 pi is added"""
    rng = np.random.default_rng(77)
    r, th, ph = rng.uniform(1.5, 2.5, 8), np.deg2rad(rng.uniform(40.0, 110.0, 8)), np.deg2rad(np.linspace(-170.0, 170.0, 8))
    c = np.stack([r * np.sin(th) * np.sin(ph), r * np.cos(th), r * np.sin(th) * np.cos(ph)], -1)

    def unit(x):
        return x / np.linalg.norm(x, axis=-1, keepdims=True)
    fwd = unit(c + rng.normal(0, 0.05, c.shape))            # not exactly through the origin: r differs between the two forms
    right = unit(np.cross(np.broadcast_to(np.array([0.0, 1.0, 0.0]), fwd.shape), fwd))
    up = np.cross(fwd, right)
    P = np.tile(np.eye(4), (8, 1, 1))
    for k in range(8):
        a = 0.1 + 0.2 * k
        roll = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        P[k, :3, :3] = np.stack([right[k], up[k], fwd[k]], -1) @ roll
    P[:, :3, 3] = c
    return P.astype(np.float32)


def make_camera_inputs():
    """inputs of the camera step: intrinsics.txt's matrix, 6 world-to-camera transformations, a radius and reference points"""
    rng = np.random.default_rng(5)
    K = np.array([[517.3, 0.0, 318.6], [0.0, 516.5, 255.3], [0.0, 0.0, 1.0]])
    T = np.tile(np.eye(4), (6, 1, 1))
    for k in range(6):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        T[k, :3, :3] = q * np.sign(np.linalg.det(q))
        T[k, :3, 3] = rng.normal(0, 0.4, 3) + (0, 0, 1.5)
    return dict(K=K, transformations=T, radius=0.4371, ref_points=rng.normal(0, 0.6, (50, 3)))


# ------------------------------------------------------------------------------------------------------------------ cameras
def cameras_from_pose_init(transformations, radius, K, ref_points=None, object_scale=1.05):
    K = np.asarray(K, dtype=np.float64)
    intrinsic = np.diag([K[0, 0], K[1, 1], 1.0, 1.0]).astype(np.float32)
    intrinsic[0, 2], intrinsic[1, 2] = K[0, 2], K[1, 2]
    radius = np.float64(radius)
    if ref_points is not None:
        radius = radius * (np.linalg.norm(np.asarray(ref_points), ord=2, axis=-1).max() * object_scale)
    T = np.asarray(transformations).reshape(-1, 4, 4)
    cams = {}
    for i in range(len(T)):
        cams[f"world_mat_{i}"] = (intrinsic @ T[i]).astype(np.float32)
    for i in range(len(T)):
        cams[f"scale_mat_{i}"] = np.diag([radius, radius, radius, 1.0]).astype(np.float32)
    return cams


def polar_from_c2w(poses, virtual):
    """fp32 [n,4,4] -> radius, theta, phi fp32 [n] (degrees), 0-dim torch operators frame by frame"""
    rs, ths, phs = [], [], []
    for c2w in torch.as_tensor(poses):
        centre, z = c2w[:3, 3], c2w[:3, 2]
        if virtual:
            r = (centre * z).sum()
            axis = z
        else:
            r = torch.sqrt(torch.sum(centre ** 2))
            axis = centre / r
        theta, phi = torch.acos(axis[1]), torch.atan2(axis[0], axis[2])
        if phi < 0.0:
            phi = phi + 2 * np.pi
        rs.append(r * 1.0)
        ths.append(theta * 180.0 / np.pi)
        phs.append(phi * 180.0 / np.pi)
    return torch.tensor(rs), torch.tensor(ths), torch.tensor(phs)


def c2w_from_polar(radius, theta, phi, x_axis):
    """fp32 [n] (degrees), x_axis fp32 [n,3] -> fp32 [n,4,4]: OpenGL, the camera looks away from the origin's side, its x axis
    is handed in and up = normalize(forward x right)"""
    def unit(x):
        return x / torch.sqrt(torch.clamp(torch.sum(x * x, -1, keepdim=True), min=1e-20))
    theta, phi = theta / 180 * np.pi, phi / 180 * np.pi
    c = torch.stack([radius * torch.sin(theta) * torch.sin(phi), radius * torch.cos(theta), radius * torch.sin(theta) * torch.cos(phi)], -1)
    fwd = unit(c - 0)
    up = unit(torch.cross(fwd, x_axis, dim=-1))
    P = torch.eye(4, dtype=torch.float32).unsqueeze(0).repeat(len(c), 1, 1)
    P[:, :3, :3] = torch.stack((x_axis, up, fwd), -1)
    P[:, :3, 3] = c
    return P


def virtual_views(poses, intrinsics, size_h, size_w):
    poses = torch.as_tensor(poses)
    r, th, ph = polar_from_c2w(poses, True)
    rr, rth, rph = polar_from_c2w(poses, False)
    x_axis = torch.stack([p[:3, 0] for p in poses], 0)
    K = np.asarray(intrinsics, dtype=np.float64)
    K_virt = np.array([[K[0, 0, 0], 0.0, size_w / 2], [0.0, K[0, 1, 1], size_h / 2], [0.0, 0.0, 1.0]])
    return dict(radius=r, theta=th, phi=ph, raw_radius=rr, raw_theta=rth, raw_phi=rph, poses_virt=c2w_from_polar(r, th, ph, x_axis),
                K_virt=K_virt)


def crop_centres(poses, intrinsics):
    """-> int64 [n,2], (px, py) of the world centre in every frame"""
    out = []
    for c2w, K in zip(np.asarray(poses, dtype=np.float32), np.asarray(intrinsics, dtype=np.float64)):
        c2w = c2w.copy()
        c2w[:, 1] *= -1
        c2w[:, 2] *= -1
        w2c = np.linalg.inv(c2w)                               # fp32
        x_c = w2c[:3, :3] @ np.zeros((3,)) + w2c[:3, -1]       # float64
        p = K[:3, :3] @ x_c
        out.append((int(p[0] / p[2]), int(p[1] / p[2])))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------------------------- frames
def depth_tables(depth_scale, scale):
    """(table_inside, table_padded) uint16 [65536]: what the reference writes for each raw value through its fp32 and its float64
    product; a value that does not fit 16 bits saturates (this build's rule)"""
    raw = np.arange(65536).astype(np.uint16)
    d = (raw / depth_scale).astype(np.float32)
    d *= np.array([scale], dtype=np.float32)
    inside = d * 1000
    padded = d.astype(np.float64) * 1000
    assert inside.dtype == np.float32 and padded.dtype == np.float64
    return tuple(np.clip(v, 0, 65535).astype(np.uint16) for v in (inside, padded))


def rotation_matrix(centre, deg):
    c, s = math.cos(deg * math.pi / 180.0), math.sin(deg * math.pi / 180.0)
    cx, cy = float(centre[0]), float(centre[1])
    return np.array([[c, s, (1 - c) * cx - s * cy], [-s, c, s * cx + (1 - c) * cy]], dtype=np.float64)


def invert_affine(M):
    """the six numbers (a0 .. a5) of the inverse of the 2 x 3 map M"""
    M = np.asarray(M, dtype=np.float64)
    det = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    i00, i01, i10, i11 = M[1, 1] / det, -M[0, 1] / det, -M[1, 0] / det, M[0, 0] / det
    return np.array([i00, i01, -(i00 * M[0, 2] + i01 * M[1, 2]), i10, i11, -(i10 * M[0, 2] + i11 * M[1, 2])], dtype=np.float64)


def _taps(img, iy, ix):
    """img [H,W,...] at integer (iy, ix) arrays, 0 outside"""
    Hh, Ww = img.shape[:2]
    ok = (iy >= 0) & (iy < Hh) & (ix >= 0) & (ix < Ww)
    v = img[np.clip(iy, 0, Hh - 1), np.clip(ix, 0, Ww - 1)]
    return np.where(ok.reshape(ok.shape + (1,) * (v.ndim - ok.ndim)), v, 0)


def prep_frames(rgb, depth, mask, origin, inv_affine, rotated, table_inside, table_padded, h, w):
    Fn, Hh, Ww = depth.shape
    out = dict(rgb=np.zeros((Fn, h, w, 3), np.uint8), depth=np.zeros((Fn, h, w), np.uint16), mask=np.zeros((Fn, h, w), np.uint8),
               padding=np.zeros((Fn, h, w), np.uint8))
    for f in range(Fn):
        top, left = int(origin[f][0]), int(origin[f][1])
        Y = np.broadcast_to(top + np.arange(h, dtype=np.int64)[:, None], (h, w))
        X = np.broadcast_to(left + np.arange(w, dtype=np.int64)[None, :], (h, w))
        on = (Y >= 0) & (Y < Hh) & (X >= 0) & (X < Ww)
        table = table_inside if is_inside(top, left, h, w, Hh, Ww) else table_padded
        if not rotated[f]:
            c, raw, m = _taps(rgb[f], Y, X), _taps(depth[f], Y, X), _taps(mask[f], Y, X)
        else:
            a = np.asarray(inv_affine[f], dtype=np.float64)
            Xd, Yd = X.astype(np.float64), Y.astype(np.float64)
            u = (a[0] * Xd + a[1] * Yd) + a[2]
            v = (a[3] * Xd + a[4] * Yd) + a[5]
            lim = 2.0 ** 40                      # integer conversion stays defined; such taps are far outside either way
            un, vn = np.floor(u + 0.5).clip(-lim, lim).astype(np.int64), np.floor(v + 0.5).clip(-lim, lim).astype(np.int64)
            raw, m = _taps(depth[f], vn, un), _taps(mask[f], vn, un)
            fu, fv = np.floor(u), np.floor(v)
            ax, ay = (u - fu)[..., None], (v - fv)[..., None]
            iu, iv = fu.clip(-lim, lim).astype(np.int64), fv.clip(-lim, lim).astype(np.int64)
            img = rgb[f].astype(np.float64) / 255.0
            p00, p01, p10, p11 = _taps(img, iv, iu), _taps(img, iv, iu + 1), _taps(img, iv + 1, iu), _taps(img, iv + 1, iu + 1)
            val = ((p00 * ((1.0 - ax) * (1.0 - ay)) + p01 * (ax * (1.0 - ay))) + p10 * ((1.0 - ax) * ay)) + p11 * (ax * ay)
            c = (val * 255.).astype(np.uint8)
        out["rgb"][f] = np.where(on[..., None], c, 0)
        out["depth"][f] = np.where(on, table[raw], 0)
        out["mask"][f] = np.where(on, m, 0)
        out["padding"][f] = np.where(on, 0, 255)
    return out
