"""Numpy restatement of the pose-initialisation conventions of include/morpheus_hip.h (mh_depth_points_*, mh_knn_d2, mh_icp_wsums)
and of morpheus_amd.poseinit's definitions (knn_median, robust_icp, init_poses), written from the header text and the docstrings.
float64 where they say float64, fp32 arrays and numpy's fp32 operators where they say fp32.  Nearest neighbours are
tests/mesheval_oracle.nearest and moved points are rounded once to fp32 (mesheval_oracle.transform_points), so correspondences are
comparable bit for bit with the device's.  Slow and plain on purpose.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from tests import mesheval_oracle as mo

F = np.float32
NU_END_K = 1.0 / (3.0 * math.sqrt(3.0))


# ---- masked back-projection ----------------------------------------------------------------------------------------------

def depth_points(depth, mask, K):
    """-> (points fp32 [n,3], pixel int32 [n]) in row-major pixel order."""
    depth = np.asarray(depth, F)
    K = np.asarray(K, np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    H, W = depth.shape
    with np.errstate(invalid="ignore"):
        keep = (np.asarray(mask) != 0) & (depth > 0)               # a NaN depth fails
    v, u = np.nonzero(keep)
    d = depth[v, u].astype(np.float64)
    x = (d * (u.astype(np.float64) - cx)) / fx
    y = (d * (v.astype(np.float64) - cy)) / fy
    return np.stack([x.astype(F), y.astype(F), depth[v, u]], axis=1).reshape(-1, 3), (v * W + u).astype(np.int32)


# ---- k nearest distances -------------------------------------------------------------------------------------------------

def knn_d2(points, k, chunk=256):
    """-> fp32 [N,k]: the k smallest admissible d2 to the other points (by index), ascending, +inf where none is left."""
    p = np.ascontiguousarray(points, F)
    N = p.shape[0]
    out = np.full((N, k), np.inf, F)
    for a in range(0, N, chunk):
        d2 = mo.pair_d2(p[a:a + chunk], p)
        with np.errstate(invalid="ignore"):
            d2 = np.where(d2 < F(np.inf), d2, F(np.inf))           # NaN and overflow never enter
        rows = np.arange(d2.shape[0])
        d2[rows, a + rows] = F(np.inf)                             # the point itself, by index
        s = np.sort(d2, axis=1)[:, :k]
        out[a:a + chunk, :s.shape[1]] = s
    return out


def knn_median(points, k=7):
    d2 = knn_d2(points, k - 1)
    if d2.shape[0] == 0:
        return math.nan
    with np.errstate(invalid="ignore"):
        return float(np.median(np.median(np.sqrt(d2.astype(np.float64)), axis=1)))


# ---- Welsch-weighted sums ------------------------------------------------------------------------------------------------

def icp_wterms(moved, target, idx, d2, inv_2nu2):
    """The [n_corr, 19] float64 terms whose column sums are the 19 numbers."""
    idx = np.asarray(idx)
    sel = (idx >= 0) & (idx < np.asarray(target).shape[0])
    p = np.asarray(moved, F)[sel].astype(np.float64)
    q = np.asarray(target, F)[idx[sel]].astype(np.float64)
    dd = np.asarray(d2, F)[sel].astype(np.float64)
    w = np.exp(-dd * inv_2nu2)
    wp = w[:, None] * p
    pq = (wp[:, :, None] * q[:, None, :]).reshape(-1, 9)
    return np.concatenate([w[:, None], (w * dd)[:, None], wp, w[:, None] * q, pq, (1.0 - w)[:, None], np.ones((p.shape[0], 1))],
                          axis=1)


def icp_wsums(moved, target, idx, d2, inv_2nu2, reverse=False):
    t = icp_wterms(moved, target, idx, d2, inv_2nu2)
    return (t[::-1] if reverse else t).sum(axis=0)


# ---- robust rigid registration -------------------------------------------------------------------------------------------

def _diagonal(p):
    p = np.asarray(p, F).astype(np.float64)
    return float(np.linalg.norm(p.max(0) - p.min(0)))


def robust_icp(source, target, init=None, nu_begin_k=3.0, nu_end_k=NU_END_K, nu_alpha=0.5, knn=7, max_icp=100, stop=1e-5,
               weighted=True, reverse=False, trace=None):
    """morpheus_amd.poseinit.robust_icp's definition.  weighted=False: the same loop with every weight 1 (one stage: plain
    point-to-point ICP with the same stopping rule).  reverse: the sums are taken in reversed point order.  trace: a list that
    receives every iteration's correspondence indices."""
    source, target = np.ascontiguousarray(source, F), np.ascontiguousarray(target, F)
    T = np.eye(4) if init is None else np.array(init, np.float64)
    out = {"transformation": T, "iterations": 0, "stages": 0, "nu": math.nan, "energy": math.nan, "weight_sum": 0.0,
           "converged": False}
    if source.shape[0] == 0 or target.shape[0] == 0:
        out["transformation"] = np.eye(4)
        return out
    scale = max(_diagonal(source), _diagonal(target))
    nu_end = nu_end_k * knn_median(target, knn)

    def correspond():
        moved = mo.transform_points(source, T)
        idx, d2 = mo.nearest(moved, target)
        if trace is not None:
            trace.append(idx.copy())
        return moved, idx, d2

    def inv(nu):
        return 1.0 / (2.0 * nu * nu) if weighted else 0.0

    moved, idx, d2 = correspond()
    first = np.sqrt(d2[idx >= 0].astype(np.float64))
    nu = max(nu_begin_k * float(np.median(first)), nu_end) if first.size else math.nan
    out["nu"] = nu
    if not (0.0 < nu < math.inf and 0.0 < nu_end and 0.0 < scale < math.inf):
        return out
    if not weighted:
        nu = nu_end
    iterations = stages = 0
    while True:
        stages += 1
        converged = False
        for _ in range(int(max_icp)):
            s = icp_wsums(moved, target, idx, d2, inv(nu), reverse)
            if not (0.0 < s[0] < math.inf) or s[18] < 3:
                out.update(transformation=T, iterations=iterations, stages=stages, nu=nu)
                return out
            T_new = mo.kabsch_update(s[:17]) @ T
            iterations += 1
            delta = T_new - T
            delta[:3, 3] /= scale
            T = T_new
            moved, idx, d2 = correspond()
            if np.linalg.norm(delta) < stop:
                converged = True
                break
        if nu == nu_end:
            break
        nu = max(nu * nu_alpha, nu_end)
    s = icp_wsums(moved, target, idx, d2, inv(nu), reverse)
    return {"transformation": T, "iterations": iterations, "stages": stages, "nu": nu, "energy": float(s[17]),
            "weight_sum": float(s[0]), "converged": converged}


# ---- registrate.py's main loop -------------------------------------------------------------------------------------------

def mask_rule(mask_png):
    m = np.array(mask_png, dtype=int) / 255
    if m.ndim == 3:
        m = np.sum(m[..., :3], 2) / 3.
    return (m > 0.5).astype(np.uint8)


def depth_rule(raw, depth_scale=1000.0):
    return np.array(raw, dtype=int).astype(F) / F(depth_scale)


def init_poses(depths, masks, K, depth_scale=1000.0, rigid_registrate=1, register=None):
    """-> dict(transformations float64 [N,4,4], radius, points: the fp32 clouds).  register(source, target) -> [4,4] gets the
    centred fp32 clouds."""
    if register is None:
        register = lambda s, t: robust_icp(s, t)["transformation"]                # noqa: E731
    total = len(depths)
    Ts = np.repeat(np.eye(4)[None], total, axis=0)
    norms, clouds = [], []
    first = previous = None
    for i in range(total):
        xyz = depth_points(depth_rule(depths[i], depth_scale), mask_rule(masks[i]), K)[0]
        clouds.append(xyz)
        xyz64 = xyz.astype(np.float64)
        mean = xyz64.mean(0)
        world = xyz64 - mean
        coarse = np.eye(4)
        coarse[:3, 3] = mean
        if rigid_registrate != 2 or i == 0:
            Ts[i] = coarse
        if rigid_registrate:
            cloud = world.astype(F)                                # x - mean in float64, rounded once
            if i == 0:
                first = cloud
            else:
                fine = np.asarray(register(first if rigid_registrate == 1 else previous, cloud), np.float64)
                if rigid_registrate == 1:
                    Ts[i] = coarse @ fine
                    rot, trans = fine[:3, :3], fine[:3, 3]
                else:
                    Ts[i:] = fine[None] @ Ts[i:]
                    Ts[i] = coarse @ Ts[i]
                    rot, trans = Ts[i, :3, :3], Ts[i, :3, 3]
                world = (world - trans[None]) @ rot
            previous = cloud
        norms.append(np.linalg.norm(world, axis=1))
    whole = np.concatenate(norms)
    radius = float(whole[whole <= np.percentile(whole, 95)].max() * 1.2)
    return {"transformations": Ts, "radius": radius, "points": clouds}


# ---- cases for the tests -------------------------------------------------------------------------------------------------

ROBUST_SEED = 3                                   # tests/test_poseinit_host.py checks that summation order cannot decide this case


def bumpy_surface(n, rng):
    """n fp32 points on an asymmetric closed surface: an ellipsoid (0.5, 0.35, 0.25) whose radius is modulated by three lobes of
    different size, so that no rotation maps it onto itself."""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = 1.0 + 0.25 * np.exp(-8.0 * (1.0 - d @ np.array([0.6, 0.0, 0.8]))) + 0.18 * np.exp(-10.0 * (1.0 - d @ np.array([-0.7, 0.6, -0.39]))) \
        - 0.15 * np.exp(-6.0 * (1.0 - d @ np.array([0.0, -1.0, 0.0])))
    return (d * r[:, None] * np.array([0.5, 0.35, 0.25])).astype(F)


def robust_case(seed=ROBUST_SEED, degrees=15.0, n=1500):
    """-> (source fp32 [n,3], target fp32, T_true [4,4]): the target is the part of the source on one side (what a camera looking
    down -z sees of it), moved by T_true -- `degrees` about a skew axis plus a shift -- with uniform outliers numbering one third
    of its points, shuffled in."""
    rng = np.random.default_rng(seed)
    source = bumpy_surface(n, rng)
    axis = np.array([0.3, 0.8, 0.52])
    axis /= np.linalg.norm(axis)
    a = math.radians(degrees)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(a) * Kx + (1 - math.cos(a)) * (Kx @ Kx)
    T[:3, 3] = (0.05, -0.03, 0.04)
    side = source[source[:, 2] > -0.05]
    moved = mo.transform_points(side, T)
    lo, hi = moved.min(0), moved.max(0)
    outliers = rng.uniform(lo - 0.1, hi + 0.1, size=(moved.shape[0] // 3, 3)).astype(F)
    target = np.concatenate([moved, outliers])
    return source, np.ascontiguousarray(target[rng.permutation(target.shape[0])]), T


def pose_error(T, T_true):
    """-> (rotation error in degrees, translation error)"""
    R = T[:3, :3] @ T_true[:3, :3].T
    return math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0)))), float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))


@functools.lru_cache(maxsize=None)
def robust_reference(seed=ROBUST_SEED):
    """The oracle's run on robust_case(seed), computed once per process and shared (treat as read-only)."""
    source, target, _ = robust_case(seed)
    trace = []
    res = robust_icp(source, target, trace=trace)
    res["trace"] = trace
    return res


def ellipsoid_frames(n_frames=4, H=48, W=64):
    """Analytic depth frames of a moved ellipsoid with bumps: -> (raw uint16 depths [n,H,W] in millimetres, masks uint8 [n,H,W]
    of 0 / 255, K [3,3]).  Frame i sees the body rotated by 4 i degrees about a skew axis and shifted; depth is found per pixel by
    bisection along the ray of the implicit function."""
    K = np.array([[70.0, 0.0, 31.5], [0.0, 70.0, 23.5], [0.0, 0.0, 1.0]])
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    rays = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], axis=-1)      # z = 1
    lobes = [(np.array([0.6, 0.0, -0.8]), 0.25, 8.0), (np.array([-0.7, 0.6, -0.39]), 0.18, 10.0), (np.array([0.0, -0.8, -0.6]), -0.15, 6.0)]
    semi = np.array([0.24, 0.17, 0.12])

    def inside(p):                                                  # p in the body's frame: f < 0 inside
        q = p / semi
        r = np.linalg.norm(q, axis=-1)
        d = q / np.maximum(r, 1e-12)[..., None]
        rad = 1.0 + sum(a * np.exp(-s * (1.0 - d @ n)) for n, a, s in lobes)
        return r < rad

    depths, masks = [], []
    for i in range(n_frames):
        M = mo.rigid(math.radians(1.5 * i), math.radians(4.0 * i), math.radians(-2.0 * i), (0.01 * i, -0.008 * i, 1.0 + 0.01 * i))
        Rinv, t = M[:3, :3].T, M[:3, 3]
        zs = np.linspace(0.5, 1.5, 201)
        hit = np.zeros((H, W), bool)
        z_lo, z_hi = np.full((H, W), 0.5), np.full((H, W), 0.5)
        for a, b in zip(zs[:-1], zs[1:]):                          # the first sign change along every ray
            ins = inside((rays * b - t) @ Rinv.T)
            new = ins & ~hit
            z_lo[new], z_hi[new] = a, b
            hit |= ins
        for _ in range(30):
            mid = 0.5 * (z_lo + z_hi)
            ins = inside((rays * mid[..., None] - t) @ Rinv.T)
            z_hi = np.where(ins, mid, z_hi)
            z_lo = np.where(ins, z_lo, mid)
        depths.append(np.where(hit, np.rint(z_hi * 1000.0), 0).astype(np.uint16))
        masks.append(np.where(hit, 255, 0).astype(np.uint8))
    return np.stack(depths), np.stack(masks), K


@functools.lru_cache(maxsize=None)
def ellipsoid_reference(reverse=False):
    """The oracle's init_poses, mode 1 with robust_icp, on ellipsoid_frames(): computed once per process and shared (treat as
    read-only).  -> init_poses' dict plus `runs` (robust_icp's dicts, each with its trace)."""
    depths, masks, K = ellipsoid_frames()
    runs = []

    def register(source, target):
        trace = []
        runs.append(dict(robust_icp(source, target, reverse=reverse, trace=trace), trace=trace))
        return runs[-1]["transformation"]

    out = init_poses(list(depths), list(masks), K, 1000.0, 1, register)
    out["runs"] = runs
    return out
