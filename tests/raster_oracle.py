"""numpy restatement of the rasteriser of csrc/raster.hip, written from the text of include/morpheus_hip.h (mesh rendering).

Not a test module.  Three things live here:
  * rasterize / resolve / vertex_normal_sums: the header's definitions operator by operator -- int64 coverage on the snapped
    coordinates, fp32 depth in the header's order, int64 fixed-point normal sums.  tests/test_gpu_raster.py holds the kernels
    to depth, tri_id and the sums bit for bit.  resolve(dtype=np.float64) is the same formulas in float64 (depth from the
    plane, not from the key): the yardstick of the float outputs;
  * ray_cast: a float64 Moeller-Trumbore ray caster over all pixels x triangles that shares nothing with the rasteriser (no
    snapping, no edge functions): the independent yardstick of tests/test_raster_host.py;
  * test meshes and cameras.
"""
from __future__ import annotations

import numpy as np

F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
SNAP_LIMIT = F(8388608.0)


def world_to_camera(c2w, convention="opengl"):
    """host side of the contract: float64 inverse of the OpenCV camera-to-world, rounded once to fp32 [3,4]"""
    m = np.eye(4)
    m[:3] = np.asarray(c2w, np.float64)[:3]
    if convention == "opengl":
        m[:3, 1:3] *= -1
    return np.ascontiguousarray(np.linalg.inv(m)[:3].astype(F))


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross_of(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _cross(a, b, c):
    return _cross_of(b - a, c - a)


def to_camera(w2c, pts, dtype=F):
    w = np.asarray(w2c, F).astype(dtype)
    p = np.asarray(pts, F).astype(dtype)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((w[r, 0] * x + w[r, 1] * y) + w[r, 2] * z) + w[r, 3] for r in range(3)], 1)


def _valid_triangles(triangles, V):
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    return t, ((t >= 0) & (t < V)).all(1)


def pixel_dirs(fx, fy, cx, cy, ii, jj, dtype=F):
    dx = ((ii.astype(dtype) + dtype(0.5)) - dtype(cx)) / dtype(fx)
    dy = ((jj.astype(dtype) + dtype(0.5)) - dtype(cy)) / dtype(fy)
    return dx, dy


def snap(vertices, triangles, w2c, fx, fy, cx, cy, near):
    """vertex stage -> (cam [V,3] fp32, XY int64 [V,2], status per triangle: 0 draw candidate, 1 counted, 2 skipped)"""
    V = len(vertices)
    tri, ok = _valid_triangles(triangles, V)
    cam = to_camera(w2c, vertices)
    fx, fy, cx, cy, near = F(fx), F(fy), F(cx), F(cy), F(near)
    with np.errstate(all="ignore"):
        sx = (fx * cam[:, 0]) / cam[:, 2] + cx
        sy = (fy * cam[:, 1]) / cam[:, 2] + cy
        X, Y = np.rint(sx * F(256.0)), np.rint(sy * F(256.0))
        in_range = (np.abs(X) < SNAP_LIMIT) & (np.abs(Y) < SNAP_LIMIT)
        front = cam[:, 2] >= near
    XY = np.stack([np.where(in_range, X, 0), np.where(in_range, Y, 0)], 1).astype(np.int64)
    status = np.full(len(tri), 2, np.int64)
    t = np.where(ok[:, None], tri, 0)
    behind = ~front[t].all(1)
    far_off = ~in_range[t].all(1)
    status[ok] = np.where(behind[ok] | far_off[ok], 1, 0)
    return cam, XY, status


def rasterize(vertices, triangles, w2c, fx, fy, cx, cy, H, W, near=0.01):
    """-> (keys uint64 [H,W], clipped): the key buffer after the depth test"""
    vertices = np.asarray(vertices, F).reshape(-1, 3)
    tri, _ = _valid_triangles(triangles, len(vertices))
    keys = np.full((H, W), EMPTY, np.uint64)
    if len(tri) == 0 or len(vertices) == 0:
        return keys, 0
    cam, XY, status = snap(vertices, tri, w2c, fx, fy, cx, cy, near)
    near = F(near)
    for t in np.flatnonzero(status == 0):
        ia, ib, ic = tri[t]
        P = XY[[ia, ib, ic]]
        area2 = (P[1, 0] - P[0, 0]) * (P[2, 1] - P[0, 1]) - (P[1, 1] - P[0, 1]) * (P[2, 0] - P[0, 0])
        if area2 == 0:
            continue
        if area2 < 0:
            P = P[[0, 2, 1]]
        i0, i1 = max((P[:, 0].min() + 127) >> 8, 0), min((P[:, 0].max() - 128) >> 8, W - 1)
        j0, j1 = max((P[:, 1].min() + 127) >> 8, 0), min((P[:, 1].max() - 128) >> 8, H - 1)
        if i0 > i1 or j0 > j1:
            continue
        ii, jj = np.arange(i0, i1 + 1), np.arange(j0, j1 + 1)
        px, py = (256 * ii + 128)[None, :], (256 * jj + 128)[:, None]
        cover = np.ones((len(jj), len(ii)), bool)
        for e in range(3):
            f = (e + 1) % 3
            dx, dy = P[f, 0] - P[e, 0], P[f, 1] - P[e, 1]
            E = dx * (py - P[e, 1]) - dy * (px - P[e, 0])
            owns = dy > 0 or (dy == 0 and dx > 0)
            cover &= (E > 0) | ((E == 0) & owns)
        if not cover.any():
            continue
        a, b, c = cam[ia], cam[ib], cam[ic]
        n = _cross(a, b, c)
        with np.errstate(all="ignore"):
            na = _dot(n, a)
            dx, dy = pixel_dirs(fx, fy, cx, cy, ii, jj)
            nd = (n[0] * dx[None, :] + n[1] * dy[:, None]) + n[2]
            z = (na / nd).astype(F)
            cover &= (z >= near) & (z < F(np.inf))
        key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
        sub = keys[j0:j1 + 1, i0:i1 + 1]
        np.minimum(sub, np.where(cover, key, EMPTY), out=sub)
    return keys, int((status == 1).sum())


def decode(keys):
    """-> (depth fp32 [H,W] 0 where empty, tri_id int32 [H,W] -1 where empty)"""
    empty = keys == EMPTY
    depth = (keys >> np.uint64(32)).astype(np.uint32).view(F).copy()
    depth[empty] = 0
    tri_id = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    tri_id[empty] = -1
    return depth, tri_id.astype(np.int32)


def _normalize(v, dtype):
    with np.errstate(all="ignore"):
        ln = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        good = (ln > 0) & (ln < np.inf)
        out = v / np.where(good, ln, np.ones_like(ln))[..., None]
    out[~good] = np.array([0, 0, 1], dtype)
    return out.astype(dtype)


def resolve(keys, vertices, triangles, w2c, fx, fy, cx, cy, colors=None, normals=None, mode="shaded", ambient=0.3,
            background=(1.0, 1.0, 1.0), dtype=F):
    """-> image [H,W,3] in `dtype`.  dtype=np.float32: the header's resolve stage, operator by operator.  dtype=np.float64: the
    same formulas in float64 on the same triangle per pixel, depth taken from the plane instead of the key."""
    H, W = keys.shape
    depth, tri_id = decode(keys)
    image = np.empty((H, W, 3), dtype)
    image[:] = np.asarray(background, F).astype(dtype)
    jj, ii = np.nonzero(tri_id >= 0)
    if len(jj) == 0:
        return image
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)[tri_id[jj, ii]]
    cam = to_camera(w2c, vertices, dtype)
    a, b, c = cam[tri[:, 0]], cam[tri[:, 1]], cam[tri[:, 2]]
    n = _cross(a, b, c)
    dx, dy = pixel_dirs(fx, fy, cx, cy, ii, jj, dtype)
    if dtype == F:
        z = depth[jj, ii]
    else:
        z = _dot(n, a) / ((n[:, 0] * dx + n[:, 1] * dy) + n[:, 2])
    P = np.stack([z * dx, z * dy, z], 1)
    r = [a - P, b - P, c - P]
    w = [_dot(n, _cross_of(r[(k + 1) % 3], r[(k + 2) % 3])) for k in range(3)]
    s = (w[0] + w[1]) + w[2]
    with np.errstate(all="ignore"):
        lam = [wk / s for wk in w]
    sliver = ~(np.isfinite(lam[0]) & np.isfinite(lam[1]) & np.isfinite(lam[2]))
    lam = [np.where(sliver, dtype(1.0) / dtype(3.0), lk) for lk in lam]

    def interp(attr):
        A = np.asarray(attr, F).astype(dtype)
        return (lam[0][:, None] * A[tri[:, 0]] + lam[1][:, None] * A[tri[:, 1]]) + lam[2][:, None] * A[tri[:, 2]]

    base = interp(colors) if colors is not None else np.full((len(jj), 3), F(0.7), F).astype(dtype)
    if mode == "color":
        out = base
    else:
        wm = np.asarray(w2c, F).astype(dtype)
        nw = interp(normals)
        nc = np.stack([(wm[r_, 0] * nw[:, 0] + wm[r_, 1] * nw[:, 1]) + wm[r_, 2] * nw[:, 2] for r_ in range(3)], 1)
        nn = _normalize(nc, dtype)
        if mode == "normal":
            out = (nn + dtype(1.0)) / dtype(2.0)
        else:
            vv = _normalize(-P, dtype)
            amb = F(ambient).astype(dtype)
            shade = amb + (dtype(1.0) - amb) * np.abs(_dot(nn, vv))
            out = base * shade[:, None]
    image[jj, ii] = out
    return image


def vertex_normal_sums(vertices, triangles):
    """-> (sums int64 [V,3] on the grid q, bits of the largest |cross component| (uint32), normals fp32 [V,3])"""
    v = np.asarray(vertices, F).reshape(-1, 3)
    tri, ok = _valid_triangles(triangles, len(v))
    tri = tri[ok]
    with np.errstate(all="ignore"):
        cr = _cross(v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]).astype(F)
    fin = np.isfinite(cr).all(1)
    tri, cr = tri[fin], cr[fin]
    m = F(np.abs(cr).max()) if len(cr) else F(0)
    bits = np.array([m], F).view(np.uint32)[0]
    E = int(bits >> np.uint32(23))
    k = np.rint(cr.astype(np.float64) * np.ldexp(1.0, 166 - E)).astype(np.int64)
    sums = np.zeros((len(v), 3), np.int64)
    for col in range(3):
        np.add.at(sums, tri[:, col], k)
    return sums, bits, _normalize(sums.astype(F), F)


def vertex_normals_f64(vertices, triangles):
    """the area-weighted normals in float64, no grid: the yardstick of the normalised normals"""
    v = np.asarray(vertices, F).astype(np.float64).reshape(-1, 3)
    tri, ok = _valid_triangles(triangles, len(v))
    tri = tri[ok]
    cr = _cross(v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]])
    sums = np.zeros((len(v), 3))
    for col in range(3):
        np.add.at(sums, tri[:, col], cr)
    return _normalize(sums, np.float64)


# ---- the independent yardstick: float64 ray casting --------------------------------------------------------------------------

def ray_cast(vertices, triangles, w2c, fx, fy, cx, cy, H, W, near=0.01, chunk=256):
    """Moeller-Trumbore, every pixel x every triangle, float64, two-sided.
    -> (tri int64 [H,W] nearest hit or -1, z float64 [H,W] camera depth (inf where none), gap float64 [H,W]: the distance in
    depth to the second-nearest hit)"""
    cam = to_camera(w2c, vertices, np.float64)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    a, b, c = cam[tri[:, 0]], cam[tri[:, 1]], cam[tri[:, 2]]
    front = (np.stack([a[:, 2], b[:, 2], c[:, 2]], 1) >= near).all(1)
    e1, e2 = b - a, c - a
    jj, ii = np.divmod(np.arange(H * W), W)
    dx, dy = pixel_dirs(float(fx), float(fy), float(cx), float(cy), ii, jj, np.float64)
    d = np.stack([dx, dy, np.ones_like(dx)], 1)
    best = np.full(H * W, -1, np.int64)
    zbest = np.full(H * W, np.inf)
    zsecond = np.full(H * W, np.inf)
    for lo in range(0, H * W, chunk):
        dd = d[lo:lo + chunk, None, :]                              # [P,1,3]; the origin is the camera centre
        pv = np.cross(dd, e2[None])
        det = (e1[None] * pv).sum(-1)
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            tv = -a[None]
            u = (tv * pv).sum(-1) * inv
            qv = np.cross(tv, e1[None])
            v = (dd * qv).sum(-1) * inv
            z = (e2[None] * qv).sum(-1) * inv
        hit = front[None] & (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (z >= near) & np.isfinite(z)
        z = np.where(hit, z, np.inf)
        order = np.argsort(z, axis=1)[:, :2]
        rows = np.arange(z.shape[0])
        z0 = z[rows, order[:, 0]]
        zbest[lo:lo + chunk] = z0
        best[lo:lo + chunk] = np.where(np.isfinite(z0), order[:, 0], -1)
        if z.shape[1] > 1:
            zsecond[lo:lo + chunk] = z[rows, order[:, 1]]
    with np.errstate(invalid="ignore"):
        gap = zsecond - zbest
    return best.reshape(H, W), zbest.reshape(H, W), gap.reshape(H, W)


def edge_distance_px(vertices, triangles, w2c, fx, fy, cx, cy, H, W, near=0.01):
    """float64: for every pixel centre the distance (in pixels) to the nearest projected edge of a triangle in front of the
    camera.  -> [H,W]"""
    cam = to_camera(w2c, vertices, np.float64)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    front = (cam[tri][:, :, 2] >= near).all(1)
    with np.errstate(all="ignore"):
        s = np.stack([fx * cam[:, 0] / cam[:, 2] + cx, fy * cam[:, 1] / cam[:, 2] + cy], 1)
    tri = tri[front]
    e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    e = np.unique(np.sort(e, 1), axis=0)
    p0, p1 = s[e[:, 0]], s[e[:, 1]]
    dist = np.full((H, W), np.inf)
    for (x0, y0), (x1, y1) in zip(p0, p1):
        i0, i1 = int(np.floor(min(x0, x1) - 1.5)), int(np.ceil(max(x0, x1) + 0.5))
        j0, j1 = int(np.floor(min(y0, y1) - 1.5)), int(np.ceil(max(y0, y1) + 0.5))
        i0, i1, j0, j1 = max(i0, 0), min(i1, W - 1), max(j0, 0), min(j1, H - 1)
        if i0 > i1 or j0 > j1:
            continue
        gx, gy = np.meshgrid(np.arange(i0, i1 + 1) + 0.5, np.arange(j0, j1 + 1) + 0.5)
        ex, ey = x1 - x0, y1 - y0
        L2 = ex * ex + ey * ey
        tt = np.clip(((gx - x0) * ex + (gy - y0) * ey) / L2, 0, 1) if L2 > 0 else np.zeros_like(gx)
        dd = np.hypot(gx - (x0 + tt * ex), gy - (y0 + tt * ey))
        sub = dist[j0:j1 + 1, i0:i1 + 1]
        np.minimum(sub, dd, out=sub)
    return dist


# ---- meshes and cameras ----------------------------------------------------------------------------------------------------

def icosphere(subdivisions=3, radius=1.0, center=(0.0, 0.0, 0.0)):
    """-> (vertices fp32 [V,3], triangles int64 [T,3]), T = 20 * 4^subdivisions, outward winding"""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(p, q):
            key = (min(p, q), max(p, q))
            if key not in mid:
                m = v[p] + v[q]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius + np.asarray(center)).astype(F), np.asarray(f, np.int64)


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """OpenGL camera-to-world [4,4] float64 (camera looks along -z, y up)"""
    eye, target, up = (np.asarray(x, np.float64) for x in (eye, target, up))
    zax = eye - target
    zax /= np.linalg.norm(zax)
    xax = np.cross(up, zax)
    xax /= np.linalg.norm(xax)
    yax = np.cross(zax, xax)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = xax, yax, zax, eye
    return m


def cv2gl_pose(c2w):
    """OpenGL <-> OpenCV camera-to-world: columns 1 and 2 negated (its own inverse)"""
    m = np.array(c2w, np.float64)
    m[:3, 1:3] *= -1
    return m


def to_unit_box(vertices, shape):
    """index-space marching-cubes vertices -> [-1, 1]^3 (the longest side spans it), fp32"""
    return (np.asarray(vertices, np.float64) / (max(shape) - 1.0) * 2 - 1).astype(F)


# the restatement's own fp32 depth error against float64 (tests/test_raster_host.py measures it: its docstring)
OWN_FP32_DEPTH_ERROR = 4.7e-7


def split_plane():
    """A planar fan cut into halves A and B along edges: vertices exactly on pixel centres and on pixel-centre lines of a
    32 x 32 image seen by an axis-aligned camera (fx = fy = 16, z = 2: world x = (sx - 16) / 8 is exact in fp32).
    -> (vertices, triangles A, triangles B, w2c, intrinsics)"""
    pts_px = np.array([(4.5, 4.5), (27.5, 4.5), (27.5, 27.5), (4.5, 27.5), (16.5, 16.5), (16.5, 4.5), (27.5, 10.5), (10.5, 27.5),
                       (4.5, 20.5)], np.float64)
    v = np.concatenate([(pts_px - 16) / 8, np.full((len(pts_px), 1), 2.0)], 1).astype(F)
    fan = [(4, 0, 5), (4, 5, 1), (4, 1, 6), (4, 6, 2), (4, 2, 7), (4, 7, 3), (4, 3, 8), (4, 8, 0)]
    A = np.array(fan[:3] + fan[6:7], np.int64)
    B = np.array(fan[3:6] + fan[7:], np.int64)[:, [0, 2, 1]]                   # the other winding: both are drawn
    w2c = np.eye(4, dtype=F)[:3]
    return v, A, B, w2c, (16.0, 16.0, 16.0, 16.0)
