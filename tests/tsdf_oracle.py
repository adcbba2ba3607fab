"""numpy restatement of the TSDF fusion of csrc/tsdf.hip and of the masked marching cubes of csrc/mesh.hip, written from the
text of include/morpheus_hip.h (TSDF fusion; marching cubes, the masked pair).

Not a test module.  Three things live here:
  * Volume: touch / integrate operator by operator in `dtype` -- np.float32 is what tests/test_gpu_tsdf.py holds the kernels to
    bit for bit; np.float64 is the same formulas on the same fp32-rounded inputs, the yardstick of the fp32 result;
  * masked_marching_cubes / vertex_colors / extract_mesh: the masked pair and the colour rule, in mc_oracle's order;
  * scene(): the synthetic RGB-D sequence of the tests (an icosphere standing on a quad, cameras on an arc, depth from
    raster_oracle.ray_cast in float64) and the closed-form distance to the surfaces it was made from.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import mc_oracle as mo
from tests import raster_oracle as ro

F = np.float32
BLOCK = 8


def host_pose(c2w):
    """host side of the contract: OpenCV camera-to-world -> (c2w fp32 [3,4], w2c fp32 [3,4] = the float64 inverse rounded once)"""
    m = np.eye(4)
    m[:3] = np.asarray(c2w, np.float64)[:3]
    return np.ascontiguousarray(m[:3].astype(F)), np.ascontiguousarray(np.linalg.inv(m)[:3].astype(F))


def host_intrinsics(K, pixel_centers="half"):
    """-> (fx, fy, cx, cy) as fp32: what the C ABI receives.  "integer": cx + 0.5, cy + 0.5 in float64, then rounded"""
    K = np.asarray(K, np.float64)
    s = 0.5 if pixel_centers == "integer" else 0.0
    return F(K[0, 0]), F(K[1, 1]), F(K[0, 2] + s), F(K[1, 2] + s)


def usable_depth(depth, mask, depth_scale, depth_trunc, dtype):
    """-> (d in dtype [H,W], usable bool [H,W])"""
    with np.errstate(all="ignore"):
        d = np.asarray(depth, F).astype(dtype) / dtype(F(depth_scale))
        ok = (d > 0) & (d <= dtype(F(depth_trunc)))
    if mask is not None:
        ok &= np.asarray(mask) != 0
    return d, ok


class Volume:
    def __init__(self, voxel_length, sdf_trunc, origin, dims, dtype=F):
        self.dt = dtype
        self.vl, self.trunc = dtype(F(voxel_length)), dtype(F(sdf_trunc))
        self.origin = np.asarray(origin, np.float64).astype(F).astype(dtype)
        self.dims = tuple(int(d) for d in dims)
        assert all(d % BLOCK == 0 and d > 0 for d in self.dims)
        self.blocks = tuple(d // BLOCK for d in self.dims)
        self.tsdf = np.zeros(self.dims, dtype)
        self.weight = np.zeros(self.dims, dtype)
        self.color = np.zeros((3,) + self.dims, dtype)
        self.active = np.zeros(self.blocks, np.uint8)

    # -- back-projection of the sampled usable pixels: P [n,3] in dtype
    def back_project(self, depth, mask, intr, c2w, depth_scale, depth_trunc, stride):
        dt = self.dt
        fx, fy, cx, cy = (dt(v) for v in intr)
        d, ok = usable_depth(depth, mask, depth_scale, depth_trunc, dt)
        H, W = d.shape
        jj, ii = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
        sel = ok[jj, ii]
        ii, jj = ii[sel], jj[sel]
        dd = d[jj, ii]
        xc = (((ii.astype(dt) + dt(0.5)) - cx) / fx) * dd
        yc = (((jj.astype(dt) + dt(0.5)) - cy) / fy) * dd
        c = np.asarray(c2w, F).astype(dt)
        return np.stack([((c[r, 0] * xc + c[r, 1] * yc) + c[r, 2] * dd) + c[r, 3] for r in range(3)], 1)

    def touch(self, depth, mask, intr, c2w, depth_scale=1.0, depth_trunc=10.0, stride=4):
        dt = self.dt
        P = self.back_project(depth, mask, intr, c2w, depth_scale, depth_trunc, stride)
        L = dt(8.0) * self.vl
        rng = []
        ok = np.ones(P.shape[0], bool)
        for a in range(3):
            with np.errstate(all="ignore"):
                lo = np.floor(((P[:, a] - self.trunc) - self.origin[a]) / L)
                hi = np.floor(((P[:, a] + self.trunc) - self.origin[a]) / L)
                ok &= (hi >= 0) & (lo <= self.blocks[a] - 1)
            rng.append((lo, hi))
        for a in range(3):
            lo, hi = rng[a]
            rng[a] = (np.maximum(lo[ok], 0).astype(np.int64), np.minimum(hi[ok], self.blocks[a] - 1).astype(np.int64))
        # the distinct block ranges (few: a range spans one or two blocks per axis for sdf_trunc of a few voxels)
        boxes = np.unique(np.stack([rng[0][0], rng[0][1], rng[1][0], rng[1][1], rng[2][0], rng[2][1]], 1), axis=0) \
            if ok.any() else np.zeros((0, 6), np.int64)
        for x0, x1, y0, y1, z0, z1 in boxes:
            self.active[x0:x1 + 1, y0:y1 + 1, z0:z1 + 1] = 1

    def integrate(self, depth, rgb, mask, intr, w2c, depth_scale=1.0, depth_trunc=10.0):
        dt = self.dt
        fx, fy, cx, cy = (dt(v) for v in intr)
        d, ok = usable_depth(depth, mask, depth_scale, depth_trunc, dt)
        H, W = d.shape
        nx, ny, nz = self.dims
        half = dt(0.5)
        px = (self.origin[0] + (np.arange(nx).astype(dt) + half) * self.vl)[:, None, None]
        py = (self.origin[1] + (np.arange(ny).astype(dt) + half) * self.vl)[None, :, None]
        pz = (self.origin[2] + (np.arange(nz).astype(dt) + half) * self.vl)[None, None, :]
        w = np.asarray(w2c, F).astype(dt)
        pc = [((w[r, 0] * px + w[r, 1] * py) + w[r, 2] * pz) + w[r, 3] for r in range(3)]
        upd = np.repeat(np.repeat(np.repeat(self.active.astype(bool), BLOCK, 0), BLOCK, 1), BLOCK, 2)
        with np.errstate(all="ignore"):
            upd = upd & (pc[2] > 0)
            u = np.floor((fx * pc[0]) / pc[2] + cx)
            v = np.floor((fy * pc[1]) / pc[2] + cy)
            upd &= (u >= 0) & (u < W) & (v >= 0) & (v < H)
            pi = np.where(upd, u, 0).astype(np.int64)
            pj = np.where(upd, v, 0).astype(np.int64)
            upd &= ok[pj, pi]
            dd = d[pj, pi]
            a = ((pi.astype(dt) + half) - cx) / fx
            b = ((pj.astype(dt) + half) - cy) / fy
            m = np.sqrt((dt(1.0) + a * a) + b * b)
            sdf = (dd - pc[2]) * m
            upd &= sdf > -self.trunc
            q = sdf / self.trunc
            t = np.where(q < 1, q, dt(1.0))
        wgt = self.weight
        w1 = wgt + dt(1.0)
        with np.errstate(all="ignore"):
            self.tsdf = np.where(upd, (self.tsdf * wgt + t) / w1, self.tsdf)
            pix = np.asarray(rgb, np.uint8)[pj, pi].astype(dt)          # [nx,ny,nz,3]
            for ch in range(3):
                self.color[ch] = np.where(upd, (self.color[ch] * wgt + pix[..., ch]) / w1, self.color[ch])
        self.weight = np.where(upd, w1, wgt)
        self.last_pixel = np.where(upd, pj * W + pi, -1)             # which pixel updated each voxel in this frame (-1: none)
        with np.errstate(all="ignore"):
            self.last_u = (fx * pc[0]) / pc[2] + cx, (fy * pc[1]) / pc[2] + cy
        return upd

    def add_frame(self, depth, rgb, K, c2w, mask=None, depth_scale=1.0, depth_trunc=10.0, stride=4, pixel_centers="half"):
        intr = host_intrinsics(K, pixel_centers)
        c, w = host_pose(c2w)
        self.touch(depth, mask, intr, c, depth_scale, depth_trunc, stride)
        return self.integrate(depth, rgb, mask, intr, w, depth_scale, depth_trunc)


# ---- the masked pair -----------------------------------------------------------------------------------------------------------

def valid_cells(weight):
    """[nx-1,ny-1,nz-1] bool: all eight corners observed (weight > 0)"""
    with np.errstate(invalid="ignore"):
        obs = np.asarray(weight) > 0
    nx, ny, nz = obs.shape
    ok = np.ones((nx - 1, ny - 1, nz - 1), bool)
    for dx, dy, dz in mo.CORNER:
        ok &= obs[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]
    return ok


def masked_marching_cubes(vol, weight, iso=0.0):
    """The header's masked pair -> (vertices float32 [V,3] index space, triangles int64 [T,3]) in mc_oracle's order: a cell exists
    only when valid_cells holds; a vertex exists on a crossed edge only when one of the cells around the edge exists."""
    vol = np.ascontiguousarray(vol, dtype=F)
    iso = F(iso)
    nx, ny, nz = vol.shape
    n = vol.size
    cells = np.zeros((nx, ny, nz), bool)                       # indexed by the cell's corner 0; False on the upper border
    cells[:-1, :-1, :-1] = valid_cells(weight)
    inside = vol < iso

    def around(axis):
        """edge from p along `axis`: any cell at p - {0, u} - {0, v} exists"""
        u, v = [a for a in range(3) if a != axis]
        out = cells.copy()
        for su, sv in ((1, 0), (0, 1), (1, 1)):
            sh = cells
            if su:
                sh = np.concatenate([np.zeros_like(np.take(sh, [0], u)), np.delete(sh, -1, u)], u)
            if sv:
                sh = np.concatenate([np.zeros_like(np.take(sh, [0], v)), np.delete(sh, -1, v)], v)
            out |= sh
        return out

    crossed = np.zeros((nx, ny, nz, 3), bool)
    crossed[:-1, :, :, 0] = inside[:-1] != inside[1:]
    crossed[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    crossed[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    for a in range(3):
        crossed[..., a] &= around(a)
    key = np.flatnonzero(crossed.reshape(-1))
    V = key.size
    edge_id = np.full(3 * n, -1, np.int64)
    edge_id[key] = np.arange(V)
    p, a = key // 3, key % 3
    stride = np.array([ny * nz, nz, 1], np.int64)
    flat = vol.reshape(-1)
    f0, f1 = flat[p], flat[p + stride[a]]
    with np.errstate(all="ignore"):
        t = (iso - f0) / (f1 - f0)
    t = np.where((t >= 0) & (t <= 1), t, F(0.5)).astype(F)
    ijk = np.stack(np.unravel_index(p, (nx, ny, nz)), 1).astype(F)
    ijk[np.arange(V), a] += t
    vertices = ijk.reshape(V, 3)

    cube = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c, (dx, dy, dz) in enumerate(mo.CORNER):
        cube |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    ci, cj, ck = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing="ij")
    cell_p = ((ci * ny + cj) * nz + ck).reshape(-1)
    words = mo.TABLE[cube.reshape(-1)]
    ntri = (words >> np.uint64(60)).astype(np.int64)
    live = (ntri > 0) & cells[:-1, :-1, :-1].reshape(-1)
    cell_p, words, ntri = cell_p[live], words[live], ntri[live]
    T = int(ntri.sum())
    tri_cell = np.repeat(np.arange(cell_p.size), ntri)
    tri_rank = np.arange(T) - np.repeat(np.cumsum(ntri) - ntri, ntri)
    tris = np.empty((T, 3), np.int64)
    corner_off = mo.CORNER @ stride
    for m in range(3):
        e = ((words[tri_cell] >> (4 * (3 * tri_rank + m)).astype(np.uint64)) & np.uint64(15)).astype(np.int64)
        owner = cell_p[tri_cell] + corner_off[mo.EDGE_OWNER[e]]
        tris[:, m] = edge_id[owner * 3 + mo.EDGE_AXIS[e]]
    assert T == 0 or tris.min() >= 0
    return vertices, tris[:, [0, 2, 1]].copy()


def vertex_colors(vertices, color, dtype=F):
    """the header's colour rule: vertices [V,3] fp32 index space, color [3,nx,ny,nz] -> [V,3] in dtype, in [0, 1]"""
    dt = dtype
    x = np.asarray(vertices, F)
    n = np.array(color.shape[1:], np.int64)
    fl = np.floor(x)
    ok = ((fl >= 0) & (fl <= (n - 1)[None])).all(1)
    q = np.where(ok[:, None], fl, 0).astype(np.int64)
    fr = x - fl                                                     # exact in fp32
    cand = (fr > 0) & (q + 1 < n[None])
    has = cand.any(1)
    axis = np.argmax(cand, 1)                                       # the first such axis
    t = np.where(has, fr[np.arange(len(x)), axis], F(0.0)).astype(dt)
    q1 = q.copy()
    q1[np.arange(len(x)), axis] += has
    out = np.zeros((len(x), 3), dt)
    for ch in range(3):
        c0 = color[ch][q[:, 0], q[:, 1], q[:, 2]].astype(dt)
        c1 = color[ch][q1[:, 0], q1[:, 1], q1[:, 2]].astype(dt)
        out[:, ch] = np.where(ok, ((dt(1.0) - t) * c0 + t * c1) / dt(255.0), dt(0.0))
    return out


def extract_mesh(vol: Volume):
    """-> (vertices world space in fp32 [V,3], triangles, colors, index-space vertices): TSDFVolume.extract_mesh's chain"""
    iv, tri = masked_marching_cubes(vol.tsdf.astype(F), vol.weight, 0.0)
    world = vol.origin.astype(F)[None] + (iv + F(0.5)) * F(vol.vl)
    return world.astype(F), tri, vertex_colors(iv, vol.color.astype(F)), iv


# ---- the synthetic sequence -------------------------------------------------------------------------------------------------------

RADIUS, PLANE_Z = 0.3, -0.3
VOXEL, TRUNC = 0.02, 0.04
H, W, FOCAL = 120, 160, 140.0
N_CAMERAS = 13                                                       # twelve on the arc, one above
BAD_ROW = 5                                                          # of frame 2: zeros / NaN / beyond depth_trunc
MASKED_FRAME = 1                                                     # its mask removes the sphere


QUAD_HALF, QUAD_CELLS = 1.5, 12


def scene_mesh():
    """icosphere (radius 0.3 at the origin) on a quad in the plane z = -0.3 -> (vertices fp32, triangles int64, number of sphere
    triangles).  The quad is cut into 12 x 12 cells: the ray caster and the rasteriser drop a triangle with a vertex behind the
    camera whole, and two triangles 3 m wide have one behind every camera of the arc."""
    sv, st = ro.icosphere(3, RADIUS)
    n = QUAD_CELLS
    g = np.linspace(-QUAD_HALF, QUAD_HALF, n + 1)
    xx, yy = np.meshgrid(g, g, indexing="ij")
    qv = np.stack([xx.reshape(-1), yy.reshape(-1), np.full((n + 1) ** 2, PLANE_Z)], 1).astype(F)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).reshape(-1)
    qt = np.concatenate([np.stack([a, a + n + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + 1], 1)]) + len(sv)
    return np.concatenate([sv, qv]), np.concatenate([st, qt.astype(np.int64)]), len(st)


def scene_color(P):
    """a smooth function of the world position, quantised to RGB8"""
    P = np.asarray(P, np.float64)
    c = 0.5 + 0.5 * np.sin(3.0 * P + np.array([0.0, 1.0, 2.0]))
    return np.floor(255.0 * c).clip(0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def scene(n_cameras=N_CAMERAS, h=H, w=W, focal=FOCAL):
    """-> dict(K [3,3] half-integer-centre intrinsics, c2w list (OpenCV), depth list fp32 [h,w], rgb list uint8 [h,w,3], masks list
    (None but for MASKED_FRAME), mesh (vertices, triangles))"""
    verts, tris, n_sphere = scene_mesh()
    K = np.array([[focal, 0, w / 2.0], [0, focal, h / 2.0], [0, 0, 1]], np.float64)
    c2ws, depths, rgbs, masks = [], [], [], []
    for f in range(n_cameras):
        ang = 0.37 + 2 * np.pi * f / (n_cameras - 1)                      # off the box's axes: an axis-aligned camera puts whole
        # rows of voxel centres exactly on pixel boundaries, where fp32 and float64 round floor(u) apart
        gl = ro.look_at((1.2 * np.cos(ang), 1.2 * np.sin(ang), 0.5), (0.0, 0.0, -0.1))
        if f == n_cameras - 1:
            # the last camera looks down from above.  The cameras of the arc see the top of the sphere at 10 degrees from its
            # tangent plane; the distance along the ray is 6 x the distance to the surface there, so the first voxel inside
            # the sphere falls behind -sdf_trunc, stays unobserved, and the masked marching cubes leaves a hole
            gl = ro.look_at((0.05, 0.03, 1.5), (0.0, 0.0, -0.3), up=(0.3, 1.0, 0.0))
        cv = ro.cv2gl_pose(gl)
        w2c = np.linalg.inv(cv)[:3]
        # the sphere is convex and seen from outside: its back faces never give the nearest hit, and every pixel x triangle
        # pair costs the same
        nrm = np.cross(verts[tris[:, 1]] - verts[tris[:, 0]], verts[tris[:, 2]] - verts[tris[:, 0]]).astype(np.float64)
        front = np.flatnonzero(((cv[:3, 3][None] - verts[tris[:, 0]]) * nrm).sum(1) > 0)
        front = np.union1d(front, np.arange(n_sphere, len(tris)))
        tri, z, _ = ro.ray_cast(verts, tris[front], w2c, focal, focal, w / 2.0, h / 2.0, h, w)
        tri = np.where(tri >= 0, front[np.maximum(tri, 0)], -1)
        hit = tri >= 0
        depth = np.where(hit, z, 0.0).astype(F)
        jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        dx, dy = ro.pixel_dirs(focal, focal, w / 2.0, h / 2.0, ii, jj, np.float64)
        zz = np.where(hit, z, 0.0)
        Pc = np.stack([dx * zz, dy * zz, zz], -1)
        Pw = Pc @ cv[:3, :3].T + cv[:3, 3]
        rgb = scene_color(Pw)
        mask = None
        if f == MASKED_FRAME:
            mask = (tri >= n_sphere).astype(F)                        # 1 on the quad, 0 on the sphere and the background
        if f == 2:
            depth[BAD_ROW, 0::3] = 0.0
            depth[BAD_ROW, 1::3] = np.nan
            depth[BAD_ROW, 2::3] = 1000.0
        c2ws.append(cv), depths.append(depth), rgbs.append(rgb), masks.append(mask)
    return {"K": K, "c2w": c2ws, "depth": depths, "rgb": rgbs, "mask": masks, "mesh": (verts, tris)}


SCENE_ORIGIN, SCENE_DIMS = (-0.64, -0.64, -0.48), (64, 64, 48)


def fuse_scene(dtype=F, stride=4, pixel_centers="half", origin=SCENE_ORIGIN, dims=SCENE_DIMS, frames=None, on_frame=None):
    s = scene()
    K = s["K"].copy()
    if pixel_centers == "integer":                                   # the same cameras described in Open3D's convention
        K[0, 2] -= 0.5
        K[1, 2] -= 0.5
    vol = Volume(VOXEL, TRUNC, origin, dims, dtype)
    for f in (range(len(s["c2w"])) if frames is None else frames):
        vol.add_frame(s["depth"][f], s["rgb"][f], K, s["c2w"][f], s["mask"][f], stride=stride, pixel_centers=pixel_centers)
        if on_frame is not None:
            on_frame(f, vol)
    return vol


def surface_distance(P):
    """closed form: distance from P [n,3] to the nearer of the sphere |x| = 0.3 and the plane z = -0.3 (float64)"""
    P = np.asarray(P, np.float64)
    return np.minimum(np.abs(np.linalg.norm(P, axis=1) - RADIUS), np.abs(P[:, 2] - PLANE_Z))
