"""numpy restatement of the pooled block-sparse TSDF store of csrc/tsdf_sparse.hip, written from the text of
include/morpheus_hip.h (TSDF fusion, the pooled block-sparse store): a dict of 8^3 blocks over a logical box that may be far too
large to hold densely.

Not a test module.  The usable-depth rule, the back-projection, the host side of poses and intrinsics, the masked marching
cubes, the colour rule and the synthetic scene are imported from tests/tsdf_oracle.py; the touch pass's block range and the
update of a voxel are its formulas again, applied to the blocks that exist instead of a dense array (tests/
test_tsdf_sparse_host.py holds the two to each other bit for bit on a box both can hold).
  * SparseVolume: touch (allocation) / integrate per frame in `dtype`, to_dense of a range of blocks, extract_mesh;
  * canonical(): a mesh in an order that does not depend on the order its vertices and triangles were emitted in.
"""
from __future__ import annotations

import numpy as np

from tests import tsdf_oracle as to

F = np.float32
BLOCK = to.BLOCK


class SparseVolume:
    """blocks: {linear block id (bx*nby + by)*nbz + bz: row of the arrays}, in the order the blocks were first touched; tsdf, weight
    [n,8,8,8], color [n,3,8,8,8] in dtype"""

    def __init__(self, voxel_length, sdf_trunc, origin, dims, dtype=F):
        self.dt = dtype
        self.vl, self.trunc = dtype(F(voxel_length)), dtype(F(sdf_trunc))
        self.origin = np.asarray(origin, np.float64).astype(F).astype(dtype)
        self.dims = tuple(int(d) for d in dims)
        assert all(d % BLOCK == 0 and d > 0 for d in self.dims)
        self.nb = tuple(d // BLOCK for d in self.dims)
        self.blocks = {}
        self.tsdf = np.zeros((0, 8, 8, 8), dtype)
        self.weight = np.zeros((0, 8, 8, 8), dtype)
        self.color = np.zeros((0, 3, 8, 8, 8), dtype)
        self._frame = to.Volume(voxel_length, sdf_trunc, origin, (8, 8, 8), dtype)        # for its back_project only

    def coords(self, ids=None):
        """block ids -> [n,3] block coordinates (default: the allocated blocks in row order)"""
        ids = np.fromiter(self.blocks, np.int64, len(self.blocks)) if ids is None else np.asarray(ids, np.int64)
        return np.stack(np.unravel_index(ids, self.nb), 1).astype(np.int64).reshape(-1, 3)

    def touched(self, depth, mask, intr, c2w, depth_scale=1.0, depth_trunc=10.0, stride=4):
        """-> the sorted ids of the blocks this frame's touch pass reaches (the header's lo / hi range, clipped to the box)"""
        dt = self.dt
        P = self._frame.back_project(depth, mask, intr, c2w, depth_scale, depth_trunc, stride)
        L = dt(8.0) * self.vl
        ok = np.ones(P.shape[0], bool)
        rng = []
        for a in range(3):
            with np.errstate(all="ignore"):
                lo = np.floor(((P[:, a] - self.trunc) - self.origin[a]) / L)
                hi = np.floor(((P[:, a] + self.trunc) - self.origin[a]) / L)
                ok &= (hi >= 0) & (lo <= self.nb[a] - 1)
            rng.append((lo, hi))
        if not ok.any():
            return np.zeros(0, np.int64)
        cols = []
        for a in range(3):
            cols += [np.maximum(rng[a][0][ok], 0).astype(np.int64), np.minimum(rng[a][1][ok], self.nb[a] - 1).astype(np.int64)]
        ids = set()
        for x0, x1, y0, y1, z0, z1 in np.unique(np.stack(cols, 1), axis=0):
            g = np.stack(np.meshgrid(np.arange(x0, x1 + 1), np.arange(y0, y1 + 1), np.arange(z0, z1 + 1), indexing="ij"), -1)
            ids.update(np.ravel_multi_index(tuple(g.reshape(-1, 3).T), self.nb).tolist())
        return np.array(sorted(ids), np.int64)

    def touch(self, *args, **kw):
        new = [b for b in self.touched(*args, **kw).tolist() if b not in self.blocks]
        for b in new:
            self.blocks[b] = len(self.blocks)
        if new:
            grow = lambda a: np.concatenate([a, np.zeros((len(new),) + a.shape[1:], a.dtype)])
            self.tsdf, self.weight, self.color = grow(self.tsdf), grow(self.weight), grow(self.color)

    def integrate(self, depth, rgb, mask, intr, w2c, depth_scale=1.0, depth_trunc=10.0):
        """every voxel of every allocated block, with its GLOBAL index: the formulas of tsdf_oracle.Volume.integrate"""
        if not self.blocks:
            return
        dt = self.dt
        fx, fy, cx, cy = (dt(v) for v in intr)
        d, ok = to.usable_depth(depth, mask, depth_scale, depth_trunc, dt)
        H, W = d.shape
        half = dt(0.5)
        g = self.coords()[:, :, None] * BLOCK + np.arange(BLOCK)[None, None]            # [n,3,8] global voxel indices
        px = (self.origin[0] + (g[:, 0].astype(dt) + half) * self.vl)[:, :, None, None]
        py = (self.origin[1] + (g[:, 1].astype(dt) + half) * self.vl)[:, None, :, None]
        pz = (self.origin[2] + (g[:, 2].astype(dt) + half) * self.vl)[:, None, None, :]
        w = np.asarray(w2c, F).astype(dt)
        pc = [((w[r, 0] * px + w[r, 1] * py) + w[r, 2] * pz) + w[r, 3] for r in range(3)]
        with np.errstate(all="ignore"):
            upd = pc[2] > 0
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
            self.tsdf = np.where(upd, (self.tsdf * wgt + t) / w1, self.tsdf)
            pix = np.asarray(rgb, np.uint8)[pj, pi].astype(dt)                             # [n,8,8,8,3]
            for ch in range(3):
                self.color[:, ch] = np.where(upd, (self.color[:, ch] * wgt + pix[..., ch]) / w1, self.color[:, ch])
            self.weight = np.where(upd, w1, wgt)

    def add_frame(self, depth, rgb, K, c2w, mask=None, depth_scale=1.0, depth_trunc=10.0, stride=4, pixel_centers="half"):
        intr = to.host_intrinsics(K, pixel_centers)
        c, w = to.host_pose(c2w)
        self.touch(depth, mask, intr, c, depth_scale, depth_trunc, stride)
        self.integrate(depth, rgb, mask, intr, w, depth_scale, depth_trunc)

    def allocated(self):
        return np.array(sorted(self.blocks), np.int64)

    def block_range(self):
        """-> (lo [3], hi [3]): the blocks [lo, hi) that bound the allocated ones"""
        c = self.coords()
        return c.min(0), c.max(0) + 1

    def to_dense(self, lo=None, hi=None):
        """the blocks [lo, hi) (default: the whole logical box) as dense arrays -> dict(tsdf, weight [nx,ny,nz], color [3,nx,ny,nz],
        active [blocks] uint8): a block without storage reads as zeros"""
        lo = np.zeros(3, np.int64) if lo is None else np.asarray(lo, np.int64)
        hi = np.array(self.nb, np.int64) if hi is None else np.asarray(hi, np.int64)
        n = tuple(int(x) for x in (hi - lo))
        out = dict(tsdf=np.zeros(tuple(8 * x for x in n), self.dt), weight=np.zeros(tuple(8 * x for x in n), self.dt),
                   color=np.zeros((3,) + tuple(8 * x for x in n), self.dt), active=np.zeros(n, np.uint8))
        for (bx, by, bz), row in zip(self.coords().tolist(), self.blocks.values()):
            x, y, z = bx - lo[0], by - lo[1], bz - lo[2]
            if not (0 <= x < n[0] and 0 <= y < n[1] and 0 <= z < n[2]):
                continue
            sl = (slice(8 * x, 8 * x + 8), slice(8 * y, 8 * y + 8), slice(8 * z, 8 * z + 8))
            out["tsdf"][sl], out["weight"][sl], out["active"][x, y, z] = self.tsdf[row], self.weight[row], 1
            out["color"][(slice(None),) + sl] = self.color[row]
        return out

    def extract_mesh(self):
        """-> (vertices world space fp32 [V,3], triangles, colors, index-space vertices): tsdf_oracle's masked marching cubes over
        the blocks that bound the allocated ones.  Blocks outside them have no storage, so no cell reaches across their border
        and the mesh is the logical box's.  The index-space vertices are the sub-box's plus its offset: for an offset other than 0
        that is one more fp32 rounding than the kernel's (float)i + t (well inside a test's geometric bound; not for bits)."""
        lo, hi = self.block_range()
        d = self.to_dense(lo, hi)
        iv, tri = to.masked_marching_cubes(d["tsdf"].astype(F), d["weight"], 0.0)
        colors = to.vertex_colors(iv, d["color"].astype(F))
        iv = (iv + (lo * BLOCK).astype(F)[None]).astype(F)
        world = self.origin.astype(F)[None] + (iv + F(0.5)) * F(self.vl)
        return world.astype(F), tri, colors, iv


def fuse_scene(dtype=F, stride=4, pixel_centers="half", origin=to.SCENE_ORIGIN, dims=to.SCENE_DIMS, frames=None):
    """tsdf_oracle.fuse_scene into a SparseVolume"""
    s = to.scene()
    K = s["K"].copy()
    if pixel_centers == "integer":
        K[:2, 2] -= 0.5
    vol = SparseVolume(to.VOXEL, to.TRUNC, origin, dims, dtype)
    for f in (range(len(s["c2w"])) if frames is None else frames):
        vol.add_frame(s["depth"][f], s["rgb"][f], K, s["c2w"][f], s["mask"][f], stride=stride, pixel_centers=pixel_centers)
    return vol


# the box the dense store refuses: 2^32 voxels, with the synthetic scene's box SHIFT whole blocks inside it
LARGE_DIMS = (2048, 2048, 1024)
LARGE_SHIFT = (101, 120, 57)


def large_origin():
    """float64 [3]: the logical box's corner, such that block LARGE_SHIFT starts at the scene box's corner"""
    return np.asarray(to.SCENE_ORIGIN, np.float64) - np.asarray(LARGE_SHIFT, np.float64) * BLOCK * to.VOXEL


def canonical(vertices, triangles, colors=None):
    """A mesh in an order of its own: vertices sorted lexicographically by coordinate (x, then y, then z: an owned edge gives one
    vertex, so the coordinates tell vertices apart -- asserted), triangles renumbered, each rotated to start at its smallest id
    (winding kept: a flipped triangle is another triangle), rows sorted.  -> (vertices, triangles int64, colors or None)"""
    v = np.asarray(vertices)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    order = np.lexsort((v[:, 2], v[:, 1], v[:, 0]))
    v = v[order]
    assert len(v) < 2 or (v[1:] != v[:-1]).any(1).all(), "two vertices share their coordinates"
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    t = rank[t]
    first = np.argmin(t, 1)
    t = t[np.arange(len(t))[:, None], (first[:, None] + np.arange(3)[None]) % 3]
    t = t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]
    return v, t, None if colors is None else np.asarray(colors)[order]
