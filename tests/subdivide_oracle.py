"""Numpy restatement of the subdivision conventions of include/morpheus_hip.h (mh_subdiv_count, mh_subdiv_emit), written from the
header text: float64 operator by operator in the written order, then one rounding to fp32.  Vectorised per depth: every split
triangle of one depth shares the lattice tables of its n = 2^d.
"""
from __future__ import annotations

import numpy as np

F = np.float32


# ---- depths and counts -----------------------------------------------------------------------------------------------------

def edge_depth(p, q, max_edge, max_iter):
    """p, q fp32 [N,3] -> the smallest d in [0, max_iter + 1] for which l2 * 4^-d > m2 is false."""
    m = float(F(max_edge))
    m2 = m * m
    p, q = np.asarray(p, F).astype(np.float64), np.asarray(q, F).astype(np.float64)
    with np.errstate(all="ignore"):
        dx, dy, dz = q[:, 0] - p[:, 0], q[:, 1] - p[:, 1], q[:, 2] - p[:, 2]
        l2 = (dx * dx + dy * dy) + dz * dz
        d = np.zeros(len(l2), np.int32)
        for k in range(max_iter + 1):
            d += (d == k) & (l2 * 4.0 ** -k > m2)                  # still too long at every depth below k, and at k
    return d


def depths(vertices, triangles, max_edge=0.01, max_iter=10):
    """-> depth int32 [T]: the largest of the three edges' depths; 0 for an index outside [0, V)."""
    v = np.asarray(vertices, F)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = ((tri >= 0) & (tri < v.shape[0])).all(axis=1)
    safe = np.where(ok[:, None], tri, 0)
    if v.shape[0] == 0:
        return np.zeros(len(tri), np.int32)
    a, b, c = v[safe[:, 0]], v[safe[:, 1]], v[safe[:, 2]]
    d = np.maximum(np.maximum(edge_depth(a, b, max_edge, max_iter), edge_depth(b, c, max_edge, max_iter)),
                   edge_depth(c, a, max_edge, max_iter))
    return np.where(ok, d, 0).astype(np.int32)


def counts(depth, max_iter=10):
    """-> (n_vert, n_tri) int64 [T]: L - 3 and n*n for a depth in [1, max_iter]; 0 and 1 otherwise."""
    d = np.asarray(depth, np.int64)
    split = (d >= 1) & (d <= max_iter)
    n = np.left_shift(np.int64(1), np.where(split, d, 0))
    return np.where(split, (n + 1) * (n + 2) // 2 - 3, 0), np.where(split, n * n, 1)


# ---- the two index maps ----------------------------------------------------------------------------------------------------

def row_q(j, n):
    """full lattice index of the first point of row j: j(n + 1) - j(j - 1)/2"""
    j = np.asarray(j, np.int64)
    return j * (n + 1) - j * (j - 1) // 2


def row_tri(j, n):
    """local index of the first triangle of row j: j(2n - j)"""
    j = np.asarray(j, np.int64)
    return j * (2 * n - j)


def lattice(n):
    """-> (i, j) int64 [L] of q = 0 .. L-1 in order, by enumeration: rows j = 0 .. n, i = 0 .. n - j."""
    j = np.repeat(np.arange(n + 1), n + 1 - np.arange(n + 1))
    return np.arange(len(j)) - row_q(j, n), j


def decode_q(q, n):
    """q -> (i, j): the last row that starts at or before q (what an emit thread computes)."""
    q = np.asarray(q, np.int64)
    j = np.searchsorted(row_q(np.arange(n + 1), n), q, side="right") - 1
    return q - row_q(j, n), j


def local_triangles(n):
    """-> (j, s) int64 [n*n] of local triangle l = 0 .. n*n - 1 in order, by enumeration: row j has 2(n - j) - 1 triangles."""
    j = np.repeat(np.arange(n), 2 * (n - np.arange(n)) - 1)
    return j, np.arange(len(j)) - row_tri(j, n)


def decode_tri(l, n):
    """l -> (j, s): the last row whose first triangle is at or before l."""
    l = np.asarray(l, np.int64)
    j = np.searchsorted(row_tri(np.arange(n), n), l, side="right") - 1
    return j, l - row_tri(j, n)


def triangle_lattice_indices(n):
    """-> q int64 [n*n, 3]: the full lattice indices of the three corners of every local triangle."""
    j, s = local_triangles(n)
    i = s >> 1
    odd = (s & 1) == 1
    q = lambda ii, jj: row_q(jj, n) + ii                           # noqa: E731
    return np.stack([np.where(odd, q(i + 1, j), q(i, j)), np.where(odd, q(i + 1, j + 1), q(i + 1, j)), q(i, j + 1)], axis=1)


# ---- emit ------------------------------------------------------------------------------------------------------------------

def lattice_points(A, B, C, n, i, j):
    """A, B, C fp32 [M,3]; i, j int [P] -> fp32 [M,P,3] = (float)(((k*A + i*B) + j*C) / n) in float64."""
    A, B, C = (np.asarray(x, F).astype(np.float64)[:, None, :] for x in (A, B, C))
    wi, wj = np.asarray(i, np.float64)[None, :, None], np.asarray(j, np.float64)[None, :, None]
    wk = float(n) - wi - wj                                        # small integers: exact
    with np.errstate(all="ignore"):
        return ((((wk * A) + (wi * B)) + (wj * C)) / float(n)).astype(F)


def subdivide(vertices, triangles, colors=None, max_edge=0.01, max_iter=10):
    """-> dict(vertices fp32 [V',3], triangles int32 [T',3], colors fp32 [V',3] or None, index int32 [T'], depth int32 [T],
    vert_start, tri_start int64 [T+1]).  A triangle of depth max_iter + 1 is copied, as the header says; the caller refuses."""
    v = np.ascontiguousarray(vertices, F)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    col = None if colors is None else np.ascontiguousarray(colors, F)
    V, T = v.shape[0], tri.shape[0]
    depth = depths(v, tri, max_edge, max_iter)
    nv, nt = counts(depth, max_iter)
    vert_start = np.concatenate([[0], np.cumsum(nv)]).astype(np.int64)
    tri_start = np.concatenate([[0], np.cumsum(nt)]).astype(np.int64)
    out_v = np.zeros((V + int(vert_start[-1]), 3), F)
    out_v[:V] = v
    out_c = None
    if col is not None:
        out_c = np.zeros_like(out_v)
        out_c[:V] = col
    out_t = np.zeros((int(tri_start[-1]), 3), np.int32)
    index = np.repeat(np.arange(T), nt).astype(np.int32)
    plain = ~((depth >= 1) & (depth <= max_iter))
    out_t[tri_start[:-1][plain]] = tri[plain]
    for d in range(1, max_iter + 1):
        ts = np.nonzero(depth == d)[0]
        if ts.size == 0:
            continue
        n = 1 << d
        L = (n + 1) * (n + 2) // 2
        i, j = lattice(n)
        new = np.ones(L, bool)
        new[[0, n, L - 1]] = False
        qs = np.nonzero(new)[0]
        slot = np.where(qs < n, qs - 1, qs - 2)                    # 0 .. L-4
        tq = triangle_lattice_indices(n)                           # [n*n, 3]
        step = max(1, (1 << 22) // L)                              # bounded temporaries
        for lo in range(0, ts.size, step):
            tt = ts[lo:lo + step]
            a, b, c = tri[tt, 0], tri[tt, 1], tri[tt, 2]
            dest = V + vert_start[tt][:, None] + slot[None, :]
            out_v[dest] = lattice_points(v[a], v[b], v[c], n, i[qs], j[qs])
            if col is not None:
                out_c[dest] = lattice_points(col[a], col[b], col[c], n, i[qs], j[qs])
            ids = np.empty((tt.size, L), np.int64)                 # output vertex of every lattice index
            ids[:, qs] = dest
            ids[:, 0], ids[:, n], ids[:, L - 1] = a, b, c
            rows = tri_start[tt][:, None] + np.arange(n * n)[None, :]
            out_t[rows] = ids[:, tq]
    return {"vertices": out_v, "triangles": out_t, "colors": out_c, "index": index, "depth": depth,
            "vert_start": vert_start, "tri_start": tri_start}


# ---- trimesh's algorithm, for the host test -----------------------------------------------------------------------------

def recursive_leaf_depths(A, B, C, max_edge, max_iter=10):
    """Triangles (float64 [N,3] corners) split as trimesh.remesh.subdivide_to_size does, all of one round at a time: a triangle
    with an edge longer than max_edge becomes four at its edge midpoints and the children are tested on their own in the next
    round.  -> (parent int64 [M], depth int64 [M]) of every leaf; a triangle still too long after max_iter rounds is a leaf of
    depth max_iter + 1."""
    a, b, c = (np.asarray(x, np.float64) for x in (A, B, C))
    parent = np.arange(len(a))
    leaves_p, leaves_d = [], []
    for d in range(max_iter + 1):
        longest = np.sqrt(np.maximum(np.maximum(((b - a) ** 2).sum(1), ((c - b) ** 2).sum(1)), ((a - c) ** 2).sum(1)))
        too_long = longest > max_edge
        leaves_p.append(parent[~too_long])
        leaves_d.append(np.full(int((~too_long).sum()), d))
        a, b, c, parent = a[too_long], b[too_long], c[too_long], parent[too_long]
        if d == max_iter or len(a) == 0:
            break
        ab, bc, ca = (a + b) / 2, (b + c) / 2, (c + a) / 2
        a, b, c = (np.concatenate(x) for x in ((a, ab, ca, ab), (ab, b, bc, bc), (ca, bc, c, ca)))
        parent = np.tile(parent, 4)
    leaves_p.append(parent)
    leaves_d.append(np.full(len(parent), max_iter + 1))
    return np.concatenate(leaves_p), np.concatenate(leaves_d)
