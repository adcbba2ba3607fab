"""numpy restatement of the marching cubes of csrc/mesh.hip (conventions: include/morpheus_hip.h, mh_mc_*).

Not a test module: tests/test_mesh_host.py checks it against geometry that does not depend on the table, and
tests/test_gpu_mesh.py checks the kernels against it bit for bit.  It reads the table the kernels are built with
(morpheus_amd/csrc/mc_table.inc) and keeps their order, winding and fp32 arithmetic.
"""
from __future__ import annotations

import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_PATH = os.path.join(ROOT, "morpheus_amd", "csrc", "mc_table.inc")

# corner c of the cell at p: p + CORNER[c] (Bourke's numbering); edge e: owner corner and axis
CORNER = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], np.int64)
EDGE_OWNER = np.array([0, 1, 3, 0, 4, 5, 7, 4, 0, 1, 2, 3], np.int64)      # as a corner number
EDGE_AXIS = np.array([0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2], np.int64)


def load_table() -> np.ndarray:
    words = re.findall(r"0x([0-9a-f]{16})ull", open(TABLE_PATH).read())
    assert len(words) == 256, len(words)
    return np.array([int(w, 16) for w in words], np.uint64)


TABLE = load_table()


def marching_cubes(vol, iso=0.0):
    """-> (vertices float32 [V,3] index space, triangles int64 [T,3])"""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    assert vol.ndim == 3 and min(vol.shape) >= 2
    iso = np.float32(iso)
    nx, ny, nz = vol.shape
    n = vol.size
    inside = vol < iso
    # crossed[p, a]: the edge from p to p + e_a exists and its ends lie on different sides
    crossed = np.zeros((nx, ny, nz, 3), bool)
    crossed[:-1, :, :, 0] = inside[:-1] != inside[1:]
    crossed[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    crossed[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    key = np.flatnonzero(crossed.reshape(-1))                 # p*3 + a, ascending: owner point, then axis
    V = key.size
    edge_id = np.full(3 * n, -1, np.int64)
    edge_id[key] = np.arange(V)
    p, a = key // 3, key % 3
    stride = np.array([ny * nz, nz, 1], np.int64)
    flat = vol.reshape(-1)
    f0, f1 = flat[p], flat[p + stride[a]]
    with np.errstate(all="ignore"):
        t = (iso - f0) / (f1 - f0)
    t = np.where((t >= 0) & (t <= 1), t, np.float32(0.5)).astype(np.float32)
    ijk = np.stack(np.unravel_index(p, (nx, ny, nz)), 1).astype(np.float32)
    ijk[np.arange(V), a] += t                                 # one fp32 addition
    vertices = ijk.reshape(V, 3)

    # cells: case index from the eight corners
    cube = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c, (dx, dy, dz) in enumerate(CORNER):
        cube |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    ci, cj, ck = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing="ij")
    cell_p = ((ci * ny + cj) * nz + ck).reshape(-1)
    words = TABLE[cube.reshape(-1)]
    ntri = (words >> np.uint64(60)).astype(np.int64)
    live = ntri > 0
    cell_p, words, ntri = cell_p[live], words[live], ntri[live]
    T = int(ntri.sum())
    tri_cell = np.repeat(np.arange(cell_p.size), ntri)
    tri_rank = np.arange(T) - np.repeat(np.cumsum(ntri) - ntri, ntri)   # triangle number inside its cell
    tris = np.empty((T, 3), np.int64)
    corner_off = CORNER @ stride
    for m in range(3):
        e = ((words[tri_cell] >> (4 * (3 * tri_rank + m)).astype(np.uint64)) & np.uint64(15)).astype(np.int64)
        owner = cell_p[tri_cell] + corner_off[EDGE_OWNER[e]]
        tris[:, m] = edge_id[owner * 3 + EDGE_AXIS[e]]
    assert T == 0 or tris.min() >= 0
    return vertices, tris[:, [0, 2, 1]].copy()                 # the table winds toward decreasing f


# ---- geometry of a triangle mesh (shared by the host and GPU tests) -------------------------------------------------------

def edge_uses(tris):
    """-> (undirected edges [E,2] sorted, how many triangles use each)"""
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]])
    e = np.sort(e, 1)
    return np.unique(e, axis=0, return_counts=True)


def euler(vertices, tris):
    used = np.unique(tris)
    edges, _ = edge_uses(tris)
    return used.size - edges.shape[0] + tris.shape[0]


def signed_volume(vertices, tris):
    v = vertices.astype(np.float64)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def area(vertices, tris):
    v = vertices.astype(np.float64)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    return float(np.linalg.norm(np.cross(b - a, c - a), axis=1).sum() / 2.0)


# ---- test volumes (fp32, index space) ------------------------------------------------------------------------------------

def _coords(shape):
    return np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), -1)


def sphere(shape, center, radius):
    return (np.linalg.norm(_coords(shape) - np.asarray(center), axis=-1) - radius).astype(np.float32)


def torus(shape, center, R, r):
    p = _coords(shape) - np.asarray(center)
    q = np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - R
    return (np.sqrt(q ** 2 + p[..., 2] ** 2) - r).astype(np.float32)


def plane(shape, normal, offset):
    """f = n . x - offset, n normalised (float64 then rounded once)"""
    n = np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    return (_coords(shape) @ n - offset).astype(np.float32), n


def gaussians(shape, rng, k=40, sigma=3.0):
    """a sum of signed Gaussian bumps minus a level: many saddles, so many ambiguous faces"""
    x = _coords(shape)
    f = np.zeros(shape)
    for _ in range(k):
        c = rng.uniform(0, np.asarray(shape) - 1)
        f += rng.choice([-1.0, 1.0]) * np.exp(-((x - c) ** 2).sum(-1) / (2 * sigma ** 2))
    return (f - 0.05).astype(np.float32)


# ---- a small reader of the binary PLY layout morpheus_amd.mesh.write_ply writes --------------------------------------------

_PLY_TYPES = {"float": "<f4", "uchar": "u1", "int": "<i4"}


def read_ply(path):
    """-> (header lines, vertex record array, faces int [F,3]); triangle faces only"""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").splitlines()
    assert header[0] == "ply" and header[1] == "format binary_little_endian 1.0", header[:2]
    elems, cur = [], None
    for line in header[2:-1]:
        w = line.split()
        if w[0] == "element":
            cur = (w[1], int(w[2]), [])
            elems.append(cur)
        elif w[0] == "property" and w[1] == "list":
            assert (w[2], w[3]) == ("uchar", "int"), line
            cur[2].append(("list", w[4]))
        else:
            assert w[0] == "property", line
            cur[2].append((_PLY_TYPES[w[1]], w[2]))
    (vname, nv, vprops), (fname, nf, fprops) = elems
    assert (vname, fname) == ("vertex", "face") and fprops == [("list", "vertex_indices")]
    vdt = np.dtype([(name, t) for t, name in vprops])
    verts = np.frombuffer(data, vdt, nv, end)
    fdt = np.dtype([("n", "u1"), ("idx", "<i4", 3)])
    faces = np.frombuffer(data, fdt, nf, end + nv * vdt.itemsize)
    assert (faces["n"] == 3).all() and end + nv * vdt.itemsize + nf * fdt.itemsize == len(data)
    return header, verts, faces["idx"].astype(np.int64)
