"""Mesh export on the device: export_mesh (morpheus.py:367-408) without the host round trip.

The reference queries the SDF on a resolution^3 grid in S^3 sub-grids, copies every sub-grid to the host, runs
mcubes.marching_cubes there, queries the colours at the vertices and writes the file with trimesh.  Here the volume stays on
the device, marching cubes runs on the HIP kernels of csrc/mesh.hip (mh_mc_count + mh_mc_emit; conventions in
include/morpheus_hip.h) and write_ply writes the binary PLY that Open3D reads (render_all_meshes,
morpheus.py:431); morpheus_amd.meshrender renders it here and read_ply reads it back.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib
from ._lib import MorpheusHipError, launch, ptr, require_gpu
from .geometry import host_array


def _count_then_emit(count_name, emit_name, count_args, emit_args, wbytes, device, extra_counters=None, check=None):
    """The two passes of every marching cubes -> (vertices float32 [V,3], triangles int64 [T,3]): count_name(*count_args, workspace,
    counts) sizes the outputs, ONE host read fetches V and T (and extra_counters, an integer device tensor, with them),
    check(V, T, *extra) may refuse them, emit_name(*emit_args, workspace, vertices, triangles) fills them unless both are empty."""
    ws = torch.empty(wbytes, dtype=torch.uint8, device=device)
    counts = torch.empty(2, dtype=torch.int64, device=device)
    launch(count_name, *count_args, ptr(ws), ptr(counts))
    V, T, *extra = (counts if extra_counters is None else torch.cat([counts, extra_counters.long()])).tolist()
    if check is not None:
        check(V, T, *extra)
    vertices = torch.empty(V, 3, dtype=torch.float32, device=device)
    triangles = torch.empty(T, 3, dtype=torch.int32, device=device)
    if V or T:
        launch(emit_name, *emit_args, ptr(ws), ptr(vertices), ptr(triangles))
    return vertices, triangles.long()


def marching_cubes(volume: torch.Tensor, isovalue: float = 0.0):
    """volume: contiguous fp32 CUDA tensor [nx,ny,nz] -> (vertices float32 [V,3] in index space, triangles int64 [T,3]),
    as mcubes.marching_cubes returns them (up to vertex order and winding).  One host synchronisation (to size the outputs)."""
    require_gpu(volume)
    if volume.dim() != 3 or volume.dtype != torch.float32 or not volume.is_contiguous():
        raise MorpheusHipError(f"marching_cubes takes a contiguous float32 [nx,ny,nz] volume, got {volume.dtype} "
                               f"{tuple(volume.shape)}")
    nx, ny, nz = volume.shape
    wbytes = _lib.load().mh_mc_workspace_bytes(nx, ny, nz)
    if wbytes < 0:
        raise MorpheusHipError(f"marching_cubes: shape {tuple(volume.shape)} unsupported (each side >= 2, < 2^31 points)")
    args = (ptr(volume), nx, ny, nz, float(isovalue))
    return _count_then_emit("mh_mc_count", "mh_mc_emit", args, args, wbytes, volume.device)


def marching_cubes_masked(volume: torch.Tensor, weight: torch.Tensor, isovalue: float = 0.0):
    """marching_cubes over the cells whose eight corners all have weight > 0 (mh_mc_count_masked + mh_mc_emit_masked): a cell
    with an unobserved corner gives no triangle and owns no vertex.  weight: contiguous fp32 like volume.  With every weight
    positive the result equals marching_cubes' bit for bit."""
    require_gpu(volume, weight)
    for name, a in (("volume", volume), ("weight", weight)):
        if a.dim() != 3 or a.dtype != torch.float32 or not a.is_contiguous() or a.shape != volume.shape:
            raise MorpheusHipError(f"marching_cubes_masked takes contiguous float32 [nx,ny,nz] volume and weight of one shape, got "
                                   f"{name} {a.dtype} {tuple(a.shape)}")
    nx, ny, nz = volume.shape
    wbytes = _lib.load().mh_mc_masked_workspace_bytes(nx, ny, nz)
    if wbytes < 0:
        raise MorpheusHipError(f"marching_cubes_masked: shape {tuple(volume.shape)} unsupported (each side >= 2, < 2^31 points)")
    args = (nx, ny, nz, float(isovalue))
    return _count_then_emit("mh_mc_count_masked", "mh_mc_emit_masked", (ptr(volume), ptr(weight)) + args, (ptr(volume),) + args,
                            wbytes, volume.device)


@torch.no_grad()
def sdf_volume(model, resolution: int = 128, S: int = 128, t=None, cano: bool = False) -> torch.Tensor:
    """The query of morpheus.py:381-395: model.density on torch.linspace(-1, 1, resolution)^3 in S^3 sub-grids, each
    sub-grid's SDF written into a [res,res,res] device volume (no host copy)."""
    dev = next(model.parameters()).device
    X = Y = Z = torch.linspace(-1, 1, resolution).split(S)
    sdf = torch.empty(resolution, resolution, resolution, dtype=torch.float32, device=dev)
    for xi, xs in enumerate(X):
        for yi, ys in enumerate(Y):
            for zi, zs in enumerate(Z):
                xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                val = model.density(pts.to(dev), t=t, cano=cano)
                sdf[xi * S: xi * S + len(xs), yi * S: yi * S + len(ys), zi * S: zi * S + len(zs)] = \
                    val["sdf"].reshape(len(xs), len(ys), len(zs))
    return sdf


@torch.no_grad()
def extract_mesh(model, resolution: int = 128, S: int = 128, t=None, cano: bool = False, color_mesh: bool = True):
    """export_mesh (morpheus.py:367-408) minus the file, on the device: sdf_volume, marching cubes at 0, vertices mapped to
    [-1, 1], albedo at the vertices.
    -> dict(vertices [V,3] fp32, triangles [T,3] int64, colors [V,3] fp32 or None, sdf [res,res,res] fp32)"""
    sdf = sdf_volume(model, resolution, S, t, cano)
    vertices, triangles = marching_cubes(sdf, 0.0)
    vertices = vertices / (resolution - 1.0) * 2 - 1
    colors = None
    if color_mesh:
        colors = model.density(vertices, t=t, cano=cano)["albedo"] if vertices.shape[0] else vertices.new_zeros(0, 3)
    return {"vertices": vertices, "triangles": triangles, "colors": colors, "sdf": sdf}


def write_ply(path: str, vertices, triangles, colors=None) -> None:
    """Binary little-endian PLY: float x y z [uchar red green blue alpha], faces as `list uchar int vertex_indices`.
    Colours in [0, 1] are stored as round(clip(c, 0, 1) * 255) with alpha 255."""
    v = host_array(vertices, "<f4").reshape(-1, 3)
    f = host_array(triangles, "<i4").reshape(-1, 3)
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}",
            "property float x", "property float y", "property float z"]
    if colors is not None:
        c = np.rint(np.clip(host_array(colors, np.float64).reshape(-1, 3), 0.0, 1.0) * 255.0).astype(np.uint8)
        head += ["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
        vrec = np.empty(v.shape[0], dtype=[("xyz", "<f4", 3), ("rgba", "u1", 4)])
        vrec["xyz"] = v
        vrec["rgba"][:, :3] = c
        vrec["rgba"][:, 3] = 255
    else:
        vrec = v
    head += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    frec = np.empty(f.shape[0], dtype=[("n", "u1"), ("idx", "<i4", 3)])
    frec["n"] = 3
    frec["idx"] = f
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


_PLY_TYPES = {"float": "<f4", "uchar": "u1", "int": "<i4"}


def read_ply(path: str):
    """The inverse of write_ply -> (vertices float32 [V,3], triangles int64 [T,3], colors float32 [V,3] = byte / 255, or None)
    as numpy arrays.  Reads the layout write_ply writes (binary little-endian, float / uchar vertex properties, triangle
    faces as `list uchar int`); anything else raises MorpheusHipError."""
    with open(path, "rb") as fh:
        data = fh.read()
    mark = data.find(b"end_header\n")
    if mark < 0:
        raise MorpheusHipError(f"{path}: no PLY header")
    end = mark + len(b"end_header\n")
    header = data[:end].decode("ascii", "replace").splitlines()
    if header[:2] != ["ply", "format binary_little_endian 1.0"]:
        raise MorpheusHipError(f"{path}: not a binary little-endian PLY")
    elems = []
    for line in header[2:-1]:
        w = line.split()
        if not w or w[0] == "comment":
            continue
        if w[0] == "element" and len(w) == 3:
            elems.append((w[1], int(w[2]), []))
        elif w[0] == "property" and elems and len(w) == 5 and w[1:4] == ["list", "uchar", "int"]:
            elems[-1][2].append(("list", w[4]))
        elif w[0] == "property" and elems and len(w) == 3 and w[1] in _PLY_TYPES:
            elems[-1][2].append((_PLY_TYPES[w[1]], w[2]))
        else:
            raise MorpheusHipError(f"{path}: unsupported header line {line!r}")
    if [e[0] for e in elems] != ["vertex", "face"] or elems[1][2] != [("list", "vertex_indices")] \
            or any(t == "list" for t, _ in elems[0][2]):
        raise MorpheusHipError(f"{path}: expected a vertex element and a face element of vertex_indices lists")
    (_, nv, vprops), (_, nf, _) = elems
    vdt = np.dtype([(name, t) for t, name in vprops])
    fdt = np.dtype([("n", "u1"), ("idx", "<i4", 3)])
    if not {"x", "y", "z"} <= set(vdt.names) or end + nv * vdt.itemsize + nf * fdt.itemsize != len(data):
        raise MorpheusHipError(f"{path}: vertex properties or file size do not match the header")
    verts = np.frombuffer(data, vdt, nv, end)
    faces = np.frombuffer(data, fdt, nf, end + nv * vdt.itemsize)
    if not (faces["n"] == 3).all():
        raise MorpheusHipError(f"{path}: only triangle faces are supported")
    vertices = np.stack([verts["x"], verts["y"], verts["z"]], 1).astype(np.float32)
    colors = None
    if {"red", "green", "blue"} <= set(vdt.names):
        colors = (np.stack([verts["red"], verts["green"], verts["blue"]], 1).astype(np.float32) / np.float32(255.0))
    return vertices, faces["idx"].astype(np.int64), colors


def export_mesh(model, mesh_savepath: str, resolution: int = 128, S: int = 128, t=None, cano: bool = False,
                color_mesh: bool = True) -> dict:
    """export_mesh (morpheus.py:367-408): extract_mesh, then write_ply to mesh_savepath (its directory is created)."""
    d = os.path.dirname(mesh_savepath)
    if d:
        os.makedirs(d, exist_ok=True)
    mesh = extract_mesh(model, resolution=resolution, S=S, t=t, cano=cano, color_mesh=color_mesh)
    write_ply(mesh_savepath, mesh["vertices"], mesh["triangles"], mesh["colors"])
    return mesh


def load_mesh(mesh_or_path, device):
    """the path of a PLY (read_ply's layout) -> dict(vertices, triangles, colors or None) on `device`; a mesh dict is handed back"""
    if not isinstance(mesh_or_path, (str, os.PathLike)):
        return mesh_or_path
    v, t, c = read_ply(os.fspath(mesh_or_path))
    return {"vertices": torch.from_numpy(v).to(device), "triangles": torch.from_numpy(t).to(device),
            "colors": None if c is None else torch.from_numpy(c).to(device)}
