"""Mesh rendering on the device: render_all_meshes (morpheus.py:418-470) without an OpenGL window.

The reference opens an Open3D Visualizer per frame, sets the frame's camera (or a 360-degree orbit), and captures the screen
and the float depth buffer; depths.npz feeds the depth-L1 evaluation (tools/culling.py:eval_depthL1) and the PNGs the
video_real / video_360 videos.  Here the mesh stays where extract_mesh left it and the HIP rasteriser of csrc/raster.hip
(mh_raster_depth + mh_raster_resolve, vertex normals by mh_mesh_vertex_normals; conventions in include/morpheus_hip.h)
renders it.  A render call does not wait for the device: every output's size follows from H and W.
"""
from __future__ import annotations

import glob
import os
import re
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import MorpheusHipError, launch, ptr
from .geometry import (cv2gl, host_array, host_ptr, intrinsics, mesh_arrays, transform_points,  # noqa: F401  (cv2gl: re-exported)
                       world_to_camera)
from .mesh import load_mesh
from .video import VideoWriter

MODES = {"color": 0, "normal": 1, "shaded": 2}
MAX_SIDE = 16384


def vertex_normal_sums(vertices: torch.Tensor, triangles: torch.Tensor):
    """-> (normals float32 [V,3], acc int64 [3V + 1]): the area-weighted vertex normals and the fixed-point sums they come
    from (acc[:3V] = sums [V][3] on the grid q, acc[3V] = the bits of the mesh's largest |cross component|)."""
    tri = mesh_arrays(vertices, triangles)
    V, T = vertices.shape[0], tri.shape[0]
    acc = torch.empty(3 * V + 1, dtype=torch.int64, device=vertices.device)
    normals = torch.empty(V, 3, dtype=torch.float32, device=vertices.device)
    launch("mh_mesh_vertex_normals", ptr(vertices), V, ptr(tri), T, ptr(acc), ptr(normals))
    return normals, acc


def vertex_normals(vertices: torch.Tensor, triangles: torch.Tensor) -> torch.Tensor:
    """Open3D's compute_vertex_normals (morpheus.py:432): the un-normalised cross products of a vertex's triangles summed
    (order-free, in fixed point), then normalised; (0, 0, 1) for a zero sum."""
    return vertex_normal_sums(vertices, triangles)[0]


def _intrinsics(K, fx, fy, cx, cy):
    if K is not None:
        return intrinsics(K)
    if None in (fx, fy, cx, cy):
        raise MorpheusHipError("render_mesh needs K or fx, fy, cx, cy")
    return float(fx), float(fy), float(cx), float(cy)


def render_mesh(vertices: torch.Tensor, triangles: torch.Tensor, colors: Optional[torch.Tensor] = None,
                normals: Optional[torch.Tensor] = None, *, c2w, H: int, W: int, K=None, fx=None, fy=None, cx=None, cy=None,
                convention: str = "opengl", mode: str = "shaded", near: float = 0.01,
                background: Sequence[float] = (1.0, 1.0, 1.0), ambient: float = 0.3, small_area: int = 0) -> dict:
    """Render a triangle mesh from a pinhole camera.
    -> dict(depth float32 [H,W] camera-space z, 0 where empty; tri_id int32 [H,W], -1 where empty; image float32 [H,W,3];
            clipped int64 [] triangles dropped because a vertex lies behind `near` or projects beyond the snapping range).
    c2w is a host pose ('opengl': the dataset's; 'opencv').  mode: 'color' | 'normal' | 'shaded'.  Vertex normals are
    computed when a mode needs them and none are given.  depth and tri_id do not depend on mode, run or triangle order."""
    if mode not in MODES:
        raise MorpheusHipError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    tri = mesh_arrays(vertices, triangles, colors, normals)
    H, W = int(H), int(W)
    V, T = vertices.shape[0], tri.shape[0]
    lib = _lib.load()
    wbytes = lib.mh_raster_workspace_bytes(H, W, T)
    if wbytes < 0:
        raise MorpheusHipError(f"render_mesh: H, W must be in [1, {MAX_SIDE}] and T below 2^31, got {H} x {W}, T = {T}")
    fx, fy, cx, cy = _intrinsics(K, fx, fy, cx, cy)
    w2c = world_to_camera(c2w, convention)
    w2c_p = host_ptr(w2c)
    if normals is None and MODES[mode] != 0:
        normals = vertex_normals(vertices, tri)
    dev = vertices.device
    ws = torch.empty(wbytes, dtype=torch.uint8, device=dev)
    clipped = torch.empty((), dtype=torch.int64, device=dev)
    depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    tri_id = torch.empty(H, W, dtype=torch.int32, device=dev)
    image = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    launch("mh_raster_depth", ptr(vertices), V, ptr(tri), T, w2c_p, fx, fy, cx, cy, H, W, float(near), int(small_area), ptr(ws),
           ptr(clipped))
    bg = [float(b) for b in background]
    launch("mh_raster_resolve", ptr(vertices), V, ptr(tri), T, ptr(colors), ptr(normals), w2c_p, fx, fy, cx, cy, H, W, MODES[mode],
           float(ambient), bg[0], bg[1], bg[2], ptr(ws), ptr(depth), ptr(tri_id), ptr(image))
    return {"depth": depth, "tri_id": tri_id, "image": image, "clipped": clipped}


def concat_meshes(geom_list, need_colors: bool = False) -> dict:
    """Several mesh dicts -> one (vertices, triangles, colors) on the device: each mesh's optional 4 x 4 `transform` (host,
    float64) is applied to its vertices through geometry.transform_points, the triangle indices are offset.  colors: None when
    no mesh has any; a mesh without colours beside coloured ones gets the rasteriser's 0.7 grey."""
    if not geom_list:
        raise MorpheusHipError("render_mesh_from_view: geom_list is empty")
    any_colors = need_colors and any(g.get("colors") is not None for g in geom_list)
    verts, tris, cols, base = [], [], [], 0
    for g in geom_list:
        v, t = g["vertices"], g["triangles"]
        mesh_arrays(v, t, g.get("colors"))
        if g.get("transform") is not None and v.shape[0]:
            v = transform_points(v, g["transform"])
        verts.append(v)
        tris.append(t.to(torch.int64) + base)
        if any_colors:
            cols.append(g["colors"] if g.get("colors") is not None else torch.full_like(v, 0.7))
        base += v.shape[0]
    return {"vertices": torch.cat(verts).contiguous(), "triangles": torch.cat(tris).contiguous(),
            "colors": torch.cat(cols).contiguous() if any_colors else None}


VIEW_MODES = {"gray": "shaded", "color": "color", "normal": "normal"}


def render_mesh_from_view(geom_list, c2w, K, H: int, W: int, mode: str = "gray", show_backface: bool = True,
                          return_result: bool = False, **render_kwargs):
    """render_mesh_from_view (tools/vis.py:216-248): the meshes of geom_list (mesh dicts, each with an optional 4 x 4
    `transform`, visualizer.py:222) in one image from the OpenCV pose c2w.  mode: "gray" (shaded, no colours), "color" (the
    vertex colours, unlit, as Open3D's MeshColorOption.Color), "normal".  -> image float32 [H,W,3] on the device (the
    reference returns the host array of capture_screen_float_buffer), or render_mesh's whole result with return_result.  Back
    faces are always drawn (show_backface is accepted for the signature's sake)."""
    if mode not in VIEW_MODES:
        raise MorpheusHipError(f"mode must be one of {sorted(VIEW_MODES)}, got {mode!r}")
    scene = concat_meshes(geom_list, need_colors=(mode == "color"))
    render_kwargs.setdefault("convention", "opencv")
    out = render_mesh(scene["vertices"], scene["triangles"], scene["colors"], c2w=c2w, K=K, H=H, W=W, mode=VIEW_MODES[mode],
                      **render_kwargs)
    return out if return_result else out["image"]


_PLY_NAME = re.compile(r"mesh_(\d+)_(\d+)\.ply$")


def mesh_sequence(meshes_or_dir, device, epoch=None):
    """-> iterator of (frame id, mesh dict on the device).  A directory holds mesh_{epoch:04d}_{frame:04d}.ply, every epoch's
    files side by side (morpheus.py:1489): `epoch` selects one; without it the directory must hold a single epoch."""
    if isinstance(meshes_or_dir, (str, os.PathLike)):
        named = []
        for path in glob.glob(os.path.join(os.fspath(meshes_or_dir), "*.ply")):
            m = _PLY_NAME.match(os.path.basename(path))
            if m:
                named.append((int(m.group(1)), int(m.group(2)), path))
        epochs = sorted({e for e, _, _ in named})
        if epoch is None:
            if len(epochs) > 1:
                raise MorpheusHipError(f"{meshes_or_dir} holds the meshes of epochs {epochs}: say which with epoch=")
        else:
            named = [n for n in named if n[0] == int(epoch)]
        if not named:
            raise MorpheusHipError(f"no mesh_EPOCH_FRAME.ply under {meshes_or_dir}" +
                                   ("" if epoch is None else f" for epoch {int(epoch)} (found epochs {epochs})"))
        for _, frame, path in sorted(named):
            yield frame, load_mesh(path, device)
    else:
        if epoch is not None:
            raise MorpheusHipError("epoch selects files of a mesh directory; it has no meaning for an iterable of meshes")
        for i, mesh in enumerate(meshes_or_dir):
            yield i, mesh


def render_all_meshes(meshes_or_dir, poses, K, H: int, W: int, save_images_dir: Optional[str] = None,
                      save_depths_dir: Optional[str] = None, scale: int = 4, epoch: Optional[int] = None,
                      convention: str = "opengl", mode: str = "shaded", near: float = 0.01,
                      background: Sequence[float] = (1.0, 1.0, 1.0), ambient: float = 0.3, device="cuda",
                      keep_results: bool = False, video_path: Optional[str] = None, fps=20):
    """The loop of render_all_meshes (morpheus.py:418-470): mesh i is rendered from poses[i] at (scale*H) x (scale*W) with
    K[:2] * scale and the principal point at the image centre -- (scale*W/2, scale*H/2) here, where a pixel centre sits at
    (i + 0.5, j + 0.5); Open3D's set_K writes w/2 - 0.5 for the same point in its integer-centre convention.
    meshes_or_dir: a directory of mesh_{epoch:04d}_{frame:04d}.ply (frame = index into poses; `epoch` selects the files, and
    is required when the directory holds several epochs) or an iterable of extract_mesh dicts, so model -> mesh -> depth need
    not touch the disk.  Writes {i:04d}.png under save_images_dir (needs PIL) and depths.npz with keys depth_{i} under
    save_depths_dir.  -> {"depth_{i}": host float32 [scale*H, scale*W]}, what depths.npz holds (the reference keeps no more
    than that across frames); with keep_results the list of render_mesh results instead, device tensors of 20 bytes per
    pixel and frame.  The per-frame depth PNGs of capture_depth_image (morpheus.py:461) are not written.  With video_path the
    frames also go, from the device, to a Motion-JPEG .avi at `fps` (video.VideoWriter: what the reference's make_video makes
    of the PNGs, morpheus.py:467-468); without it no video is written."""
    Image = None
    if save_images_dir is not None:
        try:
            from PIL import Image
        except ImportError as e:                                   # images were asked for and cannot be written
            raise MorpheusHipError("render_all_meshes: save_images_dir needs PIL to write PNGs") from e
        os.makedirs(save_images_dir, exist_ok=True)
    K = host_array(K, np.float64)                                  # only the focal lengths are read
    fx, fy = K[0, 0] * scale, K[1, 1] * scale
    h, w = int(H * scale), int(W * scale)
    results, depths = [], {}
    writer = None
    if video_path is not None:
        writer = VideoWriter(video_path, fps)
    done = False
    try:
        for i, mesh in mesh_sequence(meshes_or_dir, device, epoch):
            out = render_mesh(mesh["vertices"], mesh["triangles"], mesh.get("colors"), mesh.get("normals"), c2w=poses[i], H=h, W=w,
                              fx=fx, fy=fy, cx=w / 2.0, cy=h / 2.0, convention=convention, mode=mode, near=near,
                              background=background, ambient=ambient)
            if keep_results:
                results.append(out)
            depths[f"depth_{i}"] = out["depth"].cpu().numpy()
            if Image is not None or writer is not None:
                rgb = (out["image"].nan_to_num(0.0).clamp(0, 1) * 255).round().to(torch.uint8)
                if writer is not None:
                    writer.append(rgb)                             # coded from the device, batch by batch
                if Image is not None:
                    Image.fromarray(rgb.cpu().numpy()).save(os.path.join(save_images_dir, f"{i:04d}.png"))
        done = True
    finally:
        if writer is not None:
            writer.close(discard_pending=not done)
    if save_depths_dir is not None:
        os.makedirs(save_depths_dir, exist_ok=True)
        np.savez(os.path.join(save_depths_dir, "depths.npz"), **depths)
    return results if keep_results else depths
