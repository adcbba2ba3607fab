"""Time the TSDF fusion (morpheus_amd.tsdf, csrc/tsdf.hip) and the masked marching cubes (csrc/mesh.hip).

    python tools/bench_tsdf.py [--dims 256,512] [--frames 200] [--views 20] [--reps 20] [--out profiles/r10_tsdf_fusion.txt]
    python tools/bench_tsdf.py --store sparse [--grow 1,2] ...      the pooled block-sparse store (csrc/tsdf_sparse.hip)

Scene: synthetic (no dataset is assumed): an icosphere of radius 0.3 standing on a quad, --views cameras on a circle of radius
1.2, depth and colour at 640 x 480 from this library's own rasteriser; the views are cycled to --frames frames.  The box is the
cube [-0.64, 0.64]^3 at dims^3 voxels (voxel_length 1.28 / dims, sdf_trunc two voxels), stride 4.
  per-launch rows   mh_tsdf_touch and mh_tsdf_integrate: a HIP event pair around one pass over all --frames frames (>= 20
                    back-to-back calls), divided by the frames; --reps passes, median [min .. max].  active = share of active
                    blocks after the pass; bytes = active voxels x 40 (five fp32 arrays read and written) + the frame's 7 bytes a
                    pixel; GB/s = bytes / time (an algorithmic rate: it counts every voxel of an active block as updated)
  fusion row        run_tsdf_fusion of all frames with bounds= given, wall clock between two synchronisations (includes the
                    host's per-frame work and one extract_mesh)
  marching cubes    mesh.marching_cubes (the unmasked pair, unchanged by this feature: the yardstick) against
                    mesh.marching_cubes_masked on the same tsdf volume with every weight positive, alternating, wall clock (both
                    wait for the counts); then the masked pair with the fused weights (what extract_mesh runs)

Expectation, written before the first run: an integrate launch moves active voxels x 40 B plus the frame; at the 2.7 - 5 TB/s
this library's streaming kernels reach, a 512^3 box with 10 % of its blocks active would cost 0.1 - 0.2 ms a frame, and 200
frames of 640 x 480 would cost less than ONE 256^3 extract_mesh (17 - 75 ms) only if launches, not bytes, dominate.  On this
scene (a sphere and a ground plane in a cube) the active share should be well under 10 %, so each launch should sit near the
launch floor of a few microseconds of device time plus the host's ~10 us a call: 400 launches in ~10 ms, host-bound.  The masked
pair with all weights positive should be within the unmasked pair's own run-to-run spread, plus one streaming pass over the
weights (the cell marks: 4 B read + 1 B written a voxel, ~0.2 ms at 512^3).
--store sparse: the same scene into SparseTSDFVolume.  The logical box is the cube above grown --grow times a side (the content
stays where it is: the origin moves out by whole blocks), the pool is sized exactly (tsdf.count_touched_blocks).  Rows: the
per-launch pair (mh_tsdf_sparse_touch / mh_tsdf_sparse_integrate, timed as above; after the first pass every block has its slot,
as the dense activity bytes are all set), pool bytes (tsdf.sparse_bytes) against the dense bytes of the same box
(tsdf.volume_bytes), run_tsdf_fusion(store="sparse") and extract_mesh wall clock.
Expectation for the sparse store, written before its first run: integrate walks allocated blocks x 512 voxels x 20 B (read and
written: x 40 B), the bytes of the dense launch's active blocks, in full 256-byte lines, and skips the dense launch's pass over
the activity bytes of the whole grid; so per frame it should cost no more than the dense launch on the same box, and it should
stay flat when the logical box grows 8 x at fixed content (--grow 2), where only the index volume grows (4 B a block, touched
by the touch pass alone).  At grow 1 the allocated blocks are the dense active ones; at grow 2 the ground plane reaches beyond
the cube, so "fixed content" holds for the sphere only and the allocated count is reported beside the time.  Both launches
should sit near the launch floor on this scene, as the dense ones.  The sparse touch adds one atomic per NEW block, none in
the steady state that the passes time.  extract_mesh over the sparse store stages a 10^3 halo per block through the index
volume (2 x the block's own points); it should cost less than the dense masked pair whenever well under half of the blocks are
allocated, since the dense pair visits every point of the box.
Result: see the file named by --out and DESIGN 7d.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from morpheus_amd import geometry, mesh, meshrender, tsdf  # noqa: E402

H, W, FOCAL = 480, 640, 525.0
RADIUS, PLANE_Z, HALF = 0.3, -0.3, 0.64


def look_at(eye, target=(0.0, 0.0, -0.1), up=(0.0, 0.0, 1.0)):
    """OpenCV camera-to-world [4,4]"""
    eye, target, up = (np.asarray(x, np.float64) for x in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, eye
    return m


def uv_sphere(n=96, radius=RADIUS):
    th = np.linspace(0, np.pi, n + 1)[:, None]
    ph = np.linspace(0, 2 * np.pi, 2 * n, endpoint=False)[None]
    v = radius * np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th) * np.ones_like(ph)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n), np.arange(2 * n), indexing="ij")
    a, b = i * 2 * n + j, i * 2 * n + (j + 1) % (2 * n)
    t = np.concatenate([np.stack([a, a + 2 * n, b], -1).reshape(-1, 3), np.stack([b, a + 2 * n, b + 2 * n], -1).reshape(-1, 3)])
    return v.astype(np.float32), t.astype(np.int64)


def _stats(ms, digits=4):
    return dict(median=round(statistics.median(ms), digits), min=round(min(ms), digits), max=round(max(ms), digits))


def event_pass_ms(fn, reps, per):
    fn()
    pairs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    return _stats([a.elapsed_time(b) / per for a, b in pairs])


def wall_once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def bench_sparse(a, emit, dev, K, poses, depths, rgbs, order, dims, grow):
    """the rows of --store sparse for one cube size and one logical box"""
    vl = 2 * HALF / dims
    trunc = 2 * vl
    shift = (grow - 1) * (dims // 8) // 2                          # blocks: the cube sits in the middle of the logical box
    origin = tuple(-HALF - shift * 8 * vl for _ in range(3))
    ldims = (dims * grow,) * 3
    fx, fy, cx, cy = tsdf._intrinsics(K, "half")
    host = [geometry.pose_pair(p) for p in poses]
    views = sorted(set(order))
    need = tsdf.count_touched_blocks(K, [poses[f] for f in views], [depths[f] for f in views], None, origin, ldims, vl, trunc,
                                     pixel_centers="half", stride=4, device=dev)
    vol = tsdf.SparseTSDFVolume(vl, trunc, origin, ldims, max(need, 1), device=dev)
    box = vol._box()

    def touch_pass():
        for f in order:
            tsdf.launch("mh_tsdf_sparse_touch", tsdf.ptr(depths[f]), None, H, W, fx, fy, cx, cy, geometry.host_ptr(host[f][0]), 1.0, 10.0,
                        4, *box, vol.capacity, tsdf.ptr(vol.slot), tsdf.ptr(vol.slot_block), tsdf.ptr(vol.counters))

    def integrate_pass():
        for f in order:
            tsdf.launch("mh_tsdf_sparse_integrate", tsdf.ptr(depths[f]), tsdf.ptr(rgbs[f]), None, H, W, fx, fy, cx, cy,
                        geometry.host_ptr(host[f][1]), 1.0, 10.0, *box, vol.capacity, tsdf.ptr(vol.slot_block), tsdf.ptr(vol.counters),
                        tsdf.ptr(vol.tsdf), tsdf.ptr(vol.weight), tsdf.ptr(vol.color))

    touch = event_pass_ms(touch_pass, a.reps, a.frames)
    integ = event_pass_ms(integrate_pass, a.reps, a.frames)
    allocated = vol.check()
    nbytes = allocated * 512 * 40 + H * W * 7
    pool, dense = tsdf.sparse_bytes(ldims, vol.capacity), tsdf.volume_bytes(ldims)
    emit(dict(row="sparse_launch", dims=dims, logical_dims=ldims[0], voxel_length=round(vl, 6), allocated_blocks=allocated,
              allocated_share=round(allocated / (ldims[0] // 8) ** 3, 5), touch_ms=touch, integrate_ms=integ, integrate_bytes=int(nbytes),
              integrate_GB_per_s=round(nbytes / (integ["median"] * 1e-3) / 1e9, 1), pool_bytes=pool, dense_bytes=dense,
              pool_over_dense=round(pool / dense, 5)))
    del vol
    lo, hi = np.array(origin) + trunc, np.array(origin) + ldims[0] * vl - trunc - 0.5 * vl
    fuse = []
    for _ in range(3 + max(3, a.reps // 4)):
        ms, (m, vol) = wall_once(lambda: tsdf.run_tsdf_fusion(
            K, H, W, [poses[f] for f in order], [depths[f] for f in order], [rgbs[f] for f in order], bounds=(lo, hi),
            voxel_length=vl, sdf_trunc=trunc, pixel_centers="half", device=dev, return_volume=True, store="sparse"))
        fuse.append(ms)
    extract = [wall_once(vol.extract_mesh)[0] for _ in range(3 + a.reps)][3:]
    emit(dict(row="sparse_fusion", dims=dims, logical_dims=vol.dims[0], frames=a.frames, run_tsdf_fusion_ms=_stats(fuse[3:], 3),
              extract_mesh_ms=_stats(extract, 3), V=int(m["vertices"].shape[0]), T=int(m["triangles"].shape[0]),
              allocated_blocks=vol.check()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="256,512")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--store", default="dense", choices=tsdf.STORES)
    ap.add_argument("--grow", default="1,2", help="--store sparse: logical box sides, in multiples of the cube's")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"# tools/bench_tsdf.py: {a.frames} frames ({a.views} views cycled) of {W} x {H}; per-launch: a HIP event pair around "
             f"a pass over all frames / frames, 1 warm-up + {a.reps} passes, ms as median [min .. max]; wall rows: wall clock "
             f"between synchronisations", f"# device name reported by torch: {torch.cuda.get_device_name(0)}"]

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    sv, st = uv_sphere()
    e = 1.5
    qv = np.array([(-e, -e, PLANE_Z), (e, -e, PLANE_Z), (e, e, PLANE_Z), (-e, e, PLANE_Z)], np.float32)
    verts = torch.from_numpy(np.concatenate([sv, qv])).to(dev)
    tris = torch.from_numpy(np.concatenate([st, np.array([(0, 1, 2), (0, 2, 3)]) + len(sv)])).to(dev)
    cols = (0.5 + 0.5 * torch.sin(3.0 * verts + torch.tensor([0.0, 1.0, 2.0], device=dev))).contiguous()
    K = np.array([[FOCAL, 0, W / 2.0], [0, FOCAL, H / 2.0], [0, 0, 1.0]])
    poses, depths, rgbs = [], [], []
    for f in range(a.views):
        ang = 0.37 + 2 * np.pi * f / a.views
        c2w = look_at((1.2 * np.cos(ang), 1.2 * np.sin(ang), 0.5))
        out = meshrender.render_mesh(verts, tris, cols, c2w=c2w, K=K, H=H, W=W, convention="opencv", mode="color")
        poses.append(c2w), depths.append(out["depth"]), rgbs.append(tsdf.rgb8(out["image"], device=dev))
    order = [f % a.views for f in range(a.frames)]
    for dims in [int(x) for x in a.dims.split(",")]:
        vl = 2 * HALF / dims
        trunc = 2 * vl
        if a.store == "sparse":
            for grow in [int(x) for x in a.grow.split(",")]:
                bench_sparse(a, emit, dev, K, poses, depths, rgbs, order, dims, grow)
            continue
        box = dict(voxel_length=vl, sdf_trunc=trunc, origin=(-HALF, -HALF, -HALF), dims=(dims,) * 3, device=dev)
        vol = tsdf.TSDFVolume(**box)
        lib_args = (float(vol.origin[0]), float(vol.origin[1]), float(vol.origin[2]), vol.voxel_length, vol.sdf_trunc) + vol.blocks
        fx, fy, cx, cy = tsdf._intrinsics(K, "half")
        host = [geometry.pose_pair(p) for p in poses]

        def touch_pass():
            for f in order:
                tsdf.launch("mh_tsdf_touch", tsdf.ptr(depths[f]), None, H, W, fx, fy, cx, cy, geometry.host_ptr(host[f][0]), 1.0, 10.0, 4,
                            *lib_args, tsdf.ptr(vol.active))

        def integrate_pass():
            for f in order:
                tsdf.launch("mh_tsdf_integrate", tsdf.ptr(depths[f]), tsdf.ptr(rgbs[f]), None, H, W, fx, fy, cx, cy,
                            geometry.host_ptr(host[f][1]), 1.0, 10.0, *lib_args, tsdf.ptr(vol.active), tsdf.ptr(vol.tsdf),
                            tsdf.ptr(vol.weight), tsdf.ptr(vol.color))

        touch = event_pass_ms(touch_pass, a.reps, a.frames)
        integ = event_pass_ms(integrate_pass, a.reps, a.frames)
        share = float(vol.active.float().mean())
        nbytes = share * dims ** 3 * 40 + H * W * 7
        emit(dict(row="launch", dims=dims, voxel_length=round(vl, 6), active_share=round(share, 4), touch_ms=touch, integrate_ms=integ,
                  integrate_bytes=int(nbytes), integrate_GB_per_s=round(nbytes / (integ["median"] * 1e-3) / 1e9, 1)))
        del vol
        lo, hi = np.full(3, -HALF + trunc), np.full(3, HALF - trunc)
        fuse = []
        for _ in range(3 + max(3, a.reps // 4)):
            ms, (m, vol) = wall_once(lambda: tsdf.run_tsdf_fusion(
                K, H, W, [poses[f] for f in order], [depths[f] for f in order], [rgbs[f] for f in order], bounds=(lo, hi),
                voxel_length=vl, sdf_trunc=trunc, pixel_centers="half", device=dev, return_volume=True))
            fuse.append(ms)
        extract = [wall_once(vol.extract_mesh)[0] for _ in range(3 + a.reps)][3:]
        emit(dict(row="fusion", dims=vol.dims[0], frames=a.frames, run_tsdf_fusion_ms=_stats(fuse[3:], 3), extract_mesh_ms=_stats(extract, 3),
                  V=int(m["vertices"].shape[0]), T=int(m["triangles"].shape[0]), active_share=round(float(vol.active.float().mean()), 4)))
        ones = torch.ones_like(vol.weight)
        plain, masked, fused = [], [], []
        for k in range(3 + a.reps):
            p = wall_once(lambda: mesh.marching_cubes(vol.tsdf))[0]
            q = wall_once(lambda: mesh.marching_cubes_masked(vol.tsdf, ones))[0]
            r = wall_once(lambda: mesh.marching_cubes_masked(vol.tsdf, vol.weight))[0]
            if k >= 3:
                plain.append(p), masked.append(q), fused.append(r)
        emit(dict(row="marching_cubes", dims=vol.dims[0], unmasked_ms=_stats(plain, 3), masked_all_observed_ms=_stats(masked, 3),
                  masked_fused_weights_ms=_stats(fused, 3)))
        del vol, ones, m
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
