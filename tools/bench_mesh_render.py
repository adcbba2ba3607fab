"""Time mesh rendering (morpheus_amd.meshrender, csrc/raster.hip) against the stage it follows, extract_mesh.

    python tools/bench_mesh_render.py [--res 128,256] [--scales 1,4] [--reps 20] [--batch 50] [--out profiles/r08_mesh_render.txt]

Model `b`, a 512 x 512 view times `scale` (render_all_meshes renders at scale 1 for depths.npz and scale 4 for the videos).
Per (resolution, scale): 3 warm-up and --reps timed repetitions of every column, median [min .. max].  The C entry points run
10 - 100 us, near the resolution of an event pair, so one repetition is a pair of HIP events around --batch back-to-back calls
on the stream, divided by --batch (ms per call, launch gaps of a busy stream included, as in the frame loop).
  extract_ms   mesh.extract_mesh (wall per call, device synchronised before and after: it reads V, T on the host in the middle)
  normals_ms   mh_mesh_vertex_normals
  depth_ms     mh_raster_depth at the default small / large split; key_GBps = 8 H W bytes / depth_ms
  resolve_ms   mh_raster_resolve, mode shaded
and the sweep of the split (small_area) over depth_ms.  Kernel-level times: run this under rocprofv3 --kernel-trace --stats.
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

from morpheus_amd import _lib, geometry, harness, mesh, meshrender  # noqa: E402
from morpheus_amd._lib import check, ptr, stream  # noqa: E402

SWEEP = (16, 64, 256, 1024, 4096, 1 << 30)


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    eye, target, up = (np.asarray(x, np.float64) for x in (eye, target, up))
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, eye
    return m


BATCH = 50


def event_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    pairs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(BATCH):
            fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) / BATCH for a, b in pairs]
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def wall_ms(fn, warmup, reps):
    ms = []
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return dict(median=round(statistics.median(ms), 3), min=round(min(ms), 3), max=round(max(ms), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="128,256")
    ap.add_argument("--scales", default="1,4")
    ap.add_argument("--view", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    globals()["BATCH"] = max(1, a.batch)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    model = harness.build_model("b", dev)
    w2c = meshrender.world_to_camera(look_at((0.4, -2.4, 0.7)))
    w2c_p = geometry.host_ptr(w2c)
    lines = [f"# tools/bench_mesh_render.py: model b, {a.view} x {a.view} view x scale; every column 3 warm-up + {a.reps} timed "
             f"repetitions, ms per call as median [min .. max]; extract_ms: wall around one call; the others: HIP events around "
             f"{BATCH} calls / {BATCH}", f"# device name reported by torch: {torch.cuda.get_device_name(0)}"]
    for res in [int(r) for r in a.res.split(",")]:
        extract = wall_ms(lambda: mesh.extract_mesh(model, resolution=res), 3, a.reps)
        m = mesh.extract_mesh(model, resolution=res)
        v, col = m["vertices"], m["colors"].contiguous()
        tri = m["triangles"].to(torch.int32)
        V, T = v.shape[0], tri.shape[0]
        acc = torch.empty(3 * V + 1, dtype=torch.int64, device=dev)
        nrm = torch.empty(V, 3, device=dev)
        normals = event_ms(lambda: check(lib.mh_mesh_vertex_normals(ptr(v), V, ptr(tri), T, ptr(acc), ptr(nrm), stream()),
                                         "mh_mesh_vertex_normals"), 3, a.reps)
        for scale in [int(s) for s in a.scales.split(",")]:
            H = W = a.view * scale
            f = (W / 2) / 0.45
            ws = torch.empty(lib.mh_raster_workspace_bytes(H, W, T), dtype=torch.uint8, device=dev)
            clipped = torch.empty((), dtype=torch.int64, device=dev)
            depth = torch.empty(H, W, device=dev)
            tid = torch.empty(H, W, dtype=torch.int32, device=dev)
            img = torch.empty(H, W, 3, device=dev)

            def run_depth(small_area=0):
                check(lib.mh_raster_depth(ptr(v), V, ptr(tri), T, w2c_p, f, f, W / 2, H / 2, H, W, 0.01, small_area, ptr(ws),
                                          ptr(clipped), stream()), "mh_raster_depth")

            def run_resolve():
                check(lib.mh_raster_resolve(ptr(v), V, ptr(tri), T, ptr(col), ptr(nrm), w2c_p, f, f, W / 2, H / 2, H, W, 2, 0.3,
                                            1.0, 1.0, 1.0, ptr(ws), ptr(depth), ptr(tid), ptr(img), stream()), "mh_raster_resolve")

            d = event_ms(run_depth, 3, a.reps)
            r = event_ms(run_resolve, 3, a.reps)
            sweep = {str(s): event_ms(lambda s=s: run_depth(s), 3, a.reps)["median"] for s in SWEEP}
            covered = int((tid >= 0).sum())
            row = dict(res=res, V=V, T=T, scale=scale, H=H, W=W, covered=covered, clipped=int(clipped), extract_ms=extract,
                       normals_ms=normals, depth_ms=d, resolve_ms=r,
                       key_GBps=round(8.0 * H * W / (d["median"] * 1e-3) / 1e9, 1),
                       render_over_extract=round((d["median"] + r["median"] + normals["median"]) / extract["median"], 4),
                       mean_triangle_px=round(covered / max(T, 1), 2),
                       depth_ms_by_small_area=sweep)
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
