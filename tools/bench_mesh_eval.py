"""Time the mesh evaluation (morpheus_amd.mesheval, csrc/mesheval.hip) against the stage before it, extract_mesh, and against
the reference's route for the same point sets, a CPU KD-tree.

    python tools/bench_mesh_eval.py [--res 128,256] [--reps 20] [--batch 20] [--target 300000] [--out profiles/r09_mesh_eval.txt]

Model `b`.  Every column: 3 warm-up + --reps timed repetitions, median [min .. max] in ms.  mh_nn_search runs for a
millisecond or more and is timed as one HIP event pair per call; the entry points shorter than ~0.1 ms (mh_cull_*,
mh_mesh_area_weights + mh_sample_surface, mh_icp_transform, mh_icp_sums) as an event pair around --batch back-to-back calls,
divided by --batch.  The calls that wait for the device in the middle (cull_mesh, sample_surface, an ICP iteration, mesh_metrics,
extract_mesh) are timed by the wall clock between two device synchronisations.
  nearest rows   Nq x Nr, ms, pairs/s, and valu_fraction = pairs/s x VALU_PER_PAIR / FP32_LANE_OPS_PER_S: the share of the
                 part's fp32 VALU issue rate the search keeps busy -- VALU issue is what bounds it (no memory traffic to speak
                 of: a tile is read from LDS as broadcasts)
  cpu_kdtree_ms  scipy's cKDTree build + query for the same sets (min of 3), where scipy is installed; ratio = that / nearest
"""
from __future__ import annotations

import argparse
import json
import os
import platform
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from morpheus_amd import harness, mesh, mesheval  # noqa: E402

# vector-ALU instructions per (query, reference point) pair in nn_search_kernel's inner loop, counted in the gfx950
# disassembly: 3 v_sub, 3 v_mul, 2 v_add, 1 v_cmp, 2 v_cndmask, and one v_mov / v_add of the index per four pairs
VALU_PER_PAIR = 11.25
# 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz: unpacked fp32 lane operations per second (a wave64 VALU instruction issues in 2 cycles)
FP32_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    eye, target, up = (np.asarray(x, np.float64) for x in (eye, target, up))
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, eye
    return m


def _stats(ms, digits=4):
    return dict(median=round(statistics.median(ms), digits), min=round(min(ms), digits), max=round(max(ms), digits))


def event_ms(fn, warmup, reps, batch=1):
    for _ in range(warmup):
        fn()
    pairs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    return _stats([a.elapsed_time(b) / batch for a, b in pairs])


def wall_ms(fn, warmup, reps):
    ms = []
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return _stats(ms, 3)


def cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def kdtree_ms(q, r):
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return None
    qh, rh = q.cpu().numpy().astype(np.float64), r.cpu().numpy().astype(np.float64)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        cKDTree(rh).query(qh)
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return round(best, 2)


def nearest_row(name, q, r, reps, with_cpu=True):
    t = event_ms(lambda: mesheval.nearest(q, r), 3, reps)
    pairs = q.shape[0] * r.shape[0]
    rate = pairs / (t["median"] * 1e-3)
    row = dict(row="nearest", what=name, Nq=q.shape[0], Nr=r.shape[0], ms=t, pairs_per_s=float(f"{rate:.4g}"),
               valu_fraction=round(rate * VALU_PER_PAIR / FP32_LANE_OPS_PER_S, 3))
    cpu = kdtree_ms(q, r) if with_cpu else None
    if cpu is not None:
        row.update(cpu_kdtree_ms=cpu, cpu_over_gpu=round(cpu / t["median"], 2))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="128,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--target", type=int, default=300000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    lines = [f"# tools/bench_mesh_eval.py: model b; 3 warm-up + {a.reps} timed repetitions, ms as median [min .. max]; nearest: one "
             f"HIP event pair per call; short entry points: an event pair around {a.batch} calls / {a.batch}; calls that wait for "
             f"the device inside: wall clock between synchronisations",
             f"# device name reported by torch: {torch.cuda.get_device_name(0)}; CPU of the KD-tree column: {cpu_model()}",
             f"# valu_fraction = pairs/s x {VALU_PER_PAIR} VALU instructions per pair / {FP32_LANE_OPS_PER_S:.4g} fp32 lane ops/s"]

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    q = torch.rand(50000, 3, generator=g, device=dev) * 2 - 1
    r = torch.rand(50000, 3, generator=g, device=dev) * 2 - 1
    emit(nearest_row("50k x 50k", q, r, a.reps))
    target = torch.rand(a.target, 3, generator=g, device=dev) * 2 - 1
    model = harness.build_model("b", dev)
    H, W = 480, 640
    K = np.array([[525.0, 0, 320.0], [0, 525.0, 240.0], [0, 0, 1]])
    c2w = look_at((0.4, -2.4, 0.7))
    depth_gt = torch.full((H, W), 2.0, device=dev)
    motion = np.eye(4)
    motion[:3, 3] = (0.01, -0.006, 0.004)
    for res in [int(x) for x in a.res.split(",")]:
        extract = wall_ms(lambda: mesh.extract_mesh(model, resolution=res), 3, a.reps)
        m = mesh.extract_mesh(model, resolution=res)
        v, tri, col = m["vertices"], m["triangles"], m["colors"].contiguous()
        emit(nearest_row(f"vertices of the {res}^3 mesh x {a.target} target points", v, target, a.reps))
        cull = wall_ms(lambda: mesheval.cull_mesh(v, tri, col, c2w=c2w, K=K, H=H, W=W, depth_gt=depth_gt), 3, a.reps)
        culled = mesheval.cull_mesh(v, tri, col, c2w=c2w, K=K, H=H, W=W, depth_gt=depth_gt)
        cv, ct = culled["vertices"], culled["triangles"]
        sample = wall_ms(lambda: mesheval.sample_surface(cv, ct, 50000), 3, a.reps)
        gt = {"vertices": mesheval.transform_points(cv, motion), "triangles": ct}
        T = np.eye(4)

        def icp_iteration():
            moved = mesheval.transform_points(cv, T)
            idx, d2 = mesheval.nearest(moved, gt["vertices"], max_dist=0.1)
            return mesheval.icp_sums(moved, gt["vertices"], idx, d2).cpu()

        icp_it = wall_ms(icp_iteration, 3, a.reps)
        moved = mesheval.transform_points(cv, T)
        idx, d2 = mesheval.nearest(moved, gt["vertices"], max_dist=0.1)
        small = dict(transform_ms=event_ms(lambda: mesheval.transform_points(cv, T), 3, a.reps, a.batch),
                     sums_ms=event_ms(lambda: mesheval.icp_sums(moved, gt["vertices"], idx, d2), 3, a.reps, a.batch),
                     area_weights_ms=event_ms(lambda: mesheval.area_weights(cv, ct), 3, a.reps, a.batch))
        icp = mesheval.icp_align(cv, gt["vertices"])
        plain = wall_ms(lambda: mesheval.mesh_metrics(culled, gt, align=False), 3, a.reps)
        aligned = wall_ms(lambda: mesheval.mesh_metrics(culled, gt, align=True), 3, max(3, a.reps // 4))
        emit(dict(row="frame", res=res, V=v.shape[0], T=tri.shape[0], culled_V=cv.shape[0], culled_T=ct.shape[0],
                  extract_ms=extract, cull_mesh_ms=cull, sample_surface_50k_ms=sample, icp_iteration_ms=icp_it,
                  icp_iterations=icp["iterations"], mesh_metrics_ms=plain, mesh_metrics_aligned_ms=aligned, **small,
                  scores_over_extract=round((cull["median"] + plain["median"]) / extract["median"], 3),
                  aligned_scores_over_extract=round((cull["median"] + aligned["median"]) / extract["median"], 3)))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
