"""Time the pose initialisation (morpheus_amd.poseinit, csrc/poseinit.hip): one robust registration at the test's size and at a
frame's size, its pieces, the back-projection, and the same algorithm on the host with a KD-tree.

    python tools/bench_pose_init.py [--points 50000] [--reps 20] [--batch 20] [--no-cpu] [--out profiles/r15_pose_init.txt]

The expectations below are written into the file BEFORE anything is measured.  These are records, not gates: the reference hands
this stage to an external program (FRICP) that was never available, so there is no time of its to hold them against.
  registration rows  wall clock between two device synchronisations (the host waits once per iteration inside), min of 3;
                     ms_per_iteration = that / iterations
  piece rows         3 warm-up + --reps repetitions, median [min .. max] in ms: nearest and knn_d2 as one HIP event pair per
                     call, the short entry points as an event pair around --batch calls / --batch
  cpu column         the oracle's algorithm (tests/poseinit_oracle.py: the same schedule, sums and stopping rule) with scipy's
                     cKDTree for the correspondences and the spacing, on the same host, min of 3
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

from morpheus_amd import mesheval, poseinit  # noqa: E402
from tests import mesheval_oracle as mo  # noqa: E402
from tests import poseinit_oracle as po  # noqa: E402

EXPECTATIONS = """# expectations, written before the run:
#   an iteration = one nearest at the size (profiles/r09_mesh_eval.txt: 4.0-4.6e12 pairs/s, so 0.54-0.63 ms at 50 000 x 50 000 and
#     launch-bound, ~0.02 ms, at 1 500 x 1 200) + mh_icp_transform (one launch) + mh_icp_wsums (two launches; 5e4 points x 28 bytes
#     read, 19 float64 sums: launch-bound) + one host wait with a 152-byte copy (~0.03-0.05 ms) + numpy's 3 x 3 SVD (~0.03 ms):
#     expected 0.65-0.8 ms per iteration at 50 000 points, ~0.15 ms (all overhead) at the test's 1 500
#   mh_knn_d2 at 50 000 points: the same 2.5e9 pairs as one nearest, but unsegmented (196 workgroups on 256 CUs, one wavefront per
#     SIMD) and with the list insertion: expected 2-4 ms, once per registration
#   a registration takes 70-180 iterations over 6 stages (the CPU study: 102-174): expected 50-140 ms at 50 000 points
#   a 200-frame sequence at 5e4 points per frame = 199 registrations + 200 back-projections (three launches and one host wait
#     each, ~0.1 ms): expected 10-30 s, all of it the nearest-neighbour search
#   the host column: a KD-tree query of 5e4 points costs ~25-35 ms (r09: 35 ms build + query), so ~100x the device per iteration"""


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


def cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def case(n, seed=po.ROBUST_SEED):
    """tests/poseinit_oracle.robust_case at n source points"""
    return po.robust_case(seed, 15.0, n)


def cpu_robust_icp(source, target, nu_begin_k=3.0, nu_end_k=po.NU_END_K, nu_alpha=0.5, knn=7, max_icp=100, stop=1e-5):
    """po.robust_icp with a KD-tree in place of the brute-force searches (distances in float64: not bit-comparable, same method)"""
    from scipy.spatial import cKDTree
    tree = cKDTree(target.astype(np.float64))
    spacing = tree.query(target.astype(np.float64), k=knn)[0][:, 1:]
    nu_end = nu_end_k * float(np.median(np.median(spacing, axis=1)))
    scale = max(po._diagonal(source), po._diagonal(target))
    T = np.eye(4)

    def correspond():
        moved = mo.transform_points(source, T)
        d, idx = tree.query(moved.astype(np.float64))
        return moved, idx.astype(np.int32), (d * d).astype(np.float32)

    moved, idx, d2 = correspond()
    nu = max(nu_begin_k * float(np.median(np.sqrt(d2.astype(np.float64)))), nu_end)
    iterations = stages = 0
    while True:
        stages += 1
        for _ in range(max_icp):
            s = po.icp_wsums(moved, target, idx, d2, 1.0 / (2.0 * nu * nu))
            T_new = mo.kabsch_update(s[:17]) @ T
            iterations += 1
            delta = T_new - T
            delta[:3, 3] /= scale
            T = T_new
            moved, idx, d2 = correspond()
            if np.linalg.norm(delta) < stop:
                break
        if nu == nu_end:
            break
        nu = max(nu * nu_alpha, nu_end)
    return {"transformation": T, "iterations": iterations, "stages": stages}


def registration_row(n, dev, with_cpu):
    source, target, T_true = case(n)
    s, t = torch.from_numpy(source).to(dev), torch.from_numpy(target).to(dev)
    poseinit.robust_icp(s, t)                                      # warm-up
    best = None
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = poseinit.robust_icp(s, t)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    rot, trans = po.pose_error(res["transformation"], T_true)
    row = dict(row="registration", source=source.shape[0], target=target.shape[0], iterations=res["iterations"], stages=res["stages"],
               converged=res["converged"], ms=round(best, 2), ms_per_iteration=round(best / max(res["iterations"], 1), 4),
               rotation_error_deg=round(rot, 5), translation_error=float(f"{trans:.3g}"))
    if with_cpu:
        cpu_best = None
        for _ in range(3):
            t0 = time.perf_counter()
            cpu = cpu_robust_icp(source, target)
            ms = (time.perf_counter() - t0) * 1e3
            cpu_best = ms if cpu_best is None else min(cpu_best, ms)
        rot, trans = po.pose_error(cpu["transformation"], T_true)
        row.update(cpu_ms=round(cpu_best, 1), cpu_iterations=cpu["iterations"], cpu_ms_per_iteration=round(cpu_best / cpu["iterations"], 3),
                   cpu_rotation_error_deg=round(rot, 5), cpu_over_gpu=round(cpu_best / best, 1))
    return row, (s, t)


def pieces_row(s, t, reps, batch):
    T = np.eye(4)
    moved = mesheval.transform_points(s, T)
    idx, d2 = mesheval.nearest(moved, t)
    inv = 1.0 / (2.0 * 0.05 ** 2)
    near = event_ms(lambda: mesheval.nearest(moved, t), 3, reps)
    return dict(row="pieces", source=s.shape[0], target=t.shape[0], nearest_ms=near,
                nearest_pairs_per_s=float(f"{s.shape[0] * t.shape[0] / (near['median'] * 1e-3):.4g}"),
                knn_d2_k6_ms=event_ms(lambda: poseinit.knn_d2(t, 6), 3, reps),
                transform_ms=event_ms(lambda: mesheval.transform_points(s, T), 3, reps, batch),
                wsums_ms=event_ms(lambda: poseinit.icp_wsums(moved, t, idx, d2, inv), 3, reps, batch),
                sums_ms=event_ms(lambda: mesheval.icp_sums(moved, t, idx, d2), 3, reps, batch))


def depth_points_row(dev, reps):
    H, W = 480, 640
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    depth = torch.rand(H, W, generator=g, device=dev) + 0.5
    v, u = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    mask = ((((u - 320.0) / 150.0) ** 2 + ((v - 240.0) / 110.0) ** 2) < 1.0).to(torch.uint8).contiguous()
    K = np.array([[525.0, 0, 319.5], [0, 525.0, 239.5], [0, 0, 1]])
    ms = []
    for k in range(3 + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pts = poseinit.depth_points(depth, mask, K)
        torch.cuda.synchronize()
        if k >= 3:
            ms.append((time.perf_counter() - t0) * 1e3)
    return dict(row="depth_points", H=H, W=W, points=pts.shape[0], ms=_stats(ms, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"# tools/bench_pose_init.py: the outlier case of tests/poseinit_oracle.robust_case at 1500 and {a.points} source points; "
             f"registrations: wall clock, min of 3; pieces: 3 warm-up + {a.reps} repetitions, ms as median [min .. max]",
             f"# device name reported by torch: {torch.cuda.get_device_name(0)}; CPU of the host column: {cpu_model()}",
             EXPECTATIONS, "# measured:"]
    if a.out:                                                      # the expectations are on disk before the first measurement
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(lines[-1] + "\n")

    emit(depth_points_row(dev, a.reps))
    frame = None
    for n in (1500, a.points):
        row, (s, t) = registration_row(n, dev, not a.no_cpu)
        emit(row)
        emit(pieces_row(s, t, a.reps, a.batch))
        frame = row
    emit(dict(row="sequence, extrapolated", frames=200, registrations=199, points=a.points,
              seconds=round(199 * frame["ms"] * 1e-3, 1), note="199 x the registration above; not a run of 200 frames"))


if __name__ == "__main__":
    main()
