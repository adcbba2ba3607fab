"""Time mesh export (morpheus_amd.mesh) on the benchmark model: SDF query, marching cubes, colour query, PLY write.

    python tools/bench_mesh.py [--res 128,256,512] [--reps 5] [--out profiles/r07_mesh_export.txt]

Per resolution (S = 128, t = None, as export_mesh's defaults): the median over --reps runs, after one warm-up, of the wall
time (device synchronised before and after) of
  query_ms   sdf_volume (model.density over res^3 points in S^3 sub-grids)
  mc_ms      marching_cubes (mh_mc_count + the host read of V, T + mh_mc_emit)
  color_ms   model.density at the V vertices (albedo)
  ply_ms     write_ply to a temporary file (device-to-host copy included)
and V, T.  mc / query is the issue's budget (<= 10 %).  Kernel-level times: run this under rocprofv3 --kernel-trace --stats.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from morpheus_amd import harness, mesh  # noqa: E402


def timed(fn):
    """-> (fn(), wall ms between two device synchronisations): marching_cubes waits for V, T on the host in the middle, so
    its cost is a wall time, and the other stages are measured the same way"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def run(model, res, S, tmpdir):
    sdf, q = timed(lambda: mesh.sdf_volume(model, res, S))
    (v, t), m = timed(lambda: mesh.marching_cubes(sdf, 0.0))
    v = v / (res - 1.0) * 2 - 1
    with torch.no_grad():
        col, c = timed(lambda: model.density(v, t=None)["albedo"])
    h0 = time.perf_counter()
    mesh.write_ply(os.path.join(tmpdir, f"mesh_{res}.ply"), v, t, col)
    p = (time.perf_counter() - h0) * 1e3
    return dict(query_ms=q, mc_ms=m, color_ms=c, ply_ms=p, V=v.shape[0], T=t.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="128,256,512")
    ap.add_argument("--S", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    model = harness.build_model("b", dev)
    lines = [f"# tools/bench_mesh.py: wall ms of the extract_mesh stages on harness.build_model('b'), S={a.S}, t=None, median of {a.reps}",
             f"# device: {torch.cuda.get_device_name(0)}"]
    with tempfile.TemporaryDirectory() as tmp:
        for res in [int(r) for r in a.res.split(",")]:
            run(model, res, a.S, tmp)                                    # warm-up
            rows = [run(model, res, a.S, tmp) for _ in range(a.reps)]
            r = {k: (statistics.median(x[k] for x in rows) if k.endswith("_ms") else rows[0][k]) for k in rows[0]}
            r = {"res": res, **{k: (round(x, 3) if isinstance(x, float) else x) for k, x in r.items()}}
            r["mc_over_query"] = round(r["mc_ms"] / r["query_ms"], 4)
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
