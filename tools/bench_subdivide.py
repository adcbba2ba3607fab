"""Time the subdivision to a maximum edge (morpheus_amd.mesheval.subdivide_to_size, csrc/subdivide.hip) and the finer cull it
feeds, against the stage before them, extract_mesh.

    python tools/bench_subdivide.py [--res 256] [--coarse 32] [--reps 20] [--max-edge 0.01] [--out profiles/r13_subdivide.txt]

Model `b`.  Every figure: 3 warm-up + --reps timed repetitions, median [min .. max] in ms.  The two passes (mh_subdiv_count,
mh_subdiv_emit with colours and the parent index, into buffers allocated once) run for tens of microseconds at these sizes and are
timed as an event pair around --batch back-to-back calls, divided by --batch (the row at max_edge / 4, long enough to time a
write stream at all: one event pair per call); the calls that wait for the device in the middle (subdivide_to_size, cull_mesh, extract_mesh) by the wall clock between two device
synchronisations.
  written_bytes   what mh_subdiv_emit stores: 24 B per output vertex (position and colour), 16 B per output triangle (three
                  int32 and the parent index); written_TB_s = that / the emit pass's median
  count_GB_s      68 B per input triangle (three indices, nine gathered coordinates read; depth and two counts written)
  rows "mesh"     the --res^3 export, the same at max_edge / 4, and the --coarse^3 export (coarse enough to reach depth >= 4)
  rows "cull"     cull_mesh on the same frame with and without subdivide, beside extract_mesh of the same mesh
The expectation is written into the file before anything is measured.
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

from morpheus_amd import harness, mesh, mesheval  # noqa: E402
from morpheus_amd._lib import launch, ptr  # noqa: E402

EXPECTATION = [
    "# expectation, written before the run:",
    "#  - mh_subdiv_emit is a write stream (no reuse, a few cached reads per output): its written bytes per second are held against",
    "#    the 0.8 TB/s that the marching-cubes count pass reached at 256^3 (profiles/r07_mesh_export.txt); at or above: met",
    "#  - subdivision plus the finer cull of a frame should stay below that frame's extract_mesh (profiles/r09_mesh_eval.txt: 31.3 ms",
    "#    median at 256^3, 2.5 ms at 128^3); nobody has measured this before",
]


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


def passes_row(name, m, max_edge, reps, batch):
    """the two passes on one mesh, launched as subdivide_to_size launches them, into buffers allocated once"""
    v, col = m["vertices"], m["colors"].contiguous()
    tri = m["triangles"].to(torch.int32)
    dev = v.device
    V, T = v.shape[0], tri.shape[0]
    depth = torch.empty(T, dtype=torch.int32, device=dev)
    counts = torch.empty(2, T, dtype=torch.int64, device=dev)

    def count():
        launch("mh_subdiv_count", ptr(v), V, ptr(tri), T, float(max_edge), 10, ptr(depth), ptr(counts[0]), ptr(counts[1]))

    count_ms = event_ms(count, 3, reps, batch)
    starts = torch.zeros(2, T + 1, dtype=torch.int64, device=dev)
    starts[:, 1:] = torch.cumsum(counts, 1)
    n_new, n_tri = int(starts[0, T]), int(starts[1, T])
    out_v = torch.empty(V + n_new, 3, dtype=torch.float32, device=dev)
    out_c = torch.empty_like(out_v)
    out_t = torch.empty(n_tri, 3, dtype=torch.int32, device=dev)
    index = torch.empty(n_tri, dtype=torch.int32, device=dev)

    def emit():
        launch("mh_subdiv_emit", ptr(v), ptr(col), V, ptr(tri), T, ptr(depth), ptr(starts[0]), ptr(starts[1]), n_new, n_tri,
               ptr(out_v), ptr(out_c), ptr(out_t), ptr(index))

    emit_ms = event_ms(emit, 3, reps, batch)
    whole = wall_ms(lambda: mesheval.subdivide_to_size(v, m["triangles"], col, max_edge=max_edge), 3, reps)
    written = (V + n_new) * 24 + n_tri * 16
    return dict(row="mesh", what=name, max_edge=max_edge, V=V, T=T, depths=torch.bincount(depth).tolist(), out_V=V + n_new, out_T=n_tri,
                count_ms=count_ms, count_GB_s=round(T * 68 / (count_ms["median"] * 1e-3) / 1e9, 1),
                emit_ms=emit_ms, written_bytes=written, written_TB_s=round(written / (emit_ms["median"] * 1e-3) / 1e12, 3),
                subdivide_to_size_ms=whole)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--coarse", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--max-edge", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"# tools/bench_subdivide.py: model b, max_edge {a.max_edge}; 3 warm-up + {a.reps} timed repetitions, ms as median "
             f"[min .. max]; the two passes: an event pair around {a.batch} calls / {a.batch} (max_edge / 4: one pair per call); calls that wait for the device inside: wall clock between "
             f"synchronisations",
             f"# device name reported by torch: {torch.cuda.get_device_name(0)}"] + EXPECTATION

    def flush():
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        flush()

    flush()                                                          # the expectation is on file before the first measurement
    model = harness.build_model("b", dev)
    H, W = 480, 640
    K = np.array([[525.0, 0, 320.0], [0, 525.0, 240.0], [0, 0, 1]])
    c2w = look_at((0.4, -2.4, 0.7))
    depth_gt = torch.full((H, W), 2.0, device=dev)
    for name, res in ((f"{a.res}^3 export", a.res), (f"{a.coarse}^3 export (coarse)", a.coarse)):
        m = mesh.extract_mesh(model, resolution=res, S=min(res, 128))
        emit(passes_row(name, m, a.max_edge, a.reps, a.batch))
        if res == a.res:                                             # the same mesh two depths further: a stream long enough to time
            emit(passes_row(name + ", max_edge / 4", m, a.max_edge / 4, a.reps, 1))
        v, tri, col = m["vertices"], m["triangles"], m["colors"].contiguous()
        kw = dict(c2w=c2w, K=K, H=H, W=W, depth_gt=depth_gt)
        extract = wall_ms(lambda: mesh.extract_mesh(model, resolution=res, S=min(res, 128)), 3, a.reps)
        plain = wall_ms(lambda: mesheval.cull_mesh(v, tri, col, **kw), 3, a.reps)
        fine = wall_ms(lambda: mesheval.cull_mesh(v, tri, col, subdivide=True, max_edge=a.max_edge, **kw), 3, a.reps)
        kept, kept_fine = mesheval.cull_mesh(v, tri, col, **kw), mesheval.cull_mesh(v, tri, col, subdivide=True, max_edge=a.max_edge, **kw)
        emit(dict(row="cull", what=name, extract_ms=extract, cull_mesh_ms=plain, cull_mesh_subdivide_ms=fine,
                  kept_T=kept["triangles"].shape[0], kept_T_subdivide=kept_fine["triangles"].shape[0],
                  subdivide_cull_over_extract=round(fine["median"] / extract["median"], 3),
                  below_extract=bool(fine["median"] < extract["median"])))


if __name__ == "__main__":
    main()
