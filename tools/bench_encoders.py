"""Time the frequency and spherical-harmonics encoders (csrc/encoders.hip) forward and backward, beside the plain-torch frequency
chain the package used before (model._freq_encode_torch forward plus its autograd backward).

    python tools/bench_encoders.py [--points 2097152] [--reps 20] [--batch 10] [--out profiles/encoders_bench.txt]

FreqEncoder(3, 6), SHEncoder(3, 4) and SHEncoder(3, 8) at B = 2^21 points, straight at the C ABI (no allocation inside the timed
window): 5 warm-up windows, then --reps windows of --batch back-to-back launches between two device events, ms per launch as median
[min .. max]; clocks are left alone.
  bytes     what the kernel must move: the inputs read once and the outputs written once (frequency forward 4 B (D + C), backward
            4 B (D + C + D); SH forward 4 B (3 + degree^2), backward 4 B (3 + degree^2 + 3))
  TB_s      bytes over the median
  of_stream TB_s over STREAM_TB_S, the rate a float4 copy kernel reaches on this part (6.29 TB/s)
The torch chain runs the same input through _freq_encode_torch and backpropagates a ready-made gradient: 12 trigonometric launches
and a cat forward, about twice that backward, timed the same way with one forward + backward a launch "batch".
The expectation is written into the file before anything is measured.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from morpheus_amd._lib import launch, ptr  # noqa: E402
from morpheus_amd.model import _freq_encode_torch  # noqa: E402

STREAM_TB_S = 6.29
EXPECTATION = [
    "# expectation, written before the run:",
    "#  - all four kernels are streaming, 16 .. 268 bytes a point, and every wave's stores are whole lines: each should sit above",
    "#    half the copy rate.  What can hold one below it is arithmetic, not memory: one sincosf per (point, dimension, band) in",
    "#    the frequency kernels (38 M calls at 2^21 x 3 x 6), ~250 / ~700 fp32 operations a point in SH degree 8 forward / backward",
    "#  - SH degree 4 moves 160 .. 185 MB, less than the last-level cache holds: it may run above the copy rate",
    "#  - the torch chain moves each [B,3] block through its own launch and then through cat: several times the bytes, ~13 launches",
    "#    forward and ~25 backward; its time over the kernels' is the number that justifies them",
]


def _stats(ms, digits=4):
    return dict(median=round(statistics.median(ms), digits), min=round(min(ms), digits), max=round(max(ms), digits))


def event_ms(fn, reps, batch, warmup=5):
    for _ in range(warmup * batch):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B = a.points
    lines = [f"# tools/bench_encoders.py: B = {B} points; 5 warm-up + {a.reps} windows of {a.batch} launches between device events, "
             f"ms per launch as median [min .. max]; of_stream = TB_s / {STREAM_TB_S}",
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
    torch.manual_seed(0)
    x = torch.rand(B, 3, device=dev) * 2 - 1
    rows = {}

    def kernel(what, name, args, nbytes):
        ms = event_ms(lambda: launch(name, *args), a.reps, a.batch)
        tb_s = nbytes / (ms["median"] * 1e-3) / 1e12
        rows[what] = ms["median"]
        emit(dict(row="kernel", what=what, entry=name, ms=ms, MB=round(nbytes / 1e6, 1), TB_s=round(tb_s, 3), of_stream=round(tb_s / STREAM_TB_S, 3)))

    D, degree = 3, 6
    C = D + 2 * D * degree
    out, grad, gx = torch.empty(B, C, device=dev), torch.randn(B, C, device=dev), torch.empty(B, D, device=dev)
    kernel("FreqEncoder(3, 6) forward", "mh_freq_encode_fwd", (ptr(x), B, D, degree, degree, ptr(out)), 4 * B * (D + C))
    kernel("FreqEncoder(3, 6) backward", "mh_freq_encode_bwd", (ptr(x), ptr(grad), B, D, degree, degree, ptr(gx)), 4 * B * (D + C + D))
    for deg in (4, 8):
        C2 = deg * deg
        o, g = torch.empty(B, C2, device=dev), torch.randn(B, C2, device=dev)
        kernel(f"SHEncoder(3, {deg}) forward", "mh_sh_encode_fwd", (ptr(x), B, deg, ptr(o)), 4 * B * (3 + C2))
        kernel(f"SHEncoder(3, {deg}) backward", "mh_sh_encode_bwd", (ptr(x), ptr(g), B, deg, ptr(gx)), 4 * B * (3 + C2 + 3))
        del o, g

    xg = x.clone().requires_grad_(True)

    def torch_fwd():
        with torch.no_grad():
            _freq_encode_torch(x, degree)

    def torch_fwd_bwd():
        xg.grad = None
        _freq_encode_torch(xg, degree).backward(grad)

    fwd = event_ms(torch_fwd, a.reps, max(1, a.batch // 5))
    both = event_ms(torch_fwd_bwd, a.reps, max(1, a.batch // 5))
    emit(dict(row="torch", what="_freq_encode_torch forward (no grad)", ms=fwd))
    emit(dict(row="torch", what="_freq_encode_torch forward + autograd backward", ms=both))
    hip_both = rows["FreqEncoder(3, 6) forward"] + rows["FreqEncoder(3, 6) backward"]
    emit(dict(row="ratios", torch_forward_over_hip_forward=round(fwd["median"] / rows["FreqEncoder(3, 6) forward"], 1),
              torch_forward_backward_over_hip_forward_backward=round(both["median"] / hip_both, 1)))


if __name__ == "__main__":
    main()
