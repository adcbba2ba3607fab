"""Device time of the preprocessing launch (csrc/preprocess.hip) for one sequence, beside the oracle's numpy loop on the host.

    python tools/bench_preprocess.py [--frames 200] [--reps 1000] [--out FILE]

The sequence has the size of the bundled snoopy one: 200 frames of 480 x 640 cut to 360 x 360, windows scattered about the frame's
centre so that some leave it.  Timed with device events around five windows of `reps` / 5 launches of the entry point into fixed
output buffers, after a warm-up (unrotated, and rotated by 37.5 degrees; median, minimum and maximum are reported); the bytes are the ones the definition needs, counted from the shapes: 6 bytes read per window pixel that falls inside the
frame and 7 written per window pixel (the 256 KB of depth tables stay in cache).  The share of the memory rate is those bytes over the
device time over 6.29 TB/s, the rate a float4 copy reaches on an MI355X (8.0 TB/s is the specification).  The host figure is
tests/preprocess_oracle.prep_frames on the same frames, and its planes are compared with the device's.  Needs an MI355X.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from morpheus_amd import ops  # noqa: E402
from tests import preprocess_oracle as P  # noqa: E402

COPY_RATE = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_preprocess needs the GPU: there is no CPU path to time"
    dev = "cuda"
    F, H, W, h, w = a.frames, 480, 640, 360, 360
    gen = torch.Generator(device=dev).manual_seed(1)
    rgb = torch.randint(0, 256, (F, H, W, 3), device=dev, dtype=torch.uint8, generator=gen)
    depth = torch.randint(0, 6000, (F, H, W), device=dev, dtype=torch.int32, generator=gen).to(torch.uint16)
    mask = torch.randint(0, 2, (F, H, W), device=dev, dtype=torch.uint8, generator=gen) * 255
    rng = np.random.default_rng(2)
    centres = np.stack([rng.integers(250, 390, F), rng.integers(150, 330, F)], -1)
    origin = P.window_origins(centres, h, w)
    tabs = P.depth_tables(1000.0, 1.0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    origin_d, tin, tpad = t(origin.astype(np.int32)), t(tabs[0]), t(tabs[1])
    Y0, X0 = np.clip(origin[:, 0], 0, H), np.clip(origin[:, 1], 0, W)
    Y1, X1 = np.clip(origin[:, 0] + h, 0, H), np.clip(origin[:, 1] + w, 0, W)
    inside_px = int(((Y1 - Y0) * (X1 - X0)).sum())
    moved = 6 * inside_px + 7 * F * h * w
    res = dict(frames=F, frame=[H, W], window=[h, w], reps=a.reps, bytes_moved=moved, windows_not_inside=sum(P.window_kind(t_, l_, h, w, H, W) != "inside" for t_, l_ in origin))
    for name, deg in (("unrotated", 0.0), ("rotated_37.5", 37.5)):
        inv = t(np.stack([P.invert_affine(P.rotation_matrix(c, deg)) for c in centres]))
        rot = torch.full((F,), int(deg != 0.0), dtype=torch.uint8, device=dev)
        out = ops.prep_frames(rgb, depth, mask, origin_d, inv, rot, tin, tpad, h, w)
        # the timed launches write the same four buffers again: the entry point itself, no allocation between the launches
        args = [ops.ptr(v) for v in (rgb, depth, mask)] + [F, H, W] + [ops.ptr(v) for v in (origin_d, inv, rot, tin, tpad)] + [h, w] + \
               [ops.ptr(out[k]) for k in ("rgb", "depth", "mask", "padding")]
        for _ in range(10):
            ops.launch("mh_prep_frames", *args)
        torch.cuda.synchronize()
        windows = []
        for _ in range(5):      # five windows of reps / 5 launches: the median, and the spread beside it
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(max(1, a.reps // 5)):
                ops.launch("mh_prep_frames", *args)
            e1.record()
            torch.cuda.synchronize()
            windows.append(e0.elapsed_time(e1) / max(1, a.reps // 5))
        ms = float(np.median(windows))
        res[name] = dict(device_ms_per_sequence=ms, min_ms=min(windows), max_ms=max(windows), bytes_per_s=moved / (ms * 1e-3),
                         share_of_copy_rate=moved / (ms * 1e-3) / COPY_RATE)
        if deg == 0.0:
            host = [v.cpu().numpy() for v in (rgb, depth, mask)]
            t0 = time.perf_counter()
            want = P.prep_frames(*host, origin, np.zeros((F, 6)), np.zeros(F, np.uint8), *tabs, h, w)
            res["host_numpy_loop_ms_per_sequence"] = (time.perf_counter() - t0) * 1e3
            res["device_equals_host"] = all(np.array_equal(out[k].cpu().numpy(), want[k]) for k in want)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"# tools/bench_preprocess.py: {F} frames of {H} x {W} cut to {h} x {w}; 10 warm-up launches, then 5 windows of "
                    f"{max(1, a.reps // 5)} launches between device events (median, min, max ms per sequence); bytes counted from the "
                    f"shapes; share of {COPY_RATE / 1e12} TB/s (a float4 copy)\n# device name reported by torch: "
                    f"{torch.cuda.get_device_name(0)}\n" + line + "\n")


if __name__ == "__main__":
    main()
