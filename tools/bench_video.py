"""Time morpheus_amd.video.encode_jpeg on one MI355X against what a caller had to do without it: copy the raw uint8 frames to
the host and run PIL's JPEG encoder there.

    python tools/bench_video.py [--out profiles/video_bench.json] [--frames 8] [--repeats 7] [--inner 20]

Per case -- 360 x 360 and 1440 x 1440 (render_all_meshes' default scale of 4), RGB 4:2:0 and one component, a rendered-looking
frame (smooth shading and a hard edge, tests/video_oracle.shaded) and uniform noise as the worst case, quality 90 -- a batch
of --frames frames is coded in --repeats windows of --inner calls each, after a warm-up:
    hip_ms_per_frame     host clock around encode_jpeg: nine launches, the read of the F counts, the one device-to-host copy
                         of the used bytes and the assembly of the files; the call ends in that copy, so the clock sees all of it
    device_ms_per_frame  device events around the nine launches alone (video.encode_scans)
    pil_ms_per_frame     frames.cpu() and PIL.Image.save(format="JPEG", quality=, subsampling=, optimize=False) on a pool of at
                         most 16 threads (PIL releases the interpreter lock while it codes)
each the median over the repeats, with the lowest and the highest beside it.  Nothing is gated on these figures.
"""
import argparse
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from morpheus_amd import video  # noqa: E402
from tests import video_oracle as vo  # noqa: E402

QUALITY = 90
THREADS = min(16, os.cpu_count() or 1)


def content(kind, side, channels, frames):
    if kind == "noise":
        return vo.noise((frames, side, side, 3)[:4 if channels == 3 else 3], 1)
    base = vo.shaded(side, side)
    out = np.stack([np.roll(base, 3 * k, axis=1) for k in range(frames)])                   # the frames differ, as a video's do
    return out if channels == 3 else np.ascontiguousarray(out[..., 1])


def spread(fn, repeats, inner, warmup=3):
    """-> (median, lowest, highest) ms per call over `repeats` windows of `inner` calls each, after `warmup` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3 / inner)
    return statistics.median(times), min(times), max(times)


def device_spread(fn, repeats, inner):
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed window")
    ap.add_argument("--sides", type=int, nargs="*", default=[360, 1440])
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    pool = ThreadPoolExecutor(THREADS)
    result = dict(device=torch.cuda.get_device_name(0), frames=a.frames, repeats=a.repeats, inner=a.inner, quality=QUALITY,
                  threads=THREADS, cases=[])
    for side in a.sides:
        for channels in (3, 1):
            for kind in ("shaded", "noise"):
                host = content(kind, side, channels, a.frames)
                frames = torch.from_numpy(host).to(dev)
                sizes = {}

                def hip():
                    sizes["hip"] = sum(map(len, video.encode_jpeg(frames, QUALITY, "420")))

                def one(frame):
                    b = io.BytesIO()
                    Image.fromarray(frame).save(b, format="JPEG", quality=QUALITY, subsampling=2, optimize=False)
                    return b.tell()

                def pil():
                    sizes["pil"] = sum(pool.map(one, frames.cpu().numpy()))

                rec = dict(side=side, channels=channels, content=kind)
                for name, (med, lo, hi) in (("hip", spread(hip, a.repeats, a.inner)), ("pil", spread(pil, a.repeats, a.inner)),
                                            ("device", device_spread(lambda: video.encode_scans(frames, QUALITY, "420"), a.repeats,
                                                                     a.inner))):
                    rec[f"{name}_ms_per_frame"] = round(med / a.frames, 4)
                    rec[f"{name}_ms_per_frame_range"] = [round(lo / a.frames, 4), round(hi / a.frames, 4)]
                rec["hip_frames_per_s"] = round(1e3 / rec["hip_ms_per_frame"], 1)
                rec["pil_frames_per_s"] = round(1e3 / rec["pil_ms_per_frame"], 1)
                rec["bytes_per_frame"] = dict(hip=sizes["hip"] // a.frames, pil=sizes["pil"] // a.frames, raw=side * side * channels)
                print(json.dumps(rec), flush=True)
                result["cases"].append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
