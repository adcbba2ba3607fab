"""Time and size the stage that feeds the training step: a real-view batch and a virtual view, three ways.

    python tools/bench_dataset.py [--frames 200] [--height 480] [--width 640] [--rays 2048] [--reps 20] [--batch 10]
                                  [--out profiles/r18_dataset.txt]

  (a) reference   the reference's host procedure (datasets/dataset.py:336-433, morpheus.py:834-862), restated here: host tables of
                  rays_o, rays_d, rays_t, rays_id for every pixel of every frame, images as fp32 and masks as int64; per step
                  `v[idx]` copies whole frames, then --rays pixels are picked, then six pageable `.to(device)` copies.  Virtual
                  views: the look-at pose and all H*W rays in torch on the CPU, then four copies (dataset.py:503-578).
  (b) torch       torch indexing of the same tables resident on the device, as bench_support/trainstep.sample_real_view_rays does
                  (the synthetic stand-in the benchmark draws from; real views only)
  (c) dataset     morpheus_amd.dataset.DeviceDataset: uint8 / uint16 frames on the device, one launch per real-view batch, two per
                  virtual view; indices and angles drawn on the device
Frame contents are random: no path depends on them.  Timing: (b) and (c) are device work queued by a host that does not wait, so
they are timed twice -- medians of --reps windows of --batch calls between two device events (5 warm-up windows), and the wall clock
of the same windows ended by a synchronize; (a) is a host path and is timed by wall clock alone, each call ended by a synchronize.
ms per call as median [min .. max]; clocks are left alone.  The expectation is written into the file before anything is measured.
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

from bench_support import trainstep  # noqa: E402
from morpheus_amd import ops  # noqa: E402
from morpheus_amd.dataset import DeviceDataset, _label_bounds  # noqa: E402

EXPECTATION = [
    "# expectation, written before the run (nobody has measured this stage; no figure is fixed in advance):",
    "#  - (a) the reference's host path is dominated by `v[idx]`: seven whole-frame copies (56 B a pixel, 17 MB at 480 x 640) before",
    "#    2048 pixels are picked, then six small pageable copies each with its own synchronisation: a millisecond or more a step.",
    "#  - (b) torch indexing of device tables is ~10 small launches; host-bound, some tens of microseconds of device time.",
    "#  - (c) is one launch of 2048 threads plus two torch.randint launches: device time of a few microseconds; its wall time is",
    "#    Python (argument checks, eleven torch.empty) and may well be no better than (b)'s.  Where (c) loses to (b) it is kept for",
    "#    what it stores: 6 bytes a pixel against 56, and real uint8 / uint16 frames instead of a synthetic stand-in.",
    "#  - virtual views: (a) builds H*W rays on the CPU and copies them; (c) is two launches whatever the size.",
]


def _stats(ms, digits=4):
    return dict(median=round(statistics.median(ms), digits), min=round(min(ms), digits), max=round(max(ms), digits))


def device_ms(fn, reps, batch, warmup=5):
    """-> (ms per call between device events, ms per call by wall clock with a synchronize), over the same windows"""
    for _ in range(warmup * batch):
        fn()
    torch.cuda.synchronize()
    pairs, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3 / batch)
        pairs.append((e0, e1))
    return _stats([a.elapsed_time(b) / batch for a, b in pairs]), _stats(wall)


def host_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return _stats(ms)


def nbytes(tensors):
    return int(sum(t.numel() * t.element_size() for t in tensors))


def reference_tables(F, H, W):
    """what DeformDataset.real_view_data holds (dataset.py:380-396), random contents"""
    N = H * W
    t = torch.arange(F)
    return {"rays_o": torch.rand(F, N, 3), "rays_d": torch.rand(F, N, 3), "rays_t": (t / F)[:, None, None].repeat(1, N, 1),
            "rays_id": t[:, None, None].repeat(1, N, 1), "H": H, "W": W, "image": torch.rand(F, 3, H, W), "depth": torch.rand(F, H, W),
            "mask": torch.randint(0, 2, (F, H, W)), "pose": torch.rand(F, 4, 4), "theta": torch.rand(F), "phi": torch.rand(F),
            "radius": torch.rand(F)}


def reference_real_view(data, F, ray_num, dev):
    """dataset.py:398-433 followed by the six copies of morpheus.py:841-850"""
    idx = torch.randint(0, F, (1,))
    index = torch.randint(0, data["H"] * data["W"], (ray_num,))
    s = {}
    for k, v in data.items():
        if isinstance(v, int):
            s[k] = v
        else:
            s[k] = v[idx]
            if "ray" in k:
                s[k] = s[k][:, index]
    s["image"] = s["image"].reshape(1, 3, -1)[..., index].reshape(1, 3, ray_num, 1)
    s["mask"] = s["mask"].reshape(1, -1)[..., index].reshape(1, ray_num, 1)
    s["depth"] = s["depth"].reshape(1, -1)[..., index].reshape(1, ray_num, 1)
    return [s[k].to(dev) for k in ("rays_o", "rays_d", "rays_t", "rays_id")] + [s["depth"].view(1, -1, 1).to(dev), s["mask"].view(1, -1, 1).to(dev)]


def reference_virtual_view(K, radius, F, H, W, dev):
    """dataset.py:435-578 on the CPU (the theta/phi box), then the four copies of morpheus.py:841-844"""
    t = torch.randint(0, F, (1,))
    thetas = torch.rand(1) * (np.deg2rad(105) - np.deg2rad(45)) + np.deg2rad(45)
    phis = torch.rand(1) * (2 * np.pi)
    r = radius[t]
    c = torch.stack([r * torch.sin(thetas) * torch.sin(phis), r * torch.cos(thetas), r * torch.sin(thetas) * torch.cos(phis)], -1)
    unit = lambda x: x / torch.sqrt(torch.clamp(torch.sum(x * x, -1, keepdim=True), min=1e-20))
    fwd = unit(c)
    right = unit(torch.linalg.cross(torch.tensor([[0.0, 1.0, 0.0]]), fwd, dim=-1))
    up = unit(torch.linalg.cross(fwd, right, dim=-1))
    poses = torch.eye(4).unsqueeze(0).repeat(1, 1, 1)
    poses[:, :3, :3] = torch.stack((right, up, fwd), dim=-1)
    poses[:, :3, 3] = c
    i, j = torch.meshgrid(torch.arange(W, dtype=torch.float32), torch.arange(H, dtype=torch.float32), indexing="xy")
    dirs = torch.stack([(i + 0.5 - K[0, 2]) / K[0, 0], -(j + 0.5 - K[1, 2]) / K[1, 1], -torch.ones_like(i)], -1).to(torch.float32)
    dirs = dirs[None].repeat(1, 1, 1, 1)
    rays_o = poses[..., None, None, :3, -1].repeat(1, H, W, 1)
    rays_d = torch.sum(dirs[..., None, :] * poses[:, None, None, :3, :3], -1)
    out = (rays_o.reshape(1, -1, 3), rays_d.reshape(1, -1, 3), (t / F)[:, None, None].repeat(1, H * W, 1), t[:, None, None].repeat(1, H * W, 1))
    return [v.to(dev) for v in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    F, H, W = a.frames, a.height, a.width
    lines = [f"# tools/bench_dataset.py: {F} frames of {H} x {W}, real-view batches of {a.rays} rays, virtual views of 72 x 72 and 180 x 180; "
             f"5 warm-up + {a.reps} windows of {a.batch} calls; ms per call as median [min .. max]",
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
    cfg = {"data": {"data_dir": None, "depth_scale": 1000.0, "known_view_scale": 1.0, "novel_view_scale": 0.2, "novel_view_scale_factor": 1.0,
                    "theta_range": [45, 105], "phi_range": [-180, 180], "angle_overhead": 30, "angle_front": 60, "default_polar": 90.0,
                    "uniform_sphere_rate": 0.0, "outlier_remove": False}}
    K = np.array([[0.9 * W, 0.0, W / 2], [0.0, 0.9 * W, H / 2], [0.0, 0.0, 1.0]])

    # ---- (a) the reference's host tables
    data = reference_tables(F, H, W)
    host_bytes = nbytes(v for v in data.values() if torch.is_tensor(v))
    real_a = host_ms(lambda: reference_real_view(data, F, a.rays, dev), a.reps)
    emit(dict(row="real view", path="(a) reference host tables", resident="host", resident_MB=round(host_bytes / 1e6, 1),
              bytes_per_pixel=round(host_bytes / (F * H * W), 1), wall_ms=real_a))

    # ---- (b) the same tables on the device, torch indexing (bench_support/trainstep.py)
    table = {k: data[k].to(dev) for k in ("rays_o", "rays_d", "rays_t", "rays_id")}
    table.update(image=data["image"].permute(0, 2, 3, 1).reshape(F, H * W, 3).contiguous().to(dev),
                 depth=data["depth"].reshape(F, H * W).to(dev), mask=data["mask"].reshape(F, H * W).float().to(dev))
    del data
    dev_bytes = nbytes(table.values())

    def real_b():
        f = int(torch.randint(0, F, (1,)))                            # the benchmark's host-side frame choice
        return trainstep.sample_real_view_rays({k: v[f] for k, v in table.items()}, a.rays)
    ev, wall = device_ms(real_b, a.reps, a.batch)
    emit(dict(row="real view", path="(b) torch indexing of device tables", resident="device", resident_MB=round(dev_bytes / 1e6, 1),
              bytes_per_pixel=round(dev_bytes / (F * H * W), 1), event_ms=ev, wall_ms=wall))
    del table
    torch.cuda.empty_cache()

    # ---- (c) DeviceDataset
    ds = DeviceDataset(cfg, torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8), torch.randint(0, 4000, (F, H, W), dtype=torch.int32).to(torch.uint16),
                       torch.randint(0, 2, (F, H, W), dtype=torch.uint8) * 255, torch.rand(F, 4, 4), K, torch.rand(F) + 1.5,
                       torch.rand(F) * 60 + 45, torch.rand(F) * 360, device=dev)
    ev, wall = device_ms(lambda: ds.sample_real_view_rays(bs=1, ray_num=a.rays), a.reps, a.batch)
    row_c = dict(row="real view", path="(c) DeviceDataset.sample_real_view_rays, indices drawn on the device", resident="device",
                 resident_MB=round(ds.resident_bytes / 1e6, 1), bytes_per_pixel=round(ds.resident_bytes / (F * H * W), 1), event_ms=ev, wall_ms=wall)
    emit(row_c)
    frames = torch.randint(0, F, (1,), device=dev)
    index = torch.randint(0, H * W, (a.rays,), device=dev, dtype=torch.int32)
    tabs = (ds.poses_dev, ds.rgb_dev, ds.depth_dev, ds.mask_dev, ds.theta_dev, ds.phi_dev, ds.radius_dev)
    ev, wall = device_ms(lambda: ops.dataset_sample(K, *tabs, 1000.0, frames, index), a.reps, a.batch)
    emit(dict(row="real view", path="(c) ops.dataset_sample alone: one launch, fixed indices", event_ms=ev, wall_ms=wall))
    ev, wall = device_ms(lambda: ds.sample_real_view_rays(bs=8, ray_num=a.rays), a.reps, a.batch)
    emit(dict(row="real view, 8 frames a batch", path="(c) DeviceDataset.sample_real_view_rays", event_ms=ev, wall_ms=wall))
    emit(dict(row="real view, summary", c_over_a_wall=round(row_c["wall_ms"]["median"] / real_a["median"], 4),
              a_bytes_over_c_bytes=round(host_bytes / ds.resident_bytes, 2)))

    # ---- virtual views
    radius = ds.radius
    bounds = _label_bounds(float(np.deg2rad(60)), float(np.deg2rad(30)))
    lo, span = float(np.deg2rad(45)), float(np.deg2rad(105) - np.deg2rad(45))
    for S in (72, 180):
        Ks = ds.scale_intrinsics(ds.intrinsics, S / H)
        virt_a = host_ms(lambda: reference_virtual_view(Ks, radius, F, S, S, dev), a.reps)
        emit(dict(row=f"virtual view {S} x {S}", path="(a) reference: pose and rays on the CPU, four copies", wall_ms=virt_a))

        def virt_c():
            t = torch.randint(0, F, (1,), device=dev)
            th = torch.rand(1, device=dev) * span + lo
            ph = torch.rand(1, device=dev) * (2 * np.pi)
            v = ops.dataset_virtual_pose(ops.VIRTUAL_ANGLES, th, ph, None, t, ds.radius_dev, ds.theta_dev, ds.phi_dev, 1.0, bounds)
            return ops.generate_rays_dev(Ks, v["pose"], S, S, None, t, F)
        ev, wall = device_ms(virt_c, a.reps, a.batch)
        emit(dict(row=f"virtual view {S} x {S}", path="(c) draws on the device, mh_dataset_virtual_pose + mh_generate_rays_dev", event_ms=ev,
                  wall_ms=wall, c_over_a_wall=round(wall["median"] / virt_a["median"], 4)))


if __name__ == "__main__":
    main()
