"""What importance resampling (HotPathRenderer.importance, csrc/resample.hip) costs and buys -- a record, not a gate.

    python tools/bench_resample.py [--rays 2048] [--reps 20] [--warmup 3] [--out profiles/resample_bench.json]

Workload: model state b, an occupancy grid warmed up by the field's own density (bench.py's helper), the real-view training step
of bench_support/trainstep.py at --rays rays (albedo_normal, every regulariser, backward, Adam), one frame and one pixel draw.
Configurations:
  step0.01          render.step_size = 0.01, importance off: the shipped default
  step0.02          render.step_size = 0.02, importance off: the coarse set alone
  step0.02+n32      render.step_size = 0.02, importance = {n_importance: 32}
Recorded per configuration: the step (wall clock between synchronisations, median of --reps after --warmup), the samples the main
query sees, the two resampling kernels and the density pass (HIP events of ops.TIMER in a second pass), and the mean absolute
depth difference of a forward render of the same rays against a fine render (step 0.0025, importance off).  mh_sample_pdf is timed
alone at [rays, T] with T - 1 = the mean interval count of the coarse set and n = 32.

EXPECTATION (written before the first run, and written into the output file before anything is measured):
  * A field sample of the training step costs ~173 k MACs forward and several times that with taps and backward; the density pass
    is the ~165 k MACs of the warp nets and the sdf net, forward only.  step 0.02 marches M/2 samples; + 32 draws a ray the main
    query sees M/2 + 32 x 2048.  At the real-view shape (M ~ 137 k at step 0.01 in earlier profiles, ~67 per ray) that is
    ~68 k + 66 k = 134 k samples: about as many as the default, plus a density pass over 68 k.  So step0.02+n32 should be
    SLOWER than step0.01 by roughly the density pass, 10-20 % of the step; it can only win on time with a smaller n or a
    coarser step, and the depth figures say whether it then still wins on error.
  * mh_resample_packed reads 12 bytes and writes 12 (+ n x 8) per sample and does one LDS binary search per draw: a few
    microseconds at 2 048 rays, noise beside the density pass.  mh_resample_ranges is one block: launch latency.
  * Model state b is translucent (no ray's transmittance falls under 0.04): weights are spread along the ray, the regime of
    the beta = 0.1 row of DESIGN 7k's table, where the refined set beats the coarse set but NOT an equal-count uniform set.  The
    depth difference of step0.02+n32 should lie between step0.02's and step0.01's, not below step0.01's.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = (("step0.01", 0.01, None), ("step0.02", 0.02, None), ("step0.02+n32", 0.02, dict(n_importance=32)))
KERNELS = ("mh_resample_ranges", "mh_resample_packed")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "resample_bench.json"))
    args = ap.parse_args(argv)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    result = dict(tool="bench_resample", rays=args.rays, reps=args.reps, warmup=args.warmup,
                  expectation=__doc__.split("EXPECTATION", 1)[1].strip(), measured=None)
    with open(args.out, "w") as f:                       # the expectation stands in the file before anything runs
        f.write(json.dumps(result) + "\n")
    import torch
    from bench_support import trainstep
    from morpheus_amd import harness, ops, synth
    from morpheus_amd.occgrid import OccupancyGrid
    from morpheus_amd.optim import FlatAdam
    from morpheus_amd.render import HotPathRenderer
    if not torch.cuda.is_available():
        print("bench_resample: needs the GPU (the HIP path has no CPU fallback); the output file holds the expectation only",
              file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    model = harness.build_model("b", dev).train()
    cfg = model.config
    grid = OccupancyGrid([-model.bound] * 3 + [model.bound] * 3, 128).to(dev)
    rend = HotPathRenderer(model, cfg, grid, 200)
    frames = trainstep.make_frames([8 * k % 200 for k in range(8)], 256, 256, dev)
    ts = trainstep.RealViewTrainStep(rend, frames, ray_num=args.rays)
    ts.epoch = 1000
    opt = FlatAdam(model.get_params_all(cfg["train"]["lr"]), betas=(0.9, 0.99), eps=1e-15)
    with torch.no_grad():
        trainstep.warm_up_occupancy(ts)
    ts.global_step = 4096
    fixed_pixels = torch.randint(0, 256 * 256, (args.rays,), device=dev, generator=torch.Generator(device=dev).manual_seed(5))

    density_events, seen = [], dict(coarse=0)
    make_fn = rend._density_fn

    def timed_density_fn(*a, **kw):
        fn = make_fn(*a, **kw)

        def wrapped(t0, t1, ri):
            seen["coarse"] = int(t0.shape[0])
            if not ops.TIMER.enabled:
                return fn(t0, t1, ri)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(t0, t1, ri)
            e1.record()
            density_events.append((e0, e1))
            return out
        return wrapped

    rend._density_fn = timed_density_fn

    def train_call():
        opt.bucket.zero()
        loss = ts(frame_index=0, pixel_index=fixed_pixels)
        loss.backward()
        opt.step()

    side = int(args.rays ** 0.5) + 1
    o, d, t, rid = (v[:, :args.rays].contiguous().to(dev) for v in synth.frame_rays(25, side, side))

    def depth_of(step, importance):
        cfg["render"]["step_size"], rend.importance = step, importance
        grid.fixed_jitter = 0.5
        with torch.no_grad():
            out = rend.render_rays(o, d, t, rid, side, side, shading="albedo")
        grid.fixed_jitter = None
        n = 0 if out["sdf"] is None else int(out["sdf"].shape[0])
        return out["depth"].reshape(-1).double(), n

    step0 = cfg["render"]["step_size"]
    model.eval()
    fine, n_fine = depth_of(0.0025, None)
    measured = dict(device=torch.cuda.get_device_name(0), fine_step=0.0025, fine_samples=n_fine, configs={})
    # every forward render first: the training steps below move the weights (and refresh the grid)
    for name, step, imp in CONFIGS:
        dep, n_eval = depth_of(step, dict(imp, det=True) if imp else None)
        measured["configs"][name] = dict(step_size=step, importance=imp, eval_samples=n_eval,
                                         depth_mean_abs_diff_vs_fine=float((dep - fine).abs().mean()),
                                         depth_max_abs_diff_vs_fine=float((dep - fine).abs().max()))
    model.train()
    for name, step, imp in CONFIGS:
        rec = measured["configs"][name]
        cfg["render"]["step_size"], rend.importance = step, imp
        for _ in range(args.warmup):
            train_call()
        torch.cuda.synchronize()
        wall = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            train_call()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        per = {k: [] for k in KERNELS + ("density_pass",)}
        for _ in range(max(1, min(5, args.reps))):
            ops.TIMER.reset(True)
            density_events.clear()
            train_call()
            torch.cuda.synchronize()
            summ = ops.TIMER.summary()
            for k in KERNELS:
                per[k].append(summ.get(k, (0, 0.0))[1])
            per["density_pass"].append(sum(a.elapsed_time(b) for a, b in density_events))
            ops.TIMER.reset(False)
        rec.update(step_ms_median=round(statistics.median(wall), 3), step_ms_min=round(min(wall), 3), step_ms_max=round(max(wall), 3),
                   coarse_samples_of_the_density_pass=seen["coarse"] if imp else None,
                   **{k + "_ms": round(statistics.median(v), 4) for k, v in per.items()})
    cfg["render"]["step_size"], rend.importance = step0, None
    # the dense entry point alone, at the coarse set's mean row length
    T = max(2, seen["coarse"] // max(args.rays, 1) + 1)
    bins = torch.linspace(0.5, 2.5, T, device=dev)[None].expand(args.rays, T).contiguous()
    w, u = torch.rand(args.rays, T - 1, device=dev), torch.rand(args.rays, 32, device=dev)
    times = []
    for i in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.sample_pdf(bins, w, u)
        e1.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            times.append(e0.elapsed_time(e1))
    measured["mh_sample_pdf"] = dict(B=args.rays, T=T, n=32, ms_median=round(statistics.median(times), 4))
    result["measured"] = measured
    line = json.dumps(result)
    print(json.dumps(measured))
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
