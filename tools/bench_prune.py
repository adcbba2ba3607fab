"""What visibility pruning (HotPathRenderer.prune, csrc/visibility.hip) buys in time -- a measurement, no target.

    python tools/bench_prune.py [--res 360] [--rays 2048] [--reps 20] [--warmup 3] [--out FILE]

Workloads, both with model state b and an occupancy grid warmed up by the field's own density (bench.py's helper):
  eval   a whole view at res x res through HotPathRenderer.eval_step (forward only, shading albedo, ragged samples);
  train  the real-view training step of bench_support/trainstep.py (albedo_normal, every regulariser, backward, Adam).
Each with prune off, {early_stop_eps: 1e-4} and {early_stop_eps: 1e-4, alpha_thre: 1e-2}.
Reported per configuration: samples marched and kept; the whole call (wall clock between synchronisations, median of --reps after
--warmup); the density pass and the two new kernels (HIP events, a second pass with the per-call timer on, so that its events do
not sit in the wall-clock numbers).  The yardstick for "off" is the parent commit's time for the same call: this tool runs on
either (on the parent, where `prune` does not exist, it reports "off" only).

EXPECTATION (written before the first run):
  * The density pass runs the warp nets and the sdf net on every marched sample: ~165 k of the ~238 k MACs of one albedo_normal
    forward sample, so D ~ 0.69 F per marched sample, without taps, colour net or backward.
  * eval (forward only, albedo): off = F M; on = D M + F kept.  Pruning wins only when kept / M < 1 - D / F ~ 0.3.
  * train (albedo_normal forward with six finite-difference taps, plus backward; roughly (F + B) ~ 4-5 D per sample): on =
    D M + (F + B) kept: break-even near kept / M ~ 0.8, a gain proportional to the dropped share beyond that.
  * Model state b is translucent (float64 on the CPU: the transmittance of no ray falls under 0.04), so early_stop_eps = 1e-4 alone
    should keep ~100 % of the samples and cost the density pass for nothing; alpha_thre = 1e-2 should drop well over half of them
    (opacity under 1e-2 at step 0.01 is sigma < 1).
  * The two kernels read ~13 bytes and write ~17 per sample: a few microseconds per 100 k samples, noise beside the density pass.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = (("off", None), ("eps1e-4", dict(early_stop_eps=1e-4)), ("eps1e-4_alpha1e-2", dict(early_stop_eps=1e-4, alpha_thre=1e-2)))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, default=360)
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args(argv)
    import torch
    from bench_support import trainstep
    from morpheus_amd import harness, ops, synth
    from morpheus_amd.occgrid import OccupancyGrid
    from morpheus_amd.optim import FlatAdam
    from morpheus_amd.render import HotPathRenderer
    if not torch.cuda.is_available():
        print("bench_prune: needs the GPU (the HIP path has no CPU fallback)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    can_prune = hasattr(HotPathRenderer(None, {}, None, 1), "prune")
    configs = [c for c in CONFIGS if c[1] is None or can_prune]

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
    occ = float(grid.binaries.float().mean())

    # sample counts of ONE call: what sampling() returns (kept) and what it marched -- the length of the arrays the density
    # function is handed inside that same call (the train workload moves the model and the grid from call to call, so counts of
    # different calls do not compare); without pruning the two are the same number
    counts = dict(returned=0, marched=0, calls=0)
    sampling = grid.sample_packed      # what the renderer calls; sampling() is its first three fields

    def counting(*a, **kw):
        out = sampling(*a, **kw)
        counts["returned"] += int(out[0].numel())
        counts["calls"] += 1
        return out

    density_events = []
    if can_prune:
        make_fn = rend._density_fn

        def timed_density_fn(*a, **kw):
            fn = make_fn(*a, **kw)

            def wrapped(t0, t1, ri):
                counts["marched"] += int(t0.shape[0])
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

    o, d, t, rid = synth.frame_rays(25, args.res, args.res)
    view = dict(rays_o=o.to(dev), rays_d=d.to(dev), rays_t=t.to(dev), rays_id=rid.to(dev), H=args.res, W=args.res)

    def eval_call():
        with torch.no_grad():
            rend.eval_step(view)

    fixed_pixels = torch.randint(0, 256 * 256, (args.rays,), device=dev, generator=torch.Generator(device=dev).manual_seed(5))

    def train_call():
        opt.bucket.zero()
        loss = ts(frame_index=0, pixel_index=fixed_pixels)      # one frame, one pixel draw: the same rays in every configuration
        loss.backward()
        opt.step()

    def pruning():
        return can_prune and bool(rend.prune)

    def measure(call):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        wall = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        counts.update(returned=0, marched=0, calls=0)
        grid.sample_packed = counting
        call()
        grid.sample_packed = sampling
        torch.cuda.synchronize()
        returned = counts["returned"]
        marched = counts["marched"] if pruning() else returned
        kern = {}
        reps_k = max(1, min(5, args.reps))
        per = {"mh_visibility_mask": [], "mh_visibility_pack": [], "density_pass": []}
        for _ in range(reps_k):
            ops.TIMER.reset(True)
            density_events.clear()
            call()
            torch.cuda.synchronize()
            summ = ops.TIMER.summary()
            for k in ("mh_visibility_mask", "mh_visibility_pack"):
                per[k].append(summ.get(k, (0, 0.0))[1])
            per["density_pass"].append(sum(a.elapsed_time(b) for a, b in density_events))
            ops.TIMER.reset(False)
        for k, v in per.items():
            kern[k + "_ms"] = round(statistics.median(v), 4)
        return dict(wall_ms_median=round(statistics.median(wall), 3), wall_ms_min=round(min(wall), 3), wall_ms_max=round(max(wall), 3),
                    samples_returned=returned, samples_marched=marched, kept_share=round(returned / max(marched, 1), 4), **kern)

    result = dict(tool="bench_prune", res=args.res, rays=args.rays, reps=args.reps, warmup=args.warmup, occupied_share=round(occ, 4),
                  device=torch.cuda.get_device_name(0), eval={}, train={})
    model.eval()
    for name, prune in configs:
        if can_prune:
            rend.prune = prune
        result["eval"][name] = measure(eval_call)
    model.train()
    for name, prune in configs:
        if can_prune:
            rend.prune = prune
        result["train"][name] = measure(train_call)
    if can_prune:
        rend.prune = None
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
