"""What OccGridEstimator (morpheus_amd/estimator.py, csrc/estimator.hip) costs beside OccupancyGrid -- a measurement, no target.

    python tools/bench_estimator.py [--res 128] [--rays 2048] [--step 0.005] [--reps 300] [--warmup 3] [--out FILE]

Timed, wall clock between synchronisations (median / min / max of --reps after --warmup; the calls that are compared alternate
inside every repetition):
  update    one post-warm-up refresh at res^3 with a trivial occ_eval_fn (the norm of the point), OccupancyGrid.update_every_n_steps
            against OccGridEstimator.update_every_n_steps (levels = 1); the grid is a ball of radius 0.7 in [-1.01, 1.01]^3;
  sampling  --rays rays of a synthetic frame at default arguments, OccupancyGrid.sampling against OccGridEstimator.sampling on the
            same binaries (the two return the same samples: the count is reported once);
  cone      OccGridEstimator(levels = 4).sampling(cone_angle = 0.004) on the same rays, every level holding the ball;
  traversal the estimator's two placements on the same rays and binaries, alternating: sampling() on the lattice against
            sampling() with traversal = "dda" (cell-by-cell, mh_est_traverse_slots); the sample counts of both are reported;
  traversal_cone  the four-level cone case in both placements.

EXPECTATION (written before the first run):
  * update: OccupancyGrid's refresh runs a top-k of res^3 / 4 keys over res^3 random keys; the estimator replaces it by a count,
    a cumsum over res^3 / 2048 chunk counts and a pack, each a pass over res^3 bytes.  At 128^3 the top-k should dominate the old
    refresh; the new one should be bound by its ~12 launches (tens of microseconds each), several times faster in all.
  * sampling at defaults: the same march; the estimator adds the level loop (one level: none) and a shared-memory copy of the
    boxes.  Within a few percent of each other, both bound by the host read of the sample count.
  * cone: steps grow past t = step / cone_angle, so fewer steps than the fixed lattice, but every lane walks the 64 steps of a trip:
    about 450 VALU operations per trip and wave on top of the occupancy read.  Same order as the default call.
  * traversal (written before its first run).  A ray of the synthetic frame crosses the box on a chord of 2 to 3.5, the ball on at
    most 1.4.  Lattice at step 0.005: 400 to 700 steps, one occupancy byte each (400 - 700 bytes a ray, three steps to a cell, so
    a third of them new cache lines at worst), 7 to 11 trips of some 60 VALU operations.  Traversal: one byte per cell, 130 to
    220 a ray, in 2 to 4 trips -- but a trip walks its 64 spans in lockstep, about 35 VALU operations a span (two IEEE divisions
    for the stepped axis' exit), some 2300 a trip, plus about 15 per round of 64 samples: 5 to 10 thousand VALU operations a
    ray against the lattice's one thousand.  2048 rays are 2048 waves on 1024 SIMDs: nothing queues, so a kernel lasts as long
    as its longest wave -- the lattice's is a chain of ~10 dependent byte reads, the traversal's is VALU issue in the lockstep
    walk.  Expect the traversal KERNEL to be bound by that walk and a few times the lattice kernel; expect the CALL (what is
    timed here: two launches, a cumsum, the host read of the count, three allocations) to hide most of it: traversal slower by
    a few tens of microseconds, 10 to 30 % of the call.  Sample counts: nearly equal (the occupied chord over the step, a run's
    end rounded to the half step instead of the lattice phase).
  * traversal_cone: four levels add up to six more segments, each with its own set-up (three more divisions an axis) and a
    partly filled trip; the cone recurrence costs the writer 64 lockstep steps a round as it costs the lattice a trip.  The gap
    to the lattice should narrow: the lattice pays its 450 operations on every trip of the whole chord, the traversal only on
    rounds inside the ball.
  What came out is in DESIGN 7j ("Measured: the two placements"): the traversal call is 1.8 x and 2.0 x the lattice call, so both
  of the last two expectations were wrong -- a ray's spans are one dependent chain of scalar branches that nothing overlaps.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--step", type=float, default=0.005)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args(argv)
    import torch
    from morpheus_amd import synth
    from morpheus_amd.estimator import OccGridEstimator
    from morpheus_amd.occgrid import OccupancyGrid
    if not torch.cuda.is_available():
        print("bench_estimator: needs the GPU (the HIP path has no CPU fallback)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    R, b = args.res, 1.01
    box = [-b] * 3 + [b] * 3
    c = (torch.arange(R, device=dev).float() + 0.5) / R * 2 * b - b
    X, Y, Z = torch.meshgrid(c, c, c, indexing="ij")
    ball = (X ** 2 + Y ** 2 + Z ** 2).sqrt() < 0.7

    def measure(**calls):
        """the calls alternate inside every repetition, so that a drift of the box lands on all of them alike"""
        for _ in range(args.warmup):
            for call in calls.values():
                call()
        torch.cuda.synchronize()
        wall = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, call in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e3)
        return {k: dict(ms_median=round(statistics.median(w), 4), ms_min=round(min(w), 4), ms_max=round(max(w), 4)) for k, w in wall.items()}

    def fresh(cls, **kw):
        g = cls(box, R, **kw).to(dev)
        g.set_binary(ball.expand_as(g.binaries))
        g.occs.copy_(ball.float().reshape(-1).repeat(g.binaries.shape[0]))
        return g

    occ_eval_fn = lambda x: x.norm(dim=-1)
    old, new = fresh(OccupancyGrid), fresh(OccGridEstimator)
    result = dict(tool="bench_estimator", res=R, rays=args.rays, step=args.step, reps=args.reps, warmup=args.warmup,
                  device=torch.cuda.get_device_name(0), occupied_share=round(float(ball.float().mean()), 4))
    result["update"] = measure(occupancy_grid=lambda: old.update_every_n_steps(4096, occ_eval_fn),
                               estimator=lambda: new.update_every_n_steps(4096, occ_eval_fn))

    hw = math.isqrt(max(args.rays - 1, 0)) + 1
    o, d, _, _ = synth.frame_rays(25, hw, hw)
    o, d = o[0][:args.rays].to(dev).contiguous(), d[0][:args.rays].to(dev).contiguous()
    old, new, lv4 = fresh(OccupancyGrid), fresh(OccGridEstimator), fresh(OccGridEstimator, levels=4)
    for g in (old, new, lv4):
        g.fixed_jitter = 0.25
    a = old.sampling(o, d, render_step_size=args.step)
    bb = new.sampling(o, d, render_step_size=args.step)
    assert all(torch.equal(x, y) for x, y in zip(a, bb)), "the two samplers disagree at default arguments"
    result["sampling"] = dict(rays=int(o.shape[0]), samples=int(a[0].numel()),
                              **measure(occupancy_grid=lambda: old.sampling(o, d, render_step_size=args.step),
                                        estimator=lambda: new.sampling(o, d, render_step_size=args.step)))
    n4 = int(lv4.sampling(o, d, render_step_size=args.step, cone_angle=0.004)[0].numel())
    result["cone"] = dict(rays=int(o.shape[0]), samples=n4, levels=4, cone_angle=0.004,
                          **measure(estimator=lambda: lv4.sampling(o, d, render_step_size=args.step, cone_angle=0.004)))
    # the two placements on the same estimator: the attribute is switched between the calls, which costs nothing on the device
    def placed(g, traversal, **kw):
        def call():
            g.traversal = traversal
            return g.sampling(o, d, render_step_size=args.step, **kw)
        return call

    for key, g, kw in (("traversal", new, {}), ("traversal_cone", lv4, dict(cone_angle=0.004))):
        counts = {tr: int(placed(g, tr, **kw)()[0].numel()) for tr in ("lattice", "dda")}
        result[key] = dict(rays=int(o.shape[0]), samples=counts, levels=g.levels, **kw,
                           **measure(lattice=placed(g, "lattice", **kw), dda=placed(g, "dda", **kw)))
        g.traversal = "lattice"
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
