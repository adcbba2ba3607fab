"""Time the reference's four-call composition through morpheus_amd.volrend (csrc/volrend.hip) beside the fused compositor and
beside plain torch, forward + backward, and accumulate_along_rays alone.

    python tools/bench_volrend.py [--rays 16384] [--samples 128] [--reps 20] [--batch 5] [--out profiles/r17_volrend.txt]

Two workloads: `uniform`, --rays rays of --samples samples each, and `ragged`, the same number of rays with marcher-like counts (a
third of the rays miss, the rest hold 1 .. 2 x --samples samples).  Three columns, each one forward + backward of the same loss
(a ready-made gradient for opacity, depth and colour) on the same inputs, through autograd:
  volrend   render_weight_from_density + three accumulate_along_rays (morpheus.py:675-685) with int64 ray_indices: what a render
            loop written against nerfacc does once it imports this module in nerfacc's place
  fused     ops.composite: the one-launch form HotPathRenderer uses (ray_start / ray_cnt made once, outside the window)
  torch     the same four functions in plain torch -- a packed cumsum minus its per-ray offset, index_add_ -- which is what a user
            without nerfacc writes today
Then mh_accumulate_fwd alone at the C ABI for D = 1, 3, 48: bytes = the weights and values read once and the result written once,
TB_s over the median, of_stream over STREAM_TB_S (the rate a float4 copy kernel reaches on this part).
Timing as tools/bench_encoders.py: 5 warm-up windows, then --reps windows of --batch repetitions between two device events, ms per
repetition as median [min .. max]; clocks are left alone.  The expectation is written into the file before anything is measured.
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

from morpheus_amd import ops, volrend  # noqa: E402
from morpheus_amd._lib import launch, ptr  # noqa: E402

STREAM_TB_S = 6.29
EXPECTATION = [
    "# expectation, written before the run (nobody has measured any of this; no threshold is fixed):",
    "#  - fused < volrend: the fused compositor reads sigma, ts, te, rgb once and writes the weights once (32 B a sample forward);",
    "#    the four-call form writes weights, trans and alphas, reads the weights back three times, finds the ray boundaries four",
    "#    times and is 4 launches + their autograd nodes forward, 4 backward, with three d_weights arrays summed by autograd.",
    "#    2 .. 4 x the fused time is expected; that is why HotPathRenderer keeps the fused kernel.",
    "#  - volrend < torch: the torch form is ~25 launches forward (exp, expm1, cumsum, gathers, three index_add_) and more backward,",
    "#    each a pass over [M]; index_add_ is atomic.  3 x or more is expected, but 2 M samples are only 8 MB an array: everything",
    "#    sits in the last-level cache and launch overhead may flatten the difference.  If volrend is not faster, say so.",
    "#  - accumulate alone: streaming, one wavefront per ray, 128 samples = 2 trips a ray at D <= 4 -- short rays, little to hide",
    "#    latency with; D = 1 and 3 move 16 .. 34 MB (cache-resident) and are expected well below the copy rate, D = 48 (410 MB,",
    "#    whole lines, 128 trips a ray) nearer to it.",
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


def torch_composition(sigma, ts, te, rgb, ray_indices, ray_start, n_rays):
    """the four functions in plain torch on packed samples: a global cumsum minus the value it had where the sample's ray begins"""
    sd = sigma * (te - ts)
    incl = torch.cumsum(sd, 0)
    excl = incl - sd
    excl = excl - excl[ray_start][ray_indices]
    weights = torch.exp(-excl) * -torch.expm1(-sd)
    acc = lambda v: torch.zeros(n_rays, v.shape[1], device=v.device).index_add_(0, ray_indices, weights[:, None] * v)
    return weights, acc(torch.ones_like(weights)[:, None]), acc(((ts + te) / 2)[:, None]), acc(rgb)


def workload(kind, n_rays, n_samples, dev):
    g = torch.Generator(device="cpu").manual_seed(7)
    if kind == "uniform":
        cnt = torch.full((n_rays,), n_samples, dtype=torch.long)
    else:
        cnt = torch.randint(1, 2 * n_samples + 1, (n_rays,), generator=g)
        cnt[torch.rand(n_rays, generator=g) < 1 / 3] = 0
    ray_indices = torch.repeat_interleave(torch.arange(n_rays), cnt)
    M = int(cnt.sum())
    dt = torch.rand(M, generator=g) * 0.02 + 0.002
    start = torch.cumsum(cnt, 0) - cnt
    ts = torch.cumsum(dt, 0) - dt
    ts = ts - ts[start.clamp_max(max(M - 1, 0))][ray_indices] + 0.05
    sigma = torch.rand(M, generator=g) * (6.0 / n_samples / 0.012)
    w = dict(ts=ts, te=ts + dt, sigma=sigma, rgb=torch.rand(M, 3, generator=g), ray_indices=ray_indices,
             g_o=torch.rand(n_rays, 1, generator=g), g_d=torch.rand(n_rays, 1, generator=g), g_c=torch.rand(n_rays, 3, generator=g))
    w = {k: v.to(dev) for k, v in w.items()}
    w.update(M=M, N=n_rays, kind=kind)
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=16384)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"# tools/bench_volrend.py: {a.rays} rays x {a.samples} samples (uniform) and a ragged marcher-like case; 5 warm-up + {a.reps} "
             f"windows of {a.batch} repetitions between device events, ms per repetition as median [min .. max]; of_stream = TB_s / {STREAM_TB_S}",
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
    for kind in ("uniform", "ragged"):
        w = workload(kind, a.rays, a.samples, dev)
        ts, te, ri, N = w["ts"], w["te"], w["ray_indices"], w["N"]
        sigma, rgb = w["sigma"].clone().requires_grad_(True), w["rgb"].clone().requires_grad_(True)
        rs, rc = ops.packed_info(ri, N)
        rs64 = rs.long().clamp_max(w["M"] - 1)                     # an empty ray behind the last sample starts at M: never gathered from

        def backward(outs):
            _, o, d, c = outs
            sigma.grad = rgb.grad = None
            ((o * w["g_o"]).sum() + (d * w["g_d"]).sum() + (c * w["g_c"]).sum()).backward()

        def run_volrend():
            weights, _, _ = volrend.render_weight_from_density(ts, te, sigma, ray_indices=ri, n_rays=N)
            backward((weights, volrend.accumulate_along_rays(weights, None, ri, N),
                      volrend.accumulate_along_rays(weights, ((ts + te) / 2)[:, None], ri, N),
                      volrend.accumulate_along_rays(weights, rgb, ri, N)))

        def run_fused():
            wts, o, d, c = ops.composite(sigma, ts, te, rgb, rs, rc)
            backward((wts, o[:, None], d[:, None], c))

        def run_torch():
            backward(torch_composition(sigma, ts, te, rgb, ri, rs64, N))

        grads = {}
        for name, fn in (("volrend", run_volrend), ("fused", run_fused), ("torch", run_torch)):
            fn()
            grads[name] = sigma.grad.clone()
        scale = float(grads["fused"].abs().max())
        agree = {k: round(float((grads[k] - grads["fused"]).abs().max()) / scale, 9) for k in ("volrend", "torch")}
        ms = {name: event_ms(fn, a.reps, a.batch) for name, fn in (("volrend", run_volrend), ("fused", run_fused), ("torch", run_torch))}
        emit(dict(row="composition forward + backward", workload=kind, rays=N, samples=w["M"], ms=ms,
                  volrend_over_fused=round(ms["volrend"]["median"] / ms["fused"]["median"], 2),
                  torch_over_volrend=round(ms["torch"]["median"] / ms["volrend"]["median"], 2),
                  max_d_sigma_difference_to_fused_over_max_d_sigma=agree))
        if kind == "uniform":
            weights = torch.rand(w["M"], device=dev)
            for D in (1, 3, 48):
                values, out = torch.rand(w["M"], D, device=dev), torch.empty(N, D, device=dev)
                args = (ptr(weights), ptr(values), D, ptr(rs), ptr(rc), N, ptr(out))
                t = event_ms(lambda: launch("mh_accumulate_fwd", *args), a.reps, 4 * a.batch)
                nbytes = 4 * (w["M"] * (1 + D) + N * D)
                tb_s = nbytes / (t["median"] * 1e-3) / 1e12
                emit(dict(row="accumulate forward alone", D=D, ms=t, MB=round(nbytes / 1e6, 1), TB_s=round(tb_s, 3), of_stream=round(tb_s / STREAM_TB_S, 3)))
                del values, out


if __name__ == "__main__":
    main()
