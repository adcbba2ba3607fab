"""Time the fused Adan step (mh_adan_step, csrc/adan.hip) beside the Adam step (mh_adam_step) and beside the same rule as a
per-tensor chain of torch operators, on the snoopy bucket.

    python tools/bench_adan.py [--reps 20] [--batch 50] [--out profiles/r09_adan.txt] [--hip-only]

Model `b` (snoopy.yaml), parameters in get_params_all's groups as optim.FlatAdan lays them out (1.86 M elements, ~70 segments), one
process.  The two HIP steps run for tens of microseconds: 5 warm-up windows, then --reps windows of --batch back-to-back calls
between two device events, ms per call as median [min .. max].  The torch chain ends its norm loop in .item(), a host
synchronisation, as the reference's class does: it is timed by the wall clock between two device synchronisations, one step a window.
  streams   full-length fp32 buffers a step reads or writes: Adam 4 read + 3 written; Adan 6 read + 5 written, with clipping one
            more read (the norm pass) and one more written (g c back into the bucket)
  TB_s      streams x 4 n bytes over the median
The torch chain is tests/adan_oracle.py's rule, operator by operator, on the parameter views of the same bucket (clipping on).
The expectation is written into the file before anything is measured.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from morpheus_amd import harness  # noqa: E402
from morpheus_amd._lib import launch, ptr  # noqa: E402
from morpheus_amd.optim import FlatAdan  # noqa: E402

BETAS, EPS, WD, MAX_GRAD_NORM = (0.98, 0.92, 0.99), 1e-8, 2e-5, 5.0
EXPECTATION = [
    "# expectation, written before the run:",
    "#  - by stream count Adan moves about 12 full-length buffers against Adam's 7: about 1.7 x Adam's time; a ratio well beyond",
    "#    that needs its cause named here",
    "#  - the per-tensor torch chain makes ~15 launches per tensor over ~60 tensors plus a norm loop that ends in .item(): on the order",
    "#    of 900 launches; its time over the fused step's is the number that justifies the kernel.  Nobody has measured either",
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


def wall_ms(fn, reps, warmup=5):
    ms = []
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return _stats(ms, 3)


def torch_chain(opt, counter):
    """one Adan step as the chain of torch operators over the parameter tensors (clipping on) -> the number of tensors"""
    b1, b2, b3 = BETAS
    views = lambda buf: [buf[o:o + k].view(p.shape) for p, o, k in opt._views]
    P, G, M, N, D, Q = (views(b) for b in (opt.flat_p, opt.bucket.flat, opt.exp_avg, opt.exp_avg_sq, opt.exp_avg_diff, opt.neg_pre_grad))
    group_of = [gi for gi, pi in zip(opt._kseg_group, opt._kseg_param) if pi >= 0]

    @torch.no_grad()
    def step():
        counter[0] += 1
        t = counter[0]
        total = torch.zeros(1, device=opt.flat_p.device)
        for g in G:
            total.add_(g.pow(2).sum())
        c = torch.clamp(MAX_GRAD_NORM / (torch.sqrt(total) + EPS), max=1.0).item()
        bc3s = (1.0 - b3 ** t) ** 0.5
        for p, g, m, n, d, q, gi in zip(P, G, M, N, D, Q, group_of):
            lr = opt.param_groups[gi]["lr"]
            g.mul_(c)
            q.add_(g)
            m.mul_(b1).add_(g, alpha=1.0 - b1)
            d.mul_(b2).add_(q, alpha=1.0 - b2)
            q.mul_(b2).add_(g)
            n.mul_(b3).addcmul_(q, q, value=1.0 - b3)
            den = (n.sqrt() / bc3s).add_(EPS)
            p.addcdiv_(m, den, value=-lr / (1.0 - b1 ** t))
            p.addcdiv_(d, den, value=-lr * b2 / (1.0 - b2 ** t))
            p.div_(1.0 + lr * WD)
            q.zero_().add_(g, alpha=-1.0)
    return step, len(P)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hip-only", action="store_true", help="skip the torch chain (for a kernel trace of the HIP steps alone)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"# tools/bench_adan.py: model b (snoopy.yaml); HIP steps: 5 warm-up + {a.reps} windows of {a.batch} calls between device "
             "events, ms per call as median [min .. max]; torch chain: wall clock between synchronisations, one step a window",
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
    lr = model.config["train"]["lr"]
    opt = FlatAdan(model.get_params_all(5 * lr), eps=EPS, weight_decay=WD, max_grad_norm=MAX_GRAD_NORM, foreach=False)
    n, ns = opt.n, len(opt._kseg_end)
    opt.bucket.flat.normal_(0.0, 1e-3)
    lrs_d = (ctypes.c_double * ns)(*[float(opt.param_groups[gi]["lr"]) for gi in opt._kseg_group])
    lrs_f = (ctypes.c_float * ns)(*[float(opt.param_groups[gi]["lr"]) for gi in opt._kseg_group])
    flags = (ctypes.c_int32 * ns)(*[1 if pi < 0 else 0 for pi in opt._kseg_param])
    # the host arrays are made once: every call is at step 100 (the bias corrections do not change what a call costs)
    adan_steps = (ctypes.c_int64 * ns)(*([100] * ns))
    adam_steps = (ctypes.c_int64 * ns)(*[0 if pi < 0 else 100 for pi in opt._kseg_param])
    bufs = [ptr(b) for b in (opt.flat_p, opt.bucket.flat, opt.exp_avg, opt.exp_avg_sq, opt.exp_avg_diff, opt.neg_pre_grad)]
    counter = [0]

    def adan(max_grad_norm):
        def fn():
            launch("mh_adan_step", *bufs, n, ns, opt._kseg_end_c, lrs_d, adan_steps, flags, *BETAS, EPS, WD, max_grad_norm, 0,
                   ptr(opt._ws))
        return fn

    def adam():
        launch("mh_adam_step", *bufs[:4], n, ns, opt._kseg_end_c, lrs_f, adam_steps, 0.9, 0.99, 1e-15)

    emit(dict(row="bucket", elements=n, segments=ns, tensors=len(opt._views), MB_per_buffer=round(n * 4 / 1e6, 2)))
    rows = {}
    for name, fn, streams in (("mh_adam_step", adam, 7), ("mh_adan_step, no clipping", adan(0.0), 11),
                              ("mh_adan_step, max_grad_norm 5", adan(MAX_GRAD_NORM), 13)):
        ms = event_ms(fn, a.reps, a.batch)
        rows[name] = ms["median"]
        emit(dict(row="step", what=name, ms=ms, streams=streams, TB_s=round(streams * 4 * n / (ms["median"] * 1e-3) / 1e12, 3)))
    if a.hip_only:
        return
    counter[0] = 0
    chain, tensors = torch_chain(opt, counter)
    ms = wall_ms(chain, a.reps)
    emit(dict(row="step", what="torch chain per tensor, max_grad_norm 5 (.item() in the norm loop)", ms=ms, tensors=tensors,
              launches_estimate=tensors * 18 + 4))
    emit(dict(row="ratios", adan_clip_over_adam=round(rows["mh_adan_step, max_grad_norm 5"] / rows["mh_adam_step"], 2),
              adan_noclip_over_adam=round(rows["mh_adan_step, no clipping"] / rows["mh_adam_step"], 2),
              torch_chain_over_adan_clip=round(ms["median"] / rows["mh_adan_step, max_grad_norm 5"], 1)))


if __name__ == "__main__":
    main()
