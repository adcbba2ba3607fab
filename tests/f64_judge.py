"""The float64 judgement every "hold X to float64" suite shares -- test infrastructure, plain torch on the CPU.

A kernel's result and an fp32 restatement of the same definition are both measured against a float64 run on the same inputs, as
|x - f64| / scale with `scale` the quantity's natural size.  The restatement's own error is the measure of what fp32 can keep:
    * the kernel's worst error <= max(factor x the restatement's worst, floor)                                     (within)
    * at most int(factor x n) + slack kernel elements above a threshold that the restatement has n elements above  (judge_vs_f64)
Where the scale is 0 the value must be the yardstick's exactly.  The callers differ on purpose, and only in these parameters:

    caller                         factor  floor      count threshold                           slack  restatement at zero scale
    step_f64_oracle.judge          2       4 U        the floor                                 2      asserted exact
    losses_f64_oracle.judge        2       4 U (*)    the floor                                 2      asserted exact
    glue_f64_oracle.judge          3       count x U  max(99.9th pct of the restatement, floor)  2      not asserted
    util.assert_close_vs_f64       2       tol        the floor (scale = max(|f64|, rel floor))  2      no scale is 0
    grid_f64_cases.gate            3       2^-22      (per-level norms through `within` alone: no element count)
    (*) sums and the rotated direction: the kernel's own chain of roundings x U (mean_depth, render_depth, pose_forward_floor)
"""
import json
import os

import torch

U = 2.0 ** -24          # unit round-off of fp32
F32, F64 = torch.float32, torch.float64


def flat64(t):
    return torch.as_tensor(t).detach().double().reshape(-1).cpu()


def scaled_errors(x, f64, scale):
    """|x - f64| / scale over the elements of non-zero scale (scale: the quantity's natural size, same shape as f64, or a scalar
    for all of them), and the elements of zero scale, which must be exact.
    -> (errors of the live elements, count of inexact zero-scale elements)"""
    x, r = flat64(x), flat64(f64)
    s = torch.full_like(r, float(scale)) if isinstance(scale, (int, float)) else flat64(scale)      # (a Python float stays exact)
    assert x.shape == r.shape and s.numel() in (1, r.numel()), (x.shape, r.shape, s.shape)
    s = s.expand_as(r)
    live = s > 0
    return (x - r).abs()[live] / s[live], int((x[~live] != r[~live]).sum())


def within(err, ref_err, factor, floor):
    """the gate derived from the reference's own error: `factor` x that error, or `floor` where the reference happens to be exact"""
    return err <= max(factor * ref_err, floor)


def figures_vs_f64(hip, ref32, f64, scale, what, floor, percentile=False):
    """Kernel `hip` and fp32 restatement `ref32`, both against `f64`, at `scale` (scaled_errors).  All three must be finite.
    Elements above the threshold are counted: the floor, or with `percentile` max(the 99.9th percentile of the restatement's
    errors, floor) -- the restatement's worst where it has a single live element.
    -> dict(worst_hip, worst_ref, n_hip, n_ref, threshold, n, bad_hip, bad_ref): the raw figures; n the number of live elements,
    bad_* the inexact elements of zero scale"""
    assert bool(torch.isfinite(flat64(f64)).all()) and bool(torch.isfinite(flat64(ref32)).all()), f"{what}: the yardstick is not finite"
    assert bool(torch.isfinite(flat64(hip)).all()), f"{what}: non-finite kernel result where the yardstick is finite"
    e_h, bad_h = scaled_errors(hip, f64, scale)
    e_r, bad_r = scaled_errors(ref32, f64, scale)
    worst_h, worst_r = (float(e_h.max()), float(e_r.max())) if e_h.numel() else (0.0, 0.0)
    thr = floor
    if percentile:
        thr = max(float(torch.quantile(e_r, 0.999)) if e_r.numel() > 1 else worst_r, floor)
    return dict(worst_hip=worst_h, worst_ref=worst_r, n_hip=int((e_h > thr).sum()), n_ref=int((e_r > thr).sum()), threshold=thr,
                n=int(e_h.numel()), bad_hip=bad_h, bad_ref=bad_r)


def assert_figures(f, what, factor, floor, slack, ref_zero_scale_exact=False):
    """the rules on the figures of figures_vs_f64; `ref_zero_scale_exact`: the restatement too must be exact where the scale is 0"""
    assert not (ref_zero_scale_exact and f["bad_ref"]), f"{what}: the fp32 restatement is inexact at {f['bad_ref']} elements of zero scale"
    assert f["bad_hip"] == 0, f"{what}: {f['bad_hip']} elements of zero scale are not exactly the yardstick's value"
    assert within(f["worst_hip"], f["worst_ref"], factor, floor), \
        f"{what}: worst error vs float64 {f['worst_hip']:.3e} > {factor:g} x the fp32 restatement's own {f['worst_ref']:.3e} (floor {floor:.2e})"
    assert f["n_hip"] <= int(factor * f["n_ref"]) + slack, \
        f"{what}: {f['n_hip']} elements above {f['threshold']:.3e} vs float64; the fp32 restatement has {f['n_ref']} (allowed {factor:g} x + {slack})"


def judge_vs_f64(hip, ref32, f64, scale, what, factor, floor, slack, percentile=False, ref_zero_scale_exact=False):
    """the judgement: the figures (figures_vs_f64), then the rules on them (assert_figures).  -> the figures"""
    f = figures_vs_f64(hip, ref32, f64, scale, what, floor, percentile)
    assert_figures(f, what, factor, floor, slack, ref_zero_scale_exact)
    return f


def judge_sum(hip, f64, abs_sum, count, what, extra=0.0):
    """The rule for pure sums: |x - f64| <= count * 2^-24 * (the float64 sum of the ABSOLUTE terms) [+ extra], element by
    element -- not relative to the result.  -> record (ratio = worst error / bound)."""
    h, r, a = flat64(hip), flat64(f64), flat64(abs_sum)
    assert h.shape == r.shape == a.shape, (what, h.shape, r.shape, a.shape)
    assert bool(torch.isfinite(h).all()), f"{what}: non-finite"
    bound = count * U * a + extra
    err = (h - r).abs()
    zero = bound == 0
    assert bool((err[zero] == 0).all()), f"{what}: sums without terms must be exactly 0"
    ratio = float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0
    assert ratio <= 1.0, f"{what}: error {ratio:.3f} x the bound of {count} roundings of the absolute sum"
    return dict(worst_hip=float(err.max()), worst_chain=None, ratio=ratio, n_above=int((err > bound).sum()))


def append_jsonl(path, rec):
    """append the record as one line of the JSON-lines file `path`; a file that cannot be written is not an error"""
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def report(env_var, rec):
    """append the record to the JSON-lines file the environment variable names (nothing is written without it)"""
    path = os.environ.get(env_var)
    if path:
        append_jsonl(path, rec)
