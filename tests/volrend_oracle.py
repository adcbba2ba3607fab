"""Float64 yardsticks, fp32 restatements, cases and natural scales for morpheus_amd.volrend (csrc/volrend.hip) -- test
infrastructure, plain torch and numpy on the CPU, in the manner of tests/step_f64_oracle.py, whose sample builders it shares.

The definitions are written once, dtype-generic, as sequential per-ray loops with no reference to the shape of a kernel's scan,
and run under autograd (per ray over its samples in order, sd_i = sigma_i (te_i - ts_i) formed as the kernel forms it):
    density form   alpha_i = -expm1(-sd_i);  T_i = exp(-sum_{j<i} sd_j)
    alpha form     T_i = prod_{j<i} (1 - alpha_j): a loop product, whose autograd gradient is the product with the sample's own
                   factor left out -- finite at alpha == 1 by itself, no division
    both           w_i = T_i alpha_i;   accumulate: out[r, c] = sum_{i in r} w_i v[i, c], exactly 0 without samples
Run in float64 on the fp32 inputs they are the yardstick, run in fp32 the measure of what fp32 can keep.

The judgement is tests/f64_judge.judge_vs_f64 with the parameters step_f64_oracle.judge uses for the compositor: factor 2, floor
4 x 2^-24, slack 2, zero-scale elements exact.  The bound is the fp32 restatement's own error on the same inputs, never a number
fitted to a run.  Natural scales (all from the float64 run):
    weights, accumulated sums of weights   the ray's total weight           trans, alphas   1
    accumulate                             sum |w| |v| per output element
    d_sigma                                dt_i x the ray's largest |g| (over the probes the loss uses)
    d_alpha_i                              the sum of the absolute terms of its formula:
                                           |g_w_i| T_i + sum_{j>i} (|g_w_j| alpha_j + |g_T_j|) prod_{k<j, k != i} (1 - alpha_k)
    d_values                               |w| x |g|                        d_weights       sum_c |g v|
"""
import numpy as np
import torch

from tests.f64_judge import F32, F64, U, figures_vs_f64, judge_vs_f64, report
from tests.step_f64_oracle import _assemble, _dense, _drawn_ray, _log_uniform, form_sd, ray_index

FACTOR, FLOOR, SLACK = 2.0, 4 * U, 2


def judge(hip, ref32, f64, scale, what):
    """print the figures, append them to the JSON-lines file MORPHEUS_VOLREND_REPORT names, then f64_judge.judge_vs_f64"""
    f = figures_vs_f64(hip, ref32, f64, scale, what, FLOOR)
    rec = dict(what=what, worst_hip=f["worst_hip"], worst_ref=f["worst_ref"], ratio=(f["worst_hip"] / f["worst_ref"] if f["worst_ref"] > 0 else None),
               n_hip=f["n_hip"], n_ref=f["n_ref"], n=f["n"], factor=FACTOR)
    print(f"[volrend-f64] {what}: kernel {f['worst_hip']:.3e}  fp32 restatement {f['worst_ref']:.3e}  above {FLOOR:.1e}: {f['n_hip']} / {f['n_ref']}  of {f['n']}")
    report("MORPHEUS_VOLREND_REPORT", rec)
    judge_vs_f64(hip, ref32, f64, scale, what, FACTOR, FLOOR, SLACK, ref_zero_scale_exact=True)
    return rec


# ================================================================================================================ definitions
def _layout(cnt):
    cnt = [int(c) for c in cnt]
    ray, k = ray_index(cnt)
    return cnt, len(cnt), max(cnt + [0]), ray, k


def weights(values, ts32, te32, cnt, alpha_form):
    """-> (w, T, alpha) [M] in the dtype of `values` (sigma, or alpha in the alpha form: ts32 / te32 unused)"""
    cnt, N, K, ray, k = _layout(cnt)
    if alpha_form:
        alpha = _dense(values, ray, k, N, K)                       # padding: alpha = 0, a factor of 1
        run, cols = alpha.new_ones(N), []
        for j in range(K):                                         # the exclusive product never contains the sample's own factor
            cols.append(run)
            run = run * (1 - alpha[:, j])
    else:
        sd = _dense(form_sd(values, ts32, te32), ray, k, N, K)
        alpha = -torch.expm1(-sd)
        run, cols = sd.new_zeros(N), []
        for j in range(K):
            cols.append(torch.exp(-run))
            run = run + sd[:, j]
    T = torch.stack(cols, 1) if K else alpha.new_zeros(N, 0)
    return (T * alpha)[ray, k], T[ray, k], alpha[ray, k]


def accumulate(w, values, cnt):
    """-> [N, D]; values None: a column of ones.  One ray after the other, sample by sample."""
    cnt, N, K, ray, k = _layout(cnt)
    v = w.new_ones(w.shape[0], 1) if values is None else values
    wd, vd = _dense(w, ray, k, N, K), _dense(v, ray, k, N, K)
    out = w.new_zeros(N, v.shape[1])
    for j in range(K):
        out = out + wd[:, j, None] * vd[:, j]
    return out


DENSITY_VARIANTS = ("wTa", "w", "T", "a", "wT", "wa", "Ta")      # which outputs the loss reaches: all, each alone, each pair
ALPHA_VARIANTS = ("wT", "w", "T")


def _probe_loss(outs, names, case, variant, dev=None):
    terms = []
    for name, out in zip(names, outs):
        if name in variant:
            g = case["g_" + name].to(out.dtype)
            terms.append((out * (g.to(dev) if dev else g)).sum())
    return sum(terms)


def weights_loss(outs, case, variant, dev=None):
    """sum of <output, its probe> over the outputs (w, T[, alpha]) named in `variant`: the incoming gradients ARE the probes"""
    return _probe_loss(outs, "wTa", case, variant, dev)


def weights_run(case, dtype):
    """forward once, then the gradient to sigma / alpha of every loss variant -> dict(w, T, a, grads={variant: d_in})"""
    alpha_form = case["alpha_form"]
    x = case["alpha" if alpha_form else "sigma"].detach().to(dtype).clone().requires_grad_(True)
    outs = weights(x, case.get("ts"), case.get("te"), case["cnt"], alpha_form)
    grads = {}
    for var in (ALPHA_VARIANTS if alpha_form else DENSITY_VARIANTS):
        g, = torch.autograd.grad(weights_loss(outs[:2] if alpha_form else outs, case, var), [x], retain_graph=True, allow_unused=True)
        grads[var] = torch.zeros_like(x) if g is None else g
    return dict(w=outs[0].detach(), T=outs[1].detach(), a=outs[2].detach(), grads=grads)


def _ray_total(case, w64):
    ray, _ = ray_index(case["cnt"])
    return torch.zeros(len(case["cnt"]), dtype=F64).index_add(0, ray, w64.abs())


def weights_scales(case, run64, variant):
    """-> dict(w, T, a, d_in) of natural scales (module docstring)"""
    ray, _ = ray_index(case["cnt"])
    N, M = len(case["cnt"]), ray.numel()
    tot = _ray_total(case, run64["w"])
    g = {n: (case["g_" + n].double().abs() if n in variant else torch.zeros(M, dtype=F64)) for n in "wTa"}
    if not case["alpha_form"]:
        gmax = torch.zeros(N, dtype=F64).scatter_reduce(0, ray, torch.stack(list(g.values())).amax(0), "amax")
        d_in = (case["te"] - case["ts"]).double() * gmax[ray]
    else:
        alpha = case["alpha"].double().numpy()
        a_term = (g["w"] * case["alpha"].double() + g["T"]).numpy()
        gw, T = g["w"].numpy(), run64["T"].double().numpy()
        d_in = np.zeros(M)
        pos = 0
        for c in case["cnt"]:
            f = 1.0 - alpha[pos:pos + c]
            for i in range(c):
                fi = f.copy()
                fi[i] = 1.0                                                     # the product with factor i left out
                loo = np.concatenate([[1.0], np.cumprod(fi)[:-1]])
                d_in[pos + i] = gw[pos + i] * T[pos + i] + float((a_term[pos + i + 1:pos + c] * loo[i + 1:]).sum())
            pos += c
        d_in = torch.from_numpy(d_in)
    return dict(w=tot[ray], T=1.0, a=1.0, d_in=d_in)


# ===================================================================================================================== cases
COUNTS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 350]
BASE_RAYS = [0, 1, 2, 63, 64, 65, 0, 0, 127, 128, 129, 350]        # a 0-count ray first, two adjacent, one appended last
OPAQUE_SD = (30.0, 1e2, 1e4)
OPAQUE_AT = (0, 63, 64)                                             # lane 0, lane 63, the first lane of the second chunk
ZERO_AT = (0, 5, 63, 64, 69)
BEHIND = 6                                                          # thin samples behind a placed opaque one
NEAR_ONE = 1.0 - 2.0 ** -20                                         # an alpha with 1 - alpha = 2^-20, exact in fp32


def _start(cnt):
    return np.cumsum([0] + list(cnt[:-1]))


def _probes(case, rng):
    u = lambda *s: torch.from_numpy((rng.rand(*s) * 2 - 1).astype(np.float32))
    case["g_T"], case["g_a"] = u(case["M"]), u(case["M"])
    return case


def density_case(seed=41):
    """Every count of COUNTS with empty rays first, last and adjacent, then the placed rays:
        opaque <sd> @<k>   one sample of sd 30 / 1e2 / 1e4 at k = 0, 63, 64 behind a thin prefix, BEHIND thin samples behind it
        sigma = 0, ts == te   a translucent ray of 70 with the named samples at ZERO_AT
        underflow          100 samples: 40 of sd 0.1, then sd 20 each: the fp32 transmittance reaches 0 near position 45, mid-chunk
    25 rays: one ray in the last workgroup."""
    rng = np.random.RandomState(seed)
    rays = [_drawn_ray(rng, c, r % 2 == 1 or c >= 350) for r, c in enumerate(BASE_RAYS)]
    placed = {}
    for sd_big in OPAQUE_SD:
        for at in OPAQUE_AT:
            ray = _log_uniform(rng, at + 1 + BEHIND, 5e-4, 2e-3)
            ray[at] = sd_big
            placed[f"opaque {sd_big:g} @{at}"] = (len(rays), at)
            rays.append(ray)
    for name in ("sigma = 0", "ts == te"):
        placed[name] = (len(rays), ZERO_AT)
        rays.append(_log_uniform(rng, 70, 1e-3, 5e-2))
    placed["underflow"] = (len(rays), 45)
    rays.append(np.concatenate([np.full(40, 0.1), np.full(60, 20.0)]))
    rays.append(np.zeros(0))
    c = _assemble(rays, rng, seed)
    start = _start(c["cnt"])
    r, ks = placed["sigma = 0"]
    c["sigma"][[int(start[r]) + k for k in ks]] = 0.0
    r, ks = placed["ts == te"]
    idx = [int(start[r]) + k for k in ks]
    c["te"][idx] = c["ts"][idx]
    c.update(placed=placed, alpha_form=False)
    return _probes(c, rng)


def _alpha_assemble(rays, rng):
    cnt = [len(r) for r in rays]
    M, N = sum(cnt), len(rays)
    alpha = torch.from_numpy(np.concatenate(rays + [np.zeros(0)]).astype(np.float32))
    u = lambda *s: torch.from_numpy((rng.rand(*s) * 2 - 1).astype(np.float32))
    return dict(cnt=cnt, N=N, M=M, alpha=alpha, g_w=u(M), g_T=u(M), g_a=u(M), alpha_form=True, placed={})


def _drawn_alpha(rng, c, translucent):
    return -np.expm1(-_drawn_ray(rng, c, translucent))


def alpha_case(seed=43):
    """The counts of density_case, then the placed rays:
        alpha = 1 @<k>     alpha == 1 exactly at k = 0, 63, 64 behind a thin prefix, BEHIND thin samples behind it
        alpha = 0          a translucent ray of 70 with alpha = 0 at ZERO_AT
        two opaque         70 samples, alpha == 1 at 10 and at 40: everything behind the second has zero gradient to the first
        near one           70 translucent samples with 1 - alpha = 2^-20 at 5 and at 64
        underflow          100 samples: 40 of alpha 0.1, then 1 - alpha = 2^-20 each: T leaves fp32 near position 47, mid-chunk
    20 rays."""
    rng = np.random.RandomState(seed)
    rays = [_drawn_alpha(rng, c, r % 2 == 1 or c >= 350) for r, c in enumerate(BASE_RAYS)]
    placed = {}
    thin = lambda n: -np.expm1(-_log_uniform(rng, n, 5e-4, 2e-3))
    for at in OPAQUE_AT:
        ray = thin(at + 1 + BEHIND)
        ray[at] = 1.0
        placed[f"alpha = 1 @{at}"] = (len(rays), at)
        rays.append(ray)
    mid = lambda: -np.expm1(-_log_uniform(rng, 70, 1e-3, 5e-2))
    ray = mid()
    ray[list(ZERO_AT)] = 0.0
    placed["alpha = 0"] = (len(rays), ZERO_AT)
    rays.append(ray)
    ray = mid()
    ray[[10, 40]] = 1.0
    placed["two opaque"] = (len(rays), (10, 40))
    rays.append(ray)
    ray = mid()
    ray[[5, 64]] = NEAR_ONE
    placed["near one"] = (len(rays), (5, 64))
    rays.append(ray)
    placed["underflow"] = (len(rays), 47)
    rays.append(np.concatenate([np.full(40, 0.1), np.full(60, NEAR_ONE)]))
    rays.append(np.zeros(0))
    c = _alpha_assemble(rays, rng)
    c["placed"] = placed
    return c


def gradient_pools(case):
    """{pool name: mask over the packed samples}: which gradient elements are judged together.  d_alpha is measured against the sum
    of the absolute terms of its own formula, so where the fp32 transmittance has left the number range and float64's has not the
    fp32 restatement itself is wrong by the whole scale (error 1): the underflow ray of the alpha form is judged on its own, so
    that its bound does not become everybody's.  Each pool is held to the same rule."""
    name = "d_alpha" if case["alpha_form"] else "d_sigma"
    everything = torch.ones(case["M"], dtype=torch.bool)
    if not case["alpha_form"] or "underflow" not in case["placed"]:
        return {name: everything}
    ray, _ = ray_index(case["cnt"])
    own = ray == case["placed"]["underflow"][0]
    return {name: ~own, name + ", underflow ray": own}


RAY_COUNTS = (1, 4, 5)         # 1, 4 and 1 rays in the last workgroup of four


def rays_case(N, alpha_form, seed=47):
    rng = np.random.RandomState(seed + N)
    cnt = [65, 0, 3, 129, 1][:N]
    if alpha_form:
        return _alpha_assemble([_drawn_alpha(rng, c, r % 2 == 1) for r, c in enumerate(cnt)], rng)
    c = _assemble([_drawn_ray(rng, c, r % 2 == 1) for r, c in enumerate(cnt)], rng, seed)
    c["alpha_form"] = False
    return _probes(c, rng)


ACC_CHANNELS = (None, 1, 2, 3, 4, 5, 7, 16, 48, 65, 256)
ACC_COUNTS = BASE_RAYS + [0]


def accumulate_case(D, seed=53):
    """weights in [0, 1) with exact zeros among them, values and the incoming gradient in [-1, 1); D None: no values"""
    rng = np.random.RandomState(seed)
    cnt = list(ACC_COUNTS)
    M, N = sum(cnt), len(cnt)
    w = rng.rand(M).astype(np.float32)
    w[::17] = 0.0
    rng = np.random.RandomState(seed + 1 + (D or 0))
    u = lambda *s: torch.from_numpy((rng.rand(*s) * 2 - 1).astype(np.float32))
    return dict(cnt=cnt, N=N, M=M, D=D, w=torch.from_numpy(w), v=None if D is None else u(M, D), g=u(N, D or 1))


def accumulate_run(case, dtype):
    """-> dict(out, d_w, d_v) of loss = <out, g>"""
    w = case["w"].to(dtype).clone().requires_grad_(True)
    v = None if case["v"] is None else case["v"].to(dtype).clone().requires_grad_(True)
    out = accumulate(w, v, case["cnt"])
    gs = torch.autograd.grad((out * case["g"].to(dtype)).sum(), [w] + ([] if v is None else [v]))
    return dict(out=out.detach(), d_w=gs[0], d_v=None if v is None else gs[1])


def accumulate_scales(case):
    ray, _ = ray_index(case["cnt"])
    w, g = case["w"].double(), case["g"].double()
    v = torch.ones(case["M"], 1, dtype=F64) if case["v"] is None else case["v"].double()
    out = torch.zeros(case["N"], v.shape[1], dtype=F64).index_add(0, ray, w.abs()[:, None] * v.abs())
    return dict(out=out, d_w=(g[ray] * v).abs().sum(1), d_v=w.abs()[:, None] * g[ray].abs())
