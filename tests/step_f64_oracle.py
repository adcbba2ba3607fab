"""Float64 yardsticks, fp32 restatements and case builders for the three kernels under every training step and every rendered
pixel: the compositor (csrc/composite.hip), the weight norm (csrc/wnorm.hip) and Adam (csrc/optim.hip) -- test infrastructure,
plain torch and numpy on the CPU, like tests/glue_f64_oracle.py.

Each operation is written ONCE, dtype-generic, from its definition, in the obvious sequential order per ray, row or element, with no
reference to the shape of a kernel's scan or reduction; the gradients of the yardsticks come from torch autograd:
    compositor   the header of composite.hip as oracle/field.py:render_weights / accumulate state it; a true per-ray exclusive sum,
                 alpha = -expm1(-sd)                                                                    (composite)
    weight norm  torch._weight_norm(v, g, 0) in float64 (wnorm_f64); the fp32 restatement is the header of wnorm.hip (wnorm_f32)
    Adam         the three-line rule in the header of optim.hip, step sizes and second-moment corrections as the host entry forms
                 them: in double, then rounded to fp32                                                  (adam, adam_seg_params)
Run in float64 on the fp32 inputs they are the yardstick; run in fp32 they are the measure of what fp32 can keep: a kernel's worst
error against float64 must stay within a fixed factor of the restatement's own worst error on the same inputs (judge).

Case builders (`*_case`, `*_layout`) place the counts, tails, lanes and values at which the kernels branch;
tests/test_step_oracle_host.py asserts on the CPU that they do, tests/test_gpu_step_f64.py runs them on the GPU.
"""
import numpy as np
import torch

from tests.f64_judge import F32, F64, U, assert_figures, figures_vs_f64, report

FLOOR_ULPS = 4          # where the restatement happens to be exact a kernel is held to this many roundings of the scale


# -------------------------------------------------------------------------------------------------------- the judgement
def judge(hip, ref32, f64, scale, what, factor=2.0, slack=2):
    """The two conditions of tests/util.py:assert_close_vs_f64 at a natural scale instead of the element's own value: the kernel's
    worst error against float64 within `factor` x the fp32 restatement's own worst (or FLOOR_ULPS roundings of the scale, whichever
    is larger), and at most `factor` x as many elements (+ `slack`) above that floor as the restatement has.  Elements of zero
    scale must equal the yardstick exactly, the restatement's too.  Prints the figures and appends them to the JSON-lines file
    MORPHEUS_STEP_REPORT names, then asserts (f64_judge: figures_vs_f64, assert_figures).  -> the record the report keeps."""
    tol = FLOOR_ULPS * U
    f = figures_vs_f64(hip, ref32, f64, scale, what, tol)
    rec = dict(what=what, worst_hip=f["worst_hip"], worst_ref=f["worst_ref"], ratio=(f["worst_hip"] / f["worst_ref"] if f["worst_ref"] > 0 else None),
               n_hip=f["n_hip"], n_ref=f["n_ref"], n=f["n"], factor=factor)
    print(f"[step-f64] {what}: kernel {f['worst_hip']:.3e}  fp32 restatement {f['worst_ref']:.3e}  above {tol:.1e}: {f['n_hip']} / {f['n_ref']}  of {f['n']}")
    report("MORPHEUS_STEP_REPORT", rec)
    assert_figures(f, what, factor, tol, slack, ref_zero_scale_exact=True)
    return rec


# ============================================================================================================ compositor
def ray_index(cnt):
    """per-ray counts -> (ray [M], k [M]): the ray and the position in its ray of every packed sample"""
    cnt = torch.as_tensor(cnt, dtype=torch.long)
    ray = torch.repeat_interleave(torch.arange(cnt.numel()), cnt)
    start = torch.cumsum(cnt, 0) - cnt
    return ray, torch.arange(int(cnt.sum())) - start[ray]


def _dense(x, ray, k, N, K):
    return x.new_zeros((N, K) + tuple(x.shape[1:])).index_put((ray, k), x)


def form_sd(sigma, ts32, te32):
    """sigma * (te - ts) as the kernel forms it: the fp32 product of sigma and the fp32 difference.  In float64 the VALUE is that
    fp32 product promoted (the float64 run then integrates the same samples) and the derivative is d/d sigma = the fp32 difference."""
    dt32 = te32 - ts32
    if sigma.dtype == F32:
        return sigma * dt32
    sd32 = (sigma.detach().float() * dt32).double()
    if not sigma.requires_grad:
        return sd32
    e = sigma * dt32.double()
    return e + (sd32 - e).detach()


def composite(sigma, ts32, te32, rgb, cnt):
    """The definition, in sigma's dtype (fp32: the restatement; float64: the yardstick), one ray after the other sample by sample:
        alpha_i = -expm1(-sd_i);  T_i = exp(-sum_{j<i in ray} sd_j);  w = T alpha
        opacity = sum w;  depth = sum w (ts + te) / 2;  color = sum w rgb
    cnt: samples per ray (packed, contiguous).  -> weights [M], opacity [N], depth [N], color [N, 3] (None without rgb)"""
    dtype = sigma.dtype
    cnt = [int(c) for c in cnt]
    N, K = len(cnt), max(cnt + [0])
    ray, k = ray_index(cnt)
    sd = _dense(form_sd(sigma, ts32, te32), ray, k, N, K)
    tmid = _dense((ts32.to(dtype) + te32.to(dtype)) * 0.5, ray, k, N, K)
    live = _dense(torch.ones(ray.numel(), dtype=torch.bool), ray, k, N, K)
    acc, cols = sd.new_zeros(N), []
    for j in range(K):                       # the exclusive sum never contains the sample's own term
        cols.append(acc)
        acc = acc + sd[:, j]
    excl = torch.stack(cols, 1) if K else sd.new_zeros(N, 0)
    w = torch.where(live, torch.exp(-excl) * -torch.expm1(-sd), sd.new_zeros(()))
    rgb_d = None if rgb is None else _dense(rgb, ray, k, N, K)
    opacity, depth, color = sd.new_zeros(N), sd.new_zeros(N), sd.new_zeros(N, 3)
    for j in range(K):
        opacity = opacity + w[:, j]
        depth = depth + w[:, j] * tmid[:, j]
        if rgb_d is not None:
            color = color + w[:, j, None] * rgb_d[:, j]
    return w[ray, k], opacity, depth, (None if rgb is None else color)


VARIANTS = ("wodc", "w", "o", "d", "c", "wo", "wd", "od")       # which outputs the loss reaches; the last three leave g_color absent


def composite_loss(outs, case, variant, dtype=None, dev=None):
    """sum of <output, its probe> over the outputs named in `variant` (linear: the kernel's incoming gradients ARE the probes)"""
    terms = []
    for name, out in zip("wodc", outs):
        if name in variant and out is not None:
            g = case["g_" + name]
            g = g.to(dtype or out.dtype)
            terms.append((out * (g.to(dev) if dev else g)).sum())
    return sum(terms)


def composite_run(case, dtype, variants=VARIANTS, with_rgb=True):
    """forward once, then d/d sigma and d/d rgb of every loss variant by autograd.
    -> dict(w, o, d, c, grads={variant: (d_sigma, d_rgb)})"""
    sigma = case["sigma"].detach().to(dtype).clone().requires_grad_(True)
    rgb = case["rgb"].detach().to(dtype).clone().requires_grad_(True) if with_rgb else None
    outs = composite(sigma, case["ts"], case["te"], rgb, case["cnt"])
    grads = {}
    for var in variants:
        loss = composite_loss(outs, case, var)
        leaves = [sigma] + ([rgb] if with_rgb else [])
        gs = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
        d_rgb = None if not with_rgb else (torch.zeros_like(rgb) if gs[1] is None else gs[1])
        grads[var] = (gs[0], d_rgb)
    w, o, d, c = (None if t is None else t.detach() for t in outs)
    return dict(w=w, o=o, d=d, c=c, grads=grads)


def composite_scales(case, f64run, variant="wodc", with_rgb=True):
    """The natural scales the errors are divided by, all from the float64 run:
        weights  the ray's total weight          opacity  the same          depth  sum w |tmid|          color  the ray's total weight
        d_sigma  dt_i x the largest |g_j| of the ray (|d_sigma_i| <= dt_i max|g|: T <= 1, sum w <= 1), g_j the gradient reaching w_j
        d_rgb    the ray's total weight x the largest |g_color| component of the ray"""
    ray, _ = ray_index(case["cnt"])
    N = len(case["cnt"])
    w = f64run["w"]
    tot = torch.zeros(N, dtype=F64).index_add(0, ray, w)
    tmid = (case["ts"].double() + case["te"].double()) * 0.5
    g = torch.zeros_like(w)
    if "w" in variant:
        g = g + case["g_w"].double()
    if "o" in variant:
        g = g + case["g_o"].double()[ray]
    if "d" in variant:
        g = g + case["g_d"].double()[ray] * tmid
    gc = case["g_c"].double() if ("c" in variant and with_rgb) else torch.zeros(N, 3, dtype=F64)
    g = g + (gc[ray] * case["rgb"].double()).sum(-1)
    gmax = torch.zeros(N, dtype=F64).scatter_reduce(0, ray, g.abs(), "amax")
    dt = (case["te"] - case["ts"]).double()
    return dict(w=tot[ray], o=tot, d=torch.zeros(N, dtype=F64).index_add(0, ray, w * tmid.abs()), c=tot[:, None].expand(-1, 3),
                d_sigma=dt * gmax[ray], d_rgb=(tot * gc.abs().amax(-1))[ray][:, None].expand(-1, 3))


COUNTS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 350, 1025]
BASE_RAYS = [0, 1, 2, 63, 64, 65, 0, 0, 127, 128, 129, 191, 192, 193, 350, 1025]      # + a 0-count ray appended last
OPAQUE_SD = (30.0, 1e2, 1e4)
OPAQUE_AT = (0, 63, 64, 128)      # lane 0, lane 63, the first lane of the second and of the third chunk


def _assemble(rays, rng, seed):
    """rays: list of per-ray arrays of optical depths sd (float64 targets).  Samples of a ray are contiguous in t; dt in
    [0.002, 0.022); sigma = sd / dt in fp32.  -> case dict (fp32 tensors on the CPU)"""
    cnt = [len(r) for r in rays]
    M, N = sum(cnt), len(rays)
    dt = (rng.rand(M) * 0.02 + 0.002).astype(np.float32)
    ts = np.concatenate([0.05 + np.concatenate([[0.0], np.cumsum(dt[s:s + c][:-1], dtype=np.float64)]) for s, c in
                         zip(np.cumsum([0] + cnt[:-1]), cnt) if c] or [np.zeros(0)]).astype(np.float32)
    te = ts + dt
    sd = np.concatenate(rays + [np.zeros(0)])
    sigma = (sd / (te - ts).astype(np.float64)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    u = lambda *s: t((rng.rand(*s) * 2 - 1).astype(np.float32))
    return dict(cnt=cnt, N=N, M=M, sigma=t(sigma), ts=t(ts), te=t(te), rgb=t(rng.rand(M, 3).astype(np.float32)),
                g_w=u(M), g_o=u(N), g_d=u(N), g_c=u(N, 3), placed={})


def _log_uniform(rng, n, lo, hi):
    return 10.0 ** (np.log10(lo) + rng.rand(n) * (np.log10(hi) - np.log10(lo)))


def _drawn_ray(rng, c, translucent):
    """optical depth log-uniform over 1e-7 .. 1e2 (opaque within a dozen samples); translucent: log-uniform over 1e-7 .. 6 / c, so
    that the ray keeps weight to its last sample and every chunk's carry matters"""
    return _log_uniform(rng, c, 1e-7, max(6.0 / max(c, 1), 1e-6) if translucent else 1e2)


def composite_main_case(seed=11):
    """Every sample count of COUNTS (a 0-count ray first, last and two adjacent), then the placed rays:
        opaque <sd> @<k>   one sample of sd 30 / 1e2 / 1e4 at position k = 0, 63, 64, 128 behind a thin prefix (sd ~ 1e-3 each), 3 thin behind it
        sigma = 0          a translucent ray of 70 with sigma = 0 at 0, 5, 63, 64, 69
        ts == te           the same with zero-length samples
        underflow          100 samples: 40 of sd 0.1, then sd 20 each -- the fp32 transmittance reaches 0 near position 45, mid-chunk
        thin               200 samples of sd ~ 1e-6
    33 rays: one ray in the last workgroup."""
    rng = np.random.RandomState(seed)
    rays = [_drawn_ray(rng, c, r % 2 == 1 or c >= 350) for r, c in enumerate(BASE_RAYS)]      # odd rays and the two longest: translucent
    placed = {}
    for sd_big in OPAQUE_SD:
        for at in OPAQUE_AT:
            ray = _log_uniform(rng, at + 4, 5e-4, 2e-3)
            ray[at] = sd_big
            placed[f"opaque {sd_big:g} @{at}"] = (len(rays), at)
            rays.append(ray)
    zero_at = (0, 5, 63, 64, 69)
    placed["sigma = 0"] = (len(rays), zero_at)
    rays.append(_log_uniform(rng, 70, 1e-3, 5e-2))
    placed["ts == te"] = (len(rays), zero_at)
    rays.append(_log_uniform(rng, 70, 1e-3, 5e-2))
    placed["underflow"] = (len(rays), 45)
    rays.append(np.concatenate([np.full(40, 0.1), np.full(60, 20.0)]))
    placed["thin"] = (len(rays), None)
    rays.append(_log_uniform(rng, 200, 5e-7, 2e-6))
    rays.append(np.zeros(0))
    c = _assemble(rays, rng, seed)
    start = np.cumsum([0] + c["cnt"][:-1])
    r, ks = placed["sigma = 0"]
    c["sigma"][[int(start[r]) + k for k in ks]] = 0.0
    r, ks = placed["ts == te"]
    idx = [int(start[r]) + k for k in ks]
    c["te"][idx] = c["ts"][idx]
    c["placed"] = placed
    return c


RAY_COUNTS = (1, 3, 4, 5, 257)      # 1, 3, 0 and 1 rays in the last workgroup of four


def composite_rays_case(N, seed=23):
    rng = np.random.RandomState(seed + N)
    small = [65, 0, 3, 129, 1]
    cnt = small[:N] if N <= 5 else [int(x) for x in rng.randint(0, 40, size=N)]
    if N > 5:
        cnt[0], cnt[100], cnt[101], cnt[255], cnt[256] = 0, 0, 0, 64, 66
    return _assemble([_drawn_ray(rng, c, r % 2 == 1) for r, c in enumerate(cnt)], rng, seed)


NONFINITE_COUNTS = [5, 70, 3, 64, 130, 2, 65, 1, 9, 66, 4, 7]     # three workgroups
NONFINITE_AT = (5, 1)              # ray 5 (workgroup 1), its second sample
INF_AT = (4, 66)                   # ray 4, lane 2 of its second chunk


def composite_nonfinite_case(kind=None, seed=31):
    """twelve translucent rays; kind None: all finite; "nan": sigma = NaN at NONFINITE_AT; "inf": sigma = +inf at INF_AT"""
    rng = np.random.RandomState(seed)
    c = _assemble([_log_uniform(rng, n, 1e-4, 3.0 / n) for n in NONFINITE_COUNTS], rng, seed)
    start = np.cumsum([0] + c["cnt"][:-1])
    if kind == "nan":
        c["sigma"][int(start[NONFINITE_AT[0]]) + NONFINITE_AT[1]] = float("nan")
    elif kind == "inf":
        c["sigma"][int(start[INF_AT[0]]) + INF_AT[1]] = float("inf")
    return c


def composite_reorder(case, order):
    """the same rays presented in another order -> (case, index of every new packed sample in the old packed arrays)"""
    start = np.cumsum([0] + case["cnt"][:-1])
    idx = torch.from_numpy(np.concatenate([np.arange(start[r], start[r] + case["cnt"][r]) for r in order] + [np.zeros(0)]).astype(np.int64))
    order_t = torch.as_tensor(list(order))
    out = dict(case, cnt=[case["cnt"][r] for r in order])
    for k in ("sigma", "ts", "te", "rgb", "g_w"):
        out[k] = case[k][idx]
    for k in ("g_o", "g_d", "g_c"):
        out[k] = case[k][order_t]
    return out, idx


def composite_padded_layout(cnt, gaps=((0, 3), (2, 1), (7, 66)), trailing=7):
    """ray starts with packed entries that no ray owns behind rays 0, 2 and 7 and behind the last ray -> (start, M_padded, owned index)"""
    gap = dict(gaps)
    start, pos = [], 0
    for r, c in enumerate(cnt):
        start.append(pos)
        pos += c + gap.get(r, 0)
    owned = np.concatenate([np.arange(s, s + c) for s, c in zip(start, cnt)] + [np.zeros(0)]).astype(np.int64)
    return start, pos + trailing, torch.from_numpy(owned)


# =========================================================================================================== weight norm
def wnorm_f64(v, g):
    """the yardstick: torch._weight_norm on float64 copies (differentiate it with autograd)"""
    return torch._weight_norm(v, g, 0)


def wnorm_f32(v, g, dw=None):
    """The header of wnorm.hip in fp32, column after column:  W = v g / ||v||;  dg = <dW, v> / ||v||;
    dv = (g / ||v||) (dW - v <dW, v> / ||v||^2).  -> W, dv, dg (dv, dg None without dW)"""
    assert v.dtype == F32
    R, C = v.shape
    ss, dot = v.new_zeros(R), v.new_zeros(R)
    for c in range(C):
        ss = ss + v[:, c] * v[:, c]
        if dw is not None:
            dot = dot + dw[:, c] * v[:, c]
    norm = torch.sqrt(ss)
    s = g[:, 0] / norm
    W = v * s[:, None]
    if dw is None:
        return W, None, None
    return W, s[:, None] * (dw - v * (dot / (norm * norm))[:, None]), (dot / norm)[:, None]


WN_COLS = (1, 2, 63, 64, 65, 127, 128, 129, 300)
WN_CALLS = {
    # rows per layer; the cumulated row ends mod 4 are 1, 3, 2, 3, 3, 0, 2, 1, 2: a layer boundary at every wave of a workgroup
    "nine": dict(rows=(1, 2, 3, 5, 128, 1, 2, 3, 5), cols=WN_COLS),                                      # 150 rows: 2 in the tail
    "one": dict(rows=(5,), cols=(65,)),                                                                 # 5 rows: 1 in the tail
    "thirty-two": dict(rows=(128,) + (2, 3, 5) + (1, 2, 3, 5) * 7, cols=(WN_COLS * 4)[:32]),             # 215 rows: 3 in the tail
}
WN_GRAD_KINDS = ("random", "parallel", "orthogonal")


def wnorm_case(name, kind="random", seed=41):
    """v rows of scale 2^e, e drawn from -40 .. 40 per row; g of both signs, every seventh row's exactly 0; dW random, parallel to
    v (the exact dv is 0) or orthogonal to v (orthogonalised in float64, then rounded: the exact dg is ~0)"""
    spec = WN_CALLS[name]
    rng = np.random.RandomState(seed + len(spec["rows"]))
    vs, gs, dws = [], [], []
    row = 0
    for R, C in zip(spec["rows"], spec["cols"]):
        e = rng.randint(-40, 41, size=(R, 1)).astype(np.float64)
        v = (rng.randn(R, C) * 2.0 ** e).astype(np.float32)
        v[v == 0] = np.float32(2.0 ** -40)
        g = rng.randn(R, 1).astype(np.float32)
        g[(np.arange(row, row + R) % 7) == 3] = 0.0
        u = rng.randn(R, C)
        v64 = v.astype(np.float64)
        if kind == "parallel":
            dw = v64 * rng.randn(R, 1)
        elif kind == "orthogonal":
            # (a single column has no orthogonal direction: dW = 0 there)
            dw = (u * np.abs(v64).max(1, keepdims=True)) if C > 1 else np.zeros((R, C))
            dw = dw - v64 * ((dw * v64).sum(1, keepdims=True) / (v64 * v64).sum(1, keepdims=True))
            dw = dw / np.maximum(np.abs(dw).max(1, keepdims=True), 1e-300)
        else:
            dw = u
        vs.append(torch.from_numpy(v)), gs.append(torch.from_numpy(g)), dws.append(torch.from_numpy(dw.astype(np.float32)))
        row += R
    return dict(vs=vs, gs=gs, dws=dws, rows=spec["rows"], cols=spec["cols"])


def wnorm_reference(case, with_grad):
    """per layer: float64 (W, dv, dg) by autograd and the fp32 restatement's; with_grad[l] False: no gradient reaches layer l
    (dv = dg = 0).  -> list of dict(f64=(W, dv, dg), f32=(W, dv, dg), scale=(W, dv, dg))
    scales: W  the row's largest |W|;  dv  s max|dW_row|, s = |g| / ||v||;  dg  sum |dW v| / ||v||"""
    out = []
    for v, g, dw, on in zip(case["vs"], case["gs"], case["dws"], with_grad):
        v, g = v.detach(), g.detach()
        v64, g64 = v.double().requires_grad_(True), g.double().requires_grad_(True)
        W64 = wnorm_f64(v64, g64)
        if on:
            (W64 * dw.double()).sum().backward()
            dv64, dg64 = v64.grad, g64.grad
            W32, dv32, dg32 = wnorm_f32(v, g, dw)
        else:
            dv64, dg64 = torch.zeros_like(v64), torch.zeros_like(g64)
            W32, dv32, dg32 = wnorm_f32(v, g)[0], torch.zeros_like(v), torch.zeros_like(g)
        norm = v.double().norm(dim=1, keepdim=True)
        s = g.double().abs() / norm
        sc_dv = (s * dw.double().abs().amax(1, keepdim=True)).expand_as(v) * (1.0 if on else 0.0)
        sc_dg = (dw.double() * v.double()).abs().sum(1, keepdim=True) / norm * (1.0 if on else 0.0)
        out.append(dict(f64=(W64.detach(), dv64, dg64), f32=(W32, dv32, dg32),
                        scale=(W64.detach().abs().amax(1, keepdim=True).expand_as(v), sc_dv, sc_dg)))
    return out


# ================================================================================================================== Adam
BETA1, BETA2, EPS = (float(np.float32(x)) for x in (0.9, 0.99, 1e-15))      # what a float parameter of the C ABI holds
STEP_COUNTS = (1, 2, 10, 1000, 10 ** 6)
ADAM_N = (1, 2, 3, 4, 5, 1023, 1024, 1025, 2049)      # 2049 > 256 * 4 * 2: a third block of one lane holding one element
ADAM_MAX_SEGS = 160


def adam_seg_params(lrs, steps, b1=BETA1, b2=BETA2, round32=True):
    """per segment (step size, sqrt of the second-moment correction) as mh_adam_step forms them: lr / (1 - b1^t) and
    sqrt(1 - b2^t) in double, then rounded to fp32; step 0: skipped (-1, 1)"""
    ss, bc = [], []
    for lr, t in zip(lrs, steps):
        if t == 0:
            ss.append(-1.0), bc.append(1.0)
            continue
        lr = float(np.float32(lr)) if round32 else float(lr)
        a, b = lr / (1.0 - b1 ** float(t)), (1.0 - b2 ** float(t)) ** 0.5
        ss.append(float(np.float32(a)) if round32 else a), bc.append(float(np.float32(b)) if round32 else b)
    return np.array(ss, np.float64), np.array(bc, np.float64)


def adam_seg_of(ends, n):
    """the segment of every element: the first whose end lies beyond it"""
    return np.searchsorted(np.asarray(ends, np.int64), np.arange(n), side="right")


def adam(p, g, m, v, ss, bc2, dtype, b1=BETA1, b2=BETA2, eps=EPS):
    """The rule of optim.hip's header element by element in `dtype`; ss, bc2: per-ELEMENT step size (< 0: skipped, untouched) and
    second-moment correction.   m = m + (g - m)(1 - b1);  v = b2 v + (1 - b2) g g;  p -= ss m / (sqrt(v) / bc2 + eps)"""
    p, g, m, v, ss, bc2 = (np.asarray(a).astype(dtype) for a in (p, g, m, v, ss, bc2))
    one, b1, b2, eps = dtype(1.0), dtype(b1), dtype(b2), dtype(eps)
    with np.errstate(all="ignore"):
        m2 = m + (g - m) * (one - b1)
        v2 = b2 * v + (one - b2) * g * g
        p2 = p - ss * m2 / (np.sqrt(v2) / bc2 + eps)
    on = ss >= 0
    assert m2.dtype == v2.dtype == p2.dtype == dtype
    return np.where(on, p2, p), np.where(on, m2, m), np.where(on, v2, v)


# straddling lanes of the "mixed" layout (elements 0 .. 19):    1+3        2+2       3+1      1+3      1+1+2
ADAM_MIX_ENDS = [1, 6, 11, 12, 13, 16, 17, 18, 20]
ADAM_MIXES = {0: (1, 3), 1: (2, 2), 2: (3, 1), 3: (1, 3), 4: (1, 1, 2)}


def adam_layout(n, kind):
    """-> (ends, steps, lrs) of a bucket of n elements.
    one     a single segment
    mixed   a zero-length segment first, ADAM_MIX_ENDS, two zero-length segments in a row, odd-length segments of 7, 9, 33, 31, the rest (stepped),
            and a zero-length segment last; stepped and skipped segments alternate (ends beyond n are clipped to n: for n < 20 the
            trailing segments are empty)
    160     160 segments of lengths 1, 2, 3, 5, 0, ... and the rest in the last
    Stepped non-empty segments take their step count from STEP_COUNTS and their learning rate from 1e-2, 5e-3, 1e-3, 0, 2e-4 in turn."""
    if kind == "one":
        ends = [n]
    elif kind == "mixed":
        ends = [0] + ADAM_MIX_ENDS + [20, 20, 27, 36, 69, 100, n, n]
    else:
        lens = [(1, 2, 3, 5, 0)[i % 5] for i in range(ADAM_MAX_SEGS - 1)]
        ends = list(np.cumsum(lens)) + [n]
    ends = [int(min(e, n)) for e in ends]
    ends[-1] = n
    lr_cycle = (1e-2, 5e-3, 1e-3, 0.0, 2e-4)
    steps, lrs, j = [], [], 0
    for s in range(len(ends)):
        skipped = (kind != "one") and (s % 2 == 1)
        empty = ends[s] == (ends[s - 1] if s else 0)
        if skipped or empty:              # (an empty stepped segment takes no turn of the cycles)
            steps.append(0 if skipped else 3), lrs.append(1e-2)
            continue
        steps.append(STEP_COUNTS[j % 5]), lrs.append(lr_cycle[j % 5])
        j += 1
    return ends, steps, lrs


def adam_state(n, seed=53):
    """p ~ 0.1 N(0, 1); per element a gradient scale 10^U(-18, 4) (its square a normal fp32 number), live moments of that scale;
    element i with i % 7 == 0: zero moments (and a zero gradient), i % 7 == 1: a zero gradient into live moments"""
    rng = np.random.RandomState(seed + n)
    scale = 10.0 ** (rng.rand(n) * 22.0 - 18.0)
    p = (rng.randn(n) * 0.1).astype(np.float32)
    m = (rng.randn(n) * 0.3 * scale).astype(np.float32)
    v = ((rng.rand(n) + 0.5) * scale * scale).astype(np.float32)
    i = np.arange(n)
    m[i % 7 == 0], v[i % 7 == 0] = 0.0, 0.0
    return dict(p=p, m=m, v=v, scale=scale, n=n)


def adam_grad(state, it):
    """the gradient of iteration `it`: the element's scale x a factor in +-[0.5, 2); exact zeros at i % 7 in (0, 1)"""
    n = state["n"]
    rng = np.random.RandomState(977 + 31 * it + n)
    g = (state["scale"] * (0.5 + 1.5 * rng.rand(n)) * np.where(rng.rand(n) < 0.5, -1.0, 1.0)).astype(np.float32)
    i = np.arange(n)
    g[(i % 7 == 0) | (i % 7 == 1)] = 0.0
    return g


def adam_scales(p, g, m, v, ss, dtype=np.float64, b1=BETA1, b2=BETA2):
    """natural scales of one step, from the float64 state BEFORE it: parameter  the step size (the size of a parameter move; 0 for
    a skipped element or a learning rate of 0: exact);  exp_avg  |m| + (1 - b1) |g|;  exp_avg_sq  b2 v + (1 - b2) g^2, its own value"""
    g, m, v = (np.asarray(a, np.float64) for a in (g, m, v))
    on = np.asarray(ss) >= 0
    return (np.where(on, np.asarray(ss, np.float64), 0.0), np.where(on, np.abs(m) + (1.0 - b1) * np.abs(g), 0.0),
            np.where(on, b2 * v + (1.0 - b2) * g * g, 0.0))
