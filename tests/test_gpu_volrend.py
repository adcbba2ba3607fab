"""morpheus_amd.volrend (csrc/volrend.hip) against float64 at its scan, tail and branch edges; tests/volrend_oracle.py holds the
yardsticks, the fp32 restatements, the cases and the natural scales, tests/test_volrend_host.py shows on the CPU that the cases
reach what they name.

The rule, not fitted to a run (volrend_oracle.judge = f64_judge.judge_vs_f64): errors are |x - float64| over the quantity's natural
scale; a kernel's worst error stays within 2 x the worst error of the sequential fp32 restatement on the same inputs (floor: 4
roundings of the scale), with at most 2 x (+ 2) as many elements above that floor; elements of zero scale are exact.  Everything
else is exact: zeros, untouched buffers, bit-for-bit equalities between routes.  Every judged check prints its figures and
appends them to the JSON-lines file that MORPHEUS_VOLREND_REPORT names.

Worst figures of one run on an MI355X (error / scale; worst over the module's checks of the quantity, with the restatement's figure
of the same check).  The floor is 2.38e-07; no factor is raised above 2.

    quantity                          scale                                   kernel     fp32 restatement
    weights, density form             the ray's total weight                  4.30e-08   2.21e-08
    trans, density form               1                                       5.59e-08   1.15e-07
    alphas, density form              1                                       2.96e-08   2.96e-08
    d_sigma                           dt_i x the ray's largest |g|            2.01e-06   5.28e-06
    weights, alpha form               the ray's total weight                  3.44e-08   6.76e-08
    trans, alpha form                 1                                       2.98e-08   2.53e-07
    d_alpha                           the sum of its absolute terms           9.01e-08   3.88e-07
    d_alpha, underflow ray            the same                                1.00e+00   1.00e+00
    accumulate, out (D = 256)         sum |w| |v|                             1.67e-07   1.46e-07
    accumulate, d_weights (D = 5)     sum_c |g v|                             1.43e-07   1.05e-07
    accumulate, d_values              |w| |g|                                 5.95e-08   5.95e-08
    composition: opacity              the ray's total weight                  6.76e-08   5.08e-07
    composition: depth                sum w |tmid|                            1.52e-07   3.61e-07
    composition: colour               the ray's total weight                  9.42e-08   2.74e-07
    composition: white image          1                                       9.42e-08   1.63e-07
    composition: d_sigma              dt_i x the ray's largest |g_j|          2.21e-07   2.16e-07   (fused compositor: 1.88e-07)
    composition: d_rgb                total weight x largest |g_color|        4.71e-08   7.53e-08
The four-call composition's forward results and d_rgb equal the fused compositor's in every figure; 1613 of 1613 weights are
bit-identical.  Behind the underflow of the alpha form fp32 holds 0 where float64 holds 1e-60, and d_alpha is measured against its
own (equally small) terms: restatement and kernel are both wrong by the whole scale there, which is why that ray is judged by itself.
With the alpha form's factors and running product in fp32 (a wave scan of fp32 products, as first written) trans stood at 3.1e-07
with 36 elements above the floor against the restatement's 3, and d_alpha at 4.3e-07 against 2.2e-07: a product of n factors carries
n - 1 roundings in any order, so the scan was no better than the loop; the kernel now forms 1 - alpha, the product and the suffix
sums of the alpha form in double.
"""
import numpy as np
import pytest
import torch

from tests import step_f64_oracle as S
from tests import volrend_oracle as V
from tests.f64_judge import flat64

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
MH_ERR_ARG = 1
SENTINEL = -77.25

def _status(name, *args):
    """call a stream-taking entry point of the C ABI and hand back its status instead of raising"""
    from morpheus_amd import _lib
    _lib.load()
    return _lib._fns[name](*args, _lib.stream())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


def _pool(records, key, hip, ref32, f64, scale):
    h, c, r, s = records.setdefault(key, ([], [], [], []))
    f64 = flat64(f64)
    scale = torch.full_like(f64, float(scale)) if isinstance(scale, (int, float)) else flat64(scale)
    for lst, t in ((h, hip), (c, ref32), (r, f64), (s, scale)):
        lst.append(flat64(t))


def _judge_pool(records, prefix):
    return {key: V.judge(*(torch.cat(x) for x in v), f"{prefix} {key}") for key, v in records.items()}


_REF = {}


def _ref(name, build, run):
    """the case, its float64 run and its fp32 restatement: computed once, shared, never modified"""
    if name not in _REF:
        case = build()
        _REF[name] = (case, run(case, F64), run(case, F32))
    return _REF[name]


def _ray_idx(case, dtype=torch.int64):
    return S.ray_index(case["cnt"])[0].to(dtype).to(DEV)


# ================================================================================================================== weights
def _weights_gpu(case, r64, r32, variants, pool, **route):
    """render_weight_from_density / _from_alpha on the case (ray_indices int64 + n_rays unless `route` says otherwise); forward
    outputs and the gradient of every loss variant into `pool` -> the outputs"""
    from morpheus_amd import volrend
    alpha_form = case["alpha_form"]
    route = route or dict(ray_indices=_ray_idx(case), n_rays=case["N"])
    x = case["alpha" if alpha_form else "sigma"].to(DEV).requires_grad_(True)
    if alpha_form:
        outs = volrend.render_weight_from_alpha(x, **route)
    else:
        outs = volrend.render_weight_from_density(case["ts"].to(DEV), case["te"].to(DEV), x, **route)
    assert len(outs) == (2 if alpha_form else 3)
    sc = V.weights_scales(case, r64, "w")
    for k, name, out in zip("wTa", ("weights", "trans", "alphas"), outs):
        _pool(pool, name, out, r32[k], r64[k], sc[k])
    for var in variants:
        d, = torch.autograd.grad(V.weights_loss(outs, case, var, dev=DEV), [x], retain_graph=True)
        scale = V.weights_scales(case, r64, var)["d_in"]
        for name, mask in V.gradient_pools(case).items():
            _pool(pool, name, d.cpu()[mask], r32["grads"][var][mask], r64["grads"][var][mask], scale[mask])
    return outs, x


@pytest.mark.parametrize("form", ["density", "alpha"])
def test_weights_every_count_and_placed_sample(form):
    """Counts 0, 1, 2, 63, 64, 65, 127, 128, 129, 350 with empty rays first, last and adjacent; an opaque sample (sd 30, 1e2, 1e4, or
    alpha == 1 exactly) at lane 0, lane 63 and lane 64; sigma = 0, ts == te, alpha = 0; a transmittance that underflows mid-chunk
    with live gradients behind it; two alpha == 1 samples in one ray; 1 - alpha = 2^-20.  Losses: each output alone, each pair, all:
    the absent ones reach the kernel as NULL pointers."""
    from morpheus_amd import volrend
    alpha_form = form == "alpha"
    case, r64, r32 = _ref(form, V.alpha_case if alpha_form else V.density_case, V.weights_run)
    pool = {}
    outs, x = _weights_gpu(case, r64, r32, V.ALPHA_VARIANTS if alpha_form else V.DENSITY_VARIANTS, pool)
    _judge_pool(pool, f"volrend {form} form, every count:")
    w, T = outs[0].detach().cpu(), outs[1].detach().cpu()
    start = V._start(case["cnt"])
    exact0 = [f"alpha = 1 @{at}" for at in V.OPAQUE_AT] if alpha_form else [f"opaque 10000 @{at}" for at in V.OPAQUE_AT]
    for name in exact0:
        r, k = case["placed"][name]
        behind = slice(int(start[r]) + k + 1, int(start[r]) + case["cnt"][r])
        assert behind.stop - behind.start == V.BEHIND
        assert bool((w[behind] == 0).all()) and bool((T[behind] == 0).all()), f"{name}: weights and trans behind it exactly 0"
    r, _ = case["placed"]["underflow"]
    tail = slice(int(start[r]) + 64, int(start[r]) + case["cnt"][r])
    assert bool((w[tail] == 0).all()) and bool((T[tail] == 0).all()), "behind the underflow the fp32 results are exactly 0"
    for name in (("alpha = 0",) if alpha_form else ("sigma = 0", "ts == te")):
        r, ks = case["placed"][name]
        assert bool((w[[int(start[r]) + k for k in ks]] == 0).all()), f"{name}: weight exactly 0"
    if alpha_form:
        r, (k0, k1) = case["placed"]["two opaque"]
        d, = torch.autograd.grad(outs[0].sum() + outs[1].sum(), [x], retain_graph=True)
        s = int(start[r])
        assert bool(torch.isfinite(d).all()) and bool((d[s + k1 + 1:s + case["cnt"][r]] == 0).all()), "behind the second opaque sample: no gradient"
    # the transmittance-only calls (no weights written) give the same bits, forward and backward
    ri, n = _ray_idx(case), case["N"]
    x2 = x.detach().clone().requires_grad_(True)
    if alpha_form:
        outs2 = (volrend.render_transmittance_from_alpha(x2, ray_indices=ri, n_rays=n),)
    else:
        outs2 = volrend.render_transmittance_from_density(case["ts"].to(DEV), case["te"].to(DEV), x2, ray_indices=ri, n_rays=n)
    assert all(_same_bits(a, b) for a, b in zip(outs2, outs[1:]))
    var = "T" if alpha_form else "Ta"
    d1, = torch.autograd.grad(V.weights_loss(outs, case, var, dev=DEV), [x])
    d2, = torch.autograd.grad(V.weights_loss((None,) + tuple(outs2), case, var, dev=DEV), [x2])
    assert _same_bits(d1, d2)


@pytest.mark.parametrize("form", ["density", "alpha"])
def test_weights_ray_counts_around_a_workgroup(form):
    """N = 1, 4, 5 rays: 1, 4 and 1 rays in the last workgroup of four waves; all-outputs loss"""
    alpha_form = form == "alpha"
    pool = {}
    for N in V.RAY_COUNTS:
        case, r64, r32 = _ref(f"{form}{N}", lambda: V.rays_case(N, alpha_form), V.weights_run)
        _weights_gpu(case, r64, r32, ("wT" if alpha_form else "wTa",), pool)
    _judge_pool(pool, f"volrend {form} form, ray counts:")


def _composition(case, sigma, rgb, **route):
    """the reference's four calls (morpheus.py:675-685) in the project's own words -> weights, opacity [N], depth [N], colour [N, 3]"""
    from morpheus_amd import volrend
    ts, te = case["ts"].to(DEV), case["te"].to(DEV)
    ri, n = _ray_idx(case), case["N"]
    weights, _, _ = volrend.render_weight_from_density(ts, te, sigma, **(route or dict(ray_indices=ri, n_rays=n)))
    opacity = volrend.accumulate_along_rays(weights, values=None, ray_indices=ri, n_rays=n)
    depth = volrend.accumulate_along_rays(weights, values=((ts + te) / 2)[:, None], ray_indices=ri, n_rays=n)
    colour = volrend.accumulate_along_rays(weights, values=rgb, ray_indices=ri, n_rays=n)
    assert opacity.shape == (n, 1) and depth.shape == (n, 1) and colour.shape == (n, 3)
    return weights, opacity[:, 0], depth[:, 0], colour


def test_nonfinite_samples():
    """The assertions of test_composite_inf_and_nan_samples, forward only.  sigma = +inf: w = T there, exact zeros behind it, finite
    sums, judged against float64.  sigma = NaN poisons its own ray only: every other ray equals the batch without it bit for bit."""
    clean = S.composite_nonfinite_case()
    with torch.no_grad():
        clean_out = _composition(clean, clean["sigma"].to(DEV), clean["rgb"].to(DEV))
        ray, k = S.ray_index(clean["cnt"])
        case = S.composite_nonfinite_case("inf")
        outs = _composition(case, case["sigma"].to(DEV), case["rgb"].to(DEV))
        assert all(bool(torch.isfinite(o).all()) for o in outs)
        o64 = S.composite(case["sigma"].double(), case["ts"], case["te"], case["rgb"].double(), case["cnt"])
        o32 = S.composite(case["sigma"], case["ts"], case["te"], case["rgb"], case["cnt"])
        sc = S.composite_scales(case, dict(w=o64[0]))
        for name, key, h, c, r in zip(("weights", "opacity", "depth", "colour"), "wodc", outs, o32, o64):
            V.judge(h, c, r, sc[key], f"volrend, sigma = +inf: {name}")
        at = (ray == S.INF_AT[0]) & (k == S.INF_AT[1])
        behind = (ray == S.INF_AT[0]) & (k > S.INF_AT[1])
        w = outs[0].cpu()
        assert int(behind.sum()) == S.NONFINITE_COUNTS[S.INF_AT[0]] - S.INF_AT[1] - 1 and bool((w[behind] == 0).all())
        assert float(w[at]) > 0.05, "alpha = 1: the sample takes the whole remaining transmittance"
        case = S.composite_nonfinite_case("nan")
        outs = _composition(case, case["sigma"].to(DEV), case["rgb"].to(DEV))
    own = ray == S.NONFINITE_AT[0]
    others = torch.arange(case["N"]) != S.NONFINITE_AT[0]
    assert _same_bits(outs[0][(~own).to(DEV)], clean_out[0][(~own).to(DEV)])
    for o, c in zip(outs[1:], clean_out[1:]):
        assert _same_bits(o[others.to(DEV)], c[others.to(DEV)])
        assert bool(torch.isnan(o[S.NONFINITE_AT[0]]).all())
    before = own & (k < S.NONFINITE_AT[1])
    assert _same_bits(outs[0][before.to(DEV)], clean_out[0][before.to(DEV)])
    assert bool(torch.isnan(outs[0][(own & (k >= S.NONFINITE_AT[1])).to(DEV)]).all())


# ================================================================================================================ pack_info
PACK_CASES = {"ragged": (V.BASE_RAYS + [0], 0), "n_rays beyond the largest index": ([3, 0, 2], 4), "one sample": ([0, 0, 1, 0], 0),
              "one sample, one ray": ([1], 0), "every other ray empty": ([0, 5, 0, 70, 0, 1, 0], 0)}


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("name", list(PACK_CASES))
def test_pack_info(name, dtype):
    """int32 and int64 indices, n_rays larger than the largest index, rays without samples in every position, M = 1: equal to
    bincount / cumsum on the CPU"""
    from morpheus_amd import volrend
    cnt, extra = PACK_CASES[name]
    n = len(cnt) + extra
    idx = S.ray_index(cnt)[0]
    info = volrend.pack_info(idx.to(dtype).to(DEV), n)
    want_cnt = torch.bincount(idx, minlength=n)
    want = torch.stack((torch.cumsum(want_cnt, 0) - want_cnt, want_cnt), 1)
    assert info.dtype == torch.int64 and info.shape == (n, 2) and torch.equal(info.cpu(), want)


def test_packed_info_route_gives_the_same_bits():
    """pack_info's result is accepted back as packed_info by every function that takes one, with the bits of the ray_indices route"""
    from morpheus_amd import volrend
    case = _ref("density", V.density_case, V.weights_run)[0]
    acase = _ref("alpha", V.alpha_case, V.weights_run)[0]
    with torch.no_grad():
        for c in (case, acase):
            ri, n = _ray_idx(c, torch.int32), c["N"]
            info = volrend.pack_info(ri, n)
            by_idx, by_info = dict(ray_indices=ri, n_rays=n), dict(packed_info=info)
            if c["alpha_form"]:
                a = c["alpha"].to(DEV)
                calls = [lambda r: volrend.render_weight_from_alpha(a, **r), lambda r: (volrend.render_transmittance_from_alpha(a, **r),),
                         lambda r: (volrend.render_visibility_from_alpha(a, **r).float(),)]
            else:
                ts, te, sg = c["ts"].to(DEV), c["te"].to(DEV), c["sigma"].to(DEV)
                calls = [lambda r: volrend.render_weight_from_density(ts, te, sg, **r),
                         lambda r: volrend.render_transmittance_from_density(ts, te, sg, **r),
                         lambda r: (volrend.render_visibility_from_density(ts, te, sg, **r).float(),)]
            for call in calls:
                for x, y in zip(call(by_idx), call(by_info)):
                    assert _same_bits(x, y)
            vis = calls[2](by_idx)[0]
            assert 0 < int(vis.sum()) < vis.numel(), "early_stop_eps = 1e-4 drops the samples behind the opaque ones"


# =============================================================================================================== accumulate
@pytest.mark.parametrize("D", V.ACC_CHANNELS)
def test_accumulate(D):
    """D in {None, 1, 2, 3, 4, 5, 7, 16, 48, 65, 256} on the ragged counts: forward and both gradients against float64; weights
    without a gradient, values without one; empty rays exactly 0; rows past N of a sentinel-filled output untouched (C ABI)"""
    from morpheus_amd import volrend
    case, r64, r32 = _ref(f"acc{D}", lambda: V.accumulate_case(D), V.accumulate_run)
    sc = V.accumulate_scales(case)
    ri, n = _ray_idx(case), case["N"]
    w = case["w"].to(DEV).requires_grad_(True)
    v = None if D is None else case["v"].to(DEV).requires_grad_(True)
    g = case["g"].to(DEV)
    out = volrend.accumulate_along_rays(w, v, ri, n)
    assert out.shape == (n, D or 1)
    empty = (torch.tensor(case["cnt"]) == 0).to(DEV)
    assert bool((out[empty] == 0).all()), "a ray without samples: exactly 0"
    gs = torch.autograd.grad((out * g).sum(), [w] + ([] if v is None else [v]))
    V.judge(out, r32["out"], r64["out"], sc["out"], f"volrend accumulate D={D}: out")
    V.judge(gs[0], r32["d_w"], r64["d_w"], sc["d_w"], f"volrend accumulate D={D}: d_weights")
    if v is not None:
        V.judge(gs[1], r32["d_v"], r64["d_v"], sc["d_v"], f"volrend accumulate D={D}: d_values")
        # one side without a gradient: the other side's bits do not change
        out_w = volrend.accumulate_along_rays(w, v.detach(), ri, n)
        assert _same_bits(torch.autograd.grad((out_w * g).sum(), [w])[0], gs[0])
        out_v = volrend.accumulate_along_rays(w.detach(), v, ri, n)
        assert _same_bits(torch.autograd.grad((out_v * g).sum(), [v])[0], gs[1]) and _same_bits(out_v, out)
    # C ABI: two rows beyond N keep the sentinel
    rs, rc = (t.contiguous() for t in volrend.pack_info(ri, n).int().unbind(1))
    buf = torch.full((n + 2, D or 1), SENTINEL, device=DEV)
    assert _status("mh_accumulate_fwd", _ptr(w.detach()), _ptr(None if v is None else v.detach()), D or 1, _ptr(rs), _ptr(rc), n, _ptr(buf)) == 0
    torch.cuda.synchronize()
    assert _same_bits(buf[:n], out) and bool((buf[n:] == SENTINEL).all())


def test_dense_layout():
    """[5, 70] inputs with neither index give the packed route's bits on the same numbers, reshaped: both forms, accumulate, gradients"""
    from morpheus_amd import volrend
    rng = np.random.RandomState(5)
    N, K = 5, 70
    t = lambda a: torch.from_numpy(a.astype(np.float32)).to(DEV)
    dt = t(rng.rand(N, K) * 0.02 + 0.002)
    ts = 0.05 + torch.cumsum(dt, 1) - dt
    te = ts + dt
    sigma, alpha = t(S._log_uniform(rng, N * K, 1e-2, 30.0).reshape(N, K)), t(rng.rand(N, K) * 0.2)
    vals, gw, go = t(rng.rand(N, K, 3)), t(rng.rand(N, K) - 0.5), t(rng.rand(N, 3) - 0.5)
    ri = torch.arange(N, device=DEV).repeat_interleave(K)

    def run(dense):
        shp = (lambda x: x) if dense else (lambda x: x.reshape(N * K, *x.shape[2:]))
        route = {} if dense else dict(ray_indices=ri, n_rays=N)
        sg, al, vv = (shp(x).clone().requires_grad_(True) for x in (sigma, alpha, vals))
        w, T, a = volrend.render_weight_from_density(shp(ts), shp(te), sg, **route)
        w2, T2 = volrend.render_weight_from_alpha(al, **route)
        acc = volrend.accumulate_along_rays(w, vv, **({} if dense else dict(ray_indices=ri, n_rays=N)))
        ones = volrend.accumulate_along_rays(w2, **({} if dense else dict(ray_indices=ri, n_rays=N)))
        assert w.shape == sg.shape and T2.shape == al.shape and acc.shape == (N, 3) and ones.shape == (N, 1)
        loss = (acc * go).sum() + (w * shp(gw)).sum() + (T * shp(gw)).sum() + (a * shp(gw)).sum() + (T2 * shp(gw)).sum() + ones.sum()
        grads = torch.autograd.grad(loss, [sg, al, vv])
        return [x.reshape(-1) for x in (w, T, a, w2, T2, acc, ones) + grads]

    for d, p in zip(run(True), run(False)):
        assert _same_bits(d, p)


# ================================================================================================ the reference's composition
def test_reference_composition_beside_the_fused_compositor():
    """render_weight_from_density + three accumulate_along_rays on the ragged 0 .. 350 case with int64 ray_indices, beside
    ops.composite on the same inputs: weights, opacity, depth, colour, the white-background image rgbs + (1 - opacity) and
    d_sigma / d_rgb of a mixed loss (all four probes), both routes judged against float64.  The count of bit-identical weights is
    reported, not asserted."""
    from morpheus_amd import ops
    case, w64, _ = _ref("density", V.density_case, V.weights_run)
    if "composition" not in _REF:
        _REF["composition"] = (S.composite_run(case, F64, ("wodc",)), S.composite_run(case, F32, ("wodc",)))
    r64, r32 = _REF["composition"]
    sc = S.composite_scales(case, r64, "wodc")
    rs, rc = ops.packed_info(_ray_idx(case), case["N"])
    results = {}
    for route in ("volrend", "fused"):
        sg, rg = case["sigma"].to(DEV).requires_grad_(True), case["rgb"].to(DEV).requires_grad_(True)
        if route == "volrend":
            outs = _composition(case, sg, rg)
        else:
            outs = ops.composite(sg, case["ts"].to(DEV), case["te"].to(DEV), rg, rs, rc)
        results[route] = outs[0].detach()
        for key, name, out in zip("wodc", ("weights", "opacity", "depth", "colour"), outs):
            V.judge(out, r32[key], r64[key], sc[key], f"composition, {route}: {name}")
        white = lambda o, c: c + (1 - o[:, None])
        # scale 1: an image value, and the rounding of 1 - opacity, are of order 1
        V.judge(white(outs[1], outs[3]), white(r32["o"], r32["c"]), white(r64["o"], r64["c"]), 1.0, f"composition, {route}: white-background image")
        d_sigma, d_rgb = torch.autograd.grad(S.composite_loss(outs, case, "wodc", dev=DEV), [sg, rg])
        V.judge(d_sigma, r32["grads"]["wodc"][0], r64["grads"]["wodc"][0], sc["d_sigma"], f"composition, {route}: d_sigma")
        V.judge(d_rgb, r32["grads"]["wodc"][1], r64["grads"]["wodc"][1], sc["d_rgb"], f"composition, {route}: d_rgb")
    same = int((results["volrend"].view(torch.int32) == results["fused"].view(torch.int32)).sum())
    print(f"[volrend-f64] composition: {same} of {case['M']} weights bit-identical to the fused compositor's")


def test_rendering_equals_its_steps():
    """rendering() with an rgb_sigma_fn closure and render_bkgd, and with rgb_alpha_fn: the same steps done by hand, bit for bit"""
    from morpheus_amd import volrend
    case = _ref("density", V.density_case, V.weights_run)[0]
    ts, te, ri, n = case["ts"].to(DEV), case["te"].to(DEV), _ray_idx(case), case["N"]
    sigma, rgb = case["sigma"].to(DEV), case["rgb"].to(DEV)
    bkgd = torch.tensor([1.0, 0.5, 0.25], device=DEV)
    seen = []

    def rgb_sigma_fn(t0, t1, idx):
        seen.append((t0.shape, idx.dtype))
        return rgb, sigma

    with torch.no_grad():
        colors, opacities, depths, extras = volrend.rendering(ts, te, ri, n, rgb_sigma_fn=rgb_sigma_fn, render_bkgd=bkgd)
        w, T, a = volrend.render_weight_from_density(ts, te, sigma, ray_indices=ri, n_rays=n)
        o = volrend.accumulate_along_rays(w, None, ri, n)
        d = volrend.accumulate_along_rays(w, (ts + te)[:, None] / 2.0, ri, n) / o.clamp_min(torch.finfo(torch.float32).eps)
        c = volrend.accumulate_along_rays(w, rgb, ri, n) + bkgd * (1.0 - o)
        assert seen == [((case["M"],), torch.int64)] and set(extras) == {"weights", "alphas", "trans", "sigmas", "rgbs"}
        for x, y in ((colors, c), (opacities, o), (depths, d), (extras["weights"], w), (extras["trans"], T), (extras["alphas"], a)):
            assert _same_bits(x, y)
        alpha = a.clone()
        colors2, opacities2, _, extras2 = volrend.rendering(ts, te, ri, n, rgb_alpha_fn=lambda t0, t1, idx: (rgb, alpha))
        w2, T2 = volrend.render_weight_from_alpha(alpha, ray_indices=ri, n_rays=n)
        assert _same_bits(extras2["weights"], w2) and _same_bits(extras2["trans"], T2)
        assert _same_bits(colors2, volrend.accumulate_along_rays(w2, rgb, ri, n)) and _same_bits(opacities2, volrend.accumulate_along_rays(w2, None, ri, n))
    with pytest.raises(ValueError):
        volrend.rendering(ts, te, ri, n)


def test_prefix_trans_is_carried_by_autograd():
    from morpheus_amd import volrend
    case = _ref("alpha5", lambda: V.rays_case(5, True), V.weights_run)[0]
    a = case["alpha"].to(DEV)
    ri = _ray_idx(case)
    prefix = (torch.rand(case["M"], device=DEV) * 0.5 + 0.5).requires_grad_(True)
    w, T = volrend.render_weight_from_alpha(a, ray_indices=ri, n_rays=5, prefix_trans=prefix)
    w0, T0 = volrend.render_weight_from_alpha(a, ray_indices=ri, n_rays=5)
    assert _same_bits(T, T0 * prefix) and _same_bits(w, (T0 * prefix) * a)
    g, = torch.autograd.grad(T.sum(), [prefix])
    assert _same_bits(g, T0)


# ==================================================================================================================== C ABI
def test_c_abi_refuses_bad_arguments_and_writes_nothing():
    """a NULL required pointer, D = 0, D = 257 and a negative N: MH_ERR_ARG, and the sentinel-filled outputs keep every bit"""
    case = _ref("density5", lambda: V.rays_case(5, False), V.weights_run)[0]
    N, M = case["N"], case["M"]
    cnt = torch.tensor(case["cnt"], dtype=torch.int32)
    rs, rc = (torch.cumsum(cnt, 0) - cnt).int().to(DEV), cnt.to(DEV)
    sg, ts, te = (case[k].to(DEV) for k in ("sigma", "ts", "te"))
    ri = _ray_idx(case, torch.int32)
    outs = [torch.full((M,), SENTINEL, device=DEV) for _ in range(4)]
    acc = torch.full((N, 3), SENTINEL, device=DEV)
    vals = torch.rand(M, 3, device=DEV)
    irs, irc = torch.full((N,), -7, dtype=torch.int32, device=DEV), torch.full((N,), -7, dtype=torch.int32, device=DEV)
    P = _ptr
    bad = [("mh_pack_info", (None, 0, M, N, P(irs), P(irc))), ("mh_pack_info", (P(ri), 0, M, N, None, P(irc))),
           ("mh_pack_info", (P(ri), 0, M, -1, P(irs), P(irc))), ("mh_pack_info", (P(ri), 0, -1, N, P(irs), P(irc))),
           ("mh_ray_weights_fwd", (None, P(ts), P(te), 0, P(rs), P(rc), N, P(outs[0]), P(outs[1]), P(outs[2]))),
           ("mh_ray_weights_fwd", (P(sg), None, P(te), 0, P(rs), P(rc), N, P(outs[0]), P(outs[1]), P(outs[2]))),
           ("mh_ray_weights_fwd", (P(sg), P(ts), P(te), 0, None, P(rc), N, P(outs[0]), P(outs[1]), P(outs[2]))),
           ("mh_ray_weights_fwd", (P(sg), P(ts), P(te), 0, P(rs), P(rc), N, None, None, None)),
           ("mh_ray_weights_fwd", (P(sg), P(ts), P(te), 0, P(rs), P(rc), -1, P(outs[0]), P(outs[1]), P(outs[2]))),
           ("mh_ray_weights_bwd", (P(sg), P(ts), P(te), 0, P(rs), P(rc), N, None, P(outs[0]), None, None, P(outs[3]))),     # no saved trans
           ("mh_ray_weights_bwd", (P(sg), P(ts), P(te), 0, P(rs), P(rc), N, P(outs[1]), P(outs[0]), None, None, None)),
           ("mh_ray_weights_bwd", (P(sg), None, None, 1, P(rs), P(rc), N, None, P(outs[0]), None, P(outs[2]), P(outs[3]))), # g_alphas, alpha form
           ("mh_ray_weights_bwd", (P(sg), P(ts), P(te), 0, P(rs), P(rc), -1, P(outs[1]), P(outs[0]), None, None, P(outs[3]))),
           ("mh_accumulate_fwd", (None, P(vals), 3, P(rs), P(rc), N, P(acc))), ("mh_accumulate_fwd", (P(sg), P(vals), 3, P(rs), P(rc), N, None)),
           ("mh_accumulate_fwd", (P(sg), P(vals), 0, P(rs), P(rc), N, P(acc))), ("mh_accumulate_fwd", (P(sg), P(vals), 257, P(rs), P(rc), N, P(acc))),
           ("mh_accumulate_fwd", (P(sg), None, 3, P(rs), P(rc), N, P(acc))), ("mh_accumulate_fwd", (P(sg), P(vals), 3, P(rs), P(rc), -1, P(acc))),
           ("mh_accumulate_bwd", (P(sg), P(vals), 3, P(rs), P(rc), N, None, P(outs[3]), None)),
           ("mh_accumulate_bwd", (P(sg), P(vals), 3, P(rs), P(rc), N, P(acc), None, None)),
           ("mh_accumulate_bwd", (P(sg), P(vals), 0, P(rs), P(rc), N, P(acc), P(outs[3]), None)),
           ("mh_accumulate_bwd", (P(sg), P(vals), 257, P(rs), P(rc), N, P(acc), P(outs[3]), None)),
           ("mh_accumulate_bwd", (P(sg), P(vals), 3, P(rs), P(rc), -1, P(acc), P(outs[3]), None))]
    for name, args in bad:
        assert _status(name, *args) == MH_ERR_ARG, (name, args)
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs + [acc]) and bool((irs == -7).all()) and bool((irc == -7).all())
    # and the same calls with good arguments run: N = 0 is fine and launches nothing
    assert _status("mh_ray_weights_fwd", P(sg), P(ts), P(te), 0, P(rs), P(rc), 0, P(outs[0]), P(outs[1]), P(outs[2])) == 0
    assert _status("mh_ray_weights_fwd", P(sg), P(ts), P(te), 0, P(rs), P(rc), N, P(outs[0]), None, None) == 0
    torch.cuda.synchronize()
    assert bool((outs[0] != SENTINEL).all()) and bool((outs[1] == SENTINEL).all())
