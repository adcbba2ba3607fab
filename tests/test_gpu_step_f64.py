"""csrc/composite.hip, csrc/wnorm.hip and csrc/optim.hip against float64 at their loop, tail and branch edges
(tests/step_f64_oracle.py holds the yardsticks, the fp32 restatements and the cases; tests/test_step_oracle_host.py shows on the CPU
that the cases reach what they name).

The rule, not fitted to a run (step_f64_oracle.judge): errors are |x - float64| over the quantity's natural scale, written beside each
check; a kernel's worst error must stay within 2 x the worst error of the sequential fp32 restatement on the same inputs (floor: 4
roundings of the scale, for the case where the restatement happens to be exact), with at most 2 x (+ 2) as many elements above that
floor.  Every check uses the factor 2.  Everything else is exact: zeros, untouched buffers, bit-for-bit invariances.
Every judged check prints its figures and appends them to the JSON-lines file that MORPHEUS_STEP_REPORT names.

Worst figures of one run on an MI355X (error / scale; worst over the module's checks of the quantity; ratio taken in the check that
holds the kernel's worst).  No factor is raised above 2.

    quantity                    scale                                kernel     fp32 restatement   ratio
    weights                     the ray's total weight               8.19e-08   8.07e-08           1.01
    opacity                     the ray's total weight               1.52e-07   2.38e-07           0.64
    depth                       sum w |tmid|                         1.49e-07   2.44e-07           0.61
    colour                      the ray's total weight               1.40e-07   2.39e-07           0.59
    d_sigma                     dt_i x the ray's largest |g_j|       3.83e-06   6.19e-06           0.62
    d_rgb                       total weight x largest |g_color|     9.96e-08   9.96e-08           1.00
    W                           the row's largest |W|                1.52e-07   2.93e-07           0.52
    dv                          s max|dW_row|                        2.84e-07   5.69e-07           0.50
    dg                          sum |dW v| / ||v||                   2.31e-07   4.28e-07           0.54
    parameter, after step 1     the step size                        1.65e-05   1.65e-05           1.00
    exp_avg, after step 1       |m| + (1 - b1) |g|                   6.81e-08   9.48e-08           0.72
    exp_avg_sq, after step 1    its own value                        5.83e-08   1.03e-07           0.56
    parameter, after step 6     the step size                        2.80e-05   2.80e-05           1.00
    exp_avg, after step 6       |m| + (1 - b1) |g|                   2.12e-07   3.53e-07           0.60
    exp_avg_sq, after step 6    its own value                        1.66e-07   2.80e-07           0.59
(the parameter's error is the rounding of p - move at ulp(p) over a step size of 2e-4 .. 1e-2: the same in kernel and restatement.)
With the exclusive prefix formed as `carry + (incl - sd)` for every sample, as it was, the opaque samples of sd 1e2 and 1e4 put
weights, opacity, depth and colour at 4e-6 to 4e-4 and sigma = +inf gives NaN.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import step_f64_oracle as S
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


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _pool(records, key, hip, ref32, f64, scale):
    h, c, r, s = records.setdefault(key, ([], [], [], []))
    for lst, t in ((h, hip), (c, ref32), (r, f64), (s, scale)):
        lst.append(flat64(t))


def _judge_pool(records, prefix):
    return {key: S.judge(*(torch.cat(x) for x in v), f"{prefix} {key}") for key, v in records.items()}


# ============================================================================================================ compositor
_REF = {}


def _composite_ref(name, build):
    """the case, its float64 run and its fp32 restatement: computed once, shared, never modified"""
    if name not in _REF:
        case = build()
        _REF[name] = (case, S.composite_run(case, F64), S.composite_run(case, F32))
    return _REF[name]


def _composite_gpu(case, variants, pool, padded=False):
    """ops.packed_info + ops.composite on the case; forward outputs and the gradients of every loss variant into `pool`"""
    from morpheus_amd import ops
    _, r64, r32 = case["_ref"]
    ray, _ = S.ray_index(case["cnt"])
    rs, rc = ops.packed_info(ray.to(DEV), case["N"])
    assert rc.cpu().tolist() == case["cnt"]
    sg, rg = case["sigma"].to(DEV).requires_grad_(True), case["rgb"].to(DEV).requires_grad_(True)
    outs = ops.composite(sg, case["ts"].to(DEV), case["te"].to(DEV), rg, rs, rc, padded)
    sc = S.composite_scales(case, r64)
    # scales: weights / opacity / colour: the ray's total weight; depth: sum w |tmid|
    for k, out in zip("wodc", outs):
        _pool(pool, {"w": "weights", "o": "opacity", "d": "depth", "c": "colour"}[k], out, r32[k], r64[k], sc[k])
    empty = torch.tensor(case["cnt"]) == 0
    for out in outs[1:]:
        assert bool((out[empty.to(DEV)] == 0).all()), "a ray without samples: opacity, depth and colour exactly 0"
    for var in variants:
        d_sigma, d_rgb = torch.autograd.grad(S.composite_loss(outs, case, var, dev=DEV), [sg, rg], retain_graph=True)
        scv = S.composite_scales(case, r64, var)
        # scales: d_sigma: dt_i x the ray's largest |g_j|; d_rgb: the ray's total weight x its largest |g_color|
        _pool(pool, "d_sigma", d_sigma, r32["grads"][var][0], r64["grads"][var][0], scv["d_sigma"])
        _pool(pool, "d_rgb", d_rgb, r32["grads"][var][1], r64["grads"][var][1], scv["d_rgb"])
        if "c" not in var:
            assert bool((d_rgb == 0).all()), f"loss {var}: g_color absent, rgb requires a gradient -> d_rgb exactly 0"
    return outs


def test_composite_every_count_and_placed_sample():
    """33 rays: every sample count of S.COUNTS (1 to 17 chunks, full and ragged last chunks, 0-count rays first, last and adjacent),
    an opaque sample of sd 30 / 1e2 / 1e4 at lane 0, lane 63 and the first lane of the second and third chunk, sigma = 0, ts == te,
    a transmittance that underflows mid-chunk with live gradients behind it, a uniformly thin ray; eight losses: all four outputs,
    each alone, and the three pairs without g_color.  Before the exclusive scan stopped subtracting the sample's own term the
    opaque samples miss this by the rounding of incl: 4e-6 (sd 1e2) to 4e-4 (sd 1e4) of the ray's total against a restatement at 5e-8."""
    case, r64, r32 = _composite_ref("main", S.composite_main_case)
    pool = {}
    outs = _composite_gpu(dict(case, _ref=(case, r64, r32)), S.VARIANTS, pool)
    _judge_pool(pool, "compositor, every count:")
    w = outs[0].detach().cpu()
    start = np.cumsum([0] + case["cnt"][:-1])
    r, k = case["placed"]["underflow"]
    assert bool((w[int(start[r]) + 64:int(start[r]) + case["cnt"][r]] == 0).all()), "behind the underflow the fp32 weights are exactly 0"
    for name in ("sigma = 0", "ts == te"):
        r, ks = case["placed"][name]
        assert bool((w[[int(start[r]) + k for k in ks]] == 0).all()), f"{name}: weight exactly 0"


def test_composite_ray_counts_around_a_workgroup():
    """N = 1, 3, 4, 5, 257 rays: 1, 3, 0 and 1 rays in the last workgroup of four waves (the `ray >= N` exit), all-outputs loss"""
    pool = {}
    for N in S.RAY_COUNTS:
        case, r64, r32 = _composite_ref(f"rays{N}", lambda: S.composite_rays_case(N))
        _composite_gpu(dict(case, _ref=(case, r64, r32)), ("wodc",), pool)
    _judge_pool(pool, "compositor, ray counts:")


def _composite_fwd_raw(case, start=None, M=None, with_rgb=True, fill=None):
    """mh_composite_fwd through the C ABI on sentinel-filled outputs -> status, (weights, opacity, depth, color)"""
    cnt = torch.tensor(case["cnt"], dtype=torch.int32)
    st = (torch.cumsum(cnt, 0) - cnt).int() if start is None else torch.tensor(start, dtype=torch.int32)
    N = case["N"]
    M = case["M"] if M is None else M
    ins = fill or {k: case[k].to(DEV) for k in ("sigma", "ts", "te", "rgb")}
    outs = [torch.full(s, SENTINEL, device=DEV) for s in ((M,), (N,), (N,), (N, 3))]
    st_d, cnt_d = st.to(DEV), cnt.to(DEV)
    status = _status("mh_composite_fwd", _ptr(ins["sigma"]), _ptr(ins["ts"]), _ptr(ins["te"]), _ptr(ins["rgb"]) if with_rgb else None,
                     _ptr(st_d), _ptr(cnt_d), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]) if with_rgb else None, N)
    torch.cuda.synchronize()
    return status, outs


def test_composite_inf_and_nan_samples():
    """sigma = +inf at one sample: by the definition w = T there, exact zeros behind it, finite opacity / depth / colour (it read
    inf - inf = NaN while the exclusive prefix was formed by subtraction).  sigma = NaN poisons its own ray only: the other three
    rays of its workgroup and both neighbouring workgroups equal the same batch without the NaN bit for bit."""
    clean = S.composite_nonfinite_case()
    _, clean_out = _composite_fwd_raw(clean)
    ray, k = S.ray_index(clean["cnt"])
    # +inf
    case = S.composite_nonfinite_case("inf")
    status, outs = _composite_fwd_raw(case)
    assert status == 0 and all(bool(torch.isfinite(o).all()) for o in outs)
    with torch.no_grad():
        o64 = S.composite(case["sigma"].double(), case["ts"], case["te"], case["rgb"].double(), case["cnt"])
        o32 = S.composite(case["sigma"], case["ts"], case["te"], case["rgb"], case["cnt"])
    sc = S.composite_scales(case, dict(w=o64[0]))
    for name, key, h, c, r in zip(("weights", "opacity", "depth", "colour"), "wodc", outs, o32, o64):
        S.judge(h, c, r, sc[key], f"compositor, sigma = +inf: {name}")
    at = (ray == S.INF_AT[0]) & (k == S.INF_AT[1])
    behind = (ray == S.INF_AT[0]) & (k > S.INF_AT[1])
    w = outs[0].cpu()
    assert int(behind.sum()) == S.NONFINITE_COUNTS[S.INF_AT[0]] - S.INF_AT[1] - 1 and bool((w[behind] == 0).all())
    assert float(w[at]) > 0.05, "alpha = 1: the sample takes the whole remaining transmittance"
    # NaN
    case = S.composite_nonfinite_case("nan")
    status, outs = _composite_fwd_raw(case)
    assert status == 0
    own = ray == S.NONFINITE_AT[0]
    others = torch.arange(case["N"]) != S.NONFINITE_AT[0]
    assert _same_bits(outs[0][(~own).to(DEV)], clean_out[0][(~own).to(DEV)])
    for o, c in zip(outs[1:], clean_out[1:]):
        assert _same_bits(o[others.to(DEV)], c[others.to(DEV)])
        assert bool(torch.isnan(o[S.NONFINITE_AT[0]]).all())
    before = own & (k < S.NONFINITE_AT[1])
    assert _same_bits(outs[0][before.to(DEV)], clean_out[0][before.to(DEV)])
    assert bool(torch.isnan(outs[0][(own & (k >= S.NONFINITE_AT[1])).to(DEV)]).all())


def test_composite_c_abi_without_rgb():
    """rgb = color = NULL forward and rgb = d_rgb = NULL backward (forms the wrapper cannot produce) against float64; rgb without
    color is the argument error and launches nothing."""
    case, r64, r32 = _composite_ref("rays5", lambda: S.composite_rays_case(5))
    status, outs = _composite_fwd_raw(case, with_rgb=False)
    assert status == 0
    sc = S.composite_scales(case, r64)
    for name, key, h in zip(("weights", "opacity", "depth"), "wod", outs):
        S.judge(h, r32[key], r64[key], sc[key], f"compositor, rgb = NULL: {name}")
    assert bool((outs[3] == SENTINEL).all()), "color = NULL: nothing may be written for it"
    # backward without rgb: g_color is ignored, the gradient is that of the loss on weights, opacity and depth
    n64, n32 = S.composite_run(case, F64, ("wod",), with_rgb=False), S.composite_run(case, F32, ("wod",), with_rgb=False)
    cnt = torch.tensor(case["cnt"], dtype=torch.int32)
    st, cnt_d = (torch.cumsum(cnt, 0) - cnt).int().to(DEV), cnt.to(DEV)
    ins = {k: case[k].to(DEV) for k in ("sigma", "ts", "te", "g_w", "g_o", "g_d", "g_c")}
    for g_c in (None, ins["g_c"]):
        d_sigma = torch.full((case["M"],), SENTINEL, device=DEV)
        status = _status("mh_composite_bwd", _ptr(ins["sigma"]), _ptr(ins["ts"]), _ptr(ins["te"]), None, _ptr(st), _ptr(cnt_d),
                         _ptr(outs[0]), _ptr(ins["g_w"]), _ptr(ins["g_o"]), _ptr(ins["g_d"]), _ptr(g_c), _ptr(d_sigma), None, case["N"])
        torch.cuda.synchronize()
        assert status == 0
        scv = S.composite_scales(case, n64, "wod", with_rgb=False)
        S.judge(d_sigma, n32["grads"]["wod"][0], n64["grads"]["wod"][0], scv["d_sigma"], "compositor, rgb = d_rgb = NULL: d_sigma")
    # the mismatched pairs
    outs2 = [torch.full_like(o, SENTINEL) for o in outs]
    rgb = case["rgb"].to(DEV)
    status = _status("mh_composite_fwd", _ptr(ins["sigma"]), _ptr(ins["ts"]), _ptr(ins["te"]), _ptr(rgb), _ptr(st), _ptr(cnt_d),
                     _ptr(outs2[0]), _ptr(outs2[1]), _ptr(outs2[2]), None, case["N"])
    d_sigma = torch.full((case["M"],), SENTINEL, device=DEV)
    status_b = _status("mh_composite_bwd", _ptr(ins["sigma"]), _ptr(ins["ts"]), _ptr(ins["te"]), _ptr(rgb), _ptr(st), _ptr(cnt_d),
                       _ptr(outs[0]), _ptr(ins["g_w"]), None, None, None, _ptr(d_sigma), None, case["N"])
    torch.cuda.synchronize()
    assert status == MH_ERR_ARG and status_b == MH_ERR_ARG
    assert all(bool((o == SENTINEL).all()) for o in outs2) and bool((d_sigma == SENTINEL).all())


def test_composite_waves_past_the_last_ray_do_nothing():
    """the `ray >= N` exit of both kernels: the five-ray batch handed over with N = 1, 2, 3, so that the arrays hold valid rays behind
    N -- what an idle wave of the last workgroup would do is then seen in sentinel-filled outputs instead of lost in memory nobody
    owns: samples, opacity, depth, colour, d_sigma and d_rgb of the rays from N on stay as they were."""
    case = S.composite_rays_case(5)
    cnt = torch.tensor(case["cnt"], dtype=torch.int32)
    start = (torch.cumsum(cnt, 0) - cnt).int()
    st_d, cnt_d = start.to(DEV), cnt.to(DEV)
    ins = {k: case[k].to(DEV) for k in ("sigma", "ts", "te", "rgb", "g_w", "g_o", "g_d", "g_c")}
    _, full = _composite_fwd_raw(case)
    for N in (1, 2, 3):
        first = int(start[N])
        outs = [torch.full(s, SENTINEL, device=DEV) for s in ((case["M"],), (5,), (5,), (5, 3))]
        grads = [torch.full(s, SENTINEL, device=DEV) for s in ((case["M"],), (case["M"], 3))]
        st_f = _status("mh_composite_fwd", _ptr(ins["sigma"]), _ptr(ins["ts"]), _ptr(ins["te"]), _ptr(ins["rgb"]), _ptr(st_d), _ptr(cnt_d),
                       *[_ptr(o) for o in outs], N)
        st_b = _status("mh_composite_bwd", _ptr(ins["sigma"]), _ptr(ins["ts"]), _ptr(ins["te"]), _ptr(ins["rgb"]), _ptr(st_d), _ptr(cnt_d),
                       _ptr(full[0]), _ptr(ins["g_w"]), _ptr(ins["g_o"]), _ptr(ins["g_d"]), _ptr(ins["g_c"]), _ptr(grads[0]), _ptr(grads[1]), N)
        torch.cuda.synchronize()
        assert st_f == 0 and st_b == 0
        for o in (outs[0], grads[0], grads[1]):
            assert bool((o[first:] == SENTINEL).all()), f"N = {N}: a sample of a ray behind N was written"
            assert first == 0 or bool((o[:first] != SENTINEL).all())
        for o in outs[1:]:
            assert bool((o[N:] == SENTINEL).all()), f"N = {N}: an output of a ray behind N was written"
        assert _same_bits(outs[0][:first], full[0][:first]) and all(_same_bits(o[:N], f[:N]) for o, f in zip(outs[1:], full[1:]))


def test_composite_padding_and_ray_order():
    """padded=True with packed entries no ray owns (interior, a whole chunk's worth, trailing; NaN inputs there): weights and both
    gradients are exact zeros there and equal the unpadded call's bits elsewhere.  The same rays in reversed and in interleaved
    order give the same per-ray bits."""
    from morpheus_amd import ops
    case = S.composite_nonfinite_case()

    def run(c, start=None, M=None, owned=None):
        cnt = torch.tensor(c["cnt"], dtype=torch.int32)
        st = (torch.cumsum(cnt, 0) - cnt).int() if start is None else torch.tensor(start, dtype=torch.int32)
        leaves = {}
        for k in ("sigma", "ts", "te", "rgb", "g_w"):
            t = c[k]
            if owned is not None:
                full = torch.full((M,) + tuple(t.shape[1:]), float("nan"))
                full[owned] = t
                t = full
            leaves[k] = t.to(DEV)
        sg, rg = leaves["sigma"].requires_grad_(True), leaves["rgb"].requires_grad_(True)
        outs = ops.composite(sg, leaves["ts"], leaves["te"], rg, st.to(DEV), cnt.to(DEV), owned is not None)
        g_w = torch.nan_to_num(leaves["g_w"], nan=1.0)
        loss = (outs[0] * g_w).sum() + sum((o * c[k].to(DEV)).sum() for o, k in zip(outs[1:], ("g_o", "g_d", "g_c")))
        d_sigma, d_rgb = torch.autograd.grad(loss, [sg, rg])
        return [outs[0].detach(), d_sigma, d_rgb], [o.detach() for o in outs[1:]]

    per_sample, per_ray = run(case)
    start, M, owned = S.composite_padded_layout(case["cnt"])
    assert M - case["M"] == 3 + 1 + 66 + 7
    pad_sample, pad_ray = run(case, start, M, owned)
    hole = torch.ones(M, dtype=torch.bool)
    hole[owned] = False
    for a, b in zip(pad_sample, per_sample):
        assert bool((a[hole.to(DEV)] == 0).all()) and _same_bits(a[owned.to(DEV)], b)
    assert all(_same_bits(a, b) for a, b in zip(pad_ray, per_ray))
    N = case["N"]
    for order in (list(range(N - 1, -1, -1)), list(range(0, N, 2)) + list(range(1, N, 2))):
        other, idx = S.composite_reorder(case, order)
        o_sample, o_ray = run(other)
        assert all(_same_bits(a, b[idx.to(DEV)]) for a, b in zip(o_sample, per_sample))
        assert all(_same_bits(a, b[torch.tensor(order, device=DEV)]) for a, b in zip(o_ray, per_ray))


# =========================================================================================================== weight norm
WN_PATTERNS = {"all": lambda n: [True] * n, "not the first": lambda n: [False] + [True] * (n - 1),
               "not the last": lambda n: [True] * (n - 1) + [False], "one only": lambda n: [i == n // 2 for i in range(n)]}


def _wnorm_gpu(case, with_grad, pool):
    from morpheus_amd import ops
    vs = [v.to(DEV).clone().requires_grad_(True) for v in case["vs"]]
    gs = [g.to(DEV).clone().requires_grad_(True) for g in case["gs"]]
    ws = ops.weight_norm_all(vs, gs)
    sum((w * dw.to(DEV)).sum() for w, dw, on in zip(ws, case["dws"], with_grad) if on).backward()
    ref = S.wnorm_reference(case, with_grad)
    for v, g, w, r, on in zip(vs, gs, ws, ref, with_grad):
        if not on:
            assert bool((v.grad == 0).all()) and bool((g.grad == 0).all()), "no gradient reached the layer: dv = dg = exactly 0"
        # scales: W: the row's largest |W|; dv: s max|dW_row|; dg: sum |dW v| / ||v||
        for key, h, k in (("W", w, 0), ("dv", v.grad, 1), ("dg", g.grad, 2)):
            _pool(pool, key, h, r["f32"][k], r["f64"][k], r["scale"][k])


@pytest.mark.parametrize("kind", S.WN_GRAD_KINDS)
@pytest.mark.parametrize("name", list(S.WN_CALLS))
def test_weight_norm_rows_columns_and_layers(name, kind):
    """columns 1, 2, 63, 64, 65, 127, 128, 129, 300 (a row shorter than a wave, one to five trips of the column loop); 150, 5 and 215
    rows (2, 1 and 3 in the last workgroup); a layer boundary at every wave of a workgroup; 1, 9 and 32 layers; rows of scale 2^-40 to
    2^40, g of both signs and 0; dW random, parallel to v (exact dv = 0: the error shows at the row's input scale) and orthogonal
    to v; no gradient for the first layer, the last, all but one."""
    case = S.wnorm_case(name, kind)
    n = len(case["vs"])
    pool = {}
    for pname, pat in WN_PATTERNS.items():
        if n == 1 and pname != "all":
            continue
        _wnorm_gpu(case, pat(n), pool)
    _judge_pool(pool, f"weight norm, {name}, dW {kind}:")


def _wn_arrays(tensors):
    return (ctypes.c_void_p * len(tensors))(*[_ptr(t) for t in tensors])


def test_weight_norm_layer_limit_and_no_gradient_at_all():
    """33 layers: the call raises and nothing is written (C ABI on sentinel-filled outputs, and ops.weight_norm_all); 32 layers with
    every dW NULL: dv and dg are exact zeros everywhere."""
    from morpheus_amd import ops
    from morpheus_amd._lib import MorpheusHipError
    n = 33
    vs = [torch.randn(2, 5, device=DEV) for _ in range(n)]
    gs = [torch.randn(2, 1, device=DEV) for _ in range(n)]
    IA = ctypes.c_int32 * n
    rows, cols = IA(*[2] * n), IA(*[5] * n)
    for k in (33, 32):
        out0 = [torch.full((2, 5), SENTINEL, device=DEV) for _ in range(n)]
        out1 = [torch.full((2, 1), SENTINEL, device=DEV) for _ in range(n)]
        st_f = _status("mh_weight_norm_fwd", k, _wn_arrays(vs), _wn_arrays(gs), _wn_arrays(out0), rows, cols)
        torch.cuda.synchronize()
        if k == 33:
            assert st_f == MH_ERR_ARG and all(bool((o == SENTINEL).all()) for o in out0)
        else:
            assert st_f == 0 and all(bool((o != SENTINEL).all()) for o in out0[:32]) and bool((out0[32] == SENTINEL).all())
        out0 = [torch.full((2, 5), SENTINEL, device=DEV) for _ in range(n)]
        st_b = _status("mh_weight_norm_bwd", k, _wn_arrays(vs), _wn_arrays(gs), (ctypes.c_void_p * n)(), _wn_arrays(out0),
                       _wn_arrays(out1), rows, cols)
        torch.cuda.synchronize()
        if k == 33:
            assert st_b == MH_ERR_ARG and all(bool((o == SENTINEL).all()) for o in out0 + out1)
        else:
            assert st_b == 0 and all(bool((o == 0).all()) for o in out0[:32] + out1[:32])
            assert bool((out0[32] == SENTINEL).all()) and bool((out1[32] == SENTINEL).all())
    with pytest.raises(MorpheusHipError):
        ops.weight_norm_all(vs, gs)


def test_weight_norm_zero_row():
    """one all-zero row of v: torch._weight_norm gives NaN for that row of W (0 x g / 0), of dv and for its dg; the kernel does the
    same, and the other rows of the layer are held to float64 as everywhere else."""
    case = S.wnorm_case("one")
    case["vs"][0][2] = 0.0
    from morpheus_amd import ops
    v, g = case["vs"][0].to(DEV).requires_grad_(True), case["gs"][0].to(DEV).requires_grad_(True)
    (w,) = ops.weight_norm_all([v], [g])
    (w * case["dws"][0].to(DEV)).sum().backward()
    ref = S.wnorm_reference(case, [True])[0]
    rest = torch.tensor([0, 1, 3, 4])
    for key, h, k in (("W", w, 0), ("dv", v.grad, 1), ("dg", g.grad, 2)):
        r64 = ref["f64"][k]
        assert bool(torch.isnan(r64[2]).all()), "what torch._weight_norm gives for the zero row"
        assert bool(torch.isnan(h[2]).all()), f"{key}: the zero row is NaN, as torch's"
        S.judge(h.detach().cpu()[rest], ref["f32"][k][rest], r64[rest], ref["scale"][k][rest], f"weight norm, zero row beside: {key}")


# ================================================================================================================== Adam
def _guarded(a, n):
    """a device buffer of n elements (16-byte aligned) with 8 sentinel elements behind it"""
    buf = torch.full((n + 8,), SENTINEL, device=DEV)
    buf[:n] = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return buf


def _adam_call(bufs, n, ends, lrs, steps):
    ns = len(ends)
    return _status("mh_adam_step", *[b.data_ptr() for b in bufs], n, ns, (ctypes.c_int64 * ns)(*ends),
                   (ctypes.c_float * ns)(*lrs), (ctypes.c_int64 * ns)(*steps), S.BETA1, S.BETA2, S.EPS)


def _adam_check(bufs, before, g, ss_e, bc_e, pool, tag):
    """the three buffers after a step against the float64 rule and its fp32 restatement from the same state `before` (float64 and
    fp32 trajectories are the caller's); skipped elements and the guards bit-identical; -> nothing"""
    n = g.shape[0]
    torch.cuda.synchronize()
    got = [b[:n].cpu().numpy() for b in (bufs[0], bufs[2], bufs[3])]
    for b in bufs:
        assert bool((b[n:] == SENTINEL).all()), "a write behind the bucket"
    assert np.array_equal(bufs[1][:n].cpu().numpy().view(np.int32), g.view(np.int32)), "the gradient buffer is read only"
    p64, m64, v64 = before["f64"]
    f64 = S.adam(p64, g, m64, v64, ss_e, bc_e, np.float64)
    f32 = S.adam(before["f32"][0], g, before["f32"][1], before["f32"][2], ss_e, bc_e, np.float32)
    # scales: parameter: the step size; exp_avg: |m| + (1 - b1) |g|; exp_avg_sq: its own value
    scales = S.adam_scales(p64, g, m64, v64, ss_e)
    for key, h, c, r, s in zip(("parameter", "exp_avg", "exp_avg_sq"), got, f32, f64, scales):
        _pool(pool, f"{key}{tag}", h, c, r, s)
    skipped = ss_e < 0
    for h, b in zip(got, before["hip"]):
        assert np.array_equal(h.view(np.int32)[skipped], b.view(np.int32)[skipped]), "a skipped element changed"
    still = (~skipped) & (g == 0) & (before["hip"][1] == 0) & (before["hip"][2] == 0)
    assert np.array_equal(got[0].view(np.int32)[still], before["hip"][0].view(np.int32)[still]), \
        "a zero gradient into zero moments must not move the parameter (eps = 1e-15)"
    still = (~skipped) & (ss_e == 0)
    assert np.array_equal(got[0].view(np.int32)[still], before["hip"][0].view(np.int32)[still]), "learning rate 0: no move"
    return got, f32, f64


def _per_element(ends, lrs, steps, n):
    ss, bc = S.adam_seg_params(lrs, steps)
    seg = S.adam_seg_of(ends, n)
    return ss[seg], bc[seg]


def test_adam_segment_geometry_one_step():
    """mh_adam_step on raw buffers: n = 1, 2, 3, 4, 5, 1023, 1024, 1025, 2049 (the cnt < 4 tail of the last lane, three blocks) x one
    segment / the mixed layout (lanes holding 1+3, 2+2, 3+1 and 1+1+2 elements of stepped and skipped segments with their own step
    counts 1, 2, 10, 1000, 10^6 and learning rates, 0 among them; zero-length segments first, last, two in a row) / 160 segments;
    gradients of 1e-18 to 1e4 in one bucket, exact zeros into zero and into live moments."""
    pool = {}
    for n in S.ADAM_N:
        for kind in ("one", "mixed", "160"):
            ends, steps, lrs = S.adam_layout(n, kind)
            st = S.adam_state(n)
            g = S.adam_grad(st, 0)
            bufs = [_guarded(a, n) for a in (st["p"], g, st["m"], st["v"])]
            assert _adam_call(bufs, n, ends, lrs, steps) == 0, (n, kind)
            ss_e, bc_e = _per_element(ends, lrs, steps, n)
            state = (st["p"], st["m"], st["v"])
            _adam_check(bufs, dict(f64=state, f32=state, hip=state), g, ss_e, bc_e, pool, "")
    _judge_pool(pool, "Adam, segment geometry, one step:")


def test_adam_six_consecutive_steps():
    """six steps on one bucket of 1025 in the mixed layout, the round-off of the moments accumulating as in training: the kernel's
    state after every step against the float64 trajectory, the fp32 restatement running its own trajectory beside it."""
    n = 1025
    ends, steps0, lrs = S.adam_layout(n, "mixed")
    st = S.adam_state(n)
    hip = (st["p"], st["m"], st["v"])
    f64 = tuple(a.astype(np.float64) for a in hip)
    f32 = hip
    bufs = [_guarded(a, n) for a in (st["p"], np.zeros(n, np.float32), st["m"], st["v"])]
    for it in range(6):
        steps = [0 if t == 0 else t + it for t in steps0]
        g = S.adam_grad(st, it)
        bufs[1][:n] = torch.from_numpy(g).to(DEV)
        assert _adam_call(bufs, n, ends, lrs, steps) == 0
        ss_e, bc_e = _per_element(ends, lrs, steps, n)
        pool = {}
        hip, f32, f64 = _adam_check(bufs, dict(f64=f64, f32=f32, hip=hip), g, ss_e, bc_e, pool, f" after step {it + 1}")
        _judge_pool(pool, "Adam, six steps:")


def test_adam_argument_errors_touch_nothing():
    """161 segments, ends that decrease, a last end that differs from n, each buffer offset by 4 bytes: the argument error, and
    all four buffers as they were."""
    n = 1025
    st = S.adam_state(n)
    g = S.adam_grad(st, 0)
    src = (st["p"], g, st["m"], st["v"])
    bufs = [_guarded(a, n) for a in src]
    ends, steps, lrs = S.adam_layout(n, "mixed")
    bad = [("161 segments", list(range(160)) + [n], [1e-3] * 161, [1] * 161, None),
           ("decreasing ends", [10, 5, n], [1e-3] * 3, [1] * 3, None),
           ("last end below n", [10, n - 1], [1e-3] * 2, [1] * 2, None),
           ("last end beyond n", [10, n + 1], [1e-3] * 2, [1] * 2, None)]
    for what, e, l, s, _ in bad:
        assert _adam_call(bufs, n, e, l, s) == MH_ERR_ARG, what
    for which in range(4):
        ns = len(ends)
        ptrs = [b.data_ptr() + (4 if i == which else 0) for i, b in enumerate(bufs)]
        status = _status("mh_adam_step", *ptrs, n, ns, (ctypes.c_int64 * ns)(*ends), (ctypes.c_float * ns)(*lrs),
                         (ctypes.c_int64 * ns)(*steps), S.BETA1, S.BETA2, S.EPS)
        assert status == MH_ERR_ARG, f"buffer {which} offset by 4 bytes"
    torch.cuda.synchronize()
    for b, a in zip(bufs, src):
        assert np.array_equal(b[:n].cpu().numpy().view(np.int32), a.view(np.int32)) and bool((b[n:] == SENTINEL).all())
    assert _adam_call(bufs, n, ends, lrs, steps) == 0, "the same buffers with good arguments are accepted"


def test_adam_step_dev_flags_and_counters_in_one_process():
    """mh_adam_step_dev (adam_steps_kernel and the kernel's device-side step sizes): per-segment flags 0, 0.5, 1, 2, -1, NaN -- a NaN
    flag skips; the device counters go up by exactly one where the flag is positive; the scratch reads -1 / 1 for skipped segments;
    parameters and moments against the same float64 yardstick with the same step counts; two consecutive calls."""
    n = 2049
    ends, _, lrs = S.adam_layout(n, "mixed")
    ns = len(ends)
    flags = np.array([(0.0, 0.5, 1.0, 2.0, -1.0, float("nan"))[(s + 1) % 6] for s in range(ns)], np.float32)
    steps = np.array([(0, 1, 9, 999, 10 ** 6 - 1)[s % 5] for s in range(ns)], np.int64)
    st = S.adam_state(n)
    hip = (st["p"], st["m"], st["v"])
    f64, f32 = tuple(a.astype(np.float64) for a in hip), hip
    bufs = [_guarded(a, n) for a in (st["p"], np.zeros(n, np.float32), st["m"], st["v"])]
    flag_d, step_d = torch.from_numpy(flags).to(DEV), torch.from_numpy(steps).to(DEV)
    scratch = torch.full((2 * ns + 4,), SENTINEL, device=DEV)
    on = flags > 0                                   # NaN > 0 is false
    assert int(on.sum()) >= 6 and int((~on).sum()) >= 6
    for it in range(2):
        g = S.adam_grad(st, it)
        bufs[1][:n] = torch.from_numpy(g).to(DEV)
        status = _status("mh_adam_step_dev", *[b.data_ptr() for b in bufs], n, ns, (ctypes.c_int64 * ns)(*ends),
                         (ctypes.c_float * ns)(*lrs), _ptr(flag_d), _ptr(step_d), _ptr(scratch), S.BETA1, S.BETA2, S.EPS)
        assert status == 0
        steps = steps + on
        assert np.array_equal(step_d.cpu().numpy(), steps), "counters: + 1 where the flag is positive, untouched elsewhere"
        used = [int(t) if o else 0 for t, o in zip(steps, on)]
        ss, bc = S.adam_seg_params(lrs, used)
        sc = scratch.cpu().numpy().astype(np.float64)
        assert np.array_equal(sc[:ns][~on], np.full(int((~on).sum()), -1.0)) and np.array_equal(sc[ns:2 * ns][~on], np.ones(int((~on).sum())))
        assert bool((scratch[2 * ns:] == SENTINEL).all())
        # the device forms lr / (1 - b1^t) and sqrt(1 - b2^t) with its own double pow: the fp32 result may differ by one rounding
        assert np.all(np.abs(sc[:ns][on] - ss[on]) <= 2 * S.U * np.abs(ss[on])) and np.all(np.abs(sc[ns:2 * ns][on] - bc[on]) <= 2 * S.U)
        seg = S.adam_seg_of(ends, n)
        pool = {}
        hip, f32, f64 = _adam_check(bufs, dict(f64=f64, f32=f32, hip=hip), g, ss[seg], bc[seg], pool, f", call {it + 1}")
        _judge_pool(pool, "Adam, device-side steps:")


def test_flat_adam_grad_none_beside_stepping_lane_neighbours():
    """FlatAdam end to end: parameters of 3, 5, 2, 7 and 1 elements in one group, so that lanes hold elements of several tensors;
    the second has grad = None on the first and third of three steps while its lane neighbours step.  Against torch.optim.Adam in
    float64; torch.optim.Adam in fp32 on the CPU is the restatement.  Scale: the step size lr / (1 - b1^t)."""
    from morpheus_amd.optim import FlatAdam
    rng = np.random.RandomState(5)
    shapes = [(3,), (5,), (2,), (7,), (1,)]
    init = [(rng.randn(*s) * 0.1).astype(np.float32) for s in shapes]
    mk = lambda dev, dt: [torch.nn.Parameter(torch.from_numpy(a).to(dev).to(dt)) for a in init]
    mine, r32, r64 = mk(DEV, F32), mk("cpu", F32), mk("cpu", F64)
    lr = 1e-2
    opt = FlatAdam([{"name": "g0", "params": mine, "lr": lr}], betas=(0.9, 0.99), eps=1e-15)
    o32 = torch.optim.Adam(r32, lr=lr, betas=(0.9, 0.99), eps=1e-15, foreach=False, fused=False)
    o64 = torch.optim.Adam(r64, lr=lr, betas=(0.9, 0.99), eps=1e-15, foreach=False, fused=False)
    t_of = [0] * len(shapes)
    for it in range(3):
        opt.zero_grad()
        before = mine[1].detach().clone()
        for i, s in enumerate(shapes):
            gv = torch.from_numpy((rng.randn(*s) * 10.0 ** rng.randint(-6, 1)).astype(np.float32))
            none = i == 1 and it != 1
            t_of[i] += 0 if none else 1
            mine[i].grad = None if none else gv.clone().to(DEV)
            r32[i].grad = None if none else gv.clone()
            r64[i].grad = None if none else gv.double()
        opt.step(), o32.step(), o64.step()
        if it != 1:
            assert _same_bits(mine[1], before), "grad = None: the parameter stays bit-identical while its lane neighbours step"
        scale = torch.cat([torch.full(s, lr / (1.0 - 0.9 ** max(t, 1))) for s, t in zip(shapes, t_of)])
        S.judge(torch.cat([p.detach().cpu() for p in mine]), torch.cat([p.detach() for p in r32]), torch.cat([p.detach() for p in r64]),
                scale, f"FlatAdam, grad = None inside a group, step {it + 1}: parameter")
    assert [int(float(opt.state_dict()["state"][i]["step"])) for i in range(5)] == [3, 1, 3, 3, 3]
