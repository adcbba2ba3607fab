"""Float64 yardsticks, fp32 restatements and case builders for the caller-side loss kernels of csrc/losses.hip -- test
infrastructure, plain torch on the CPU, like tests/step_f64_oracle.py.

Each of the six operations is written ONCE, dtype-generic, from the reference's definition with torch operators, with no reference to
the shape of a kernel's loops or reductions; gradients come from torch autograd:
    masked mean     morpheus.py:1090-1145 and :556      (mean_run)        ortho perturb   :518-528, F.normalize      (ortho_run)
    pose apply      models/pose.py:4-64, model.py:335-346 (pose_run)      render loss     :929-983, F.binary_cross_entropy (render_run)
    smooth points   :530-547                            (smooth_run)      bg blend        :686-694                   (blend_run)
Run in float64 on the fp32 inputs they are the yardstick; run in fp32 they are the restatement whose own error against float64 sets
the allowance: a kernel's worst error over the quantity's natural scale stays within FACTOR x the restatement's worst (judge), or a
floor of so many roundings where the restatement happens to be exact.  Decisions that fp32 data makes (clamps at the fp32 bounds, the
`valid` / `keep` radius test) are made on the fp32 values in both runs: the float64 run integrates the same selection.

The `*_check` functions hold the judgement of one call; tests/test_losses_oracle_host.py passes the fp32 restatement (and
deliberately wrong ones) through them on the CPU, tests/test_gpu_losses_f64.py the kernels' results.  The `*_case` builders place the
sizes and values at which the kernels branch; the host test asserts that they do.
"""
import math

import numpy as np
import torch
import torch.nn.functional as Fn

from tests.f64_judge import F32, F64, U, assert_figures, figures_vs_f64, flat64, judge_sum, report

REPORT = "MORPHEUS_LOSSES_REPORT"
FACTOR = 2.0            # never raised
FLOOR_ULPS = 4

# constants of csrc/losses.hip, repeated (the GPU module cross-checks mh_masked_mean_workspace_floats() == 2 * MEAN_BLOCKS)
MEAN_BLOCKS, MEAN_THREADS, POSE_RAYS_PER_BLOCK, RENDER_THREADS = 512, 256, 1024, 1024
LO = float(np.float32(1e-5))                        # the clamp / clip bounds as the fp32 numbers the kernels compare with
HI = float(np.float32(1.0) - np.float32(1e-5))
RADIUS = float(np.float32(1.1))


def _t32(v):
    return torch.tensor(v, dtype=F32)


def _next(v, towards):
    return float(torch.nextafter(_t32(v), _t32(towards)))


def ceil_div(a, b):
    return -(-int(a) // int(b))


# -------------------------------------------------------------------------------------------------------- the judgement
def judge(hip, ref32, f64, scale, what, floor=FLOOR_ULPS * U, slack=2):
    """f64_judge.judge_vs_f64 at FACTOR, with the figures printed and appended to the JSON-lines file MORPHEUS_LOSSES_REPORT names.
    Elements of zero scale must equal the yardstick exactly, the restatement's too.  -> the record"""
    f = figures_vs_f64(hip, ref32, f64, scale, what, floor)
    rec = dict(what=what, worst_hip=f["worst_hip"], worst_ref=f["worst_ref"], ratio=(f["worst_hip"] / f["worst_ref"] if f["worst_ref"] > 0 else None),
               n_hip=f["n_hip"], n_ref=f["n_ref"], n=f["n"], floor=floor, factor=FACTOR)
    print(f"[losses-f64] {what}: kernel {f['worst_hip']:.3e}  fp32 restatement {f['worst_ref']:.3e}  above {floor:.1e}: {f['n_hip']} / {f['n_ref']}  of {f['n']}")
    report(REPORT, rec)
    assert_figures(f, what, FACTOR, floor, slack, ref_zero_scale_exact=True)
    return rec


def judged_sum(hip, ref32, f64, abs_sum, count, what):
    """f64_judge.judge_sum with the restatement's own error as `extra`, printed and reported like judge"""
    extra = (flat64(ref32) - flat64(f64)).abs()
    rec = dict(judge_sum(hip, f64, abs_sum, count, what, extra=extra), what=what, count=count, worst_ref=float(extra.max()) if extra.numel() else 0.0)
    print(f"[losses-f64] {what}: kernel {rec['worst_hip']:.3e}  fp32 restatement {rec['worst_ref']:.3e}  = {rec['ratio']:.3f} x the bound of {count} roundings")
    report(REPORT, rec)
    return rec


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == F32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


# =========================================================================================================== masked mean
MEAN_KINDS = ("identity", "square", "abs", "entropy", "eikonal", "absdiff", "sqdiff")
MEAN_M_C1 = (1, 255, 256, 257, 1024, 1025, 2049, 524288, 524289)     # one partial block, wave / block tails, block 2, the cap, trip 5
MEAN_M_C3 = (1, 85, 86, 342, 174763)                                   # i / C crosses block edges inside a row; 3 x 174763 = 524289
MEAN_C3_KINDS = ("abs", "absdiff", "sqdiff", "eikonal")
MEAN_FULL_M = {1: (257, 2049), 3: (86,)}                               # every n_valid and every weight kind at these sizes
MEAN_G = 1.75                                                          # the gradient arriving at the mean (exact in fp32)
# roundings inside one term f(a[, b]) as the kernel forms it (each fp32 operator one; log2f / logf two; sqrtf one)
#   entropy: clamp exact; two log2f (4), 1 - x twice (2), two products, one subtraction = 9.  The rounding of 1 - x enters
#   log2(1 - x) as an ABSOLUTE U / 2 ln 2, not relative to the term: covered by the term count as long as the call's mean term is
#   above 0.1 (the host test asserts it for the entropy cases)
#   eikonal: three squares, two adds, sqrtf, - 1, the square = 8
MEAN_TERM_ROUNDINGS = dict(identity=0, square=1, abs=0, entropy=9, eikonal=8, absdiff=1, sqdiff=2)
ENTROPY_EDGES = (LO, HI, _next(LO, 0.0), _next(LO, 1.0), _next(HI, 0.0), _next(HI, 1.0), 0.0, 1.5, 0.5)


def mean_blocks(n):
    """the grid of masked_mean_partial_kernel: one block per 4 x MEAN_THREADS elements, at least 1, at most MEAN_BLOCKS"""
    return min(max(ceil_div(n, 4 * MEAN_THREADS), 1), MEAN_BLOCKS)


def mean_trips(n):
    return max(ceil_div(n, mean_blocks(n) * MEAN_THREADS), 1)


def mean_depth(kind, M, C, weighted):
    """The kernel's longest chain of roundings behind out[0], from the constants: `trips` adds in a lane, 6 shuffle adds, 3 wave
    adds, the final pass (ceil(blocks / 256) lane adds + 6 + 3), the division, the roundings inside one term; with row weights the
    product f * w, the same chain of adds for the sum of the weights, and per_row * sum (the max with 1 is exact)."""
    n = M if kind == "eikonal" else M * C
    adds = mean_trips(n) + 6 + 3 + ceil_div(mean_blocks(n), MEAN_THREADS) + 9
    return adds + 1 + MEAN_TERM_ROUNDINGS[kind] + ((1 + adds + 1) if weighted else 0)


def mean_term(kind, a, b):
    if kind == "identity":
        return a
    if kind == "square":
        return a ** 2
    if kind == "abs":
        return a.abs()
    if kind == "entropy":
        x = a.clamp(LO, HI)
        return -x * torch.log2(x) - (1 - x) * torch.log2(1 - x)
    if kind == "eikonal":
        return (torch.linalg.norm(a, ord=2, dim=-1) - 1.0) ** 2
    if kind == "absdiff":
        return (a - b).abs()
    assert kind == "sqdiff"
    return torch.square(a - b)


def mean_case(kind, M, C, n_valid=None, weights=None, seed=3):
    """a (and b) [M] for C = 1, [M, C] otherwise ([M, 3] for eikonal).  The data edges sit in the first elements: entropy
    ENTROPY_EDGES; abs / absdiff exact zeros and a == b; eikonal a zero row and rows of norm exactly 1.  n_valid: an int of any
    sign and size; the rows behind it hold NaN in a, b and the weights.  weights: None, "01", "nonint", "tiny" (their sum below
    1 / per_row: the denominator clamps to 1) or "zero"."""
    assert C == 3 or kind != "eikonal"
    rng = np.random.RandomState(seed + 7 * M + C)
    shape = (M,) if C == 1 else (M, C)
    a = (rng.randn(*shape) * 0.6).astype(np.float32)
    b = rng.randn(*shape).astype(np.float32) if kind in ("absdiff", "sqdiff") else None
    flat = a.reshape(-1)
    if kind == "entropy":
        flat[:] = (rng.rand(flat.size) * 1.2 - 0.1).astype(np.float32)          # a tenth outside [0, 1]
        k = min(flat.size, len(ENTROPY_EDGES))
        flat[:k] = np.array(ENTROPY_EDGES[:k], np.float32)
    elif kind == "eikonal":
        rows = np.array([[0, 0, 0], [1, 0, 0], [0, -1, 0], [0.6, 0.8, 0]], np.float32)
        a[:min(M, 4)] = rows[:min(M, 4)]
    elif kind in ("abs", "absdiff", "sqdiff"):
        k = min(flat.size, 6)
        if b is None:
            flat[:k:2] = 0.0                               # sign(0) = 0
        else:
            b.reshape(-1)[:k] = flat[:k]                   # a == b
    w = None
    per_row = 1 if kind == "eikonal" else C
    if weights == "01":
        w = (rng.rand(M) < 0.7).astype(np.float32)
    elif weights == "nonint":
        w = (rng.rand(M) * 2.0).astype(np.float32)
    elif weights == "tiny":
        w = (rng.rand(M) * (0.5 / (per_row * max(M, 1))) + 1e-4 / (per_row * max(M, 1))).astype(np.float32)
    elif weights == "zero":
        w = np.zeros(M, np.float32)
    else:
        assert weights is None
    if n_valid is not None:
        r = min(max(n_valid, 0), M)
        a[r:] = np.nan
        if b is not None:
            b[r:] = np.nan
        if w is not None:
            w[r:] = np.nan
    t = lambda x: None if x is None else torch.from_numpy(x)
    return dict(kind=kind, M=M, C=C, per_row=per_row, a=t(a), b=t(b), w=t(w), n_valid=n_valid, weights=weights, g=MEAN_G,
                name=f"{kind} M={M} C={C} n_valid={n_valid} weights={weights}")


def mean_cases(kind, C):
    """every size x (all rows, n_valid, row_weight, both); at MEAN_FULL_M every n_valid of {0, 1, M - 1, M, M + 5, -3} without and
    with weights, and every weight kind"""
    out = []
    for M in (MEAN_M_C1 if C == 1 else MEAN_M_C3):
        nv = max(M - 1, 1) if M > 1 else 1
        out += [mean_case(kind, M, C), mean_case(kind, M, C, n_valid=nv), mean_case(kind, M, C, weights="nonint"),
                mean_case(kind, M, C, n_valid=nv, weights="01")]
        if M in MEAN_FULL_M[C]:
            for n_valid in (0, 1, M - 1, M, M + 5, -3):
                out += [mean_case(kind, M, C, n_valid=n_valid), mean_case(kind, M, C, n_valid=n_valid, weights="nonint")]
            out += [mean_case(kind, M, C, weights=wk) for wk in ("01", "tiny", "zero")]
    return out


def mean_empty_case(kind):
    C = 3 if kind == "eikonal" else 1
    a = torch.zeros((0, 3) if kind == "eikonal" else (0,))
    return dict(kind=kind, M=0, C=C, per_row=1, a=a, b=(a.clone() if kind in ("absdiff", "sqdiff") else None), w=None, n_valid=None,
                weights=None, g=MEAN_G, name=f"{kind} empty")


def mean_run(case, dtype, wrong=None):
    """value = sum over the valid rows of f * w / den;  den = per_row * max(rows, 1), rows = clamp(n_valid, 0, M) (the reference's
    .mean() over the samples) or max(per_row * sum of the weights, 1) (morpheus.py:556).  The rows behind n_valid are never touched.
    wrong: "weights_per_channel", "n_valid_unclamped", "clamp_gt", "den_no_max" -- the deliberately wrong restatements of the host
    test.  -> dict(value, ga, gb, abs_mean, fprime) (abs_mean: sum |f w| / den; fprime: |d f / d a| element by element)"""
    kind, M, C, per_row = case["kind"], case["M"], case["C"], case["per_row"]
    a = case["a"].to(dtype).clone().requires_grad_(True)
    b = None if case["b"] is None else case["b"].to(dtype).clone().requires_grad_(True)
    rows = M if case["n_valid"] is None else max(case["n_valid"], 0)
    if wrong != "n_valid_unclamped":
        rows = min(rows, M)
    r = min(rows, M)
    av, bv = a[:r], (None if b is None else b[:r])
    if wrong == "clamp_gt" and kind == "entropy":           # the clamp's gradient with > and < at the bounds
        x = torch.where((av > LO) & (av < HI), av, av.detach().clamp(LO, HI))
        f = -x * torch.log2(x) - (1 - x) * torch.log2(1 - x)
    else:
        f = mean_term(kind, av, bv)
    if case["w"] is None:
        fw, den = f, torch.tensor(float(per_row * max(rows, 1)), dtype=dtype)
    else:
        w = case["w"][:r].to(dtype)
        fw = f * w.view(-1, *([1] * (f.dim() - 1)))
        sw = w.sum() * (C if wrong == "weights_per_channel" and kind != "eikonal" else 1)
        den = per_row * sw
        if wrong != "den_no_max":
            den = den.clamp(min=1.0)
    value = fw.sum() / den
    leaves = [a] + ([b] if b is not None else [])
    grads = torch.autograd.grad(value * case["g"], leaves, retain_graph=True)
    fprime = torch.autograd.grad(f.sum(), a)[0].abs()
    return dict(value=value.detach(), ga=grads[0], gb=(grads[1] if b is not None else None), abs_mean=(fw.detach().abs().sum() / den).detach(),
                den=den.detach(), fprime=fprime)


def mean_scales(case, r64):
    """value: the float64 mean of the absolute weighted terms, sum |f w| / den.
    gradient element: |g| x max |f'| over the call x the row's weight / den; 0 behind n_valid, at zero weight and wherever the
    float64 gradient is an exact zero of the definition (outside the clamp, sign(0), a zero row)"""
    M = case["M"]
    r = M if case["n_valid"] is None else min(max(case["n_valid"], 0), M)
    fmax = float(r64["fprime"].max()) if r64["fprime"].numel() and r > 0 else 0.0
    w = torch.ones(M, dtype=F64) if case["w"] is None else torch.nan_to_num(case["w"].double(), nan=0.0)
    w[r:] = 0.0
    s = (abs(case["g"]) * fmax * w / float(r64["den"])).view(-1, *([1] * (case["a"].dim() - 1))).expand_as(case["a"]).clone()
    s[r64["ga"] == 0] = 0.0
    return float(r64["abs_mean"]), s


def mean_check(case, got, r32, r64, what=None):
    """got: dict(value, ga[, gb]) of the kernel (or of a restatement).  Value: within FACTOR x the restatement's error, floor
    mean_depth x U.  Gradients: judge at FACTOR, floor 4 U, exact where the scale is 0."""
    what = what or case["name"]
    vs, gs = mean_scales(case, r64)
    depth = mean_depth(case["kind"], case["M"], case["C"], case["w"] is not None)
    recs = [judge(got["value"], r32["value"], r64["value"], vs, f"mean {what}: value", floor=depth * U)]
    if got.get("ga") is not None:
        assert tuple(got["ga"].shape) == tuple(case["a"].shape)
        recs.append(judge(got["ga"], r32["ga"], r64["ga"], gs, f"mean {what}: g_a"))
    if got.get("gb") is not None:
        recs.append(judge(got["gb"], r32["gb"], r64["gb"], gs, f"mean {what}: g_b"))
    return recs


# ========================================================================================================= ortho perturb
ORTHO_M = (1, 63, 64, 255, 256, 257, 1025)
ORTHO_SCALES = (0.004, 1.0)
ORTHO_EDGES = (("u = 0, +z", (0.0, 0.0, 1.0)), ("u = 0, -z", (0.0, 0.0, -1.0)), ("u = 0, length 5", (0.0, 0.0, 5.0)),
               ("nearly vertical", (1e-7, 0.0, 1.0)), ("zero", (0.0, 0.0, 0.0)), ("below the clamp", (6e-14, -5e-14, 6.2e-14)),
               ("x axis", (1.0, 0.0, 0.0)), ("-x axis", (-2.0, 0.0, 0.0)), ("y axis", (0.0, 1.0, 0.0)), ("-y axis", (0.0, -3.0, 0.0)),
               ("below the clamp along z", (0.0, 0.0, 1e-13)))
ORTHO_PHI = (0.0, math.pi / 2, math.pi, 2 * math.pi)


ORTHO_MAX_CONDITION = 8.0


def ortho_condition(n, phi, g):
    """Float64, per row: how much the two projections of the backward pass cancel -- the size of what enters them (the gradient
    reaching u over |u_raw|, and the one reaching n^ directly) over the size of what is left behind them, |n| g_n; 1 in the
    degenerate rows, which take the branches without a projection.  A rounding of u or n^ enters g_n multiplied by this number,
    and for a random g it is heavy-tailed (P(> k) ~ 1 / k): without a bound the one worst row of a call decides the call's figure,
    and there two correct fp32 evaluations differ by a random factor that a fixed factor of 2 cannot hold."""
    n, phi, g = n.double(), phi.double().reshape(-1, 1), g.double()
    m = n.norm(dim=-1, keepdim=True)
    nh = n / m.clamp(min=1e-12)
    ur = torch.stack([nh[:, 1], -nh[:, 0], torch.zeros_like(nh[:, 2])], -1)
    r = ur.norm(dim=-1, keepdim=True)
    u = ur / r.clamp(min=1e-12)
    c, s = torch.cos(phi), torch.sin(phi)
    gu = c * g + s * torch.cross(g, nh, dim=-1)
    gu[:, 2] = 0.0
    pu = gu - u * (u * gu).sum(-1, keepdim=True)
    gur = pu / r.clamp(min=1e-12)
    gn = s * torch.cross(u, g, dim=-1) + torch.stack([-gur[:, 1], gur[:, 0], torch.zeros_like(gur[:, 2])], -1)
    pn = gn - nh * (nh * gn).sum(-1, keepdim=True)
    k = (gu.norm(dim=-1) / r.clamp(min=1e-12).reshape(-1) + (s * torch.cross(u, g, dim=-1)).norm(dim=-1)) / pn.norm(dim=-1)
    live = ((r > 1e-12) & (m > 1e-12)).reshape(-1)
    return torch.where(live, torch.nan_to_num(k, nan=float("inf")), torch.ones_like(k))


def ortho_case(M, seed=5):
    """x: random in the even rows, exactly 0 in the odd ones (there the output IS the displacement); normals random at lengths
    1e-3 .. 1e3, the edge normals of ORTHO_EDGES in the first rows (the list rotated by M, so that M = 1 does not always meet
    the first one); phi 0, pi/2, pi, 2 pi in the edge rows, random elsewhere.  edge[i]: the edge's name per row (None: random).
    The incoming gradient g is random, redrawn in the rows whose ortho_condition exceeds ORTHO_MAX_CONDITION."""
    rng = np.random.RandomState(seed + M)
    x = rng.randn(M, 3).astype(np.float32)
    x[1::2] = 0.0
    dirs = rng.randn(M, 3)
    n = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * 10.0 ** (rng.rand(M, 1) * 6 - 3)).astype(np.float32)
    phi = (rng.rand(M) * 2 * math.pi).astype(np.float32)
    edge = [None] * M
    for i in range(min(M, len(ORTHO_EDGES))):
        name, v = ORTHO_EDGES[(i + M) % len(ORTHO_EDGES)]
        n[i], edge[i] = np.array(v, np.float32), name
        phi[i] = np.float32(ORTHO_PHI[(i + M // 7) % 4])
    t = torch.from_numpy
    u_zero = torch.tensor([e is not None and (e.startswith("u = 0") or e in ("zero", "below the clamp along z")) for e in edge])
    g = t(rng.randn(M, 3).astype(np.float32))
    for _ in range(200):
        bad = ortho_condition(t(n), t(phi), g) > ORTHO_MAX_CONDITION
        if not bool(bad.any()):
            break
        g[bad] = t(rng.randn(int(bad.sum()), 3).astype(np.float32))
    return dict(M=M, x=t(x), n=t(n), phi=t(phi)[:, None], g=g, edge=edge, u_zero=u_zero)


def ortho_run(case, scale, dtype):
    """x + scale (cos(phi) u + sin(phi) v),  n^ = normalize(n), u = normalize((n^_y, -n^_x, 0 n^_z)), v = n^ x u, normalize as
    F.normalize (a division by max(|.|, 1e-12)).  -> dict(out, disp, gn, gx)"""
    x = case["x"].to(dtype).clone().requires_grad_(True)
    n = case["n"].to(dtype).clone().requires_grad_(True)
    phi = case["phi"].to(dtype)
    nh = Fn.normalize(n, dim=-1)
    u = Fn.normalize(torch.stack([nh[..., 1], -nh[..., 0], nh[..., 2] * 0.0], -1), dim=-1)
    v = torch.cross(nh, u, dim=-1)
    disp = (torch.cos(phi) * u + torch.sin(phi) * v) * scale
    out = x + disp
    gx, gn = torch.autograd.grad(out, [x, n], case["g"].to(dtype))
    return dict(out=out.detach(), disp=disp.detach(), gn=gn, gx=gx)


def ortho_check(case, scale, got, r32, r64, what, pool=None):
    """got: dict(out, gn, gx).  Output, displacement out - x, and the displacement where x = 0 (the output itself): scale |scale|,
    floor 4 U.  Rows with u = 0: the point does not move, bit for bit.  g_n per row, the scale the row's largest |g_n| in float64
    (the degenerate rows reach 1e12 |g| and more), judged in every call on that call's rows; with `pool` (a list) the rows are
    also collected for one further judgement over the calls of every size (ortho_judge_pool), the steadier figure for the table.
    x.grad is g bit for bit."""
    x64 = case["x"].double()
    out = got["out"].detach().cpu()
    recs = [judge(out, r32["out"], r64["out"], abs(scale), f"ortho {what}: output")]
    recs.append(judge(out.double() - x64, r32["out"].double() - x64, r64["disp"], abs(scale), f"ortho {what}: displacement"))
    still = (case["x"] == 0).all(-1)
    if bool(still.any()):
        recs.append(judge(out[still], r32["out"][still], r64["disp"][still], abs(scale), f"ortho {what}: displacement at x = 0"))
    uz = case["u_zero"]
    assert bool((r64["disp"][uz] == 0).all()) and same_bits(out[uz], case["x"][uz]), f"ortho {what}: a row with u = 0 moved"
    row_scale = r64["gn"].abs().amax(-1, keepdim=True).expand(-1, 3)
    recs.append(judge(got["gn"], r32["gn"], r64["gn"], row_scale, f"ortho {what}: g_n"))
    if pool is not None:
        pool.append(tuple(flat64(t) for t in (got["gn"], r32["gn"], r64["gn"], row_scale)))
    assert same_bits(got["gx"], case["g"]), f"ortho {what}: x.grad is not g bit for bit"
    return recs


def ortho_judge_pool(pool, what):
    return judge(*(torch.cat(ts) for ts in zip(*pool)), f"ortho {what}: g_n, pooled")


# ============================================================================================================ pose apply
POSE_N = (1, 63, 64, 255, 256, 257, 1023, 1024, 1025, 2049)
POSE_FRAMES = ([4], [4, 7], [4, 7, 4], [4, 7, 4, 7], [2, 2, 2])
POSE_F = 9
POSE_ZERO_FRAME = 7
POSE_MODES = ("both", "o", "d")
POSE_MAX_CANCELLATION = 4.0        # no entry of a case's R is a difference smaller than a quarter of its monomials' absolute sum
# roundings behind one angle gradient besides the adds of the sum: the product g_d' d (1); a monomial of dR/dtheta: three sin / cos
# of 2 each (6), two products, the add of a two-monomial entry (9); the product with the sum (1); the eight adds of the contraction
POSE_CONTRACTION_ROUNDINGS = 1 + 9 + 1 + 8


def pose_count(n, rows_of_frame):
    """adds in a lane (ceil(min(n, 1024) / 256) trips), 6 shuffle adds, 3 wave adds, the blocks of a row, the rows of the frame, and
    the contraction with dR / dtheta"""
    return ceil_div(min(n, POSE_RAYS_PER_BLOCK), 256) + 6 + 3 + ceil_div(n, POSE_RAYS_PER_BLOCK) + rows_of_frame + POSE_CONTRACTION_ROUNDINGS


def pose_case(n, frames, seed=11):
    """F = 9 frames, angles uniform in +-3 (redrawn while an entry of R cancels beyond POSE_MAX_CANCELLATION, so that the floor of
    pose_forward_floor stays within 4 x its count), translations ~ 0.3 N(0, 1), frame 7 all zero; B = len(frames) rows of n rays"""
    rng = np.random.RandomState(seed + 13 * n + len(frames))
    pose = np.concatenate([rng.rand(POSE_F, 3) * 6 - 3, rng.randn(POSE_F, 3) * 0.3], 1).astype(np.float32)
    pose[POSE_ZERO_FRAME] = 0.0
    for _ in range(1000):               # angles redrawn while an entry of R cancels beyond POSE_MAX_CANCELLATION (pose_forward_floor)
        rot = torch.from_numpy(pose[:, :3]).double()
        bad = ((_abs_rotation(rot) / _rotation(rot).abs()).amax((1, 2)) > POSE_MAX_CANCELLATION).numpy()
        if not bad.any():
            break
        pose[bad, :3] = (rng.rand(int(bad.sum()), 3) * 6 - 3).astype(np.float32)
    N = n * len(frames)
    d = rng.randn(N, 3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return dict(n=n, frames=list(frames), B=len(frames), pose=t(pose), o=t(rng.randn(N, 3)), d=t(d / np.linalg.norm(d, axis=1, keepdims=True)),
                go=t(rng.randn(N, 3)), gd=t(rng.randn(N, 3)), name=f"n={n} frames={list(frames)}")


def _rotation(rot):
    """models/pose.py:41-58: Euler angles [B, 3] -> R [B, 3, 3], the three columns stacked last"""
    ca, cb, cg = torch.cos(rot[:, 0]), torch.cos(rot[:, 1]), torch.cos(rot[:, 2])
    sa, sb, sg = torch.sin(rot[:, 0]), torch.sin(rot[:, 1]), torch.sin(rot[:, 2])
    c1 = torch.stack([ca * cb, sa * cb, -sb], -1)
    c2 = torch.stack([ca * sb * sg - sa * cg, sa * sb * sg + ca * cg, cb * sg], -1)
    c3 = torch.stack([ca * sb * cg + sa * sg, sa * sb * cg - ca * sg, cb * cg], -1)
    return torch.stack([c1, c2, c3], -1)


def pose_run(case, dtype, wrong=None):
    """o' = o + t_f, d' = sum_c R_f[r, c] d_c for the frame f of the ray's row; d pose of <o', go>, of <d', gd> and of their sum.
    wrong = "pose_overwrite": the rows of one frame overwrite each other's gradient instead of adding.
    -> dict(o1, d1, R, t, grads={"both", "o", "d"})"""
    B, n = case["B"], case["n"]
    ids = torch.tensor(case["frames"])
    pose = case["pose"].to(dtype).clone().requires_grad_(True)
    rows = pose[ids]                                   # the gather: its adjoint adds the rows of one frame up
    if wrong == "pose_overwrite":
        rows = rows.detach().requires_grad_(True)
    R, t = _rotation(rows[:, 0:3]), rows[:, 3:6]
    o, d = case["o"].to(dtype), case["d"].to(dtype)
    o1 = (o.view(B, n, 3) + t[:, None]).view(-1, 3)
    d1 = (d.view(B, n, 1, 3) * R[:, None]).sum(-1).view(-1, 3)
    lo, ld = (o1 * case["go"].to(dtype)).sum(), (d1 * case["gd"].to(dtype)).sum()
    grads = {}
    for mode, loss in (("both", lo + ld), ("o", lo), ("d", ld)):
        if wrong == "pose_overwrite":
            g_rows = torch.autograd.grad(loss, rows, retain_graph=True)[0]
            g = torch.zeros_like(pose)
            for r in range(B):
                g[case["frames"][r]] = g_rows[r]
            grads[mode] = g
        else:
            grads[mode] = torch.autograd.grad(loss, pose, retain_graph=True)[0]
    return dict(o1=o1.detach(), d1=d1.detach(), R=R.detach(), t=t.detach(), grads=grads)


def _abs_rotation_derivatives(rot):
    """the sums of the ABSOLUTE monomials of dR/dalpha, dR/dbeta, dR/dgamma [B, 3(angle), 3, 3]"""
    A, B_, G = (torch.cos(rot[:, k]).abs() for k in range(3))
    a, b, g = (torch.sin(rot[:, k]).abs() for k in range(3))
    z = torch.zeros_like(A)
    st = lambda rows: torch.stack([torch.stack(r, -1) for r in rows], -2)
    da = st([[a * B_, a * b * g + A * G, a * b * G + A * g], [A * B_, A * b * g + a * G, A * b * G + a * g], [z, z, z]])
    db = st([[A * b, A * B_ * g, A * B_ * G], [a * b, a * B_ * g, a * B_ * G], [B_, b * g, b * G]])
    dg = st([[z, A * b * G + a * g, A * b * g + a * G], [z, a * b * G + A * g, a * b * g + A * G], [z, B_ * G, B_ * g]])
    return torch.stack([da, db, dg], 1)


def pose_abs_sums(case, mode):
    """float64: per frame and pose parameter the sum over the frame's rays of the absolute contracted terms
    |gd_r| |dR_rc / dtheta| |d_c| (angles) and |go_k| (translations); 0 where the loss does not reach"""
    B, n = case["B"], case["n"]
    ids = torch.tensor(case["frames"])
    rot = case["pose"].double()[ids][:, 0:3]
    S = (case["gd"].double().abs().view(B, n, 3, 1) * case["d"].double().abs().view(B, n, 1, 3)).sum(1)      # [B, 3, 3]
    ang = (_abs_rotation_derivatives(rot) * S[:, None]).sum((2, 3))                                            # [B, 3]
    tr = case["go"].double().abs().view(B, n, 3).sum(1)
    per_row = torch.cat([ang * (mode != "o"), tr * (mode != "d")], 1)
    return torch.zeros(POSE_F, 6, dtype=F64).index_add(0, ids, per_row)


def pose_forward_scales(case, r64):
    """o': |o| + |t|;  d': sum_c |R_rc d_c|"""
    B, n = case["B"], case["n"]
    so = (case["o"].double().abs().view(B, n, 3) + r64["t"].abs()[:, None]).view(-1, 3)
    sd = (case["d"].double().abs().view(B, n, 1, 3) * r64["R"].abs()[:, None]).sum(-1).view(-1, 3)
    return so, sd


def _abs_rotation(rot):
    """the sums of the ABSOLUTE monomials of R [B, 3, 3]"""
    A, B_, G = (torch.cos(rot[:, k]).abs() for k in range(3))
    a, b, g = (torch.sin(rot[:, k]).abs() for k in range(3))
    st = lambda rows: torch.stack([torch.stack(r, -1) for r in rows], -2)
    return st([[A * B_, A * b * g + a * G, A * b * G + a * g], [a * B_, a * b * g + A * G, a * b * G + A * g], [b, B_ * g, B_ * G]])


# roundings behind one d'_r = sum_c R_rc d_c in units of U = 2^-24: three sin / cos of one ulp = 2 U each (6), the two products of
# a monomial (2), the add of a two-monomial entry (1), the product with d_c (1), the two adds of the sum (2)
POSE_FORWARD_ROUNDINGS = 12


def pose_forward_floor(case, r64):
    """The floor for d' at the scale sum_c |R_rc d_c|.  An entry of R that is a difference of two monomials carries the roundings
    of the monomials, not of their difference: the first-order bound of an fp32 evaluation is POSE_FORWARD_ROUNDINGS x U x
    sum_c Rabs_rc |d_c| with Rabs the sums of the absolute monomials.  Over the issue's scale that is the count times the call's
    largest ratio of the two sums (1 where no entry cancels).  R is one set of nine numbers per frame, so this error is common to
    all rays of a row: kernel and restatement each draw it once per frame, and a factor between two single draws means nothing."""
    B, n = case["B"], case["n"]
    rot = case["pose"].double()[torch.tensor(case["frames"])][:, 0:3]
    d = case["d"].double().abs().view(B, n, 1, 3)
    ratio = (d * _abs_rotation(rot)[:, None]).sum(-1) / (d * r64["R"].abs()[:, None]).sum(-1)
    return POSE_FORWARD_ROUNDINGS * U * float(ratio.max())


def pose_check_forward(case, o1, d1, r32, r64, what=None):
    what = what or case["name"]
    so, sd = pose_forward_scales(case, r64)
    B, n = case["B"], case["n"]
    rot = case["pose"].double()[torch.tensor(case["frames"])][:, 0:3]
    sd_abs = (case["d"].double().abs().view(B, n, 1, 3) * _abs_rotation(rot)[:, None]).sum(-1).view(-1, 3)
    # The second judgement of d' is at the scale the floor's reasoning is about, where the floor is the bare count.  The count is
    # kept at its derived 12 and not lowered to the 4 U of a single operator: R costs three sin / cos of up to one ulp (2 U) each
    # before any product is rounded, a frame draws that error once for all its rays, and a floor below the chain's own bound would
    # hold a correct kernel only by the luck of the frames drawn.
    return [judge(o1, r32["o1"], r64["o1"], so, f"pose {what}: o'"),
            judge(d1, r32["d1"], r64["d1"], sd, f"pose {what}: d'", floor=pose_forward_floor(case, r64)),
            judge(d1, r32["d1"], r64["d1"], sd_abs, f"pose {what}: d' over the absolute monomials", floor=POSE_FORWARD_ROUNDINGS * U)]


def pose_check_grad(case, mode, g_pose, r32, r64, what=None):
    """judge_sum with the derived count; frames outside the batch (and parameters the loss does not reach) are exactly 0"""
    what = what or case["name"]
    g_pose = g_pose.detach().cpu()
    count = pose_count(case["n"], max(case["frames"].count(f) for f in set(case["frames"])))
    rec = judged_sum(g_pose, r32["grads"][mode], r64["grads"][mode], pose_abs_sums(case, mode), count, f"pose {what}: g_pose, loss on {mode}")
    outside = [f for f in range(POSE_F) if f not in case["frames"]]
    assert bool((g_pose[outside] == 0).all()), f"pose {what}: a frame outside the batch has a gradient"
    return rec


# =========================================================================================================== render loss
RENDER_N = (0, 1, 63, 64, 1023, 1024, 1025, 2049, 3000)
RENDER_WEIGHTS = {"ones": (1.0, 1.0, 1.0), "no mask": (1.0, 0.0, 0.1)}       # + the config's, which the tests read
RENDER_G = 0.75
MASK_EDGES = (0.0, 0.5, _next(0.5, 1.0), 1.0)
OPACITY_EDGES = (0.0, LO, _next(LO, 0.0), _next(LO, 1.0), HI, _next(HI, 0.0), _next(HI, 1.0), 1.0)
DEPTH_EDGES = (0.0, -0.1, 1e-30)
# the placed rays: axis-aligned, every operation of the chain exact, |o + depth d| = the radius, one ulp under, one ulp over
_R_UNDER, _R_OVER = _next(RADIUS, 0.0), _next(RADIUS, 2.0)
PLACED_RAYS = (("on", (0.25, 0.0, 0.0), (1.0, 0.0, 0.0), float(np.float32(RADIUS) - np.float32(0.25))),
               ("under", (0.0, -0.5, 0.0), (0.0, 1.0, 0.0), float(np.float32(_R_UNDER) + np.float32(0.5))),
               ("over", (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), _R_OVER))
RENDER_EDGE_RAYS = 3 + 2 * len(OPACITY_EDGES) + len(MASK_EDGES) + len(DEPTH_EDGES)        # 26


def render_case(N, seed=2):
    """one batch of N rays in the layouts mh_render_loss_* takes: pred_rgb [N, 3], pred_depth [N], opacity [N], image [3, N],
    depth [N], mask [N], bg [N, 3], rays [N, 3].  The first RENDER_EDGE_RAYS rays (as many as N holds) are the edges: the three
    placed rays, every opacity edge under mask 1 and under mask 0, every mask edge, every depth edge (under mask 1)."""
    rng = np.random.RandomState(seed + N)
    r = lambda *s: rng.rand(*s).astype(np.float32)
    mask = np.where(rng.rand(N) < 0.8, (rng.rand(N) < 0.7).astype(np.float32), r(N))
    depth = np.maximum(r(N) * 2.0 - 0.3, 0.0).astype(np.float32)
    o = (rng.randn(N, 3) * 0.2 + np.array([0.0, 0.0, -1.2])).astype(np.float32)
    d = rng.randn(N, 3) * 0.3 + np.array([0.0, 0.0, 1.0])
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    opacity = r(N)
    rows, placed = [], {}
    for name, oo, dd, dep in PLACED_RAYS:
        placed[name] = len(rows)
        rows.append(dict(mask=1.0, depth=dep, o=oo, d=dd))
    for m in (1.0, 0.0):
        rows += [dict(mask=m, opacity=v) for v in OPACITY_EDGES]
    rows += [dict(mask=v) for v in MASK_EDGES]
    rows += [dict(mask=1.0, depth=v, o=(0.1, 0.2, -0.5)) for v in DEPTH_EDGES]        # inside the sphere: depth > 0 alone decides
    assert len(rows) == RENDER_EDGE_RAYS
    arrays = dict(mask=mask, depth=depth, o=o, d=d, opacity=opacity)
    for i, row in enumerate(rows[:N]):
        for k, v in row.items():
            arrays[k][i] = np.array(v, np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return dict(N=N, pred_rgb=t(r(N, 3)), pred_depth=t(r(N) * 2.0), opacity=t(opacity), image=t(r(3, N)), depth=t(depth), mask=t(mask),
                bg=t(r(N, 3)), o=t(o), d=t(d), placed={k: v for k, v in placed.items() if v < N}, name=f"N={N}")


def radius32(o, d, t):
    """|o + t d| in fp32 with the kernels' operation order: x = o + t d component by component, every product and sum rounded on
    its own (csrc/losses.hip is built with -ffp-contract=off), then sqrtf((x x + y y) + z z)"""
    assert o.dtype == d.dtype == t.dtype == F32
    p = o + t[..., None] * d
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return torch.sqrt(x * x + y * y + z * z)


def render_valid32(case, wrong=None):
    """depth > 0 and |o + depth d| <= 1.1f and mask > 0.5, as 0 / 1, decided on the fp32 data"""
    rad = radius32(case["o"], case["d"], case["depth"])
    inside = (rad < _t32(RADIUS)) if wrong == "valid_lt" else (rad <= _t32(RADIUS))
    return ((case["depth"] > 0) & inside & (case["mask"] > 0.5)).float()


def render_near_radius(case):
    """rays whose float64 radius lies within one fp32 ulp of 1.1f: there alone the comparison may fall either way"""
    p = case["o"].double() + case["depth"].double()[:, None] * case["d"].double()
    return (p.norm(dim=-1) - RADIUS).abs() <= 2.0 ** -23 * (1.0 + 1e-9)


def render_depth(N, which):
    """the longest chain of roundings behind a term of render_loss_kernel: per lane ceil(N / 1024) trips (three adds a trip for
    rgb), 6 shuffle adds, 16 wave adds, the roundings of one term, the denominator and the division; the weighted loss: the longest
    of them, three products and two adds.  Term roundings: rgb: the difference and its square (the 0 / 1 blend is exact);
    mask: logf (2), 1 - p (an absolute U / 2 under the log: the mean term is of order 1), the add of the two branches; depth: the
    difference and its square (the products with valid are exact)."""
    trips = max(ceil_div(N, RENDER_THREADS), 1)
    each = dict(rgb=3 * trips + 22 + 2 + 2, mask=trips + 22 + 4 + 1, depth=trips + 22 + 2 + 1)
    return max(each.values()) + 5 if which == "loss" else each[which]


def render_run(case, weights, dtype, wrong=None):
    """gt = image m + bg (1 - m), m = mask > 0.5;  rgb = mean (pred_rgb - gt)^2;  mask = F.binary_cross_entropy(clip(opacity), m);
    depth = mean (valid pred_depth - valid depth)^2;  loss = their weighted sum.  Means of an empty batch are 0.
    -> dict(loss, terms [3], gt_rgb [3, N], valid [N], grads=(g_rgb, g_depth, g_opacity)) for the gradient RENDER_G on the loss"""
    N = case["N"]
    leaves = [case[k].to(dtype).clone().requires_grad_(True) for k in ("pred_rgb", "pred_depth", "opacity")]
    pr, pd, op = leaves
    m = (case["mask"] > 0.5).to(dtype)
    gt = case["image"].to(dtype) * m[None] + case["bg"].to(dtype).t() * (1 - m[None])
    valid = render_valid32(case, wrong).to(dtype)
    n = max(N, 1)
    rgb = ((pr.t() - gt) ** 2).sum() / (3 * n)
    bce = Fn.binary_cross_entropy(op.clip(LO, HI), m, reduction="sum") / n
    dep = ((pd * valid - case["depth"].to(dtype) * valid) ** 2).sum() / n
    loss = weights[0] * rgb + weights[1] * bce + weights[2] * dep
    grads = torch.autograd.grad(loss * RENDER_G, leaves, allow_unused=True)
    grads = tuple(torch.zeros_like(l) if g is None else g for g, l in zip(grads, leaves))
    return dict(loss=loss.detach(), terms=torch.stack([rgb, bce, dep]).detach(), gt_rgb=gt, valid=valid, grads=grads)


def render_grad_scales(case, weights, r64):
    """g_rgb: |g| w_rgb 2 max|pred - gt| / 3 N;  g_depth: |g| w_depth 2 max|valid (pred - depth)| / N where valid, 0 elsewhere;
    g_opacity: |g| w_mask (m / p + (1 - m) / (1 - p)) / N, the element's own size, inside the clip, 0 outside"""
    N = max(case["N"], 1)
    g = abs(RENDER_G)
    pr, gt = case["pred_rgb"].double(), r64["gt_rgb"]
    s_rgb = torch.full_like(pr, g * weights[0] * 2.0 * float((pr.t() - gt).abs().max()) / (3 * N)) if case["N"] else pr
    v = r64["valid"]
    dd = ((case["pred_depth"].double() - case["depth"].double()) * v).abs()
    s_dep = v * (g * weights[2] * 2.0 * float(dd.max()) / N) if case["N"] else v
    op, m = case["opacity"].double(), (case["mask"] > 0.5).double()
    p = op.clamp(LO, HI)
    s_op = g * weights[1] * (m / p + (1 - m) / (1 - p)) / N * ((op >= LO) & (op <= HI))
    return s_rgb, s_dep, s_op


def render_check(case, weights, got, r32, r64, what):
    """got: dict(loss, terms, gt_rgb, valid, grads).  gt_rgb bit for bit; valid equal except at the rays within an ulp of the radius;
    the loss and its terms as means (scale: the mean of the absolute terms -- every term is positive); the gradients at FACTOR,
    floor 4 U, exactly 0 outside the clip and where valid = 0."""
    N = case["N"]
    what = f"{case['name']} {what}"
    assert same_bits(got["gt_rgb"], r32["gt_rgb"]), f"render {what}: gt_rgb differs from the operator chain"
    near = render_near_radius(case)
    v = got["valid"].detach().cpu()
    assert bool((v[~near] == r32["valid"][~near]).all()), f"render {what}: valid differs away from the radius"
    assert bool(((v == 0) | (v == 1)).all())
    recs = []
    if got["loss"] is not None:
        scale = float((torch.tensor(weights, dtype=F64) * r64["terms"]).sum())
        recs.append(judge(got["loss"], r32["loss"], r64["loss"], scale, f"render {what}: loss", floor=render_depth(N, "loss") * U))
        for k, name in enumerate(("rgb", "mask", "depth")):
            recs.append(judge(got["terms"][k], r32["terms"][k], r64["terms"][k], float(r64["terms"][k]), f"render {what}: {name} term",
                              floor=render_depth(N, name) * U))
    if got["grads"] is not None and N:
        same_valid = bool((v == r32["valid"]).all())        # (a comparison fallen the other way moves g_depth of that ray)
        for name, h, c, r, s in zip(("g_rgb", "g_depth", "g_opacity"), got["grads"], r32["grads"], r64["grads"], render_grad_scales(case, weights, r64)):
            if h is None:
                continue
            if name == "g_depth" and not same_valid:
                at = torch.nonzero(v != r32["valid"]).reshape(-1).tolist()
                print(f"[losses-f64] render {what}: g_depth NOT judged: valid differs from the fp32 chain at rays {at} (within an ulp of the radius)")
                report(REPORT, dict(what=f"render {what}: g_depth", skipped=True, valid_differs_at=at))
                continue
            recs.append(judge(h.reshape(r.shape), c, r, s, f"render {what}: {name}"))
    return recs


# ========================================================================================================= smooth points
SMOOTH_NK = ((1, 1), (1, 11), (255, 11), (256, 1), (257, 3), (2048, 11))


def smooth_case(N, K, seed=9):
    rng = np.random.RandomState(seed + N + K)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    off = np.linspace(-0.05, 0.05, K) + 0.01 * rng.rand(K)
    return dict(N=N, K=K, depth=t(rng.rand(1, N) * 2.0 + 0.2), off=t(off), o=t(rng.randn(N, 3) * 0.1 + np.array([0.0, 0.0, 1.5])),
                d=t(rng.randn(N, 3) * 0.5), g=t(rng.randn(K * N, 3)), name=f"N={N} K={K}")


def smooth_run(case, dtype):
    """pts[k N + n] = (depth[n] + off[k]) d[n] + o[n];  keep = |pts| < 1.1f decided on the fp32 points;  the gradients of <pts, g>
    -> dict(pts, keep, grads=(g_depth [1, N], g_o, g_d))"""
    leaves = [case[k].to(dtype).clone().requires_grad_(True) for k in ("depth", "o", "d")]
    depth, o, d = leaves
    pts = ((depth + case["off"].to(dtype)[:, None])[..., None] * d[None] + o[None]).view(-1, 3)
    t32 = (case["depth"] + case["off"][:, None]).reshape(-1)
    keep = (radius32(case["o"].repeat(case["K"], 1), case["d"].repeat(case["K"], 1), t32) < _t32(RADIUS)).float()
    return dict(pts=pts.detach(), keep=keep, grads=torch.autograd.grad(pts, leaves, case["g"].to(dtype)))


def smooth_near_radius(case, r64):
    return (r64["pts"].norm(dim=-1) - 1.1).abs() < 1e-6


def smooth_grad_scales(case):
    """the absolute sums over k: g_depth  sum_k sum_c |g d|;  g_o  sum_k |g|;  g_d  sum_k |g (depth + off_k)|"""
    N, K = case["N"], case["K"]
    g = case["g"].double().abs().view(K, N, 3)
    t = (case["depth"].double() + case["off"].double()[:, None]).abs()                  # [K, N]
    return (g * case["d"].double().abs()[None]).sum((0, 2)).view(1, N), g.sum(0), (g * t[..., None]).sum(0)


def smooth_check(case, got, r32, r64, what=None):
    """got: dict(pts, keep, grads).  Points bit for bit the operator chain; keep equal away from the radius; gradients against
    float64 at the absolute-sum scale, floor (K + 3) U"""
    what = what or case["name"]
    assert same_bits(got["pts"], r32["pts"]), f"smooth {what}: points differ from the operator chain"
    near = smooth_near_radius(case, r64)
    assert torch.equal(got["keep"].detach().cpu()[~near], r32["keep"][~near]), f"smooth {what}: keep differs away from the radius"
    return [judge(h, c, r, s, f"smooth {what}: {name}", floor=(case["K"] + 3) * U)
            for name, h, c, r, s in zip(("g_depth", "g_o", "g_d"), got["grads"], r32["grads"], r64["grads"], smooth_grad_scales(case))]


# ============================================================================================================== bg blend
BLEND_N = (1, 255, 256, 257, 5000)


def blend_case(N, seed=10):
    rng = np.random.RandomState(seed + N)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    opacity = rng.rand(N, 1)
    opacity[0::5] = 0.0
    opacity[N // 2::7] = 1.0
    return dict(N=N, color=t(rng.rand(N, 3)), opacity=t(opacity), bg=t(rng.rand(N, 3)), g=t(rng.randn(N, 3)), name=f"N={N}")


def blend_run(case, dtype):
    """image = color + (1 - opacity) bg -> dict(image, grads=(g_color, g_opacity [N, 1], g_bg))"""
    leaves = [case[k].to(dtype).clone().requires_grad_(True) for k in ("color", "opacity", "bg")]
    color, opacity, bg = leaves
    image = color + (1 - opacity) * bg
    return dict(image=image.detach(), grads=torch.autograd.grad(image, leaves, case["g"].to(dtype)))


def blend_check(case, got, r32, r64, what=None):
    """image, g_color and g_bg bit for bit the operator chain; g_opacity against float64, scale sum_c |g_c bg_c|, floor 3 U"""
    what = what or case["name"]
    assert same_bits(got["image"], r32["image"]), f"blend {what}: image differs from the operator chain"
    assert same_bits(got["grads"][0], case["g"]), f"blend {what}: g_color is not g"
    if got["grads"][2] is not None:
        assert same_bits(got["grads"][2], r32["grads"][2]), f"blend {what}: g_bg differs from the operator chain"
    scale = (case["g"].double() * case["bg"].double()).abs().sum(-1, keepdim=True)
    return [judge(got["grads"][1], r32["grads"][1], r64["grads"][1], scale, f"blend {what}: g_opacity", floor=3 * U)]
