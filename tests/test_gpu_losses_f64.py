"""csrc/losses.hip against float64 at every loop, launch and branch edge (tests/losses_f64_oracle.py holds the yardsticks, the fp32
restatements, the cases and the judgement of one call; tests/test_losses_oracle_host.py shows on the CPU that the cases reach what
they name and that wrong restatements fail).

The rule, not fitted to a run (losses_f64_oracle.judge): errors are |x - float64| over the quantity's natural scale, written beside
each check in the oracle; a kernel's worst error must stay within 2 x the worst error of the fp32 restatement on the same inputs, or
a floor where the restatement happens to be exact: 4 roundings of the scale for elementwise quantities, the kernel's own longest
chain of roundings (derived from the header's constants: mean_depth, render_depth, pose_count) for sums.  Elements of zero scale
are exact.  Every check uses the factor 2.  Every judged check prints its figures and appends them to the JSON-lines file that
MORPHEUS_LOSSES_REPORT names.

Worst figures of one run on an MI355X (error / scale; worst over the module's checks of the quantity; the restatement's figure and the
ratio are those of the check that holds the kernel's worst).  No factor is raised above 2; where a ratio is above 2 the kernel's
figure is under the check's floor, which is named.

    quantity                      scale                                   kernel     fp32 restatement   ratio
    mean value, identity          sum |f w| / den                         1.22e-08   3.35e-09           3.65   (floor 45 U, weighted M = 257)
    mean value, square            "                                       1.03e-07   1.48e-08           7.00   (floor 24 U)
    mean value, abs               "                                       1.16e-07   7.09e-09           16.4   (floor 45 U)
    mean value, entropy           "                                       1.09e-04   1.08e-04           1.00   (M = 1: the one element is the lower clamp bound)
    mean value, absdiff           "                                       1.17e-07   1.50e-08           7.84   (floor 48 U)
    mean value, sqdiff            "                                       1.90e-07   4.09e-09           46.5   (floor 49 U: 3.2 U of it used)
    mean value, eikonal           "                                       1.37e-07   3.68e-08           3.71   (floor 53 U)
    mean gradient, identity       |g| max|f'| w / den                     1.39e-07   6.96e-08           1.99
    mean gradient, square         "                                       1.20e-07   1.20e-07           1.00
    mean gradient, abs            "                                       1.39e-07   6.96e-08           1.99
    mean gradient, entropy        "                                       2.05e-07   2.29e-07           0.90
    mean gradient, absdiff        "                                       2.19e-07   8.13e-08           2.70   (floor 4 U = 2.38e-07)
    mean gradient, sqdiff         "                                       1.71e-07   1.16e-07           1.48
    mean gradient, eikonal        "                                       1.28e-07   6.14e-08           2.09   (floor 4 U)
    ortho output, displacement    |scale|                                 2.97e-05   2.97e-05           1.00   (the rounding of x + w at scale 0.004)
    ortho displacement at x = 0   |scale|                                 1.83e-07   1.48e-07           1.24
    ortho g_n, call by call       the row's largest |g_n|                 1.11e-06   6.30e-07           1.76
    ortho g_n, all sizes pooled   "                                       1.11e-06   1.08e-06           1.03
    pose o'                       |o| + |t|                               5.96e-08   5.96e-08           1.00
    pose d'                       sum_c |R_rc d_c|                        4.03e-07   1.36e-07           2.95   (floor 12 U x the call's cancellation of R, at most 4)
    pose d'                       sum_c Rabs_rc |d_c| (abs. monomials)    2.16e-07   1.52e-07           1.42   (floor 12 U)
    pose gradient                 (judge_sum) abs sum x count x U         1.42e-05 absolute: 0.002 x the bound
    render loss                   sum_k w_k term_k                        1.35e-07   2.10e-08           6.43   (floor 40 U)
    render rgb / mask / depth     the term                                1.32e-07   4.12e-08           3.20   (floors 29 U, 30 U, 26 U)
    render g_rgb                  |g| w 2 max|pred - gt| / 3 N            1.14e-07   8.19e-08           1.39
    render g_depth                |g| w 2 max|valid (pred - depth)| / N   1.24e-07   1.18e-07           1.06
    render g_opacity              the element's own size                  1.74e-07   1.40e-07           1.24
    smooth g_depth, g_o, g_d      the absolute sums over k                1.65e-07   1.65e-07           1.00
    blend g_opacity               sum_c |g_c bg_c|                        1.25e-07   1.25e-07           1.00
The launch's o' and d' had the bits of the fp32 operator chain on the device in all 50 (n, frames) cases (recorded, not asserted).
The weighted mean's gradient carries the rounding of the fp32 sum of the weights in every element: absdiff at M = 2049 reads 3.7 U
against the floor of 4 U.

What the checks found, and the wrapper fix: ops.masked_mean took C as numel // max(M, 1), which is 1 for an empty [0, 3] tensor, so
masked_mean("eikonal", empty) was refused with the argument error (eikonal needs C = 3) where the project's rule is that an empty
selection gives 0; and an empty gradient tensor has no address, so mh_masked_mean_bwd took g_a = g_b = NULL and refused backward
on an empty tensor of every kind.  C now comes from the trailing shape, and backward launches nothing for an empty tensor
(test_masked_mean_of_empty_tensors).  No kernel missed its rule.
Two of the module's own first choices were wrong and are corrected with their reasons in the oracle: a floor of 4 U for d' (the
entries of R that are differences of monomials cost their monomials' roundings: 3.6e-07 to 4.0e-07 against restatements at 1.3e-07
to 2.2e-07, once per frame, not per ray -- pose_forward_floor), and an unbounded condition number of the rows of g_n (one row of 1025
read 8.7e-06 against 3.7e-06 -- ortho_condition).
Limits of the cases, by construction and asserted by the host test: the gradient entering ortho perturb is redrawn in the rows
(about one random row in eight) whose backward projections cancel more than 8-fold, so g_n never meets a strongly cancelling
backward; the pose angles are redrawn while an entry of R is a difference smaller than a quarter of its monomials' absolute sum,
so the floor of d' at the issue's scale stays within 48 U.  The count of 12 behind d' is derived (three sin / cos of up to one ulp
= 2 U each, the monomial's two products, the add of two monomials, the product with d_c, two adds) and is not lowered to what
this run would have passed.
"""
import pytest
import torch

from tests import losses_f64_oracle as L
from tests.f64_judge import report

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


def _dev(t, grad=False):
    return None if t is None else t.to(DEV).requires_grad_(grad)


_REF = {}


def _ref(key, build, run):
    """the case, its float64 run and its fp32 restatement: computed once, shared, never modified"""
    if key not in _REF:
        case = build()
        _REF[key] = (case, run(case, F64), run(case, F32))
    return _REF[key]


# =========================================================================================================== masked mean
def _mean_gpu(case):
    from morpheus_amd import ops
    a, b = _dev(case["a"], True), _dev(case["b"], True)
    nv = None if case["n_valid"] is None else torch.tensor(case["n_valid"], dtype=torch.int32, device=DEV)
    got = ops.masked_mean(case["kind"], a, b, n_valid=nv, row_weight=_dev(case["w"]))
    (got * case["g"]).backward()
    return dict(value=got.detach(), ga=a.grad, gb=None if b is None else b.grad)


def test_mean_workspace_is_two_floats_per_block():
    from morpheus_amd import _lib
    assert _lib.load().mh_masked_mean_workspace_floats() == 2 * L.MEAN_BLOCKS


@pytest.mark.parametrize("kind,C", [(k, 1) for k in L.MEAN_KINDS if k != "eikonal"] + [(k, 3) for k in L.MEAN_C3_KINDS])
def test_masked_mean_sizes_modes_and_data_edges(kind, C):
    """C = 1: M = 1, 255, 256, 257, 1024, 1025, 2049, 524288, 524289 (one partial block, wave and block tails, the second block, the
    cap of 512 blocks, the first element of the fifth trip); C = 3: M = 1, 85, 86, 342, 174763 (rows straddling the edges); all rows,
    n_valid, row_weight and both; n_valid = 0, 1, M - 1, M, M + 5, -3 with NaN behind it in a, b and the weights; 0 / 1, non-integer,
    denominator-clamping and all-zero weights; the clamp bounds and their neighbours, exact zeros, a == b, a zero row."""
    for case in L.mean_cases(kind, C):
        r64, r32 = L.mean_run(case, F64), L.mean_run(case, F32)
        got = _mean_gpu(case)
        L.mean_check(case, got, r32, r64)
        if case["weights"] == "zero" or case["n_valid"] in (0, -3):
            assert float(got["value"]) == 0.0 and bool((got["ga"] == 0).all())


@pytest.mark.parametrize("kind", L.MEAN_KINDS)
def test_masked_mean_of_empty_tensors(kind):
    """M = 0 with the right trailing shape: the value is 0 and backward hands back empty gradients.  (With C taken as
    numel // max(M, 1) the wrapper sent C = 1 for an empty [0, 3] tensor and eikonal was refused with the argument error; an empty
    gradient's NULL address made backward of every kind an argument error.)"""
    from morpheus_amd import ops
    case = L.mean_empty_case(kind)
    a, b = _dev(case["a"], True), _dev(case["b"], True)
    for kw in ({}, dict(n_valid=torch.tensor(0, dtype=torch.int32, device=DEV)), dict(row_weight=torch.zeros(0, device=DEV))):
        got = ops.masked_mean(kind, a, b, **kw)
        assert float(got.detach()) == 0.0 == float(L.mean_run(case, F64)["value"])
        grads = torch.autograd.grad(got, [a] + ([b] if b is not None else []))
        assert all(g.shape == a.shape and g.numel() == 0 for g in grads)


def test_masked_mean_c_abi_forms_and_argument_errors():
    """g_b alone (g_a = NULL) against float64; g_a = g_b = NULL, a bad kind, C <= 0 and eikonal with C != 3 are argument errors that
    leave sentinel-filled ws, out and gradients untouched."""
    from morpheus_amd import _lib, ops
    n_ws = _lib.load().mh_masked_mean_workspace_floats()
    for kind, M, C in (("absdiff", 86, 3), ("sqdiff", 257, 1)):
        case, r64, r32 = _ref(("mean", kind, M, C), lambda: L.mean_case(kind, M, C), L.mean_run)
        a, b = case["a"].to(DEV), case["b"].to(DEV)
        ws, out = torch.full((n_ws,), SENTINEL, device=DEV), torch.full((2,), SENTINEL, device=DEV)
        k = ops.MEAN_KINDS[kind]
        assert _status("mh_masked_mean_fwd", k, _ptr(a), _ptr(b), None, M, C, None, _ptr(ws), _ptr(out)) == 0
        g = torch.tensor([case["g"]], device=DEV)
        g_b = torch.full_like(b, SENTINEL)
        assert _status("mh_masked_mean_bwd", k, _ptr(a), _ptr(b), None, M, C, None, _ptr(out), _ptr(g), None, _ptr(g_b)) == 0
        torch.cuda.synchronize()
        L.mean_check(case, dict(value=out[0], gb=g_b), r32, r64, what=f"{case['name']}, g_a = NULL")
        g_a = torch.full_like(a, SENTINEL)
        assert _status("mh_masked_mean_bwd", k, _ptr(a), _ptr(b), None, M, C, None, _ptr(out), _ptr(g), _ptr(g_a), None) == 0
        torch.cuda.synchronize()
        assert L.same_bits(g_a, -g_b), "g_b = -g_a"
        assert _status("mh_masked_mean_bwd", k, _ptr(a), _ptr(b), None, M, C, None, _ptr(out), _ptr(g), None, None) == MH_ERR_ARG
    a = torch.randn(64, 3, device=DEV)
    bad = [("kind -1", -1, 64, 3), ("kind 7", 7, 64, 3), ("C = 0", 2, 64, 0), ("C = -1", 2, 64, -1), ("eikonal, C = 1", 4, 64, 1),
           ("eikonal, C = 4", 4, 48, 4), ("eikonal, M = 0 and C = 1", 4, 0, 1)]
    g = torch.ones(1, device=DEV)
    for what, kind, M, C in bad:
        ws, out, g_a = torch.full((n_ws,), SENTINEL, device=DEV), torch.full((2,), SENTINEL, device=DEV), torch.full((64, 3), SENTINEL, device=DEV)
        assert _status("mh_masked_mean_fwd", kind, _ptr(a), _ptr(a), None, M, C, None, _ptr(ws), _ptr(out)) == MH_ERR_ARG, what
        assert _status("mh_masked_mean_bwd", kind, _ptr(a), _ptr(a), None, M, C, None, _ptr(out), _ptr(g), _ptr(g_a), None) == MH_ERR_ARG, what
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in (ws, out, g_a)), what


# ========================================================================================================= ortho perturb
@pytest.mark.parametrize("scale", L.ORTHO_SCALES)
def test_ortho_perturb_every_normal_and_tail(scale):
    """M = 1, 63, 64, 255, 256, 257, 1025; scale 0.004 and 1; normals random at lengths 1e-3 .. 1e3, (0, 0, +-1), (0, 0, 5) (u = 0),
    (1e-7, 0, 1), zero, of length 1e-13, axis-aligned; phi 0, pi/2, pi, 2 pi and random.  Output, displacement and g_n are judged call
    by call; g_n row by row, the degenerate rows (both else-branches of ortho_perturb_bwd_kernel) included.  The rows of all seven
    sizes are judged once more together, for the table's figure."""
    from morpheus_amd import ops
    pool = []
    for M in L.ORTHO_M:
        case = L.ortho_case(M)
        r64, r32 = L.ortho_run(case, scale, F64), L.ortho_run(case, scale, F32)
        x, n = _dev(case["x"], True), _dev(case["n"], True)
        out = ops.ortho_perturb(x, n, case["phi"].to(DEV), scale)
        out.backward(case["g"].to(DEV))
        L.ortho_check(case, scale, dict(out=out, gn=n.grad, gx=x.grad), r32, r64, f"M={M} scale={scale}", pool=pool)
    L.ortho_judge_pool(pool, f"all sizes, scale={scale}")


# ============================================================================================================ pose apply
def _chain_bits_match(case, o1, d1):
    """whether the launch gives the bits of the fp32 operator chain on this device (recorded, not asserted: the order in which
    the chain adds three products is the library's choice for a shape, not a definition)"""
    from morpheus_amd.model import PoseArray
    B, n = case["B"], case["n"]
    pa = PoseArray(L.POSE_F).to(DEV)
    with torch.no_grad():
        pa.data.copy_(case["pose"].to(DEV))
        ids = torch.tensor(case["frames"], device=DEV)
        R32, t32 = pa.get_rotation_matrices(ids), pa.get_translations(ids)
        o, d = case["o"].to(DEV), case["d"].to(DEV)
        return (torch.equal(o1, (o.view(B, n, 3) + t32[:, None]).view(-1, 3)),
                torch.equal(d1, (d.view(B, n, 1, 3) * R32[:, None]).sum(-1).view(-1, 3)))


@pytest.mark.parametrize("frames", L.POSE_FRAMES, ids=str)
def test_pose_apply_rows_frames_and_gradient_subsets(frames):
    """n_per_row = 1, 63, 64, 255, 256, 257, 1023, 1024, 1025, 2049 (below a wave, around POSE_RAYS_PER_BLOCK, three blocks a row);
    frames [4], [4, 7], [4, 7, 4], [4, 7, 4, 7], [2, 2, 2] of 9 (non-adjacent and adjacent rows of one frame); angles up to +-3,
    frame 7 all zero; the gradient of both outputs, of o' alone and of d' alone; rows of frames outside the batch exactly 0."""
    from morpheus_amd import ops
    for n in L.POSE_N:
        case, r64, r32 = _ref(("pose", n, tuple(frames)), lambda: L.pose_case(n, frames), L.pose_run)
        pose = _dev(case["pose"], True)
        o1, d1 = ops.pose_apply(case["o"].to(DEV), case["d"].to(DEV), pose, torch.tensor(frames, device=DEV), n)
        L.pose_check_forward(case, o1, d1, r32, r64)
        om, dm = _chain_bits_match(case, o1.detach(), d1.detach())
        report(L.REPORT, dict(what=f"pose {case['name']}: bits of the fp32 operator chain", o_match=om, d_match=dm))
        print(f"[losses-f64] pose {case['name']}: bits of the fp32 operator chain on this device: o' {om}, d' {dm}")
        go, gd = case["go"].to(DEV), case["gd"].to(DEV)
        (both,) = torch.autograd.grad([o1, d1], pose, [go, gd], retain_graph=True)
        (o_only,) = torch.autograd.grad(o1, pose, go, retain_graph=True)
        (d_only,) = torch.autograd.grad(d1, pose, gd)
        for mode, g in (("both", both), ("o", o_only), ("d", d_only)):
            L.pose_check_grad(case, mode, g, r32, r64)


def test_pose_gradient_overwrites_what_the_buffer_held():
    """mh_pose_apply_bwd on a sentinel-filled g_pose: every element is written, frames outside the batch with 0"""
    from morpheus_amd import _lib, ops
    n, frames = 257, [4, 7, 4]
    case, r64, r32 = _ref(("pose", n, tuple(frames)), lambda: L.pose_case(n, frames), L.pose_run)
    pose = _dev(case["pose"], True)
    ids = torch.tensor(frames, device=DEV)
    d, go, gd = case["d"].to(DEV), case["go"].to(DEV), case["gd"].to(DEV)
    o1, d1 = ops.pose_apply(case["o"].to(DEV), d, pose, ids, n)
    (want,) = torch.autograd.grad([o1, d1], pose, [go, gd])
    ws = torch.empty(_lib.load().mh_pose_bwd_workspace_floats(len(frames), n), device=DEV)
    g_pose = torch.full((L.POSE_F, 6), SENTINEL, device=DEV)
    p = pose.detach()
    assert _status("mh_pose_apply_bwd", _ptr(d), _ptr(p), _ptr(ids), len(frames), n, L.POSE_F, _ptr(go), _ptr(gd), _ptr(ws), _ptr(g_pose)) == 0
    torch.cuda.synchronize()
    assert bool((g_pose != SENTINEL).all()) and L.same_bits(g_pose, want)
    assert bool((g_pose[[0, 1, 2, 3, 5, 6, 8]] == 0).all())


# =========================================================================================================== render loss
def _render_weights():
    from morpheus_amd import harness
    tr = harness.load_config()["train"]
    return dict(L.RENDER_WEIGHTS, config=(float(tr["rgb_weight"]), float(tr["mask_weight"]), float(tr["depth_weight"])))


def _render_gpu(case, w, need=(True, True, True)):
    from morpheus_amd import ops
    N = case["N"]
    pr, pd, op = (_dev(case[k], nd) for k, nd in zip(("pred_rgb", "pred_depth", "opacity"), need))
    got, terms, gt, valid = ops.real_view_render_loss(pr.view(1, N, 3), pd.view(1, N), op.view(1, N, 1), case["image"].to(DEV).view(1, 3, N, 1),
                                                      case["depth"].to(DEV).view(1, N, 1), case["mask"].to(DEV).view(1, N, 1), case["bg"].to(DEV),
                                                      case["o"].to(DEV).view(1, N, 3), case["d"].to(DEV).view(1, N, 3), *w)
    (got * L.RENDER_G).backward()
    return dict(loss=got.detach(), terms=terms, gt_rgb=gt, valid=valid, grads=(pr.grad, pd.grad, op.grad))


@pytest.mark.parametrize("N", L.RENDER_N)
def test_render_loss_sizes_edges_and_gradient_subsets(N):
    """N = 0, 1, 63, 64, 1023, 1024, 1025, 2049, 3000 (below a wave, below the block, one to three trips); masks 0, 0.5, the next
    float and 1; opacity at both clip bounds, their neighbours, 0 and 1, under either mask; depths 0, -0.1, 1e-30; rays placed on,
    one ulp under and one ulp over the radius 1.1f; weights (1, 1, 1), the config's and one without the mask term; each gradient
    wanted alone equals the run that wants all three bit for bit."""
    case = L.render_case(N)
    for name, w in _render_weights().items():
        r64, r32 = L.render_run(case, w, F64), L.render_run(case, w, F32)
        got = _render_gpu(case, w)
        L.render_check(case, w, got, r32, r64, name)
        if N == 0:
            assert float(got["loss"]) == 0.0 and bool((got["terms"] == 0).all())
            continue
        op = case["opacity"]
        assert bool((got["grads"][2].reshape(-1).cpu()[(op < L.LO) | (op > L.HI)] == 0).all()), "opacity outside the clip: no gradient"
        assert bool((got["grads"][1].reshape(-1)[got["valid"] == 0] == 0).all()), "no valid depth: no gradient"
        if name == "config":
            for k in range(3):
                alone = _render_gpu(case, w, tuple(i == k for i in range(3)))
                assert L.same_bits(alone["grads"][k], got["grads"][k]) and L.same_bits(alone["loss"], got["loss"])
                assert all(alone["grads"][i] is None for i in range(3) if i != k)


# ================================================================================================ smooth points, bg blend
@pytest.mark.parametrize("N,K", L.SMOOTH_NK)
def test_smooth_points_sizes_and_gradient_subsets(N, K):
    """(N, K) = (1, 1), (1, 11), (255, 11), (256, 1), (257, 3), (2048, 11); the points are the operator chain bit for bit; the
    gradients against float64; depth alone and depth with o equal the full run bit for bit"""
    from morpheus_amd import ops
    case = L.smooth_case(N, K)
    r64, r32 = L.smooth_run(case, F64), L.smooth_run(case, F32)
    off, g = case["off"].to(DEV), case["g"].to(DEV)
    depth, o, d = (_dev(case[k], True) for k in ("depth", "o", "d"))
    pts, keep = ops.smooth_points(depth, off, o, d)
    full = torch.autograd.grad(pts, [depth, o, d], g)
    L.smooth_check(case, dict(pts=pts, keep=keep, grads=full), r32, r64)
    pts1, _ = ops.smooth_points(depth, off, o.detach(), d.detach())
    (g1,) = torch.autograd.grad(pts1, [depth], g)
    pts2, _ = ops.smooth_points(depth, off, o, d.detach())
    g2 = torch.autograd.grad(pts2, [depth, o], g)
    assert L.same_bits(g1, full[0]) and L.same_bits(g2[0], full[0]) and L.same_bits(g2[1], full[1])
    assert L.same_bits(pts1, pts) and L.same_bits(pts2, pts)


@pytest.mark.parametrize("N", L.BLEND_N)
def test_bg_blend_sizes_and_a_detached_background(N):
    """N = 1, 255, 256, 257, 5000; opacity exactly 0 and exactly 1 among the rays; image, g_color and g_bg bit for bit the chain,
    g_opacity against float64; a background without a gradient gives the same bits"""
    from morpheus_amd import ops
    case = L.blend_case(N)
    r64, r32 = L.blend_run(case, F64), L.blend_run(case, F32)
    color, opacity, bg = (_dev(case[k], True) for k in ("color", "opacity", "bg"))
    g = case["g"].to(DEV)
    out = ops.bg_blend(color, opacity, bg)
    full = torch.autograd.grad(out, [color, opacity, bg], g)
    L.blend_check(case, dict(image=out, grads=full), r32, r64)
    out2 = ops.bg_blend(color, opacity, bg.detach())
    g2 = torch.autograd.grad(out2, [color, opacity], g)
    assert L.same_bits(out2, out) and L.same_bits(g2[0], full[0]) and L.same_bits(g2[1], full[1])


# ========================================================================================================== weighted sum
def test_weighted_sum_after_the_weight_cache_is_evicted():
    """65 distinct weight tuples clear the cache of 64; the first tuple then still gives its own value and gradients"""
    from morpheus_amd import ops
    vals = (0.3, -1.2, 4.0, 0.07)

    def run(ws):
        ts = [torch.tensor(v, device=DEV, requires_grad=True) for v in vals]
        got = ops.weighted_sum(list(zip(ws, ts)))
        (got * 2.0).backward()
        return float(got), [float(t.grad) for t in ts]

    tuples = [(1.0, 0.5, 0.01, 30.0 + k) for k in range(65)]
    first = run(tuples[0])
    for ws in tuples[1:]:
        run(ws)
    assert len(ops._WEIGHT_CACHE) <= 64
    for ws in (tuples[0], tuples[64], tuples[1]):
        value, grads = run(ws)
        want = sum(float(torch.tensor(w, dtype=F32)) * v for w, v in zip(ws, [float(torch.tensor(v, dtype=F32)) for v in vals]))
        scale = sum(abs(w * v) for w, v in zip(ws, vals))
        assert abs(value - want) <= 8 * L.U * scale, (ws, value, want)
        assert grads == [float(torch.tensor(2.0 * w, dtype=F32)) for w in ws], (ws, grads)
    assert run(tuples[0]) == first
