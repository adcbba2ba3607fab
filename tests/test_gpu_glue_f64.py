"""csrc/normal.hip against float64 at every loop trip and branch (tests/glue_f64_oracle.py holds the yardstick and the cases;
tests/test_glue_oracle_host.py shows on the CPU that the cases reach what they name).

Rules, none of them fitted to a run:
  * bit for bit (torch.equal with the fp32 torch chain on the same device): taps, topo6, xyz; exact zeros on empty rays, on
    padding and where every tap of an axis is clamped;
  * pure sums (segment sums, tap sums, loss totals): rounding count x 2^-24 x the float64 sum of the ABSOLUTE terms, the count
    written beside the assertion (glue_f64_oracle.judge_sum);
  * everything with a division, sqrt, expf or the lerp: the fp32 torch chain on the same device, measured against float64, is
    the measure -- worst HIP element within 3 x the chain's worst, at most 3 x (+ 2) as many elements above the chain's own
    99.9th percentile (glue_f64_oracle.judge).
Every test appends {kernel, case, worst_hip, worst_chain, ratio, n_above} to the JSON-lines file that the environment variable
MORPHEUS_GLUE_REPORT names (nothing is written without it); profiles/r07_glue_f64_report.jsonl is the committed copy of one run."""
import pytest
import torch

from tests import glue_f64_oracle as G
from tests.f64_judge import report

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64


def _report(kernel, case, rec):
    report("MORPHEUS_GLUE_REPORT", dict(kernel=kernel, case=case, **rec))


def _dev(t, dtype=None):
    if t is None:
        return None
    t = t.to(DEV)
    return t if dtype is None or not t.is_floating_point() else t.to(dtype)


def _leaf(t, dtype=F32):
    return _dev(t, dtype).clone().requires_grad_(True)


# ----------------------------------------------------------------------------------------------------- sample positions
def test_sample_positions_every_trip_count():
    """mh_sample_positions / _bwd at 13 rays of 0, 1, 63, 64, 65, 0, 127, 128, 129, 200, 2, 64, 0 samples: one to four trips of
    the wave's i += 64 loop, full and ragged last trips, an empty ray first and last, a block with three idle waves."""
    from morpheus_amd import ops
    c = G.positions_case()
    ri, ts, te, g = _dev(c["ri"]), _dev(c["ts"]), _dev(c["te"]), _dev(c["g"])
    oa, da = _leaf(c["o"]), _leaf(c["d"])
    xyz_t = G.positions(oa, da, ri, ts, te)
    ob, db = _leaf(c["o"]), _leaf(c["d"])
    xyz_h = ops.sample_positions(ob, db, ri, ts, te, _dev(c["start"]), _dev(c["cnt"]))
    assert torch.equal(xyz_h, xyz_t)
    (xyz_h * g).sum().backward()
    o64, d64 = _leaf(c["o"], F64), _leaf(c["d"], F64)
    (G.positions(o64, d64, ri, ts.double(), te.double()) * g.double()).sum().backward()
    # the absolute terms: |g| for d/d o, |g tm| for d/d d, per ray and axis
    idx = ri.long()[:, None].expand(-1, 3)
    tm = ((ts.double() + te.double()) / 2)[:, None]
    abs_o = torch.zeros(c["N"], 3, dtype=F64, device=DEV).scatter_add(0, idx, g.double().abs())
    abs_d = torch.zeros(c["N"], 3, dtype=F64, device=DEV).scatter_add(0, idx, (g.double() * tm).abs())
    # roundings of one term: ceil(n / 64) adds in its lane + 6 shuffle steps; + 1 for the product g * tm in d/d d
    trips = ((c["cnt"].double() + 63) // 64)[:, None].expand(-1, 3)
    for name, got, want, a, extra in (("d/d rays_o", ob.grad, o64.grad, abs_o, 0), ("d/d rays_d", db.grad, d64.grad, abs_d, 1)):
        for t in sorted(set(trips[:, 0].tolist())):
            rows = _dev(trips[:, 0] == t)
            rec = G.judge_sum(got[rows], want[rows], a[rows], int(t) + 6 + extra, f"{name}, {int(t)} trips")
            _report("sample_positions_bwd", f"{name}, {int(t)} trips", rec)
    empty = _dev(c["cnt"]) == 0
    assert int(empty.sum()) == 3
    assert bool((ob.grad[empty] == 0).all()) and bool((db.grad[empty] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- taps
@pytest.mark.parametrize("eps", G.EPS_CASES)
@pytest.mark.parametrize("C", [None, 1, 2, 5])
def test_fd_taps_clamp_edges_and_block_edges(C, eps):
    """mh_fd_taps / _bwd: M on both sides of a forward block (6 x 42 = 252, 6 x 43 = 258 taps) and of a backward block (255,
    256, 257); points exactly on +-bound, points whose +-eps tap lands exactly on +-bound, their fp32 neighbours; points
    beyond bound + eps.  Forward bit for bit; backward against float64 with the clamp masks of the fp32 sums."""
    from morpheus_amd import ops
    for M in (1, 42, 43, 255, 256, 257):
        c = G.taps_case(M, C, eps)
        bound = c["bound"]
        g_taps, g_topo6 = _dev(c["g_taps"]), _dev(c["g_topo6"])
        inside = G.taps_decisions(_dev(c["x"]), eps, bound)

        def loss(taps, topo6, dtype):
            s = (taps * g_taps.to(dtype)).sum()
            return s if topo6 is None else s + (topo6 * g_topo6.to(dtype)).sum()

        xa, ta = _leaf(c["x"]), (None if C is None else _leaf(c["topo"]))
        taps_t, topo_t = G.taps(xa, ta, eps, bound)
        x64, t64 = _leaf(c["x"], F64), (None if C is None else _leaf(c["topo"], F64))
        loss(*G.taps(x64, t64, eps, bound, inside), F64).backward()
        abs_x = (g_taps.double().abs().view(M, 6, 3) * inside).sum(1)
        abs_t = None if C is None else g_topo6.double().abs().view(M, 6, C).sum(1)
        combos = [(True, True), (True, False), (False, True)] if C is not None else [(True, False)]
        for need_x, need_t in combos:
            xb = _leaf(c["x"]) if need_x else _dev(c["x"])
            tb = None if C is None else (_leaf(c["topo"]) if need_t else _dev(c["topo"]))
            taps_h, topo_h = ops.fd_taps(xb, tb, eps, bound)
            assert torch.equal(taps_h, taps_t), (M, C)
            assert (topo_h is None) if C is None else torch.equal(topo_h, topo_t)
            assert taps_h.requires_grad == need_x, "taps of positions without gradient are non-differentiable"
            if C is not None:
                assert topo_h.requires_grad == need_t
            terms = [(taps_h * g_taps).sum()] if need_x else []
            terms += [(topo_h * g_topo6).sum()] if need_t else []
            sum(terms).backward()
            case = f"M={M} C={C} eps={eps} x={need_x} topo={need_t}"
            if need_x:      # six adds per component
                _report("fd_taps_bwd", case + " d/dx", G.judge_sum(xb.grad, x64.grad, abs_x, 6, "d taps / dx " + case))
                assert bool((xb.grad[abs_x == 0] == 0).all())
                dead = ~inside.any(1)                                  # all six taps of the axis clamped
                assert M < 42 or int(dead.sum()) >= 6
                assert bool((xb.grad[dead] == 0).all())
            else:
                assert xb.grad is None
            if need_t:
                _report("fd_taps_bwd", case + " d/dtopo", G.judge_sum(tb.grad, t64.grad, abs_t, 6, "d topo6 / d topo " + case))
            elif tb is not None:
                assert tb.grad is None
        taps_n, topo_n = ops.fd_taps(_dev(c["x"]), _dev(c["topo"]), eps, bound)      # no gradient anywhere
        assert not taps_n.requires_grad and torch.equal(taps_n, taps_t) and (C is None or not topo_n.requires_grad)


# -------------------------------------------------------------------------------------------------------------- normal
@pytest.mark.parametrize("eps", G.EPS_CASES)
@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_fd_normal_across_the_length_clamp(M, eps):
    """mh_fd_normal_fwd / _bwd on exactly flat rows, rows with |raw|^2 = 1e-20 x {1/16, 1/4, 4, 16}, ordinary rows and rows with
    |raw| ~ 1e3; g_normal only, g_raw only, both.  Gradient errors are normalised PER ROW by the row's own scale
    (|g_normal| / len + |g_raw|) / eps, so a near-flat row is not judged by an ordinary row's magnitude."""
    from morpheus_amd import ops
    c = G.normal_case(M, eps)
    s6, g_n, g_r = _dev(c["s6"]), _dev(c["g_n"]), _dev(c["g_r"])
    clamped = G.normal_decisions(s6, eps)
    for use_n, use_r in ((True, True), (True, False), (False, True)):
        def loss(n, r, dtype):
            return sum(([(n * g_n.to(dtype)).sum()] if use_n else []) + ([(r * g_r.to(dtype)).sum()] if use_r else []))

        sa, sb, s64 = _leaf(c["s6"]), _leaf(c["s6"]), _leaf(c["s6"], F64)
        n_t, r_t = G.normal(sa, eps)
        n_h, r_h = ops.fd_normal(sb, eps)
        n_64, r_64 = G.normal(s64, eps, clamped)
        for out, l in (((n_t, r_t), F32), ((n_h, r_h), F32), ((n_64, r_64), F64)):
            loss(*out, l).backward()
        case = f"M={M} eps={eps} g_normal={use_n} g_raw={use_r}"
        length = torch.sqrt(torch.where(clamped[:, None], torch.full_like(r_64[:, :1], G.f32_scalar(1e-20)), (r_64 * r_64).sum(-1, keepdim=True))).detach()
        # raw: subtraction, halving (exact), division -> 3 roundings of its own magnitude;  normal: + squares, sum, sqrt, division
        _report("fd_normal_fwd", case + " raw", G.judge(r_h, r_t, r_64, r_64.detach().abs(), 3, "raw " + case))
        _report("fd_normal_fwd", case + " normal", G.judge(n_h, n_t, n_64, (r_64.detach().abs().amax(-1, keepdim=True) / length).expand(-1, 3), 10, "normal " + case))
        scale = ((g_n.double().abs().amax(-1, keepdim=True) / length if use_n else 0.0) +
                 (g_r.double().abs().amax(-1, keepdim=True) if use_r else 0.0)) / eps
        rec = G.judge(sb.grad, sa.grad, s64.grad, scale.expand(-1, 6), 16, "d / d sdf6 " + case)
        _report("fd_normal_bwd", case, rec)
        assert torch.equal(sb.grad[:, 0::2], -sb.grad[:, 1::2])


def test_fd_normal_forward_nan_to_num():
    """forward only: a row with one NaN, +-inf or overflowing tap equals the fp32 torch chain's nan_to_num output exactly
    wherever that output is 0 or +-FLT_MAX (torch itself returns NaN gradients there: no backward)."""
    from morpheus_amd import ops
    c = G.normal_nonfinite_case()
    s6 = _dev(c["s6"])
    n_t, _ = G.normal(s6, c["eps"])
    n_h, _ = ops.fd_normal(s6, c["eps"])
    fmax = torch.finfo(F32).max
    acted = (n_t == 0) | (n_t.abs() == fmax)
    assert int(acted.sum()) >= 18 and bool(torch.isfinite(n_h).all())
    assert torch.equal(n_h[acted], n_t[acted])
    _report("fd_normal_fwd", "nan_to_num", dict(worst_hip=0.0, worst_chain=0.0, ratio=0.0, n_above=int((n_h != n_t).sum())))


# ------------------------------------------------------------------------------------------------------------ MultiCode
@pytest.mark.parametrize("sizes", [(2, 3, 200), (25, 50, 200)])
@pytest.mark.parametrize("C,F", [(16, 1), (16, 5), (16, 6), (1, 85), (1, 86), (16, 600), (1, 600)])
def test_multicode_knots_edges_and_atomics(sizes, C, F):
    """mh_multicode_fwd / _bwd against float64 F.grid_sample: a two-entry table, every knot of every level, 0, 1, the fp32 below
    1, times outside [0, 1], F x 3 x C on both sides of a 256-lane block, 200 times in one cell (a hot atomic address).
    Errors are relative to the sum of the ABSOLUTE lerp terms (float64 grid_sample of |table|, resp. of |g|)."""
    from morpheus_amd import ops
    c = G.multicode_case(sizes, C, F)
    t, g = _dev(c["t"]), _dev(c["g"])
    va, vb, v64 = ([_leaf(v, d) for v in c["vols"]] for d in (F32, F32, F64))
    out_t = G.multicode(t, va)
    out_h = ops.multicode_sample(t, vb)
    out_64 = G.multicode(t.double(), v64)
    for out, d in ((out_t, F32), (out_h, F32), (out_64, F64)):
        (out * g.to(d)).sum().backward()
    with torch.no_grad():
        abs_out = G.multicode(t.double(), [v.detach().abs() for v in v64])
    vz = [v.detach().clone().requires_grad_(True) for v in v64]
    (G.multicode(t.double(), vz) * g.double().abs()).sum().backward()
    # floor where the chain is exact: the row coordinate t (size - 1) carries 3 roundings of size - 1 cells, the lerp 4 more
    count = 4 + 3 * max(sizes)
    case = f"sizes={sizes} C={C} F={F}"
    _report("multicode_fwd", case, G.judge(out_h, out_t, out_64, abs_out, count, "MultiCode.sample " + case))
    for k in range(3):
        assert bool((vb[k].grad[vz[k].grad == 0] == 0).all()), "table entries no time touches keep a zero gradient"
        rec = G.judge(vb[k].grad, va[k].grad, v64[k].grad, vz[k].grad, count + F, f"d volumes.{k} " + case)
        _report("multicode_bwd", case + f" level {k}", rec)


# ----------------------------------------------------------------------------------------------------------- sdf losses
@pytest.mark.parametrize("M", [1, 255, 256, 257, 32768, 33069])
def test_sdf_losses_every_branch_stride_loop_and_padding(M):
    """mh_sdf_losses_fwd / _bwd on the dyadic ray table tiled to M (33 069: the first size with a second, ragged stride trip):
    mask given / None, n_valid None / M - 300 / M / M + 5 with NaN in the padding, both losses / fs only / sdf only.

    The zero ties: at a predicted sdf of exactly 0 in free space torch autograd of utils.py:109 gives -5 / n (clamp(min=0)
    passes its gradient AT 0; tests/test_glue_oracle_host.py pins that on the CPU); the kernel returned 0 there until
    `pos = mx >= 0` in sdf_loss_term.  The second tie (p == 0, bnd == 0, where max() splits -5 and +1 in halves) lies on the
    surface, which is never free space, so both give 0 there; the rows are asserted either way."""
    from morpheus_amd import ops
    c = G.sdf_case(M)
    trunc, ri = c["trunc"], _dev(c["ri"])
    ts, te, depth = _dev(c["ts"]), _dev(c["te"]), _dev(c["depth"])
    count = G.loss_rounding_count(M)
    nvs = [None] + ([M - 300] if M > 300 else []) + [M, M + 5]
    for use_mask in (True, False):
        mask = _dev(c["mask"]) if use_mask else None
        br = G.sdf_branches(c, use_mask)
        for nv in nvs:
            rows = M if nv is None else min(nv, M)
            pred = _dev(c["pred"]).clone()
            pred[rows:] = float("nan")
            nv_t = None if nv is None else torch.tensor(nv, dtype=torch.int32, device=DEV)
            dec = {k: v[:rows] for k, v in G.sdf_decisions(ts, te, depth, mask, ri, trunc).items()}
            for w_fs, w_sl in ((2.0, 3.0), (2.0, None), (None, 3.0)):
                def loss(fs, sl):
                    return sum(([w_fs * fs] if w_fs else []) + ([w_sl * sl] if w_sl else []))

                pa, p64 = pred[:rows].clone().requires_grad_(True), pred[:rows].double().requires_grad_(True)
                fs_t, sl_t, fst_t, slt_t, _ = G.sdf_losses(pa, ts[:rows], te[:rows], depth, mask, ri[:rows], trunc, terms=True)
                fs_64, sl_64, fst_64, slt_64, nd = G.sdf_losses(p64, ts[:rows].double(), te[:rows].double(), depth.double(),
                                                               None if mask is None else mask.double(), ri[:rows], trunc, dec, terms=True)
                loss(fs_t, sl_t).backward()
                loss(fs_64, sl_64).backward()
                pb = pred.clone().requires_grad_(True)
                fs_h, sl_h = ops.sdf_losses(pb, ts, te, ri, depth, mask, trunc, nv_t)
                loss(fs_h, sl_h).backward()
                case = f"M={M} mask={use_mask} n_valid={nv} fs={w_fs} sl={w_sl}"
                assert bool((pb.grad[rows:] == 0).all()), "padding behind n_valid: gradient exactly 0 (NaN predictions there)"
                # totals: `count` roundings of the absolute sum on the way of a term into the total, plus the terms' own error --
                # 3 x what the fp32 chain's terms (expf, the subtraction, the division by n) are off, at least 2 roundings each
                for name, got, want, t32, t64 in (("fs", fs_h, fs_64, fst_t, fst_64), ("sl", sl_h, sl_64, slt_t, slt_64)):
                    t64 = t64.detach()
                    per_term = torch.maximum(3.0 * (t32.detach().double() - t64).abs(), 2 * G.U * t64.abs()).sum() / nd
                    rec = G.judge_sum(got, want, t64.abs().sum() / nd, count, f"{name}_loss " + case, extra=float(per_term))
                    _report("sdf_losses_fwd", case + " " + name, rec)
                # d/d pred: expf and two divisions per element; relative to the element, floored at 1e-3 of the largest
                g64 = p64.grad
                scale = g64.abs().clamp(min=1e-3 * float(g64.abs().max()))
                _report("sdf_losses_bwd", case, G.judge(pb.grad[:rows], pa.grad, g64, scale, 4, "d / d pred " + case))
                if M >= 255 and w_fs:
                    t1 = _dev(br["zero tie: p == 0 in free space"])[:rows]
                    t2 = _dev(br["zero tie: p == 0 on the surface"])[:rows]
                    assert int(t1.sum()) >= 4 and int(t2.sum()) >= 4
                    want1 = w_fs * -5.0 / float(nd)
                    assert bool(((pb.grad[:rows][t1].double() - want1).abs() <= 4 * G.U * abs(want1)).all()), "p == 0 in free space: -5 / n"
                    assert bool((pb.grad[:rows][t2] == 0).all())
