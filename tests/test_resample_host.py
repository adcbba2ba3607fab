"""Importance resampling without a GPU: the numpy restatements (tests/resample_oracle.py) against the reference's recorded results
(tests/golden/sample_pdf.npz, tools/make_resample_golden.py), the packed restatement against the dense one, the refinement
property on an analytic sphere, and the refusals of the Python layer."""
import os

import numpy as np
import pytest
import torch

from tests import f64_judge as J
from tests import resample_oracle as ro

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_pdf.npz")
FACTOR, FLOOR = 3, 4 * J.U          # f64_judge's table: glue_f64_oracle / grid_f64_cases use the factor, step / losses the floor


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _case(golden, name):
    return tuple(golden[f"{name}_{k}"] for k in ("bins", "weights", "u", "s32", "s64"))


def test_golden_holds_every_case(golden):
    names = [c[0] for c in ro.cases()]
    assert len(names) == len(set(names)) == len(ro.T_SET) * len(ro.KINDS)
    assert {c[1] for c in ro.cases()} == set(ro.T_SET) and {c[2] for c in ro.cases()} == set(ro.N_SET)
    assert {c[3] for c in ro.cases()} == set(ro.B_SET)
    for name, T, n, B, kind in ro.cases():
        bins, w, u, s32, s64 = _case(golden, name)
        assert bins.shape == (B, T) and w.shape == (B, T - 1) and u.shape == s32.shape == s64.shape == (B, n)
        assert bins.dtype == w.dtype == u.dtype == s32.dtype == np.float32 and s64.dtype == np.float64
        assert u.reshape(-1)[0] == 0.0 and (B * n == 1 or np.float32(1 - J.U) in u)          # the forced draws
        if kind == "sparse" and T > 3:
            assert 0.6 < (w == 0).mean() < 0.95
    assert os.path.getsize(GOLDEN) < 512 * 1024


def test_oracle_against_golden(golden):
    """float64 restatement == the reference's float64 run up to the order of its sums: both are float64 chains of <= 200 terms
    (200 x 2^-53 = 2.2e-14 relative in the CDF), and the `denom >= 1e-5` rule bounds the conditioning of t by 1e5, so positions
    agree to 2.2e-9 of the span; 1e-8 is asserted.  The fp32 restatements -- the reference's form, and the kernel's form (float64
    sums rounded once, running maximum, the sample held in its bin) -- are judged in the measure against the reference's own
    fp32 run: worst e <= max(3 x its worst e, 4 U)."""
    for name, T, n, B, kind in ro.cases():
        bins, w, u, s32, s64 = _case(golden, name)
        span = (bins[:, -1:] - bins[:, :1]).astype(np.float64)
        o64 = ro.sample_pdf_np(bins, w, u, np.float64)
        assert bool((np.abs(o64 - s64) <= 1e-8 * span).all()), name
        e_ref = ro.score_dense(s32, s64, u, bins, w)
        for form in ("reference", "kernel"):
            o32 = ro.sample_pdf_np(bins, w, u, np.float32, cdf=form, hold=form == "kernel")
            e = ro.score_dense(o32, s64, u, bins, w)
            print(f"{name:14s} {form:9s}: worst e {e / J.U:6.2f} U; the reference's fp32 run {e_ref / J.U:5.2f} U")
            assert J.within(e, e_ref, FACTOR, FLOOR), (name, form, e / J.U, e_ref / J.U)
            assert bool(np.isfinite(o32).all()), (name, form)
            if form == "kernel":
                assert bool(((o32 >= bins[:, :1]) & (o32 <= bins[:, -1:])).all()), name
    for n in ro.N_SET:
        assert np.array_equal(golden[f"det_n{n}"], torch.linspace(0. + 0.5 / n, 1. - 0.5 / n, steps=n).numpy())


def _contiguous(bins):
    B, T = bins.shape
    rs = (np.arange(B) * (T - 1)).astype(np.int32)
    rc = np.full(B, T - 1, dtype=np.int32)
    return rs, rc, bins[:, :-1].reshape(-1).copy(), bins[:, 1:].reshape(-1).copy()


@pytest.mark.parametrize("name", ["T3_uniform", "T65_laplace", "T66_sparse", "T129_span20", "T200_zero"])
def test_packed_oracle_on_contiguous_rays(golden, name):
    """On contiguous fixed-S rays the packed restatement's cut points are the dense restatement's samples (same CDF form, the
    sample held in its bin) at the draws u_k = (k + j_k) / n, sorted -- bit for bit -- and the refined set keeps the invariants."""
    bins, w, _, _, _ = _case(golden, name)
    B, T = bins.shape
    n = 33
    jit = np.random.default_rng(5).random((B, n)).astype(np.float32)
    jit[0, :2] = 0.0, np.float32(1 - J.U)
    rs, rc, ts, te = _contiguous(bins)
    for form in ("reference", "kernel"):
        out = ro.resample_packed_np(rs, rc, ts, te, w.reshape(-1), n, jit, dtype=np.float32, cdf=form)
        ro.check_invariants(out, rs, rc, ts, te, n)
        u = ((np.arange(n, dtype=np.float32)[None] + jit) / np.float32(n)).astype(np.float32)
        dense = ro.sample_pdf_np(bins, w, u, np.float32, cdf=form, hold=True)
        for b in range(B):
            row = out["t_starts"][out["ray_start"][b]:out["ray_start"][b] + T - 1 + n]
            assert np.array_equal(ro.draws_of(row, bins[b, :-1]), np.sort(dense[b])), (name, form, b)
            assert bool((np.diff(out["draws"][b][1]) >= 0).all())                   # draws are ordered in k as they are


def test_packed_oracle_gaps_empty_rays_and_zero_width():
    """rays of 0, 1 and 7 intervals with gaps, a zero-width interval and all-zero weights: the invariants, and no draw in a gap"""
    rng = np.random.default_rng(11)
    cnt = np.array([0, 1, 7, 0, 5, 3], dtype=np.int32)
    rs = (np.cumsum(cnt) - cnt).astype(np.int32)
    ts, te = [], []
    for c in cnt:
        edges = np.sort(rng.random(2 * c)).astype(np.float32) + np.float32(0.5)
        ts += list(edges[0::2])
        te += list(edges[1::2])
    ts, te = np.array(ts, dtype=np.float32), np.array(te, dtype=np.float32)
    te[rs[4] + 2] = ts[rs[4] + 2]                                   # a zero-width interval inside ray 4
    ts[rs[5]:rs[5] + 3] = te[rs[5]:rs[5] + 3] = 0.0                 # a miss ray of the uniform sampler: zero-width at t = 0
    w = rng.random(ts.shape[0]).astype(np.float32)
    w[rs[2]:rs[2] + 7] = 0.0
    for n in (1, 8):
        out = ro.resample_packed_np(rs, cnt, ts, te, w, n, rng.random((6, n)).astype(np.float32))
        ro.check_invariants(out, rs, cnt, ts, te, n)
        assert out["draws"][0] is None and int(out["ray_cnt"][0]) == 0
    with pytest.raises(AssertionError):                             # the checker does see a draw in a gap
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out.items()}
        p = int(bad["ray_start"][2])
        gap = np.float32(0.5 * (te[rs[2]] + ts[rs[2] + 1]))
        bad["t_ends"][p], bad["t_starts"][p + 1] = gap, gap
        ro.check_invariants(bad, rs, cnt, ts, te, n)


def test_refinement_on_the_sphere():
    """Analytic sphere (radius 0.5, Laplace density, beta = 0.02), 256 rays from z = -1.5, t in [0.5, 2.5]: S = 32 coarse
    intervals against the same cut at n = 32 draws (seeded jitter), depth by the midpoint rule, error against a 16 384-interval
    quadrature.  The refined set's mean error must be at most half the coarse set's."""
    beta, S, n, rays = 0.02, 32, 32, 256
    o, d = ro.sphere_rays(rays, seed=0)
    edges = np.linspace(0.5, 2.5, S + 1)
    ts, te = np.tile(edges[:-1], (rays, 1)), np.tile(edges[1:], (rays, 1))
    fine = np.linspace(0.5, 2.5, 16384 + 1)
    f_ts, f_te = np.tile(fine[:-1], (rays, 1)), np.tile(fine[1:], (rays, 1))
    truth, _ = ro.render_depth(f_ts, f_te, ro.sphere_sigma(o, d, 0.5 * (f_ts + f_te), beta))
    coarse, w = ro.render_depth(ts, te, ro.sphere_sigma(o, d, 0.5 * (ts + te), beta))
    rs, rc = (np.arange(rays) * S).astype(np.int32), np.full(rays, S, dtype=np.int32)
    jit = np.random.default_rng(3).random((rays, n)).astype(np.float32)
    out = ro.resample_packed_np(rs, rc, ts.reshape(-1).astype(np.float32), te.reshape(-1).astype(np.float32),
                                w.reshape(-1).astype(np.float32), n, jit, dtype=np.float32)
    r_ts, r_te = (out[k].astype(np.float64).reshape(rays, S + n) for k in ("t_starts", "t_ends"))
    refined, _ = ro.render_depth(r_ts, r_te, ro.sphere_sigma(o, d, 0.5 * (r_ts + r_te), beta))
    e_c, e_r = float(np.abs(coarse - truth).mean()), float(np.abs(refined - truth).mean())
    print(f"sphere beta {beta}: mean |depth error| coarse S={S} {e_c:.3e}, refined +{n} {e_r:.3e} ({e_c / e_r:.1f} x)")
    assert e_r <= 0.5 * e_c


def test_refusals_and_opt_in():
    from morpheus_amd import _lib, ops, resample
    from morpheus_amd.render import HotPathRenderer
    bins, w = torch.linspace(0, 1, 5)[None], torch.ones(1, 4)
    with pytest.raises(_lib.MorpheusHipError):                      # no CPU path
        resample.sample_pdf(bins, w, 4, det=True)
    with pytest.raises(_lib.MorpheusHipError):
        ops.sample_pdf(bins, w, torch.rand(1, 4))
    rs, rc = torch.zeros(1, dtype=torch.int32), torch.full((1,), 4, dtype=torch.int32)
    ts, te = bins[0, :-1].contiguous(), bins[0, 1:].contiguous()
    with pytest.raises(_lib.MorpheusHipError):
        resample.importance_sampling(rs, rc, ts, te, 4, weights=w[0])
    with pytest.raises(_lib.MorpheusHipError):
        ops.resample_packed(w[0], ts, te, rs, rc, 4)
    with pytest.raises(ValueError):                                 # both, neither
        resample.importance_sampling(rs, rc, ts, te, 4, weights=w[0], sigmas=w[0])
    with pytest.raises(ValueError):
        resample.importance_sampling(rs, rc, ts, te, 4)
    with pytest.raises(ValueError):
        resample.importance_sampling(rs, rc, ts, te, 4, weights=w[0], det=True, jitter=torch.rand(1, 4))
    with pytest.raises(ValueError):
        resample.sample_pdf(bins, torch.ones(1, 5), 4)
    # the renderer's opt-in
    cfg = {"render": {"step_size": 0.01}}
    rend = HotPathRenderer(None, cfg, None, 1)
    assert rend.importance is None and rend._importance_args() is None
    rend.importance = dict(n_importance=8, jiter=None)
    with pytest.raises(ValueError, match="jiter"):
        rend._importance_args()
    rend.importance = dict(n_importance=8)
    assert rend._importance_args() == dict(n_importance=8, det=False, jitter=None, eps=1e-5)
    rend.importance = dict(n_importance=0)
    assert rend._importance_args() is None
    seeded = HotPathRenderer(None, {"render": {"step_size": 0.02, "n_importance": 32}}, None, 1)
    assert seeded.importance == dict(n_importance=32)
    from morpheus_amd import harness
    for name in ("snoopy", "teddy"):                                # the shipped configs do not opt in
        assert "n_importance" not in harness.load_config(name)["render"]
        assert HotPathRenderer(None, harness.load_config(name), None, 1).importance is None


def test_entry_points_are_declared_and_abi_unchanged():
    from morpheus_amd import _lib
    for name in ("mh_resample_stage", "mh_sample_pdf", "mh_resample_ranges", "mh_resample_packed"):
        assert name in _lib.EXPORTS
    assert _lib._ABI == 10
    lib = _lib.load()
    # the LDS staging holds the longest ray the shipped step marches in the shipped boxes
    assert int(lib.mh_resample_stage()) == 384 >= max(int(lib.mh_march_cap(0.01, 1.0)), int(lib.mh_march_cap(0.01, 1.01)))
