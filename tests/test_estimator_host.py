"""morpheus_amd.estimator, everything that needs no GPU: signatures and buffers as recalled from nerfacc 0.5.x, the state_dict round
trip with OccupancyGrid, the level boxes, the refusals, the restatement (tests/estimator_oracle.py) against oracle/field.py where
the two definitions meet, and every case of the GPU tests reaching what it names -- asserted from the restatement."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from oracle import field as of
from tests import estimator_oracle as eo
from tests import sampler_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

SIGNATURES = {
    "__init__": "(self, roi_aabb, resolution=128, levels=1)",
    "sampling": "(self, rays_o, rays_d, sigma_fn=None, alpha_fn=None, near_plane=0.0, far_plane=10000000000.0, t_min=None, "
                "t_max=None, render_step_size=0.001, early_stop_eps=0.0001, alpha_thre=0.0, stratified=False, cone_angle=0.0)",
    "mark_invisible_cells": "(self, K, c2w, width, height, near_plane=0.0)",
}


def _sig(fn):
    sig = inspect.signature(fn)
    return "(" + ", ".join(p.name if p.default is inspect.Parameter.empty else f"{p.name}={p.default!r}" for p in sig.parameters.values()) + ")"


def test_public_signatures_are_nerfaccs():
    from morpheus_amd import estimator, volrend
    for name, want in SIGNATURES.items():
        assert _sig(getattr(estimator.OccGridEstimator, name)) == want, name
    # nerfacc's update_every_n_steps, with the optional draws= behind it
    assert _sig(estimator.OccGridEstimator.update_every_n_steps) == \
        "(self, step, occ_eval_fn, occ_thre=0.01, ema_decay=0.95, warmup_steps=256, n=16, draws=None)"
    assert volrend.OccGridEstimator is estimator.OccGridEstimator and "OccGridEstimator" in volrend.__all__
    for doc in (estimator.__doc__, estimator.OccGridEstimator.sampling.__doc__):
        assert "recalled, agreement unverified" in doc
    assert "OccupancyGrid.sampling` raises" in estimator.OccGridEstimator.sampling.__doc__
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 7j." in design and "recalled, agreement unverified" in design[design.index("## 7j."):]


def test_buffers_and_state_dict_round_trip_with_occupancy_grid():
    from morpheus_amd.estimator import OccGridEstimator
    from morpheus_amd.occgrid import OccupancyGrid
    e = OccGridEstimator([-1.01] * 3 + [1.01] * 3, resolution=8)
    g = OccupancyGrid([-1.01] * 3 + [1.01] * 3, 8)
    se, sg = e.state_dict(), g.state_dict()
    assert list(se) == list(sg) == ["resolution", "aabbs", "occs", "binaries"]
    for k in se:
        assert se[k].dtype == sg[k].dtype and se[k].shape == sg[k].shape, k
    assert torch.equal(se["aabbs"], sg["aabbs"]) and torch.equal(se["resolution"], sg["resolution"])
    g.occs.copy_(torch.rand(512))
    g.set_binary(torch.rand(8, 8, 8) > 0.5)
    e.load_state_dict(g.state_dict())
    assert torch.equal(e.occs, g.occs) and torch.equal(e.binaries, g.binaries)
    e.occs.mul_(0.5)
    e.set_binary(~e.binaries)
    g.load_state_dict(e.state_dict())
    assert torch.equal(e.occs, g.occs) and torch.equal(e.binaries, g.binaries)
    # a non-cubic multi-level grid
    m = OccGridEstimator(eo.ROOT, resolution=eo.RES, levels=3)
    assert m.resolution.dtype == torch.int32 and m.resolution.tolist() == [8, 12, 16]
    assert m.aabbs.dtype == torch.float32 and m.aabbs.shape == (3, 6)
    assert m.occs.dtype == torch.float32 and m.occs.shape == (3 * 8 * 12 * 16,) and m.cells_per_lvl == 8 * 12 * 16
    assert m.binaries.dtype == torch.bool and m.binaries.shape == (3, 8, 12, 16)
    assert m.thre is None and m.packed is None and m.sample_capacity is None and m.fixed_jitter is None
    # loading a box keeps the host diagonal of the slot-row bound in step
    m2 = OccGridEstimator([0, 0, 0, 1, 1, 1], resolution=eo.RES, levels=3)
    m2.load_state_dict(m.state_dict())
    assert m2._diagonal == m._diagonal == pytest.approx(np.sqrt(4.0 + 9.0 + 16.0))


def test_level_boxes_of_a_non_centred_box():
    from morpheus_amd.estimator import OccGridEstimator, level_aabbs
    box = (0.1, -0.7, 0.3, 0.4, 0.5, 1.7)
    a = OccGridEstimator(box, resolution=4, levels=3).aabbs.numpy()
    b64 = np.array(box, np.float64)
    c, h = (b64[:3] + b64[3:]) / 2, (b64[3:] - b64[:3]) / 2
    for l in range(3):
        want = np.concatenate([c - h * 2 ** l, c + h * 2 ** l]).astype(F)        # float64, rounded once
        assert a[l].tobytes() == want.tobytes(), l
    assert np.array_equal(level_aabbs(eo.ROOT, 3)[2], np.array(eo.COARSE, F))
    assert np.array_equal(level_aabbs(eo.ROOT, 3).astype(np.float64)[1], [0.0, -0.5, -0.25, 1.0, 1.0, 1.75])       # exact in fp32


def test_refusals():
    from morpheus_amd._lib import MorpheusHipError
    from morpheus_amd.estimator import OccGridEstimator
    for bad in ([0, 0, 0, 1, 1], [0, 0, 0, 1, 0, 1], [0, 0, 0, 1, -1, 1], [0, 0, 0, 1, float("nan"), 1], [0, 0, 0, float("inf"), 1, 1]):
        with pytest.raises(ValueError, match="roi_aabb"):
            OccGridEstimator(bad, 4)
    for lv in (0, -1, 1.5, 17):
        with pytest.raises(ValueError, match="levels"):
            OccGridEstimator([0, 0, 0, 1, 1, 1], 4, levels=lv)
    for res in (0, (4, 4), (4, 0, 4)):
        with pytest.raises(ValueError, match="resolution"):
            OccGridEstimator([0, 0, 0, 1, 1, 1], res)
    e = OccGridEstimator([0, 0, 0, 1, 1, 1], 4)
    o, d = torch.zeros(2, 3), torch.ones(2, 3)
    fn = lambda ts, te, ri: ts
    with pytest.raises(ValueError, match="not both"):
        e.sampling(o, d, sigma_fn=fn, alpha_fn=fn)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        e.sampling(o, d, alpha_thre=1.5)
    with pytest.raises(ValueError, match="cone_angle"):
        e.sampling(o, d, cone_angle=-0.1)
    with pytest.raises(MorpheusHipError, match="no CPU path"):
        e.sampling(o, d)                                                   # the defaults, early_stop_eps = 1e-4 among them
    with pytest.raises(MorpheusHipError, match="no CPU path"):
        e.update_every_n_steps(0, lambda x: x[:, 0])
    with pytest.raises(MorpheusHipError, match="no CPU path"):
        e.mark_invisible_cells(torch.eye(3), torch.eye(4)[None], 8, 8)
    e.update_every_n_steps(3, None)                                        # not an n-th step: nothing is touched


def test_c_abi_and_build():
    from morpheus_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "morpheus_hip.h")).read()
    lib = _lib.load()
    for name in ("mh_est_march_cap", "mh_est_march_slots", "mh_est_occ_count", "mh_est_occ_pack", "mh_est_select", "mh_est_ema",
                 "mh_est_threshold", "mh_est_mark_invisible", "mh_est_occ_chunk", "mh_est_max_partials"):
        assert len(re.findall(r"\b%s\s*\(" % name, hdr)) == 1 and name in _lib.EXPORTS, name
    assert "estimator.hip" in build.SOURCES and "estimator.hip" not in build.FILE_FLAGS        # its own pragma, like sampler.hip
    src = open(os.path.join(ROOT, "morpheus_amd", "csrc", "estimator.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    # host-validated arguments: a status, never a launch
    assert lib.mh_est_march_cap(0.05, float(np.sqrt(29.0)), 0.0, 1e10) == 111 == eo.retry_case()["cap"]
    assert lib.mh_est_march_cap(0.01, 10.0, 0.8, 1.7) == int(0.9 / 0.01) + 4 and lib.mh_est_march_cap(0.0, 1.0, 0.0, 1.0) == 0
    assert lib.mh_est_march_cap(0.01, 10.0, 2.0, 1.0) == 4
    assert lib.mh_est_march_slots(*([None] * 5), 0, 0.01, 0.0, 0.0, 1e10, None, 1, 4, 4, 4, None, 8, None, None, None, None, None) == 0
    assert lib.mh_est_march_slots(*([None] * 5), 3, 0.01, 0.0, 0.0, 1e10, None, 1, 4, 4, 4, None, 8, None, None, None, None, None) == 1
    assert lib.mh_est_select(1, 17, 4, 4, 4, 64, *([None] * 8), None) == 1                      # more than 16 levels
    assert lib.mh_est_ema(None, None, 1, 0, 64, None, 0.95, None, None) == 0 and lib.mh_est_ema(None, None, 1, 8, 64, None, 0.95, None, None) == 1
    assert lib.mh_est_threshold(None, 64, 0.01, None, None, None, None) == 1
    assert lib.mh_est_mark_invisible(None, None, 1, 8.0, 8.0, 0.0, None, 1, 4, 4, 4, None, None) == 1
    assert lib.mh_est_occ_chunk() == 2048 and lib.mh_est_max_partials() == 1024


# ------------------------------------------------------------------------------------------- the restatement against itself
def test_restatement_equals_oracle_field_where_they_meet():
    """cone_angle = 0, one level, a centred cubic box: estimator_oracle.march is oracle.field.march_samples bit for bit on the
    marcher cases of tests/sampler_cases.py (the nonfinite rows among them)"""
    n = 0
    for c in sc.marcher_cases() + sc.nonfinite_cases():
        if c["grid"].shape[0] == 128 and c.get("u") not in (0.0, sc.BELOW_ONE):
            continue                                                       # the 128^3 grid at two jitters is enough
        b = F(c["bound"])
        aabbs = np.array([[-b, -b, -b, b, b, b]], F)
        ri, ts, te, n_steps, k = of.march_samples(c["o"], c["d"], c["jitter"], c["step"], c["bound"], c["grid"], return_steps=True)
        m = eo.march(c["o"], c["d"], c["jitter"], c["step"], aabbs, c["grid"][None])
        assert torch.equal(m["ri"], ri) and torch.equal(m["n_steps"], n_steps) and torch.equal(m["k"], k), c["name"]
        assert m["ts"].numpy().tobytes() == ts.numpy().tobytes() and m["te"].numpy().tobytes() == te.numpy().tobytes(), c["name"]
        n += ri.numel()
    assert n > 10000
    # the constructor's box for that bound is the same row
    from morpheus_amd.estimator import level_aabbs
    assert level_aabbs([-sc.BOUND] * 3 + [sc.BOUND] * 3, 1).tobytes() == np.array([[-F(sc.BOUND)] * 3 + [F(sc.BOUND)] * 3], F).tobytes()


@pytest.fixture(scope="module")
def marched():
    aabbs, binaries = eo.marcher_grid()
    return aabbs, binaries, {c["name"]: (c, eo.run_case(c, aabbs, binaries)) for c in eo.marcher_cases()}


def test_marcher_cases_reach_what_they_name(marched):
    aabbs, binaries, by = marched
    a = aabbs.numpy()
    assert a.shape == (3, 6) and np.array_equal(a[2], np.array(eo.COARSE, F)) and not np.allclose(a[0, :3], -a[0, 3:])
    assert tuple(binaries.shape) == (3, 8, 12, 16) and all(0.2 < float(binaries[l].float().mean()) < 0.8 for l in range(3))
    # the miss names are finite_specials' rows without a step
    so, sd, sn = sc.finite_specials()
    steps = of.march_samples(so, sd, None, sc.STEP, sc.BOUND, torch.ones(1, 1, 1, dtype=torch.uint8), return_steps=True)[3]
    assert tuple(nm for nm, s in zip(sn, steps.tolist()) if s == 0) == eo.MISS_NAMES
    for name in ("counts", "counts-cone"):
        c, m = by[name]
        n = dict(zip(c["names"], m["n_steps"].tolist()))
        assert all(n[nm] == 0 for nm in eo.MISS_NAMES), name
        if name == "counts":
            assert [n[f"count{k}"] for k in eo.COUNT_STEPS] == [63, 64, 65, 128, 129]
        else:
            assert {-(-n[f"count{k}"] // 64) for k in eo.COUNT_STEPS} == {1, 2, 3}
        assert 0 < int(m["cnt"].sum()) < int(m["n_steps"].sum())             # some steps kept, some dropped
    # the recurrence is not the closed form: the same rays give other bits
    assert not torch.equal(by["counts"][1]["ts"], by["counts-cone"][1]["ts"][:by["counts"][1]["ts"].numel()])
    # cone switch at ts = step / cone_angle = 1
    c, _ = by["cone-switch"]
    full = eo.march(c["o"], c["d"], c["jitter"], c["step"], aabbs, torch.ones_like(binaries), c["cone_angle"])
    sw = c["step"] / c["cone_angle"]
    per = {nm: full["ts"][full["ri"] == i].numpy() for i, nm in enumerate(c["names"])}
    assert per["switch_inside"].min() < sw < per["switch_inside"].max() and len(per["switch_inside"]) > 128
    assert per["before_switch"].max() < sw and len(per["before_switch"]) > 64
    assert per["after_switch"].min() > sw and len(per["after_switch"]) > 64
    dts = np.diff(per["switch_inside"])
    assert abs(dts[0] - c["step"]) < 1e-6 and dts[-1] > 4 * c["step"]
    # faces: y sits on / one ulp off a face of level 0 and level 1, and the level read changes there
    c, m = by["faces"]
    o = c["o"].numpy()
    for l in (0, 1):
        for side, col, flip in (("lo", 1, ("below", "on")), ("hi", 4, ("below", "on"))):
            ys = {tag: o[c["names"].index(f"y_{side}{l}_{tag}"), 1] for tag in ("below", "on", "above")}
            assert ys["on"] == a[l, col] and ys["below"] == np.nextafter(a[l, col], F(-np.inf)) and ys["above"] == np.nextafter(a[l, col], F(np.inf))
            lv = {tag: eo.level_of(np.array([[0.5, ys[tag], 0.75]], F), a)[0] for tag in ys}
            assert lv[flip[0]] != lv[flip[1]] and l in lv.values() and l + 1 in lv.values(), (l, side, lv)
    kept = {nm: tuple(m["k"][m["ri"] == i].tolist()) for i, nm in enumerate(c["names"])}
    assert sum(kept[f"y_{s}{l}_{p}"] != kept[f"y_{s}{l}_{q}"] for l in (0, 1) for s, p, q in (("lo", "below", "on"), ("hi", "below", "on"))) >= 3
    i = c["names"].index("x_faces")
    tm = (F(0.5) + F(0.5) * F(c["step"])) + np.arange(64, dtype=F) * F(c["step"]) + F(c["step"]) / 2
    xs = F(-1.0) + tm
    assert {0.0, 0.25, 0.75, 1.0} <= set(xs.tolist())                       # midpoints exactly on x faces of levels 0 and 1
    assert int(m["n_steps"][i]) == 64
    # planes
    c, m = by["planes"]
    n = dict(zip(c["names"], m["n_steps"].tolist()))
    assert n["tmin_gt_tmax"] == 0 and n["entry_before_near"] == 90 and 64 < n["entry_before_near"] < 128     # far_plane inside trip 2
    first = float(eo.march(c["o"][:1], c["d"][:1], None, c["step"], aabbs, torch.ones_like(binaries), 0.0, c["near_plane"], c["far_plane"])["ts"][0])
    assert first == float(F(0.8)) and float(eo.clip(c["o"].numpy()[:1], c["d"].numpy()[:1], a[2])[0][0]) == 0.5
    assert n["tmax_cuts"] == 50 and n["tmin_raises"] == 70 and n["inside"] == 90
    c, m = by["planes-cone"]
    assert all(64 < s for s in m["n_steps"].tolist())
    # retry: 200 steps against a slot row of 111 -> one doubling
    c = eo.retry_case()
    m = eo.run_case(c, aabbs, binaries)
    assert m["n_steps"].tolist()[1] == 200 and max(m["n_steps"].tolist()[0], m["n_steps"].tolist()[2]) <= 111
    assert sc.slot_expect(m, 111)[3] == 1 and sc.slot_expect(m, 222)[3] == 0


def test_update_cases_reach_what_they_name():
    L, cells = eo.UPD_LEVELS, int(np.prod(eo.UPD_RES))
    k = cells // 4
    aabbs = eo.level_aabbs(eo.UPD_ROOT, L)
    states = eo.update_states()
    assert set(states) == {"c>k", "c<=k", "c=0"}
    draws = eo.update_draws(False)
    occ = eo.occ_of_entries(L, 2 * k)
    assert bool((occ < 0).any()) and bool((occ > 0.5).any())
    for name, (occs, binaries) in states.items():
        ids, pts = eo.select(aabbs, binaries, False, draws)
        assert ids.shape == (L, 2 * k) and pts.shape == (L, 2 * k, 3)
        assert (ids[:, k:] == -1).any() == (name != "c>k") and ((ids[:, k:] == -1).all() == (name == "c=0"))
        # duplicates with different evaluations, in the uniform part and (c > k) in the occupied part
        for l in range(L):
            u, inv = np.unique(ids[l, :k], return_inverse=True)
            assert len(u) < k
            first = ids[l, 0]
            vals = occ[l].numpy()[:k][ids[l, :k] == first]
            assert len(vals) >= 8 and len(set(vals.tolist())) > 1
        # points lie inside their level's box and in their cell
        lo, hi = aabbs[:, None, :3], aabbs[:, None, 3:]
        assert ((pts >= lo) & (pts <= hi)).all()
        # invisible cells are named and stay -1; named visible cells change
        new = eo.ema(ids, occ, occs, 0.95)
        old = occs.numpy()
        named = np.zeros(L * cells, bool)
        for l in range(L):
            named[ids[l][ids[l] >= 0].astype(np.int64) + l * cells] = True
        assert (named & (old < 0)).any() and (new[old < 0] == -1).all()
        assert (new[~named] == old[~named]).all() and (new[named & (old >= 0)] != old[named & (old >= 0)]).any()
        assert (new[named & (old >= 0)] >= (old * F(0.95))[named & (old >= 0)]).all()
        thre, mean64 = eo.threshold(new, 0.01)
        assert thre == F(0.01) and mean64 > 0.01                            # the cap branch; the mean branch:
        thre2, mean2 = eo.threshold(new, 0.9)
        assert thre2 == F(mean2) and 0 < thre2 < 0.9
        assert 0 < (new > thre2).sum() < new.size
    ids, pts = eo.select(aabbs, states["c>k"][1], True, eo.update_draws(True))
    assert ids.shape == (L, cells) and (ids == np.arange(cells)).all()
    cell_lo = aabbs[0, :3] + (np.array([3, 5, 7], F) / F(16)) * (aabbs[0, 3:] - aabbs[0, :3])
    p = pts[0, (3 * 16 + 5) * 16 + 7]
    assert (p >= cell_lo - 1e-6).all() and (p <= cell_lo + (aabbs[0, 3:] - aabbs[0, :3]) / 16 + 1e-6).all()
    assert eo.threshold(np.full(8, -1.0, F), 0.01)[0] == F(0.01)          # nothing visible: the cap


def test_camera_case_reaches_both_values_for_both_reasons():
    cam = eo.cameras()
    aabbs = eo.level_aabbs(eo.UPD_ROOT, eo.UPD_LEVELS)
    occs = eo.mark_invisible(cam["K"], cam["c2w"], cam["width"], cam["height"], cam["near_plane"], aabbs, eo.UPD_RES)
    assert set(np.unique(occs).tolist()) == {-1.0, 0.0} and 0.05 < (occs == 0).mean() < 0.95
    # camera 0 sits inside the root box: part of the box is behind it
    assert aabbs[0, 0] < 0.1 < aabbs[0, 3]
    # each camera alone sees cells, and the near-plane rule removes cells that a zero near plane would keep
    one = [eo.mark_invisible(cam["K"], cam["c2w"][i:i + 1], cam["width"], cam["height"], cam["near_plane"], aabbs, eo.UPD_RES) for i in (0, 1)]
    assert all((o == 0).any() and (o == -1).any() for o in one)
    no_near = eo.mark_invisible(cam["K"], cam["c2w"], cam["width"], cam["height"], 0.0, aabbs, eo.UPD_RES)
    assert ((no_near == 0) & (occs == -1)).sum() > 10
    # a cell both cameras see: one at a good depth, the other too near -> invisible
    both = (one[0] == 0) & (occs == -1)
    assert both.any()
