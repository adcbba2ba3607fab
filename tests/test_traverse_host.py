"""`OccGridEstimator(traversal="dda")`, everything that needs no GPU: the restatement (tests/traverse_oracle.py) reaching what every
case of tests/test_gpu_traverse.py names, its samples in order and disjoint, the float64 judge (every sample's midpoint in an
occupied cell), the coverage of every run, the attribute and its refusals, and the C ABI of mh_est_traverse_slots.

Coverage bound.  Behind its last sample a run goes on for at most half of the step that the NEXT sample would have had: that one's
midpoint te_last + dt_next / 2 is the first not before B.  With cone_angle == 0 dt_next is dt_last (both are `step`) and the bound
asserted is B - te_last <= dt_last / 2.  With cone steps dt_next = min(max(te_last * cone_angle, step), 1e10) exceeds dt_last by up
to the factor 1 + cone_angle once the steps grow, so by the definition itself a run may pass dt_last / 2 by that much: of the 244
runs of `levels3-cone` one does (B - te_last = 0.50295 dt_last; te_last = 2.17604, dt_last = 0.021545, dt_next = 0.021760,
cone_angle = 0.01), none of `rand40-cone`.  For cone steps dt_next / 2 is what is asserted.
"""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import estimator_oracle as eo
from tests import sampler_cases as sc
from tests import traverse_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CASES = to.cases()


@pytest.fixture(scope="module")
def ran():
    return {c["name"]: (c, to.run_case(c)) for c in CASES + [to.overflow_case()]}


def _per_ray(c, m):
    ri = m["ri"].numpy()
    return {nm: (m["ts"].numpy()[ri == i], m["te"].numpy()[ri == i]) for i, nm in enumerate(c["names"])}


def _occupied(m, r, i, bn):
    s, e, l, c = m["spans"][r][i]
    return e > s and bn[l, c[0], c[1], c[2]] != 0


# ------------------------------------------------------------------------------------------------------ what the cases reach
def test_cases_are_small_and_complete(ran):
    assert [c["name"] for c in CASES] == ["full8", "rand40", "levels3", "degenerate", "planes", "rand40-cone", "levels3-cone", "empty"]
    for c, m in ran.values():
        assert len(c["names"]) == m["N"] <= 64 and len(set(c["names"])) == m["N"], c["name"]
        assert (int(m["cnt"].sum()) > 0) == (c["name"] != "empty"), c["name"]


def test_full8_one_run_a_ray_and_several_writer_rounds(ran):
    c, m = ran["full8"]
    assert all(len(runs) == 1 for runs in m["runs"])
    cnt = dict(zip(c["names"], m["cnt"].tolist()))
    assert cnt["corner"] > 128 and cnt["corner_back"] > 128 and min(cnt.values()) > 64          # three rounds / two at least
    # a run's samples are te_k == ts_{k+1}, the same bits
    ts, te = _per_ray(c, m)["corner"]
    assert ts[1:].tobytes() == te[:-1].tobytes()


def test_rand40_trip_boundary(ran):
    """more than 64 spans a diagonal ray; at spans 63 / 64 (the last of the first trip, the first of the second): a run open across,
    a run that ends with span 63, a run that starts with span 64, and both empty"""
    c, m = ran["rand40"]
    bn = to.grid_rand40()[1].numpy()
    assert 0.3 < bn.mean() < 0.4
    long_rays = [r for r in range(m["N"]) if len(m["spans"][r]) > 65]
    assert len(long_rays) >= 8 and max(len(s) for s in m["spans"]) < 128
    kinds = set()
    for r in long_rays:
        sp = m["spans"][r]
        if not (sp[63][1] > sp[63][0] and sp[64][1] > sp[64][0]):
            continue
        a, b = _occupied(m, r, 63, bn), _occupied(m, r, 64, bn)
        kinds.add((bool(a), bool(b)))
        if a and b:
            assert any(f <= 63 and l >= 64 for _, _, f, l in m["runs"][r])
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    # many short runs: several runs end inside one trip
    assert max(len(runs) for runs in m["runs"]) > 10
    _, mc = ran["rand40-cone"]
    assert int(mc["cnt"].sum()) > 300 and mc["spans"] == m["spans"]


def test_levels3_reaches_level_changes(ran):
    c, m = ran["levels3"]
    aabbs = to.grid_levels3()[0].numpy()
    by = dict(zip(c["names"], range(m["N"])))
    lv = lambda r: [s[2] for s in m["spans"][r] if s[1] > s[0]]
    # a ray that starts inside level 0: no descent, its first span is level 0's
    for nm in ("inside_l0", "inside_l0_neg"):
        seq = lv(by[nm])
        assert seq[0] == 0 and 1 in seq and seq[-1] == 2 and seq == sorted(seq), nm
    # a ray that misses level 0 (and level 1) but crosses level 2
    assert set(lv(by["misses_l0"])) == {2} and int(m["cnt"][by["misses_l0"]]) > 0
    assert set(lv(by["misses_l0_l1_oblique"])) == {2}
    assert set(lv(by["through_l1"])) == {1, 2} and lv(by["through_all"])[0] == 2 and 0 in lv(by["through_all"])
    # descending and ascending through every level
    seq = lv(by["through_all"])
    assert [k for k, _ in __import__("itertools").groupby(seq)] == [2, 1, 0, 1, 2]
    # runs that continue across a level change, in both directions
    down = up = 0
    for r in range(m["N"]):
        sp = m["spans"][r]
        for _, _, f, l in m["runs"][r]:
            levels = [sp[i][2] for i in range(f, l + 1) if sp[i][1] > sp[i][0]]
            down += any(x > y for x, y in zip(levels, levels[1:]))
            up += any(x < y for x, y in zip(levels, levels[1:]))
    assert down >= 3 and up >= 3
    # the segment boundaries are monotone and stay inside [t_near, t_far]
    T = m["T"]
    assert (np.diff(T, axis=1) >= 0).all() and T.shape == (m["N"], 6)
    assert float(aabbs[0, 0]) == 0.25


def test_degenerate_directions(ran):
    c, m = ran["degenerate"]
    by = dict(zip(c["names"], range(m["N"])))
    d = c["d"].numpy()
    assert [(d[by[nm]] == 0).sum() for nm in ("one_zero", "one_zero_neg", "two_zero_x", "two_zero_y_neg", "two_zero_z")] == [1, 1, 2, 2, 2]
    for nm in ("one_zero", "one_zero_neg", "two_zero_x", "two_zero_y_neg", "two_zero_z"):
        r = by[nm]
        cells = np.array([s[3] for s in m["spans"][r]])
        for a in np.nonzero(d[r] == 0)[0]:                                  # that axis is never stepped inside a level
            for l in range(3):
                sel = np.array([s[2] for s in m["spans"][r]]) == l
                assert len(set(cells[sel, a].tolist())) <= 1, (nm, a, l)
        assert int(m["cnt"][r]) > 0, nm
    # the existing miss rule: a ray in a face plane of the coarsest box, a ray leaving from a face
    for nm in ("in_face_plane", "on_face_leaving"):
        assert len(m["spans"][by[nm]]) == 0 and int(m["cnt"][by[nm]]) == 0, nm
    # through an edge: two exits tie and a span of no width appears; it neither breaks nor extends a run
    ties = {nm: sum(1 for s in m["spans"][by[nm]] if not (s[1] > s[0])) for nm in ("through_edge", "through_l0_edge", "through_corner")}
    assert all(v >= 1 for v in ties.values()), ties
    assert ties["through_corner"] >= 2
    # negative directions on every axis
    assert (d[by["all_negative"]] < 0).all() and int(m["cnt"][by["all_negative"]]) > 0
    assert int(m["cnt"][by["neg_x"]]) > 0 and int(m["cnt"][by["neg_yz"]]) > 0


def test_planes_and_limits(ran):
    c, m = ran["planes"]
    per = _per_ray(c, m)
    us = {"0.00": 0.0, "0.37": to.U, "1.00": sc.BELOW_ONE}
    assert sorted(set(c["jitter"].tolist())) == sorted(float(F(u)) for u in us.values())
    full = to.traverse(c["o"], c["d"], c["jitter"], c["step"], to.grid_levels3()[0], torch.ones(3, 8, 12, 16, dtype=torch.uint8),
                       0.0, c["near_plane"], c["far_plane"], c["t_min"], c["t_max"])
    pf = _per_ray(c, full)
    for tag, u in us.items():
        # the planes cut a cell in two: the first span starts at near_plane + u * step, inside a cell, and the last ends at far_plane
        for nm in (f"planes_only_u{tag}", f"planes_only_oblique_u{tag}"):
            r = c["names"].index(nm)
            sp = full["spans"][r]
            first = F(F(c["near_plane"]) + F(u) * F(c["step"]))
            assert sp[0][0] == first and sp[-1][1] == F(c["far_plane"]) and pf[nm][0][0] == first
        r = c["names"].index(f"planes_only_u{tag}")                          # +z through the root box: z = -1.75 + t
        z0 = -1.75 + float(full["spans"][r][0][0])
        cell = (z0 + 1.25) / (4.0 / 16)                                      # level 2: z in [-1.25, 2.75], 16 cells
        assert 0.05 < cell - np.floor(cell) < 0.95
        assert len(per[f"tmax_lt_tmin_u{tag}"][0]) == 0 and len(pf[f"tmax_lt_tmin_u{tag}"][0]) == 0
        assert pf[f"tmin_raises_u{tag}"][0][0] == F(F(1.93) + F(u) * F(c["step"]))
        ts, te = pf[f"tmax_cuts_u{tag}"]
        assert (ts + te).max() / 2 < F(2.31) and te.max() > F(2.31) - F(c["step"])
        assert len(per[f"planes_only_u{tag}"][0]) > 0
    # the three jitters give three different placements of the same ray
    a, b, cc = (pf[f"planes_only_u{tag}"][0] for tag in us)
    assert a[0] < b[0] < cc[0] <= a[1]                                    # u below one: within an ulp of a whole step


def test_empty_and_overflow_cases(ran):
    c, m = ran["empty"]
    assert int(m["cnt"].sum()) == 0 and all(len(s) > 0 for s in m["spans"]) and all(len(r) == 0 for r in m["runs"])
    c, m = ran["overflow"]
    cnt = dict(zip(c["names"], m["cnt"].tolist()))
    cap = c["cap"]
    assert cap == int(np.sqrt(12.0) / 0.05) + 4 == 73
    assert cap < cnt["scaled"] <= 2 * cap and max(cnt["unit"], cnt["oblique"]) <= cap
    assert sc.slot_expect(m, cap)[3] == 1 and sc.slot_expect(m, 2 * cap)[3] == 0
    want_cnt, rows_s, _, _ = sc.slot_expect(m, cap)
    assert want_cnt.tolist() == [cap, cnt["unit"], cnt["oblique"]] and float(rows_s[0, cap - 1]) != sc.SENTINEL


# ---------------------------------------------------------------------------------------------------------- the properties
@pytest.mark.parametrize("name", [c["name"] for c in CASES] + ["overflow"])
def test_samples_are_ordered_and_disjoint(ran, name):
    c, m = ran[name]
    ri, ts, te = m["ri"].numpy(), m["ts"].numpy(), m["te"].numpy()
    assert (np.diff(ri) >= 0).all() and (te > ts).all()
    same = ri[1:] == ri[:-1]
    assert (ts[1:] >= te[:-1])[same].all()
    assert (te - ts >= F(c["step"]) * F(0.999)).all()
    # every ts lies in [t_near, t_far): what lets mh_est_march_cap bound the slot row
    T = m["T"]
    assert (ts >= T[ri, 0]).all() and (ts < T[ri, -1]).all()
    assert torch.equal(m["n_steps"], m["cnt"]) and (m["k"].numpy() == np.concatenate([np.arange(n) for n in m["cnt"].tolist()] or [np.zeros(0)])).all()


def test_the_recalled_rule_overlaps_and_the_departure_does_not(ran):
    """restarting every run at its own entry (the recalled rule) makes samples overlap behind a gap shorter than half a step"""
    c, m = ran["rand40"]
    rec = to.recalled_samples(c["o"], c["d"], c["jitter"], c["step"], *to.grid_rand40())
    overlaps = sum(int((ts[1:] < te[:-1]).sum()) for ts, te in rec)
    assert overlaps > 0
    # and the departure only ever delays a run's first sample
    late = 0
    for r, runs in enumerate(m["runs"]):
        sel = m["ri"].numpy() == r
        for q, (A, B, _, _) in enumerate(runs):
            ts = m["ts"].numpy()[sel][m["run_of"][sel] == q]
            late += int(ts.size > 0 and ts[0] > A)
            assert ts.size == 0 or ts[0] >= A
    assert late > 0


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["name"] != "empty"])
def test_float64_judge(ran, name):
    c, m = ran[name]
    outside, aside, total = to.judge(m, c["o"], c["d"], *to.GRIDS[c["grid"]]())
    print(f"{name}: {total} samples, {outside} outside, {aside} set aside")
    assert total > 0 and outside == 0
    assert aside <= 0.01 * total


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["name"] != "empty"])
def test_coverage_of_every_run(ran, name):
    c, m = ran[name]
    late, short, short_last, n = to.coverage(m, c["step"], c["cone_angle"])
    print(f"{name}: {n} runs with samples, {late} late starts, {short} past dt_next / 2, {short_last} past dt_last / 2")
    assert n > 0 and late == 0 and short == 0
    if c["cone_angle"] == 0:
        assert short_last == 0


# ------------------------------------------------------------------------------------------------------- attribute and ABI
def test_traversal_attribute_and_refusals():
    from morpheus_amd._lib import MorpheusHipError
    from morpheus_amd.estimator import OccGridEstimator
    e = OccGridEstimator([0, 0, 0, 1, 1, 1], 4)
    before = list(e.state_dict())
    assert e.traversal == "lattice"
    e.traversal = "dda"
    assert e.traversal == "dda" and list(e.state_dict()) == before == ["resolution", "aabbs", "occs", "binaries"]
    for bad in ("DDA", "", None, 1, "grid"):
        with pytest.raises(ValueError, match="traversal"):
            e.traversal = bad
        assert e.traversal == "dda"
    o, d = torch.zeros(2, 3), torch.ones(2, 3)
    with pytest.raises(ValueError, match="traversal"):
        e.sampling_as("nerfacc", o, d)
    for tr in ("lattice", "dda"):
        with pytest.raises(MorpheusHipError, match="no CPU path"):
            e.sampling_as(tr, o, d)
        assert e.traversal == "dda"                                          # one call only
    with pytest.raises(MorpheusHipError, match="no CPU path"):
        e.sampling(o, d)
    # a fresh estimator loads the state of one that traverses and stays on the lattice: the placement is not state
    f = OccGridEstimator([0, 0, 0, 1, 1, 1], 4)
    f.load_state_dict(e.state_dict())
    assert f.traversal == "lattice"
    # the signature of sampling stays the recalled one
    assert "traversal" not in inspect.signature(OccGridEstimator.sampling).parameters


def test_c_abi():
    from morpheus_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "morpheus_hip.h")).read()
    lib = _lib.load()
    assert len(re.findall(r"\bmh_est_traverse_slots\s*\(", hdr)) == 1 and "mh_est_traverse_slots" in _lib.EXPORTS
    assert re.search(r"int mh_est_march_slots\((.*?)\);", hdr, re.S).group(1).split() == \
        re.search(r"int mh_est_traverse_slots\((.*?)\);", hdr, re.S).group(1).split()
    assert inspect.signature(ops.est_traverse_rays) == inspect.signature(ops.est_march_rays)
    args = lambda **kw: [kw.get("N", 3), kw.get("step", 0.01), kw.get("cone", 0.0), kw.get("near", 0.0), kw.get("far", 1e10), None,
                         kw.get("L", 1), 4, 4, kw.get("Rz", 4), None, kw.get("cap", 8), None, None, None, None, None]
    for fn in (lib.mh_est_march_slots, lib.mh_est_traverse_slots):             # the same argument rules, before any launch
        assert fn(*([None] * 5), *args(N=0)) == 0
        for kw in ({}, {"N": -1}, {"step": 0.0}, {"cone": -0.1}, {"cone": float("nan")}, {"near": float("nan")}, {"far": float("nan")},
                   {"L": 0}, {"L": 17}, {"Rz": 0}, {"cap": 0}):
            assert fn(*([None] * 5), *args(**kw)) == 1, kw
    src = open(os.path.join(ROOT, "morpheus_amd", "csrc", "estimator.hip")).read()
    assert "est_traverse_kernel" in src and src.count("extern \"C\" int32_t mh_est_march_cap") == 1 and "traverse_cap" not in src
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "mh_est_traverse_slots" in design[design.index("## 7j."):]
