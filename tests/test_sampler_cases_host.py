"""CPU: the sampler cases of tests/sampler_cases.py reach what they name, the miss rule holds for every non-finite row, and the
fp32 definition the kernels are held to lies within a rounding-count bound of its float64 evaluation.
An assertion here fails when a case is edited so that it no longer reaches its edge."""
import numpy as np
import pytest
import torch

from oracle import field as of
from tests import sampler_cases as sc


@pytest.fixture(scope="module")
def marcher():
    return [(c, sc.march_full(c["o"], c["d"], c["jitter"], c["step"], c["bound"], c["grid"])) for c in sc.marcher_cases()]


def test_parameter_sets_are_the_issue_s():
    assert sc.CAPS == (1, 21, 63, 64, 65, 128, 129) and sc.JITTERS == (None, 0.0, float(np.nextafter(np.float32(1), np.float32(0))))
    assert sc.BELOW_ONE < 1.0 and np.float32(sc.BELOW_ONE) == np.float32(1) - np.float32(2.0 ** -24)
    assert sorted({g.shape[0] for g in sc.grids().values()}) == [1, 2, 3, 5, 128]
    assert [c["o"].shape[0] for c in sc.small_n_cases()] == [1, 3, 4, 5]
    assert sc.UNIFORM_S == (1, 2, 7, 255, 256, 257) and [h * w for h, w in sc.RAYGEN_SHAPES] == [255, 256, 257]
    assert all(c["o"].shape[0] <= 8 for c in sc.nonfinite_cases())
    g = sc.grids()
    assert g["full_R1"].all() and not g["empty_R2"].any() and int(g["single_R3"].sum()) == 1
    for name in ("random_R128", "random_R5"):                       # asymmetric: a transposed cell index reads another grid
        assert not torch.equal(g[name], g[name].transpose(0, 1)) and not torch.equal(g[name], g[name].transpose(1, 2))
        assert 0.2 < float(g[name].float().mean()) < 0.8
    assert not torch.equal(g["single_R3"], g["single_R3"].transpose(0, 1))


def test_count_rays_take_their_count_in_fp32_and_float64(marcher):
    """every prescribed step count is met by the fp32 oracle AND by the float64 evaluation, at every jitter; cap - 1, cap and
    cap + 1 occur for every cap, from inside, from a face and from outside"""
    seen = set()
    for c, m in marcher:
        if c["gname"] != "full_R1":
            continue
        want = c["want_steps"]
        got32 = m["n_steps"].numpy()
        got64 = sc.steps_f64(c["o"], c["d"], c["jitter"], c["step"], c["bound"])
        pres = want >= 0
        assert (got32[pres] == want[pres]).all() and (got64[pres] == want[pres]).all(), c["name"]
        assert (got32 == got64).all(), c["name"]                   # the specials too: no fp32 / float64 flip in the whole set
        assert (m["cnt"].numpy() == got32).all()                   # full grid: every step is kept
        seen |= {(int(n), nm.split("_")[1]) for n, nm in zip(want[pres], np.array(c["names"])[pres])}
        o, d = c["o"].numpy(), c["d"].numpy()
        inside = np.array([nm.endswith("_inside") and n > 0 for nm, n in zip(c["names"], want)])
        assert (np.abs(o[inside]) < c["bound"]).all()                                           # t_near = 0
        face = np.array([nm.endswith("_face") and n > 0 for nm, n in zip(c["names"], want)])
        assert (o[face][:, 2] == -np.float32(c["bound"])).all() and face.sum() == len(sc.COUNTS) - 1
    for cap in sc.CAPS:
        for e in (-1, 0, 1):
            for where in ("inside", "face", "outside"):
                assert (cap + e, where) in seen


def test_marcher_cases_reach_trips_overflow_halves_and_the_guard(marcher):
    trips, first_half, second_half_only, neither = set(), set(), set(), set()
    for c, m in marcher:
        for cap in c["caps"]:
            cnt, rows_s, rows_e, flag = sc.slot_expect(m, cap)
            over_n, over_w = sc.overflow_halves(m, cap)
            assert flag == int(bool(over_n.any() or over_w.any()))
            assert (cnt.long() == torch.minimum(m["cnt"], torch.tensor(cap))).all() or bool(over_w.any())
            trips |= {sc.trips(n, cap) for n in m["n_steps"].tolist()}
            if over_n.any():
                first_half.add((c["gname"], cap))
                # the LAST ray overflows on the full grid: a kernel without `pos < cap` writes into the guard row
                if c["gname"] == "full_R1":
                    assert bool(over_n[-1]) and c["names"][-1] == "long_diagonal"
                # ... and some overflowing ray is followed by one with room in its row: the surplus lands on sentinels
                nxt = over_n[:-1] & (cnt[1:] < cap)
                assert bool(nxt.any()) or cap == 1, (c["name"], cap)
            elif over_w.any():
                second_half_only.add((c["gname"], cap))
            else:
                neither.add((c["gname"], cap))
    assert {0, 1, 2, 3} <= trips
    # a row whose length is a multiple of 64 holds every step the loop walks: n > cap needs a partly used last trip
    assert {cap for g, cap in first_half if g == "full_R1"} == {cap for cap in sc.CAPS if cap % 64}
    assert {cap for g, cap in second_half_only if g == "full_R1"} == {64, 128}
    # the empty grid keeps nothing: only unwalked steps can set the flag, and they do at every cap (269 steps > 192 walked)
    assert {cap for g, cap in second_half_only if g == "empty_R2"} == set(sc.CAPS)
    assert not any(g == "empty_R2" for g, cap in first_half)
    # the single-cell grid at the long rows: no ray keeps more than cap, the flag comes from unwalked steps alone
    assert ("single_R3", 129) in second_half_only


def test_special_rays_are_what_they_are_named(marcher):
    c, m = next((c, m) for c, m in marcher if c["gname"] == "full_R1" and c["u"] == 0.0)
    n = dict(zip(c["names"], m["n_steps"].tolist()))
    for miss in ("points_away", "passes_beside", "edge_touch", "on_face_leaving"):
        assert n[miss] == 0, miss
    assert n["edge_thin"] == 2 and n["signed_zero_dir"] == 270 and n["long_diagonal"] == 270 and n["on_face_entering"] > 100
    assert n["face_graze_in"] == 270
    d = c["d"][c["names"].index("signed_zero_dir")].numpy()
    assert d[0] == 0 and not np.signbit(d[0]) and d[1] == 0 and np.signbit(d[1])
    # the grazing ray's z cell is R before the clamp, at R = 128 and R = 5: only `min(.., R - 1)` keeps it in the grid
    z, b = np.float32(sc.clamp_live_z()), np.float32(sc.BOUND)
    for R in (5, 128):
        assert int(np.floor((z + b) / (np.float32(2) * b) * np.float32(R))) == R
    # ... and the cell it must read differs from the one an unclamped index reads (the next row's first cell), somewhere
    g = sc.grids()["random_R128"]
    r = c["names"].index("face_graze_in")
    mm = next(m for cc, m in marcher if cc["gname"] == "random_R128" and cc["u"] == 0.0)
    assert 0 < int(mm["cnt"][r]) < 270                                                  # kept samples of the clamped index
    c1 = int(np.floor((np.float32(0.25) + b) / (np.float32(2) * b) * 128))
    rows = g[:, c1, 127].bool(), g[:, c1 + 1, 0].bool()                                 # clamped cell / unclamped cell, per x cell
    assert not torch.equal(rows[0], rows[1])


def test_small_n_and_nonfinite_cases():
    for c in sc.small_n_cases():
        m = sc.march_full(c["o"], c["d"], c["jitter"], c["step"], c["bound"], c["grid"])
        assert int(m["n_steps"][0]) == 270 and all(sc.slot_expect(m, cap)[3] == 1 for cap in c["caps"])
    for c in sc.nonfinite_cases():
        m = sc.march_full(c["o"], c["d"], c["jitter"], c["step"], c["bound"], c["grid"])    # returns: no OverflowError
        assert ((m["n_steps"].numpy() == 0) == c["miss"]).all(), c["name"]
        assert int(m["n_steps"][c["names"].index("plain_hit")]) in (269, 270)
        assert torch.isfinite(m["ts"]).all() and torch.isfinite(m["te"]).all()


def test_miss_rule_in_both_oracle_samplers():
    """every non-finite row is a miss: zero-width samples at t = 0 from the uniform sampler, none from the marcher; the d = 0
    row no longer raises; the issue's own example row is among them"""
    o, d, names, miss = sc.nonfinite_rows()
    assert names[0] == "nan_dir_x" and torch.isnan(d[0, 0]) and d[0, 1:].tolist() == [0.0, -1.0] and o[0].tolist() == [0.0, 0.0, 2.0]
    # what fmax / fmin arithmetic makes of that row: [0.99, 3.01] -- the behaviour the rule replaces
    b = np.float32(1.01)
    with np.errstate(all="ignore"):
        ta, tb = (-b - o.numpy()) / d.numpy(), (b - o.numpy()) / d.numpy()
    lo = np.fmax(np.fmax.reduce(np.fmin(ta, tb), -1), np.float32(0))          # the kernel starts from -inf / +inf
    hi = np.fmin(np.fmin.reduce(np.fmax(ta, tb), -1), np.float32(np.inf))
    assert abs(lo[0] - 0.99) < 1e-6 and abs(hi[0] - 3.01) < 1e-6 and np.isinf(hi[1]) and np.isinf(hi[2])
    for S in (1, 7):
        for u in sc.UNIFORM_JITTERS:
            ri, ts, te = of.uniform_samples(o, d, sc.jitter_tensor(u, 8), S, 1.01)
            ts, te = ts.view(8, S), te.view(8, S)
            assert (ts[miss] == 0).all() and (te[miss] == 0).all()
            assert (te[~miss] > ts[~miss]).all() and torch.isfinite(ts).all() and torch.isfinite(te).all()
    full = torch.ones(2, 2, 2, dtype=torch.uint8)
    ri, ts, te, n_steps, k = of.march_samples(o, d, None, 0.0075, 1.01, full, return_steps=True)
    assert set(ri.tolist()) == {3, 7} and (n_steps[miss] == 0).all()
    # the d = 0 row alone, and an all-miss batch: kmax meets no infinity and no empty maximum
    ri, ts, te = of.march_samples(o[2:3], d[2:3], None, 0.0075, 1.01, full)
    assert ri.numel() == 0
    # finite rays are untouched: a three-argument call returns what it always did
    assert len(of.march_samples(o[3:4], d[3:4], None, 0.0075, 1.01, full)) == 3


def test_retry_cases_double_as_often_as_claimed():
    by = {c["name"]: c for c in sc.retry_cases()}
    assert sc.RETRY_CAP == int(2.0 * 1.0 * 1.7320508075688772 / 0.2) + 4 == 21
    assert by["retry-third-full"]["caps_visited"] == [21, 42]                    # one doubling
    assert by["retry-tenth-full"]["caps_visited"] == [21, 42, 84, 168]           # several
    assert by["retry-tenth-empty"]["caps_visited"] == [21, 42, 84]               # unwalked steps alone
    assert by["retry-third-empty"]["caps_visited"] == [21]                       # 30 steps, all walked in the first trip: no retry
    for c in by.values():
        m, r = c["oracle"], c["scaled_ray"]
        steps = m["n_steps"].tolist()
        assert steps[r] == (30 if "third" in c["name"] else 100)
        assert all(0 < s <= sc.RETRY_CAP for i, s in enumerate(steps) if i != r)  # only the scaled ray overflows
        over_n, over_w = sc.overflow_halves(m, sc.RETRY_CAP)
        if c["name"].endswith("empty"):
            assert not over_n.any() and over_w.tolist() == [i == r and "tenth" in c["name"] for i in range(7)]
        else:
            assert over_n.tolist() == [i == r for i in range(7)]
        assert 2 * 7 * c["caps_visited"][-1] < 4096                              # the largest allocation: a few thousand floats


def test_pack_case_counts_and_capacities():
    c = sc.pack_case()
    m = sc.march_full(c["o"], c["d"], c["jitter"], c["step"], c["bound"], c["grid"])
    cnt = m["cnt"].tolist()
    assert tuple(cnt) == c["counts"] and {0, 1, 63, 64, 65, 129} == set(cnt) and c["total"] == sum(cnt) == 322
    assert {-(-n // 64) for n in cnt} == {0, 1, 2, 3}                            # trips of the pack kernel's loop
    assert all(cnt[i] == 0 for i in range(1, len(cnt), 2))                       # empty rays between
    ends = np.cumsum(cnt)
    caps = c["capacities"]
    assert caps["total"] == ends[-1] and caps["total-1"] == ends[-1] - 1 and caps["one"] == 1
    assert caps["ray-boundary"] in ends and caps["ray-boundary-before-empty"] == ends[0] == ends[1]
    assert caps["mid-ray"] not in ends and ends[3] < caps["mid-ray"] < ends[4]
    assert 1 < caps["below-first-ray"] < cnt[0]
    for name, cap in caps.items():
        start, cnt_c, n_valid, ovf = sc.capped_expect(m["cnt"], cap)
        assert int(cnt_c.sum()) == n_valid and bool((start + cnt_c <= cap).all()) and ovf == int(name != "total")
        assert torch.equal(start, torch.cumsum(cnt_c, 0) - cnt_c)                # ray_start stays the scan of ray_cnt
    from morpheus_amd import _lib                                                 # the slot row never overflows in this case
    assert _lib.load().mh_march_cap(c["step"], c["bound"]) > max(cnt)


def test_fp32_definition_within_rounding_count_of_float64(marcher):
    """ts / te of every kept sample of the finite cases against a float64 evaluation of the same formulas: 7 roundings on the
    longest path, each at most 2^-24 of a partial result (sampler_cases.march_f64 / uniform_f64 derive the bound)"""
    worst = 0.0
    for c, m in marcher:
        if c["gname"] not in ("full_R1", "random_R128"):
            continue
        ts64, te64, bound = sc.march_f64(c["o"], c["d"], c["jitter"], c["step"], c["bound"], m)
        for a32, a64 in ((m["ts"], ts64), (m["te"], te64)):
            err = np.abs(a32.numpy().astype(np.float64) - a64)
            assert (err <= bound).all(), (c["name"], float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
    so, sd, _ = sc.finite_specials()
    for S in sc.UNIFORM_S:
        for u in sc.UNIFORM_JITTERS:
            jit = sc.jitter_tensor(u, so.shape[0])
            ri, ts, te = of.uniform_samples(so, sd, jit, S, sc.BOUND)
            ts64, te64, bound, hit = sc.uniform_f64(so, sd, jit, S, sc.BOUND)
            assert hit.sum() >= 9
            for a32, a64 in ((ts, ts64), (te, te64)):
                err = np.abs(a32.view(-1, S).numpy().astype(np.float64) - a64)
                assert (err[hit] <= bound[hit]).all(), (S, u, float((err[hit] / bound[hit]).max()))
                assert (err[~hit] == 0).all()
                worst = max(worst, float((err[hit] / bound[hit]).max()))
    assert 0.0 < worst <= 1.0


def test_pixel_ray_restatement_and_pixel_sets():
    """the restatement against a float64 evaluation (5 roundings per direction component) and the pixel sets' claims"""
    for c in sc.raygen_cases():
        o, d = sc.pixel_rays(c["fx"], c["fy"], c["cx"], c["cy"], c["c2w"], c["H"], c["W"])
        assert c["fx"] != c["fy"] and c["cx"] != c["W"] / 2 and c["cy"] != c["H"] / 2
        R = c["c2w"][:3, :3].astype(np.float64)
        assert np.abs(R - np.eye(3)).min() > 0.05 and np.allclose(R @ R.T, np.eye(3), atol=1e-6)
        idx = np.arange(c["H"] * c["W"])
        cam = np.stack([((idx % c["W"]) + 0.5 - np.float64(np.float32(c["cx"]))) / c["fx"],
                        -((idx // c["W"]) + 0.5 - np.float64(np.float32(c["cy"]))) / c["fy"], -np.ones(len(idx))], -1)
        d64 = cam @ R.T
        mag = np.abs(cam) @ np.abs(R.T)
        assert (np.abs(d.numpy() - d64) <= 5 * sc.U * mag * (1 + 5 * sc.U)).all()
        assert (o.numpy() == c["c2w"][:3, 3]).all()
    for c in sc.fused_cases():
        pix = c["pix"]
        assert pix.max() == c["H"] * c["W"] - 1 and len(set(pix.tolist())) < len(pix) and pix.min() == 0
    assert {(c["H"], c["W"]) for c in sc.fused_cases()} >= {(1, 7), (7, 1)}
    sets = sc.uniform_ray_sets()
    assert sets["N1"][0].shape[0] == 1 and sets["N3"][0].shape[0] == 3
    for S in (255, 256, 257):
        assert {(1 * S + 255) // 256, (3 * S + 255) // 256} <= {1, 2, 3, 4}
    assert (1 * 255 + 255) // 256 == 1 and (1 * 257 + 255) // 256 == 2 and (3 * 257 + 255) // 256 == 4
    for name in ("N1", "N3"):                                                    # the sliced rays all hit
        o, d = sets[name]
        ri, ts, te = of.uniform_samples(o, d, sc.jitter_tensor(0.0, o.shape[0]), 2, sc.BOUND)
        assert (te > ts).all()


# capacity -> (start, cnt_c) for the counts [3, 0, 5, 2] (exclusive scan [0, 3, 3, 8], total 10), written out from the
# definition: start = min(exclusive scan, capacity), cnt_c = min(cnt, capacity - start)
CAPPED_WANT = {
    1: ([0, 1, 1, 1], [1, 0, 0, 0]),        # the cut falls inside the first ray
    3: ([0, 3, 3, 3], [3, 0, 0, 0]),        # on a ray boundary, an empty ray behind it
    4: ([0, 3, 3, 4], [3, 0, 1, 0]),        # inside the third ray
    10: ([0, 3, 3, 8], [3, 0, 5, 2]),       # exactly the total
    11: ([0, 3, 3, 8], [3, 0, 5, 2]),       # above the total
}


@pytest.mark.parametrize("capacity", sorted(CAPPED_WANT))
def test_fixed_capacity_bookkeeping(capacity):
    """ops.capped_ranges, the one place the fixed-capacity marches (march_rays_capped, est_march_rays with a capacity) clamp the
    ray ranges: on CPU tensors, against values written out above"""
    from morpheus_amd import ops
    cnt, total = torch.tensor([3, 0, 5, 2], dtype=torch.int32), 10
    excl = [0, 3, 3, 8]
    want_start, want_cnt = CAPPED_WANT[capacity]
    assert want_start == [min(e, capacity) for e in excl]
    start, cnt_c, n_valid, overflow = ops.capped_ranges(cnt, torch.tensor(0, dtype=torch.int32), capacity)
    assert start.dtype == cnt_c.dtype == overflow.dtype == torch.int32
    assert start.tolist() == want_start and cnt_c.tolist() == want_cnt
    assert all(s + c <= capacity for s, c in zip(start.tolist(), cnt_c.tolist()))
    for r, e in enumerate(excl):
        if e >= capacity:                                          # a ray behind the cut
            assert start[r] == capacity and cnt_c[r] == 0
    assert int(n_valid) == min(total, capacity) and n_valid.dim() == 0
    assert int(overflow) == int(total > capacity) and overflow.dim() == 0
    assert cnt.tolist() == [3, 0, 5, 2]                            # the counts are not written


def test_fixed_capacity_overflow_carries_the_slot_row_flag():
    from morpheus_amd import ops
    cnt = torch.tensor([3, 0, 5, 2], dtype=torch.int32)
    start, cnt_c, n_valid, overflow = ops.capped_ranges(cnt, torch.tensor(1, dtype=torch.int32), 11)
    assert int(overflow) == 1 and int(n_valid) == 10
    assert start.tolist() == CAPPED_WANT[11][0] and cnt_c.tolist() == CAPPED_WANT[11][1]
