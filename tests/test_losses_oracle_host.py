"""tests/losses_f64_oracle.py on the CPU: the conditions tests/test_gpu_losses_f64.py relies on.  Every case builder is run here and
shown to deliver the sizes, trip counts and values it names; the fp32 restatement passes the judgement the kernels will face (judged
against itself, so only the floors, the exact-zero rules and finiteness bite); deliberately wrong restatements fail it."""
import numpy as np
import pytest
import torch

from tests import losses_f64_oracle as L

F32, F64 = torch.float32, torch.float64


def _count(t, v):
    return int((t == torch.tensor(v, dtype=F32)).sum())


# =========================================================================================================== masked mean
def test_mean_block_and_trip_counts_from_the_constants():
    """one partial block, the wave and block tails, the second block, the cap of 512 blocks and the first element of the fifth trip"""
    assert (L.MEAN_BLOCKS, L.MEAN_THREADS, L.POSE_RAYS_PER_BLOCK) == (512, 256, 1024)
    want = {1: (1, 1), 255: (1, 1), 256: (1, 1), 257: (1, 2), 1024: (1, 4), 1025: (2, 3), 2049: (3, 3), 524288: (512, 4), 524289: (512, 5)}
    assert tuple(want) == L.MEAN_M_C1
    for n, (blocks, trips) in want.items():
        assert (L.mean_blocks(n), L.mean_trips(n)) == (blocks, trips), n
    assert 524288 == L.MEAN_BLOCKS * 4 * L.MEAN_THREADS, "the cap is reached exactly, then exceeded by one element"
    # C = 3: the same element counts n = 3 M, with rows that straddle the wave, trip and block edges
    assert [3 * M for M in L.MEAN_M_C3] == [3, 255, 258, 1026, 524289]
    assert [L.mean_blocks(3 * M) for M in L.MEAN_M_C3] == [1, 1, 1, 2, 512] and L.mean_trips(258) == 2 and L.mean_trips(524289) == 5
    assert 255 // 3 == 256 // 3 == 257 // 3 == 85, "row 85 holds elements 255 .. 257: it straddles the edge at 256"
    # eikonal walks rows, not elements
    assert L.mean_blocks(174763) == 171 and L.mean_depth("eikonal", 174763, 3, False) == 4 + 6 + 3 + 1 + 9 + 1 + 8
    # the derived depth: trips + 6 + 3 + (ceil(blocks / 256) + 9) + the division + the term
    assert L.mean_depth("identity", 524289, 1, False) == 5 + 6 + 3 + 2 + 9 + 1
    assert L.mean_depth("sqdiff", 1, 1, True) == 2 * (1 + 6 + 3 + 1 + 9) + 1 + 2 + 2


@pytest.mark.parametrize("kind,C", [(k, 1) for k in L.MEAN_KINDS if k != "eikonal"] + [(k, 3) for k in L.MEAN_C3_KINDS])
def test_mean_cases_reach_their_edges_and_the_restatement_passes(kind, C):
    cases = L.mean_cases(kind, C)
    sizes = L.MEAN_M_C1 if C == 1 else L.MEAN_M_C3
    assert {c["M"] for c in cases} == set(sizes)
    for M in sizes:
        modes = {(c["n_valid"] is not None, c["w"] is not None) for c in cases if c["M"] == M}
        assert modes == {(False, False), (True, False), (False, True), (True, True)}, "all rows, n_valid, row_weight, both"
    for M in L.MEAN_FULL_M[C]:
        assert {c["n_valid"] for c in cases if c["M"] == M} >= {0, 1, M - 1, M, M + 5, -3}
        assert {c["n_valid"] for c in cases if c["M"] == M and c["w"] is not None} >= {0, 1, M - 1, M, M + 5, -3}
        assert {c["weights"] for c in cases if c["M"] == M} == {None, "01", "nonint", "tiny", "zero"}
    for c in cases:
        M, a, w = c["M"], c["a"], c["w"]
        r = M if c["n_valid"] is None else min(max(c["n_valid"], 0), M)
        assert bool(torch.isnan(a[r:]).all()) and bool(torch.isfinite(a[:r]).all()), "NaN exactly behind n_valid"
        if w is not None and c["n_valid"] is not None:
            assert bool(torch.isnan(w[r:]).all())
        if c["b"] is not None:
            assert bool(torch.isnan(c["b"][r:]).all())
        r64, r32 = L.mean_run(c, F64), L.mean_run(c, F32)
        L.mean_check(c, r32, r32, r64)
        assert bool((r64["ga"].reshape(M, -1)[r:] == 0).all())
        den = float(r64["den"])
        if c["weights"] == "tiny":
            assert den == 1.0 and float(w.double().sum()) * c["per_row"] < 1.0, "the weighted denominator clamps to 1"
        if c["weights"] == "zero":
            assert float(r64["value"]) == 0.0 and bool((r64["ga"] == 0).all()) and float(r32["value"]) == 0.0
        if c["weights"] == "nonint":
            assert bool((w[:r] != w[:r].round()).any()) or r == 0
        if r == 0:
            assert float(r64["value"]) == 0.0 and den == (1.0 if w is not None else c["per_row"])
        full = M >= 255 and r >= M - 1
        if kind == "entropy" and full:
            flat = a.reshape(-1)
            for v in L.ENTROPY_EDGES:
                assert _count(flat, v) >= 1, v
            assert _count(flat, L.LO) == 1 and _count(flat, L.HI) == 1
            assert L._next(L.LO, 0.0) < L.LO < L._next(L.LO, 1.0) and L._next(L.HI, 0.0) < L.HI < L._next(L.HI, 1.0) < 1.0
            g = r64["ga"].reshape(-1)
            on = (flat == L.LO) | (flat == L.HI)
            if w is None or c["weights"] == "nonint":
                assert bool((g[on] != 0).all()) or bool((w[:2] == 0).any()), "the clamp passes the gradient AT its bounds"
            outside = (flat < L.LO) | (flat > L.HI)
            assert int(outside.sum()) >= 4 and bool((g[outside] == 0).all())
            if w is None:
                assert float(r64["abs_mean"]) > 0.1, "the mean term the entropy term count relies on"
        if kind in ("abs", "absdiff") and full:
            z = (a == 0) if c["b"] is None else (a == c["b"])
            assert int(z.sum()) >= 3 and bool((r64["ga"][z] == 0).all()), "exact zeros / a == b: sign(0) = 0"
        if kind == "eikonal" and r >= 4:
            assert bool((a[0] == 0).all()) and float(a[1].double().norm()) == 1.0 and float(a[2].double().norm()) == 1.0
            assert bool((r64["ga"][:3] == 0).all()) and bool((r32["ga"][:3] == 0).all())


def test_mean_of_empty_tensors():
    for kind in L.MEAN_KINDS:
        c = L.mean_empty_case(kind)
        assert tuple(c["a"].shape) == ((0, 3) if kind == "eikonal" else (0,))
        r64 = L.mean_run(c, F64)
        assert float(r64["value"]) == 0.0 and r64["ga"].numel() == 0 and tuple(r64["ga"].shape) == tuple(c["a"].shape)


def _fails(fn):
    with pytest.raises(AssertionError):
        fn()


def test_wrong_mean_restatements_fail_the_judgement():
    def attempt(case, wrong):
        r64, r32 = L.mean_run(case, F64), L.mean_run(case, F32)
        L.mean_check(case, r32, r32, r64)                                         # (the right one passes)
        _fails(lambda: L.mean_check(case, L.mean_run(case, F32, wrong=wrong), r32, r64))

    attempt(L.mean_case("absdiff", 86, 3, weights="nonint"), "weights_per_channel")
    attempt(L.mean_case("abs", 342, 3, weights="01"), "weights_per_channel")
    attempt(L.mean_case("square", 257, 1, n_valid=257 + 5), "n_valid_unclamped")
    attempt(L.mean_case("entropy", 257, 1), "clamp_gt")
    attempt(L.mean_case("identity", 257, 1, weights="tiny"), "den_no_max")
    attempt(L.mean_case("eikonal", 86, 3, weights="tiny"), "den_no_max")


# ========================================================================================================= ortho perturb
def test_ortho_cases_hold_every_edge_normal_and_the_restatement_passes():
    names = {name for name, _ in L.ORTHO_EDGES}
    seen, phis = set(), set()
    pools = {scale: [] for scale in L.ORTHO_SCALES}
    for M in L.ORTHO_M:
        c = L.ortho_case(M)
        here = {e for e in c["edge"] if e}
        seen |= here
        if M >= 63:
            assert here == names
            assert int(c["u_zero"].sum()) == 5
            lengths = c["n"][len(names):].double().norm(dim=-1)
            assert M < 255 or (float(lengths.min()) < 1e-2 and float(lengths.max()) > 1e2), "random normals at lengths 1e-3 .. 1e3"
        phis |= {float(c["phi"][i]) for i, e in enumerate(c["edge"]) if e}
        assert bool((c["x"][1::2] == 0).all()) and (M < 2 or bool((c["x"][0::2] != 0).any()))
        assert float(L.ortho_condition(c["n"], c["phi"], c["g"]).max()) <= L.ORTHO_MAX_CONDITION, "no row's projections cancel beyond the bound"
        for scale in L.ORTHO_SCALES:
            r64, r32 = L.ortho_run(c, scale, F64), L.ortho_run(c, scale, F32)
            assert bool(torch.isfinite(r32["gn"]).all()) and bool(torch.isfinite(r64["gn"]).all())
            L.ortho_check(c, scale, dict(out=r32["out"], gn=r32["gn"], gx=r32["gx"]), r32, r64, f"M={M} scale={scale}", pool=pools[scale])
            for i, e in enumerate(c["edge"]):
                if e in ("zero", "u = 0, +z", "u = 0, length 5"):
                    assert float(r64["gn"][i].abs().max()) > 1e9 * abs(scale) * float(c["g"][i, :2].abs().max()) * 0.01, "the degenerate rows' huge g_n"
    for scale, pool in pools.items():
        assert sum(p[0].numel() for p in pool) == 3 * sum(L.ORTHO_M)
        L.ortho_judge_pool(pool, f"all sizes, scale={scale}")
    assert seen == names and phis == {float(np.float32(p)) for p in L.ORTHO_PHI}
    c = L.ortho_case(257)
    below = c["n"][[i for i, e in enumerate(c["edge"]) if e and e.startswith("below")]]
    assert below.shape[0] == 2 and float(below.double().norm(dim=-1).max()) < 1e-12 and float(below.abs().max()) > 0
    # a wrong degenerate branch is seen: g_n of the u = 0 rows projected as if the clamp were not there
    r64, r32 = L.ortho_run(c, 1.0, F64), L.ortho_run(c, 1.0, F32)
    bad = r32["gn"].clone()
    bad[c["u_zero"]] = 0.0
    _fails(lambda: L.ortho_check(c, 1.0, dict(out=r32["out"], gn=bad, gx=r32["gx"]), r32, r64, "wrong"))


# ============================================================================================================ pose apply
def test_pose_cases_and_counts():
    assert [L.ceil_div(n, L.POSE_RAYS_PER_BLOCK) for n in L.POSE_N] == [1, 1, 1, 1, 1, 1, 1, 1, 2, 3]
    assert [L.ceil_div(min(n, 1024), 256) for n in L.POSE_N] == [1, 1, 1, 1, 1, 2, 4, 4, 4, 4]
    assert L.pose_count(2049, 3) == 4 + 6 + 3 + 3 + 3 + 19
    assert [f.count(max(f, key=f.count)) for f in L.POSE_FRAMES] == [1, 1, 2, 2, 3]
    assert L.POSE_FRAMES[2] == [4, 7, 4], "non-adjacent rows of one frame"
    c = L.pose_case(64, [4, 7, 4])
    assert bool((c["pose"][L.POSE_ZERO_FRAME] == 0).all()) and float(c["pose"][:, :3].abs().max()) > 2.5 and c["pose"].shape == (L.POSE_F, 6)
    assert float(c["pose"][:, :3].abs().max()) <= 3.0


@pytest.mark.parametrize("frames", L.POSE_FRAMES, ids=str)
def test_pose_restatement_passes_and_overwriting_rows_fails(frames):
    for n in L.POSE_N:
        c = L.pose_case(n, frames)
        r64, r32 = L.pose_run(c, F64), L.pose_run(c, F32)
        L.pose_check_forward(c, r32["o1"], r32["d1"], r32, r64)
        floor = L.pose_forward_floor(c, r64)
        assert L.POSE_FORWARD_ROUNDINGS * L.U <= floor <= L.POSE_MAX_CANCELLATION * L.POSE_FORWARD_ROUNDINGS * L.U, "entries of R cancel within the bound"
        for mode in L.POSE_MODES:
            L.pose_check_grad(c, mode, r32["grads"][mode], r32, r64)
            g = r64["grads"][mode]
            assert bool((g[:, :3] == 0).all()) == (mode == "o") and bool((g[:, 3:] == 0).all()) == (mode == "d")
        zero_rows = [r for r, f in enumerate(frames) if f == L.POSE_ZERO_FRAME]
        for r in zero_rows:
            assert torch.equal(r64["R"][r], torch.eye(3, dtype=F64)) and bool((r64["t"][r] == 0).all())
    if len(set(frames)) < len(frames):
        c = L.pose_case(257, frames)
        r64, r32 = L.pose_run(c, F64), L.pose_run(c, F32)
        wrong = L.pose_run(c, F32, wrong="pose_overwrite")
        _fails(lambda: L.pose_check_grad(c, "both", wrong["grads"]["both"], r32, r64))


# =========================================================================================================== render loss
def _render_weights():
    from morpheus_amd import harness
    tr = harness.load_config()["train"]
    return dict(L.RENDER_WEIGHTS, config=(float(tr["rgb_weight"]), float(tr["mask_weight"]), float(tr["depth_weight"])))


def test_render_cases_hold_their_edges():
    assert [max(L.ceil_div(N, 1024), 1) for N in L.RENDER_N] == [1, 1, 1, 1, 1, 1, 2, 3, 3] and L.RENDER_EDGE_RAYS == 26
    assert L.RENDER_WEIGHTS["no mask"][1] == 0.0 and all(w > 0 for w in _render_weights()["config"])
    for N in L.RENDER_N:
        c = L.render_case(N)
        assert all(c[k].shape[0] == N for k in ("pred_rgb", "pred_depth", "opacity", "depth", "mask", "bg", "o", "d")) and c["image"].shape == (3, N)
        v32 = L.render_valid32(c)
        near = L.render_near_radius(c)
        placed = sorted(c["placed"].values())
        assert int(near.sum()) <= 3 and torch.nonzero(near).reshape(-1).tolist() == placed, "only the placed rays lie within an ulp of the radius"
        if N >= 1:
            i = c["placed"]["on"]
            rad = L.radius32(c["o"], c["d"], c["depth"])
            assert float(rad[i]) == L.RADIUS and float(v32[i]) == 1.0, "exactly on the radius in fp32: <= holds"
            assert float(L.render_valid32(c, wrong="valid_lt")[i]) == 0.0
        if N < 63:
            continue
        rad = L.radius32(c["o"], c["d"], c["depth"])
        assert [float(rad[c["placed"][k]]) for k in ("on", "under", "over")] == [L.RADIUS, L._R_UNDER, L._R_OVER]
        assert [float(v32[c["placed"][k]]) for k in ("on", "under", "over")] == [1.0, 1.0, 0.0], "both sides of the comparison"
        for v in L.OPACITY_EDGES:
            assert _count(c["opacity"], v) >= 2 and {float(m) for m in c["mask"][c["opacity"] == torch.tensor(v, dtype=F32)]} == {0.0, 1.0}, v
        assert _count(c["opacity"], L.LO) == 2 and _count(c["opacity"], L.HI) == 2
        for v in L.MASK_EDGES:
            assert _count(c["mask"], v) >= 1
        assert _count(c["mask"], 0.5) == 1 and float(torch.nextafter(torch.tensor(0.5), torch.tensor(1.0))) == L.MASK_EDGES[2]
        assert _count(c["depth"], 0.0) >= 1 and _count(c["depth"], -0.1) == 1 and _count(c["depth"], 1e-30) == 1
        assert float(c["depth"][25]) > 0 and float(v32[25]) == 1.0 and float(v32[23]) == 0.0 and float(v32[24]) == 0.0
        if N >= 1023:
            assert 0.05 < float(v32.mean()) < 0.95


@pytest.mark.parametrize("N", L.RENDER_N)
def test_render_restatement_passes_and_a_strict_radius_fails(N):
    c = L.render_case(N)
    for name, w in _render_weights().items():
        r64, r32 = L.render_run(c, w, F64), L.render_run(c, w, F32)
        L.render_check(c, w, r32, r32, r64, name)
        if N == 0:
            assert float(r64["loss"]) == 0.0 and float(r32["loss"]) == 0.0
        else:
            op = c["opacity"]
            out = (op < L.LO) | (op > L.HI)
            assert bool((r64["grads"][2][out] == 0).all()) and bool((r64["grads"][1][r64["valid"] == 0] == 0).all())
            if w[1] > 0:
                on = (op == L.LO) | (op == L.HI)
                assert bool((r64["grads"][2][on] != 0).all())
    if N >= 1:
        w = L.RENDER_WEIGHTS["ones"]
        r64, r32 = L.render_run(c, w, F64), L.render_run(c, w, F32)
        wrong = L.render_run(c, w, F32, wrong="valid_lt")
        assert int((wrong["valid"] != r32["valid"]).sum()) == 1
        # the value and the gradient of the depth term see it, even where the valid mask itself is not compared
        _fails(lambda: L.judge(wrong["terms"][2], r32["terms"][2], r64["terms"][2], float(r64["terms"][2]), "wrong", floor=L.render_depth(N, "depth") * L.U))
        _fails(lambda: L.judge(wrong["grads"][1], r32["grads"][1], r64["grads"][1], L.render_grad_scales(c, w, r64)[1], "wrong"))


# ================================================================================================ smooth points, bg blend
@pytest.mark.parametrize("N,K", L.SMOOTH_NK)
def test_smooth_restatement_passes(N, K):
    c = L.smooth_case(N, K)
    r64, r32 = L.smooth_run(c, F64), L.smooth_run(c, F32)
    L.smooth_check(c, r32, r32, r64)
    near = L.smooth_near_radius(c, r64)
    assert int(near.sum()) <= 2, "points within 1e-6 of the radius, where keep is not compared"
    assert r32["pts"].shape == (K * N, 3) and r32["grads"][0].shape == (1, N)
    if N * K >= 2048:
        assert 0.05 < float(r32["keep"].mean()) < 0.95
    keep64 = (r64["pts"].norm(dim=-1) < L.RADIUS).float()
    assert torch.equal(keep64[~near], r32["keep"][~near])


@pytest.mark.parametrize("N", L.BLEND_N)
def test_blend_restatement_passes(N):
    c = L.blend_case(N)
    r64, r32 = L.blend_run(c, F64), L.blend_run(c, F32)
    L.blend_check(c, r32, r32, r64)
    if N >= 255:
        assert _count(c["opacity"], 0.0) >= 10 and _count(c["opacity"], 1.0) >= 10
    else:
        assert _count(c["opacity"], 0.0) + _count(c["opacity"], 1.0) == 1
