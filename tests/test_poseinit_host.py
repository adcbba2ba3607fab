"""Pose initialisation without a GPU: the numpy oracle (tests/poseinit_oracle.py) against what the reference's registrate.py
recorded (tests/golden/poseinit.npz, tools/make_poseinit_golden.py), the oracle's robust ICP on the outlier case, argument
refusals and the header."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest
import torch

from tests import poseinit_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 4


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "poseinit.npz")))


def frames_of(g):
    return [g[f"depth_{i}"] for i in range(FRAMES)], [g[f"mask_{i}"] for i in range(FRAMES)]


def injected(g):
    """register(source, target) that hands out the fixture's prescribed matrices frame by frame (frames 1..)"""
    it = iter(g["prescribed"][1:])
    return lambda source, target: next(it)


def point_bound(g):
    """2^-23 x the largest |coordinate| of the reference's points: fp32 rounding of the clouds"""
    return 2.0 ** -23 * max(np.abs(g[f"points_{i}"]).max() for i in range(FRAMES))


def test_oracle_back_projection_is_the_references(golden):
    for i in range(FRAMES):
        depth, mask = po.depth_rule(golden[f"depth_{i}"], float(golden["depth_scale"])), po.mask_rule(golden[f"mask_{i}"])
        assert np.array_equal(mask != 0, (golden[f"mask_{i}"].reshape(24, 32, -1)[..., :3].mean(-1) / 255) > 0.5)
        assert np.array_equal((mask != 0) & (depth > 0), golden[f"kept_{i}"] != 0)
        pts, pix = po.depth_points(depth, mask, golden["K"])
        ref = golden[f"points_{i}"]
        assert ref.dtype == np.float64 and pts.dtype == np.float32 and pts.shape == ref.shape
        assert np.array_equal(pts, np.float32(ref)), i             # exactly, order included
        assert np.array_equal(pix, np.flatnonzero(golden[f"kept_{i}"]))
    assert (golden["mask_1"].ndim, golden["mask_0"].ndim) == (3, 2)                          # both mask layouts are in the fixture
    assert any((golden[f"depth_{i}"][golden[f"mask_{i}"].reshape(24, 32, -1)[..., 0] > 127] == 0).any() for i in range(FRAMES))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_oracle_init_poses_is_the_references(golden, mode):
    depths, masks = frames_of(golden)
    out = po.init_poses(depths, masks, golden["K"], float(golden["depth_scale"]), mode, injected(golden))
    ref = golden[f"transformations_{mode}"].reshape(-1, 4, 4)
    err = np.abs(out["transformations"] - ref).max()
    rel = abs(out["radius"] - float(golden[f"radius_{mode}"])) / float(golden[f"radius_{mode}"])
    print(f"mode {mode}: |dT| {err:.3e} (bound {point_bound(golden):.3e}), radius rel {rel:.3e} (bound {2.0 ** -21:.3e})")
    assert err <= point_bound(golden)
    assert rel <= 2.0 ** -21
    if mode:                                                       # the prescribed matrices were really used
        assert np.abs(ref[1:, :3, :3] - np.eye(3)).max() > 0.01
    assert not np.allclose(golden["transformations_1"], golden["transformations_2"])


def test_oracle_robust_icp_on_the_outlier_case():
    """1 500 source points; the target is one side of them, moved by 15 degrees, plus uniform outliers numbering a third of its
    points.  The bounds: 0.1 degrees and 5e-4 for the Welsch-weighted graduated ICP -- 2.5 x the worst of the numpy / scipy study
    that preceded the kernels (0.014 - 0.038 degrees, <= 1e-4 over 4 seeds x 3 rotations) --, and plain ICP at least 1 degree off
    (2.6 - 7.8 degrees there).  Seeds 0..3 of this surface gave, weighted / plain: 0.0031 / 0.69, 0.0016 / 5.3, 0.0037 / 0.76,
    0.0010 / 2.5 degrees; ROBUST_SEED = 3 is one on which plain ICP fails as in that study, and one that summation order cannot
    decide (the next test)."""
    source, target, T_true = po.robust_case()
    assert source.shape == (1500, 3) and target.shape[0] > 1000
    res = po.robust_reference()
    rot, trans = po.pose_error(res["transformation"], T_true)
    plain = po.robust_icp(source, target, weighted=False)
    rot_plain, trans_plain = po.pose_error(plain["transformation"], T_true)
    print(f"weighted: {rot:.4f} deg, {trans:.2e}, {res['iterations']} iterations in {res['stages']} stages; "
          f"plain: {rot_plain:.3f} deg, {trans_plain:.2e}, {plain['iterations']} iterations")
    assert res["converged"] and res["stages"] > 1 and res["nu"] == po.NU_END_K * po.knn_median(target, 7)
    assert rot <= 0.1 and trans <= 5e-4
    assert rot_plain >= 1.0 and plain["stages"] == 1


def test_summation_order_cannot_decide_the_robust_case():
    """What tests/test_gpu_poseinit.py relies on: with the sums taken in forward and in reversed point order the oracle keeps
    identical correspondences at every iteration, and T to 1e-10."""
    source, target, _ = po.robust_case()
    fwd = po.robust_reference()
    trace = []
    rev = po.robust_icp(source, target, reverse=True, trace=trace)
    assert (rev["iterations"], rev["stages"]) == (fwd["iterations"], fwd["stages"])
    assert len(trace) == len(fwd["trace"]) and all(np.array_equal(a, b) for a, b in zip(trace, fwd["trace"]))
    assert np.abs(rev["transformation"] - fwd["transformation"]).max() <= 1e-10


def test_summation_order_cannot_decide_the_ellipsoid_frames():
    """The same for the analytic frames that tests/test_gpu_poseinit.py registers with the default `register`."""
    fwd, rev = po.ellipsoid_reference(), po.ellipsoid_reference(reverse=True)
    assert len(fwd["runs"]) == 3 and all(r["converged"] and r["stages"] > 1 for r in fwd["runs"])
    for a, b in zip(fwd["runs"], rev["runs"]):
        assert (a["iterations"], a["stages"]) == (b["iterations"], b["stages"])
        assert all(np.array_equal(x, y) for x, y in zip(a["trace"], b["trace"]))
    assert np.abs(fwd["transformations"] - rev["transformations"]).max() <= 1e-10
    assert all(400 < len(p) < 3072 for p in fwd["points"])


def test_oracle_small_cases():
    rng = np.random.default_rng(5)
    p = rng.normal(size=(40, 3)).astype(np.float32)
    p[7] = p[3]                                                    # a duplicate counts with 0
    p[11] = np.nan
    d2 = po.knn_d2(p, 6)
    assert d2.shape == (40, 6) and d2[3, 0] == 0 and d2[7, 0] == 0 and np.isinf(d2[11]).all()
    assert (np.diff(d2[np.isfinite(d2).all(1)], axis=1) >= 0).all()
    assert np.isinf(po.knn_d2(p[:3], 8)[:, 2:]).all()
    six = np.sqrt(po.knn_d2(p, 6).astype(np.float64))
    assert po.knn_median(p, 7) == np.median(0.5 * (six[:, 2] + six[:, 3]))      # of 6: the mean of the 3rd and 4th
    # with every weight 1 the first 17 sums are the unweighted ones
    from tests import mesheval_oracle as mo
    q = rng.normal(size=(50, 3)).astype(np.float32)
    idx, dd = mo.nearest(p, q)
    s = po.icp_wsums(p, q, idx, dd, 0.0)
    assert np.array_equal(s[:17], mo.icp_sums(p, q, idx, dd)) and s[17] == 0 and s[18] == 39
    assert po.robust_icp(p[:0], q)["transformation"].tolist() == np.eye(4).tolist()
    assert not po.robust_icp(q[:2], q)["converged"]                # fewer than 3 correspondences


def test_argument_refusals():
    from morpheus_amd import poseinit
    from morpheus_amd._lib import MorpheusHipError
    pts = torch.zeros(10, 3)
    with pytest.raises(MorpheusHipError, match="MI355X only"):
        poseinit.depth_points(torch.zeros(4, 5), torch.zeros(4, 5, dtype=torch.uint8), np.eye(3))
    with pytest.raises(MorpheusHipError, match="MI355X only"):
        poseinit.knn_d2(pts, 3)
    with pytest.raises(MorpheusHipError, match="MI355X only"):
        poseinit.robust_icp(pts, pts)
    with pytest.raises(MorpheusHipError, match="MI355X only"):
        poseinit.icp_wsums(pts, pts, torch.zeros(10, dtype=torch.int32), torch.zeros(10), 1.0)
    with pytest.raises(MorpheusHipError, match="no CPU path"):
        poseinit.init_poses([np.ones((4, 5), int)], [np.ones((4, 5), int)], np.eye(3), device="cpu")
    for k in (0, 9, -1):
        with pytest.raises(MorpheusHipError, match=r"k must be in \[1, 8\]"):
            poseinit.knn_d2(pts, k)
    for k in (1, 10):
        with pytest.raises(MorpheusHipError, match=r"k must be in \[2, 9\]"):
            poseinit.knn_median(pts, k)
    with pytest.raises(MorpheusHipError, match="like depth"):     # mismatched image shapes
        poseinit.depth_points(torch.zeros(4, 5), torch.zeros(5, 4, dtype=torch.uint8), np.eye(3))
    with pytest.raises(MorpheusHipError, match="depth .* and mask"):
        poseinit.init_poses([np.ones((4, 5), int)], [np.ones((5, 4), int)], np.eye(3))
    with pytest.raises(MorpheusHipError, match="1 depth images and 2 masks"):
        poseinit.init_poses([np.ones((4, 5), int)], [np.ones((4, 5), int)] * 2, np.eye(3))
    with pytest.raises(MorpheusHipError, match="rigid_registrate"):
        poseinit.init_poses([], [], np.eye(3), rigid_registrate=3)
    assert np.array_equal(poseinit.mask_rule(np.array([[0, 127, 128, 255]])), [[0, 0, 1, 1]])
    assert poseinit.depth_rule(np.array([[0, 1500]], np.uint16)).tolist() == [[0.0, 1.5]]


def test_c_abi_refusals_and_empty_inputs():
    """status codes before any launch: no device is needed"""
    from morpheus_amd import _lib, build
    build.build()
    lib = _lib.load()
    one = np.zeros(8)
    P = one.ctypes.data                                            # any non-NULL address: refused or empty before it is read
    assert lib.mh_depth_points_tile() == 256 and lib.mh_knn_tile_points() == 1024
    assert lib.mh_icp_wsums_workspace_bytes() == 512 * 19 * 8
    assert lib.mh_depth_points_count(None, None, 0, 7, None, None) == 0                     # an empty image
    assert lib.mh_depth_points_count(None, None, 4, 4, None, None) == 1
    assert lib.mh_depth_points_count(P, P, 4, 16385, P, None) == 1
    assert lib.mh_depth_points_emit(P, P, 4, 4, 1.0, 1.0, 0.0, 0.0, P, 0, None, None, None) == 0   # an empty mask
    assert lib.mh_depth_points_emit(P, P, 4, 4, 0.0, 1.0, 0.0, 0.0, P, 3, P, None, None) == 1      # fx = 0
    assert lib.mh_depth_points_emit(P, P, 4, 4, 1.0, float("nan"), 0.0, 0.0, P, 3, P, None, None) == 1
    assert lib.mh_depth_points_emit(P, P, 4, 4, 1.0, 1.0, 0.0, 0.0, P, 17, P, None, None) == 1     # more points than pixels
    assert lib.mh_knn_d2(None, 0, 3, None, None) == 0
    for k in (0, 9):
        assert lib.mh_knn_d2(P, 5, k, P, None) == 1
    assert lib.mh_knn_d2(None, 5, 3, P, None) == 1
    assert lib.mh_icp_wsums(None, 0, None, 0, None, None, 1.0, None, None, None) == 0
    assert lib.mh_icp_wsums(P, 5, P, 5, P, P, -1.0, P, P, None) == 1
    assert lib.mh_icp_wsums(P, 5, P, 5, P, P, float("inf"), P, P, None) == 1
    assert lib.mh_icp_wsums(P, 5, P, 5, P, P, float("nan"), P, P, None) == 1
    assert lib.mh_icp_wsums(P, 5, P, 5, P, P, 1.0, None, P, None) == 1


def test_header_and_build_list_the_new_entry_points():
    from morpheus_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "morpheus_hip.h")).read()
    for name in ("mh_depth_points_tile", "mh_depth_points_count", "mh_depth_points_emit", "mh_knn_tile_points", "mh_knn_d2",
                 "mh_icp_wsums_workspace_bytes", "mh_icp_wsums"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTS, name
    assert "poseinit.hip" in build.SOURCES and build.FILE_FLAGS["poseinit.hip"] == ["-ffp-contract=off"]
    assert hdr.count("#define MH_ABI_VERSION 10 ") == 1
    import ctypes
    sig = _lib._DECLARED["mh_icp_wsums"]
    assert sig[1][6] is ctypes.c_double and len(sig[1]) == 10      # inv_2nu2 is a host double
    assert _lib._DECLARED["mh_depth_points_emit"][1][4:8] == [ctypes.c_double] * 4
