"""GPU: pose initialisation (csrc/poseinit.hip, morpheus_amd.poseinit) against the numpy restatement tests/poseinit_oracle.py and
the reference's recorded results (tests/golden/poseinit.npz) -- back-projected points and k nearest distances bit for bit, the
Welsch-weighted sums to 1e-12 of the sum of |terms| and byte-equal to mh_icp_sums at w = 1, robust_icp's stages, iterations and T
on a case that summation order cannot decide (tests/test_poseinit_host.py), init_poses in its three modes, the files."""
import os

import numpy as np
import pytest
import torch

from tests import poseinit_oracle as po

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FRAMES = 4


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "poseinit.npz")))


# ---- depth_points --------------------------------------------------------------------------------------------------------

def test_depth_points_bit_identical():
    from morpheus_amd import _lib, poseinit
    tile = _lib.load().mh_depth_points_tile()
    H, W = 37, 53                                                  # 1961 pixels: 7 full tiles and a part of one; W is no divisor of the tile
    rng = np.random.default_rng(11)
    depth = rng.uniform(0.3, 2.5, (H, W)).astype(F)
    mask = (rng.random((H, W)) < 0.6).astype(np.uint8) * rng.choice(np.array([1, 7, 255], np.uint8), (H, W))
    mask[14:16] = 0                                                # empty rows
    mask[10] = 1                                                   # a fully masked row
    flat_m, flat_d = mask.reshape(-1), depth.reshape(-1)
    flat_m[4 * tile:5 * tile] = 0                                  # tile 4 keeps nothing
    flat_d[rng.choice(H * W, 150, replace=False)] = 0.0            # no depth
    flat_d[rng.choice(H * W, 60, replace=False)] = np.nan
    flat_d[rng.choice(H * W, 20, replace=False)] = -1.0
    for edge in (tile, 2 * tile, 7 * tile):                        # a kept pixel on either side of a tile boundary
        flat_m[edge - 1:edge + 1] = 1
        flat_d[edge - 1:edge + 1] = (1.25, 0.75)
    flat_m[[0, H * W - 1]] = 1                                     # the first and the last pixel
    flat_d[[0, H * W - 1]] = (0.5, 2.0)
    K = np.array([[61.3, 0.0, 25.7], [0.0, 59.9, 18.2], [0.0, 0.0, 1.0]])
    want, want_pix = po.depth_points(depth, mask, K)
    assert not mask[14:16].any() and mask[10].all()
    assert 600 < len(want) < H * W and np.isnan(flat_d[flat_m != 0]).any() and (flat_d[flat_m != 0] == 0).any()
    pts, pix = poseinit.depth_points(_dev(depth), _dev(mask), K, return_pixels=True)
    assert pts.dtype == torch.float32 and pix.dtype == torch.int32 and tuple(pts.shape) == want.shape
    assert np.array_equal(pix.cpu().numpy(), want_pix)
    assert np.array_equal(_bits(pts.cpu().numpy()), _bits(want))
    for edge in (tile, 2 * tile, 7 * tile):
        assert edge - 1 in want_pix and edge in want_pix
    assert np.array_equal(_bits(poseinit.depth_points(_dev(depth), _dev(mask), torch.from_numpy(K)).cpu().numpy()), _bits(want))
    # an empty mask, a mask over pixels without depth, one pixel
    assert tuple(poseinit.depth_points(_dev(depth), _dev(np.zeros((H, W), np.uint8)), K).shape) == (0, 3)
    assert tuple(poseinit.depth_points(_dev(np.zeros((H, W), F)), _dev(mask), K).shape) == (0, 3)
    one = poseinit.depth_points(_dev(np.array([[1.5]], F)), _dev(np.array([[9]], np.uint8)), K).cpu().numpy()
    assert np.array_equal(_bits(one), _bits(po.depth_points(np.array([[1.5]], F), np.array([[9]], np.uint8), K)[0]))


# ---- mh_knn_d2 -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def knn_pool():
    from morpheus_amd import _lib
    tile = _lib.load().mh_knn_tile_points()
    rng = np.random.default_rng(12)
    p = rng.uniform(-1, 1, (tile + 1, 3)).astype(F)
    p[3] = p[1]                                                    # duplicates, also across a wavefront, a workgroup and a tile
    p[70:80] = p[40:50]
    p[300] = p[2]
    p[tile] = p[5]
    p[4] = (np.nan, 0.1, 0.2)                                      # one NaN point: it has no neighbour and is nobody's
    return tile, p


@pytest.mark.parametrize("which", ["1", "5", "64", "65", "257", "tile-1", "tile", "tile+1"])
def test_knn_d2_bit_identical(knn_pool, which):
    from morpheus_amd import poseinit
    tile, pool = knn_pool
    N = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1}.get(which) or int(which)
    p = pool[:N]
    want = po.knn_d2(p, 8)
    for k in (1, 6, 8):
        got = poseinit.knn_d2(_dev(p), k).cpu().numpy()
        assert got.shape == (N, k) and got.dtype == F
        assert np.array_equal(_bits(got), _bits(want[:, :k])), (N, k)
    if N >= 5:
        assert np.isinf(want[4]).all() and want[1, 0] == 0 and want[3, 0] == 0
    if N <= 5:
        assert np.isinf(want[:, N - 1:]).all()                     # fewer than k other points: +inf
    if N >= 64:
        assert poseinit.knn_median(_dev(p), 7) == po.knn_median(p, 7)


# ---- mh_icp_wsums --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,Nt", [(3001, 700), (140001, 900)])     # 12 workgroups; more points than 512 workgroups hold at once
def test_wsums_against_the_oracle(N, Nt):
    from morpheus_amd import mesheval, poseinit
    rng = np.random.default_rng(13)
    p = rng.uniform(-1, 1, (N, 3)).astype(F)
    q = rng.uniform(-1, 1, (Nt, 3)).astype(F)
    dp, dq = _dev(p), _dev(q)
    idx, d2 = mesheval.nearest(dp, dq, max_dist=0.25)              # pinned bit for bit by tests/test_gpu_mesheval.py
    hi, hd = idx.cpu().numpy(), d2.cpu().numpy()
    n_corr = int((hi >= 0).sum())
    assert 0 < n_corr < N and hd[hi >= 0].min() > 0                # some idx = -1 are skipped; no zero distance
    nu = 0.08
    inv = 1.0 / (2.0 * nu * nu)
    terms = po.icp_wterms(p, q, hi, hd, inv)
    want, scale = terms.sum(axis=0), np.abs(terms).sum(axis=0)
    got = poseinit.icp_wsums(dp, dq, idx, d2, inv)
    assert got.dtype == torch.float64 and tuple(got.shape) == (19,)
    again = poseinit.icp_wsums(dp, dq, idx, d2, inv)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), again.cpu().numpy().view(np.uint64))      # two runs, the same bytes
    got = got.cpu().numpy()
    err = np.abs(got - want) / scale
    print(f"N {N}: max |d sums| / sum |terms| = {err.max():.3e}")
    assert (err <= 1e-12).all(), err
    assert got[18] == n_corr and 0.05 * n_corr < got[0] < 0.95 * n_corr
    # w = 1: the bytes of mh_icp_sums
    ones = poseinit.icp_wsums(dp, dq, idx, d2, 0.0).cpu().numpy()
    plain = mesheval.icp_sums(dp, dq, idx, d2).cpu().numpy()
    assert np.array_equal(ones[:17].view(np.uint64), plain.view(np.uint64))
    assert ones[17] == 0.0 and ones[18] == n_corr
    # a nu so small that every weight underflows
    tiny = poseinit.icp_wsums(dp, dq, idx, d2, 1e30).cpu().numpy()
    assert tiny[0] == 0.0 and (tiny[1:17] == 0.0).all() and tiny[17] == n_corr and tiny[18] == n_corr
    # no correspondence at all, and indices beyond the target are skipped like -1
    none = poseinit.icp_wsums(dp, dq, torch.full_like(idx, -1), d2, inv).cpu().numpy()
    assert (none == 0.0).all()
    beyond = poseinit.icp_wsums(dp, dq[:Nt // 2].contiguous(), idx, d2, inv).cpu().numpy()
    half = po.icp_wterms(p, q[:Nt // 2], hi, hd, inv)
    assert beyond[18] == half.shape[0] and abs(beyond[0] - half[:, 0].sum()) <= 1e-12 * half[:, 0].sum()


# ---- robust_icp ----------------------------------------------------------------------------------------------------------

def test_robust_icp_end_to_end():
    """the host test's case, with the seed for which summation order cannot decide an iteration (checked there on the CPU)"""
    from morpheus_amd import poseinit
    source, target, T_true = po.robust_case()
    want = po.robust_reference()
    got = poseinit.robust_icp(_dev(source), _dev(target))
    dT = np.abs(got["transformation"] - want["transformation"]).max()
    rot, trans = po.pose_error(got["transformation"], T_true)
    print(f"stages {got['stages']} / {want['stages']}, iterations {got['iterations']} / {want['iterations']}, |dT| {dT:.3e}, "
          f"{rot:.4f} deg, {trans:.2e}")
    assert (got["stages"], got["iterations"]) == (want["stages"], want["iterations"])
    assert dT <= 1e-8
    assert got["converged"] and got["nu"] == want["nu"]
    assert abs(got["energy"] - want["energy"]) <= 1e-8 * len(source) and abs(got["weight_sum"] - want["weight_sum"]) <= 1e-8 * len(source)
    assert rot <= 0.1 and trans <= 5e-4
    # init: started at the answer it stays there; degenerate inputs
    at = poseinit.robust_icp(_dev(source), _dev(target), init=want["transformation"])
    rot, trans = po.pose_error(at["transformation"], T_true)
    assert at["converged"] and at["iterations"] < want["iterations"] and rot <= 0.1 and trans <= 5e-4
    empty = poseinit.robust_icp(_dev(source[:0]), _dev(target))
    assert np.array_equal(empty["transformation"], np.eye(4)) and not empty["converged"] and empty["iterations"] == 0
    two = poseinit.robust_icp(_dev(source[:2]), _dev(target))
    assert not two["converged"] and two["iterations"] == 0 and np.array_equal(two["transformation"], np.eye(4))


# ---- init_poses ----------------------------------------------------------------------------------------------------------

def _frames(g):
    return [g[f"depth_{i}"] for i in range(FRAMES)], [g[f"mask_{i}"] for i in range(FRAMES)]


def _injected(g, seen=None):
    it = iter(g["prescribed"][1:])

    def register(source, target):
        if seen is not None:
            seen.append((source, target))
        return next(it)
    return register


def _bounds(g):
    return 2.0 ** -23 * max(np.abs(g[f"points_{i}"]).max() for i in range(FRAMES)), 2.0 ** -21


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_init_poses_is_the_references(golden, mode):
    from morpheus_amd import poseinit
    depths, masks = _frames(golden)
    seen = []
    out = poseinit.init_poses(depths, masks, golden["K"], depth_scale=float(golden["depth_scale"]), rigid_registrate=mode,
                              register=_injected(golden, seen))
    ref = golden[f"transformations_{mode}"].reshape(-1, 4, 4)
    tol_T, tol_r = _bounds(golden)
    err = np.abs(out["transformations"] - ref).max()
    rel = abs(out["radius"] - float(golden[f"radius_{mode}"])) / float(golden[f"radius_{mode}"])
    print(f"mode {mode}: |dT| {err:.3e} (bound {tol_T:.3e}), radius rel {rel:.3e} (bound {tol_r:.3e})")
    assert out["transformations"].dtype == np.float64 and out["transformations"].shape == (FRAMES, 4, 4)
    assert err <= tol_T and rel <= tol_r
    assert len(seen) == (FRAMES - 1 if mode else 0)
    if mode:                                                       # what `register` is handed: the centred fp32 clouds, on the device
        clouds = po.init_poses(depths, masks, golden["K"], 1000.0, 0)["points"]
        for i, (source, target) in enumerate(seen, start=1):
            src = clouds[0 if mode == 1 else i - 1].astype(np.float64)
            tgt = clouds[i].astype(np.float64)
            assert source.is_cuda and source.dtype == torch.float32
            for got, cloud in ((source, src), (target, tgt)):      # x - mean in float64, rounded once (the mean to round-off)
                assert got.shape == cloud.shape and np.abs(got.cpu().numpy() - (cloud - cloud.mean(0))).max() <= 2.0 ** -23 * np.abs(cloud).max()


def test_init_poses_registers_analytic_frames():
    """mode 1 with the default register (robust_icp) on 4 analytic 48 x 64 frames of a moved ellipsoid with bumps, against the
    oracle's run (on which summation order decides nothing: tests/test_poseinit_host.py).  The bound on T is robust_icp's 1e-8
    (coarse @ fine with entries of order 1), the radius bound the scores' 2^-21."""
    from morpheus_amd import poseinit
    depths, masks, K = po.ellipsoid_frames()
    want = po.ellipsoid_reference()
    runs = []

    def register(source, target):
        runs.append(poseinit.robust_icp(source, target))
        return runs[-1]["transformation"]

    out = poseinit.init_poses(list(depths), list(masks), K, register=register)
    assert [(r["stages"], r["iterations"]) for r in runs] == [(r["stages"], r["iterations"]) for r in want["runs"]]
    err = np.abs(out["transformations"] - want["transformations"]).max()
    rel = abs(out["radius"] - want["radius"]) / want["radius"]
    print(f"|dT| {err:.3e}, radius rel {rel:.3e}, iterations {[r['iterations'] for r in runs]}")
    assert err <= 1e-8 and rel <= 2.0 ** -21
    default = poseinit.init_poses(list(depths[:2]), list(masks[:2]), K)                     # register=None is the same function
    assert np.array_equal(default["transformations"], out["transformations"][:2])


def test_init_poses_from_dir_round_trip(golden, tmp_path):
    from PIL import Image

    from morpheus_amd import poseinit
    depths, masks = _frames(golden)
    os.makedirs(tmp_path / "depth")
    os.makedirs(tmp_path / "mask")
    np.savetxt(tmp_path / "intrinsics.txt", golden["K"])
    for i in range(FRAMES):
        Image.fromarray(depths[i]).save(tmp_path / "depth" / ("%06d.png" % i))
        Image.fromarray(masks[i]).save(tmp_path / "mask" / ("%06d.png" % i))
    out = poseinit.init_poses_from_dir(str(tmp_path), rigid_registrate=2, register=_injected(golden))
    assert sorted(os.listdir(tmp_path / "intermediate")) == ["radius.txt", "transformations.npy"]      # no .obj clouds
    # as create_camera.py loads them
    transformations = np.load(str(tmp_path) + "/" + "intermediate/transformations.npy").reshape(-1, 4, 4)
    radius = np.loadtxt(str(tmp_path) + "/" + "intermediate/radius.txt")
    assert np.load(tmp_path / "intermediate" / "transformations.npy").shape == (FRAMES, 16)
    assert np.array_equal(transformations, out["transformations"]) and transformations.dtype == np.float64
    assert radius.shape == () and abs(float(radius) - out["radius"]) <= 0.5e-8
    assert open(tmp_path / "intermediate" / "radius.txt").read() == "%.8f\n" % out["radius"]
    tol_T, tol_r = _bounds(golden)
    assert np.abs(transformations - golden["transformations_2"].reshape(-1, 4, 4)).max() <= tol_T
    assert abs(float(radius) - float(golden["radius_2"])) <= tol_r * float(golden["radius_2"]) + 0.5e-8
    scale_mat = np.diag([radius, radius, radius, 1.0]).astype(np.float32)                   # create_camera.py's next step runs
    assert scale_mat[0, 0] > 0
