"""GPU: midpoint subdivision to a maximum edge (csrc/subdivide.hip, morpheus_amd.mesheval.subdivide_to_size and the subdivide=
argument of cull_mesh / eval_mesh) against the numpy restatement tests/subdivide_oracle.py -- depths, counts, vertices, colours,
triangles and parent indices byte for byte (a NaN equals a NaN) -- and against properties that need no oracle.

test_cull_mesh_subdivides_before_it_culls: the issue asks that the subdivided result "has fewer vertices outside the frustum than
the flap had".  By count that cannot hold for any subdivision: the unsplit triangle has 2 vertices outside, and a kept set that
ends at the frustum's edge ends in a row of triangles with one vertex each just outside it.  What is asserted is the meaning: a
smaller share of the kept vertices lies outside (the flap: 2 of 3), and none of them further than one output edge from a vertex
inside, where the flap reached 0.5."""
import numpy as np
import pytest
import torch

from tests import mesheval_oracle as eo
from tests import raster_oracle as ro
from tests import subdivide_oracle as so

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F = np.float32
M = F(0.01)                    # max_edge as it crosses the ABI
BLOCK = 256                    # outputs per workgroup of the two emit kernels (SD_THREADS)


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == F:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what
        got, want = np.where(nan, F(0), got).view(np.uint32), np.where(nan, F(0), want).view(np.uint32)
    assert np.array_equal(got, want), (what, int((got != want).sum()))


def _count(v, t, max_edge=M, max_iter=10):
    """mh_subdiv_count as the module launches it -> depth, n_vert, n_tri on the host"""
    from morpheus_amd._lib import launch, ptr
    vd, td = _dev(v, F), _dev(t, np.int32)
    T = td.shape[0]
    depth = torch.full((T,), -7, dtype=torch.int32, device=DEV)
    n = torch.full((2, T), -7, dtype=torch.int64, device=DEV)
    launch("mh_subdiv_count", ptr(vd), vd.shape[0], ptr(td), T, float(max_edge), int(max_iter), ptr(depth), ptr(n[0]), ptr(n[1]))
    return depth.cpu().numpy(), n[0].cpu().numpy(), n[1].cpu().numpy()


def _subdivide_same(v, t, colors=None, max_edge=M, max_iter=10):
    """the device's result and the oracle's, compared byte for byte -> (device result on the host, oracle result)"""
    from morpheus_amd import mesheval
    ref = so.subdivide(v, t, colors, max_edge, max_iter)
    depth, nv, nt = _count(v, t, max_edge, max_iter)
    _same_bytes(depth, ref["depth"], "depth")
    rv, rt = so.counts(ref["depth"], max_iter)
    _same_bytes(nv, rv, "n_vert")
    _same_bytes(nt, rt, "n_tri")
    out = mesheval.subdivide_to_size(_dev(v, F), _dev(t, np.int64), _dev(colors, F), max_edge=float(max_edge), max_iter=max_iter,
                                     return_index=True)
    assert out["vertices"].dtype == torch.float32 and out["triangles"].dtype == torch.int64 and out["index"].dtype == torch.int64
    assert out["vertices"].is_contiguous() and out["triangles"].is_contiguous()
    got = {k: None if x is None else x.cpu().numpy() for k, x in out.items()}
    _same_bytes(got["vertices"], ref["vertices"], "vertices")
    _same_bytes(got["triangles"].astype(np.int32), ref["triangles"], "triangles")
    _same_bytes(got["index"].astype(np.int32), ref["index"], "index")
    if colors is None:
        assert got["colors"] is None
    else:
        _same_bytes(got["colors"], ref["colors"], "colors")
    return got, ref


def _one_triangle(longest):
    """a scalene triangle in general position whose longest edge is (a, b), `longest` long up to fp32 rounding"""
    a = np.array((0.1, 0.2, 0.3))
    e = np.array((0.6, 0.64, 0.48))                                  # a unit vector
    w = np.array((0.8, -0.6, 0.0))                                   # another, orthogonal to it
    return np.stack([a, a + longest * e, a + longest * (0.45 * e + 0.5 * w)]).astype(F), np.array([(0, 1, 2)])


# 1 -- one triangle at every depth ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", range(11))
def test_one_triangle_at_every_depth(d):
    v, t = _one_triangle(0.75 * float(M) * 2.0 ** d)
    rng = np.random.default_rng(d)
    got, ref = _subdivide_same(v, t, rng.random(v.shape).astype(F))
    assert ref["depth"].tolist() == [d]
    n = 1 << d
    assert got["triangles"].shape[0] == n * n and got["vertices"].shape[0] == (n + 1) * (n + 2) // 2
    if d:
        assert np.array_equal(np.unique(got["triangles"]), np.arange(got["vertices"].shape[0]))       # every lattice point is used


# 2 -- ties ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", (0, 1, 5))
def test_an_edge_exactly_on_the_threshold(d):
    """m * 2^d is exact in fp32 and its square in float64: l2 * 4^-d == m2, which is not above it -> depth d; one ulp more -> d + 1"""
    e = F(M * F(2.0 ** d))
    v = np.array([(0, 0, 0), (e, 0, 0), (e * F(0.5), e * F(0.5), 0)], F)
    t = np.array([(0, 1, 2)])
    _, ref = _subdivide_same(v, t)
    assert ref["depth"].tolist() == [d]
    v[1, 0] = np.nextafter(e, F(np.inf))
    _, ref = _subdivide_same(v, t)
    assert ref["depth"].tolist() == [d + 1]


# 3, 8 -- meshes around the block size -----------------------------------------------------------------------------------------

def _pool():
    """A deformed 16 x 16 grid, 450 triangles that share their vertices, spacings mixed so that depths 0 .. 3 all occur."""
    rng = np.random.default_rng(31)
    steps = np.array((0.003, 0.008, 0.018, 0.04))
    x = np.concatenate([[0], np.cumsum(steps[rng.integers(0, 4, 15)])]) - 0.1
    y = np.concatenate([[0], np.cumsum(steps[rng.integers(0, 4, 15)])]) - 0.2
    X, Y = np.meshgrid(x, y, indexing="ij")
    Z = 0.3 + 0.0005 * rng.standard_normal(X.shape)
    v = np.stack([X, Y, Z], -1).reshape(-1, 3).astype(F)
    idx = np.arange(256).reshape(16, 16)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    t = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    return v, t, so.depths(v, t, M, 10)


def _mesh_with_totals(T, residue):
    """T triangles of the pool in shuffled order whose sub-triangle total is `residue` (-1, 0, 1) off a multiple of the emit
    block; unreferenced vertices are appended until the vertex total is, too."""
    v, t, depth = _pool()
    assert sorted(set(depth.tolist())) == [0, 1, 2, 3]
    rng = np.random.default_rng(1000 * T + residue + 1)
    for _ in range(20000):
        pick = rng.permutation(len(t))[:T]
        if (int((4 ** depth[pick].astype(np.int64)).sum()) - residue) % BLOCK == 0 and len(set(depth[pick].tolist())) == 4:
            break
    else:
        raise AssertionError("no subset with the wanted total")
    nv, nt = so.counts(depth[pick], 10)
    pad = (residue - (len(v) + int(nv.sum()))) % BLOCK
    v = np.concatenate([v, rng.uniform(-1, 1, (pad, 3)).astype(F)])
    assert (len(v) + int(nv.sum()) - residue) % BLOCK == 0 and (int(nt.sum()) - residue) % BLOCK == 0
    return v, t[pick]


@pytest.mark.parametrize("with_colors", (False, True))
@pytest.mark.parametrize("residue", (-1, 0, 1))
@pytest.mark.parametrize("T", (255, 256, 257))
def test_meshes_around_the_block_size(T, residue, with_colors):
    v, t = _mesh_with_totals(T, residue)
    colors = np.random.default_rng(5).random(v.shape).astype(F) if with_colors else None
    got, ref = _subdivide_same(v, t, colors)
    depth, m = ref["depth"].astype(np.int64), float(M)
    # 8 -- what needs no oracle: 4^d children per parent, in parent order
    assert np.array_equal(np.bincount(got["index"], minlength=T), 4 ** depth) and np.all(np.diff(got["index"]) >= 0)
    # every child faces the way its parent does (the smallest parent, 0.003 x 0.003, has |normal| ~ 10^-5; rounding moves a
    # child's normal by ~ 10^-10)
    p64 = got["vertices"].astype(np.float64)
    normal = lambda tri: np.cross(p64[tri[:, 1]] - p64[tri[:, 0]], p64[tri[:, 2]] - p64[tri[:, 0]])     # noqa: E731
    assert np.all((normal(got["triangles"]) * normal(t)[got["index"]]).sum(1) > 0)
    # every output edge is at most m + 2 ulp32(largest |coordinate|): each coordinate is within half an fp32 ulp of its exact
    # lattice value, so an edge moves by at most sqrt(3) ulp
    tri = got["triangles"]
    edges = np.concatenate([p64[tri[:, k]] - p64[tri[:, (k + 1) % 3]] for k in range(3)])
    longest = np.sqrt((edges ** 2).sum(1)).max()
    bound = m + 2 * float(np.spacing(np.abs(got["vertices"][np.unique(tri)]).max()))
    print(f"T {T} -> {len(tri)} triangles, {len(got['vertices'])} vertices; longest output edge {longest!r}, bound {bound!r}")
    assert longest <= bound


# 4 -- a shared edge -----------------------------------------------------------------------------------------------------------

def test_shared_edge_points_are_the_same_bytes_from_both_sides():
    v = np.array([(0.113, -0.207, 0.31), (0.171, -0.19, 0.335), (0.15, -0.15, 0.3), (0.14, -0.25, 0.33)], F)
    t = np.array([(0, 1, 2), (1, 0, 3)])                             # the edge 0 - 1 runs a -> b in one, b -> a in the other
    got, ref = _subdivide_same(v, t)
    d = int(ref["depth"][0])
    assert d >= 2 and ref["depth"][1] == d
    n, V = 1 << d, len(v)
    first = V + ref["vert_start"][:2]
    ours = got["vertices"][first[0]:first[0] + n - 1]                # row j = 0 without its corners: q = 1 .. n - 1
    theirs = got["vertices"][first[1]:first[1] + n - 1][::-1]
    assert np.array_equal(ours.view(np.uint32), theirs.view(np.uint32))


# 5 -- nothing to split ---------------------------------------------------------------------------------------------------------

def test_nothing_to_split_returns_the_input():
    from morpheus_amd import mesheval
    v, t = ro.icosphere(2, 0.01)                                     # edges ~ 0.003
    vd, td, cd = _dev(v, F), _dev(t, np.int64), _dev(np.random.default_rng(2).random(v.shape), F)
    out = mesheval.subdivide_to_size(vd, td, cd, return_index=True)
    assert out["vertices"].data_ptr() == vd.data_ptr() and out["triangles"].data_ptr() == td.data_ptr()
    assert out["colors"].data_ptr() == cd.data_ptr() and out["vertices"].shape == vd.shape
    assert torch.equal(out["index"], torch.arange(len(t), device=DEV))
    _subdivide_same(v, t)
    empty = mesheval.subdivide_to_size(vd, td[:0], return_index=True)
    assert empty["vertices"].data_ptr() == vd.data_ptr() and empty["triangles"].shape == (0, 3) and empty["index"].shape == (0,)
    assert empty["colors"] is None


# 6 -- pass-through --------------------------------------------------------------------------------------------------------------

def test_bad_indices_and_nan_vertices_pass_through():
    v = np.array([(0, 0, 0), (0.05, 0, 0), (0, 0.05, 0), (np.nan, 0.01, 0), (0.001, 0.001, 0), (0.03, 0.03, 0.03)], F)
    t = np.array([(0, 1, 2),          # depth 3
                  (0, 1, 6),          # an index past V: depth 0, copied
                  (-1, 1, 2),         # a negative index: depth 0, copied
                  (0, 4, 3),          # two NaN edges and a short one: depth 0, copied
                  (0, 1, 3),          # two NaN edges and a long one: split, NaN wherever the NaN corner has weight
                  (5, 1, 2)])
    got, ref = _subdivide_same(v, t, np.random.default_rng(3).random(v.shape).astype(F))
    assert ref["depth"][:5].tolist() == [3, 0, 0, 0, 3]
    first = ref["tri_start"]
    assert got["triangles"][first[1]].tolist() == [0, 1, 6] and got["triangles"][first[2]].tolist() == [-1, 1, 2]
    assert got["triangles"][first[3]].tolist() == [0, 4, 3]
    assert np.isnan(got["vertices"][len(v) + ref["vert_start"][4]:len(v) + ref["vert_start"][5]]).any()
    assert np.isfinite(got["vertices"][len(v):len(v) + ref["vert_start"][4]]).all()


# 7 -- refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_come_before_any_allocation():
    from morpheus_amd import mesheval
    from morpheus_amd._lib import MorpheusHipError

    def refused(match, v, t, **kw):
        vd, td = _dev(v, F), _dev(t, np.int64)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with pytest.raises(MorpheusHipError, match=match):
            mesheval.subdivide_to_size(vd, td, **kw)
        assert torch.cuda.max_memory_allocated() - before < 32768    # the count pass's few words; no output

    v, t = _one_triangle(0.75 * float(M) * 2.0 ** 11)
    refused(r"1 of 1 triangles still have an edge above max_edge .* \(longest edge 15\.3", v, t)
    _, ref = _subdivide_same(*_one_triangle(0.75 * float(M) * 2.0 ** 10), max_iter=10)
    assert ref["depth"].tolist() == [10]
    assert _count(v, t)[0].tolist() == [11] and so.depths(v, t, M, 10).tolist() == [11]
    v8, t8 = _one_triangle(0.75 * float(M) * 2.0 ** 8)
    refused("after max_iter = 7", v8, t8, max_iter=7)
    assert _count(v8, t8, max_iter=7)[0].tolist() == [8] and so.depths(v8, t8, M, 7).tolist() == [8]
    vi = v8.copy()
    vi[2, 1] = np.inf
    refused("longest edge inf", vi, t8)
    assert _count(vi, t8)[0].tolist() == [11] and so.depths(vi, t8, M, 10).tolist() == [11]
    for bad in (0.0, -0.01, float("nan"), float("inf"), 1e-50):
        refused("max_edge must be finite and positive", v8, t8, max_edge=bad)
    for bad in (-1, 11):
        refused("max_iter must be in", v8, t8, max_iter=bad)
    # depth 8: 65 536 triangles and 33 153 vertices, ~ 2.4 MB with the int64 triangles; a cap of 1 MB refuses it, 1 GB does not
    refused(r"become 33153 vertices / 65536 triangles .* larger max_edge", v8, t8, max_gb=1e-3)
    assert mesheval.subdivide_to_size(_dev(v8, F), _dev(t8, np.int64), max_gb=1.0)["triangles"].shape == (65536, 3)


# 9 -- cull_mesh ------------------------------------------------------------------------------------------------------------------

def test_cull_mesh_subdivides_before_it_culls():
    from morpheus_amd import mesheval
    H, W = 24, 32
    K = np.array([[150.0, 0, 16], [0, 150.0, 12], [0, 0, 1]])       # at distance 2 the image is 0.43 x 0.32 wide
    c2w = ro.look_at((0, -2.0, 0), up=(0, 0, 1))
    v = np.array([(0, 0, 0), (0.5, 0, 0), (0.25, 0, 0.4330127)], F)   # 0.5-long edges; corner 0 at the image centre
    t = np.array([(0, 1, 2)])
    colors = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1)], F)
    depth = np.full((H, W), 5.0, F)
    depth_gt = np.ones((H, W), F)
    fr, obs, _ = eo.cull_vertices(v, eo.world_to_camera_f64(c2w), K, H, W, depth, depth_gt, 0.005)
    assert fr.tolist() == [True, False, False] and obs.tolist() == [True, False, False]
    kw = dict(c2w=c2w, K=K, H=H, W=W, depth_gt=_dev(depth_gt), rendered_depth=_dev(depth))
    vd, td, cd = _dev(v), _dev(t), _dev(colors)
    plain, off = mesheval.cull_mesh(vd, td, cd, **kw), mesheval.cull_mesh(vd, td, cd, subdivide=False, **kw)
    for k in ("vertices", "triangles", "colors"):
        assert torch.equal(plain[k], off[k])
    assert torch.equal(plain["vertices"], vd) and plain["triangles"].tolist() == [[0, 1, 2]]      # the flap: kept whole

    fine = mesheval.cull_mesh(vd, td, cd, subdivide=True, return_masks=True, **kw)
    sub = so.subdivide(v, t, colors, M, 10)
    assert sub["depth"].tolist() == [6]
    ref = eo.cull_mesh(sub["vertices"], sub["triangles"], sub["colors"], c2w, K, H, W, depth, depth_gt, 0.005, True)
    for k in ("vertices", "triangles", "colors"):
        _same_bytes(fine[k].cpu().numpy(), ref[k] if k != "triangles" else ref[k].astype(np.int64), k)
    for k in ("frustum", "observed", "invalid", "keep"):
        assert fine[k].shape[0] == (len(sub["triangles"]) if k == "keep" else len(sub["vertices"]))
        assert np.array_equal(fine[k].cpu().numpy(), ref[k]), k
    assert 0 < len(ref["triangles"]) < len(sub["triangles"])
    # what lies outside the frustum: 2 of the flap's 3 vertices, up to 0.5 away from the one inside
    kept = ref["vertices"]
    inside = eo.cull_vertices(kept, eo.world_to_camera_f64(c2w), K, H, W, depth, depth_gt, 0.005)[0]
    assert 0 < (~inside).sum() and (~inside).mean() < 2 / 3
    k64 = kept.astype(np.float64)
    reach = np.sqrt(((k64[~inside][:, None] - k64[inside][None]) ** 2).sum(-1)).min(1).max()
    print(f"kept {len(ref['triangles'])} of {len(sub['triangles'])} triangles, {len(kept)} vertices, {int((~inside).sum())} outside "
          f"the frustum, none further than {reach!r} from one inside")
    assert reach <= float(M) + 2 * float(np.spacing(F(0.5)))


# 10 -- eval_mesh ------------------------------------------------------------------------------------------------------------------

def test_eval_mesh_with_subdivision_end_to_end():
    from morpheus_amd import harness, mesh, mesheval
    model = harness.build_model("b", DEV)
    H, W = 120, 160
    K = np.array([[150.0, 0, 80.0], [0, 150.0, 60.0], [0, 0, 1]])
    pose = ro.look_at((2.2, 0.8, 0.7))
    m = mesh.extract_mesh(model, resolution=64, S=64, t=25 / 200)
    motion = eo.rigid(np.radians(1.0), np.radians(-0.8), np.radians(1.2), (0.01, -0.006, 0.004))
    gt = {"vertices": mesheval.transform_points(m["vertices"], motion), "triangles": m["triangles"]}
    dgt = [torch.full((H, W), 2.0, device=DEV)]
    out = mesheval.eval_mesh([m], [gt], [pose], K, H, W, dgt, num_points=5000, subdivide=True)
    assert out["frames"] == [0] and np.isfinite(out["acc"] + out["comp"] + out["comp ratio"]).all()
    coarse = mesheval.eval_mesh([m], [gt], [pose], K, H, W, dgt, num_points=5000)
    culled = mesheval.cull_mesh(m["vertices"], m["triangles"], m["colors"], c2w=pose, K=K, H=H, W=W, depth_gt=dgt[0], subdivide=True)
    assert culled["triangles"].shape[0] > m["triangles"].shape[0] > 0 and culled["colors"].shape == culled["vertices"].shape
    area = lambda x: float(mesheval.area_weights(x["vertices"], x["triangles"])[0].double().sum())      # noqa: E731
    print(f"mesh {m['triangles'].shape[0]} triangles, area {area(m)!r}; kept {culled['triangles'].shape[0]} subdivided triangles, "
          f"area {area(culled)!r}; scores {out} against {coarse} without subdivision")
    assert 0 < area(culled) <= area(m)
