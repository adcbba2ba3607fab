"""GPU: importance resampling on the HIP kernels (csrc/resample.hip) -- the dense form against the reference's recorded results
(tests/golden/sample_pdf.npz) in the measure of tests/resample_oracle.score, the packed form's exact invariants, its agreement
with the dense form bit for bit and with the fp32 restatement in the measure, the fixed-capacity form (also under graph capture),
and the renderer's opt-in."""
import os

import numpy as np
import pytest
import torch

from morpheus_amd import synth
from tests import f64_judge as J
from tests import resample_oracle as ro

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_pdf.npz")
FACTOR, FLOOR = 3, 4 * J.U


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(golden, name):
    return tuple(golden[f"{name}_{k}"] for k in ("bins", "weights", "u", "s32", "s64"))


# ------------------------------------------------------------------------------------------------------------------ dense form
@pytest.mark.parametrize("T", ro.T_SET)
def test_sample_pdf_against_the_golden(golden, T):
    """every kind of weights at this T (n and B cycle through their sets over the cases): finite, inside the bins, and the worst
    e against the reference's float64 result <= max(3 x the worst e of the reference's own fp32 run, 4 U)"""
    from morpheus_amd import resample
    for name, T_, n, B, kind in ro.cases():
        if T_ != T:
            continue
        bins, w, u, s32, s64 = _case(golden, name)
        s = resample.sample_pdf(_t(bins), _t(w), n, u=_t(u))
        assert s.shape == (B, n) and s.dtype == torch.float32
        s = s.cpu().numpy()
        assert bool(np.isfinite(s).all()), name
        assert bool(((s >= bins[:, :1]) & (s <= bins[:, -1:])).all()), name
        e, e_ref = ro.score_dense(s, s64, u, bins, w), ro.score_dense(s32, s64, u, bins, w)
        mirror = ro.sample_pdf_np(bins, w, u, np.float32, cdf="kernel", hold=True)
        print(f"{name:14s} B {B} n {n:3d}: worst e {e / J.U:5.2f} U; the reference's fp32 run {e_ref / J.U:5.2f} U; "
              f"{int((s != mirror).sum())} of {s.size} samples differ from the kernel-form restatement")
        assert J.within(e, e_ref, FACTOR, FLOOR), (name, e / J.U, e_ref / J.U)
        assert s[0, 0] == bins[0, 0], name                            # u = 0: the first edge


def test_sample_pdf_top_of_the_cdf(golden):
    """u = 1 - 2^-24 at or above a CDF that tops out below 1: the last edge, exactly.  The rows where the kernel's CDF (float64
    sums rounded once: resample_oracle's "kernel" form) tops out at or below that u are found on the host; there must be some."""
    from morpheus_amd import resample
    top_u, reached = np.float32(1 - J.U), 0
    for name, T, n, B, kind in ro.cases():
        bins, w, u, _, _ = _case(golden, name)
        s = resample.sample_pdf(_t(bins), _t(w), n, u=_t(u)).cpu().numpy()
        top = ro.cdf_np(w, ro.EPS, np.float32, "kernel")[:, -1]
        for b in range(B):
            hit = (u[b] == top_u) & (top[b] <= top_u)
            reached += int(hit.sum())
            assert bool((s[b][hit] == bins[b, -1]).all()), (name, b)
    print(f"u = 1 - 2^-24 met a CDF topping out at or below it in {reached} rows")
    assert reached >= 3


def test_sample_pdf_det_batch_dims_and_long_rows(golden):
    from morpheus_amd import _lib, resample
    bins, w, _, _, _ = _case(golden, "T65_laplace")
    B = bins.shape[0]
    for n in ro.N_SET:                  # det=True is the call with u = the reference's linspace grid, bit for bit
        grid = _t(golden[f"det_n{n}"])[None].expand(B, n)
        assert torch.equal(resample.sample_pdf(_t(bins), _t(w), n, det=True), resample.sample_pdf(_t(bins), _t(w), n, u=grid))
    # leading batch dimensions are flattened
    b3, w3 = _t(bins[:6]).view(2, 3, -1), _t(w[:6]).view(2, 3, -1)
    u3 = torch.rand(2, 3, 7, device=DEV)
    out = resample.sample_pdf(b3, w3, 7, u=u3)
    assert out.shape == (2, 3, 7) and torch.equal(out.view(6, 7), resample.sample_pdf(b3.view(6, -1), w3.view(6, -1), 7, u=u3.view(6, 7)))
    # rows longer than the LDS staging go through the global scratch: the staged length, one more, and a long one
    stage = int(_lib.load().mh_resample_stage())
    for ci, T in enumerate((stage + 1, stage + 2, 3 * stage)):
        bb, ww, uu = ro.make_case(T, 65, 5, "span20" if ci else "laplace", seed=77 + ci)
        s = resample.sample_pdf(_t(bb), _t(ww), 65, u=_t(uu)).cpu().numpy()
        s64 = ro.sample_pdf_np(bb, ww, uu, np.float64)
        e = ro.score_dense(s, s64, uu, bb, ww)
        e_ref = ro.score_dense(ro.sample_pdf_np(bb, ww, uu, np.float32), s64, uu, bb, ww)
        print(f"T {T}: worst e {e / J.U:.2f} U, the fp32 restatement {e_ref / J.U:.2f} U")
        assert bool(np.isfinite(s).all()) and bool(((s >= bb[:, :1]) & (s <= bb[:, -1:])).all())
        assert J.within(e, e_ref, FACTOR, FLOOR), (T, e / J.U, e_ref / J.U)


# ------------------------------------------------------------------------------------------------------------------ packed form
def _scene(counts, seed, special=True):
    """packed rays of the given interval counts: steps of 0.01 from a per-ray start, every third ray with gaps (intervals
    dropped from a longer march); with `special`, the last three rays are: one with a zero-width interval inside, a miss ray of
    the uniform sampler (zero-width intervals at t = 0) and one whose weights are all zero"""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int32)
    rs = (np.cumsum(counts) - counts).astype(np.int32)
    ts, te = [], []
    for r, c in enumerate(counts):
        t0, step = np.float32(0.3 + rng.random()), np.float32(0.01)
        k = np.arange(2 * c if r % 3 == 2 else c)
        if r % 3 == 2 and c > 0:
            k = np.sort(rng.choice(k, size=c, replace=False))
        # one list of edges per ray, so that te_i <= ts_{i+1} holds exactly (te_i == ts_{i+1} where steps are consecutive)
        edges = (t0 + np.arange(2 * c + 1, dtype=np.float32) * step).astype(np.float32)
        ts.append(edges[k])
        te.append(edges[k + 1])
    ts, te = np.concatenate(ts), np.concatenate(te)
    w = (rng.random(ts.shape[0]) * (rng.random(ts.shape[0]) > 0.3)).astype(np.float32)
    if special:
        a, b, z = len(counts) - 3, len(counts) - 2, len(counts) - 1
        te[rs[a] + counts[a] // 2] = ts[rs[a] + counts[a] // 2]
        ts[rs[b]:rs[b] + counts[b]] = te[rs[b]:rs[b] + counts[b]] = 0.0
        w[rs[z]:rs[z] + counts[z]] = 0.0
    return rs, counts, ts, te, w


def _run_packed(rs, rc, ts, te, w, n, jit, **kw):
    from morpheus_amd import ops
    out = ops.resample_packed(_t(w), _t(ts), _t(te), _t(rs), _t(rc), n, None if jit is None else _t(jit), **kw)
    keys = ("ray_idx", "t_starts", "t_ends", "ray_start", "ray_cnt")
    return out, {k: v.cpu().numpy() for k, v in zip(keys, out)}


SCENES = {
    # 0, 1, 63, 64, 65 and 130 intervals in one call, one ray at the staging capacity and one past it, the special rays
    "mixed": lambda stage: _scene([0, 1, 63, 64, 65, 130, stage, stage + 1, 0, 7, 5, 3, 9], seed=21),
    "five": lambda stage: _scene([3, 0, 65, 1, 12], seed=22),
    "one": lambda stage: _scene([17], seed=23, special=False),
}


@pytest.mark.parametrize("n", [1, 64, 65])
@pytest.mark.parametrize("scene", list(SCENES))
def test_resample_packed_invariants_oracle_and_fixed_capacity(scene, n):
    from morpheus_amd import _lib
    stage = int(_lib.load().mh_resample_stage())
    rs, rc, ts, te, w = SCENES[scene](stage)
    N, M = rs.shape[0], ts.shape[0]
    jit = np.random.default_rng(31).random((N, n)).astype(np.float32)
    jit[:, 0] = 0.0
    jit[:, -1] = np.float32(1 - J.U)                                 # u_{n-1} rounds to 1: at or above every CDF's top
    dev, got = _run_packed(rs, rc, ts, te, w, n, jit)
    assert got["t_starts"].shape[0] == int(np.where(rc > 0, rc + n, 0).sum())
    ro.check_invariants(got, rs, rc, ts, te, n)                      # exact, nothing to a tolerance
    # against the restatements, in the measure: the kernel's draws and the fp32 restatement's, both against the float64 one's
    o32 = ro.resample_packed_np(rs, rc, ts, te, w, n, jit, dtype=np.float32)
    o64 = ro.resample_packed_np(rs, rc, ts, te, w, n, jit, dtype=np.float64)
    e_hip = e_ref = 0.0
    for r in range(N):
        c = int(rc[r])
        if c == 0:
            continue
        sl = slice(int(rs[r]), int(rs[r]) + c)
        a = int(got["ray_start"][r])
        mine = ro.draws_of(got["t_starts"][a:a + c + n], ts[sl])
        u, s32, _ = o32["draws"][r]
        s64 = o64["draws"][r][1]
        e_hip = max(e_hip, float(ro.score(mine, s64, u, ts[sl], te[sl], w[sl]).max()))
        e_ref = max(e_ref, float(ro.score(s32, s64, u, ts[sl], te[sl], w[sl]).max()))
    print(f"{scene} n {n}: worst e of the kernel's draws {e_hip / J.U:.2f} U, of the fp32 restatement's {e_ref / J.U:.2f} U")
    assert J.within(e_hip, e_ref, FACTOR, FLOOR), (e_hip / J.U, e_ref / J.U)
    # the null jitter is j = 0.5
    _, det = _run_packed(rs, rc, ts, te, w, n, None)
    _, half = _run_packed(rs, rc, ts, te, w, n, np.full((N, n), 0.5, dtype=np.float32))
    ro.check_invariants(det, rs, rc, ts, te, n)
    assert all(np.array_equal(det[k], half[k]) for k in det)
    # fixed capacity: the inputs padded to a capacity, outputs of length capacity + n N, n_valid on the device; the first
    # n_valid entries are the ragged result, the rest is the marcher's padding (ray 0, t = 0)
    pad = 37
    z = lambda a: np.concatenate([a, np.zeros(pad, dtype=a.dtype)])
    out_p, got_p = _run_packed(rs, rc, z(ts), z(te), z(w), n, jit, padded=True)
    total = got["t_starts"].shape[0]
    assert out_p[6].dtype == torch.int32 and out_p[6].dim() == 0 and int(out_p[6]) == total
    assert got_p["t_starts"].shape[0] == M + pad + n * N
    for k in ("ray_idx", "t_starts", "t_ends"):
        assert np.array_equal(got_p[k][:total], got[k]) and not got_p[k][total:].any(), k
    assert np.array_equal(got_p["ray_start"], got["ray_start"]) and np.array_equal(got_p["ray_cnt"], got["ray_cnt"])
    # midpoints' positions: the samplers' arithmetic, one rounding per operation
    o = np.random.default_rng(41).standard_normal((N, 3)).astype(np.float32)
    d = np.random.default_rng(42).standard_normal((N, 3)).astype(np.float32)
    out_x, got_x = _run_packed(rs, rc, ts, te, w, n, jit, rays_o=_t(o), rays_d=_t(d))
    assert all(np.array_equal(got_x[k], got[k]) for k in got)
    tm = (got["t_starts"] + got["t_ends"]) / np.float32(2)
    want = o[got["ray_idx"]] + d[got["ray_idx"]] * tm[:, None]
    assert np.array_equal(out_x[5].cpu().numpy(), want.astype(np.float32))


@pytest.mark.parametrize("name", ["T2_uniform", "T65_laplace", "T129_span20", "T200_sparse"])
def test_resample_packed_equals_sample_pdf_on_contiguous_rays(golden, name):
    """both entry points call the one inverse-CDF device function: on contiguous rays the cut points are mh_sample_pdf's samples
    at u_k = (k + j_k) / n, sorted, bit for bit"""
    from morpheus_amd import ops
    bins, w, _, _, _ = _case(golden, name)
    B, T = bins.shape
    rs = (np.arange(B) * (T - 1)).astype(np.int32)
    rc = np.full(B, T - 1, dtype=np.int32)
    ts, te = bins[:, :-1].reshape(-1).copy(), bins[:, 1:].reshape(-1).copy()
    for n in (1, 64, 65):
        jit = np.random.default_rng(n).random((B, n)).astype(np.float32)
        _, got = _run_packed(rs, rc, ts, te, w.reshape(-1), n, jit)
        u = ((np.arange(n, dtype=np.float32)[None] + jit) / np.float32(n)).astype(np.float32)
        dense = ops.sample_pdf(_t(bins), _t(w), _t(u)).cpu().numpy()
        for b in range(B):
            a = int(got["ray_start"][b])
            assert np.array_equal(ro.draws_of(got["t_starts"][a:a + T - 1 + n], bins[b, :-1]), np.sort(dense[b])), (name, n, b)


def test_importance_sampling_arguments():
    """sigmas go through the compositor's weights kernel; n_importance = 0 returns the input; det is the null jitter"""
    from morpheus_amd import resample, volrend
    rs, rc, ts, te, w = _scene([5, 0, 40, 9, 3, 4], seed=51)
    d_rs, d_rc, d_ts, d_te = _t(rs), _t(rc), _t(ts), _t(te)
    sig = torch.rand(ts.shape[0], device=DEV) * 30
    wts = volrend.render_weight_from_density(d_ts, d_te, sig, packed_info=torch.stack((d_rs, d_rc), 1))[0]
    jit = torch.rand(6, 16, device=DEV)
    a = resample.importance_sampling(d_rs, d_rc, d_ts, d_te, 16, sigmas=sig, jitter=jit)
    b = resample.importance_sampling(d_rs, d_rc, d_ts, d_te, 16, weights=wts, jitter=jit)
    assert len(a) == len(b) == 5 and all(torch.equal(x, y) for x, y in zip(a, b))
    z = resample.importance_sampling(d_rs, d_rc, d_ts, d_te, 0, weights=wts)
    assert z[1] is d_ts and z[2] is d_te and z[3] is d_rs and z[4] is d_rc
    assert torch.equal(z[0].long(), torch.repeat_interleave(torch.arange(6, device=DEV), d_rc.long()))
    det = resample.importance_sampling(d_rs, d_rc, d_ts, d_te, 16, weights=wts, det=True)
    half = resample.importance_sampling(d_rs, d_rc, d_ts, d_te, 16, weights=wts, jitter=torch.full((6, 16), 0.5, device=DEV))
    assert all(torch.equal(x, y) for x, y in zip(det, half))
    o, d = torch.randn(6, 3, device=DEV), torch.randn(6, 3, device=DEV)
    x = resample.importance_sampling(d_rs, d_rc, d_ts, d_te, 16, weights=wts, jitter=jit, with_xyz=(o, d),
                                     n_valid=torch.tensor(ts.shape[0], dtype=torch.int32, device=DEV))
    assert len(x) == 7 and x[5].shape == (ts.shape[0] + 16 * 6, 3) and int(x[6]) == b[1].shape[0]
    assert torch.equal(x[1][:int(x[6])], b[1])


def test_fixed_capacity_resampling_under_graph_capture():
    """No host synchronisation in the fixed-capacity form: the call is captured into a graph (a synchronising call inside a
    capture is an error); two replays leave the bytes of the eager run.  One stream, one chain, as the pruning test captures."""
    from morpheus_amd import ops
    rs, rc, ts, te, w = _scene([5, 0, 400, 9, 65, 3, 4], seed=61)
    pad, n, N = 100, 24, 7
    z = lambda a: _t(np.concatenate([a, np.zeros(pad, dtype=a.dtype)]))
    args = (z(w), z(ts), z(te), _t(rs), _t(rc), n, torch.rand(N, n, device=DEV))

    def body():
        out = ops.resample_packed(*args, padded=True)
        return out[0], out[1], out[2], out[3], out[4], out[6]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            eager = [t.clone() for t in body()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert int(eager[5]) == int(np.where(rc > 0, rc + n, 0).sum())
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        outs = body()
    ops.graph_replace_memset_nodes(g)        # small memset nodes replay wrongly on this runtime (csrc/graph.hip), as trainstep does
    g.instantiate()
    for _ in range(2):
        for t in outs:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager):
            assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------------------------ renderer
def _view(hw):
    o, d, t, rid = synth.frame_rays(25, hw, hw)
    return dict(rays_o=o.to(DEV), rays_d=d.to(DEV), rays_t=t.to(DEV), rays_id=rid.to(DEV), H=hw, W=hw)


def _renderer(model, n_rays, S=16):
    from morpheus_amd.render import HotPathRenderer, UniformSampler
    jit = synth.ray_jitter(n_rays).to(DEV)
    return HotPathRenderer(model, model.config, UniformSampler(S, model.bound, jit), 200)


PER_RAY = ("image", "depth", "weights_sum")
PER_SAMPLE = ("sdf", "weights", "deform")


def test_render_with_importance_equals_render_of_the_refined_samples():
    """64 rays, UniformSampler(16), n_importance = 16 with a given jitter: the keys and per-ray shapes of a plain render, outputs
    and parameter gradients torch.equal to a render through PresetSampler fed what importance_sampling returns for the same
    densities and jitter; backward runs and every gradient is finite."""
    from morpheus_amd import harness, resample
    from morpheus_amd.render import HotPathRenderer, PresetSampler
    hw, S, n = 8, 16, 16
    data = _view(hw)
    N = hw * hw
    args = (data["rays_o"], data["rays_d"], data["rays_t"], data["rays_id"], hw, hw)
    timg, tdep = (v.to(DEV) for v in synth.targets(N))
    model = harness.build_model("b", DEV).train()
    for k_ in ("normal_smoothness", "normal_smooth_3d"):
        model.config["train"][k_] = 0.0
    Jit = torch.rand(N, n, device=DEV)

    def run(r):
        model.zero_grad(set_to_none=True)
        res = r.render_rays(*args, ambient_ratio=1.0, shading="albedo")
        harness.bench_loss(res, timg, tdep).backward()
        return res, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    plain, _ = run(_renderer(model, N, S))
    rend = _renderer(model, N, S)
    rend.importance = dict(n_importance=n, jitter=Jit)
    res_a, g_a = run(rend)
    assert set(res_a) == set(plain)
    for k in PER_RAY:
        assert res_a[k].shape == plain[k].shape, k
    for k in PER_SAMPLE:
        assert res_a[k].shape[0] == N * (S + n) and res_a[k].shape[1:] == plain[k].shape[1:], k
    assert len(g_a) >= 20 and all(bool(torch.isfinite(g).all()) for g in g_a.values())
    # the same refinement by hand: the sampler's samples, one density pass, importance_sampling
    sampler = _renderer(model, N, S).occupancy_grid
    o, d, t = (data[k].view(-1, data[k].shape[-1]) for k in ("rays_o", "rays_d", "rays_t"))
    with torch.no_grad(), model.operand_scope():
        ri, ts, te = sampler.sampling(o, d)
        sig = rend._density_fn(o, d, t, False, True)(ts, te, ri)
    ref = resample.importance_sampling(*sampler.packed, ts, te, n, sigmas=sig, jitter=Jit)
    assert ref[1].shape[0] == N * (S + n)
    res_b, g_b = run(HotPathRenderer(model, model.config, PresetSampler(ref[0], ref[1], ref[2]), 200))
    for k in PER_RAY + PER_SAMPLE:
        assert torch.equal(res_a[k], res_b[k]), k
    assert set(g_a) == set(g_b)
    for k in g_a:
        assert torch.equal(g_a[k], g_b[k]), k


def test_render_importance_off_prune_reuse_eval_step_and_empty():
    from morpheus_amd import harness
    from morpheus_amd.occgrid import OccupancyGrid
    from morpheus_amd.render import HotPathRenderer
    hw = 8
    data = _view(hw)
    N = hw * hw
    args = (data["rays_o"], data["rays_d"], data["rays_t"], data["rays_id"], hw, hw)
    model = harness.build_model("b", DEV).eval()
    with torch.no_grad():
        # importance = None is the call as it was: a second renderer object, the same seed
        torch.manual_seed(7)
        a = _renderer(model, N).render_rays(*args, shading="albedo")
        torch.manual_seed(7)
        off = _renderer(model, N)
        off.importance = None
        b = off.render_rays(*args, shading="albedo")
        assert set(a) == set(b)
        for k in PER_RAY + PER_SAMPLE:
            assert torch.equal(a[k], b[k]), k
        # with prune set as well the render has ONE density pass: the pruning pass's values weigh the survivors
        rend = _renderer(model, N)
        rend.prune, rend.importance = dict(early_stop_eps=0.2), dict(n_importance=16, det=True)
        calls, make = [], rend._density_fn

        def counting(*a_, **kw):
            fn = make(*a_, **kw)

            def counted(*x):
                calls.append(x[0].shape[0])
                return fn(*x)
            return counted

        rend._density_fn = counting
        out = rend.render_rays(*args, shading="albedo")
        assert len(calls) == 1 and calls[0] == N * 16
        kept = rend.occupancy_grid.packed[1]
        print(f"prune + importance: {int(kept.sum())} of {N * 16} samples survive the pruning pass")
        assert 0 < int(kept.sum()) <= N * 16
        assert out["sdf"].shape[0] == int(torch.where(kept > 0, kept + 16, 0).sum())
        assert all(bool(torch.isfinite(out[k]).all()) for k in PER_RAY)
        calls.clear()
        rend.prune = None
        rend.render_rays(*args, shading="albedo")
        assert len(calls) == 1
        # eval_step honours it (the draws are torch.rand's here)
        view = _view(12)
        from morpheus_amd.render import UniformSampler
        ev = HotPathRenderer(model, model.config, UniformSampler(16, model.bound), 200)      # chunks of 73 and 71 rays
        ev.importance = dict(n_importance=16)
        rgb, dep = ev.eval_step(view, max_chunk=100)
        assert rgb.shape == (1, 12, 12, 3) and dep.shape == (1, 12, 12)
        assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(dep).all())
        # zero marched samples still render: empty in, empty out, the white image
        grid = OccupancyGrid([-1.01] * 3 + [1.01] * 3, 32).to(DEV)
        empty = HotPathRenderer(model, model.config, grid, 200)
        empty.importance = dict(n_importance=16)
        res = empty.render_rays(*args, shading="albedo")
        assert res["sdf"] is None and bool((res["image"] == 1).all()) and res["image"].shape == (1, N, 3)


def test_fixed_capacity_render_with_importance_equals_the_ragged_render():
    """OccupancyGrid.sample_capacity with `importance` (and with `prune` as well): the refined arrays have the length capacity +
    n N, n_valid counts the refined samples, and the render is the ragged render's bytes; padding rows carry weight 0."""
    from morpheus_amd import harness
    from morpheus_amd.occgrid import OccupancyGrid
    from morpheus_amd.render import HotPathRenderer
    hw, n = 16, 8
    data = _view(hw)
    N = hw * hw
    args = (data["rays_o"], data["rays_d"], data["rays_t"], data["rays_id"], hw, hw)
    model = harness.build_model("b", DEV).eval()
    c = (torch.arange(128).float() + 0.5) / 128 * 2.02 - 1.01
    X, Y, Z = torch.meshgrid(c, c, c, indexing="ij")
    ball = ((X ** 2 + Y ** 2 + Z ** 2).sqrt() < 0.7).to(torch.uint8).contiguous()
    grid = OccupancyGrid([-1.01] * 3 + [1.01] * 3, 128).to(DEV)
    grid.set_binary(ball.to(DEV))
    grid.occs.copy_(ball.reshape(-1).float())
    grid.fixed_jitter = 0.25
    rend = HotPathRenderer(model, model.config, grid, 200)
    rend.importance = dict(n_importance=n, det=True)
    for prune in (None, dict(early_stop_eps=1e-4, alpha_thre=1e-3)):
        rend.prune = prune
        grid.sample_capacity = None
        with torch.no_grad():
            ragged = rend.render_rays(*args, shading="albedo")
            M1 = ragged["sdf"].shape[0]
            kept, hit = int(grid.packed[1].sum()), int((grid.packed[1] > 0).sum())       # of the render's own sampling call
            marched = int(grid.sampling(data["rays_o"][0], data["rays_d"][0], render_step_size=model.config["render"]["step_size"])[0].numel())
            assert M1 == kept + n * hit and 0 < hit <= N and kept <= marched
            grid.sample_capacity = (marched + 1024) // 1024 * 1024
            capped = rend.render_rays(*args, shading="albedo")
        assert int(grid.overflow) == 0 and int(capped["n_valid"]) == M1
        assert capped["weights"].shape[0] == grid.sample_capacity + n * N
        assert torch.equal(capped["image"], ragged["image"]) and torch.equal(capped["depth"], ragged["depth"])
        assert torch.equal(capped["weights"][:M1], ragged["weights"]) and not capped["weights"][M1:].any()
