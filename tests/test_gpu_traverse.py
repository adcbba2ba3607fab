"""GPU: `OccGridEstimator(traversal="dda")` on mh_est_traverse_slots (csrc/estimator.hip) -- ray_indices, t_starts, t_ends and
`packed` bit for bit against the fp32 restatement (tests/traverse_oracle.py) at every case, the slot rows themselves (sentinel-filled,
with a guard behind the last row), the doubling retry, fixed capacity without a host read, pruning, HotPathRenderer taking the
placement unchanged, and the lattice untouched by it.  tests/test_traverse_host.py asserts that every case reaches what it names."""
import numpy as np
import pytest
import torch

from morpheus_amd import synth
from tests import estimator_oracle as eo
from tests import sampler_cases as sc
from tests import traverse_oracle as to
from tests import visibility_oracle as vo

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
CASES = {c["name"]: c for c in to.cases()}


def _same(got, want, what):
    g, w = got.cpu().numpy(), want.cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), what


def _dev(t):
    return None if t is None else t.to(DEV)


@pytest.fixture(scope="module")
def oracle():
    """every case's restatement, computed once"""
    return {name: to.run_case(c) for name, c in CASES.items()}


@pytest.fixture(scope="module")
def estimators():
    from morpheus_amd.estimator import OccGridEstimator
    out = {}
    for name, (root, res, levels) in {"full8": (to.BOX1, 8, 1), "rand40": (to.BOX40, 40, 1), "levels3": (eo.ROOT, eo.RES, eo.LEVELS),
                                      "empty": (eo.ROOT, eo.RES, eo.LEVELS)}.items():
        aabbs, binaries = to.GRIDS[name]()
        est = OccGridEstimator(root, resolution=res, levels=levels).to(DEV)
        est.set_binary(binaries.to(DEV))
        _same(est.aabbs, aabbs, name + " aabbs")
        est.traversal = "dda"
        out[name] = est
    return out


def _sample(est, c, **kw):
    est.fixed_jitter = _dev(c["jitter"])
    try:
        return est.sampling(c["o"].to(DEV), c["d"].to(DEV), near_plane=c["near_plane"], far_plane=c["far_plane"], t_min=_dev(c["t_min"]),
                            t_max=_dev(c["t_max"]), render_step_size=c["step"], cone_angle=c["cone_angle"], **kw)
    finally:
        est.fixed_jitter = None


def _check(est, out, m, what, capacity=None):
    ri, ts, te = out
    rs, rc = est.packed
    M = int(m["cnt"].sum())
    want_rs, want_rc = eo.packed_of(m)
    if capacity is None:
        assert est.n_valid is None
    else:
        assert ri.shape == ts.shape == te.shape == (capacity,) and int(est.n_valid) == M and int(est.overflow) == 0
        assert not ri[M:].any() and not ts[M:].any() and not te[M:].any()
        ri, ts, te = ri[:M], ts[:M], te[:M]
    assert ri.dtype == torch.int32
    _same(ri, m["ri"].to(torch.int32), what + " ray_indices")
    _same(ts, m["ts"], what + " t_starts")
    _same(te, m["te"], what + " t_ends")
    _same(rs, want_rs, what + " packed start")
    _same(rc, want_rc, what + " packed cnt")


def _slots(est, c, cap):
    """mh_est_traverse_slots with a slot row of `cap` into sentinel-filled buffers with a guard behind the last row"""
    from morpheus_amd import ops
    N = c["o"].shape[0]
    cnt = torch.full((N + 2,), sc.CNT_SENTINEL, dtype=torch.int32, device=DEV)          # [ray_cnt | flag | guard]
    cnt[N] = 0
    bufs = torch.full((2, N * cap + sc.guard_len(cap)), sc.SENTINEL, device=DEV)
    o, d, j = c["o"].to(DEV), c["d"].to(DEV), _dev(c["jitter"])
    tmn, tmx = _dev(c["t_min"]), _dev(c["t_max"])
    b8 = est.binaries.view(torch.uint8)
    ptr = lambda t: None if t is None else t.data_ptr()
    ops.launch("mh_est_traverse_slots", ptr(o), ptr(d), ptr(j), ptr(tmn), ptr(tmx), N, c["step"], c["cone_angle"], c["near_plane"],
               c["far_plane"], est.aabbs.data_ptr(), est.levels, *est._res, b8.data_ptr(), cap, cnt.data_ptr(), bufs[0].data_ptr(),
               bufs[1].data_ptr(), cnt.data_ptr() + 4 * N)
    cnt, bufs = cnt.cpu(), bufs.cpu()
    return (cnt[:N], bufs[0, :N * cap].view(N, cap), bufs[1, :N * cap].view(N, cap), bufs[:, N * cap:], int(cnt[N]), int(cnt[N + 1]))


def _check_slots(est, c, m, cap):
    want_cnt, want_s, want_e, want_flag = sc.slot_expect(m, cap)
    cnt, rows_s, rows_e, guard, flag, cnt_guard = _slots(est, c, cap)
    what = (c["name"], cap)
    assert flag == want_flag, what
    assert torch.equal(cnt, want_cnt), (what, cnt.tolist(), want_cnt.tolist())
    assert torch.equal(rows_s, want_s) and torch.equal(rows_e, want_e), what           # the sentinel stays behind ray_cnt
    assert bool((guard == sc.SENTINEL).all()) and cnt_guard == sc.CNT_SENTINEL, what


# ------------------------------------------------------------------------------------------------ 1 - 6: the restatement's bits
@pytest.mark.parametrize("name", ["full8", "rand40", "levels3", "degenerate", "planes", "rand40-cone", "levels3-cone"])
def test_traversal_equals_restatement(estimators, oracle, name):
    c, m = CASES[name], oracle[name]
    est = estimators[c["grid"]]
    assert int(m["cnt"].sum()) > 0
    _check(est, _sample(est, c), m, name)
    # the slot rows at the real bound: no flag, the sentinel behind every row
    from morpheus_amd import _lib
    cap = int(_lib.load().mh_est_march_cap(c["step"], est._diagonal, c["near_plane"], c["far_plane"]))
    assert cap >= int(m["cnt"].max())
    _check_slots(est, c, m, cap)


# ---------------------------------------------------------------------------------------------------------- 7: nothing occupied
def test_empty_grid_writes_nothing(estimators, oracle):
    c, m = CASES["empty"], oracle["empty"]
    est = estimators["empty"]
    for cap in (1, 64, 130):
        cnt, rows_s, rows_e, guard, flag, cnt_guard = _slots(est, c, cap)
        assert flag == 0 and not cnt.any() and cnt_guard == sc.CNT_SENTINEL
        assert bool((rows_s == sc.SENTINEL).all()) and bool((rows_e == sc.SENTINEL).all()) and bool((guard == sc.SENTINEL).all())
    ri, ts, te = _sample(est, c)
    assert ri.numel() == ts.numel() == te.numel() == 0 and not est.packed[1].any()


# ------------------------------------------------------------------------------------------------------- 8: slot-row overflow
def test_slot_row_overflows_once_and_is_retried(estimators, monkeypatch):
    from morpheus_amd import ops
    est = estimators["full8"]
    c = to.overflow_case()
    m = to.run_case(c)
    caps = []
    timed = ops._timed

    def counting(name, *args, **kw):
        if name == "mh_est_traverse_slots":
            caps.append(args[16])
        assert name != "mh_est_march_slots"
        return timed(name, *args, **kw)

    monkeypatch.setattr(ops, "_timed", counting)
    _check(est, _sample(est, c), m, "overflow")
    assert caps == [c["cap"], 2 * c["cap"]]
    monkeypatch.setattr(ops, "_timed", timed)
    # direct launches with short rows: nothing past cap, the flag set; at twice the bound the flag is clear
    for cap in (1, 40, 64, c["cap"], 2 * c["cap"]):
        _check_slots(est, c, m, cap)
    assert sc.slot_expect(m, c["cap"])[3] == 1 and sc.slot_expect(m, 2 * c["cap"])[3] == 0


# ----------------------------------------------------------------------------------------------- 9: fixed capacity, no host read
def _capture(body):
    """capture body() into a HIP graph the way tests/test_gpu_estimator.py does: a device->host read inside a capture is an error"""
    from morpheus_amd import ops
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()                                                           # warm the allocator outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        outs = body()
    ops.graph_replace_memset_nodes(g)
    g.instantiate()
    return g, outs


def test_sample_capacity_pads_and_replays_in_a_graph(estimators, oracle, monkeypatch):
    from morpheus_amd import ops
    c, m = CASES["levels3-cone"], oracle["levels3-cone"]
    est = estimators["levels3"]
    cap = int(m["cnt"].sum()) + 19
    launches = []
    timed = ops._timed

    def counting(name, *args, **kw):
        launches.append(name)
        return timed(name, *args, **kw)

    monkeypatch.setattr(ops, "_timed", counting)
    est.sample_capacity, est.overflow = cap, None
    try:
        _check(est, _sample(est, c), m, "capped", capacity=cap)
        assert launches == ["mh_est_traverse_slots", "mh_march_pack"]      # one march, no retry, one pack
        monkeypatch.setattr(ops, "_timed", timed)
        # a capacity inside the batch truncates and raises the flag
        est.sample_capacity, est.overflow = cap // 2, None
        ri, ts, te = _sample(est, c)
        assert int(est.overflow) == 1 and int(est.n_valid) == cap // 2
        _same(ts, m["ts"][:cap // 2], "truncated t_starts")
        # captured: no host read on the way, and the replay leaves the same bytes
        o, d, j = c["o"].to(DEV), c["d"].to(DEV), c["jitter"].to(DEV)
        est.sample_capacity, est.overflow, est.fixed_jitter = cap, torch.zeros((), dtype=torch.int32, device=DEV), j

        def sample():
            ri, ts, te = est.sampling(o, d, render_step_size=c["step"], cone_angle=c["cone_angle"])
            return ri, ts, te, est.packed[0], est.packed[1], est.n_valid

        g, outs = _capture(sample)
        for t in outs:
            t.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        M = int(outs[5])
        assert M == cap - 19 and int(est.overflow) == 0
        _same(outs[0][:M], m["ri"].to(torch.int32), "replayed ray_indices")
        _same(outs[1][:M], m["ts"], "replayed t_starts"), _same(outs[2][:M], m["te"], "replayed t_ends")
        assert not outs[1][M:].any()
    finally:
        est.sample_capacity, est.fixed_jitter, est.overflow = None, None, None


# ------------------------------------------------------------------------------------------------------------------ 10: pruning
def test_pruning_keeps_what_the_visibility_oracle_keeps(estimators, oracle):
    c, m = CASES["levels3"], oracle["levels3"]
    est = estimators["levels3"]
    est.occs.copy_(synth.hash_tensor((est.occs.numel(),), 7400, 0.05, 0.04).to(DEV))      # in [-0.01, 0.09): some invisible
    calls = []

    def sigma_fn(t_starts, t_ends, ray_indices):
        # multiplications by powers of two, floor and differences of nearby values: the same bits on the host and on the device
        calls.append((t_starts.clone(), t_ends.clone(), ray_indices.clone()))
        x = t_starts * 4.0
        return 2.0 + 32.0 * (x - torch.floor(x))

    rs0, rc0 = (t.numpy() for t in eo.packed_of(m))
    ts0, te0 = m["ts"], m["te"]
    sig = sigma_fn(ts0, te0, m["ri"]).numpy()
    try:
        for eps, a_thre in ((1e-4, 0.0), (1e-2, 0.5), (0.0, 0.5)):
            calls.clear()
            ri, ts, te = _sample(est, c, sigma_fn=sigma_fn, early_stop_eps=eps, alpha_thre=a_thre)
            # the density function saw the traversal's own marched samples, once
            assert len(calls) == 1
            _same(calls[0][0], ts0, "marched t_starts"), _same(calls[0][1], te0, "marched t_ends")
            _same(calls[0][2], m["ri"].to(torch.int32), "marched ray_indices")
            vis = est.occs[est.occs >= 0]
            thre = float(torch.clamp(vis.double().mean().float(), max=a_thre)) if a_thre > 0 else 0.0
            mk = vo.mask(sig, ts0.numpy(), te0.numpy(), rs0, rc0, eps, thre, f64=True)
            src = est.src_index.cpu().numpy()
            keep = np.zeros(ts0.numel(), np.uint8)
            keep[src] = 1
            diff = keep != mk["keep"]
            assert not (diff & ~vo.band(mk, eps, thre)).any() and diff.sum() <= vo.BAND_CAP * keep.size
            assert 0 < keep.sum() < keep.size, (eps, a_thre)
            want = vo.pack(keep, ts0.numpy(), te0.numpy(), rs0, rc0)
            for g, w in zip((ri, ts, te) + est.packed + (est.src_index,), want):
                assert g.cpu().numpy().tobytes() == w.tobytes()
    finally:
        est.occs.zero_()


# ----------------------------------------------------------------------------------------------------------------- 11: renderer
def test_hot_path_renderer_takes_the_traversal_unchanged():
    """HotPathRenderer on 64 rays with estimator.traversal = "dda" against the same renderer fed the restatement's samples through
    render.PresetSampler: every output equal bit for bit"""
    from morpheus_amd import harness
    from morpheus_amd.estimator import OccGridEstimator
    from morpheus_amd.render import HotPathRenderer, PresetSampler
    hw = 8
    o, d, t, rid = (x.to(DEV) for x in synth.frame_rays(25, hw, hw))
    model = harness.build_model("b", DEV).eval()
    cc = (torch.arange(16).float() + 0.5) / 16 * 2.02 - 1.01
    X, Y, Z = torch.meshgrid(cc, cc, cc, indexing="ij")
    ball = ((X ** 2 + Y ** 2 + Z ** 2).sqrt() < 0.7)
    box = [-1.01] * 3 + [1.01] * 3
    est = OccGridEstimator(box, 16).to(DEV)
    est.set_binary(ball.to(DEV))
    est.fixed_jitter = 0.25
    est.traversal = "dda"
    step = model.config["render"]["step_size"]
    m = to.traverse(o.view(-1, 3).cpu(), d.view(-1, 3).cpu(), torch.full((hw * hw,), 0.25), step, est.aabbs.cpu(), ball[None].to(torch.uint8))
    assert int(m["cnt"].sum()) > 500 and m["N"] == 64
    preset = PresetSampler(m["ri"].to(torch.int32).to(DEV), m["ts"].to(DEV), m["te"].to(DEV))
    outs = []
    for sampler in (est, preset):
        rend = HotPathRenderer(model, model.config, sampler, 200)
        with torch.no_grad():
            outs.append(rend.render_rays(o, d, t, rid, hw, hw, shading="albedo"))
    a, b = outs
    assert set(a) == set(b) and a["sdf"].shape[0] == int(m["cnt"].sum())
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] is None and b[k] is None or a[k] == b[k], k
    # and the lattice gives this renderer other samples: the attribute is what chose
    est.traversal = "lattice"
    with torch.no_grad():
        lat = HotPathRenderer(model, model.config, est, 200).render_rays(o, d, t, rid, hw, hw, shading="albedo")
    assert lat["sdf"].shape[0] != a["sdf"].shape[0] or not torch.equal(lat["sdf"], a["sdf"])


# ------------------------------------------------------------------------------------------------- 12: the lattice is untouched
def test_lattice_and_default_still_return_the_march():
    from morpheus_amd import ops
    from morpheus_amd.estimator import OccGridEstimator
    c = CASES["levels3"]
    aabbs, binaries = to.grid_levels3()
    est = OccGridEstimator(eo.ROOT, resolution=eo.RES, levels=eo.LEVELS).to(DEV)
    est.set_binary(binaries.to(DEV))
    o, d, j = c["o"].to(DEV), c["d"].to(DEV), c["jitter"].to(DEV)
    want = ops.est_march_rays(o, d, j, c["step"], est.aabbs, est.binaries.view(torch.uint8), est._diagonal)
    m = eo.march(c["o"], c["d"], c["jitter"], c["step"], aabbs, binaries)
    _same(want[1], m["ts"], "est_march_rays t_starts")
    if hasattr(est, "traversal"):
        assert est.traversal == "lattice"
    for setting in (None, "lattice"):
        if setting is not None:
            est.traversal = setting
        got = _sample(est, c)
        for g, w, what in zip(got + est.packed, want, ("ray_indices", "t_starts", "t_ends", "ray_start", "ray_cnt")):
            _same(g, w, f"{setting}: {what}")
