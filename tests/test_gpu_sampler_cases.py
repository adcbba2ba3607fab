"""GPU: the five kernels of csrc/sampler.hip and the Python around them (ops.march_rays, march_rays_capped, march_count,
generate_rays, sample_uniform, rays_sample_uniform) against the fp32 restatements, at every case of tests/sampler_cases.py.
These kernels have no tolerance: every comparison is torch.equal (tests/test_sampler_cases_host.py shows on the CPU that the cases
reach the loop trips, slot edges and retries they name, and that the fp32 definition is the intended one).

The marcher cases call mh_march_slots directly with a slot row of the test's own length into buffers filled with a sentinel,
with a guard behind the last row: a kernel that writes past a ray's row is seen in the next row or in the guard."""
import numpy as np
import pytest
import torch

from oracle import field as of
from tests import sampler_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(t):
    return None if t is None else t.to(DEV)


def _run_slots(o, d, jit, step, bound, grid, cap):
    """mh_march_slots with a slot row of `cap` -> (ray_cnt [N], rows_ts [N,cap], rows_te [N,cap], guard_ts, guard_te, flag,
    cnt_guard) on the CPU"""
    from morpheus_amd._lib import launch, ptr
    N, R = o.shape[0], grid.shape[0]
    cnt = torch.full((N + 2,), sc.CNT_SENTINEL, dtype=torch.int32, device=DEV)          # [ray_cnt | flag | guard]
    cnt[N] = 0
    bufs = torch.full((2, N * cap + sc.guard_len(cap)), sc.SENTINEL, device=DEV)
    launch("mh_march_slots", ptr(o), ptr(d), ptr(jit), N, float(step), float(bound), R, ptr(grid), cap, ptr(cnt), ptr(bufs[0]),
           ptr(bufs[1]), cnt.data_ptr() + 4 * N)
    cnt, bufs = cnt.cpu(), bufs.cpu()
    return (cnt[:N], bufs[0, :N * cap].view(N, cap), bufs[1, :N * cap].view(N, cap), bufs[0, N * cap:], bufs[1, N * cap:],
            int(cnt[N]), int(cnt[N + 1]))


def _check_slots(c, m, tag):
    o, d, jit, grid = _dev(c["o"]), _dev(c["d"]), _dev(c["jitter"]), _dev(c["grid"])
    for cap in c["caps"]:
        want_cnt, want_s, want_e, want_flag = sc.slot_expect(m, cap)
        cnt, rows_s, rows_e, guard_s, guard_e, flag, cnt_guard = _run_slots(o, d, jit, c["step"], c["bound"], grid, cap)
        what = (tag, c["name"], cap)
        assert flag == want_flag, what
        assert torch.equal(cnt, want_cnt), (what, cnt.tolist(), want_cnt.tolist())       # min(n, cap), every ray written
        # the row prefix bit for bit and the sentinel behind it: want_* hold SENTINEL beyond ray_cnt
        assert torch.equal(rows_s, want_s) and torch.equal(rows_e, want_e), what
        assert bool((guard_s == sc.SENTINEL).all()) and bool((guard_e == sc.SENTINEL).all()) and cnt_guard == sc.CNT_SENTINEL, what


@pytest.mark.parametrize("u", sc.JITTERS, ids=["nojit", "jit0", "jit1-"])
def test_march_slots_caps_counts_grids(u):
    """cap in {1, 21, 63, 64, 65, 128, 129} x five grids (R = 1, 2, 3, 5, 128) x 58 rays whose step counts sit at cap - 1, cap,
    cap + 1: flag, ray_cnt = min(n, cap), the row prefix, the sentinel behind it, the guard row"""
    for c in sc.marcher_cases():
        if c["u"] == u:
            _check_slots(c, sc.march_full(c["o"], c["d"], c["jitter"], c["step"], c["bound"], c["grid"]), "caps")


def test_march_slots_small_batches():
    """N = 1, 3, 4, 5: four rays per workgroup, the last workgroup partly and exactly filled"""
    for c in sc.small_n_cases():
        _check_slots(c, sc.march_full(c["o"], c["d"], c["jitter"], c["step"], c["bound"], c["grid"]), "N")


def test_nonfinite_rays_are_misses_everywhere():
    """The eight rows of the miss rule through the slot marcher, march_rays (which must not retry), march_rays_capped,
    march_count and the uniform sampler"""
    from morpheus_amd import ops
    for c in sc.nonfinite_cases():
        m = sc.march_full(c["o"], c["d"], c["jitter"], c["step"], c["bound"], c["grid"])
        _check_slots(c, m, "nonfinite")
        args = (_dev(c["o"]), _dev(c["d"]), _dev(c["jitter"]), c["step"], c["bound"], _dev(c["grid"]))
        ri, ts, te, rs, rc = ops.march_rays(*args)
        assert torch.equal(ri.cpu().long(), m["ri"]) and torch.equal(ts.cpu(), m["ts"]) and torch.equal(te.cpu(), m["te"]), c["name"]
        assert torch.equal(rc.cpu().long(), m["cnt"]) and bool((rc.cpu()[torch.from_numpy(c["miss"])] == 0).all())
        assert int(ops.march_count(*args)) == m["ri"].numel()
        out = ops.march_rays_capped(*args, capacity=1024)
        assert int(out[6]) == 0 and int(out[5]) == m["ri"].numel() and torch.equal(out[1][:int(out[5])].cpu(), m["ts"])
    o, d, names, miss = sc.nonfinite_rows()
    miss = torch.from_numpy(miss)
    for S in (1, 7, 257):
        for u in sc.UNIFORM_JITTERS:
            _check_uniform(o, d, sc.jitter_tensor(u, 8), S, True, ("nonfinite", S, u))
            ts = ops.sample_uniform(_dev(o), _dev(d), _dev(sc.jitter_tensor(u, 8)), S, sc.BOUND)[1].cpu().view(8, S)
            assert bool((ts[miss] == 0).all())


def test_march_rays_retries_with_a_longer_slot_row(monkeypatch):
    """The retry path of ops.march_rays at the real mh_march_cap = 21: a direction scaled by 1/3 (one doubling) and by 1/10
    (several); full grid (n > cap) and empty grid (unwalked steps only).  The packed result is the oracle's for every ray."""
    from morpheus_amd import _lib, ops
    assert int(_lib.load().mh_march_cap(sc.RETRY_STEP, sc.RETRY_BOUND)) == sc.RETRY_CAP
    caps_seen = []
    real = ops._timed

    def spy(name, *args, **kw):
        if name == "mh_march_slots":
            caps_seen.append(args[8])
        return real(name, *args, **kw)

    monkeypatch.setattr(ops, "_timed", spy)
    for c in sc.retry_cases():
        m = c["oracle"]
        del caps_seen[:]
        args = (_dev(c["o"]), _dev(c["d"]), _dev(c["jitter"]), c["step"], c["bound"], _dev(c["grid"]))
        ri, ts, te, rs, rc = ops.march_rays(*args)
        assert caps_seen == c["caps_visited"], (c["name"], caps_seen)
        assert torch.equal(ri.cpu().long(), m["ri"]) and torch.equal(ts.cpu(), m["ts"]) and torch.equal(te.cpu(), m["te"]), c["name"]
        assert torch.equal(rc.cpu().long(), m["cnt"]) and torch.equal(rs.cpu().long(), torch.cumsum(m["cnt"], 0) - m["cnt"])
        count = int(ops.march_count(*args))
        if len(c["caps_visited"]) == 1:
            assert count == m["ri"].numel()
        else:
            # march_count does not read the flag: a LOWER BOUND, the overflowing ray counted at the slot-row length
            assert count == int(torch.minimum(m["cnt"], torch.tensor(sc.RETRY_CAP)).sum()) and \
                (count < m["ri"].numel() or c["name"].endswith("empty"))
        # the fixed-capacity form reports the slot-row overflow instead of retrying
        assert int(ops.march_rays_capped(*args, capacity=512)[6]) == int(len(c["caps_visited"]) > 1)


def test_pack_counts_and_capacities():
    """march_pack at per-ray counts 65, 1, 63, 64, 129 with empty rays between; march_rays_capped at capacities equal to the
    total, one below it, inside a ray, at ray boundaries, below the first ray's count and 1"""
    from morpheus_amd import ops
    c = sc.pack_case()
    m = sc.march_full(c["o"], c["d"], c["jitter"], c["step"], c["bound"], c["grid"])
    args = (_dev(c["o"]), _dev(c["d"]), _dev(c["jitter"]), c["step"], c["bound"], _dev(c["grid"]))
    ri, ts, te, rs, rc = ops.march_rays(*args)
    assert torch.equal(ri.cpu().long(), m["ri"]) and torch.equal(ts.cpu(), m["ts"]) and torch.equal(te.cpu(), m["te"])
    assert rc.cpu().tolist() == list(c["counts"]) and torch.equal(rs.cpu().long(), torch.cumsum(m["cnt"], 0) - m["cnt"])
    assert int(ops.march_count(*args)) == c["total"]
    ri, ts, te = ri.cpu(), ts.cpu(), te.cpu()
    for name, capacity in c["capacities"].items():
        ri_c, ts_c, te_c, start, cnt_c, n_valid, overflow = [t.cpu() for t in ops.march_rays_capped(*args, capacity=capacity)]
        w_start, w_cnt, w_valid, w_ovf = sc.capped_expect(m["cnt"], capacity)
        assert ri_c.shape == ts_c.shape == te_c.shape == (capacity,), name
        assert int(n_valid) == w_valid and int(overflow) == w_ovf, (name, int(n_valid), int(overflow))
        n = w_valid
        assert torch.equal(ri_c[:n], ri[:n]) and torch.equal(ts_c[:n], ts[:n]) and torch.equal(te_c[:n], te[:n]), name
        assert bool((ri_c[n:] == 0).all()) and bool((ts_c[n:] == 0).all()) and bool((te_c[n:] == 0).all()), name   # padding
        assert int(cnt_c.sum()) == n and bool((start.long() + cnt_c.long() <= capacity).all()), name
        assert torch.equal(cnt_c.long(), w_cnt) and torch.equal(start.long(), w_start), name


def test_march_count_checks_and_empty_batch():
    from morpheus_amd import ops
    grid = torch.ones(2, 2, 2, dtype=torch.uint8, device=DEV)
    e = torch.zeros(0, 3, device=DEV)
    z = ops.march_count(e, e, None, 0.01, 1.01, grid)
    assert z.dtype == torch.int32 and z.dim() == 0 and int(z) == 0 and z.is_cuda
    assert all(t.numel() == 0 for t in ops.march_rays(e, e, None, 0.01, 1.01, grid))
    o = torch.tensor([[0.0, 0.0, 2.0]], device=DEV)
    d = torch.tensor([[0.0, 0.0, -1.0]], device=DEV)
    for bad in (grid.float(), grid[:, :, ::2], grid[0]):            # the assertions march_rays / march_rays_capped make
        for fn in (ops.march_count, ops.march_rays):
            with pytest.raises(AssertionError):
                fn(o, d, None, 0.01, 1.01, bad)
        with pytest.raises(AssertionError):
            ops.march_rays_capped(o, d, None, 0.01, 1.01, bad, capacity=8)


def test_march_count_equals_march_rays_total_on_the_marcher_cases():
    from morpheus_amd import ops
    for c in sc.marcher_cases():
        if c["gname"] in ("random_R128", "single_R3", "random_R5"):
            args = (_dev(c["o"]), _dev(c["d"]), _dev(c["jitter"]), c["step"], c["bound"], _dev(c["grid"]))
            ri, ts, te, rs, rc = ops.march_rays(*args)
            m = sc.march_full(c["o"], c["d"], c["jitter"], c["step"], c["bound"], c["grid"])
            assert torch.equal(ri.cpu().long(), m["ri"]) and torch.equal(ts.cpu(), m["ts"]) and torch.equal(te.cpu(), m["te"]), c["name"]
            assert int(ops.march_count(*args)) == ri.numel() == m["ri"].numel(), c["name"]


# ------------------------------------------------------------------------------------------------- uniform sampler, rays
def _check_uniform(o, d, jit, S, with_xyz, what):
    from morpheus_amd import ops
    w_ri, w_ts, w_te, w_xyz, w_rs, w_rc = sc.uniform_expect(o, d, jit, S, sc.BOUND)
    ri, ts, te, xyz, rs, rc = ops.sample_uniform(_dev(o), _dev(d), _dev(jit), S, sc.BOUND, with_xyz=with_xyz)
    assert torch.equal(ri.cpu(), w_ri) and torch.equal(ts.cpu(), w_ts) and torch.equal(te.cpu(), w_te), what
    assert torch.equal(rs.cpu(), w_rs) and torch.equal(rc.cpu(), w_rc), what
    assert (xyz is None) == (not with_xyz)
    if with_xyz:
        assert sc.same_values(xyz.cpu(), w_xyz), what


@pytest.mark.parametrize("S", sc.UNIFORM_S)
def test_sample_uniform_bins_blocks_and_special_rays(S):
    for name, (o, d) in sc.uniform_ray_sets().items():
        if name == "nonfinite":
            continue                                                # test_nonfinite_rays_are_misses_everywhere
        for u in sc.UNIFORM_JITTERS:
            for with_xyz in (True, False):
                _check_uniform(o, d, sc.jitter_tensor(u, o.shape[0]), S, with_xyz, (name, S, u, with_xyz))


@pytest.mark.parametrize("c", sc.raygen_cases(), ids=lambda c: c["name"])
def test_generate_rays_against_the_restatement(c):
    from morpheus_amd import ops
    o, d = ops.generate_rays(c["fx"], c["fy"], c["cx"], c["cy"], c["c2w"], c["H"], c["W"], DEV)
    w_o, w_d = sc.pixel_rays(c["fx"], c["fy"], c["cx"], c["cy"], c["c2w"], c["H"], c["W"])
    assert torch.equal(o.cpu(), w_o) and torch.equal(d.cpu(), w_d)


@pytest.mark.parametrize("c", sc.fused_cases(), ids=lambda c: c["name"])
def test_fused_rays_and_samples_equal_the_two_kernels(c):
    """mh_rays_sample_uniform == mh_generate_rays -> gather -> mh_sample_uniform bit for bit, and both equal the restatements;
    drawn pixels (repeated, the last one) and the whole image (pix = NULL)"""
    from morpheus_amd import ops
    K = (c["fx"], c["fy"], c["cx"], c["cy"])
    o_all, d_all = ops.generate_rays(*K, c["c2w"], c["H"], c["W"], DEV)
    for pix in (c["pix"], None):
        idx = np.arange(c["H"] * c["W"]) if pix is None else pix
        N = len(idx)
        sel = torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(DEV)
        w_o, w_d = sc.pixel_rays(*K, c["c2w"], c["H"], c["W"], pix)
        for S in sc.UNIFORM_S:
            for u in sc.UNIFORM_JITTERS:
                jit = sc.jitter_tensor(u, N)
                for with_xyz in (True, False):
                    what = (c["name"], pix is None, S, u, with_xyz)
                    fused = ops.rays_sample_uniform(*K, c["c2w"], c["H"], c["W"], None if pix is None else torch.from_numpy(pix).to(DEV),
                                                    _dev(jit), S, sc.BOUND, with_xyz=with_xyz)
                    two = (o_all[sel].contiguous(), d_all[sel].contiguous()) + tuple(
                        ops.sample_uniform(o_all[sel].contiguous(), d_all[sel].contiguous(), _dev(jit), S, sc.BOUND, with_xyz=with_xyz))
                    for a, b in zip(fused, two):
                        assert (a is None and b is None) or torch.equal(a, b), what
                    want = (w_o, w_d) + sc.uniform_expect(w_o, w_d, jit, S, sc.BOUND)
                    for k, (a, b) in enumerate(zip(fused, want)):
                        if a is not None:
                            assert torch.equal(a.cpu(), b), (what, k)
