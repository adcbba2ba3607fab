"""csrc/adan.hip and optim.FlatAdan against float64 (tests/adan_oracle.py holds the rule, the scales and the golden's access;
tests/test_adan_host.py pins them on the CPU against the reference class's recorded results).

The rule is step_f64_oracle.judge, as for the Adam step: errors are |x - float64| over the quantity's natural scale (adan_oracle's
docstring lists them); the kernel's worst error stays within 2 x the fp32 yardstick's own worst on the same inputs (floor: 4 roundings
of the scale), with at most 2 x (+ 2) as many elements above that floor.  The fp32 yardstick is the reference class's own fp32 result
where the golden has one and the oracle in fp32 elsewhere.  Everything else is exact: skipped elements, guard words, the gradient
buffer as g c, counters, bit-identical repeats.

Worst figures of one run on an MI355X (error / scale; worst over the module's checks of the quantity):

    quantity        scale (adan_oracle)            at the ABI: kernel / fp32 oracle    FlatAdan: kernel / the reference's fp32 class
    p               |p| + ss + sd                  1.59e-07 / 1.59e-07                 1.41e-07 / 1.41e-07
    g' (bucket)     |g'|                           9.34e-08 / 9.34e-08                 9.82e-08 / 1.11e-07
    exp_avg         b1 |m| + (1 - b1) |g'|         1.21e-07 / 1.21e-07                 1.36e-07 / 1.50e-07
    exp_avg_sq      b3 n + (1 - b3) Q^2            1.20e-07 / 1.20e-07                 2.45e-07 / 2.98e-07
    exp_avg_diff    b2 |d| + (1 - b2) D            1.40e-07 / 1.40e-07                 1.38e-07 / 1.36e-07
    neg_pre_grad    |g'|                           9.34e-08 / 9.34e-08                 9.82e-08 / 1.11e-07
    last_clip against the reference's c: at most 1.33 U (bound 2 U); the sum of squares of 2^20 + 3 gradients: 0.13 U (bound 2 U).
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import adan_oracle as A
from tests import step_f64_oracle as S
from tests.f64_judge import flat64

pytestmark = pytest.mark.gpu
DEV = "cuda"
MH_ERR_ARG = 1
SENTINEL = -77.25
B1, B2, B3 = A.BETAS
EPS, WD = 1e-8, 2e-2


def _status(name, *args):
    """call a stream-taking entry point of the C ABI and hand back its status instead of raising"""
    from morpheus_amd import _lib
    _lib.load()
    return _lib._fns[name](*args, _lib.stream())


def _guarded(a, n):
    """a device buffer of n elements (16-byte aligned) with 8 sentinel elements behind it"""
    buf = torch.full((n + 8,), SENTINEL, device=DEV)
    buf[:n] = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return buf


def _workspace():
    """-> (the workspace as floats with 8 sentinel floats behind it, its size in floats)"""
    from morpheus_amd import _lib
    words = int(_lib.load().mh_adan_workspace_bytes()) // 4
    ws = torch.zeros(words + 8, device=DEV)
    ws[words:] = SENTINEL
    return ws, words


def _step(bufs, n, ends, lrs, steps, flags, no_prox, max_grad_norm, ws, eps=EPS, wd=WD, betas=A.BETAS):
    ns = len(ends)
    return _status("mh_adan_step", *[b if isinstance(b, int) else b.data_ptr() for b in bufs], n, ns, (ctypes.c_int64 * ns)(*ends),
                   (ctypes.c_double * ns)(*lrs), (ctypes.c_int64 * ns)(*steps), (ctypes.c_int32 * ns)(*flags), *betas, eps, wd,
                   max_grad_norm, int(no_prox), ws if isinstance(ws, int) else ws.data_ptr())


def _pool(records, key, hip, ref32, f64, scale):
    h, c, r, s = records.setdefault(key, ([], [], [], []))
    for lst, t in ((h, hip), (c, ref32), (r, f64), (s, scale)):
        lst.append(flat64(t))


def _judge_pool(records, prefix):
    return {key: S.judge(*(torch.cat(x) for x in v), f"{prefix} {key}") for key, v in records.items()}


def _layout(n, kind):
    """step_f64_oracle.adam_layout for Adan: its step counts become GROUP steps (a skipped segment's group is at step 5), its
    skipped segments the skip flag; every third stepped segment sees its first gradient (a group step of 1 implies that too)
    -> ends, lrs, group steps, flags, first (what the kernel must treat as a first gradient)"""
    ends, steps, lrs = S.adam_layout(n, kind)
    flags = [A.SKIP if t == 0 else (A.FIRST if s % 3 == 0 else 0) for s, t in enumerate(steps)]
    gsteps = [5 if t == 0 else t for t in steps]
    return ends, lrs, gsteps, flags, _first(flags, gsteps)


def _first(flags, gsteps):
    return [bool(f & A.FIRST) or t == 1 for f, t in zip(flags, gsteps)]


def _state(n):
    """step_f64_oracle.adam_state (p, m, v as exp_avg_sq; gradient scales 1e-18 .. 1e4) plus live exp_avg_diff and neg_pre_grad of
    the element's scale; i % 7 == 0: all four states zero -> the six host arrays (p, g, m, n, d, q) with g zero, and the state"""
    st = S.adam_state(n)
    rng = np.random.RandomState(611 + n)
    d, q = (rng.randn(n) * 0.2 * st["scale"]).astype(np.float32), (rng.randn(n) * st["scale"]).astype(np.float32)
    z = np.arange(n) % 7 == 0
    d[z], q[z] = 0.0, 0.0
    return [st["p"], np.zeros(n, np.float32), st["m"], st["v"], d, q], st


def _read(bufs, n):
    return [b[:n].cpu().numpy() for b in bufs]


def _check(bufs, ws, words, before, n, ends, lrs, gsteps, skip, first, no_prox, max_grad_norm, pool, tag, wd=WD):
    """the six buffers after a step against the float64 rule and its fp32 restatement from the state `before`; guards intact,
    skipped elements bit-identical in all six, the gradient buffer exactly g c with the workspace's c; -> the buffers as read"""
    torch.cuda.synchronize()
    got = _read(bufs, n)
    for b in bufs:
        assert bool((b[n:] == SENTINEL).all()), "a write behind the bucket"
    assert bool((ws[words:] == SENTINEL).all()), "a write behind the workspace"
    seg = A.seg_of(ends, n)
    on, first_e = ~np.asarray(skip, bool)[seg], np.asarray(first, bool)[seg]
    g = before[1]
    c_dev = ws[:3].cpu().numpy()
    c64 = A.clip_factor(g, on, max_grad_norm, EPS, np.float64)
    c32 = A.clip_factor(g, on, max_grad_norm, EPS, np.float32)
    if max_grad_norm == 0:
        assert c_dev.tolist() == [1.0, 0.0, 0.0], "no clipping: c = 1, no norm pass"
    else:
        ssq = A.sum_squares(g, on)
        assert abs(float(c_dev[1]) - ssq) <= 2 * A.U * ssq and abs(float(c_dev[0]) - float(c64)) <= A.U * float(c64), (c_dev, ssq, c64)
    assert (c_dev[0] == 1.0) == (float(c64) == 1.0)
    for b, a in zip(got, before):
        assert np.array_equal(b.view(np.int32)[~on], a.view(np.int32)[~on]), "a skipped element changed"
    # with clipping the bucket holds g' = g c, bit for bit (c = 1 leaves the bits as they were)
    assert np.array_equal(got[1].view(np.int32)[on], (g * c_dev[0])[on].view(np.int32)), "the gradient buffer is g c"
    par32 = [a[seg] for a in A.seg_params(lrs, gsteps, wd, no_prox, round32=True)]
    par64 = [a[seg] for a in A.seg_params(lrs, gsteps, wd, no_prox, round32=False)]
    f32 = A.adan(*before, *par32, on, first_e, c32, np.float32, eps=EPS, no_prox=no_prox)
    f64 = A.adan(*before, *par64, on, first_e, c64, np.float64, eps=EPS, no_prox=no_prox)
    scales = A.scales(*before, par64[0], par64[1], on, first_e, c64)
    for key, h, c, r, s in zip(A.NAMES, got, f32, f64, scales):
        _pool(pool, f"{key}{tag}", h, c, r, s)
    return got


def _clip_setting(kind, g, on):
    """max_grad_norm for "off" (0), "inactive" (far above the norm: c = 1 exactly) and "active" (0.37 of the norm)"""
    norm = float(np.sqrt(A.sum_squares(g, on)))
    return {"off": 0.0, "inactive": float(np.float32(1e3 * norm)), "active": float(np.float32(0.37 * norm))}[kind]


@pytest.mark.parametrize("no_prox", [False, True])
@pytest.mark.parametrize("clip", ["off", "inactive", "active"])
def test_single_steps_at_the_abi(no_prox, clip):
    """mh_adan_step on raw buffers, n = 1025 in adam_layout's mixed layout (zero-length segments, lanes that straddle segments,
    stepped and skipped segments alternating, first gradients mixed in, group steps 1, 2, 10, 1000, 10^6, a learning rate of 0);
    three steps, each judged from the kernel's own buffers before it."""
    n = 1025
    ends, lrs, gsteps, flags, first = _layout(n, "mixed")
    skip = [bool(f & A.SKIP) for f in flags]
    on = ~np.asarray(skip)[A.seg_of(ends, n)]
    host, st = _state(n)
    bufs = [_guarded(a, n) for a in host]
    ws, words = _workspace()
    pool = {}
    for it in range(3):
        g = S.adam_grad(st, it)
        bufs[1][:n] = torch.from_numpy(g).to(DEV)
        before = _read(bufs, n)
        mgn = _clip_setting(clip, g, on)
        steps = [t + it for t in gsteps]
        first_it = _first(flags, steps)
        assert _step(bufs, n, ends, lrs, steps, flags, no_prox, mgn, ws) == 0
        got = _check(bufs, ws, words, before, n, ends, lrs, steps, skip, first_it, no_prox, mgn, pool, "")
        c = float(ws[0])
        assert (c == 1.0) if clip != "active" else (0.3 < c < 0.4), c
        if clip != "active":
            assert np.array_equal(got[1].view(np.int32), g.view(np.int32)), "c = 1: the gradient buffer keeps its bits"
    _judge_pool(pool, f"Adan at the ABI, no_prox {no_prox}, clipping {clip}:")


def test_sizes_and_160_segments():
    """n = 1, 3, 4, 5 (the cnt < 4 tail of a lane, alone and behind a full lane) in one segment and in the mixed layout, and 160
    segments over 1025 elements (two prologue launches); one clipped step each"""
    pool = {}
    for n, kind in [(k, kind) for k in (1, 3, 4, 5) for kind in ("one", "mixed")] + [(1025, "160")]:
        ends, lrs, gsteps, flags, first = _layout(n, kind)
        assert kind != "160" or len(ends) == 160
        skip = [bool(f & A.SKIP) for f in flags]
        on = ~np.asarray(skip)[A.seg_of(ends, n)]
        host, st = _state(n)
        host[1] = S.adam_grad(st, 0)
        bufs = [_guarded(a, n) for a in host]
        ws, words = _workspace()
        mgn = _clip_setting("active", host[1], on) if on.any() and A.sum_squares(host[1], on) > 0 else 5.0
        assert _step(bufs, n, ends, lrs, gsteps, flags, False, mgn, ws) == 0, (n, kind)
        _check(bufs, ws, words, host, n, ends, lrs, gsteps, skip, first, False, mgn, pool, "")
    _judge_pool(pool, "Adan, sizes and 160 segments:")


def test_norm_skips_segments_without_gradient_and_repeats_bit_for_bit():
    """n = 2^20 + 3 over 512 workgroups of the norm pass; the two skipped segments hold 1e30, which must not count; the sum of
    squares within two fp32 roundings of the float64 sum (double partial sums: the accumulation error n 2^-53 is far below),
    c within one; a second call on the same gradients gives the same bits"""
    n = 2 ** 20 + 3
    ends = [1000, 5003, 2 ** 19 + 1, 2 ** 19 + 6, n]
    flags = [0, A.SKIP, 0, A.SKIP, 0]
    seg = A.seg_of(ends, n)
    on = ~np.asarray([bool(f) for f in flags])[seg]
    rng = np.random.RandomState(3)
    g = (rng.randn(n) * 10.0 ** (rng.rand(n) * 3.0 - 3.0)).astype(np.float32)
    g[~on] = 1e30
    zeros = torch.zeros(n, device=DEV)
    bufs = [zeros.clone() for _ in range(6)]
    ws, words = _workspace()
    ssq = A.sum_squares(g, on)
    seen = []
    for _ in range(2):
        bufs[1].copy_(torch.from_numpy(g))
        assert _step(bufs, n, ends, [1e-3] * 5, [3] * 5, flags, False, 5.0, ws) == 0
        torch.cuda.synchronize()
        seen.append(ws[:3].cpu().numpy().copy())
        assert bool((ws[words:] == SENTINEL).all())
    c, sumsq, norm = (float(x) for x in seen[0])
    print(f"sum of squares {sumsq!r} vs float64 {ssq!r}: {abs(sumsq - ssq) / ssq / A.U:.3f} U; c {c!r}")
    assert abs(sumsq - ssq) <= 2 * A.U * ssq
    exact = 5.0 / (np.sqrt(ssq) + EPS)
    assert exact < 1.0 and abs(c - exact) <= A.U * exact and abs(norm - np.sqrt(ssq)) <= A.U * np.sqrt(ssq)
    assert np.array_equal(seen[0].view(np.int32), seen[1].view(np.int32)), "two calls, two results"
    after = bufs[1].cpu().numpy()
    assert np.array_equal(after[~on].view(np.int32), g[~on].view(np.int32)), "a skipped gradient was scaled"
    assert np.array_equal(after[on].view(np.int32), (g * np.float32(c))[on].view(np.int32))


def test_argument_errors_touch_nothing():
    """161 segments, decreasing ends, a last end that is not n, each of the six buffers and the workspace offset by 4 bytes, a
    negative eps, weight decay or max_grad_norm, a beta of 1, a flag with unknown bits, a step of 0 on a stepped segment:
    MH_ERR_ARG, and all six buffers and the workspace as they were"""
    n = 1025
    ends, lrs, gsteps, flags, _ = _layout(n, "mixed")
    host, st = _state(n)
    host[1] = S.adam_grad(st, 0)
    bufs = [_guarded(a, n) for a in host]
    ws, words = _workspace()
    ws[:words] = 3.5
    ok = dict(ends=ends, lrs=lrs, steps=gsteps, flags=flags)
    bad = [("161 segments", dict(ends=list(range(160)) + [n], lrs=[1e-3] * 161, steps=[1] * 161, flags=[0] * 161)),
           ("decreasing ends", dict(ends=[10, 5, n], lrs=[1e-3] * 3, steps=[1] * 3, flags=[0] * 3)),
           ("last end below n", dict(ends=[10, n - 1], lrs=[1e-3] * 2, steps=[1] * 2, flags=[0] * 2)),
           ("last end beyond n", dict(ends=[10, n + 1], lrs=[1e-3] * 2, steps=[1] * 2, flags=[0] * 2)),
           ("unknown flag bits", dict(ok, flags=[4] + flags[1:])),
           ("step 0 on a stepped segment", dict(ok, steps=[0 if f == 0 else t for f, t in zip(flags, gsteps)])),
           ("negative learning rate", dict(ok, lrs=[-1e-3] + lrs[1:]))]
    for what, a in bad:
        assert _step(bufs, n, a["ends"], a["lrs"], a["steps"], a["flags"], False, 5.0, ws) == MH_ERR_ARG, what
    for what, kw in [("negative eps", dict(eps=-1e-8)), ("negative weight decay", dict(wd=-1e-2)), ("beta1 = 1", dict(betas=(1.0, B2, B3))),
                     ("beta2 < 0", dict(betas=(B1, -0.1, B3))), ("beta3 = NaN", dict(betas=(B1, B2, float("nan"))))]:
        assert _step(bufs, n, ends, lrs, gsteps, flags, False, 5.0, ws, **kw) == MH_ERR_ARG, what
    assert _step(bufs, n, ends, lrs, gsteps, flags, False, -5.0, ws) == MH_ERR_ARG, "negative max_grad_norm"
    for which in range(6):
        ptrs = [b.data_ptr() + (4 if i == which else 0) for i, b in enumerate(bufs)]
        assert _step(ptrs, n, ends, lrs, gsteps, flags, False, 5.0, ws) == MH_ERR_ARG, f"buffer {which} offset by 4 bytes"
    assert _step(bufs, n, ends, lrs, gsteps, flags, False, 5.0, ws.data_ptr() + 4) == MH_ERR_ARG, "workspace offset by 4 bytes"
    torch.cuda.synchronize()
    for b, a in zip(bufs, host):
        assert np.array_equal(b[:n].cpu().numpy().view(np.int32), a.view(np.int32)) and bool((b[n:] == SENTINEL).all())
    assert bool((ws[:words] == 3.5).all()) and bool((ws[words:] == SENTINEL).all())
    assert _step(bufs, n, ends, lrs, gsteps, flags, False, 5.0, ws) == 0, "the same buffers with good arguments are accepted"


def test_step_dev_flags_and_seen_counters_in_one_process():
    """mh_adan_step_dev: per-segment device flags 0, 0.5, 1, 2, -1, NaN -- only a positive flag steps; the counts of gradients seen
    go up by exactly one there and nowhere else; a count of 0 before (or a group step of 1) makes it a first gradient; results
    against the same float64 rule with the same per-element values; two consecutive calls"""
    n = 2049
    ends, _, lrs = S.adam_layout(n, "mixed")
    ns = len(ends)
    flags = np.array([(0.0, 0.5, 1.0, 2.0, -1.0, float("nan"))[(s + 1) % 6] for s in range(ns)], np.float32)
    seen = np.array([(0, 0, 3, 1)[s % 4] for s in range(ns)], np.int64)
    gsteps = [(1, 2, 10, 1000, 10 ** 6)[s % 5] for s in range(ns)]
    on_s = flags > 0                                   # NaN > 0 is false
    assert int(on_s.sum()) >= 6 and int((~on_s).sum()) >= 6 and int((on_s & (seen == 0)).sum()) >= 2 and int((on_s & (seen > 0)).sum()) >= 2
    host, st = _state(n)
    bufs = [_guarded(a, n) for a in host]
    ws, words = _workspace()
    flag_d, seen_d = torch.from_numpy(flags).to(DEV), torch.from_numpy(seen).to(DEV)
    for it in range(2):
        g = S.adam_grad(st, it)
        bufs[1][:n] = torch.from_numpy(g).to(DEV)
        before = _read(bufs, n)
        steps = [t + it for t in gsteps]
        mgn = _clip_setting("active", g, on_s[A.seg_of(ends, n)])
        status = _status("mh_adan_step_dev", *[b.data_ptr() for b in bufs], n, ns, (ctypes.c_int64 * ns)(*ends),
                         (ctypes.c_double * ns)(*lrs), (ctypes.c_int64 * ns)(*steps), flag_d.data_ptr(), seen_d.data_ptr(), *A.BETAS,
                         EPS, WD, mgn, 1, ws.data_ptr())
        assert status == 0
        first = [(c == 0) or t == 1 for c, t in zip(seen, steps)]
        seen = seen + on_s
        assert np.array_equal(seen_d.cpu().numpy(), seen), "seen: + 1 where the flag is positive, untouched elsewhere"
        pool = {}
        _check(bufs, ws, words, before, n, ends, lrs, steps, ~on_s, first, True, mgn, pool, f", call {it + 1}")
        _judge_pool(pool, "Adan, device-side flags:")


# --------------------------------------------------------------------------------------------------------------- optim.FlatAdan
def _flat_adan(run, dev=DEV):
    from morpheus_amd.optim import FlatAdan
    G = A.golden()
    s = A.golden_step(run, 0, False)
    ps = [torch.nn.Parameter(torch.zeros(int(k), device=dev)) for k in G["sizes"]]
    groups = [{"name": "a", "params": ps[:3], "lr": 5e-3}, {"name": "b", "params": ps[3:], "lr": 1e-3}]
    return ps, FlatAdan(groups, eps=s["eps"], weight_decay=s["weight_decay"], max_grad_norm=s["max_grad_norm"], no_prox=s["no_prox"],
                        foreach=False)


def _set_step(ps, opt, s, sd):
    """the golden's state before the step into the optimiser, its parameters and its gradients (None where the golden has None)"""
    G = A.golden()
    opt.load_state_dict(sd)
    ends = np.cumsum(G["sizes"])
    opt.zero_grad()
    with torch.no_grad():
        for i, (p, e, k) in enumerate(zip(ps, ends, G["sizes"])):
            p.copy_(torch.from_numpy(s["before_p"][e - k:e].copy()))
            p.grad = torch.from_numpy(s["grads"][e - k:e].copy()).to(p.device) if s["has_grad"][i] else None


def _flat(opt, what):
    buf = {"p": opt.flat_p, "g": opt.bucket.flat}.get(what)
    buf = getattr(opt, what) if buf is None else buf
    return torch.cat([buf[o:o + k] for _, o, k in opt._views]).cpu().numpy()


@pytest.mark.parametrize("run", [0, 1, 2, 3])
def test_flat_adan_against_the_reference_class(run):
    """FlatAdan through load_state_dict / step against tests/golden/adan.npz, step by step: every step starts from the golden's
    fp32 state, the reference's own fp32 result is the yardstick, its float64 step the truth.  Group steps 1..6, the late parameter
    has state from its first gradient on, parameters with grad None keep their bits beside stepping lane neighbours, every stepped
    parameter's version counter moves, `last_clip` is the reference's c to 2 U; group "b"'s lr is halved BY NAME before step 4."""
    ps, opt = _flat_adan(run)
    pool = {}
    for step in range(6):
        s = A.golden_step(run, step, False)
        sd = A.golden_state_dict(run, step)
        if step == 3:
            sd["param_groups"][1]["lr"] = 1e-3              # as it was; the new value arrives the way update_learning_rate sets it
        _set_step(ps, opt, s, sd)
        if step == 3:
            for g in opt.param_groups:
                if g["name"] == "b":
                    g["lr"] = g["lr"] * 0.5
        assert [g["lr"] for g in opt.param_groups] == s["lrs"].tolist()
        versions = [p._version for p in ps]
        before_p = [p.detach().clone() for p in ps]
        opt.step()
        torch.cuda.synchronize()
        assert [g["step"] for g in opt.param_groups] == [step + 1, step + 1] == s["steps_after"].tolist()
        state = opt.state_dict()["state"]
        assert sorted(state) == [i for i in range(6) if s["seen_after"][i]], "state exactly for the parameters that have had a gradient"
        for i, p in enumerate(ps):
            if s["has_grad"][i]:
                assert p._version > versions[i], f"parameter {i}: the version counter did not move"
            else:
                assert torch.equal(p.detach().view(torch.int32), before_p[i].view(torch.int32)), f"parameter {i} has no gradient"
        c = float(opt.last_clip)
        print(f"run {run} step {step + 1}: c {c!r}, reference {float(s['c32'])!r}: {abs(c - s['c32']) / s['c32'] / A.U:.2f} U; float64 {s['c64']!r}")
        assert abs(c - s["c32"]) <= 2 * A.U * s["c32"]
        scales = A.scales(s["before_p"], s["grads"], *(s["before_" + k] for k in A.KEYS), s["ss"], s["sd"], s["on"], s["first"], s["c64"],
                          betas=s["betas"])
        for name, sc in zip(A.NAMES, scales):
            got = _flat(opt, name)
            if name != "g":        # (p.grad of a parameter without gradient is the bucket's zeros here and None in the reference)
                assert np.array_equal(got[~s["on"]].view(np.int32), s["after32_" + name][~s["on"]].view(np.int32)), name
            _pool(pool, name, got, s["after32_" + name], s["after64_" + name], sc)
    _judge_pool(pool, f"FlatAdan against the reference class, run {run}:")


def test_flat_adan_restart_and_data_parallel_bookkeeping(monkeypatch):
    """restart_opt() (steps 0, m, n, d zero: the next step is a first one for everybody), and the several-rank path in one process:
    with the bucket's all-reduced flags set by hand, mh_adan_step_dev must leave the bits mh_adan_step leaves, and the device-side
    `seen` counts reach state_dict()"""
    from morpheus_amd import optim
    run = 1
    results = []
    for several in (False, True):
        ps, opt = _flat_adan(run)
        monkeypatch.setattr(optim, "_multi_rank", lambda several=several: several)
        for step in (2, 3):
            s = A.golden_step(run, step, False)
            _set_step(ps, opt, s, A.golden_state_dict(run, step))
            if step == 3:
                opt.restart_opt()
                assert [g["step"] for g in opt.param_groups] == [0, 0]
            if several:
                opt.bucket.collect()
                opt.bucket._flags.copy_(torch.from_numpy(s["has_grad"].astype(np.float32)))
                opt.bucket.exchanged = True
            opt.step()
            if step == 3:
                assert [g["step"] for g in opt.param_groups] == [1, 1]
        sd = opt.state_dict()
        assert sorted(sd["state"]) == [0, 1, 2, 3, 4, 5]
        results.append([_flat(opt, k) for k in A.NAMES] + [float(opt.last_clip)])
    for a, b, name in zip(*results, A.NAMES + ("c",)):
        assert np.array_equal(np.asarray(a).view(np.int32 if name != "c" else np.int64), np.asarray(b).view(np.int32 if name != "c" else np.int64)), name
    # after restart_opt the step is the rule from zero moments with every gradient a first one
    s = A.golden_step(run, 3, False)
    el = s["element_tensor"]
    grp = A.golden()["group_of"][el]
    ss, sd_, bc3s, decay = (a[grp] for a in A.seg_params(s["lrs"], [1, 1], s["weight_decay"], s["no_prox"], s["betas"], round32=False))
    zero = np.zeros_like(s["before_p"])
    c64 = A.clip_factor(s["grads"], s["on"], s["max_grad_norm"], s["eps"], np.float64)
    first = np.ones_like(s["on"])
    args = (s["before_p"], s["grads"], zero, zero, zero, s["before_neg_pre_grad"])
    f64 = A.adan(*args, ss, sd_, bc3s, decay, s["on"], first, c64, np.float64, betas=s["betas"], eps=s["eps"], no_prox=s["no_prox"])
    r32 = [a[grp] for a in A.seg_params(s["lrs"], [1, 1], s["weight_decay"], s["no_prox"], s["betas"], round32=True)]
    f32 = A.adan(*args, *r32, s["on"], first, A.clip_factor(s["grads"], s["on"], s["max_grad_norm"], s["eps"], np.float32), np.float32,
                 betas=s["betas"], eps=s["eps"], no_prox=s["no_prox"])
    for name, h, c, r, sc in zip(A.NAMES, results[0], f32, f64, A.scales(*args, ss, sd_, s["on"], first, c64, betas=s["betas"])):
        S.judge(torch.from_numpy(h), torch.from_numpy(c), torch.from_numpy(r), torch.from_numpy(sc), f"FlatAdan after restart_opt: {name}")
