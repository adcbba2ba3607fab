"""tests/step_f64_oracle.py on the CPU: the conditions tests/test_gpu_step_f64.py relies on.  Every case builder is run here and shown
to deliver the counts, tails, lanes and values it names; the fp32 restatement's error against float64 is finite and non-zero on
every case, so that the tolerance derived from it is never vacuous and never infinite; the float64 definitions are checked against
the project's restatement of the reference (oracle/field.py) and against torch.optim.Adam."""
import numpy as np
import pytest
import torch

from oracle import field as of
from tests import step_f64_oracle as S
from tests.f64_judge import scaled_errors

F32, F64 = torch.float32, torch.float64


def _measure(x32, x64, scale):
    e, bad = scaled_errors(x32, x64, scale)
    assert bad == 0 and e.numel() > 0
    worst = float(e.max())
    assert np.isfinite(worst) and worst > 0.0, "the restatement's own error must be finite and non-zero"
    return worst


# ============================================================================================================ compositor
def test_composite_main_case_counts_and_placed_samples():
    c = S.composite_main_case()
    cnt = c["cnt"]
    assert set(S.COUNTS) <= set(cnt) and cnt[0] == 0 and cnt[-1] == 0
    assert any(a == 0 and b == 0 for a, b in zip(cnt[:-1], cnt[1:])), "two adjacent 0-count rays"
    assert c["N"] == 33 and c["N"] % 4 == 1
    start = np.cumsum([0] + cnt[:-1])
    sd = (c["sigma"] * (c["te"] - c["ts"])).double().numpy()
    assert bool(torch.isfinite(c["sigma"]).all()) and bool((c["te"] >= c["ts"]).all())
    for big in S.OPAQUE_SD:
        for at in S.OPAQUE_AT:
            r, k = c["placed"][f"opaque {big:g} @{at}"]
            assert k == at and (k % 64, k // 64) == {0: (0, 0), 63: (63, 0), 64: (0, 1), 128: (0, 2)}[at]
            ray = sd[start[r]:start[r] + cnt[r]]
            assert cnt[r] == at + 4 and abs(ray[k] / big - 1) < 1e-6
            assert ray[:k].sum() < 0.3 and (ray[:k] > 0).all() and ray[k + 1:].max() < 3e-3, "a thin prefix, thin samples behind"
    r, ks = c["placed"]["sigma = 0"]
    assert all(float(c["sigma"][start[r] + k]) == 0.0 for k in ks) and {k % 64 for k in ks} >= {0, 63} and max(ks) >= 64
    r, ks = c["placed"]["ts == te"]
    assert all(float(c["ts"][start[r] + k]) == float(c["te"][start[r] + k]) for k in ks)
    r, k = c["placed"]["underflow"]
    ray = sd[start[r]:start[r] + cnt[r]].astype(np.float32)
    T = np.exp(-np.concatenate([[0.0], np.cumsum(ray, dtype=np.float32)[:-1]]).astype(np.float32))
    dead = np.nonzero(T == 0)[0]
    assert 0 < dead[0] % 64 < 63 and dead[0] // 64 == 0 and abs(int(dead[0]) - k) <= 1, "fp32 transmittance reaches 0 mid-chunk"
    assert bool((c["g_w"][start[r] + dead[0]:start[r] + cnt[r]] != 0).all()), "live gradients behind the underflow"
    r, _ = c["placed"]["thin"]
    ray = sd[start[r]:start[r] + cnt[r]]
    assert cnt[r] == 200 and ray.min() > 4e-7 and ray.max() < 3e-6
    # the drawn rays: optical depth over 1e-7 .. 1e2, and translucent rays that keep weight in their last chunk
    drawn = sd[:int(start[16])]
    assert drawn.min() < 1e-6 and drawn.max() > 50.0
    with torch.no_grad():
        w = S.composite(c["sigma"].double(), c["ts"], c["te"], None, cnt)[0]
    for r in (14, 15):            # 350 and 1025 samples
        assert cnt[r] in (350, 1025) and float(w[start[r] + cnt[r] - 30:start[r] + cnt[r]].sum()) > 1e-4


@pytest.mark.parametrize("N", S.RAY_COUNTS)
def test_composite_ray_count_cases(N):
    c = S.composite_rays_case(N)
    assert c["N"] == N and len(c["cnt"]) == N and N % 4 == {1: 1, 3: 3, 4: 0, 5: 1, 257: 1}[N]
    if N == 257:
        assert c["cnt"][0] == 0 and c["cnt"][100] == c["cnt"][101] == 0 and c["cnt"][256] == 66 and 2000 < c["M"] < 8000


def test_composite_restatement_errors_are_finite_and_non_zero():
    for build in (S.composite_main_case, lambda: S.composite_rays_case(5), lambda: S.composite_rays_case(257)):
        c = build()
        variants = S.VARIANTS if c["N"] == 33 else ("wodc",)
        r64, r32 = S.composite_run(c, F64, variants), S.composite_run(c, F32, variants)
        sc = S.composite_scales(c, r64)
        for k in "wodc":
            _measure(r32[k], r64[k], sc[k])
        for var in variants:
            scv = S.composite_scales(c, r64, var)
            _measure(r32["grads"][var][0], r64["grads"][var][0], scv["d_sigma"])
            if "c" in var:
                _measure(r32["grads"][var][1], r64["grads"][var][1], scv["d_rgb"])
            else:
                assert bool((r64["grads"][var][1] == 0).all()) and bool((scv["d_rgb"] == 0).all())
    n64, n32 = S.composite_run(c, F64, ("wod",), with_rgb=False), S.composite_run(c, F32, ("wod",), with_rgb=False)
    _measure(n32["grads"]["wod"][0], n64["grads"]["wod"][0], S.composite_scales(c, n64, "wod", with_rgb=False)["d_sigma"])


def test_composite_definition_is_the_oracles_on_the_existing_ragged_case():
    """the float64 definition against oracle/field.py:render_weights_loop (python double arithmetic on the fp32 sigma dt, returned
    in fp32) on the ragged case of tests/test_gpu_ops.py: equal to the rounding of the fp32 result"""
    from morpheus_amd import synth
    from tests.test_gpu_ops import _ragged_samples
    N = 300
    ri, ts, te, cnt = _ragged_samples(N, 5)
    sig = synth.hash_tensor((ri.shape[0],), 77, 20.0, 20.0)
    w_loop = of.render_weights_loop(ts, te, sig, ri, N)
    with torch.no_grad():
        w64, o64, _, _ = S.composite(sig.double(), ts, te, None, [int(c) for c in cnt])
    assert float(((w64 - w_loop.double()).abs() / w64.clamp(min=1e-30)).max()) <= 2.0 ** -24 * (1 + 1e-6)
    assert float((o64 - of.accumulate(w64, None, ri, N)[:, 0]).abs().max()) <= 1e-14
    # and the gradient convention: the VALUE of sd is the fp32 product, d sd / d sigma the fp32 difference
    s = sig.double().requires_grad_(True)
    sd = S.form_sd(s, ts, te)
    assert torch.equal(sd.detach(), (sig * (te - ts)).double())
    sd.sum().backward()
    assert torch.equal(s.grad, (te - ts).double())


def test_composite_nonfinite_cases_and_layouts():
    clean, nan, inf = S.composite_nonfinite_case(), S.composite_nonfinite_case("nan"), S.composite_nonfinite_case("inf")
    assert clean["cnt"] == S.NONFINITE_COUNTS and clean["N"] == 12
    assert S.NONFINITE_AT[0] // 4 == 1, "the NaN ray sits in the middle workgroup of three"
    ray, k = S.ray_index(clean["cnt"])
    for case, at, test in ((nan, S.NONFINITE_AT, torch.isnan), (inf, S.INF_AT, torch.isinf)):
        bad = ~torch.isfinite(case["sigma"])
        assert int(bad.sum()) == 1 and bool(test(case["sigma"][bad]).all())
        assert (int(ray[bad]), int(k[bad])) == at
        assert torch.equal(case["sigma"][~bad], clean["sigma"][~bad]) and torch.equal(case["ts"], clean["ts"])
    assert S.INF_AT[1] // 64 == 1 and S.INF_AT[1] < S.NONFINITE_COUNTS[S.INF_AT[0]] - 1
    with torch.no_grad():
        w, o, d, col = S.composite(inf["sigma"].double(), inf["ts"], inf["te"], inf["rgb"].double(), inf["cnt"])
        w32 = S.composite(inf["sigma"], inf["ts"], inf["te"], inf["rgb"], inf["cnt"])[0]
    assert all(bool(torch.isfinite(t).all()) for t in (w, o, d, col, w32)), "the definition is finite at sigma = +inf"
    at = (ray == S.INF_AT[0]) & (k == S.INF_AT[1])
    assert float(w[at]) > 0.05 and bool((w[(ray == S.INF_AT[0]) & (k > S.INF_AT[1])] == 0).all())
    start, M, owned = S.composite_padded_layout(clean["cnt"])
    assert M == clean["M"] + 77 and owned.numel() == clean["M"] and int(owned[-1]) == M - 8
    assert [start[r + 1] - start[r] - clean["cnt"][r] for r in range(11)] == [3, 0, 1, 0, 0, 0, 0, 66, 0, 0, 0]
    other, idx = S.composite_reorder(clean, list(range(11, -1, -1)))
    assert other["cnt"] == clean["cnt"][::-1] and torch.equal(other["sigma"][:7], clean["sigma"][-7:]) and torch.equal(other["sigma"], clean["sigma"][idx])


# =========================================================================================================== weight norm
def test_weight_norm_calls_rows_columns_and_boundaries():
    tails, waves, cols = set(), set(), set()
    for name, spec in S.WN_CALLS.items():
        assert len(spec["rows"]) == len(spec["cols"]) and set(spec["rows"]) <= {1, 2, 3, 5, 128}
        ends = np.cumsum(spec["rows"])
        tails.add(int(ends[-1]) % 4)
        waves |= {int(e) % 4 for e in ends[:-1]}
        cols |= set(spec["cols"])
    assert tails == {1, 2, 3} and waves == {0, 1, 2, 3} and cols == set(S.WN_COLS) == {1, 2, 63, 64, 65, 127, 128, 129, 300}
    assert sorted(len(s["rows"]) for s in S.WN_CALLS.values()) == [1, 9, 32]
    assert {r for s in S.WN_CALLS.values() for r in s["rows"]} == {1, 2, 3, 5, 128}


@pytest.mark.parametrize("kind", S.WN_GRAD_KINDS)
def test_weight_norm_case_values_and_restatement_error(kind):
    c = S.wnorm_case("nine", kind)
    e = torch.cat([torch.log2(v.double().abs().amax(1)) for v in c["vs"]])
    assert float(e.min()) < -30 and float(e.max()) > 30, "row scales spread over 2^-40 .. 2^40 within one call"
    g = torch.cat([g.reshape(-1) for g in c["gs"]])
    assert int((g == 0).sum()) >= 10 and int((g > 0).sum()) >= 20 and int((g < 0).sum()) >= 20
    ref = S.wnorm_reference(c, [True] * 9)
    for l, (v, dw, r) in enumerate(zip(c["vs"], c["dws"], ref)):
        assert all(bool(torch.isfinite(t).all()) for t in r["f64"] + r["f32"])
        v64, d64 = v.double(), dw.double()
        cos = (v64 * d64).sum(1).abs() / (v64.norm(dim=1) * d64.norm(dim=1)).clamp(min=1e-300)
        if kind == "parallel":
            assert bool((cos > 1 - 1e-6).all())
            live = r["scale"][1] > 0
            assert float((r["f64"][1].abs()[live] / r["scale"][1][live]).max()) < 1e-6, "dW parallel to v: the exact dv is ~0 at its scale"
        elif kind == "orthogonal" and v.shape[1] > 1:
            assert bool((cos < 1e-6).all())
    pooled = [torch.cat([r[key][k].reshape(-1) for r in ref]) for key in ("f32", "f64", "scale") for k in range(3)]
    for k in range(3):
        _measure(pooled[k], pooled[3 + k], pooled[6 + k])
    # no gradient for a layer: zero yardstick, zero scale
    ref = S.wnorm_reference(c, [False] + [True] * 8)
    assert all(bool((t == 0).all()) for t in (ref[0]["f64"][1], ref[0]["f64"][2], ref[0]["scale"][1], ref[0]["scale"][2]))


def test_weight_norm_zero_row_is_nan_in_torch():
    c = S.wnorm_case("one")
    c["vs"][0][2] = 0.0
    ref = S.wnorm_reference(c, [True])[0]
    for k in range(3):
        assert bool(torch.isnan(ref["f64"][k][2]).all()) and bool(torch.isnan(ref["f32"][k][2]).all())
        rest = torch.tensor([0, 1, 3, 4])
        assert bool(torch.isfinite(ref["f64"][k][rest]).all())


# ================================================================================================================== Adam
def test_adam_layouts_hold_the_lanes_they_name():
    assert set(S.ADAM_N) >= {1, 2, 3, 4, 5, 1023, 1024, 1025} and max(S.ADAM_N) > 256 * 4 * 2 and max(S.ADAM_N) % 4 == 1
    for n in S.ADAM_N:
        for kind in ("one", "mixed", "160"):
            ends, steps, lrs = S.adam_layout(n, kind)
            assert ends[-1] == n and all(a <= b for a, b in zip(ends[:-1], ends[1:])) and len(ends) == len(steps) == len(lrs) <= 160
            assert len(ends) == {"one": 1, "160": 160}.get(kind, len(ends))
    n = 1025
    ends, steps, lrs = S.adam_layout(n, "mixed")
    seg = S.adam_seg_of(ends, n)
    for lane, mix in S.ADAM_MIXES.items():
        own = seg[4 * lane:4 * lane + 4]
        runs = [int((own == s).sum()) for s in sorted(set(own))]
        assert tuple(runs) == mix, (lane, runs)
        assert len({steps[s] == 0 for s in set(own)}) == 2, "stepped and skipped elements share the lane"
        assert len({(steps[s], lrs[s]) for s in set(own) if steps[s]}) == len([s for s in set(own) if steps[s]])
    lens = np.diff([0] + ends)
    assert lens[0] == 0 and lens[-1] == 0 and any(a == 0 and b == 0 for a, b in zip(lens[:-1], lens[1:]))
    assert any(e % 4 for e in ends) and n % 4 == 1
    used = {steps[s] for s in set(seg)}
    assert used >= set(S.STEP_COUNTS) | {0}
    assert any(lrs[s] == 0.0 and steps[s] > 0 and lens[s] > 0 for s in range(len(ends))), "a stepped segment with learning rate 0"
    ss, bc = S.adam_seg_params(lrs, steps)
    t6 = steps.index(10 ** 6)
    assert bc[t6] == 1.0 and ss[t6] == float(np.float32(lrs[t6])), "at 10^6 steps both bias corrections have reached 1"
    ends160, steps160, _ = S.adam_layout(2049, "160")
    assert len(set(S.adam_seg_of(ends160, 2049))) > 90 and 0 in np.diff([0] + ends160)


def test_adam_values_and_restatement_error():
    n = 1025
    st = S.adam_state(n)
    g = S.adam_grad(st, 0)
    nz = g[g != 0].astype(np.float64)
    assert np.abs(nz).min() < 1e-16 and np.abs(nz).max() > 1e2
    assert (np.float32(nz) * np.float32(nz) >= np.finfo(np.float32).tiny).all(), "every non-zero gradient's square is a normal fp32"
    i = np.arange(n)
    assert (g[i % 7 == 0] == 0).all() and (st["m"][i % 7 == 0] == 0).all() and (st["v"][i % 7 == 0] == 0).all()
    assert (g[i % 7 == 1] == 0).all() and (st["v"][i % 7 == 1] > 0).all()
    ends, steps, lrs = S.adam_layout(n, "mixed")
    ss, bc = S.adam_seg_params(lrs, steps)
    seg = S.adam_seg_of(ends, n)
    f64 = tuple(a.astype(np.float64) for a in (st["p"], st["m"], st["v"]))
    f32 = (st["p"], st["m"], st["v"])
    for it in range(6):
        g = S.adam_grad(st, it)
        scales = S.adam_scales(f64[0], g, f64[1], f64[2], ss[seg])
        f64n, f32n = S.adam(f64[0], g, f64[1], f64[2], ss[seg], bc[seg], np.float64), S.adam(f32[0], g, f32[1], f32[2], ss[seg], bc[seg], np.float32)
        for a32, a64, s in zip(f32n, f64n, scales):
            assert np.isfinite(a64).all() and np.isfinite(a32).all()
            _measure(a32, a64, s)
        skipped = ss[seg] < 0
        assert all(np.array_equal(a[skipped], b[skipped]) for a, b in zip(f32n, f32))
        still = (~skipped) & (i % 7 == 0)
        assert np.array_equal(f32n[0][still], st["p"][still]) and np.array_equal(f64n[0][still], st["p"][still].astype(np.float64))
        f64, f32 = f64n, f32n


def test_adam_rule_is_torch_adam_in_float64():
    """the restated rule, with exact betas and unrounded step sizes, IS torch.optim.Adam(foreach=False, fused=False) in float64:
    three parameters with their own step counts, one of them without a gradient on the second step"""
    rng = np.random.RandomState(3)
    sizes, lr = (5, 7, 2), 3e-3
    ps = [torch.nn.Parameter(torch.from_numpy(rng.randn(k) * 0.1)) for k in sizes]
    opt = torch.optim.Adam(ps, lr=lr, betas=(0.9, 0.99), eps=1e-15, foreach=False, fused=False)
    ends = list(np.cumsum(sizes))
    seg = S.adam_seg_of(ends, sum(sizes))
    p = np.concatenate([q.detach().numpy() for q in ps])
    m, v, t = np.zeros_like(p), np.zeros_like(p), [0, 0, 0]
    for it in range(4):
        g = rng.randn(sum(sizes)) * 10.0 ** rng.randint(-6, 1)
        for i, q in enumerate(ps):
            none = i == 1 and it == 1
            t[i] += 0 if none else 1
            q.grad = None if none else torch.from_numpy(g[ends[i] - sizes[i]:ends[i]].copy())
        opt.step()
        used = [0 if (i == 1 and it == 1) else t[i] for i in range(3)]
        ss, bc = S.adam_seg_params([lr] * 3, used, 0.9, 0.99, round32=False)
        p, m, v = S.adam(p, g, m, v, ss[seg], bc[seg], np.float64, 0.9, 0.99, 1e-15)
        want = np.concatenate([q.detach().numpy() for q in ps])
        assert np.abs(p - want).max() <= 1e-13 * lr + 4 * np.finfo(np.float64).eps * np.abs(want).max()
        assert np.allclose(m, np.concatenate([opt.state[q]["exp_avg"].numpy() for q in ps]), rtol=1e-13, atol=0)
        assert np.allclose(v, np.concatenate([opt.state[q]["exp_avg_sq"].numpy() for q in ps]), rtol=1e-13, atol=0)
