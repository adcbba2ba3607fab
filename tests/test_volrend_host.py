"""morpheus_amd.volrend, everything that needs no GPU: the cases of tests/volrend_oracle.py reach what they name, the oracle's
density form is the compositor's yardstick, the public signatures are nerfacc 0.5.x's as recalled, the refusals (no n_rays, CPU
tensors, gradients to t), empty inputs, and the new entry points of the C ABI."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import step_f64_oracle as S
from tests import volrend_oracle as V
from tests.f64_judge import F32, F64, scaled_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worst(x32, x64, scale):
    e, bad = scaled_errors(x32, x64, scale)
    assert bad == 0, "the fp32 restatement is exact where the scale is 0"
    return float(e.max()) if e.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("build", [V.density_case, V.alpha_case])
def test_weight_cases_reach_what_they_name(build):
    case = build()
    cnt = case["cnt"]
    assert set(V.COUNTS) <= set(cnt) and cnt[0] == 0 and cnt[-1] == 0 and any(a == 0 and b == 0 for a, b in zip(cnt, cnt[1:]))
    assert case["N"] % 4 in (0, 1) and case["M"] == sum(cnt)
    start = V._start(cnt)
    r64, r32 = V.weights_run(case, F64), V.weights_run(case, F32)
    w32, T32 = r32["w"], r32["T"]
    if case["alpha_form"]:
        alpha = case["alpha"]
        for at in V.OPAQUE_AT:
            r, k = case["placed"][f"alpha = 1 @{at}"]
            i = int(start[r]) + k
            assert k == at and float(alpha[i]) == 1.0 and cnt[r] == at + 1 + V.BEHIND
            assert bool((w32[i + 1:i + 1 + V.BEHIND] == 0).all()) and bool((T32[i + 1:i + 1 + V.BEHIND] == 0).all())
            # the gradient to the opaque sample itself lives on the samples BEHIND it: finite, and not zero
            d = r64["grads"]["wT"][i]
            assert bool(torch.isfinite(d)) and abs(float(d) - float(case["g_w"][i]) * float(r64["T"][i])) > 1e-3
        r, ks = case["placed"]["alpha = 0"]
        assert bool((alpha[[int(start[r]) + k for k in ks]] == 0).all())
        r, (k0, k1) = case["placed"]["two opaque"]
        s = int(start[r])
        assert float(alpha[s + k0]) == 1.0 and float(alpha[s + k1]) == 1.0
        # moving a sample behind the second opaque one leaves the gradient of the first where it was
        moved = dict(case, alpha=case["alpha"].clone())
        moved["alpha"][s + k1 + 3] = 0.9
        assert float(V.weights_run(moved, F64)["grads"]["wT"][s + k0]) == float(r64["grads"]["wT"][s + k0])
        moved["alpha"][s + k1 - 3] = 0.9
        assert float(V.weights_run(moved, F64)["grads"]["wT"][s + k0]) != float(r64["grads"]["wT"][s + k0])
        r, ks = case["placed"]["near one"]
        assert all(float(1 - alpha[int(start[r]) + k].double()) == 2.0 ** -20 for k in ks)
        names = ("w", "T")
    else:
        sd = case["sigma"].double() * (case["te"] - case["ts"]).double()
        for sd_big in V.OPAQUE_SD:
            for at in V.OPAQUE_AT:
                r, k = case["placed"][f"opaque {sd_big:g} @{at}"]
                i = int(start[r]) + k
                assert k == at and abs(float(sd[i]) / sd_big - 1) < 1e-3
                behind = slice(i + 1, i + 1 + V.BEHIND)
                assert float(T32[behind].max()) < 1e-12
                if sd_big == 1e4:       # exp(-30) and exp(-1e2) are fp32 numbers; exp(-1e4) is exactly 0
                    assert bool((w32[behind] == 0).all()) and bool((T32[behind] == 0).all())
        r, ks = case["placed"]["sigma = 0"]
        assert bool((case["sigma"][[int(start[r]) + k for k in ks]] == 0).all())
        r, ks = case["placed"]["ts == te"]
        idx = [int(start[r]) + k for k in ks]
        assert bool((case["ts"][idx] == case["te"][idx]).all())
        names = ("w", "T", "a")
    # underflow: the fp32 transmittance is exactly 0 from mid-chunk on, the float64 gradients behind it are live
    r, k = case["placed"]["underflow"]
    s = int(start[r])
    first0 = int((T32[s:s + cnt[r]] == 0).nonzero()[0])
    assert 40 < first0 < 63 and abs(first0 - k) <= 3
    assert bool((r64["grads"]["wTa" if "a" in names else "wT"][s + first0:s + first0 + 5] != 0).all())
    # every judged quantity has a non-zero, finite restatement error
    for var in (V.ALPHA_VARIANTS if case["alpha_form"] else V.DENSITY_VARIANTS):
        sc = V.weights_scales(case, r64, var)
        for pool, mask in V.gradient_pools(case).items():
            e = _worst(r32["grads"][var][mask], r64["grads"][var][mask], sc["d_in"][mask])
            # behind the underflow of the alpha form fp32 holds 0 where float64 holds 1e-60: wrong by the whole (tiny) scale
            assert 0 < e < 1e-4 or ("underflow" in pool and e <= 1.0 + 1e-9), (var, pool, e)
    sc = V.weights_scales(case, r64, "w")
    for n in names:
        e = _worst(r32[n], r64[n], sc[n])
        assert 0 < e < 1e-5, (n, e)


@pytest.mark.parametrize("alpha_form", [False, True])
def test_ray_count_cases(alpha_form):
    assert [V.rays_case(N, alpha_form)["cnt"] for N in V.RAY_COUNTS] == [[65], [65, 0, 3, 129], [65, 0, 3, 129, 1]]


def test_accumulate_cases():
    assert V.ACC_CHANNELS == (None, 1, 2, 3, 4, 5, 7, 16, 48, 65, 256)
    for D in (None, 3, 65):
        case = V.accumulate_case(D)
        assert set(V.COUNTS) <= set(case["cnt"]) and case["cnt"][0] == 0 and case["cnt"][-1] == 0
        assert int((case["w"] == 0).sum()) > 10
        r64, r32, sc = V.accumulate_run(case, F64), V.accumulate_run(case, F32), V.accumulate_scales(case)
        empty = torch.tensor(case["cnt"]) == 0
        assert bool((r32["out"][empty] == 0).all()) and r64["out"].shape == (case["N"], D or 1)
        assert 0 < _worst(r32["out"], r64["out"], sc["out"]) < 1e-5
        if D == 65:
            assert 0 < _worst(r32["d_w"], r64["d_w"], sc["d_w"]) < 1e-5
            assert 0 < _worst(r32["d_v"], r64["d_v"], sc["d_v"]) < 1e-6


def test_density_form_is_the_compositors_yardstick():
    """weights of the density form and the four accumulations of the reference's composition equal tests/step_f64_oracle.composite
    on a shared case, bit for bit in float64 and in fp32"""
    case = V.density_case()
    tmid = (case["ts"] + case["te"]) * 0.5
    for dtype in (F64, F32):
        sigma, rgb = case["sigma"].to(dtype), case["rgb"].to(dtype)
        w, o, d, c = S.composite(sigma, case["ts"], case["te"], rgb, case["cnt"])
        w2, _, _ = V.weights(sigma, case["ts"], case["te"], case["cnt"], False)
        assert torch.equal(w, w2)
        assert torch.equal(o, V.accumulate(w2, None, case["cnt"])[:, 0])
        assert torch.equal(c, V.accumulate(w2, rgb, case["cnt"]))
        tm = ((case["ts"].to(dtype) + case["te"].to(dtype)) * 0.5)
        assert torch.equal(d, V.accumulate(w2, tm[:, None], case["cnt"])[:, 0])
    assert tmid.dtype == F32


# ------------------------------------------------------------------------------------------------------------ the module
SIGNATURES = {
    "pack_info": "(ray_indices, n_rays=None)",
    "render_transmittance_from_density": "(t_starts, t_ends, sigmas, packed_info=None, ray_indices=None, n_rays=None, prefix_trans=None)",
    "render_transmittance_from_alpha": "(alphas, packed_info=None, ray_indices=None, n_rays=None, prefix_trans=None)",
    "render_weight_from_density": "(t_starts, t_ends, sigmas, packed_info=None, ray_indices=None, n_rays=None, prefix_trans=None)",
    "render_weight_from_alpha": "(alphas, packed_info=None, ray_indices=None, n_rays=None, prefix_trans=None)",
    "accumulate_along_rays": "(weights, values=None, ray_indices=None, n_rays=None)",
    "render_visibility_from_density": "(t_starts, t_ends, sigmas, packed_info=None, ray_indices=None, n_rays=None, early_stop_eps=0.0001, "
                                      "alpha_thre=0.0, prefix_trans=None)",
    "render_visibility_from_alpha": "(alphas, packed_info=None, ray_indices=None, n_rays=None, early_stop_eps=0.0001, alpha_thre=0.0, "
                                    "prefix_trans=None)",
    "rendering": "(t_starts, t_ends, ray_indices=None, n_rays=None, rgb_sigma_fn=None, rgb_alpha_fn=None, render_bkgd=None)",
}


def test_public_signatures_are_nerfaccs():
    from morpheus_amd import volrend
    for name, want in SIGNATURES.items():
        sig = inspect.signature(getattr(volrend, name))
        got = "(" + ", ".join(p.name if p.default is inspect.Parameter.empty else f"{p.name}={p.default!r}" for p in sig.parameters.values()) + ")"
        assert got == want, name
        assert name in volrend.__all__
    assert "recalled" in volrend.__doc__ and "NON-DECREASING" in volrend.__doc__ and "inf / NaN" in volrend.__doc__


def test_refusals_without_a_gpu():
    from morpheus_amd import volrend
    from morpheus_amd._lib import MorpheusHipError
    M = 6
    ts, te, x = torch.rand(M), torch.rand(M) + 1, torch.rand(M)
    idx = torch.tensor([0, 0, 1, 3, 3, 3])
    # CPU tensors: no CPU path
    for call in (lambda: volrend.pack_info(idx, 4),
                 lambda: volrend.render_weight_from_density(ts, te, x, ray_indices=idx, n_rays=4),
                 lambda: volrend.render_transmittance_from_density(ts, te, x, ray_indices=idx, n_rays=4),
                 lambda: volrend.render_weight_from_alpha(x, ray_indices=idx, n_rays=4),
                 lambda: volrend.render_transmittance_from_alpha(x.view(2, 3)),
                 lambda: volrend.accumulate_along_rays(x, None, idx, 4),
                 lambda: volrend.render_visibility_from_alpha(x, ray_indices=idx, n_rays=4),
                 lambda: volrend.render_visibility_from_density(ts, te, x, ray_indices=idx, n_rays=4),
                 lambda: volrend.rendering(ts, te, idx, 4, rgb_sigma_fn=lambda a, b, i: (torch.rand(M, 3), x))):
        with pytest.raises(MorpheusHipError):
            call()


class _OnGpu(torch.Tensor):
    """a CPU tensor that says it is on the GPU: argument checks behind require_gpu can be reached without a device"""
    is_cuda = True


def _fake(t):
    return t.as_subclass(_OnGpu)


def test_argument_rules_without_a_gpu(monkeypatch):
    """ray_indices without n_rays -> ValueError; t_starts / t_ends that require a gradient -> NotImplementedError; M == 0 ->
    zeros of the right shape without a launch (a launch would raise here: there is no device)"""
    from morpheus_amd import volrend

    def no_launch(name, *args, **kw):
        raise AssertionError(f"{name} launched")
    monkeypatch.setattr(volrend, "_timed", no_launch)
    M = 6
    ts, te, x = _fake(torch.rand(M)), _fake(torch.rand(M) + 1), _fake(torch.rand(M))
    idx = _fake(torch.tensor([0, 0, 1, 3, 3, 3]))
    for call in (lambda: volrend.pack_info(idx), lambda: volrend.render_weight_from_density(ts, te, x, ray_indices=idx),
                 lambda: volrend.render_transmittance_from_density(ts, te, x, ray_indices=idx),
                 lambda: volrend.render_weight_from_alpha(x, ray_indices=idx), lambda: volrend.render_transmittance_from_alpha(x, ray_indices=idx),
                 lambda: volrend.accumulate_along_rays(x, None, idx), lambda: volrend.render_visibility_from_alpha(x, ray_indices=idx),
                 lambda: volrend.rendering(ts, te, idx, rgb_alpha_fn=lambda a, b, i: (x, x))):
        with pytest.raises(ValueError, match="n_rays"):
            call()
    for a, b in ((_fake(torch.rand(M)).requires_grad_(True), te), (ts, _fake(torch.rand(M)).requires_grad_(True))):
        with pytest.raises(NotImplementedError):
            volrend.render_weight_from_density(a, b, x, ray_indices=idx, n_rays=4)
        with pytest.raises(NotImplementedError):
            volrend.render_transmittance_from_density(a, b, x, ray_indices=idx, n_rays=4)
    # empty inputs
    e, ei = _fake(torch.zeros(0)), _fake(torch.zeros(0, dtype=torch.long))
    info = volrend.pack_info(ei, 5)
    assert info.shape == (5, 2) and info.dtype == torch.int64 and not bool(info.any())
    outs = volrend.render_weight_from_density(e, e, e, ray_indices=ei, n_rays=5)
    assert len(outs) == 3 and all(o.shape == (0,) for o in outs)
    outs = volrend.render_weight_from_alpha(e, ray_indices=ei, n_rays=5)
    assert len(outs) == 2 and all(o.shape == (0,) for o in outs)
    assert volrend.render_transmittance_from_alpha(e, ray_indices=ei, n_rays=5).shape == (0,)
    for values, D in ((None, 1), (_fake(torch.zeros(0, 3)), 3)):
        out = volrend.accumulate_along_rays(e, values, ei, 5)
        assert out.shape == (5, D) and not bool(out.any())
    dense = volrend.render_weight_from_alpha(_fake(torch.zeros(4, 0)))
    assert all(o.shape == (4, 0) for o in dense)
    out = volrend.accumulate_along_rays(_fake(torch.zeros(4, 0)), _fake(torch.zeros(4, 0, 2)))
    assert out.shape == (4, 2) and not bool(out.any())
    assert volrend.render_visibility_from_alpha(e, ray_indices=ei, n_rays=5).dtype == torch.bool
    colors, opacities, depths, extras = volrend.rendering(e, e, ei, 5, rgb_sigma_fn=lambda a, b, i: (_fake(torch.zeros(0, 3)), e),
                                                          render_bkgd=torch.ones(3))
    assert colors.shape == (5, 3) and opacities.shape == (5, 1) and depths.shape == (5, 1)
    assert bool((colors == 1).all()) and not bool(opacities.any()) and not bool(depths.any())
    assert set(extras) == {"weights", "alphas", "trans", "sigmas", "rgbs"}


# ------------------------------------------------------------------------------------------------------------ the C ABI
NEW = ("mh_pack_info", "mh_ray_weights_fwd", "mh_ray_weights_bwd", "mh_accumulate_fwd", "mh_accumulate_bwd")


def test_header_build_and_argument_checks():
    from morpheus_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "morpheus_hip.h")).read()
    assert hdr.count("#define MH_ABI_VERSION 10 ") == 1
    for name in NEW:
        assert len(re.findall(r"\b%s\s*\(" % name, hdr)) == 1 and name in _lib.EXPORTS
    assert "volrend.hip" in build.SOURCES and "volrend.hip" not in build.FILE_FLAGS           # the default flags
    assert "composite.hip" in build.SOURCES
    build.build()
    lib = _lib.load()
    assert lib.mh_abi_version() == 10
    # bad arguments: a status, no launch (there is no device here)
    assert lib.mh_pack_info(None, 0, 0, 0, None, None, None) == 0
    assert lib.mh_pack_info(None, 0, 5, 3, None, None, None) == 1
    assert lib.mh_pack_info(None, 1, 5, -1, None, None, None) == 1
    assert lib.mh_pack_info(None, 1, 1 << 31, 3, None, None, None) == 1
    assert lib.mh_ray_weights_fwd(*([None] * 3), 0, None, None, 0, None, None, None, None) == 0
    assert lib.mh_ray_weights_fwd(*([None] * 3), 0, None, None, 4, None, None, None, None) == 1
    assert lib.mh_ray_weights_fwd(*([None] * 3), 1, None, None, -1, None, None, None, None) == 1
    assert lib.mh_ray_weights_bwd(*([None] * 3), 0, None, None, 0, *([None] * 6)) == 0
    assert lib.mh_ray_weights_bwd(*([None] * 3), 1, None, None, 4, *([None] * 6)) == 1
    assert lib.mh_accumulate_fwd(None, None, 1, None, None, 0, None, None) == 0
    assert lib.mh_accumulate_fwd(None, None, 1, None, None, 4, None, None) == 1
    assert lib.mh_accumulate_fwd(None, None, 0, None, None, 0, None, None) == 1
    assert lib.mh_accumulate_fwd(None, None, 257, None, None, 0, None, None) == 1
    assert lib.mh_accumulate_fwd(None, None, 3, None, None, 0, None, None) == 1              # no values: D must be 1
    assert lib.mh_accumulate_fwd(None, None, 1, None, None, -2, None, None) == 1
    assert lib.mh_accumulate_bwd(None, None, 1, None, None, 0, None, None, None, None) == 0
    assert lib.mh_accumulate_bwd(None, None, 0, None, None, 0, None, None, None, None) == 1
    assert lib.mh_accumulate_bwd(None, None, 257, None, None, 4, None, None, None, None) == 1
    assert lib.mh_accumulate_bwd(None, None, 1, None, None, -1, None, None, None, None) == 1


def test_the_yardsticks_do_not_know_the_module():
    """the module is additive: the driver, the benchmark and the test configuration need nothing from it"""
    for rel in ("__graft_entry__.py", "bench.py", os.path.join("tests", "conftest.py")):
        assert "volrend" not in open(os.path.join(ROOT, rel)).read(), rel
    src = open(os.path.join(ROOT, "morpheus_amd", "csrc", "composite.hip")).read()
    assert "volrend" not in src and open(os.path.join(ROOT, "morpheus_amd", "render.py")).read().count("volrend") == 0
