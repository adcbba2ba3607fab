"""Host: the visibility-pruning oracle (tests/visibility_oracle.py) against closed forms, the C ABI's declarations, the argument
rules of `sampling`, and the condition the GPU mask test rests on: in float64 the share of its fixture's samples inside the
float32 error band of a threshold is under the cap on disagreements."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import visibility_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one_ray(n, step=0.01, t0=0.5):
    ts = (t0 + np.arange(n) * step).astype(np.float32)
    return ts, (ts + np.float32(step)).astype(np.float32), np.zeros(1, np.int32), np.array([n], np.int32)


@pytest.mark.parametrize("f64", [False, True])
def test_constant_sigma_ray_closed_form(f64):
    """T_i = exp(-sigma i D); the first dropped index is ceil(ln(1/eps) / (sigma D))."""
    n, sigma, eps = 300, 7.0, 1e-3
    ts, te, rs, rc = _one_ray(n)
    m = vo.mask(np.full(n, sigma, np.float32), ts, te, rs, rc, eps, f64=f64)
    Di = te.astype(np.float64) - ts.astype(np.float64)               # the float32 step: 0.01 to within an ulp of t
    D = float(np.mean(Di))
    S = sigma * (np.cumsum(Di) - Di)
    # float32: the band of visibility_oracle.band -- (cnt + 4) ulps of max(S, 1), relative to T
    rtol = 1e-12 if f64 else (n + 4) * 2.0 ** -23 * np.maximum(S, 1)
    assert np.all(np.abs(m["T"] - np.exp(-S)) <= rtol * np.exp(-S))
    assert np.allclose(m["T"], np.exp(-sigma * 0.01 * np.arange(n)), rtol=1e-3, atol=0)      # the closed form itself
    assert np.allclose(m["alpha"], -np.expm1(-sigma * D), rtol=1e-6)
    first = math.ceil(math.log(1 / eps) / (sigma * D))
    assert 0 < first < n
    assert m["keep"][:first].all() and not m["keep"][first:].any() and m["kept_cnt"][0] == first
    # eps = 0 keeps everything; an opacity threshold above the constant alpha drops everything
    assert vo.mask(np.full(n, sigma, np.float32), ts, te, rs, rc, 0.0, f64=f64)["keep"].all()
    assert not vo.mask(np.full(n, sigma, np.float32), ts, te, rs, rc, 0.0, alpha_thre=0.1, f64=f64)["keep"].any()


@pytest.mark.parametrize("f64", [False, True])
def test_constant_alpha_ray_closed_form(f64):
    """alpha form: T_i = (1 - a)^i; out-of-range opacities are clamped; an opaque sample hides everything behind it."""
    n, a, eps = 200, 0.05, 1e-2
    ts, te, rs, rc = _one_ray(n)
    m = vo.mask(np.full(n, a, np.float32), None, None, rs, rc, eps, alpha_form=True, f64=f64)
    assert np.allclose(m["T"], (1 - float(np.float32(a))) ** np.arange(n), rtol=1e-12 if f64 else 2e-5)
    first = math.ceil(math.log(eps) / math.log(1 - float(np.float32(a))))
    assert m["keep"][:first].all() and not m["keep"][first:].any()
    v = np.array([0.1, 1.7, 0.1, 0.1], np.float32)                  # 1.7 clamps to 1: T = 0 behind it
    m = vo.mask(v, None, None, rs, np.array([4], np.int32), 1e-4, alpha_form=True, f64=f64)
    assert m["keep"].tolist() == [1, 1, 0, 0] and m["alpha"][1] == 1 and m["T"][2] == 0
    assert vo.mask(v, None, None, rs, np.array([4], np.int32), 0.0, alpha_form=True, f64=f64)["keep"].all()      # T = 0 >= 0
    m = vo.mask(np.array([-0.5, 0.2], np.float32), None, None, rs, np.array([2], np.int32), 0.0, alpha_thre=0.1, alpha_form=True)
    assert m["keep"].tolist() == [0, 1] and m["T"][1] == 1                                  # -0.5 clamps to 0


def test_nan_and_negative_sigma():
    """A NaN sample is dropped and adds 0; a negative density is clamped to x = 0 (alpha = 0, T unchanged): kept at
    alpha_thre = 0, dropped above it."""
    ts, te, rs, _ = _one_ray(5)
    v = np.array([10.0, np.nan, -3.0, 10.0, 10.0], np.float32)
    rc = np.array([5], np.int32)
    m = vo.mask(v, ts, te, rs, rc, 0.0, f64=True)
    assert m["keep"].tolist() == [1, 0, 1, 1, 1]
    D = te.astype(np.float64) - ts.astype(np.float64)
    assert m["S"][3] == 10.0 * D[0] and m["alpha"][2] == 0 and m["T"][2] == m["T"][3]
    assert np.all(np.diff(m["T"]) <= 0)                                                 # T never rises
    assert vo.mask(v, ts, te, rs, rc, 0.0, alpha_thre=1e-3)["keep"].tolist() == [1, 0, 0, 1, 1]
    # a NaN in the alpha form likewise
    assert vo.mask(np.array([0.5, np.nan, 0.5], np.float32), None, None, rs, np.array([3], np.int32), 0.3,
                   alpha_form=True)["keep"].tolist() == [1, 0, 1]


def test_empty_rays_and_pack():
    """Empty rays keep their place in ray_start / ray_cnt; the compaction preserves order and names the source positions."""
    ts = np.arange(10, dtype=np.float32)
    te = ts + 1
    rs, rc = np.array([0, 0, 4, 4, 10], np.int32), np.array([0, 4, 0, 6, 0], np.int32)
    m = vo.mask(np.full(10, 0.5, np.float32), ts, te, rs, rc, 0.2)
    assert m["kept_cnt"].tolist() == [0, 4, 0, 4, 0]                 # T = exp(-0.5 i) >= 0.2 for i <= 3
    ri, pts, pte, prs, prc, src = vo.pack(m["keep"], ts, te, rs, rc)
    assert ri.tolist() == [1] * 4 + [3] * 4 and src.tolist() == [0, 1, 2, 3, 4, 5, 6, 7]
    assert prs.tolist() == [0, 0, 4, 4, 8] and prc.tolist() == [0, 4, 0, 4, 0] and np.array_equal(pts, ts[src]) and np.array_equal(pte, te[src])
    out = vo.pack(m["keep"], ts, te, rs, rc, capacity=12)
    assert out[6] == 8 and len(out[0]) == 12 and not out[0][8:].any() and not out[1][8:].any() and not out[5][8:].any()
    z = np.zeros(0, np.float32)
    m0 = vo.mask(z, z, z, np.zeros(3, np.int32), np.zeros(3, np.int32), 1e-4)
    assert m0["keep"].shape == (0,) and m0["kept_cnt"].tolist() == [0, 0, 0]


def test_alpha_thre_eff_takes_the_mean_branch():
    occs = np.zeros(1000, np.float32)
    occs[:5] = 1.0                                                    # mean 5e-3
    assert vo.alpha_thre_eff(1e-2, occs) == pytest.approx(5e-3) and vo.alpha_thre_eff(1e-3, occs) == 1e-3
    ts, te, rs, rc = _one_ray(3)
    v = np.array([0.3, 0.7, 2.0], np.float32)                         # alpha = 3e-3, 7e-3, 2e-2
    assert vo.mask(v, ts, te, rs, rc, 0.0, alpha_thre=1e-2)["keep"].tolist() == [0, 0, 1]
    assert vo.mask(v, ts, te, rs, rc, 0.0, alpha_thre=vo.alpha_thre_eff(1e-2, occs))["keep"].tolist() == [0, 1, 1]


def test_header_declares_the_entry_points_and_abi_is_still_9():
    from morpheus_amd import _lib, build
    import ctypes
    with open(build.HEADER) as f:
        text = f.read()
    abi, sigs = _lib.parse_header(text)
    assert abi == 10 and _lib._ABI == 10
    v = ctypes.c_void_p
    assert sigs["mh_visibility_mask"] == (ctypes.c_int32, [v, ctypes.c_int32, v, v, v, v, ctypes.c_int32, ctypes.c_int64,
                                                            ctypes.c_float, v, v, v, v])
    assert sigs["mh_visibility_pack"] == (ctypes.c_int32, [v, v, v, v, v, v, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64,
                                                            v, v, v, v, v])
    assert "mh_visibility_mask" in _lib.EXPORTS and "mh_visibility_pack" in _lib.EXPORTS
    assert "visibility.hip" in build.SOURCES
    # the conventions are text in the header: the recalled rule is marked as such, and the monotonicity the early exit rests on
    sect = text[text.index("visibility pruning of packed samples"):text.index("int mh_visibility_mask")]
    assert "NOT verified" in sect and "non-increasing" in sect and re.search(r"min\(alpha_thre, mean\(occs\)\)", sect)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """MH_ERR_ARG (1) for bad arguments, MH_OK (0) without a launch for N == 0 or M == 0: the status comes back on a machine
    without a GPU, where a launch could only fail."""
    from morpheus_amd import _lib
    _lib.load()
    mask, pack = _lib._fns["mh_visibility_mask"], _lib._fns["mh_visibility_pack"]
    p = 4096                                                          # any non-null address: never dereferenced on these paths
    assert mask(p, 0, p, p, p, p, 0, 10, 1e-4, None, p, p, None) == 0
    assert mask(p, 0, p, p, p, p, 10, 0, 1e-4, None, p, p, None) == 0
    assert mask(None, 0, None, None, None, None, 0, 0, 0.0, None, None, None, None) == 0
    assert mask(p, 0, p, p, p, p, -1, 10, 1e-4, None, p, p, None) == 1
    assert mask(p, 0, p, p, p, p, 4, -1, 1e-4, None, p, p, None) == 1
    assert mask(p, 0, p, p, p, p, 4, 1 << 31, 1e-4, None, p, p, None) == 1
    assert mask(p, 0, p, p, p, p, 4, 10, -0.5, None, p, p, None) == 1
    assert mask(p, 0, p, p, p, p, 4, 10, float("nan"), None, p, p, None) == 1
    assert mask(p, 2, p, p, p, p, 4, 10, 0.0, None, p, p, None) == 1
    assert mask(None, 0, p, p, p, p, 4, 10, 0.0, None, p, p, None) == 1
    assert mask(p, 0, None, p, p, p, 4, 10, 0.0, None, p, p, None) == 1        # the sigma form reads t_starts / t_ends
    assert mask(p, 0, p, p, p, p, 4, 10, 0.0, None, None, p, None) == 1
    assert pack(p, p, p, p, p, p, 0, 10, 10, p, p, p, p, None) == 0
    assert pack(p, p, p, p, p, p, 4, 10, 0, p, p, p, p, None) == 0
    assert pack(p, p, p, p, p, p, 4, 10, 11, p, p, p, p, None) == 1            # the kept set is a subset
    assert pack(p, p, p, p, p, p, -1, 10, 10, p, p, p, p, None) == 1
    assert pack(None, p, p, p, p, p, 4, 10, 10, p, p, p, p, None) == 1
    assert pack(p, p, p, p, p, None, 4, 10, 10, p, p, p, p, None) == 1
    assert pack(p, p, p, p, p, p, 4, 10, 10, p, p, p, None, None) == 1


def test_sampling_argument_rules():
    """Thresholds without a density function: ValueError naming what is missing (nerfacc ignores them silently); cone marching
    still NotImplementedError; `alpha_fn` exists on both samplers; the defaults are the reference's call."""
    import inspect
    from morpheus_amd.occgrid import OccupancyGrid
    from morpheus_amd.render import HotPathRenderer, UniformSampler
    o, d = torch.zeros(2, 3), torch.ones(2, 3)
    for smp in (OccupancyGrid([-1.01] * 3 + [1.01] * 3, 16), UniformSampler(8, 1.01)):
        for kw in (dict(alpha_thre=1e-2), dict(early_stop_eps=1e-4), dict(alpha_thre=1e-2, early_stop_eps=1e-4)):
            with pytest.raises(ValueError, match="density function is required"):
                smp.sampling(o, d, **kw)
        with pytest.raises(NotImplementedError):
            smp.sampling(o, d, cone_angle=0.004)
        with pytest.raises(NotImplementedError):
            smp.sampling(o, d, sigma_fn=lambda *a: None, cone_angle=0.004, early_stop_eps=1e-4)
        with pytest.raises(ValueError, match="not both"):
            smp.sampling(o, d, sigma_fn=lambda *a: None, alpha_fn=lambda *a: None)
        sig = inspect.signature(smp.sampling).parameters
        assert sig["alpha_fn"].default is None and sig["sigma_fn"].default is None
        assert sig["early_stop_eps"].default == 0 and sig["alpha_thre"].default == 0 and sig["cone_angle"].default == 0.0
    assert "1e-4" in OccupancyGrid.sampling.__doc__                    # nerfacc's own default is named
    assert HotPathRenderer(None, {}, None, 1).prune is None            # pruning is opt-in


@pytest.mark.parametrize("alpha_form", [False, True])
def test_gpu_fixture_stays_under_its_band_cap(alpha_form):
    """The condition of tests/test_gpu_visibility.py::test_mask_against_float64_oracle: computed in float64 on the CPU, fewer
    than 0.1 % of the fixture's samples lie inside the float32 error band of a threshold, for every case of the GPU test --
    so the cap on disagreements there is never reached by honest rounding, and the fixture exercises both thresholds."""
    fx = vo.fixture(alpha_form=alpha_form)
    M = fx["values"].shape[0]
    assert fx["ray_cnt"].max() == 350 and fx["ray_cnt"].min() == 0 and M > 300000
    assert {64, 128, 320, 65, 129} <= set(fx["ray_cnt"][:8].tolist())
    for eps in vo.EPS_CASES:
        for thre in vo.THRE_CASES:
            m = vo.mask(fx["values"], fx["t_starts"], fx["t_ends"], fx["ray_start"], fx["ray_cnt"], eps, thre, alpha_form, f64=True)
            share = float(vo.band(m, eps, thre).sum()) / M
            assert share < vo.BAND_CAP, (eps, thre, share)
            s8, s9 = fx["ray_start"][fx["all_dropped"]], fx["ray_start"][fx["all_kept"]]
            assert not m["keep"][s8:s8 + 100].any() and m["keep"][s9:s9 + 100].all()
            kept = float(m["keep"].sum()) / M
            if eps > 0 or thre > 0:
                assert 0.05 < kept < 0.95, (eps, thre, kept)           # the thresholds bite, and do not bite everything
            else:
                assert kept > 0.99                                       # only the NaN samples leave
