"""The pair form of the fused field backward (two waves per SIMD: csrc/mlp.hip field_pair_color_kernel / field_pair_sdf_kernel)
against the one-wave kernels it replaces for the with-colour pass of the b3 mode: every output bit for bit, through
ops._field_bwd, at the sizes where the pair structure can go wrong."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUTPUTS = ("g_xc", "g_fs", "g_fc", "g_tp", "raw", "gmax")
_cache = {}


def _cus():
    """the library's mh_cu_count(): the device's multiprocessor count"""
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def _setup(M, n_bands):
    """one forward per (M, n_bands), shared by the cases: operands, parked activations, upstream gradients"""
    from morpheus_amd import _lib, ops
    key = (M, n_bands)
    if key not in _cache:
        lib = _lib.load()
        g = torch.Generator().manual_seed(77 + M)
        rn = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(DEV)
        Ws = [rn(64, 73, k=0.2), rn(64, 64, k=0.2), rn(33, 64, k=0.2)]
        Wc = [rn(64, 64, k=0.2), rn(64, 64, k=0.2), rn(3, 64, k=0.2)]
        bs = [rn(64, k=0.1), rn(64, k=0.1), rn(33, k=0.1)]
        bc = [rn(64, k=0.1), rn(64, k=0.1), rn(3, k=0.1)]
        fop = ops.prepare_field_operands([p.requires_grad_() for p in Ws + Wc + bs + bc], mode="b3")
        x = (torch.rand(M, 3, generator=g) * 2 - 1).to(DEV).contiguous()
        fs, fc, tp = rn(M, 32, k=0.1), rn(M, 32, k=0.1), rn(M, 2, k=0.1)
        beta = torch.tensor([0.1], device=DEV)
        sdf, sigma, albedo, acts = ops._field_fwd(lib, x, fs, fc, tp, beta, n_bands, True, fop, True)
        ups = (rn(M), rn(M, k=0.01), rn(M, 3))
        _cache[key] = (lib, fop, x, beta, sdf, albedo, acts, ups)
    return _cache[key]


def _backward(monkeypatch, form, M, n_bands, need_dx=True, has_topo=True, raw_into=None):
    from morpheus_amd import ops
    lib, fop, x, beta, sdf, albedo, acts, (g_sdf, g_sig, g_alb) = _setup(M, n_bands)
    monkeypatch.setattr(ops, "FIELD_BWD", form)
    wT, b3 = ops._field_wT(fop, True)
    assert b3
    out = ops._field_bwd(lib, x, wT, beta, acts, sdf, albedo, g_sdf, g_sig, g_alb, n_bands, True, has_topo, True, need_dx, fop.jp,
                         raw_into=raw_into, b3=b3)
    torch.cuda.synchronize()
    return {n: (None if v is None else v.clone()) for n, v in zip(OUTPUTS, out)}


def _assert_same(one, pair, what):
    for n in OUTPUTS:
        a, b = one[n], pair[n]
        assert (a is None) == (b is None), (what, n)
        if a is not None:
            assert not torch.isnan(a.float()).any(), (what, n)
            assert torch.equal(a, b), (what, n, float((a.double() - b.double()).abs().max()))


def _sizes():
    cus = _cus() if torch.cuda.is_available() else 256
    return cus, (32 * (4 * cus + 1) + 1, 32 * (8 * cus) + 33)


@pytest.mark.parametrize("M", [1, 31, 32, 33, 129, 161])
def test_pair_form_is_the_one_wave_form_bit_for_bit_small(M, monkeypatch):
    """tile edge (1, 31, 32, 33 points: one workgroup, pairs 1 .. 3 on dead tiles) and two workgroups (129, 161 points: 5 and 6 live
    tiles of 8), with d/dx, topo and all six bands"""
    one = _backward(monkeypatch, "b3w1", M, 6)
    pair = _backward(monkeypatch, "b3", M, 6)
    assert one["g_xc"] is not None and one["g_tp"] is not None and one["g_fc"] is not None
    _assert_same(one, pair, M)


@pytest.mark.parametrize("which", [0, 1])
def test_pair_form_is_the_one_wave_form_bit_for_bit_more_trips_than_workgroups(which, monkeypatch):
    """M = 32 (4 CUs + 1) + 1: the first workgroup makes a second trip while the others have none left; M = 32 (8 CUs) + 33: two
    full trips and a third for the first workgroups"""
    cus, sizes = _sizes()
    M = sizes[which]
    one = _backward(monkeypatch, "b3w1", M, 6)
    pair = _backward(monkeypatch, "b3", M, 6)
    _assert_same(one, pair, M)


@pytest.mark.parametrize("n_bands,need_dx,has_topo", [(4, True, True), (6, False, True), (6, True, False), (4, False, False)])
def test_pair_form_switches(n_bands, need_dx, has_topo, monkeypatch):
    """progressive encoding level, without g_xc (NULL skips the d/dx stage), without topo; 161 points = two workgroups"""
    one = _backward(monkeypatch, "b3w1", 161, n_bands, need_dx, has_topo)
    pair = _backward(monkeypatch, "b3", 161, n_bands, need_dx, has_topo)
    assert (one["g_xc"] is None) == (not need_dx) and (one["g_tp"] is None) == (not has_topo)
    _assert_same(one, pair, (n_bands, need_dx, has_topo))


def test_pair_form_accumulates_into_a_running_sum(monkeypatch):
    """two calls (161 and 33 points) adding into one running raw sum: bit for bit the one-wave kernels' running sum, and the sum of
    the two calls' own gradients to the existing gate (2e-5 of the tensor's maximum: the running sum adds in another order)"""
    from morpheus_amd import ops
    sums = {}
    for form in ("b3w1", "b3"):
        raw_len = _setup(161, 6)[1].jp.raw_len
        run = torch.zeros(raw_len + 1, device=DEV)
        for M in (161, 33):
            out = _backward(monkeypatch, form, M, 6, raw_into=run.data_ptr())
            assert out["raw"] is None
        torch.cuda.synchronize()
        sums[form] = run.clone()
    assert torch.equal(sums["b3w1"], sums["b3"])
    apart = _backward(monkeypatch, "b3", 161, 6)["raw"].double() + _backward(monkeypatch, "b3", 33, 6)["raw"].double()
    assert float((sums["b3"].double() - apart).abs().max()) <= 2e-5 * float(apart.abs().max())


def test_the_selector_reaches_the_library(monkeypatch):
    """ops.FIELD_BWD = "b3w1" moves the library's threshold out of reach for the call, "b3" puts the default back"""
    from morpheus_amd import ops
    lib = _setup(33, 6)[0]
    _backward(monkeypatch, "b3w1", 33, 6)
    assert lib.mh_field_bwd_pair_min_points(-1) == ops._PAIR_NEVER
    _backward(monkeypatch, "b3", 33, 6)
    assert lib.mh_field_bwd_pair_min_points(-1) == ops._pair_min_default == 0
