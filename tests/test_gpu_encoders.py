"""csrc/encoders.hip, morpheus_amd.ops.freq_encode / sh_encode and morpheus_amd.encoders on the GPU, against tests/encoders_oracle.py.

Every result is computed once at the largest batch (4096 + 37 points) and judged there; the smaller batches -- 1, 63, 64, 65, 257:
a lone lane, one short of a wave, a wave, a wave and a tail, more than one workgroup -- must give the same rows bit for bit (no
result depends on its neighbours), with the eight sentinel words behind every output intact.

Frequency forward: identity columns and masked blocks exact; sine / cosine columns by f64_judge.judge_vs_f64 at scale 1 against
numpy's fp32 and float64 sine / cosine of the exactly scaled argument (factor 3, floor 4 U, slack 2).  The worst error of the
reference's own fp32 wording (cosine as the sine of arg + fp32(pi/2)) is recorded beside it.
Frequency backward: f64_judge.judge_sum with the oracle's count 2 n_keep + 6 and absolute sum.
SH forward / backward: bit for bit the numpy walk of the generated program (and of the header's summation order), and within the
program's own chain count of the float64 definition.

Figures of one run on an MI355X are in DESIGN 7f.
"""
import functools

import numpy as np
import pytest
import torch

from tests import encoders_oracle as O
from tests import f64_judge as J

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -77.25
BATCHES = (1, 63, 64, 65, 257)
B_MAX = 4096 + 37
FACTOR, FLOOR, SLACK = 3, 4 * J.U, 2
REPORT = "MORPHEUS_ENCODER_REPORT"


def _status(name, *args):
    """call a stream-taking entry point of the C ABI and hand back its status instead of raising"""
    from morpheus_amd import _lib
    _lib.load()
    return _lib._fns[name](*args, _lib.stream())


def _guarded(n, offset=0):
    """-> (the whole buffer, its n-element view `offset` floats in): 16-byte aligned at offset 0, eight sentinels behind the view"""
    buf = torch.full((offset + n + 8,), SENTINEL, device=DEV)
    return buf, buf[offset:offset + n]


def _intact(buf, n, offset=0):
    return bool((buf[:offset] == SENTINEL).all()) and bool((buf[offset + n:] == SENTINEL).all())


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


@functools.lru_cache(maxsize=None)
def _freq_x(D):
    x = np.random.default_rng(100 + D).uniform(-1.5, 1.5, (B_MAX, D)).astype(np.float32)
    x[:3] = np.array([0.0, 1.0, -1.0], dtype=np.float32)[:, None]          # exact 0 and +-1, in the one-point batch too
    x[64:67] = np.array([-1.0, 0.0, 1.0], dtype=np.float32)[:, None]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _freq_grad(D, degree):
    g = np.random.default_rng(7 * D + degree).standard_normal((B_MAX, O.freq_width(D, degree))).astype(np.float32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _sh_x():
    pts = O.sh_points()
    rest = np.random.default_rng(5).uniform(-1.0, 1.0, (B_MAX - len(pts), 3)).astype(np.float32)
    x = np.concatenate([pts, rest])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _sh_grad(degree):
    g = np.random.default_rng(40 + degree).standard_normal((B_MAX, degree * degree)).astype(np.float32)
    g.setflags(write=False)
    return g


def _freq_fwd(x, degree, n_keep, B, offset=0):
    D = x.shape[1]
    C = O.freq_width(D, degree)
    buf, out = _guarded(B * C, offset)
    assert _status("mh_freq_encode_fwd", _dev(x[:B]).data_ptr(), B, D, degree, n_keep, out.data_ptr()) == 0
    assert _intact(buf, B * C, offset), ("sentinels", D, degree, n_keep, B)
    return out.view(B, C).clone()


def _freq_bwd(x, grad, degree, n_keep, B):
    D = x.shape[1]
    buf, out = _guarded(B * D)
    assert _status("mh_freq_encode_bwd", _dev(x[:B]).data_ptr(), _dev(grad[:B]).data_ptr(), B, D, degree, n_keep, out.data_ptr()) == 0
    assert _intact(buf, B * D), ("sentinels", D, degree, n_keep, B)
    return out.view(B, D).clone()


def _sh_fwd(x, degree, B, offset=0):
    C2 = degree * degree
    buf, out = _guarded(B * C2, offset)
    assert _status("mh_sh_encode_fwd", _dev(x[:B]).data_ptr(), B, degree, out.data_ptr()) == 0
    assert _intact(buf, B * C2, offset), ("sentinels", degree, B)
    return out.view(B, C2).clone()


def _sh_bwd(x, grad, degree, B, offset=0):
    buf, out = _guarded(B * 3, offset)
    gbuf, g = _guarded(B * degree * degree, offset)
    g.copy_(_dev(grad[:B]).reshape(-1))
    assert _status("mh_sh_encode_bwd", _dev(x[:B]).data_ptr(), g.data_ptr(), B, degree, out.data_ptr()) == 0
    assert _intact(buf, B * 3, offset), ("sentinels", degree, B)
    return out.view(B, 3).clone()


# ------------------------------------------------------------------------------------------------ 5. frequency forward
@pytest.mark.parametrize("D", (1, 2, 3, 4))
def test_freq_forward(D):
    x = _freq_x(D)
    xt = _dev(x)
    worst = dict(hip=0.0, ref=0.0, formula=0.0)
    for degree in (0, 1, 4, 6, 10):
        C = O.freq_width(D, degree)
        formula = O.freq_ref_reference_formula(x, degree)
        for n_keep in sorted({0, degree // 2, degree}):
            got = _freq_fwd(x, degree, n_keep, B_MAX)
            what = f"freq fwd D={D} degree={degree} n_keep={n_keep}"
            assert torch.equal(got[:, :D], xt), what
            live = D + 2 * n_keep * D
            tail = got[:, live:]
            assert bool((tail == 0).all()) and not bool(torch.signbit(tail).any()), what + ": masked blocks are +0.0"
            assert torch.equal(got, _freq_fwd(x, degree, n_keep, B_MAX)), what + ": two runs"
            if n_keep:
                r32, r64 = O.freq_ref(x, degree, n_keep, np.float32), O.freq_ref(x, degree, n_keep, np.float64)
                f = J.figures_vs_f64(got[:, D:live], r32[:, D:live], r64[:, D:live], 1.0, what, FLOOR)
                e_formula = float(np.abs(formula[:, D:live].astype(np.float64) - r64[:, D:live]).max())
                rec = dict(what=what, worst_hip_U=f["worst_hip"] / J.U, worst_numpy_fp32_U=f["worst_ref"] / J.U,
                           worst_reference_formula_U=e_formula / J.U, n_hip=f["n_hip"], n_ref=f["n_ref"])
                print(rec)
                J.report(REPORT, rec)
                worst = dict(hip=max(worst["hip"], f["worst_hip"]), ref=max(worst["ref"], f["worst_ref"]), formula=max(worst["formula"], e_formula))
                J.assert_figures(f, what, FACTOR, FLOOR, SLACK)
            for B in BATCHES:
                assert torch.equal(_freq_fwd(x, degree, n_keep, B), got[:B]), (what, B)
    print(f"freq fwd D={D}: worst vs float64 in U: kernel {worst['hip'] / J.U:.3f}, numpy fp32 {worst['ref'] / J.U:.3f}, "
          f"the reference's formula {worst['formula'] / J.U:.3f}")


def test_freq_forward_unaligned_output_takes_the_dword_path():
    x = _freq_x(3)
    for B in (1, 65, 257):
        assert torch.equal(_freq_fwd(x, 6, 3, B, offset=1), _freq_fwd(x, 6, 3, B))
        assert torch.equal(_freq_fwd(x, 6, 6, B, offset=3), _freq_fwd(x, 6, 6, B))


# ------------------------------------------------------------------------------------------------ 6. frequency backward
@pytest.mark.parametrize("D", (1, 2, 3, 4))
def test_freq_backward(D):
    x = _freq_x(D)
    worst = 0.0
    for degree in (0, 1, 4, 6, 10):
        grad = _freq_grad(D, degree)
        for n_keep in sorted({0, degree // 2, degree}):
            what = f"freq bwd D={D} degree={degree} n_keep={n_keep}"
            got = _freq_bwd(x, grad, degree, n_keep, B_MAX)
            if n_keep == 0:
                assert torch.equal(got, _dev(grad[:, :D])), what
            ref, ab = O.freq_bwd_ref(x, grad, degree, n_keep)
            rec = J.judge_sum(got, ref, ab, O.freq_bwd_count(n_keep), what)
            worst = max(worst, rec["ratio"])
            assert torch.equal(got, _freq_bwd(x, grad, degree, n_keep, B_MAX)), what + ": two runs"
            for B in BATCHES:
                assert torch.equal(_freq_bwd(x, grad, degree, n_keep, B), got[:B]), (what, B)
    print(f"freq bwd D={D}: worst error / bound {worst:.3f}")
    J.report(REPORT, dict(what=f"freq bwd D={D}", worst_ratio=worst))


def test_freq_autograd_against_the_torch_encoder_in_double():
    """d/dx of sum(enc(x, max_level=0.5)^2): the incoming gradient 2 out carries the forward's own sincosf error (2 ulp, 4 U) on top
    of the backward's count"""
    from morpheus_amd.encoders import FreqEncoder, FreqEncoderTorch
    x_np = _freq_x(3)[:257]
    x = _dev(x_np).requires_grad_(True)
    (g,) = torch.autograd.grad(FreqEncoder(3, 6)(x, max_level=0.5).square().sum(), x)
    xd = torch.from_numpy(x_np).double().requires_grad_(True)
    ref_out = FreqEncoderTorch(3, 5, 6)(xd, max_level=0.5)
    (gd,) = torch.autograd.grad(ref_out.square().sum(), xd)
    _, ab = O.freq_bwd_ref(x_np, (2.0 * ref_out).detach().numpy().astype(np.float32), 6, 3)
    J.judge_sum(g, gd, ab, O.freq_bwd_count(3) + 2 * O.SINCOS_ULP + 1, "freq autograd")
    assert g.dtype == torch.float32 and g.shape == (257, 3)


# ------------------------------------------------------------------------------------------------ 7. SH forward
@pytest.mark.parametrize("degree", range(1, 9))
def test_sh_forward(degree):
    x = _sh_x()
    got = _sh_fwd(x, degree, B_MAX)
    walk = O.sh_walk(x, degree, np.float32)
    assert torch.equal(got, _dev(walk)), f"SH degree {degree}: not the walk of the generated program bit for bit"
    f = J.judge_vs_f64(got, walk, O.sh_def64(x, degree), O.sh_abs_walk(x, degree), f"SH fwd degree {degree}", FACTOR,
                       O.sh_chain_count(degree, "y") * J.U, SLACK)
    print(f"SH fwd degree {degree}: worst / absolute-term value in U: {f['worst_hip'] / J.U:.3f} (chain count {O.sh_chain_count(degree, 'y')})")
    assert torch.equal(got, _sh_fwd(x, degree, B_MAX))
    for B in BATCHES:
        assert torch.equal(_sh_fwd(x, degree, B), got[:B]), (degree, B)
    assert torch.equal(_sh_fwd(x, degree, 65, offset=1), got[:65])          # an output that is not 16-byte aligned


# ------------------------------------------------------------------------------------------------ 8. SH backward
@pytest.mark.parametrize("degree", range(1, 9))
def test_sh_backward(degree):
    x, grad = _sh_x(), _sh_grad(degree)
    got = _sh_bwd(x, grad, degree, B_MAX)
    assert torch.equal(got, _dev(O.sh_bwd_contract(x, grad, degree))), f"SH bwd degree {degree}: not the header's order bit for bit"
    ref, ab = O.sh_bwd_ref64(x, grad, degree)
    rec = J.judge_sum(got, ref, ab, O.sh_bwd_count(degree), f"SH bwd degree {degree}")
    print(f"SH bwd degree {degree}: worst error / bound {rec['ratio']:.3f} (count {O.sh_bwd_count(degree)})")
    assert torch.equal(got, _sh_bwd(x, grad, degree, B_MAX))
    for B in BATCHES:
        assert torch.equal(_sh_bwd(x, grad, degree, B), got[:B]), (degree, B)
    assert torch.equal(_sh_bwd(x, grad, degree, 65, offset=1), got[:65])


def test_backward_is_launched_only_for_an_input_that_needs_it():
    from morpheus_amd import ops
    from morpheus_amd.encoders import FreqEncoder, SHEncoder
    x = _dev(_sh_x()[:257])
    for enc, fwd, bwd, width in ((SHEncoder(3, 4), "mh_sh_encode_fwd", "mh_sh_encode_bwd", 16),
                                 (FreqEncoder(3, 6), "mh_freq_encode_fwd", "mh_freq_encode_bwd", 39)):
        w = torch.ones(width, device=DEV, requires_grad=True)
        try:
            ops.TIMER.reset(True)
            (enc(x) * w).sum().backward()
            assert fwd in ops.TIMER.records and bwd not in ops.TIMER.records
            xg = x.clone().requires_grad_(True)
            (enc(xg) * w).sum().backward()
            assert len(ops.TIMER.records[fwd]) == 2 and len(ops.TIMER.records[bwd]) == 1 and xg.grad.shape == (257, 3)
        finally:
            ops.TIMER.reset(False)


def test_modules_prefix_shapes_strides_size_and_autocast():
    from morpheus_amd.encoders import FreqEncoder, SHEncoder
    x = _sh_x()
    sh, fr = SHEncoder(3, 5), FreqEncoder(3, 4)
    xt = _dev(x[:10]).view(2, 5, 3)
    assert torch.equal(sh(xt), _sh_fwd(x, 5, 10).view(2, 5, 25))
    assert torch.equal(fr(xt), _freq_fwd(x[:, :3], 4, 4, 10).view(2, 5, 27))
    assert torch.equal(fr(xt, max_level=0.5), _freq_fwd(x[:, :3], 4, 2, 10).view(2, 5, 27))
    wide = _dev(np.concatenate([x[:257], x[:257]], 1))[:, ::2]          # non-contiguous: columns 0, 2, 4 of a [257, 6] buffer
    assert not wide.is_contiguous()
    dense = wide.contiguous()
    assert torch.equal(sh(wide), sh(dense)) and torch.equal(fr(wide), fr(dense))
    half = _dev((x[:257] / np.float32(2.0)).astype(np.float32))
    assert torch.equal(sh(_dev(x[:257]), size=2.0), _sh_fwd(half.cpu().numpy(), 5, 257))
    with torch.autocast("cuda", dtype=torch.float16):
        assert sh(dense).dtype == torch.float32 and fr(dense).dtype == torch.float32
        assert torch.equal(sh(dense), _sh_fwd(dense.cpu().numpy(), 5, 257))
    x16 = dense.half().requires_grad_(True)          # a half input: computed in fp32 of its values, the gradient comes back as half
    out = sh(x16)
    assert out.dtype == torch.float32 and torch.equal(out, _sh_fwd(x16.detach().float().cpu().numpy(), 5, 257))
    out.sum().backward()
    assert x16.grad.dtype == torch.float16


# ------------------------------------------------------------------------------------------------ 9. get_encoder
def test_get_encoder_on_the_device():
    from morpheus_amd.encoders import get_encoder
    from morpheus_amd.model import GridEncoder
    x = _dev(_sh_x()[:257])
    for name in ("None", "frequency_torch", "frequency", "sphere_harmonics", "hashgrid", "tiledgrid"):
        torch.manual_seed(0)
        enc, dim = get_encoder(name)
        if isinstance(enc, torch.nn.Module):
            enc = enc.to(DEV)
        out = enc(x)
        assert out.shape == (257, dim) and bool(torch.isfinite(out).all()), name
        if name == "frequency":
            assert torch.equal(out, _freq_fwd(_sh_x(), 6, 6, 257))
        if name == "sphere_harmonics":
            assert torch.equal(out, _sh_fwd(_sh_x(), 4, 257))
        if name == "hashgrid":
            twin = GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=2048,
                               gridtype="hash", align_corners=False, interpolation="linear").to(DEV)
            twin.load_state_dict(enc.state_dict())
            assert torch.equal(out, twin(x)) and bool((out != 0).any())
