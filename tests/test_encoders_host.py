"""Frequency / spherical-harmonics encoders, everything that needs no GPU: argument checks of the four entry points, the generated
table against its generator and against the definition, and the modules' surface (morpheus_amd/encoders.py)."""
import os

import numpy as np
import pytest
import torch

from tests import encoders_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG = 0, 1
P = 4096          # a non-null address that is never dereferenced: every case below returns before any device call


def _fns():
    from morpheus_amd import _lib
    lib = _lib.load()
    return lib, _lib._fns


# ------------------------------------------------------------------------------------------------ 1. entry points
def test_library_version_build_list_and_flags():
    from morpheus_amd import _lib, build
    lib, fns = _fns()
    assert lib.mh_abi_version() == 10 and _lib._ABI == 10
    assert "encoders.hip" in build.SOURCES
    assert build.FILE_FLAGS["encoders.hip"] == ["-ffp-contract=off"]
    for name in ("mh_freq_encode_fwd", "mh_freq_encode_bwd", "mh_sh_encode_fwd", "mh_sh_encode_bwd"):
        assert name in _lib.EXPORTS and name in fns


def test_header_lists_the_replaced_interfaces_and_says_what_is_not_reproduced():
    from morpheus_amd import build
    text = open(build.HEADER).read()
    head = text[:text.index("#ifndef MORPHEUS_HIP_H")]
    assert "mh_freq_encode_fwd / _bwd" in head and "mh_sh_encode_fwd / _bwd" in head
    assert "__sinf(arg + pi/2)" in text and "Neither is reproduced" in text


def test_freq_entry_points_refuse_bad_arguments_without_a_device():
    _, f = _fns()
    fwd, bwd = f["mh_freq_encode_fwd"], f["mh_freq_encode_bwd"]
    # B == 0: MH_OK without a launch, whatever the pointers
    assert fwd(None, 0, 3, 6, 6, None, None) == OK
    assert bwd(None, None, 0, 3, 6, 6, None, None) == OK
    # null pointers with B > 0
    assert fwd(None, 5, 3, 6, 6, P, None) == ERR_ARG
    assert fwd(P, 5, 3, 6, 6, None, None) == ERR_ARG
    assert bwd(None, P, 5, 3, 6, 6, P, None) == ERR_ARG
    assert bwd(P, None, 5, 3, 6, 6, P, None) == ERR_ARG
    assert bwd(P, P, 5, 3, 6, 6, None, None) == ERR_ARG
    # ranges: 1 <= D <= 8, 0 <= degree <= 16, 0 <= n_keep <= degree, B >= 0 -- also with B == 0
    for B in (0, 5):
        for D, degree, n_keep in ((0, 6, 6), (9, 6, 6), (-1, 6, 6), (3, -1, 0), (3, 17, 0), (3, 6, -1), (3, 6, 7), (3, 0, 1)):
            assert fwd(P, B, D, degree, n_keep, P, None) == ERR_ARG, (B, D, degree, n_keep)
            assert bwd(P, P, B, D, degree, n_keep, P, None) == ERR_ARG, (B, D, degree, n_keep)
    assert fwd(P, -1, 3, 6, 6, P, None) == ERR_ARG
    assert bwd(P, P, -1, 3, 6, 6, P, None) == ERR_ARG
    assert fwd(P, 2 ** 62, 3, 6, 6, P, None) == ERR_ARG          # B C does not fit the index type


def test_sh_entry_points_refuse_bad_arguments_without_a_device():
    _, f = _fns()
    fwd, bwd = f["mh_sh_encode_fwd"], f["mh_sh_encode_bwd"]
    for degree in range(1, 9):
        assert fwd(None, 0, degree, None, None) == OK
        assert bwd(None, None, 0, degree, None, None) == OK
    assert fwd(None, 5, 4, P, None) == ERR_ARG
    assert fwd(P, 5, 4, None, None) == ERR_ARG
    assert bwd(None, P, 5, 4, P, None) == ERR_ARG
    assert bwd(P, None, 5, 4, P, None) == ERR_ARG
    assert bwd(P, P, 5, 4, None, None) == ERR_ARG
    for B in (0, 5):
        for degree in (0, 9, -1):
            assert fwd(P, B, degree, P, None) == ERR_ARG
            assert bwd(P, P, B, degree, P, None) == ERR_ARG
    assert fwd(P, -1, 4, P, None) == ERR_ARG
    assert bwd(P, P, -1, 4, P, None) == ERR_ARG
    assert fwd(P, 2 ** 40, 4, P, None) == ERR_ARG                 # more 64-point tiles than a grid has workgroups


# ------------------------------------------------------------------------------------------------ 2. the generated table
def test_committed_table_is_what_the_generator_writes(tmp_path):
    mod = O.table_module()
    committed = open(os.path.join(ROOT, "morpheus_amd", "csrc", "sh_table.inc"), "rb").read()
    out = tmp_path / "sh_table.inc"
    out.write_text(mod.text())
    assert out.read_bytes() == committed
    assert mod.verify() == 256          # 64 columns and their 192 partial derivatives, symbolically, exact coefficients


def test_program_is_data_in_one_order():
    common, fwd, bwd = O.program()
    seen = {"x", "y", "z"}
    for tgt, op, args in common + fwd + bwd:
        assert op in ("set", "neg", "mul", "add", "sub") and tgt not in seen
        assert all(a in seen if isinstance(a, str) else isinstance(a, float) for a in args), (tgt, args)
        seen.add(tgt)
    assert [t for t, _, _ in fwd] == [f"y{c}" for c in range(64)]
    dx, dy, dz = O.sh_present(8)
    m = np.array([c - (l * l + l) for l in range(8) for c in range(l * l, (l + 1) ** 2)])
    l = np.array([l for l in range(8) for _ in range(2 * l + 1)])
    assert np.array_equal(dx, (m != 0) & (m != -1)) and np.array_equal(dy, (m != 0) & (m != 1)) and np.array_equal(dz, np.abs(m) != l)


# ------------------------------------------------------------------------------------------------ 3. table against definition
@pytest.fixture(scope="module")
def points():
    return O.sh_points()


def test_definition_stays_within_the_float64_bound(points):
    """the 1e-13 of the next test is a float64 rounding bound for 64 polynomials of degree <= 7 on [-1, 1]^3: the definition alone
    must stay within it -- its Legendre-series evaluation against the same polynomials as power series"""
    from numpy.polynomial import legendre as L
    z = points[:, 2].astype(np.float64)
    worst = 0.0
    for l in range(8):
        for a in range(l + 1):
            s = L.Legendre.basis(l).deriv(a) if a else L.Legendre.basis(l)
            worst = max(worst, float(np.abs(s(z) - s.convert(kind=np.polynomial.Polynomial)(z)).max() / max(1.0, np.abs(s(z)).max())))
    assert worst < 1e-13, worst


@pytest.mark.parametrize("degree", range(1, 9))
def test_walk_in_float64_is_the_definition(points, degree):
    got, want = O.sh_walk(points, degree, np.float64), O.sh_def64(points, degree)
    assert got.shape == want.shape == (1050, degree * degree)
    assert float(np.abs(got - want).max()) <= 1e-13


def test_definition_is_scipys_harmonics_in_the_reference_real_basis(points):
    """on unit vectors: column(l, m > 0) = sqrt(2) Re Y_l^m, column(l, m < 0) = sqrt(2) Im Y_l^|m|, column(l, 0) = Y_l^0 -- the
    reference's signs: no further (-1)^m in front, unlike the usual real basis"""
    from scipy.special import sph_harm_y
    u = points[:512].astype(np.float64)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    u32 = u.astype(np.float32)
    got = O.sh_def64(u32, 8)
    u = u32.astype(np.float64)
    r = np.linalg.norm(u, axis=1)
    theta, phi = np.arccos(np.clip(u[:, 2] / r, -1, 1)), np.arctan2(u[:, 1], u[:, 0])
    for l in range(8):
        for m in range(-l, l + 1):
            y = sph_harm_y(l, abs(m), theta, phi)
            want = y.real if m == 0 else np.sqrt(2.0) * (y.real if m > 0 else y.imag)
            # fp32 unit vectors are off the sphere by ~6e-8: the polynomial has z^2 substituted, scipy has sin(theta)^m -- they
            # agree on the sphere only, so the comparison is to the size of that offset times the polynomial's slope (< 100)
            assert float(np.abs(got[:, l * l + l + m] - want).max()) < 1e-5, (l, m)


@pytest.mark.parametrize("degree", range(1, 9))
def test_gradient_walk_is_the_central_difference_of_the_definition(points, degree):
    h = 2.0 ** -20
    p = points.astype(np.float64)
    grads = O.sh_grad_walk(points, degree, np.float64)
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        fd = (O.sh_def64_at(p + e, degree) - O.sh_def64_at(p - e, degree)) / (2 * h)
        assert float(np.abs(grads[a] - fd).max()) <= 1e-7, (degree, a)


def test_chain_counts_are_the_derived_ones():
    assert [O.sh_chain_count(d, "y") for d in range(1, 9)] == [1, 2, 3, 5, 7, 9, 11, 13]
    assert O.sh_chain_count(8, "d") == 11 and O.sh_bwd_count(8) == 64 + 1 + 11
    assert O.freq_bwd_count(6) == 18


def test_fp32_walk_is_within_its_chain_count_of_the_definition(points):
    for degree in (4, 8):
        w, r, a = O.sh_walk(points, degree, np.float32), O.sh_def64(points, degree), O.sh_abs_walk(points, degree)
        live = a > 0
        assert np.all(w[~live] == r[~live])
        assert float((np.abs(w - r)[live] / a[live]).max()) <= O.sh_chain_count(degree, "y") * O.U


# ------------------------------------------------------------------------------------------------ 4. module surface
def test_output_dims_and_repr():
    from morpheus_amd.encoders import FreqEncoder, SHEncoder
    for D in (1, 2, 3, 4):
        for degree in (0, 4, 6, 10):
            enc = FreqEncoder(D, degree)
            assert enc.output_dim == D + 2 * D * degree == O.freq_width(D, degree)
    assert repr(FreqEncoder(3, 6)) == "FreqEncoder: input_dim=3 degree=6 output_dim=39"
    assert [SHEncoder(3, d).output_dim for d in range(1, 9)] == [d * d for d in range(1, 9)]
    assert repr(SHEncoder(3, 4)) == "SHEncoder: input_dim=3 degree=4"


def test_sh_constructor_assertions():
    from morpheus_amd.encoders import SHEncoder
    with pytest.raises(AssertionError, match="SH encoder only support input dim == 3"):
        SHEncoder(input_dim=2)
    for degree in (0, 9):
        with pytest.raises(AssertionError, match=r"SH encoder only supports degree in \[1, 8\]"):
            SHEncoder(degree=degree)


def test_hip_encoders_refuse_cpu_tensors():
    from morpheus_amd._lib import MorpheusHipError
    from morpheus_amd.encoders import FreqEncoder, SHEncoder
    with pytest.raises(MorpheusHipError):
        FreqEncoder(3, 4)(torch.zeros(2, 5, 3))
    with pytest.raises(MorpheusHipError):
        SHEncoder(3, 4)(torch.zeros(2, 5, 3))


@pytest.mark.parametrize("D", (1, 2, 3, 4))
def test_freq_encoder_torch_is_the_reference_semantics(D):
    """FreqEncoder_torch's max_level (encodings.py:35-57), which is model._freq_encode_torch's: int(max_level N) bands, a
    zero-filled tail, the same width; and the oracle's layout"""
    from morpheus_amd.encoders import FreqEncoderTorch
    from morpheus_amd.model import _freq_encode_torch
    x = torch.from_numpy(np.random.default_rng(D).uniform(-1.5, 1.5, (2, 5, D)).astype(np.float32))
    enc = FreqEncoderTorch(input_dim=D, max_freq_log2=5, N_freqs=6, log_sampling=True)
    assert enc.output_dim == D + 12 * D and enc.freq_bands == [1.0, 2.0, 4.0, 8.0, 16.0, 32.0]
    for max_level, keep in ((None, 6), (0.5, 3), (0.75, 4), (0, 0)):
        got = enc(x, max_level=max_level)
        assert got.shape == (2, 5, enc.output_dim)
        assert torch.equal(got, _freq_encode_torch(x, 6, max_level))
        assert torch.equal(got[..., D + 2 * keep * D:], torch.zeros(2, 5, (6 - keep) * 2 * D))
        want = O.freq_ref(x.reshape(-1, D).numpy(), 6, keep, np.float64)
        assert float(np.abs(got.reshape(-1, enc.output_dim).numpy() - want).max()) < 1e-6
    lin = FreqEncoderTorch(input_dim=D, max_freq_log2=2, N_freqs=3, log_sampling=False, include_input=False)
    assert lin.freq_bands == [1.0, 2.5, 4.0] and lin.output_dim == 6 * D and lin(x).shape == (2, 5, 6 * D)


def test_get_encoder_table():
    from morpheus_amd.encoders import FreqEncoder, FreqEncoderTorch, SHEncoder, get_encoder
    from morpheus_amd.model import GridEncoder
    ident, dim = get_encoder("None", input_dim=5)
    x = torch.zeros(2, 5)
    assert dim == 5 and ident(x) is x and ident(x, max_level=0.5) is x
    enc, dim = get_encoder("frequency_torch", input_dim=2, multires=4)
    assert isinstance(enc, FreqEncoderTorch) and dim == enc.output_dim == 2 + 16 and enc.freq_bands == [1.0, 2.0, 4.0, 8.0]
    enc, dim = get_encoder("frequency")
    assert isinstance(enc, FreqEncoder) and (enc.input_dim, enc.degree, dim) == (3, 6, 39)
    enc, dim = get_encoder("frequency", input_dim=1, multires=10)
    assert (enc.input_dim, enc.degree, dim) == (1, 10, 21)
    enc, dim = get_encoder("sphere_harmonics")          # the reference's factory fails here, on a module name that does not exist
    assert isinstance(enc, SHEncoder) and (enc.degree, dim) == (4, 16)
    assert get_encoder("sphere_harmonics", degree=8)[1] == 64
    for name, gridtype in (("hashgrid", "hash"), ("tiledgrid", "tiled")):
        enc, dim = get_encoder(name, num_levels=4, log2_hashmap_size=10, desired_resolution=64, align_corners=True, interpolation="smoothstep")
        assert isinstance(enc, GridEncoder) and dim == 8
        assert (enc.gridtype, enc.align_corners, enc.interpolation, enc.num_levels, enc.level_dim, enc.base_resolution,
                enc.log2_hashmap_size) == (gridtype, True, "smoothstep", 4, 2, 16, 10)
        assert enc.per_level_scale == pytest.approx(np.exp2(np.log2(64 / 16) / 3))
    # the factory's own defaults, not GridEncoder's (2^15 rows, 128): 16 levels of 2 channels up to 2048 on 2^19 rows
    enc, dim = get_encoder("hashgrid")
    assert dim == 32 and enc.log2_hashmap_size == 19 and enc.per_level_scale == pytest.approx(np.exp2(np.log2(2048 / 16) / 15))
    assert int(enc._res_np[-1]) == 2048 and enc.embeddings.shape[0] == int(enc.offsets[-1]) and int(enc.offsets[-1] - enc.offsets[-2]) == 2 ** 19
    with pytest.raises(NotImplementedError, match=r"Unknown encoding mode, choose from \[None, frequency, sphere_harmonics, hashgrid, tiledgrid\]"):
        get_encoder("triplane")


def test_freq_encoder_max_level_follows_the_torch_encoder():
    """n_keep = degree for None, int(max_level degree) otherwise -- observed through the argument the op receives"""
    from morpheus_amd import encoders, ops
    seen = []
    orig = ops.freq_encode
    try:
        ops.freq_encode = lambda x, degree, n_keep=None: seen.append((tuple(x.shape), degree, n_keep)) or x.new_zeros(x.shape[0], 3 + 6 * degree)
        enc = encoders.FreqEncoder(3, 6)
        for ml in (None, 0.5, 0.75, 0, 1.0):
            assert enc(torch.zeros(2, 5, 3), max_level=ml).shape == (2, 5, 39)
    finally:
        ops.freq_encode = orig
    assert seen == [((10, 3), 6, k) for k in (6, 3, 4, 0, 6)]
