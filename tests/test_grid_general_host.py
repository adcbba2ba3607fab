"""The grid encoder in full, on the CPU: the yardsticks of tests/test_gpu_grid_general.py are themselves pinned here, and the
Python surface that needs no GPU.

The reference operator is CUDA-only and cannot run here, so no golden comes from it; tests/grid_general_oracle.py restates the
cited lines of gridencoder.cu, and what ties that restatement down is (1) bit-equality with the pinned C restatement
oracle/hashgrid.c on the one configuration that has, (2) properties that follow from the definition on every switch combination.
"""
import itertools
import os

import numpy as np
import pytest
import torch

from morpheus_amd import _lib, ops, synth
from morpheus_amd.model import GridEncoder
from oracle.hashgrid import OracleGridEncoder
from tests import grid_general_oracle as gg

F32, F64 = np.float32, np.float64
# (gridtype, align_corners, interp) by the ids the C ABI takes
COMBOS = list(itertools.product(ops.GRID_TYPES.values(), (0, 1), ops.GRID_INTERPS.values()))
SMALL = dict(num_levels=6, base_resolution=4, desired_resolution=32, log2_hashmap_size=9)


def small_table(C, seed=11, scale=0.1):
    enc = GridEncoder(level_dim=C, **SMALL)
    emb = synth.hash_tensor((int(enc._offsets_np[-1]), C), seed, scale).numpy()
    return emb, enc._offsets_np, enc._res_np


def test_restatement_equals_the_pinned_oracle_bit_for_bit():
    """default switches, L = 16, C = 2, the 16..128 pyramid, 257 points of which some lie outside the box: forward, d/dx and table
    gradient of the fp32 restatement are the bits of oracle/hashgrid.c.  (Its table gradient has one fixed order -- levels in parallel,
    points ascending inside -- so that quantity is bit-exact too.)  bound = 1: the chain factor 1 / (2 bound) is exact either way."""
    torch.manual_seed(0)
    ora = OracleGridEncoder(log2_hashmap_size=15, desired_resolution=128)
    offs, s = synth.grid_offsets()
    assert np.array_equal(ora.offsets.numpy(), offs)
    emb = synth.hash_tensor((int(offs[-1]), 2), 9001, 0.1)
    with torch.no_grad():
        ora.embeddings.copy_(emb)
    x = synth.hash_tensor((257, 3), 77, 1.04)
    x[5] = torch.tensor([1.0, -1.0, 0.25])                  # u = 1, 0 exactly: inside
    x[9] = torch.tensor([1.5, 0.0, 0.0])
    grad = synth.hash_tensor((257, 32), 78, 1.0)
    n_out = int(((x.abs() > 1).any(1)).sum())
    assert 3 <= n_out < 200, n_out
    for max_level in (None, 0.5):
        xr = x.clone().requires_grad_(True)
        ora.embeddings.grad = None
        out = ora(xr, bound=1, max_level=max_level)
        out.backward(grad)
        case = gg.Case(x.numpy(), emb.numpy(), offs, ops.level_resolutions(16, s, 16), 1.0, ops.effective_levels(max_level, 16), 2)
        assert np.array_equal(case.forward(), out.detach().numpy())
        assert np.array_equal(case.grad_x(grad.numpy()), xr.grad.numpy())
        assert np.array_equal(case.grad_emb(grad.numpy()), ora.embeddings.grad.numpy())


def test_fma32_is_the_single_rounding():
    """against exact rational arithmetic on operands built to land next to ties"""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.standard_normal(4000).astype(F32)
    b = rng.standard_normal(4000).astype(F32)
    c = (-(a.astype(F64) * b.astype(F64))).astype(F32) * F32(1 + 2.0 ** -12)          # heavy cancellation
    c[::2] = (rng.standard_normal(2000) * 2.0 ** 20).astype(F32)                    # and wide exponent gaps
    got = gg.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], F32(-np.inf)), np.nextafter(got[i], F32(np.inf))
        e = abs(Fraction(float(got[i])) - exact)
        assert e <= abs(Fraction(float(lo)) - exact) and e <= abs(Fraction(float(hi)) - exact), i


def index_literal(gridtype, T, res, p):
    """get_grid_index (gridencoder.cu:61-79) transcribed statement by statement, uint32 arithmetic"""
    stride, index = 1, 0
    for d in range(3):
        if not stride <= T:
            break
        index = (index + p[d] * stride) & gg.M32
        stride = (stride * res) & gg.M32
    if gridtype == 0 and stride > T:
        index = ((p[0] * 1) & gg.M32) ^ ((p[1] * gg.P1) & gg.M32) ^ ((p[2] * gg.P2) & gg.M32)
    return index % T


@pytest.mark.parametrize("gridtype", (0, 1))
def test_index_follows_the_stride_loop(gridtype):
    """dense, half-covered (res <= T < res^2 and res^2 <= T < res^3) and hashed levels, coordinates up to res (total variation's
    right neighbour); a tiled level whose res^3 > rows wraps by % and never hashes"""
    rng = np.random.default_rng(5)
    for res, T in ((4, 64), (7, 344), (10, 512), (32, 512), (32, 24), (128, 32768), (1700, 2 ** 22)):
        lv = gg.Level([0, T], [res], 0, gridtype)
        p = rng.integers(0, res + 1, size=(200, 3))
        want = np.array([index_literal(gridtype, T, res, [int(v) for v in q]) for q in p])
        assert np.array_equal(lv.rows(p[:, 0], p[:, 1], p[:, 2]), want), (res, T)
        if gridtype == 1:
            assert not lv.hashed
    lv = gg.Level([0, 512], [32], 0, 1)                      # res^3 = 32768 > 512 rows: x + 32 y, z dropped, modulo the rows
    p = rng.integers(0, 32, size=(100, 3))
    assert np.array_equal(lv.rows(p[:, 0], p[:, 1], p[:, 2]), (p[:, 0] + 32 * p[:, 1]) % 512)


@pytest.mark.parametrize("gridtype,align,interp", COMBOS)
def test_weights_sum_to_one_and_a_vertex_returns_its_row(gridtype, align, interp):
    emb, offs, res = small_table(2)
    x = synth.hash_tensor((65, 3), 21, 1.0).numpy()
    case = gg.Case(x, emb, offs, res, 1.0, 6, 2, gridtype, align, interp)
    for lv in case.levels:
        _, _, _, _, w = case._geom(lv, F64)
        assert np.abs(w.sum(1) - 1).max() <= 8 * 2.0 ** -53
        _, _, _, _, w32 = case._geom(lv, F32)
        assert np.abs(w32.astype(F64).sum(1) - 1).max() <= 8 * 2.0 ** -24
    # one level whose vertices are dyadic in u: res 4 (res - 1 = 4 under align_corners: res 5), 64 rows
    r = 5 if align else 4
    T = 64
    tab = synth.hash_tensor((T, 2), 22, 0.1).numpy()
    k = np.array([[0, 0, 0], [1, 2, 3], [3, 3, 3], [2, 0, 1]])
    u = k / 4.0 if align else (k + 0.5) / 4.0
    one = gg.Case((2 * u - 1).astype(F32), tab, [0, T], [r], 1.0, 1, 2, gridtype, align, interp)
    rows = one.levels[0].rows(k[:, 0], k[:, 1], k[:, 2])
    assert np.array_equal(one.forward(), tab[rows])
    assert np.array_equal(one.forward(F64), tab[rows].astype(F64))


@pytest.mark.parametrize("gridtype,align,interp", COMBOS)
def test_ddx_is_the_central_difference_away_from_cell_faces(gridtype, align, interp):
    """float64: the kernel's d/dx rule against (forward(x + h) - forward(x - h)) / 2h contracted with the same gradient, at points
    whose position inside the cell is in [0.1, 0.9] on every level used (no face, no clamp band within h)"""
    emb, offs, res = small_table(2)
    rng = np.random.default_rng(9)
    x = rng.uniform(-0.9, 0.9, size=(4000, 3)).astype(F32)
    probe = gg.Case(x, emb, offs, res, 1.0, 3, 2, gridtype, align, interp)
    keep = np.ones(len(x), bool)
    for lv in probe.levels[:3]:
        g, _ = gg.cell32(probe.u32, lv.res, align)
        f = gg.cell64(probe.u64, lv.res, align, g)
        keep &= ((f > 0.1) & (f < 0.9)).all(1)
    x = x[keep][:64]
    assert len(x) >= 16
    grad = rng.standard_normal((len(x), 12)).astype(F32)
    case = gg.Case(x, emb, offs, res, 1.0, 3, 2, gridtype, align, interp)
    got = case.grad_x(grad, F64)
    h = 2.0 ** -20                                           # exact in fp32 next to |x| < 1: x +- h are the points evaluated
    for d in range(3):
        e = np.zeros(3, F32)
        e[d] = h
        up = gg.Case(x + e, emb, offs, res, 1.0, 3, 2, gridtype, align, interp)
        dn = gg.Case(x - e, emb, offs, res, 1.0, 3, 2, gridtype, align, interp)
        step = (up.x.astype(F64) - dn.x.astype(F64))[:, d]
        fd = ((up.forward(F64) - dn.forward(F64)) * grad.astype(F64)).sum(1) / step
        assert np.abs(fd - got[:, d]).max() <= 1e-6 * np.abs(got).max(), (d, np.abs(fd - got[:, d]).max(), np.abs(got).max())


@pytest.mark.parametrize("gridtype,align", list(itertools.product((0, 1), (0, 1))))
def test_total_variation_of_a_constant_table_is_zero(gridtype, align):
    _, offs, res = small_table(4)
    emb = np.full((int(offs[-1]), 4), 0.37, F32)
    x = synth.hash_tensor((257, 3), 31, 1.02).numpy()
    case = gg.Case(x, emb, offs, res, 1.0, 6, 4, gridtype, align)
    for dtype in (F32, F64):
        t, a, cnt = case.tv(1e-3, dtype)
        assert not t.any() and not a.any() and cnt.sum() == 6 * int(case.inb.sum())


def test_total_variation_on_a_two_valued_table_matches_the_hand_computed_rows():
    """one dense level, res 4, 64 rows, one channel: every row a except the row of cell (1,1,1), which is b.
    A point in cell (1,1,1): six neighbours a -> r = 6 (b - a), q = 6 (b - a)^2.
    A point in cell (2,1,1): its left neighbour on x is b -> r = a - b, q = (a - b)^2.
    A point in cell (0,1,1): its right neighbour on x is b, no left neighbour on x -> the same r and q."""
    a, b, weight = 0.25, -0.5, 1e-2
    tab = np.full((64, 1), a, F32)
    tab[1 + 4 + 16] = b
    cells = np.array([[1, 1, 1], [2, 1, 1], [0, 1, 1], [3, 3, 3]])
    x = (2 * (cells + 0.75) / 4.0 - 1).astype(F32)          # u res - 0.5 = cell + 0.25
    case = gg.Case(x, tab, [0, 64], [4], 1.0, 1, 1)
    t, absum, cnt = case.tv(weight, F64)
    w6 = float(F32(weight)) / 6
    want = np.zeros(64)
    want[21] = w6 * 6 * (b - a) / np.sqrt(6 * (b - a) ** 2 + 1e-9)
    want[22] = want[20] = w6 * (a - b) / np.sqrt((a - b) ** 2 + 1e-9)
    assert np.abs(t[:, 0] - want).max() <= 1e-15
    assert cnt[21] == cnt[22] == cnt[20] == cnt[63] == 1 and cnt.sum() == 4
    assert abs(absum[21, 0] - abs(want[21])) <= 1e-15       # no cancellation in r here: the absolute terms are the addend


def test_weight_decay_sums_to_twice_the_weight_times_the_level_mean():
    emb, offs, res = small_table(8)
    case = gg.Case(np.zeros((1, 3), F32), emb, offs, res, 1.0, 6, 8)
    wd = case.wd(0.1, F64)
    for l in range(6):
        a, b = int(offs[l]), int(offs[l + 1])
        want = 2 * float(F32(0.1)) * emb[a:b].astype(F64).mean(0)
        assert np.abs(wd[a:b].sum(0) - want).max() <= 1e-15
    assert np.abs(case.wd(0.1, F32).astype(F64) - wd).max() <= 2 * 2.0 ** -24 * np.abs(wd).max()


# ---- the module's surface ---------------------------------------------------------------------------------------------------------
def reference_offsets(num_levels, base, log2_size, per_level_scale):
    """grid.py:125-134 written out"""
    offsets, offset = [], 0
    for i in range(num_levels):
        resolution = int(np.ceil(base * per_level_scale ** i))
        params = min(2 ** log2_size, resolution ** 3)
        params = int(np.ceil(params / 8) * 8)
        offsets.append(offset)
        offset += params
    return offsets + [offset]


def test_grid_encoder_sizes_its_table_as_the_reference_does():
    enc = GridEncoder(level_dim=4, gridtype="tiled", align_corners=True, interpolation="smoothstep", **SMALL)
    s = np.exp2(np.log2(32 / 4) / 5)                                           # grid.py:108-109
    assert enc.offsets.tolist() == reference_offsets(6, 4, 9, s) and enc.embeddings.shape == (enc.offsets[-1], 4)
    assert (enc.gridtype_id, enc.interp_id, enc.align_corners, enc.output_dim) == (1, 1, True, 24)
    enc = GridEncoder(num_levels=6, base_resolution=4, log2_hashmap_size=9, desired_resolution=None, per_level_scale=2, level_dim=1)
    assert enc.offsets.tolist() == reference_offsets(6, 4, 9, 2) and enc._res_np.tolist() == [4, 8, 16, 32, 64, 128]
    with pytest.raises(ValueError):
        GridEncoder(level_dim=3)
    with pytest.raises(ValueError):
        GridEncoder(gridtype="dense")
    with pytest.raises(ValueError):
        GridEncoder(interpolation="cubic")


def test_bare_grid_encoder_is_unchanged():
    enc = GridEncoder()
    offs, s = synth.grid_offsets()
    assert np.array_equal(enc._offsets_np, offs) and enc.offsets.dtype == torch.int32
    assert np.array_equal(enc._res_np, ops.level_resolutions(16, s, 16))
    assert enc.per_level_scale == float(s) and enc.embeddings.shape == (int(offs[-1]), 2) and enc._default_switches


def test_regularisers_before_any_backward_raise_value_error():
    enc = GridEncoder(**SMALL)
    with pytest.raises(ValueError):
        enc.grad_total_variation()
    with pytest.raises(ValueError):
        enc.grad_weight_decay()


def test_new_entry_points_are_declared_and_exported():
    names = ("mh_grid_general_fwd", "mh_grid_general_bwd", "mh_grid_grad_tv", "mh_grid_grad_wd")
    with open(os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), "..", "include", "morpheus_hip.h")) as f:
        header = f.read()
    for n in names:
        assert n in _lib.EXPORTS and f"int {n}(" in header, n
