"""CPU: properties of the hash-grid restatement (oracle/hashgrid.c).

The reference's encoder is CUDA-only and has no tests or golden vectors, so this operator's
parity is pinned by construction + invariants: level table, trilinear partition of
unity, exact table values at cell centres, dy_dx against finite differences, OOB -> 0, scatter
conservation, dense/hash switch, and a pure-python scalar re-derivation on a few points.
"""
import numpy as np
import torch

from morpheus_amd import synth
from oracle.hashgrid import (OracleGridEncoder, effective_levels, level_resolutions, oracle_grid_encode)


def make(scale=0.1):
    offs, s = synth.grid_offsets()
    emb = synth.hash_tensor((int(offs[-1]), 2), 9001, scale)
    return emb, torch.from_numpy(offs), torch.from_numpy(level_resolutions(16, s, 16)), s


def test_level_table():
    emb, offs, res, s = make()
    assert res.tolist() == [16, 19, 22, 25, 28, 32, 37, 43, 49, 56, 64, 74, 85, 98, 112, 128]
    rows = (offs[1:] - offs[:-1]).tolist()
    assert rows == [4096, 6864, 10648, 15632, 21952] + [32768] * 11
    assert int(offs[-1]) == 419640
    assert effective_levels(None, 16) == 16 and effective_levels(0.5, 16) == 8 and effective_levels(0.01, 16) == 1
    enc = OracleGridEncoder(num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=15, desired_resolution=128)
    assert enc.offsets.tolist() == offs.tolist() and enc.res_tab.tolist() == res.tolist()


def test_partition_of_unity_and_oob():
    emb, offs, res, _ = make()
    ones = torch.ones_like(emb)
    x = synth.hash_tensor((512, 3), 9002, 1.2)
    out = oracle_grid_encode(x, ones, offs, res, 1.01)
    inside = ((x.abs() <= 1.01).all(-1))
    assert torch.allclose(out[inside], torch.ones_like(out[inside]), atol=2e-6)
    assert (out[~inside] == 0).all() and (~inside).any()
    half = oracle_grid_encode(x, ones, offs, res, 1.01, max_level=0.5)
    assert (half[:, 16:] == 0).all() and torch.allclose(half[inside][:, :16], torch.ones(int(inside.sum()), 16), atol=2e-6)


def _py_index(T, r, c):
    stride, index = 1, 0
    for d in range(3):
        if stride > T:
            break
        index += c[d] * stride
        stride *= r
    if stride > T:
        index = ((c[0] * 1) ^ (c[1] * 2654435761) ^ (c[2] * 805459861)) & 0xFFFFFFFF
    return index % T


def test_cell_centres_and_scalar_rederivation():
    emb, offs, res, _ = make()
    bound = 1.0
    rng = np.random.RandomState(0)
    for l in (0, 4, 5, 6, 11, 15):
        r, T = int(res[l]), int(offs[l + 1] - offs[l])
        cells = rng.randint(0, r, size=(32, 3))
        u = (cells + 0.5) / r                       # cell centres: pos - 0.5 is an exact integer
        x = torch.tensor(u * 2 - 1, dtype=torch.float32)
        out = oracle_grid_encode(x, emb, offs, res, bound)
        for k in range(32):
            row = _py_index(T, r, [int(v) for v in cells[k]])
            want = emb[int(offs[l]) + row]
            assert torch.allclose(out[k, 2 * l:2 * l + 2], want, atol=2e-6), (l, k)
    # dense below, hashed above (res^3 <= T  <=>  l <= 5)
    assert all((int(res[l]) ** 3 <= int(offs[l + 1] - offs[l])) == (l <= 5) for l in range(16))


def test_dydx_matches_finite_differences_and_autograd_scatter():
    emb, offs, res, _ = make()
    emb = emb.clone().requires_grad_(True)
    # keep away from the half-cell border band, where the kernel's slope deliberately ignores the clamp
    x = (synth.hash_tensor((256, 3), 9003, 0.9)).requires_grad_(True)
    out = oracle_grid_encode(x, emb, offs, res, 1.01)
    w = synth.hash_tensor(tuple(out.shape), 9004, 1.0)
    (out * w).sum().backward()
    gx = x.grad.clone()
    eps = 1e-3
    fd = torch.zeros_like(gx)
    with torch.no_grad():
        for d in range(3):
            e = torch.zeros(1, 3)
            e[0, d] = eps
            fp = oracle_grid_encode(x + e, emb, offs, res, 1.01).double()
            fm = oracle_grid_encode(x - e, emb, offs, res, 1.01).double()
            fd[:, d] = (((fp - fm) * w.double()).sum(-1) / (2 * eps)).float()
    # piecewise-linear function: central differences straddle kinks at fine levels -> loose check
    rel = (gx - fd).abs().median() / fd.abs().median()
    assert rel < 0.05, rel
    # scatter conservation: sum of grad_emb over a level == sum_b grad[b, level] (weights sum to 1)
    ge = emb.grad
    inside = (x.detach().abs() <= 1.01).all(-1)
    for l in range(16):
        tot = ge[int(offs[l]):int(offs[l + 1])].sum(0)
        want = w[inside][:, 2 * l:2 * l + 2].sum(0)
        assert torch.allclose(tot, want, rtol=1e-4, atol=1e-4), l


def test_border_band_slope_follows_kernel():
    """Inside the half-cell border band the value is flat (pos clamped) but dy_dx is NOT zeroed
    (gridencoder.cu:205-247 ignores the clamp) -- the oracle must follow the kernel."""
    emb, offs, res, _ = make()
    x = torch.tensor([[-1.0 + 1e-3, 0.1, 0.2]], requires_grad=True)   # u ~ 5e-4 < 0.5/res for all levels
    out = oracle_grid_encode(x, emb, offs, res, 1.0)
    out[:, 0].sum().backward()
    with torch.no_grad():
        flat = oracle_grid_encode(x + torch.tensor([[1e-4, 0, 0]]), emb, offs, res, 1.0)
    assert torch.allclose(flat[:, 0], out[:, 0].detach(), atol=1e-7)
    assert x.grad[0, 0].abs() > 0


def test_second_derivation_agrees_on_1e5_points():
    """oracle/hashgrid.c against oracle/hashgrid_np.py -- a second restatement written independently from the .cu
    (vectorised numpy over [points, corners]) -- on 10^5 points: interior, the border band, exact cell boundaries and
    out-of-range inputs, all 16 levels (dense rows for levels 0-5, hashed from level 6: 37^3 > 32768): features to 2
    ulp, d/du to 1e-5 of the level's slope scale, embedding gradients to 1e-6 relative."""
    from oracle import hashgrid_np as hnp
    from oracle.hashgrid import _OracleGridEncode
    emb, offs, res, _ = make()
    M = 100_000
    u = (synth.hash_tensor((M, 3), 9100, 0.55) + 0.5).clamp_(-0.05, 1.05)             # ~9% outside [0,1] before the clamp
    u[:2000] = (torch.round(u[:2000] * 37) + 0.5) / 37                                   # level-6 cell boundaries (res 37)
    u[2000:4000] = torch.round(u[2000:4000] * 32) / 32                                   # level-5 cell centres / borders
    u[4000:4200, 0] = 0.0
    u[4200:4400, 1] = 1.0
    u[4400:4500] = 1.0 + 1e-7                                                            # just outside
    offs_np, res_np, emb_np = offs.numpy(), res.numpy(), emb.numpy()
    for n_levels in (16, 8):
        ut = u.clone().requires_grad_(True)
        embt = emb.clone().requires_grad_(True)
        out_c = _OracleGridEncode.apply(ut, embt, offs, res, n_levels, True)
        out_np = hnp.forward(u.numpy(), emb_np, offs_np, res_np, n_levels)
        ulp = np.spacing(np.abs(out_np).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(out_c.detach().numpy().astype(np.float64) - out_np) <= 2 * ulp + 1e-12)
        # the dense -> hash switch really happens between levels 5 and 6
        T = offs_np[1:] - offs_np[:-1]
        assert res_np[5] ** 3 <= T[5] and res_np[6] ** 3 > T[6]
        go = synth.hash_tensor((M, 32), 9101, 1.0)
        (out_c * go).sum().backward()
        g_np = hnp.backward_embeddings(u.numpy(), go.numpy(), offs_np, res_np, n_levels, emb.shape[0], 2)
        ge = embt.grad.numpy().astype(np.float64)
        assert np.abs(ge - g_np).max() <= 1e-6 * np.abs(g_np).max() + 1e-9
        d_np = hnp.dy_du(u.numpy()[:20000], emb_np, offs_np, res_np, n_levels)          # [m, L, 3, C]
        gu_np = np.einsum("mldc,mlc->md", d_np.astype(np.float64), go.numpy()[:20000].reshape(-1, 16, 2).astype(np.float64))
        gu_c = ut.grad.numpy()[:20000].astype(np.float64)
        assert np.abs(gu_c - gu_np).max() <= 1e-5 * np.abs(gu_np).max()


def test_float64_encoder_agrees_with_the_c_restatement():
    """oracle/hashgrid_f64.py (the yardstick's encoder: vectorised torch, double) against oracle/hashgrid.c (scalar C, fp32) on
    20 000 points incl. out-of-box ones: the same cells, corners, hash and weights -- the difference is the fp32 round-off of the
    position (u * res - 0.5 carries ~res * 6e-8 of a cell) times the feature slope."""
    import torch
    from morpheus_amd import synth
    from oracle.hashgrid import OracleGridEncoder
    from oracle.hashgrid_f64 import OracleGridEncoderF64
    kw = dict(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=15, desired_resolution=128)
    a, b = OracleGridEncoder(**kw), OracleGridEncoderF64(**kw)
    emb = synth.make_state("b")["encoder.embeddings"]
    a.embeddings.data.copy_(emb)
    b.embeddings.data.copy_(emb.double())
    assert torch.equal(a.offsets, b.offsets)
    x = synth.hash_tensor((20000, 3), 300, 1.15)
    with torch.no_grad():
        for ml in (None, 0.5):
            ya, yb = a(x, bound=1.01, max_level=ml), b(x.double(), bound=1.01, max_level=ml)
            assert yb.dtype == torch.float64
            assert float((ya.double() - yb).abs().max()) < 5e-6 and float(yb.abs().max()) > 0.05
            assert torch.equal(ya == 0, yb == 0) or float(((ya == 0) != (yb == 0)).float().mean()) < 1e-4   # OOB points and skipped levels


def _dydx_points():
    """u in [0,1]^3 (plus a few just outside) where the clamp and the cells matter: the half-texel band at each of the six faces of
    every level (u < 0.5 / res or u > 1 - 0.5 / res), the faces themselves (u = 0, u = 1), cell faces of the finest level (res 128)
    and of level 5 (res 32), random interior points, and points just outside.  Every coordinate is a multiple of 2^-16 or one of
    the exact values above, so that u * res - 0.5 is exact in fp32 as well as in double: the three implementations then place every
    point in the same cell and differ by the round-off of the weights and differences only (a point within an fp32 ulp of a cell face
    would otherwise switch cells between them, a discrete event that is not what this compares)."""
    q = 2.0 ** -16
    rnd = ((synth.hash_tensor((3000, 3), 9200, 0.5) + 0.5).double() / q).round() * q
    band = rnd[:1200].clone()
    for k in range(1200):                                             # 200 points per face: one axis in the band of level 0
        ax, hi = (k // 200) % 3, (k // 600) == 1
        v = float((synth.hash_tensor((1,), 9300 + k, 0.5) + 0.5).item()) * (0.5 / 16)
        v = round(v / q) * q
        band[k, ax] = 1.0 - v if hi else v
    faces = rnd[1200:1500].clone()
    for k in range(300):
        faces[k, k % 3] = 0.0 if (k // 3) % 2 == 0 else 1.0
    cells = rnd[1500:2100].clone()
    cells[:300, 0] = (torch.floor(cells[:300, 0] * 128) + 0.5) / 128        # pos = u * 128 - 0.5 an integer: a cell face of level 15
    cells[300:, 1] = (torch.floor(cells[300:, 1] * 32) + 0.5) / 32          # ... of level 5 (dense)
    out = rnd[2100:2200].clone()
    out[:50, 0] = 1.0 + q
    out[50:, 2] = -q
    u = torch.cat([band, faces, cells, out, rnd[2200:]])
    assert torch.equal(u.float().double(), u)
    return u


def test_float64_encoder_input_gradient_follows_the_kernel_rule():
    """The float64 yardstick's d/dx (oracle/hashgrid_f64.py) is the kernel's rule (gridencoder.cu:206-246: per axis, the sum over
    the 4 corner pairs of w * (right - left) * res, the border clamp ignored; zero outside the box) -- the rule of oracle/hashgrid.c
    and oracle/hashgrid_np.py -- not autograd's slope through the clamp, which is zero in the half-texel band at every face of the
    box: compared to both fp32 restatements, per point, on the band at all six faces, the faces themselves, cell faces of a dense
    and of a hashed level and points just outside, all 16 levels and the first 8 (max_level None / 0.5)."""
    from oracle import hashgrid_np as hnp
    from oracle.hashgrid import _OracleGridEncode
    from oracle import hashgrid_f64
    from oracle.hashgrid_f64 import grid_encode_f64
    emb, offs, res, _ = make()
    u = _dydx_points()
    M = u.shape[0]
    go = synth.hash_tensor((M, 32), 9201, 1.0)
    offs_np, res_np, emb_np = offs.numpy(), res.numpy(), emb.numpy()
    for ml, n_levels in ((None, 16), (0.5, 8)):
        # the f64 grid through autograd, in world units with bound 0.5 (x = u - 0.5 exactly, dx/du = 1)
        x = (u - 0.5).requires_grad_(True)
        y = grid_encode_f64(x, emb.double(), offs.tolist(), res_np, 0.5, ml)
        (y * go.double()).sum().backward()
        g64 = x.grad.numpy()
        # the numpy restatement, per level / axis / channel, contracted with the same output gradient
        d_np = hnp.dy_du(u.float().numpy(), emb_np, offs_np, res_np, n_levels).astype(np.float64)
        g_np = np.einsum("mldc,mlc->md", d_np, go.numpy().reshape(M, 16, 2).astype(np.float64))
        # the C restatement's backward (its dydx buffer)
        ut = u.float().requires_grad_(True)
        (_OracleGridEncode.apply(ut, emb, offs, res, n_levels, True) * go).sum().backward()
        g_c = ut.grad.numpy().astype(np.float64)
        scale = np.abs(g_np).max()
        assert scale > 1.0
        # per point: the fp32 restatements carry ~1e-7 relative round-off of each of the 16 levels' slope (up to res 128 x 0.2)
        tol = 2e-6 * scale
        for name, other in (("hashgrid_np.dy_du", g_np), ("hashgrid.c dydx", g_c)):
            bad = np.abs(g64 - other).max(-1) > tol
            assert not bad.any(), (name, ml, int(bad.sum()), np.nonzero(bad)[0][:10], float(np.abs(g64 - other).max()))
        # the per-level Jacobian too (not only its contraction), where the band lies: the first 1 500 points
        d64 = hashgrid_f64.grid_dy_du_f64(u[:1500], emb.double(), offs.tolist(), res_np, n_levels).numpy()
        assert np.abs(d64 - d_np[:1500]).max() <= 2e-6 * np.abs(d_np).max()
        # the band is not vacuous: at the three lower faces the kernel keeps the slope of the border cell along the band's axis
        # (autograd through the clamp: zero); at the upper faces the clamped right corner is the left one, zero in both; points
        # outside get none
        lower = g64[np.arange(600), np.arange(600) // 200]
        assert (np.abs(lower) > 1e-3 * scale).mean() > 0.95
        assert (g64[2100:2200] == 0).all() and (g_np[2100:2200] == 0).all()
        assert (d_np[:, n_levels:] == 0).all()


def test_float64_encoder_values_and_table_gradient():
    """Values of the float64 grid unchanged by its backward (the same function with and without a graph), and its table gradient
    (autograd's scatter) equal to hashgrid_np.backward_embeddings on the same points, dense and hashed levels, max_level None / 0.5."""
    from oracle import hashgrid_np as hnp
    from oracle.hashgrid_f64 import grid_encode_f64
    emb, offs, res, _ = make()
    u = _dydx_points()
    M = u.shape[0]
    go = synth.hash_tensor((M, 32), 9202, 1.0)
    offs_np, res_np = offs.numpy(), res.numpy()
    for ml, n_levels in ((None, 16), (0.5, 8)):
        with torch.no_grad():
            y0 = grid_encode_f64(u - 0.5, emb.double(), offs.tolist(), res_np, 0.5, ml)
        e = emb.double().requires_grad_(True)
        x = (u - 0.5).requires_grad_(True)
        y = grid_encode_f64(x, e, offs.tolist(), res_np, 0.5, ml)
        assert torch.equal(y.detach(), y0)
        ref = hnp.forward(u.float().numpy(), emb.numpy(), offs_np, res_np, n_levels).astype(np.float64)
        assert np.abs(y0.numpy() - ref).max() <= 1e-6 * np.abs(ref).max()
        (y * go.double()).sum().backward()
        g_np = hnp.backward_embeddings(u.float().numpy(), go.numpy(), offs_np, res_np, n_levels, emb.shape[0], 2)
        ge = e.grad.numpy()
        assert np.abs(ge - g_np).max() <= 1e-6 * np.abs(g_np).max()
        rows_touched = np.abs(g_np).sum(-1) > 0
        assert rows_touched[:int(offs[6])].any() and rows_touched[int(offs[6]):].any() == (n_levels > 6)


# ---- the float64 table-gradient helpers and the inputs of tests/test_gpu_grid_f64.py -----------------------------------------------
def test_table_gradient_helper_equals_the_autograd_route_exactly():
    """grid_table_grad_f64 (one pass of the scatter, no value graph) against _GridEncodeF64's table gradient: the same bits --
    interior, faces, points outside, all levels and the first eight."""
    from tests import grid_f64_cases as gc
    from oracle.hashgrid_f64 import grid_encode_f64, grid_table_grad_f64
    emb, offs, res = gc.grid_setup()
    for gen in (lambda: gc.gen_faces_outside(6000), lambda: gc.gen_graded(5000)):
        x, grad = gen()
        for ml in (None, 0.5):
            e = emb.double().requires_grad_(True)
            grid_encode_f64(x.double(), e, offs.tolist(), res, gc.BOUND, ml).backward(grad.double())
            t = grid_table_grad_f64(x, grad, offs.tolist(), res, gc.BOUND, effective_levels(ml, 16))
            assert t.dtype == torch.float64 and float(t.abs().max()) > 0 and torch.equal(t, e.grad)


def test_term_counts_equal_a_brute_force_count():
    """grid_term_counts against a count over hashgrid_np's corner rows, point by point: interior points, the band, the faces, cell faces
    and points outside the box (which count nothing); coordinates chosen so that fp32 and double agree on every cell."""
    from oracle import hashgrid_np as hnp
    from oracle.hashgrid_f64 import grid_term_counts
    emb, offs, res, _ = make()
    u = _dydx_points()
    for n_levels in (16, 8):
        want = np.zeros(int(offs[-1]), dtype=np.int64)
        for l in range(n_levels):
            T = int(offs[l + 1] - offs[l])
            rows, _, _, _, ok = hnp._level(u.float().numpy(), int(res[l]), T)
            for k in np.nonzero(ok)[0]:
                for c in range(8):
                    want[int(offs[l]) + int(rows[k, c])] += 1
        got = grid_term_counts(u - 0.5, offs.tolist(), res.numpy(), 0.5, n_levels)
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
        inside = int(((u >= 0) & (u <= 1)).all(-1).sum())
        assert inside < u.shape[0] and int(got.sum()) == inside * 8 * n_levels
        assert int(got[int(offs[n_levels]):].sum()) == 0


def test_gpu_case_inputs_are_fair_to_the_reference():
    """Every input generator of tests/test_gpu_grid_f64.py at a reduced size through the fp32 C restatement: the reference itself
    stays inside what the GPU test asks of the HIP kernel -- finite per-level errors against float64 on every level that is on (so
    that 3 x its error is a gate and not a blank cheque: below 2^-13 in relative L2 and max-norm, 50 fp32 ulps per level), exactly
    zero rows where no term lands, and the headroom rule's thresholds where the GPU test expects them."""
    from tests import grid_f64_cases as gc
    emb, offs, res = gc.grid_setup()
    assert [gc.acc_shift_of(M) for M in (1 << 19, (1 << 19) + 1, (1 << 20) + 1, (1 << 21) + 1)] == [0, 1, 2, 3]
    cases = [("uniform", gc.gen_uniform(1 << 15), None), ("rays", gc.gen_rays(512, 64), None),
             ("faces", gc.gen_faces_outside(1 << 15), None), ("progressive 0.5", gc.gen_uniform(1 << 15), 0.5),
             ("progressive 0.75", gc.gen_uniform(1 << 15), 0.75), ("graded", gc.gen_graded((1 << 15) + 1), None)]
    for name, (x, grad), ml in cases:
        ora, t64, cnt = gc.oracle_tables(x, grad, emb, offs, res, gc.BOUND, ml)
        n_on = effective_levels(ml, 16)
        l2, mx = gc.level_metrics(ora, t64, offs)
        assert all(0 < v < 2.0 ** -13 for v in l2[:n_on] + mx[:n_on]), (name, l2, mx)
        assert all(v == 0 for v in l2[n_on:] + mx[n_on:]), name
        assert not ora[cnt == 0].any() and int((cnt == 0).sum()) > 0, name
        assert not t64[cnt == 0].any()
        gc.check_levels(name, ora, ora, t64, cnt, offs, log=lambda *_: None)      # the gate's own code on a result that must pass
    x, _ = gc.gen_faces_outside(1 << 15)
    assert int((~(x.abs() <= gc.BOUND).all(-1)).sum()) >= (1 << 15) // 3


def test_one_cell_closed_form_agrees_with_float64():
    """the closed form the GPU test holds the 2^21 + 1 copies of one point to (n * rint(w g0 / q) * q) against the float64 scatter of a
    reduced number of copies, scaled: they differ by the rounding of each term onto the grid only, at most n q / 2 per row"""
    from tests import grid_f64_cases as gc
    from oracle.hashgrid_f64 import grid_table_grad_f64
    emb, offs, res = gc.grid_setup()
    M = (1 << 21) + 1
    want, cnt = gc.one_cell_expected(M, emb.shape[0], offs, res)
    _, q = gc.quantum(torch.tensor([gc.ONE_CELL_G0]), M)
    assert q == 2.0 ** -37
    m = 64
    x = torch.tensor([[2 * u - 1 for u in gc.ONE_CELL_U]], dtype=torch.float32).repeat(m, 1)
    t64 = grid_table_grad_f64(x, torch.full((m, 32), gc.ONE_CELL_G0), offs.tolist(), res, gc.ONE_CELL_BOUND, 16)
    assert int((cnt > 0).sum()) == 128 and int(cnt.max()) == M
    assert torch.equal(t64[:, 0], t64[:, 1]) and torch.equal(t64[:, 0] != 0, want != 0)
    assert float((want - t64[:, 0] * (M / m)).abs().max()) <= M * q / 2
    # the largest row's fixed-point sum: inside the +-2^62 the headroom rule keeps, and far above what a 32-bit or a double (2^53)
    # intermediate holds exactly
    assert 2.0 ** 53 < float(want.max()) / q < 2.0 ** 62


def test_graded_input_exception_share_of_the_reference():
    """The dynamic-range input at the GPU test's own size (2^20 + 1 points) through the fp32 C restatement:
      * it bites: whole buckets of entries lie below the grid's quantum on some levels and none on the fully hashed ones;
      * the restatement passes the per-entry bound and every bucket's gate by construction (its own error defines them);
      * the share of entries for which the restatement on points moved by one fp32 ulp per coordinate breaks the bound without its
        n q / 2 term is measured: grid_f64_cases.MOVED_EXCEPTION_SHARE records it (the GPU test allows twice that)."""
    from tests import grid_f64_cases as gc
    emb, offs, res = gc.grid_setup()
    M = (1 << 20) + 1
    x, grad = gc.gen_graded(M)
    ora, t64, cnt = gc.oracle_tables(x, grad, emb, offs, res, gc.BOUND)
    G, q = gc.quantum(grad, M)
    assert gc.acc_shift_of(M) == 2 and q == G * 2.0 ** -38
    below = [(int(((t64[int(offs[l]):int(offs[l + 1])].abs() < q) & (t64[int(offs[l]):int(offs[l + 1])] != 0)).sum())) for l in range(16)]
    assert below[0] > 1000 and below[5] > 5000 and below[15] == 0, below
    n_checked, bad, n_broke, allowed = gc.graded_checks(ora.double(), ora, t64, cnt, grad, M, offs, log=lambda *_: None)
    assert n_checked >= 12 and not bad and n_broke == 0 and allowed == 2 * gc.MOVED_EXCEPTIONS_MEASURED
    share, n = gc.moved_exception_share(x, grad, emb, offs, res, ora, t64, gc.buckets(t64, offs))
    print(f"moved-by-one-ulp exception share of the fp32 restatement: {n} of {t64.numel()} = {share:.3e}")
    assert 0 < n <= gc.MOVED_EXCEPTIONS_MEASURED and share <= gc.MOVED_EXCEPTION_SHARE
