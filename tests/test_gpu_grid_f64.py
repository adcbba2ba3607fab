"""GPU: the hash-grid table gradient (grid_bwd_brick_kernel + grid_acc_finalize_kernel, csrc/hashgrid.hip) held to FLOAT64, level
by level, at full size -- and the max|grad| words the field backward hands to it.

Yardsticks: oracle/hashgrid_f64.py (float64) and oracle/hashgrid.c (the fp32 restatement of the reference's kernel, float atomics)
on the same fp32 inputs; gate hip <= max(3 x oracle_fp32, 2^-22) per level in relative L2 and in max-norm (tests/grid_f64_cases.py
has the definitions, the input generators and the reasons for each constant), plus the zero pattern.

Every size listed in the cases below ALWAYS runs -- there is no slow subset: the oracle work of the whole file (float64 scatter,
term counts and the C restatement, 4 - 15 us per point on 16 CPU threads) is between 35 s and 2.5 minutes, under the three allowed: uniform 2^19, 2^19 + 1,
2^20 + 1, 2^21 + 1 (acc_shift 0, 1, 2, 3), the 1.5 M converging-ray cloud, 2^18 faces / outside, 2 x 2^18 progressive, 2^19 + 1
through field_query (two tables), 2^20 + 1 graded, 2^18 after a non-finite gradient; an input's yardsticks are computed once and
shared by the runs with and without d/dx.  The one-cell case (2^21 + 1 points, acc_shift 3) has a closed form and costs nothing.
Each test prints its figures (lines starting GRIDF64) before it asserts."""
import functools
import time

import numpy as np
import pytest
import torch

from tests import grid_f64_cases as gc
from tests.grid_f64_cases import BOUND

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _hip_table(x, grad, emb, offs, res, bound=BOUND, max_level=None, need_dx=False, finite_dx=True):
    """table gradient of the public autograd op (the form is chosen by call size, as in production)"""
    from morpheus_amd import ops
    xg = x.to(DEV).requires_grad_(need_dx)
    e = emb.to(DEV).clone().requires_grad_(True)
    t0 = time.time()
    ops.grid_encode(xg, e, offs, res, bound, max_level).backward(grad.to(DEV))
    torch.cuda.synchronize()
    print(f"GRIDF64 time gpu {time.time() - t0:.2f} s for {x.shape[0]} points")
    if need_dx:
        assert xg.grad is not None and (not finite_dx or bool(torch.isfinite(xg.grad).all()))
    return e.grad.cpu()


@functools.lru_cache(maxsize=None)
def _case(name, M=0, max_level=None):
    """(x, grad, C restatement's table gradient, float64 table gradient, term counts) of a named input -- computed once"""
    emb, offs, res = gc.grid_setup()
    x, grad = {"uniform": lambda: gc.gen_uniform(M), "rays": gc.gen_rays, "faces": lambda: gc.gen_faces_outside(M),
               "graded": lambda: gc.gen_graded(M)}[name]()
    t0 = time.time()
    ora, t64, cnt = gc.oracle_tables(x, grad, emb, offs, res, BOUND, max_level)
    print(f"GRIDF64 time oracle {time.time() - t0:.2f} s for {x.shape[0]} points ({name})")
    return x, grad, ora, t64, cnt


# ---- 2. table gradient against float64, per level ------------------------------------------------------------------------------
@pytest.mark.parametrize("need_dx", [False, True])
@pytest.mark.parametrize("M", [1 << 19, (1 << 19) + 1, (1 << 20) + 1, (1 << 21) + 1])
def test_uniform_points_per_level(M, need_dx):
    """acc_shift = 0, 1, 2, 3 (the launcher's headroom rule); the last two sizes also take the staged forms when d/dx is asked for"""
    assert gc.acc_shift_of(M) == {1 << 19: 0, (1 << 19) + 1: 1, (1 << 20) + 1: 2, (1 << 21) + 1: 3}[M]
    emb, offs, res = gc.grid_setup()
    x, grad, ora, t64, cnt = _case("uniform", M)
    hip = _hip_table(x, grad, emb, offs, res, need_dx=need_dx)
    gc.check_levels(f"uniform M={M} dx={int(need_dx)}", hip, ora, t64, cnt, offs)


@pytest.mark.parametrize("need_dx", [False, True])
def test_converging_rays_per_level(need_dx):
    """hot bricks split into many work items that share rows (1.5 M points)"""
    emb, offs, res = gc.grid_setup()
    x, grad, ora, t64, cnt = _case("rays")
    hip = _hip_table(x, grad, emb, offs, res, need_dx=need_dx)
    gc.check_levels(f"rays M={x.shape[0]} dx={int(need_dx)}", hip, ora, t64, cnt, offs)


def test_faces_and_outside_per_level():
    """the border clamp min(g + 1, res - 1) and rows written by nobody: a third of the points on the box's faces, a third within one
    fine cell of a face, a third outside"""
    emb, offs, res = gc.grid_setup()
    x, grad, ora, t64, cnt = _case("faces", 1 << 18)
    outside = ~(x.abs() <= BOUND).all(-1)
    assert int(outside.sum()) >= (1 << 18) // 3 and int((x.abs() == BOUND).any(-1).sum()) >= (1 << 18) // 3
    assert int((cnt == 0).sum()) > 0
    hip = _hip_table(x, grad, emb, offs, res, need_dx=True)
    gc.check_levels("faces+outside M=2^18", hip, ora, t64, cnt, offs)


@pytest.mark.parametrize("max_level", [0.5, 0.75])
def test_progressive_levels_per_level(max_level):
    """rows of switched-off levels stay exactly 0 (they have no terms: the zero-pattern assertion), the others pass the gate"""
    emb, offs, res = gc.grid_setup()
    x, grad, ora, t64, cnt = _case("uniform", 1 << 18, max_level)
    n_on = int(max_level * 16)
    assert int(cnt[int(offs[n_on]):].sum()) == 0 and int(cnt[:int(offs[n_on])].sum()) > 0
    hip = _hip_table(x, grad, emb, offs, res, max_level=max_level, need_dx=True)
    assert not hip[int(offs[n_on]):].any()
    gc.check_levels(f"progressive max_level={max_level}", hip, ora, t64, cnt, offs)


def test_one_cell_closed_form():
    """The int64 headroom case: 2^21 + 1 copies of ONE point, every upstream gradient +g0 -- 2 M terms of the same sign on eight
    rows per level.  Every touched row is n * rint(w g0 / q) * q exactly before its one conversion to fp32
    (grid_f64_cases.one_cell_expected); a lost acc_shift, a 32-bit intermediate or a wrapped sum is a gross error.  Equality to
    one fp32 ulp (the conversion goes int64 -> double -> float: a sum above 2^53 is rounded twice)."""
    emb, offs, res = gc.grid_setup()
    M = (1 << 21) + 1
    assert gc.acc_shift_of(M) == 3
    want, cnt = gc.one_cell_expected(M, emb.shape[0], offs, res)
    x = torch.tensor([[2 * u - 1 for u in gc.ONE_CELL_U]], dtype=torch.float32).repeat(M, 1)
    grad = torch.full((M, 32), gc.ONE_CELL_G0)
    hip = _hip_table(x, grad, emb, offs, res, bound=gc.ONE_CELL_BOUND).double()
    w32 = want.float()
    ulp = torch.from_numpy(np.spacing(w32.abs().numpy())).double()
    touched = cnt > 0
    assert int(touched.sum()) == 128 and int((want[touched] > 0).sum()) >= 100
    for ch in range(2):
        err = (hip[:, ch] - w32.double()).abs()
        worst = float((err[touched] / ulp[touched]).max())
        print(f"GRIDF64 one cell channel {ch}: worst error {worst:.2f} ulp, largest row {float(want.max()):.6e} (hip {float(hip[:, ch].max()):.6e})")
        assert bool((err <= ulp).all()), f"channel {ch}: {worst} ulp"
        assert not hip[~touched, ch].any()


def test_field_query_table_gradients(monkeypatch):
    """the accumulate_dx = 2 form with the producer-supplied gmax words, through the model's one-node field query: both tables'
    gradients against float64 evaluated on the g_fs / g_fc the field backward produced, and the words it handed over"""
    from morpheus_amd import ops, harness
    M = (1 << 19) + 1
    model = harness.build_model("b", DEV, None)
    assert not model.composed_field
    offs, res = model.encoder._offsets_np, model.encoder._res_np
    g = torch.Generator().manual_seed(61)
    x = (torch.rand(M, 3, generator=g) * 2 - 1) * BOUND
    topo = torch.randn(M, 2, generator=g) * 0.3
    ws, wg, wc = torch.randn(M, generator=g), torch.randn(M, generator=g) * 0.01, torch.randn(M, 3, generator=g)
    seen, orig = {}, ops._field_bwd

    def spy(*a, **k):
        r = orig(*a, **k)
        seen["g_fs"], seen["g_fc"], seen["gmax"], seen["given"] = r[1].clone(), r[2].clone(), r[5].clone(), k.get("gmax") is not None
        return r

    monkeypatch.setattr(ops, "_field_bwd", spy)
    xg = x.to(DEV).requires_grad_(True)
    model.zero_grad()
    sdf, sigma, albedo = model.get_sigma_albedo(xg, topo.to(DEV))
    ((sdf * ws.to(DEV)).sum() + (sigma * wg.to(DEV)).sum() + (albedo * wc.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    assert seen and seen["given"], "the query did not join the pass's accumulator: the handed-over words were not exercised"
    assert float(model.bound) == pytest.approx(BOUND, rel=1e-7)
    emb = model.encoder.embeddings.detach().cpu()
    for name, gf, word, table in (("sdf table", seen["g_fs"], seen["gmax"][0], model.encoder.embeddings),
                                  ("colour table", seen["g_fc"], seen["gmax"][1], model.encoder_c.embeddings)):
        assert int(word) == int(gf.abs().max().view(torch.int32)), name
        t0 = time.time()
        ora, t64, cnt = gc.oracle_tables(x, gf.cpu(), emb, offs, res, BOUND)
        print(f"GRIDF64 time oracle {time.time() - t0:.2f} s for {M} points (field_query {name})")
        gc.check_levels(f"field_query {name} M={M}", table.grad.cpu(), ora, t64, cnt, offs)


# ---- 3. dynamic range: the fixed-point grid as a checked bound ---------------------------------------------------------------
def test_graded_gradients_dynamic_range():
    """2^20 + 1 uniform points, |upstream gradient| falling by 2^-60 across the box.  G = the power of two strictly above
    max|grad|, q = G 2^-(40 - acc_shift), n_i = the entry's term count -- recomputed here from the inputs.
      * entries bucketed by level and floor(log2|f64| / 8); every bucket of >= 64 entries that all satisfy |f64| >= 2^20 n q (the grid
        is finer than fp32 for them) passes the per-level gate with the bucket's own norm and maximum: small-gradient regions are
        held to their own scale, not the table's;
      * ALL entries: |hip - f64| <= n q / 2 + 2^-23 |f64| + 3 e, e = the C restatement's largest error in the entry's level and
        bucket; counted exceptions at most twice MOVED_EXCEPTION_SHARE (grid_f64_cases.py: the rate at which an equally valid fp32
        evaluation of the cell index differs);
      * reported, not gated: per level, the share of entries non-zero in float64 and zero in the HIP result, and the smallest
        |f64| / max|grad| that survives."""
    emb, offs, res = gc.grid_setup()
    M = (1 << 20) + 1
    x, grad, ora, t64, cnt = _case("graded", M)
    G, q = gc.quantum(grad, M)
    assert gc.acc_shift_of(M) == 2 and q == G * 2.0 ** -38 and G > float(grad.abs().max()) >= G / 2
    hip = _hip_table(x, grad, emb, offs, res, need_dx=True).double()
    n_checked, bad, n_broke, allowed = gc.graded_checks(hip, ora, t64, cnt, grad, M, offs)
    assert n_checked >= 12, "the graded input no longer fills enough buckets"
    assert not bad, f"(level, log2 bucket, l2 hip, l2 oracle, mx hip, mx oracle) beyond max(3 x oracle, 2^-22): {bad}"
    assert n_broke <= allowed
    assert not hip[cnt == 0].any()


# ---- 4. the handed-over maximum ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 31, 33, 255, 4099, 65537])
@pytest.mark.parametrize("mlp", ["b3", "f32"])
@pytest.mark.parametrize("with_color", [True, False])
def test_field_backward_hands_over_the_maximum(with_color, mlp, M, monkeypatch):
    """ops._field_bwd with a zeroed gmax pair and upstream gradients of mixed magnitude: the words are bit-equal to max|g_fs| /
    max|g_fc| of the tensors it wrote (too small a word saturates the largest terms of the table gradient, too large a one -- a
    padding lane, a stale value -- coarsens its grid).  A second call into the SAME words with gradients 2^-20 times as large
    leaves them where they were: the kernel only ever raises a word (atomicMax), which is why the pool hands every query fresh
    zeroed words and why the brick kernel clamps against a stale maximum."""
    from morpheus_amd import ops
    from tests.test_gpu_ops import _set_mlp, _state, _wn
    _set_mlp(monkeypatch, ops, mlp)
    g = torch.Generator().manual_seed(1000 + M)
    pg = _state("b", DEV)
    x = (torch.rand(M, 3, generator=g) * 2 - 1).to(DEV).requires_grad_(True)
    fs, fc = [(torch.randn(M, 32, generator=g) * 0.1).to(DEV).requires_grad_(True) for _ in range(2)]
    topo = (torch.randn(M, 2, generator=g) * 0.3).to(DEV).requires_grad_(True)
    mag = torch.exp2(-20 * torch.rand(M, generator=g))                           # mixed magnitude, by point
    ws, wg, wc = [(torch.randn(s, generator=g) * mag.reshape(-1, *[1] * (len(s) - 1)) * k).to(DEV)
                  for s, k in (((M,), 1.0), ((M,), 0.01), ((M, 3), 1.0))]
    Ws = [pg[f"sdf_net.net.{l}.weight"] for l in range(3)]
    Wc = [_wn(pg, "color_net", l) for l in range(3)]
    bs = [pg[f"sdf_net.net.{l}.bias"] for l in range(3)]
    bc = [pg[f"color_net.net.{l}.bias"] for l in range(3)]
    beta = pg["sdf2density.beta"].abs() + 1e-4
    seen, orig = {}, ops._field_bwd

    def bits(t):
        return None if t is None else int(t.abs().max().view(torch.int32))

    def spy(lib, xc, wT, beta_c, acts, sdf, albedo, g_sdf, g_sigma, g_albedo, *rest, **kw):
        words = torch.zeros(2, dtype=torch.int32, device=DEV)
        kw["gmax"] = words
        r = orig(lib, xc, wT, beta_c, acts, sdf, albedo, g_sdf, g_sigma, g_albedo, *rest, **kw)
        assert r[5] is words
        seen["first"] = (words.clone().tolist(), bits(r[1]), bits(r[2]))
        small = [None if t is None else t * 2.0 ** -20 for t in (g_sdf, g_sigma, g_albedo)]
        r2 = orig(lib, xc, wT, beta_c, acts, sdf, albedo, *small, *rest, **kw)
        seen["second"] = (words.clone().tolist(), bits(r2[1]), bits(r2[2]))
        return r2

    monkeypatch.setattr(ops, "_field_bwd", spy)
    sdf, sigma, albedo = ops.field_mlp(x, fs, fc if with_color else None, topo, beta, 6, with_color,
                                       ops.prepare_field_operands(Ws + Wc + bs + bc))
    loss = (sdf * ws).sum() + (sigma * wg).sum()
    if with_color:
        loss = loss + (albedo * wc).sum()
    loss.backward()
    torch.cuda.synchronize()
    (w1, s1, c1), (w2, s2, c2) = seen["first"], seen["second"]
    print(f"GRIDF64 gmax with_color={with_color} {mlp} M={M}: words {w1[0]:#x} {w1[1]:#x} tensors {s1:#x} {c1 if c1 is None else hex(c1)}; "
          f"second call tensors {s2:#x} {c2 if c2 is None else hex(c2)} words {w2[0]:#x} {w2[1]:#x}")
    assert s1 > 0 and w1[0] == s1, "max|g_fs| word"
    if with_color:
        assert c1 > 0 and w1[1] == c1, "max|g_fc| word"
        assert 0 < c2 < c1
    else:
        assert c1 is None and w1[1] == 0, "no colour pass: its word stays zero"
    assert 0 < s2 < s1, "the second call's gradients are smaller"
    assert w2 == w1, "a word is only ever raised: the stale maximum of the first call stays"


def test_every_query_starts_from_zeroed_words(monkeypatch):
    """40 consecutive field queries of ONE backward pass (more than one pool of 32 pairs): each is handed a pair of words that
    starts at zero and that no other live query of the pass holds"""
    from morpheus_amd import ops, harness
    model = harness.build_model("b", DEV, None)
    g = torch.Generator().manual_seed(77)
    starts, ptrs, keep, orig = [], [], [], ops._field_bwd

    def spy(*a, **k):
        w = k.get("gmax")
        starts.append(None if w is None else int(w.abs().max()))
        r = orig(*a, **k)
        if w is not None:
            ptrs.append(w.data_ptr())
            keep.append(w)
        return r

    monkeypatch.setattr(ops, "_field_bwd", spy)
    model.zero_grad()
    tot = 0
    for k in range(40):
        x = ((torch.rand(257, 3, generator=g) * 2 - 1) * BOUND).to(DEV)
        sdf, sigma, albedo = model.get_sigma_albedo(x, (torch.randn(257, 2, generator=g) * 0.3).to(DEV))
        tot = tot + (sdf.sum() + 0.01 * sigma.sum() + albedo.sum()) * 2.0 ** -(k % 7)
    tot.backward()
    torch.cuda.synchronize()
    assert len(starts) == 40 and all(s == 0 for s in starts), starts
    assert len(set(ptrs)) == 40
    assert all(int(w[0]) > 0 and int(w[1]) > 0 for w in keep), "every query left its maxima in its own words"
    acc = ops._QueryAccumulator()
    for k in range(40):                                        # the pool alone, its words dirtied as a query's backward leaves them
        w = acc.gmax_words(DEV)
        assert w.dtype == torch.int32 and w.shape == (2,) and not w.any()
        w.fill_(0x7F000000 - k)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_one_non_finite_gradient_among_finite_ones(bad):
    """one upstream gradient entry inf / NaN among 2^18 finite ones -- ordinary input.  What the header promises and nothing more:
    the call returns MH_OK (ops.check raises otherwise), every table entry not among the affected point's 8 x 16 rows is finite,
    and a following call with finite gradients gives the per-level result (nothing leaks through the scratch word)."""
    emb, offs, res = gc.grid_setup()
    M = 1 << 18
    x, grad, ora, t64, cnt = _case("uniform", M)
    p = 12345
    u = (x[p].double() + BOUND) / (2 * BOUND)
    for r in res:                                              # the point is well inside its cell at every level: no doubt about its rows
        f = (u * int(r) - 0.5) % 1.0
        assert bool(((f > 1e-3) & (f < 1 - 1e-3)).all()) and bool(((u > 0.01) & (u < 0.99)).all())
    rows = gc.grid_term_counts(x[p:p + 1], list(map(int, offs)), res, BOUND, 16) > 0
    assert int(rows.sum()) == 128
    dirty = grad.clone()
    dirty[p, 5] = bad
    hip = _hip_table(x, dirty, emb, offs, res, need_dx=True, finite_dx=False)      # (the affected point's own d/dx is not finite)
    others = hip[~rows]
    print(f"GRIDF64 non-finite {bad}: entries outside the point's rows {others.numel()}, non-finite {int((~torch.isfinite(others)).sum())}, "
          f"non-zero {int((others != 0).sum())}; the point's rows non-finite {int((~torch.isfinite(hip[rows])).sum())}")
    assert bool(torch.isfinite(others).all())
    clean = _hip_table(x, grad, emb, offs, res, need_dx=True)
    gc.check_levels(f"after a {bad} gradient, M=2^18", clean, ora, t64, cnt, offs)


# ---- 5. no level switched on, through the C ABI -----------------------------------------------------------------------------
@pytest.mark.parametrize("with_dx", [True, False])
@pytest.mark.parametrize("M", [5000, (1 << 20) + 1])
def test_zero_levels_through_the_c_abi(M, with_dx):
    """mh_grid_encode_bwd_binned with n_levels == 0 (the launchers accept it): all-zero table gradient and d/dx, direct and staged
    size classes"""
    from morpheus_amd import ops, _lib
    lib = _lib.load()
    emb, offs, res = gc.grid_setup()
    x, grad = gc.gen_uniform(M, seed=5)
    x, grad, embg = x.to(DEV).contiguous(), grad.to(DEV).contiguous(), emb.to(DEV)
    o_np, o_p = ops._i32arr(offs)
    r_np, r_p = ops._i32arr(res)
    perm, bstart = ops._bin_points(lib, x, BOUND)
    g_emb = torch.zeros_like(embg)
    acc = torch.empty(embg.numel(), dtype=torch.int64, device=DEV)
    g_x = torch.full((M, 3), 7.0, device=DEV) if with_dx else None
    ops.check(lib.mh_grid_encode_bwd_binned(ops.ptr(grad), ops.ptr(x), ops.ptr(embg), o_p, r_p, ops.ptr(perm), ops.ptr(bstart),
                                            ops.ptr(g_emb), ops.ptr(acc), ops.ptr(g_x), 0, M, 16, 0, BOUND, None, ops.stream()),
              "mh_grid_encode_bwd_binned, n_levels = 0")
    torch.cuda.synchronize()
    assert not g_emb.any()
    if with_dx:
        assert not g_x.any()
