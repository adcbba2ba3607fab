"""Inputs, yardsticks and gates of the hash-grid table-gradient tests (tests/test_gpu_grid_f64.py on the GPU, the "reference stays
inside the caps" tests of tests/test_oracle_hashgrid.py on the CPU) -- test infrastructure, no test lives here.

Every generator is seeded (torch.Generator) and takes its size, so that the CPU tests run the very same inputs at a reduced
size through the fp32 C restatement (oracle/hashgrid.c) and the float64 helper (oracle/hashgrid_f64.py).

The gate: per level (row block offsets[l]:offsets[l+1]), for the HIP result and for the fp32 C restatement, both against float64,
    l2 = ||x - f64||_2 / ||f64||_2        mx = max|x - f64| / max|f64|
and hip <= max(3 x oracle_fp32, 2^-22) for both.  3 is the project's convention for gates derived from the reference's own error;
2^-22 is four ulps of the final fp32 conversion, there only so that a level where the fp32 restatement happens to be exact cannot
fail the kernel for its one rounding."""
import math

import numpy as np
import torch

from morpheus_amd import synth
from oracle.hashgrid import effective_levels, level_resolutions, oracle_grid_encode
from oracle.hashgrid_f64 import grid_table_grad_f64, grid_term_counts
from tests.f64_judge import within

BOUND = float(np.float32(1.01))       # the same number in fp32 and in double: u = (x + bound) / (2 bound) differs by round-off only
FACTOR, FLOOR = 3.0, 2.0 ** -22
FX_BITS = 40                          # bits of the fixed-point grid below G
# Share of table entries for which the fp32 C restatement, run on the same points with every coordinate moved by one fp32 ulp,
# breaks |moved - f64| <= 2^-23 |f64| + 3 e (e: the unmoved restatement's largest error in the entry's level and magnitude bucket) on
# the graded input of 2^20 + 1 points: the rate at which an equally valid fp32 evaluation of u * res - 0.5 puts a point into the
# neighbouring cell or moves a small entry by more than the bucket's worst.  Measured by
# test_graded_input_exception_share_of_the_reference (which asserts that a fresh measurement does not exceed it); the GPU test
# allows twice this share of counted exceptions and nothing beyond.
MOVED_EXCEPTIONS_MEASURED = 42          # of 839 280 entries
MOVED_EXCEPTION_SHARE = MOVED_EXCEPTIONS_MEASURED / 839280.0      # 5.0e-5


def grid_setup(scale=0.1):
    offs, s = synth.grid_offsets()
    emb = synth.hash_tensor((int(offs[-1]), 2), 9001, scale)
    return emb, offs, level_resolutions(16, s, 16)


def acc_shift_of(M):
    """headroom bits of a call of M points: 8 M terms of at most 2^(40 - shift) stay inside +-2^62"""
    s = 0
    while s < 40 and M * 8.0 > 2.0 ** (62 - FX_BITS + s):
        s += 1
    return s


def quantum(grad, M):
    """(G, q): G = the power of two strictly above max|grad| (never below 2^-67), q = G 2^-(40 - acc_shift), recomputed from the
    inputs: the step of the grid every term w * g is rounded onto."""
    m = float(grad.abs().max())
    e = max(math.floor(math.log2(m)) + 1, 60 - 127) if m > 0 else 60 - 127
    G = 2.0 ** e
    return G, G * 2.0 ** -(FX_BITS - acc_shift_of(M))


# ---- input generators: -> x [M,3] fp32, grad [M,32] fp32 ----------------------------------------------------------------------
def gen_uniform(M, seed=31):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(M, 3, generator=g) * 2 - 1) * BOUND, torch.randn(M, 32, generator=g)


def gen_rays(n_r=8192, S=128, seed=21):
    """the converging-ray cloud of test_grid_large_batch_gradients: two thirds along rays through the box, dense near the near
    plane (hot bricks split into many work items sharing rows), one third uniform"""
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor([0.0, 0.0, 2.2]) + 0.05 * torch.randn(n_r, 3, generator=g)
    d = torch.nn.functional.normalize(torch.cat([torch.randn(n_r, 2, generator=g) * 0.35, -torch.ones(n_r, 1)], 1), dim=1)
    ts = 1.2 + 2.0 * (torch.arange(S).float()[None] + torch.rand(n_r, S, generator=g)) / S
    rays = (o[:, None] + d[:, None] * ts[..., None]).reshape(-1, 3).clamp(-1.0, 1.0)
    x = torch.cat([rays, torch.rand(n_r * S // 2, 3, generator=g) * 2 - 1])
    return x, torch.randn(x.shape[0], 32, generator=g)


def gen_faces_outside(M, seed=41):
    """a third ON the box's faces (one coordinate exactly +-bound: u = 0 or 1 in fp32 and in double), a third within one cell of
    the finest level (2 bound / 128) of a face, a third outside by at least 2^-18 of the bound (clear of the fp32 rounding of
    x + bound, so that every implementation agrees on who is outside)"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(M, 3, generator=g) * 2 - 1) * BOUND
    ax = torch.randint(0, 3, (M,), generator=g)
    sgn = (torch.randint(0, 2, (M,), generator=g) * 2 - 1).float()
    t = torch.rand(M, generator=g)
    third = M // 3
    v = torch.empty(M)
    v[:third] = BOUND
    v[third:2 * third] = BOUND - t[third:2 * third] * (2 * BOUND / 128)
    v[2 * third:] = BOUND * (1 + 2.0 ** -18) + t[2 * third:] * 0.3
    x[torch.arange(M), ax] = sgn * v
    return x, torch.randn(M, 32, generator=g)


def gen_graded(M, seed=51):
    """uniform points, upstream gradient randn * 2^(-60 (z + 1) / 2) with z the third coordinate: magnitude falls by 2^-60 across the
    box, whole regions of the dense levels see only tiny gradients"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(M, 3, generator=g) * 2 - 1
    return x, torch.randn(M, 32, generator=g) * torch.exp2(-30.0 * (x[:, 2:3] + 1))


ONE_CELL_U = (37.0 / 128, 90.0 / 128, 5.0 / 128)     # multiples of 2^-7: u res - 0.5, f and the corner weights (<= 21 bits) are exact
ONE_CELL_G0 = float(np.float32(0.7))
ONE_CELL_BOUND = 1.0                                 # x = 2 u - 1 and back: exact


def one_cell_expected(M, emb_rows, offs, res):
    """The closed form of M copies of one point with every upstream gradient +g0, bound 1: -> (expected float64 [rows], count int64
    [rows]).  Every touched row holds n w g0 with n = M; the fixed-point sum is exact up to ONE rounding per term (w g0 onto the
    grid q, ties to even as the kernel's fused multiply-add does), so the row is M * rint(w g0 / q) * q before its single
    conversion to fp32."""
    x1 = torch.tensor([[2 * u - 1 for u in ONE_CELL_U]], dtype=torch.float32)
    cnt = grid_term_counts(x1, offs.tolist(), res, ONE_CELL_BOUND, 16)
    assert int(cnt.max()) == 1 and int(cnt.sum()) == 8 * 16, "the eight corners of every level are distinct rows"
    w = grid_table_grad_f64(x1, torch.ones(1, 32), offs.tolist(), res, ONE_CELL_BOUND, 16)[:, 0]     # one term per row: w itself
    _, q = quantum(torch.tensor([ONE_CELL_G0]), M)
    t = w.numpy() * ONE_CELL_G0 / q                  # exact in double: 21 x 24 bits times a power of two
    return torch.from_numpy(np.rint(t) * M * q), cnt * M


# ---- yardsticks ------------------------------------------------------------------------------------------------------------
def oracle_tables(x, grad, emb, offs, res, bound, max_level=None, f64=True):
    """-> (fp32 C restatement's table gradient, float64 table gradient or None, term counts) on the same fp32 inputs"""
    e = emb.clone().requires_grad_(True)
    out = oracle_grid_encode(x, e, torch.from_numpy(np.asarray(offs)), torch.from_numpy(np.asarray(res)), bound, max_level)
    out.backward(grad)
    n_levels = effective_levels(max_level, 16)
    t64 = grid_table_grad_f64(x, grad, list(map(int, offs)), res, bound, n_levels) if f64 else None
    return e.grad.detach(), t64, grid_term_counts(x, list(map(int, offs)), res, bound, n_levels)


def level_metrics(t, t64, offs):
    """-> (l2 [16], mx [16]) of t against float64, each over the level's own block; a level float64 leaves at zero: 0 if t is zero
    there too, inf otherwise"""
    d = (t.double().cpu() - t64).abs()
    l2, mx = [], []
    for l in range(16):
        a, b = int(offs[l]), int(offs[l + 1])
        n, m = float(t64[a:b].norm()), float(t64[a:b].abs().max())
        dn, dm = float(d[a:b].norm()), float(d[a:b].max())
        l2.append(dn / n if n > 0 else (0.0 if dn == 0 else math.inf))
        mx.append(dm / m if m > 0 else (0.0 if dm == 0 else math.inf))
    return l2, mx


def gate(hip, ora):
    return within(hip, ora, FACTOR, FLOOR)


def check_levels(what, hip, ora, t64, cnt, offs, log=print):
    """the section-2 gate of one case: per-level l2 and mx of HIP against 3 x the fp32 restatement's (floor 2^-22), and the zero
    pattern -- a row no term lands on is exactly 0 in the HIP result.  Every figure is printed before anything is asserted."""
    hl2, hmx = level_metrics(hip, t64, offs)
    ol2, omx = level_metrics(ora, t64, offs)
    for l in range(16):
        log(f"GRIDF64 {what} level {l:2d} l2 hip {hl2[l]:.3e} oracle {ol2[l]:.3e} | mx hip {hmx[l]:.3e} oracle {omx[l]:.3e}")
    untouched = (cnt == 0)
    stray = int((hip.cpu()[untouched] != 0).sum())
    log(f"GRIDF64 {what} untouched rows {int(untouched.sum())} non-zero among them {stray}")
    bad = [(l, k, h, o) for l in range(16) for k, h, o in (("l2", hl2[l], ol2[l]), ("mx", hmx[l], omx[l])) if not gate(h, o)]
    assert not bad, f"{what}: (level, metric, hip, oracle) beyond max(3 x oracle, 2^-22): {bad}"
    assert stray == 0, f"{what}: {stray} rows without a term are not exactly zero"
    return hl2, hmx, ol2, omx


def buckets(t64, offs):
    """int64 [rows, C]: level * 1024 + (floor(log2|f64| / 8) + 512), zeros of a level in its slot 0"""
    a = t64.abs()
    b = torch.where(a > 0, torch.floor(torch.log2(a.clamp(min=1e-300)) / 8) + 512, torch.zeros_like(a)).long()
    lev = torch.bucketize(torch.arange(t64.shape[0]), torch.as_tensor(np.asarray(offs)[1:-1], dtype=torch.long), right=True)
    return lev[:, None] * 1024 + b


def bucket_max(err, bk):
    """e of every entry: the largest err among the entries of its bucket"""
    flat, idx = err.reshape(-1), bk.reshape(-1)
    m = torch.zeros(16 * 1024, dtype=err.dtype).scatter_reduce_(0, idx, flat, "amax", include_self=True)
    return m[idx].reshape(err.shape)


def moved_exception_share(x, grad, emb, offs, res, ora, t64, bk):
    """the share of entries for which the fp32 restatement on points moved by one fp32 ulp per coordinate breaks
    |moved - f64| <= 2^-23 |f64| + 3 e, e = the unmoved restatement's largest error in the entry's level and bucket"""
    g = torch.Generator().manual_seed(7)
    up = torch.randint(0, 2, x.shape, generator=g).bool()
    xm = torch.where(up, torch.nextafter(x, torch.full_like(x, 4.0)), torch.nextafter(x, torch.full_like(x, -4.0)))
    moved, _, _ = oracle_tables(xm, grad, emb, offs, res, BOUND, f64=False)
    e = bucket_max((ora.double() - t64).abs(), bk)
    broke = (moved.double() - t64).abs() > 2.0 ** -23 * t64.abs() + 3 * e
    return float(broke.double().mean()), int(broke.sum())


def graded_checks(hip, ora, t64, cnt, grad, M, offs, log=print):
    """section 3 on one result `hip` [rows, C] float64 (see test_graded_gradients_dynamic_range): prints the per-level report and
    every bucket's figures -> (buckets checked, buckets beyond the gate, entries beyond the per-entry bound, entries allowed)"""
    G, q = quantum(grad, M)
    n = cnt.double()[:, None].expand_as(t64)
    bk = buckets(t64, offs)
    a64 = t64.abs()
    fine = a64 >= 2.0 ** 20 * n * q
    gmaxf = float(grad.abs().max())
    # reported
    lev_of = bk // 1024
    for l in range(16):
        m = lev_of == l
        nz = m & (a64 > 0)
        lost = nz & (hip == 0)
        alive = nz & (hip != 0)
        small = float(a64[alive].min()) / gmaxf if bool(alive.any()) else float("nan")
        log(f"GRIDF64 graded level {l:2d} non-zero in f64 {int(nz.sum())} of {int(m.sum())}, zero in hip {int(lost.sum())} "
              f"({float(lost.sum()) / max(int(nz.sum()), 1):.4f}), below q/2 in f64 {int((nz & (a64 < q / 2)).sum())}, "
              f"smallest surviving |f64| / max|grad| {small:.3e}")
    # buckets held to their own scale
    bad, n_checked = [], 0
    for b in torch.unique(bk).tolist():
        m = bk == b
        if b % 1024 == 0 or int(m.sum()) < 64 or not bool(fine[m].all()):
            continue
        n_checked += 1
        ref, dh, do = t64[m], (hip[m] - t64[m]).abs(), (ora.double()[m] - t64[m]).abs()
        hl2, ol2 = float(dh.norm() / ref.norm()), float(do.norm() / ref.norm())
        hmx, omx = float(dh.max() / ref.abs().max()), float(do.max() / ref.abs().max())
        log(f"GRIDF64 graded bucket level {b // 1024:2d} 2^{8 * (b % 1024 - 512):4d} n {int(m.sum()):6d} l2 hip {hl2:.3e} oracle {ol2:.3e}"
              f" | mx hip {hmx:.3e} oracle {omx:.3e}")
        if not (gate(hl2, ol2) and gate(hmx, omx)):
            bad.append((b // 1024, 8 * (b % 1024 - 512), hl2, ol2, hmx, omx))
    # every entry
    e = bucket_max((ora.double() - t64).abs(), bk)
    broke = (hip - t64).abs() > n * q / 2 + 2.0 ** -23 * a64 + 3 * e
    allowed = int(2 * MOVED_EXCEPTION_SHARE * t64.numel())
    log(f"GRIDF64 graded G 2^{int(np.log2(G))} q 2^{int(np.log2(q))} buckets checked {n_checked}; entries beyond the bound "
          f"{int(broke.sum())} of {t64.numel()} (share {float(broke.double().mean()):.3e}, cap {2 * MOVED_EXCEPTION_SHARE:.3e} = {allowed})")
    return n_checked, bad, int(broke.sum()), allowed
