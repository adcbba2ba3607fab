"""GPU: the grid encoder in full (csrc/hashgrid_general.hip) -- every channel count, grid type, alignment and interpolation -- and its
total-variation and weight-decay gradients, held to float64.

The reference operator is CUDA-only and cannot run where these tests run, so no golden comes from it (oracle/hashgrid.py says the
same of its one configuration).  Yardsticks: tests/grid_general_oracle.py -- an fp32 restatement of the cited lines of gridencoder.cu
(pinned bit for bit to oracle/hashgrid.c on the default switches by tests/test_grid_general_host.py) and a float64 evaluation that
takes its cells from it.  Forward, d/dx and the table gradient go through the hash-grid suite's own gate (grid_f64_cases.gate: the
kernel's error against float64 <= max(3 x the restatement's, 2^-22), per level, in relative L2 and in max-norm); total variation and
weight decay are pure sums and go through f64_judge.judge_sum.  No tolerance is made up here.

Tables: L = 6, base 4, desired 32, 2^9 rows at most (two dense levels, four hashed or tiled ones); L = 1 and L = 16 on the default
16..128 pyramid.  Points: 1, 63, 64, 65 and 257 rows of one seeded set (a wave, a wave +- 1, more than one block) followed by fixed
rows -- u = 0 and u = 1 exactly, the half-texel clamp band, cell vertices, three rows outside the box."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

from morpheus_amd import ops, synth
from morpheus_amd.model import GridEncoder
from tests import grid_general_oracle as gg
from tests.f64_judge import judge_sum
from tests.grid_f64_cases import gate

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = np.float32, np.float64
BOUND = 1.0
SMALL = dict(num_levels=6, base_resolution=4, desired_resolution=32, log2_hashmap_size=9)
SIZES = (1, 63, 64, 65, 257)
COMBOS = list(itertools.product(ops.GRID_CHANNELS, ops.GRID_TYPES.values(), (0, 1), ops.GRID_INTERPS.values()))

FIXED = np.array([
    [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [-1.0, 1.0, 0.3],                   # u = 0 and u = 1 exactly
    [-1.0 + 1.0 / 32, 0.1, 1.0 - 1.0 / 64],                                  # inside the half-texel clamp band
    [-0.75, -0.25, 0.25], [0.75, -0.75, 0.25],                               # u = (k + 0.5) / 4: vertices of level 0
    [-1.0 + 2 * 6.5 / 32, -1.0 + 2 * 17.5 / 32, -1.0 + 2 * 31.5 / 32],       # u = (k + 0.5) / 32: vertices of level 5
    [-0.5, 0.0, 0.5],                                                        # u = k / 4
    [1.5, 0.0, 0.0], [0.2, -3.0, 0.1], [0.0, 0.0, 1.0 + 2.0 ** -22],           # outside the box (the last by two ulps: u = 1 + 2^-23)
], dtype=F32)
N_OUTSIDE = 3


@functools.lru_cache(maxsize=None)
def points(n):
    """the first n rows of the seeded set, then the fixed rows"""
    return np.concatenate([synth.hash_tensor((257, 3), 4242, 1.0).numpy()[:n], FIXED])


@functools.lru_cache(maxsize=None)
def table(kind, C):
    """-> (emb [rows, C] numpy, offsets, resolutions)"""
    if kind == "small":
        enc = GridEncoder(level_dim=C, **SMALL)
        offs, res = enc._offsets_np, enc._res_np
    else:
        offs, s = synth.grid_offsets()
        res = ops.level_resolutions(16, s, 16)
        if kind == "one":
            offs, res = offs[:2], res[:1]
    return synth.hash_tensor((int(offs[-1]), C), 9100 + C, 0.1).numpy(), offs, res


def upstream(n_rows, width):
    return synth.hash_tensor((n_rows, width), 515, 1.0).numpy()


def hip_run(x, emb, offs, res, grad, max_level, C, gridtype, align, interp):
    xg = torch.from_numpy(x).to(DEV).requires_grad_(True)
    e = torch.from_numpy(emb).to(DEV).requires_grad_(True)
    out = ops.grid_encode_general(xg, e, offs, res, BOUND, max_level, C, gridtype, bool(align), interp)
    out.backward(torch.from_numpy(grad).to(DEV))
    return out.detach().cpu().numpy(), xg.grad.cpu().numpy(), e.grad.cpu().numpy()


def norms(t, t64):
    """(relative L2, relative max) of t against float64; where float64 is all zero: 0 if t is too, inf otherwise"""
    d = np.abs(t.astype(F64) - t64)
    n, m = float(np.linalg.norm(t64)), float(np.abs(t64).max()) if t64.size else 0.0
    dn, dm = float(np.linalg.norm(d)), float(d.max()) if d.size else 0.0
    return (dn / n if n > 0 else (0.0 if dn == 0 else math.inf)), (dm / m if m > 0 else (0.0 if dm == 0 else math.inf))


def judge_blocks(what, hip, ref32, f64, blocks):
    """the gate on every block (a level's columns or rows; one block for d/dx): every figure is printed before anything is asserted"""
    bad = []
    for name, sl in blocks:
        h, o = norms(hip[sl], f64[sl]), norms(ref32[sl], f64[sl])
        print(f"GRIDGEN {what} {name} l2 hip {h[0]:.3e} restatement {o[0]:.3e} | mx hip {h[1]:.3e} restatement {o[1]:.3e}")
        bad += [(name, k, a, b) for k, a, b in (("l2", h[0], o[0]), ("mx", h[1], o[1])) if not gate(a, b)]
    assert not bad, f"{what}: (block, metric, hip, restatement) beyond max(3 x restatement, 2^-22): {bad}"


def check_case(what, kind, n, max_level, C, gridtype, align, interp):
    emb, offs, res = table(kind, C)
    L = len(res)
    x = points(n)
    grad = upstream(len(x), L * C)
    n_levels = ops.effective_levels(max_level, L)
    out, g_x, g_emb = hip_run(x, emb, offs, res, grad, max_level, C, gridtype, align, interp)
    case = gg.Case(x, emb, offs, res, BOUND, n_levels, C, gridtype, align, interp)
    assert int((~case.inb).sum()) == N_OUTSIDE and not case.inb[-N_OUTSIDE:].any()
    assert not out[~case.inb].any() and not g_x[~case.inb].any(), f"{what}: rows outside the box must be exactly zero"
    cols = [(f"level {l}", (slice(None), slice(l * C, (l + 1) * C))) for l in range(L)]
    rows = [(f"level {l}", slice(int(offs[l]), int(offs[l + 1]))) for l in range(L)]
    judge_blocks(f"{what} forward", out, case.forward(F32), case.forward(F64), cols)
    judge_blocks(f"{what} d/dx", g_x, case.grad_x(grad, F32), case.grad_x(grad, F64), [("all", slice(None))])
    judge_blocks(f"{what} table gradient", g_emb, case.grad_emb(grad, F32), case.grad_emb(grad, F64), rows)
    assert not g_emb[case.term_counts() == 0].any(), f"{what}: a row without a term must stay exactly zero"


@pytest.mark.parametrize("C,gridtype,align,interp", COMBOS)
def test_forward_and_gradients_against_float64(C, gridtype, align, interp):
    """the small table at every size and at max_level None and 0.5 (3 of 6 levels; the others' columns and rows exactly zero)"""
    for max_level in (None, 0.5):
        for n in SIZES:
            check_case(f"C={C} type={gridtype} align={align} interp={interp} max_level={max_level} n={n}", "small", n, max_level, C,
                       gridtype, align, interp)


@pytest.mark.parametrize("kind", ("one", "default"))
@pytest.mark.parametrize("C,gridtype,align,interp", [c for c in COMBOS if c[0] in (1, 8) or c[1:] == (0, 0, 0)])
def test_one_and_sixteen_levels_of_the_default_pyramid(kind, C, gridtype, align, interp):
    """L = 1 and L = 16 (tables of 4096 and 419 640 rows) at 257 + fixed points"""
    check_case(f"{kind} C={C} type={gridtype} align={align} interp={interp}", kind, 257, None, C, gridtype, align, interp)


def test_bad_arguments_are_refused_and_empty_calls_launch_nothing():
    emb, offs, res = table("small", 2)
    e = torch.from_numpy(emb).to(DEV)
    out = ops.grid_encode_general(torch.zeros(0, 3, device=DEV), e, offs, res, BOUND)
    assert out.shape == (0, 12)
    with pytest.raises(ValueError):
        ops.grid_encode_general(torch.zeros(4, 3, device=DEV), e, offs, res, BOUND, None, 4)
    with pytest.raises(ValueError):
        ops.grid_encode_general(torch.zeros(4, 3, device=DEV), e, offs, res, BOUND, None, 2, "dense")
    from morpheus_amd._lib import MorpheusHipError
    with pytest.raises(MorpheusHipError):
        ops.grid_encode_general(torch.zeros(4, 3, device=DEV), e, offs, res, -1.0)


# ---- dispatch ---------------------------------------------------------------------------------------------------------------------
def test_default_switches_keep_the_specialised_kernels_bit_for_bit():
    torch.manual_seed(3)
    enc = GridEncoder().to(DEV)
    with torch.no_grad():
        enc.embeddings.copy_(synth.hash_tensor(tuple(enc.embeddings.shape), 9001, 0.1))
    x = torch.from_numpy(points(257)).to(DEV)
    grad = torch.from_numpy(upstream(x.shape[0], 32)).to(DEV)
    for max_level in (None, 0.5):
        xa = x.clone().requires_grad_(True)
        enc.embeddings.grad = None
        ops.TIMER.reset(True)
        a = enc(xa, bound=BOUND, max_level=max_level)
        a.backward(grad)
        torch.cuda.synchronize()
        names = set(ops.TIMER.summary())
        ops.TIMER.reset(False)
        assert names and not any(n.startswith("mh_grid_general") for n in names), names
        xb = x.clone().requires_grad_(True)
        e = enc.embeddings.detach().clone().requires_grad_(True)
        b = ops.grid_encode(xb, e, enc._offsets_np, enc._res_np, BOUND, max_level)
        b.backward(grad)
        assert torch.equal(a, b) and torch.equal(xa.grad, xb.grad) and torch.equal(enc.embeddings.grad, e.grad)


def test_eight_levels_with_an_input_gradient():
    """the specialised backward refuses d/dx at L != 16; the module now routes that call to the general path, and the same module
    without an input gradient stays on the specialised kernels with the same features"""
    enc = GridEncoder(num_levels=8).to(DEV)
    x = torch.from_numpy(points(65)).to(DEV)
    grad = torch.from_numpy(upstream(x.shape[0], 16)).to(DEV)
    xg = x.clone().requires_grad_(True)
    ops.TIMER.reset(True)
    out = enc(xg, bound=BOUND)
    out.backward(grad)
    torch.cuda.synchronize()
    names = set(ops.TIMER.summary())
    ops.TIMER.reset(False)
    assert {"mh_grid_general_fwd", "mh_grid_general_bwd"} <= names
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all()) and bool(xg.grad.abs().sum() > 0)
    with torch.no_grad():
        plain = enc(x, bound=BOUND)
    assert torch.equal(plain, out.detach())
    case = gg.Case(x.cpu().numpy(), enc.embeddings.detach().cpu().numpy(), enc._offsets_np, enc._res_np, BOUND, 8, 2)
    g = grad.cpu().numpy()
    judge_blocks("L=8 d/dx", xg.grad.cpu().numpy(), case.grad_x(g, F32), case.grad_x(g, F64), [("all", slice(None))])


@pytest.mark.parametrize("C", (1, 4))
def test_upstream_gradient_starting_one_float_into_a_buffer(C):
    """a contiguous upstream gradient whose storage starts 4 bytes into an allocation (what autograd hands over for one half of a
    `cat`): the maximum pre-pass and the row loads may make no 16-byte access to it, so x.grad and the table gradient equal, bit
    for bit, those of the same values in a tensor of their own"""
    emb, offs, res = table("one", C)
    assert emb.shape[0] == 4096
    x = points(65)
    values = torch.from_numpy(upstream(len(x), C)).to(DEV)
    buf = torch.zeros(values.numel() + 1, device=DEV)
    buf[1:] = values.reshape(-1)
    view = buf[1:].view_as(values)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 and buf.data_ptr() % 16 == 0

    def run(grad):
        xg = torch.from_numpy(x).to(DEV).requires_grad_(True)
        e = torch.from_numpy(emb).to(DEV).requires_grad_(True)
        ops.grid_encode_general(xg, e, offs, res, BOUND, None, C).backward(grad)
        return xg.grad, e.grad

    (gx_view, ge_view), (gx_own, ge_own) = run(view), run(values.clone())
    assert bool(ge_own.abs().sum() > 0) and bool(gx_own.abs().sum() > 0)
    assert torch.equal(gx_view, gx_own) and torch.equal(ge_view, ge_own)


# ---- total variation and weight decay ---------------------------------------------------------------------------------------------
TV_WEIGHT = 1e-3


def tv_inputs(C, normalized):
    emb, offs, res = table("small", C)
    x = points(257)
    if normalized:
        x = ((x + F32(1)) / F32(2)).astype(F32)
    return emb, offs, res, x


def tv_hip(emb, offs, res, x, C, gridtype, align, normalized, into=None):
    e = torch.from_numpy(emb).to(DEV)
    grad = torch.zeros_like(e) if into is None else into
    ops.grid_grad_tv(torch.from_numpy(x).to(DEV), e, grad, offs, res, TV_WEIGHT, BOUND, C, gridtype, bool(align), normalized)
    return grad


@pytest.mark.parametrize("normalized", (False, True))
@pytest.mark.parametrize("C,gridtype,align", list(itertools.product(ops.GRID_CHANNELS, (0, 1), (0, 1))))
def test_total_variation_against_float64(C, gridtype, align, normalized):
    """judge_sum per table entry: |hip - f64| <= (16 + n) 2^-24 x the float64 sum of the addends' absolute terms + n x half a step of
    the fixed-point grid (grid_general_oracle: where the 16 comes from, and the quantum, sized from |weight| sqrt(6) / 6 >= any addend);
    rows no point reaches stay exactly zero; two runs are bit-identical; a pre-filled buffer receives exactly the same sums."""
    emb, offs, res, x = tv_inputs(C, normalized)
    case = gg.Case(x, emb, offs, res, BOUND, 6, C, gridtype, align, 0, normalized)
    t64, absum, cnt = case.tv(TV_WEIGHT, F64)
    assert np.abs(t64).max() <= abs(TV_WEIGHT) * math.sqrt(6) / 6 * cnt.max() * (1 + 1e-12)
    first = tv_hip(emb, offs, res, x, C, gridtype, align, normalized)
    n = torch.from_numpy(cnt).double()[:, None].expand(-1, C)
    rec = judge_sum(first, t64, absum, gg.TV_CHAIN_ROUNDINGS + n.reshape(-1), f"tv C={C} type={gridtype} align={align}",
                    extra=n.reshape(-1) * gg.tv_fixed_point_quantum(TV_WEIGHT, len(x)))
    print(f"GRIDGEN tv C={C} type={gridtype} align={align} normalized={normalized} worst {rec['worst_hip']:.3e} ratio {rec['ratio']:.3f}")
    assert not first.cpu().numpy()[cnt == 0].any() and bool(first.abs().sum() > 0)
    assert torch.equal(first, tv_hip(emb, offs, res, x, C, gridtype, align, normalized))
    fill = synth.hash_tensor(emb.shape, 77, 1e-3).to(DEV)
    fill[0, 0] = -0.0
    got = tv_hip(emb, offs, res, x, C, gridtype, align, normalized, into=fill.clone())
    assert torch.equal(got, fill + first)
    untouched = torch.from_numpy(cnt == 0).to(DEV)
    assert torch.equal(got[untouched].view(torch.int32), fill[untouched].view(torch.int32)), "rows no point touches stay bit-identical"


@pytest.mark.parametrize("C", ops.GRID_CHANNELS)
def test_weight_decay_against_float64(C):
    """one product, one quotient, one add into the buffer: judge_sum with 3 roundings of |addend| + |what the buffer held|"""
    emb, offs, res = table("small", C)
    e = torch.from_numpy(emb).to(DEV)
    case = gg.Case(np.zeros((1, 3), F32), emb, offs, res, BOUND, 6, C)
    w64 = case.wd(0.1, F64)
    first = ops.grid_grad_wd(e, torch.zeros_like(e), offs, 0.1, C)
    judge_sum(first, w64, np.abs(w64), 3, f"wd C={C}")
    assert torch.equal(first, ops.grid_grad_wd(e, torch.zeros_like(e), offs, 0.1, C))
    fill = synth.hash_tensor(emb.shape, 78, 1e-2).to(DEV)
    got = ops.grid_grad_wd(e, fill.clone(), offs, 0.1, C)
    assert torch.equal(got, fill + first)
    judge_sum(got, fill.cpu().double().numpy() + w64, np.abs(w64) + fill.cpu().abs().double().numpy(), 3, f"wd into a filled buffer C={C}")


@pytest.mark.parametrize("kw", (dict(), dict(level_dim=4, gridtype="tiled", align_corners=True, interpolation="smoothstep", **SMALL)))
def test_regularisers_add_into_a_flat_adam_bucket_view(kw):
    """the module's methods on the default configuration and on a general one, with the table's parameter and gradient living in
    FlatAdam's flat buffers one element off any vector alignment: the sums land in the bucket's view, next to what backward left
    there, and nothing else in the bucket moves"""
    from morpheus_amd.optim import FlatAdam
    torch.manual_seed(5)
    enc = GridEncoder(**kw).to(DEV)
    with torch.no_grad():
        enc.embeddings.copy_(synth.hash_tensor(tuple(enc.embeddings.shape), 31, 0.1))
    lead, tail = torch.nn.Parameter(torch.ones(1, device=DEV)), torch.nn.Parameter(torch.ones(3, device=DEV))
    opt = FlatAdam([lead, enc.embeddings, tail], lr=1e-3)
    assert enc.embeddings.data_ptr() % 8 == 4 and enc.embeddings.grad.data_ptr() == opt.bucket.flat.data_ptr() + 4
    C, offs, res = enc.level_dim, enc._offsets_np, enc._res_np
    x = torch.from_numpy(points(257)).to(DEV)
    opt.zero_grad()
    if kw:
        enc(x.clone().requires_grad_(True), bound=BOUND).square().sum().backward()      # the general kernels' element-wise row access
    else:
        enc.embeddings.grad = synth.hash_tensor(tuple(enc.embeddings.shape), 32, 1e-3).to(DEV)     # what a backward would leave
    opt.bucket.collect()
    view = enc.embeddings.grad
    assert view.data_ptr() == opt.bucket.flat.data_ptr() + 4
    before = opt.bucket.flat.clone()
    enc.grad_total_variation(weight=TV_WEIGHT, inputs=x, bound=BOUND)
    enc.grad_weight_decay(weight=0.1)
    e = enc.embeddings.detach().clone()             # an aligned copy of the same table
    tv = ops.grid_grad_tv(x, e, torch.zeros_like(e), offs, res, TV_WEIGHT, BOUND, C, enc.gridtype_id, enc.align_corners)
    want = ops.grid_grad_wd(e, before[1:1 + e.numel()].view_as(e) + tv, offs, 0.1, C)
    assert torch.equal(view, want)
    assert torch.equal(opt.bucket.flat[:1], before[:1]) and torch.equal(opt.bucket.flat[1 + e.numel():], before[1 + e.numel():])
    enc.grad_total_variation(weight=TV_WEIGHT, B=1000)                          # the module's own random points: runs, stays finite
    assert bool(torch.isfinite(opt.bucket.flat).all())
    opt.step()
