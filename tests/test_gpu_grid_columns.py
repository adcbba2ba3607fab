"""The staged hash-grid backward keeps a brick's sums in per-level COLUMNS of LDS (csrc/hashgrid.hip:brick_layout); the direct form
keeps them end to end.  The sums are exact integers in both, so the two forms must give the same bits: every case runs the same
inputs through the staged call (mh_grid_stage_min_points(0)) and through the direct one (1 << 40) and compares the table
gradient and d/dx with torch.equal.  The cases sit where a layout can go wrong: the brick at the box's upper corner (border
clamps, slots past the last vertex), a work item of one point, the 96-point threshold between staging and gathering, a
lattice that reaches every vertex of a brick, points on brick faces, points outside the box, and fewer levels switched on."""
import numpy as np
import pytest
import torch

from tests import grid_f64_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = gc.BOUND
_setup = {}


def _grid():
    if not _setup:
        emb, offs, res = gc.grid_setup()
        _setup["g"] = (emb.to(DEV), np.ascontiguousarray(offs, np.int32), np.ascontiguousarray(res, np.int32))
    return _setup["g"]


def _u_to_x(u, bound=BOUND):
    return (u * (2.0 * bound) - bound).float()


def _in_brick(n, brick, seed, lo=0.0, hi=1.0):
    """n points with u uniform inside brick (bx, by, bz) of the 16^3"""
    g = torch.Generator().manual_seed(seed)
    t = lo + (hi - lo) * torch.rand(n, 3, generator=g, dtype=torch.float64)
    return _u_to_x((torch.tensor(brick, dtype=torch.float64) + t) / 16.0)


def _grad(n, seed):
    return torch.randn(n, 32, generator=torch.Generator().manual_seed(seed))


def _case_corner_2049():
    x = _in_brick(2049, (15, 15, 15), 1)
    x[0] = BOUND                        # u = 1 exactly on every axis
    return x, _grad(2049, 2), BOUND, 16


def _case_interior(n):
    return lambda: (_in_brick(n, (7, 8, 5), 3 + n, 0.01, 0.99), _grad(n, 4 + n), BOUND, 16)


def _case_lattice():
    t = (torch.arange(11, dtype=torch.float64) + 0.5) / 11.0
    u = (torch.tensor([7.0, 7.0, 7.0], dtype=torch.float64) + torch.stack(torch.meshgrid(t, t, t, indexing="ij"), -1).reshape(-1, 3)) / 16.0
    return _u_to_x(u), _grad(u.shape[0], 5), BOUND, 16


def _case_faces():
    # bound 1: x = i / 8 - 1 and u = (x + 1) / 2 = i / 16 are exact in fp32, 0 and 1 included
    t = torch.arange(17, dtype=torch.float64) / 16.0
    u = torch.stack(torch.meshgrid(t, t, t, indexing="ij"), -1).reshape(-1, 3)
    return _u_to_x(u, 1.0), _grad(u.shape[0], 6), 1.0, 16


def _case_outside_and_nan():
    g = torch.Generator().manual_seed(7)
    x = (torch.rand(3000, 3, generator=g) * 2 - 1) * (1.2 * BOUND)
    x[::500] = _in_brick(6, (3, 12, 9), 8)          # some surely inside, the rest in or out
    x[17, 1] = float("nan")
    assert int(((x.abs() > BOUND).any(1)).sum()) > 100
    return x, _grad(3000, 9), BOUND, 16


def _case_levels(n_levels):
    return lambda: (gc.gen_uniform(5000, seed=40 + n_levels)[0], _grad(5000, 41 + n_levels), BOUND, n_levels)


CASES = {"corner_2049": _case_corner_2049, "interior_96": _case_interior(96), "interior_95": _case_interior(95),
         "lattice_11": _case_lattice, "brick_faces": _case_faces, "outside_and_nan": _case_outside_and_nan,
         "levels_1": _case_levels(1), "levels_8": _case_levels(8)}


def _run(lib, knob, x, grad, bound, n_levels, accumulate):
    """bin and run the d/dx backward with the staging threshold `knob`; -> (table gradient, d/dx, work items of the launch)"""
    from morpheus_amd import ops
    emb, o_np, r_np = _grid()
    M = x.shape[0]
    lib.mh_grid_stage_min_points(knob)
    ws = torch.empty(lib.mh_grid_bin_workspace_ints(), dtype=torch.int32, device=DEV)
    perm = torch.empty(M, dtype=torch.int32, device=DEV)
    bstart = torch.zeros(lib.mh_grid_bin_index_ints(), dtype=torch.int32, device=DEV)
    ops.check(lib.mh_grid_bin_points(ops.ptr(x), M, bound, ops.ptr(ws), ops.ptr(perm), ops.ptr(bstart), ops.stream()), "mh_grid_bin_points")
    g_emb = torch.zeros_like(emb)
    acc = torch.empty(emb.numel(), dtype=torch.int64, device=DEV)
    g_x = (torch.arange(M * 3, device=DEV, dtype=torch.float32).reshape(M, 3) * 0.25 - 3.0) if accumulate else torch.full((M, 3), 7.0, device=DEV)
    ops.check(lib.mh_grid_encode_bwd_binned(ops.ptr(grad), ops.ptr(x), ops.ptr(emb), o_np.ctypes.data, r_np.ctypes.data, ops.ptr(perm),
                                            ops.ptr(bstart), ops.ptr(g_emb), ops.ptr(acc), ops.ptr(g_x), int(accumulate), M, 16, n_levels,
                                            bound, None, ops.stream()), "mh_grid_encode_bwd_binned")
    torch.cuda.synchronize()
    nbrk = lib.mh_grid_bin_bricks()
    return g_emb, g_x, int(bstart[nbrk + 2 + nbrk])


@pytest.mark.parametrize("accumulate", [False, True], ids=["dx_fresh", "dx_accumulated"])
@pytest.mark.parametrize("name", list(CASES))
def test_staged_columns_give_the_direct_forms_bits(name, accumulate):
    from morpheus_amd import _lib
    lib = _lib.load()
    x, grad, bound, n_levels = CASES[name]()
    x, grad = x.to(DEV).contiguous(), grad.to(DEV).contiguous()
    knob = lib.mh_grid_stage_min_points(-1)
    try:
        t_staged, dx_staged, items = _run(lib, 0, x, grad, bound, n_levels, accumulate)
        t_direct, dx_direct, _ = _run(lib, 1 << 40, x, grad, bound, n_levels, accumulate)
    finally:
        lib.mh_grid_stage_min_points(knob)
    if name == "corner_2049":
        assert items == 2           # 2048 points staged, and one point gathered directly
    if name in ("interior_96", "interior_95", "lattice_11"):
        assert items == 1
    print(f"GRIDCOL {name} accumulate={int(accumulate)}: work items {items}, table entries set {int((t_direct != 0).sum())}, "
          f"differing {int((t_staged != t_direct).sum())}; d/dx rows differing {int((dx_staged != dx_direct).any(1).sum())}")
    assert bool(t_direct.any()) and bool(torch.isfinite(t_direct).all()) and bool(torch.isfinite(dx_direct).all())
    if not accumulate:
        assert bool((dx_direct != 0).any()) and not bool((dx_direct == 7.0).any())      # fresh: fully written, zeros outside the box
    assert torch.equal(t_staged, t_direct)
    assert torch.equal(dx_staged, dx_direct)
