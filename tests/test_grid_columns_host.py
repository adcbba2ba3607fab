"""The staged hash-grid backward's accumulator layout (csrc/hashgrid.hip:brick_layout), read through mh_grid_bwd_layout: no GPU.

A lane group of an 8-byte LDS atomic is the 16 levels of one point; the layout gives every level its own column of the 16 words a
128-byte row has, for each of a vertex's three words, so that a group never shares a bank pair.  Checked here: the columns are
permutations, no two segments overlap, the rows fit the kernel's accumulator, the shipped pyramid reaches the 1091-row bound, and a
geometry that cannot be packed comes back with the linear layout."""
import ctypes

import numpy as np
import pytest

from morpheus_amd import synth
from morpheus_amd.ops import level_resolutions

OK, ERR_ARG = 0, 1
ACC_ROWS = 1152                 # BRK_ACC_ROWS: with flush_par (1 KB) and item the kernel stays inside 160 KB of LDS
LDS_BYTES = 160 * 1024
BRK = 16


def _layout(res):
    from morpheus_amd import _lib
    _lib.load()
    res = np.ascontiguousarray(res, np.int32)
    cbase = np.full(48, -1, np.int32)
    stride, rows = ctypes.c_int32(-1), ctypes.c_int32(-1)
    st = _lib._fns["mh_grid_bwd_layout"](res.ctypes.data_as(ctypes.c_void_p), len(res), cbase.ctypes.data_as(ctypes.c_void_p),
                                         ctypes.byref(stride), ctypes.byref(rows))
    return st, cbase.reshape(3, 16), stride.value, rows.value


def _sizes(res):
    return [int((int(r) + BRK - 1) // BRK + 2) ** 3 for r in res]


def _pyramid(top):
    """16 levels from 16 to `top`, the shipped rule (the shipped pyramid is top = 128)."""
    return level_resolutions(16, float(np.exp2(np.log2(top / 16.0) / 15.0)), 16)


def _check_columns(res, cbase, stride, rows):
    sz = _sizes(res)
    assert stride == 128
    assert (cbase % 8 == 0).all() and (cbase >= 0).all()
    col, row0 = (cbase // 8) % 16, cbase // 128
    taken = {}
    for k in range(3):
        assert sorted(col[k].tolist()) == list(range(16)), f"word {k}: the levels' columns are no permutation: {col[k]}"
        for l in range(16):
            taken.setdefault(int(col[k][l]), []).append((int(row0[k][l]), int(row0[k][l]) + sz[l]))
    top = 0
    for c, segs in taken.items():
        segs.sort()
        assert len(segs) == 3
        for (a0, a1), (b0, b1) in zip(segs, segs[1:]):
            assert a1 <= b0, f"column {c}: segments overlap: {segs}"
        top = max(top, segs[-1][1])
    assert top == rows, "the row count is the tallest column"
    assert rows <= ACC_ROWS and rows * 128 + 16 * 16 * 4 + 3 * 4 <= LDS_BYTES
    # every word of every vertex inside the accumulator
    assert max(int(cbase[k][l]) + (sz[l] - 1) * stride + 8 for k in range(3) for l in range(16)) <= ACC_ROWS * 128


def test_getter_is_declared_and_exported():
    from morpheus_amd import _lib
    _lib.load()
    assert "mh_grid_bwd_layout" in _lib.EXPORTS and "mh_grid_bwd_layout" in _lib._fns


def test_shipped_pyramid_packs_into_the_1091_row_bound():
    offs, s = synth.grid_offsets()
    res = level_resolutions(16, s, 16)
    assert sorted(_sizes(res)) == [27] + [64] * 5 + [125] * 2 + [216] * 3 + [343, 512, 729, 729, 1000]
    st, cbase, stride, rows = _layout(res)
    assert st == OK
    _check_columns(res, cbase, stride, rows)
    # three 1000-vertex segments need three columns, and each word has one 27: the best is 1000 + 27 + 64
    assert rows == 1091


@pytest.mark.parametrize("top", [64, 96, 128])
def test_pyramids_get_conflict_free_columns(top):
    res = _pyramid(top)
    assert int(res[-1]) == top and sum(_sizes(res)) <= 4608
    st, cbase, stride, rows = _layout(res)
    assert st == OK
    _check_columns(res, cbase, stride, rows)
    # no packing beats the mean column height, nor the largest level with the two smallest of the other words
    sz = sorted(_sizes(res))
    assert rows >= max(-(-3 * sum(sz) // 16), sz[-1] + sz[0] + sz[0])


def test_geometry_that_does_not_pack_gets_the_linear_layout():
    # 15 segments of 729 take 15 columns (two of them, or one beside a 512, pass 1152 rows): the three 512s share the last, 1536 rows
    res = np.array([100] * 5 + [90] + [8] * 10, np.int32)
    sz = _sizes(res)
    assert sz == [729] * 5 + [512] + [27] * 10 and sum(sz) <= 4608
    st, cbase, stride, rows = _layout(res)
    assert st == OK
    assert stride == 24
    first = np.concatenate([[0], np.cumsum(sz)[:-1]])
    for k in range(3):
        assert cbase[k].tolist() == (8 * (3 * first + k)).tolist()
    assert rows == -(-24 * sum(sz) // 128) and rows <= ACC_ROWS


def test_getter_refuses_what_the_binned_calls_refuse():
    res = _pyramid(128)
    assert _layout(res[:8])[0] == ERR_ARG                       # L != 16
    assert _layout(np.full(16, 128, np.int32))[0] == ERR_ARG    # 16 x 1000 vertices: more than the brick kernels hold
    bad = res.copy()
    bad[3] = 1
    assert _layout(bad)[0] == ERR_ARG
    from morpheus_amd import _lib
    f = _lib._fns["mh_grid_bwd_layout"]
    r = np.ascontiguousarray(res, np.int32)
    assert f(None, 16, 4096, 4096, 4096) == ERR_ARG
    assert f(r.ctypes.data_as(ctypes.c_void_p), 16, None, 4096, 4096) == ERR_ARG
