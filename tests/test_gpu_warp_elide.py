"""Eliding: the b3 warp chain kernels do not send an all-zero parked line to memory (round 9).

A call that opts in (ops.warp_mlp(elide=True)) and meets mh_warp_elides(M) leaves the rows whose line-word bit is 0 unwritten
(csrc/mlp_b3.hip: B3Park) and binds its backward to read the scratch by the words.  Here the scratch buffers are filled with a NaN
bit pattern before every run: an elided line must still hold it afterwards, a line whose bit is 1 must equal the non-eliding run's
line, and no NaN may reach an output or a gradient.

ELIDING names the writers that elide by default: the forward (the H blocks, "acts") and backward-data (the dPre blocks);
mh_warp_elide_zero_lines(1) leaves backward-data alone eliding, (0) nobody.  DESIGN.md section 8.1 has the measurements.

Points, weight sets ("b", "pos", "neg") and the word / row helpers are tests/test_gpu_warp_zero_lines.py's.
Sizes: 33 (a partial tile) and 257 (the merged small-batch kernels): an opt-in call must not elide there; 2^19 + 33: the smallest size
class of the per-layer path, a partial last tile and a tail wave.
"""
import pytest
import torch

from tests import test_gpu_warp_zero_lines as zl

pytestmark = pytest.mark.gpu
DEV = "cuda"
ELIDING = ("acts", "dpre")
BIG = (1 << 19) + 33
SIZES = [33, 257, BIG]
TILE, ACT_ROWS, DPRE_ROWS = 32, zl.ACT_ROWS, 2 * 672
POISON = 0x7FC0DEAD          # a quiet NaN no kernel produces
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _cache.clear()
    zl._cache.clear()
    torch.cuda.empty_cache()


def _run(kind, M, elide, flip=False, slots=1, level=None):
    """forward, backward-data and weight gradients of M ray-ordered points through ops.warp_mlp, every scratch buffer poisoned
    -> outputs, g_x, parameter gradients, the acts and dPre tiles as the backward left them.
    flip: mh_warp_skip_zero_lines(0) between forward and backward.  slots: rows of the first-layer bias (points alternate).
    level: mh_warp_elide_zero_lines for the call."""
    from morpheus_amd import ops
    lib = ops._lib.load()
    x = zl._points()[0][:M].to(DEV)
    nets = zl._nets(kind)
    ps = [[W[0][:, :39].contiguous().to(DEV)] + [w.to(DEV) for w in W[1:]] + [t.to(DEV) for t in b] for W, b, _ in nets]
    ps = [[p.requires_grad_(True) for p in net] for net in ps]
    bb = [bias0.to(DEV).repeat(slots, 1).requires_grad_(True) for _, _, bias0 in nets]
    slot = None if slots == 1 else (torch.arange(M, device=DEV, dtype=torch.int32) % slots).contiguous()
    xg = x.clone().requires_grad_(True)
    g = torch.Generator().manual_seed(11)
    wd_, wt_ = torch.randn(M, 3, generator=g).to(DEV), torch.randn(M, 2, generator=g).to(DEV)
    made, real = [], ops._scratch

    def poisoned(n, device, dtype=torch.float32):
        t = real(n, device, dtype)
        if dtype == torch.float32:
            t.view(torch.int32).fill_(POISON)
            made.append(t)
        return t

    before, level_before = lib.mh_warp_skip_zero_lines(-1), lib.mh_warp_elide_zero_lines(-1)
    ops._scratch = poisoned
    try:
        if level is not None:
            lib.mh_warp_elide_zero_lines(level)
        d, t = ops.warp_mlp(xg, slot, bb[0], bb[1], 6, ops.prepare_warp_operands(ps[0], ps[1], mode="b3"), elide=elide)
        elided = d.grad_fn.elided
        acts = d.grad_fn.saved_tensors[4]
        if flip:
            lib.mh_warp_skip_zero_lines(0)
        ((d * wd_).sum() + (t * wt_).sum()).backward()
    finally:
        ops._scratch = real
        lib.mh_warp_skip_zero_lines(before)
        lib.mh_warp_elide_zero_lines(level_before)
    n_tiles = lib.mh_mlp_tiles(M)
    dpre = [b for b in made if b.numel() == lib.mh_warp_dpre_floats(M)]
    assert len(dpre) == 1 and acts.numel() == lib.mh_warp_acts_floats(M)
    return dict(d=d.detach(), t=t.detach(), gx=xg.grad, grads=[[p.grad for p in net] for net in ps], gb0=[t.grad for t in bb],
                acts=acts[:n_tiles * ACT_ROWS * TILE].view(n_tiles, ACT_ROWS, TILE).view(torch.int32),
                dpre=dpre[0][:n_tiles * DPRE_ROWS * TILE].view(n_tiles, DPRE_ROWS, TILE).view(torch.int32), elided=elided)


def _ref(kind, M, slots=1):
    """the non-eliding run (the default call), made once per (weights, size) and shared"""
    key = (kind, M, slots)
    if key not in _cache:
        _cache[key] = _run(kind, M, elide=False, slots=slots)
        assert not _cache[key]["elided"]
    return _cache[key]


def _same_results(on, off):
    """outputs, g_x, every weight and bias gradient and both first-layer bias rows: equal bits, all finite"""
    for k in ("d", "t", "gx"):
        assert torch.equal(on[k], off[k]), k
        assert bool(torch.isfinite(on[k]).all()), k
    n = 0
    for ga, gb in zip([g for net in on["grads"] for g in net] + on["gb0"], [g for net in off["grads"] for g in net] + off["gb0"]):
        assert (ga is None) == (gb is None)
        if ga is not None:
            n += 1
            assert torch.equal(ga, gb), (tuple(ga.shape), float((ga - gb).abs().max()))
            assert bool(torch.isfinite(ga).all())
    assert n >= 24      # 2 x (6 weights + b1 .. b5) + the two first-layer bias rows at least


def _blocks(run):
    """-> row bits [tiles, net, layer, row] of the parked words, the H blocks and the dPre blocks 0..4 as [tiles, net, 5, 128, 32]
    int32 (dPre block k of a net lies under the word of H_(k+1), the same index)"""
    bits, _ = zl._words_and_lines(run["acts"].view(torch.float32))
    n = run["acts"].shape[0]
    H = run["acts"][:, 64:64 + 1280].view(n, 2, 5, 128, TILE)
    D = run["dpre"].view(n, 2, 672, TILE)[:, :, :640].reshape(n, 2, 5, 128, TILE)
    return bits, H, D


def _check_tiles(on, off, elided_writers):
    """words, masks and encoding rows equal; a line whose bit is 1 equals the non-eliding run's; a line whose bit is 0 holds the
    poison where its writer elides and the non-eliding run's zeros where it does not.
    -> {writer: share of the lines it would have written that it elided}"""
    for a, b in zip(zl._written(on["acts"])[:2], zl._written(off["acts"])[:2]):      # the 40 encoding rows, the line words
        assert torch.equal(a, b)
    assert torch.equal(on["acts"][:, zl.ACT_ROWS - 40:], off["acts"][:, zl.ACT_ROWS - 40:])      # the sign masks
    bits, H, D = _blocks(on)
    bits_off, H_off, D_off = _blocks(off)
    assert torch.equal(bits, bits_off)
    live = bits[..., None]
    share = {}
    for name, got, want in (("acts", H, H_off), ("dpre", D, D_off)):
        # (a block nobody writes -- dPre4 at the large size -- holds the poison in both runs and compares equal)
        assert torch.equal(torch.where(live, got, 0), torch.where(live, want, 0)), name
        dead_got, dead_want = got[~bits], want[~bits]
        if name in elided_writers:
            assert bool((dead_got == POISON).all()), name
            gone = int((dead_want != POISON).any(-1).sum())              # rows the non-eliding run wrote (as zeros)
            share[name] = gone / max(int((want.reshape(-1, TILE) != POISON).any(-1).sum()), 1)
        else:
            assert torch.equal(dead_got, dead_want), name
    # everything else of the dPre tile (dPre5's live rows, rows nobody writes)
    n = on["dpre"].shape[0]
    assert torch.equal(on["dpre"].view(n, 2, 672, TILE)[:, :, 640:], off["dpre"].view(n, 2, 672, TILE)[:, :, 640:])
    return share


@pytest.mark.parametrize("kind", ["b", "pos", "neg"])
def test_eliding_leaves_zero_lines_unwritten_and_keeps_every_bit(kind):
    """the large size: results equal and finite over a poisoned scratch; lines with bit 0 keep the poison, lines with bit 1 equal"""
    off, on = _ref(kind, BIG), _run(kind, BIG, elide=True)
    assert on["elided"]
    _same_results(on, off)
    share = _check_tiles(on, off, ELIDING)
    bits, H, D = _blocks(on)
    if kind == "pos":
        assert bool(bits.all()) and not any(share.values())                     # nothing to elide: the tiles are equal everywhere
        assert torch.equal(on["acts"][:, 64:], off["acts"][:, 64:]) and torch.equal(on["dpre"], off["dpre"])
    if kind == "neg":
        assert not bool(bits[:, :, 2].any()) and bool(bits[:, :, 1].any())
        if "acts" in ELIDING:
            assert bool((H[:, :, 2] == POISON).all())                           # all of H3 keeps the poison
        assert bool((D[:, :, 2] == POISON).all())                               # and all of dPre2
        for net in on["grads"]:                                                 # W0..W2, b1, b2: nothing reaches below H3
            for g_ in (net[0], net[1], net[2], net[7], net[8]):
                assert not bool(g_.view(torch.int32).bool().any()), tuple(g_.shape)
        for g_ in on["gb0"] + [on["gx"]]:
            assert not bool(g_.view(torch.int32).bool().any())
    if kind == "b":
        assert 1.0 - float(bits.float().mean()) >= 0.1                          # a tenth of the lines have bit 0 ...
        assert set(share) == set(ELIDING) and min(share.values()) >= 0.1, share # ... and each eliding writer left a tenth of its lines out


@pytest.mark.parametrize("M", [33, 257])
@pytest.mark.parametrize("kind", ["b", "pos", "neg"])
def test_small_batches_do_not_elide(kind, M):
    """an opt-in call below the per-layer path writes every line: tiles and results equal the default call's bit for bit"""
    off, on = _ref(kind, M), _run(kind, M, elide=True)
    assert not on["elided"]
    _same_results(on, off)
    assert torch.equal(on["acts"], off["acts"]) and torch.equal(on["dpre"], off["dpre"])
    assert _check_tiles(on, off, ()) == {}


def test_the_backward_reads_by_the_words_whatever_the_switch_says():
    """mh_warp_skip_zero_lines(0) between forward and backward of an eliding call: the decision travelled in the ctx"""
    off, on = _ref("b", BIG), _run("b", BIG, elide=True, flip=True)
    assert on["elided"]
    _same_results(on, off)
    _check_tiles(on, off, ELIDING)


@pytest.mark.parametrize("level, writers", [(0, ()), (1, ("dpre",))])
def test_the_switch_takes_writers_out(level, writers):
    """mh_warp_elide_zero_lines: 1 = the forward writes every H line and backward-data alone elides, 0 = the call elides nothing"""
    off, on = _ref("b", BIG), _run("b", BIG, elide=True, level=level)
    assert bool(on["elided"]) == (level > 0)
    _same_results(on, off)
    assert set(_check_tiles(on, off, writers)) == set(writers)


def test_two_slots_read_dpre0_rows_and_elide_nothing():
    """n_slots != 1: the per-slot bias gradients are sums over dPre0's rows read out of the scratch -- equal to the default call's.
    (The sums are torch's index_add_, whose default form on the GPU adds with atomics in any order: both runs ask for its
    deterministic form, or two runs of the SAME call differ in the last bits.)"""
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        off, on = _ref("b", BIG, slots=2), _run("b", BIG, elide=True, slots=2)
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])
    assert not on["elided"] and on["gb0"][0].shape == (2, 128)
    _same_results(on, off)
    assert _check_tiles(on, off, ()) == {}


def test_switches_and_the_small_batch_refusal():
    """mh_warp_elides follows both switches and the size.  (An elided tile handed to the merged small-batch kernels is MH_ERR_ARG:
    host-validated, tests/test_host.py::test_mlp_entries_validate_arithmetic_and_flags_without_gpu.)"""
    from morpheus_amd import ops
    lib = ops._lib.load()
    assert lib.mh_warp_elide_zero_lines(-1) == 2 and lib.mh_warp_elides(BIG) == 2 and lib.mh_warp_elides(257) == 0
    try:
        assert lib.mh_warp_elide_zero_lines(0) == 0 and lib.mh_warp_elides(BIG) == 0
        assert lib.mh_warp_elide_zero_lines(1) == 1 and lib.mh_warp_elides(BIG) == 1 and lib.mh_warp_elides(257) == 0
        assert lib.mh_warp_skip_zero_lines(0) == 0 and lib.mh_warp_elides(BIG) == 0
    finally:
        lib.mh_warp_elide_zero_lines(2)
        lib.mh_warp_skip_zero_lines(1)
