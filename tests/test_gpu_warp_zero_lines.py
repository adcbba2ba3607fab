"""Line words of the b3 warp forward and the weight-gradient kernels that skip all-zero parked lines (round 8).

The forward parks, per tile, net, hidden layer and lane half, a 64-bit word saying which of the layer's 128 parked rows (one
128-byte line of 32 points each) carry a non-zero (csrc/mlp_b3.hip: b3_park_line_word); the per-layer kernels of
mh_warp_wgrad fetch a zero line in place of a row whose bit is 0 (csrc/mlp.hip: wg_line_ptr), for H rows and for the dPre rows
masked by the same ReLU signs.  Points are consecutive samples of synthetic rays (tools/parked_line_zeros.py), as in training:
only then do whole lines vanish.

Sizes: 1, 31, 33 (a partial tile: the lanes past M store values too and count), 257 (three workgroups, the merged small-batch
kernels: no skipping, the words must still be right) and 2^19 + 33 (>= 16 384 tiles: the per-layer kernels that skip; a
partial last tile and a tail wave).

Stage 2 of the issue (writers that do not store skipped lines, and its NaN-line knob) was not built -- DESIGN.md section 8.1 --
so there is no test of it here.
"""
import importlib.util
import os

import pytest
import torch

from morpheus_amd import synth
from oracle import field as of

_spec = importlib.util.spec_from_file_location(
    "parked_line_zeros", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "parked_line_zeros.py"))
plz = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(plz)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 31, 33, 257, (1 << 19) + 33]
TILE, ACT_ROWS, LINE_ROW = 32, 64 + 2 * 640 + 40, 40
_cache = {}


def _points():
    """ray-ordered sample points of frame 0, enough for the largest size (CPU, once)"""
    if "x" not in _cache:
        st = synth.make_state("b")
        n_rays = (max(SIZES) + 127) // 128
        x, t, hit = plz.ray_points(st, 0, n_rays, 128, 128)
        assert hit == 1.0
        code = of.multicode_sample([st[f"deform_code.volumes.{k}"] for k in range(3)], torch.tensor([t]))[0]
        _cache["x"], _cache["code"], _cache["state"] = x, code, st
    return _cache["x"], _cache["code"], _cache["state"]


def _nets(kind):
    """-> per net [W0 .. W5, b0 .. b5] (natural, weight norm applied) and the per-frame first-layer bias [1, 128], on the CPU.
    "b": synth state b.  "pos": first-layer and hidden biases so large that no unit is ever zero (|W h| <= ||w||_1 max|h| <=
    14 max|h| for these rows of norm <= 1.2, each bias is 100 x the layer below's).  "neg": the third hidden layer's biases
    large and negative: H3 is zero everywhere."""
    x, code, st = _points()
    out = []
    for prefix in ("deform_net", "topo_net"):
        W, b = plz.warp_params(st, prefix)
        b = [t.clone() for t in b]
        if kind == "pos":
            for l in range(5):
                b[l] = torch.full_like(b[l], 1e3 * 100.0 ** l)
        if kind == "neg":
            b[2] = torch.full_like(b[2], -1e6)
        bias0 = (W[0][:, 39:] @ code + b[0])[None].contiguous()
        out.append((W, b, bias0))
    return out


def _run(kind, M, skip):
    """forward, backward-data and weight gradients of M ray-ordered points -> outputs, g_x, parameter gradients, parked tiles"""
    from morpheus_amd import ops
    lib = ops._lib.load()
    x = _points()[0][:M].to(DEV)
    nets = _nets(kind)
    ps = [[W[0][:, :39].contiguous().to(DEV)] + [w.to(DEV) for w in W[1:]] + [t.to(DEV) for t in b] for W, b, _ in nets]
    ps = [[p.requires_grad_(True) for p in net] for net in ps]
    bb = [bias0.to(DEV).requires_grad_(True) for _, _, bias0 in nets]
    xg = x.clone().requires_grad_(True)
    g = torch.Generator().manual_seed(11)
    wd_, wt_ = torch.randn(M, 3, generator=g).to(DEV), torch.randn(M, 2, generator=g).to(DEV)
    before = lib.mh_warp_skip_zero_lines(-1)
    lib.mh_warp_skip_zero_lines(int(skip))
    try:
        d, t = ops.warp_mlp(xg, None, bb[0], bb[1], 6, ops.prepare_warp_operands(ps[0], ps[1], mode="b3"))
        acts = d.grad_fn.saved_tensors[4]
        n_tiles = lib.mh_mlp_tiles(M)
        tiles = acts[:n_tiles * ACT_ROWS * TILE].view(n_tiles, ACT_ROWS, TILE).clone()
        ((d * wd_).sum() + (t * wt_).sum()).backward()
    finally:
        lib.mh_warp_skip_zero_lines(before)
    grads = [[p.grad for p in net] for net in ps]
    return dict(d=d.detach(), t=t.detach(), gx=xg.grad, grads=grads, gb0=[t.grad for t in bb], tiles=tiles)


def _ref(kind, M):
    """the skipping-off run, made once per (weights, size) and shared"""
    key = ("off", kind, M)
    if key not in _cache:
        _cache[key] = _run(kind, M, skip=False)
    return _cache[key]


def _words(tiles):
    """the 160 bytes of line words at the head of H0's dead rows, as 40 floats per tile"""
    return tiles[:, LINE_ROW:LINE_ROW + 2].reshape(tiles.shape[0], 2 * TILE)[:, :40].contiguous()


def _written(tiles):
    """what the forward writes of a tile: the 40 encoding rows, the line words, H1..H5 of both nets and the sign masks (the rest of
    rows 40..63 is never written)"""
    return tiles[:, :LINE_ROW], _words(tiles), tiles[:, 64:]


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _cache.clear()
    torch.cuda.empty_cache()


def _words_and_lines(tiles):
    """parked tiles -> (bits the forward parked [tiles, net, layer, row] bool, (H != 0).any over the 32 stored values, same shape)"""
    n = tiles.shape[0]
    w = _words(tiles).view(torch.int32).reshape(n, 2, 5, 2, 2)                  # [net][layer][half][dword]
    bit = torch.arange(64, device=tiles.device)
    got64 = ((w[..., (bit >> 5)] >> (bit & 31)) & 1).bool()                      # [n, net, layer, half, bit 16 t + r]
    t_, r_ = bit >> 4, bit & 15
    got = torch.zeros(n, 2, 5, 128, dtype=torch.bool, device=tiles.device)
    for h in range(2):
        got[..., 32 * t_ + (r_ & 3) + 8 * (r_ >> 2) + 4 * h] = got64[..., h, :]
    H = tiles[:, 64:64 + 1280].view(n, 2, 5, 128, TILE)
    return got, (H.view(torch.int32) != 0).any(-1)


@pytest.mark.parametrize("M", SIZES)
def test_line_words_match_the_parked_rows(M):
    """every word bit of every tile == (H != 0).any over the row's 32 stored values (the padded tiles of the last block included)"""
    got, want = _words_and_lines(_ref("b", M)["tiles"])
    assert torch.equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("kind", ["b", "pos", "neg"])
def test_skipping_keeps_every_bit(kind, M):
    """outputs, g_x, parked tiles and every weight / bias gradient with skipping on are torch.equal to skipping off"""
    off, on = _ref(kind, M), _run(kind, M, skip=True)
    for k in ("d", "t", "gx"):
        assert torch.equal(on[k], off[k]), k
    for a, b in zip(_written(on["tiles"]), _written(off["tiles"])):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    n = 0
    for ga, gb in zip([g for net in on["grads"] for g in net] + on["gb0"], [g for net in off["grads"] for g in net] + off["gb0"]):
        assert (ga is None) == (gb is None)
        if ga is not None:
            n += 1
            assert torch.equal(ga, gb), (tuple(ga.shape), float((ga - gb).abs().max()))
            assert bool(torch.isfinite(ga).all())
    assert n >= 24 and bool(torch.isfinite(on["gx"]).all())      # 2 x (6 weights + b1 .. b5) + the two first-layer bias rows at least
    got, lines = _words_and_lines(on["tiles"])
    assert torch.equal(got, lines)
    if kind == "pos":
        assert bool(got.all())                                                  # nothing to skip
    if kind == "neg":
        assert not bool(got[:, :, 2].any()) and bool(got[:, :, 1].any())        # every line of H3 is zero, and is skipped
        for net in on["grads"]:                                                 # W0..W2, b1, b2: nothing reaches below H3
            for g_ in (net[0], net[1], net[2], net[7], net[8]):
                assert not bool(g_.view(torch.int32).bool().any()), tuple(g_.shape)
        for g_ in on["gb0"] + [on["gx"]]:
            assert not bool(g_.view(torch.int32).bool().any())


def test_the_inputs_have_zero_lines():
    """state b at 257 ray-ordered points: at least one tenth of the H lines are all zero (the CPU tool measures 0.2-0.45 per
    layer on these rays) -- otherwise the tests above could pass without ever skipping; and the per-layer kernels are the ones
    the largest size runs"""
    from morpheus_amd import ops
    got, _ = _words_and_lines(_ref("b", 257)["tiles"])
    share = 1.0 - float(got.float().mean())
    assert share >= 0.1, share
    big, _ = _words_and_lines(_ref("b", SIZES[-1])["tiles"])
    assert 1.0 - float(big.float().mean()) >= 0.1
    lib = ops._lib.load()
    assert lib.mh_warp_regen_dpre4(SIZES[-1]) == 1 and lib.mh_warp_regen_dpre4(257) == 0      # the per-layer path's own threshold
    assert lib.mh_warp_skip_zero_lines(-1) == 1                                                # on by default
