"""GPU: the image kernels (csrc/imageops.hip) in the float64 judgement of tests/f64_judge -- the kernel's worst scaled error against
the float64 result at most max(3 x the worst error of the fp32 reference, 4 U).  The bilinear reference is torch's own
F.interpolate on the CPU (float64: the record; fp32: the yardstick), the area reference tests/imageops_oracle.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import f64_judge as J
from tests import imageops_oracle as io

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR, FLOOR = 3, 4 * J.U
B, C = 2, 3
IDS = [f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in io.RESIZE_CASES]


def _judge(hip, ref32, f64, scale, what):
    f = J.figures_vs_f64(hip, ref32, f64, scale, what, FLOOR)
    print(f"{what}: worst {f['worst_hip'] / J.U:.2f} U vs float64; the fp32 reference's own {f['worst_ref'] / J.U:.2f} U")
    assert f["bad_hip"] == 0, what
    assert J.within(f["worst_hip"], f["worst_ref"], FACTOR, FLOOR), (what, f["worst_hip"] / J.U, f["worst_ref"] / J.U)


@pytest.fixture(scope="module")
def records():
    """per case: x, g (fp32 numpy, nchw) and F.interpolate's forward / backward on the CPU in float64 and fp32 -- computed once"""
    out = {}
    for (hi, wi), (ho, wo) in io.RESIZE_CASES:
        x, g = io.images((B, C, hi, wi), 21), io.images((B, C, ho, wo), 22) - np.float32(0.5)
        rec = dict(x=x, g=g)
        for tag, dt in (("64", torch.float64), ("32", torch.float32)):
            xt = torch.from_numpy(x).to(dt).requires_grad_(True)
            y = F.interpolate(xt, (ho, wo), mode="bilinear", align_corners=False)
            y.backward(torch.from_numpy(g).to(dt))
            rec["y" + tag], rec["gx" + tag] = y.detach(), xt.grad
        # the natural size of a gradient element: the adjoint applied to |g|
        rec["gscale"] = torch.from_numpy(io.bilinear_bwd(np.abs(g), (hi, wi)))
        out[((hi, wi), (ho, wo))] = rec
    return out


def _run(rec, size, layout, mul=1.0, add=0.0):
    from morpheus_amd import imageops
    x = torch.from_numpy(rec["x"]).to(DEV)
    if layout == "nhwc":
        x = x.permute(0, 2, 3, 1).contiguous()
    x.requires_grad_(True)
    y = imageops.resize_bilinear(x, size, layout=layout, mul=mul, add=add)
    y.backward(torch.from_numpy(rec["g"]).to(DEV))
    gx = x.grad if layout == "nchw" else x.grad.permute(0, 3, 1, 2)
    return x.detach(), y.detach(), gx


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("case", io.RESIZE_CASES, ids=IDS)
def test_resize_bilinear_against_float64(records, case, layout):
    (hi, wi), (ho, wo) = case
    rec = records[case]
    x, y, gx = _run(rec, (ho, wo), layout)
    assert y.shape == (B, C, ho, wo) and gx.shape == (B, C, hi, wi) and y.dtype == gx.dtype == torch.float32
    what = f"{hi}x{wi}->{ho}x{wo} {layout}"
    _judge(y, rec["y32"], rec["y64"], 1.0, what + " forward")                       # images in [0, 1): their size is 1
    _judge(gx, rec["gx32"], rec["gx64"], rec["gscale"], what + " backward")
    if (hi, wi) == (ho, wo):                                                         # identity: the permuted input bit for bit
        assert torch.equal(y.cpu(), torch.from_numpy(rec["x"]))
    # the adjoint: <fwd(x), g> = <x, bwd(g)>, both products in float64.  Every term |g_o| w_oi |x_i| passes through at most
    # 8 roundings forward (three products, two sums per row pair, the affine map) and 2 + K backward (the weight's product, the
    # term's product, K accumulations), K the most output pixels one input pixel is read by
    K = (2 * -(-ho // hi) + 2) * (2 * -(-wo // wi) + 2)
    g64, x64 = torch.from_numpy(rec["g"]).double(), torch.from_numpy(rec["x"]).double()
    lhs, rhs = (y.double().cpu() * g64).sum(), (x64 * gx.double().cpu()).sum()
    terms = (torch.from_numpy(io.bilinear_fwd(np.abs(rec["x"]), (ho, wo))) * g64.abs()).sum()
    r = J.judge_sum(rhs.reshape(1), lhs.reshape(1), terms.reshape(1), 10 + K, what + " adjoint")
    print(f"{what} adjoint: {r['ratio']:.3f} of the bound")
    _, _, again = _run(rec, (ho, wo), layout)
    assert torch.equal(gx, again)                                                    # a gather in a fixed order


def test_resize_bilinear_affine_map_is_the_references_two_statements(records):
    """`F.interpolate(...) * 2 - 1` (zero123_utils.py:155, :288) folded into the kernel: forward and backward"""
    case = ((36, 36), (32, 32))
    rec = records[case]
    _, y, gx = _run(rec, case[1], "nhwc", mul=2.0, add=-1.0)
    _judge(y, rec["y32"] * 2 - 1, rec["y64"] * 2 - 1, 1.0, "36->32 * 2 - 1 forward")
    _judge(gx, rec["gx32"] * 2, rec["gx64"] * 2, rec["gscale"] * 2, "36->32 * 2 - 1 backward")


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "uint8"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("case", io.AREA_CASES, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in io.AREA_CASES])
def test_masked_area_resize(case, masked, u8):
    from morpheus_amd import imageops
    (hi, wi), (ho, wo) = case
    img = io.images((hi, wi, 3), 31)
    if u8:
        img = (img * 255).astype(np.uint8)
    mask = io.images((hi, wi), 32) if masked else None
    out = imageops.masked_area_resize(torch.from_numpy(img).to(DEV), None if mask is None else torch.from_numpy(mask).to(DEV), (ho, wo))
    assert out.shape == (1, 3, ho, wo) and out.dtype == torch.float32
    _judge(out, io.masked_area(img, mask, (ho, wo), np.float32), io.masked_area(img, mask, (ho, wo)), 1.0,
           f"area {hi}x{wi}->{ho}x{wo} mask {masked} uint8 {u8}")
    if (hi, wi) == (ho, wo) and not u8:
        assert np.array_equal(out.cpu().numpy(), io.masked_area(img, mask, (ho, wo), np.float32))


def test_masked_area_resize_refuses_to_enlarge():
    from morpheus_amd import imageops
    with pytest.raises(NotImplementedError, match="enlarges"):
        imageops.masked_area_resize(torch.zeros(4, 4, 3, device=DEV), None, (8, 8))


def test_frames_to_uint8():
    from morpheus_amd import imageops
    x = io.images((37, 53, 3), 41)
    x.reshape(-1)[:4] = [0.0, 1.0, 0.5, 254.5 / 255]
    got = imageops.frame_to_u8(torch.from_numpy(x).to(DEV))
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), io.frame_u8(x))
    for shape, seed in (((37, 53), 42), ((300, 301), 43)):                            # one block's share, and more than the grid covers at once
        d = io.images(shape, seed) * np.float32(3.0) + np.float32(0.25)
        got = imageops.depth_to_u8(torch.from_numpy(d).to(DEV))
        assert got.dtype == torch.uint8 and got.shape == shape and np.array_equal(got.cpu().numpy(), io.depth_u8(d))
        assert int(got.max()) == 254 and int(got.min()) == 0
    flat = torch.full((19, 23), 1.75, device=DEV)
    assert int(imageops.depth_to_u8(flat).max()) == 0                                 # max - min = 0: all 0


def test_clip_pair():
    from morpheus_amd import imageops
    pred, gt, mask = io.images((1, 20, 28, 3), 51), io.images((1, 3, 20, 28), 52), io.images((1, 1, 20, 28), 53)
    a, b = imageops.clip_pair(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(mask).to(DEV), size=24)
    m = (mask > 0.5).astype(np.float32)
    for got, src, what in ((a, pred.transpose(0, 3, 1, 2), "pred"), (b, gt * m + 1 - m, "gt")):
        _judge(got, io.bilinear_fwd(src, (24, 24), np.float32), io.bilinear_fwd(src, (24, 24)), 1.0, "clip_pair " + what)
    same = imageops.clip_pair(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(mask).to(DEV), size=(20, 28))
    assert torch.equal(same[0].cpu(), torch.from_numpy(pred).permute(0, 3, 1, 2))
