"""numpy restatements of csrc/imageops.hip -- the checker, not the product.

bilinear_*: PyTorch's upsample_bilinear2d with align_corners=False and no scale factor, statement by statement in `dtype`.  The
source coordinate and the weights are formed in `coord` (default: `dtype`, as F.interpolate forms them in the type of its input;
coord=np.float32 with dtype=np.float64 is the kernel's taps with exact sums behind them).
area_*: the shrinking area rule with exact fractional overlaps.
"""
import numpy as np

# (Hi, Wi) -> (Ho, Wo): single source pixel; tiny mixed; non-square mixed; non-integer shrink; the as_latent path; the training
# render size; identity
RESIZE_CASES = (((1, 1), (4, 4)), ((2, 3), (3, 2)), ((5, 7), (4, 9)), ((37, 53), (23, 31)), ((36, 36), (32, 32)),
                ((72, 72), (256, 256)), ((16, 16), (16, 16)))
AREA_CASES = (((12, 12), (4, 4)), ((13, 17), (5, 8)), ((8, 8), (8, 8)))


def axis_taps(n_in, n_out, coord=np.float32):
    """-> (i0, i1, l0, l1) of every output index of one axis; coord: the type the source coordinate is formed in"""
    f = coord
    scale = f(n_in) / f(n_out)
    src = scale * (np.arange(n_out).astype(f) + f(0.5)) - f(0.5)
    src = np.where(src < 0, f(0), src).astype(f)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(f)).astype(f)
    l0 = (f(1) - l1).astype(f)
    return i0, i1, l0, l1


def bilinear_fwd(x, size, dtype=np.float64, coord=None, mul=1.0, add=0.0):
    """x [B,C,Hi,Wi] -> [B,C,Ho,Wo] in `dtype`"""
    coord = coord or dtype
    x = np.asarray(x).astype(dtype)
    h0, h1, lh0, lh1 = axis_taps(x.shape[2], size[0], coord)
    w0, w1, lw0, lw1 = axis_taps(x.shape[3], size[1], coord)
    lh0, lh1 = lh0.astype(dtype)[:, None], lh1.astype(dtype)[:, None]
    lw0, lw1 = lw0.astype(dtype)[None, :], lw1.astype(dtype)[None, :]
    top = lw0 * x[:, :, h0][:, :, :, w0] + lw1 * x[:, :, h0][:, :, :, w1]
    bot = lw0 * x[:, :, h1][:, :, :, w0] + lw1 * x[:, :, h1][:, :, :, w1]
    return (dtype(mul) * (lh0 * top + lh1 * bot) + dtype(add)).astype(dtype)


def axis_matrix(n_in, n_out, dtype=np.float64, coord=None):
    """the interpolation of one axis as a matrix [n_out, n_in]"""
    i0, i1, l0, l1 = axis_taps(n_in, n_out, coord or dtype)
    M = np.zeros((n_out, n_in), dtype)
    np.add.at(M, (np.arange(n_out), i0), l0.astype(dtype))
    np.add.at(M, (np.arange(n_out), i1), l1.astype(dtype))
    return M


def bilinear_bwd(gy, in_size, dtype=np.float64, coord=None, mul=1.0):
    """the adjoint: gy [B,C,Ho,Wo] -> gx [B,C,Hi,Wi]"""
    gy = np.asarray(gy).astype(dtype)
    Mh = axis_matrix(in_size[0], gy.shape[2], dtype, coord)
    Mw = axis_matrix(in_size[1], gy.shape[3], dtype, coord)
    return (dtype(mul) * np.einsum("oi,bcop,pj->bcij", Mh, gy, Mw)).astype(dtype)


def area_weights(n_in, n_out, dtype=np.float64):
    """[n_out, n_in]: the share of source pixel i in output pixel o's box [o n_in / n_out, (o + 1) n_in / n_out), as exact
    integer overlaps in units of 1 / n_out over n_in"""
    assert n_out <= n_in
    o, i = np.arange(n_out)[:, None], np.arange(n_in)[None, :]
    overlap = np.minimum((o + 1) * n_in, (i + 1) * n_out) - np.maximum(o * n_in, i * n_out)
    return (np.maximum(overlap, 0).astype(dtype) / dtype(n_in)).astype(dtype)


def masked_area(image, mask, size, dtype=np.float64):
    """image [H,W,3] float in [0,1] or uint8, mask [H,W] or None -> [1,3,Ho,Wo]"""
    image = np.asarray(image)
    img = image.astype(dtype) / dtype(255) if image.dtype == np.uint8 else image.astype(dtype)
    m = np.ones(img.shape[:2], dtype) if mask is None else (np.asarray(mask).astype(np.float32) > 0.5).astype(dtype)
    comp = img * m[..., None] + (1 - m[..., None])
    Wh, Ww = area_weights(img.shape[0], size[0], dtype), area_weights(img.shape[1], size[1], dtype)
    return np.einsum("oi,ijc,pj->cop", Wh, comp, Ww)[None].astype(dtype)


def frame_u8(x):
    """morpheus.py:1318"""
    return (np.asarray(x, np.float32) * 255).astype(np.uint8)


def depth_u8(d):
    """morpheus.py:1321-1322"""
    d = np.asarray(d, np.float32)
    d = (d - d.min()) / (d.max() - d.min() + 1e-6)
    return (d * 255).astype(np.uint8)


def images(shape, seed):
    """the test images: uniform in [0, 1), fp32"""
    return np.random.RandomState(seed).rand(*shape).astype(np.float32)
