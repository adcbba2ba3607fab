"""Image resampling without a GPU: the numpy restatements (tests/imageops_oracle.py) against torch's own F.interpolate in float64,
forward and backward; the area rule's weights; the refusals of the Python layer; the build tables."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import imageops_oracle as io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = 2.0 ** -53


@pytest.mark.parametrize("case", io.RESIZE_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1][0]}x{c[1][1]}")
def test_bilinear_restatement_is_f_interpolate_in_float64(case):
    """forward and autograd backward; values are in [0, 1) and the weights sum to 1, so a few double round-offs of 1 (forward) and
    of the largest column sum of weights (backward) bound the difference of two float64 evaluations of the same rule"""
    (Hi, Wi), (Ho, Wo) = case
    x = io.images((2, 3, Hi, Wi), 11).astype(np.float64)
    g = io.images((2, 3, Ho, Wo), 12).astype(np.float64) - 0.5
    xt = torch.from_numpy(x).requires_grad_(True)
    y = F.interpolate(xt, (Ho, Wo), mode="bilinear", align_corners=False)
    y.backward(torch.from_numpy(g))
    mine = io.bilinear_fwd(x, (Ho, Wo))
    assert np.abs(mine - y.detach().numpy()).max() <= 8 * E
    back = io.bilinear_bwd(g, (Hi, Wi))
    bound = 16 * E * max(1.0, float(np.abs(xt.grad.numpy()).max()))
    assert np.abs(back - xt.grad.numpy()).max() <= bound
    if (Hi, Wi) == (Ho, Wo):
        assert np.array_equal(mine, x) and np.array_equal(io.bilinear_fwd(x.astype(np.float32), (Ho, Wo), np.float32), x.astype(np.float32))


def test_bilinear_affine_map_and_fp32_taps():
    x = io.images((1, 2, 5, 7), 13)
    y = io.bilinear_fwd(x, (4, 9), np.float64, mul=2.0, add=-1.0)
    assert np.allclose(y, 2 * io.bilinear_fwd(x, (4, 9), np.float64) - 1, rtol=0, atol=4 * E)
    i0, i1, l0, l1 = io.axis_taps(7, 9, np.float32)
    assert l0.dtype == l1.dtype == np.float32 and i0.min() == 0 and i1.max() == 6 and bool(((i1 - i0) >= 0).all())
    assert i0[0] == 0 and l1[0] == 0                                    # the clamp of the negative source coordinate


@pytest.mark.parametrize("case", io.AREA_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1][0]}x{c[1][1]}")
def test_area_weights(case):
    (Hi, Wi), (Ho, Wo) = case
    for n_in, n_out in ((Hi, Ho), (Wi, Wo)):
        W = io.area_weights(n_in, n_out)
        assert np.abs(W.sum(axis=1) - 1).max() <= 4 * E and bool((W >= 0).all())
        assert np.abs(W.sum(axis=0) - n_out / n_in).max() <= 4 * E      # every source pixel is used once in all
    img = io.images((Hi, Wi, 3), 14)
    out = io.masked_area(img, None, (Ho, Wo))
    assert out.shape == (1, 3, Ho, Wo)
    if Hi % Ho == 0 and Wi % Wo == 0:                                   # an integer ratio: the block mean
        blocks = img.astype(np.float64).reshape(Ho, Hi // Ho, Wo, Wi // Wo, 3).mean(axis=(1, 3)).transpose(2, 0, 1)[None]
        assert np.abs(out - blocks).max() <= 8 * E
    mask = io.images((Hi, Wi), 15)
    comp = io.masked_area(img, mask, (Ho, Wo))
    white = io.masked_area(img, np.zeros((Hi, Wi), np.float32), (Ho, Wo))
    assert np.abs(white - 1).max() <= 4 * E and bool((comp >= out - 4 * E).all())      # white where masked out: never darker
    u8 = (img * 255).astype(np.uint8)
    assert np.abs(io.masked_area(u8, mask, (Ho, Wo)) - io.masked_area(u8.astype(np.float64) / 255, mask, (Ho, Wo))).max() <= 4 * E


def test_u8_restatements():
    x = np.array([0.0, 0.5, 1.0, 0.999], np.float32)
    assert io.frame_u8(x).tolist() == [0, 127, 255, 254]
    assert io.depth_u8(np.full((3, 4), 2.5, np.float32)).tolist() == [[0] * 4] * 3
    assert io.depth_u8(np.array([1.0, 2.0, 3.0], np.float32)).tolist() == [0, 127, 254]


def test_argument_checks_need_no_device():
    from morpheus_amd import imageops
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(ValueError, match="layout"):
        imageops.resize_bilinear(x, (8, 8), layout="hwc")
    with pytest.raises(ValueError, match="channels"):
        imageops.resize_bilinear(torch.zeros(2, 5, 4, 4), (8, 8))
    with pytest.raises(ValueError, match="channels"):
        imageops.resize_bilinear(torch.zeros(2, 4, 4, 5), (8, 8), layout="nhwc")
    with pytest.raises(ValueError, match="size"):
        imageops.resize_bilinear(x, (8, 0))
    with pytest.raises(ValueError, match="float32"):
        imageops.resize_bilinear(x.double(), (8, 8))
    with pytest.raises(NotImplementedError, match="enlarges"):
        imageops.masked_area_resize(torch.zeros(4, 4, 3), None, (8, 8))
    with pytest.raises(NotImplementedError, match="enlarges"):
        imageops.masked_area_resize(torch.zeros(8, 4, 3), None, (4, 8))
    with pytest.raises(ValueError, match="mask"):
        imageops.masked_area_resize(torch.zeros(4, 4, 3), torch.zeros(4, 5), (2, 2))
    with pytest.raises(ValueError, match="frame"):
        imageops.masked_area_resize(torch.zeros(4, 4, 4), None, (2, 2))
    with pytest.raises(ValueError, match="float32"):
        imageops.frame_to_u8(torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="float32"):
        imageops.depth_to_u8(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="clip_pair"):
        imageops.clip_pair(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8), torch.zeros(1, 1, 8, 8))
    # with valid arguments the next thing asked for is the GPU
    from morpheus_amd._lib import MorpheusHipError
    with pytest.raises(MorpheusHipError, match="MI355X"):
        imageops.resize_bilinear(x, (8, 8))


def test_sources_and_entry_points():
    from morpheus_amd import _lib, build
    assert "imageops.hip" in build.SOURCES and "imageops.hip" not in build.FILE_FLAGS          # its own pragma, like sampler.hip
    src = open(os.path.join(build.CSRC, "imageops.hip")).read()
    assert "#pragma clang fp contract(off)" in src and '#include "wave.h"' in src
    hdr = open(os.path.join(ROOT, "include", "morpheus_hip.h")).read()
    for name in ("mh_resize_bilinear_fwd", "mh_resize_bilinear_bwd", "mh_resize_area_masked", "mh_frame_to_u8", "mh_depth_to_u8",
                 "mh_depth_range_words"):
        assert len(re.findall(r"\b%s\s*\(" % name, hdr)) == 1 and name in _lib.EXPORTS, name
    lib = _lib.load()
    assert lib.mh_depth_range_words() == 512
    # status codes, never launches, for bad arguments
    assert lib.mh_resize_bilinear_fwd(None, 1, 3, 4, 4, 8, 8, 0, 1.0, 0.0, None, None) == 1
    assert lib.mh_resize_bilinear_bwd(None, 1, 5, 4, 4, 8, 8, 0, 1.0, None, None) == 1
    assert lib.mh_resize_area_masked(None, 0, None, 4, 4, 2, 2, None, None) == 1
    assert lib.mh_frame_to_u8(None, 0, None, None) == 0 and lib.mh_frame_to_u8(None, 4, None, None) == 1
    assert lib.mh_depth_to_u8(None, 0, None, None, None) == 0 and lib.mh_depth_to_u8(None, 4, None, None, None) == 1
