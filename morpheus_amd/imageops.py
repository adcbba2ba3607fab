"""Image resampling around the guidance and the test video, on the HIP kernels of csrc/imageops.hip (which states every operation):

    resize_bilinear      F.interpolate(mode="bilinear", align_corners=False) with the renderer's [B,H,W,C] layout and an affine map
                         (`* 2 - 1`) folded in; differentiable, the backward a deterministic gather
    masked_area_resize   get_embeddings' composite on white and cv2.INTER_AREA shrink (morpheus.py:254-259)
    frame_to_u8, depth_to_u8   render_test_video's uint8 frames (morpheus.py:1317-1322), the depth's range found on the device
    clip_pair            the two CLIP inputs of morpheus.py:1341-1353

Arguments are checked before a device is asked for; the kernels themselves run on the GPU only.
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import _lib
from ._lib import launch, ptr, require_gpu

MAX_CHANNELS = 4
_LAYOUTS = ("nchw", "nhwc")


def _size(size) -> Tuple[int, int]:
    if isinstance(size, int):
        size = (size, size)
    if len(size) != 2 or int(size[0]) < 1 or int(size[1]) < 1:
        raise ValueError(f"size: (H, W) with both at least 1 expected, got {size!r}")
    return int(size[0]), int(size[1])


def _geometry(shape, layout):
    """-> (B, C, H, W) of an image batch in `layout`"""
    if layout not in _LAYOUTS:
        raise ValueError(f"layout: one of {_LAYOUTS} expected, got {layout!r}")
    if len(shape) != 4:
        raise ValueError(f"resize_bilinear: a 4-d image batch expected, got {tuple(shape)}")
    B, C, H, W = shape if layout == "nchw" else (shape[0], shape[3], shape[1], shape[2])
    if not 1 <= C <= MAX_CHANNELS or H < 1 or W < 1:
        raise ValueError(f"resize_bilinear: 1 to {MAX_CHANNELS} channels and a non-empty image expected, got {tuple(shape)} as {layout}")
    return B, C, H, W


class _ResizeBilinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Ho, Wo, nhwc, mul, add):
        x = x.contiguous()
        B, C, Hi, Wi = _geometry(x.shape, "nhwc" if nhwc else "nchw")
        y = torch.empty(B, C, Ho, Wo, device=x.device, dtype=torch.float32)
        launch("mh_resize_bilinear_fwd", ptr(x), B, C, Hi, Wi, Ho, Wo, int(nhwc), mul, add, ptr(y))
        ctx.geom = (B, C, Hi, Wi, Ho, Wo, nhwc, mul, tuple(x.shape))
        return y

    @staticmethod
    def backward(ctx, gy):
        B, C, Hi, Wi, Ho, Wo, nhwc, mul, shape = ctx.geom
        gy = gy.contiguous().float()
        gx = torch.empty(shape, device=gy.device, dtype=torch.float32)
        launch("mh_resize_bilinear_bwd", ptr(gy), B, C, Hi, Wi, Ho, Wo, int(nhwc), mul, ptr(gx))
        return gx, None, None, None, None, None


def resize_bilinear(x, size, layout: str = "nchw", mul: float = 1.0, add: float = 0.0):
    """x fp32 [B,C,Hi,Wi] ("nchw") or [B,Hi,Wi,C] ("nhwc", what render_rays returns), C <= 4 -> [B,C,Ho,Wo] =
    mul * F.interpolate(x as nchw, size, mode="bilinear", align_corners=False) + add.  Differentiable in x."""
    Ho, Wo = _size(size)
    _geometry(x.shape, layout)
    if x.dtype != torch.float32:
        raise ValueError(f"resize_bilinear: float32 expected, got {x.dtype}")
    require_gpu(x)
    return _ResizeBilinear.apply(x, Ho, Wo, layout == "nhwc", float(mul), float(add))


@torch.no_grad()
def masked_area_resize(image, mask, size):
    """image [H,W,3] fp32 in [0,1] or uint8, mask [H,W] or None -> fp32 [1,3,Ho,Wo]: image * m + (1 - m) with m = mask > 0.5
    (the frame on white, morpheus.py:254-258), averaged over every output pixel's source box with its exact fractional overlaps
    (cv2.INTER_AREA when shrinking, :259).  No backward.  An enlarging axis is refused."""
    Ho, Wo = _size(size)
    if image.dim() != 3 or image.shape[2] != 3 or image.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"masked_area_resize: a float32 or uint8 frame [H,W,3] expected, got {image.dtype} {tuple(image.shape)}")
    H, W = image.shape[:2]
    if mask is not None and tuple(mask.shape) != (H, W):
        raise ValueError(f"masked_area_resize: mask [{H},{W}] expected, got {tuple(mask.shape)}")
    if Ho > H or Wo > W:
        raise NotImplementedError(f"masked_area_resize: ({H},{W}) -> ({Ho},{Wo}) enlarges an axis; only the shrinking area rule "
                                  "(every output pixel the weighted mean of its source box) is served")
    require_gpu(image, mask)
    image = image.contiguous()
    mask = None if mask is None else mask.float().contiguous()
    out = torch.empty(1, 3, Ho, Wo, device=image.device, dtype=torch.float32)
    launch("mh_resize_area_masked", ptr(image), int(image.dtype == torch.uint8), ptr(mask), H, W, Ho, Wo, ptr(out))
    return out


@torch.no_grad()
def frame_to_u8(x):
    """(x * 255).astype(uint8) of a float32 frame in [0,1] (morpheus.py:1318), any shape, on the device"""
    if x.dtype != torch.float32:
        raise ValueError(f"frame_to_u8: float32 expected, got {x.dtype}")
    require_gpu(x)
    x = x.contiguous()
    out = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    launch("mh_frame_to_u8", ptr(x), x.numel(), ptr(out))
    return out


@torch.no_grad()
def depth_to_u8(depth):
    """((d - d.min()) / (d.max() - d.min() + 1e-6) * 255).astype(uint8) (morpheus.py:1321-1322), any shape; the range is found on
    the device and nothing is read by the host"""
    if depth.dtype != torch.float32:
        raise ValueError(f"depth_to_u8: float32 expected, got {depth.dtype}")
    require_gpu(depth)
    d = depth.contiguous()
    out = torch.empty(d.shape, device=d.device, dtype=torch.uint8)
    scratch = torch.empty(int(_lib.load().mh_depth_range_words()), device=d.device, dtype=torch.int32)
    launch("mh_depth_to_u8", ptr(d), d.numel(), ptr(scratch), ptr(out))
    return out


@torch.no_grad()
def clip_pair(pred_nhwc, gt, gt_mask, size: int = 224):
    """The CLIP inputs of render_test_video (morpheus.py:1341-1353): pred_nhwc [B,H,W,3] (the renderer's layout) and the ground
    truth gt [B,3,H',W'] composited on white through gt_mask [B,1,H',W'] (thresholded at 0.5), both resized bilinearly to
    size x size unless they have it already -> (image_pred, image_gt), each [B,3,size,size]"""
    S = _size(size)
    if pred_nhwc.dim() != 4 or pred_nhwc.shape[3] != 3 or gt.dim() != 4 or gt.shape[1] != 3:
        raise ValueError(f"clip_pair: pred [B,H,W,3] and gt [B,3,H,W] expected, got {tuple(pred_nhwc.shape)}, {tuple(gt.shape)}")
    if gt_mask.dim() != 4 or gt_mask.shape[1] != 1 or gt_mask.shape[0] != gt.shape[0] or tuple(gt_mask.shape[2:]) != tuple(gt.shape[2:]):
        raise ValueError(f"clip_pair: gt_mask [B,1,H,W] beside gt {tuple(gt.shape)} expected, got {tuple(gt_mask.shape)}")
    require_gpu(pred_nhwc, gt, gt_mask)
    m = (gt_mask.float() > 0.5).float()
    image_gt = gt * m + 1 - m
    if tuple(pred_nhwc.shape[1:3]) != S:
        # the reference resizes both when the PREDICTION is not at size (:1351)
        return resize_bilinear(pred_nhwc.float(), S, layout="nhwc"), resize_bilinear(image_gt.float(), S)
    return pred_nhwc.permute(0, 3, 1, 2), image_gt
