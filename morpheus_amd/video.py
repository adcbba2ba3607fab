"""Video output: baseline JPEG frames encoded on the device (csrc/video.hip, which states every operation) and the Motion-JPEG
AVI container around them.  What the reference writes with imageio / ffmpeg as H.264 .mp4 (morpheus.py:1285-1375,
tools/vis.py:21-33, visualizer.py:248) is written here as .avi: every frame an independent JFIF image that any player, a
browser, ffmpeg and PIL read; no inter-frame coding.

    encode_jpeg, write_jpeg     device uint8 frames -> complete JFIF files; the host adds the markers to the device's entropy bytes
    VideoWriter, write_video    RIFF 'AVI ' with one MJPG video stream, streamed to disk batch by batch (imageio.mimwrite's place)
    make_video                  tools/vis.py:make_video: a directory of PNGs -> a video
    read_video                  the container read back: fps, size and the JPEG of every frame
    render_test_video           the loop of morpheus.py:1285-1336 on device frames, without its CLIP leg

Arguments are checked before a device is asked for; the encoder itself runs on the GPU only.
"""
from __future__ import annotations

import os
import re
import struct
from array import array
from fractions import Fraction
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import _lib
from . import jpeg_tables as T
from ._lib import MorpheusHipError, launch, ptr, require_gpu
from .geometry import memory_cap_bytes
from .imageops import depth_to_u8, frame_to_u8

SUBSAMPLINGS = ("420", "444")
MAX_SIDE = 65535                     # SOF0 holds the size in 16 bits
MAX_BATCH = 64                       # frames per encoder call at most: bounds the pending frames and the latency of a flush
AVI_MAX_BYTES = 2 ** 31 - 1          # a plain RIFF AVI; OpenDML (AVIX) is not written


# ---- JFIF markers ---------------------------------------------------------------------------------------------------------------
def _segment(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def jpeg_header(H: int, W: int, channels: int, quality: int, subsampling: str) -> bytes:
    """SOI, APP0 (JFIF 1.01, no density), DQT, SOF0 with the true size, DHT (the Annex K tables), SOS: everything in front of the
    entropy-coded segment.  One table set for a single component, two for YCbCr."""
    tabs = 2 if channels == 3 else 1
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    for t in range(tabs):
        q = T.quant_table(quality, t)
        out += _segment(0xDB, bytes([t]) + bytes(q[n] for n in T.ZIGZAG))
    comps = [(1, 0x22 if channels == 3 and subsampling == "420" else 0x11, 0)]
    if channels == 3:
        comps += [(2, 0x11, 1), (3, 0x11, 1)]
    out += _segment(0xC0, struct.pack(">BHHB", 8, H, W, channels) + b"".join(bytes(c) for c in comps))
    for t in range(tabs):
        out += _segment(0xC4, bytes([t]) + bytes(T.DC_BITS[t]) + bytes(T.DC_VALS[t]))
        out += _segment(0xC4, bytes([0x10 + t]) + bytes(T.AC_BITS[t]) + bytes(T.AC_VALS[t]))
    return out + _segment(0xDA, bytes([channels]) + b"".join(bytes([cid, 0x11 * tab]) for cid, _, tab in comps) + b"\x00\x3f\x00")


JPEG_EOI = b"\xff\xd9"


# ---- the encoder's face ---------------------------------------------------------------------------------------------------------
def _check_coding(quality, subsampling):
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"quality: an integer 1 .. 100 expected, got {quality!r}")
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"subsampling: one of {SUBSAMPLINGS} expected, got {subsampling!r}")


def frame_geometry(shape) -> Tuple[int, int, int, int]:
    """-> (F, H, W, channels) of [F,H,W,3], [F,H,W], or one frame [H,W,3] / [H,W].  A 3-d shape that ends in 3 is one RGB frame."""
    shape = tuple(int(s) for s in shape)
    if len(shape) == 4 and shape[3] == 3:
        F, H, W, C = shape
    elif len(shape) == 3 and shape[2] == 3:
        F, (H, W, C) = 1, shape
    elif len(shape) == 3:
        (F, H, W), C = shape, 1
    elif len(shape) == 2:
        F, (H, W), C = 1, shape, 1
    else:
        raise ValueError(f"frames: [F,H,W,3], [F,H,W] or a single frame [H,W,3] / [H,W] expected, got {shape}")
    if F < 1 or not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"frames: at least one frame with sides 1 .. {MAX_SIDE} expected, got {shape}")
    return F, H, W, C


def _check_frames(frames, what="frames"):
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
        raise ValueError(f"{what}: a uint8 tensor expected, got {getattr(frames, 'dtype', type(frames))}")
    return frame_geometry(frames.shape)


def workspace_bytes_per_frame(H: int, W: int, channels: int, subsampling: str = "420") -> int:
    """device bytes one frame costs inside encode_jpeg: the kernel scratch and the output at its proven capacity"""
    lib = _lib.load()
    blocks = lib.mh_jpeg_blocks(H, W, channels, int(subsampling))
    if blocks < 0:
        raise MorpheusHipError(f"encode_jpeg: a frame of {H} x {W} has more blocks than one scan's bit count allows")
    cap = lib.mh_jpeg_scan_capacity(blocks)
    return int(lib.mh_jpeg_workspace_bytes(1, blocks, cap) + cap)


@torch.no_grad()
def encode_scans(frames, quality: int, subsampling: str, cap: Optional[int] = None, out: Optional[torch.Tensor] = None):
    """The raw entry point: frames uint8 [F,H,W,C] / [F,H,W] on the device -> (out uint8 [F,cap], counts int32 [F + 1]) on the
    device: counts[:F] the bytes of every frame's entropy-coded segment, counts[F] the overflow flag.  cap defaults to the proven
    capacity; a smaller one (a positive multiple of 32) is legal and raises the flag instead of writing past out[f]."""
    F, H, W, C = frame_geometry(frames.shape)
    lib = _lib.load()
    blocks = lib.mh_jpeg_blocks(H, W, C, int(subsampling))
    if blocks < 0:
        raise MorpheusHipError(f"encode_jpeg: a frame of {H} x {W} has more blocks than one scan's bit count allows")
    cap = int(lib.mh_jpeg_scan_capacity(blocks)) if cap is None else int(cap)
    wbytes = lib.mh_jpeg_workspace_bytes(F, blocks, cap)
    if wbytes < 0:
        raise MorpheusHipError(f"encode_jpeg: F = {F} (at most 65535) with capacity {cap} (a positive multiple of 32) is not served")
    frames = frames.contiguous()
    if frames.data_ptr() % 4:
        frames = frames.clone()
    dev = frames.device
    ws = torch.empty(int(wbytes), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty(F, cap, dtype=torch.uint8, device=dev)
    counts = torch.empty(F + 1, dtype=torch.int32, device=dev)
    launch("mh_jpeg_encode", ptr(frames), F, H, W, C, int(subsampling), int(quality), ptr(ws), out.data_ptr(), cap, ptr(counts),
           counts.data_ptr() + 4 * F)
    return out, counts


@torch.no_grad()
def encode_jpeg(frames, quality: int = 90, subsampling: str = "420") -> List[bytes]:
    """frames: device uint8 [F,H,W,3] (RGB -> YCbCr, `subsampling` "420" or "444"), [F,H,W] (one component) or a single frame
    [H,W,3] / [H,W] -> one complete baseline JFIF file per frame.  The device codes all frames in one pass; the host reads the F
    byte counts, copies the used bytes once and puts the markers around them."""
    _check_coding(quality, subsampling)
    F, H, W, C = _check_frames(frames)
    require_gpu(frames)
    out, counts = encode_scans(frames.reshape(F, H, W, C) if C == 3 else frames.reshape(F, H, W), quality, subsampling)
    counts = counts.cpu().tolist()
    if counts[F]:
        raise MorpheusHipError("encode_jpeg: the entropy-coded segment passed its proven capacity (device overflow flag)")
    data = bytes(torch.cat([out[f, :counts[f]] for f in range(F)]).cpu().numpy())
    head = jpeg_header(H, W, C, quality, subsampling)
    files, at = [], 0
    for f in range(F):
        files.append(head + data[at:at + counts[f]] + JPEG_EOI)
        at += counts[f]
    return files


def write_jpeg(path, frame, quality: int = 90, subsampling: str = "420") -> None:
    """one device uint8 frame [H,W,3] or [H,W] -> a .jpg file"""
    _check_coding(quality, subsampling)
    _check_frames(frame, "frame")
    if frame.dim() not in (2, 3) or (frame.dim() == 3 and frame.shape[2] != 3):
        raise ValueError(f"write_jpeg: one frame [H,W,3] or [H,W] expected, got {tuple(frame.shape)}")
    data, = encode_jpeg(frame, quality, subsampling)
    with open(path, "wb") as f:
        f.write(data)


# ---- Motion-JPEG AVI ------------------------------------------------------------------------------------------------------------
def _chunk(fourcc: bytes, payload: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(payload)) + payload + b"\x00" * (len(payload) & 1)


def _rate_scale(fps) -> Tuple[int, int]:
    fr = Fraction(fps).limit_denominator(1001 * 1000)
    if fr <= 0 or fr.numerator >= 2 ** 31:
        raise ValueError(f"fps: a positive frame rate expected, got {fps!r}")
    return fr.numerator, fr.denominator


def _avi_header(W: int, H: int, rate: int, scale: int, frames: int, largest: int, movi_bytes: int, riff_bytes: int) -> bytes:
    """RIFF 'AVI ' up to and including the `movi` list's fourcc; its length does not depend on the values"""
    avih = struct.pack("<14I", round(1e6 * scale / rate), min(2 ** 32 - 1, -(-largest * rate // scale)), 0, 0x10, frames, 0, 1,
                       largest, W, H, 0, 0, 0, 0)
    strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, scale, rate, 0, frames, largest, 0xFFFFFFFF, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", min(W * H * 3, 2 ** 32 - 1), 0, 0, 0, 0)
    strl = b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf)
    hdrl = b"hdrl" + _chunk(b"avih", avih) + _chunk(b"LIST", strl)
    return b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + _chunk(b"LIST", hdrl) + b"LIST" + struct.pack("<I", movi_bytes) + b"movi"


class VideoWriter:
    """Motion-JPEG in a RIFF AVI: one `vids` stream, handler and compression MJPG, every frame a keyframe.

        with VideoWriter(path, fps=25) as w:
            w.append(frames)           # device uint8 [F,H,W,3] / [F,H,W] / one frame, or float32 in [0,1] (imageops.frame_to_u8)

    Frames wait on the device until a batch is full -- as many as keep the encoder's workspace under geometry.memory_cap_bytes,
    MAX_BATCH at most -- are coded in one pass and streamed to the file as `00dc` chunks (padded to even length); the host keeps
    eight bytes of index per frame and nothing else.  close() codes what is pending, writes `idx1` and puts the sizes and the frame
    count into the headers.  A file that would pass 2^31 - 1 bytes is refused before the write that would cross it.
    encoder: a callable (frames, quality, subsampling) -> [bytes] in encode_jpeg's place (the container's tests use one); frames
    then only need a shape."""

    def __init__(self, path, fps, quality: int = 90, subsampling: str = "420", encoder: Optional[Callable] = None,
                 max_gb: Optional[float] = None):
        _check_coding(quality, subsampling)
        self.rate, self.scale = _rate_scale(fps)
        self.path, self.quality, self.subsampling, self.max_gb = os.fspath(path), quality, subsampling, max_gb
        self._encoder = encoder
        self.size: Optional[Tuple[int, int]] = None            # (W, H)
        self._channels = None
        self._pending: list = []
        self._pending_frames = 0
        self._batch = None
        self._index = array("I")                               # offset from the `movi` fourcc and size, per frame
        self._largest = 0
        self._file = open(self.path, "wb")
        self._head = len(_avi_header(0, 0, 1, 1, 0, 0, 0, 0))
        self._file.write(b"\x00" * self._head)
        self._pos = self._head                                 # bytes in the file so far; the 2 GB rule is judged on this
        self.closed = False

    frames = property(lambda self: len(self._index) // 2)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close(discard_pending=exc[0] is not None)

    def append(self, frames) -> None:
        if self.closed:
            raise ValueError("VideoWriter.append: the writer is closed")
        if self._encoder is None:
            if isinstance(frames, torch.Tensor) and frames.dtype == torch.float32:
                frame_geometry(frames.shape)
                require_gpu(frames)
                frames = frame_to_u8(frames)
            F, H, W, C = _check_frames(frames)
            require_gpu(frames)
        else:
            F, H, W, C = frame_geometry(frames.shape)
        if self.size is None:
            self.size, self._channels = (W, H), C
        elif self.size != (W, H) or self._channels != C:
            raise ValueError(f"VideoWriter.append: frames of {self.size[0]} x {self.size[1]} with {self._channels} channel(s) so far, "
                             f"got {W} x {H} with {C}")
        self._pending.append(frames.reshape((F, H, W, 3) if C == 3 else (F, H, W)))
        self._pending_frames += F
        if self._batch is None:
            self._batch = self._batch_frames(frames, H, W, C)
        if self._pending_frames >= self._batch:
            self.flush()

    def _batch_frames(self, frames, H, W, C) -> int:
        if self._encoder is not None:
            return 1
        per_frame = workspace_bytes_per_frame(H, W, C, self.subsampling) + H * W * C
        return int(max(1, min(MAX_BATCH, memory_cap_bytes(frames.device, self.max_gb) // per_frame)))

    def flush(self) -> None:
        """code the pending frames, batch by batch, and write their chunks"""
        if not self._pending:
            return
        pending, self._pending, self._pending_frames = self._pending, [], 0
        if self._encoder is not None:
            for frames in pending:
                self._write_chunks(self._encoder(frames, self.quality, self.subsampling))
            return
        frames = pending[0] if len(pending) == 1 else torch.cat(pending)
        for at in range(0, frames.shape[0], self._batch):
            self._write_chunks(encode_jpeg(frames[at:at + self._batch], self.quality, self.subsampling))

    def _write_chunks(self, jpegs: Sequence[bytes]) -> None:
        for data in jpegs:
            chunk = _chunk(b"00dc", data)
            index_after = 8 + 8 * (len(self._index) + 2)
            if self._pos + len(chunk) + index_after > AVI_MAX_BYTES:
                raise MorpheusHipError(f"{self.path}: frame {self.frames} would take the file past 2^31 - 1 bytes; a plain AVI ends "
                                       "there (OpenDML is not written): close this file and start another")
            self._file.write(chunk)
            self._index.extend((self._pos - self._head + 4, len(data)))
            self._largest = max(self._largest, len(data))
            self._pos += len(chunk)

    def close(self, discard_pending: bool = False) -> None:
        if self.closed:
            return
        try:
            if not discard_pending:
                self.flush()
            idx = b"".join(struct.pack("<4sIII", b"00dc", 0x10, self._index[i], self._index[i + 1]) for i in range(0, len(self._index), 2))
            self._file.write(_chunk(b"idx1", idx))
            end = self._pos + 8 + len(idx)
            W, H = self.size or (0, 0)
            self._file.seek(0)
            self._file.write(_avi_header(W, H, self.rate, self.scale, self.frames, self._largest, self._pos - self._head + 4, end - 8))
        finally:
            self.closed = True
            self._file.close()


def write_video(path, frames, fps=25, quality: int = 90, subsampling: str = "420") -> None:
    """imageio.mimwrite's place: frames (a tensor [F,H,W,3] / [F,H,W], or an iterable of frames or batches; device uint8, or
    float32 in [0,1]) -> a Motion-JPEG .avi"""
    with VideoWriter(path, fps, quality, subsampling) as w:
        if isinstance(frames, torch.Tensor):
            w.append(frames)
        else:
            for f in frames:
                w.append(f)


def _chunks(data: bytes, at: int, end: int):
    while at + 8 <= end:
        fourcc, size = data[at:at + 4], struct.unpack_from("<I", data, at + 4)[0]
        yield fourcc, at + 8, size
        at += 8 + size + (size & 1)


def read_video(path):
    """-> (fps, (W, H), [the JPEG file of every frame]) of a Motion-JPEG AVI as VideoWriter writes it; PIL decodes the frames"""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError(f"{path}: not a RIFF AVI file")
    fps, size, frames = None, None, []
    for fourcc, at, n in _chunks(data, 12, 8 + struct.unpack_from("<I", data, 4)[0]):
        kind = data[at:at + 4]
        if fourcc == b"LIST" and kind == b"hdrl":
            for c, a, m in _chunks(data, at + 4, at + n):
                if c == b"avih":
                    size = struct.unpack_from("<II", data, a + 32)
                elif c == b"LIST" and data[a:a + 4] == b"strl":
                    for c2, a2, _m2 in _chunks(data, a + 4, a + m):
                        if c2 == b"strh":
                            if data[a2:a2 + 8] != b"vidsMJPG":
                                raise ValueError(f"{path}: not a Motion-JPEG video stream")
                            scale, rate = struct.unpack_from("<II", data, a2 + 20)
                            fps = rate / scale
        elif fourcc == b"LIST" and kind == b"movi":
            frames = [data[a:a + m] for c, a, m in _chunks(data, at + 4, at + n) if c == b"00dc"]
    if fps is None or size is None:
        raise ValueError(f"{path}: no avih / strh header")
    return fps, (int(size[0]), int(size[1])), frames


def alphanum_key(s: str):
    """tools/vis.py:11-15: "z23a" -> ["z", 23, "a"]"""
    return [int(x) if x.isdigit() else x for x in re.split("([0-9]+)", s)]


def video_frames(names: Sequence[str]) -> List[str]:
    """tools/vis.py:23-26's rule: the names in alphanumeric order, those that contain 'png'.  (The reference removes the others
    from the list it is iterating over, which skips the name behind each removed one; the rule it means is applied here.)"""
    return [n for n in sorted(names, key=alphanum_key) if "png" in n]


def make_video(log_path, video_path, video_name, fps=20, quality: int = 90, subsampling: str = "420", device="cuda") -> str:
    """tools/vis.py:make_video: the PNGs under video_path, in alphanumeric order, -> log_path/video_name.avi.  PIL reads every
    frame; it is uploaded and coded on the device.  -> the path written"""
    _check_coding(quality, subsampling)
    _rate_scale(fps)
    import numpy as np
    from PIL import Image
    os.makedirs(log_path, exist_ok=True)
    out = os.path.join(log_path, video_name + ".avi")
    with VideoWriter(out, fps, quality, subsampling) as w:
        for name in video_frames(os.listdir(video_path)):
            with Image.open(os.path.join(video_path, name)) as im:
                frame = np.asarray(im if im.mode == "L" else im.convert("RGB"))
            w.append(torch.from_numpy(frame.copy()).to(device))
    return out


@torch.no_grad()
def render_test_video(renderer, dataset, save_path, name, fps=25, cano=False, real_view=False, view_360=False, phis=0, scale=1.0,
                      write_video: bool = True, quality: int = 90, subsampling: str = "420") -> List[str]:
    """The loop of MorpheuS.render_test_video (morpheus.py:1285-1336) without its CLIP leg (the CLIP model is the caller's;
    imageops.clip_pair prepares its inputs): for every frame i of `dataset` (a DeviceDataset) the view of get_render_data
    (:1271-1282) -- cano: the canonical shape's orbit; real_view: frame i's camera; view_360: an orbit through time; else frame
    i from the fixed angle phis -- rendered by renderer.eval_step (a HotPathRenderer; model.eval() and an EMA swap are the
    caller's, as they are the trainer's there), converted by imageops.frame_to_u8 / depth_to_u8 and coded from the device:
    save_path/{name}_rgb.avi and {name}_depth.avi, or with write_video=False the two PNGs per frame (:1335-1336).
    Departure: the reference doubles a frame with an odd side because its H.264 writer needs even sizes (:1328-1330); JPEG codes
    any size, so frames keep theirs.  -> the paths written"""
    _check_coding(quality, subsampling)
    _rate_scale(fps)
    os.makedirs(save_path, exist_ok=True)
    n = dataset.num_frames
    written: List[str] = []
    writers = []
    if write_video:
        written = [os.path.join(save_path, f"{name}_rgb.avi"), os.path.join(save_path, f"{name}_depth.avi")]
        writers = [VideoWriter(p, fps, quality, subsampling) for p in written]
    else:
        from PIL import Image
    failed = True
    try:
        for i in range(n):
            if cano:
                data = dataset.get_virtual_view_rays(t=0, is_train=False, phis=i / n)
            elif real_view:
                data = dataset.sample_real_view_rays(idx=i)
            elif view_360:
                data = dataset.get_virtual_view_rays(t=i, is_train=False, phis=i / n, scale=scale)
            else:
                data = dataset.get_virtual_view_rays(t=i, is_train=False, phis=phis)
            preds, preds_depth = renderer.eval_step(data, cano=cano, optimize_pose=bool(real_view))
            pred = frame_to_u8(preds[0].float())
            pred_depth = depth_to_u8(preds_depth[0].float())
            if write_video:
                writers[0].append(pred)
                writers[1].append(pred_depth)
            else:
                for arr, kind in ((pred, "rgb"), (pred_depth, "depth")):
                    written.append(os.path.join(save_path, f"{name}_{i:04d}_{kind}.png"))
                    Image.fromarray(arr.cpu().numpy()).save(written[-1])
        failed = False
    finally:
        for w in writers:
            w.close(discard_pending=failed)
    return written
