"""Sequential numpy restatement of the baseline JPEG encoder of morpheus_amd/csrc/video.hip, written from the definition in that
file's header: int64 numpy for the colour transform, the sub-sampling, the integer DCT and the quantiser; a writer that appends
one bit at a time for the entropy coder; the JFIF header.  It shares the constant tables (morpheus_amd/jpeg_tables.py) with
the product and nothing else: no bit packing, no scan, no header code of morpheus_amd.video is used here.

    encode(frame, quality, subsampling) -> Encoded: .data (the whole file), .scan (the entropy-coded segment before stuffing),
        .bits (its length in bits before the 1-padding), .planes (the padded sample planes), .coefs (the quantised coefficients of
        every component, [by, bx, 8, 8] natural order), .qtabs, .events (what the coverage conditions of the tests count)
    dct_float64 / reconstruct: the float64 forward and inverse DCT the tests judge the integer transform with
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field

import numpy as np

from morpheus_amd import jpeg_tables as T

COS = np.array(T.COS, dtype=np.int64)                                  # [u][x]
ZZ = np.array(T.ZIGZAG)
_u = np.arange(8)
BASIS = np.where(_u[:, None] == 0, np.sqrt(0.5), 1.0) / 2 * np.cos((2 * _u[None, :] + 1) * _u[:, None] * np.pi / 16)   # [u][x]


def pad_edge(plane: np.ndarray, mh: int, mw: int) -> np.ndarray:
    """edge replication up to multiples of (mh, mw)"""
    H, W = plane.shape[:2]
    ph, pw = -H % mh, -W % mw
    return np.pad(plane, ((0, ph), (0, pw)) + ((0, 0),) * (plane.ndim - 2), mode="edge")


def sample_planes(frame: np.ndarray, subsampling: str):
    """uint8 [H,W] or [H,W,3] -> [(plane int64 [8 by, 8 bx], table 0 / 1)] per component, padded to the MCU by edge replication"""
    if frame.ndim == 2:
        return [(pad_edge(frame.astype(np.int64), 8, 8), 0)]
    m = 16 if subsampling == "420" else 8
    rgb = pad_edge(frame.astype(np.int64), m, m)
    ycc = [(c[0] * rgb[..., 0] + c[1] * rgb[..., 1] + c[2] * rgb[..., 2] + c[3]) >> 16 for c in T.YCC]
    assert all(0 <= p.min() and p.max() <= 255 for p in ycc)
    if subsampling == "420":
        for k in (1, 2):
            p = ycc[k]
            ycc[k] = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2
    return [(ycc[0], 0), (ycc[1], 1), (ycc[2], 1)]


def to_blocks(plane: np.ndarray) -> np.ndarray:
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)            # [by, bx, y, x]


def dct_int(blocks: np.ndarray) -> np.ndarray:
    """level-shifted samples [..., y, x] -> the integer transform's coefficients [..., v, u], 2^OUT_BITS times the DCT"""
    s = blocks.astype(np.int64) - 128
    rows = np.einsum("ux,...yx->...yu", COS, s)
    assert np.abs(rows).max() < 2 ** 31
    rows = (rows + (1 << (T.ROW_SHIFT - 1))) >> T.ROW_SHIFT
    out = np.einsum("vy,...yu->...vu", COS, rows)
    assert np.abs(out).max() < 2 ** 31
    return out


def quantise(F: np.ndarray, q: np.ndarray) -> np.ndarray:
    """round half away from zero on the magnitude: sign(F) * ((|F| + D / 2) // D), D = Q 2^OUT_BITS"""
    D = q.reshape(8, 8).astype(np.int64) << T.OUT_BITS
    mag = (np.abs(F) + (D >> 1)) // D
    assert (np.abs(F) + (D >> 1)).max() < 2 ** 31
    return np.sign(F) * mag


def dct_float64(blocks: np.ndarray) -> np.ndarray:
    s = blocks.astype(np.float64) - 128.0
    return np.einsum("vy,...yx,ux->...vu", BASIS, s, BASIS)


def idct_float64(coefs: np.ndarray) -> np.ndarray:
    return np.einsum("vy,...vu,ux->...yx", BASIS, coefs.astype(np.float64), BASIS) + 128.0


class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, value: int, length: int):
        for i in range(length - 1, -1, -1):
            self.bits.append((value >> i) & 1)


def category(v: int) -> int:
    return int(abs(v)).bit_length()


def value_bits(v: int, cat: int) -> int:
    return v if v >= 0 else v + (1 << cat) - 1


@dataclass
class Encoded:
    data: bytes = b""
    scan: bytes = b""
    bits: int = 0
    planes: list = field(default_factory=list)
    coefs: list = field(default_factory=list)
    qtabs: list = field(default_factory=list)
    events: dict = field(default_factory=dict)


def code_block(w: BitWriter, zz, pred: int, dc_tab, ac_tab, ev: dict):
    """one block, zz = its 64 quantised coefficients in zigzag order"""
    diff = max(-2047, min(2047, int(zz[0]) - pred))
    cat = category(diff)
    ev["max_dc_cat"] = max(ev["max_dc_cat"], cat)
    code, length = dc_tab[cat]
    w.put(code, length)
    w.put(value_bits(diff, cat), cat)
    run, ac_symbols = 0, 0
    for k in range(1, 64):
        v = max(-1023, min(1023, int(zz[k])))
        if v == 0:
            run += 1
            continue
        while run > 15:
            w.put(*ac_tab[T.ZRL])
            ev["zrl"] += 1
            ev["max_code_len"] = max(ev["max_code_len"], ac_tab[T.ZRL][1])
            run -= 16
        cat = category(v)
        code, length = ac_tab[(run << 4) | cat]
        ev["max_code_len"] = max(ev["max_code_len"], length)
        w.put(code, length)
        w.put(value_bits(v, cat), cat)
        run, ac_symbols = 0, ac_symbols + 1
    if run:
        w.put(*ac_tab[T.EOB])
        if ac_symbols == 0:
            ev["eob_only"] += 1
    else:
        ev["coef63"] += 1


def header(H: int, W: int, ncomp: int, subsampling: str, qtabs) -> bytes:
    def seg(marker, payload):
        return b"\xff" + bytes([marker]) + struct.pack(">H", len(payload) + 2) + payload
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, q in enumerate(qtabs):
        out += seg(0xDB, bytes([i]) + bytes(int(q[z]) for z in T.ZIGZAG))
    comps = [(1, 0x22 if (ncomp == 3 and subsampling == "420") else 0x11, 0)] + [(2, 0x11, 1), (3, 0x11, 1)][:ncomp - 1]
    out += seg(0xC0, struct.pack(">BHHB", 8, H, W, ncomp) + b"".join(bytes(c) for c in comps))
    for t in range(len(qtabs)):
        out += seg(0xC4, bytes([t]) + bytes(T.DC_BITS[t]) + bytes(T.DC_VALS[t]))
        out += seg(0xC4, bytes([0x10 | t]) + bytes(T.AC_BITS[t]) + bytes(T.AC_VALS[t]))
    out += seg(0xDA, bytes([ncomp]) + b"".join(bytes([c[0], c[2] * 0x11]) for c in comps) + b"\x00\x3f\x00")
    return out


def encode(frame: np.ndarray, quality: int = 90, subsampling: str = "420") -> Encoded:
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and (frame.ndim == 2 or (frame.ndim == 3 and frame.shape[2] == 3))
    H, W = frame.shape[:2]
    r = Encoded()
    planes = sample_planes(frame, subsampling)
    ncomp = len(planes)
    r.qtabs = [np.array(T.quant_table(quality, t), dtype=np.int64) for t in range(2 if ncomp == 3 else 1)]
    for plane, t in planes:
        r.planes.append(plane)
        r.coefs.append(quantise(dct_int(to_blocks(plane)), r.qtabs[t]))
    dc = [T.huffman_codes(T.DC_BITS[t], T.DC_VALS[t]) for t in (0, 1)]
    ac = [T.huffman_codes(T.AC_BITS[t], T.AC_VALS[t]) for t in (0, 1)]
    ev = r.events = {"zrl": 0, "max_code_len": 0, "max_dc_cat": 0, "eob_only": 0, "coef63": 0, "stuffed": 0}
    w = BitWriter()
    pred = [0] * ncomp
    two = ncomp == 3 and subsampling == "420"
    mcuy, mcux = r.coefs[-1].shape[:2]                               # the last component has one block per MCU in every layout
    for my in range(mcuy):
        for mx in range(mcux):
            for c in range(ncomp):
                t = planes[c][1]
                n = 2 if (two and c == 0) else 1
                for j in range(n * n):
                    blk = r.coefs[c][my * n + j // n, mx * n + j % n]
                    code_block(w, blk.reshape(64)[ZZ], pred[c], dc[t], ac[t], ev)
                    pred[c] = int(blk[0, 0])
    r.bits = len(w.bits)
    bits = w.bits + [1] * (-r.bits % 8)
    r.scan = bytes(int("".join(map(str, bits[i:i + 8])), 2) for i in range(0, len(bits), 8))
    ev["stuffed"] = r.scan.count(b"\xff")
    r.data = header(H, W, ncomp, subsampling, r.qtabs) + r.scan.replace(b"\xff", b"\xff\x00") + b"\xff\xd9"
    return r


def reconstruct(r: Encoded):
    """the float64 dequantise + inverse DCT of the coded coefficients -> one float64 plane per component (padded size)"""
    out = []
    for c, coefs in enumerate(r.coefs):
        q = r.qtabs[0 if c == 0 else 1].reshape(8, 8)
        px = idct_float64(coefs * q)
        by, bx = coefs.shape[:2]
        out.append(px.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8))
    return out


# ---- the case list the host and the GPU tests share --------------------------------------------------------------------------
def _yx(H, W):
    return np.mgrid[0:H, 0:W]


def sine(H=37, W=75):
    y, x = _yx(H, W)
    return (127 + 100 * np.sin(x / 9) * np.cos(y / 7)).astype(np.uint8)


def checker(H=37, W=75):
    y, x = _yx(H, W)
    return (((x // 8 + y // 8) % 2) * 255).astype(np.uint8)


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def shaded(H, W):
    """a rendered-looking RGB frame: smooth shading, a dark disc with a hard edge, a little grain"""
    y, x = _yx(H, W)
    base = np.stack([120 + 90 * np.sin(x / 37.0 + y / 11.0), 128 + 70 * np.cos(x / 23.0), 90 + 0.1 * x + 2 * y], -1)
    base[(x - 0.4 * W) ** 2 + (2 * (y - 0.5 * H)) ** 2 < (0.8 * H) ** 2] *= 0.35
    return np.clip(base + noise((H, W, 3), 7) % 5, 0, 255).astype(np.uint8)


def rgb_of(gray):
    return np.stack([gray, gray[::-1], 255 - gray], -1)


def cases():
    """-> {name: (frames uint8 [F,H,W] or [F,H,W,3], quality, subsampling)}: every size at which the kernels take another path
    (one pixel, one block, one MCU, edge padding on both axes, a scan across a wavefront and across a workgroup, several frames)
    and the contents that reach every branch of the entropy coder"""
    const = np.full((37, 75), 93, np.uint8)
    return {
        "gray_1x1": (np.full((1, 1, 1), 200, np.uint8), 90, "420"),
        "gray_8x8": (noise((1, 8, 8), 1), 90, "420"),
        "rgb_16x16_420": (shaded(16, 16)[None], 90, "420"),
        "rgb_17x23_420": (noise((1, 17, 23, 3), 2), 50, "420"),
        "rgb_17x23_444": (noise((1, 17, 23, 3), 3), 100, "444"),
        "gray_24x520": (sine(24, 520)[None], 90, "420"),
        "rgb_40x1048_420": (shaded(40, 1048)[None], 90, "420"),
        "gray_checker_q100": (checker()[None], 100, "420"),
        "gray_sine_q100": (sine()[None], 100, "420"),
        "rgb_noise_q100_444": (noise((1, 37, 75, 3), 4), 100, "444"),
        "batch_gray_q100": (np.stack([const, noise((37, 75), 5), sine()]), 100, "420"),
        "batch_rgb_q50_420": (np.stack([rgb_of(const), noise((37, 75, 3), 6), rgb_of(sine())]), 50, "420"),
    }


_ENCODED = {}


def encoded(name):
    """the oracle's result for every frame of a case, computed once"""
    if name not in _ENCODED:
        frames, quality, sub = cases()[name]
        _ENCODED[name] = [encode(f, quality, sub) for f in frames]
    return _ENCODED[name]


def psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return np.inf if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)
