"""CPU (no GPU): the JPEG restatement (tests/video_oracle.py) and the host code of morpheus_amd/video.py judged against PIL --
tables, decodability, decoded pixels, quality against PIL's own encoder, the coefficient bound of the integer DCT -- plus the
coverage the shared case list must have, the AVI container, the argument checks and the plumbing of the new entry points."""
import importlib.util
import io
import os
import re
import struct

import numpy as np
import pytest
import torch
from PIL import Image

from morpheus_amd import jpeg_tables as T
from tests import video_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = vo.cases()
PIL_SUB = {"420": 2, "444": 0}
PSNR_MARGIN_DB = 0.5          # three times the 0.17 dB two correct encoders (PIL, a float64-DCT one) were seen to disagree by
DCT_EPS = 0.25                # csrc/video.hip, `error`: |F 2^-19 - c| <= 0.25


def pil_jpeg(frame, quality, sub) -> bytes:
    b = io.BytesIO()
    Image.fromarray(frame).save(b, "JPEG", quality=quality, subsampling=PIL_SUB[sub], optimize=False)
    return b.getvalue()


def segments(data: bytes):
    """-> [(marker, payload)] up to and including SOS"""
    assert data[:2] == b"\xff\xd8"
    at, out = 2, []
    while True:
        assert data[at] == 0xFF
        marker, n = data[at + 1], struct.unpack_from(">H", data, at + 2)[0]
        out.append((marker, data[at + 4:at + 2 + n]))
        at += 2 + n
        if marker == 0xDA:
            return out


# ---- tables ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", [10, 50, 75, 90, 100])
def test_quantisation_tables_are_pils(quality):
    q = Image.open(io.BytesIO(pil_jpeg(vo.noise((16, 16, 3), 0), quality, "420"))).quantization
    for t in (0, 1):
        assert list(q[t]) == list(T.quant_table(quality, t)), (quality, t)            # natural order on both sides


def test_huffman_tables_are_the_ones_pil_writes():
    found = {}
    for marker, p in segments(pil_jpeg(vo.noise((16, 16, 3), 0), 75, "420")):
        while marker == 0xC4 and p:
            n = sum(p[1:17])
            found[p[0]] = (tuple(p[1:17]), tuple(p[17:17 + n]))
            p = p[17 + n:]
    for t in (0, 1):
        assert found[t] == (T.DC_BITS[t], T.DC_VALS[t])
        assert found[0x10 | t] == (T.AC_BITS[t], T.AC_VALS[t])


def test_table_file_is_the_generator_output():
    spec = importlib.util.spec_from_file_location("gen_jpeg_tables", os.path.join(ROOT, "tools", "gen_jpeg_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert open(gen.OUT).read() == gen.render()
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    exact = (1 << T.COS_BITS) * np.where(u == 0, np.sqrt(0.5), 1.0) / 2 * np.cos((2 * x + 1) * u * np.pi / 16)
    assert np.abs(np.array(T.COS) - exact).max() <= 0.5 + 1e-9
    assert sorted(T.ZIGZAG) == list(range(64)) and T.ZIGZAG[:6] == (0, 1, 8, 16, 9, 2) and T.ZIGZAG[-1] == 63


# ---- the oracle against PIL -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_pil_decodes_every_stream(name):
    frames, quality, sub = CASES[name]
    for frame, r in zip(frames, vo.encoded(name)):
        im = Image.open(io.BytesIO(r.data))
        im.load()
        rgb = frame.ndim == 3
        assert im.mode == ("RGB" if rgb else "L") and im.size == (frame.shape[1], frame.shape[0])
        h = 2 if (rgb and sub == "420") else 1
        assert [layer[:3] for layer in im.layer] == ([(1, h, h), (2, 1, 1), (3, 1, 1)] if rgb else [(1, 1, 1)])
        assert r.data.endswith(b"\xff\xd9") and len(r.scan) == -(-r.bits // 8)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c[0].ndim == 3 or c[2] == "444"])
def test_decoded_pixels_are_within_one_level(name):
    """grey and 4:4:4: PIL's decoder without colour conversion against the float64 inverse DCT of the same coefficients"""
    frames, quality, sub = CASES[name]
    for frame, r in zip(frames, vo.encoded(name)):
        im = Image.open(io.BytesIO(r.data))
        if frame.ndim == 3:
            im.draft("YCbCr", None)
            assert im.mode == "YCbCr"
        got = np.asarray(im).astype(np.int64).reshape(frame.shape)
        H, W = frame.shape[:2]
        want = np.stack([np.rint(np.clip(p, 0, 255))[:H, :W] for p in vo.reconstruct(r)], -1).reshape(frame.shape)
        assert np.abs(got - want).max() <= 1, (name, np.abs(got - want).max())


@pytest.mark.parametrize("name", list(CASES))
def test_quality_is_pils_own(name):
    frames, quality, sub = CASES[name]
    for frame, r in zip(frames, vo.encoded(name)):
        ours = vo.psnr(np.asarray(Image.open(io.BytesIO(r.data))), frame)
        pils = vo.psnr(np.asarray(Image.open(io.BytesIO(pil_jpeg(frame, quality, sub)))), frame)
        print(f"{name}: oracle {ours:.2f} dB, PIL {pils:.2f} dB, bytes {len(r.data)} / {len(pil_jpeg(frame, quality, sub))}")
        assert ours >= pils - PSNR_MARGIN_DB, (name, ours, pils)


@pytest.mark.parametrize("name", list(CASES))
def test_coefficients_round_the_float64_dct(name):
    for r in vo.encoded(name):
        for c, (plane, coefs) in enumerate(zip(r.planes, r.coefs)):
            Q = r.qtabs[min(c, 1)].reshape(8, 8)
            exact = vo.dct_float64(vo.to_blocks(plane))
            assert np.abs(vo.dct_int(vo.to_blocks(plane)) / 2.0 ** T.OUT_BITS - exact).max() <= DCT_EPS
            assert (np.abs(coefs * Q - exact) <= Q / 2 + DCT_EPS).all(), (name, c)


def test_the_case_list_reaches_every_branch_of_the_coder():
    ev = [r.events for n in CASES for r in vo.encoded(n)]
    assert any(e["zrl"] for e in ev)
    assert any(e["max_code_len"] == 16 for e in ev)
    assert any(e["stuffed"] for e in ev)
    assert any(e["max_dc_cat"] == 11 for e in ev)
    assert any(e["eob_only"] for e in ev)
    assert any(e["coef63"] for e in ev)
    assert any(r.bits % 8 for n in CASES for r in vo.encoded(n))
    for n in CASES:
        for r in vo.encoded(n):
            assert r.data.count(b"\xff\x00") >= r.events["stuffed"]


def test_header_of_the_python_face_is_the_oracles():
    from morpheus_amd import video
    for C, sub, q in ((1, "420", 90), (3, "420", 50), (3, "444", 100)):
        qt = [np.array(T.quant_table(q, t)) for t in range(2 if C == 3 else 1)]
        assert video.jpeg_header(17, 23, C, q, sub) == vo.header(17, 23, C, sub, qt)


# ---- the AVI container ------------------------------------------------------------------------------------------------------------
def _stub(blobs):
    return lambda frames, quality, subsampling: [blobs[int(f.reshape(-1)[0])] for f in frames]


def test_avi_round_trip_index_and_headers(tmp_path):
    from morpheus_amd import video
    blobs = [b"\xff\xd8abc", b"\xff\xd8defg" * 3, b"\xff\xd8h", b"\xff\xd8ij"]                 # odd and even lengths
    path = tmp_path / "a.avi"
    with video.VideoWriter(path, 12.5, encoder=_stub(blobs)) as w:
        w.append(np.array([0, 1], np.uint8).reshape(2, 1, 1) * np.ones((1, 6, 10), np.uint8))
        for i in (2, 3):
            w.append(np.full((6, 10), i, np.uint8))
        with pytest.raises(ValueError):
            w.append(np.zeros((6, 11), np.uint8))
    fps, size, frames = video.read_video(path)
    assert (fps, size, frames) == (12.5, (10, 6), blobs)
    data = path.read_bytes()
    assert len(data) % 2 == 0 and struct.unpack_from("<I", data, 4)[0] == len(data) - 8
    movi = data.index(b"movi")
    assert struct.unpack_from("<I", data, movi - 4)[0] == data.index(b"idx1") - movi
    idx = data.index(b"idx1")
    n = struct.unpack_from("<I", data, idx + 4)[0]
    assert n == 16 * len(blobs) and idx + 8 + n == len(data)
    for k, blob in enumerate(blobs):
        fourcc, flags, off, size_k = struct.unpack_from("<4sIII", data, idx + 8 + 16 * k)
        assert (fourcc, flags, size_k) == (b"00dc", 0x10, len(blob))
        assert data[movi + off:movi + off + 8] == b"00dc" + struct.pack("<I", len(blob))
        assert data[movi + off + 8:movi + off + 8 + len(blob)] == blob
        assert (movi + off) % 2 == 0                                                            # odd chunks are padded
    avih = data.index(b"avih") + 8
    usec, _, _, flags, total, _, streams, _, W, H = struct.unpack_from("<10I", data, avih)
    assert (usec, flags, total, streams, W, H) == (80000, 0x10, 4, 1, 10, 6)
    strh = data.index(b"strh") + 8
    assert data[strh:strh + 8] == b"vidsMJPG"
    scale, rate, _, length = struct.unpack_from("<4I", data, strh + 20)
    assert (rate, scale, length) == (25, 2, 4)
    strf = data.index(b"strf") + 8
    assert struct.unpack_from("<IiiHH4s", data, strf) == (40, 10, 6, 1, 24, b"MJPG")


def test_avi_refuses_to_pass_two_gigabytes(tmp_path):
    from morpheus_amd import video
    from morpheus_amd._lib import MorpheusHipError
    path = tmp_path / "big.avi"
    w = video.VideoWriter(path, 25, encoder=_stub([b"x" * 100]))
    w.append(np.zeros((4, 4), np.uint8))
    w._pos = video.AVI_MAX_BYTES - 8 - 16 * 2 - 108 + 1                  # one byte short of room for the chunk and the index
    w._file.flush()
    before = os.path.getsize(path)
    with pytest.raises(MorpheusHipError, match="2\\^31"):
        w.append(np.zeros((4, 4), np.uint8))
    w._file.flush()
    assert os.path.getsize(path) == before and w.frames == 1             # refused before the write
    w._pos -= 1
    w.append(np.zeros((4, 4), np.uint8))                                 # with exactly enough room it is written
    assert w.frames == 2
    w._file.close()


def test_make_video_orders_and_filters_like_the_reference():
    from morpheus_amd import video
    names = ["10.png", "9.png", "notes.txt", "a2b.png", "a10b.png", "1.jpg", "png_list.csv"]
    key = lambda s: [int(x) if x.isdigit() else x for x in re.split("([0-9]+)", s)]      # noqa: E731  (tools/vis.py:11-15)
    want = [n for n in sorted(names, key=key) if "png" in n]
    assert video.video_frames(names) == want == ["9.png", "10.png", "a2b.png", "a10b.png", "png_list.csv"]


# ---- argument checks before a device is asked for -----------------------------------------------------------------------------
def test_arguments_are_checked_before_a_device_is_asked_for(tmp_path, monkeypatch):
    from morpheus_amd import _lib, video

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(video, "launch", no_device)
    monkeypatch.setattr(video, "require_gpu", no_device)
    ok = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    for bad in (dict(quality=0), dict(quality=101), dict(quality=90.0), dict(quality=True), dict(subsampling="422"),
                dict(subsampling=420)):
        with pytest.raises(ValueError):
            video.encode_jpeg(ok, **bad)
        with pytest.raises(ValueError):
            video.write_jpeg(tmp_path / "x.jpg", ok[0], **bad)
        with pytest.raises(ValueError):
            video.VideoWriter(tmp_path / "x.avi", 25, **bad)
        with pytest.raises(ValueError):
            video.write_video(tmp_path / "x.avi", ok, **bad)
        with pytest.raises(ValueError):
            video.make_video(tmp_path, tmp_path, "x", **bad)
        with pytest.raises(ValueError):
            video.render_test_video(None, None, tmp_path, "x", **bad)
    for frames in (ok.float(), ok.numpy(), torch.zeros(2, 8, 8, 4, dtype=torch.uint8), torch.zeros(0, 8, 8, dtype=torch.uint8),
                   torch.zeros(8, dtype=torch.uint8), torch.zeros(1, 1, 1, 8, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            video.encode_jpeg(frames)
    with pytest.raises(ValueError):
        video.write_jpeg(tmp_path / "x.jpg", ok)                          # a batch is not one image
    for fps in (0, -1):
        with pytest.raises(ValueError):
            video.VideoWriter(tmp_path / "x.avi", fps)
        with pytest.raises(ValueError):
            video.make_video(tmp_path, tmp_path, "x", fps=fps)
        with pytest.raises(ValueError):
            video.render_test_video(None, None, tmp_path, "x", fps=fps)
    with video.VideoWriter(tmp_path / "y.avi", 25) as w:
        for frames in (torch.zeros(2, 8, 8, dtype=torch.int16), torch.zeros(8, dtype=torch.float32)):
            with pytest.raises(ValueError):
                w.append(frames)
    with pytest.raises(ValueError):
        video.read_video(__file__)


def test_cpu_tensors_are_refused():
    from morpheus_amd import video
    from morpheus_amd._lib import MorpheusHipError
    with pytest.raises(MorpheusHipError):
        video.encode_jpeg(torch.zeros(8, 8, dtype=torch.uint8))


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
NAMES = ("mh_jpeg_blocks", "mh_jpeg_scan_capacity", "mh_jpeg_workspace_bytes", "mh_jpeg_quant_table", "mh_jpeg_encode")


def test_entry_points_are_declared_once_and_built():
    from morpheus_amd import _lib, build
    text = open(build.HEADER).read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NAMES:
        assert len(re.findall(rf"\b{name}\s*\(", code)) == 1 and name in _lib.EXPORTS
    assert re.search(r"#define MH_ABI_VERSION 10\b", text)
    assert "video.hip" in build.SOURCES and "video.hip" not in build.FILE_FLAGS
    source = open(os.path.join(build.CSRC, "video.hip")).read()
    assert "float" not in re.sub(r"//[^\n]*", "", source) and "double" not in re.sub(r"//[^\n]*", "", source)
    assert "asm" not in source and "fp contract" not in source


def test_host_only_queries():
    import ctypes
    from morpheus_amd import _lib, build
    build.build()
    lib = _lib.load()
    assert lib.mh_jpeg_blocks(17, 23, 1, 420) == 9 and lib.mh_jpeg_blocks(17, 23, 3, 444) == 27
    assert lib.mh_jpeg_blocks(17, 23, 3, 420) == 24 and lib.mh_jpeg_blocks(1440, 1440, 3, 420) == 90 * 90 * 6
    for bad in ((0, 8, 1, 420), (8, 65536, 1, 420), (8, 8, 2, 420), (8, 8, 3, 422), (65535, 65535, 3, 444)):
        assert lib.mh_jpeg_blocks(*bad) == -1, bad
    assert T.MAX_BLOCK_BITS == 1658
    for blocks in (1, 6, 1188, 48600):
        cap = lib.mh_jpeg_scan_capacity(blocks)
        assert cap % 32 == 0 and cap // 2 >= -(-blocks * 1658 // 8) and cap // 2 - 16 < -(-blocks * 1658 // 8)
        assert lib.mh_jpeg_workspace_bytes(2, blocks, cap) >= 2 * (blocks * 128 + cap // 2)
        assert lib.mh_jpeg_workspace_bytes(2, blocks, cap + 8) == -1 and lib.mh_jpeg_workspace_bytes(0, blocks, cap) == -1
    assert lib.mh_jpeg_scan_capacity(0) == -1 and lib.mh_jpeg_scan_capacity((2 ** 31 - 1) // 1658 + 1) == -1
    table = (ctypes.c_int32 * 64)()
    for quality in (1, 10, 49, 50, 75, 90, 100):
        for t in (0, 1):
            assert lib.mh_jpeg_quant_table(quality, t, table) == 0 and tuple(table) == T.quant_table(quality, t)
    assert lib.mh_jpeg_quant_table(0, 0, table) == 1 and lib.mh_jpeg_quant_table(50, 2, table) == 1
    # bad arguments return before anything is launched (no device is needed to see it)
    assert _lib._fns["mh_jpeg_encode"](None, 1, 8, 8, 1, 420, 90, None, None, 64, None, None, None) == 1
