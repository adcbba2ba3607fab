"""GPU: morpheus_amd.video's encoder (csrc/video.hip) against its sequential restatement tests/video_oracle.py -- the same bytes,
header included, for every case of the shared list (tests/test_video_host.py judges that restatement against PIL) -- the
capacity clamp of the raw entry point, and the writers on device frames: write_video, make_video, render_all_meshes(video_path=)
and render_test_video, read back through read_video and PIL."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from tests import raster_oracle as ro
from tests import video_oracle as vo
from tests.test_video_host import PSNR_MARGIN_DB, pil_jpeg

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = vo.cases()


def stuffed(r):
    return r.scan.replace(b"\xff", b"\xff\x00")


def decode(jpeg):
    return np.asarray(Image.open(io.BytesIO(jpeg)))


def assert_quality_is_pils(jpeg, frame, quality=90, sub="420"):
    """the host test's rule: the decoded frame is no further from its source than PIL's own encoding, less the margin"""
    got = decode(jpeg)
    assert got.shape == frame.shape
    ours, pils = vo.psnr(got, frame), vo.psnr(decode(pil_jpeg(frame, quality, sub)), frame)
    assert ours >= pils - PSNR_MARGIN_DB, (ours, pils)


@pytest.mark.parametrize("name", list(CASES))
def test_bytes_equal_the_oracle(name):
    from morpheus_amd import video
    frames, quality, sub = CASES[name]
    dev = torch.from_numpy(frames).to(DEV)
    got = video.encode_jpeg(dev, quality, sub)
    want = [r.data for r in vo.encoded(name)]
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        assert a == b, f"{name} frame {k}: {len(a)} bytes against {len(b)}, first difference at byte {first}"
    assert video.encode_jpeg(dev, quality, sub) == got                                  # the same bytes on every run
    out, counts = video.encode_scans(dev, quality, sub)
    counts = counts.cpu().tolist()
    assert counts[-1] == 0 and counts[:-1] == [len(stuffed(r)) for r in vo.encoded(name)]   # no overflow at the proven capacity


def test_a_single_frame_is_a_batch_of_one():
    from morpheus_amd import video
    frames, quality, sub = CASES["rgb_17x23_444"]
    assert video.encode_jpeg(torch.from_numpy(frames[0]).to(DEV), quality, sub) == [vo.encoded("rgb_17x23_444")[0].data]
    gray = CASES["gray_8x8"][0]
    assert video.encode_jpeg(torch.from_numpy(gray[0]).to(DEV), 90) == [vo.encoded("gray_8x8")[0].data]


@pytest.mark.parametrize("name,cap", [("rgb_noise_q100_444", 64), ("batch_gray_q100", 512)])
def test_a_capacity_too_small_is_reported_and_respected(name, cap):
    """a legal argument of the raw entry point: every write stays inside out[f][0 .. cap), the flag is raised, and a frame that
    does fit is still coded right"""
    from morpheus_amd import video
    frames, quality, sub = CASES[name]
    F = frames.shape[0]
    guard = 4096
    out = torch.full((F * cap + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    _, counts = video.encode_scans(torch.from_numpy(frames).to(DEV), quality, sub, cap=cap, out=out)
    counts, host = counts.cpu().tolist(), out.cpu().numpy()
    assert counts[-1] == 1 and all(0 <= c <= cap for c in counts[:-1])
    assert (host[F * cap:] == 0xA5).all()
    fitted = 0
    for f, r in enumerate(vo.encoded(name)):
        # the packed segment is cut at cap / 2 bytes, its stuffed form at cap: what is inside is still the oracle's
        want = r.scan[:cap // 2].replace(b"\xff", b"\xff\x00")[:cap]
        assert counts[f] == len(want) and bytes(host[f * cap:f * cap + counts[f]]) == want, f
        fitted += want == stuffed(r)
    assert fitted == (1 if F > 1 else 0)                                 # the constant frame of the batch fits, the others do not


def test_write_video_round_trip(tmp_path):
    from morpheus_amd import imageops, video
    frames, quality, sub = CASES["batch_rgb_q50_420"]
    dev = torch.from_numpy(frames).to(DEV)
    jpegs = video.encode_jpeg(dev, quality, sub)
    video.write_video(tmp_path / "a.avi", dev, fps=25, quality=quality, subsampling=sub)
    fps, size, got = video.read_video(tmp_path / "a.avi")
    assert (fps, size) == (25.0, (75, 37)) and got == jpegs
    for jpeg in got:
        im = Image.open(io.BytesIO(jpeg))
        assert im.mode == "RGB" and im.size == (75, 37)
    # one frame at a time, grey, float32 in [0, 1]: the frames of imageops.frame_to_u8
    gray = torch.from_numpy(CASES["batch_gray_q100"][0]).to(DEV).float() / 255
    video.write_video(tmp_path / "b.avi", list(gray), fps=12.5)
    fps, size, got = video.read_video(tmp_path / "b.avi")
    assert (fps, size) == (12.5, (75, 37)) and got == video.encode_jpeg(imageops.frame_to_u8(gray))
    assert all(Image.open(io.BytesIO(j)).mode == "L" for j in got)
    video.write_jpeg(tmp_path / "c.jpg", dev[2], quality, sub)
    assert (tmp_path / "c.jpg").read_bytes() == jpegs[2]


def test_make_video_reads_the_pngs_in_order(tmp_path):
    from morpheus_amd import video
    src = tmp_path / "frames"
    src.mkdir()
    frames = {"10.png": vo.shaded(20, 28), "2.png": vo.rgb_of(vo.sine(20, 28)), "1.png": vo.noise((20, 28, 3), 11)}
    for name, f in frames.items():
        Image.fromarray(f).save(src / name)
    (src / "notes.txt").write_text("not a frame")
    path = video.make_video(str(tmp_path / "log"), str(src), "video_real_test")
    assert path.endswith("video_real_test.avi")
    fps, size, got = video.read_video(path)
    assert (fps, size, len(got)) == (20.0, (28, 20), 3)
    for jpeg, name in zip(got, ("1.png", "2.png", "10.png")):
        assert jpeg == video.encode_jpeg(torch.from_numpy(frames[name]).to(DEV))[0]


def test_render_all_meshes_writes_the_video(tmp_path):
    from morpheus_amd import meshrender, video
    v = torch.tensor([[0.5, 0.5, 0.5], [0.5, -0.5, -0.5], [-0.5, 0.5, -0.5], [-0.5, -0.5, 0.5]], device=DEV)
    t = torch.tensor([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], device=DEV)
    meshes = [{"vertices": v, "triangles": t}, {"vertices": (v * 0.7).contiguous(), "triangles": t}]
    poses = [ro.look_at((2.4, 0.3 * i, 0.5)) for i in range(2)]
    K = np.array([[40.0, 0, 16.0], [0, 40.0, 16.0], [0, 0, 1]])
    plain = meshrender.render_all_meshes(meshes, poses, K, 32, 32, scale=1)
    res = meshrender.render_all_meshes(meshes, poses, K, 32, 32, save_images_dir=str(tmp_path / "img"), scale=1,
                                       video_path=str(tmp_path / "video_real_0001.avi"), fps=20)
    assert all(np.array_equal(res[k], plain[k]) for k in plain)                          # nothing else changes
    fps, size, got = video.read_video(tmp_path / "video_real_0001.avi")
    assert (fps, size, len(got)) == (20.0, (32, 32), 2)
    for i, jpeg in enumerate(got):
        png = np.asarray(Image.open(tmp_path / "img" / f"{i:04d}.png"))
        assert png.std() > 0                                                             # the tetrahedron is in view
        assert_quality_is_pils(jpeg, png)


def test_render_test_video_on_a_synthetic_dataset(tmp_path):
    from morpheus_amd import harness, imageops, synth, video
    from morpheus_amd.dataset import DeviceDataset
    from tests import dataset_oracle as D
    n, hw = 2, 16
    rng = np.random.default_rng(5)
    radius, theta, phi = np.array([2.0, 2.2]), np.array([70.0, 80.0]), np.array([10.0, 30.0])
    th, ph = np.deg2rad(theta), np.deg2rad(phi)
    centres = np.stack([radius * np.sin(th) * np.sin(ph), radius * np.cos(th), radius * np.sin(th) * np.cos(ph)], -1)
    K = np.array([[18.0, 0.0, 8.0], [0.0, 18.0, 8.0], [0.0, 0.0, 1.0]])
    ds = DeviceDataset(D.CONFIG, rng.integers(0, 256, (n, hw, hw, 3), dtype=np.uint8),
                       rng.integers(300, 4000, (n, hw, hw)).astype(np.uint16), np.full((n, hw, hw), 255, np.uint8),
                       D.look_at_np(centres).astype(np.float32), K, radius, theta, phi, device=DEV, is_train=False)
    model = harness.build_model("b", DEV).eval()                       # its code tables hold 200 frames; the dataset uses two
    rend = harness.make_renderer(model, 24, jitter=synth.ray_jitter(hw * hw).to(DEV))                     # pinned: renders repeat
    paths = video.render_test_video(rend, ds, str(tmp_path), "test_ep0001", fps=25, phis=0.1)
    assert [p.rsplit("/", 1)[1] for p in paths] == ["test_ep0001_rgb.avi", "test_ep0001_depth.avi"]
    (fps, size, rgb), (_, dsize, depth) = video.read_video(paths[0]), video.read_video(paths[1])
    assert fps == 25.0 and size == dsize == (hw, hw) and len(rgb) == len(depth) == n
    for i in range(n):
        with torch.no_grad():
            preds, pd = rend.eval_step(ds.get_virtual_view_rays(t=i, is_train=False, phis=0.1))
        assert_quality_is_pils(rgb[i], imageops.frame_to_u8(preds[0]).cpu().numpy())
        assert_quality_is_pils(depth[i], imageops.depth_to_u8(pd[0]).cpu().numpy())
        assert Image.open(io.BytesIO(depth[i])).mode == "L"
    pngs = video.render_test_video(rend, ds, str(tmp_path / "png"), "t", phis=0.1, write_video=False)
    assert len(pngs) == 2 * n and Image.open(pngs[0]).size == (hw, hw) and Image.open(pngs[1]).mode == "L"
