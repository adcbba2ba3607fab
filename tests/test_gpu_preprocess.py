"""GPU: csrc/preprocess.hip (`ops.prep_frames`, `morpheus_amd.preprocess`, `DeviceDataset.from_raw`) against the reference's own
results (tests/golden/preprocess.npz) and, where the reference cannot run or cv2 would be needed, against tests/preprocess_oracle.py.

Every comparison is BIT FOR BIT on all four planes: the kernel copies bytes, looks depth up in tables made on the host, and for
rotated frames follows the oracle's float64 order of operations without contraction.
"""
import numpy as np
import pytest
import torch

from tests import preprocess_oracle as P
from tests.test_preprocess_host import inputs, run_scale, write_raw_dir

pytestmark = pytest.mark.gpu
DEV = "cuda"
PLANES = ("rgb", "depth", "mask", "padding")


@pytest.fixture(scope="module")
def g():
    return P.load_golden()


def device_frames(rgb, depth, mask, origin, inv, rotated, tables, h, w):
    from morpheus_amd import ops
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a if dt is None else np.asarray(a).astype(dt))).to(DEV)
    out = ops.prep_frames(t(rgb), t(depth), t(mask), t(origin, np.int32), t(inv, np.float64), t(rotated, np.uint8), t(tables[0]), t(tables[1]), h, w)
    torch.cuda.synchronize()
    return out


def same_planes(got, want, what):
    for k in PLANES:
        a, b = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, a.shape, b.dtype, b.shape)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, (what, k, len(bad), bad[:5].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


def rotated_inputs(centres, deg):
    return np.stack([P.invert_affine(P.rotation_matrix(c, deg)) for c in centres])


@pytest.mark.parametrize("run", range(len(P.RUNS)))
def test_preprocess_equals_the_golden(g, run):
    from morpheus_amd import preprocess as pp
    tag, h, w, radius = P.RUNS[run]
    i = inputs(g)
    cams = (torch.from_numpy(i["poses"]), torch.from_numpy(i["K"]), torch.full((P.F, 1), run_scale(radius)))
    cfg = {"data": {"size_h": h, "size_w": w, "rot_degree": 0, "depth_scale": P.DEPTH_SCALE}}
    res = pp.preprocess(i["rgb"], i["depth"], i["mask"], cams, cfg, device=DEV)
    assert all(getattr(res, k).is_cuda for k in PLANES)
    same_planes({k: getattr(res, k) for k in PLANES}, {k: g[tag + k] for k in PLANES}, tag)
    assert np.array_equal(res.crop_centres, g[tag + "centres"]) and torch.equal(res.poses_virt, torch.from_numpy(g[tag + "poses_virt"]))
    tabs = P.depth_tables(P.DEPTH_SCALE, run_scale(radius))
    assert np.array_equal(res.table_inside, tabs[0]) and np.array_equal(res.table_padded, tabs[1])
    # frame 0 is the one window inside the frame: its depth went through the fp32 product, every other through the float64 one
    t, l = res.origin[0]
    assert np.array_equal(res.depth[0].cpu().numpy(), tabs[0][i["depth"][0, t:t + h, l:l + w]])
    assert not np.array_equal(tabs[0][i["depth"][0, t:t + h, l:l + w]], tabs[1][i["depth"][0, t:t + h, l:l + w]])


def test_windows_the_reference_cannot_run_equal_the_oracle(g):
    """a window across two different sides, one wholly outside the frame, one larger than the frame -- and a few more of each
    kind, far outside included (the sums are formed in 64 bits)"""
    i = inputs(g)
    tabs = P.depth_tables(P.DEPTH_SCALE, 1.0)
    for h, w, origins in ((8, 8, [(-2, 11), (9, -3), (2, 19), (-8, 4), (12, 0), (-2 ** 31, 5), (2 ** 31 - 1, 2 ** 31 - 1), (-3, -3), (5, 9)]),
                          (14, 18, [(-1, 0), (-1, -1), (0, 0), (-13, -17), (11, 15), (12, 3)]),
                          (13, 5, [(-1, 2), (0, 13), (3, -4)])):
        kinds = [P.window_kind(t, l, h, w, P.H, P.W) for t, l in origins]
        assert {"two_sides", "outside"} <= set(kinds) or set(kinds) == {"larger"}, kinds
        n = len(origins)
        args = (i["rgb"][:n], i["depth"][:n], i["mask"][:n], np.array(origins, np.int64), np.zeros((n, 6)), np.zeros(n, np.uint8))
        want = P.prep_frames(*args, *tabs, h, w)
        same_planes(device_frames(*args, tabs, h, w), want, (h, w))
        for k, kind in enumerate(kinds):
            if kind == "outside":
                assert (want["padding"][k] == 255).all() and not want["rgb"][k].any() and not want["depth"][k].any()
    for kind, (py, px, h, w) in P.EXCLUDED.items():      # the three the golden tool showed the reference to raise on
        origin = P.window_origins([(px, py)], h, w)
        args = (i["rgb"][:1], i["depth"][:1], i["mask"][:1], origin, np.zeros((1, 6)), np.zeros(1, np.uint8))
        same_planes(device_frames(*args, tabs, h, w), P.prep_frames(*args, *tabs, h, w), kind)


@pytest.mark.parametrize("deg", P.ANGLES)
def test_rotated_frames_equal_the_oracle(g, deg):
    i = inputs(g)
    tabs = P.depth_tables(P.DEPTH_SCALE, run_scale(1.25))
    for tag, h, w, _ in P.RUNS:
        centres = g[tag + "centres"]
        origin = P.window_origins(centres, h, w)
        inv = rotated_inputs(centres, deg)
        args = (i["rgb"], i["depth"], i["mask"], origin, inv, np.ones(P.F, np.uint8))
        want = P.prep_frames(*args, *tabs, h, w)
        got = device_frames(*args, tabs, h, w)
        same_planes(got, want, (tag, deg))
        plain = device_frames(*args[:5], np.zeros(P.F, np.uint8), tabs, h, w)
        if deg == 0.0:      # the rotated path with the identity map is the unrotated path
            same_planes(got, {k: plain[k].cpu().numpy() for k in PLANES}, (tag, "identity"))
        else:
            assert not torch.equal(got["rgb"], plain["rgb"]) and not torch.equal(got["depth"], plain["depth"])
            assert torch.equal(got["padding"], plain["padding"])
    # frames that are rotated beside frames that are not
    mixed = (np.arange(P.F) % 2).astype(np.uint8)
    args = (i["rgb"], i["depth"], i["mask"], origin, inv, mixed)
    same_planes(device_frames(*args, tabs, h, w), P.prep_frames(*args, *tabs, h, w), ("mixed", deg))


def test_a_shape_across_lane_vector_and_block_edges():
    """F = 3 frames of 5 x 261 cut to 5 x 259: rows of 259 pixels put every group of four on another phase against the rows and the
    frames, 3 x 5 x 259 = 3885 pixels are 971 whole groups and one pixel (the element-store tail) over four blocks"""
    rng = np.random.default_rng(3)
    F, H, W, h, w = 3, 5, 261, 5, 259
    rgb = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    depth = rng.integers(0, 65536, (F, H, W)).astype(np.uint16)
    mask = rng.integers(0, 256, (F, H, W), dtype=np.uint8)
    tabs = P.depth_tables(1000.0, run_scale(1.25))
    for origin in ([(0, 1), (-2, -100), (1, 3)], [(0, 0), (0, 2), (4, 260)]):
        origin = np.array(origin, np.int64)
        centres = np.stack([origin[:, 1] + 129, origin[:, 0] + 2], -1)
        for rotated, deg in (((0, 0, 0), 0.0), ((1, 0, 1), 3.0), ((1, 1, 1), -77.0)):
            args = (rgb, depth, mask, origin, rotated_inputs(centres, deg), np.array(rotated, np.uint8))
            same_planes(device_frames(*args, tabs, h, w), P.prep_frames(*args, *tabs, h, w), (origin.tolist(), rotated))


def test_a_real_size_pair_equals_the_oracle():
    rng = np.random.default_rng(11)
    F, H, W, h, w = 2, 480, 640, 360, 360
    rgb = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    depth = rng.integers(0, 6000, (F, H, W)).astype(np.uint16)
    mask = rng.choice(np.array([0, 255], np.uint8), (F, H, W))
    tabs = P.depth_tables(1000.0, 1.0)
    centres = np.array([(320, 240), (500, 130)], np.int64)          # inside; beyond the right edge and above the top
    origin = P.window_origins(centres, h, w)
    assert [P.window_kind(t, l, h, w, H, W) for t, l in origin] == ["inside", "two_sides"]
    for rotated, deg in (((0, 0), 0.0), ((1, 1), 37.5)):
        args = (rgb, depth, mask, origin, rotated_inputs(centres, deg), np.array(rotated, np.uint8))
        same_planes(device_frames(*args, tabs, h, w), P.prep_frames(*args, *tabs, h, w), deg)


def test_from_raw_equals_from_dir_of_write_dir(g, tmp_path):
    from morpheus_amd import preprocess as pp
    from morpheus_amd.dataset import DeviceDataset
    cfg = write_raw_dir(tmp_path / "raw", g)
    pre = {"size_h": 7, "size_w": 7, "rot_degree": 0}
    a = DeviceDataset.from_raw(cfg, device=DEV, pre=pre)
    assert "size_h" not in cfg["data"] and a.cfg is cfg
    res = pp.preprocess_dir({"data": dict(cfg["data"], **pre)}, device=DEV)
    res.write_dir(str(tmp_path / "cut"))
    b = DeviceDataset.from_dir({"data": dict(cfg["data"], data_dir=str(tmp_path / "cut"))}, device=DEV)
    for k in PLANES[:3]:
        x, y = getattr(a, k + "_dev"), getattr(b, k + "_dev")
        assert x.is_cuda and x.dtype == y.dtype and torch.equal(x, y), k
        assert np.array_equal(x.cpu().numpy(), g["s7_" + k]), k          # and both are the reference's frames
    for k in ("poses", "radius", "theta", "phi", "intrinsics", "poses_dev", "radius_dev", "theta_dev", "phi_dev"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y), k
    assert np.array_equal(a.preprocessed.table_inside, res.table_inside) and np.array_equal(a.preprocessed.table_padded, res.table_padded)
    assert np.array_equal(a.preprocessed.padding.cpu().numpy(), g["s7_padding"])
    ra, rb = a.sample_real_view_rays(idx=1), b.sample_real_view_rays(idx=1)
    assert list(ra) == list(rb)
    for k in ra:
        if torch.is_tensor(ra[k]):
            assert ra[k].dtype == rb[k].dtype and torch.equal(ra[k], rb[k]), k
        else:
            assert ra[k] == rb[k], k


def test_refused_arguments_launch_nothing(g):
    from morpheus_amd import _lib, ops
    i = inputs(g)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    tabs = [t(x) for x in P.depth_tables(1000.0, 1.0)]
    rgb, depth, mask = t(i["rgb"]), t(i["depth"]), t(i["mask"])
    origin, inv, rot = torch.zeros(P.F, 2, dtype=torch.int32, device=DEV), torch.zeros(P.F, 6, dtype=torch.float64, device=DEV), torch.zeros(P.F, dtype=torch.uint8, device=DEV)
    outs = [torch.full((P.F * 8 * 8 * n,), 7, dtype=torch.uint8, device=DEV) for n in (3, 2, 1, 1)]
    _lib.load()
    fn = _lib._fns["mh_prep_frames"]
    ok = [rgb.data_ptr(), depth.data_ptr(), mask.data_ptr(), P.F, P.H, P.W, origin.data_ptr(), inv.data_ptr(), rot.data_ptr(), tabs[0].data_ptr(),
          tabs[1].data_ptr(), 8, 8] + [o.data_ptr() for o in outs]
    for at, bad in ((3, -1), (4, 0), (11, -8), (12, 0), (5, 2 ** 31 - 1), (11, 2 ** 30), (0, None), (6, None), (9, None), (13, None),
                    (13, outs[0].data_ptr() + 1), (14, outs[1].data_ptr() + 4)):
        args = list(ok)
        args[at] = bad
        assert fn(*args, _lib.stream()) == 1, (at, bad)
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)                   # nothing was written
    assert fn(*ok[:3], 0, *ok[4:], _lib.stream()) == 0 and all(bool((o == 7).all()) for o in outs)
    for bad in (dict(depth=depth.to(torch.float32)), dict(origin=origin.long()), dict(inv=inv.float()), dict(rot=rot[:3]), dict(tin=tabs[0][:100]),
                dict(h=0), dict(rgb=rgb[..., :2])):
        kw = dict(rgb=rgb, depth=depth, mask=mask, origin=origin, inv=inv, rot=rot, tin=tabs[0], tpad=tabs[1], h=8, w=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.prep_frames(kw["rgb"], kw["depth"], kw["mask"], kw["origin"], kw["inv"], kw["rot"], kw["tin"], kw["tpad"], kw["h"], kw["w"])
    with pytest.raises(_lib.MorpheusHipError, match="no CPU path"):
        ops.prep_frames(rgb.cpu(), depth, mask, origin, inv, rot, tabs[0], tabs[1], 8, 8)
