"""GPU: morpheus_amd.dataset.DeviceDataset (csrc/dataset.hip) against the reference's own results, tests/golden/dataset.npz.

Bit for bit (`torch.equal`, dtypes and shapes included): every tensor of both real-view cases; whole-frame rays against
`ops.generate_rays`; for virtual views the label, degree values and deltas, and the rays against `ops.generate_rays` fed the device's
own pose.  The look-at pose is judged against float64 (tests/f64_judge.judge_vs_f64 with the factor, floor and slack of
tests/test_gpu_volrend.py: 2, 4 x 2^-24, 2), the golden's fp32 pose being the fp32 restatement, on a scale of 1 for rotation entries
and of the view's radius for the translation.

In the uniform-sphere branch the fp32 angles are not inputs: the kernel restates the reference's fp32 normalize / acos / atan2
chain (dataset_oracle.sphere_angles says how), and test_sphere_angles_equal_the_oracle_in_every_quadrant holds it to that
restatement over draws that reach every branch of the arctangent.
"""
import numpy as np
import pytest
import torch

from tests import dataset_oracle as D
from tests.f64_judge import U, figures_vs_f64, judge_vs_f64

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR, FLOOR, SLACK = 2.0, 4 * U, 2      # tests/volrend_oracle.py


@pytest.fixture(scope="module")
def g():
    return D.load_golden()


def inputs(g):
    return {k[3:]: g[k] for k in g if k.startswith("in_")}


@pytest.fixture(scope="module")
def ds(g):
    from morpheus_amd.dataset import DeviceDataset
    i = inputs(g)
    return DeviceDataset(D.CONFIG, i["rgb"], i["depth"], i["mask"], i["poses"], i["K"], i["radius"], i["theta"], i["phi"], device=DEV)


def same(got, want, what):
    want = torch.as_tensor(want)
    assert got.is_cuda, what
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert torch.equal(got.cpu(), want), (what, got.cpu().tolist(), want.tolist())


@pytest.mark.parametrize("tag,on_device", [("rv0_", False), ("rv1_", True), ("rv2_", False)])
def test_real_views_equal_the_golden(g, ds, tag, on_device):
    idx = torch.from_numpy(g[tag + "idx"])
    if g[tag + "index"].size:
        index = torch.from_numpy(g[tag + "index"])
        res = ds.sample_real_view_rays(idx=idx.to(DEV) if on_device else idx, ray_num=37, index=index.to(DEV) if on_device else index)
        assert (res["H"], res["W"]) == (37, 1)
    else:
        res = ds.sample_real_view_rays(idx=int(idx[0]))
        assert (res["H"], res["W"]) == (D.H, D.W)
    assert list(res) == ["rays_o", "rays_d", "rays_t", "rays_id", "H", "W", "image", "depth", "mask", "intri", "pose", "theta", "phi", "radius"]
    for k in D.REAL_KEYS:
        same(res[k], g[tag + k], tag + k)
    assert res["intri"].dtype == torch.float64 and not res["intri"].is_cuda and np.array_equal(res["intri"].numpy(), g["in_K"])


def test_whole_frame_rays_equal_generate_rays(g, ds):
    from morpheus_amd import ops
    K = g["in_K"]
    res = ds.sample_real_view_rays(idx=torch.tensor([3, 0]))
    for b, f in enumerate((3, 0)):
        o, d = ops.generate_rays(K[0, 0], K[1, 1], K[0, 2], K[1, 2], g["in_poses"][f], D.H, D.W, DEV)
        assert torch.equal(res["rays_o"][b], o) and torch.equal(res["rays_d"][b], d), f


def fp32_depth_dataset(g):
    from morpheus_amd.dataset import DeviceDataset
    i = inputs(g)
    return DeviceDataset(D.CONFIG, i["rgb"], i["depth"].astype(np.float32), i["mask"], i["poses"], i["K"], i["radius"], i["theta"],
                         i["phi"], device=DEV)


def test_fp32_depth_storage_gives_the_same_depth(g):
    same(fp32_depth_dataset(g).sample_real_view_rays(idx=3)["depth"], g["rv2_depth"], "depth from fp32 storage")


def virtual(g, ds, name):
    p = f"vv_{name}_"
    mode = int(g[p + "mode"])
    scale = None if np.isnan(g[p + "scale"]) else float(g[p + "scale"])
    ds.is_train = bool(g[p + "ds_is_train"])
    try:
        if mode == D.POLAR:
            res = ds.get_virtual_view_rays(t=int(g[p + "t"][0]), is_train=False, scale=scale, phis=float(g[p + "b"][0]) / 360)
        else:
            if mode == D.ANGLES:
                draws = {"thetas": torch.from_numpy(g[p + "a"]), "phis": torch.from_numpy(g[p + "b"])}
            else:
                draws = {"normals": torch.from_numpy(np.stack([g[p + "a"], g[p + "b"], g[p + "c"]], -1))}
            res = ds.get_virtual_view_rays(bs=len(g[p + "t"]), t=torch.from_numpy(g[p + "t"]), is_train=True, scale=scale, draws=draws)
    finally:
        ds.is_train = True
    return p, mode, res


@pytest.mark.parametrize("name", D.VIRTUAL_CASES)
def test_virtual_views(g, ds, name):
    from morpheus_amd import ops
    p, mode, res = virtual(g, ds, name)
    H, W = int(g[p + "H"]), int(g[p + "W"])
    assert (res["H"], res["W"]) == (H, W)
    for k in ("dir", "radius", "rays_t", "rays_id"):
        same(res[k], g[p + k], p + k)
    # ---- the pose against float64, the golden's fp32 pose as the fp32 restatement
    pose = res["pose"]
    B = pose.shape[0]
    assert pose.is_cuda and pose.dtype == torch.float32 and pose.shape == (B, 4, 4)
    assert torch.equal(pose[:, 3].cpu(), torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(B, 4))
    scale = torch.ones(B, 3, 4, dtype=torch.float64)
    scale[:, :, 3] = torch.from_numpy(g[p + "view_radius"]).double()[:, None]
    f = figures_vs_f64(pose[:, :3], g[p + "pose32"][:, :3], g[p + "pose64"][:, :3], scale, name, FLOOR)
    print(f"[dataset-f64] {name} pose: kernel {f['worst_hip']:.3e}  reference fp32 {f['worst_ref']:.3e}  above {FLOOR:.1e}: "
          f"{f['n_hip']} / {f['n_ref']} of {f['n']}")
    judge_vs_f64(pose[:, :3], g[p + "pose32"][:, :3], g[p + "pose64"][:, :3], scale, name + " pose", FACTOR, FLOOR, SLACK)
    # ---- the rays: ops.generate_rays fed the device's own pose, copied to the host
    assert res["rays_o"].shape == (B, H * W, 3) and res["rays_d"].shape == (B, H * W, 3)
    K = D.virtual_view(inputs(g), D.CONFIG, mode, g[p + "a"], g[p + "b"], g[p + "c"] if g[p + "c"].size else None, g[p + "t"],
                       bool(g[p + "ds_is_train"]), None if np.isnan(g[p + "scale"]) else float(g[p + "scale"]))["K"].numpy()
    host = pose.cpu().numpy()
    for b in range(B):
        o, d = ops.generate_rays(K[0, 0], K[1, 1], K[0, 2], K[1, 2], host[b], H, W, DEV)
        assert torch.equal(res["rays_o"][b], o) and torch.equal(res["rays_d"][b], d), (name, b)


@pytest.mark.parametrize("name", D.VIRTUAL_CASES)
def test_virtual_view_angles_equal_the_golden(g, ds, name):
    """degree values and deltas, bit for bit, in every branch"""
    p, mode, res = virtual(g, ds, name)
    print(f"[dataset] {name}: degrees {res['deg'].cpu().tolist()} golden {g[p + 'deg'].tolist()}")
    for k in ("deg", "polar", "azimuth"):
        same(res[k], g[p + k], p + k)


def test_sphere_angles_equal_the_oracle_in_every_quadrant(g, ds):
    """the uniform-sphere branch over 256 views: label, degree values and deltas equal the oracle's fp32 chain bit for bit.  The
    draws reach every form of the arctangent: all four sign pairs of (x, z), |x / z| in each of its five ranges (below 7/16, to
    11/16, to 19/16, to 39/16, above), x = 0, z = 0, and a centre on the pole (x = z = 0)."""
    rng = np.random.default_rng(11)
    n = rng.standard_normal((256, 3)).astype(np.float32)
    ratio = np.array([0.2, 0.5, 0.9, 1.7, 5.0], np.float32)
    k = 0
    for sx in (1, -1):
        for sz in (1, -1):
            for r in ratio:
                n[k, 0], n[k, 2] = sx * r, sz
                k += 1
    n[k], n[k + 1], n[k + 2], n[k + 3] = (0.0, 0.7, 1.3), (0.0, 0.7, -1.3), (-0.8, 0.3, 0.0), (0.0, 2.0, 0.0)
    t = torch.from_numpy(rng.integers(0, D.F, 256))
    res = ds.get_virtual_view_rays(bs=256, t=t, is_train=True, draws={"normals": torch.from_numpy(n)})
    o = D.virtual_view(inputs(g), D.CONFIG, D.SPHERE, n[:, 0], n[:, 1], n[:, 2], t, True, None)
    assert bool((o["ph"] >= 0).all()) and bool((o["ph"] > np.pi).any()) and set(o["dir"].tolist()) == {0, 1, 2, 3, 4}
    for k_ in ("deg", "polar", "azimuth", "dir", "radius"):
        same(res[k_], o[k_], "sphere " + k_)


def test_a_test_id_subset_samples_with_the_first_rows_of_the_tables(g, tmp_path):
    """from_dir(test_id=[3, 0, 4]) keeps every row of poses and r_theta_phi, as the reference does, and frame k of the subset goes
    with row k of those tables (its `v[idx]`): real views and virtual views equal the oracle fed the same arrays, and every
    integer form of `idx` names the same frame"""
    from morpheus_amd.dataset import DeviceDataset
    from tests.test_dataset_host import write_dir
    sel, i = [3, 0, 4], inputs(g)
    sub = DeviceDataset.from_dir(write_dir(tmp_path, g), device=DEV, test_id=sel)
    assert sub.num_frames == 3 and sub.poses.shape == (D.F, 4, 4) and sub.poses_dev.shape == (3, 4, 4)
    inp = dict(i, rgb=i["rgb"][sel], depth=i["depth"][sel], mask=i["mask"][sel])
    index = torch.tensor([0, D.H * D.W - 1, 13, 13, 21], dtype=torch.int32)
    res = sub.sample_real_view_rays(idx=torch.tensor([2, 0, 2, 1]), index=index)
    orc = D.real_view(inp, [2, 0, 2, 1], index)
    for k in D.REAL_KEYS:
        same(res[k], orc[k], "subset " + k)
    assert torch.equal(res["image"][0].cpu(), D.real_view(i, [4], index)["image"][0])      # the picture of frame 4 ...
    assert np.array_equal(res["pose"][0].cpu().numpy(), i["poses"][2])                      # ... with row 2 of the poses
    whole = D.real_view(inp, [1])
    for one in (1, np.int64(1), np.int32(1), torch.tensor(1), torch.tensor(1, device=DEV), np.array(1)):
        got = sub.sample_real_view_rays(idx=one)
        for k in D.REAL_KEYS:
            same(got[k], whole[k], f"subset, idx {type(one).__name__}: {k}")
    th, ph, t = np.array([1.0, 1.3, 0.4], np.float32), np.array([0.5, -2.0, 4.0], np.float32), np.array([2, 0, 1])
    v = sub.get_virtual_view_rays(bs=3, t=torch.from_numpy(t), draws={"thetas": torch.from_numpy(th), "phis": torch.from_numpy(ph)})
    o = D.virtual_view(inp, D.CONFIG, D.ANGLES, th, ph, None, t, True, None)
    for k in ("dir", "deg", "polar", "azimuth", "radius", "rays_t", "rays_id"):
        same(v[k], o[k], "subset virtual " + k)
    drawn = sub.sample_real_view_rays(bs=64, ray_num=4)["rays_id"]
    assert int(drawn.min()) >= 0 and int(drawn.max()) < 3


def test_generate_rays_dev_pix_subset_equals_the_gathered_image(g, ds):
    from morpheus_amd import ops
    K, poses = g["in_K"], ds.poses_dev[[1, 4, 1]]
    o, d = ops.generate_rays_dev(K, poses, D.H, D.W)
    assert o.shape == (3, D.H * D.W, 3) and d.shape == o.shape
    for b, f in enumerate((1, 4, 1)):
        ho, hd = ops.generate_rays(K[0, 0], K[1, 1], K[0, 2], K[1, 2], g["in_poses"][f], D.H, D.W, DEV)
        assert torch.equal(o[b], ho) and torch.equal(d[b], hd)
    pix = torch.tensor([47, 0, 13, 13, 8, 7, 40], dtype=torch.int32, device=DEV)
    so, sd = ops.generate_rays_dev(K, poses, D.H, D.W, pix)
    assert so.shape == (3, 7, 3) and torch.equal(so, o[:, pix.long()]) and torch.equal(sd, d[:, pix.long()])
    frames = torch.tensor([1, 4, 1], device=DEV)
    to, td, tt, ti = ops.generate_rays_dev(K, poses, D.H, D.W, pix, frames, D.F)
    assert torch.equal(to, so) and torch.equal(td, sd)
    assert ti.dtype == torch.int64 and torch.equal(ti.cpu(), torch.tensor([1, 4, 1])[:, None, None].repeat(1, 7, 1))
    assert torch.equal(tt.cpu(), (torch.tensor([1.0, 4.0, 1.0]) / torch.tensor(5.0))[:, None, None].repeat(1, 7, 1))
    with pytest.raises(ValueError, match="int32"):
        ops.generate_rays_dev(K, poses, D.H, D.W, pix.long())


def test_device_drawn_batches_feed_the_renderer(g, ds):
    from morpheus_amd import harness, synth
    torch.manual_seed(3)
    a = ds.sample_real_view_rays(bs=4, ray_num=64)
    b = ds.sample_real_view_rays(bs=4, ray_num=64)
    for r in (a, b):
        assert r["rays_id"].shape == (4, 64, 1) and int(r["rays_id"].min()) >= 0 and int(r["rays_id"].max()) < D.F
        assert torch.equal(r["rays_t"].cpu(), r["rays_id"].cpu().float() / torch.tensor(float(D.F)))
        assert bool((r["rays_id"] == r["rays_id"][:, :1]).all())          # one frame per batch row
    assert not torch.equal(a["rays_d"], b["rays_d"])                      # another draw of pixels (and frames)
    v = ds.get_virtual_view_rays(bs=2)
    assert v["rays_o"].shape == (2, v["H"] * v["W"], 3) and int(v["dir"].min()) >= 0 and int(v["dir"].max()) <= 5
    assert int(v["rays_id"].min()) >= 0 and int(v["rays_id"].max()) < D.F and bool(torch.isfinite(v["pose"]).all())
    # the batch is what HotPathRenderer.render_rays takes
    one = ds.sample_real_view_rays(bs=1, ray_num=64)
    model = harness.build_model("b", DEV).eval()
    rend = harness.make_renderer(model, 8, jitter=synth.ray_jitter(64).to(DEV))
    light = torch.nn.functional.normalize(one["rays_o"][0] + torch.tensor([0.3, -0.2, 0.5], device=DEV), dim=-1)
    with torch.no_grad():
        res = rend.render_rays(one["rays_o"], one["rays_d"], one["rays_t"], one["rays_id"], one["H"], one["W"], ambient_ratio=1.0,
                               light_d=light, shading="albedo")
    assert bool(torch.isfinite(res["image"]).all()) and bool(torch.isfinite(res["depth"]).all())


def test_indices_are_clamped_and_nothing_else_is_written(g, ds):
    from morpheus_amd import _lib
    from morpheus_amd._lib import ptr
    HW = D.H * D.W
    wild = torch.tensor([HW + 5, -1, 3, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device=DEV)
    tame = torch.tensor([HW - 1, 0, 3, HW - 1, 0], dtype=torch.int32, device=DEV)
    frames_wild = torch.tensor([7, -3, 2], device=DEV)
    frames_tame = torch.tensor([4, 0, 2], device=DEV)
    got = ds.sample_real_view_rays(idx=frames_wild, index=wild)
    want = ds.sample_real_view_rays(idx=frames_tame, index=tame)
    orc = D.real_view(inputs(g), [4, 0, 2], tame.cpu())
    for k in D.REAL_KEYS:
        assert torch.equal(got[k], want[k]), k
        same(got[k], orc[k], k)
    # ---- the same launch into sentinel-padded buffers: the pads stay untouched
    PAD, B, N = 64, 3, 5
    shapes = dict(rays_o=(B * N * 3, torch.float32), rays_d=(B * N * 3, torch.float32), rays_t=(B * N, torch.float32),
                  rays_id=(B * N, torch.int64), image=(B * 3 * N, torch.float32), depth=(B * N, torch.float32),
                  mask=(B * N, torch.int64), pose=(B * 16, torch.float32), theta=(B, torch.float32), phi=(B, torch.float32),
                  radius=(B, torch.float32))
    bufs = {k: torch.full((n + 2 * PAD,), -77, dtype=dt, device=DEV) for k, (n, dt) in shapes.items()}
    inner = {k: bufs[k][PAD:PAD + n] for k, (n, dt) in shapes.items()}
    K = g["in_K"]
    _lib.launch("mh_dataset_sample", float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), ptr(ds.poses_dev), ptr(ds.rgb_dev),
                ptr(ds.depth_dev), 0, ds.depth_scale, ptr(ds.mask_dev), ptr(ds.theta_dev), ptr(ds.phi_dev), ptr(ds.radius_dev), D.F, D.H,
                D.W, ptr(frames_wild), B, ptr(wild), N, *(inner[k].data_ptr() for k in shapes))
    torch.cuda.synchronize()
    for k, (n, dt) in shapes.items():
        assert bool((bufs[k][:PAD] == -77).all()) and bool((bufs[k][PAD + n:] == -77).all()), k
        assert torch.equal(inner[k], want[k].reshape(-1)), k
    # virtual views: wild frame indices on the device are clamped too
    v = ds.get_virtual_view_rays(t=torch.tensor([99, -5], device=DEV), draws={"thetas": torch.tensor([1.0, 1.2]), "phis": torch.tensor([0.5, 4.0])})
    w = ds.get_virtual_view_rays(t=torch.tensor([4, 0], device=DEV), draws={"thetas": torch.tensor([1.0, 1.2]), "phis": torch.tensor([0.5, 4.0])})
    for k in ("pose", "dir", "polar", "azimuth", "radius", "rays_o", "rays_d", "rays_t", "rays_id"):
        assert torch.equal(v[k], w[k]), k
