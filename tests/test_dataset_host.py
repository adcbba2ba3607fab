"""CPU (no GPU): the host side of morpheus_amd.dataset and the restatement tests/dataset_oracle.py against the reference's own
results (tests/golden/dataset.npz, recorded by tools/make_dataset_golden.py from datasets/dataset.py:DeformDataset).

The oracle equals the golden BIT FOR BIT wherever the definition is a chain of rounded fp32 operators: every tensor of both
real-view cases, the rays of every virtual view from the reference's fp32 pose, and the view labels, degree values and deltas of
every branch (in the uniform-sphere branch from dataset_oracle.sphere_angles, the reference's fp32 normalize / acos / atan2 chain).
Poses are float64 in the oracle and are compared with the recorded float64 pose within the recorded error of the reference's fp32
pose.
"""
import os

import numpy as np
import pytest
import torch

from tests import dataset_oracle as D


@pytest.fixture(scope="module")
def g():
    return D.load_golden()


def inputs(g):
    return {k[3:]: g[k] for k in g if k.startswith("in_")}


def host_dataset(g, **data):
    from morpheus_amd.dataset import DeviceDataset
    cfg = {"data": dict(D.CONFIG["data"], **data)}
    i = inputs(g)
    return DeviceDataset(cfg, i["rgb"], i["depth"], i["mask"], i["poses"], i["K"], i["radius"], i["theta"], i["phi"], device="cpu")


def test_golden_holds_the_cases_the_definition_turns_on(g):
    i = inputs(g)
    assert os.path.getsize(D.GOLDEN) < 100_000
    assert i["rgb"].shape == (D.F, D.H, D.W, 3) and D.H != D.W
    assert i["rgb"].min() == 0 and i["rgb"].max() == 255 and i["depth"].min() == 0 and i["depth"].max() == 65535
    assert set(np.unique(i["mask"])) == {0, 128, 254, 255}
    for k in i:      # the shared definition of the inputs is what the golden was recorded from
        assert np.array_equal(i[k], D.make_inputs()[k]), k
    R = i["poses"][:, :3, :3]
    assert (np.abs(R) > 1e-3).all() and (np.abs(R) < 0.999).all()      # no axis-aligned rotation
    assert g["rv0_idx"].tolist() == [2, 2, 4] and g["rv0_index"].shape == (37,)
    forced = g["rv1_index"]
    assert 0 in forced and D.H * D.W - 1 in forced and len(set(forced.tolist())) < len(forced)
    assert (g["vv_sphere0_H"], g["vv_sphere0_W"]) == (2, 2) and (g["vv_box_H"], g["vv_box_W"]) == (3, 4)
    assert (g["vv_polar0_H"], g["vv_polar0_W"]) == (D.H, D.W)
    az = g["vv_box_azimuth"]
    assert (az < 0).any() and ((az > 100) & (az <= 180)).any()
    assert set(g["vv_box_dir"].tolist()) == {0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize("tag", ["rv0_", "rv1_", "rv2_"])
def test_oracle_real_views_equal_the_reference(g, tag):
    index = g[tag + "index"] if g[tag + "index"].size else None
    o = D.real_view(inputs(g), g[tag + "idx"], index)
    for k in D.REAL_KEYS:
        want = torch.from_numpy(g[tag + k])
        assert o[k].dtype == want.dtype and o[k].shape == want.shape and torch.equal(o[k], want), k
    if index is None:
        assert o["image"].shape == (1, 3, D.H, D.W) and o["depth"].shape == (1, D.H, D.W) and o["mask"].dtype == torch.int64
    else:
        assert o["image"].shape == (3, 3, 37, 1) and o["mask"].shape == (3, 37, 1) and o["rays_t"].shape == (3, 37, 1)


def virtual(g, name):
    p = f"vv_{name}_"
    c = g[p + "c"] if g[p + "c"].size else None
    scale = None if np.isnan(g[p + "scale"]) else float(g[p + "scale"])
    return p, D.virtual_view(inputs(g), D.CONFIG, int(g[p + "mode"]), g[p + "a"], g[p + "b"], c, g[p + "t"],
                             bool(g[p + "ds_is_train"]), scale)


@pytest.mark.parametrize("name", D.VIRTUAL_CASES)
def test_oracle_virtual_views_equal_the_reference(g, name):
    p, o = virtual(g, name)
    assert (o["H"], o["W"]) == (int(g[p + "H"]), int(g[p + "W"]))
    for k in ("dir", "radius", "rays_t", "rays_id", "polar", "azimuth", "deg"):
        want = torch.from_numpy(g[p + k])
        assert o[k].dtype == want.dtype and torch.equal(o[k], want), (k, o[k], want)
    # the pose: float64 here, within the reference's own fp32 error of the recorded float64 pose (rotation on a scale of 1, the
    # translation on the scale of the radius); the reference's error is a few 1e-8
    e = np.abs(o["pose64"].numpy() - g[p + "pose64"])
    rot, tr = e[:, :3, :3].max(), (e[:, :3, 3] / g[p + "view_radius"].astype(np.float64)[:, None]).max()
    assert 0 < g[p + "err32"].max() < 4 * 2.0 ** -24
    assert rot <= g[p + "err32"][0] and tr <= g[p + "err32"][1], (rot, tr, g[p + "err32"])
    # the rays follow from the reference's fp32 pose bit for bit
    ro, rd = D.rays(o["K"], g[p + "pose32"], o["H"], o["W"])
    assert torch.equal(ro, torch.from_numpy(g[p + "rays_o"])) and torch.equal(rd, torch.from_numpy(g[p + "rays_d"]))


def write_dir(tmp_path, g):
    from PIL import Image
    i = inputs(g)
    for sub in ("color_virt", "depth_raw_crop", "mask_virt", "poses_virt"):
        os.makedirs(tmp_path / sub)
    for f in range(D.F):
        Image.fromarray(i["rgb"][f], "RGB").save(tmp_path / "color_virt" / f"{f:04d}.png")
        Image.fromarray(i["depth"][f]).save(tmp_path / "depth_raw_crop" / f"{f:04d}.png")
        Image.fromarray(i["mask"][f]).save(tmp_path / "mask_virt" / f"{f:04d}.png")
        np.savetxt(tmp_path / "poses_virt" / f"{f:04d}.txt", i["poses"][f].astype(np.float64))
    np.savetxt(tmp_path / "K_virt.txt", i["K"])
    np.savetxt(tmp_path / "r_theta_phi.txt", np.stack([i["radius"], i["theta"], i["phi"]], -1).astype(np.float64))
    return {"data": dict(D.CONFIG["data"], data_dir=str(tmp_path))}


def test_from_dir_reads_the_reference_layout(tmp_path, g):
    from morpheus_amd.dataset import DeviceDataset
    import sys
    cfg, i = write_dir(tmp_path, g), inputs(g)
    ds = DeviceDataset.from_dir(cfg, device="cpu")
    assert "cv2" not in sys.modules
    assert (ds.num_frames, ds.H, ds.W) == (D.F, D.H, D.W) and ds.data_dir == str(tmp_path) and ds.cfg is cfg
    assert ds.rgb_dev.dtype == torch.uint8 and ds.depth_dev.dtype == torch.uint16 and ds.mask_dev.dtype == torch.uint8
    assert np.array_equal(ds.rgb_dev.numpy(), i["rgb"]) and np.array_equal(ds.depth_dev.numpy(), i["depth"])
    assert np.array_equal(ds.mask_dev.numpy(), i["mask"])
    assert ds.intrinsics.dtype == torch.float64 and ds.intrinsics.device.type == "cpu" and np.array_equal(ds.intrinsics.numpy(), i["K"])
    assert ds.poses.dtype == torch.float32 and ds.poses.shape == (D.F, 4, 4) and np.array_equal(ds.poses.numpy(), i["poses"])
    for k in ("radius", "theta", "phi"):
        assert np.array_equal(getattr(ds, k).numpy(), i[k]), k
    assert torch.equal(ds.bounding_box, torch.tensor([-1.01] * 3 + [1.01] * 3)) and float(ds.bound) == pytest.approx(1.01)
    # the lazy host views the reference's evaluation reads
    assert np.array_equal(ds.depths, i["depth"] / 1000.0) and np.array_equal(ds.masks, i["mask"] / 255.0)
    assert ds.depths is ds.depths
    assert float(ds.get_radius(3)) == float(i["radius"][3])
    K2 = ds.scale_intrinsics(ds.intrinsics, 0.5)
    assert np.array_equal(K2.numpy()[:2], i["K"][:2] * 0.5) and np.array_equal(K2.numpy()[2], i["K"][2]) and np.array_equal(ds.intrinsics.numpy(), i["K"])
    assert ds.resident_bytes == D.F * D.H * D.W * 6 + D.F * (16 + 3) * 4
    # the test_id subset: frames of the three image lists, in the order asked for
    sub = DeviceDataset.from_dir(cfg, device="cpu", test_id=[3, 1])
    assert sub.num_frames == 2 and np.array_equal(sub.rgb_dev.numpy(), i["rgb"][[3, 1]])
    assert np.array_equal(sub.depth_dev.numpy(), i["depth"][[3, 1]]) and np.array_equal(sub.mask_dev.numpy(), i["mask"][[3, 1]])
    # poses and r_theta_phi keep every row on the host, as the reference's; the device tables hold the rows the frames can name
    assert sub.poses.shape == (D.F, 4, 4) and sub.radius.shape == (D.F,) and sub.poses_dev.shape == (2, 4, 4)
    assert np.array_equal(sub.poses_dev.numpy(), i["poses"][:2])
    for k in ("radius", "theta", "phi"):
        assert np.array_equal(getattr(sub, k + "_dev").numpy(), i[k][:2]), k


def test_host_poses_from_polar_angles(g):
    """get_c2w_from_polar / get_c2w_from_cam_center under the reference's names: the recorded is_train=False pose and label"""
    ds = host_dataset(g)
    p = "vv_polar0_"
    pose, dirs = ds.get_c2w_from_polar(t=torch.tensor([int(g[p + "t"][0])]), theta=torch.from_numpy(g[p + "a"]), phi=torch.from_numpy(g[p + "b"]))
    assert pose.shape == (1, 4, 4) and pose.dtype == torch.float32 and torch.equal(dirs, torch.from_numpy(g[p + "dir"]))
    assert float((pose.double() - torch.from_numpy(g[p + "pose64"])).abs().max()) <= 8 * 2.0 ** -24 * float(g[p + "view_radius"][0])


def test_remove_outlier_equals_the_reference(g):
    from morpheus_amd.dataset import DeviceDataset, remove_outlier
    poses, rtp = D.outlier_sequence()
    assert np.array_equal(poses, g["ol_poses_in"]) and np.array_equal(rtp, g["ol_rtp_in"])
    r, th, ph = (torch.from_numpy(rtp[:, k].copy()) for k in range(3))
    fixed, repaired = remove_outlier(torch.from_numpy(poses.copy()), th, ph, r, len(poses))
    assert repaired == [4, 5]
    assert torch.equal(fixed, torch.from_numpy(g["ol_poses"]))
    assert torch.equal(fixed[4], torch.from_numpy(poses[3])) and torch.equal(fixed[5], torch.from_numpy(poses[3]))
    for got, k in ((r, "ol_radius"), (th, "ol_theta"), (ph, "ol_phi")):
        assert torch.equal(got, torch.from_numpy(g[k])), k
    # through the constructor, when data.outlier_remove is set: poses and the three tables are rewritten, the device copies too
    n = len(poses)
    z = np.zeros((n, 2, 2), np.uint8)
    cfg = {"data": dict(D.CONFIG["data"], outlier_remove=True)}
    ds = DeviceDataset(cfg, np.zeros((n, 2, 2, 3), np.uint8), np.zeros((n, 2, 2), np.uint16), z, poses, np.eye(3), rtp[:, 0], rtp[:, 1],
                       rtp[:, 2], device="cpu")
    assert ds.outliers == [4, 5] and torch.equal(ds.poses, fixed) and torch.equal(ds.poses_dev, fixed)
    assert torch.equal(ds.theta, th) and torch.equal(ds.theta_dev, th) and torch.equal(ds.radius, r) and torch.equal(ds.phi, ph)
    cfg["data"]["outlier_remove"] = False
    ds = DeviceDataset(cfg, np.zeros((n, 2, 2, 3), np.uint8), np.zeros((n, 2, 2), np.uint16), z, poses, np.eye(3), rtp[:, 0], rtp[:, 1],
                       rtp[:, 2], device="cpu")
    assert ds.outliers == [] and np.array_equal(ds.poses.numpy(), poses)


def test_argument_rules(g):
    from morpheus_amd._lib import MorpheusHipError
    with pytest.raises(NotImplementedError, match="cv2"):
        host_dataset(g, known_view_scale=0.5)
    ds = host_dataset(g)
    with pytest.raises(IndexError, match=r"idx outside \[0, 5\)"):
        ds.sample_real_view_rays(idx=5, ray_num=4)
    with pytest.raises(IndexError, match=r"idx outside"):
        ds.sample_real_view_rays(idx=torch.tensor([0, -1]), ray_num=4)
    for five in (np.int64(5), torch.tensor(5), np.array(5)):      # every integer form the reference's v[idx] takes
        with pytest.raises(IndexError, match=r"idx outside \[0, 5\)"):
            ds.sample_real_view_rays(idx=five, ray_num=4)
    for four in (np.int64(4), torch.tensor(4), np.array(4), np.int32(4)):
        with pytest.raises(MorpheusHipError, match="no CPU path"):
            ds.sample_real_view_rays(idx=four, ray_num=4)
    with pytest.raises(ValueError, match="one-dimensional"):
        ds.sample_real_view_rays(idx=torch.tensor([[0, 1]]), ray_num=4)
    with pytest.raises(IndexError, match=r"index outside \[0, 48\)"):
        ds.sample_real_view_rays(idx=0, index=torch.tensor([0, 48], dtype=torch.int32))
    with pytest.raises(IndexError, match=r"index outside"):
        ds.sample_real_view_rays(idx=0, index=torch.tensor([-1], dtype=torch.int32))
    with pytest.raises(ValueError, match="int32"):
        ds.sample_real_view_rays(idx=0, index=torch.tensor([1]))
    with pytest.raises(ValueError, match="ray_num"):
        ds.sample_real_view_rays(idx=0, ray_num=3, index=torch.tensor([1], dtype=torch.int32))
    with pytest.raises(IndexError, match=r"t outside"):
        ds.get_virtual_view_rays(t=7)
    # no CPU path: the frames of this dataset are on the CPU
    with pytest.raises(MorpheusHipError, match="no CPU path"):
        ds.sample_real_view_rays(idx=0, ray_num=4)
    with pytest.raises(MorpheusHipError, match="no CPU path"):
        ds.sample_real_view_rays(idx=1)
    with pytest.raises(MorpheusHipError, match="no CPU path"):
        ds.get_virtual_view_rays(t=1)
    i = inputs(g)
    from morpheus_amd.dataset import DeviceDataset
    with pytest.raises(ValueError, match="uint8"):
        DeviceDataset(D.CONFIG, i["rgb"].astype(np.float32), i["depth"], i["mask"], i["poses"], i["K"], i["radius"], i["theta"], i["phi"], device="cpu")
    with pytest.raises(ValueError, match="depth must be"):
        DeviceDataset(D.CONFIG, i["rgb"], i["depth"].astype(np.int32), i["mask"], i["poses"], i["K"], i["radius"], i["theta"], i["phi"], device="cpu")


def test_library_takes_bad_dataset_arguments_without_a_launch():
    from morpheus_amd import _lib, build
    build.build()
    lib = _lib.load()
    assert lib.mh_dataset_sample(1.0, 1.0, 0.0, 0.0, *([None] * 3), 0, 1000.0, *([None] * 4), 5, 6, 8, None, 0, None, 4, *([None] * 11), None) == 0
    assert lib.mh_dataset_sample(1.0, 1.0, 0.0, 0.0, *([None] * 3), 0, 1000.0, *([None] * 4), 5, 6, 8, None, 2, None, 4, *([None] * 11), None) == 1
    assert lib.mh_generate_rays_dev(1.0, 1.0, 0.0, 0.0, None, 0, 6, 8, None, 48, None, 0, *([None] * 4), None) == 0
    assert lib.mh_generate_rays_dev(1.0, 1.0, 0.0, 0.0, None, 2, 6, 8, None, 48, None, 0, *([None] * 4), None) == 1
    assert lib.mh_dataset_virtual_pose(0, *([None] * 4), 0, *([None] * 3), 5, 1.0, *([0.0] * 6), *([None] * 6), None) == 0
    assert lib.mh_dataset_virtual_pose(3, *([None] * 4), 2, *([None] * 3), 5, 1.0, *([0.0] * 6), *([None] * 6), None) == 1
    assert lib.mh_abi_version() == 10


def test_dataset_source_is_built_without_contraction():
    from morpheus_amd import build
    assert "dataset.hip" in build.SOURCES and build.FILE_FLAGS["dataset.hip"] == ["-ffp-contract=off"]
    src = open(os.path.join(build.CSRC, "dataset.hip")).read()
    assert '#include "rays.h"' in src and '#include "rays.h"' in open(os.path.join(build.CSRC, "sampler.hip")).read()
