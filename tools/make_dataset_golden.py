"""Record tests/golden/dataset.npz from the reference's own DeformDataset (build container only: needs the reference tree).

    python tools/make_dataset_golden.py <reference tree>

datasets/dataset.py is loaded by file path, with a stub `cv2` module whose `resize` asserts that the size is unchanged and returns
its input (the golden is recorded at known_view_scale = 1.0).  A DeformDataset is filled without touching disk from the frames of
tests/dataset_oracle.make_inputs (F = 5, H = 6, W = 8) and run with tests/dataset_oracle.CONFIG.  Recorded, numeric arrays only:

  in_*        the frames, poses, intrinsics and r / theta / phi tables
  rv0_*       sample_real_view_rays(idx = [2, 2, 4], ray_num = 37): the pixel draw is recovered by re-seeding torch
  rv1_*       the same frames with a forced draw (torch.randint answers it): duplicates, pixel 0 and pixel H W - 1
  rv2_*       sample_real_view_rays(idx = 3): the whole frame
  ol_*        remove_outlier on a 20-pose sequence with two consecutive translation outliers: poses, theta, phi, radius after
  vv_<case>_* get_virtual_view_rays, for the cases of dataset_oracle.VIRTUAL_CASES, each with the draws used (mode, a, b, c: the
              radians or normals that torch.rand / torch.randn were made to answer; get_view_direction is wrapped to record the
              radians the reference really used), the frames t, the dataset's is_train, the scale (nan: None), every tensor of the
              returned dictionary, the degree values, the reference's fp32 pose, the float64 pose (dataset_oracle.look_at_np
              on the float64 chain from the same fp32 inputs) and err32 = max |fp32 pose - float64 pose| over the rotation
              entries and over the translation / radius.
      box      the theta/phi box, 16 views, novel_view_scale = 0.5: phis on the four fp32 label boundaries and one fp32 step
               either side, thetas on both overhead boundaries and one step either side, azimuth deltas on each side of 180
      sphere0-2  the uniform sphere, one view each (the reference's `radius * unit_centers` broadcasts for one view only);
               sphere0 with scale = 0.35, so that int() truncates to 2 x 2
      polar0/1 is_train = False through get_c2w_from_polar: the dataset not in training (full size) / in training (0.5)
Finally tests/dataset_oracle.py is checked against all of it: bit for bit, poses within the recorded fp32 error.
"""
import contextlib
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dataset_oracle as D  # noqa: E402


def load_module(ref):
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR, cv2.INTER_NEAREST = 1, 0

    def resize(img, size, interpolation=None):
        assert tuple(size) == (img.shape[1], img.shape[0]), "the golden is recorded without resizing"
        return img
    cv2.resize = resize
    sys.modules["cv2"] = cv2
    pkg_dir = os.path.join(ref, "datasets")
    pkg = types.ModuleType("reference_datasets")
    pkg.__path__ = [pkg_dir]
    sys.modules["reference_datasets"] = pkg
    spec = importlib.util.spec_from_file_location("reference_datasets.dataset", os.path.join(pkg_dir, "dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def make_dataset(mod, inp, cfg, is_train=True):
    ds = object.__new__(mod.DeformDataset)
    ds.cfg, ds.data_dir = cfg, cfg["data"]["data_dir"]
    ds.images = inp["rgb"] / 255.0
    ds.depths = inp["depth"] / cfg["data"]["depth_scale"]
    ds.masks = inp["mask"] / 255.0
    ds.num_frames = ds.images.shape[0]
    ds.intrinsics = torch.from_numpy(inp["K"].copy())
    ds.radius, ds.theta, ds.phi = (torch.from_numpy(inp[k].copy()).to(torch.float32) for k in ("radius", "theta", "phi"))
    ds.poses = torch.from_numpy(inp["poses"].copy()).to(torch.float32)
    ds.bounding_box = ds.load_bounding_box()
    ds.bound = ds.bounding_box.abs().max()
    ds.H, ds.W = ds.get_HW()
    ds.outlier_remove, ds.is_train = True, is_train
    ds.real_view_data = ds.get_real_view_rays(load=True)
    return ds


@contextlib.contextmanager
def answers(mod, rand=(), randn=(), randint=None, coin=None):
    """torch.rand / torch.randn answer the queued tensors, torch.randint `randint`, random.random `coin`; get_view_direction of
    the module records the radians it is called with -> the record"""
    saved = (torch.rand, torch.randn, torch.randint, random.random, mod.get_view_direction)
    rand, randn, seen = list(rand), list(randn), {}

    def spy(thetas, phis, overhead, front):
        seen["th"], seen["ph"] = thetas.clone(), phis.clone()
        return saved[4](thetas, phis, overhead, front)
    if rand:
        torch.rand = lambda size: rand.pop(0).clone()
    if randn:
        torch.randn = lambda size: randn.pop(0).clone()
    if randint is not None:
        torch.randint = lambda lo, hi, size: randint.clone()
    if coin is not None:
        random.random = lambda: coin
    mod.get_view_direction = spy
    try:
        yield seen
    finally:
        torch.rand, torch.randn, torch.randint, random.random, mod.get_view_direction = saved


def f32(x):
    return np.float32(x)


def step(x, up):
    return np.nextafter(f32(x), f32(np.inf if up else -np.inf))


def box_draws():
    """16 views: radians on and beside the fp32 thresholds"""
    front, over = np.deg2rad(60.0), np.deg2rad(30.0)
    bounds = [f32(front / 2), f32(np.pi - front / 2), f32(np.pi + front / 2), f32(2 * np.pi - front / 2)]
    phis = []
    for bnd in bounds:
        phis += [step(bnd, False), bnd, step(bnd, True)]
    phis += [f32(3.2), f32(3.4), f32(-0.3), f32(0.0)]            # azimuth deltas below / above 180; a negative draw; zero
    thetas = [f32(1.1)] * 9 + [step(over, False), f32(over), step(over, True), step(np.pi - over, False), f32(np.pi - over),
                               step(np.pi - over, True), f32(1.4)]
    # the overhead rows ride on phis of the list above (any label below them must be overridden)
    t = [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 2]
    return np.array(thetas, np.float32), np.array(phis, np.float32), np.array(t, np.int64)


def err32(pose32, pose64, radius):
    e = np.abs(pose32.astype(np.float64) - pose64)
    return np.array([e[:, :3, :3].max(), (e[:, :3, 3] / np.asarray(radius, np.float64).reshape(-1, 1)).max()])


def virtual_case(mod, inp, out, name, mode, a, b, c, t, ds_is_train, scale, phis_arg=0.0):
    cfg = {"data": dict(D.CONFIG["data"])}
    if mode == D.ANGLES:      # ranges of exactly one radian from zero: torch.rand's answer IS the angle
        cfg["data"]["theta_range"] = cfg["data"]["phi_range"] = [0.0, 57.29577951308232]
        assert np.float32(np.deg2rad(57.29577951308232)) == np.float32(1.0)
    ds = make_dataset(mod, inp, cfg, is_train=ds_is_train)
    tt = torch.from_numpy(t)
    if mode == D.POLAR:
        with answers(mod) as seen:
            ref = ds.get_virtual_view_rays(t=int(t[0]), is_train=False, scale=scale, phis=phis_arg)
        a = np.array([cfg["data"]["default_polar"]], np.float32)
        b = np.array([phis_arg * 360], np.float32)
        deg = np.stack([a, b], -1)
    else:
        poses_seen = {}
        inner = ds.get_virtual_view_data

        def data_spy(*args, **kw):
            res = inner(*args, **kw)
            poses_seen["pose"], poses_seen["deg"] = res[0].clone(), torch.stack([res[2], res[3]], -1).clone()
            return res
        ds.get_virtual_view_data = data_spy
        if mode == D.ANGLES:
            kw = dict(rand=[torch.from_numpy(a), torch.from_numpy(b)], coin=1.0)
        else:
            kw = dict(randn=[torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(c)], coin=0.0)
        with answers(mod, **kw) as seen:
            ref = ds.get_virtual_view_rays(bs=len(t), t=tt, is_train=True, scale=scale)
        deg = poses_seen["deg"].numpy()
    # the reference's fp32 pose: the rays carry it (rays_o = translation; the rotation through get_c2w_from_*)
    if mode == D.POLAR:
        pose32 = ds.get_c2w_from_polar(t=int(t[0]), theta=torch.from_numpy(a), phi=torch.from_numpy(b))[0].numpy()
    else:
        pose32 = poses_seen["pose"].numpy()
    orc = D.virtual_view(inp, D.CONFIG, mode, a, b, c, t, ds_is_train, scale)
    if mode == D.ANGLES:      # the radians the reference used are the injected ones (negative phis moved up by 2 pi)
        assert torch.equal(seen["th"], orc["th"]) and torch.equal(seen["ph"], orc["ph"]), name
    pose64 = orc["pose64"].numpy()
    rad = (inp["radius"][t] * np.float32(1.0 if mode == D.POLAR else cfg["data"]["novel_view_scale_factor"])).astype(np.float32)
    e = err32(pose32, pose64, rad)
    assert e.max() < 1e-5, (name, e)
    p = f"vv_{name}_"
    out.update({p + "mode": np.int64(mode), p + "a": a, p + "b": b, p + "c": np.zeros(0, np.float32) if c is None else c, p + "t": t,
                p + "ds_is_train": np.int64(ds_is_train), p + "scale": np.float64(np.nan if scale is None else scale),
                p + "H": np.int64(ref["H"]), p + "W": np.int64(ref["W"]), p + "deg": deg.astype(np.float32), p + "pose32": pose32,
                p + "pose64": pose64, p + "err32": e, p + "view_radius": rad})
    for k in ("rays_o", "rays_d", "rays_t", "rays_id", "dir", "polar", "azimuth", "radius"):
        out[p + k] = ref[k].numpy()
    # ---- the oracle against the reference
    assert (orc["H"], orc["W"]) == (ref["H"], ref["W"]), name
    for k in ("dir", "polar", "azimuth", "radius", "rays_t", "rays_id"):
        assert ref[k].dtype == orc[k].dtype and torch.equal(ref[k], orc[k]), (name, k, ref[k], orc[k])
    assert np.array_equal(deg, orc["deg"].numpy()), (name, deg, orc["deg"])
    o, d = D.rays(orc["K"], pose32, orc["H"], orc["W"])
    assert torch.equal(o, ref["rays_o"]) and torch.equal(d, ref["rays_d"]), name
    print(f"{name}: H x W = {ref['H']} x {ref['W']}, labels {ref['dir'].tolist()}, fp32 pose error {e}")


def main(ref):
    mod = load_module(ref)
    inp = D.make_inputs()
    out = {"in_" + k: v for k, v in inp.items()}
    ds = make_dataset(mod, inp, D.CONFIG)
    HW = D.H * D.W

    def record(tag, res, idx, index):
        out[tag + "idx"] = np.asarray(idx, np.int64)
        out[tag + "index"] = np.zeros(0, np.int32) if index is None else index.numpy().astype(np.int32)
        orc = D.real_view(inp, idx, None if index is None else index)
        assert (res["H"], res["W"]) == (orc["H"], orc["W"])
        assert torch.equal(res["intri"], orc["intri"])
        for k in D.REAL_KEYS:
            assert res[k].dtype == orc[k].dtype and res[k].shape == orc[k].shape and torch.equal(res[k], orc[k]), (tag, k)
            out[tag + k] = res[k].numpy()

    torch.manual_seed(7)
    res = ds.sample_real_view_rays(idx=torch.tensor([2, 2, 4]), ray_num=37)
    torch.manual_seed(7)
    index = torch.randint(0, HW, (37,))
    record("rv0_", res, [2, 2, 4], index)
    forced = index.clone()
    forced[:6] = torch.tensor([0, HW - 1, 5, 5, HW - 1, 0])
    with answers(mod, randint=forced):
        res = ds.sample_real_view_rays(idx=torch.tensor([2, 2, 4]), ray_num=37)
    record("rv1_", res, [2, 2, 4], forced)
    record("rv2_", ds.sample_real_view_rays(idx=3), [3], None)
    for tag in ("rv0_", "rv1_", "rv2_"):
        assert out[tag + "mask"].dtype == np.int64 and set(np.unique(out[tag + "mask"])) <= {0, 1}

    # ---- remove_outlier
    poses, rtp = D.outlier_sequence()
    ol = object.__new__(mod.DeformDataset)
    ol.num_frames = len(poses)
    ol.radius, ol.theta, ol.phi = (torch.from_numpy(rtp[:, k].copy()) for k in range(3))
    fixed = ol.remove_outlier(torch.from_numpy(poses.copy()))
    changed = [f for f in range(len(poses)) if not np.array_equal(fixed[f].numpy(), poses[f])]
    assert changed == [4, 5], changed
    out.update(ol_poses_in=poses, ol_rtp_in=rtp, ol_poses=fixed.numpy(), ol_radius=ol.radius.numpy(), ol_theta=ol.theta.numpy(),
               ol_phi=ol.phi.numpy())

    # ---- virtual views
    th, ph, t = box_draws()
    virtual_case(mod, inp, out, "box", D.ANGLES, th, ph, None, t, True, None)
    az = out["vv_box_azimuth"]
    assert (az < 0).any() and ((az > 100) & (az <= 180)).any()      # wrapped by -360, and left alone
    rng = np.random.default_rng(5)
    for k, (sc, sign) in enumerate(((0.35, (1, 1, 1)), (None, (1, -1, 1)), (None, (-1, 1, -1)))):
        n = (np.abs(rng.standard_normal(3)) * np.array(sign)).astype(np.float32)
        virtual_case(mod, inp, out, f"sphere{k}", D.SPHERE, n[0:1], n[1:2], n[2:3], np.array([k + 1], np.int64), True, sc)
    virtual_case(mod, inp, out, "polar0", D.POLAR, None, None, None, np.array([2], np.int64), False, None, phis_arg=0.3)
    virtual_case(mod, inp, out, "polar1", D.POLAR, None, None, None, np.array([4], np.int64), True, None, phis_arg=0.75)

    path = os.path.join(ROOT, "tests", "golden", "dataset.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
