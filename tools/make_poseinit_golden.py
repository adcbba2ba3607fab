"""Record tests/golden/poseinit.npz from the reference's own preprocess/pose_init/registrate.py (build container only).

    python tools/make_poseinit_golden.py REF        # REF: a checkout of the reference

registrate.py calls an external registration program through os.system and reads the matrix it leaves behind.  That program is
not available anywhere; what this records is everything AROUND it: back-projection, centring, how the matrices are composed in the
three modes, the world points and the radius.  So the tool writes a small stand-in executable of its own (this file's code, not
the reference's) that takes the program's four arguments (target .obj, source .obj, record prefix, method) and writes a PRESCRIBED
matrix to <prefix>m3trans.txt, and runs registrate.py as __main__ (runpy) for --rigid_registrate 0, 1 and 2 on a temporary data
directory of 4 synthetic 24 x 32 frames.  The fixture holds data only: the frames (raw depth and mask images as arrays), the
intrinsics, the prescribed matrices, and per mode transformations.npy and radius.txt; and mask2camera's output per frame.
"""
from __future__ import annotations

import math
import os
import runpy
import stat
import sys
import tempfile

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "poseinit.npz")
H, W, FRAMES = 24, 32, 4

STAND_IN = """#!{python}
# stand-in for the registration program: <target.obj> <source.obj> <record prefix> <method> -> <prefix>m3trans.txt
import os, shutil, sys
target, source, prefix, method = sys.argv[1:5]
assert method == "3" and os.path.exists(target) and os.path.exists(source), sys.argv
frame = int(os.path.basename(prefix).rstrip("_"))
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "calls.txt"), "a") as fh:
    print(frame, os.path.basename(target), os.path.basename(source), file=fh)
shutil.copy(os.path.join(os.path.dirname(os.path.abspath(__file__)), "prescribed_%d.txt" % frame), prefix + "m3trans.txt")
"""


def rigid(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    m = np.eye(4)
    m[:3, :3] = Rz @ Ry @ Rx
    m[:3, 3] = t
    return m


def frames():
    """4 frames: a bumpy blob in front of a far wall.  Raw depth in millimetres (uint16) with holes (0) inside the mask; masks
    with the values around the 0.5 rule (127 / 128), one of them a colour image whose channels differ."""
    rng = np.random.default_rng(20240611)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    depths, masks = [], []
    for i in range(FRAMES):
        cu, cv = 15.0 + 1.5 * i, 11.0 - 0.7 * i
        r2 = ((u - cu) / 11.0) ** 2 + ((v - cv) / 8.0) ** 2
        z = 0.9 + 0.03 * i - 0.25 * np.sqrt(np.maximum(1.0 - r2, 0.0)) + 0.02 * np.sin(0.9 * u + i) * np.cos(0.7 * v)
        z = np.where(r2 < 1.0, z, 2.5)
        raw = np.rint(z * 1000.0).astype(np.uint16)
        raw[rng.random((H, W)) < 0.04] = 0                         # holes: no depth
        m = np.where(r2 < 1.0, 255, 0).astype(np.uint8)
        edge = (r2 >= 0.8) & (r2 < 1.0)
        m[edge] = np.where(rng.random(edge.sum()) < 0.5, 128, 127)  # 128 / 255 > 0.5 >= 127 / 255
        m[2, 3] = 255                                              # a stray pixel on the wall
        if i == 1:                                                 # a colour mask: mean of three channels
            m = np.stack([m, m, m], axis=-1)
            m[5, 14] = (255, 255, 0)                               # 2/3 > 0.5
            m[6, 14] = (255, 0, 0)                                 # 1/3
        depths.append(raw)
        masks.append(m)
    return depths, masks


def main(ref):
    script = os.path.join(ref, "preprocess", "pose_init", "registrate.py")
    K = np.array([[40.0, 0.0, 15.5], [0.0, 42.0, 11.25], [0.0, 0.0, 1.0]])
    prescribed = np.stack([np.eye(4)] + [rigid(0.05 * i, -0.08 * i, 0.03 * i, (0.01 * i, -0.02, 0.015 * i)) for i in range(1, FRAMES)])
    depths, masks = frames()
    out = {"K": K, "prescribed": prescribed, "depth_scale": np.array(1000.0)}
    for i in range(FRAMES):
        out[f"depth_{i}"], out[f"mask_{i}"] = depths[i], masks[i]
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "data") + os.sep                  # registrate.py concatenates: the separator is part of the path
        os.makedirs(data + "depth")
        os.makedirs(data + "mask")
        np.savetxt(data + "intrinsics.txt", K)
        for i in range(FRAMES):
            Image.fromarray(depths[i]).save(data + "depth/%06d.png" % i)
            Image.fromarray(masks[i]).save(data + "mask/%06d.png" % i)
            np.savetxt(os.path.join(tmp, "prescribed_%d.txt" % i), prescribed[i])
        exe = os.path.join(tmp, "stand_in")
        with open(exe, "w") as fh:
            fh.write(STAND_IN.format(python=sys.executable))
        os.chmod(exe, os.stat(exe).st_mode | stat.S_IXUSR)
        argv = sys.argv
        for mode in (0, 1, 2):
            sys.argv = [script, "--data_path", data, "--depth_scale", "1000.0", "--registration_alg_path", exe,
                        "--rigid_registrate", str(mode)]
            try:
                runpy.run_path(script, run_name="__main__")
            finally:
                sys.argv = argv
            out[f"transformations_{mode}"] = np.load(data + "intermediate/transformations.npy")
            out[f"radius_{mode}"] = np.loadtxt(data + "intermediate/radius.txt")
            assert out[f"transformations_{mode}"].shape == (FRAMES, 16)
        calls = open(os.path.join(tmp, "calls.txt")).read().split("\n")
        assert len([c for c in calls if c]) == 2 * (FRAMES - 1), calls   # modes 1 and 2 called the stand-in once per later frame
        fns = runpy.run_path(script, run_name="registrate")        # its functions, without its main block
        for i in range(FRAMES):
            depth = fns["depth_read"](data + "depth/%06d.png" % i, 1000.0)
            mask = fns["mask_read"](data + "mask/%06d.png" % i) * (depth != -1.)
            out[f"points_{i}"] = np.asarray(fns["mask2camera"](mask, depth, [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]))
            out[f"kept_{i}"] = (mask != 0).astype(np.uint8)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes;", {k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
