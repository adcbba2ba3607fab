"""Build libmorpheus_hip.so (gfx950) in-tree with hipcc.

`python -m morpheus_amd.build` or morpheus_amd.build.build().  hipcc cross-compiles without a
GPU; the .so lands in morpheus_amd/_build/ (git-ignored, shipped to the GPU box by gpurun).
Each source is compiled to its own object (in parallel, only when it or a header changed), then linked.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT_DIR = os.path.join(HERE, "_build")
SO = os.path.join(OUT_DIR, "libmorpheus_hip.so")
SOURCES = ["hashgrid.hip", "hashgrid_general.hip", "composite.hip", "sampler.hip", "mlp.hip", "mlp_b3.hip", "optim.hip", "wnorm.hip", "normal.hip", "graph.hip", "losses.hip",
           "mesh.hip", "raster.hip", "mesheval.hip", "subdivide.hip", "tsdf.hip", "tsdf_sparse.hip", "visibility.hip", "adan.hip", "poseinit.hip", "encoders.hip", "volrend.hip", "dataset.hip", "preprocess.hip", "estimator.hip", "resample.hip"]
HEADER = os.path.join(HERE, "..", "include", "morpheus_hip.h")      # the C ABI; _lib.py binds the library from this text
HEADERS = [os.path.join(CSRC, "common.h"), HEADER]
# -fno-slp-vectorize: hipcc's SLP pass packs adjacent scalar fp32 adds / muls of the epilogues into v_pk_* instructions, which
# cost more than two plain ones beside MFMAs (MI355X_MICROARCH.md); measured on one box, whole library, cfg3: 15.61 -> 15.38
# ms/step (fused field backward 2.27 -> 2.17 ms, warp forward / backward-data -0.045 / -0.04, hash-grid backward -0.05).  Same
# IEEE results instruction for instruction.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize"] + os.environ.get("MH_EXTRA_FLAGS", "").split()
# losses.hip restates chains of rounded fp32 operators (the pose correction: R from six sin / cos, then R d): with hipcc's default
# -ffp-contract=fast the compiler fuses its products and sums into FMAs and R moves by an ulp -- enough to move SDF values next to
# zero past the counted parity gate (tests/test_gpu_losses.py compares with the operator chain bit for bit)
# mesh.hip: the vertex position (p + (iso - f0) / (f1 - f0)) is pinned bit for bit by tests/mc_oracle.py, the same reason
# raster.hip: projected positions, depth and coverage are pinned bit for bit by tests/raster_oracle.py, the same reason
# mesheval.hip: squared distances, sampled points and cull masks are pinned bit for bit by tests/mesheval_oracle.py, the same reason
# subdivide.hip: depths and the new vertices (float64, one rounding) are pinned bit for bit by tests/subdivide_oracle.py, the same reason
# tsdf.hip: the fused tsdf / weight / colour volumes and the active blocks are pinned bit for bit by tests/tsdf_oracle.py, the same reason
# tsdf_sparse.hip: the same voxels behind an index volume, pinned bit for bit against the dense store and tests/tsdf_sparse_oracle.py
# poseinit.hip: back-projected points, k nearest distances and the weighted sums' order are pinned by tests/poseinit_oracle.py, the same reason
# adan.hip: every operator of the reference's rule is rounded on its own there (tests/adan_oracle.py states the chain)
# encoders.hip: the spherical harmonics are the statements of sh_table.inc, walked bit for bit by tests/encoders_oracle.py
# dataset.hip: rays, conversions, view labels and degree values are pinned bit for bit by tests/dataset_oracle.py, the same reason as sampler.hip's pragma
# preprocess.hip: the float64 source coordinates and the bilinear sums of rotated frames are pinned bit for bit by tests/preprocess_oracle.py, the same reason
# estimator.hip: un-contracted by its own pragma, like sampler.hip (tests/estimator_oracle.py states the operations)
# resample.hip: un-contracted by its own pragma, the same way (tests/resample_oracle.py states the operations)
FILE_FLAGS = {"adan.hip": ["-ffp-contract=off"], "losses.hip": ["-ffp-contract=off"], "mesh.hip": ["-ffp-contract=off"], "raster.hip": ["-ffp-contract=off"],
              "mesheval.hip": ["-ffp-contract=off"], "subdivide.hip": ["-ffp-contract=off"], "tsdf.hip": ["-ffp-contract=off"],
              "tsdf_sparse.hip": ["-ffp-contract=off"], "poseinit.hip": ["-ffp-contract=off"], "encoders.hip": ["-ffp-contract=off"],
              "dataset.hip": ["-ffp-contract=off"], "preprocess.hip": ["-ffp-contract=off"]}


def _newer(deps, target) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _stale() -> bool:
    return _newer([os.path.join(CSRC, f) for f in os.listdir(CSRC)] + HEADERS, SO)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale():
        return SO
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OUT_DIR, exist_ok=True)
    extra = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h") or f.endswith(".inc")]

    def compile_one(src):
        obj = os.path.join(OUT_DIR, src.replace(".hip", ".o"))
        if force or _newer([os.path.join(CSRC, src)] + HEADERS + extra, obj):
            cmd = [hipcc] + FLAGS + FILE_FLAGS.get(src, []) + ["-c", os.path.join(CSRC, src), "-o", obj]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            subprocess.check_call(cmd)
        return obj

    with ThreadPoolExecutor(max_workers=len(SOURCES)) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO] + objs
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return SO


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
