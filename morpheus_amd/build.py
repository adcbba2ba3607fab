"""Build libmorpheus_hip.so (gfx950) in-tree with hipcc.

`python -m morpheus_amd.build` or morpheus_amd.build.build().  hipcc cross-compiles without a
GPU; the .so lands in morpheus_amd/_build/ (git-ignored, shipped to the GPU box by gpurun).
Each source is compiled to its own object (in parallel, only when it, a header or its command line changed), then linked.

build_library() is the one recipe that turns a source tree into a library; the product build and every side build for a same-box
A/B (loaded through MORPHEUS_HIP_LIB) go through it with the same per-file flags:
  python -m morpheus_amd.build [--force]                             the product, morpheus_amd/_build/libmorpheus_hip.so
  python -m morpheus_amd.build --name NAME [--rev REV] [-- FLAG ...]   morpheus_amd/_build/libmorpheus_NAME.so: the working tree, or
      revision REV with that revision's own SOURCES / FLAGS / FILE_FLAGS, compiled with FLAG ... behind the product's flags
"""
from __future__ import annotations

import argparse
import io
import os
import runpy
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OUT_DIR = os.path.join(HERE, "_build")
SO = os.path.join(OUT_DIR, "libmorpheus_hip.so")
SOURCES = ["hashgrid.hip", "hashgrid_general.hip", "composite.hip", "sampler.hip", "mlp.hip", "mlp_b3.hip", "optim.hip", "wnorm.hip", "normal.hip", "graph.hip", "losses.hip",
           "mesh.hip", "raster.hip", "mesheval.hip", "subdivide.hip", "tsdf.hip", "tsdf_sparse.hip", "visibility.hip", "adan.hip", "poseinit.hip", "encoders.hip", "volrend.hip", "dataset.hip", "preprocess.hip", "estimator.hip", "resample.hip", "imageops.hip", "guidance.hip", "video.hip"]
HEADER = os.path.join(HERE, "..", "include", "morpheus_hip.h")      # the C ABI; _lib.py binds the library from this text
# -fno-slp-vectorize: hipcc's SLP pass packs adjacent scalar fp32 adds / muls of the epilogues into v_pk_* instructions, which
# cost more than two plain ones beside MFMAs (MI355X_MICROARCH.md); measured on one box, whole library, cfg3: 15.61 -> 15.38
# ms/step (fused field backward 2.27 -> 2.17 ms, warp forward / backward-data -0.045 / -0.04, hash-grid backward -0.05).  Same
# IEEE results instruction for instruction.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize"] + os.environ.get("MH_EXTRA_FLAGS", "").split()
# losses.hip restates chains of rounded fp32 operators (the pose correction: R from six sin / cos, then R d): with hipcc's default
# -ffp-contract=fast the compiler fuses its products and sums into FMAs and R moves by an ulp -- enough to move SDF values next to
# zero past the counted parity gate (tests/test_gpu_losses.py compares with the operator chain bit for bit).  A pragma on the file's
# first line is not enough there: the flag also reaches library code inlined into pose_apply_kernel and render_loss_kernel, which a
# pragma in the file never sees (80 against 90 and 24 against 26 FMAs), so this table, not the sources, states each file's arithmetic
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
# imageops.hip, guidance.hip: un-contracted by their own pragmas, the same way (tests/imageops_oracle.py, tests/guidance_oracle.py)
# video.hip: integer arithmetic only (tests/video_oracle.py): nothing to contract, neither a pragma nor an entry here
FILE_FLAGS = {"adan.hip": ["-ffp-contract=off"], "losses.hip": ["-ffp-contract=off"], "mesh.hip": ["-ffp-contract=off"], "raster.hip": ["-ffp-contract=off"],
              "mesheval.hip": ["-ffp-contract=off"], "subdivide.hip": ["-ffp-contract=off"], "tsdf.hip": ["-ffp-contract=off"],
              "tsdf_sparse.hip": ["-ffp-contract=off"], "poseinit.hip": ["-ffp-contract=off"], "encoders.hip": ["-ffp-contract=off"],
              "dataset.hip": ["-ffp-contract=off"], "preprocess.hip": ["-ffp-contract=off"]}


def _newer(deps, target) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _hipcc() -> str:
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _recorded(obj):
    try:
        with open(obj + ".cmd") as f:
            return f.read()
    except OSError:
        return None


def _plan(root, obj_dir, extra_flags, tables):
    """One (obj, cmd, record, deps) per source of the tree at `root`, laid out like the repository.  `record` is `cmd` with its two
    paths written relative to the tree and to the object directory: the text kept beside the object as <obj>.cmd, which a moved
    tree or another unpacking of the same revision must not change."""
    sources, flags, file_flags = tables or (SOURCES, FLAGS, FILE_FLAGS)
    csrc = os.path.join(root, "morpheus_amd", "csrc")
    shared = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".inc"))] + [os.path.join(root, "include", "morpheus_hip.h")]
    plan = []
    for src in sources:
        name = src.replace(".hip", ".o")
        head = [_hipcc()] + list(flags) + list(file_flags.get(src, [])) + list(extra_flags)
        obj = os.path.join(obj_dir, name)
        plan.append((obj, head + ["-c", os.path.join(csrc, src), "-o", obj],
                     " ".join(head + ["-c", "morpheus_amd/csrc/" + src, "-o", name]) + "\n", [os.path.join(csrc, src)] + shared))
    return plan


def _stale(so, plan) -> bool:
    """The library is older than a source, a header or an object that is there, or an object's recorded command is missing or is
    not the one this build would run.  (Objects may be absent beside a complete library: they do not travel with it.)"""
    inputs = {d for _, _, _, deps in plan for d in deps} | {obj for obj, _, _, _ in plan if os.path.exists(obj)}
    return _newer(inputs, so) or any(_recorded(obj) != record for obj, _, record, _ in plan)


def build_library(root, so, *, obj_dir, extra_flags=(), tables=None, force=False, verbose=False) -> str:
    """Compile the tree at `root` (morpheus_amd/csrc, include/) into the shared library `so`, objects and their command records in
    `obj_dir`: every source with FLAGS + FILE_FLAGS[src] + extra_flags, the three tables being this module's or `tables` =
    (SOURCES, FLAGS, FILE_FLAGS) of another revision.  An object is rebuilt when a dependency is newer, or when the command recorded
    beside it is missing or differs; the link is written beside `so` and moved over it, so a reader never maps a partial file."""
    plan = _plan(root, obj_dir, extra_flags, tables)
    if not force and not _stale(so, plan):
        return so
    os.makedirs(obj_dir, exist_ok=True)
    os.makedirs(os.path.dirname(so), exist_ok=True)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)

    def compile_one(job):
        obj, cmd, record, deps = job
        if force or _newer(deps, obj) or _recorded(obj) != record:
            if os.path.exists(obj + ".cmd"):
                os.remove(obj + ".cmd")              # an interrupted compile leaves no record that vouches for its object
            run(cmd)
            with open(obj + ".cmd", "w") as f:
                f.write(record)
        return obj

    jobs = int(os.environ["MAX_JOBS"]) if os.environ.get("MAX_JOBS") else min(16, os.cpu_count() or 1)
    with ThreadPoolExecutor(max_workers=max(1, min(len(plan), jobs))) as ex:
        objs = list(ex.map(compile_one, plan))
    tmp = f"{so}.{os.getpid()}.tmp"
    try:
        run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + objs)
        os.replace(tmp, so)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return so


def build(force: bool = False, verbose: bool = False) -> str:
    return build_library(ROOT, SO, obj_dir=OUT_DIR, force=force, verbose=verbose)


def build_named(name, rev=None, extra_flags=(), *, root=ROOT, tables=None, force=False, verbose=False) -> str:
    """A side build for a same-box A/B: <root>/morpheus_amd/_build/libmorpheus_<name>.so, objects under _build/obj/<name>/, of
    the working tree at `root` or of its git revision `rev`.  A revision is compiled with its own build.py's three tables by this
    tree's procedure: the way that revision's product library was built, also across a commit that changes a flag."""
    if name == "hip" or not name or os.sep in name:
        raise ValueError(f"--name {name!r}: libmorpheus_hip.so is the product's library; a side build needs a name of its own")
    out = os.path.join(root, "morpheus_amd", "_build")
    so, obj_dir = os.path.join(out, f"libmorpheus_{name}.so"), os.path.join(out, "obj", name)
    if rev is None:
        return build_library(root, so, obj_dir=obj_dir, extra_flags=extra_flags, tables=tables, force=force, verbose=verbose)
    archive = subprocess.run(["git", "-C", root, "archive", rev, "morpheus_amd/csrc", "include", "morpheus_amd/build.py"],
                             check=True, stdout=subprocess.PIPE).stdout
    with tempfile.TemporaryDirectory() as tree:
        tarfile.open(fileobj=io.BytesIO(archive)).extractall(tree)
        their = runpy.run_path(os.path.join(tree, "morpheus_amd", "build.py"))
        # force: the unpacked files carry the commit's time, which says nothing about objects that another revision left here
        return build_library(tree, so, obj_dir=obj_dir, extra_flags=extra_flags, force=True, verbose=verbose,
                             tables=(their["SOURCES"], their["FLAGS"], their["FILE_FLAGS"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--force", action="store_true", help="recompile every object")
    ap.add_argument("--name", help="build morpheus_amd/_build/libmorpheus_NAME.so beside the product instead of the product")
    ap.add_argument("--rev", help="with --name: build this git revision, with its own flag tables")
    ap.add_argument("flags", nargs="*", help="with --name: extra compiler flags, after `--`")
    a = ap.parse_args()
    if a.name is None:
        if a.rev or a.flags:
            ap.error("--rev and extra flags belong to a named build (--name NAME); the product takes MH_EXTRA_FLAGS")
        print(build(force=a.force, verbose=True))
    else:
        print(build_named(a.name, a.rev, a.flags, force=a.force, verbose=True))
