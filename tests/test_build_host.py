"""CPU, no compiler run: the one build recipe of morpheus_amd/build.py -- per-file flags in the product and in every side build,
the command line as part of staleness, side builds that leave the product alone, a revision's own flag tables, the atomic link and
the bounded pool.  HIPCC points at a stub that logs its argv and creates its -o file, so every test runs in milliseconds."""
import json
import os
import subprocess
import sys
import time

import pytest

from morpheus_amd import build

SOURCES = ["a.hip", "b.hip", "c.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3"]
FILE_FLAGS = {"b.hip": ["-ffp-contract=off"]}
TABLES = (SOURCES, FLAGS, FILE_FLAGS)

STUB = """#!{python}
import json, os, sys, time
argv = sys.argv[1:]
out = argv[argv.index("-o") + 1]
final = os.environ.get("STUB_FINAL_SO")
seen = None
if "-shared" in argv and final:                 # the "linker": what stands at the library's final path while it runs
    seen = open(final).read() if os.path.exists(final) else None
t0 = time.time()
time.sleep(float(os.environ.get("STUB_SLEEP", "0")))
with open(out, "w") as f:
    f.write("built at %r by %s" % (t0, " ".join(argv)))
with open({log!r}, "a") as f:
    f.write(json.dumps({{"argv": argv, "t0": t0, "t1": time.time(), "seen": seen}}) + "\\n")
"""


def make_tree(root, sources=SOURCES):
    os.makedirs(os.path.join(root, "morpheus_amd", "csrc"))
    os.makedirs(os.path.join(root, "include"))
    for f in list(sources) + ["common.h"]:
        open(os.path.join(root, "morpheus_amd", "csrc", f), "w").close()
    open(os.path.join(root, "include", "morpheus_hip.h"), "w").close()
    past = time.time() - 100                     # every input is older than anything the stub writes
    for d, _, files in os.walk(root):
        for f in files:
            os.utime(os.path.join(d, f), (past, past))


class Tree:
    def __init__(self, tmp_path, monkeypatch):
        self.root = str(tmp_path / "tree")
        make_tree(self.root)
        self.log = str(tmp_path / "stub.log")
        stub = str(tmp_path / "hipcc_stub")
        with open(stub, "w") as f:
            f.write(STUB.format(python=sys.executable, log=self.log))
        os.chmod(stub, 0o755)
        monkeypatch.setenv("HIPCC", stub)
        monkeypatch.delenv("MAX_JOBS", raising=False)
        self.out = os.path.join(self.root, "morpheus_amd", "_build")
        self.so = os.path.join(self.out, "libmorpheus_hip.so")

    def csrc(self, f):
        return os.path.join(self.root, "morpheus_amd", "csrc", f)

    def product(self, **kw):
        """a product-shaped build: the library and its objects where build() puts them"""
        return build.build_library(self.root, self.so, obj_dir=self.out, tables=TABLES, **kw)

    def runs(self):
        """the stub's runs since the last look, as argv lists"""
        if not os.path.exists(self.log):
            return []
        with open(self.log) as f:
            calls = [json.loads(line) for line in f]
        os.remove(self.log)
        return calls

    def compiled(self):
        """{source name: argv} and the link's argv (None when nothing was linked) of the runs since the last look"""
        calls = [c["argv"] for c in self.runs()]
        links = [a for a in calls if "-shared" in a]
        assert len(links) <= 1
        return {os.path.basename(a[a.index("-c") + 1]): a for a in calls if "-c" in a}, (links[0] if links else None)


@pytest.fixture
def tree(tmp_path, monkeypatch):
    return Tree(tmp_path, monkeypatch)


def touch(path):
    now = time.time() + 5                        # newer than the objects, whatever the file system's time stamps resolve
    os.utime(path, (now, now))


# ---- flags

def test_product_build_carries_flags_and_file_flags(tree):
    assert tree.product() == tree.so and os.path.exists(tree.so)
    objs, link = tree.compiled()
    assert sorted(objs) == SOURCES
    for src, argv in objs.items():
        obj = os.path.join(tree.out, src.replace(".hip", ".o"))
        assert argv == FLAGS + FILE_FLAGS.get(src, []) + ["-c", tree.csrc(src), "-o", obj]
        assert os.path.exists(obj)
    assert [a for a in link if a.endswith(".o")] == [os.path.join(tree.out, s.replace(".hip", ".o")) for s in SOURCES]


def test_named_build_carries_the_same_flags_with_the_extras_behind(tree):
    so = build.build_named("trace", None, ["-DMH_PHASE_TRACE", "-DX=1"], root=tree.root, tables=TABLES)
    assert so == os.path.join(tree.out, "libmorpheus_trace.so") and os.path.exists(so)
    objs, _ = tree.compiled()
    assert sorted(objs) == SOURCES
    for src, argv in objs.items():
        obj = os.path.join(tree.out, "obj", "trace", src.replace(".hip", ".o"))
        assert argv == FLAGS + FILE_FLAGS.get(src, []) + ["-DMH_PHASE_TRACE", "-DX=1", "-c", tree.csrc(src), "-o", obj]


def test_real_tables_uncontract_the_same_twelve_files_in_both_kinds_of_build(tree):
    uncontracted = {"adan.hip", "losses.hip", "mesh.hip", "raster.hip", "mesheval.hip", "subdivide.hip", "tsdf.hip", "tsdf_sparse.hip",
                    "poseinit.hip", "encoders.hip", "dataset.hip", "preprocess.hip"}
    assert set(build.FILE_FLAGS) == uncontracted
    for f in build.SOURCES:
        open(tree.csrc(f), "w").close()
    build.build_library(tree.root, tree.so, obj_dir=tree.out)                  # tables=None: the module's own, as build() uses them
    product, _ = tree.compiled()
    build.build_named("variant", None, ["-DX"], root=tree.root)
    named, _ = tree.compiled()
    for objs in (product, named):
        assert sorted(objs) == sorted(build.SOURCES)
        assert {src for src, argv in objs.items() if "-ffp-contract=off" in argv} == uncontracted
        for src, argv in objs.items():
            assert argv[:len(build.FLAGS)] == build.FLAGS and argv.count("-ffp-contract=off") == (src in uncontracted)


# ---- staleness

def test_second_build_runs_nothing(tree):
    tree.product()
    assert len(tree.runs()) == len(SOURCES) + 1
    tree.product()
    assert tree.runs() == []


def test_changed_extra_flags_recompile_everything_and_relink(tree):
    tree.product()
    tree.runs()
    tree.product(extra_flags=["-DMH_PHASE_TRACE"])
    objs, link = tree.compiled()
    assert sorted(objs) == SOURCES and link is not None and all("-DMH_PHASE_TRACE" in a for a in objs.values())
    tree.product(extra_flags=["-DMH_PHASE_TRACE"])
    assert tree.runs() == []
    tree.product()                                                             # and back: the plain build is not the library that is there
    objs, link = tree.compiled()
    assert sorted(objs) == SOURCES and link is not None and not any("-DMH_PHASE_TRACE" in a for a in objs.values())


def test_changed_flag_table_rebuilds_through_stale_alone(tree, monkeypatch):
    """MH_EXTRA_FLAGS reaches the build through FLAGS: another FLAGS with nothing else changed is another build"""
    tree.product()
    tree.runs()
    build.build_library(tree.root, tree.so, obj_dir=tree.out, tables=(SOURCES, FLAGS + ["-DX"], FILE_FLAGS))
    objs, link = tree.compiled()
    assert sorted(objs) == SOURCES and link is not None


def test_touched_source_recompiles_that_object(tree):
    tree.product()
    tree.runs()
    touch(tree.csrc("b.hip"))
    tree.product()
    objs, link = tree.compiled()
    assert sorted(objs) == ["b.hip"] and link is not None


@pytest.mark.parametrize("header", ["morpheus_amd/csrc/common.h", "include/morpheus_hip.h"])
def test_touched_header_recompiles_every_object(tree, header):
    tree.product()
    tree.runs()
    touch(os.path.join(tree.root, header))
    tree.product()
    objs, link = tree.compiled()
    assert sorted(objs) == SOURCES and link is not None


def test_deleted_command_record_recompiles_that_object(tree):
    tree.product()
    tree.runs()
    record = os.path.join(tree.out, "c.o.cmd")
    assert "-c morpheus_amd/csrc/c.hip -o c.o" in open(record).read()
    os.remove(record)
    tree.product()
    objs, link = tree.compiled()
    assert sorted(objs) == ["c.hip"] and link is not None and os.path.exists(record)


def test_library_without_its_objects_is_not_stale(tree):
    """a complete library travels without its objects (they are large); the records that travel with it still vouch for it"""
    tree.product()
    tree.runs()
    for s in SOURCES:
        os.remove(os.path.join(tree.out, s.replace(".hip", ".o")))
    tree.product()
    assert tree.runs() == []


# ---- isolation

def test_named_build_leaves_the_product_alone(tree):
    build.build_named("side", None, ["-DX"], root=tree.root, tables=TABLES)
    made = sorted(os.path.relpath(os.path.join(d, f), tree.out) for d, _, files in os.walk(tree.out) for f in files)
    assert made == sorted(["libmorpheus_side.so"] + [f"obj/side/{n}.o{e}" for n in "abc" for e in ("", ".cmd")])
    tree.product()
    before = {p: (os.stat(p).st_mtime_ns, open(p).read()) for p in
              [tree.so] + [os.path.join(tree.out, n + e) for n in "abc" for e in (".o", ".o.cmd")]}
    tree.runs()
    build.build_named("side", None, ["-DY"], root=tree.root, tables=TABLES, force=True)
    assert len(tree.runs()) == len(SOURCES) + 1
    assert {p: (os.stat(p).st_mtime_ns, open(p).read()) for p in before} == before


def test_name_hip_is_refused(tree):
    with pytest.raises(ValueError):
        build.build_named("hip", None, [], root=tree.root, tables=TABLES)
    assert tree.runs() == [] and not os.path.exists(tree.out)
    r = subprocess.run([sys.executable, "-m", "morpheus_amd.build", "--name", "hip"], capture_output=True, text=True,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(build.__file__))))
    assert r.returncode != 0 and "ValueError" in r.stderr and tree.runs() == []


# ---- a revision's own tables

def test_rev_build_takes_the_revisions_own_tables(tree):
    def git(*args):
        subprocess.run(["git", "-C", tree.root, "-c", "user.name=t", "-c", "user.email=t@t", *args], check=True, capture_output=True)

    def commit(file_flags):
        with open(os.path.join(tree.root, "morpheus_amd", "build.py"), "w") as f:
            f.write(f"SOURCES = {SOURCES!r}\nFLAGS = {FLAGS!r}\nFILE_FLAGS = {file_flags!r}\n")
        git("add", "-A")
        git("commit", "-q", "-m", "tables")

    git("init", "-q")
    commit({"a.hip": ["-ffp-contract=off"]})
    first = subprocess.run(["git", "-C", tree.root, "rev-parse", "HEAD"], check=True, capture_output=True, text=True).stdout.strip()
    commit({})
    so = build.build_named("head", first, [], root=tree.root)
    assert so == os.path.join(tree.out, "libmorpheus_head.so") and os.path.exists(so)
    objs, _ = tree.compiled()
    assert sorted(objs) == SOURCES
    assert "-ffp-contract=off" in objs["a.hip"] and not any("-ffp-contract=off" in objs[s] for s in ("b.hip", "c.hip"))
    assert not objs["a.hip"][objs["a.hip"].index("-c") + 1].startswith(tree.root)           # the unpacked revision, not the working tree
    build.build_named("tree", None, [], root=tree.root, tables=(SOURCES, FLAGS, {}))         # the working tree's table has none
    objs, _ = tree.compiled()
    assert not any("-ffp-contract=off" in a for a in objs.values())


# ---- the link

def test_link_is_written_beside_the_library_and_moved_over_it(tree, monkeypatch):
    monkeypatch.setenv("STUB_FINAL_SO", tree.so)
    tree.product()
    (link,) = [c for c in tree.runs() if "-shared" in c["argv"]]
    target = link["argv"][link["argv"].index("-o") + 1]
    assert target != tree.so and os.path.dirname(target) == os.path.dirname(tree.so)
    assert link["seen"] is None                                                # first build: nothing at the final path while linking
    previous = open(tree.so).read()
    tree.product(extra_flags=["-DX"])
    (link,) = [c for c in tree.runs() if "-shared" in c["argv"]]
    assert link["seen"] == previous                                            # the previous complete file, until the move
    assert open(tree.so).read() != previous
    assert sorted(f for f in os.listdir(tree.out) if "libmorpheus" in f) == ["libmorpheus_hip.so"]      # no temporary left behind


# ---- the pool

def test_pool_is_bounded_by_max_jobs(tmp_path, monkeypatch):
    many = [f"s{i}.hip" for i in range(8)]
    t = Tree(tmp_path, monkeypatch)
    for f in many:
        open(t.csrc(f), "w").close()
    monkeypatch.setenv("MAX_JOBS", "3")
    monkeypatch.setenv("STUB_SLEEP", "0.05")
    build.build_library(t.root, t.so, obj_dir=t.out, tables=(many, FLAGS, {}))
    spans = [(c["t0"], c["t1"]) for c in t.runs() if "-c" in c["argv"]]
    assert len(spans) == len(many)
    assert max(sum(1 for a, b in spans if a <= t0 < b) for t0, _ in spans) <= 3


# ---- SOURCES is the directory

def test_sources_are_the_hip_files_of_csrc():
    assert sorted(build.SOURCES) == sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))
    assert len(set(build.SOURCES)) == len(build.SOURCES) and set(build.FILE_FLAGS) <= set(build.SOURCES)
