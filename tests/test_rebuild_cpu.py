"""gbl_rebuild_mesh and gbl_mesh_tree_stats without a GPU.

 1. ABI     both entry points are declared in include/goblin_hip.h, mirrored in goblin_amd/_abi.py and exported by
            libgoblin_hip.so (without the feature this fails), GBL_ABI_VERSION stays 14, gbl_tree_stats has the C layout, and
            a NULL context is GBL_ERR_INVALID before anything touches a device.
 2. stats   the numpy restatement of the statistics (tests/rebuild_reference.py), run over the tables tests/refit_dump.cpp
            writes for the meshes of tests/meshes.py: the leaf slots' triangle counts sum to the mesh's tri_count, the leaves
            partition the mesh's range of the triangle table, and nodes and levels are the C++ plan's.  On a valid tree the sums
            are finite, every child's area is counted once, and node_cost is at least 1.

Every bar is exact.
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import meshes
import rebuild_reference as rb
import refit_reference as rr
from goblin_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "goblin_amd", "lib")
CSRC = os.path.join(REPO, "goblin_amd", "csrc")
GENERATED = {"all": meshes.ALL, "deep_spiral": ["deep_spiral"], "tiny": ["tiny"], "degenerate": ["degenerate"]}
NAMES = ("gbl_rebuild_mesh", "gbl_mesh_tree_stats")


def test_abi(tmp_path):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "goblin_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+GBL_ABI_VERSION\s+14\b", header) and _abi.GBL_ABI_VERSION == 14
    lib = _abi.hip_lib()   # dlopen only; no compute without a GPU
    assert lib.gbl_abi_version() == 14
    for name in NAMES:
        assert re.search(r"\bgbl_status\s+%s\s*\(" % name, header), name
        assert name in _abi.HIP_SYMBOLS
        assert getattr(lib, name) is not None, name
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "goblin_hip.h"\nint main(void){\n'
                   'printf("%zu %zu %zu %zu\\n", sizeof(gbl_tree_stats), offsetof(gbl_tree_stats, leaves), offsetof(gbl_tree_stats, root_area), '
                   'offsetof(gbl_tree_stats, tri_area));\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    T = _abi.gbl_tree_stats
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [C.sizeof(T), T.leaves.offset, T.root_area.offset, T.tri_area.offset]


def test_a_null_context_is_invalid():
    lib = _abi.hip_lib()
    out = _abi.gbl_tree_stats()
    assert lib.gbl_rebuild_mesh(None, 0, 0) == _abi.GBL_ERR_INVALID
    assert lib.gbl_mesh_tree_stats(None, 0, C.byref(out)) == _abi.GBL_ERR_INVALID


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """name -> the tables tests/refit_dump.cpp writes for the generated scene `name`, the host builder's."""
    work = tmp_path_factory.mktemp("rebuild")
    exe = os.path.join(str(work), "refit_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(REPO, "tests", "refit_dump.cpp"),
                           os.path.join(CSRC, "scene_prep.cpp"), os.path.join(CSRC, "scene_refit.cpp"), "-o", exe, "-L" + LIB, "-lgoblin_host",
                           "-Wl,-rpath," + LIB, "-lpthread"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("GBL_")}   # the builders' tuning knobs
    scene_dir = work / "scenes"
    scene_dir.mkdir()
    meshes.write_meshes(scene_dir, meshes.ALL)
    out = {}
    for name, names in GENERATED.items():
        path = str(scene_dir / (name + ".json"))
        with open(path, "w") as f:
            json.dump(meshes.scene_doc(names), f)
        d = work / ("dump_" + name)
        d.mkdir()
        subprocess.check_call([exe, str(d), path], env=env)
        t = {"nodes": np.fromfile(str(d / "nodes"), rr.NODE), "mesh_root": np.fromfile(str(d / "mesh_root"), np.int32),
             "meshes": np.fromfile(str(d / "meshes"), np.uint32).reshape(-1, 6), "plans": {}}
        for m, row in enumerate(t["meshes"]):
            if row[0] == 0:   # GBL_SHAPE_MESH
                t["plans"][m] = (np.fromfile(str(d / ("plan_%d" % m)), rr.RECORD), [int(x) for x in np.fromfile(str(d / ("levels_%d" % m)), np.uint32)])
        out[name] = t
    return out


@pytest.mark.parametrize("name", list(GENERATED))
def test_the_restated_statistics_describe_the_packed_trees(dumps, name):
    d = dumps[name]
    trees = 0
    for m, (records, level_first) in d["plans"].items():
        tri_count, tri_first = int(d["meshes"][m][4]), int(d["meshes"][m][5])
        s = rb.tree_stats(d["nodes"], d["mesh_root"][m])
        assert s["nodes"] == len(records) and s["levels"] == max(0, len(level_first) - 1), (name, m)
        assert s["leaves"] == len(s["leaf_ranges"])
        assert sum(c for _, c in s["leaf_ranges"]) == tri_count, (name, m)
        covered = np.zeros(tri_count, np.int64)                 # the leaves partition the mesh's range
        for first, count in s["leaf_ranges"]:
            assert tri_first <= first and first + count <= tri_first + tri_count, (name, m, first, count)
            covered[first - tri_first:first - tri_first + count] += 1
        assert (covered == 1).all(), (name, m)
        node_cost, tri_cost = rb.costs(s)
        if s["nodes"] == 0:
            assert (s["leaves"], s["root_area"], s["node_area"], s["tri_area"], node_cost, tri_cost) == (1, 0.0, 0.0, 0.0, 0.0, 0.0)
            continue
        trees += 1
        assert s["terms"] == (s["nodes"] - 1, s["leaves"])      # every node but the root is some slot's interior child
        assert all(np.isfinite([s["root_area"], s["node_area"], s["tri_area"]])) and min(s["root_area"], s["node_area"], s["tri_area"]) >= 0.0
        assert node_cost >= 1.0 and tri_cost >= 0.0
        print(name, m, {k: s[k] for k in ("nodes", "levels", "leaves")}, "node_cost %.3f tri_cost %.3f" % (node_cost, tri_cost))
    assert trees > 0
