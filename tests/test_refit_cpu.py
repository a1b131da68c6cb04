"""Vertex edits without a GPU: tests/refit_dump.cpp is compiled with g++ against goblin_amd/csrc/scene_prep.cpp,
goblin_amd/csrc/scene_refit.cpp and libgoblin_host.so (without the feature it does not compile), packs scenes with the host
builder and dumps the tables a vertex edit touches together with the plan scene_refit.cpp builds per mesh.  Against them:

 1. identity   the numpy restatement of the refit (tests/refit_reference.py), run over the scene's own positions, reproduces
               nodes, tris and tri_bounds_leaf byte for byte: the restated quantiser IS Flat4::emit's;
 2. plan       the C++ plan equals the restated walk, holds every node reachable by reference from the mesh's root exactly
               once, a child one level below its parent, and is empty for a mesh whose root is a leaf;
 3. conservative  after a jitter and after a stretch every quantised child box, evaluated in float32, contains every vertex of
               every triangle beneath the child, and contains the exact extent of the child's own four boxes.  (Of their
               QUANTISED extent that cannot be asked: a child rounds its boxes outwards on its own grid, by up to one step
               of that grid, while its parent rounds the child's exact box outwards on another; the packers' own trees
               break that nesting -- on bunny.json as packed, at 9284 of the 18618 interior child slots -- and no kernel
               needs it: a ray that misses the parent's box for a child never looks at the child's boxes.)
 4. ABI        GBL_ABI_VERSION stays 14 and the three entry points are declared, mirrored and exported.

Every bar is exact: equality of bytes, containment without a tolerance.
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import meshes
import refit_reference as rr
from goblin_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "goblin_amd", "lib")
CSRC = os.path.join(REPO, "goblin_amd", "csrc")
SCENES = os.path.join(REPO, "goblin_amd", "scenes")
GENERATED = {"all": meshes.ALL, "deep_spiral": ["deep_spiral"], "tiny": ["tiny"], "degenerate": ["degenerate"]}
SHIPPED = ["bunny", "cornell", "grid"]
NAMES = ("gbl_update_vertices", "gbl_get_vertices", "gbl_selftest_geometry")


@pytest.fixture(scope="module")
def dumper(tmp_path_factory):
    """dump(name) -> the dumped tables of a scene as numpy arrays, computed once per scene."""
    work = tmp_path_factory.mktemp("refit")
    exe = os.path.join(str(work), "refit_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(REPO, "tests", "refit_dump.cpp"),
                           os.path.join(CSRC, "scene_prep.cpp"), os.path.join(CSRC, "scene_refit.cpp"), "-o", exe, "-L" + LIB, "-lgoblin_host",
                           "-Wl,-rpath," + LIB, "-lpthread"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("GBL_")}   # the builders' tuning knobs
    scene_dir = work / "scenes"
    scene_dir.mkdir()
    meshes.write_meshes(scene_dir, meshes.ALL)
    cache = {}

    def dump(name):
        if name in cache:
            return cache[name]
        if name in GENERATED:
            path = str(scene_dir / (name + ".json"))
            with open(path, "w") as f:
                json.dump(meshes.scene_doc(GENERATED[name]), f)
        else:
            path = os.path.join(SCENES, name + ".json")
        out = work / ("dump_" + name)
        out.mkdir()
        subprocess.check_call([exe, str(out), path], env=env)

        def load(member, dtype):
            return np.fromfile(str(out / member), dtype)
        d = {"nodes": load("nodes", rr.NODE), "tris": load("tris", rr.TRI), "bounds": load("tri_bounds_leaf", rr.BOUND),
             "tri_shade": load("tri_shade", rr.SHADE), "positions": load("positions", np.float32).reshape(-1, 3),
             "mesh_root": load("mesh_root", np.int32), "hot_nodes": int(load("hot_nodes", np.uint32)[0]),
             "meshes": load("meshes", np.uint32).reshape(-1, 6), "plans": {}}
        for m, row in enumerate(d["meshes"]):
            if row[0] == 0:   # GBL_SHAPE_MESH
                d["plans"][m] = (load("plan_%d" % m, rr.RECORD), [int(x) for x in load("levels_%d" % m, np.uint32)])
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        cache[name] = d
        return d
    return dump


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def refit_all(d, positions):
    """Fresh copies of the three tables with every triangle mesh refitted over `positions`, along the C++ plans."""
    nodes, tris, bounds = d["nodes"].copy(), d["tris"].copy(), d["bounds"].copy()
    for m, plan in d["plans"].items():
        row = d["meshes"][m]
        rr.refit_mesh(nodes, tris, bounds, d["tri_shade"], positions, d["mesh_root"][m], int(row[5]), int(row[4]), plan=plan)
    return nodes, tris, bounds


@pytest.mark.parametrize("name", list(GENERATED) + SHIPPED)
def test_identity_the_restated_refit_reproduces_the_packed_tables(dumper, name):
    d = dumper(name)
    nodes, tris, bounds = refit_all(d, d["positions"])
    touched = sum(len(p[0]) for p in d["plans"].values())
    print(name, "nodes", len(nodes), "of which refitted", touched, "tris", len(tris), "hot", d["hot_nodes"])
    assert touched > 0
    assert same_bytes(tris, d["tris"])
    assert same_bytes(bounds, d["bounds"])
    wrong = np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(nodes, d["nodes"])]) if not same_bytes(nodes, d["nodes"]) else []
    assert len(wrong) == 0, (name, wrong[:8], nodes[wrong[:2]], d["nodes"][wrong[:2]])


@pytest.mark.parametrize("name", list(GENERATED) + SHIPPED)
def test_plan_holds_every_referenced_node_once_sorted_by_level(dumper, name):
    d = dumper(name)
    nodes, hot = d["nodes"], d["hot_nodes"]
    in_some_plan = set()
    for m, (records, level_first) in d["plans"].items():
        root = int(d["mesh_root"][m])
        want, want_levels = rr.plan_walk(nodes, root)
        assert same_bytes(records, want) and level_first == want_levels, (name, m)
        if root < 0:   # the whole mesh is one leaf
            assert len(records) == 0 and level_first == []
            assert rr.leaf_range(root) == (int(d["meshes"][m][5]), int(d["meshes"][m][4]))
            continue
        # every node reachable by reference, by an independent depth-first walk, exactly once
        reach, stack = [], [root]
        while stack:
            i = stack.pop()
            reach.append(i)
            stack += [int(c) for c in nodes["child"][i] if 0 <= c < rr.REF_NONE]
        assert sorted(reach) == sorted(int(x) for x in records["node"]) and len(set(reach)) == len(reach)
        assert not in_some_plan & set(reach)   # meshes share no node
        in_some_plan |= set(reach)
        assert level_first[0] == 0 and level_first[-1] == len(records) and level_first == sorted(set(level_first))
        for l in range(len(level_first) - 1):
            assert (records["level"][level_first[l]:level_first[l + 1]] == l).all()
        referenced = {root}
        for r in records:
            child = nodes["child"][r["node"]]
            for c in range(4):
                interior = 0 <= child[c] < rr.REF_NONE
                assert (r["child_plan"][c] >= 0) == bool(interior)
                if interior:
                    k = records[r["child_plan"][c]]
                    assert k["node"] == child[c] and k["level"] == r["level"] + 1
                    referenced.add(int(child[c]))
                elif child[c] < 0:
                    first, count = rr.leaf_range(child[c])
                    assert d["meshes"][m][5] <= first and first + count <= d["meshes"][m][5] + d["meshes"][m][4]
        # nothing below hot_nodes (nor anywhere else) is in the plan unless a reference led there
        assert set(int(x) for x in records["node"]) == referenced
    if name == "all":
        leaf_roots = [m for m in d["plans"] if d["mesh_root"][m] < 0]
        assert len(leaf_roots) >= 2, leaf_roots   # the floor and few1 (the host's SAH splits few3 and few4)
    if hot:   # the hot prefix's originals are unreferenced: no plan holds a node twice, under either index
        assert len(in_some_plan) > 0 and any(i < hot for i in in_some_plan)


def generated_mesh_names(name):
    """Mesh index -> tests/meshes.py name for a generated scene (mesh 0 is the floor)."""
    return {m + 1: n for m, n in enumerate(GENERATED[name])}


@pytest.mark.parametrize("name", list(GENERATED))
@pytest.mark.parametrize("how", ["jitter", "stretch"])
def test_refitted_boxes_contain_the_deformed_triangles(dumper, name, how):
    d = dumper(name)
    P = d["positions"].copy()
    for m, mesh_name in generated_mesh_names(name).items():
        row = d["meshes"][m]
        v = slice(int(row[1]), int(row[1]) + int(row[2]))
        radius = meshes.MESHES[mesh_name][1]
        P[v] = rr.jitter(P[v], radius) if how == "jitter" else rr.stretch(P[v], radius)
    nodes, tris, bounds = refit_all(d, P)
    assert not same_bytes(nodes, d["nodes"])
    corners = P[d["tri_shade"]["v"][tris["shade"]]]            # [T, 3, 3], straight from the positions
    tlo, thi = corners.min(axis=1), corners.max(axis=1)
    checked = 0
    for m in generated_mesh_names(name):
        records, level_first = d["plans"][m]
        if len(records) == 0:
            continue
        # the exact box of every record's child slots, straight from the positions, children before parents
        ex_lo = np.full((len(records), 4, 3), np.inf, np.float32)
        ex_hi = np.full((len(records), 4, 3), -np.inf, np.float32)
        for r in range(len(records) - 1, -1, -1):
            rec = records[r]
            blo, bhi = rr.child_boxes(nodes, np.array([rec["node"]]))
            child = nodes["child"][rec["node"]]
            for c in range(4):
                if child[c] == rr.REF_NONE:
                    assert (blo[0, c] > bhi[0, c]).all()       # qlo = 255 > qhi = 0: empty for every ray
                    continue
                if child[c] < 0:
                    first, count = rr.leaf_range(child[c])
                    ex_lo[r, c], ex_hi[r, c] = tlo[first:first + count].min(axis=0), thi[first:first + count].max(axis=0)
                else:
                    k = rec["child_plan"][c]
                    kused = nodes["child"][records[k]["node"]] != rr.REF_NONE
                    # the child's own four boxes (their exact extent: see the module's note) lie inside the box its parent holds for it
                    assert (blo[0, c] <= ex_lo[k][kused]).all() and (bhi[0, c] >= ex_hi[k][kused]).all(), (name, m, r, c)
                    ex_lo[r, c], ex_hi[r, c] = ex_lo[k][kused].min(axis=0), ex_hi[k][kused].max(axis=0)
                assert (blo[0, c] <= ex_lo[r, c]).all() and (bhi[0, c] >= ex_hi[r, c]).all(), (name, m, r, c, blo[0, c], ex_lo[r, c], bhi[0, c], ex_hi[r, c])
                checked += 1
    print(name, how, "child boxes checked", checked)
    assert checked > 0


def test_abi():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "goblin_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+GBL_ABI_VERSION\s+14\b", header) and _abi.GBL_ABI_VERSION == 14
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libgoblin_hip.so"))
    for name in NAMES:
        assert re.search(r"\bgbl_status\s+%s\s*\(" % name, header), name
        assert name in _abi.HIP_SYMBOLS
        assert getattr(lib, name) is not None, name
