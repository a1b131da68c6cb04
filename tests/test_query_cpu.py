"""gbl_trace_rays without a GPU: the ABI's new names, and the inputs of the device suite's brute-force comparison.

1. The three new names (gbl_trace_rays, gbl_selftest_query, and the gbl_ray / gbl_ray_hit records with their constants) are
   declared in the header, mirrored in goblin_amd/_abi.py and exported by libgoblin_hip.so; a compiled C snippet prints the
   sizes and constants.
2. tests/test_gpu_query.py compares the lean query with a float64 brute force on query_cases.BENIGN under populations (B)
   and (C), leaving out "edge rays", which may be at most 5 % of a population.  That is a condition on the INPUTS: here the
   oracle's intersect stands in for the device against the same brute force, and the test shows that the populations keep
   the cap, that at least a quarter of their rays hit, and that the comparison's tolerance holds for the reference itself.

Measured (the oracle, CPU): (B) 1 673 of 2 000 rays hit, 15 edge rays; (C) 593 of 2 000 hit, no edge ray; hit flags agree on
every other ray; the largest |t32 - t64| |d| is 0.16 of the tolerance (float32 epsilon x scene extent x 64).
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import meshes
import oracle_binding as ob
import query_cases as qc
from goblin_amd import _abi
from goblin_amd import scene as gs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "goblin_hip.h")


def test_the_new_names_are_declared_mirrored_and_exported():
    text = open(HEADER).read()
    for name in ("gbl_trace_rays", "gbl_selftest_query"):
        assert "gbl_status %s(" % name in text, name
        assert name in _abi.HIP_SYMBOLS, name
    assert "} gbl_ray;" in text and "} gbl_ray_hit;" in text
    assert C.sizeof(_abi.gbl_ray) == C.sizeof(_abi.gbl_ray_hit) == 32
    assert [n for n, _ in _abi.gbl_ray._fields_] == ["o", "mint", "d", "maxt"]
    assert [n for n, _ in _abi.gbl_ray_hit._fields_] == ["t", "b1", "b2", "instance", "primitive", "n"]
    assert (_abi.gbl_ray_hit.instance.offset, _abi.gbl_ray_hit.primitive.offset, _abi.gbl_ray_hit.n.offset) == (12, 16, 20)
    assert (_abi.GBL_QUERY_CLOSEST, _abi.GBL_QUERY_ANY, _abi.GBL_QUERY_EXACT_TIES, _abi.GBL_QUERY_SHADING_NORMAL) == (0, 1, 1, 2)
    lib = os.path.join(_abi.LIB_DIR, "libgoblin_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ("gbl_trace_rays", "gbl_selftest_query"):
        assert " T %s\n" % name in exported, name


def test_a_c_program_sees_the_records_and_constants(tmp_path):
    src = tmp_path / "q.c"
    # (the two prototypes again: a redeclaration that did not match the header's would not compile)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "goblin_hip.h"\n'
                   'gbl_status gbl_trace_rays(gbl_ctx*, uint32_t, const gbl_ray*, uint64_t, void*, uint32_t, void*);\n'
                   'gbl_status gbl_selftest_query(gbl_ctx*, uint32_t, const gbl_ray*, uint64_t, void*, uint32_t, uint32_t);\n'
                   'int main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %u %u %u %u %d\\n", sizeof(gbl_ray), sizeof(gbl_ray_hit), offsetof(gbl_ray, d),\n'
                   '         offsetof(gbl_ray_hit, instance), offsetof(gbl_ray_hit, n), GBL_QUERY_CLOSEST, GBL_QUERY_ANY, GBL_QUERY_EXACT_TIES,\n'
                   '         GBL_QUERY_SHADING_NORMAL, GBL_ABI_VERSION);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "q"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["32", "32", "16", "12", "20", "0", "1", "1", "2", "14"], out
    assert _abi.GBL_ABI_VERSION == 14


@pytest.fixture(scope="module")
def benign(tmp_path_factory):
    d = tmp_path_factory.mktemp("query_cpu")
    meshes.write_meshes(d, qc.BENIGN)
    scene = gs.load_scene_text(json.dumps(meshes.scene_doc(qc.BENIGN)), str(d))
    return scene, ob.Oracle(scene), qc.world_triangles(scene), qc.scene_bound(scene)


@pytest.mark.parametrize("population", ["sphere", "chords"])
def test_the_populations_keep_the_brute_force_comparisons_caps(benign, population):
    scene, oracle, W, bound = benign
    rays = qc.sphere_rays(bound) if population == "sphere" else qc.chord_rays(bound)
    bf = qc.brute_force(W, rays)
    edge = bf["near_edge"]
    hit32, t32 = np.zeros(len(rays), bool), np.zeros(len(rays))
    for i, r in enumerate(rays):
        h = oracle.intersect(r[0:3], r[4:7], float(r[3]), float(r[7]) if np.isfinite(r[7]) else -1.0)
        hit32[i] = h is not None
        t32[i] = h[0] if h is not None else -1.0
    print(population, "hit", int(bf["hit"].sum()), "of", len(rays), "edge rays", int(edge.sum()))
    assert edge.sum() <= qc.EDGE_CAP * len(rays)
    assert bf["hit"].sum() >= 0.25 * len(rays)
    assert np.array_equal(hit32[~edge], bf["hit"][~edge]), np.flatnonzero((hit32 != bf["hit"]) & ~edge)
    both = bf["hit"] & hit32 & ~edge
    tol = qc.tolerance(bound, rays[both], bf["t"][both], W["tri"][bf["index"][both]])
    err = np.abs(t32[both] - bf["t"][both]) * np.linalg.norm(rays[both, 4:7].astype(np.float64), axis=1)
    print(population, "largest error / tolerance %.3g" % float((err / tol).max()))
    assert (err <= tol).all()
