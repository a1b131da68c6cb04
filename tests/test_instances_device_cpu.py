"""gbl_update_instances_device / gbl_get_instances_device / gbl_selftest_instances without a GPU: the ABI (header, ctypes mirror,
exported names), and the arithmetic the compose kernel runs -- goblin_amd/csrc/kernels/instances.h, compiled for the host -- against
scene_prep.cpp's own, bit for bit (tests/instances_compose.cpp: pack_transform for m / inv and the invertibility verdict, build_tlas
over a one-instance TlasInput for the eight-corner box and the record), and build_tlas_nodes against build_tlas.

Measured: 10^5 random transforms (98 924 invertible, 1 076 refused) and 45 edge cases; every difference count is 0; the file takes
7 s, nearly all of it compiling scene_prep.cpp twice."""
import ctypes as C
import os
import re
import subprocess

import pytest

from goblin_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "goblin_amd", "csrc")
NAMES = ("gbl_update_instances_device", "gbl_get_instances_device", "gbl_selftest_instances")


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "goblin_hip.h")).read(), flags=re.S)


@pytest.mark.parametrize("name", NAMES)
def test_declared_mirrored_exported(name):
    """Fails without the feature."""
    assert re.search(r"\bgbl_status\s+%s\s*\(" % name, header())
    assert name in _abi.HIP_SYMBOLS
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libgoblin_hip.so"))
    assert getattr(lib, name) is not None


def test_the_flag_and_the_abi_version(tmp_path):
    src = tmp_path / "flag.c"
    src.write_text('#include <stdio.h>\n#include "goblin_hip.h"\nint main(void){printf("%u %d %zu\\n", GBL_INSTANCES_DEVICE_TLAS, GBL_ABI_VERSION, sizeof(gbl_trs));return 0;}\n')
    exe = tmp_path / "flag"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])   # plain C
    flag, abi, trs = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert flag == _abi.GBL_INSTANCES_DEVICE_TLAS == 1
    assert abi == _abi.GBL_ABI_VERSION == 14       # new entry points only: no existing layout changed
    assert trs == C.sizeof(_abi.gbl_trs) == 40     # a tensor's row of ten floats is one record


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    """tests/instances_compose.cpp, built with g++ -ffp-contract=off beside scene_prep.cpp, run once."""
    exe = str(tmp_path_factory.mktemp("instances_compose") / "instances_compose")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", os.path.join(REPO, "tests", "instances_compose.cpp"),
                           os.path.join(CSRC, "scene_prep.cpp"), "-o", exe, "-lpthread"])
    out = {}
    for line in subprocess.check_output([exe]).decode().splitlines():
        key, value = line.split()
        out[key] = int(value)
    print(out)
    return out


DIFFERENCES = ("verdict_differs", "m_differs", "inv_differs", "box_differs", "record_differs", "flag_wrong")


def test_random_transforms_compose_to_the_host_bits(counts):
    assert counts["random_cases"] == 100000
    # the draw reaches both verdicts: scales down to e^-4 fall below |det| = 1e-5
    assert counts["random_invertible"] > 80000 and counts["random_singular"] > 1000
    assert counts["random_invertible"] + counts["random_singular"] == counts["random_cases"]
    for k in DIFFERENCES:
        assert counts["random_" + k] == 0, k
    assert counts["random_flagged_not_finite"] == 0


def test_edge_transforms_compose_to_the_host_bits(counts):
    """Non-uniform and negative scales, an unnormalised quaternion, -0.0 components, translations of 1e6, uniform scales on both
    sides of the determinant's threshold (0.0217 accepted, 0.0215 refused), denormal and zero scales."""
    assert counts["edge_list_valid"] == 9 and counts["edge_list_singular"] == 6
    assert counts["edge_cases"] == 15 and counts["edge_invertible"] == 9 and counts["edge_singular"] == 6
    for k in DIFFERENCES:
        assert counts["edge_" + k] == 0, k


def test_non_finite_floats_are_flagged_in_every_slot(counts):
    """NaN, +inf and -inf in each of the ten floats: the compose kernel refuses on inst_trs_not_finite before it composes.  The
    host composes these too (it has no such check), and what it composes is compared as well: bit for bit where a float is a
    number, NaN against NaN where it is not -- a NaN's sign and payload are the implementation's (on x86 the first operand's,
    and the compiler orders operands), so 10 of the 30 inverses differ there in payload alone."""
    assert counts["nonfinite_cases"] == 30 and counts["nonfinite_flagged_not_finite"] == 30
    for k in DIFFERENCES:
        assert counts["nonfinite_" + k] == 0, k


def test_build_tlas_nodes_is_build_tlas(tmp_path):
    """The tree gbl_update_instances_device builds on the host from boxes read back is build_tlas's: over 1, 2, 5, 65 and 300
    instances on the line of tests/meshes.instances_doc, the same nodes, root and depth."""
    src = tmp_path / "nodes.cpp"
    src.write_text(r'''
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "scene_prep.h"
int main() {
    long differs = 0, nodes = 0;
    for (unsigned n : {1u, 2u, 5u, 65u, 300u}) {
        std::vector<gbl_instance> inst(n);
        for (unsigned k = 0; k < n; ++k) {
            memset(&inst[k], 0, sizeof(gbl_instance));
            const float g = std::pow(1.02f, float(k));
            const float t[10] = {0.6f * (g - 1.0f), 0.01f * k, -0.8f * (g - 1.0f), 0.9238795f, 0.0f, 0.3826834f, 0.0f, 0.6f * g, 0.6f * g, 0.6f * g};
            memcpy(&inst[k].to_world, t, sizeof(t));
            inst[k].area_light = -1;
        }
        gbl_mesh mesh;
        memset(&mesh, 0, sizeof(mesh));
        gbl_material mat;
        memset(&mat, 0, sizeof(mat));
        const float lo[3] = {-1.0f, -0.5f, -1.0f}, hi[3] = {1.0f, 0.5f, 1.0f};
        const int32_t root = 0;
        const TlasInput in = {inst.data(), n, &mesh, &mat, lo, hi, &root, 17};
        TlasResult built;
        std::string err;
        if (build_tlas(in, &built, &err) != GBL_OK) return 1;
        std::vector<DevNode> again;
        int32_t r = -1;
        int depth = -1;
        build_tlas_nodes(built.instance_bounds.data(), n, 17, &again, &r, &depth);
        nodes += long(again.size());
        if (r != built.root || depth != built.depth || again.size() != built.nodes.size() ||
            (!again.empty() && memcmp(again.data(), built.nodes.data(), again.size() * sizeof(DevNode)) != 0)) differs += 1;
    }
    printf("%ld %ld\n", differs, nodes);
    return 0;
}
''')
    exe = str(tmp_path / "nodes")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, str(src), os.path.join(CSRC, "scene_prep.cpp"), "-o", exe, "-lpthread"])
    differs, nodes = (int(x) for x in subprocess.check_output([exe]).split())
    assert differs == 0 and nodes > 100
