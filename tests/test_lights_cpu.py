"""gbl_update_lights / gbl_get_lights / gbl_selftest_lights without a GPU: the ABI (header, ctypes mirror, exported names, gbl_light's
layout as a C compiler sees it), and the repacker against the packer -- tests/lights_repack.cpp, compiled with g++ -ffp-contract=off
beside scene_prep.cpp as tests/scene_prep_digest.cpp is, applies each edit of CASES to a shipped scene's packed light tables through
repack_lights and packs the edited description from scratch: `lights`, `light_cdf` and `light_pick_pdf` byte for byte the same,
light_tris, ibl_dist, wh_slots, extended and has_ibl where they were, and the inverse edit restores the first bytes.  Both packings
run in one process, so the machine's libm does not enter.

Measured: the 30 cases take 0.4 s to run; the file takes 6 s, nearly all of it compiling scene_prep.cpp."""
import ctypes as C
import os
import re
import subprocess

import pytest

from goblin_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "goblin_amd", "csrc")
LIB = os.path.join(REPO, "goblin_amd", "lib")
NAMES = ("gbl_update_lights", "gbl_get_lights", "gbl_selftest_lights")
# grid: a spot and a point light -- colour, position, a spot direction along an axis, with |x| > |y| and |x| <= |y| (both branches of
# orientation_of), with a rotation of non-positive trace, both cone cosines, both lights in one call, a light left without power.
# cornell: the one-light CDF {0, 1}, an area light over a mesh -- colour, translation, a non-uniform scale (its power changes).
# shapes: sphere / disk area lights and the directional light.  volume: lights in a medium.  ibl: the orientation.
CASES = {
    "grid": ["spot_colour", "point_colour", "spot_position", "point_position", "spot_direction_axis_z", "spot_direction_axis_y",
             "spot_direction_x_over_y", "spot_direction_y_over_x", "spot_direction_x_equals_y", "spot_direction_trace_not_positive",
             "spot_direction_trace_negative_x", "spot_cos_theta_max", "spot_cos_falloff_start", "both_lights_at_once", "point_without_power"],
    "cornell": ["one_light", "area_colour", "area_translation", "area_scale_changes_power"],
    "shapes": ["area0_colour", "area1_colour", "directional_colour", "directional_direction", "directional_direction_not_unit"],
    "volume": ["area0_colour", "area1_colour", "spot_direction"],
    "ibl": ["ibl_orientation", "ibl_orientation_not_unit", "point_colour_beside_the_ibl"],
}


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "goblin_hip.h")).read(), flags=re.S)


@pytest.mark.parametrize("name", NAMES)
def test_declared_mirrored_exported(name):
    """Fails without the feature."""
    assert re.search(r"\bgbl_status\s+%s\s*\(" % name, header())
    assert name in _abi.HIP_SYMBOLS
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libgoblin_hip.so"))
    assert getattr(lib, name) is not None


def test_the_signatures_take_what_the_mirror_passes():
    h = " ".join(header().split())
    assert "gbl_status gbl_update_lights(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_light* lights , void* stream);" in h
    assert "gbl_status gbl_get_lights(const gbl_ctx* ctx, uint32_t first, uint32_t count, gbl_light* out );" in h
    assert "gbl_status gbl_selftest_lights(gbl_ctx* ctx, void* records_out, float* cdf_out, float* pick_pdf_out, uint64_t* total);" in h


def test_gbl_light_as_a_c_compiler_lays_it_out(tmp_path):
    fields = [name for name, _ in _abi.gbl_light._fields_]
    prints = "".join('printf(" %%zu", offsetof(gbl_light, %s));' % f for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "goblin_hip.h"\n'
                   'int main(void){printf("%%d %%zu", GBL_ABI_VERSION, sizeof(gbl_light));%sprintf("\\n");return 0;}\n' % prints)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == _abi.GBL_ABI_VERSION == 14       # new entry points only: no existing layout changed
    assert got[1] == C.sizeof(_abi.gbl_light) == 100
    assert got[2:] == [getattr(_abi.gbl_light, f).offset for f in fields]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """tests/lights_repack.cpp, built as tests/scene_prep_digest.cpp is and run once: {(scene, case): "ok" | "FAIL ..."}."""
    exe = str(tmp_path_factory.mktemp("lights_repack") / "lights_repack")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", os.path.join(REPO, "tests", "lights_repack.cpp"),
                           os.path.join(CSRC, "scene_prep.cpp"), "-o", exe, "-L" + LIB, "-lgoblin_host", "-Wl,-rpath," + LIB, "-lpthread"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("GBL_")}   # the builders' tuning knobs
    out = {}
    for line in subprocess.check_output([exe, os.path.join(REPO, "goblin_amd", "scenes")], env=env).decode().splitlines():
        print(line)
        word, rest = line.split(" ", 1)
        if word == "case":
            scene, case, verdict = rest.split(" ", 2)
            out[(scene, case)] = verdict
    return out


def test_the_program_ran_every_case_and_no_other(results):
    assert sorted(results) == sorted((scene, case) for scene, cases in CASES.items() for case in cases)


@pytest.mark.parametrize("scene,case", [(scene, case) for scene, cases in CASES.items() for case in cases])
def test_repacked_tables_are_the_packers_bytes(results, scene, case):
    assert results[(scene, case)] == "ok", (scene, case, results[(scene, case)])
