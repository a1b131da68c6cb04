"""pack_scene's device tables, byte for byte (no GPU): tests/scene_prep_digest.cpp is compiled with g++ against
goblin_amd/csrc/scene_prep.cpp and libgoblin_host.so, run over every shipped scene with host- and device-built BLASes, and
its digests are compared with tests/golden/scene_prep_digests.json, recorded from the tree before pack_scene was broken up
into validate_desc and one packer per table.

Only members whose values pass through no transcendental library call are recorded (MEMBERS), so the file does not depend on
a machine's libm; filter_table, ewa_lut, ibl_dist, camera, lights, light_cdf, light_pick_pdf and volume go through
expf / sinf / cosf / tanf and are covered by the GPU parity suite.
(tri_order and the trees follow std::nth_element / std::partition where centroids tie: a standard library that breaks such
ties differently needs the file recorded again, from a tree whose GPU parity suite passes.)

    python tests/test_scene_prep_cpu.py     # prints the digests of the working tree in the golden file's format
"""
import glob
import json
import os
import subprocess
import sys
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "scene_prep_digests.json")
LIB = os.path.join(REPO, "goblin_amd", "lib")
MEMBERS = ["nodes", "tris", "tri_shade", "tri_bounds", "tri_bounds_leaf", "tri_order", "instances", "instance_bounds", "materials",
           "textures", "images", "light_tris", "mesh_root", "mesh_stack_need",
           "tlas_root", "tlas_base", "tlas_capacity", "hot_nodes", "stack_entries", "extended", "scene_extended", "has_masks",
           "has_bssrdf", "has_ibl", "wh_slots", "blas_nodes", "tlas_nodes", "blas_max_depth", "tlas_depth"]


def digests(workdir):
    """{scene file: {"0" | "1" (device_blas): {member: "count hash" | "= value"}}} of the shipped scenes."""
    exe = os.path.join(str(workdir), "scene_prep_digest")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(REPO, "tests", "scene_prep_digest.cpp"),
                           os.path.join(REPO, "goblin_amd", "csrc", "scene_prep.cpp"), "-o", exe, "-L" + LIB, "-lgoblin_host",
                           "-Wl,-rpath," + LIB, "-lpthread"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("GBL_")}   # the builders' tuning knobs
    scenes = sorted(glob.glob(os.path.join(REPO, "goblin_amd", "scenes", "*.json")))
    text = subprocess.check_output([exe] + scenes, env=env, stderr=subprocess.DEVNULL).decode()
    out, cur = {}, None
    for line in text.splitlines():
        name, rest = line.split(" ", 1)
        if name == "scene":
            scene, flavour = rest.split(" device_blas=")
            cur = out.setdefault(scene, {}).setdefault(flavour, {})
        elif name in MEMBERS:
            cur[name] = rest
    return out


@pytest.fixture(scope="module")
def digest(tmp_path_factory):
    return digests(tmp_path_factory.mktemp("scene_prep"))


def test_the_golden_file_covers_every_shipped_scene_and_member():
    with open(GOLDEN) as f:
        golden = json.load(f)
    shipped = sorted(os.path.basename(p) for p in glob.glob(os.path.join(REPO, "goblin_amd", "scenes", "*.json")))
    assert sorted(golden) == shipped
    for scene in golden:
        assert sorted(golden[scene]) == ["0", "1"], scene
        for flavour in golden[scene]:
            assert sorted(golden[scene][flavour]) == sorted(MEMBERS), (scene, flavour)


def test_packed_tables_are_byte_identical_to_the_recorded_digests(digest):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(digest) == sorted(golden)   # no scene fewer, none more
    wrong = []
    for scene in sorted(golden):
        assert sorted(digest[scene]) == sorted(golden[scene]), scene
        for flavour in sorted(golden[scene]):
            got, want = digest[scene][flavour], golden[scene][flavour]
            assert sorted(got) == sorted(want), (scene, flavour)   # no member fewer
            wrong += ["%s device_blas=%s %s: %s, recorded %s" % (scene, flavour, m, got[m], want[m]) for m in MEMBERS if got[m] != want[m]]
    assert not wrong, "\n".join(wrong)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        json.dump(digests(tmp), sys.stdout, indent=0, sort_keys=True)
