"""gbl_update_materials / gbl_update_textures, their device forms, gbl_get_* and gbl_selftest_materials without a GPU.

The ABI: header, ctypes mirror, exported names, signatures, gbl_material's and gbl_texture's layout as a C compiler sees them, the ABI
version.  The repacker against the packer: tests/materials_repack.cpp, compiled with g++ -ffp-contract=off beside scene_prep.cpp as
tests/lights_repack.cpp is, applies each case of tests/material_edit_cases.py to a shipped scene's packed tables through
repack_materials / repack_textures and packs the edited description from scratch -- `materials` and `textures` byte for byte the
same, every other table and flag where it was, the inverse edit restoring the first bytes.  The compose functions of
kernels/materials.h, compiled for the host, against the packer over 10^5 random rows and the edge rows.  The oracle on every case:
the edited description's per-sample radiance differs from the scene's own at the GPU tests' frame, so "the frames differ" there is
a property of the input.  The Python face's refusals, made before any library call.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import material_edit_cases as mc
import oracle_binding as ob
from goblin_amd import _abi, renderer
from goblin_amd import scene as gs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "goblin_amd", "csrc")
LIB = os.path.join(REPO, "goblin_amd", "lib")
NAMES = ("gbl_update_materials", "gbl_get_materials", "gbl_update_textures", "gbl_get_textures", "gbl_update_materials_device",
         "gbl_update_textures_device", "gbl_selftest_materials")


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
    assert "gbl_status gbl_update_materials(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_material* materials , void* stream);" in h
    assert "gbl_status gbl_update_textures(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_texture* textures , void* stream);" in h
    assert "gbl_status gbl_get_materials(gbl_ctx* ctx, uint32_t first, uint32_t count, gbl_material* out );" in h
    assert "gbl_status gbl_get_textures(gbl_ctx* ctx, uint32_t first, uint32_t count, gbl_texture* out );" in h
    assert "gbl_status gbl_update_materials_device(gbl_ctx* ctx, uint32_t first, uint32_t count, const float* d_rows , void* stream);" in h
    assert "gbl_status gbl_update_textures_device(gbl_ctx* ctx, uint32_t first, uint32_t count, const float* d_rows , void* stream);" in h
    assert "gbl_status gbl_selftest_materials(gbl_ctx* ctx, void* materials_out, void* textures_out, uint64_t* num_materials, uint64_t* num_textures);" in h


@pytest.mark.parametrize("record,size", [("gbl_material", 80), ("gbl_texture", 108)])
def test_the_records_as_a_c_compiler_lays_them_out(tmp_path, record, size):
    mirror = getattr(_abi, record)
    fields = [name for name, _ in mirror._fields_]
    prints = "".join('printf(" %%zu", offsetof(%s, %s));' % (record, f) for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "goblin_hip.h"\n'
                   'int main(void){printf("%%d %%zu", GBL_ABI_VERSION, sizeof(%s));%sprintf("\\n");return 0;}\n' % (record, prints))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == _abi.GBL_ABI_VERSION == 14       # new entry points only: no existing layout changed
    assert got[1] == C.sizeof(mirror) == size
    assert got[2:] == [getattr(mirror, f).offset for f in fields]


def test_the_abi_version_stays_14():
    assert re.search(r"#define\s+GBL_ABI_VERSION\s+14\b", header())
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libgoblin_hip.so"))
    lib.gbl_abi_version.restype = C.c_uint32
    assert lib.gbl_abi_version() == 14


def test_the_device_records_the_python_face_reads_back(tmp_path):
    """renderer._MATERIAL / _TEXTURE against DevMaterial / DevTexture as the compiler lays them out."""
    src = tmp_path / "records.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "device_scene.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(DevMaterial), '
                   'offsetof(DevMaterial, color3), offsetof(DevMaterial, tex_normal), sizeof(DevTexture), offsetof(DevTexture, to_tex), offsetof(DevTexture, max_aniso));}\n')
    exe = tmp_path / "records"
    subprocess.check_call(["g++", "-I", CSRC, str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    m, t = renderer.HipPathTracer._MATERIAL, renderer.HipPathTracer._TEXTURE
    assert got == [m.itemsize, m.fields["color3"][1], m.fields["tex_normal"][1], t.itemsize, t.fields["to_tex"][1], t.fields["max_aniso"][1]]
    assert got[0] == 88 and got[3] == 120


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/materials_repack.cpp, built as tests/lights_repack.cpp is."""
    exe = str(tmp_path_factory.mktemp("materials_repack") / "materials_repack")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", os.path.join(REPO, "tests", "materials_repack.cpp"),
                           os.path.join(CSRC, "scene_prep.cpp"), "-o", exe, "-L" + LIB, "-lgoblin_host", "-Wl,-rpath," + LIB, "-lpthread"])
    return exe


@pytest.fixture(scope="module")
def results(program, tmp_path_factory):
    """The program run once over the cases: {(scene, case): "ok" | "FAIL ..."}."""
    cases = tmp_path_factory.mktemp("material_cases") / "cases.txt"
    cases.write_text(mc.case_file_text())
    env = {k: v for k, v in os.environ.items() if not k.startswith("GBL_")}   # the builders' tuning knobs
    out = {}
    for line in subprocess.check_output([program, "cases", os.path.join(REPO, "goblin_amd", "scenes"), str(cases)], env=env).decode().splitlines():
        print(line)
        word, rest = line.split(" ", 1)
        if word == "case":
            scene, case, verdict = rest.split(" ", 2)
            out[(scene, case)] = verdict
    return out


def test_the_program_ran_every_case_and_no_other(results):
    assert sorted(results) == sorted((scene, name) for scene, name, _ in mc.CASES)


def test_the_cases_cover_what_the_edits_offer():
    """Each editable field of each material type, a wrapped material under its mask, re-pointed slots, each editable texture field
    (a spherical to_tex among them), a float texture's value."""
    seen = set()
    for scene, _, edits in mc.CASES:
        d = scene_of(scene).desc
        for table, index, field, _ in edits:
            seen.add((d.materials[index].type, field) if table == "m" else ("t", field, bool(d.textures[index].is_float)))
    L, B, T, M, K, S = (_abi.GBL_MAT_LAMBERT, _abi.GBL_MAT_BLINN, _abi.GBL_MAT_TRANSPARENT, _abi.GBL_MAT_MIRROR, _abi.GBL_MAT_MASK, _abi.GBL_MAT_SUBSURFACE)
    want = {(L, "color"), (B, "color"), (B, "index"), (B, "k"), (B, "exponent"), (T, "color"), (T, "color2"), (T, "index"), (M, "color"), (M, "index"), (M, "k"),
            (K, "color"), (K, "exponent"), (K, "tex_exponent"), (S, "color"), (S, "color2"), (S, "color3"), (S, "index"), (S, "k"),
            (L, "tex_color"), (L, "tex_bump"), (L, "tex_normal"),
            ("t", "value", False), ("t", "value", True), ("t", "uv_scale", False), ("t", "uv_scale", True), ("t", "uv_offset", False), ("t", "uv_offset", True),
            ("t", "to_tex", False), ("t", "max_anisotropy", False)}
    assert want <= seen, want - seen
    wrapped = [(s, n) for s, n, edits in mc.CASES for tb, i, _, _ in edits
               if tb == "m" and any(scene_of(s).desc.materials[k].type == K and scene_of(s).desc.materials[k].masked_material == i for k in range(scene_of(s).desc.num_materials))]
    assert len(wrapped) >= 3


@pytest.mark.parametrize("scene,name", [(s, n) for s, n, _ in mc.CASES], ids=mc.IDS)
def test_repacked_tables_are_the_packers_bytes(results, scene, name):
    assert results[(scene, name)] == "ok", (scene, name, results[(scene, name)])


@pytest.fixture(scope="module")
def counts(program):
    out = {}
    for line in subprocess.check_output([program, "compose"]).decode().splitlines():
        key, value = line.split()
        out[key] = int(value)
    print(out)
    return out


def test_the_compose_functions_are_the_packer_bit_for_bit(counts):
    """10^5 random rows and 154 edge rows (index 1 and its neighbours, below and above 1, zeros of both signs, denormals, the largest
    finite float, infinities and NaN, whose payloads are not compared), each on a live record of every material type and on three
    textures: against pack_scene's functions and against the expressions pack_materials / pack_textures held before the split."""
    assert counts["random_rows"] == 100000 and counts["edge_rows"] == 154
    assert counts["material_cases"] == 6 * (100000 + 154) and counts["texture_cases"] == 3 * (100000 + 154)
    assert counts["index_below_one"] > 10000 and counts["index_above_one"] > 10000       # both branches of the polynomial
    assert counts["differs_from_the_packer"] == 0
    assert counts["differs_from_the_former_expressions"] == 0
    assert counts["texture_differs"] == 0


# ---------------------------------------------------------------------------
# the oracle on the cases: the edited frame differs from the scene's own
# ---------------------------------------------------------------------------
_SCENES = {}


def scene_of(name):
    if name not in _SCENES:
        _SCENES[name] = gs.load_scene(name, gs.config_overrides(resolution=(16, 16), spp=2, depth=3))
    return _SCENES[name]


_ORACLE_LI = {}


def oracle_li(scene):
    oracle = ob.Oracle(scene)
    return oracle.li_replay(oracle.native_samples(mc.SEED), threads=4)[0]


@pytest.mark.parametrize("scene,name,edits", mc.CASES, ids=mc.IDS)
def test_the_oracle_sees_every_case(scene, name, edits):
    sa = scene_of(scene)
    if scene not in _ORACLE_LI:
        _ORACLE_LI[scene] = oracle_li(sa)
    sb = gs.load_scene(scene, gs.config_overrides(resolution=(16, 16), spp=2, depth=3))
    mc.write_desc(sb, *mc.edited_records(sa, edits))
    li_b = oracle_li(sb)
    assert np.isfinite(li_b).all()
    differing = int((li_b.view(np.uint32) != _ORACLE_LI[scene].view(np.uint32)).any(axis=1).sum())
    print(scene, name, "samples that differ:", differing, "of", len(li_b))
    assert differing >= 1


# ---------------------------------------------------------------------------
# the Python face
# ---------------------------------------------------------------------------
class NoLibrary:
    """Stands where the tracer keeps libgoblin_hip.so: any call is a failure."""

    def __getattr__(self, name):
        raise AssertionError("the library was reached: " + name)


def tracer_without_a_device(scene):
    import torch
    r = renderer.HipPathTracer.__new__(renderer.HipPathTracer)
    r.lib, r.scene, r.handle, r.device = NoLibrary(), scene, None, torch.device("cuda", 0)
    return r


def test_the_python_methods_refuse_before_any_library_call():
    """Fails without the feature."""
    import torch
    s = scene_of("textured")
    r = tracer_without_a_device(s)
    nm, nt = s.desc.num_materials, s.desc.num_textures
    for method, row, total in ((r.update_materials, 12, nm), (r.update_textures, 7, nt)):
        for bad in (torch.zeros((1, row), dtype=torch.float64), torch.zeros((1, row), dtype=torch.float16),
                    torch.zeros((1, row), dtype=torch.float32),                    # the right dtype and shape on another device
                    torch.zeros((1, row + 1), dtype=torch.float32), torch.zeros((row,), dtype=torch.float32), torch.zeros((1, 1, row), dtype=torch.float32),
                    torch.zeros((2, 2 * row), dtype=torch.float32)[:, ::2]):       # not contiguous
            with pytest.raises(ValueError):
                method(0, bad, stream=object())
        with pytest.raises(TypeError):
            method(0, torch.zeros((1, row)), stream=object(), color=[1, 2, 3])     # a tensor and fields
        with pytest.raises(TypeError):
            method(0, stream=object(), no_such_field=1.0)
        with pytest.raises(TypeError):
            method(0, [object()], stream=object())
        with pytest.raises(ValueError):
            method(total, stream=object(), **({"color": [1, 2, 3]} if row == 12 else {"value": [1, 2, 3]}))
    with pytest.raises(TypeError):
        r.update_materials(0, [_abi.gbl_texture()], stream=object())
    with pytest.raises(TypeError):
        r.update_textures(0, [_abi.gbl_material()], stream=object())
    with pytest.raises(ValueError):
        r.update_materials(nm, [_abi.gbl_material()], stream=object())
    with pytest.raises(ValueError):
        r.update_materials(nm - 1, [_abi.gbl_material(), _abi.gbl_material()], stream=object())
    with pytest.raises(ValueError):
        r.update_textures(-1, [_abi.gbl_texture()], stream=object())
    # ... and what passes them reaches the library
    with pytest.raises(AssertionError, match="the library was reached: gbl_update_materials"):
        r.update_materials(0, [_abi.gbl_material()], stream=object())
    with pytest.raises(AssertionError, match="the library was reached: gbl_update_textures"):
        r.update_textures(nt - 1, [_abi.gbl_texture()], stream=object())
    with pytest.raises(AssertionError, match="the library was reached: gbl_get_materials"):
        r.materials()
    with pytest.raises(AssertionError, match="the library was reached: gbl_get_textures"):
        r.textures()
