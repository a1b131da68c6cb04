"""The C ABI: every function include/goblin_hip.h declares is exported by the library
that implements it, the ctypes mirror has the C layout, and the device library refuses
to work without a GPU instead of falling back."""
import ctypes as C
import os
import re
import subprocess

import pytest

from goblin_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "goblin_hip.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gbl_[a-z_0-9]+)\s*\(", text)))


def test_every_declared_symbol_is_exported():
    names = declared_functions()
    host = [n for n in names if n.startswith("gbl_host_")]
    hip = [n for n in names if not n.startswith("gbl_host_")]
    assert sorted(host) == sorted(_abi.HOST_SYMBOLS)
    assert sorted(hip) == sorted(_abi.HIP_SYMBOLS)
    hl = _abi.host_lib()
    for n in host:
        assert hasattr(hl, n), n
    dl = _abi.hip_lib()          # dlopen only; no compute without a GPU
    for n in hip:
        assert hasattr(dl, n), n
    assert dl.gbl_abi_version() == _abi.GBL_ABI_VERSION


def test_ctypes_mirror_has_the_c_layout(tmp_path):
    structs = ["gbl_trs", "gbl_mesh", "gbl_texture", "gbl_image", "gbl_material", "gbl_instance", "gbl_light", "gbl_camera", "gbl_film", "gbl_volume",
               "gbl_render_setting", "gbl_scene_desc", "gbl_render_params", "gbl_stats", "gbl_info"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "goblin_hip.h"\nint main(void){\n' +
                   "".join('printf("%s %%zu\\n", sizeof(%s));\n' % (s, s) for s in structs) +
                   'printf("off_film %zu\\n", offsetof(gbl_scene_desc, film));\n'
                   'printf("off_seed %zu\\n", offsetof(gbl_render_params, seed));\nreturn 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])   # plain C
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for s in structs:
        assert C.sizeof(getattr(_abi, s)) == int(out[s]), s
    assert _abi.gbl_scene_desc.film.offset == int(out["off_film"])
    assert _abi.gbl_render_params.seed.offset == int(out["off_seed"])


def test_device_library_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("this box has a GPU")
    from goblin_amd import scene as gs
    from goblin_amd.renderer import HipPathTracer
    scene = gs.load_scene("bunny", gs.config_overrides(resolution=(16, 16), spp=1, depth=2))
    with pytest.raises(RuntimeError):
        HipPathTracer(scene, 0)
    h = C.c_void_p()
    st = _abi.hip_lib().gbl_create(scene.desc_ptr, 0, C.byref(h))
    assert st == _abi.GBL_ERR_DEVICE and not h
    assert b"no CPU fallback" in _abi.hip_lib().gbl_last_error(None)


def test_bad_descriptions_are_rejected_before_touching_the_device():
    from goblin_amd import scene as gs
    scene = gs.load_scene("bunny", gs.config_overrides(resolution=(16, 16), spp=1, depth=2))
    desc = _abi.gbl_scene_desc.from_buffer_copy(scene.desc)
    desc.abi_version = 99
    h = C.c_void_p()
    assert _abi.hip_lib().gbl_create(C.byref(desc), 0, C.byref(h)) == _abi.GBL_ERR_INVALID
    desc = _abi.gbl_scene_desc.from_buffer_copy(scene.desc)
    desc.film.filter_width[0] = 9.0     # LDS film tile halo limit
    assert _abi.hip_lib().gbl_create(C.byref(desc), 0, C.byref(h)) == _abi.GBL_ERR_UNSUPPORTED


def test_degenerate_march_steps_are_rejected_not_hung():
    """A heterogeneous medium is ray marched in steps of step_size (kernels/medium.h): zero, negative, NaN, or a step so small
    that the region is more than 10^6 steps across would never come back from the device.  pack_scene refuses them."""
    from goblin_amd import scene as gs
    scene = gs.load_scene("hetero", gs.config_overrides(resolution=(16, 16), spp=1, depth=2))
    h = C.c_void_p()
    for step in (0.0, -0.1, float("nan"), float("inf"), 1e-12):
        desc = _abi.gbl_scene_desc.from_buffer_copy(scene.desc)
        desc.volume.step_size = step
        assert _abi.hip_lib().gbl_create(C.byref(desc), 0, C.byref(h)) == _abi.GBL_ERR_INVALID, step
        assert b"step_size" in _abi.hip_lib().gbl_last_error(None)
    desc = _abi.gbl_scene_desc.from_buffer_copy(scene.desc)
    desc.volume.grid[0] = 1 << 16
    desc.volume.grid[1] = 1 << 16
    assert _abi.hip_lib().gbl_create(C.byref(desc), 0, C.byref(h)) == _abi.GBL_ERR_INVALID
    assert b"2^31" in _abi.hip_lib().gbl_last_error(None)


def _own(desc, field, n, extra=0):
    """Give a description copy its own array behind `field` (its n elements and `extra` zeroed ones), so that a case can edit it."""
    ptr = getattr(desc, field)
    arr = (ptr._type_ * max(1, n + extra))()
    C.memmove(arr, ptr, n * C.sizeof(ptr._type_))
    setattr(desc, field, C.cast(arr, type(ptr)))
    desc.__dict__.setdefault("_arrays", []).append(arr)
    return arr


def _first(items, n, pred):
    return next(i for i in range(n) if pred(items[i]))


def _bad_instance(field):
    def edit(d):
        limit = {"mesh": d.num_meshes, "material": d.num_materials, "area_light": d.num_lights}[field]
        setattr(_own(d, "instances", d.num_instances)[0], field, limit)
    return edit


def _mesh_edit(**fields):
    def edit(d):
        m = _own(d, "meshes", d.num_meshes)[_first(d.meshes, d.num_meshes, lambda m: m.shape == _abi.GBL_SHAPE_MESH)]
        for k, v in fields.items():
            setattr(m, k, v)
    return edit


def _bad_vertex_index(d):
    m = d.meshes[_first(d.meshes, d.num_meshes, lambda m: m.shape == _abi.GBL_SHAPE_MESH)]
    _own(d, "indices", 3 * d.num_triangles)[3 * m.tri_offset + 1] = m.vertex_count


def _degenerate_uv(d):
    m = d.meshes[_first(d.meshes, d.num_meshes, lambda m: m.shape == _abi.GBL_SHAPE_MESH and m.has_uv)]
    uv = _own(d, "uvs", 2 * d.num_vertices)
    for v in range(m.vertex_count):   # every vertex of the mesh at one texture coordinate
        uv[2 * (m.vertex_offset + v)], uv[2 * (m.vertex_offset + v) + 1] = 0.25, 0.75


def _flat_instance(d):
    _own(d, "instances", d.num_instances)[0].to_world.scale[1] = 0.0


def _material_edit(**fields):
    def edit(d):
        m = _own(d, "materials", d.num_materials)[0]
        for k, v in fields.items():
            setattr(m, k, v(d) if callable(v) else v)
    return edit


def _mask_of_a_mask(d):
    i = _first(d.materials, d.num_materials, lambda m: m.type == _abi.GBL_MAT_MASK)
    _own(d, "materials", d.num_materials)[i].masked_material = i


def _texture_chain(levels, cyclic=False):
    """Material 0's colour slot gets a chain of `levels` scale textures over a constant (or over itself), appended to the scene's."""
    def edit(d):
        n = d.num_textures
        tex = _own(d, "textures", n, levels + 1)
        for k in range(levels):
            tex[n + k].type = _abi.GBL_TEX_SCALE
            nxt = n if (cyclic and k == levels - 1) else n + k + 1
            tex[n + k].child[0], tex[n + k].child[1] = nxt, n + levels
        tex[n + levels].type = _abi.GBL_TEX_CONSTANT
        d.num_textures = n + levels + 1
        _own(d, "materials", d.num_materials)[0].tex_color = n
    return edit


def _image_edit(**fields):
    def edit(d):
        for k, v in fields.items():
            setattr(_own(d, "images", d.num_images)[0], k, v(d) if callable(v) else v)
    return edit


def _image_texture_edit(**fields):
    def edit(d):
        t = _own(d, "textures", d.num_textures)[_first(d.textures, d.num_textures, lambda t: t.type == _abi.GBL_TEX_IMAGE)]
        for k, v in fields.items():
            setattr(t, k, v)
    return edit


def _light_edit(kind, **fields):
    def edit(d):
        lt = _own(d, "lights", d.num_lights)[_first(d.lights, d.num_lights, lambda lt: kind is None or lt.type == kind)]
        for k, v in fields.items():
            setattr(lt, k, v(d) if callable(v) else v)
    return edit


def _volume_edit(**fields):
    def edit(d):
        for k, v in fields.items():
            if k == "grid":
                d.volume.grid[0], d.volume.grid[1] = v
            else:
                setattr(d.volume, k, v)
    return edit


def _film_edit(xres=None, width=None):
    def edit(d):
        if xres is not None:
            d.film.xres = xres
        if width is not None:
            d.film.filter_width[0] = width
    return edit


def _camera_type(d):
    d.camera.type = 7


def _abi_version(d):
    d.abi_version = 99


def _both(*edits):
    def edit(d):
        for e in edits:
            e(d)
    return edit


_INV, _UNS = _abi.GBL_ERR_INVALID, _abi.GBL_ERR_UNSUPPORTED
# (id, scene, edit of a copy of its description, status, part of the message), in the order pack_scene refuses them
REFUSALS = [
    ("abi_version", "shapes", _abi_version, _INV, "wrong abi_version"),
    ("camera_type", "shapes", _camera_type, _INV, "unknown camera type"),
    ("instance_mesh", "shapes", _bad_instance("mesh"), _INV, "instance 0 references a mesh/material/light out of range"),
    ("instance_material", "shapes", _bad_instance("material"), _INV, "instance 0 references a mesh/material/light out of range"),
    ("instance_light", "shapes", _bad_instance("area_light"), _INV, "instance 0 references a mesh/material/light out of range"),
    ("mesh_shape", "shapes", _mesh_edit(shape=9), _INV, "has an unknown shape"),
    ("mesh_empty", "shapes", _mesh_edit(tri_count=0), _INV, "is empty or out of range"),
    ("mesh_vertex_range", "shapes", _mesh_edit(vertex_offset=1 << 30), _INV, "is empty or out of range"),
    ("mesh_vertex_index", "shapes", _bad_vertex_index, _INV, "has a vertex index out of range"),
    ("mesh_degenerate_uv", "imagetex", _degenerate_uv, _UNS, "triangle 0 has degenerate texture coordinates"),
    ("instance_not_invertible", "shapes", _flat_instance, _INV, "instance 0: |det(toWorld)| < 1e-5"),
    ("material_type", "shapes", _material_edit(type=99), _INV, "unknown material type"),
    ("mask_of_a_mask", "masked", _mask_of_a_mask, _INV, "must wrap a non-mask, non-subsurface material"),
    ("mask_of_subsurface", "subsurface", _material_edit(type=_abi.GBL_MAT_MASK, masked_material=lambda d: _first(
        d.materials, d.num_materials, lambda m: m.type == _abi.GBL_MAT_SUBSURFACE)), _INV, "must wrap a non-mask, non-subsurface material"),
    ("texture_out_of_range", "shapes", _material_edit(tex_color=lambda d: d.num_textures), _INV, "material 0 references a texture out of range"),
    ("texture_cycle", "shapes", _texture_chain(2, cyclic=True), _INV, "material 0 references a texture out of range (or a cyclic texture graph)"),
    ("texture_too_deep", "shapes", _texture_chain(3), _UNS, "material 0: texture graph deeper than 2 levels"),
    ("image_shape", "imagetex", _image_edit(width=3), _INV, "image 0: sides must be powers of two"),
    ("image_levels", "imagetex", _image_edit(levels=19), _INV, "image 0: sides must be powers of two"),
    ("image_texels", "imagetex", _image_edit(texel_offset=lambda d: d.num_texels), _INV, "image 0: texels out of range"),
    ("texture_mapping", "imagetex", _image_texture_edit(mapping=9), _INV, "unknown texture or mapping type"),
    ("image_texture_index", "imagetex", _image_texture_edit(image=-1), _INV, ": bad image index, filter, address mode or channel count"),
    ("image_texture_filter", "imagetex", _image_texture_edit(image_filter=9), _INV, ": bad image index, filter, address mode or channel count"),
    ("image_texture_address", "imagetex", _image_texture_edit(address=9), _INV, ": bad image index, filter, address mode or channel count"),
    ("image_texture_channels", "imagetex", _image_texture_edit(is_float=1), _INV, ": bad image index, filter, address mode or channel count"),
    ("area_light_mesh", "shapes", _light_edit(_abi.GBL_LIGHT_AREA, mesh=lambda d: d.num_meshes), _INV, "area light references a mesh out of range"),
    ("ibl_image", "ibl", _light_edit(_abi.GBL_LIGHT_IBL, image=-1), _INV, "image based light 0: bad image index"),
    ("light_type", "shapes", _light_edit(None, type=99), _INV, "unknown light type"),
    ("volume_grid", "hetero", _volume_edit(grid_channels=2), _INV, "the density grid needs positive dimensions, 1 or 3 channels and its data"),
    ("volume_step", "hetero", _volume_edit(step_size=0.0), _INV, "step_size must be a positive finite number"),
    ("volume_cells", "hetero", _volume_edit(grid=(1 << 16, 1 << 16)), _INV, "holds 2^31 values or more"),
    ("volume_steps", "hetero", _volume_edit(step_size=1e-12), _INV, "more than 10^6 steps across it"),
    ("volume_type", "hetero", _volume_edit(type=9), _INV, "unknown volume type"),
    ("film_resolution", "shapes", _film_edit(xres=0), _INV, "film resolution must be positive"),
    ("filter_width", "shapes", _film_edit(width=9.0), _UNS, "filter width must be in (0, 5.5"),
    # two faults: the earlier section's message wins
    ("material_before_film", "shapes", _both(_film_edit(width=9.0), _material_edit(type=99)), _INV, "unknown material type"),
    ("instance_before_light", "shapes", _both(_light_edit(None, type=99), _flat_instance), _INV, "instance 0: |det(toWorld)| < 1e-5"),
    ("image_before_volume", "imagetex", _both(_volume_edit(type=9), _image_edit(width=3)), _INV, "image 0: sides must be powers of two"),
]
_refusal_scenes = {}


@pytest.mark.parametrize("name,scene_name,edit,status,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_refusal_of_pack_scene_by_status_and_text(name, scene_name, edit, status, message):
    """gbl_create packs the description before it looks for a device, so every refusal of pack_scene comes back with its own
    status and message with or without a GPU.  One case per refusal, plus three descriptions with two faults that pin the order
    the sections are checked in (description, camera, instance references, meshes, instance transforms, materials, images,
    textures, lights, medium, film)."""
    from goblin_amd import scene as gs
    if scene_name not in _refusal_scenes:
        _refusal_scenes[scene_name] = gs.load_scene(scene_name, gs.config_overrides(resolution=(16, 16), spp=1, depth=2))
    desc = _abi.gbl_scene_desc.from_buffer_copy(_refusal_scenes[scene_name].desc)
    edit(desc)
    h = C.c_void_p()
    got = _abi.hip_lib().gbl_create(C.byref(desc), 0, C.byref(h))
    text = _abi.hip_lib().gbl_last_error(None).decode()
    assert (got, message in text) == (status, True), (name, got, text)
    assert not h


def test_product_never_touches_the_oracle():
    """Only tests/, smoke() and bench.py's cpu_baseline leg may use oracle/."""
    pkg = os.path.join(REPO, "goblin_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip")):
                text = open(os.path.join(root, f), errors="ignore").read()
                for needle in ("oracle_binding", "liboracle", "orc_", "oracle/"):
                    if needle in text:
                        # comments that merely point at the oracle's restated definition are fine; code use is not
                        for line in text.splitlines():
                            if needle in line:
                                stripped = line.strip()
                                assert stripped.startswith(("//", "#", "*", '"""')) or "oracle/goblin_oracle.cpp" in line, (f, line)


def test_integration_binding_compiles_against_the_reference_headers(tmp_path):
    """INTEGRATION.md's `HipPathTracer : Renderer` is the binding a Goblin maintainer would add: it must at least be
    well-formed C++ against the reference's own headers and this repository's include/ (flags = oracle/Makefile's)."""
    import re
    import subprocess
    ref = "/root/reference/src"
    if not os.path.exists(os.path.join(ref, "GoblinRenderer.h")) or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs the reference's headers and the HIP runtime API header")
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        code = re.findall(r"```cpp\n(.*?)```", f.read(), re.S)[0]
    assert "class HipPathTracer : public Renderer" in code
    src = tmp_path / "GoblinHipPathtracer.cpp"
    src.write_text(code)
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-w", "-include", "math.h", "-include", "condition_variable", "-include", "random",
                        "-Duniform_real=uniform_real_distribution", "-Duniform_int=uniform_int_distribution", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I" + ref, "-I" + os.path.join(REPO, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[:4000]


def test_source_stamp_counts_code_not_comments():
    """goblin_amd/build.py source_stamp ties the committed rocprof counters to the tree they were collected from (bench.py only
    quotes counters whose stamp is the running tree's).  It hashes code: a note beside a kernel must not orphan the counters,
    a changed token must."""
    from goblin_amd import build
    a = 'int f(int x) {   // adds one\n    return x + 1; /* really */\n}\nconst char* s = "// not a comment /* nor this */";\n'
    b = 'int f(int x) {\n  return x + 1;\n}\n\n// a later note\nconst char* s = "// not a comment /* nor this */";'
    assert build._code_only(a) == build._code_only(b)
    assert build._code_only(a) != build._code_only(a.replace("x + 1", "x + 2"))
    assert build._code_only(a) != build._code_only(a.replace("// not a comment", "// no comment"))   # (inside a literal: code)
    stamp = build.source_stamp()
    assert len(stamp) == 16 and int(stamp, 16) >= 0
    # the committed counter summaries carry the stamp of the tree they came from
    import json
    for name in ("pmc_bunny_megakernel", "pmc_cornell_wavefront", "pmc_grid_megakernel", "pmc_ao_megakernel"):
        with open(os.path.join(REPO, "profiles", name + ".json")) as f:
            assert len(json.load(f)["source_stamp"]) == 16
