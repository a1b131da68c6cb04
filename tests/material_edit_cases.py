"""The material and texture edits that tests/test_materials_cpu.py (through tests/materials_repack.cpp) and
tests/test_gpu_materials.py share, stated once.

A case is (scene, name, edits); an edit is ("m" | "t", record index, field, value): a material's or a texture's field takes the
value (a float, an int for a texture slot, or a list of floats; to_tex is the ten floats of a gbl_trs: position, orientation
wxyz, scale).  The indices are those of the bundled scenes' descriptions as the loader makes them (materials in the file's order,
the textures the materials reach, children before their parents).

Every case's values are chosen so that the oracle's per-sample radiance of the edited description differs from the scene's own
at the tests' frame (16 x 16, 2 spp, depth 3, seed 20261020): test_materials_cpu.py checks that on the CPU, so "the frames
differ" in the GPU tests is a property of the input.  Two things that check found: the path tracer's frame of the bundled scenes
does not see a transparent material's Kt at depth 3 (the Whitted scene does, so the case is there), and the oracle's radiance of
a subsurface material with an index below 1 is not finite at this frame, so that branch of the A polynomial is left to the CPU
test of the compose functions.
"""
import ctypes as C

from goblin_amd import _abi

SEED = 20261020
Q90X = [0.7071068, 0.7071068, 0.0, 0.0]   # 90 degrees about x

CASES = [
    # ---- cornell: a lambert wall, the transparent, mirror and blinn boxes (materials 1, 3, 4, 5); no texture
    ("cornell", "lambert_color", [("m", 1, "color", [0.2, 0.6, 0.9])]),
    ("cornell", "transparent_color", [("m", 3, "color", [0.6, 0.9, 0.7])]),
    ("cornell", "transparent_index", [("m", 3, "index", 1.2)]),
    ("cornell", "mirror_color", [("m", 4, "color", [0.5, 0.9, 0.4])]),
    ("cornell", "mirror_index", [("m", 4, "index", 1.4)]),
    ("cornell", "mirror_k", [("m", 4, "k", 2.0)]),
    ("cornell", "blinn_color", [("m", 5, "color", [0.3, 0.7, 0.9])]),
    ("cornell", "blinn_index", [("m", 5, "index", 2.5)]),
    ("cornell", "blinn_k_conductor", [("m", 5, "k", 3.0)]),
    ("cornell", "blinn_exponent", [("m", 5, "exponent", 8.0)]),
    ("cornell", "several_records", [("m", 0, "color", [0.4, 0.5, 0.6]), ("m", 1, "color", [0.1, 0.8, 0.1]), ("m", 2, "color", [0.9, 0.2, 0.2]),
                                    ("m", 3, "index", 1.3)]),
    # ---- shapes: analytic shapes (the EXT kernels)
    ("shapes", "lambert_color", [("m", 1, "color", [0.1, 0.3, 0.8])]),
    ("shapes", "transparent_index", [("m", 2, "index", 1.25)]),
    ("shapes", "blinn_exponent", [("m", 3, "exponent", 6.0)]),
    # ---- masked: masks 2 (wraps 1, alpha from float checkerboard 2), 4 (wraps 3), 6 (wraps mirror 5, checkerboard 5), 8 (wraps glass 7)
    ("masked", "mask_alpha", [("m", 4, "exponent", 0.9)]),
    ("masked", "mask_transparent_color", [("m", 4, "color", [0.2, 0.9, 0.4])]),
    ("masked", "wrapped_lambert_color", [("m", 1, "color", [0.8, 0.2, 0.7])]),
    ("masked", "wrapped_mirror_color", [("m", 5, "color", [0.2, 0.9, 0.3])]),
    ("masked", "mask_slot_repointed", [("m", 2, "tex_exponent", 5)]),
    ("masked", "float_checkerboard_scrolled", [("t", 2, "uv_offset", [0.5, 0.25])]),
    ("masked", "float_constant_value", [("t", 3, "value", [0.2, 0.0, 0.0])]),
    # ---- subsurface: 1 sigma_a / sigma_s' / eta / g / Kr constants, 2 with a checkerboard in sigma_s'
    ("subsurface", "sigma_a", [("m", 1, "color", [0.5, 0.2, 0.1])]),
    ("subsurface", "sigma_s_prime", [("m", 1, "color2", [20.0, 35.0, 12.0])]),
    ("subsurface", "index", [("m", 1, "index", 1.1)]),
    ("subsurface", "g", [("m", 2, "k", -0.3)]),
    ("subsurface", "kr", [("m", 1, "color3", [0.4, 0.6, 0.9])]),
    ("subsurface", "sigma_s_prime_texture_value", [("t", 0, "value", [30.0, 200.0, 60.0])]),
    # ---- whitted (the Whitted integrator): glass 1, mirror 2, lambert 3, blinn 4, a filtered checkerboard 2 on the floor
    ("whitted", "transparent_index", [("m", 1, "index", 1.2)]),
    ("whitted", "transparent_color2", [("m", 1, "color2", [0.2, 0.3, 0.9])]),
    ("whitted", "mirror_color", [("m", 2, "color", [0.4, 0.8, 0.5])]),
    ("whitted", "lambert_color", [("m", 3, "color", [0.1, 0.6, 0.3])]),
    ("whitted", "blinn_exponent", [("m", 4, "exponent", 5.0)]),
    ("whitted", "checkerboard_uv_scale", [("t", 2, "uv_scale", [3.0, 5.0])]),
    # ---- textured: checkerboards 2 (uv), 10 (spherical), scale 7 = checkerboard 5 x float constant 6, float checkerboard 13
    ("textured", "checkerboard_scrolled", [("t", 2, "uv_offset", [0.75, 0.5])]),
    ("textured", "constant_behind_a_scale", [("t", 6, "value", [0.2, 0.0, 0.0])]),
    ("textured", "constant_two_levels_down", [("t", 3, "value", [0.1, 0.8, 0.3])]),
    ("textured", "spherical_to_tex", [("t", 10, "to_tex", [0.0, 0.0, 0.0] + Q90X + [1.0, 1.0, 1.0])]),
    ("textured", "float_checkerboard_uv_scale", [("t", 13, "uv_scale", [5.0, 2.0])]),
    ("textured", "blinn_color_beside_a_slot", [("m", 3, "color", [0.3, 0.4, 0.9])]),
    ("textured", "color_slot_repointed", [("m", 1, "tex_color", 2)]),
    ("textured", "materials_and_textures", [("m", 3, "index", 2.2), ("m", 4, "color", [0.7, 0.9, 0.8]), ("t", 15, "value", [0.2, 0.3, 0.9]),
                                            ("t", 16, "uv_offset", [0.5, 0.0])]),
    # ---- bumpy: bump maps 2 (image x constant) and 14 (float checkerboard), normal maps 6 (image) and 19 (constant); mask 5 wraps 1
    ("bumpy", "bump_slot_repointed", [("m", 0, "tex_bump", 14)]),
    ("bumpy", "normal_slot_repointed_under_its_mask", [("m", 1, "tex_normal", 19)]),
    ("bumpy", "float_image_texture_scrolled", [("t", 0, "uv_offset", [0.3, 0.6])]),
    ("bumpy", "bump_height_constant", [("t", 1, "value", [0.25, 0.0, 0.0])]),
    ("bumpy", "normal_map_constant", [("t", 19, "value", [0.2, 0.6, 0.9])]),
    # ---- imagetex: EWA image texture 0, a spherical image texture 4, a bordered one 8
    ("imagetex", "image_texture_scrolled", [("t", 0, "uv_offset", [0.6, 0.35])]),
    ("imagetex", "image_texture_max_anisotropy", [("t", 0, "max_anisotropy", 1.0)]),
    ("imagetex", "spherical_image_to_tex", [("t", 4, "to_tex", [0.0, 0.0, 0.0] + Q90X + [1.0, 1.0, 1.0])]),
]
IDS = ["%s-%s" % (scene, name) for scene, name, _ in CASES]
MATERIAL_FLOATS = {"color": 3, "color2": 3, "color3": 3, "index": 1, "k": 1, "exponent": 1}
MATERIAL_SLOTS = ("tex_color", "tex_color2", "tex_exponent", "tex_color3", "tex_bump", "tex_normal")
TEXTURE_FLOATS = {"value": 3, "uv_scale": 2, "uv_offset": 2, "to_tex": 10, "max_anisotropy": 1}


def case(scene, name):
    return next(c for c in CASES if c[0] == scene and c[1] == name)


def as_list(value):
    return [float(v) for v in value] if isinstance(value, (list, tuple)) else [value]


def case_file_text():
    """The cases as tests/materials_repack.cpp reads them: `case scene name`, one `m|t index field n values...` line per edit, `end`."""
    lines = []
    for scene, name, edits in CASES:
        lines.append("case %s %s" % (scene, name))
        for table, index, field, value in edits:
            values = as_list(value)
            lines.append("%s %d %s %d %s" % (table, index, field, len(values), " ".join(repr(v) for v in values)))
        lines.append("end")
    return "\n".join(lines) + "\n"


def set_field(rec, field, value):
    if field == "to_tex":
        v = as_list(value)
        rec.to_tex.position[:], rec.to_tex.orientation[:], rec.to_tex.scale[:] = v[0:3], v[3:7], v[7:10]
    elif isinstance(getattr(rec, field), C.Array):
        whole = getattr(rec, field)._type_ is not C.c_float      # (a texture's children)
        getattr(rec, field)[:] = [int(v) if whole else float(v) for v in value]
    else:
        setattr(rec, field, value)
    return rec


def records(scene):
    """Copies of the description's gbl_material and gbl_texture records."""
    d = scene.desc
    return ([_abi.gbl_material.from_buffer_copy(d.materials[i]) for i in range(d.num_materials)],
            [_abi.gbl_texture.from_buffer_copy(d.textures[i]) for i in range(d.num_textures)])


def edited_records(scene, edits):
    materials, textures = records(scene)
    for table, index, field, value in edits:
        set_field((materials if table == "m" else textures)[index], field, value)
    return materials, textures


def ranges(edits):
    """{table: (first, count)} of the contiguous ranges a case's edits span."""
    out = {}
    for table in ("m", "t"):
        idx = [e[1] for e in edits if e[0] == table]
        if idx:
            out[table] = (min(idx), max(idx) - min(idx) + 1)
    return out


def write_desc(scene, materials, textures):
    """The edited description: the scene's records overwritten in place."""
    d = scene.desc
    for i, rec in enumerate(materials):
        d.materials[i] = rec
    for i, rec in enumerate(textures):
        d.textures[i] = rec


def material_rows(materials):
    """The (n, 12) rows of gbl_update_materials_device for these records."""
    return [list(m.color) + list(m.color2) + list(m.color3) + [m.index, m.k, m.exponent] for m in materials]


def texture_rows(textures):
    return [list(t.value) + list(t.uv_scale) + list(t.uv_offset) for t in textures]


def device_form_takes(edits):
    """The case changes nothing but what a row holds: no slot index, to_tex or max_anisotropy."""
    return all(field in ("color", "color2", "color3", "index", "k", "exponent", "value", "uv_scale", "uv_offset") for _, _, field, _ in edits)
