"""gbl_render_aov without a GPU: the ctypes mirrors of its two structs have the C layout, and the reference helper the GPU tests
compare against (tests/aov_reference.py) is sane and reproduces the counts measured with the oracle for this feature."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from goblin_amd import _abi
import aov_reference as ar

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# scene -> (camera samples, hits, misses, hits on an instance that carries an area light) at aov_reference.SHAPE, seed 7
COUNTS = {"cornell": (1600, 1146, 454, 14), "shapes": (1600, 1040, 560, 21)}


def test_ctypes_mirror_has_the_c_layout(tmp_path):
    fields = {"gbl_aov_sample": ["albedo", "t", "normal", "instance", "position", "hit"],
              "gbl_aov_targets": ["albedo_accum", "normal_accum", "depth_accum", "samples_out"]}
    src = tmp_path / "aov_sizes.c"
    body = "".join('printf("%s %%zu\\n", sizeof(%s));\n' % (s, s) for s in fields)
    body += "".join('printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (s, f, s, f) for s, fs in fields.items() for f in fs)
    src.write_text('#include <stdio.h>\n#include "goblin_hip.h"\nint main(void){\n' + body + "return 0;}\n")
    exe = tmp_path / "aov_sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])   # plain C
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["gbl_aov_sample"]) == 48 == C.sizeof(_abi.gbl_aov_sample)
    for s, fs in fields.items():
        assert C.sizeof(getattr(_abi, s)) == int(out[s]), s
        for f in fs:
            assert getattr(getattr(_abi, s), f).offset == int(out[s + "." + f]), (s, f)
    # the words of a record row as the Python face hands them out: 7 = instance, 11 = hit
    assert _abi.gbl_aov_sample.instance.offset == 7 * 4 and _abi.gbl_aov_sample.hit.offset == 11 * 4
    assert _abi.GBL_ABI_VERSION == 14
    assert "gbl_render_aov" in _abi.HIP_SYMBOLS and "gbl_aov_resolve_depth" in _abi.HIP_SYMBOLS


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_reference_helper_is_sane(name):
    ref = ar.reference(name)
    hit = ref.hit == 1
    n, hits, misses, emitter = COUNTS[name]
    print(name, "samples", ref.n, "hits", int(hit.sum()), "misses", int((~hit).sum()), "on the emitter", int(ref.emitter_hits().sum()))
    assert (ref.n, int(hit.sum()), int((~hit).sum()), int(ref.emitter_hits().sum())) == (n, hits, misses, emitter)
    assert ref.window == (-2, 18, -2, 18)
    # misses carry the fields of the table
    assert (ref.t[~hit] == -1).all() and (ref.instance[~hit] == -1).all() and not ref.position[~hit].any() and not ref.normal[~hit].any()
    assert (ref.instance[hit] >= 0).all() and (ref.instance[hit] < ref.scene.desc.num_instances).all() and (ref.t[hit] > 0).all()
    length = np.sqrt((ref.normal[hit].astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(length - 1.0).max() <= 1e-5
    along = ref.o[hit].astype(np.float64) + ref.t[hit, None].astype(np.float64) * ref.d[hit].astype(np.float64)
    err = np.abs(along - ref.position[hit]).max(axis=1)
    assert (err <= 1e-4 * np.maximum(1.0, ref.t[hit])).all(), err.max()
    # every first colour slot of these scenes is a constant, within [0, 1]
    assert ref.albedo_known.all() and ref.albedo.min() >= 0.0 and ref.albedo.max() <= 1.0 and ref.albedo[hit].max() > 0.0
    films = ref.films()
    assert set(films) == {"albedo", "normal", "depth"}
    for f in films.values():
        assert f.shape == (16, 16, 4) and np.isfinite(f).all() and (f[..., 3] > 0).all()
    np.testing.assert_array_equal(films["albedo"][..., 3], films["depth"][..., 3])
    depth, coverage = ar.depth_and_coverage(films["depth"])
    assert coverage.min() >= 0.0 and coverage.max() <= 1.0 + 1e-6 and 0.0 < coverage.mean() < 1.0
    assert depth[coverage > 0].min() >= ref.t[hit].min() * (1 - 1e-6) and depth.max() <= ref.t[hit].max() * (1 + 1e-6)


def test_albedo_slot_follows_the_material_table():
    """Subsurface reads Kr from color3, a mask answers with the material it wraps, everything else reads color."""
    sub = ar.scene("subsurface").desc
    kinds = {sub.materials[i].type for i in range(sub.num_materials)}
    assert _abi.GBL_MAT_SUBSURFACE in kinds
    for i in range(sub.num_materials):
        m = sub.materials[i]
        color, tex = ar.albedo_slot(sub, i)
        want = m.color3 if m.type == _abi.GBL_MAT_SUBSURFACE else m.color
        assert tuple(color) == tuple(np.array(want[:], np.float32)) and tex == (m.tex_color3 if m.type == _abi.GBL_MAT_SUBSURFACE else m.tex_color)
    masked = ar.scene("masked").desc
    wrappers = [i for i in range(masked.num_materials) if masked.materials[i].type == _abi.GBL_MAT_MASK]
    assert wrappers
    for i in wrappers:
        inner = masked.materials[masked.materials[i].masked_material]
        color, tex = ar.albedo_slot(masked, i)
        assert tuple(color) == tuple(np.array(inner.color[:], np.float32)) and tex == inner.tex_color
