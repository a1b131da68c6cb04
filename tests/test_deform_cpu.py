"""gbl_render_motion_deform without a GPU: the ABI (header, ctypes mirror, exported name), the numpy restatement the GPU tests
compare against (tests/deform_reference.py) -- that its deforming fixture makes the static treatment ghost where the
deformation-aware planes do not, and its normal rule -- and the host side of the previous poses (goblin_amd/csrc/motion_stage.cpp)
driven stand-alone under AddressSanitizer and UBSan by tests/deform_stage.cpp."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from goblin_amd import _abi
import deform_reference as dr
import meshes
import motion_reference as mr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "goblin_amd", "csrc")
F = np.float32
NAME = "gbl_render_motion_deform"
NOT_DEFORMED = -2 ** 31


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_abi(tmp_path):
    """Declared, mirrored, exported; no existing layout changed.  Fails without the feature."""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "goblin_hip.h")).read(), flags=re.S)
    assert re.search(r"\bgbl_status\s+%s\s*\(" % NAME, header)
    assert NAME in _abi.HIP_SYMBOLS
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libgoblin_hip.so"))
    assert getattr(lib, NAME) is not None
    structs = {"gbl_motion_mesh": ["mesh", "reserved", "positions"], "gbl_motion_params": ["prev_camera", "prev_to_world", "normal_accum", "stream"]}
    body = 'printf("floats %d\\n", GBL_MOTION_FLOATS_PER_PIXEL);\nprintf("abi %d\\n", GBL_ABI_VERSION);\n'
    for s, fields in structs.items():
        body += 'printf("%s.size %%zu\\n", sizeof(%s));\n' % (s, s)
        body += "".join('printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (s, f, s, f) for f in fields)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "goblin_hip.h"\nint main(void){\n' + body + "return 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])   # plain C
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for s, fields in structs.items():
        mirror = getattr(_abi, s)
        assert C.sizeof(mirror) == int(out[s + ".size"]), s
        assert [f for f, _ in mirror._fields_] == fields
        for f in fields:
            assert getattr(mirror, f).offset == int(out["%s.%s" % (s, f)]), (s, f)
    # gbl_motion_params is what it was: a camera, two pointers after it, the stream
    assert C.sizeof(_abi.gbl_motion_params) == C.sizeof(_abi.gbl_camera) + 3 * C.sizeof(C.c_void_p)
    assert _abi.GBL_MOTION_FLOATS_PER_PIXEL == int(out["floats"]) == 8
    assert _abi.GBL_ABI_VERSION == int(out["abi"]) == 14


# ---- the ghost fixture ---------------------------------------------------------------------------------------------------
def sq_error(a, b, where):
    return float(((a.astype(np.float64) - b.astype(np.float64))[where] ** 2).sum())


def test_the_deforming_fixture_ghosts_when_the_sheet_is_treated_as_static():
    s = dr.deforming_sequence()
    sheet = s["inst"] == 1
    stayed = sheet & (s["prev_inst"] == 1)
    stale = np.abs(s["analytic"].astype(np.float64) - s["prev_analytic"])[stayed][:, :2]
    print("pixels of the sheet %d, covered by it in both frames %d; |current - stale| over them: mean %.3f" % (sheet.sum(), stayed.sum(), stale.mean()))
    assert sheet.sum() >= 60 and stayed.sum() >= 40 and stale.mean() > 0.1
    # depth and normal have not changed: nothing but the planes can tell the frames apart
    np.testing.assert_array_equal(s["t"][stayed], s["prev_t"][stayed])
    assert mr.moved_instances(s["instances"], s["instances"]) == []
    for variance in (None, s["variance"]):
        static = mr.accumulate_motion(s["film"], s["depth"], s["motion_static"], variance=variance, normal=s["normal"], history=s["history"], **s["params"])
        aware = mr.accumulate_motion(s["film"], s["depth"], s["motion"], variance=variance, normal=s["normal"], history=s["history"], **s["params"])
        ghost = stayed & static["has_history"]
        both = sheet & aware["valid"] & static["has_history"] & aware["has_history"]
        e_static, e_aware = sq_error(static["film"][..., :3], s["analytic"], both), sq_error(aware["film"][..., :3], s["analytic"], both)
        print("variance plane %s: ghost pixels %d of %d; on %d pixels of the sheet with history in both: squared error static %.4g, deformation-aware %.4g "
              "(ratio %.4f)" % (variance is not None, ghost.sum(), stayed.sum(), both.sum(), e_static, e_aware, e_aware / e_static))
        assert ghost.sum() >= 0.8 * stayed.sum()
        assert both.sum() >= 40 and e_aware < e_static
        wall = s["inst"] == 0
        for k in ("film", "variance", "history"):
            a, b = aware[k], static[k]
            if k == "history":
                a, b = np.moveaxis(a, 0, 2), np.moveaxis(b, 0, 2)
            np.testing.assert_array_equal(bits(a[wall]), bits(b[wall]), err_msg=k)
    np.testing.assert_array_equal(bits(s["motion"][:, s["inst"] != 1]), bits(s["motion_static"][:, s["inst"] != 1]))
    # the planes themselves: a sheet pixel points back along x by the shear at its height, at the same depth, with the same normal
    H, W = s["inst"].shape
    info = {}
    planes = dr.deform_planes(s["t"], s["inst"], s["cur_camera"], s["prev_camera"], s["instances"], s["instances"], s["normal"], s["instance_mesh"],
                              s["meshes"], info=info)
    np.testing.assert_array_equal(bits(planes), bits(s["motion"]))
    np.testing.assert_array_equal(info["on"], sheet)
    assert info["t_miss"][sheet].max() < 1e-5 and set(np.unique(info["tri"][sheet])) == {0, 1}
    px = (s["motion"][0, ..., 0] - s["motion_static"][0, ..., 0]).astype(np.float64)
    assert (px[sheet] <= 1e-4).all() and px[sheet].min() < -2.0           # up to SHEAR at the upper edge, in pixels
    o, d = dr.camera_ray(dr.pack_camera(s["prev_camera"], W, H), s["motion"][0, ..., 0].astype(np.float64), s["motion"][0, ..., 1].astype(np.float64), np.float64)
    back = tuple(o[k] + d[k] * s["motion"][0, ..., 2] for k in range(3))        # the previous point again, from where it is seen and how far
    assert np.abs(back[2][sheet] - mr.SQUARE_Z).max() < 1e-4                    # still in the sheet's plane
    hy = dr.SHEET_HALF[1]
    cur = dr.camera_ray(dr.pack_camera(s["cur_camera"], W, H), *(np.mgrid[0:H, 0:W][::-1] + 0.5), np.float64)
    here = tuple(cur[0][k] + cur[1][k] * s["t"].astype(np.float64) for k in range(3))
    want_x = here[0] - dr.SHEAR * (here[1] + hy) / (2.0 * hy)
    assert np.abs(back[0] - want_x)[sheet].max() < 1e-4 and np.abs(back[1] - here[1])[sheet].max() < 1e-4
    np.testing.assert_allclose(s["motion"][1, ..., :3][sheet], np.broadcast_to(np.array([0, 0, -1], F), (int(sheet.sum()), 3)), atol=1e-6)
    np.testing.assert_array_equal(s["motion"][1, ..., 3], (s["inst"] + 1).astype(F))


@pytest.mark.parametrize("shape", [(37, 23), (9, 9), (1, 1)])
def test_zero_shear_is_motion_planes_bit_for_bit(shape):
    s = dr.deforming_sequence(shape[0], shape[1], 0.0)
    assert dr.deformed_meshes(s["meshes"]) == {}
    np.testing.assert_array_equal(bits(s["motion"]), bits(s["motion_static"]))
    for normal in (None, s["normal"]):
        a = dr.deform_planes(s["t"], s["inst"], s["cur_camera"], s["prev_camera"], s["instances"], None, normal, s["instance_mesh"], s["meshes"])
        b = mr.motion_planes(s["t"], s["inst"], s["cur_camera"], s["prev_camera"], s["instances"], None, normal)
        np.testing.assert_array_equal(bits(a), bits(b))


# ---- the normal rule -----------------------------------------------------------------------------------------------------
def cols(a, T=F):
    return tuple(np.asarray(a, T)[..., k] for k in range(3))


def test_normal_rule():
    rng = np.random.default_rng(5)
    n = 64
    e1, e2, u = (rng.normal(size=(n, 3)) for _ in range(3))
    # identity: u comes back bitwise in float32
    x = dr.normal_rule(cols(u), cols(e1), cols(e2), cols(e1), cols(e2), F)
    # (the rule recombines u from its three components: exact only up to rounding; what must be bitwise is the fallback, and the
    #  identity in the sense of the contract -- an unchanged mesh never reaches the rule -- is test_zero_shear's)
    np.testing.assert_allclose(np.stack(x, -1), u.astype(F), rtol=0, atol=2e-5 * np.abs(u).max())
    # a rigid rotation R of the triangle carries u to R u
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    R = q * np.sign(np.linalg.det(q))
    x = dr.normal_rule(cols(u, np.float64), cols(e1, np.float64), cols(e2, np.float64), cols(e1 @ R.T, np.float64), cols(e2 @ R.T, np.float64), np.float64)
    np.testing.assert_allclose(np.stack(x, -1), u @ R.T, rtol=0, atol=1e-12)
    x32 = dr.normal_rule(cols(u), cols(e1), cols(e2), cols((e1.astype(F) @ R.T.astype(F))), cols((e2.astype(F) @ R.T.astype(F))), F)
    np.testing.assert_allclose(np.stack(x32, -1), u @ R.T, rtol=0, atol=2e-5 * np.abs(u).max())
    # the defining equations under a general deformation
    f1, f2 = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    x = np.stack(dr.normal_rule(cols(u, np.float64), cols(e1, np.float64), cols(e2, np.float64), cols(f1, np.float64), cols(f2, np.float64), np.float64), -1)
    g, gp = np.cross(e1, e2), np.cross(f1, f2)
    gh, ghp = g / np.linalg.norm(g, axis=1)[:, None], gp / np.linalg.norm(gp, axis=1)[:, None]
    for a, b in ((f1, e1), (f2, e2), (ghp, gh)):
        np.testing.assert_allclose((a * x).sum(1), (b * u).sum(1), rtol=0, atol=1e-10)
    # a previous (or current) triangle without area returns u, bitwise
    flat = e1 * 2.0
    for args in ((cols(e1), cols(e2), cols(e1), cols(flat)), (cols(e1), cols(flat), cols(f1), cols(f2)), (cols(e1), cols(e2), cols(np.zeros((n, 3))), cols(f2))):
        x = dr.normal_rule(cols(u), *args, F)
        np.testing.assert_array_equal(bits(np.stack(x, -1)), bits(u.astype(F)))


def test_identity_deformation_returns_u_bitwise():
    """On exactly representable edges (an axis-aligned right triangle) the rule's three terms are exact: u comes back bitwise."""
    e1, e2 = np.array([[2.0, 0.0, 0.0]]), np.array([[0.0, 0.5, 0.0]])
    u = np.array([[0.25, -3.0, 1.5]])
    x = dr.normal_rule(cols(u), cols(e1), cols(e2), cols(e1), cols(e2), F)
    np.testing.assert_array_equal(bits(np.stack(x, -1)), bits(u.astype(F)))


# ---- the host side of the previous poses, stand-alone under the sanitizers ------------------------------------------------
@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    work = tmp_path_factory.mktemp("deform_stage")
    exe = os.path.join(str(work), "deform_stage")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(REPO, "tests", "deform_stage.cpp"), os.path.join(CSRC, "motion_stage.cpp"), "-o", exe])
    count = [0]

    def run(mesh_table, positions, prev, list_is_null=False, num_prev=None):
        """mesh_table: [(vertex_offset, vertex_count, shape)]; prev: [(mesh, reserved, positions or None)]."""
        words = [np.array([len(mesh_table)], "<u4"), np.array(mesh_table, "<u4").reshape(-1)]
        positions = np.asarray(positions, "<f4").reshape(-1, 3)
        words += [np.array([len(positions)], "<u4"), positions.reshape(-1)]
        words += [np.array([1 if list_is_null else 0, len(prev) if num_prev is None else num_prev], "<u4")]
        if not list_is_null:
            for mesh, reserved, pos in prev:
                flat = np.zeros(0, "<f4") if pos is None else np.asarray(pos, "<f4").reshape(-1)
                words += [np.array([mesh, reserved, 1 if pos is None else 0, len(flat)], "<u4"), flat]
        job = os.path.join(str(work), "job%d.bin" % count[0])
        count[0] += 1
        with open(job, "wb") as f:
            for w in words:
                f.write(np.ascontiguousarray(w).tobytes())
        p = subprocess.run([exe, job], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr.decode()[-2000:])      # clean under both sanitizers
        lines = dict(line.split(" ", 1) if " " in line else (line, "") for line in p.stdout.decode().splitlines())
        if lines["ok"] == "0":
            return False, lines["err"]
        table = np.array(lines["table"].split(), np.int64)
        packed = np.array([int(w, 16) for w in lines["packed"].split()], np.uint32).view(F).reshape(-1, 3)
        return True, (table, packed)
    return run


def numpy_stage(mesh_table, positions, prev):
    """The table and the packed positions by the issue's rule."""
    table = np.full(len(mesh_table), NOT_DEFORMED, np.int64)
    packed = []
    first = 0
    for mesh, _, pos in prev:
        off, count, _ = mesh_table[mesh]
        pos = np.asarray(pos, F).reshape(-1, 3)
        if count == 0 or pos.tobytes() == np.asarray(positions, F).reshape(-1, 3)[off:off + count].tobytes():
            continue
        table[mesh] = first - off
        packed.append(pos)
        first += count
    return table, (np.concatenate(packed) if packed else np.zeros((0, 3), F))


def test_staging_program(stage):
    names = list(meshes.ALL)
    V = [meshes.floor()[0]] + [meshes.mesh(n)[0] for n in names]
    mesh_table, off = [], 0
    for v in V:
        mesh_table.append((off, len(v), 0))
        off += len(v)
    mesh_table.append((off, 0, 1))           # a sphere ...
    mesh_table.append((off, 0, 2))           # ... and a disk
    sphere, disk = len(V), len(V) + 1
    positions = np.concatenate(V)
    rng = np.random.default_rng(11)
    moved = [(v + rng.uniform(-0.01, 0.01, v.shape).astype(F)).astype(F) for v in V]

    def check(prev):
        ok, got = stage(mesh_table, positions, prev)
        assert ok, got
        table, packed = numpy_stage(mesh_table, positions, prev)
        np.testing.assert_array_equal(got[0], table)
        np.testing.assert_array_equal(bits(got[1]), bits(packed))
        return got
    # nothing listed, and every mesh listed unchanged: no mesh is deformed
    table, packed = check([])
    assert (table == NOT_DEFORMED).all() and len(packed) == 0
    table, packed = check([(m, 0, V[m]) for m in range(len(V))])
    assert (table == NOT_DEFORMED).all() and len(packed) == 0
    # every mesh deformed, in order and out of order; the table then points each mesh's absolute vertex ids into the packed block
    for order in (list(range(len(V))), list(reversed(range(len(V)))), [3, 1, 7]):
        table, packed = check([(m, 0, moved[m]) for m in order])
        for m in order:
            o, c, _ = mesh_table[m]
            np.testing.assert_array_equal(bits(packed[o + table[m]:o + table[m] + c]), bits(moved[m]))
        assert (table != NOT_DEFORMED).sum() == len(order)
    # an unchanged mesh between two deformed ones is dropped, and takes no room
    table, packed = check([(2, 0, moved[2]), (4, 0, V[4]), (5, 0, moved[5])])
    assert table[4] == NOT_DEFORMED and len(packed) == len(V[2]) + len(V[5])
    # one vertex differing in one bit (-0.0 against 0.0 compares equal as a number) deforms the mesh
    flipped = V[0].copy()
    assert flipped[0, 1] == 0.0
    flipped[0, 1] = -0.0
    table, packed = check([(0, 0, flipped)])
    assert table[0] == 0 and len(packed) == len(V[0])
    # the refusals, each naming the entry point
    nan, inf = V[1].copy(), V[3].copy()
    nan[-1, 2], inf[0, 0] = np.nan, -np.inf
    refusals = [(dict(prev=[], list_is_null=True, num_prev=2), "is NULL with num_prev_meshes > 0"),
                (dict(prev=[(1, 0, None)]), "positions is NULL"),
                (dict(prev=[(len(mesh_table), 0, moved[1])]), "out of range"),
                (dict(prev=[(0xffffffff, 0, moved[1])]), "out of range"),
                (dict(prev=[(sphere, 0, moved[1])]), "sphere or a disk"),
                (dict(prev=[(disk, 0, moved[1])]), "sphere or a disk"),
                (dict(prev=[(1, 0, moved[1]), (2, 0, moved[2]), (1, 0, V[1])]), "listed twice"),
                (dict(prev=[(2, 0, V[2]), (2, 0, V[2])]), "listed twice"),
                (dict(prev=[(1, 7, moved[1])]), "reserved"),
                (dict(prev=[(0, 0, moved[0]), (1, 0, nan)]), "not finite"),
                (dict(prev=[(3, 0, inf)]), "not finite")]
    for kw, needle in refusals:
        ok, msg = stage(mesh_table, positions, **kw)
        print(needle, "->", ok, repr(msg))
        assert not ok and needle in msg and NAME in msg, (kw.get("num_prev"), needle, msg)
    # a NULL list with no entries is no list
    ok, got = stage(mesh_table, positions, [], list_is_null=True, num_prev=0)
    assert ok and (got[0] == NOT_DEFORMED).all()
