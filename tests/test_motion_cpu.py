"""gbl_get_instances / gbl_render_motion / gbl_film_accumulate_motion without a GPU: the ABI (header, ctypes mirror, exported
names) and the numpy restatement the GPU tests compare against (tests/motion_reference.py) -- that its moving fixture makes the
plain accumulation ghost where the motion-aware one does not, reaches every branch, and that over a static scene the two
accumulations are one."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from goblin_amd import _abi
import motion_reference as mr
import temporal_reference as tr
from test_temporal_cpu import only

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = ("gbl_get_instances", "gbl_render_motion", "gbl_film_accumulate_motion")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_abi(tmp_path):
    """(c) of the issue: declared, mirrored, exported.  Fails without the feature."""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "goblin_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bgbl_status\s+%s\s*\(" % name, header), name
        assert name in _abi.HIP_SYMBOLS
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libgoblin_hip.so"))
    for name in NAMES:
        assert getattr(lib, name) is not None, name
    fields = ["prev_camera", "prev_to_world", "normal_accum", "stream"]
    src = tmp_path / "sizes.c"
    body = 'printf("size %zu\\n", sizeof(gbl_motion_params));\nprintf("floats %d\\n", GBL_MOTION_FLOATS_PER_PIXEL);\nprintf("abi %d\\n", GBL_ABI_VERSION);\n'
    body += "".join('printf("%s %%zu\\n", offsetof(gbl_motion_params, %s));\n' % (f, f) for f in fields)
    src.write_text('#include <stdio.h>\n#include "goblin_hip.h"\nint main(void){\n' + body + "return 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])   # plain C
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert C.sizeof(_abi.gbl_motion_params) == int(out["size"])
    for f in fields:
        assert getattr(_abi.gbl_motion_params, f).offset == int(out[f]), f
    assert [f for f, _ in _abi.gbl_motion_params._fields_] == fields
    assert _abi.GBL_MOTION_FLOATS_PER_PIXEL == int(out["floats"]) == 8
    assert _abi.GBL_ABI_VERSION == int(out["abi"]) == 14      # new entry points only: no existing layout changed


def sq_error(a, b, where):
    return float(((a.astype(np.float64) - b.astype(np.float64))[where] ** 2).sum())


def test_the_moving_fixture_ghosts_without_the_planes():
    """(a): 37 x 23, the square slides by half a stripe period under a still camera."""
    s = mr.moving_sequence()
    H, W = s["inst"].shape
    mover = s["inst"] == 1
    stayed = mover & (s["prev_inst"] == 1)          # the square covers the pixel in both frames: the plain path's ghost
    # the fixture first: a stale texel of the square is the opposite stripe, so accepting it must hurt
    stale = np.abs(s["analytic"].astype(np.float64) - s["prev_analytic"])[stayed][:, :2]
    print("pixels of the square %d, covered by it in both frames %d; |current - stale| over them: mean %.3f" % (mover.sum(), stayed.sum(), stale.mean()))
    assert mover.sum() >= 60 and stayed.sum() >= 40 and stale.mean() > 0.3
    assert mr.moved_instances(s["cur_instances"], s["prev_instances"]) == [1]
    for variance in (None, s["variance"]):
        plain = tr.accumulate(s["film"], s["depth"], s["cur_camera"], variance=variance, normal=s["normal"], history=s["history"],
                              prev_camera=s["prev_camera"], **s["params"])
        aware = mr.accumulate_motion(s["film"], s["depth"], s["motion"], variance=variance, normal=s["normal"], history=s["history"], **s["params"])
        valid = aware["valid"]
        np.testing.assert_array_equal(valid, plain["valid"])
        ok = s["motion"][0, ..., 3] != 0
        taps, has = aware["taps"], aware["has_history"]
        covered = valid & aware["surf"]
        # the plain path accepts the ghost: the square's depth and normal have not changed
        ghost = stayed & plain["has_history"]
        both = mover & valid & plain["has_history"] & has
        e_plain, e_aware = sq_error(plain["film"][..., :3], s["analytic"], both), sq_error(aware["film"][..., :3], s["analytic"], both)
        left = mover & covered & ok & ~taps["inside"].any(0)
        disoccluded = (s["inst"] == 0) & (s["prev_inst"] == 1) & covered
        accepted = taps["accepted"].sum(0)
        print("variance plane %s: ghost pixels %d of %d; on %d pixels of the square with history in both: squared error plain %.4g, motion-aware %.4g "
              "(ratio %.4f); P_prev outside the image %d, ok = 0: %d, disoccluded wall %d of which depth-only rejections %d, 1-3 taps accepted %d, "
              "N >= 4: %d, N < 4 with history: %d" %
              (variance is not None, ghost.sum(), stayed.sum(), both.sum(), e_plain, e_aware, e_aware / e_plain, left.sum(), (~ok).sum(), disoccluded.sum(),
               (disoccluded & only(taps, "depth_ok")).sum(), ((accepted >= 1) & (accepted <= 3)).sum(), (aware["N"] >= 4).sum(), (has & (aware["N"] < 4)).sum()))
        assert ghost.sum() >= 0.8 * stayed.sum()
        assert both.sum() >= 40 and e_aware < e_plain
        assert left.any() and not has[left].any()
        assert (~ok).any() and not has[~ok].any() and not s["motion"][0][~ok].any()
        assert np.array_equal(ok, s["inst"] >= 0)                 # a still camera: every hit lies in front of it
        assert disoccluded.any() and (disoccluded & only(taps, "depth_ok")).any() and not has[disoccluded & only(taps, "depth_ok")].any()
        assert ((accepted >= 1) & (accepted <= 3)).any()
        assert (aware["N"] >= 4).any() and (has & (aware["N"] < 4)).any()
        assert (~valid).sum() == 2 and not has[~covered].any()
        assert (aware["N"][valid & ~has] == 1).all() and not aware["history"][:, ~valid].any()
        assert np.isfinite(aware["film"]).all() and np.isfinite(aware["variance"]).all() and np.isfinite(aware["history"]).all()
        assert aware["film"].dtype == np.float32
        # the wall did not move: there the two accumulations are one
        wall = (s["inst"] == 0) & (s["prev_inst"] == 0)
        np.testing.assert_array_equal(bits(aware["film"][wall]), bits(plain["film"][wall]))
    # the planes themselves: the square's pixels point SHIFT to the left, at the square's depth; the wall's at themselves
    px = s["motion"][0, ..., 0] - (np.arange(W, dtype=np.float64) + 0.5)[None, :]
    pixel = 2.0 * mr.SQUARE_Z / float(tr.pack_camera(s["cur_camera"], W, H)["proj00"]) / W
    assert np.abs(px[mover] + mr.SHIFT / pixel).max() < 1e-3 and np.abs(px[s["inst"] == 0]).max() < 1e-4
    np.testing.assert_array_equal(s["motion"][1, ..., 3], (s["inst"] + 1).astype(F))
    np.testing.assert_array_equal(s["motion"][1, ..., :3][s["inst"] >= 0], np.broadcast_to(np.array([0, 0, -1], F), (int((s["inst"] >= 0).sum()), 3)))


def test_a_static_scene_is_the_plain_accumulation():
    """(b): the planes of a static scene, whose films resolve to the centre rays' depth exactly, give gbl_film_accumulate's bits."""
    for shape in ((37, 23), (9, 9), (5, 3), (1, 1)):
        s = mr.moving_sequence(shape[0], shape[1], 0.0)
        assert mr.moved_instances(s["cur_instances"], s["prev_instances"]) == []
        z = tr.prepare(s["film"], None, s["normal"], s["depth"])["z"]
        np.testing.assert_array_equal(bits(z), bits(np.where(s["inst"] >= 0, s["t"], F(0.0))))      # film depth == centre-ray depth, everywhere
        planes = mr.motion_planes(s["t"], s["inst"], s["cur_camera"], s["prev_camera"], s["cur_instances"], None, s["normal"])
        np.testing.assert_array_equal(bits(planes), bits(s["motion"]))
        for variance in (None, s["variance"]):
            for normal in (None, s["normal"]):
                plain = tr.accumulate(s["film"], s["depth"], s["cur_camera"], variance=variance, normal=normal, history=s["history"],
                                      prev_camera=s["prev_camera"], **s["params"])
                aware = mr.accumulate_motion(s["film"], s["depth"], planes, variance=variance, normal=normal, history=s["history"], **s["params"])
                for k in ("film", "variance", "history"):
                    np.testing.assert_array_equal(bits(aware[k]), bits(plain[k]), err_msg="%s %s" % (shape, k))
                np.testing.assert_array_equal(aware["has_history"], plain["has_history"])
        if shape == (37, 23):
            assert plain["has_history"].sum() > 300
