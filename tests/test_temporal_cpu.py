"""gbl_update_camera / gbl_film_accumulate without a GPU: the ABI (header, ctypes mirror, exported names) and the numpy
restatement the GPU tests compare against (tests/temporal_reference.py) -- that its fixture reaches every branch of the contract,
and that a still camera over a uniform history gives the running mean."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from goblin_amd import _abi
import temporal_reference as tr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_abi(tmp_path):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "goblin_hip.h")).read(), flags=re.S)
    for name in ("gbl_update_camera", "gbl_get_camera", "gbl_film_accumulate"):
        assert re.search(r"\bgbl_status\s+%s\s*\(" % name, header), name
        assert name in _abi.HIP_SYMBOLS
    fields = ["prev_camera", "alpha_min", "max_history", "sigma_depth", "cos_normal", "reserved", "stream"]
    src = tmp_path / "sizes.c"
    body = 'printf("size %zu\\n", sizeof(gbl_temporal_params));\nprintf("camera %zu\\n", sizeof(gbl_camera));\n'
    body += 'printf("floats %d\\n", GBL_HISTORY_FLOATS_PER_PIXEL);\nprintf("abi %d\\n", GBL_ABI_VERSION);\n'
    body += "".join('printf("%s %%zu\\n", offsetof(gbl_temporal_params, %s));\n' % (f, f) for f in fields)
    src.write_text('#include <stdio.h>\n#include "goblin_hip.h"\nint main(void){\n' + body + "return 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])   # plain C
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert C.sizeof(_abi.gbl_temporal_params) == int(out["size"])
    assert C.sizeof(_abi.gbl_camera) == int(out["camera"])
    for f in fields:
        assert getattr(_abi.gbl_temporal_params, f).offset == int(out[f]), f
    assert [f for f, _ in _abi.gbl_temporal_params._fields_] == fields
    assert [f for f, _ in _abi.gbl_camera._fields_] == list(tr.CAMERA_FIELDS)
    assert _abi.GBL_HISTORY_FLOATS_PER_PIXEL == int(out["floats"]) == 12
    assert _abi.GBL_ABI_VERSION == int(out["abi"]) == 14      # new entry points only: no existing layout changed


def test_symbols_resolve_in_the_built_library():
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libgoblin_hip.so"))
    for name in ("gbl_update_camera", "gbl_get_camera", "gbl_film_accumulate"):
        assert getattr(lib, name) is not None, name


def only(taps, reason):
    """Pixels without an accepted tap whose live taps inside the image all pass every test but ``reason``, and fail that one."""
    live = taps["live"]
    other = "normal_ok" if reason == "depth_ok" else "depth_ok"
    fails = live & ~taps[reason] & taps[other]
    clean = live & ~fails
    return fails.any(0) & ~clean.any(0)


def test_the_fixture_reaches_every_branch():
    s = tr.synthetic_sequence()
    for variance in (None, s["variance"]):
        out = tr.accumulate(s["film"], s["depth"], s["cur_camera"], variance=variance, normal=s["normal"], history=s["history"],
                            prev_camera=s["prev_camera"], **s["params"])
        taps, has, N = out["taps"], out["has_history"], out["N"]
        covered = out["valid"] & out["surf"]
        share = has.sum() / covered.sum()
        accepted = taps["accepted"].sum(0)
        outside = covered & ~taps["inside"].all(0)
        print("covered %d, with history %d (%.0f %%), depth-only rejections %d, normal-only %d, a tap outside the image %d, all four outside %d, "
              "1-3 taps accepted %d, N >= 4: %d, N < 4 with history: %d" %
              (covered.sum(), has.sum(), 100 * share, (covered & only(taps, "depth_ok")).sum(), (covered & only(taps, "normal_ok")).sum(),
               outside.sum(), (covered & ~taps["inside"].any(0)).sum(), ((accepted >= 1) & (accepted <= 3)).sum(), (N >= 4).sum(), (has & (N < 4)).sum()))
        assert (~out["valid"]).sum() == 2 and (out["valid"] & ~out["surf"]).sum() == 20
        assert 0.2 <= share <= 0.95
        assert (covered & only(taps, "depth_ok")).any()
        assert (covered & only(taps, "normal_ok")).any()
        assert (covered & ~taps["inside"].any(0)).any()
        assert ((accepted >= 1) & (accepted <= 3)).any()
        assert (N >= 4).any() and (has & (N < 4)).any()
        assert not has[~covered].any()
        assert (N[out["valid"] & ~has] == 1).all() and not out["history"][:, ~out["valid"]].any()
        assert (s["history"][0, ..., 3] == 0).sum() > 10 and s["history"][0, ..., 3].max() <= s["params"]["max_history"]
        assert np.isfinite(out["film"]).all() and np.isfinite(out["variance"]).all() and np.isfinite(out["history"]).all()
        assert out["film"].dtype == np.float32


def test_a_still_camera_gives_the_running_mean():
    """prev_camera = the current camera: a pixel centre reprojects onto itself to within rounding, so an interior covered pixel
    takes (nearly) all its weight from its own history.  Over a uniform history of length k, with alpha_min out of the way,
    N_out = min(k + 1, max_history) and c_out = c_prev + (c - c_prev) / (k + 1), the running mean: a handful of float32
    roundings, held to 1e-5 relative (a sanity bound on the contract, not a device tolerance)."""
    H, W = 23, 37
    rng = np.random.default_rng(11)
    cam = tr.camera(position=(0.3, -0.2, 0.1), orientation=(np.cos(0.05), 0.0, np.sin(0.05), 0.0), fov_degrees=50.0)
    colour = rng.uniform(0.2, 1.0, (H, W, 3)).astype(F)
    film = np.concatenate([colour, np.ones((H, W, 1), F)], -1)
    z = np.full((H, W), 6.0, F)
    depth = np.stack([z, np.ones((H, W), F), np.zeros((H, W), F), np.ones((H, W), F)], -1)
    mean = np.array([0.4, 0.5, 0.6], F)
    for k, max_history in ((1, 64.0), (5, 64.0), (20, 64.0), (20, 8.0)):
        history = np.zeros((3, H, W, 4), F)
        history[0, ..., :3], history[0, ..., 3] = mean, k
        history[1, ..., 3], history[2, ..., 3] = z, 1.0
        out = tr.accumulate(film, depth, cam, history=history, prev_camera=cam, alpha_min=1e-6, max_history=max_history, sigma_depth=0.05)
        inner = np.zeros((H, W), bool)
        inner[1:-1, 1:-1] = True
        assert out["has_history"][inner].all()
        n_out = min(k + 1, max_history)
        assert np.abs(out["N"][inner] - n_out).max() <= 1e-5 * n_out
        want = mean.astype(np.float64) + (colour.astype(np.float64) - mean) / n_out
        rel = np.abs(out["film"][..., :3][inner] - want[inner]).max() / want.max()
        print("k = %d, max_history %g: N_out %g, running mean to %.3g relative" % (k, max_history, n_out, rel))
        assert rel <= 1e-5
