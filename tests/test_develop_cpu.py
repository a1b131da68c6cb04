"""gbl_film_develop / gbl_host_write_ppm8 without a GPU: the ABI's new struct, the argument check that comes before any
device call, the byte writer, and the fixtures of tests/golden/make_develop_golden.py (tests/test_gpu_develop.py runs the
device path against them)."""
import ctypes as C
import os
import subprocess

import numpy as np

from goblin_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


def _fixture(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def test_develop_params_mirror_has_the_c_layout(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "goblin_hip.h"\nint main(void){\n'
                   'printf("%zu %zu %zu\\n", sizeof(gbl_develop_params), offsetof(gbl_develop_params, tone_mapping), '
                   'offsetof(gbl_develop_params, stream));\nreturn 0;}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])   # plain C
    size, off_tone, off_stream = (int(v) for v in subprocess.check_output([str(exe)]).decode().split())
    assert C.sizeof(_abi.gbl_develop_params) == size
    assert _abi.gbl_develop_params.tone_mapping.offset == off_tone
    assert _abi.gbl_develop_params.stream.offset == off_stream


def test_develop_rejects_null_arguments_before_the_device():
    lib = _abi.hip_lib()          # dlopen only
    p = _abi.gbl_develop_params()
    p.bloom_radius, p.bloom_weight, p.tone_mapping = 0.1, 0.3, 1
    buf = (C.c_float * 16)()
    assert lib.gbl_film_develop(None, buf, C.byref(p), buf, None) == _abi.GBL_ERR_INVALID
    assert lib.gbl_film_develop(None, None, None, None, None) == _abi.GBL_ERR_INVALID


def test_write_ppm8_writes_the_references_text(tmp_path):
    """The integers of the reference's own .ppm, handed back as bytes, come out as exactly that file."""
    lib = _abi.host_lib()
    for name in ("image_b", "develop_b"):
        fx = _fixture(name)
        h, w, _ = fx["input"].shape
        want = bytes(fx["ppm_bytes"])
        toks = want.split()
        assert toks[:4] == [b"P3", str(w).encode(), str(h).encode(), b"255"]
        vals = np.array(toks[4:], np.int32)
        assert vals.size == w * h * 3 and vals.min() >= 0 and vals.max() <= 255
        rgb8 = np.ascontiguousarray(vals.astype(np.uint8))
        out = tmp_path / (name + ".ppm")
        assert lib.gbl_host_write_ppm8(os.fsencode(str(out)), rgb8.ctypes.data_as(C.c_void_p), w, h) == _abi.GBL_OK
        assert out.read_bytes() == want
    assert lib.gbl_host_write_ppm8(None, None, 1, 1) == _abi.GBL_ERR_INVALID
    assert lib.gbl_host_write_ppm8(os.fsencode(str(tmp_path / "no" / "such" / "dir.ppm")), rgb8.ctypes.data_as(C.c_void_p), w, h) == _abi.GBL_ERR_IO


def test_develop_fixtures():
    want = {"develop_a": ((40, 96, 4), 24), "develop_b": ((45, 67, 4), 5), "develop_c": ((45, 67, 4), 5)}
    for name, (shape, fw) in want.items():
        fx = _fixture(name)
        assert fx["input"].shape == shape and fx["input"].dtype == np.float32
        for k in ("bloom", "tone", "bloom_tone"):
            assert fx[k].shape == shape and fx[k].dtype == np.float32 and np.isfinite(fx[k]).all()
        assert int(fx["fw"]) == fw
        h, w, _ = shape
        assert int(np.ceil(np.float32(fx["bloom_radius"]) * np.float32(max(w, h)))) // 2 == fw     # Goblin::bloom's filterWidth
        for k in ("ppm_bytes", "bloom_tone_ppm"):
            toks = bytes(fx[k]).split()
            assert toks[:4] == [b"P3", str(w).encode(), str(h).encode(), b"255"] and len(toks) == 4 + w * h * 3
    # develop_c spans eleven decades of luminance: what makes the order of the tone map's sum visible
    lum = _fixture("develop_c")["input"][..., :3] @ np.array([0.212671, 0.715160, 0.072169], np.float32)
    assert lum.min() < 1e-2 and lum.max() > 1e7
