"""The device-pointer vertex entries without a GPU: gbl_update_vertices_device, gbl_get_vertices_device, gbl_order_pending and
gbl_render_motion_deform_device are declared in the header, mirrored in goblin_amd/_abi.py and exported by the library; the ABI
version stays 14; a NULL context is GBL_ERR_INVALID from each (which touches no device).  All fail without the feature.  What
the entries do is tests/test_gpu_vertices_device.py's."""
import ctypes as C
import os
import re
import subprocess

import pytest

from goblin_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gbl_update_vertices_device", "gbl_get_vertices_device", "gbl_order_pending", "gbl_render_motion_deform_device")


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "goblin_hip.h")).read(), flags=re.S)


@pytest.mark.parametrize("name", NAMES)
def test_declared_mirrored_exported(name):
    assert re.search(r"\bgbl_status\s+%s\s*\(" % name, header())
    assert name in _abi.HIP_SYMBOLS
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libgoblin_hip.so"))
    assert getattr(lib, name) is not None


def test_flag_and_version(tmp_path):
    """The header's constants as a C compiler reads them, and the mirror's."""
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include "goblin_hip.h"\nint main(void){printf("%u %d\\n", GBL_VERTICES_DEFER_ORDER, GBL_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "consts"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])   # plain C
    flag, version = (int(x) for x in subprocess.check_output([str(exe)]).decode().split())
    assert flag == _abi.GBL_VERTICES_DEFER_ORDER == 1
    assert version == _abi.GBL_ABI_VERSION == 14


def test_a_null_context_is_invalid():
    lib = _abi.hip_lib()
    word = C.c_uint32(7)
    params = _abi.gbl_motion_params()
    listed = (_abi.gbl_motion_mesh * 1)()
    assert lib.gbl_update_vertices_device(None, 0, 0, 0, None, None, 0) == _abi.GBL_ERR_INVALID
    assert lib.gbl_get_vertices_device(None, 0, 0, 0, None) == _abi.GBL_ERR_INVALID
    assert lib.gbl_order_pending(None, 0, C.byref(word)) == _abi.GBL_ERR_INVALID and word.value == 7
    assert lib.gbl_render_motion_deform_device(None, C.byref(params), listed, 1, None) == _abi.GBL_ERR_INVALID
