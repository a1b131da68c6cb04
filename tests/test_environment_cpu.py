"""gbl_update_environment_device / gbl_update_environment / gbl_selftest_environment without a GPU: the ABI (header, ctypes mirror,
exported names, the ABI version, which new entry points leave at 14), the Python face's refusals, which come before any library
call, and the shape of the cases tests/test_gpu_environment.py holds the device to (tests/environment_cases.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from goblin_amd import _abi
import environment_cases as ec
import image_edit_cases as ic
from test_image_edit_cpu import header, tracer_without_a_device

NAMES = ("gbl_update_environment_device", "gbl_update_environment", "gbl_selftest_environment")


@pytest.mark.parametrize("name", NAMES)
def test_declared_and_mirrored(name):
    assert re.search(r"\bgbl_status\s+%s\s*\(" % name, header())
    assert name in _abi.HIP_SYMBOLS


@pytest.mark.parametrize("name", NAMES)
def test_exported(name):
    """Fails without the feature."""
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libgoblin_hip.so"))
    assert getattr(lib, name) is not None


def test_the_signatures_take_what_the_mirror_passes():
    h = " ".join(header().split())
    assert "gbl_status gbl_update_environment_device(gbl_ctx* ctx, uint32_t light, const float* d_level0 , void* stream);" in h
    assert "gbl_status gbl_update_environment(gbl_ctx* ctx, uint32_t light, const float* level0 , void* stream);" in h
    assert "gbl_status gbl_selftest_environment(gbl_ctx* ctx, uint32_t light, float* dist_out , uint64_t* dist_floats, uint32_t dims_out[3] );" in h


def test_the_abi_version_stays_14():
    assert re.search(r"#define\s+GBL_ABI_VERSION\s+14\b", header())
    assert _abi.GBL_ABI_VERSION == 14
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libgoblin_hip.so"))
    lib.gbl_abi_version.restype = C.c_uint32
    assert lib.gbl_abi_version() == 14


def test_the_python_method_refuses_before_any_library_call():
    """Fails without the feature."""
    import torch
    sa, _ = ec.pair("16x16", "lamp_first")
    r = tracer_without_a_device(sa)
    lamp, sky = 0, 1
    assert ec.ibl_lights(sa) == [sky]
    for bad in (torch.zeros((16, 16, 4), dtype=torch.float64), torch.zeros((16, 16, 4), dtype=torch.float16),
                torch.zeros((16, 16, 4), dtype=torch.float32),                     # the right dtype and shape on another device
                torch.zeros((16, 16, 8), dtype=torch.float32)[:, :, ::2],           # not contiguous
                np.zeros((16, 16, 3), np.float32), np.zeros((16, 8, 4), np.float32), np.zeros((16, 16), np.float32), np.zeros(1024, np.float32),
                np.zeros((16, 16, 4), np.float64), np.zeros((16, 16, 4), np.int32), [[0.0] * 4] * 256, None):
        with pytest.raises(ValueError):
            r.update_environment(sky, bad)
    for light in (-1, lamp, sa.desc.num_lights):                                    # out of range, and a point light
        with pytest.raises(ValueError):
            r.update_environment(light, np.zeros((16, 16, 4), np.float32))
    # ... and what passes them reaches it
    with pytest.raises(AssertionError, match="the library was reached"):
        r.update_environment(sky, np.zeros((16, 16, 4), np.float32), stream=object())
    with pytest.raises(AssertionError, match="the library was reached"):
        r._environment_raw(sky)


@pytest.mark.parametrize("size", list(ec.SIZES))
def test_the_cases_have_the_shape_the_edits_assume(size):
    sa, sb = ec.pair(size)
    assert sa.desc.num_images == sb.desc.num_images == 1 and ec.ibl_lights(sa) == ec.ibl_lights(sb) == [1]
    a, b = sa.desc.images[0], sb.desc.images[0]
    assert bytes(a) == bytes(b) and (a.width, a.height, a.channels) == ec.LOADED[size] + (4,)
    assert a.levels == max(a.width, a.height).bit_length()
    la, lb = ec.environment_level0(sa, 1), ec.environment_level0(sb, 1)
    assert not np.array_equal(la, lb)
    for lv in (la, lb):                                # strictly positive and below the light's filter colour
        assert (lv[..., :3] > 0).all() and (lv[..., :3] <= 1).all()
    level = a.levels - 9 if a.levels > 9 else 0
    assert max(a.width >> level, a.height >> level) <= 256
    assert (level > 0) == (size in ("512x256", "1024x4", "4x1024"))


def test_the_variants():
    kinds = {v: [ec.pair("16x16", v)[0].desc.lights[i].type for i in range(ec.pair("16x16", v)[0].desc.num_lights)] for v in ec.VARIANTS}
    P, I = _abi.GBL_LIGHT_POINT, _abi.GBL_LIGHT_IBL
    assert kinds == {"lamp_first": [P, I], "whitted": [P, I], "ibl_first": [I, P], "only": [I], "two": [I, P, I]}
    two = ec.pair("16x16", "two")[0].desc
    assert two.num_images == 2 and two.lights[0].image != two.lights[2].image


def test_the_table_only_cases():
    _, wide = ec.pair(ec.WIDE_SIZE, "lamp_first", "wide")
    lv = ec.environment_level0(wide, 1)[..., :3]
    assert (lv < 0).any() and (lv > 0).any() and np.isfinite(ic.pyramid(wide, 0)).all()
    a, black = ec.pair(ec.BLACK_SIZE, "lamp_first", "blackrow")
    lb = ec.environment_level0(black, 1)[..., :3]
    assert not lb[ec.BLACK_ROW].any() and (np.delete(lb, ec.BLACK_ROW, axis=0) > 0).all() and (ec.environment_level0(a, 1)[..., :3] > 0).all()
