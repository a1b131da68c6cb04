"""gbl_update_image_device / gbl_update_image / gbl_get_image without a GPU: the ABI (header, ctypes mirror, exported names, the ABI
version, which new entry points leave at 14), the Python face's refusals, which come before any library call, and the shared tap
helper: the pyramid builder (csrc/host/mipmap.cpp) and the image edits (csrc/api_images.hip) take resizeImage's taps from one
function, so the pyramids of tests/image_edit_cases.py -- what tests/test_gpu_image_edit.py holds the device to -- have the
shape the edits assume: back to back in the pool, level l of max(1, w >> l) x max(1, h >> l) texels, alpha 1 above level 0."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from goblin_amd import _abi
from goblin_amd import renderer
import image_edit_cases as ic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gbl_update_image_device", "gbl_update_image", "gbl_get_image")


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
    assert "gbl_status gbl_update_image_device(gbl_ctx* ctx, uint32_t image, const float* d_level0 , void* stream);" in h
    assert "gbl_status gbl_update_image(gbl_ctx* ctx, uint32_t image, const float* level0 , void* stream);" in h
    assert "gbl_status gbl_get_image(gbl_ctx* ctx, uint32_t image, gbl_image* info_out , float* texels_out );" in h


def test_the_abi_version_stays_14():
    assert re.search(r"#define\s+GBL_ABI_VERSION\s+14\b", header())
    assert _abi.GBL_ABI_VERSION == 14
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libgoblin_hip.so"))
    lib.gbl_abi_version.restype = C.c_uint32
    assert lib.gbl_abi_version() == 14


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
    sa, _ = ic.pair("sizes")
    r = tracer_without_a_device(sa)
    colour, flt = ic.SIZE_IMAGES.index(("16x16", "color")), ic.SIZE_IMAGES.index(("16x16", "float"))
    assert callable(r.update_image) and callable(r.image)
    for bad in (torch.zeros((16, 16, 4), dtype=torch.float64), torch.zeros((16, 16, 4), dtype=torch.float16),
                torch.zeros((16, 16, 4), dtype=torch.float32),                     # the right dtype and shape on another device
                torch.zeros((16, 16, 8), dtype=torch.float32)[:, :, ::2],           # not contiguous
                np.zeros((16, 16, 3), np.float32), np.zeros((16, 8, 4), np.float32), np.zeros((16, 16), np.float32), np.zeros(1024, np.float32),
                [[0.0] * 4] * 256, None):
        with pytest.raises(ValueError):
            r.update_image(colour, bad)
    for bad in (np.zeros((16, 16, 4), np.float32), np.zeros((16, 16, 2), np.float32), np.zeros((8, 16), np.float32)):
        with pytest.raises(ValueError):
            r.update_image(flt, bad)
    for image in (-1, sa.desc.num_images):
        with pytest.raises(ValueError):
            r.update_image(image, np.zeros((16, 16, 4), np.float32))
        with pytest.raises(ValueError):
            r.image(image)
    # ... and what passes them reaches it
    for image, ok in ((colour, np.zeros((16, 16, 4), np.float32)), (flt, np.zeros((16, 16), np.float32)), (flt, np.zeros((16, 16, 1), np.float32))):
        with pytest.raises(AssertionError, match="the library was reached"):
            r.update_image(image, ok, stream=object())


@pytest.mark.parametrize("case", ic.CASES)
def test_the_cases_pools_have_the_shape_the_edits_assume(case):
    sa, sb = ic.pair(case)
    assert sa.desc.num_images == sb.desc.num_images > 0 and sa.desc.num_texels == sb.desc.num_texels
    at = 0
    for i in range(sa.desc.num_images):
        a, b = sa.desc.images[i], sb.desc.images[i]
        assert bytes(a) == bytes(b) and a.texel_offset == at, (case, i)          # the same sizes at the same place, back to back
        assert a.levels == max(a.width, a.height).bit_length() and a.channels in (1, 4)
        at += len(ic.pyramid(sa, i))
        if a.channels == 4:
            assert (ic.pyramid(sb, i)[4 * a.width * a.height + 3::4] == 1.0).all()     # alpha above level 0
        assert not np.array_equal(ic.level0(sa, i), ic.level0(sb, i)), (case, i)       # B is another image
        assert np.isfinite(ic.pyramid(sa, i)).all() and np.isfinite(ic.pyramid(sb, i)).all()
    assert at == sa.desc.num_texels


def test_the_sizes_pool():
    sa, _ = ic.pair("sizes")
    d = sa.desc
    assert [(d.images[i].width, d.images[i].height, d.images[i].channels) for i in range(d.num_images)] == [
        ((8, 4) if name == "5x3" else ic.SIZES[name]) + ((4,) if kind == "color" else (1,)) for name, kind in ic.SIZE_IMAGES]
    odd = [i for i in range(d.num_images) if d.images[i].channels == 4 and d.images[i].texel_offset % 4]
    assert odd, "no 4-channel pyramid at a float offset that is no multiple of four"
    lv0 = ic.level0(sa, ic.SIZE_IMAGES.index((ic.BIG, "color")))[..., :3]
    assert (lv0 < 0).any() and (lv0 == 0).any() and np.abs(lv0).max() > 1e4 and np.abs(lv0[lv0 != 0]).min() < 1e-4
