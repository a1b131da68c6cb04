"""gbl_update_image_device, gbl_update_image and gbl_get_image on the device.  Every tolerance is zero.

The expected texels are the loader's (tests/image_edit_cases.py): scene A and scene B of a case are one document over two
directories of image files of the same sizes.  A context made from A whose image was given B's level 0 must hold B's pyramid for
that image -- B.desc.texels' slice, which csrc/host/mipmap.cpp built -- and A's for every other, bit for bit; with every image
edited, each render, AOV pass and stream-ordered pair of renders must equal a fresh context made from B bit for bit in the
per-sample values (the film's float atomics have no fixed order, tests/test_gpu_lights.py, so the per-sample radiance and the
first-hit records are what is compared).

1 pyramid bytes per size (colour and float, one to nine levels, a level of many workgroups, pyramids at odd float offsets);
2 the host form; 3 renders; 4 editing back; 5 stream order; 6 refusals, with the pool read back after each."""
import ctypes as C

import numpy as np
import pytest

import image_edit_cases as ic
from test_gpu_last_ray import torch   # noqa: F401  (module fixture)
from goblin_amd import _abi
from goblin_amd import scene as gs

pytestmark = pytest.mark.gpu
SEED = 20261021
INVALID, UNSUPPORTED, OK = _abi.GBL_ERR_INVALID, _abi.GBL_ERR_UNSUPPORTED, _abi.GBL_OK
RENDER_CASES = ["chart_16x16", "chart_5x3", "slots", "imagetex", "bumpy"]


def tracer(scene):
    from goblin_amd.renderer import HipPathTracer
    return HipPathTracer(scene, 0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def held(r, image):
    """The image's pyramid as the context holds it (gbl_get_image), flat; the record is checked against the scene's on the way."""
    record, levels = r.image(image)
    im = r.scene.desc.images[image]
    assert (record.width, record.height, record.levels, record.channels, record.texel_offset) == (im.width, im.height, im.levels, im.channels, 0)
    assert [l.shape for l in levels] == ic.level_shapes(im)
    return np.concatenate([l.ravel() for l in levels])


def assert_pool(r, expected, what):
    """Every image of the context against `expected` (a list of flat pyramids), bit for bit."""
    for i, want in enumerate(expected):
        got = held(r, i)
        wrong = np.flatnonzero(bits(got) != bits(want))
        assert wrong.size == 0, "%s: image %d differs in %d of %d floats, first at %d: device %r expected %r" % (
            what, i, wrong.size, want.size, wrong[0], got[wrong[0]], want[wrong[0]])


def pyramids(scene):
    return [ic.pyramid(scene, i) for i in range(scene.desc.num_images)]


def on_device(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).copy()).to("cuda:0")


def edit_all(torch, r, source, form="device"):
    for i in range(source.desc.num_images):
        r.update_image(i, on_device(torch, ic.level0(source, i)) if form == "device" else np.array(ic.level0(source, i)))


# ---------------------------------------------------------------------------
# 1: pyramid bytes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("image", range(len(ic.SIZE_IMAGES)), ids=["%s_%s" % c for c in ic.SIZE_IMAGES])
def test_pyramid_bytes(torch, image):
    sa, sb = ic.pair("sizes")
    r = tracer(sa)
    expected = pyramids(sa)
    assert_pool(r, expected, "as created")
    r.update_image(image, on_device(torch, ic.level0(sb, image)))
    expected[image] = ic.pyramid(sb, image)
    assert not np.array_equal(bits(expected[image]), bits(ic.pyramid(sa, image)))
    assert_pool(r, expected, "after the edit of image %d" % image)


def test_pyramid_bytes_in_the_slot_charts_pool(torch):
    """A 4-channel pyramid behind 1-channel ones, at a float offset that is no multiple of four; one context, image after image."""
    sa, sb = ic.pair("slots")
    d = sa.desc
    assert any(d.images[i].channels == 4 and d.images[i].texel_offset % 4 for i in range(d.num_images))
    r = tracer(sa)
    expected = pyramids(sa)
    for i in range(d.num_images):
        r.update_image(i, on_device(torch, ic.level0(sb, i)))
        expected[i] = ic.pyramid(sb, i)
        assert_pool(r, expected, "after the edit of image %d" % i)


def test_a_tensor_is_read_where_it_lies(torch):
    """A slice with a storage offset (no 16-byte alignment), and (h, w) for a float image."""
    sa, sb = ic.pair("sizes")
    r = tracer(sa)
    expected = pyramids(sa)
    for image in (ic.SIZE_IMAGES.index(("64x4", "color")), ic.SIZE_IMAGES.index(("4x64", "float"))):
        lv0 = ic.level0(sb, image)
        room = torch.zeros(lv0.size + 7, dtype=torch.float32, device="cuda:0")
        room[3:3 + lv0.size] = on_device(torch, lv0).reshape(-1)
        t = room[3:3 + lv0.size].view(lv0.shape if lv0.shape[2] == 4 else lv0.shape[:2])
        assert t.is_contiguous() and t.data_ptr() == room.data_ptr() + 12
        r.update_image(image, t)
        expected[image] = ic.pyramid(sb, image)
    assert_pool(r, expected, "after both edits")


# ---------------------------------------------------------------------------
# 2: the host form
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sizes", "slots"])
def test_the_host_form_leaves_the_device_forms_bytes(torch, case):
    sa, sb = ic.pair(case)
    dev, host = tracer(sa), tracer(sa)
    edit_all(torch, dev, sb, "device")
    edit_all(torch, host, sb, "host")
    assert_pool(dev, pyramids(sb), "device form")
    assert_pool(host, [held(dev, i) for i in range(sa.desc.num_images)], "host form against device form")


# ---------------------------------------------------------------------------
# 3 and 4: renders after the edit, and the edit back
# ---------------------------------------------------------------------------
def shots(torch, r):
    """The per-sample radiance under each schedule and the first-hit records, as bytes."""
    out = {}
    for schedule in ("megakernel", "wavefront", "auto"):
        li = r.render(seed=SEED, want_li=True, schedule=schedule)["li"]
        torch.cuda.synchronize()
        out[schedule] = li.cpu().numpy()
        assert np.isfinite(out[schedule]).all(), schedule
    rows = r.render_aov(albedo=False, normal=False, depth=False, want_samples=True, seed=SEED)["samples_i32"]
    torch.cuda.synchronize()
    out["aov"] = rows.cpu().numpy()
    return {k: v.tobytes() for k, v in out.items()}


@pytest.mark.parametrize("case", RENDER_CASES)
def test_renders_equal_a_fresh_context(torch, case):
    sa, sb = ic.pair(case)
    r = tracer(sa)
    before = shots(torch, r)
    fresh_a, fresh_b = shots(torch, tracer(sa)), shots(torch, tracer(sb))
    assert before == fresh_a
    edit_all(torch, r, sb)
    after = shots(torch, r)
    for what in after:
        assert after[what] == fresh_b[what], (case, what, "after the edit")
        assert after[what] != before[what], (case, what, "the edit changed nothing that is seen")
    assert_pool(r, pyramids(sb), "after the edit")
    edit_all(torch, r, sa)                                     # 4: back
    assert_pool(r, pyramids(sa), "after the edit back")
    assert shots(torch, r) == before


def test_editing_back_restores_the_sizes_pool(torch):
    sa, sb = ic.pair("sizes")
    r = tracer(sa)
    edit_all(torch, r, sb)
    assert_pool(r, pyramids(sb), "after the edit")
    edit_all(torch, r, sa, "host")
    assert_pool(r, pyramids(sa), "after the edit back")


# ---------------------------------------------------------------------------
# 5: stream order
# ---------------------------------------------------------------------------
def test_edits_keep_the_streams_order(torch):
    sa, sb = ic.pair("chart_16x16")
    long_setting = type(sa.desc.setting).from_buffer_copy(sa.desc.setting)
    long_setting.sample_per_pixel = 256                         # still running when the edit is queued behind it
    a = tracer(sa)
    level0s = [on_device(torch, ic.level0(sb, i)) for i in range(sb.desc.num_images)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=a.device)
    assert stream.cuda_stream != torch.cuda.default_stream(a.device).cuda_stream
    with torch.cuda.stream(stream):
        first = a.render(seed=SEED, want_li=True, schedule="megakernel", setting=long_setting)
        for i, t in enumerate(level0s):
            a.update_image(i, t, stream=stream)
        second = a.render(seed=SEED, want_li=True, schedule="megakernel")
    stream.synchronize()
    unedited = tracer(sa)
    fresh_before = unedited.render(seed=SEED, want_li=True, schedule="megakernel", setting=long_setting)
    short_before = unedited.render(seed=SEED, want_li=True, schedule="megakernel")
    fresh_after = tracer(sb).render(seed=SEED, want_li=True, schedule="megakernel")
    torch.cuda.synchronize()
    assert torch.equal(first["li"], fresh_before["li"]), "queued before the edit"
    assert torch.equal(second["li"], fresh_after["li"]), "queued after the edit"
    assert not torch.equal(second["li"], short_before["li"])


# ---------------------------------------------------------------------------
# 6: refusals
# ---------------------------------------------------------------------------
class Refusals:
    """A tracer and its pool; `refused` makes one call and checks status, message and that no texel moved."""

    def __init__(self, scene):
        self.r = tracer(scene)
        self.pool = [held(self.r, i) for i in range(scene.desc.num_images)]

    def refused(self, form, status, words, image, pointer):
        lib, h = self.r.lib, self.r.handle
        got = (lib.gbl_update_image_device if form == "device" else lib.gbl_update_image)(h, image, pointer, None)
        text = lib.gbl_last_error(h).decode()
        assert got == status, (got, text)
        for w in words:
            assert w in text, (w, text)
        assert_pool(self.r, self.pool, "after the refusal: " + text)


def test_refusals(torch):
    sa, sb = ic.pair("sizes")
    x = Refusals(sa)
    lib, h, n = x.r.lib, x.r.handle, sa.desc.num_images
    image = ic.SIZE_IMAGES.index(("16x16", "color"))
    good_h = np.array(ic.level0(sb, image))
    good = on_device(torch, good_h)
    torch.cuda.synchronize()
    # 1: NULL context or pointer
    assert lib.gbl_update_image_device(None, image, good.data_ptr(), None) == INVALID
    assert lib.gbl_update_image(None, image, good_h.ctypes.data, None) == INVALID
    x.refused("device", INVALID, ["gbl_update_image_device", "d_level0 is NULL"], image, None)
    x.refused("host", INVALID, ["gbl_update_image:", "level0 is NULL"], image, None)
    x.refused("device", INVALID, ["d_level0 is NULL"], n, None)                       # the arguments before the range
    # 2: the range
    for form, pointer in (("device", good.data_ptr()), ("host", good_h.ctypes.data)):
        x.refused(form, INVALID, ["image %d out of range" % n], n, pointer)
        x.refused(form, INVALID, ["out of range"], 0xFFFFFFFF, pointer)
    x.refused("device", INVALID, ["out of range"], n, good_h.ctypes.data)             # the range before the pointer
    # 3: the device form's pointer
    x.refused("device", INVALID, ["d_level0 is not device memory"], image, good_h.ctypes.data)   # refused before anything reads it
    with open("/proc/self/maps") as f:   # the HIP runtime this process already runs on, not a second copy of it
        hip = C.CDLL(next(line.split()[-1] for line in f if "libamdhip64" in line))
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(good_h.nbytes - 4)) == 0          # 4 bytes short of level 0; checked by the refusal, never read
    try:
        x.refused("device", INVALID, ["d_level0: its allocation ends"], image, short.value)
    finally:
        assert hip.hipFree(short) == 0
    # gbl_get_image
    record, out = _abi.gbl_image(), np.zeros(x.pool[image].size, np.float32)
    assert lib.gbl_get_image(None, image, C.byref(record), out.ctypes.data) == INVALID
    assert lib.gbl_get_image(h, n, C.byref(record), out.ctypes.data) == INVALID
    assert lib.gbl_get_image(h, image, None, None) == INVALID
    assert not out.any() and record.width == 0
    assert lib.gbl_get_image(h, image, C.byref(record), None) == OK and (record.width, record.height, record.levels, record.channels) == (16, 16, 5, 4)
    assert lib.gbl_get_image(h, image, None, out.ctypes.data) == OK and np.array_equal(bits(out), bits(x.pool[image]))
    # ... and what is not refused: the same call with the good pointer; an image nothing reads was accepted all along (test 1)
    assert lib.gbl_update_image_device(h, image, good.data_ptr(), None) == OK
    assert np.array_equal(bits(held(x.r, image)), bits(ic.pyramid(sb, image)))


def test_refusal_in_a_scene_without_images(torch):
    scene = gs.load_scene("grid", gs.config_overrides(resolution=(16, 16), spp=1, depth=2))
    assert scene.desc.num_images == 0
    r = tracer(scene)
    one = np.zeros(4, np.float32)
    dev = on_device(torch, one)
    assert r.lib.gbl_update_image(r.handle, 0, one.ctypes.data, None) == INVALID and "out of range" in r.lib.gbl_last_error(r.handle).decode()
    assert r.lib.gbl_update_image_device(r.handle, 0, dev.data_ptr(), None) == INVALID and "out of range" in r.lib.gbl_last_error(r.handle).decode()
    assert r.lib.gbl_get_image(r.handle, 0, C.byref(_abi.gbl_image()), None) == INVALID
    with pytest.raises(ValueError):
        r.update_image(0, one)


def test_refusal_of_an_image_based_lights_image(torch):
    scene = gs.load_scene("ibl", gs.config_overrides(resolution=(16, 16), spp=1, depth=2))
    d = scene.desc
    light = next(i for i in range(d.num_lights) if d.lights[i].type == _abi.GBL_LIGHT_IBL)
    image = d.lights[light].image
    x = Refusals(scene)
    li = x.r.render(seed=SEED, want_li=True)["li"].cpu().numpy().tobytes()
    lv0 = np.array(ic.level0(scene, image)) * np.float32(0.5)
    words = ["image %d" % image, "image based light %d" % light]
    x.refused("host", UNSUPPORTED, ["gbl_update_image:"] + words, image, lv0.ctypes.data)
    x.refused("device", UNSUPPORTED, ["gbl_update_image_device:"] + words, image, on_device(torch, lv0).data_ptr())
    x.refused("device", INVALID, ["not device memory"], image, lv0.ctypes.data)      # the pointer before the light
    with pytest.raises(_abi.GoblinError, match="image based light"):
        x.r.update_image(image, lv0)
    assert x.r.render(seed=SEED, want_li=True)["li"].cpu().numpy().tobytes() == li
