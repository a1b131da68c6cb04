"""gbl_update_environment_device, gbl_update_environment and gbl_selftest_environment on the device.  Every tolerance is zero.

The expected tables are a fresh context's (tests/environment_cases.py): scene A and scene B of a case are one document over two
directories whose env.exr differ.  A context made from A whose image based light was given B's level 0 must hold what a context
made from B holds -- the image's pyramid (gbl_get_image), the light's block of ibl_dist and its dims (gbl_selftest_environment),
the light records, light_cdf and light_pick_pdf (gbl_selftest_lights) -- bit for bit where the fresh value is not a NaN and a NaN
where it is one, and every per-sample radiance and first-hit record rendered afterwards must be the fresh context's bit for bit
(the film's float atomics have no fixed order, tests/test_gpu_lights.py).

1 tables per size and form; 2 the table-only cases; 3 interleaving with gbl_update_lights; 4 two image based lights; 5 renders
and the edit back; 6 the bundled scene; 7 stream order; 8 refusals, with the tables read back after each."""
import ctypes as C

import numpy as np
import pytest

import environment_cases as ec
from test_gpu_last_ray import torch   # noqa: F401  (module fixture)
from test_gpu_image_edit import bits, held, on_device, tracer
from test_gpu_lights import records, set_fields
from goblin_amd import _abi

pytestmark = pytest.mark.gpu
SEED = 20261021
INVALID, UNSUPPORTED, OK = _abi.GBL_ERR_INVALID, _abi.GBL_ERR_UNSUPPORTED, _abi.GBL_OK


def tables(r):
    """Everything an environment edit may write, read back: {name: float32 or uint8 array}."""
    d = r.scene.desc
    out = {"image %d" % i: held(r, i) for i in range(d.num_images)}
    for light in ec.ibl_lights(r.scene):
        raw = r._environment_raw(light)
        im = d.images[d.lights[light].image]
        level = im.levels - 9 if im.levels > 9 else 0
        assert (raw["level"], raw["dist_w"], raw["dist_h"]) == (level, max(1, im.width >> level), max(1, im.height >> level))
        assert raw["dist"].size == (2 * raw["dist_h"] + 2) + raw["dist_h"] * (2 * raw["dist_w"] + 2)
        out["ibl_dist of light %d" % light] = raw["dist"]
    t = r._lights_raw()
    assert t["total"] == d.num_lights
    out["records"] = np.frombuffer(t["records"].tobytes(), np.uint8)
    out["light_cdf"], out["light_pick_pdf"] = t["cdf"], t["pick_pdf"]
    return out


def same(got, want):
    """Bit for bit where `want` is not a NaN; a NaN where it is one."""
    if got.dtype == np.uint8:
        return np.array_equal(got, want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(bits(got)[~nan], bits(want)[~nan]) and np.isnan(got[nan]).all()


def assert_tables(got, want, what, names=None):
    for name in (names or want):
        g, w = got[name], want[name]
        if not same(g, w):
            wrong = np.flatnonzero(~((bits(g) == bits(w)) | (np.isnan(g) & np.isnan(w)))) if g.dtype != np.uint8 else np.flatnonzero(g != w)
            raise AssertionError("%s: %s differs in %d of %d, first at %d: device %r expected %r" % (what, name, wrong.size, w.size, wrong[0], g[wrong[0]], w[wrong[0]]))


def edit(torch, r, source, light, form="device", **kw):
    lv0 = ec.environment_level0(source, light)
    r.update_environment(light, on_device(torch, lv0) if form == "device" else np.array(lv0), **kw)


@pytest.fixture(scope="module")
def fresh():
    """Tables of fresh contexts, made once per scene and left unchanged."""
    cache = {}

    def of(scene):
        if id(scene) not in cache:
            cache[id(scene)] = tables(tracer(scene))
        return cache[id(scene)]
    return of


# ---------------------------------------------------------------------------
# 1: tables per size and form
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("size", list(ec.SIZES))
def test_tables_equal_a_fresh_context(torch, fresh, size, form):
    """Fails without the feature."""
    sa, sb = ec.pair(size)
    sky = ec.ibl_lights(sa)[0]
    r = tracer(sa)
    ta, tb = tables(r), fresh(sb)
    assert_tables(ta, fresh(sa), "as created")
    edit(torch, r, sb, sky, form)
    got = tables(r)
    assert_tables(got, tb, "after the edit (%s form)" % form)
    for name in ("image 0", "ibl_dist of light %d" % sky, "light_cdf", "light_pick_pdf"):
        assert not same(got[name], ta[name]), (name, "the edit changed nothing")
    assert same(got["records"], ta["records"])                   # DevLight itself does not change
    assert np.isfinite(got["ibl_dist of light %d" % sky]).all()


# ---------------------------------------------------------------------------
# 2: table-only cases
# ---------------------------------------------------------------------------
def test_sums_that_cancel(torch, fresh):
    sa, sb = ec.pair(ec.WIDE_SIZE, "lamp_first", "wide")
    tb = fresh(sb)
    dist = tb["ibl_dist of light 1"]
    assert np.isfinite(dist).all(), "the case's condition: fresh B's distribution is all finite"
    h, w = 128, 256
    integrals = dist[2 * h + 2:].reshape(h, 2 * w + 2)[:, -1]
    assert (integrals < 0).any() and (integrals > 0).any()
    for form in ("device", "host"):
        r = tracer(sa)
        edit(torch, r, sb, 1, form)
        assert_tables(tables(r), tb, "wide texels, %s form" % form)


def test_a_black_row(torch, fresh):
    sa, sb = ec.pair(ec.BLACK_SIZE, "lamp_first", "blackrow")
    tb = fresh(sb)
    rows = tb["ibl_dist of light 1"][2 * 16 + 2:].reshape(16, 2 * 16 + 2)
    assert np.isnan(rows[ec.BLACK_ROW, 17:33]).all() and rows[ec.BLACK_ROW, 16] == 0 and rows[ec.BLACK_ROW, 33] == 0   # cdf[1..] = 0 / 0
    assert np.isfinite(np.delete(rows, ec.BLACK_ROW, axis=0)).all() and np.isfinite(tb["ibl_dist of light 1"][:2 * 16 + 2]).all()
    r = tracer(sa)
    edit(torch, r, sb, 1)
    got = tables(r)
    assert_tables(got, tb, "a black row")
    assert np.array_equal(np.isnan(got["ibl_dist of light 1"]), np.isnan(tb["ibl_dist of light 1"]))
    edit(torch, r, sa, 1, "host")
    assert_tables(tables(r), fresh(sa), "back from a black row")


# ---------------------------------------------------------------------------
# 3: interleaving with gbl_update_lights
# ---------------------------------------------------------------------------
def light_edits(scene):
    """{light: record}: the point light's colour and the image based light's orientation changed."""
    recs = records(scene)
    out = {}
    for i, rec in enumerate(recs):
        if rec.type == _abi.GBL_LIGHT_POINT:
            out[i] = set_fields(rec, color=(3.0, 9.5, 4.25))
        elif rec.type == _abi.GBL_LIGHT_IBL and i == ec.ibl_lights(scene)[0]:
            q = (0.8660254, 0.0, 0.0, 0.5)
            out[i] = set_fields(rec, to_world=(rec.to_world.position[:], q, rec.to_world.scale[:]))
    return out


@pytest.mark.parametrize("order", ["environment_first", "lights_first", "environment_between"])
@pytest.mark.parametrize("variant", ["lamp_first", "ibl_first"])
def test_interleaved_with_light_edits(torch, variant, order):
    sa, sb = ec.pair("16x16", variant)
    sky = ec.ibl_lights(sa)[0]
    edits = light_edits(sa)
    assert len(edits) == 2
    b = tracer(sb)
    for i, rec in edits.items():
        b.update_lights(i, [rec])            # (gbl_update_lights on a fresh context is the parent's own path: tests/test_gpu_lights.py)
    want = tables(b)
    r = tracer(sa)
    steps = {"environment_first": ["env", "lights"], "lights_first": ["lights", "env"], "environment_between": ["light0", "env", "light1"]}[order]
    for step in steps:
        if step == "env":
            edit(torch, r, sb, sky)
        else:
            for k, (i, rec) in enumerate(sorted(edits.items())):
                if step == "lights" or step == "light%d" % k:
                    r.update_lights(i, [rec])
    assert_tables(tables(r), want, "%s, %s" % (variant, order))
    li_r, li_b = (x.render(seed=SEED, want_li=True)["li"].cpu().numpy().tobytes() for x in (r, b))
    assert li_r == li_b
    # ... and once more around: the host's powers followed the device's
    edit(torch, r, sa, sky, "host")
    for i in edits:
        r.update_lights(i, [records(sa)[i]])
    assert_tables(tables(r), tables(tracer(sa)), "%s, %s, back" % (variant, order))


# ---------------------------------------------------------------------------
# 4: two image based lights
# ---------------------------------------------------------------------------
def test_two_image_based_lights(torch, fresh):
    sa, sb = ec.pair("64x4", "two")
    first, second = ec.ibl_lights(sa)
    r = tracer(sa)
    ta, tb = tables(r), fresh(sb)
    edit(torch, r, sb, first)
    got = tables(r)
    im1, im2 = sa.desc.lights[first].image, sa.desc.lights[second].image
    assert_tables(got, tb, "the first light's", ["image %d" % im1, "ibl_dist of light %d" % first])
    assert_tables(got, ta, "the second light's, untouched", ["image %d" % im2, "ibl_dist of light %d" % second, "records"])
    assert not same(got["light_cdf"], ta["light_cdf"]) and not same(got["light_cdf"], tb["light_cdf"])
    edit(torch, r, sb, second, "host")
    assert_tables(tables(r), tb, "after both")
    r.update_lights(1, [set_fields(records(sa)[1], color=(1.0, 2.0, 3.0))])          # both powers settle on the host
    b = tracer(sb)
    b.update_lights(1, [set_fields(records(sb)[1], color=(1.0, 2.0, 3.0))])
    assert_tables(tables(r), tables(b), "after both and a light edit")


def test_the_only_light(torch, fresh):
    sa, sb = ec.pair("16x16", "only")
    r = tracer(sa)
    edit(torch, r, sb, 0)
    got = tables(r)
    assert_tables(got, fresh(sb), "the only light")
    assert got["light_cdf"].tolist() == [0.0, 1.0] and got["light_pick_pdf"].tolist() == [1.0]


# ---------------------------------------------------------------------------
# 5 and 6: renders after the edit, and the edit back
# ---------------------------------------------------------------------------
def shots(torch, r, whitted=False):
    """The per-sample radiance under each schedule and the first-hit records, as bytes."""
    out = {}
    for schedule in ((None,) if whitted else ("megakernel", "wavefront", "auto")):
        li = r.render(seed=SEED, want_li=True, **({"schedule": schedule} if schedule else {}))["li"]
        torch.cuda.synchronize()
        out[schedule or "whitted"] = li.cpu().numpy()
        assert np.isfinite(out[schedule or "whitted"]).all(), schedule
    rows = r.render_aov(albedo=False, normal=False, depth=False, want_samples=True, seed=SEED)["samples_i32"]
    torch.cuda.synchronize()
    out["aov"] = rows.cpu().numpy()
    return {k: v.tobytes() for k, v in out.items()}


def check_renders(torch, fresh, sa, sb, whitted=False, aov_changes=False):
    lights = ec.ibl_lights(sa)
    r = tracer(sa)
    before = shots(torch, r, whitted)
    fresh_b = shots(torch, tracer(sb), whitted)
    for light in lights:
        edit(torch, r, sb, light)
    after = shots(torch, r, whitted)
    for what in after:
        assert after[what] == fresh_b[what], (what, "after the edit")
        if what != "aov" or aov_changes:
            assert after[what] != before[what], (what, "the edit changed nothing that is seen")
    assert_tables(tables(r), fresh(sb), "after the edit")
    for light in lights:
        edit(torch, r, sa, light, "host")
    assert_tables(tables(r), fresh(sa), "after the edit back")
    assert shots(torch, r, whitted) == before


@pytest.mark.parametrize("variant", ["lamp_first", "only", "two", "whitted"])
def test_renders_equal_a_fresh_context(torch, fresh, variant):
    sa, sb = ec.pair("16x16", variant)
    check_renders(torch, fresh, sa, sb, whitted=variant == "whitted")


def test_renders_with_the_distribution_from_level_1(torch, fresh):
    sa, sb = ec.pair("512x256")
    check_renders(torch, fresh, sa, sb)


def test_the_bundled_scene(torch, fresh):
    sa, sb = ec.bundled_pair()
    assert sa.desc.num_images == sb.desc.num_images and bytes(sa.desc.images[0]) == bytes(sb.desc.images[0])
    check_renders(torch, fresh, sa, sb)


# ---------------------------------------------------------------------------
# 7: stream order
# ---------------------------------------------------------------------------
def test_edits_keep_the_streams_order(torch):
    sa, sb = ec.pair("16x16")
    long_setting = type(sa.desc.setting).from_buffer_copy(sa.desc.setting)
    long_setting.sample_per_pixel = 256                         # still running when the edit is queued behind it
    a = tracer(sa)
    level0 = on_device(torch, ec.environment_level0(sb, 1))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=a.device)
    assert stream.cuda_stream != torch.cuda.default_stream(a.device).cuda_stream
    with torch.cuda.stream(stream):
        first = a.render(seed=SEED, want_li=True, schedule="megakernel", setting=long_setting)
        a.update_environment(1, level0, stream=stream)
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
# 8: refusals
# ---------------------------------------------------------------------------
class Refusals:
    """A tracer and its tables; `refused` makes one call and checks status, message and that no table moved."""

    def __init__(self, scene):
        self.r = tracer(scene)
        self.tables = tables(self.r)

    def refused(self, form, status, words, light, pointer):
        lib, h = self.r.lib, self.r.handle
        got = (lib.gbl_update_environment_device if form == "device" else lib.gbl_update_environment)(h, light, pointer, None)
        text = lib.gbl_last_error(h).decode()
        assert got == status, (got, text)
        for w in words:
            assert w in text, (w, text)
        assert_tables(tables(self.r), self.tables, "after the refusal: " + text)


def test_refusals(torch):
    sa, sb = ec.pair("16x16")
    x = Refusals(sa)
    lib, h, n = x.r.lib, x.r.handle, sa.desc.num_lights
    lamp, sky = 0, 1
    good_h = np.array(ec.environment_level0(sb, sky))
    good = on_device(torch, good_h)
    torch.cuda.synchronize()
    # 1 and 2: NULL context or pointer
    assert lib.gbl_update_environment_device(None, sky, good.data_ptr(), None) == INVALID
    assert lib.gbl_update_environment(None, sky, good_h.ctypes.data, None) == INVALID
    x.refused("device", INVALID, ["gbl_update_environment_device", "d_level0 is NULL"], sky, None)
    x.refused("host", INVALID, ["gbl_update_environment:", "level0 is NULL"], sky, None)
    x.refused("device", INVALID, ["d_level0 is NULL"], n, None)                      # the pointer before the range
    x.refused("host", INVALID, ["level0 is NULL"], lamp, None)                       # ... and before the type
    # 3: the range
    for form, pointer in (("device", good.data_ptr()), ("host", good_h.ctypes.data)):
        x.refused(form, INVALID, ["light %d out of range" % n], n, pointer)
        x.refused(form, INVALID, ["out of range"], 0xFFFFFFFF, pointer)
    x.refused("device", INVALID, ["out of range"], n, good_h.ctypes.data)            # the range before the pointer
    # 4: the type
    for form, pointer in (("device", good.data_ptr()), ("host", good_h.ctypes.data)):
        x.refused(form, INVALID, ["light %d is a point light" % lamp, "not an image based one"], lamp, pointer)
    x.refused("device", INVALID, ["point light"], lamp, good_h.ctypes.data)          # the type before the pointer
    # 5: the device form's pointer
    x.refused("device", INVALID, ["d_level0 is not device memory"], sky, good_h.ctypes.data)   # refused before anything reads it
    with open("/proc/self/maps") as f:   # the HIP runtime this process already runs on, not a second copy of it
        hip = C.CDLL(next(line.split()[-1] for line in f if "libamdhip64" in line))
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(good_h.nbytes - 4)) == 0         # 4 bytes short of level 0; checked by the refusal, never read
    try:
        x.refused("device", INVALID, ["d_level0: its allocation ends"], sky, short.value)
    finally:
        assert hip.hipFree(short) == 0
    # the hook
    floats, dims = C.c_uint64(), (C.c_uint32 * 3)()
    assert lib.gbl_selftest_environment(None, sky, None, C.byref(floats), C.byref(dims)) == INVALID
    assert lib.gbl_selftest_environment(h, n, None, C.byref(floats), C.byref(dims)) == INVALID
    assert lib.gbl_selftest_environment(h, lamp, None, C.byref(floats), C.byref(dims)) == INVALID and floats.value == 0
    assert lib.gbl_selftest_environment(h, sky, None, C.byref(floats), C.byref(dims)) == OK and (floats.value, list(dims)) == (34 + 16 * 34, [0, 16, 16])
    assert lib.gbl_selftest_environment(h, sky, None, None, None) == OK
    # ... and what is not refused: the same call with the good pointer
    assert lib.gbl_update_environment_device(h, sky, good.data_ptr(), None) == OK
    assert_tables(tables(x.r), tables(tracer(sb)), "the accepted call")


def test_refusal_of_a_shared_image(torch):
    """6: two image based lights over one file share one image."""
    import json
    from goblin_amd import scene as gs
    d = ec.doc("two")
    d["lights"][2]["file"] = "env.exr"
    scene = gs.load_scene_text(json.dumps(d), ec.directory("16x16", "render", "A"))
    first, second = ec.ibl_lights(scene)
    assert scene.desc.lights[first].image == scene.desc.lights[second].image      # the loader caches by file and filter
    x = Refusals(scene)
    lv0 = np.array(ec.environment_level0(scene, first)) * np.float32(0.5)
    words = ["image %d" % scene.desc.lights[first].image, "also read by image based light"]
    x.refused("host", UNSUPPORTED, ["gbl_update_environment:", "light %d" % second] + words, first, lv0.ctypes.data)
    x.refused("device", UNSUPPORTED, ["gbl_update_environment_device:", "light %d" % first] + words, second, on_device(torch, lv0).data_ptr())
    x.refused("device", INVALID, ["not device memory"], first, lv0.ctypes.data)      # the pointer before the second reader
    with pytest.raises(_abi.GoblinError, match="also read by"):
        x.r.update_environment(first, lv0)


def test_the_image_edits_still_refuse_the_lights_image(torch):
    sa, sb = ec.pair("16x16")
    x = Refusals(sa)
    lv0 = np.array(ec.environment_level0(sb, 1))
    for form, pointer in (("host", lv0.ctypes.data), ("device", on_device(torch, lv0).data_ptr())):
        fn = x.r.lib.gbl_update_image_device if form == "device" else x.r.lib.gbl_update_image
        assert fn(x.r.handle, 0, pointer, None) == UNSUPPORTED
        assert "is read by image based light 1" in x.r.lib.gbl_last_error(x.r.handle).decode()
        assert_tables(tables(x.r), x.tables, "after gbl_update_image's refusal")
