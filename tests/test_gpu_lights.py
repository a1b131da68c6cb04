"""gbl_update_lights, gbl_get_lights and gbl_selftest_lights on the device.

The bar is the project's usual one and every tolerance is zero.  `check_edit` builds a tracer, edits it, and builds a second
tracer from the edited description (a second load of the scene whose gbl_light records -- and, for a moved area light, the
transforms of the instances that emit through it -- are overwritten with the edited values).  It compares
(a) gbl_selftest_lights' three tables, and for area-light moves gbl_selftest_instances' records, bounds, tlas_root and
    stack_entries, byte for byte;
(b) render(want_li=True): the per-sample radiance bit for bit, and the film (see below);
(c) the edited frame against the frame before the edit, which must differ, so (b) is not vacuous;
and the inverse edit must put the first frame and the first tables back.

The film of two renders.  gbl_render's film goes through wf_splat, whose waves add into the LDS tile and whose tiles add into the
film with float atomics in the order the hardware schedules them: two renders of ONE context differ in the film's last bits at
these frame sizes (tests/test_gpu_denoise.py measured 971 and 1104 of 3072 floats, relL2 7.4e-8 and 4.6e-8), so
byte identity of two films is not a property of any context, edited or fresh.  `same_frame` therefore asks what is one: the
per-sample radiance the film is the sum of, bit for bit, and the film within the suite's summation-order bound (FILM_RELL2_TOL
of tests/test_gpu_parity.py / test_gpu_temporal.py / test_gpu_aov.py).  Films ARE compared byte for byte in
test_films_where_the_splat_order_is_fixed, on the frame whose splat order is fixed (28 x 4 at 1 spp: one row of tiles, one wave
per tile), after two renders of one context have been seen to agree there.  (c) is asked of the radiance, which no summation
order can move.

One thing the byte comparison of a move knows (tests/test_gpu_refit.py `settled`): a host-built context
numbers the hot prefix -- the copies of the tree's top nodes that the lean kernels keep in LDS -- breadth first from its FIRST
TLAS, and the prefix stays as gbl_create made it when a TLAS is rebuilt (gbl_update_instances' limit, which a moved lamp shares).
A fresh context of the moved scene numbers its prefix from another TLAS, so the `root` word of a mesh instance's record (an index
into the prefix) and tlas_root are the two things its bytes may differ in; a host-built pair is compared on the records without
that word, the bounds and stack_entries.  A context with device-built BLASes has no prefix and is compared on every byte,
tlas_root included.

Frames are 16 x 16 or 24 x 16 at 1-4 spp, depth 2-3, SEED 20261020; the stream-order test renders 64 x 64 at 16 spp first.

Measured on an MI355X: the 49 tests take 4.6 s, the slowest 0.28 s (1.6 s more for the first one's imports); scaling a light's
colour by 4 in the two-light box moves the pick probabilities from the oracle's powers to [0.8 0.2] and [0.2 0.8], exactly.
"""
import ctypes as C
import math

import numpy as np
import pytest

import helpers
import oracle_binding as ob
import test_gpu_last_ray as lr
from test_gpu_last_ray import scene_dir, torch   # noqa: F401  (module fixtures)
from goblin_amd import _abi
from goblin_amd import scene as gs

pytestmark = pytest.mark.gpu
SEED = 20261020
INVALID, UNSUPPORTED, OK = _abi.GBL_ERR_INVALID, _abi.GBL_ERR_UNSUPPORTED, _abi.GBL_OK
POINT, DIRECTIONAL, SPOT, AREA, IBL = _abi.GBL_LIGHT_POINT, _abi.GBL_LIGHT_DIRECTIONAL, _abi.GBL_LIGHT_SPOT, _abi.GBL_LIGHT_AREA, _abi.GBL_LIGHT_IBL
F32 = np.float32
FILM_RELL2_TOL = 2.5e-5     # two renders of one frame: the film's float summation order (tests/test_gpu_parity.py)
_SCENES = {}


def pair(name, resolution=(16, 16), spp=2, depth=3, method=None):
    """Two loads of a shipped scene: the first is never written to, the second is `write_desc`'s to edit (and is restored from
    the first each time it is asked for)."""
    key = (name, resolution, spp, depth, method)
    if key not in _SCENES:
        o = gs.config_overrides(resolution=resolution, spp=spp, depth=depth, method=method)
        _SCENES[key] = (gs.load_scene(name, o), gs.load_scene(name, o))
    a, b = _SCENES[key]
    restore(a, b)
    return a, b


def restore(a, b):
    C.memmove(b.desc.lights, a.desc.lights, a.desc.num_lights * C.sizeof(_abi.gbl_light))
    C.memmove(b.desc.instances, a.desc.instances, a.desc.num_instances * C.sizeof(_abi.gbl_instance))


def records(scene):
    """Copies of the description's gbl_light records."""
    return [_abi.gbl_light.from_buffer_copy(scene.desc.lights[i]) for i in range(scene.desc.num_lights)]


def raw(rec):
    return bytes(rec) if not isinstance(rec, (list, tuple)) else b"".join(bytes(r) for r in rec)


def find(scene, kind, nth=0):
    return [i for i in range(scene.desc.num_lights) if scene.desc.lights[i].type == kind][nth]


def carriers(scene, light):
    return [i for i in range(scene.desc.num_instances) if scene.desc.instances[i].area_light == light]


def write_desc(scene, lights):
    """The edited description: the lights replaced, and every instance that emits through an area light given the light's
    transform where it had the light's old one (the loader writes the two bit for bit the same)."""
    d = scene.desc
    for i, rec in enumerate(lights):
        for k in carriers(scene, i):
            if raw(d.instances[k].to_world) == raw(d.lights[i].to_world):
                d.instances[k].to_world = rec.to_world
        d.lights[i] = rec


def tracer(scene, bvh="host"):
    from goblin_amd.renderer import HipPathTracer
    return HipPathTracer(scene, 0, bvh=bvh)


def light_bytes(r):
    t = r._lights_raw()
    assert t["total"] == r.scene.desc.num_lights == len(t["records"]) and len(t["cdf"]) == t["total"] + 1
    return t["records"].tobytes(), t["cdf"].tobytes(), t["pick_pdf"].tobytes()


def instance_bytes(r):
    t = r._instances_raw()
    return t["records"].tobytes(), t["bounds"].tobytes(), t["tlas_root"], t["stack_entries"]


def info_of(r):
    return [getattr(r.info, f) for f, _ in _abi.gbl_info._fields_ if f not in ("build_ms", "window")]


def shot(r, **kw):
    out = r.render(seed=SEED, want_li=True, **kw)
    film, li = out["film"].numpy(), out["li"].cpu().numpy()
    assert np.isfinite(film).all() and np.isfinite(li).all()
    return film, li.tobytes()


def same_frame(x, y, what=None):
    """Two `shot`s of one frame: the per-sample radiance bit for bit, the film up to its summation order (the module's text)."""
    assert x[1] == y[1], ("per-sample radiance differs", what)
    rel = helpers.rel_l2(x[0], y[0])
    assert rel <= FILM_RELL2_TOL, ("film relL2 %.3g" % rel, what)
    return True


def moved_instance_bytes(r, bvh):
    """What a moved lamp's context is compared on (the module's text): every byte with device-built BLASes; without the records'
    `root` word and tlas_root in a host-built context."""
    t = r._instances_raw()
    records = t["records"].copy()
    if bvh == "host":
        records["root"] = 0
    return records.tobytes(), t["bounds"].tobytes(), t["tlas_root"] if bvh == "device" else None, t["stack_entries"]


def set_fields(rec, **fields):
    for name, value in fields.items():
        if name == "to_world":
            for part, values in zip(("position", "orientation", "scale"), value):
                getattr(rec.to_world, part)[:] = [float(v) for v in values]
        elif isinstance(getattr(rec, name), C.Array):
            getattr(rec, name)[:] = [float(v) for v in value]
        else:
            setattr(rec, name, value)
    return rec


def check_edit(scenes, edits, bvh="host", moves=False, **kw):
    """edits: {light index: {field: value}} over one contiguous range.  Returns (edited tracer, fresh tracer of the edited
    description, the edited records); the second scene of the pair holds the edited description until the pair is asked for again."""
    sa, sb = scenes
    first, count = min(edits), max(edits) - min(edits) + 1
    a = tracer(sa, bvh)
    tables0, film0, inst0 = light_bytes(a), shot(a, **kw), instance_bytes(a)
    before, edited = records(sa), records(sa)
    for i, fields in edits.items():
        set_fields(edited[i], **fields)
    a.update_lights(first, edited[first:first + count])
    write_desc(sb, edited)
    b = tracer(sb, bvh)
    film_a, film_b = shot(a, **kw), shot(b, **kw)
    for k, name in enumerate(("DevLight records", "light_cdf", "light_pick_pdf")):
        assert light_bytes(a)[k] == light_bytes(b)[k], (name, edits)
    same_frame(film_a, film_b, ("the fresh context's", edits))
    assert film_a[1] != film0[1] and helpers.rel_l2(film_a[0], film0[0]) > FILM_RELL2_TOL, ("the edit left the frame alone", edits)
    assert raw(a.lights()) == raw(edited)
    if moves:
        for k, name in enumerate(("DevInstance records", "DevInstanceBound records", "tlas_root", "stack_entries")):
            assert moved_instance_bytes(a, bvh)[k] == moved_instance_bytes(b, bvh)[k], (name, edits)
        assert instance_bytes(a)[0] != inst0[0] and instance_bytes(a)[1] != inst0[1]
        assert info_of(a) == info_of(b) and a.instances() == b.instances()
    else:
        assert instance_bytes(a) == inst0
    # the inverse edit
    a.update_lights(first, before[first:first + count])
    assert light_bytes(a) == tables0 and same_frame(shot(a, **kw), film0, ("the inverse edit", edits))
    if moves:
        assert instance_bytes(a)[:2] == inst0[:2] and instance_bytes(a)[3] == inst0[3]
    a.update_lights(first, edited[first:first + count])   # ... and forth again, for the caller
    same_frame(shot(a, **kw), film_a, ("the edit made again", edits))
    return a, b, edited


def scaled(v, k):
    return [float(F32(x) * F32(k)) for x in v]


def moved(v, d):
    return [float(F32(x) + F32(y)) for x, y in zip(v, d)]


# ---------------------------------------------------------------------------
# 3: each editable field of each light type
# ---------------------------------------------------------------------------
def field_edits(scene, kind, field, nth=0):
    i = find(scene, kind, nth)
    l = scene.desc.lights[i]
    value = {"color": lambda: scaled(l.color, 2.5), "position": lambda: moved(l.position, (0.75, -0.5, 1.25)),
             "direction": lambda: moved(l.direction, (0.35, 0.1, -0.25)), "cos_theta_max": lambda: float(F32(l.cos_theta_max) * F32(0.9)),
             "cos_falloff_start": lambda: float(F32(0.5) * (F32(l.cos_falloff_start) + F32(l.cos_theta_max))),
             "orientation": lambda: (tuple(l.to_world.position), (0.9238795, 0.0, 0.3826834, 0.0), tuple(l.to_world.scale))}[field]()
    return {i: {("to_world" if field == "orientation" else field): value}}


FIELDS = [("grid", SPOT, "color", 0), ("grid", SPOT, "position", 0), ("grid", SPOT, "direction", 0), ("grid", SPOT, "cos_theta_max", 0),
          ("grid", SPOT, "cos_falloff_start", 0), ("grid", POINT, "color", 0), ("grid", POINT, "position", 0),
          ("cornell", AREA, "color", 0),
          ("volume", AREA, "color", 0), ("volume", AREA, "color", 1), ("volume", SPOT, "color", 0), ("volume", SPOT, "direction", 0),
          ("volume", SPOT, "position", 0),
          ("ibl", IBL, "orientation", 0), ("ibl", POINT, "color", 0), ("ibl", POINT, "position", 0),
          ("shapes", DIRECTIONAL, "color", 0), ("shapes", DIRECTIONAL, "direction", 0), ("shapes", AREA, "color", 0), ("shapes", AREA, "color", 1)]


@pytest.mark.parametrize("name,kind,field,nth", FIELDS, ids=["%s-%d.%d-%s" % (n, k, i, f) for n, k, f, i in FIELDS])
def test_each_field_under_the_megakernel(torch, name, kind, field, nth):
    scenes = pair(name)
    check_edit(scenes, field_edits(scenes[0], kind, field, nth), schedule="megakernel")


@pytest.mark.parametrize("name,kind,field", [("grid", SPOT, "direction"), ("grid", POINT, "color"), ("cornell", AREA, "color")])
def test_fields_under_the_tie_rule(torch, name, kind, field):
    scenes = pair(name)
    check_edit(scenes, field_edits(scenes[0], kind, field), schedule="megakernel", exact_ties=True)


@pytest.mark.parametrize("bvh", ("host", "device"))
def test_cornell_under_the_wavefront_schedule(torch, bvh):
    scenes = pair("cornell", resolution=(24, 16))
    check_edit(scenes, field_edits(scenes[0], AREA, "color"), bvh=bvh, schedule="wavefront")


@pytest.mark.parametrize("kind,field", [(SPOT, "direction"), (POINT, "color")])
def test_grid_under_the_stream_sampler(torch, kind, field):
    scenes = pair("grid", spp=4)
    check_edit(scenes, field_edits(scenes[0], kind, field), sampler="stream")


@pytest.mark.parametrize("name,kind,field,nth", [("grid", SPOT, "cos_theta_max", 0), ("volume", AREA, "color", 1), ("ibl", IBL, "orientation", 0)])
def test_whitted(torch, name, kind, field, nth):
    scenes = pair(name, method="whitted")
    assert scenes[0].desc.setting.integrator == _abi.GBL_INTEGRATOR_WHITTED
    check_edit(scenes, field_edits(scenes[0], kind, field, nth))


def test_both_lights_of_grid_in_one_call(torch):
    scenes = pair("grid")
    edits = dict(field_edits(scenes[0], SPOT, "direction"))
    edits.update(field_edits(scenes[0], POINT, "color"))
    assert sorted(edits) == [0, 1]
    check_edit(scenes, edits, schedule="megakernel")


@pytest.mark.parametrize("name", ("grid", "cornell"))
def test_films_where_the_splat_order_is_fixed(torch, name):
    """28 x 4 at 1 spp (a 32 x 8 sample window: four tiles in a row, one wave per tile; tests/test_gpu_denoise.py): two renders of
    one context write the same film bytes there, so the edited context's film can be held to the fresh one's byte for byte --
    after a colour edit on grid, after the lamp's move on cornell -- and so can the film the inverse edit puts back."""
    sa, sb = pair(name, resolution=(28, 4), spp=1, depth=3)
    a = tracer(sa)
    film0, again = shot(a, schedule="megakernel"), shot(a, schedule="megakernel")
    assert film0[0].tobytes() == again[0].tobytes() and film0[1] == again[1], "two renders of one context differ: the frame's splat order is not fixed"
    edited = records(sa)
    if name == "grid":
        set_fields(edited[0], color=scaled(edited[0].color, 3.0))
    else:
        old = edited[0].to_world
        set_fields(edited[0], to_world=((0.4, 1.7, 0.2), tuple(old.orientation), (0.45, 0.3, 0.25)))
    a.update_lights(0, [edited[0]])
    write_desc(sb, edited)
    got, want = shot(a, schedule="megakernel"), shot(tracer(sb), schedule="megakernel")
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
    assert got[0].tobytes() != film0[0].tobytes() and got[1] != film0[1]
    a.update_lights(0, [records(sa)[0]])
    back = shot(a, schedule="megakernel")
    assert back[0].tobytes() == film0[0].tobytes() and back[1] == film0[1]


# ---------------------------------------------------------------------------
# 4: pick probabilities
# ---------------------------------------------------------------------------
def pick_pdf_of(power):
    """pack_light_distribution's floats over the given powers (CDF1D::init, then (power / integral) * dx)."""
    power = np.asarray(power, F32)
    n = len(power)
    dx = F32(1.0) / F32(n)
    cdf = F32(0.0)
    for p in power:
        cdf = F32(cdf + F32(p * dx))
    return np.array([F32(F32(p / cdf) * dx) for p in power], F32)


def test_pick_probabilities_follow_the_oracles_powers(torch, scene_dir):
    import json
    doc = lr._doc("box-mixed", (16, 16), 1)
    sa, sb = (gs.load_scene_text(json.dumps(doc), scene_dir) for _ in range(2))
    a = tracer(sa)
    kinds = [sa.desc.lights[i].type for i in range(2)]
    assert sorted(kinds) == [POINT, AREA]
    assert np.array_equal(a._lights_raw()["pick_pdf"], pick_pdf_of(ob.Oracle(sa).light_power()[:, 3]))
    for light in (kinds.index(POINT), kinds.index(AREA)):
        edited = records(sa)
        set_fields(edited[light], color=scaled(edited[light].color, 4.0))
        a.update_lights(light, [edited[light]])
        restore(sa, sb)
        write_desc(sb, edited)
        want = pick_pdf_of(ob.Oracle(sb).light_power()[:, 3])
        got = a._lights_raw()["pick_pdf"]
        print("light", light, "x 4: pick_pdf", got, "from the oracle's powers", want)
        assert np.array_equal(got, want) and got[light] > 0.5
        a.update_lights(light, [records(sa)[light]])


# ---------------------------------------------------------------------------
# 5: moving Cornell's lamp
# ---------------------------------------------------------------------------
LAMP_MOVES = {"translate": ((0.5, 1.68, 0.3), None, None), "scale": (None, None, (0.5, 0.3, 0.2)), "both": ((-0.4, 1.7, 0.35), None, (0.2, 0.45, 0.3))}


@pytest.mark.parametrize("bvh", ("host", "device"))
@pytest.mark.parametrize("how", list(LAMP_MOVES))
def test_moving_cornells_lamp(torch, how, bvh):
    scenes = pair("cornell", resolution=(24, 16))
    sa = scenes[0]
    lamp, = carriers(sa, 0)
    old = sa.desc.lights[0].to_world
    new = tuple(tuple(given) if given is not None else tuple(have) for given, have in zip(LAMP_MOVES[how], (old.position, old.orientation, old.scale)))
    a, b, edited = check_edit(scenes, {0: {"to_world": new}}, bvh=bvh, moves=True, schedule="megakernel")
    as_f32 = tuple(tuple(float(F32(x)) for x in part) for part in new)
    assert a.instances()[lamp] == as_f32
    # a ray straight up at the lamp's new centre meets the lamp; one at its old centre does not (the ceiling is behind it)
    rays = np.array([[new[0][0], 1.3, new[0][2], 1e-3, 0, 1, 0, np.inf], [old.position[0], 1.3, old.position[2], 1e-3, 0, 1, 0, np.inf]], F32)
    hits = a.trace(torch.from_numpy(rays).to(a.device), exact_ties=True)
    inst, t = hits["instance"].cpu().numpy(), hits["t"].cpu().numpy()
    assert inst[0] == lamp and abs(float(t[0]) - (new[0][1] - 1.3)) < 1e-4
    if how != "scale":
        assert inst[1] >= 0 and inst[1] != lamp
    assert torch.equal(hits["records"], b.trace(torch.from_numpy(rays).to(b.device), exact_ties=True)["records"])
    aov_a, aov_b = a.render_aov(seed=SEED, want_samples=True), b.render_aov(seed=SEED, want_samples=True)
    assert torch.equal(aov_a["samples_i32"], aov_b["samples_i32"])   # the first-hit records, bit for bit; their films up to the summation order
    for plane in ("albedo", "normal", "depth"):
        assert helpers.rel_l2(aov_a[plane].numpy(), aov_b[plane].numpy()) <= FILM_RELL2_TOL, plane
    # the instance itself stays out of gbl_update_instances' reach, in today's words
    tables = light_bytes(a), instance_bytes(a)
    with pytest.raises(_abi.GoblinError) as e:
        a.update_instances(lamp, a.instances()[lamp:lamp + 1])
    assert e.value.status == UNSUPPORTED and "instance %d carries an area light, whose own transform would have to move with it" % lamp in str(e.value)
    assert (light_bytes(a), instance_bytes(a)) == tables


def test_a_moved_lamp_moves_again_and_back(torch):
    """Accepted edits keep the instance's transform the light's, so a second move is accepted too."""
    sa, sb = pair("cornell", resolution=(24, 16))
    a = tracer(sa)
    film0, inst0 = shot(a), instance_bytes(a)
    old = sa.desc.lights[0].to_world
    back = (tuple(old.position), tuple(old.orientation), tuple(old.scale))
    a.update_lights(0, to_world=((0.3, 1.5, 0.0), back[1], back[2]))
    a.update_lights(0, to_world=((0.3, 1.5, 0.0), back[1], (0.4, 0.2, 0.3)), color=(9.0, 9.0, 9.0))
    edited = records(sa)
    set_fields(edited[0], to_world=((0.3, 1.5, 0.0), back[1], (0.4, 0.2, 0.3)), color=(9.0, 9.0, 9.0))
    write_desc(sb, edited)
    b = tracer(sb)
    assert same_frame(shot(a), shot(b)) and light_bytes(a) == light_bytes(b)
    a.update_lights(0, to_world=back, color=tuple(sa.desc.lights[0].color))
    assert same_frame(shot(a), film0) and instance_bytes(a)[:2] == inst0[:2]


# ---------------------------------------------------------------------------
# 6: stream order
# ---------------------------------------------------------------------------
def test_uploads_keep_the_streams_order(torch):
    big, small = dict(resolution=(64, 64), spp=16, depth=3), dict(resolution=(64, 64), spp=1, depth=2)
    sa, sb = pair("grid", **big)
    point = find(sa, POINT)
    edited = records(sa)
    set_fields(edited[point], color=scaled(edited[point].color, 6.0))
    small_setting = type(sa.desc.setting).from_buffer_copy(sa.desc.setting)
    small_setting.sample_per_pixel, small_setting.max_ray_depth = small["spp"], small["depth"]
    a = tracer(sa)
    stream = torch.cuda.Stream(device=a.device)
    assert stream.cuda_stream != torch.cuda.default_stream(a.device).cuda_stream
    with torch.cuda.stream(stream):
        first = a.render(seed=SEED, want_li=True, schedule="megakernel")
        a.update_lights(point, [edited[point]], stream=stream)
        second = a.render(seed=SEED, want_li=True, schedule="megakernel", setting=small_setting)
    stream.synchronize()
    unedited = tracer(sa)
    fresh_before = unedited.render(seed=SEED, want_li=True, schedule="megakernel")
    small_before = unedited.render(seed=SEED, want_li=True, schedule="megakernel", setting=small_setting)
    write_desc(sb, edited)
    fresh_after = tracer(sb).render(seed=SEED, want_li=True, schedule="megakernel", setting=small_setting)
    torch.cuda.synchronize()
    for got, want, what in ((first, fresh_before, "queued before the edit"), (second, fresh_after, "queued after the edit")):
        assert torch.equal(got["li"], want["li"]), what
        assert helpers.rel_l2(got["film"].numpy(), want["film"].numpy()) <= FILM_RELL2_TOL, what
    assert not torch.equal(second["li"], small_before["li"])   # the second render saw another light


# ---------------------------------------------------------------------------
# 7: gbl_get_lights
# ---------------------------------------------------------------------------
def test_get_lights_round_trips(torch):
    sa, _ = pair("volume")
    a = tracer(sa)
    n = sa.desc.num_lights
    assert raw(a.lights()) == raw(records(sa)) and len(a.lights()) == n == 3
    edited = records(sa)
    set_fields(edited[1], color=(1.0, 2.0, 3.0), position=(0.5, 2.0, -1.0), direction=(0.0, -1.0, 0.25), cos_theta_max=0.75, cos_falloff_start=0.875)
    a.update_lights(1, [edited[1]])
    assert raw(a.lights()) == raw(edited)
    one = (_abi.gbl_light * 1)()
    for i in range(n):   # ranges
        assert a.lib.gbl_get_lights(a.handle, i, 1, one) == OK and raw(one[0]) == raw(edited[i])
    tables = light_bytes(a)
    assert a.lib.gbl_get_lights(a.handle, n, 0, one) == OK
    assert a.lib.gbl_update_lights(a.handle, n, 0, one, None) == OK and a.lib.gbl_update_lights(a.handle, 0, 0, one, None) == OK
    assert light_bytes(a) == tables and raw(a.lights()) == raw(edited)
    assert a.lib.gbl_get_lights(a.handle, n, 1, one) == INVALID and a.lib.gbl_get_lights(a.handle, 0, 1, None) == INVALID
    assert a.lib.gbl_get_lights(None, 0, 1, one) == INVALID


# ---------------------------------------------------------------------------
# 8: every refusal, in its order
# ---------------------------------------------------------------------------
class Refusals:
    """A tracer, its tables and its film; `refused` makes one call and checks that nothing moved."""

    def __init__(self, scene, bvh="host"):
        self.r, self.scene = tracer(scene, bvh), scene
        self.tables, self.inst, self.film, self.held = light_bytes(self.r), instance_bytes(self.r), shot(self.r), raw(self.r.lights())

    def refused(self, status, words, first, recs):
        arr = (_abi.gbl_light * max(1, len(recs)))(*recs)
        got = self.r.lib.gbl_update_lights(self.r.handle, first, len(recs), arr, None)
        text = self.r.lib.gbl_last_error(self.r.handle).decode()
        assert got == status, (got, text)
        for w in words:
            assert w in text, (w, text)
        assert light_bytes(self.r) == self.tables and instance_bytes(self.r) == self.inst and raw(self.r.lights()) == self.held, text
        same_frame(shot(self.r), self.film, text)


def test_refusals_arguments_range_and_fixed_fields(torch):
    sa, _ = pair("grid", spp=1, depth=2)
    x = Refusals(sa)
    recs = records(sa)
    spot, point = find(sa, SPOT), find(sa, POINT)
    lib, h = x.r.lib, x.r.handle
    assert lib.gbl_update_lights(None, 0, 1, (_abi.gbl_light * 1)(recs[0]), None) == INVALID
    assert lib.gbl_update_lights(h, 0, 1, None, None) == INVALID and "lights is NULL" in lib.gbl_last_error(h).decode()
    assert lib.gbl_update_lights(h, 5, 0, None, None) == INVALID and "lights is NULL" in lib.gbl_last_error(h).decode()   # arguments before the range
    x.refused(INVALID, ["light range out of bounds"], 1, recs)
    x.refused(INVALID, ["light range out of bounds"], 2, recs[:1])
    x.refused(INVALID, ["light range out of bounds"], 3, [])
    bad_type = set_fields(records(sa)[spot], type=POINT)
    x.refused(INVALID, ["light range out of bounds"], 2, [bad_type])                       # the range before the fields
    x.refused(INVALID, ["light %d" % spot, "type cannot change"], spot, [bad_type])
    x.refused(INVALID, ["light %d" % point, "type cannot change"], point, [set_fields(records(sa)[point], type=AREA)])
    x.refused(INVALID, ["light %d" % point, "type cannot change"], point, [set_fields(records(sa)[point], type=77)])
    x.refused(INVALID, ["light %d" % spot, "mesh cannot change"], spot, [set_fields(records(sa)[spot], mesh=1)])
    x.refused(INVALID, ["light %d" % spot, "sample_num cannot change"], spot, [set_fields(records(sa)[spot], sample_num=4)])
    x.refused(INVALID, ["light %d" % point, "image cannot change"], point, [set_fields(records(sa)[point], image=0)])
    # two faults: the field that cannot change is met before the value, in whichever light it sits
    nan = float("nan")
    x.refused(INVALID, ["light %d" % spot, "type cannot change"], spot, [set_fields(records(sa)[spot], type=POINT, color=(nan, 1.0, 1.0))])
    both = records(sa)
    set_fields(both[0], color=(nan, 1.0, 1.0))
    set_fields(both[1], sample_num=9)
    x.refused(INVALID, ["light 1", "sample_num cannot change"], 0, both)
    both = records(sa)
    set_fields(both[0], mesh=3, sample_num=9)
    x.refused(INVALID, ["light 0", "mesh cannot change"], 0, both)                         # ... and type, mesh, sample_num, image in that order


def test_refusals_values(torch):
    sa, _ = pair("grid", spp=1, depth=2)
    x = Refusals(sa)
    spot, point = find(sa, SPOT), find(sa, POINT)
    for bad in (float("nan"), float("inf"), -float("inf")):
        for field in ("color", "position", "direction"):
            for slot in range(3):
                v = list(getattr(sa.desc.lights[spot], field))
                v[slot] = bad
                x.refused(INVALID, ["light %d" % spot, field + " is not finite"], spot, [set_fields(records(sa)[spot], **{field: v})])
        for field in ("cos_theta_max", "cos_falloff_start"):
            x.refused(INVALID, ["light %d" % spot, field + " is not finite"], spot, [set_fields(records(sa)[spot], **{field: bad})])
        for field in ("color", "position"):
            x.refused(INVALID, ["light %d" % point, field + " is not finite"], point, [set_fields(records(sa)[point], **{field: (1.0, bad, 1.0)})])
    x.refused(INVALID, ["light %d" % spot, "direction has no length"], spot, [set_fields(records(sa)[spot], direction=(0.0, -0.0, 0.0))])
    # a field the light's type does not read is not looked at: a point light's direction may hold anything
    assert x.r.lib.gbl_update_lights(x.r.handle, point, 1, (_abi.gbl_light * 1)(set_fields(records(sa)[point], direction=(float("nan"), 0.0, 0.0))), None) == OK
    assert light_bytes(x.r) == x.tables and same_frame(shot(x.r), x.film)
    # a light without power is accepted, as gbl_create accepts it
    x.r.update_lights(point, color=(0.0, 0.0, 0.0))
    assert x.r._lights_raw()["pick_pdf"][point] == 0.0 and x.r._lights_raw()["pick_pdf"][spot] == 1.0


def test_refusals_directional_and_image_based(torch):
    sa, _ = pair("shapes", spp=1, depth=2)
    x = Refusals(sa)
    sun, a0 = find(sa, DIRECTIONAL), find(sa, AREA)
    x.refused(INVALID, ["light %d" % sun, "direction has no length"], sun, [set_fields(records(sa)[sun], direction=(0.0, 0.0, 0.0))])
    x.refused(INVALID, ["light %d" % sun, "direction is not finite"], sun, [set_fields(records(sa)[sun], direction=(0.0, float("inf"), 0.0))])
    # the area light's move, in a scene whose directional light is sized by the scene bound
    old = sa.desc.lights[a0].to_world
    there = ((old.position[0] + 0.5, old.position[1], old.position[2]), tuple(old.orientation), tuple(old.scale))
    assert carriers(sa, a0)
    x.refused(UNSUPPORTED, ["gbl_update_lights: a directional or image based light's power", "depends on the scene bound"], a0,
              [set_fields(records(sa)[a0], to_world=there)])
    x.refused(INVALID, ["light %d" % a0, "to_world is not finite"], a0,                    # values before the area light's rules
              [set_fields(records(sa)[a0], to_world=((float("nan"), 0.0, 0.0), there[1], there[2]))])
    si, _ = pair("ibl", spp=1, depth=2)
    y = Refusals(si)
    ibl = find(si, IBL)
    y.refused(UNSUPPORTED, ["light %d" % ibl, "baked into its texels"], ibl, [set_fields(records(si)[ibl], color=(2.0, 2.0, 2.0))])
    y.refused(INVALID, ["light %d" % ibl, "image cannot change"], ibl, [set_fields(records(si)[ibl], color=(2.0, 2.0, 2.0), image=-1)])
    y.refused(INVALID, ["light %d" % ibl, "to_world.orientation is not finite"], ibl,
              [set_fields(records(si)[ibl], to_world=((0.0, 0.0, 0.0), (1.0, float("nan"), 0.0, 0.0), (1.0, 1.0, 1.0)))])


@pytest.mark.parametrize("bvh", ("host", "device"))
def test_refusals_of_the_area_lights_move(torch, bvh):
    sa, sb = pair("cornell", spp=1, depth=2)
    lamp, = carriers(sa, 0)
    old = sa.desc.lights[0].to_world
    back = (tuple(old.position), tuple(old.orientation), tuple(old.scale))
    x = Refusals(sa, bvh)
    # a transform the reference cannot invert: build_tlas's refusal, before anything is written
    x.refused(INVALID, ["instance %d" % lamp], 0, [set_fields(records(sa)[0], to_world=(back[0], back[1], (0.0, 0.3, 0.3)))])
    x.refused(INVALID, ["light 0", "to_world is not finite"], 0, [set_fields(records(sa)[0], to_world=(back[0], back[1], (0.3, float("inf"), 0.3)))])
    # a hand-made description whose instance does not sit where its light does
    sb.desc.instances[lamp].to_world.position[1] = 1.9
    y = Refusals(sb, bvh)
    y.refused(UNSUPPORTED, ["light 0", "instance %d emits through this light from a transform of its own" % lamp], 0,
              [set_fields(records(sb)[0], to_world=((0.2, 1.7, 0.0), back[1], back[2]))])
    # ... which still takes every edit that moves nothing
    y.r.update_lights(0, color=(5.0, 5.0, 5.0))
    assert light_bytes(y.r) != y.tables and instance_bytes(y.r) == y.inst


# ---------------------------------------------------------------------------
# 9: the Python face
# ---------------------------------------------------------------------------
def test_the_python_face(torch):
    sa, _ = pair("grid", spp=1, depth=2)
    a, b = tracer(sa), tracer(sa)
    assert len(a.lights()) == sa.desc.num_lights == 2
    spot = find(sa, SPOT)
    a.update_lights(spot, color=(100.0, 200.0, 300.0), cos_theta_max=0.9)
    rec = set_fields(records(sa)[spot], color=(100.0, 200.0, 300.0), cos_theta_max=0.9)
    assert b.lib.gbl_update_lights(b.handle, spot, 1, (_abi.gbl_light * 1)(rec), None) == OK
    assert light_bytes(a) == light_bytes(b) and raw(a.lights()) == raw(b.lights()) and same_frame(shot(a), shot(b))
    before = light_bytes(a)
    with pytest.raises(TypeError):
        a.update_lights(spot, colour=(1.0, 1.0, 1.0))
    with pytest.raises(TypeError):
        a.update_lights(spot, color=(1.0, 1.0, 1.0), radiance=(1.0, 1.0, 1.0))
    assert light_bytes(a) == before
    with pytest.raises(_abi.GoblinError) as e:
        a.update_lights(spot, type=POINT)
    assert e.value.status == INVALID and "type cannot change" in str(e.value)
    a.update_lights(0)   # nothing named: nothing changes
    assert light_bytes(a) == before and math.isclose(a.lights()[spot].cos_theta_max, 0.9, rel_tol=1e-6)
