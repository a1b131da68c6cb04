"""gbl_update_materials / gbl_update_textures, their device forms, gbl_get_* and gbl_selftest_materials on the device.

The expectation is always a fresh context, never the code under test: scene B is scene A's description with the edited values
(a second load of the scene whose gbl_material / gbl_texture records are overwritten).  `check_case` makes a context from A, edits
it to B and asks, with every tolerance zero:
 1. gbl_selftest_materials' two tables are B's byte for byte, and every other table read back (lights, light CDFs, instances,
    instance bounds, TLAS root, stack entries, nodes, triangles, gbl_info) holds A's bytes;
 2. render(want_li=True): the per-sample radiance equals the fresh context of B's bit for bit (the film within the suite's
    summation-order bound, as tests/test_gpu_lights.py explains);
 3. (test_aov_records_follow_the_edit) gbl_render_aov's per-sample records, albedo included, are B's;
 4. the per-sample radiance equals the oracle's on B's description (native sampler; LI_FLIP_TOL = 0 and relL2 = 0 of
    tests/test_gpu_parity.py);
 5. the radiance differs from A's -- a property of the cases (tests/material_edit_cases.py; tests/test_materials_cpu.py asks the
    oracle on the CPU);
 6. the inverse edit puts A's tables and frame back.
The cases are tests/material_edit_cases.py's, through the host forms and, where a row holds everything the case changes, from a
tensor through the device forms.  Frames are test_gpu_lights.py's pair() frame: 16 x 16, 2 spp, depth 3, SEED 20261020; the
stream-order test renders 64 x 64 at 16 spp first.
"""
import ctypes as C

import numpy as np
import pytest

import helpers
import material_edit_cases as mc
import oracle_binding as ob
from test_gpu_last_ray import scene_dir, torch   # noqa: F401  (module fixtures)
from test_gpu_lights import FILM_RELL2_TOL, info_of, instance_bytes, light_bytes, raw, same_frame, tracer
from goblin_amd import _abi
from goblin_amd import scene as gs

pytestmark = pytest.mark.gpu
SEED = mc.SEED
INVALID, UNSUPPORTED, OK = _abi.GBL_ERR_INVALID, _abi.GBL_ERR_UNSUPPORTED, _abi.GBL_OK
F32 = np.float32
_SCENES = {}
_ORACLE = {}


def pair(name, resolution=(16, 16), spp=2, depth=3, method=None):
    """Two loads of a shipped scene: the first is never written to, the second is `write_desc`'s to edit (and is restored from
    the first each time it is asked for)."""
    key = (name, resolution, spp, depth, method)
    if key not in _SCENES:
        o = gs.config_overrides(resolution=resolution, spp=spp, depth=depth, method=method)
        _SCENES[key] = (gs.load_scene(name, o), gs.load_scene(name, o))
    a, b = _SCENES[key]
    C.memmove(b.desc.materials, a.desc.materials, a.desc.num_materials * C.sizeof(_abi.gbl_material))
    if a.desc.num_textures:
        C.memmove(b.desc.textures, a.desc.textures, a.desc.num_textures * C.sizeof(_abi.gbl_texture))
    return a, b


def shot(r, **kw):
    out = r.render(seed=SEED, want_li=True, **kw)
    film, li = out["film"].numpy(), out["li"].cpu().numpy()
    assert np.isfinite(film).all() and np.isfinite(li).all()
    return film, li.tobytes()


def tables(r):
    t = r._materials_raw()
    assert len(t["materials"]) == r.scene.desc.num_materials and len(t["textures"]) == r.scene.desc.num_textures
    return t["materials"].tobytes(), t["textures"].tobytes()


def others(r):
    """Every other table the self-test hooks read back, and gbl_info."""
    return light_bytes(r), instance_bytes(r), r._geometry("nodes").tobytes(), r._geometry("tris").tobytes(), info_of(r)


def oracle_li(scene, key=None):
    """The oracle's per-sample radiance of a description at the tests' seed; A's is kept per scene."""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    oracle = ob.Oracle(scene)
    li = oracle.li_replay(oracle.native_samples(SEED), threads=4)[0]
    if key is not None:
        _ORACLE[key] = li
    return li


def equals_the_oracle(frame, li_ref, what):
    li = np.frombuffer(frame[1], F32).reshape(-1, 4)
    flips, rel = helpers.li_mismatch_fraction(li, li_ref), helpers.rel_l2(li[:, :3], li_ref[:, :3])
    print(what, "against the oracle: flips", flips, "relL2", rel)
    assert flips == 0.0 and rel == 0.0, (what, flips, rel)


def apply(r, edits, materials, textures, form="host", stream=None):
    """The case's ranges taken to the given records: the host forms, or rows in a tensor on the tracer's device."""
    import torch as th
    for table, (first, count) in mc.ranges(edits).items():
        recs = (materials if table == "m" else textures)[first:first + count]
        update = r.update_materials if table == "m" else r.update_textures
        if form == "host":
            update(first, recs, stream=stream)
        else:
            rows = mc.material_rows(recs) if table == "m" else mc.texture_rows(recs)
            update(first, th.tensor(rows, dtype=th.float32, device=r.device).reshape(count, -1), stream=stream)


def check_case(scene, edits, form="host", bvh="host", oracle=True, **kw):
    sa, sb = pair(scene) if isinstance(scene, str) else scene
    a = tracer(sa, bvh)
    tables0, others0, frame0 = tables(a), others(a), shot(a, **kw)
    held = mc.records(sa)
    edited = mc.edited_records(sa, edits)
    apply(a, edits, *edited, form=form)
    mc.write_desc(sb, *edited)
    b = tracer(sb, bvh)
    # 1: B's two tables, A's bytes everywhere else
    for k, name in enumerate(("DevMaterial records", "DevTexture records")):
        assert tables(a)[k] == tables(b)[k], (name, edits)
    assert tables(a) != tables0 and others(a) == others0, edits
    # 2: the fresh context's frame; 5: not A's
    frame_a, frame_b = shot(a, **kw), shot(b, **kw)
    same_frame(frame_a, frame_b, ("the fresh context's", edits))
    assert frame_a[1] != frame0[1], ("the edit left the frame alone", edits)
    # 4: the oracle on B's description
    if oracle and kw.get("sampler", "native") == "native":
        equals_the_oracle(frame_a, oracle_li(sb), edits)
    # the mirror holds the description last set
    assert raw(a.materials()) == raw(edited[0]) and raw(a.textures()) == raw(edited[1]), edits
    # 6: the inverse edit
    apply(a, edits, *held, form=form)
    assert tables(a) == tables0 and others(a) == others0 and same_frame(shot(a, **kw), frame0, ("the inverse edit", edits))
    assert raw(a.materials()) == raw(held[0]) and raw(a.textures()) == raw(held[1])
    apply(a, edits, *edited, form=form)   # ... and forth again, for the caller
    same_frame(shot(a, **kw), frame_a, ("the edit made again", edits))
    return a, b, edited


# ---------------------------------------------------------------------------
# every case through the host forms and, where a row holds it, through the device forms
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scene,name,edits", mc.CASES, ids=mc.IDS)
def test_each_case_through_the_host_form(torch, scene, name, edits):
    a, _, _ = check_case(scene, edits)
    if scene == "whitted":
        assert a.scene.desc.setting.integrator == _abi.GBL_INTEGRATOR_WHITTED


DEVICE_CASES = [c for c in mc.CASES if mc.device_form_takes(c[2])]


@pytest.mark.parametrize("scene,name,edits", DEVICE_CASES, ids=["%s-%s" % c[:2] for c in DEVICE_CASES])
def test_each_case_from_a_tensor(torch, scene, name, edits):
    check_case(scene, edits, form="device")


def test_the_device_cases_are_all_but_slots_to_tex_and_anisotropy():
    left = {f for c in mc.CASES if c not in DEVICE_CASES for _, _, f, _ in c[2]}
    assert left == {"tex_exponent", "tex_color", "tex_bump", "tex_normal", "to_tex", "max_anisotropy"} and len(DEVICE_CASES) >= 40


# ---------------------------------------------------------------------------
# the schedules, the tie rule, the stream sampler, both builders
# ---------------------------------------------------------------------------
VARIANTS = [("cornell", "blinn_exponent"), ("masked", "mask_alpha"), ("textured", "checkerboard_scrolled"), ("subsurface", "sigma_a")]


@pytest.mark.parametrize("scene,name", VARIANTS)
@pytest.mark.parametrize("schedule", ("megakernel", "wavefront", "auto"))
@pytest.mark.parametrize("form", ("host", "device"))
def test_under_each_schedule(torch, scene, name, schedule, form):
    check_case(scene, mc.case(scene, name)[2], form=form, schedule=schedule)


@pytest.mark.parametrize("scene,name", [("cornell", "lambert_color"), ("cornell", "several_records"), ("shapes", "blinn_exponent")])
@pytest.mark.parametrize("form", ("host", "device"))
def test_under_the_tie_rule(torch, scene, name, form):
    check_case(scene, mc.case(scene, name)[2], form=form, schedule="megakernel", exact_ties=True)


@pytest.mark.parametrize("scene,name", [("cornell", "mirror_color"), ("textured", "constant_behind_a_scale"), ("masked", "mask_transparent_color")])
@pytest.mark.parametrize("form", ("host", "device"))
def test_under_the_stream_sampler(torch, scene, name, form):
    check_case(scene, mc.case(scene, name)[2], form=form, sampler="stream")


@pytest.mark.parametrize("scene,name", [("cornell", "transparent_index"), ("bumpy", "bump_slot_repointed"), ("masked", "wrapped_lambert_color"),
                                        ("subsurface", "kr")])
def test_with_device_built_trees(torch, scene, name):
    check_case(scene, mc.case(scene, name)[2], bvh="device")


def test_auto_measures_again_after_an_edit(torch):
    """GBL_SCHEDULE_AUTO's pilot belongs to the old surfaces: an edited context under AUTO renders the fresh context's frame
    whichever schedule the new pilot picks (check_case under "auto"), also when the pilot ran BEFORE the edit."""
    sa, sb = pair("masked")
    edits = mc.case("masked", "mask_alpha")[2]
    a = tracer(sa)
    shot(a, schedule="auto")
    edited = mc.edited_records(sa, edits)
    for form in ("host", "device"):
        apply(a, edits, *edited, form=form)
        mc.write_desc(sb, *edited)
        same_frame(shot(a, schedule="auto"), shot(tracer(sb), schedule="auto"), form)
        apply(a, edits, *mc.records(sa), form=form)
        shot(a, schedule="auto")


# ---------------------------------------------------------------------------
# 3: the first-hit records
# ---------------------------------------------------------------------------
AOV_CASES = [("textured", "checkerboard_scrolled"), ("textured", "constant_behind_a_scale"), ("textured", "color_slot_repointed"),
             ("masked", "wrapped_lambert_color"), ("masked", "mask_alpha"), ("subsurface", "kr"), ("subsurface", "sigma_a")]


@pytest.mark.parametrize("scene,name,form", [(s, n, f) for s, n in AOV_CASES for f in ("host", "device") if f == "host" or mc.device_form_takes(mc.case(s, n)[2])])
def test_aov_records_follow_the_edit(torch, scene, name, form):
    edits = mc.case(scene, name)[2]
    sa, sb = pair(scene)
    a = tracer(sa)
    edited = mc.edited_records(sa, edits)
    apply(a, edits, *edited, form=form)
    mc.write_desc(sb, *edited)
    b = tracer(sb)
    got, want = (r.render_aov(seed=SEED, want_samples=True) for r in (a, b))
    assert got["samples"].cpu().numpy().tobytes() == want["samples"].cpu().numpy().tobytes(), (scene, name)
    for film in ("albedo", "normal", "depth"):
        assert helpers.rel_l2(got[film].numpy(), want[film].numpy()) <= FILM_RELL2_TOL, film
    oracle = ob.Oracle(sb)
    ref = oracle.first_hit(oracle.native_samples(SEED))
    assert got["samples"].cpu().numpy().view(np.uint32).tolist() == ref.view(np.uint32).tolist(), (scene, name, "the oracle's first hits")


# ---------------------------------------------------------------------------
# the device form: tensors, the mirror, host edits after device edits
# ---------------------------------------------------------------------------
def test_a_tensor_slice_with_a_storage_offset(torch):
    sa, sb = pair("cornell")
    a, h = tracer(sa), tracer(sa)
    edited, _ = mc.edited_records(sa, mc.case("cornell", "several_records")[2])
    flat = torch.full((1 + 9 * 12,), float("nan"), dtype=torch.float32, device=a.device)
    rows = flat[1:].view(9, 12)                                  # one float into the allocation: rows that are 4-byte aligned only
    rows[3:7] = torch.tensor(mc.material_rows(edited[0:4]), dtype=torch.float32)
    part = rows[3:7]
    assert part.storage_offset() == 37 and part.is_contiguous() and part.data_ptr() % 16 == 4
    a.update_materials(0, part)
    h.update_materials(0, edited[0:4])
    mc.write_desc(sb, edited, [])
    assert tables(a) == tables(h) == tables(tracer(sb))          # the host form against the device form: byte-equal tables
    same_frame(shot(a), shot(h))
    assert raw(a.materials()) == raw(edited)
    # one record out of the middle of the tensor
    a.update_materials(5, rows[4:5])
    got = a.materials()[5]
    assert raw(got)[4:40] == raw(edited[1])[4:40] and got.type == edited[5].type


@pytest.mark.parametrize("scene,name", [("textured", "materials_and_textures"), ("subsurface", "sigma_s_prime_texture_value"), ("masked", "float_constant_value")])
def test_the_host_form_against_the_device_form(torch, scene, name):
    sa, _ = pair(scene)
    edits = mc.case(scene, name)[2]
    a, h = tracer(sa), tracer(sa)
    edited = mc.edited_records(sa, edits)
    apply(a, edits, *edited, form="device")
    apply(h, edits, *edited, form="host")
    assert tables(a) == tables(h) and others(a) == others(h)
    same_frame(shot(a), shot(h))


def test_what_a_row_cannot_say_stays(torch):
    """color3 stays zero outside a subsurface material, a subsurface row's exponent is ignored (A comes from the index), a float
    texture's value[0] is broadcast: rows that say otherwise leave the packer's record."""
    sa, sb = pair("subsurface")
    a = tracer(sa)
    M, T = mc.records(sa)
    rows = torch.tensor(mc.material_rows(M), dtype=torch.float32, device=a.device)
    rows[:, 6:9] = 0.625        # a colour3 for every material
    rows[:, 11] = 123.0         # an exponent for the subsurface ones too
    rows[1, 9] = 1.25
    a.update_materials(0, rows)
    for m in M:
        m.color3[:] = [0.625] * 3
        m.exponent = 123.0
    M[1].index = 1.25
    mc.write_desc(sb, M, T)
    b = tracer(sb)
    assert tables(a) == tables(b)
    rec = a._materials_raw()["materials"]
    assert (rec["color3"][0] == 0).all() and (rec["color3"][1] == F32(0.625)).all() and rec["exponent"][1] != 123.0 and rec["exponent"][0] == 123.0
    assert raw(a.materials()) == raw(M)                          # the mirror holds the rows as given
    sm, sn = pair("masked")
    c = tracer(sm)
    M, T = mc.records(sm)
    trow = torch.tensor(mc.texture_rows(T), dtype=torch.float32, device=c.device)
    trow[3, 0:3] = torch.tensor([0.3, 0.6, 0.9])                  # a float constant
    c.update_textures(3, trow[3:4])
    T[3].value[:] = [0.3, 0.6, 0.9]
    mc.write_desc(sn, M, T)
    assert tables(c) == tables(tracer(sn))
    assert c._materials_raw()["textures"]["value"][3].tolist() == [F32(0.3)] * 3 and raw(c.textures()) == raw(T)


def test_round_trips_and_a_host_edit_after_a_device_edit(torch):
    sa, sb = pair("textured")
    a = tracer(sa)
    M, T = mc.records(sa)
    n, nt = sa.desc.num_materials, sa.desc.num_textures
    assert raw(a.materials()) == raw(M) and raw(a.textures()) == raw(T) and len(a.materials()) == n == 6 and len(a.textures()) == nt == 17
    # two device edits with a gap between them: the stale range is their union, the gap keeps the host's values
    M[0].color[:] = [0.1, 0.2, 0.3]
    M[4].color[:], M[4].index = [0.4, 0.5, 0.6], 1.75
    T[2].uv_offset[:] = [0.5, 0.125]
    T[16].uv_scale[:] = [2.0, 7.0]
    for i in (0, 4):
        a.update_materials(i, torch.tensor(mc.material_rows(M[i:i + 1]), dtype=torch.float32, device=a.device))
    for i in (2, 16):
        a.update_textures(i, torch.tensor(mc.texture_rows(T[i:i + 1]), dtype=torch.float32, device=a.device))
    assert raw(a.materials()) == raw(M) and raw(a.textures()) == raw(T)
    one = (_abi.gbl_material * 1)()
    for i in range(n):   # ranges
        assert a.lib.gbl_get_materials(a.handle, i, 1, one) == OK and raw(one[0]) == raw(M[i])
    # a host edit inside the gap, then a device edit on either side of it: the row table follows host edits too
    M[2].color[:] = [0.9, 0.8, 0.7]
    a.update_materials(2, [M[2]])
    M[1].color[:], M[3].k = [0.3, 0.3, 0.9], 2.5
    for i in (1, 3):
        a.update_materials(i, torch.tensor(mc.material_rows(M[i:i + 1]), dtype=torch.float32, device=a.device))
    assert raw(a.materials()) == raw(M)
    # a host edit right after a device edit refreshes the mirror first: its fixed-field checks read it, and what the device edit
    # wrote survives in the records the host edit does not name
    M[5].color[:] = [0.25, 0.5, 0.75]
    a.update_materials(5, torch.tensor(mc.material_rows(M[5:6]), dtype=torch.float32, device=a.device))
    T[13].uv_scale[:] = [4.0, 4.0]
    a.update_textures(13, torch.tensor(mc.texture_rows(T[13:14]), dtype=torch.float32, device=a.device))
    M[3].exponent = 0.5
    a.update_materials(3, exponent=0.5)                          # (keyword fields read the record through materials())
    T[2].max_anisotropy = 4.0
    a.update_textures(2, max_anisotropy=4.0)
    assert raw(a.materials()) == raw(M) and raw(a.textures()) == raw(T)
    mc.write_desc(sb, M, T)
    b = tracer(sb)
    assert tables(a) == tables(b) and same_frame(shot(a), shot(b))
    # count == 0 with a valid pointer changes nothing
    before = tables(a)
    assert a.lib.gbl_update_materials(a.handle, n, 0, one, None) == OK and a.lib.gbl_update_materials(a.handle, 0, 0, one, None) == OK
    assert a.lib.gbl_get_materials(a.handle, n, 0, one) == OK and tables(a) == before
    assert a.lib.gbl_get_materials(a.handle, n, 1, one) == INVALID and a.lib.gbl_get_materials(a.handle, 0, 1, None) == INVALID
    assert a.lib.gbl_get_materials(None, 0, 1, one) == INVALID and a.lib.gbl_get_textures(a.handle, nt, 1, (_abi.gbl_texture * 1)()) == INVALID


def test_more_edits_than_staging_slots(torch):
    """Nine host edits back to back without a wait: a staging slot is written again only after its upload."""
    sa, sb = pair("cornell")
    a = tracer(sa)
    M, T = mc.records(sa)
    for k in range(9):
        M[1].color[:] = [0.1 * (k + 1), 0.05 * k, 0.9 - 0.1 * k]
        M[5].exponent = 4.0 + k
        a.update_materials(1, [M[1]])
        a.update_materials(5, [M[5]])
    mc.write_desc(sb, M, T)
    assert tables(a) == tables(tracer(sb)) and raw(a.materials()) == raw(M)


# ---------------------------------------------------------------------------
# stream order
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("host", "device"))
def test_edits_keep_the_streams_order(torch, form):
    big, small = dict(resolution=(64, 64), spp=16, depth=3), dict(spp=1, depth=2)
    sa, sb = pair("textured", **big)
    edits = mc.case("textured", "materials_and_textures")[2]
    edited = mc.edited_records(sa, edits)
    small_setting = type(sa.desc.setting).from_buffer_copy(sa.desc.setting)
    small_setting.sample_per_pixel, small_setting.max_ray_depth = small["spp"], small["depth"]
    a = tracer(sa)
    stream = torch.cuda.Stream(device=a.device)
    assert stream.cuda_stream != torch.cuda.default_stream(a.device).cuda_stream
    with torch.cuda.stream(stream):
        first = a.render(seed=SEED, want_li=True, schedule="megakernel")
        apply(a, edits, *edited, form=form, stream=stream)
        second = a.render(seed=SEED, want_li=True, schedule="megakernel", setting=small_setting)
    stream.synchronize()
    unedited = tracer(sa)
    fresh_before = unedited.render(seed=SEED, want_li=True, schedule="megakernel")
    small_before = unedited.render(seed=SEED, want_li=True, schedule="megakernel", setting=small_setting)
    mc.write_desc(sb, *edited)
    fresh_after = tracer(sb).render(seed=SEED, want_li=True, schedule="megakernel", setting=small_setting)
    torch.cuda.synchronize()
    for got, want, what in ((first, fresh_before, "queued before the edit"), (second, fresh_after, "queued after the edit")):
        assert torch.equal(got["li"], want["li"]), what
        assert helpers.rel_l2(got["film"].numpy(), want["film"].numpy()) <= FILM_RELL2_TOL, what
    assert not torch.equal(second["li"], small_before["li"])   # the second render saw other surfaces


# ---------------------------------------------------------------------------
# every refusal, with both tables read back unchanged after it
# ---------------------------------------------------------------------------
class Refusals:
    """A tracer, its tables, its mirror and its frame; `refused` makes one call and checks that nothing moved."""

    def __init__(self, scene):
        self.r, self.scene = tracer(scene), scene
        self.tables, self.others, self.frame = tables(self.r), others(self.r), shot(self.r)
        self.held = raw(self.r.materials()), raw(self.r.textures())

    def unchanged(self, text):
        assert tables(self.r) == self.tables and others(self.r) == self.others, text
        assert (raw(self.r.materials()), raw(self.r.textures())) == self.held, text
        same_frame(shot(self.r), self.frame, text)

    def refused(self, status, words, first, recs):
        material = not recs or isinstance(recs[0], _abi.gbl_material)
        arr = ((_abi.gbl_material if material else _abi.gbl_texture) * max(1, len(recs)))(*recs)
        fn = self.r.lib.gbl_update_materials if material else self.r.lib.gbl_update_textures
        got = fn(self.r.handle, first, len(recs), arr, None)
        text = self.r.lib.gbl_last_error(self.r.handle).decode()
        assert got == status, (got, text)
        for w in words:
            assert w in text, (w, text)
        self.unchanged(text)

    def refused_device(self, words, fn, first, count, ptr):
        got = fn(self.r.handle, first, count, ptr, None)
        text = self.r.lib.gbl_last_error(self.r.handle).decode()
        assert got == INVALID, (got, text)
        for w in words:
            assert w in text, (w, text)
        self.unchanged(text)


def mat(scene, i, **fields):
    rec = mc.records(scene)[0][i]
    for f, v in fields.items():
        mc.set_field(rec, f, v)
    return rec


def tex(scene, i, **fields):
    rec = mc.records(scene)[1][i]
    for f, v in fields.items():
        mc.set_field(rec, f, v)
    return rec


def test_material_refusals_in_their_order(torch):
    sa, _ = pair("bumpy", spp=1, depth=2)
    x = Refusals(sa)
    lib, h = x.r.lib, x.r.handle
    M, _ = mc.records(sa)
    n = len(M)
    nan = float("nan")
    assert lib.gbl_update_materials(None, 0, 1, (_abi.gbl_material * 1)(M[0]), None) == INVALID
    assert lib.gbl_update_materials(h, 0, 1, None, None) == INVALID and "materials is NULL" in lib.gbl_last_error(h).decode()
    assert lib.gbl_update_materials(h, n + 5, 0, None, None) == INVALID and "materials is NULL" in lib.gbl_last_error(h).decode()   # arguments before the range
    x.refused(INVALID, ["material range out of bounds"], 1, M)
    x.refused(INVALID, ["material range out of bounds"], n, M[:1])
    x.refused(INVALID, ["material range out of bounds"], n + 1, [])
    x.refused(INVALID, ["material range out of bounds"], n, [mat(sa, 3, type=0)])                       # the range before the fields
    # the fixed fields, naming the entry, the field and both values
    x.refused(INVALID, ["material 3", "type cannot change", "holds 1", "gives 0"], 3, [mat(sa, 3, type=0)])
    x.refused(INVALID, ["material 5", "type cannot change", "holds 4", "gives 77"], 5, [mat(sa, 5, type=77)])
    x.refused(INVALID, ["material 5", "masked_material cannot change", "holds 1", "gives 0"], 5, [mat(sa, 5, masked_material=0)])
    x.refused(INVALID, ["material 0", "masked_material cannot change", "holds -1", "gives 1"], 0, [mat(sa, 0, masked_material=1)])
    for slot, have in (("tex_color", 5), ("tex_bump", 2)):
        x.refused(INVALID, ["material 0", slot, "cannot be occupied or vacated", "holds %d" % have, "gives -1"], 0, [mat(sa, 0, **{slot: -1})])
    for slot in ("tex_color2", "tex_exponent", "tex_color3", "tex_normal"):
        x.refused(INVALID, ["material 0", slot, "cannot be occupied or vacated", "holds -1", "gives 3"], 0, [mat(sa, 0, **{slot: 3})])
    # two faults: the field that cannot change is met before the value, in whichever record it sits
    x.refused(INVALID, ["material 3", "type cannot change"], 3, [mat(sa, 3, type=2, color=[nan, 1.0, 1.0])])
    both = [mat(sa, 0, color=[nan, 1.0, 1.0]), mat(sa, 1, tex_normal=-1)]
    x.refused(INVALID, ["material 1", "tex_normal", "occupied or vacated"], 0, both)
    # values: every editable float, naming the field
    for bad in (nan, float("inf"), -float("inf")):
        for field in ("color", "color2"):
            for k in range(3):
                v = [0.5, 0.5, 0.5]
                v[k] = bad
                x.refused(INVALID, ["material 3", field + " is not finite"], 3, [mat(sa, 3, **{field: v})])
        for field in ("index", "k", "exponent"):
            x.refused(INVALID, ["material 3", field + " is not finite"], 3, [mat(sa, 3, **{field: bad})])
    # a value before a reference, and colour3 outside a subsurface material is not looked at
    x.refused(INVALID, ["material 0", "k is not finite"], 0, [mat(sa, 0, k=nan, tex_bump=99)])
    assert lib.gbl_update_materials(h, 3, 1, (_abi.gbl_material * 1)(mat(sa, 3, color3=[nan, 0.0, 0.0])), None) == OK
    assert tables(x.r) == x.tables
    assert lib.gbl_update_materials(h, 3, 1, (_abi.gbl_material * 1)(M[3]), None) == OK
    x.unchanged("the record put back")
    # references, on the patched table: range, the slot's kind, depth
    nt = sa.desc.num_textures
    x.refused(INVALID, ["material 0", "references a texture out of range"], 0, [mat(sa, 0, tex_bump=nt)])
    x.refused(INVALID, ["material 0", "tex_bump", "texture 5 is a colour texture", "takes a float texture"], 0, [mat(sa, 0, tex_bump=5)])
    x.refused(INVALID, ["material 0", "tex_color", "texture 14 is a float texture", "takes a colour texture"], 0, [mat(sa, 0, tex_color=14)])
    x.refused(INVALID, ["material 1", "tex_normal", "texture 2 is a float texture"], 1, [mat(sa, 1, tex_normal=2)])


def test_material_refusals_of_a_graph_too_deep_and_of_color3(torch):
    """A hand-made description: texture 3 is a scale of a scale of a checkerboard, three levels below a slot, which no material
    of the scene reaches; pointing a slot at it is gbl_create's GBL_ERR_UNSUPPORTED."""
    sa, sb = pair("textured", spp=1, depth=2)
    T = mc.records(sa)[1]
    # 7 = scale(5 = checkerboard(3, 4), 6); make 9 (a constant nobody else reads but checkerboard 10) a scale of 7: 10 = checkerboard(8, 9) is then four levels
    T[9].type, T[9].child[0], T[9].child[1] = _abi.GBL_TEX_SCALE, 7, 6
    mc.write_desc(sb, mc.records(sa)[0], T)
    sb.desc.materials[2].tex_color = 2          # material 2 leaves the deep graph alone in the description the context is made of
    x = Refusals(sb)
    x.refused(UNSUPPORTED, ["material 2", "texture graph deeper than 2 levels"], 2, [mat(sb, 2, tex_color=10)])
    x.refused(UNSUPPORTED, ["material 2", "texture graph deeper than 2 levels"], 2, [mat(sb, 2, tex_color=9)])
    assert x.r.lib.gbl_update_materials(x.r.handle, 2, 1, (_abi.gbl_material * 1)(mat(sb, 2, tex_color=7)), None) == OK   # two levels: accepted
    ss, _ = pair("subsurface", spp=1, depth=2)
    y = Refusals(ss)
    y.refused(INVALID, ["material 1", "color3 is not finite"], 1, [mat(ss, 1, color3=[1.0, float("inf"), 1.0])])
    y.refused(INVALID, ["material 2", "references a texture out of range"], 2, [mat(ss, 2, tex_color2=9)])


def test_texture_refusals_in_their_order(torch):
    sa, _ = pair("imagetex", spp=1, depth=2)
    x = Refusals(sa)
    lib, h = x.r.lib, x.r.handle
    T = mc.records(sa)[1]
    n = len(T)
    nan = float("nan")
    assert lib.gbl_update_textures(None, 0, 1, (_abi.gbl_texture * 1)(T[0]), None) == INVALID
    assert lib.gbl_update_textures(h, 0, 1, None, None) == INVALID and "textures is NULL" in lib.gbl_last_error(h).decode()
    x.refused(INVALID, ["texture range out of bounds"], 1, T)
    x.refused(INVALID, ["texture range out of bounds"], n, T[:1])
    x.refused(INVALID, ["texture range out of bounds"], n, [tex(sa, 0, type=0)])
    x.refused(INVALID, ["texture 0", "type cannot change", "holds 3", "gives 0"], 0, [tex(sa, 0, type=0)])
    x.refused(INVALID, ["texture 0", "is_float cannot change", "holds 0", "gives 1"], 0, [tex(sa, 0, is_float=1)])
    x.refused(INVALID, ["texture 3", "child[0] cannot change", "holds 1", "gives 0"], 3, [tex(sa, 3, child=[0, 2])])
    x.refused(INVALID, ["texture 3", "child[1] cannot change", "holds 2", "gives 6"], 3, [tex(sa, 3, child=[1, 6])])
    x.refused(INVALID, ["texture 0", "mapping cannot change", "holds 0", "gives 1"], 0, [tex(sa, 0, mapping=1)])
    x.refused(INVALID, ["texture 0", "image cannot change", "holds 0", "gives 1"], 0, [tex(sa, 0, image=1)])
    x.refused(INVALID, ["texture 0", "filter cannot change", "holds 0", "gives 1"], 0, [tex(sa, 0, filter=1)])
    x.refused(INVALID, ["texture 0", "image_filter cannot change", "holds 3", "gives 1"], 0, [tex(sa, 0, image_filter=1)])
    x.refused(INVALID, ["texture 8", "address cannot change", "holds 2", "gives 0"], 8, [tex(sa, 8, address=0)])
    x.refused(INVALID, ["texture 0", "type cannot change"], 0, [tex(sa, 0, type=1, value=[nan, 0.0, 0.0])])      # fixed fields before values
    for bad in (nan, float("inf")):
        x.refused(INVALID, ["texture 2", "value is not finite"], 2, [tex(sa, 2, value=[bad, 0.0, 0.0])])
        x.refused(INVALID, ["texture 0", "uv_scale is not finite"], 0, [tex(sa, 0, uv_scale=[1.0, bad])])
        x.refused(INVALID, ["texture 0", "uv_offset is not finite"], 0, [tex(sa, 0, uv_offset=[bad, 0.0])])
        x.refused(INVALID, ["texture 0", "max_anisotropy is not finite"], 0, [tex(sa, 0, max_anisotropy=bad)])
        x.refused(INVALID, ["texture 4", "to_tex is not finite"], 4, [tex(sa, 4, to_tex=[0.0, bad, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0])])
    # a to_tex the reference cannot invert, in pack_transform's words -- where the texture reads it
    x.refused(INVALID, ["texture 4", "to_tex", "|det(toWorld)| < 1e-5", "the reference cannot invert this transform"], 4,
              [tex(sa, 4, to_tex=[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.01, 0.01, 0.01])])
    assert lib.gbl_update_textures(h, 0, 1, (_abi.gbl_texture * 1)(tex(sa, 0, to_tex=[0.0] * 3 + [1.0, 0.0, 0.0, 0.0] + [0.0] * 3)), None) == OK   # a uv mapping does not
    assert tables(x.r) == x.tables
    assert lib.gbl_update_textures(h, 0, 1, (_abi.gbl_texture * 1)(T[0]), None) == OK
    x.unchanged("the record put back")
    # a scene without textures refuses every range but the empty one
    sc, _ = pair("cornell", spp=1, depth=2)
    y = Refusals(sc)
    y.refused(INVALID, ["texture range out of bounds"], 0, [T[0]])
    assert y.r.lib.gbl_update_textures(y.r.handle, 0, 0, (_abi.gbl_texture * 1)(), None) == OK and y.r.textures() == []


def test_device_form_refusals(torch):
    sa, _ = pair("textured", spp=1, depth=2)
    x = Refusals(sa)
    lib = x.r.lib
    nm, nt = sa.desc.num_materials, sa.desc.num_textures
    with open("/proc/self/maps") as f:   # the HIP runtime this process already runs on, not a second copy of it
        hip = C.CDLL(next(line.split()[-1] for line in f if "libamdhip64" in line))
    for fn, row, total, what in ((lib.gbl_update_materials_device, 12, nm, "material"), (lib.gbl_update_textures_device, 7, nt, "texture")):
        name = fn.__name__
        rows = torch.zeros((total, row), dtype=torch.float32, device=x.r.device)
        assert fn(None, 0, 1, rows.data_ptr(), None) == INVALID
        x.refused_device([name, "rows is NULL"], fn, 0, 1, None)
        x.refused_device([name, "rows is NULL"], fn, total + 1, 1, None)                        # arguments before the range
        x.refused_device([name, what + " range out of bounds"], fn, 1, total, rows.data_ptr())
        x.refused_device([name, what + " range out of bounds"], fn, total, 1, rows.data_ptr())
        host = np.zeros((total, row), np.float32)
        x.refused_device([name, "rows", "not device memory"], fn, 0, total, host.ctypes.data)  # a plain host pointer: refused before anything reads it
        short = C.c_void_p()
        assert hip.hipMalloc(C.byref(short), C.c_size_t(4 * row * total - 4)) == 0              # 4 bytes short of the rows; checked by the refusal, never read
        try:
            x.refused_device([name, "rows: its allocation ends"], fn, 0, total, short.value)
            x.refused_device([name, "rows: its allocation ends"], fn, 1, total - 1, short.value + 4 * row)
        finally:
            assert hip.hipFree(short) == 0
        assert fn(x.r.handle, 0, 0, rows.data_ptr(), None) == OK and fn(x.r.handle, total, 0, rows.data_ptr(), None) == OK
        x.unchanged("count == 0")


def test_the_python_face(torch):
    sa, _ = pair("textured", spp=1, depth=2)
    a, b = tracer(sa), tracer(sa)
    a.update_materials(3, color=(0.2, 0.4, 0.6), index=2.0)
    a.update_textures(10, to_tex=((0.0, 0.0, 0.0), tuple(mc.Q90X), (1.0, 2.0, 1.0)), value=(0.5, 0.5, 0.5))
    assert b.lib.gbl_update_materials(b.handle, 3, 1, (_abi.gbl_material * 1)(mat(sa, 3, color=[0.2, 0.4, 0.6], index=2.0)), None) == OK
    assert b.lib.gbl_update_textures(b.handle, 10, 1, (_abi.gbl_texture * 1)(tex(sa, 10, to_tex=[0.0] * 3 + mc.Q90X + [1.0, 2.0, 1.0], value=[0.5] * 3)), None) == OK
    assert tables(a) == tables(b) and raw(a.materials()) == raw(b.materials()) and raw(a.textures()) == raw(b.textures()) and same_frame(shot(a), shot(b))
    before = tables(a)
    with pytest.raises(TypeError):
        a.update_materials(3, colour=(1.0, 1.0, 1.0))
    with pytest.raises(_abi.GoblinError) as e:
        a.update_materials(3, type=0)
    assert e.value.status == INVALID and "type cannot change" in str(e.value)
    with pytest.raises(_abi.GoblinError) as e:
        a.update_textures(10, mapping=0)
    assert e.value.status == INVALID and "mapping cannot change" in str(e.value)
    with pytest.raises(ValueError):
        a.update_materials(0, torch.zeros((1, 12), dtype=torch.float32))       # a tensor on the host
    with pytest.raises(ValueError):
        a.update_materials(5, torch.zeros((2, 12), dtype=torch.float32, device=a.device))
    a.update_materials(0)   # nothing named: nothing changes
    a.update_materials(0, torch.zeros((0, 12), dtype=torch.float32, device=a.device))
    assert tables(a) == before
