"""Surface shading and the lights on generated charts (tests/surface_chart.py), host side: the oracle against the compiled
reference, and what the charts' cases actually meet.

Fixtures: tests/golden/surface_<case>.npz, written by the compiled reference (tests/golden/make_surface_golden.py).  The charts'
frame makes a Film pixel one sample's w * Li (asserted below, not assumed).  Coverage is asserted on the probe (Oracle.surface)
under the reference stream's own draws -- the samples the fixtures' li were computed from -- with a margin of MARGIN samples, and
the counts are printed.

No case was dropped: the compiled reference returns on every one.  None of them gives a NaN: under the transparent material an
index below 1 is total reflection behind specularRefract's `f == 1.0f`, not the NaN the subsurface term computes there, so the
"weight 0 exactly where li is NaN" rule is asserted on every case and holds with no pixel dropped.
"""
import os

import numpy as np
import pytest

import oracle_binding as ob
from goblin_amd import _abi
import surface_chart as sc
from oracle_binding import Oracle
from test_gpu_splat_fastpath import add_samples_f64

SPP1 = list(sc.CASES)
SEED = 0x5EEDC0FFEE
MARGIN = 8           # every coverage count below holds with at least this many samples
EVENT = {name: i for i, name in enumerate(Oracle.SURF_EVENTS)}
LAMBERT, BLINN, GLASS, MIRROR = (t + 1 for t in (_abi.GBL_MAT_LAMBERT, _abi.GBL_MAT_BLINN, _abi.GBL_MAT_TRANSPARENT, _abi.GBL_MAT_MIRROR))
MASKED = 16          # added to the material word under a mask


@pytest.fixture(scope="module")
def runs():
    """Per case, once: the oracle's render under the reference stream, with the probe's records of the same samples."""
    cache = {}

    def get(case):
        if case not in cache:
            o = Oracle(sc.scene(case))
            run = o.render(threads=1, want_samples=True)
            run["probe"], run["probe_li"] = o.surface(run["samples"])
            cache[case] = (o, run)
        return cache[case]
    return get


def count(run, event, where=None):
    """The number of camera samples at which some vertex noted the event (among `where`)."""
    hit = run["probe"][:, Oracle.SURF_COUNTS + EVENT[event]] > 0
    return int((hit if where is None else hit & where).sum())


def first(run, event):
    """Camera samples whose first vertex noted the event."""
    return (run["probe"][:, Oracle.SURF_FIRST].astype(np.int64) >> EVENT[event]) & 1 != 0


def material(run, kind):
    return run["probe"][:, Oracle.SURF_MATERIAL] == kind


def seen(run, *events, where=None):
    return {e: count(run, e, where) for e in events}


def on_instance(o, run, case, name):
    """Camera samples whose first hit is the named instance."""
    return o.first_hit(run["samples"]).view(np.int32)[:, 7] == sc.instance_id(case, name)


def on_emitter(o, run, case):
    """Camera samples whose first hit is an emitter."""
    d = sc.scene(case).desc
    emitters = [i for i in range(d.num_instances) if d.instances[i].area_light >= 0]
    hit = o.first_hit(run["samples"]).view(np.int32)
    return np.isin(hit[:, 7], emitters) & (hit[:, 11] != 0)


def differing(a, b):
    fa, fb = sc.golden(a)["film"], sc.golden(b)["film"]
    return int((fa[..., :3] != fb[..., :3]).any(axis=-1).sum())


# ---------------------------------------------------------------------------
# the oracle is the compiled reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.ALL_CASES)
def test_oracle_is_the_reference(runs, case):
    """Same stream, Li bit for bit with NaN positions equal, every Film accumulator bit for bit, no NaN in a Film; and the splat
    dropped a pixel exactly where its sample's Li is NaN."""
    g, run = sc.golden(case), runs(case)[1]
    assert np.array_equal(run["samples"][:, :4], g["samples"])
    assert sc.same_bits(run["li"], g["li"]), sc.sample_report(case, "oracle against reference", run["li"], g["li"], run["samples"])
    assert not np.isnan(g["film"]).any() and not np.isnan(run["film"]).any()
    assert np.array_equal(run["film"].view(np.uint32), g["film"].view(np.uint32)), sc.film_report(case, run["film"], g["film"])
    if case in sc.CASES:
        nan = np.isnan(g["li"][:, :3]).any(axis=1)
        x, y = np.floor(g["samples"][:, 0]).astype(int), np.floor(g["samples"][:, 1]).astype(int)
        inside = (x >= 0) & (x < 24) & (y >= 0) & (y < 16)
        dropped = np.zeros((16, 24), bool)
        dropped[y[nan & inside], x[nan & inside]] = True
        assert np.array_equal(g["film"][..., 3] == 0, dropped), case


@pytest.mark.skipif(not os.path.exists(ob.REF_HARNESS), reason="needs the compiled reference (oracle/_ref/ref_harness)")
@pytest.mark.parametrize("case", sc.ALL_CASES)
def test_fixture_is_what_the_reference_gives_now(tmp_path, case):
    """The harness run again gives exactly the committed fixture, byte for byte: a fixture gone stale against surface_chart.py fails."""
    import sys
    sys.path.insert(0, sc.GOLDEN_DIR)
    try:
        import make_surface_golden as mg
    finally:
        sys.path.remove(sc.GOLDEN_DIR)
    live, kept = mg.run_case(case, str(tmp_path)), sc.golden(case)
    for k in ("film", "samples", "li"):
        assert live[k].shape == kept[k].shape and np.array_equal(live[k].view(np.uint32), kept[k].view(np.uint32)), (case, k)
    mg.save(str(tmp_path / "again.npz"), live)
    with open(tmp_path / "again.npz", "rb") as a, open(os.path.join(sc.GOLDEN_DIR, "surface_" + case + ".npz"), "rb") as b:
        assert a.read() == b.read(), case


@pytest.mark.parametrize("case", SPP1)
def test_a_film_pixel_is_one_sample(runs, case):
    """No pixel has more than two addends (decided by the float32 footprint rule of ImageTile::addSample on the reference's own
    image positions), so float addition's order cannot matter; and the reference's Film is the splat of its logged Li."""
    g = sc.golden(case)
    o = runs(case)[0]
    n = g["samples"].shape[0]
    yres, xres = g["film"].shape[:2]
    hits, cells = add_samples_f64(sc.scene(case), np.ones(256, np.float32), g["samples"][:, :2], np.ones((n, 4), np.float32))
    assert hits[..., 3].max() <= 2, (case, hits[..., 3].max())
    assert (hits[..., 3] >= 1).all() and cells >= xres * yres
    film = o.splat(np.ascontiguousarray(g["samples"]), np.ascontiguousarray(g["li"]))
    assert np.array_equal(film.view(np.uint32), g["film"].view(np.uint32)), sc.film_report(case, film, g["film"])


@pytest.mark.parametrize("case", sc.ALL_CASES)
def test_probe_is_the_function_li_calls(runs, case):
    """The probe's li is li_replay's and the render's: noting changes nothing."""
    o, run = runs(case)
    li, _ = o.li_replay(run["samples"])
    assert sc.same_bits(run["probe_li"], li) and sc.same_bits(li, run["li"])
    assert np.array_equal(run["probe"][:, Oracle.SURF_NAN] != 0, np.isnan(li[:, :3]).any(axis=1))


@pytest.mark.parametrize("case", sc.LEAN)
def test_twin_is_the_case(runs, case):
    """The `+ext` twin -- a sphere model far below the floor, which makes the device take the EXT kernels -- is reached by no ray:
    same stream, same li, bit for bit."""
    run = runs(case)[1]
    twin = sc.scene(case + "+ext")
    d = twin.desc
    assert any(d.meshes[i].shape == _abi.GBL_SHAPE_SPHERE for i in range(d.num_meshes))
    other = Oracle(twin).render(threads=1, want_samples=True)
    assert np.array_equal(other["samples"], run["samples"])
    assert sc.same_bits(other["li"], run["li"]), sc.sample_report(case, "twin", other["li"], run["li"], run["samples"])


def test_native_draws_meet_the_same_edges(runs):
    """The device tests run the native sampler's records: the bases meet their events under those too."""
    for case, events in (("lean", ("REFRACT", "BSDF_BLACK", "OCCLUDED", "UNOCCLUDED", "END_SURFACE", "END_ESCAPED")),
                         ("deep", ("ENTERING", "LEAVING", "TOTAL_REFLECTION", "REFLECT", "REFRACT", "PUNCHED", "ATTENUATED")),
                         ("wh", ("ENTERING", "LEAVING", "TOTAL_REFLECTION", "OCCLUDED", "UNOCCLUDED"))):
        o = runs(case)[0]
        p, _ = o.surface(o.native_samples(SEED))
        for e in events:
            assert (p[:, Oracle.SURF_COUNTS + EVENT[e]] > 0).sum() >= MARGIN, (case, e)


# ---------------------------------------------------------------------------
# the charts test something: what the probe saw, under the stream's draws
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.BASES)
def test_bases(runs, case):
    """Every material of the row is the first vertex of MARGIN samples or more (each cube covers twenty), the light sample is both
    shadowed and not, the BSDF is black towards the light (the specular cubes, the faces turned away)."""
    run = runs(case)[1]
    kinds = {k: int(material(run, k).sum()) for k in (LAMBERT, BLINN, GLASS, MIRROR)}
    got = seen(run, "BSDF_BLACK", "OCCLUDED", "UNOCCLUDED", "ENTERING")
    if case in ("deep", "wh"):
        got.update(seen(run, "LEAVING", "TOTAL_REFLECTION"))
    if case == "deep":
        got.update(seen(run, "REFLECT", "REFRACT", "PUNCHED", "ATTENUATED"))
        got["masked first"] = int(material(run, LAMBERT + MASKED).sum())
    if case != "wh":
        got.update(seen(run, "END_SURFACE", "END_ESCAPED"))
    print(case, "first vertex by material", kinds, got, "vertices", int(run["probe"][:, Oracle.SURF_VERTICES].sum()))
    assert min(kinds.values()) >= 20 and min(got.values()) >= MARGIN, (case, kinds, got)
    assert not np.isnan(run["li"]).any()
    depth = sc.doc(case)["render_setting"]["max_ray_depth"]
    if case != "wh":
        assert run["probe"][:, Oracle.SURF_VERTICES].max() == depth - 1
    d = sc.scene(case).desc
    shapes = {d.meshes[i].shape for i in range(d.num_meshes)}
    assert (shapes == {_abi.GBL_SHAPE_MESH}) == (case in ("lean", "deep"))       # what makes `ext` and `wh` extended


def test_transparent(runs):
    """index 1: the two Fresnel quotients are 0 or a rounding residue (cost is sqrt(1 - (1 - cosi^2)), not cosi): reflectChance is
    exactly 0 or below 1e-9 at every glass vertex, and never drawn.  1.0001: a reflectChance of 2.5e-9 at normal incidence.  2.4:
    both lobes.  0.8: total reflection on entering -- Fresnel 1, specularRefract returns 0 behind `f == 1.0f`, reflectChance 1 --
    and no NaN.  Black Kr / Kt / both: the `f != Black` exit.  The index and Kr cases stand on `deep`: at max_ray_depth 2 under a
    point light a specular vertex's one continuation is never shaded, and the Film would be the base's."""
    one, near, base = runs("deep_index_1")[1], runs("deep_index_1.0001")[1], runs("lean")[1]
    g = material(one, GLASS)
    chance = one["probe"][g, Oracle.SURF_REFLECT_CHANCE]
    print("index 1: reflectChance exactly 0 at", int((chance == 0).sum()), "of", int(g.sum()), "glass samples, at most %.3g" % chance.max())
    assert g.sum() >= 20 and (chance == 0).sum() >= MARGIN and chance.max() < 1e-9
    assert count(one, "REFLECT") == 0 and count(one, "REFRACT", g) == g.sum()
    chance = near["probe"][material(near, GLASS), Oracle.SURF_REFLECT_CHANCE]
    print("index 1.0001: reflectChance from %.3g to %.3g" % (chance.min(), chance.max()))
    assert (chance > 0).sum() >= MARGIN and chance.max() < 1e-3
    dense = runs("deep_index_2.4")[1]
    got = seen(dense, "REFLECT", "REFRACT", "TOTAL_REFLECTION", "LEAVING")
    print("deep_index_2.4", got)
    assert min(got.values()) >= MARGIN
    for case in ("deep_index_0.8", "wh_glass_0.8"):
        run = runs(case)[1]
        tir = first(run, "TOTAL_REFLECTION") & first(run, "ENTERING") & material(run, GLASS)
        print(case, "glass samples", int(material(run, GLASS).sum()), "totally reflected on entering", int(tir.sum()))
        assert tir.sum() >= MARGIN and (material(run, GLASS) & ~tir).sum() >= MARGIN and not np.isnan(run["li"]).any()
        if case != "wh_glass_0.8":
            chance = run["probe"][tir, Oracle.SURF_REFLECT_CHANCE]       # (1 / cos) * cos: 1 to an ulp or two
            assert (np.abs(chance - 1) < 1e-6).all() and (first(run, "REFLECT") & tir).sum() >= MARGIN
    assert count(base, "TOTAL_REFLECTION") == 0
    # black lobes: the sampled value is black at the glass vertices that drew the black lobe
    kt, both, kr = runs("glass_kt_black")[1], runs("glass_both_black")[1], runs("deep_kr_black")[1]
    g = material(kt, GLASS)
    assert (first(kt, "SAMPLE_BLACK") & first(kt, "REFRACT") & g).sum() >= MARGIN and not (first(kt, "SAMPLE_BLACK") & first(kt, "REFLECT") & g).any()
    g = material(both, GLASS)
    assert (first(both, "SAMPLE_BLACK") & g).sum() == g.sum() >= 20
    assert count(kr, "SAMPLE_BLACK") >= count(runs("deep")[1], "SAMPLE_BLACK") + MARGIN
    for a, b in (("glass_kt_black", "lean"), ("glass_both_black", "lean"), ("deep_kr_black", "deep"), ("deep_index_1", "deep_index_1.0001"),
                 ("deep_index_2.4", "deep"), ("deep_index_0.8", "deep"), ("deep_index_1", "deep")):
        n = differing(a, b)
        print(a, "against", b, "pixels that differ:", n)
        assert n >= MARGIN, (a, b, n)
    # the pane seen at grazing incidence from its front: cosines of a few hundredths, a reflectChance of 0.59 to 0.78, both lobes drawn
    o, pane = runs("glass_grazing")
    on = on_instance(o, pane, "glass_grazing", "pane")
    got = {"on the pane": int(on.sum()), "entering": int((on & first(pane, "ENTERING")).sum()), "reflected": int((on & first(pane, "REFLECT")).sum())}
    print("glass_grazing", got, "reflectChance", np.sort(pane["probe"][on, Oracle.SURF_REFLECT_CHANCE])[[0, -1]])
    chance = pane["probe"][on, Oracle.SURF_REFLECT_CHANCE]
    assert got["entering"] == got["on the pane"] and got["reflected"] >= MARGIN and (on & first(pane, "REFRACT")).sum() >= MARGIN
    assert chance.min() > 0.5 and chance.max() < 1


def test_blinn(runs):
    """Exponent 0 and 1: a lobe as wide as the hemisphere, sampled directions below the surface (pdf 0).  1e3 and 1e5: pow()
    underflows towards the light -- the value is black at Blinn vertices that the base lights.  k 0.5 and 6: the conductor's
    Fresnel term; k 0 and a negative k are the dielectric (`k > 0`), bit for bit the base.  index 1: Fresnel 0 or a rounding residue, a lobe that is black or below 1e-9."""
    base = runs("lean")[1]
    b = material(base, BLINN)
    lit = int((b & ~first(base, "BSDF_BLACK") & first(base, "UNOCCLUDED")).sum())
    for case in ("blinn_exponent_0", "blinn_exponent_1"):
        run = runs(case)[1]
        below = int((material(run, BLINN) & first(run, "SAMPLE_PDF_ZERO")).sum())
        print(case, "Blinn samples whose sampled direction has pdf 0:", below)
        assert below >= MARGIN
    for case in ("blinn_exponent_1e3", "blinn_exponent_1e5"):
        run = runs(case)[1]
        black = int((material(run, BLINN) & first(run, "BSDF_BLACK")).sum())
        print(case, "Blinn samples black towards the light:", black, "of", int(material(run, BLINN).sum()), "(base: lit", lit, ")")
        assert black >= int((b & first(base, "BSDF_BLACK")).sum()) + MARGIN
        assert not np.isnan(run["li"]).any()
    for case in ("blinn_k_0", "blinn_k_negative"):
        assert sc.same_bits(sc.golden(case)["li"], sc.golden("lean")["li"]), case
    one = runs("blinn_index_1")[1]
    m = material(one, BLINN)
    black = int((m & first(one, "SAMPLE_BLACK")).sum())
    print("blinn_index_1: sampled value exactly black at", black, "of", int(m.sum()), "Blinn samples; brightest Blinn sample %.3g" % one["li"][m, :3].max())
    assert m.sum() >= 20 and black >= MARGIN and one["li"][m, :3].max() < 1e-9
    for a, b_ in (("blinn_k_0.5", "lean"), ("blinn_k_6", "blinn_k_0.5"), ("blinn_index_1", "lean"), ("blinn_exponent_0", "blinn_exponent_1"),
                  ("blinn_exponent_1e3", "lean"), ("wh_conductor", "wh")):
        n = differing(a, b_)
        print(a, "against", b_, "pixels that differ:", n)
        assert n >= MARGIN, (a, b_, n)


def test_mirror_and_lambert(runs):
    for a, b in (("deep_mirror_k_0.5", "deep"), ("deep_mirror_k_0", "deep_mirror_k_0.5"), ("lambert_kd_0", "lean"), ("lambert_kd_1", "lean")):
        n = differing(a, b)
        print(a, "against", b, "pixels that differ:", n)
        assert n >= MARGIN, (a, b, n)
    black = runs("lambert_kd_0")[1]
    m = material(black, LAMBERT) & first(black, "SAMPLE_BLACK")
    assert m.sum() >= 20                                   # the Lambert cube: value black, the path ends there
    o, mirrors = runs("deep_facing_mirrors")
    long = int((mirrors["probe"][:, Oracle.SURF_VERTICES] == 5).sum())
    print("deep_facing_mirrors: first vertex on a mirror", int(material(mirrors, MIRROR).sum()), "paths of five vertices", long)
    assert material(mirrors, MIRROR).sum() >= 60 and long >= 40


def test_exactly_zero_cosine(runs):
    """The lamp in the floor's plane.  The reference's fragment position is o + t d, whose y is 0 or -1.2e-7 on this floor: at most
    floor samples dot(n, wi) is exactly 0, getSampleType's `> 0` makes the direction a transmission and the Lambert and the Blinn
    value are black (Blinn::bsdf's `cosi == 0` is never reached); at the rest the cosine is about 1e-7 and the sample is lit."""
    for case in ("in_plane_lambert", "in_plane_blinn"):
        o, run = runs(case)
        floor = on_instance(o, run, case, "floor")
        print(case, "floor samples", int(floor.sum()), "black towards the lamp", int((floor & first(run, "BSDF_BLACK")).sum()))
        zero, tiny = floor & first(run, "BSDF_BLACK"), floor & first(run, "UNOCCLUDED")
        print(case, "of those, lit under a cosine of about 1e-7:", int(tiny.sum()))
        assert zero.sum() >= 40 and zero.sum() + tiny.sum() == floor.sum() and not first(run, "LIGHT_BLACK")[floor].any()
        assert (material(run, BLINN if case.endswith("blinn") else LAMBERT)[floor]).all()
    # and with the lamp 1e-4 above the plane the same samples are lit
    o, near = runs("light_near_floor")
    floor = on_instance(o, near, "light_near_floor", "floor")
    assert (floor & ~first(near, "BSDF_BLACK")).sum() >= 40
    assert differing("in_plane_lambert", "light_near_floor") >= 40 and differing("in_plane_blinn", "in_plane_lambert") >= 40
    assert not np.isnan(runs("light_on_vertex")[1]["li"]).any()


def test_light_inside_a_fragments_epsilon(runs):
    """From 400 units away a fragment's epsilon is 0.4: the wall's fragments within that of the lamp trace a shadow ray of negative
    maxt = dist - epsilon, which nothing occludes -- they are lit, at up to 1 / 0.05^2 of the intensity."""
    o, run = runs("light_inside_epsilon")
    inside = run["probe"][:, Oracle.SURF_INSIDE_EPSILON] > 0
    wall = on_instance(o, run, "light_inside_epsilon", "wall")
    print("light_inside_epsilon: samples whose shadow ray has a negative maxt", int(inside.sum()), "brightest %.3g" % run["li"][inside, :3].max())
    assert inside.sum() >= MARGIN and wall[inside].all() and first(run, "UNOCCLUDED")[inside].all() and not first(run, "OCCLUDED")[inside].any()
    assert (run["li"][inside, :3] > 0).all() and not np.isnan(run["li"]).any()
    assert (runs("lean")[1]["probe"][:, Oracle.SURF_INSIDE_EPSILON] == 0).all()


def test_spot(runs):
    spot = runs("spot")[1]
    got = seen(spot, "SPOT_OUTSIDE", "SPOT_FALLOFF", "SPOT_FULL")
    print("spot", got)
    assert min(got.values()) >= MARGIN
    o = runs("spot")[0]      # the cone's edge and the falloff's start both cross the row: every zone among samples that start on a cube
    cubes = np.isin(o.first_hit(spot["samples"]).view(np.int32)[:, 7], [sc.instance_id("spot", k) for k in sc.ROW])
    on_cubes = {zone: int((cubes & first(spot, zone)).sum()) for zone in got}
    print("spot, among the", int(cubes.sum()), "samples that start on a cube", on_cubes)
    assert min(on_cubes.values()) >= MARGIN, on_cubes
    none, all_, wide = runs("spot_no_falloff")[1], runs("spot_falloff_0")[1], runs("spot_90")[1]
    # falloff_start == theta_max: what the base calls falloff is full; falloff_start 0: what it calls full is falloff
    assert count(none, "SPOT_FALLOFF") == 0 and count(none, "SPOT_FULL") == got["SPOT_FALLOFF"] + got["SPOT_FULL"] and count(none, "SPOT_OUTSIDE") == got["SPOT_OUTSIDE"]
    assert count(all_, "SPOT_FULL") == 0 and count(all_, "SPOT_FALLOFF") == got["SPOT_FALLOFF"] + got["SPOT_FULL"]
    # theta_max 90: nothing below the lamp is outside
    got90 = seen(wide, "SPOT_OUTSIDE", "SPOT_FALLOFF", "SPOT_FULL")
    print("spot_90", got90)
    assert got90["SPOT_OUTSIDE"] == 0 and got90["SPOT_FALLOFF"] >= 100 and got90["SPOT_FULL"] >= MARGIN
    inside = runs("spot_in_glass")[1]       # inside the glass cube: every sample in the cone is shadowed by the cube's own wall
    got = seen(inside, "SPOT_FALLOFF", "SPOT_FULL", "OCCLUDED", "UNOCCLUDED")
    print("spot_in_glass", got)
    assert got["UNOCCLUDED"] == 0 and got["OCCLUDED"] >= MARGIN and got["SPOT_FULL"] >= MARGIN
    for a, b in (("spot_no_falloff", "spot"), ("spot_falloff_0", "spot"), ("spot_90", "lean"), ("wh_spot", "wh")):
        assert differing(a, b) >= MARGIN, (a, b)


def test_area_lights(runs):
    P = Oracle
    quad = runs("quad")[1]
    got = seen(quad, "UNOCCLUDED", "BSDF_BLACK")
    print("quad", got, seen(quad, "OCCLUDED", "END_PICKED"))
    assert min(got.values()) >= MARGIN and count(quad, "EMITTER_BACK") == 0
    behind = runs("quad_behind")[1]         # seen only from behind: every L is black, the frame shows no direct light
    n = len(behind["probe"])
    assert count(behind, "EMITTER_BACK") == n and count(behind, "LIGHT_BLACK") == n and count(behind, "UNOCCLUDED") == 0
    for case in ("quad_edge_on", "disk_edge_on"):     # in the floor's plane: dot(ns, -wi) is exactly 0 from the floor, `> 0` says black
        o, run = runs(case)
        floor = on_instance(o, run, case, "floor")
        edge = floor & first(run, "EMITTER_BACK") & first(run, "LIGHT_BLACK")
        print(case, "floor samples", int(floor.sum()), "that see the emitter edge-on", int(edge.sum()), "pdf 0", int((floor & first(run, "LIGHT_PDF_ZERO")).sum()))
        assert edge.sum() >= 40 and count(run, "UNOCCLUDED") >= MARGIN
    cube = runs("cube_emitter")[1]          # twelve triangles: faces seen from behind and from the front
    got = seen(cube, "EMITTER_BACK", "UNOCCLUDED")
    print("cube_emitter", got)
    assert min(got.values()) >= 40
    d = sc.scene("cube_emitter").desc
    assert d.meshes[d.lights[0].mesh].tri_count == 12
    sphere, around = runs("sphere_emitter")[1], runs("sphere_around")[1]
    assert count(sphere, "SPHERE_INSIDE") == 0 and count(sphere, "UNOCCLUDED") >= 100
    got = seen(around, "SPHERE_INSIDE", "END_PICKED", "UNOCCLUDED")
    print("sphere_around", got)
    assert min(got.values()) >= MARGIN
    disk = runs("disk_emitter")[1]
    assert count(disk, "UNOCCLUDED") >= 100 and count(disk, "EMITTER_BACK") == 0
    # emitters hit by camera rays: Intersection::Le from the front is the radiance, from the back black
    for case, lit in (("emitter_front", True), ("emitter_back", False)):
        o, run = runs(case)
        e = on_emitter(o, run, case)
        le = run["li"][e, 0] >= 4.0
        print(case, "camera samples on the emitter", int(e.sum()), "with Le", int(le.sum()))
        assert e.sum() >= MARGIN and (le.all() if lit else not le.any())
        if not lit:
            assert first(run, "EMITTER_BACK")[e].all()
    two = runs("two_emitters")[1]
    got = seen(two, "END_PICKED", "END_OTHER")
    picked = [int((two["probe"][:, P.SURF_LIGHT] == k + 1).sum()) for k in range(2)]
    print("two_emitters", got, "picked", picked)
    assert min(got.values()) >= MARGIN and min(picked) >= 40
    for a, b in (("quad", "lean"), ("cube_emitter", "quad"), ("sphere_emitter", "quad"), ("disk_emitter", "quad"), ("sphere_around", "sphere_emitter"),
                 ("emitter_front", "emitter_back"), ("wh_quad_4", "wh_quad_1"), ("wh_sphere_4", "wh_quad_4")):
        assert differing(a, b) >= MARGIN, (a, b)


def test_other_lights(runs):
    P = Oracle
    sun = runs("directional")[1]
    assert min(seen(sun, "OCCLUDED", "UNOCCLUDED").values()) >= MARGIN
    for case in ("ibl", "ibl_pole", "wh_ibl_3"):
        run = runs(case)[1]
        got = seen(run, "END_ESCAPED", "ENV_ADDED", "OCCLUDED", "UNOCCLUDED")
        sky = int((run["probe"][:, P.SURF_MATERIAL] == 0).sum())
        print(case, got, "camera samples on the sky", sky)
        assert min(got.values()) >= MARGIN and sky >= 100 and not np.isnan(run["li"]).any()
    assert differing("ibl_pole", "ibl") >= 100
    two = runs("lights_two")[1]["probe"][:, P.SURF_LIGHT]
    assert ((two == 2) | (two == 0)).all() and (two == 2).sum() >= 100                # the powerless light is never picked
    three = runs("lights_three")[1]["probe"][:, P.SURF_LIGHT]
    picked = [int((three == k + 1).sum()) for k in range(3)]
    print("three lights, samples that picked each:", picked)
    assert min(picked) >= MARGIN
    for case in ("lights_none", "wh_none"):
        run = runs(case)[1]
        assert count(run, "UNOCCLUDED") == 0 and count(run, "OCCLUDED") == 0
    assert (sc.golden("lights_none")["film"][..., :3] == 0).all()


def test_shapes(runs):
    """The sphere at its pole, stretched, grazed (its silhouette: camera samples just inside it) and around the camera; the disk
    head-on through its centre and edge-on."""
    o, pole = runs("sphere_pole")
    ball = on_instance(o, pole, "sphere_pole", "ball")
    hit = o.first_hit(pole["samples"])
    centre = np.asarray(sc.BALL_AT)
    towards = (np.asarray(sc.CAMERA_AT) - centre) / np.linalg.norm(np.asarray(sc.CAMERA_AT) - centre)
    cosines = ((hit[ball, 8:11] - centre) / 0.45) @ towards
    print("sphere_pole: samples on the ball", int(ball.sum()), "nearest to the pole: %.2f degrees" % np.degrees(np.arccos(min(1.0, cosines.max()))),
          "within 30 degrees", int((cosines > 0.866).sum()))
    assert ball.sum() >= MARGIN and (cosines > 0.866).sum() >= MARGIN and cosines.max() > np.cos(np.radians(5.0))
    for case, least in (("sphere_stretched", MARGIN), ("sphere_large", 40)):
        o, run = runs(case)
        ball = on_instance(o, run, case, "ball")
        grazed = ball & (np.abs(np.einsum("ij,ij->i", o.first_hit(run["samples"])[:, 4:7], _directions(o, run))) < 0.5)
        print(case, "samples on the ball", int(ball.sum()), "met beyond 60 degrees of incidence", int(grazed.sum()))
        assert ball.sum() >= least and grazed.sum() >= MARGIN, case
    o, shell = runs("camera_in_sphere")
    got = seen(shell, "END_SURFACE", "END_ESCAPED")
    print("camera_in_sphere", got, "first hit on the shell", int(on_instance(o, shell, "camera_in_sphere", "shell").sum()))
    assert got["END_ESCAPED"] == 0 and on_instance(o, shell, "camera_in_sphere", "shell").sum() >= 100
    o, disk = runs("disk_head_on")
    plate = on_instance(o, disk, "disk_head_on", "plate")
    r = np.linalg.norm(o.first_hit(disk["samples"])[plate, 8:11] - np.asarray([0.0, 0.8, 0.5]), axis=1)
    print("disk_head_on: samples on the disk", int(plate.sum()), "nearest to its centre %.3f of radius 0.36" % r.min())
    assert plate.sum() >= MARGIN and r.min() < 0.1
    o, edge = runs("disk_edge_on_camera")
    plate = on_instance(o, edge, "disk_edge_on_camera", "plate")
    print("disk_edge_on_camera: samples on the disk", int(plate.sum()))
    assert plate.sum() <= 24                                           # a line across the frame at most
    assert differing("disk_edge_on_camera", "ext") >= MARGIN and differing("sphere_pole", "ext") >= MARGIN


def _directions(o, run):
    return np.stack([o.camera_ray(float(x), float(y))[3:6] for x, y in run["samples"][:, :2]])


def test_masks(runs):
    """alpha 0: every masked vertex is punched through; 1: none; 0.5: both.  Over Lambert and over glass.  The stacked quads
    attenuate shadow rays twice.  In front of the sky the punched-through camera path adds the environment (the `firstBounce`
    rule); seen in a mirror the same escape adds none."""
    for inner, kind in (("lambert", LAMBERT), ("glass", GLASS)):
        zero, half, full = (runs("mask_%s_%s" % (inner, a))[1] for a in ("0", "0.5", "1"))
        m = [material(r, kind + MASKED) for r in (zero, half, full)]
        got = {"alpha 0 punched": int((m[0] & first(zero, "PUNCHED")).sum()), "alpha 0.5 punched": int((m[1] & first(half, "PUNCHED")).sum()),
               "alpha 0.5 kept": int((m[1] & ~first(half, "PUNCHED")).sum()), "alpha 1 kept": int((m[2] & ~first(full, "PUNCHED")).sum())}
        print("mask over", inner, got)
        assert min(got.values()) >= MARGIN and (first(zero, "PUNCHED")[m[0]]).all() and count(full, "PUNCHED") == 0
        assert (zero["probe"][m[0], Oracle.SURF_MASKED_PROB] == 0).all() and (full["probe"][m[2], Oracle.SURF_MASKED_PROB] == 1).all()
    stacked = runs("mask_stacked")[1]
    assert count(stacked, "ATTENUATED") >= count(runs("deep")[1], "ATTENUATED") + MARGIN and count(stacked, "PUNCHED") >= 40
    sky, mirror = runs("mask_before_sky")[1], runs("mask_behind_mirror")[1]
    early = first(sky, "PUNCHED") & (sky["probe"][:, Oracle.SURF_EARLY_ESCAPE] > 0) & (sky["li"][:, :3] > 0).any(axis=1)
    late = ~first(mirror, "PUNCHED") & material(mirror, MIRROR) & (mirror["probe"][:, Oracle.SURF_LATE_ESCAPE] > 0)
    print("mask_before_sky: punched through to the sky at bounce 0:", int(early.sum()), " mask_behind_mirror: escapes without environment:", int(late.sum()))
    assert early.sum() >= MARGIN and late.sum() >= MARGIN
    wh = runs("wh_mask")[1]
    assert count(wh, "PUNCHED") >= MARGIN and material(wh, LAMBERT + MASKED).sum() >= MARGIN
    for a, b in (("mask_lambert_0", "mask_lambert_0.5"), ("mask_lambert_1", "mask_lambert_0.5"), ("mask_glass_0.5", "mask_lambert_0.5"),
                 ("mask_glass_1", "mask_glass_0.5"), ("mask_stacked", "deep"), ("mask_behind_mirror", "mask_before_sky")):
        assert differing(a, b) >= MARGIN, (a, b)
    assert differing("mask_glass_0", "mask_lambert_0") == 0           # alpha 0: the wrapped material is never asked


def test_cameras_and_integrators(runs):
    for case in ("orthographic", "thinlens"):
        run = runs(case)[1]
        kinds = [int(material(run, k).sum()) for k in (LAMBERT, BLINN, GLASS, MIRROR)]
        assert min(kinds) >= MARGIN and differing(case, "lean") >= 100, (case, kinds)
    ao = runs("ao")[1]
    assert ao["probe"][:, Oracle.SURF_VERTICES].sum() == 0 and (sc.golden("ao")["li"][:, :3] > 0).any(axis=1).sum() >= 100
    for case in ("wh_quad_1", "wh_quad_4", "wh_sphere_4"):
        run = runs(case)[1]
        assert min(seen(run, "OCCLUDED", "UNOCCLUDED", "LEAVING", "TOTAL_REFLECTION").values()) >= MARGIN, case
    one, four = runs("wh_quad_1")[1], runs("wh_quad_4")[1]             # sample_num 4: four light samples per vertex
    n1, n4 = (r["probe"][:, Oracle.SURF_COUNTS + EVENT["OCCLUDED"]] + r["probe"][:, Oracle.SURF_COUNTS + EVENT["UNOCCLUDED"]] for r in (one, four))
    print("wh_quad: shadow rays per sample, sample_num 1: %.2f, 4: %.2f" % (n1.mean(), n4.mean()))
    assert n4.sum() >= 3 * n1.sum()


# ---------------------------------------------------------------------------
# draws no generator gives
# ---------------------------------------------------------------------------
def crafted_probe(runs, case, name):
    o, run = runs(case)
    p, li = o.surface(sc.crafted(o, run["samples"], name))
    return run, {"probe": p, "li": li}


def test_reflect_chance_is_a_strict_bound(runs):
    """TransparentMaterial::sampleBSDF reads `uComponent < reflectChance`: a draw equal to the sample's own reflectChance refracts,
    the float below it reflects, the float above it refracts -- at every glass vertex of the base."""
    base, below = crafted_probe(runs, "lean", "bsdf_comp_below_chance")
    g = material(base, GLASS)
    assert g.sum() >= 20 and (base["probe"][g, Oracle.SURF_REFLECT_CHANCE] > 0).all()
    assert first(below, "REFLECT")[g].all()
    for name in ("bsdf_comp_at_chance", "bsdf_comp_above_chance"):
        _, at = crafted_probe(runs, "lean", name)
        assert first(at, "REFRACT")[g].all() and not first(at, "REFLECT")[g].any(), name
    # and in radiance, where the path goes on (`deep`): the draw at the threshold gives what the float above it gives, bit for bit,
    # and not what the float below it gives
    li = {name: crafted_probe(runs, "deep", "bsdf_comp_%s_chance" % name)[1]["li"] for name in ("below", "at", "above")}
    differ = int((li["at"][:, :3] != li["below"][:, :3]).any(axis=1).sum())
    print("deep: samples whose li differs between a draw at reflectChance and the float below it:", differ)
    assert sc.same_bits(li["at"], li["above"]) and differ >= MARGIN


def test_masked_prob_is_a_strict_bound(runs):
    """MaskMaterial::sampleBSDF reads `uComponent < maskedProb`: equal punches through."""
    base, below = crafted_probe(runs, "mask_lambert_0.5", "bsdf_comp_below_masked")
    m = material(base, LAMBERT + MASKED)
    assert m.sum() >= MARGIN and (base["probe"][m, Oracle.SURF_MASKED_PROB] == 0.5).all()
    assert not first(below, "PUNCHED")[m].any()
    for name in ("bsdf_comp_at_masked", "bsdf_comp_above_masked"):
        _, at = crafted_probe(runs, "mask_lambert_0.5", name)
        assert first(at, "PUNCHED")[m].all(), name
    li = {name: crafted_probe(runs, "mask_lambert_0.5", "bsdf_comp_%s_masked" % name)[1]["li"] for name in ("below", "at", "above")}
    differ = int((li["at"][:, :3] != li["below"][:, :3]).any(axis=1).sum())
    print("mask_lambert_0.5: samples whose li differs between a draw at maskedProb and the float below it:", differ)
    assert sc.same_bits(li["at"], li["above"]) and differ >= MARGIN


def test_light_pick_ends(runs):
    """Scene::sampleLight's `cdf[i] < u` walk: u = 0 ends on light 0 though it has no power (its term is 0 / 0: the samples are NaN
    and dropped), the largest float below 1 on the last light."""
    base, zero = crafted_probe(runs, "lights_two", "pick_0")
    hit = base["probe"][:, Oracle.SURF_MATERIAL] > 0
    assert (zero["probe"][hit, Oracle.SURF_LIGHT] == 1).all() and hit.sum() >= 100
    print("lights_two, light pick 0: NaN samples", int(np.isnan(zero["li"]).any(axis=1).sum()), "of", int(hit.sum()))
    assert np.isnan(zero["li"][hit, :3]).any(axis=1).all()
    o = runs("lights_two")[0]
    assert (o.splat(runs("lights_two")[1]["samples"], zero["li"])[..., 3] == 0).all()          # every sample dropped
    _, last = crafted_probe(runs, "lights_two", "pick_below_1")
    assert (last["probe"][hit, Oracle.SURF_LIGHT] == 2).all()
    for name in ("pick_0", "pick_below_1"):
        _, one = crafted_probe(runs, "lean", name)
        assert sc.same_bits(one["li"], base_li(runs, "lean")), name


def base_li(runs, case):
    return runs(case)[1]["li"]


def test_direction_and_geometry_draws_at_their_ends(runs):
    """BSDF direction draws of 0 and of the largest float below 1 -- Blinn's pow(0, .) and the cosine hemisphere's rim -- and light
    geometry draws of 0: nothing is NaN, and the records differ from the drawn ones where the draws are read."""
    for case, names in sc.CRAFTED_CASES.items():
        for name in names:
            if not name.startswith(("bsdf_dir", "light_geo")) or (case == "lean" and name == "light_geo_0"):     # a point light reads none
                continue
            run, got = crafted_probe(runs, case, name)
            changed = int((got["li"][:, :3] != run["li"][:, :3]).any(axis=1).sum())
            zero_pdf = int(((got["probe"][:, Oracle.SURF_COUNTS + EVENT["SAMPLE_PDF_ZERO"]] > 0)).sum())
            print(case, name, "samples whose li changed", changed, "sampled pdf 0", zero_pdf, "NaN", int(np.isnan(got["li"]).any(axis=1).sum()))
            assert changed >= MARGIN, (case, name)
            assert not np.isnan(got["li"]).any(), (case, name)
