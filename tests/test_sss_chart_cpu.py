"""Subsurface scattering on generated charts (tests/sss_chart.py), host side: the oracle against the compiled reference, and what
the charts' cases actually meet.

Fixtures: tests/golden/sss_<case>.npz, written by the compiled reference (tests/golden/make_sss_golden.py).  The charts' frame makes
a Film pixel one sample's w * Li (asserted below, not assumed), and under the path tracer at max_ray_depth 1 a body sample's Li is
the subsurface term alone (asserted below on the probe's two terms).  Coverage is asserted on the probe (Oracle.subsurface) under the
reference stream's own draws -- the samples the fixtures' li were computed from -- and the counts are printed.

No case was dropped: the compiled reference returns on every one.
"""
import os

import numpy as np
import pytest

import oracle_binding as ob
from goblin_amd import _abi
import sss_chart as sc
from oracle_binding import Oracle
from test_gpu_splat_fastpath import add_samples_f64

SPP1 = list(sc.CASES)
SEED = 0x5EEDC0FFEE
MARGIN = 8           # every coverage count below holds with at least this many samples


@pytest.fixture(scope="module")
def runs():
    """Per case, once: the oracle's render under the reference stream, with the probe's records of the same samples."""
    cache = {}

    def get(case):
        if case not in cache:
            o = Oracle(sc.scene(case))
            run = o.render(threads=1, want_samples=True)
            run["probe"], run["probe_li"] = o.subsurface(run["samples"])
            cache[case] = (o, run)
        return cache[case]
    return get


def count(run, word, where=None):
    """The number of camera samples with a non-zero probe word (among `where`)."""
    hit = run["probe"][:, word] > 0
    return int((hit if where is None else hit & where).sum())


def body(run):
    return run["probe"][:, Oracle.SSS_CALLS] > 0


# ---------------------------------------------------------------------------
# the oracle is the compiled reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.ALL_CASES)
def test_oracle_is_the_reference(runs, case):
    """Same stream, Li bit for bit with NaN positions equal, every Film accumulator bit for bit, no NaN in a Film."""
    g, run = sc.golden(case), runs(case)[1]
    assert np.array_equal(run["samples"][:, :4], g["samples"])
    assert sc.same_bits(run["li"], g["li"]), sc.sample_report(case, "oracle against reference", run["li"], g["li"], run["samples"])
    assert not np.isnan(g["film"]).any() and not np.isnan(run["film"]).any()
    assert np.array_equal(run["film"].view(np.uint32), g["film"].view(np.uint32)), sc.film_report(case, run["film"], g["film"])


@pytest.mark.skipif(not os.path.exists(ob.REF_HARNESS), reason="needs the compiled reference (oracle/_ref/ref_harness)")
@pytest.mark.parametrize("case", sc.ALL_CASES)
def test_fixture_is_what_the_reference_gives_now(tmp_path, case):
    """The harness run again gives exactly the committed fixture, byte for byte: a fixture gone stale against sss_chart.py fails."""
    import sys
    sys.path.insert(0, sc.GOLDEN_DIR)
    try:
        import make_sss_golden as mg
    finally:
        sys.path.remove(sc.GOLDEN_DIR)
    live, kept = mg.run_case(case, str(tmp_path)), sc.golden(case)
    for k in ("film", "samples", "li"):
        assert live[k].shape == kept[k].shape and np.array_equal(live[k].view(np.uint32), kept[k].view(np.uint32)), (case, k)
    mg.save(str(tmp_path / "again.npz"), live)
    with open(tmp_path / "again.npz", "rb") as a, open(os.path.join(sc.GOLDEN_DIR, "sss_" + case + ".npz"), "rb") as b:
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
    """The probe's li is li_replay's and the render's; under the path tracer at depth 1 a body sample's radiance is
    float32(single + multi) of the probe's two terms and every other sample is black: Li = Le + Lsubsurface there."""
    o, run = runs(case)
    li, _ = o.li_replay(run["samples"])
    assert sc.same_bits(run["probe_li"], li) and sc.same_bits(li, run["li"])
    rs = sc.doc(case)["render_setting"]
    if rs["render_method"] == "path_tracing" and rs["max_ray_depth"] == 1:
        p, b = run["probe"], body(run)
        assert sc.same_bits(li[b, :3], p[b, Oracle.SSS_SINGLE] + p[b, Oracle.SSS_MULTI]), case
        if "ibl" not in case:
            assert (li[~b, :3] == 0).all()


def test_native_draws_meet_the_same_edges(runs):
    """The device tests run the native sampler's records: the bases meet every axis and outcome under those too."""
    for case in ("pt", "wh"):
        o = runs(case)[0]
        p, _ = o.subsurface(o.native_samples(SEED))
        for word in (Oracle.SSS_AXIS_N, Oracle.SSS_AXIS_U, Oracle.SSS_AXIS_V, Oracle.SSS_PROBE_MISS, Oracle.SSS_PROBE_OTHER, Oracle.SSS_PROBE_OCCLUDED,
                     Oracle.SSS_PROBE_ACCEPTED, Oracle.SSS_SINGLE_OCCLUDED, Oracle.SSS_SINGLE_ACCEPTED):
            assert (p[:, word] > 0).sum() >= MARGIN, (case, word)


# ---------------------------------------------------------------------------
# the charts test something: what the probe saw, under the stream's draws
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["pt", "wh"])
def test_bases_meet_every_axis_and_outcome(runs, case):
    run = runs(case)[1]
    seen = {name: count(run, getattr(Oracle, "SSS_" + name)) for name in
            ("AXIS_N", "AXIS_U", "AXIS_V", "PROBE_MISS", "PROBE_OTHER", "PROBE_OCCLUDED", "PROBE_ACCEPTED", "SINGLE_OCCLUDED", "SINGLE_ACCEPTED")}
    print(case, "body samples %d of %d:" % (body(run).sum(), len(run["probe"])), seen)
    assert 0.2 <= body(run).mean() <= 0.45
    assert min(seen.values()) >= MARGIN, (case, seen)
    assert not np.isnan(run["li"]).any()


def test_whitted_base_evaluates_the_term_below_the_first_level(runs):
    """Through the mirror and through the glass pane: camera samples whose first hit is either and whose Lsubsurface ran at a
    recursion level above 0; on the cube itself it runs at level 0."""
    o, run = runs("wh")
    first = o.first_hit(run["samples"]).view(np.int32)[:, 7]
    deep = run["probe"][:, Oracle.SSS_CALLS_DEEP] > 0
    seen = {name: int((deep & (first == sc.instance_id("wh", name))).sum()) for name in ("mirror", "pane")}
    level0 = int(((first == sc.instance_id("wh", "body")) & (run["probe"][:, Oracle.SSS_FIRST_LEVEL] == 0) & body(run)).sum())
    print("wh: term below level 0 behind", seen, "at level 0 on the cube", level0)
    assert min(seen.values()) >= MARGIN and level0 >= MARGIN
    # max_ray_depth 12 (GBL_WHITTED_MAX_DEPTH) behind twelve clear panes: the term is evaluated at level 12, the last frame
    run12 = runs("wh_depth_12")[1]
    last = int((run12["probe"][:, Oracle.SSS_MAX_LEVEL] == 12).sum())
    print("wh_depth_12: samples whose term ran at level 12:", last)
    assert last >= MARGIN and run12["probe"][:, Oracle.SSS_MAX_LEVEL].max() == 12
    assert count(runs("wh_depth_1")[1], Oracle.SSS_CALLS_DEEP) >= MARGIN     # depth 1 still follows one specular bounce (depth < max_ray_depth)


@pytest.mark.parametrize("name", [n for n in sc.CRAFTED if n.startswith("axis")])
def test_axis_thresholds_include_their_value(runs, name):
    """BSSRDF::sampleProbeRay (GoblinMaterial.cpp:141,147) reads `uPickAxis <= 0.5f` and `<= 0.75f`: records whose every axis pick
    is the threshold itself take N and U, one ulp above U and V."""
    o, run = runs("pt")
    p, _ = o.subsurface(sc.crafted(o, run["samples"], name))
    b = p[:, Oracle.SSS_CALLS] > 0
    word = {"N": Oracle.SSS_AXIS_N, "U": Oracle.SSS_AXIS_U, "V": Oracle.SSS_AXIS_V}[sc.CRAFTED[name][2]]
    assert b.sum() >= 40 and (p[b, word] == 4).all(), name


def test_light_pick_of_zero_stops_at_the_first_light(runs):
    """Scene::sampleLight's `cdf[i] < u` walk with u = 0 ends on light 0 even where it has no power."""
    o, run = runs("pt_light_two")
    p, li = o.subsurface(sc.crafted(o, run["samples"], "light_0"))
    b = p[:, Oracle.SSS_CALLS] > 0
    assert b.sum() >= 40 and (p[b, Oracle.SSS_LIGHTS] == 1).all()
    print("pt_light_two, light pick 0: NaN samples", int(np.isnan(li).any(axis=1).sum()), "of", int(b.sum()))


def test_partial_tiles(runs):
    run = runs("pt_partial_tiles")[1]
    assert sc.golden("pt_partial_tiles")["film"].shape == (13, 21, 4) and body(run).sum() >= 40


def test_bodies(runs):
    P = Oracle
    thin, eps, base = runs("pt_slab_thin")[1], runs("pt_slab_epsilon")[1], runs("pt")[1]
    seen = {"thin accepted": count(thin, P.SSS_PROBE_ACCEPTED), "thin occluded": count(thin, P.SSS_PROBE_OCCLUDED),
            "epsilon body": int(body(eps).sum()), "epsilon accepted": count(eps, P.SSS_PROBE_ACCEPTED), "epsilon occluded": count(eps, P.SSS_PROBE_OCCLUDED)}
    print(seen)
    # a slab thinner than rmax still returns probes on all three axes; one thinner than a fragment's epsilon shadows every probe
    # point from the far side: its own other face lies inside the shadow ray's epsilon or just beyond it
    assert seen["thin accepted"] >= MARGIN and seen["epsilon body"] >= 40 and seen["epsilon occluded"] >= 40
    for case in ("pt_sphere_pole", "pt_disk", "pt_bunny", "pt_stretched", "pt_peg"):
        run = runs(case)[1]
        got = [count(run, w) for w in (P.SSS_AXIS_N, P.SSS_AXIS_U, P.SSS_AXIS_V, P.SSS_PROBE_ACCEPTED, P.SSS_PROBE_MISS)]
        print(case, "body %d, N U V accepted missed:" % body(run).sum(), got)
        assert body(run).sum() >= 40 and min(got) >= MARGIN, (case, got)
        assert not np.isnan(run["li"]).any(), case
    disk = runs("pt_disk")[1]            # an open surface: the single-scatter point lies behind nothing, its exit finds no surface
    assert count(disk, P.SSS_SINGLE_MISS) + count(disk, P.SSS_SINGLE_OTHER) + count(disk, P.SSS_SINGLE_ACCEPTED) >= 40
    peg = runs("pt_peg")[1]              # the peg takes probes the base's cube received
    more = (peg["probe"][:, P.SSS_PROBE_OTHER] > base["probe"][:, P.SSS_PROBE_OTHER]).sum()
    print("pt_peg: samples with more probes on another material than the base", int(more))
    assert more >= MARGIN
    huge = runs("pt_huge")[1]
    print("pt_huge: body", int(body(huge).sum()), "other", count(huge, P.SSS_PROBE_OTHER), "accepted", count(huge, P.SSS_PROBE_ACCEPTED))
    assert body(huge).sum() >= 200 and count(huge, P.SSS_PROBE_OTHER) == 0 and count(huge, P.SSS_PROBE_ACCEPTED) >= 100


def test_material_identity(runs):
    """The neighbour of the same model and material counts; the neighbour of another material is rejected, and so is the neighbour
    whose material is a separate entry with identical parameters (the reference compares BSSRDF objects): both show as probes and
    single-scatter exits on `another material` that the same-material twins do not have, and as a different Film."""
    P = Oracle
    same, other, equal, base = (runs(c)[1] for c in ("pt_twins_same", "pt_twins_other", "pt_twins_equal", "pt"))
    assert np.array_equal(same["samples"], other["samples"]) and np.array_equal(same["samples"], equal["samples"])
    for name, run in (("pt_twins_other", other), ("pt_twins_equal", equal)):
        more = int((run["probe"][:, P.SSS_PROBE_OTHER] > same["probe"][:, P.SSS_PROBE_OTHER]).sum())
        differ = int((run["li"][:, :3] != same["li"][:, :3]).any(axis=1).sum())
        print(name, "samples with more rejected probes than pt_twins_same:", more, "samples whose li differs:", differ)
        assert more >= MARGIN and differ >= MARGIN, name
    # two instances of one material are one body: as many accepted probes as the undivided cube, within the seam's few
    a, b = count(same, P.SSS_PROBE_ACCEPTED), count(base, P.SSS_PROBE_ACCEPTED)
    print("accepted probes: twins of one material", a, "the base's one cube", b)
    assert abs(a - b) <= MARGIN and count(same, P.SSS_PROBE_ACCEPTED) >= count(equal, P.SSS_PROBE_ACCEPTED)
    # the loader keeps equal materials apart
    s = sc.scene("pt_twins_equal").desc
    sub = [i for i in range(s.num_materials) if s.materials[i].type == _abi.GBL_MAT_SUBSURFACE]
    assert len(sub) == 2
    used = {s.instances[i].material for i in range(s.num_instances)}
    assert set(sub) <= used


def test_coefficients(runs):
    P = Oracle
    base = runs("pt")[1]
    dense, clear = runs("pt_dense")[1], runs("pt_clear")[1]
    # dense: rmax = sqrt(log(100) / sigma_tr) is 0.06 where the base's is 0.46 -- far fewer probes leave the cube for the floor
    print("probes on another material: dense", count(dense, P.SSS_PROBE_OTHER), "base", count(base, P.SSS_PROBE_OTHER))
    assert count(dense, P.SSS_PROBE_OTHER) + MARGIN <= count(base, P.SSS_PROBE_OTHER) and count(dense, P.SSS_PROBE_ACCEPTED) >= 40
    # nearly clear: rmax exceeds the scene, every probe starts outside every object and returns nothing of the body's
    b = body(clear)
    print("clear: body", int(b.sum()), "accepted", count(clear, P.SSS_PROBE_ACCEPTED), "missed", count(clear, P.SSS_PROBE_MISS))
    assert b.sum() >= 40 and count(clear, P.SSS_PROBE_ACCEPTED) == 0 and count(clear, P.SSS_PROBE_MISS, b) == b.sum()
    # zero absorb: sigma_tr 0, rmax infinite, the probe ray NaN -- every probe of every body sample misses, nothing is NaN
    zero = runs("pt_absorb_zero")[1]
    b = body(zero)
    slots = zero["probe"][b, P.SSS_AXIS_N] + zero["probe"][b, P.SSS_AXIS_U] + zero["probe"][b, P.SSS_AXIS_V]
    print("absorb zero: body", int(b.sum()), "NaN samples", int(np.isnan(zero["li"]).any(axis=1).sum()))
    assert b.sum() >= 40 and np.array_equal(zero["probe"][b, P.SSS_PROBE_MISS], slots) and (slots == 4).all()
    assert (zero["probe"][:, P.SSS_NAN] == 0).all() and not np.isnan(zero["li"]).any()
    assert (zero["probe"][b, P.SSS_MULTI] == 0).all() and (zero["probe"][b, P.SSS_SINGLE] > 0).any(axis=1).sum() >= 40
    for case in ("pt_absorb_zero_r", "pt_scatter_zero", "pt_coloured", "pt_checker_scatter", "pt_image_absorb", "wh_image_absorb"):
        run = runs(case)[1]
        assert not np.isnan(run["li"]).any() and count(run, P.SSS_PROBE_ACCEPTED) >= 40, case
    # a check edge through the visible faces, an image across them: the exit fragment (mi) and the probe fragment (mp) resolve
    # other coefficients than the shaded fragment (mo) does; with constant textures they never do
    for case in ("pt_checker_scatter", "pt_image_absorb", "wh_image_absorb"):
        run = runs(case)[1]
        seen = (count(run, P.SSS_MI_DIFFERS), count(run, P.SSS_MP_DIFFERS))
        print(case, "samples with a slot whose mi / mp differs from mo:", seen)
        assert min(seen) >= MARGIN, (case, seen)
    assert count(base, P.SSS_MI_DIFFERS) == 0 and count(base, P.SSS_MP_DIFFERS) == 0
    zero_r = runs("pt_absorb_zero_r")[1]
    assert ((zero_r["li"][:, 0] > 0) & (zero_r["li"][:, 1] > 0)).sum() >= 40
    no_scatter = runs("pt_scatter_zero")[1]       # no single scattering and alpha' = 0: the term is black
    assert (no_scatter["li"][body(no_scatter), :3] == 0).all()


def test_films_that_must_differ():
    def differing(a, b):
        fa, fb = sc.golden(a)["film"], sc.golden(b)["film"]
        lit = (fa[..., :3] != 0).any(axis=-1) | (fb[..., :3] != 0).any(axis=-1)
        return int(((fa != fb).any(axis=-1) & lit).sum())
    pairs = [("pt_g_0.001", "pt_g_0.0009"), ("pt_g_0.0011", "pt_g_0.001"), ("pt_g_0.6", "pt_g_-0.6"), ("pt_g_0.95", "pt_g_0.6"),
             ("pt_index_1", "pt_index_1.0001"), ("pt_index_1.5", "pt"), ("pt_index_2.4", "pt"), ("pt_checker_scatter", "pt"), ("pt_image_absorb", "pt"),
             ("pt_kr", "pt_depth_6"), ("pt_coloured", "pt"), ("pt_samples_1", "pt"), ("pt_samples_5", "pt"), ("pt_samples_10", "pt_samples_5"),
             ("pt_kd_0", "pt_kd_mixed"), ("pt_kd_0.999", "pt_kd_mixed"), ("pt_kd_mfp_1e-4", "pt_kd_mfp_1e3"), ("pt_twins_other", "pt_twins_equal"),
             ("wh_depth_1", "wh"), ("pt_depth_6", "pt"), ("pt_thinlens", "pt"), ("pt_light_two", "pt_light_three")]
    for a, b in pairs:
        n = differing(a, b)
        print(a, "against", b, "pixels that differ:", n)
        assert n >= 40, (a, b, n)
    # only an accepted probe across the seam tells equal materials from one material: the pixels beside the seam
    n = differing("pt_twins_equal", "pt_twins_same")
    print("pt_twins_equal against pt_twins_same pixels that differ:", n)
    assert n >= MARGIN
    # 10 and 16 both become 16 slots; 2 becomes the base's 4; Kd 0.999 already lies above diffuseReflectance at the last alpha' sixteen halvings reach
    # (0.98 at 1 - 2^-17), so it ends at the upper bracket as Kd 1 does
    for a, b in (("pt_samples_16", "pt_samples_10"), ("pt_samples_2", "pt"), ("pt_kd_0.999", "pt_kd_1")):
        assert differing(a, b) == 0, (a, b)


def test_g_threshold(runs):
    """`g < 1e-3` compares the float g with the double 1e-3: float(0.0009) is below, float(0.001) = 0.00100000005 and float(0.0011)
    are not, every negative g is below.  Each case has single-scatter exits that are accepted -- the phase function is evaluated --
    and the fixtures, which every device test is held to bit for bit, differ pairwise across the threshold
    (test_films_that_must_differ)."""
    assert np.float32(0.0009) < 1e-3 and not (np.float32(0.001) < 1e-3) and not (np.float32(0.0011) < 1e-3)
    for case in sc.G_CASES:
        run = runs(case)[1]
        assert count(run, Oracle.SSS_SINGLE_ACCEPTED) >= 40 and not np.isnan(run["li"]).any(), case


def test_index(runs):
    """index 1: Fresnel reflectance 0 and et = 1, nothing degenerate.  index 0.8: both loaders take it, and where the refracted cosine
    has no real value the single term is NaN -- ImageTile::addSample drops exactly those samples."""
    for case in ("pt_index_1", "pt_index_1.0001", "pt_index_1.5", "pt_index_2.4"):
        assert not np.isnan(runs(case)[1]["li"]).any(), case
    run, g = runs("pt_index_0.8")[1], sc.golden("pt_index_0.8")
    nan = np.isnan(g["li"][:, :3]).any(axis=1)
    print("index 0.8: NaN samples", int(nan.sum()), "of", int(body(run).sum()), "body samples")
    assert nan.sum() >= MARGIN and (body(run) & ~nan).sum() >= MARGIN and not (nan & ~body(run)).any()
    assert np.array_equal(nan, (run["probe"][:, Oracle.SSS_NAN].astype(np.int64) & 1) != 0)
    x, y = np.floor(g["samples"][:, 0]).astype(int), np.floor(g["samples"][:, 1]).astype(int)
    inside = (x >= 0) & (x < 24) & (y >= 0) & (y < 16)
    dropped = np.zeros((16, 24), bool)
    dropped[y[nan & inside], x[nan & inside]] = True
    assert np.array_equal(g["film"][..., 3] == 0, dropped) and dropped.sum() >= MARGIN


def kd_to_coefficients(kd, mean_free_path, eta):
    """BSSRDF::convertFromDiffuse in float32 numpy: 16 bisection steps on alpha' per channel."""
    f = np.float32
    eta = f(eta)
    fdr = f(-1.4399) / (eta * eta) + f(0.7099) / eta + f(0.6681) + f(0.0636) * eta if eta >= 1 else \
        f(-0.4399) + f(0.7099) / eta - f(0.3319) / (eta * eta) + f(0.0636) / (eta * eta * eta)
    A = (f(1) + fdr) / (f(1) - fdr)
    absorb, scatter = np.zeros(3, f), np.zeros(3, f)
    for i in range(3):
        sigma_tr = f(1) / f(mean_free_path[i])
        lo, hi = f(0), f(1)
        for _ in range(16):
            mid = f(0.5) * (lo + hi)
            sq = np.sqrt(f(3) * (f(1) - mid))
            rd = f(0.5) * mid * (f(1) + np.exp(-(f(4) / f(3)) * A * sq)) * np.exp(-sq)
            if rd > f(kd[i]):
                hi = mid
            else:
                lo = mid
        alpha = f(0.5) * (lo + hi)
        sigma_tp = sigma_tr / np.sqrt(f(3) * (f(1) - alpha))
        scatter[i] = alpha * sigma_tp
        absorb[i] = sigma_tp - scatter[i]
    return absorb, scatter


@pytest.mark.parametrize("name", list(sc.KD_CASES))
def test_kd_conversion(runs, name):
    """The loader's material table against the float32 restatement, bit for bit.  Kd 0 ends at the lower bracket (alpha' = 2^-17),
    Kd 1 at the upper one (1 - 2^-17)."""
    s = sc.scene("pt_" + name).desc
    m = next(s.materials[i] for i in range(s.num_materials) if s.materials[i].type == _abi.GBL_MAT_SUBSURFACE)
    kd, mfp = sc.KD_CASES[name]
    absorb, scatter = kd_to_coefficients(kd, mfp, sc.KD_INDEX)
    got_a, got_s = np.array(list(m.color), np.float32), np.array(list(m.color2), np.float32)
    print(name, "absorb", got_a.tolist(), "scatter_prime", got_s.tolist())
    assert np.array_equal(got_a, absorb) and np.array_equal(got_s, scatter), (name, got_a, absorb, got_s, scatter)
    alpha = got_s / (got_s + got_a)
    for i in range(3):
        if kd[i] == 0.0:
            assert abs(alpha[i] - 2.0 ** -17) < 1e-7
        if kd[i] == 1.0:
            assert abs(alpha[i] - (1 - 2.0 ** -17)) < 1e-6
    run = runs("pt_" + name)[1]
    assert body(run).sum() >= 40 and not np.isnan(run["li"]).any()


def test_lights(runs):
    P = Oracle
    inside = runs("pt_light_point_in")[1]       # the lamp inside the cube: no single-scatter shadow ray reaches a surface, every probe point is lit
    b = body(inside)
    print("point light inside: single exits missed on", count(inside, P.SSS_SINGLE_MISS, b), "of", int(b.sum()), "accepted probes", count(inside, P.SSS_PROBE_ACCEPTED))
    assert count(inside, P.SSS_SINGLE_MISS, b) >= b.sum() - MARGIN and count(inside, P.SSS_PROBE_ACCEPTED) >= 40 and count(inside, P.SSS_PROBE_OCCLUDED) == 0
    spot = runs("pt_light_spot")[1]             # the cone's edge crosses the body: black and non-black light samples, in both terms
    seen = [count(spot, w) for w in (P.SSS_PROBE_BLACK, P.SSS_PROBE_ACCEPTED, P.SSS_SINGLE_BLACK, P.SSS_SINGLE_ACCEPTED)]
    print("spot: probe black / accepted, single black / accepted:", seen)
    assert min(seen) >= MARGIN
    for case in ("pt_light_directional", "pt_light_quad", "pt_light_sphere", "pt_light_disk", "pt_light_ibl", "wh_light_quad"):
        run = runs(case)[1]
        seen = [count(run, w) for w in (P.SSS_PROBE_ACCEPTED, P.SSS_PROBE_OCCLUDED, P.SSS_SINGLE_ACCEPTED, P.SSS_SINGLE_OCCLUDED)]
        print(case, "probe accepted / occluded, single accepted / occluded:", seen)
        assert min(seen) >= MARGIN and not np.isnan(run["li"]).any(), case
    two = runs("pt_light_two")[1]["probe"][:, P.SSS_LIGHTS].astype(np.int64)
    assert ((two & 1) == 0).all() and ((two & 2) != 0).sum() >= 40             # the powerless light is never picked
    three = runs("pt_light_three")[1]["probe"][:, P.SSS_LIGHTS].astype(np.int64)
    picked = [int(((three >> k) & 1).sum()) for k in range(3)]
    print("three lights, samples that picked each:", picked)
    assert min(picked) >= MARGIN
    for case in ("pt_light_none", "wh_light_none"):                               # no lights: the term is not evaluated, the frame is black
        run = runs(case)[1]
        assert not body(run).any() and (run["li"][:, :3] == 0).all() and (sc.golden(case)["film"][..., :3] == 0).all()


def test_sample_counts(runs):
    """roundToSquare: 1, 2, 5, 10, 16 -> 1, 4, 9, 16, 16 slots per evaluation."""
    for n, slots in ((1, 1), (2, 4), (5, 9), (10, 16), (16, 16)):
        run = runs("pt_samples_%d" % n)[1]
        p, b = run["probe"], body(run)
        assert b.sum() >= 40 and (p[b, Oracle.SSS_AXIS_N] + p[b, Oracle.SSS_AXIS_U] + p[b, Oracle.SSS_AXIS_V] == slots).all(), n
    wh = runs("wh_samples_5")[1]["probe"]
    b = wh[:, Oracle.SSS_CALLS] > 0
    assert (wh[b, Oracle.SSS_AXIS_N] + wh[b, Oracle.SSS_AXIS_U] + wh[b, Oracle.SSS_AXIS_V] == 9 * wh[b, Oracle.SSS_CALLS]).all()
    assert sc.golden("box_pt_spp_4")["li"].shape[0] == 4 * sc.golden("pt")["li"].shape[0]


def test_integrators_and_cameras(runs):
    """The term is added once, at the first vertex, whatever the path's length; AO has none."""
    deep, ao = runs("pt_depth_6")[1], runs("pt_ao")[1]
    b = body(deep)
    assert b.sum() >= 40 and (deep["probe"][b, Oracle.SSS_CALLS] == 1).all()
    assert not body(ao).any()
    for case in ("pt_orthographic", "pt_thinlens", "wh_orthographic"):
        run = runs(case)[1]
        assert body(run).sum() >= 40 and count(run, Oracle.SSS_PROBE_ACCEPTED) >= 40, case
