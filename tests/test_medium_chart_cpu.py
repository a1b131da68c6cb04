"""The participating medium on generated charts (tests/medium_chart.py), host side: the oracle against the compiled reference.

With a medium present the compiled reference's probes log Li while the tile receives tr * L + Lv, so per-sample records cannot pin the
medium.  The charts' frame makes the Film do it: one sample per pixel under a box filter of half a pixel, so that a Film pixel is one
sample's w * (tr * L + Lv) bit for bit (asserted below, not assumed).  Fixtures: tests/golden/medium_<case>.npz, written by the
compiled reference (tests/golden/make_medium_golden.py).
"""
import os

import numpy as np
import pytest

import medium_chart as mc
import oracle_binding as ob
from oracle_binding import Oracle
from test_gpu_splat_fastpath import add_samples_f64

SPP1 = list(mc.CASES)
SEED = 0x5EEDC0FFEE


@pytest.fixture(scope="module")
def runs():
    """Per case, once: the oracle's render with the medium probe along, under the stream's own draws."""
    cache = {}

    def get(case):
        if case not in cache:
            o = Oracle(mc.scene(case))
            cache[case] = (o, o.render_medium())
        return cache[case]
    return get


def flags(run):
    return run["medium"][:, 7].astype(np.int64)


@pytest.mark.parametrize("case", mc.ALL_CASES)
def test_oracle_film_is_the_reference_film(case):
    """Oracle.render(threads=1) against the compiled reference's Film: every accumulator bit for bit, and no NaN in a Film."""
    ref = mc.golden(case)["film"]
    film = Oracle(mc.scene(case)).render(threads=1)["film"]
    assert not np.isnan(ref).any() and not np.isnan(film).any()
    assert np.array_equal(film.view(np.uint32), ref.view(np.uint32)), mc.pixel_report(case, film, ref)


@pytest.mark.skipif(not os.path.exists(ob.REF_HARNESS), reason="needs the compiled reference (oracle/_ref/ref_harness)")
@pytest.mark.parametrize("case", mc.ALL_CASES)
def test_fixture_is_what_the_reference_gives_now(tmp_path, case):
    """The harness run again gives exactly the committed fixture: a fixture gone stale against medium_chart.py fails here."""
    import sys
    sys.path.insert(0, mc.GOLDEN_DIR)
    try:
        import make_medium_golden as mg
    finally:
        sys.path.remove(mc.GOLDEN_DIR)
    live, kept = mg.run_case(case, str(tmp_path)), mc.golden(case)
    for k in ("film", "samples", "li"):
        assert live[k].shape == kept[k].shape and np.array_equal(live[k].view(np.uint32), kept[k].view(np.uint32)), (case, k)


@pytest.mark.parametrize("case", SPP1)
def test_a_film_pixel_is_one_sample(runs, case):
    """No pixel has more than two addends (decided by the float32 footprint rule of ImageTile::addSample on the reference's own
    image positions), so float addition's order cannot matter; and every pixel is float32(w * (tr * L + Lv)) with L the reference's
    logged Li and tr, Lv the oracle's medium probe under the stream's draws."""
    g = mc.golden(case)
    o, run = runs(case)
    scene = mc.scene(case)
    n = g["samples"].shape[0]
    count, cells = add_samples_f64(scene, np.ones(256, np.float32), g["samples"][:, :2], np.ones((n, 4), np.float32))
    assert count[..., 3].max() <= 2, (case, count[..., 3].max())
    assert (count[..., 3] >= 1).all() and cells >= 24 * 16
    assert np.array_equal(run["samples"][:, :4], g["samples"])          # the same stream
    assert mc.same_bits(run["li"], g["li"])
    m, L = run["medium"], g["li"]
    out = np.empty((n, 4), np.float32)
    out[:, :3] = (m[:, 0:3] * L[:, :3]).astype(np.float32) + m[:, 3:6]  # float32 product, then float32 sum: RenderTask::run
    out[:, 3] = L[:, 3]
    film = o.splat(np.ascontiguousarray(g["samples"]), out)
    assert np.array_equal(film.view(np.uint32), g["film"].view(np.uint32)), mc.pixel_report(case, film, g["film"])


@pytest.mark.parametrize("case", mc.ALL_CASES)
def test_li_replay_is_tr_L_plus_Lv(case):
    """Under the hashed draws of the replay and native samplers: li_replay == float32(tr * L + Lv), tr and Lv from Oracle.medium,
    L from the same replay of the scene without its `volume` block.  Bit for bit, NaN positions equal."""
    o, clear = Oracle(mc.scene(case)), Oracle(mc.scene(case, clear=True))
    samples = o.native_samples(SEED)
    assert clear.dims() == o.dims()
    li, _ = o.li_replay(samples)
    L, _ = clear.li_replay(samples)
    m = o.medium(samples)
    want = (m[:, 0:3] * L[:, :3]).astype(np.float32) + m[:, 3:6]
    assert mc.same_bits(li[:, :3], want), case
    assert np.array_equal(li[:, 3], L[:, 3])


# ---------------------------------------------------------------------------
# the charts test something: what the probe saw, under the stream's draws
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.ALL_CASES)
def test_crossing_and_missing_samples(runs, case):
    f = flags(runs(case)[1])
    cross = (f & Oracle.MEDIUM_CROSSES) != 0
    if case.endswith("_behind"):
        assert not cross.any() and ((f & Oracle.MEDIUM_CLIPPED) != 0).all()     # every ray ends on the wall or the floor
    elif case.endswith("_inside"):
        assert cross.all()
    else:
        assert cross.sum() >= 40 and (~cross).sum() >= 40, (case, cross.sum(), (~cross).sum())


@pytest.mark.parametrize("case", ["hom_clipped", "het_clipped"])
def test_clipped_rays_end_inside_the_region(runs, case):
    f = flags(runs(case)[1])
    assert ((f & Oracle.MEDIUM_ENDS_INSIDE) != 0).sum() >= 30


@pytest.mark.parametrize("case", ["hom_thin", "het_thin"])
def test_thin_region_lies_on_both_sides_of_the_early_out(runs, case):
    f = flags(runs(case)[1])
    cross, thin = (f & Oracle.MEDIUM_CROSSES) != 0, (f & Oracle.MEDIUM_THIN) != 0
    assert not (thin & ~cross).any()
    assert thin.sum() >= 10 and (cross & ~thin).sum() >= 10, (thin.sum(), (cross & ~thin).sum())


def test_march_length_sets_the_number_of_draws(runs):
    """A step longer than the region: the transmittance's jitter and Lv's, then no sample point (2 draws) or one -- pick, three
    LightSample numbers and, unoccluded, the shadow ray's jitter (6 or 7).  One cell: tens.  diagonal / 200: hundreds."""
    draws = {}
    for case in ("het_step_long", "het_step_cell", "het_step_fine"):
        run = runs(case)[1]
        draws[case] = run["medium"][(flags(run) & Oracle.MEDIUM_CROSSES) != 0, 6].astype(np.int64)
    assert set(draws["het_step_long"]) <= {2, 6, 7} and 2 in draws["het_step_long"] and draws["het_step_long"].max() >= 6
    assert 10 <= draws["het_step_cell"].max() < 100
    assert draws["het_step_fine"].max() >= 300
    for case in mc.CASES:          # a sample that misses draws the heterogeneous transmittance's nothing: it returns before the jitter
        run = runs(case)[1]
        assert (run["medium"][(flags(run) & Oracle.MEDIUM_CROSSES) == 0, 6] == 0).all(), case


def test_films_that_must_differ():
    def crossing(a, b):
        """Pixels that differ, among those neither Film leaves black (a sample that misses a heterogeneous region is black)."""
        fa, fb = mc.golden(a)["film"], mc.golden(b)["film"]
        lit = (fa[..., :3] != 0).any(axis=-1) & (fb[..., :3] != 0).any(axis=-1)
        return ((fa != fb).any(axis=-1) & lit).sum()
    # grid_eval's index scale is normalize * n - 0.5: for n = 1 the scale halves, a 1x1x1 grid is not a homogeneous region
    assert crossing("het_grid_1x1x1", "hom") >= 40
    assert crossing("hom_g_0.6", "hom_g_-0.6") >= 40 and crossing("het_g_0.6", "het_g_-0.6") >= 40
    for a in ("het_grid_2x1x1", "het_grid_1x1x8", "het_grid_5x3x2", "het_grid_16x16x16", "het_step_long", "het_step_cell", "het_step_fine"):
        assert crossing(a, "het") >= 40, a


def test_clear_medium_samples_are_dropped(runs):
    """Zero attenuation: 0 / 0 in the distance sampling, NaN Lv on every crossing sample, and ImageTile::addSample drops exactly
    those -- their pixels have weight 0 in the reference's Film."""
    run, g = runs("hom_clear")[1], mc.golden("hom_clear")
    cross = (flags(run) & Oracle.MEDIUM_CROSSES) != 0
    nan = np.isnan(run["medium"][:, 3:6]).any(axis=1)
    assert cross.sum() >= 40 and np.array_equal(nan, cross)
    x, y = np.floor(g["samples"][:, 0]).astype(int), np.floor(g["samples"][:, 1]).astype(int)
    inside = (x >= 0) & (x < 24) & (y >= 0) & (y < 16)
    dropped = np.zeros((16, 24), bool)
    dropped[y[cross & inside], x[cross & inside]] = True
    assert dropped.sum() >= 40 and np.array_equal(g["film"][..., 3] == 0, dropped)
    assert (g["film"][dropped] == 0).all()


@pytest.mark.parametrize("case", ["hom_light_two", "het_light_two"])
def test_powerless_light_is_never_picked(runs, case):
    f = flags(runs(case)[1])
    assert ((f & Oracle.MEDIUM_LIGHT0) == 0).all() and ((f & (Oracle.MEDIUM_LIGHT0 << 1)) != 0).sum() >= 40


@pytest.mark.parametrize("case", mc.EMITTER_CASES)
def test_emitters_are_seen_and_hidden_from_inside_the_region(runs, case):
    """Light samples taken from inside the medium end exactly on the emitter: some are occluded, some are not."""
    f = flags(runs(case)[1])
    assert ((f & Oracle.MEDIUM_OCCLUDED) != 0).sum() >= 5 and ((f & Oracle.MEDIUM_UNOCCLUDED) != 0).sum() >= 5


def test_no_lights_leaves_the_path_tracers_ray_unclipped(runs):
    """Without lights PathTracer::Li returns before its first scene query and the camera ray's maxt stays infinite; Whitted and AO
    do query the scene.  The light pick is drawn all the same."""
    for case, clipped in (("het_light_none", False), ("hom_light_none", False), ("het_light_none_whitted", True), ("het_light_none_ao", True)):
        run = runs(case)[1]
        f = flags(run)
        assert ((f & Oracle.MEDIUM_CLIPPED) != 0).all() == clipped and ((f & Oracle.MEDIUM_CLIPPED) != 0).any() == clipped, case
        assert (f >> 8 == 0).all()
        assert run["medium"][(f & Oracle.MEDIUM_CROSSES) != 0, 6].min() >= 2
        assert (run["medium"][:, 3:6] == 0).all()
