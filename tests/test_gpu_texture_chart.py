"""The texture charts (tests/texture_chart.py) on the device: seven pyramid shapes x four filters x three address modes, and one
chart of texture graphs and material slots, under the three cameras.  These are the image lookups kernels/image.h has edges for
and no bundled scene visits: levels where one side is already 1, one- and two-level pyramids, the level clamp at the top, EWA's
empty-ellipse fallback, negative coordinates under repeat, clamp's "t from s" on a non-square level, border outside the image.

Held to the oracle (pinned to the compiled reference on these very scenes, tests/test_first_hit_cpu.py): the first-hit records
of gbl_render_aov bit for bit, albedo included, native and replayed; the radiance of the native sampler's samples bit for bit
under both schedules; the stream sampler's film within the bound of tests/test_gpu_fuzz.py's round-2 test."""
import functools

import numpy as np
import pytest
import torch

from goblin_amd.renderer import HipPathTracer
import aov_reference as ar
import helpers
import oracle_binding as ob
import texture_chart as tc

pytestmark = pytest.mark.gpu

SEED = ar.SEED
STREAM_FILM_TOL = 6e-5      # tests/test_gpu_fuzz.py test_random_scene_with_round2_features_matches_oracle
CASES = [(chart, camera) for chart in tc.CHARTS for camera in tc.CAMERAS]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def tracer(chart, camera, method=None):
    return HipPathTracer(tc.scene(chart, camera, method), 0)


def rows(out):
    torch.cuda.synchronize()
    return out["samples_i32"].cpu().numpy()


def assert_rows_equal(got, ref, what):
    """Field by field, so a failure names the field; then the whole rows."""
    f = got.view(np.float32)
    np.testing.assert_array_equal(got[:, 11].view(np.uint32), ref.hit, err_msg=str(what))
    np.testing.assert_array_equal(got[:, 7], ref.instance, err_msg=str(what))
    np.testing.assert_array_equal(bits(f[:, 3]), bits(ref.t), err_msg=str(what))
    np.testing.assert_array_equal(bits(f[:, 8:11]), bits(ref.position), err_msg=str(what))
    np.testing.assert_array_equal(bits(f[:, 4:7]), bits(ref.normal), err_msg=str(what))
    wrong = (bits(f[:, 0:3]) != bits(ref.oracle_albedo)).any(axis=1)
    if wrong.any():
        cells = tc.cell_instances(ref.scene)
        per_cell = {k: int((wrong & (ref.instance == i)).sum()) for k, i in enumerate(cells) if (wrong & (ref.instance == i)).any()}
        i = int(np.flatnonzero(wrong)[0])
        raise AssertionError("%s: albedo differs at %d of %d hits, per cell %s; first: sample %d device %s oracle %s" % (
            what, int(wrong.sum()), int((ref.hit == 1).sum()), per_cell, i, f[i, 0:3], ref.oracle_albedo[i]))
    np.testing.assert_array_equal(got, ref.rows, err_msg=str(what))


@pytest.mark.parametrize("chart,camera", CASES)
def test_records_equal_the_oracle_bit_for_bit(chart, camera):
    ref = tc.reference(chart, camera)
    assert ref.hit.sum() > 0 and (ref.hit == 0).sum() > 0
    r = tracer(chart, camera)
    native = rows(r.render_aov(albedo=False, normal=False, depth=False, want_samples=True, seed=SEED, exact_ties=True))
    assert_rows_equal(native, ref, (chart, camera, "native"))
    replayed = rows(r.render_aov(albedo=False, normal=False, depth=False, want_samples=True, replay_samples=ref.samples.copy()))
    assert_rows_equal(replayed, ref, (chart, camera, "replay"))


@pytest.mark.parametrize("chart,camera", CASES)
def test_radiance_equals_the_oracle(chart, camera):
    """The assertions of test_random_scene_with_round2_features_matches_oracle."""
    ref = tc.reference(chart, camera)
    o = ref.oracle
    li_ref, _ = o.li_replay(ref.samples, threads=4)
    assert np.isfinite(li_ref).all() and li_ref[:, :3].max() > 0
    r = tracer(chart, camera)
    for schedule in ("megakernel", "wavefront"):
        li = r.render(seed=SEED, want_li=True, schedule=schedule)["li"].cpu().numpy()
        assert np.isfinite(li).all(), (chart, camera, schedule)
        flips = helpers.li_mismatch_fraction(li, li_ref)
        rel = helpers.rel_l2(li[:, :3], li_ref[:, :3])
        print(chart, camera, schedule, "flips %.5f relL2 %.2e" % (flips, rel))
        assert flips == 0.0 and rel == 0.0, (chart, camera, schedule, flips, rel)
    want = o.render(threads=1)["film"]
    film = r.render(sampler="stream")["film"].numpy()
    rel = helpers.rel_l2(ob.normalize_film(film), ob.normalize_film(want))
    print(chart, camera, "stream film relL2 %.2e" % rel)
    np.testing.assert_allclose(film[..., 3], want[..., 3], rtol=1e-5, atol=1e-6)
    assert rel <= STREAM_FILM_TOL, (chart, camera, rel)


@pytest.mark.parametrize("chart", ["64x4", "slots"])
def test_whitted_radiance_equals_the_oracle(chart):
    scene = tc.scene(chart, "perspective", "whitted")
    o = ob.Oracle(scene)
    samples = o.native_samples(SEED)
    li_ref, _ = o.li_replay(samples, threads=4)
    assert np.isfinite(li_ref).all() and li_ref[:, :3].max() > 0
    r = tracer(chart, "perspective", "whitted")
    li = r.render(seed=SEED, want_li=True)["li"].cpu().numpy()
    flips = helpers.li_mismatch_fraction(li, li_ref)
    rel = helpers.rel_l2(li[:, :3], li_ref[:, :3])
    print(chart, "whitted flips %.5f relL2 %.2e" % (flips, rel))
    assert flips == 0.0 and rel == 0.0, (chart, flips, rel)
    want = o.render(threads=1)["film"]
    film = r.render(sampler="stream")["film"].numpy()
    rel = helpers.rel_l2(ob.normalize_film(film), ob.normalize_film(want))
    print(chart, "whitted stream film relL2 %.2e" % rel)
    np.testing.assert_allclose(film[..., 3], want[..., 3], rtol=1e-5, atol=1e-6)
    assert rel <= STREAM_FILM_TOL, (chart, rel)
