"""Oracle.first_hit and the texture charts without a GPU.

first_hit is the probe the AOV tests take their expected records from (tests/aov_reference.py).  Here it is held (1) to the
per-sample probes it replaced, camera_ray + intersect, bit for bit in t, instance, position and normal; (2) to the scene
description where the first colour slot is a constant; (3) to the compiled reference, live where oracle/_ref/ref_harness exists and
by the firsthit_* fixtures of tests/golden/ everywhere: for a Lambert hit the reference's bsdf(fragment, n, n) is Kd's lookup
times INV_PI (GoblinMaterial.cpp:437-445), so float32(albedo * INV_PI) must be that value and t, position and normal equal.  The
other slots (Kg, Kr, a mask's wrapped material) go through the same lookup code.  Then the charts themselves
(tests/texture_chart.py) are checked to test something: hits in every cell, the top of the pyramid reached and not reached, zero
and non-zero border lookups, filters that differ.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import aov_reference as ar
import oracle_binding as ob
import texture_chart as tc
from goblin_amd import scene as gs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(REPO, "oracle", "_ref", "ref_harness")
GOLDEN = os.path.join(REPO, "tests", "golden")
INV_PI = np.float32(0.31830988618379067154)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# 1 ------------------------------------------------------------------------------------------------------------------
LOOP_SCENES = ["cornell", "shapes", "grid", "volume", "textured", "imagetex", "bumpy", "masked", "subsurface", "ibl"]
LOOP_CHARTS = [("16x16", "perspective"), ("5x3", "orthographic"), ("slots", "perspective")]


def loop_case(case):
    return tc.reference(*case) if isinstance(case, tuple) else ar.reference(case)


@pytest.mark.parametrize("case", LOOP_SCENES + LOOP_CHARTS, ids=str)
def test_first_hit_equals_the_probe_loop(case):
    """(pinhole and orthographic cameras: orc_camera_ray takes no lens sample)"""
    ref = loop_case(case)
    hit, t, instance, position, normal = ar.loop_records(ref.oracle, ref.samples)
    assert hit.sum() > 0 and (hit == 0).sum() > 0
    np.testing.assert_array_equal(ref.hit, hit)
    np.testing.assert_array_equal(ref.instance, instance)
    np.testing.assert_array_equal(bits(ref.t), bits(t))
    np.testing.assert_array_equal(bits(ref.position), bits(position))
    np.testing.assert_array_equal(bits(ref.normal), bits(normal))
    miss = hit == 0
    assert not ref.records[miss][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].any() and (ref.t[miss] == -1).all() and (ref.instance[miss] == -1).all()
    # where the description alone says what the first colour slot is, the lookup is that constant
    known = ref.albedo_known
    np.testing.assert_array_equal(bits(ref.oracle_albedo[known]), bits(ref.albedo[known]))
    assert np.isfinite(ref.records[:, [0, 1, 2, 3, 4, 5, 6, 8, 9, 10]]).all()


def test_first_hit_draws_the_lens_sample():
    """Under a thin lens the camera ray leaves the lens at (lens_u1, lens_u2): other records than from the lens centre."""
    ref = tc.reference("16x16", "thinlens")
    centred = ref.samples.copy()
    centred[:, 2:4] = 0.5
    other = ref.oracle.first_hit(centred)
    assert ref.hit.sum() > 0 and (bits(other[:, 3]) != bits(ref.t)).sum() > ref.hit.sum() // 2


# 2 ------------------------------------------------------------------------------------------------------------------
def harness_first_hit(tmp_path, name, samples):
    d, directory, not_bilinear, _ = tc.firsthit_case(name)
    with open(tmp_path / "s.json", "w") as f:
        json.dump(tc.harness_doc(d, directory, not_bilinear), f)
    np.ascontiguousarray(samples[:, :4], np.float32).tofile(tmp_path / "in.f32")
    try:
        subprocess.check_output([HARNESS, "firsthit", str(tmp_path / "s.json"), str(tmp_path / "in.f32"), str(tmp_path / "out.f32")],
                                stderr=subprocess.DEVNULL, timeout=300)
    except (OSError, subprocess.SubprocessError) as e:   # a harness built for another machine
        pytest.skip("ref_harness did not run here: %s" % e)
    return np.fromfile(tmp_path / "out.f32", np.float32).reshape(-1, 12)


def firsthit_reference(name):
    d, directory, _, excluded = tc.firsthit_case(name)
    scene = gs.load_scene_text(json.dumps(d), directory)
    ref = ar.Reference(scene, seed=tc.FIRSTHIT_SEED)
    base = scene.desc.num_instances - tc.COLS * tc.ROWS if name.startswith("chart_") else 0
    return ref, [base + k for k in excluded]


def assert_equals_the_compiled_reference(name, ref, excluded, rows, got, what):
    """rows: the sample indices `got` (the harness's records) stands for."""
    hit = ref.hit[rows] == 1
    np.testing.assert_array_equal(got[:, 11], hit.astype(np.float32), err_msg=what)
    np.testing.assert_array_equal(bits(got[:, 3]), bits(ref.t[rows]), err_msg=what)
    np.testing.assert_array_equal(bits(got[:, 4:7]), bits(ref.normal[rows]), err_msg=what)
    np.testing.assert_array_equal(bits(got[:, 8:11]), bits(ref.position[rows]), err_msg=what)
    lambert = (got[:, 7] == 1) & hit & ~np.isin(ref.instance[rows], excluded)   # (the bilinear colour slots: see texture_chart.firsthit_case)
    want = (ref.oracle_albedo[rows] * INV_PI).astype(np.float32)
    print(what, "samples", len(rows), "hits", int(hit.sum()), "Lambert hits compared", int(lambert.sum()))
    assert lambert.sum() >= 100, what
    np.testing.assert_array_equal(bits(got[lambert, 0:3]), bits(want[lambert]), err_msg=what)


@pytest.mark.skipif(not os.path.exists(HARNESS), reason="oracle/_ref/ref_harness not built (needs the reference's sources)")
@pytest.mark.parametrize("name", tc.FIRSTHIT_CASES)
def test_first_hit_equals_the_compiled_reference(tmp_path, name):
    ref, excluded = firsthit_reference(name)
    got = harness_first_hit(tmp_path, name, ref.samples)
    assert_equals_the_compiled_reference(name, ref, excluded, np.arange(ref.n), got, name + " live")


@pytest.mark.parametrize("name", tc.FIRSTHIT_CASES)
def test_first_hit_equals_the_recorded_reference(name):
    """The same comparison against tests/golden/firsthit_<name>.npz (make_golden.py: every fifth sample of the same stream).
    On another libm than the fixtures' the spherical mappings' atan2f / acosf may round differently: positions, normals and t
    stay bit-exact (no libm call on that path), the colours are then held to one decade above float epsilon."""
    data = np.load(os.path.join(GOLDEN, "firsthit_" + name + ".npz"))
    ref, excluded = firsthit_reference(name)
    rows = np.arange(0, ref.n, tc.FIRSTHIT_STRIDE)
    np.testing.assert_array_equal(bits(ref.samples[rows, :4]), bits(data["samples"]))
    got = data["records"]
    if os.path.exists(HARNESS):   # where the fixtures can be made: every bit
        assert_equals_the_compiled_reference(name, ref, excluded, rows, got, name + " recorded")
        return
    hit = ref.hit[rows] == 1
    np.testing.assert_array_equal(got[:, 11], hit.astype(np.float32))
    np.testing.assert_allclose(got[:, 3], ref.t[rows], rtol=1e-6)
    np.testing.assert_allclose(got[:, 4:7], ref.normal[rows], rtol=0, atol=1e-6)
    np.testing.assert_allclose(got[:, 8:11], ref.position[rows], rtol=1e-6, atol=1e-6)
    lambert = (got[:, 7] == 1) & hit & ~np.isin(ref.instance[rows], excluded)
    assert lambert.sum() >= 100
    close = np.isclose(got[lambert, 0:3], (ref.oracle_albedo[rows] * INV_PI).astype(np.float32)[lambert], rtol=1e-6, atol=1e-7).all(axis=1)
    assert close.mean() >= 0.999, (name, close.mean())   # (a lookup that lands on another texel after a last-bit change of s or t)


# 3 ------------------------------------------------------------------------------------------------------------------
def proportional(a, top):
    """Rows of `a` that are one number times the pyramid's top texel -- what every lookup of the 1x1 level returns, whatever its
    bilinear weights and the border's zeros make that number.  (The chart images change hue from texel to texel, so a blend of
    lower levels is not.)"""
    ratio = a.astype(np.float64) / top.astype(np.float64)
    return (np.abs(ratio - ratio[:, :1]).max(axis=1) <= 1e-6) & a.any(axis=1)


@pytest.mark.parametrize("camera", tc.CAMERAS)
@pytest.mark.parametrize("image", list(tc.IMAGES))
def test_chart_tests_something(image, camera):
    """The conditions that keep a chart from testing nothing, from the oracle alone.

    Every cell receives at least 16 hits; some border lookup is exactly zero and some is not; the four filters of a row do not
    all return the same values (asked where the pyramid has more than its one 1x1 level to choose from).  Under the two projective cameras, in every trilinear and EWA cell the far half holds a sample
    whose lookup came from the 1x1 top of the pyramid, and (where the pyramid has another level) the near half one whose did
    not.  `From the top` is bitwise the top texel under repeat and clamp.  Under border the level's bilinear lookup weighs the one
    texel against the border's zeros, so no sample returns the texel itself: there it is a multiple of it (proportional), and the
    few non-zero samples lie where the footprint is about the image, so only the first half of the condition is asked.  The
    orthographic camera has one footprint per cell: it is compared like the others, these two conditions are not its to meet."""
    ref = tc.reference(image, camera)
    scene = ref.scene
    top = tc.top_texel(scene)
    levels = scene.desc.images[0].levels
    cells = tc.cell_masks(ref)
    y = ref.samples[:, 1]
    for k, on in enumerate(cells):
        assert on.sum() >= 16, (image, camera, k, int(on.sum()))
    for row, mode in enumerate(tc.MODES):
        per_filter = [ref.oracle_albedo[cells[row * tc.COLS + col]] for col in range(tc.COLS)]
        if levels > 1:
            assert len({a.tobytes() for a in per_filter}) > 1, (image, camera, mode)
        for col, filt in enumerate(tc.FILTERS):
            on = cells[row * tc.COLS + col]
            a = ref.oracle_albedo[on]
            if mode == "border":
                zero = ~a.any(axis=1)
                assert zero.any() and (~zero).any(), (image, camera, filt)
            if camera == "orthographic" or filt not in ("trilinear", "EWA"):
                continue
            far = y[on] < 0.5 * (y[on].min() + y[on].max())
            if mode == "border":
                assert proportional(a[far], top).any(), (image, camera, mode, filt)
                continue
            is_top = (bits(a) == bits(top)).all(axis=1)
            print(image, camera, mode, filt, "far: top", int(is_top[far].sum()), "of", int(far.sum()), "near: top", int(is_top[~far].sum()), "of", int((~far).sum()))
            assert is_top[far].any(), (image, camera, mode, filt)
            if levels > 1:
                assert (~is_top[~far]).any(), (image, camera, mode, filt)


@pytest.mark.parametrize("camera", tc.CAMERAS)
def test_slot_chart_tests_something(camera):
    """Every cell of the slot chart is hit, by lookups that vary over the cell (no slot answers with a constant), and the cells
    differ from one another."""
    ref = tc.reference("slots", camera)
    cells = tc.cell_masks(ref)
    seen = set()
    for name, on in zip(tc.SLOT_CELLS, cells):
        a = ref.oracle_albedo[on]
        assert on.sum() >= 16 and len(np.unique(a, axis=0)) >= 8, (camera, name, int(on.sum()))
        seen.add(a.tobytes())
    assert len(seen) == len(cells)
    desc = ref.scene.desc
    assert sorted({desc.images[i].levels for i in range(desc.num_images)}) == [4, 5]      # the 5x3 (resampled to 8x4) and the 16x16 image


def test_chart_images_are_the_pyramids_the_fixtures_lack():
    got = {}
    for image in tc.IMAGES:
        im = tc.scene(image).desc.images[0]
        got[image] = (im.width, im.height, im.levels)
    assert got == {"1x1": (1, 1, 1), "2x1": (2, 1, 2), "1x8": (1, 8, 4), "5x3": (8, 4, 4), "64x4": (64, 4, 7), "4x64": (4, 64, 7), "16x16": (16, 16, 5)}
    for image, (w, h) in tc.IMAGES.items():
        t = tc.texels(w, h)
        assert t.min() >= 0.05 and t.max() <= 0.95 and np.array_equal(t, t.astype(np.float16).astype(np.float32))
