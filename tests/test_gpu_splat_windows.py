"""The windowed variants of wf_splat's fast path (kernels/wavefront.h, wf_splat_window): per sample the wave's lanes vote on the
4 x 4 window of the 5 x 5 block that the sample's footprint covers, and a scalar branch runs straight-line code for those 16
cells; any other sample takes the 25-cell body.  A lane's sums are meant to be bit for bit the 25-cell body's.

What is compared: the device's film against the oracle's film on identical samples (the oracle's restatement of the native
sampler, same seed, its own radiance of those records splatted by its restatement of ImageTile::addSample), as bench.py's
l2_vs_cpu does.  Tolerance: the suite's bound for summation order on the accumulators (tests/test_gpu_parity.py: rtol 1e-5,
atol 1e-6), nothing wider.  As a precondition the device's per-sample radiance equals the oracle's (no flipped sample).

The cases are the smallest at which a variant can go wrong:
  * film 13 x 11: every tile is an edge tile, the crop predicates are live in every variant;
  * film 24 x 16 with a crop window strictly inside, and without one (two tiles whose 5 x 5 blocks all lie inside the crop, the
    build without predicates, next to edge tiles in one launch);
  * 4 and 16 spp (root 2 and 4: all four windows, each uniform over the wave), 9 spp (root 3: the middle sub-cell straddles the
    centre lines, so every record still has one of the four windows but the lanes of a wave disagree) and 1 spp (likewise);
  * gaussian 2, Mitchell and triangle of width 2, box 0.5 (fewer than four columns: the 25-cell body), gaussian 1.5 (the bins'
    division form), widths (2, 1);
  * the stream sampler's positions (RenderArgs::image_xy), and a window near x = 2048 where px + u rounds onto a centre line.
The counted cells (render(stats=True), wf_splat<.., true>) must equal the number of cells the oracle's records touch.
"""
import numpy as np
import pytest

import helpers
import oracle_binding as ob
from goblin_amd import scene as gs

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-6   # tests/test_gpu_parity.py, the accumulators
SEED = 20261020
GAUSS2 = {"type": "gaussian", "width": [2, 2], "falloff": 2}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def load(resolution, spp, filt=GAUSS2, crop=None):
    ov = gs.config_overrides(resolution=resolution, spp=spp, depth=3, filter=filt)
    if crop:
        ov["camera"]["film"]["crop"] = list(crop)
    return gs.load_scene("cornell", ov)


def crop_bounds(scene):
    """Film's xstart, xend, ystart, yend (inclusive ends), as GoblinFilm.cpp computes them."""
    f = scene.desc.film
    ceil_i = lambda v: int(np.ceil(np.float32(v)))
    xs = ceil_i(np.float32(f.xres) * np.float32(f.crop[0]))
    xc = max(1, ceil_i(np.float32(f.xres) * np.float32(f.crop[1])) - xs)
    ys = ceil_i(np.float32(f.yres) * np.float32(f.crop[2]))
    yc = max(1, ceil_i(np.float32(f.yres) * np.float32(f.crop[3])) - ys)
    return xs, xs + xc - 1, ys, ys + yc - 1


def footprints(scene, xy):
    """Per record the footprint ImageTile::addSample walks, in float32 as it does: x0, x1, y0, y1 before the crop."""
    wx, wy = np.float32(scene.desc.film.filter_width[0]), np.float32(scene.desc.film.filter_width[1])
    dx = (xy[:, 0] - np.float32(0.5)).astype(np.float32)
    dy = (xy[:, 1] - np.float32(0.5)).astype(np.float32)
    return (np.ceil((dx - wx).astype(np.float32)).astype(np.int64), np.floor((dx + wx).astype(np.float32)).astype(np.int64),
            np.ceil((dy - wy).astype(np.float32)).astype(np.int64), np.floor((dy + wy).astype(np.float32)).astype(np.int64))


def touched_cells(scene, xy, li):
    """The number of film cells the oracle's records touch: footprint clipped to the crop, NaN samples dropped."""
    xs, xe, ys, ye = crop_bounds(scene)
    x0, x1, y0, y1 = footprints(scene, xy)
    ok = ~np.isnan(li[:, :3]).any(axis=1)
    nx = np.maximum(np.minimum(x1, xe) - np.maximum(x0, xs) + 1, 0)
    ny = np.maximum(np.minimum(y1, ye) - np.maximum(y0, ys) + 1, 0)
    return int((nx * ny)[ok].sum())


def window_census(scene, xy):
    """How many records have a 4 x 4 footprint that starts at column / row 0 or 1 of their pixel's 5 x 5 block, per (column
    start, row start), and how many have any other footprint."""
    x0, x1, y0, y1 = footprints(scene, xy)
    px, py = np.floor(xy[:, 0]).astype(np.int64), np.floor(xy[:, 1]).astype(np.int64)
    sx, sy = x0 - (px - 2), y0 - (py - 2)
    fits = (x1 - x0 == 3) & (y1 - y0 == 3) & (sx >= 0) & (sx <= 1) & (sy >= 0) & (sy <= 1)
    census = {(a, b): int((fits & (sx == a) & (sy == b)).sum()) for a in (0, 1) for b in (0, 1)}
    census["other"] = int((~fits).sum())
    return census


_refs = {}


def reference(key, scene, window=None):
    """The oracle's records, radiance and film for a case: computed once, shared, left unchanged."""
    if key not in _refs:
        o = ob.Oracle(scene)
        samples = o.native_samples(SEED, window=window)
        li, _ = o.li_replay(samples, threads=4)
        film = o.splat(samples, li)
        for a in (samples, li, film):
            a.setflags(write=False)
        _refs[key] = (samples, li, film)
    return _refs[key]


def check_film(label, film, ref):
    dev = film.astype(np.float64)
    err = np.abs(dev - ref)
    over = err - (ATOL + RTOL * np.abs(ref))
    print("%s: largest |device - oracle| %.4g, largest excess over atol + rtol |oracle| %.4g (<= 0 passes)" % (label, float(err.max()), float(over.max())))
    np.testing.assert_allclose(film, ref, rtol=RTOL, atol=ATOL, err_msg=label)


def run_case(label, scene, key, want):
    """Render with and without the counters (wf_splat<false, true> and <false, false>); both films against the oracle's; the
    counted cells against the oracle's records.  `want`: which census entries the case must hold (it is about those)."""
    from goblin_amd.renderer import HipPathTracer
    samples, li_ref, film_ref = reference(key, scene)
    census = window_census(scene, samples[:, :2])
    print(label, "windows of the oracle's records:", census)
    for k in want:
        assert census[k] > 0, (label, k, census)
    r = HipPathTracer(scene, 0)
    counted = r.render(seed=SEED, want_li=True, stats=True)
    li = counted["li"].cpu().numpy()
    assert helpers.li_mismatch_fraction(li, li_ref) == 0.0, label   # precondition: the same radiance goes into both splats
    cells = touched_cells(scene, samples[:, :2], li_ref)
    print(label, "cells counted by the device", counted["stats"]["splats"], "touched by the oracle's records", cells)
    assert counted["stats"]["splats"] == cells, label
    check_film(label + " (counters)", counted["film"].numpy(), film_ref)
    check_film(label, r.render(seed=SEED)["film"].numpy(), film_ref)


ALL_FOUR = [(0, 0), (1, 0), (0, 1), (1, 1)]


@pytest.mark.parametrize("spp,want", [(4, ALL_FOUR), (16, ALL_FOUR), (9, ALL_FOUR), (1, ALL_FOUR)])
@pytest.mark.parametrize("resolution,crop", [((13, 11), None), ((24, 16), (0.13, 0.9, 0.13, 0.9)), ((24, 16), None)])
def test_gaussian_2_every_window(torch, resolution, crop, spp, want):
    """13 x 11: edge tiles only.  24 x 16 cropped to columns 4 .. 21, rows 3 .. 14: tiles in the middle of the launch and on its
    edge, all with live crop predicates.  24 x 16 whole: tiles (1, 1) and (2, 1) of the 4 x 3 have every 5 x 5 block inside."""
    scene = load(resolution, spp, crop=crop)
    if crop:
        assert crop_bounds(scene) == (4, 21, 3, 14)
    run_case("%dx%d crop %s spp %d" % (resolution + (crop, spp)), scene, ("g2", resolution, crop, spp), want)


@pytest.mark.parametrize("filt,want", [
    ({"type": "mitchell", "width": [2, 2]}, ALL_FOUR),
    ({"type": "triangle", "width": [2, 2]}, ALL_FOUR),
    ({"type": "box", "width": [0.5, 0.5]}, ["other"]),                     # one or two columns: the 25-cell body
    ({"type": "gaussian", "width": [1.5, 1.5], "falloff": 2}, ["other"]),  # the division form of the bins; 3 or 4 columns
    ({"type": "gaussian", "width": [2, 1], "falloff": 2}, ["other"]),      # 4 columns, 2 or 3 rows
])
@pytest.mark.parametrize("resolution", [(13, 11), (24, 16)])
def test_other_filters(torch, resolution, filt, want):
    scene = load(resolution, 4, filt=filt)
    run_case("%dx%d %s %s" % (resolution + (filt["type"], filt["width"])), scene, ("f", resolution, filt["type"], tuple(filt["width"])), want)


def test_stream_sampler_positions(torch):
    """sampler="stream", 8 x 8, 4 spp: the positions come from image_xy and differ from lane to lane, so a wave agrees on a
    window only by chance and a sample on a centre line must fall back.  Against the oracle's whole render of that stream."""
    from goblin_amd.renderer import HipPathTracer
    scene = load((8, 8), 4)
    o = ob.Oracle(scene)
    res = o.render(threads=1, want_samples=True)
    print("stream: windows of the oracle's records:", window_census(scene, res["samples"][:, :2]))
    out = HipPathTracer(scene, 0).render(sampler="stream", want_li=True)
    idx = helpers.tile_order_index(o.window(), 4)
    assert helpers.li_mismatch_fraction(out["li"].cpu().numpy(), res["li"][idx]) == 0.0
    check_film("stream", out["film"].numpy(), res["film"])


def test_positions_that_round_onto_a_centre_line(torch):
    """A 16 x 8 window at x = 2040 .. 2055 of a 2064-pixel-wide film, 16 spp: there a float has 11 or 12 fraction bits, so px + u
    lands exactly on n + 0.5 for some samples of the sub-cells beside the centre; their footprint is 5 columns wide and the wave
    must take the 25-cell body for them."""
    from goblin_amd.renderer import HipPathTracer
    scene = load((2064, 8), 16)
    r = HipPathTracer(scene, 0)
    x0, x1, y0, y1 = r.window
    sub = (x0 + 2042, x0 + 2058, y0, y0 + 8)
    o = ob.Oracle(scene)
    samples = o.native_samples(SEED, window=sub)
    on_line = int(((samples[:, 0] - np.floor(samples[:, 0]) == 0.5) | (samples[:, 1] - np.floor(samples[:, 1]) == 0.5)).sum())
    print("records exactly on a pixel centre line: %d of %d; windows:" % (on_line, samples.shape[0]), window_census(scene, samples[:, :2]))
    if on_line == 0:
        pytest.skip("no record of this seed sits exactly on a centre line")
    li_ref, _ = o.li_replay(samples, threads=4)
    out = r.render(seed=SEED, window=sub, want_li=True, stats=True)
    assert helpers.li_mismatch_fraction(out["li"].cpu().numpy(), li_ref) == 0.0
    assert out["stats"]["splats"] == touched_cells(scene, samples[:, :2], li_ref)
    check_film("near x = 2048", out["film"].numpy(), o.splat(samples, li_ref))


def inside_tile(scene, px0, py0):
    """wf_splat's per-workgroup test: the 5 x 5 blocks of all 64 pixels of the tile at (px0, py0) lie inside the crop."""
    xs, xe, ys, ye = crop_bounds(scene)
    return px0 - 2 >= xs and px0 + 9 <= xe and py0 - 2 >= ys and py0 + 9 <= ye


def test_bytes_of_a_frame_whose_splat_order_is_fixed(torch):
    """The fast path's film, byte for byte, against the same record replayed without image_xy, which takes the splat's general
    path; precondition: the per-sample radiance of the two renders is bit-equal.

    The frames: one-pixel windows of a 24 x 16 film at 1 spp -- every third pixel of the sample window, and every pixel whose tile
    (the window starts it) has all its 5 x 5 blocks inside the crop, 13 x 5 of them.  A frame of one sample
    gives every film cell ONE addend, so its bytes do not depend on the order of any additions, and the one live lane agrees
    with itself: the sample runs the variant of its window (all four, in tiles with and without live crop predicates; counted
    below from the oracle's records) where a whole tile of 1-spp pixels would disagree and take the 25-cell body.

    Why not the 28 x 4 frame of tests/test_gpu_lights.py: its bytes are fixed per path, but not the same for the two paths, and
    were not before the variants either.  Both add the same addends to a cell of the LDS tile, in another order: the general
    path's lanes walk their own footprints from (y0, x0) in lockstep, the fast path's walk their pixel's 5 x 5 block, so lanes
    whose footprints start a column or a row apart meet in a shared cell at different steps.  Restating the two walks in
    float32 on the CPU (order by (y - y0, x - x0, lane) against (y - (py - 2), x - (px - 2), lane), the oracle's records and
    radiance) gives 75 differing words of 448; the device measured 75 of 448, with this library and with its parent alike."""
    from goblin_amd.renderer import HipPathTracer
    scene = load((24, 16), 1)
    o = ob.Oracle(scene)
    r = HipPathTracer(scene, 0)
    x0, x1, y0, y1 = r.window
    pixels = [(x, y) for y in range(y0, y1) for x in range(x0, x1) if inside_tile(scene, x, y) or ((x - x0) % 3 == 0 and (y - y0) % 3 == 0)]
    seen = {True: set(), False: set()}
    differing = 0
    for x, y in pixels:
        win = (x, x + 1, y, y + 1)
        rec = o.native_samples(SEED, window=win)
        census = window_census(scene, rec[:, :2])
        seen[inside_tile(scene, x, y)].update(k for k, n in census.items() if n)
        native = r.render(seed=SEED, window=win, want_li=True)
        replay = r.render(replay_samples=rec, window=win, want_li=True)
        assert np.array_equal(native["li"].cpu().numpy().view(np.uint32), replay["li"].cpu().numpy().view(np.uint32)), (x, y)
        a, b = native["film"].numpy(), replay["film"].numpy()
        differing += int((a.view(np.uint32) != b.view(np.uint32)).sum())
        assert a.tobytes() == b.tobytes(), (x, y, census)
    print("one-pixel frames: %d, windows seen in tiles inside the crop %s, in edge tiles %s, differing film words %d"
          % (len(pixels), sorted(seen[True], key=str), sorted(seen[False], key=str), differing))
    for k in ALL_FOUR:
        assert k in seen[True] and k in seen[False], (k, seen)
