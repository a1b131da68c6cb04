"""wf_splat (kernels/wavefront.h), the kernel that filters per-sample radiance into the film at the end of every render: the
device film against a float64 numpy restatement of ImageTile::addSample (GoblinFilm.cpp:61-90) fed with the device's OWN
per-sample radiance and the oracle's image positions -- so only the splat is under test, not the integrator.

The restatement takes every decision (footprint bounds, filter-table bins) in float32 exactly as the reference does and only
accumulates in float64; what is left between it and the device is the rounding of w * L and of <= 25 x spp float32 additions
per pixel, in whatever order the LDS and global atomics land.

Tolerance, measured and not chosen: the largest relative deviation |device - restatement| / |restatement| over every pixel and
channel of every case below was 5.461e-07 (MEASURED_PARENT_MAX_REL) with the kernel as it was before its fast path was rewritten
(one MI355X; the replay case under the wavefront schedule held the maximum, the fast path's own was 4.905e-07 at spp 81, filter
(2, 2)); the bar is twice that, for the order of the additions.  The figure moves from run to run with the order in which the
LDS and global atomics land: the rewritten kernel, which adds the same addends in the same order per (wave, lane), measured
between 1.7e-07 and 5.8e-07 on these cases.  Every case prints its figure before it asserts.
The weight plane (sums of filter-table values) is held to 1e-4 relative in every pixel, none left out.
"""
import numpy as np
import pytest

import helpers
import oracle_binding as ob
from goblin_amd import scene as gs

MEASURED_PARENT_MAX_REL = 5.461e-07
FILM_REL_TOL = 2.0 * MEASURED_PARENT_MAX_REL
WEIGHT_REL_TOL = 1e-4
TILE = 8


# ---------------------------------------------------------------------------
# The bin arithmetic of the fast path (no GPU)
# ---------------------------------------------------------------------------
def _bin_div(x, dx, w):
    """min(int(floorf(fabsf(16 * (x - dx) / w))), 15) in float32, as FilterTable::evaluate computes it."""
    t = (np.float32(16) * (x.astype(np.float32) - dx)).astype(np.float32)
    return np.minimum(np.floor(np.abs((t / np.float32(w)).astype(np.float32))), 15).astype(np.int32)


def _bin_mul(x, dx, w):
    """The fast path's form for a power-of-two w: the same product times the exact reciprocal."""
    t = (np.float32(16) * (x.astype(np.float32) - dx)).astype(np.float32)
    inv = np.float32(1) / np.float32(w)
    return np.minimum(np.floor(np.abs((t * inv).astype(np.float32))), 15).astype(np.int32)


def test_multiply_form_gives_the_division_forms_bin():
    """Every dx = image_x - 0.5 a sample of pixel p can have lies in [p - 0.5, p + 0.5]; the five footprint columns are
    p - 2 ... p + 2.  Dense sweep of that interval (every float32 near its ends and near every bin edge's neighbourhood is
    covered by stepping ulp by ulp there), its float neighbours outside, pixels 0, 7 and 511, every power-of-two width the
    film accepts from 0.25 to 4."""
    for p in (0, 7, 511):
        lo, hi = np.float32(p - 0.5), np.float32(p + 0.5)
        grid = np.linspace(lo, hi, 200001, dtype=np.float64).astype(np.float32)
        # ulp-by-ulp runs at both ends (neighbours outside included) and around the pixel centre
        runs = []
        for c in (lo, hi, np.float32(p)):
            v = [c]
            for _ in range(2000):
                v.append(np.nextafter(v[-1], np.float32(np.inf), dtype=np.float32))
            u = [c]
            for _ in range(2000):
                u.append(np.nextafter(u[-1], np.float32(-np.inf), dtype=np.float32))
            runs.append(np.array(v + u, np.float32))
        # ... and around every bin edge of every width: x - dx = j * w / 16
        edges = []
        for w in (0.25, 0.5, 1.0, 2.0, 4.0):
            for o in range(-2, 3):
                j = np.arange(-16, 17, dtype=np.float64)
                e = (p + o - j * w / 16).astype(np.float32)
                e = e[(e >= lo) & (e <= hi)]
                for k in range(-3, 4):
                    q = e.copy()
                    for _ in range(abs(k)):
                        q = np.nextafter(q, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
                    edges.append(q)
        dx = np.unique(np.concatenate([grid] + runs + edges))
        for w in (0.25, 0.5, 1.0, 2.0, 4.0):
            for o in range(-2, 3):
                x = np.full(dx.shape, p + o, np.int32)
                a, b = _bin_div(x, dx, w), _bin_mul(x, dx, w)
                assert np.array_equal(a, b), (p, o, w, int((a != b).sum()))


# ---------------------------------------------------------------------------
# The film (GPU)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def add_samples_f64(scene, table, xy, li):
    """ImageTile::addSample for n samples: decisions in float32, sums in float64.  xy (n, 2) float32, li (n, 4) float32."""
    f = scene.desc.film
    xres, yres = int(f.xres), int(f.yres)
    wx, wy = np.float32(f.filter_width[0]), np.float32(f.filter_width[1])
    ceil_i = lambda v: int(np.ceil(np.float32(v)))
    xstart = ceil_i(np.float32(xres) * np.float32(f.crop[0]))
    xcount = max(1, ceil_i(np.float32(xres) * np.float32(f.crop[1])) - xstart)
    ystart = ceil_i(np.float32(yres) * np.float32(f.crop[2]))
    ycount = max(1, ceil_i(np.float32(yres) * np.float32(f.crop[3])) - ystart)
    film = np.zeros((yres, xres, 4), np.float64)
    ok = ~np.isnan(li[:, :3]).any(axis=1)
    xy, li = xy[ok], li[ok]
    dx = (xy[:, 0] - np.float32(0.5)).astype(np.float32)
    dy = (xy[:, 1] - np.float32(0.5)).astype(np.float32)
    x0 = np.maximum(np.ceil((dx - wx).astype(np.float32)).astype(np.int64), xstart)
    x1 = np.minimum(np.floor((dx + wx).astype(np.float32)).astype(np.int64), xstart + xcount - 1)
    y0 = np.maximum(np.ceil((dy - wy).astype(np.float32)).astype(np.int64), ystart)
    y1 = np.minimum(np.floor((dy + wy).astype(np.float32)).astype(np.int64), ystart + ycount - 1)
    bx, by = np.floor(dx).astype(np.int64), np.floor(dy).astype(np.int64)
    rx, ry = int(np.ceil(wx)) + 1, int(np.ceil(wy)) + 1
    L = li[:, :3].astype(np.float64)
    cells = 0
    for oy in range(-ry, ry + 1):
        y = by + oy
        iy = np.minimum(np.floor(np.abs(((np.float32(16) * (y.astype(np.float32) - dy)).astype(np.float32) / wy).astype(np.float32))), 15).astype(np.int64)
        for ox in range(-rx, rx + 1):
            x = bx + ox
            ix = np.minimum(np.floor(np.abs(((np.float32(16) * (x.astype(np.float32) - dx)).astype(np.float32) / wx).astype(np.float32))), 15).astype(np.int64)
            m = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
            w = table[iy[m] * 16 + ix[m]].astype(np.float64)
            np.add.at(film, (y[m], x[m], 0), w * L[m, 0])
            np.add.at(film, (y[m], x[m], 1), w * L[m, 1])
            np.add.at(film, (y[m], x[m], 2), w * L[m, 2])
            np.add.at(film, (y[m], x[m], 3), w)
            cells += int(m.sum())
    return film, cells


def shard_mask(window, spp, shard):
    """Which pixel-major samples of `window` belong to the 8x8 tiles of shard (index, count)."""
    x0, x1, y0, y1 = window
    tiles_x = (x1 - x0 + TILE - 1) // TILE
    ys, xs = np.mgrid[y0:y1, x0:x1]
    tile = ((ys - y0) // TILE) * tiles_x + (xs - x0) // TILE
    return np.repeat((tile % shard[1] == shard[0]).reshape(-1), spp)


def compare(label, device_film, ref, min_cells=1):
    dev = device_film.astype(np.float64)
    assert np.isfinite(dev).all()
    zero = ref == 0.0
    assert (dev[zero] == 0.0).all(), (label, "the device wrote where the restatement has nothing")
    rel = float((np.abs(dev - ref)[~zero] / np.abs(ref[~zero])).max()) if (~zero).any() else 0.0
    wrel = float((np.abs(dev[..., 3] - ref[..., 3])[ref[..., 3] != 0] / np.abs(ref[..., 3][ref[..., 3] != 0])).max())
    print("%s: max relative deviation %.4g (bar %.4g), weight plane %.4g (bar %.1g), pixels with weight %d of %d"
          % (label, rel, FILM_REL_TOL, wrel, WEIGHT_REL_TOL, int((ref[..., 3] != 0).sum()), ref[..., 3].size))
    assert ((dev[..., 3] != 0) == (ref[..., 3] != 0)).all(), label
    assert wrel <= WEIGHT_REL_TOL, (label, wrel)
    assert rel <= FILM_REL_TOL, (label, rel)
    return rel


_cache = {}


def cornell(spp, width):
    key = (spp, width)
    if key not in _cache:
        ov = gs.config_overrides(resolution=(20, 12), spp=spp, depth=3, filter={"type": "gaussian", "width": list(width)})
        scene = gs.load_scene("cornell", ov)
        _cache[key] = (scene, ob.Oracle(scene))
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["megakernel", "wavefront"])
@pytest.mark.parametrize("spp,width", [(1, (2.0, 2.0)), (5, (2.0, 2.0)), (67, (2.0, 2.0)), (5, (1.0, 2.0)), (5, (1.5, 2.0)), (67, (0.5, 0.5))])
def test_native_film_is_addsample_of_the_devices_radiance(torch, schedule, spp, width):
    """20 x 12 film (tiles clipped on both axes); sample counts that are no multiple of the four waves or of the staging block
    (1, 9 and 81 after the sampler's rounding to a square); power-of-two and true-division bins; a footprint under 5 x 5."""
    from goblin_amd.renderer import HipPathTracer
    scene, o = cornell(spp, width)
    seed = 4711
    out = HipPathTracer(scene, 0).render(seed=seed, want_li=True, schedule=schedule)
    samples = o.native_samples(seed)
    ref, cells = add_samples_f64(scene, o.filter_table(), samples[:, :2], out["li"].cpu().numpy())
    assert cells > 0
    compare("native %s spp %d width %s" % (schedule, spp, width), out["film"].numpy(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["megakernel", "wavefront"])
def test_unaligned_window_and_tile_shard(torch, schedule):
    from goblin_amd.renderer import HipPathTracer
    scene, o = cornell(5, (2.0, 2.0))
    r = HipPathTracer(scene, 0)
    seed = 99
    x0, x1, y0, y1 = r.window
    sub = (x0 + 3, x0 + 16, y0 + 2, y0 + 11)           # 13 x 9 pixels from an origin that is no multiple of 8
    out = r.render(seed=seed, want_li=True, window=sub, schedule=schedule)
    ref, _ = add_samples_f64(scene, o.filter_table(), o.native_samples(seed, window=sub)[:, :2], out["li"].cpu().numpy())
    compare("sub-window %s" % schedule, out["film"].numpy(), ref)
    out = r.render(seed=seed, want_li=True, shard=(1, 3), schedule=schedule)
    spp = out["paths"] // ((x1 - x0) * (y1 - y0))
    mine = shard_mask(r.window, spp, (1, 3))
    assert 0 < mine.sum() < mine.size
    ref, _ = add_samples_f64(scene, o.filter_table(), o.native_samples(seed)[mine, :2], out["li"].cpu().numpy()[mine])
    compare("shard (1, 3) %s" % schedule, out["film"].numpy(), ref)


@pytest.mark.gpu
def test_stream_sampler_film(torch):
    """GBL_SAMPLES_STREAM: the fast path with the image positions the stream kernel kept (RenderArgs::image_xy)."""
    from goblin_amd.renderer import HipPathTracer
    scene, o = cornell(5, (2.0, 2.0))
    res = o.render(threads=1, want_samples=True)
    spp = res["samples"].shape[0] // ((o.window()[1] - o.window()[0]) * (o.window()[3] - o.window()[2]))
    xy = res["samples"][helpers.tile_order_index(o.window(), spp)][:, :2]
    out = HipPathTracer(scene, 0).render(sampler="stream", want_li=True)
    ref, _ = add_samples_f64(scene, o.filter_table(), xy, out["li"].cpu().numpy())
    compare("stream", out["film"].numpy(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["megakernel", "wavefront"])
def test_replayed_records_anywhere_near_their_pixel(torch, schedule):
    """Arbitrary replay records take the general path (one LDS atomic per footprint cell): image positions up to 0.9 pixel
    outside their own pixel, whose footprints still lie inside the tile's halo."""
    from goblin_amd.renderer import HipPathTracer
    scene, o = cornell(5, (2.0, 2.0))
    r = HipPathTracer(scene, 0)
    samples = o.native_samples(7).copy()
    x0, x1, y0, y1 = r.window
    spp = samples.shape[0] // ((x1 - x0) * (y1 - y0))
    ys, xs = np.mgrid[y0:y1, x0:x1]
    rng = np.random.default_rng(5)
    samples[:, 0] = np.repeat(xs.reshape(-1), spp) + rng.uniform(-0.4, 1.4, samples.shape[0])
    samples[:, 1] = np.repeat(ys.reshape(-1), spp) + rng.uniform(-0.4, 1.4, samples.shape[0])
    out = r.render(replay_samples=samples, want_li=True, schedule=schedule)
    ref, _ = add_samples_f64(scene, o.filter_table(), samples[:, :2], out["li"].cpu().numpy())
    compare("replay %s" % schedule, out["film"].numpy(), ref)
