"""The lean quad path kernels take their work wave by wave (kernels/render_kernels.h wave_take): a wave owns a unit -- a band of rows
of a tile x a chunk of samples -- hands its paths to its idle lanes, and takes the next unit in the same regeneration round when that
one runs out, so lanes of one wave hold paths of two units and no wave waits for another.  A sample's radiance is a function of
(pixel, k, seed) alone, so whichever wave and lane a path lands on, the per-sample radiance must be bit for bit what the renderings
that do not run this loop give: the wavefront schedule, and the one-ray-per-lane megakernel (GBL_MK_QUAD=0), which keeps the
workgroup's item loop.  Every sample must be written exactly once (li[:, 3] == 1 over a buffer that starts at zero), with and without
exact_ties, with the primary pass and (the marked cases) without it.  The shapes are the smallest at which the loop can go wrong:
fewer units than waves, units far smaller than a wave, a chunk size that is no multiple of 64, clipped edge tiles whose lower bands
are empty, strided tiles, runs of units the primary pass found nothing in, an instanced scene, long paths.
"""
import math
import os

import numpy as np
import pytest

from goblin_amd import scene as gs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _sky_camera():
    """bunny.json's camera (its floor fills the frame) opened to 100 degrees and rolled by 150 degrees about its own axis: the horizon
    crosses the frame on a slant, so rows of tiles end in runs of tiles that see nothing, and the last rows see nothing at all."""
    w, x, y, z = 0.352428, 0.114509, -0.883349, 0.287014
    c, s = math.cos(math.radians(75.0)), math.sin(math.radians(75.0))   # q * (c, 0, 0, s)
    return {"orientation": [w * c - z * s, x * c + y * s, y * c - x * s, w * s + z * c], "fov": 100.0}


def _with(overrides, camera):
    o = dict(overrides)
    o["camera"] = dict(o.get("camera", {}), **camera)
    return o


CASES = [
    # id, scene, overrides, render kwargs, also without the primary pass
    ("fewer-units-than-waves", "bunny", gs.config_overrides(resolution=(8, 8), spp=4, depth=3), {}, False),
    ("units-below-a-wave", "bunny", gs.config_overrides(resolution=(24, 16), spp=4, depth=4), {}, True),
    ("partly-filled-chunk", "bunny", gs.config_overrides(resolution=(64, 64), spp=100, depth=4), {}, False),
    ("clipped-edge-tiles", "bunny", gs.config_overrides(resolution=(96, 96), spp=16, depth=4), {"window": "inner"}, True),
    ("strided-tiles", "bunny", gs.config_overrides(resolution=(96, 96), spp=16, depth=4), {"shard": (1, 3)}, False),
    ("all-miss-units", "bunny", _with(gs.config_overrides(resolution=(96, 96), spp=16, depth=4), _sky_camera()), {}, False),
    ("instanced", "grid", gs.config_overrides(resolution=(64, 64), spp=32, depth=4), {}, False),
    ("long-paths", "cornell", gs.config_overrides(resolution=(64, 64), spp=32, depth=6), {}, False),
]
# smallest case first; the runs of one case stand together, so its context and reference renderings live only that long
PARAMS = [(c, primary, exact) for c in CASES for exact in (False, True) for primary in ([True, False] if c[4] else [True])]

_refs = {}   # of the case in hand only: "renderer" -> (case id, renderer, render kwargs); exact -> the two renderings that do not run the wave loop


def _render(r, exact, kwargs, schedule="megakernel", env=None):
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        return r.render(seed=424243, want_li=True, schedule=schedule, exact_ties=exact, **kwargs)
    finally:
        for k in (env or {}):
            os.environ.pop(k, None)


def _reference(case, exact):
    if _refs.get("renderer", (None,))[0] != case[0]:
        _refs.clear()   # (drops the previous case's context and tensors)
        from goblin_amd.renderer import HipPathTracer
        r = HipPathTracer(gs.load_scene(case[1], case[2]), 0)
        kw = dict(case[3])
        if kw.get("window") == "inner":
            x0, x1, y0, y1 = r.window
            kw["window"] = (x0 + 9, x1 - 14, y0 + 5, y1 - 3)   # not tile aligned: edge tiles with clipped pixels
        _refs["renderer"] = (case[0], r, kw)
    _, r, kw = _refs["renderer"]
    if exact not in _refs:
        wavefront = _render(r, exact, kw, schedule="wavefront")
        one_ray = _render(r, exact, kw, env={"GBL_MK_QUAD": "0"})
        _refs[exact] = (wavefront["li"], one_ray["li"], wavefront["film"].numpy().copy())
    return (r, kw) + _refs[exact]


@pytest.fixture(scope="module", autouse=True)
def _free_the_last_case():
    yield
    _refs.clear()


def _tiles_without_radiance(r, kw, li, spp):
    """Per 8x8 tile of the render window (row-major, as the work units are numbered): True where no sample carries radiance"""
    x0, x1, y0, y1 = kw.get("window") or r.window
    w, h = x1 - x0, y1 - y0
    lit = (li[:, :3] != 0).any(dim=1).reshape(h, w, spp).any(dim=2).cpu().numpy()
    ty, tx = (h + 7) // 8, (w + 7) // 8
    pad = np.zeros((ty * 8, tx * 8), bool)
    pad[:h, :w] = lit
    return ~pad.reshape(ty, 8, tx, 8).any(axis=(1, 3))


@pytest.mark.parametrize("case,primary,exact", PARAMS,
                         ids=["%s-%s%s" % (c[0], "exact_ties" if e else "lean", "" if p else "-no-primary") for c, p, e in PARAMS])
def test_wave_owned_units_give_every_sample_its_radiance(torch, case, primary, exact):
    r, kw, li_wavefront, li_one_ray, film_ref = _reference(case, exact)
    out = _render(r, exact, kw, env=None if primary else {"GBL_PRIMARY": "0"})
    li = out["li"]
    written = li[:, 3] == 1
    if "shard" in kw:   # the other ranks' tiles stay as the buffer started
        assert torch.equal(written, li_wavefront[:, 3] == 1) and bool(written.any())
        assert bool((li[~written] == 0).all())
    else:
        assert bool(written.all())
    assert torch.isfinite(li).all()
    assert torch.equal(li, li_wavefront)
    assert torch.equal(li, li_one_ray)
    # (the film sums the same radiance; tiles add their halos with float atomics, whose order is free)
    np.testing.assert_allclose(out["film"].numpy(), film_ref, rtol=1e-5, atol=1e-6)
    assert float(li[:, :3].sum()) > 0.0


def test_the_all_miss_case_has_runs_of_units_with_nothing_in_them(torch):
    """What the all-miss case relies on, read off the reference rendering and the first-hit records: whole tiles whose camera rays
    all left the scene (no hit, no radiance) -- the last one of the range among them, and one in the middle of it, followed by a
    tile that has hits."""
    case = [c for c in CASES if c[0] == "all-miss-units"][0]
    r, kw, li_wavefront, _, _ = _reference(case, False)
    spp = li_wavefront.shape[0] // ((r.window[1] - r.window[0]) * (r.window[3] - r.window[2]))
    dark = _tiles_without_radiance(r, kw, li_wavefront, spp)
    aov = r.render_aov(want_samples=True, seed=424243)
    hit = torch.zeros_like(li_wavefront)
    hit[:, 0] = (aov["samples_i32"][:, 11] != 0).float()
    missed = _tiles_without_radiance(r, kw, hit, spp)
    empty = (dark & missed).ravel()
    assert empty[-1], "the last tile of the range sees something"
    assert (empty[:-1] & ~missed.ravel()[1:]).any(), "no empty tile is followed by one with hits"
    assert empty.sum() >= dark.shape[1], "less than a row of tiles is empty"
