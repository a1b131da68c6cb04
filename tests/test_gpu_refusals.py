"""gbl_render's refusals: the status and the message of every check of the call's plan, which check wins when a call fails
several, the budgets of the per-sample buffers, a shard that owns no tile, and that a context renders as before after all of
them.  The parameter blocks are built straight from the ABI: HipPathTracer._params cannot express bad values."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from goblin_amd import _abi
from goblin_amd import scene as gs
from goblin_amd.renderer import HipPathTracer
import helpers

pytestmark = pytest.mark.gpu

SEED = 7
SHAPE = dict(resolution=(16, 16), spp=4, depth=2)   # a 20x20 sample window: 3x3 tiles of 8x8
FILM_RELL2_TOL = 2.5e-5          # summation order (tests/test_gpu_parity.py)
GBL_WHITTED_MAX_DEPTH = 12       # csrc/device_scene.h
INVALID, UNSUPPORTED = _abi.GBL_ERR_INVALID, _abi.GBL_ERR_UNSUPPORTED


def load(name, resolution, spp, depth):
    return gs.load_scene(name, gs.config_overrides(resolution=resolution, spp=spp, depth=depth))


@functools.lru_cache(maxsize=None)
def cornell():
    return HipPathTracer(load("cornell", **SHAPE), 0)


def params(r, **fields):
    """A valid parameter block of r's scene, then ``fields`` set as given."""
    s = r.scene.desc.setting
    p = _abi.gbl_render_params()
    p.integrator, p.sample_per_pixel, p.max_ray_depth = s.integrator, s.sample_per_pixel, s.max_ray_depth
    p.ao_sample_num, p.bssrdf_sample_num = s.ao_sample_num, s.bssrdf_sample_num
    p.sample_mode = _abi.GBL_SAMPLES_NATIVE
    p.seed = SEED
    p.schedule = _abi.GBL_SCHEDULE_AUTO
    p.stream = torch.cuda.current_stream(r.device).cuda_stream
    for name, value in fields.items():
        if name == "window":
            p.window[:] = value
        else:
            setattr(p, name, value)
    return p


def call(r, p, film=None, stats=None):
    """(status, message) of gbl_render."""
    film = r.new_film() if film is None else film
    st = r.lib.gbl_render(r.handle, C.byref(p), film.accum.data_ptr(), C.byref(stats) if stats is not None else None)
    return st, r.lib.gbl_last_error(r.handle).decode()


def off_grid(r):
    """Inside the sample window, its left edge not on the 8x8 tiling of the full window."""
    x0, x1, y0, y1 = r.window
    return (x0 + 3, x1, y0, y1)


# (fields, status, substring of gbl_last_error)
SINGLE = {
    "integrator": (dict(integrator=7), INVALID, "unknown integrator"),
    "spp": (dict(sample_per_pixel=0), INVALID, "must be >= 1"),
    "depth": (dict(max_ray_depth=0), INVALID, "must be >= 1"),
    "schedule": (dict(schedule=3), INVALID, "unknown schedule"),
    "window": (dict(window=(-3, 18, -2, 18)), INVALID, "outside the film's sample window"),
    "replay_null": (dict(sample_mode=_abi.GBL_SAMPLES_REPLAY, replay_samples=None), INVALID, "replay mode needs"),
    "sample_mode": (dict(sample_mode=9), INVALID, "unknown sample_mode"),
    "shard": (dict(tile_shard_index=2, tile_shard_count=2), INVALID, "tile_shard_index"),
    "stream_wavefront": (dict(sample_mode=_abi.GBL_SAMPLES_STREAM, schedule=_abi.GBL_SCHEDULE_WAVEFRONT), UNSUPPORTED, "megakernel schedule"),
    "stream_window": (lambda r: dict(sample_mode=_abi.GBL_SAMPLES_STREAM, window=off_grid(r)), INVALID, "whole 8x8 tiles"),
    "ao_wavefront": (dict(integrator=_abi.GBL_INTEGRATOR_AO, schedule=_abi.GBL_SCHEDULE_WAVEFRONT), UNSUPPORTED, "path tracer only"),
    "whitted_depth": (dict(integrator=_abi.GBL_INTEGRATOR_WHITTED, max_ray_depth=GBL_WHITTED_MAX_DEPTH + 1), UNSUPPORTED, "frame stack"),
}
# calls with several faults: the first check in plan_render's order wins
ORDER = {
    "integrator_before_spp": (dict(integrator=7, sample_per_pixel=0), INVALID, "unknown integrator"),
    "schedule_before_window": (dict(schedule=3, window=(-3, 18, -2, 18)), INVALID, "unknown schedule"),
    "window_before_replay": (dict(window=(-3, 18, -2, 18), sample_mode=_abi.GBL_SAMPLES_REPLAY, replay_samples=None), INVALID,
                             "outside the film's sample window"),
    "stream_schedule_before_tiles": (lambda r: dict(sample_mode=_abi.GBL_SAMPLES_STREAM, schedule=_abi.GBL_SCHEDULE_WAVEFRONT, window=off_grid(r)),
                                     UNSUPPORTED, "megakernel schedule"),
}
CASES = {**SINGLE, **ORDER}


def refuse(r, case):
    fields, status, text = CASES[case]
    st, msg = call(r, params(r, **(fields(r) if callable(fields) else fields)))
    print(case, "->", st, repr(msg))
    assert st == status, (case, st, msg)
    assert text in msg, (case, msg)


@pytest.mark.parametrize("case", sorted(SINGLE))
def test_refusal(case):
    refuse(cornell(), case)


@pytest.mark.parametrize("case", sorted(ORDER))
def test_first_check_wins(case):
    refuse(cornell(), case)


# Budgets ------------------------------------------------------------------------------------------------------------
BUDGET = 1 << 20   # GBL_LI_BUDGET_MB=1, read once per context


def budget_tracer(name, bytes_per_sample):
    """A fresh context of the scene on a 64x64 film, at the fewest (square) samples per pixel whose count crosses the budget at
    ``bytes_per_sample``."""
    over = gs.config_overrides(resolution=(64, 64), spp=1, depth=2)
    x0, x1, y0, y1 = HipPathTracer(gs.load_scene(name, over), 0).window
    npix = (x1 - x0) * (y1 - y0)
    root = next(k for k in range(1, 6) if npix * k * k * bytes_per_sample > BUDGET)
    assert 9 <= root * root <= 25 and npix * (root - 1) ** 2 * bytes_per_sample <= BUDGET
    over["render_setting"]["sample_per_pixel"] = root * root
    return HipPathTracer(gs.load_scene(name, over), 0), npix * root * root


@pytest.mark.parametrize("name,bytes_per_sample,text", [
    ("volume", 32, "32 bytes per camera sample"),
    ("whitted", 16, "16 bytes per camera sample of the call"),
    ("subsurface", 16, "subsurface materials keeps 16 bytes"),
])
def test_budget_refusal(name, bytes_per_sample, text, monkeypatch):
    monkeypatch.setenv("GBL_LI_BUDGET_MB", "1")
    r, entries = budget_tracer(name, bytes_per_sample)
    st, msg = call(r, params(r))
    print(name, entries, "camera samples ->", st, repr(msg))
    assert st == UNSUPPORTED and text in msg, (st, msg)
    # ... and under the default budget the same call renders
    monkeypatch.delenv("GBL_LI_BUDGET_MB")
    fresh = HipPathTracer(r.scene, 0)
    film = fresh.new_film()
    st, msg = call(fresh, params(fresh), film)
    torch.cuda.synchronize()
    assert st == _abi.GBL_OK, msg
    assert np.isfinite(film.numpy()).all() and film.numpy()[..., :3].max() > 0


def test_small_budget_renders_through_the_lds_tile(monkeypatch):
    """No medium, no subsurface material, native sampler, no li_out: a per-sample radiance buffer over the budget is no
    refusal.  plan_render's defer = li_out || entries * 16 <= budget is false, so the megakernel splats through its LDS tile as
    it goes instead of keeping the radiance for wf_splat; the film is the default budget's up to the summation order."""
    monkeypatch.setenv("GBL_LI_BUDGET_MB", "1")
    r, entries = budget_tracer("cornell", 16)
    assert entries * 16 > BUDGET
    film = r.new_film()
    p = params(r)
    assert not p.li_out
    st, msg = call(r, p, film)
    assert st == _abi.GBL_OK, msg
    monkeypatch.delenv("GBL_LI_BUDGET_MB")
    fresh = HipPathTracer(r.scene, 0)
    want = fresh.new_film()
    st, msg = call(fresh, params(fresh), want)
    assert st == _abi.GBL_OK, msg
    torch.cuda.synchronize()
    rel = helpers.rel_l2(film.numpy(), want.numpy())
    print("LDS tile splat against the deferred splat, film relL2", rel)
    assert want.numpy()[..., :3].max() > 0
    assert rel <= FILM_RELL2_TOL


# A shard that owns no tile --------------------------------------------------------------------------------------------
def test_shard_without_tiles_is_ok_and_touches_nothing():
    r = cornell()
    film = r.new_film()
    film.accum.copy_(torch.arange(film.accum.numel(), dtype=torch.float32, device=r.device).reshape(film.accum.shape) * 0.37 - 5.0)
    before = film.accum.clone()
    stats = _abi.gbl_stats()
    C.memset(C.byref(stats), 0xFF, C.sizeof(stats))
    x0, x1, y0, y1 = r.window
    tiles = ((x1 - x0 + 7) // 8) * ((y1 - y0 + 7) // 8)
    st, msg = call(r, params(r, tile_shard_index=tiles + 4, tile_shard_count=tiles + 5), film, stats)
    torch.cuda.synchronize()
    assert st == _abi.GBL_OK, msg
    assert bytes(stats) == bytes(C.sizeof(stats)), stats.as_dict()
    assert torch.equal(film.accum.view(torch.int32), before.view(torch.int32))


# Afterwards -----------------------------------------------------------------------------------------------------------
def test_context_renders_the_same_after_every_refusal():
    r = cornell()
    for case in sorted(CASES):
        refuse(r, case)
    li = r.render(seed=SEED, want_li=True, exact_ties=True)["li"].cpu().numpy()
    fresh = HipPathTracer(r.scene, 0).render(seed=SEED, want_li=True, exact_ties=True)["li"].cpu().numpy()
    assert li[:, :3].max() > 0
    np.testing.assert_array_equal(li, fresh)
