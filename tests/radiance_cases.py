"""TEST INFRASTRUCTURE for gbl_radiance_rays (tests/test_radiance_cpu.py, tests/test_gpu_radiance.py): the charts whose camera rays
the call is pinned on, the rays themselves, the ray counts around the 64-ray regions a wave owns, and the invalid-ray table.

A continuation ray of the reference is a RayDifferential without differentials, and a caller's ray is that object at vertex 0: if
the rays handed in are a frame's own camera rays, the answers are that frame's per-sample Li.  So the references are the ones the
surface charts (tests/surface_chart.py) already have: the oracle's Li, the compiled reference's logged Li and gbl_render's li_out.

Rays are (n, 8) float32 rows {o, mint, d, maxt}: gbl_ray's layout.
"""
import numpy as np

import surface_chart as sc

F32 = np.float32
SEED = 0x5EEDC0FFEE

# every path-traced chart but the thin-lens one: its camera ray needs a lens draw Oracle.camera_ray does not take
CHARTS = [c for c in sc.CASES if sc.is_path(c) and c != "thinlens"]
SUMMED = [c for c in sc.SUMMED if sc.is_path(c)]
TWINS = [c for c in sc.TWINS if c != "thinlens+ext"][:8]
BASES = [b for b in sc.BASES if sc.is_path(b)]

COUNTS = (0, 1, 63, 64, 65, 129, 257)   # around one and two regions of a wave, and past a workgroup's first round
UNIT_TOL = 1e-4                         # the call's validity bound on |d.d - 1| ...
UNIT_HEADROOM = 1e-5                    # ... and what the oracle's own normalise must stay within on the charts


def camera_rays(oracle, samples):
    """(n, 8) rays of the camera samples' image positions (columns 0, 1 of `samples`): Oracle.camera_ray gives {o, d, mint, maxt}."""
    samples = np.asarray(samples, F32)
    out = np.zeros((samples.shape[0], 8), F32)
    for i in range(samples.shape[0]):
        r = oracle.camera_ray(float(samples[i, 0]), float(samples[i, 1]))
        out[i] = [r[0], r[1], r[2], r[6], r[3], r[4], r[5], r[7]]
    return out


def _unit(scale):
    d = np.array([0.6, 0.0, 0.8], np.float64) * scale
    return [F32(d[0]), F32(d[1]), F32(d[2])]


# {o, mint, d, maxt}; origins are replaced by a valid neighbour's (mixed_rays), so an invalid ray that did enter would find the scene
INVALID_RAYS = np.array([
    [np.nan, 0, 0, 1e-3, 0, 0, 1, np.inf], [0, 0, 0, 1e-3, 0, np.nan, 1, np.inf], [0, 0, 0, np.nan, 0, 0, 1, np.inf], [0, 0, 0, 1e-3, 0, 0, 1, np.nan],   # a NaN component
    [0, np.inf, 0, 1e-3, 0, 0, 1, np.inf], [0, 0, 0, 1e-3, -np.inf, 0, 0, np.inf],   # an infinite component
    [0, 0, 0, 1e-3, 0, 0, 0, np.inf], [0, 0, 0, 1e-3, -0.0, 0.0, -0.0, np.inf],      # a zero direction
    [0, 0, 0, 2.0, 0, 0, 1, 1.0],                                                    # mint > maxt
    [0, 0, 0, 1e-3] + _unit(1.01) + [np.inf],                                        # |d| = 1.01
    [0, 0, 0, 1e-3] + _unit(0.5) + [np.inf],                                         # |d| = 0.5
], F32)


def mixed_rays(valid, every=7):
    """Rows of INVALID_RAYS in turn at every `every`-th position of `valid`, their finite origins moved to the replaced ray's.
    Returns (rays, is_valid)."""
    rays, ok = np.array(valid, F32), np.ones(len(valid), bool)
    for k, i in enumerate(range(3, len(valid), every)):
        bad = INVALID_RAYS[k % len(INVALID_RAYS)].copy()
        bad[0:3] = np.where(np.isfinite(bad[0:3]), valid[i, 0:3], bad[0:3])
        rays[i], ok[i] = bad, False
    return rays, ok


def unit_rays(rays):
    """`rays` with the directions normalised in float32 and t rescaled with them (query_cases' populations are not unit)."""
    out = np.array(rays, F32)
    norm = np.sqrt((out[:, 4:7] * out[:, 4:7]).sum(axis=1, dtype=F32)).astype(F32)
    out[:, 4:7] = out[:, 4:7] / norm[:, None]
    out[:, 7] = out[:, 7] * norm
    return out
