"""gbl_film_variance / gbl_film_denoise without a GPU: the ABI (header, ctypes mirror, exported names) and the numpy restatement
of the contract the GPU tests compare against (tests/denoise_reference.py) -- its float32 / float64 gap, what it does to a
noisy Cornell box rendered by the oracle, that it leaves a pixel of zero variance alone, and how it treats holes."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np

from goblin_amd import _abi
import aov_reference as ar
import denoise_reference as dr
import oracle_binding as ob

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_abi(tmp_path):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "goblin_hip.h")).read(), flags=re.S)
    for name in ("gbl_film_variance", "gbl_film_denoise"):
        assert re.search(r"\bgbl_status\s+%s\s*\(" % name, header), name
        assert name in _abi.HIP_SYMBOLS
    fields = ["iterations", "sigma_luminance", "sigma_normal", "sigma_albedo", "sigma_depth", "demodulate", "stream"]
    src = tmp_path / "sizes.c"
    body = 'printf("size %zu\\n", sizeof(gbl_denoise_params));\n'
    body += "".join('printf("%s %%zu\\n", offsetof(gbl_denoise_params, %s));\n' % (f, f) for f in fields)
    src.write_text('#include <stdio.h>\n#include "goblin_hip.h"\nint main(void){\n' + body + "return 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])   # plain C
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert C.sizeof(_abi.gbl_denoise_params) == int(out["size"])
    for f in fields:
        assert getattr(_abi.gbl_denoise_params, f).offset == int(out[f]), f
    assert [f for f, _ in _abi.gbl_denoise_params._fields_] == fields
    assert _abi.GBL_ABI_VERSION == 14      # new entry points only: no existing layout changed


def test_float32_against_float64_on_the_synthetic_film():
    """The float32 restatement (the kernel's arithmetic) against the same formula in float64, six levels.  Per level a pixel is
    a normalised sum of 25 products: some 60 roundings of 2^-24 each, and the exponent -(e + g2), rounded at a magnitude of up
    to ~20 where the weight still matters, moves a weight by up to ~4e-6 relative -- about 1e-5 per level, 6e-5 over six, of
    the largest value.  The gap is printed (recorded in DESIGN.md 4.6) and held under 1e-4 of the largest value."""
    s = dr.synthetic()
    guides = dict(variance=s["variance"], albedo=s["albedo"], normal=s["normal"], depth=s["depth"])
    ref32 = dr.denoise(s["film"], dtype=np.float32, iterations=6, **guides)
    ref64 = dr.denoise(s["film"], dtype=np.float64, iterations=6, **guides)
    assert ref32.dtype == np.float32 and ref64.dtype == np.float64
    gap, top = float(np.abs(ref32.astype(np.float64) - ref64).max()), float(np.abs(ref64).max())
    print("float32 against float64: max gap %.3g at a largest value of %.3g (%.3g relative)" % (gap, top, gap / top))
    assert 10.0 < top < 20.0
    assert gap <= 1e-4 * top
    np.testing.assert_array_equal(ref32[..., 3], ref64[..., 3])      # validity is decided in float32 in both


@functools.lru_cache(maxsize=None)
def cornell(spp):
    """Cornell 64 x 64, depth 4, through the oracle: 4 spp (seed 7) with its variance and feature films, or the 256 spp (seed 11)
    film it is measured against."""
    scene = ar.scene("cornell", (64, 64), spp, 4)
    if spp == 256:
        oracle = ob.Oracle(scene)
        return dict(film=oracle.splat(oracle.native_samples(11), oracle.li_native(11, threads=ob.hardware_threads())))
    ref = ar.Reference(scene, seed=7)
    li = ref.oracle.li_native(7)
    out = dict(film=ref.oracle.splat(ref.samples, li), variance=dr.variance(li, ref.window, spp, 64, 64), **ref.films())
    return out


def test_quality_on_cornell():
    noisy, clean = cornell(4), ob.normalize_film(cornell(256)["film"])
    out = dr.denoise(noisy["film"], noisy["variance"], noisy["albedo"], noisy["normal"], noisy["depth"], iterations=3)
    assert (out[..., 3] == 1).all()
    before, after = dr.rel_mse(ob.normalize_film(noisy["film"]), clean), dr.rel_mse(out[..., :3], clean)
    print("Cornell 64^2, 4 spp: relMSE noisy %.4g, denoised %.4g, ratio %.3f" % (before, after, after / before))
    assert after <= 0.5 * before


def ladder(shape, rng):
    """Colours whose luminances are pairwise at least 2.4e-4 apart: a distinct multiple of 2^-12 per pixel, plus 0, 1/4, 1/2 in
    the three channels.  Every value has at most 13 significant bits."""
    H, W = shape
    g = (rng.permutation(H * W).reshape(H, W) + 1).astype(F) / F(4096.0)
    return np.stack([g, g + F(0.25), g + F(0.5)], -1).astype(F)


def taps_are_apart(c, valid, iterations):
    """Every pair of pixels a tap of the first ``iterations`` levels joins differs by more than 1e-4 in luminance."""
    l = dr.lum(c[..., 0], c[..., 1], c[..., 2])
    for level in range(iterations):
        s = 1 << level
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if (dx or dy):
                    pair = valid & dr.shift(valid, s * dy, s * dx)
                    if pair.any() and np.abs(dr.shift(l, s * dy, s * dx) - l)[pair].min() <= 1e-4:
                        return False
    return True


def test_zero_variance_leaves_the_pixel_alone():
    """Variance 0 makes the luminance weight 1 / 1e-6 per unit: a neighbour more than 1e-4 away weighs expf(-100) = 4e-44 at
    most, which changes neither the sum nor the weight sum, and the pixel comes out as (h c) / h with h = 9/64.  That is c
    exactly whenever h c is exact in float32 -- colours of at most 20 significant bits, the first case -- and within one rounding
    per level otherwise: the second case, demodulated, whose c / d uses the whole mantissa."""
    rng = np.random.default_rng(5)
    H, W = 23, 37
    zeros = np.zeros((H, W), F)
    c = ladder((H, W), rng)
    film = np.concatenate([c, np.ones((H, W, 1), F)], -1)
    assert taps_are_apart(c, np.ones((H, W), bool), 3)
    out = dr.denoise(film, variance=zeros, iterations=3)
    np.testing.assert_array_equal(out[..., :3], c)
    assert (out[..., 3] == 1).all()
    # demodulated: film = (c d) w with the synthetic film's albedo and weights
    s = dr.synthetic()
    alb = s["albedo"][..., :3] / s["albedo"][..., 3:]
    weight = np.where(s["film"][..., 3:] > 0, s["film"][..., 3:], F(1.0))
    film = (np.concatenate([c * np.where(alb >= F(1e-2), alb, F(1.0)), np.ones((H, W, 1), F)], -1) * weight).astype(F)
    p = dr.prepare(film, zeros, s["albedo"])
    assert p["valid"].all() and (p["d"] != 1).any() and taps_are_apart(p["c"], p["valid"], 3)
    out = dr.denoise(film, variance=zeros, albedo=s["albedo"], iterations=3)
    want = p["c"] * p["d"]
    assert np.abs(out[..., :3] - want).max() <= 4 * 2.0 ** -23 * np.abs(want).max()
    assert (np.abs(out[..., :3] - want) <= 4 * 2.0 ** -23 * np.abs(want)).all()


def test_holes():
    s = dr.synthetic()
    H, W = s["left"].shape
    hole, nan = (H // 2, W // 4), (1, (3 * W) // 4)
    assert s["film"][hole][3] == 0 and np.isnan(s["film"][nan]).any()
    for guides in (dict(), dict(variance=s["variance"], albedo=s["albedo"], normal=s["normal"], depth=s["depth"])):
        out = dr.denoise(s["film"], iterations=4, **guides)
        assert not out[hole].any() and not out[nan].any()
        rest = np.ones((H, W), bool)
        rest[hole] = rest[nan] = False
        assert np.isfinite(out[rest]).all() and (out[rest][:, 3] == 1).all()
        assert (out[rest][:, :3] > 0).all()
        # an invalid pixel gives nothing to a neighbour: the same film with other values in the holes filters to the same image
        other = s["film"].copy()
        other[hole] = (5.0, 5.0, 5.0, 0.0)
        other[nan] = (np.inf, 1.0, 1.0, 1.0)
        np.testing.assert_array_equal(dr.denoise(other, iterations=4, **guides), out)


def test_variance_restatement():
    """Against the textbook formula in float64 on random samples, and its rules: non-finite samples are dropped, fewer than two
    left give 0, the border of the window is ignored, pixels outside the window are not written."""
    rng = np.random.default_rng(3)
    window, S = (-2, 9, -2, 7), 4
    ww, wh = window[1] - window[0], window[3] - window[2]
    li = rng.uniform(0.0, 3.0, (wh, ww, S, 4)).astype(F)
    li[3, 4, 1, 0] = np.nan          # pixel (2, 1): three samples left
    li[4, 5, :3, 1] = np.inf         # pixel (3, 2): one sample left
    out = np.full((5, 7), F(-1.0))
    got = dr.variance(li.reshape(-1, 4), window, 3, 7, 5, out=out)      # spp 3 rounds up to 4
    assert got is out and got.dtype == F
    l = (0.2126 * li[..., 0].astype(np.float64) + 0.7152 * li[..., 1]) + 0.0722 * li[..., 2]
    for y in range(5):
        for x in range(7):
            k = l[y + 2, x + 2]
            k = k[np.isfinite(k)]
            want = k.var(ddof=1) / len(k) if len(k) >= 2 else 0.0
            assert abs(got[y, x] - want) <= 1e-5 * max(want, 1e-3), (x, y)
    assert got[2, 3] == 0 and got[1, 2] > 0
    sub = dr.variance(li[2:4, 3:6].reshape(-1, 4), (1, 4, 0, 2), 4, 7, 5, out=np.full((5, 7), F(-1.0)))
    np.testing.assert_array_equal(sub[0:2, 1:4], got[0:2, 1:4])
    assert (sub[2:] == -1).all() and (sub[:, 0] == -1).all() and (sub[:, 4:] == -1).all()
