"""gbl_film_variance and gbl_film_denoise on the device against tests/denoise_reference.py, the contract in numpy.

"Within the bound" is |gpu - ref64| <= 8 max|ref32 - ref64| + 1e-6 max|ref64|, the right-hand side computed here on the same
inputs: ref32 is the kernel's arithmetic with numpy's exp, ref64 the same formula in double.  The factor 8 covers gbl_expf and
numpy's exp each being an ulp off in opposite directions in every weight, compounding over up to eight levels.  The variance
plane has no transcendental function in it and is compared bit for bit."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from goblin_amd import _abi
from goblin_amd import scene as gs
from goblin_amd.renderer import HipPathTracer
import aov_reference as ar
import denoise_reference as dr
import integration_helpers as ih

pytestmark = pytest.mark.gpu

F = np.float32
CLI = os.path.join(ih.REPO, "goblin_amd", "lib", "g_ray_hip")
GUIDES = ("variance", "albedo", "normal", "depth")
INVALID = _abi.GBL_ERR_INVALID


@functools.lru_cache(maxsize=None)
def cornell(width, height, spp=4, depth=4):
    return HipPathTracer(ar.scene("cornell", (width, height), spp, depth), 0)


def upload(a):
    return None if a is None else torch.from_numpy(np.array(a, copy=True)).cuda()


def run(r, film, guides, **params):
    """(device output as numpy, the uploaded tensors) of HipPathTracer.denoise on numpy inputs."""
    dev = {k: upload(v) for k, v in dict(film=film, **guides).items()}
    out = r.denoise(dev["film"], **{k: dev.get(k) for k in GUIDES}, **params)
    torch.cuda.synchronize()
    return out.numpy(), dev


def check_within_bound(gpu, film, guides, what, **params):
    ref32 = dr.denoise(film, dtype=np.float32, **guides, **params)
    ref64 = dr.denoise(film, dtype=np.float64, **guides, **params)
    gap = float(np.abs(ref32.astype(np.float64) - ref64).max())
    bound = dr.bound(ref32, ref64)
    err = float(np.abs(gpu.astype(np.float64) - ref64).max())
    err32 = float(np.abs(gpu.astype(np.float64) - ref32).max())
    print(what, "max|gpu - ref64| %.3g, max|ref32 - ref64| %.3g (ratio %.3g), bound %.3g, max|gpu - ref32| %.3g, largest value %.3g"
          % (err, gap, err / gap if gap else 0.0, bound, err32, float(np.abs(ref64).max())))
    assert np.isfinite(gpu).all(), what
    np.testing.assert_array_equal(gpu[..., 3], ref32[..., 3], err_msg=str(what))       # validity: decided in float32 by both
    assert err <= bound, (what, err, bound)


def all_guides(s):
    return {k: s[k] for k in GUIDES}


# 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds", [None, "0", "1"])
def test_six_levels_on_the_synthetic_film(lds, monkeypatch):
    """Stride 32 at 37 x 23: the halo exceeds both extents.  GBL_DENOISE_LDS forces the global-memory taps ("0") or, for the
    strides whose staged tile fits a workgroup's LDS (1 .. 8), the LDS taps ("1"); unset is the shipped choice per stride."""
    if lds is not None:
        monkeypatch.setenv("GBL_DENOISE_LDS", lds)
    s = dr.synthetic()
    r = cornell(37, 23)
    gpu, dev = run(r, s["film"], all_guides(s), iterations=6)
    check_within_bound(gpu, s["film"], all_guides(s), ("37x23", lds), iterations=6)
    again = r.denoise(dev["film"], **{k: dev[k] for k in GUIDES}, iterations=6)
    torch.cuda.synchronize()
    assert torch.equal(again.accum, upload(gpu))
    for k, t in dev.items():        # every input is as it was uploaded (bitwise: one of them holds a NaN)
        np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(s[k]).view(np.uint32), err_msg=k)


def test_both_level_kernels_compute_the_same_bits(monkeypatch):
    s = dr.synthetic()
    r = cornell(37, 23)
    monkeypatch.setenv("GBL_DENOISE_LDS", "0")
    a, _ = run(r, s["film"], all_guides(s), iterations=4)
    monkeypatch.setenv("GBL_DENOISE_LDS", "1")
    b, _ = run(r, s["film"], all_guides(s), iterations=4)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


# 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (5, 3)])
def test_tiny_images_at_eight_levels(shape):
    r = cornell(*shape)
    s = dr.synthetic(shape[0], shape[1], holes=shape != (1, 1))
    gpu, _ = run(r, s["film"], all_guides(s), iterations=8)
    check_within_bound(gpu, s["film"], all_guides(s), shape, iterations=8)
    assert gpu[..., 3].sum() >= 1
    dead = s["film"].copy()
    dead[..., 3] = 0.0
    gpu, _ = run(r, dead, all_guides(s), iterations=8)
    assert not gpu.any()
    dead = s["film"].copy()
    dead[..., 0] = np.nan
    gpu, _ = run(r, dead, all_guides(s), iterations=8)
    assert not gpu.any()


# 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", range(16))
def test_every_combination_of_guides(mask):
    s = dr.synthetic()
    guides = {k: s[k] for i, k in enumerate(GUIDES) if mask >> i & 1}
    demodulate = "albedo" in guides
    gpu, _ = run(cornell(37, 23), s["film"], guides, iterations=3, demodulate=demodulate)
    check_within_bound(gpu, s["film"], guides, sorted(guides), iterations=3, demodulate=demodulate)


# 4 ------------------------------------------------------------------------------------------------------------------
def test_an_edge_holds_exactly():
    """sigma_normal 0.1: across the halves |n_q - n_p|^2 / sigma^2 = 200 and expf(-200) is exactly 0 in float32, so a pixel is a
    convex combination of the valid pixels of its own half: 25 additions and one division, 26 x 2^-24 relative."""
    s = dr.synthetic()
    gpu, _ = run(cornell(37, 23), s["film"], all_guides(s), iterations=5, sigma_normal=0.1, demodulate=False)
    p = dr.prepare(s["film"], s["variance"], s["albedo"], s["normal"], s["depth"], demodulate=False)
    valid, left = p["valid"], s["left"]
    assert (~valid).sum() == 2
    np.testing.assert_array_equal(gpu[..., 3] == 1, valid)
    slack = 26 * 2.0 ** -24
    for half in (left, ~left):
        pix = valid & half
        assert pix.sum() > 100
        lo, hi = p["c"][pix].min(axis=0).astype(np.float64), p["c"][pix].max(axis=0).astype(np.float64)
        got = gpu[..., :3][pix].astype(np.float64)
        print("half: input range", lo, hi, "output range", got.min(axis=0), got.max(axis=0))
        assert (got >= lo * (1 - slack)).all() and (got <= hi * (1 + slack)).all()
    assert not gpu[~valid].any()


# 5 ------------------------------------------------------------------------------------------------------------------
def test_variance_is_the_restatement_bit_for_bit():
    r = cornell(37, 23)
    li = r.render(seed=7, want_li=True)["li"]
    torch.cuda.synchronize()
    x0, x1, y0, y1 = r.window
    poisoned = ((10 - y0) * (x1 - x0) + (12 - x0)) * 4 + 2      # sample 2 of pixel (12, 10)
    li[poisoned, 1] = float("nan")
    host = li.cpu().numpy()
    assert np.isnan(host).sum() == 1 and np.nanmax(host[:, :3]) > 0
    got = r.variance(li)
    torch.cuda.synchronize()
    want = dr.variance(host, r.window, 4, 37, 23)
    assert want.max() > 0 and np.isfinite(want).all() and want[10, 12] >= 0
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # a sub-window (it reaches into the filter border on the left) writes its own pixels only
    win = (x0, 9, 3, 17)
    rows = np.arange(win[2], win[3])[:, None] - y0
    cols = np.arange(win[0], win[1])[None, :] - x0
    index = ((rows * (x1 - x0) + cols).reshape(-1)[:, None] * 4 + np.arange(4)[None, :]).reshape(-1)
    plane = torch.full((23, 37), -1.0, dtype=torch.float32, device=r.device)
    st = r.lib.gbl_film_variance(r.handle, upload(host[index]).data_ptr(), (C.c_int32 * 4)(*win), 4, plane.data_ptr(),
                                 torch.cuda.current_stream(r.device).cuda_stream)
    torch.cuda.synchronize()
    assert st == _abi.GBL_OK, r.lib.gbl_last_error(r.handle)
    plane = plane.cpu().numpy()
    np.testing.assert_array_equal(plane[3:17, 0:9].view(np.uint32), want[3:17, 0:9].view(np.uint32))
    outside = np.ones((23, 37), bool)
    outside[3:17, 0:9] = False
    assert (plane[outside] == -1).all()
    # one sample per pixel has no variance
    setting = _abi.gbl_render_setting.from_buffer_copy(r.scene.desc.setting)
    setting.sample_per_pixel = 1
    with pytest.raises(_abi.GoblinError) as e:
        r.variance(li[::4].contiguous(), setting=setting)
    assert e.value.status == INVALID and "sample_per_pixel" in str(e.value)


# 6 ------------------------------------------------------------------------------------------------------------------
def test_end_to_end_on_cornell():
    r = cornell(64, 64)
    beauty = r.render(seed=7, want_li=True)
    aov = r.render_aov(seed=7)
    variance = r.variance(beauty["li"])
    out = r.denoise(beauty["film"], variance, aov["albedo"], aov["normal"], aov["depth"], iterations=3)
    torch.cuda.synchronize()
    film = beauty["film"].numpy()
    guides = dict(variance=variance.cpu().numpy(), albedo=aov["albedo"].numpy(), normal=aov["normal"].numpy(), depth=aov["depth"].numpy())
    check_within_bound(out.numpy(), film, guides, "cornell 64x64", iterations=3)
    clean = cornell(64, 64, 256).render(seed=11)["film"].normalized().cpu().numpy()
    before = dr.rel_mse(beauty["film"].normalized().cpu().numpy(), clean)
    after = dr.rel_mse(out.normalized().cpu().numpy(), clean)
    print("Cornell 64^2, 4 spp on the device: relMSE noisy %.4g, denoised %.4g, ratio %.3f" % (before, after, after / before))
    assert after <= 0.5 * before
    developed = r.develop(out, want_rgb8=True)
    torch.cuda.synchronize()
    assert torch.isfinite(developed["rgb"]).all() and developed["rgb"].max() > 0 and developed["rgb8"].max() > 0


# 7 ------------------------------------------------------------------------------------------------------------------
def raw_call(r, t, **change):
    """(status, message) of gbl_film_denoise called straight through the ABI: valid arguments over the tensors ``t``, then
    ``change`` applied -- a params field, or an argument by name (None for NULL)."""
    p = _abi.gbl_denoise_params()
    p.iterations, p.sigma_luminance, p.sigma_normal, p.sigma_albedo, p.sigma_depth, p.demodulate = 3, 4.0, 0.5, 0.1, 0.1, 1
    p.stream = torch.cuda.current_stream(r.device).cuda_stream
    args = {k: t[k].data_ptr() for k in ("film", "variance", "albedo", "normal", "depth", "out")}
    args["ctx"], args["params"] = r.handle, C.byref(p)
    for k, v in change.items():
        if k in args:
            args[k] = v
        else:
            setattr(p, k, v)
    st = r.lib.gbl_film_denoise(args["ctx"], args["film"], args["variance"], args["albedo"], args["normal"], args["depth"], args["params"], args["out"])
    return st, r.lib.gbl_last_error(r.handle).decode()


def test_refusals():
    r = cornell(37, 23)
    s = dr.synthetic()
    t = {k: upload(s[k]) for k in ("film",) + GUIDES}
    t["out"] = torch.zeros((23, 37, 4), dtype=torch.float32, device=r.device)
    nan, inf = float("nan"), float("inf")
    cases = [(dict(film=None), "film_accum"), (dict(params=None), "params"), (dict(out=None), "film_out"),
             (dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"), (dict(iterations=-1), "iterations"),
             (dict(albedo=None), "demodulate"),
             (dict(out=t["film"].data_ptr()), "alias"), (dict(out=t["normal"].data_ptr()), "alias"),
             (dict(out=t["film"].data_ptr() + 16), "alias")]
    for field in ("sigma_luminance", "sigma_normal", "sigma_albedo", "sigma_depth"):
        cases += [({field: bad}, field) for bad in (0.0, -1.0, nan, inf)]
    for change, text in cases:
        st, msg = raw_call(r, t, **change)
        print(change, "->", st, repr(msg))
        assert st == INVALID and text in msg, (change, st, msg)
    assert raw_call(r, t, ctx=None)[0] == INVALID
    # a sigma is checked only when its film is read
    st, msg = raw_call(r, t, normal=None, sigma_normal=-1.0)
    assert st == _abi.GBL_OK, msg
    st, msg = raw_call(r, t, albedo=None, demodulate=0, sigma_albedo=nan)
    assert st == _abi.GBL_OK, msg
    # ... and the context filters as before
    st, msg = raw_call(r, t)
    torch.cuda.synchronize()
    assert st == _abi.GBL_OK, msg
    check_within_bound(t["out"].cpu().numpy(), s["film"], all_guides(s), "after the refusals", iterations=3)


def test_python_face_drops_demodulation_without_an_albedo_film():
    """gbl_film_denoise refuses demodulate without albedo_accum (test_refusals); HipPathTracer.denoise, whose demodulate defaults
    to True, passes it on only when there is an albedo film, as its docstring says."""
    s = dr.synthetic()
    r = cornell(37, 23)
    guides = dict(variance=s["variance"], normal=s["normal"], depth=s["depth"])
    default, _ = run(r, s["film"], guides, iterations=2)
    off, _ = run(r, s["film"], guides, iterations=2, demodulate=False)
    np.testing.assert_array_equal(default.view(np.uint32), off.view(np.uint32))
    check_within_bound(default, s["film"], guides, "no albedo, demodulate left at its default", iterations=2, demodulate=False)


def test_keeping_li_changes_neither_schedule_nor_film():
    """g_ray_hip --denoise hands its one gbl_render call an li_out where the frame's li fits the per-sample budget: the call then
    runs under the schedule it runs under without, and the film is the same up to its float summation order."""
    r = cornell(32, 32, 4, 3)
    plain = r.render(seed=0, timed=True)
    kept = r.render(seed=0, timed=True, want_li=True)
    torch.cuda.synchronize()
    assert plain["stats"]["schedule"] == kept["stats"]["schedule"] != 0
    a, b = plain["film"].numpy().astype(np.float64), kept["film"].numpy().astype(np.float64)
    rel = float(np.linalg.norm(a - b) / np.linalg.norm(a))
    print("film with li_out against without, relL2 %.3g" % rel)
    assert kept["li"][:, :3].max() > 0 and rel <= 2.5e-5


# 8 ------------------------------------------------------------------------------------------------------------------
FILM_RELL2_TOL = 2.5e-5     # two renders of one frame: the film's float summation order (tests/test_gpu_parity.py)


def pixels(data):
    return np.frombuffer(data[-32 * 32 * 12:], "<f4")


@functools.lru_cache(maxsize=None)
def tool_runs():
    """g_ray_hip on Cornell 32 x 32, 4 spp: twice without --denoise, once with.  The files' bytes by run, the listings, stderr."""
    import tempfile
    out = {}
    for run_name, flags in (("plain", []), ("plain_again", []), ("denoise", ["--denoise=3"])):
        with tempfile.TemporaryDirectory() as d:
            js, image = os.path.join(d, "cornell.json"), os.path.join(d, "cornell.pfm")
            ih.write_scene("cornell", gs.config_overrides(resolution=(32, 32), spp=4, depth=3), js, film_file=image)
            p = subprocess.run([CLI, js] + flags, capture_output=True, text=True, timeout=120)
            assert p.returncode == 0 and "Render Complete" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
            out[run_name] = dict(files={f: open(os.path.join(d, f), "rb").read() for f in os.listdir(d)}, stderr=p.stderr)
    return out


def test_command_line_tool_writes_the_denoised_image():
    runs = tool_runs()
    assert sorted(runs["plain"]["files"]) == ["cornell.json", "cornell.pfm"]
    assert sorted(runs["denoise"]["files"]) == ["cornell.denoised.pfm", "cornell.json", "cornell.pfm"]
    assert "variance" not in runs["denoise"]["stderr"]          # 32 x 32 x 4 samples fit any budget: the variance plane is used
    image, same_frame = pixels(runs["plain"]["files"]["cornell.pfm"]), pixels(runs["denoise"]["files"]["cornell.pfm"])
    denoised = pixels(runs["denoise"]["files"]["cornell.denoised.pfm"])
    assert len(runs["denoise"]["files"]["cornell.denoised.pfm"]) == len(runs["plain"]["files"]["cornell.pfm"])
    assert np.isfinite(denoised).all() and denoised.max() > 0 and not np.array_equal(denoised, image)
    assert abs(float(denoised.mean()) - float(image.mean())) <= 0.25 * float(image.mean())
    # the image itself is the frame a run without the flag renders, up to the film's float summation order
    rel = float(np.linalg.norm(same_frame.astype(np.float64) - image) / np.linalg.norm(image.astype(np.float64)))
    print("image with --denoise against the image without, relL2 %.3g" % rel)
    assert rel <= FILM_RELL2_TOL


def tool_run(tmp_path, name, shape, flags):
    d = tmp_path / name
    d.mkdir()
    js, image = str(d / "cornell.json"), str(d / "cornell.pfm")
    ih.write_scene("cornell", gs.config_overrides(**shape), js, film_file=image)
    p = subprocess.run([CLI, js] + flags, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "Render Complete" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    return {f: open(str(d / f), "rb").read() for f in os.listdir(str(d))}, p.stderr


def test_command_line_tool_leaves_the_image_byte_identical(tmp_path):
    """The ordinary output of a run with --denoise against a run without the flag, byte for byte.

    Bytes can only be compared where the tool writes the same bytes twice.  gbl_render's film goes through wf_splat, whose four
    waves add their lanes' sums into the LDS tile and whose tiles add into the film with float atomics, in the order the hardware
    schedules them: at 32 x 32 and 4 spp two runs WITHOUT the flag differed in 971 and in 1104 of 3072 floats in two sessions
    (relL2 7.4e-8 and 4.6e-8), just as a run with the flag differed from one without (987 and 891 floats, relL2 1.1e-7 and
    7.8e-8); the test above holds that frame, whose render keeps li_out, to the summation-order tolerance.  The order is fixed where only one wave of a tile's workgroup has a sample (1 spp: a wave's LDS atomics retire in
    program order) and no film pixel collects from more than two tiles (a single row of tiles: 0 + a + b = 0 + b + a), so this
    frame is 28 x 4 at 1 spp: a 32 x 8 sample window, four tiles in a row.  Two runs without the flag must agree first.  With
    one sample per pixel there is no variance to take: the tool filters without the plane and says so, which is checked too."""
    shape = dict(resolution=(28, 4), spp=1, depth=3)
    plain, _ = tool_run(tmp_path, "plain", shape, [])
    again, _ = tool_run(tmp_path, "again", shape, [])
    flagged, err = tool_run(tmp_path, "flagged", shape, ["--denoise=2"])
    assert sorted(plain) == ["cornell.json", "cornell.pfm"]
    assert sorted(flagged) == ["cornell.denoised.pfm", "cornell.json", "cornell.pfm"]
    assert again["cornell.pfm"] == plain["cornell.pfm"]
    assert flagged["cornell.pfm"] == plain["cornell.pfm"]
    assert "without a variance plane" in err
    image = np.frombuffer(plain["cornell.pfm"][-28 * 4 * 12:], "<f4")
    denoised = np.frombuffer(flagged["cornell.denoised.pfm"][-28 * 4 * 12:], "<f4")
    assert np.isfinite(denoised).all() and denoised.max() > 0 and image.max() > 0 and not np.array_equal(denoised, image)
