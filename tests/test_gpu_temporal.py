"""gbl_update_camera / gbl_get_camera and gbl_film_accumulate on the device.

The camera edit is held against a context created with the edited camera: the same per-sample radiance, bit for bit.  The
accumulation is held against tests/temporal_reference.py, the contract in numpy float32: there is no transcendental function in
it, so every output plane is compared bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from goblin_amd import _abi
from goblin_amd import scene as gs
from goblin_amd.renderer import HipPathTracer
import aov_reference as ar
import denoise_reference as dr
import temporal_reference as tr

pytestmark = pytest.mark.gpu

F = np.float32
INVALID = _abi.GBL_ERR_INVALID
FILM_RELL2_TOL = 2.5e-5     # two renders of one frame: the film's float summation order (tests/test_gpu_parity.py)


@functools.lru_cache(maxsize=None)
def cornell(width, height, spp=4, depth=4):
    return HipPathTracer(ar.scene("cornell", (width, height), spp, depth), 0)


def as_gbl(cam):
    """gbl_camera of a temporal_reference.camera dict."""
    out = _abi.gbl_camera()
    for name in tr.CAMERA_FIELDS:
        if name in ("position", "orientation"):
            getattr(out, name)[:] = cam[name]
        else:
            setattr(out, name, cam[name])
    return out


def fields(cam):
    return {name: (tuple(getattr(cam, name)) if name in ("position", "orientation") else getattr(cam, name)) for name in tr.CAMERA_FIELDS}


def set_camera(r, cam):
    f = fields(cam if isinstance(cam, _abi.gbl_camera) else as_gbl(cam))
    r.update_camera(f.pop("position"), f.pop("orientation"), **f)


def upload(a):
    return None if a is None else torch.from_numpy(np.array(a, copy=True)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# 1 ------------------------------------------------------------------------------------------------------------------
CAM1 = dict(position=(0.1, 1.05, -3.5), orientation=(float(np.cos(0.03)), 0.0, float(np.sin(0.03)), 0.0))
LENS = dict(lens_radius=0.05, focal_distance=3.6)


def fresh_context(**camera_fields):
    """A context CREATED with the Cornell camera edited in the description (no scene file is involved, so a thin lens brings no
    lens disk instance with it: the same scene as an edited context's)."""
    scene = gs.load_scene("cornell", gs.config_overrides(resolution=(24, 16), spp=4, depth=3))
    for name, value in camera_fields.items():
        if name in ("position", "orientation"):
            getattr(scene.desc.camera, name)[:] = value
        else:
            setattr(scene.desc.camera, name, value)
    return HipPathTracer(scene, 0)


def frame(r):
    out = {}
    for schedule in ("megakernel", "wavefront"):
        got = r.render(seed=3, want_li=True, schedule=schedule)
        out[schedule] = (got["li"].cpu().numpy(), got["film"].numpy())
    out["aov"] = r.render_aov(seed=3, want_samples=True)["samples_i32"].cpu().numpy()
    torch.cuda.synchronize()
    return out


def same_frame(a, b, what):
    for schedule in ("megakernel", "wavefront"):
        np.testing.assert_array_equal(bits(a[schedule][0]), bits(b[schedule][0]), err_msg="%s li %s" % (what, schedule))
        fa, fb = a[schedule][1].astype(np.float64), b[schedule][1].astype(np.float64)
        rel = float(np.linalg.norm(fa - fb) / np.linalg.norm(fb))
        print(what, schedule, "film relL2 %.3g" % rel)
        assert rel <= FILM_RELL2_TOL and np.abs(fb).max() > 0, (what, schedule, rel)
    np.testing.assert_array_equal(a["aov"], b["aov"], err_msg="%s aov records" % what)


def test_camera_edit_equals_a_fresh_context():
    a = fresh_context()
    cam0 = a.camera()
    assert fields(cam0) == fields(a.scene.desc.camera)
    first = frame(a)
    a.update_camera(**CAM1)
    got = fields(a.camera())
    assert got["position"] == tuple(float(F(v)) for v in CAM1["position"]) and got["orientation"] == tuple(float(F(v)) for v in CAM1["orientation"])
    assert got["fov_degrees"] == cam0.fov_degrees and got["lens_radius"] == 0.0 and got["type"] == 0
    moved = frame(a)
    same_frame(moved, frame(fresh_context(**CAM1)), "edited to camera 1")
    assert not np.array_equal(moved["megakernel"][0], first["megakernel"][0])
    # pinhole -> thin lens: the EXT kernels
    a.update_camera(**LENS)
    assert fields(a.camera())["lens_radius"] == float(F(LENS["lens_radius"]))
    lens = frame(a)
    same_frame(lens, frame(fresh_context(**CAM1, **LENS)), "edited to a thin lens")
    assert not np.array_equal(lens["megakernel"][0], moved["megakernel"][0])
    # ... and back to camera 0 and the lean kernels: its own first render
    set_camera(a, cam0)
    assert fields(a.camera()) == fields(cam0)
    back = frame(a)
    same_frame(back, first, "back at camera 0")
    # refusals leave the camera alone
    bad_type, bad_pos = a.camera(), a.camera()
    bad_type.type = 7
    bad_pos.position[1] = float("nan")
    for arg, text in ((None, "NULL"), (C.byref(bad_type), "unknown camera type"), (C.byref(bad_pos), "position")):
        st = a.lib.gbl_update_camera(a.handle, arg)
        msg = a.lib.gbl_last_error(a.handle).decode()
        print(text, "->", st, repr(msg))
        assert st == INVALID and text in msg
    assert a.lib.gbl_update_camera(None, C.byref(cam0)) == INVALID and a.lib.gbl_get_camera(a.handle, None) == INVALID
    assert fields(a.camera()) == fields(cam0)
    same_frame(frame(a), first, "after the refusals")


# 2 ------------------------------------------------------------------------------------------------------------------
PLANES = ("film", "variance", "history")


def run(r, s, variance, normal, history, **override):
    """(device outputs as numpy, the uploaded tensors) of HipPathTracer.accumulate on the fixture's numpy inputs, under the
    fixture's current camera."""
    set_camera(r, s["cur_camera"])
    dev = dict(film=upload(s["film"]), depth=upload(s["depth"]), variance=upload(s["variance"]) if variance else None,
               normal=upload(s["normal"]) if normal else None, history=upload(s["history"]) if history else None)
    out = r.accumulate(dev["film"], dev["depth"], dev["variance"], dev["normal"], dev["history"], as_gbl(s["prev_camera"]) if history else None,
                       **dict(s["params"], **override))
    torch.cuda.synchronize()
    return dict(film=out["film"].numpy(), variance=out["variance"].cpu().numpy(), history=out["history"].cpu().numpy()), dev


def restated(s, variance, normal, history, **override):
    return tr.accumulate(s["film"], s["depth"], s["cur_camera"], variance=s["variance"] if variance else None, normal=s["normal"] if normal else None,
                         history=s["history"] if history else None, prev_camera=s["prev_camera"], **dict(s["params"], **override))


def check_bits(gpu, ref, what):
    # the decisions first, so that a failure names them: validity, the history length, which pixels have history
    np.testing.assert_array_equal(gpu["film"][..., 3] == 1, ref["valid"], err_msg="%s validity" % (what,))
    np.testing.assert_array_equal(bits(gpu["history"][0, ..., 3]), bits(ref["N"]), err_msg="%s N" % (what,))
    for k in PLANES:
        diff = int((bits(gpu[k]) != bits(ref[k])).sum())
        print(what, k, "words that differ:", diff, "of", gpu[k].size)
        np.testing.assert_array_equal(bits(gpu[k]), bits(ref[k]), err_msg="%s %s" % (what, k))


@pytest.mark.parametrize("variance", [False, True])
@pytest.mark.parametrize("normal", [False, True])
def test_the_contract_bit_for_bit(variance, normal):
    """37 x 23: no multiple of the 32 x 8 tile."""
    s = tr.synthetic_sequence()
    r = cornell(37, 23)
    gpu, dev = run(r, s, variance, normal, True)
    ref = restated(s, variance, normal, True)
    assert ref["has_history"].sum() > 100 and (ref["valid"] & ~ref["has_history"]).sum() > 50
    check_bits(gpu, ref, ("37x23", variance, normal))
    again = r.accumulate(dev["film"], dev["depth"], dev["variance"], dev["normal"], dev["history"], as_gbl(s["prev_camera"]), **s["params"])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(again["film"].numpy()), bits(gpu["film"]))
    np.testing.assert_array_equal(bits(again["variance"].cpu().numpy()), bits(gpu["variance"]))
    np.testing.assert_array_equal(bits(again["history"].cpu().numpy()), bits(gpu["history"]))
    for k, t in dev.items():        # every input is as it was uploaded (bitwise: the film holds a NaN)
        if t is not None:
            np.testing.assert_array_equal(bits(t.cpu().numpy()), bits(s[k]), err_msg=k)


# 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variance", [False, True])
def test_first_frame(variance):
    s = tr.synthetic_sequence()
    gpu, _ = run(cornell(37, 23), s, variance, True, False)
    ref = restated(s, variance, True, False)
    check_bits(gpu, ref, ("first frame", variance))
    valid = ref["valid"]
    with np.errstate(all="ignore"):
        resolved = (s["film"][..., :3] * (F(1.0) / s["film"][..., 3])[..., None]).astype(F)
    np.testing.assert_array_equal(gpu["film"][..., :3][valid], resolved[valid])
    assert (gpu["film"][..., 3][valid] == 1).all() and not gpu["film"][~valid].any()
    assert (gpu["history"][0, ..., 3][valid] == 1).all() and not gpu["history"][:, ~valid].any()
    if variance:
        np.testing.assert_array_equal(gpu["variance"][valid], s["variance"][valid])
    else:
        assert gpu["variance"][valid].max() > 0      # the spatial estimate (compared with the restatement above)
    assert not gpu["variance"][~valid].any()


# 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (33, 9)])
def test_tiny_and_awkward_sizes(shape):
    """33 x 9 is one pixel past a tile in both directions."""
    r = cornell(*shape)
    s = tr.synthetic_sequence(shape[0], shape[1])
    for variance in (False, True):
        gpu, _ = run(r, s, variance, True, True)
        check_bits(gpu, restated(s, variance, True, True), (shape, variance))
        assert gpu["film"][..., 3].sum() >= 1
    dead = dict(s)
    dead["film"] = s["film"].copy()
    dead["film"][..., 3] = 0.0
    for variance in (False, True):
        gpu, _ = run(r, dead, variance, True, True)
        assert not gpu["film"].any() and not gpu["variance"].any() and not gpu["history"].any()


# 5 ------------------------------------------------------------------------------------------------------------------
def raw_call(r, t, prev_camera, **change):
    """(status, message) of gbl_film_accumulate called straight through the ABI: valid arguments over the tensors ``t``, then
    ``change`` applied -- a params field, or an argument by name (None for NULL)."""
    p = _abi.gbl_temporal_params()
    p.prev_camera = prev_camera
    p.alpha_min, p.max_history, p.sigma_depth, p.cos_normal = 0.1, 8.0, 0.05, 0.9
    p.stream = torch.cuda.current_stream(r.device).cuda_stream
    names = ("film", "variance", "normal", "depth", "history", "history_out", "film_out", "variance_out")
    args = {k: t[k].data_ptr() for k in names}
    args["ctx"], args["params"] = r.handle, C.byref(p)
    for k, v in change.items():
        if k in args:
            args[k] = v
        elif k == "prev_type":
            p.prev_camera.type = v
        else:
            setattr(p, k, v)
    st = r.lib.gbl_film_accumulate(args["ctx"], args["film"], args["variance"], args["normal"], args["depth"], args["history"], args["history_out"],
                                   args["params"], args["film_out"], args["variance_out"])
    return st, r.lib.gbl_last_error(r.handle).decode()


def test_refusals():
    r = cornell(37, 23)
    s = tr.synthetic_sequence()
    set_camera(r, s["cur_camera"])
    # the inputs in one allocation, each in a slot the size of a history and a little more: an output put on one input, the largest
    # (history_out) included, then overlaps that input and no other
    names = ("film", "variance", "normal", "depth", "history")
    slot = 3 * 23 * 37 * 4 + 64
    arena = torch.zeros(len(names) * slot, dtype=torch.float32, device=r.device)
    t = {}
    for i, k in enumerate(names):
        t[k] = arena[i * slot:i * slot + s[k].size].view(s[k].shape)
        t[k].copy_(upload(s[k]))
    t["history_out"] = torch.full((3, 23, 37, 4), -1.0, dtype=torch.float32, device=r.device)
    t["film_out"] = torch.full((23, 37, 4), -1.0, dtype=torch.float32, device=r.device)
    t["variance_out"] = torch.full((23, 37), -1.0, dtype=torch.float32, device=r.device)
    prev = as_gbl(s["prev_camera"])
    nan, inf = float("nan"), float("inf")
    ptr = {k: v.data_ptr() for k, v in t.items()}
    cases = [(dict(film=None), "film_accum"), (dict(depth=None), "depth_accum"), (dict(history_out=None), "history_out"), (dict(params=None), "params"),
             (dict(film_out=None), "film_out"), (dict(prev_type=7), "prev_camera.type"),
             (dict(history_out=ptr["history"]), "history_in"), (dict(history_out=ptr["history"] + 16 * 37 * 23), "history_in"),
             (dict(history_out=ptr["history"] - 16), "history_in")]
    for bad in (0.0, -0.5, 1.5, nan, inf):
        cases.append((dict(alpha_min=bad), "alpha_min"))
    for bad in (0.5, 0.0, -1.0, nan, inf):
        cases.append((dict(max_history=bad), "max_history"))
    for bad in (0.0, -1.0, nan, inf):
        cases.append((dict(sigma_depth=bad), "sigma_depth"))
    for bad in (-1.5, 1.5, nan, inf):
        cases.append((dict(cos_normal=bad), "cos_normal"))
    for out in ("film_out", "variance_out", "history_out"):
        for name, text in (("film", "film_accum"), ("variance", "variance"), ("normal", "normal_accum"), ("depth", "depth_accum"), ("history", "history_in")):
            cases.append(({out: ptr[name]}, text))
        cases.append(({out: ptr["depth"] + 8}, "depth_accum"))
    for change, text in cases:
        st, msg = raw_call(r, t, prev, **change)
        print(change, "->", st, repr(msg))
        assert st == INVALID and text in msg and "gbl_film_accumulate" in msg, (change, st, msg)
    assert raw_call(r, t, prev, ctx=None)[0] == INVALID
    torch.cuda.synchronize()
    for k in ("history_out", "film_out", "variance_out"):
        assert (t[k] == -1).all(), k          # nothing was written
    # what a call does not read is not checked
    st, msg = raw_call(r, t, prev, normal=None, cos_normal=5.0)
    assert st == _abi.GBL_OK, msg
    st, msg = raw_call(r, t, prev, history=None, prev_type=7)
    assert st == _abi.GBL_OK, msg
    st, msg = raw_call(r, t, prev, variance_out=None)
    assert st == _abi.GBL_OK, msg
    # ... and the context accumulates as before
    st, msg = raw_call(r, t, prev)
    torch.cuda.synchronize()
    assert st == _abi.GBL_OK, msg
    gpu = dict(film=t["film_out"].cpu().numpy(), variance=t["variance_out"].cpu().numpy(), history=t["history_out"].cpu().numpy())
    check_bits(gpu, restated(s, True, True, True), "after the refusals")


# 6 ------------------------------------------------------------------------------------------------------------------
FRAMES = 8
TRAVEL = 0.1      # the box is 2 units wide: 5 % of it over the eight frames


def camera_of_frame(cam0, i):
    x = cam0.position[0] + TRAVEL * (i / (FRAMES - 1) - 1.0)      # the last frame is the scene's own camera
    return (x, cam0.position[1], cam0.position[2])


@pytest.mark.parametrize("with_variance", [True, False])
def test_end_to_end_on_cornell(with_variance):
    """Eight frames of 4 spp along a sideways move, accumulated; the last against 256 spp from the last camera.  Both assertions
    compare with what the last frame alone gives: more samples must not make the image worse, so neither has a margin."""
    r = cornell(64, 64)
    cam0 = as_gbl(fields(r.scene.desc.camera))
    history, prev = None, None
    for i in range(FRAMES):
        r.update_camera(position=camera_of_frame(cam0, i))
        beauty = r.render(seed=i, want_li=True)
        aov = r.render_aov(seed=i)
        variance = r.variance(beauty["li"])
        acc = r.accumulate(beauty["film"], aov["depth"], variance if with_variance else None, aov["normal"], history, prev)
        history, prev = acc["history"], r.camera()
    single = r.denoise(beauty["film"], variance, aov["albedo"], aov["normal"], aov["depth"], iterations=3)
    both = r.denoise(acc["film"], acc["variance"], aov["albedo"], aov["normal"], aov["depth"], iterations=3)
    torch.cuda.synchronize()
    assert fields(r.camera()) == fields(cam0)
    N = history[0, ..., 3].cpu().numpy()
    clean = cornell(64, 64, 256).render(seed=11)["film"].normalized().cpu().numpy()
    noisy = dr.rel_mse(beauty["film"].normalized().cpu().numpy(), clean)
    accumulated = dr.rel_mse(acc["film"].normalized().cpu().numpy(), clean)
    denoised_single = dr.rel_mse(single.normalized().cpu().numpy(), clean)
    denoised_both = dr.rel_mse(both.normalized().cpu().numpy(), clean)
    print("Cornell 64^2, 8 x 4 spp on the device, variance plane %s: history length mean %.2f, max %.2f; relMSE single frame %.4g, accumulated %.4g "
          "(ratio %.3f); single frame denoised %.4g, accumulated then denoised %.4g (ratio %.3f)" %
          (with_variance, N.mean(), N.max(), noisy, accumulated, accumulated / noisy, denoised_single, denoised_both, denoised_both / denoised_single))
    assert abs(N.max() - FRAMES) < 0.01 and torch.isfinite(acc["film"].accum).all() and torch.isfinite(acc["variance"]).all()
    assert accumulated < noisy
    assert denoised_both <= denoised_single
    developed = r.develop(acc["film"], want_rgb8=True)
    torch.cuda.synchronize()
    assert torch.isfinite(developed["rgb"]).all() and developed["rgb8"].max() > 0
