"""gbl_get_instances, gbl_render_motion and gbl_film_accumulate_motion on the device.

The accumulation is held against tests/motion_reference.py bit for bit, like gbl_film_accumulate against its restatement.  The
motion planes are held against the gbl_render_aov records of the same centre rays: the instance exactly, on every pixel, and the
reprojection against the restatement evaluated from the record's hit distance.  No getter exposes the device's float32 instance
matrices, so the restatement composes them in float64 and each plane is compared under temporal_reference.bound(float32
restatement, float64 restatement)."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

from goblin_amd import _abi
from goblin_amd import scene as gs
from goblin_amd.renderer import HipPathTracer
import aov_reference as ar
import motion_reference as mr
import temporal_reference as tr

pytestmark = pytest.mark.gpu

F = np.float32
INVALID = _abi.GBL_ERR_INVALID
PLANES = ("film", "variance", "history")


@functools.lru_cache(maxsize=None)
def tracer(name, width, height, spp=1, depth=4, tag=""):
    """One context per (scene, size, tag); a test that edits one restores it."""
    return HipPathTracer(ar.scene(name, (width, height), spp, depth), 0)


def as_gbl(cam):
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


def check_bits(gpu, ref, what):
    np.testing.assert_array_equal(gpu["film"][..., 3] == 1, ref["valid"], err_msg="%s validity" % (what,))
    np.testing.assert_array_equal(bits(gpu["history"][0, ..., 3]), bits(ref["N"]), err_msg="%s N" % (what,))
    for k in PLANES:
        diff = int((bits(gpu[k]) != bits(ref[k])).sum())
        print(what, k, "words that differ:", diff, "of", gpu[k].size)
        np.testing.assert_array_equal(bits(gpu[k]), bits(ref[k]), err_msg="%s %s" % (what, k))


# 1 ------------------------------------------------------------------------------------------------------------------
def run(r, s, variance, normal, history):
    set_camera(r, s["cur_camera"])
    dev = dict(film=upload(s["film"]), depth=upload(s["depth"]), variance=upload(s["variance"]) if variance else None,
               normal=upload(s["normal"]) if normal else None, history=upload(s["history"]) if history else None, motion=upload(s["motion"]))

    def call():
        out = r.accumulate(dev["film"], dev["depth"], dev["variance"], dev["normal"], dev["history"], None, motion=dev["motion"], **s["params"])
        torch.cuda.synchronize()
        return dict(film=out["film"].numpy(), variance=out["variance"].cpu().numpy(), history=out["history"].cpu().numpy())
    return call(), dev, call


def restated(s, variance, normal, history):
    return mr.accumulate_motion(s["film"], s["depth"], s["motion"], variance=s["variance"] if variance else None, normal=s["normal"] if normal else None,
                                history=s["history"] if history else None, **s["params"])


@pytest.mark.parametrize("variance", [False, True])
@pytest.mark.parametrize("normal", [False, True])
def test_accumulate_motion_bit_for_bit(variance, normal):
    """37 x 23: no multiple of the 32 x 8 tile.  The context is only a film size here: the planes are the fixture's."""
    s = mr.moving_sequence()
    gpu, dev, call = run(tracer("cornell", 37, 23), s, variance, normal, True)
    ref = restated(s, variance, normal, True)
    assert ref["has_history"].sum() > 100 and (ref["valid"] & ~ref["has_history"]).sum() > 50
    check_bits(gpu, ref, ("37x23", variance, normal))
    again = call()
    for k in PLANES:
        np.testing.assert_array_equal(bits(again[k]), bits(gpu[k]), err_msg="second call %s" % k)
    for k, t in dev.items():        # every input is as it was uploaded (bitwise: the film holds a NaN)
        if t is not None:
            np.testing.assert_array_equal(bits(t.cpu().numpy()), bits(s[k]), err_msg=k)


@pytest.mark.parametrize("variance", [False, True])
def test_accumulate_motion_first_frame(variance):
    s = mr.moving_sequence()
    gpu, _, _ = run(tracer("cornell", 37, 23), s, variance, True, False)
    ref = restated(s, variance, True, False)
    check_bits(gpu, ref, ("first frame", variance))
    valid = ref["valid"]
    assert (gpu["history"][0, ..., 3][valid] == 1).all() and not gpu["history"][:, ~valid].any()


@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (8, 8), (9, 9), (33, 9)])
def test_accumulate_motion_tiny_and_awkward_sizes(shape):
    r = tracer("cornell", *shape)
    s = mr.moving_sequence(shape[0], shape[1])
    for variance in (False, True):
        gpu, _, _ = run(r, s, variance, True, True)
        check_bits(gpu, restated(s, variance, True, True), (shape, variance))
        assert gpu["film"][..., 3].sum() >= 1


# 2 ------------------------------------------------------------------------------------------------------------------
def centre_records(r):
    """The AOV records of the centre rays: t (H, W), instance (H, W), position (H, W, 3), and the normal film of the same call."""
    h, w = r.info.yres, r.info.xres
    dims = _abi.host_lib().gbl_host_sample_dimension_scene(C.byref(r.scene.desc), C.byref(r.scene.desc.setting))
    rec = np.zeros((h * w, dims), F)
    ys, xs = np.mgrid[0:h, 0:w]
    rec[:, 0], rec[:, 1] = xs.ravel() + 0.5, ys.ravel() + 0.5
    out = r.render_aov(albedo=False, normal=True, depth=False, want_samples=True, replay_samples=rec, window=(0, w, 0, h))
    torch.cuda.synchronize()
    rows = out["samples"].cpu().numpy().reshape(h, w, 12)
    ints = out["samples_i32"].cpu().numpy().reshape(h, w, 12)
    return dict(t=rows[..., 3].copy(), inst=ints[..., 7].copy(), position=rows[..., 8:11].copy(), hit=ints[..., 11] != 0, normal=out["normal"].accum)


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw)


def check_planes(r, rec, prev_camera, prev_instances, what, expect_ok=None):
    """Device planes against the restatement from the records; returns the device planes."""
    gpu = r.motion(as_gbl(prev_camera), prev_instances, normal=rec["normal"]).cpu().numpy()
    cur_camera, cur_instances = fields(r.camera()), r.instances()
    normal = rec["normal"].cpu().numpy()
    t = np.where(rec["hit"], rec["t"], F(0.0))
    inst = np.where(rec["hit"], rec["inst"], -1)
    # the instance under EVERY pixel, exactly
    np.testing.assert_array_equal(gpu[1, ..., 3].astype(np.int64) - 1, inst, err_msg="%s: M1.w - 1 against the records' instance" % what)
    np.testing.assert_array_equal(gpu[1, ..., 3], (inst + 1).astype(F))
    ref32 = mr.motion_planes(t, inst, cur_camera, prev_camera, cur_instances, prev_instances, normal, T=F)
    ref64 = mr.motion_planes(t, inst, cur_camera, prev_camera, cur_instances, prev_instances, normal, T=np.float64)
    ok = ref64[0, ..., 3] != 0
    np.testing.assert_array_equal(gpu[0, ..., 3] != 0, ok, err_msg="%s: ok" % what)
    assert set(np.unique(gpu[0, ..., 3])) <= {0.0, 1.0}
    assert not gpu[0][~ok].any(), "%s: a texel without ok is all zeros" % what
    assert not ok[~rec["hit"]].any()
    if expect_ok is not None:
        np.testing.assert_array_equal(ok, expect_ok, err_msg="%s: which pixels are ok" % what)
    for k, name in ((0, "M0"), (1, "M1")):
        tol = tr.bound(ref32[k], ref64[k])
        err = float(np.abs(gpu[k].astype(np.float64) - ref64[k]).max())
        print("%s %s: largest difference from the float64 restatement %.3g, bound %.3g (hits %d of %d, ok %d)" % (what, name, err, tol, rec["hit"].sum(), ok.size, ok.sum()))
        assert err <= tol, (what, name, err, tol)
    return gpu, tr.bound(ref32[0], ref64[0])


def grid_moves(r):
    """The six instance edits of test_instance_edits_rebuild_the_tlas_in_place: each moved, turned by 45 degrees and grown."""
    with open(gs.scene_path("grid")) as f:
        doc = json.load(f)
    inst = [p for p in doc["primitives"] if p["type"] == "instance"]
    moves = []
    for k in range(6):
        p = inst[k]
        pos = [p["position"][0] * 1.3 + 0.1 * k, p["position"][1] + 0.15 * k, p["position"][2] * 0.8 - 0.05 * k]
        scale = [s * (1.0 + 0.1 * k) for s in p.get("scale", [1, 1, 1])]
        moves.append((pos, [0.9238795, 0.0, 0.3826834, 0.0], scale))
    return moves


@pytest.mark.parametrize("case", [("grid", 40, 40, ""), ("grid", 9, 9, ""), ("textured", 40, 40, ""), ("grid", 40, 40, "ortho")])
def test_motion_planes_against_the_aov_records(case):
    name, w, h, tag = case
    r = tracer(name, w, h, 1, 4, tag)
    if tag == "ortho":
        r.update_camera(type=_abi.GBL_CAMERA_ORTHOGRAPHIC, film_width=6.0)
    rec = centre_records(r)
    hit = rec["hit"]
    assert hit.sum() > 0.3 * hit.size
    cam = fields(r.camera())
    # no motion: every hit pixel reprojects onto itself
    gpu, tol = check_planes(r, rec, cam, None, "%s no motion" % (case,), expect_ok=hit)
    ys, xs = np.mgrid[0:h, 0:w]
    err = max(np.abs(gpu[0, ..., 0] - (xs + 0.5))[hit].max(), np.abs(gpu[0, ..., 1] - (ys + 0.5))[hit].max())
    print(case, "no motion: M0.xy off the pixel centre by at most %.3g (allowed %.3g); misses %d" % (err, tol, (~hit).sum()))
    assert err <= tol
    # the unedited transforms passed explicitly are "no instance moved", bit for bit
    same = r.motion(as_gbl(cam), r.instances(), normal=rec["normal"]).cpu().numpy()
    np.testing.assert_array_equal(bits(same), bits(gpu))
    # camera move only
    moved_cam = dict(cam, position=(cam["position"][0] + 0.2, cam["position"][1] - 0.1, cam["position"][2] + 0.15),
                     orientation=quat_mul(cam["orientation"], (float(np.cos(0.02)), 0.0, float(np.sin(0.02)), 0.0)))
    moved_cam = tr.camera(**{k: moved_cam[k] for k in ("position", "orientation", "fov_degrees", "type", "film_width", "lens_radius", "focal_distance",
                                                          "near_plane", "far_plane")})
    check_planes(r, rec, moved_cam, None, "%s camera move" % (case,))
    # the previous camera turned away by 180 degrees: nothing lies in front of it
    away = tr.camera(**dict({k: cam[k] for k in ("position", "fov_degrees", "type", "film_width", "lens_radius", "focal_distance", "near_plane", "far_plane")},
                            orientation=quat_mul(cam["orientation"], (0.0, 0.0, 1.0, 0.0))))
    gpu_away, _ = check_planes(r, rec, away, None, "%s turned away" % (case,), expect_ok=np.zeros_like(hit))
    assert not gpu_away[0].any()
    # six instances moved (grid): the previous transforms are the scene's, the current ones the edited
    if name == "grid":
        before = r.instances()
        try:
            r.update_instances(0, grid_moves(r))
            rec2 = centre_records(r)
            assert mr.moved_instances(r.instances(), before) == list(range(6))
            on_moved = rec2["hit"] & (rec2["inst"] < 6)
            gpu2, _ = check_planes(r, rec2, cam, before, "%s six instances moved" % (case,))
            carried = np.abs(gpu2[1, ..., :3] - tr.prepare(np.ones((h, w, 4), F), None, rec2["normal"].cpu().numpy(), np.ones((h, w, 4), F))["n"])[on_moved]
            print(case, "pixels on a moved instance %d; the normal carried back differs from n by up to %.3g" % (on_moved.sum(), carried.max() if carried.size else 0.0))
            if (w, h) == (40, 40):
                assert on_moved.sum() >= 20 and carried.max() > 0.05        # the carry-back is not the identity
            # ... and the other way round: back to the scene's transforms, the edited ones as the previous frame
            edited = r.instances()
            r.update_instances(0, before[:6])
            assert r.instances() == before
            check_planes(r, centre_records(r), moved_cam, edited, "%s moved back, camera moved" % (case,))
        finally:
            r.update_instances(0, before[:6])


# 3 ------------------------------------------------------------------------------------------------------------------
def test_instances_round_trip():
    r = tracer("grid", 9, 9)
    desc = r.scene.desc
    first = r.instances()
    assert len(first) == desc.num_instances == r.info.instances
    for i, (pos, quat, scale) in enumerate(first):
        tw = desc.instances[i].to_world
        assert (pos, quat, scale) == (tuple(tw.position), tuple(tw.orientation), tuple(tw.scale))
    # the unedited transforms as the previous frame: no instance moved, the bits of prev_instances=None
    cam = r.camera()
    np.testing.assert_array_equal(bits(r.motion(cam, first).cpu().numpy()), bits(r.motion(cam, None).cpu().numpy()))
    moves = grid_moves(r)
    try:
        r.update_instances(0, moves)
        got = r.instances()
        for k, (pos, quat, scale) in enumerate(moves):
            assert got[k] == (tuple(float(F(v)) for v in pos), tuple(float(F(v)) for v in quat), tuple(float(F(v)) for v in scale))
        assert got[6:] == first[6:]
        buf = (_abi.gbl_trs * 2)()
        assert r.lib.gbl_get_instances(r.handle, 4, 2, buf) == _abi.GBL_OK and tuple(buf[1].position) == got[5][0]
        n = len(first)
        for args in ((None, 0, 1, buf), (r.handle, 0, 1, None), (r.handle, n, 1, buf), (r.handle, n - 1, 2, buf), (r.handle, 0xffffffff, 2, buf)):
            assert r.lib.gbl_get_instances(*args) == INVALID, args
        assert r.lib.gbl_get_instances(r.handle, n, 0, buf) == _abi.GBL_OK
    finally:
        r.update_instances(0, first[:6])
    assert r.instances() == first


# 4 ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    r = tracer("grid", 9, 9)
    n = 9 * 9
    cam = r.camera()
    normal = torch.zeros((9, 9, 4), dtype=torch.float32, device=r.device)
    normal[..., 2], normal[..., 3] = -2.0, 2.0
    arena = torch.full((4 * n * 4,), -1.0, dtype=torch.float32, device=r.device)        # room for the planes and a film inside them
    out = arena[:2 * n * 4]
    prev = r.instances()
    good = r.motion(cam, prev, normal=normal).cpu().numpy()

    def call(params=True, motion_out=True, **change):
        p = _abi.gbl_motion_params()
        p.prev_camera = cam
        arr = (_abi.gbl_trs * len(prev))()
        for i, (pos, quat, scale) in enumerate(prev):
            arr[i].position[:], arr[i].orientation[:], arr[i].scale[:] = pos, quat, scale
        p.prev_to_world = arr
        p.normal_accum = normal.data_ptr()
        p.stream = torch.cuda.current_stream(r.device).cuda_stream
        for k, v in change.items():
            if k == "prev_type":
                p.prev_camera.type = v
            elif k == "normal":
                p.normal_accum = v
            else:
                i, field, j, value = v
                getattr(arr[i], field)[j] = value
        st = r.lib.gbl_render_motion(r.handle, C.byref(p) if params else None, out.data_ptr() if motion_out is True else motion_out)
        return st, r.lib.gbl_last_error(r.handle).decode()
    nan, inf = float("nan"), float("inf")
    cases = [(dict(params=False), INVALID, "params"), (dict(motion_out=None), INVALID, "motion_out"), (dict(prev_type=7), INVALID, "prev_camera.type"),
             (dict(normal=out.data_ptr()), INVALID, "normal_accum"), (dict(normal=out.data_ptr() + 2 * n * 16 - 16), INVALID, "normal_accum"),
             (dict(normal=out.data_ptr() - n * 16 + 16), INVALID, "normal_accum"),
             (dict(edit=(3, "position", 1, nan)), INVALID, "not finite"), (dict(edit=(0, "scale", 2, inf)), INVALID, "not finite"),
             (dict(edit=(2, "orientation", 0, nan)), INVALID, "not finite"),
             (dict(edit=(1, "scale", 0, 0.0)), INVALID, "|det(toWorld)| < 1e-5"), (dict(edit=(5, "scale", 1, 1e-9)), INVALID, "instance 5")]
    for change, status, text in cases:
        st, msg = call(**change)
        print(change, "->", st, repr(msg))
        assert st == status and text in msg and "gbl_render_motion" in msg, (change, st, msg)
        torch.cuda.synchronize()
        assert (arena == -1).all(), change          # nothing was written
        # ... and the context's next valid call gives the bits it gave before
        np.testing.assert_array_equal(bits(r.motion(cam, prev, normal=normal).cpu().numpy()), bits(good), err_msg=str(change))
    assert r.lib.gbl_render_motion(None, None, None) == INVALID
    # what a call does not read is not checked: a film right behind the planes does not overlap them
    st, msg = call(normal=out.data_ptr() + 2 * n * 16)
    assert st == _abi.GBL_OK, msg
    # gbl_film_accumulate_motion: gbl_film_accumulate's refusals under its own name, and the planes
    s = mr.moving_sequence(9, 9)
    t = {k: upload(s[k]) for k in ("film", "variance", "normal", "depth", "history", "motion")}
    t["history_out"] = torch.full((3, 9, 9, 4), -1.0, dtype=torch.float32, device=r.device)
    t["film_out"] = torch.full((9, 9, 4), -1.0, dtype=torch.float32, device=r.device)
    t["variance_out"] = torch.full((9, 9), -1.0, dtype=torch.float32, device=r.device)

    def accumulate(**change):
        p = _abi.gbl_temporal_params()
        p.prev_camera.type = 7              # not read
        p.alpha_min, p.max_history, p.sigma_depth, p.cos_normal = 0.1, 8.0, 0.05, 0.9
        p.stream = torch.cuda.current_stream(r.device).cuda_stream
        a = {k: v.data_ptr() for k, v in t.items()}
        for k, v in change.items():
            if k in a:
                a[k] = v
            else:
                setattr(p, k, v)
        st = r.lib.gbl_film_accumulate_motion(r.handle, a["film"], a["variance"], a["normal"], a["depth"], a["history"], a["history_out"], a["motion"],
                                              C.byref(p), a["film_out"], a["variance_out"])
        return st, r.lib.gbl_last_error(r.handle).decode()
    ptr = {k: v.data_ptr() for k, v in t.items()}
    for change, text in ((dict(motion=None), "motion"), (dict(film_out=ptr["motion"]), "motion"), (dict(variance_out=ptr["motion"] + 16 * n), "motion"),
                         (dict(history_out=ptr["motion"] + 16), "motion"), (dict(film=None), "film_accum"), (dict(depth=None), "depth_accum"),
                         (dict(alpha_min=0.0), "alpha_min"), (dict(max_history=0.5), "max_history"), (dict(sigma_depth=nan), "sigma_depth"),
                         (dict(cos_normal=1.5), "cos_normal"), (dict(history_out=ptr["history"]), "history_in"), (dict(film_out=ptr["depth"]), "depth_accum")):
        st, msg = accumulate(**change)
        print(change, "->", st, repr(msg))
        assert st == INVALID and text in msg and "gbl_film_accumulate_motion" in msg, (change, st, msg)
    torch.cuda.synchronize()
    for k in ("history_out", "film_out", "variance_out"):
        assert (t[k] == -1).all(), k
    set_camera(r, r.camera())
    st, msg = accumulate()
    torch.cuda.synchronize()
    assert st == _abi.GBL_OK, msg
    gpu = dict(film=t["film_out"].cpu().numpy(), variance=t["variance_out"].cpu().numpy(), history=t["history_out"].cpu().numpy())
    check_bits(gpu, mr.accumulate_motion(s["film"], s["depth"], s["motion"], variance=s["variance"], normal=s["normal"], history=s["history"],
                                         alpha_min=0.1, max_history=8.0, sigma_depth=0.05, cos_normal=0.9), "after the refusals")


# 5 ------------------------------------------------------------------------------------------------------------------
FRAMES = 6
STEP = (0.06, 0.0, 0.0)       # per frame: the globe's cube is 0.9 wide


def test_end_to_end_a_moving_globe():
    """Six frames of 4 spp of `textured` at 64 x 64 under a still camera while the globe slides by STEP per frame; the albedo film
    accumulated with and without the planes, compared on the globe's final pixels with the last frame's own albedo.

    The globe's checker is a SphericalMapping of the WORLD position of the hit (kernels/shade.h tex_map reads fr.p) about a fixed
    centre, so the pattern does not travel with the cube: no step makes a stale texel of the plain path the wrong check, and the
    step is chosen as the cube's travel, 0.3 of its width over the sequence, not as a fraction of a check.  What the plain path
    loses on a mover here is history -- every face slides through its pixels, the depth test rejects the taps and the pixel starts
    again from 4 spp of a filtered checker -- and the motion-aware path keeps it.  Measured (MI355X): MSE 5.03e-4 against 9.14e-4,
    ratio 0.55; mean history length 4.26 against 2.85."""
    r = tracer("textured", 64, 64, 4, 4, "moving")
    names = [p["name"] for p in json.load(open(gs.scene_path("textured")))["primitives"] if p["type"] == "instance"]
    globe = names.index("globe")
    assert r.scene.desc.instances[globe].area_light < 0
    first = r.instances()
    cam = r.camera()
    try:
        hist = {True: None, False: None}
        prev_instances = None
        for i in range(FRAMES):
            pos = tuple(first[globe][0][k] + STEP[k] * (i - (FRAMES - 1)) for k in range(3))       # the last frame is the scene's own
            r.update_instances(globe, [(pos, first[globe][1], first[globe][2])])
            aov = r.render_aov(seed=i)
            planes = r.motion(cam, prev_instances, normal=aov["normal"])
            for aware in (True, False):
                acc = r.accumulate(aov["albedo"], aov["depth"], None, aov["normal"], hist[aware], cam, motion=planes if aware else None)
                hist[aware] = acc["history"]
            prev_instances = r.instances()
        torch.cuda.synchronize()
        assert r.instances() == first
        on_globe = planes[1, ..., 3].cpu().numpy() == globe + 1
        assert on_globe.sum() >= 50
        last = aov["albedo"].normalized().cpu().numpy()
        err = {aware: float(((hist[aware][0, ..., :3].cpu().numpy() - last)[on_globe] ** 2).mean()) for aware in (True, False)}
        length = {aware: float(hist[aware][0, ..., 3].cpu().numpy()[on_globe].mean()) for aware in (True, False)}
        print("textured 64^2, %d x 4 spp, globe step %s per frame, %d pixels on the globe: albedo MSE against the last frame motion-aware %.4g, plain %.4g "
              "(ratio %.3f); mean history length there motion-aware %.2f, plain %.2f" %
              (FRAMES, STEP, on_globe.sum(), err[True], err[False], err[True] / err[False] if err[False] > 0 else float("inf"), length[True], length[False]))
        assert err[True] < err[False]
        assert length[True] > 1
        assert torch.isfinite(hist[True]).all()
    finally:
        r.update_instances(globe, [first[globe]])
