"""gbl_render_motion_deform on the device: motion planes that follow vertex edits.

 1. bit for bit   with no mesh deformed -- nothing listed, the unedited positions listed, the positions an edit A -> B -> A came
                  back to -- the planes are gbl_render_motion's, on every kernel flavour
 2. restatement   after rr.jitter / rr.stretch through update_vertices the planes are tests/deform_reference.py's, which follows the
                  AOV records' hit through the triangle's previous pose: the instance exactly on every pixel, M0 and M1 within
                  temporal_reference.bound(float32 restatement, float64 restatement), the project's rule for planes that are not
                  restatable bit for bit.  A pixel beyond it may only be beyond it by the restatement's own sensitivity to the
                  barycentrics times their float32 uncertainty at that hit (deform_reference.barycentric_uncertainty), no constant
                  added; every case prints whether that term was needed.
 3. rigid         a previous pose that is the current one translated gives the planes of gbl_render_motion for the same world
                  motion expressed as an instance edit
 4. refusals      leave nothing written and the next call's planes unchanged
 5. end to end    a sheared, uv-mapped floor accumulated over six frames with and without prev_vertices

The deformations move vertices as a function of their POSITION (``by_position``), so vertices an OBJ file repeats stay together and
the surface stays continuous across shared edges.
"""
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
import deform_reference as dr
import meshes
import motion_reference as mr
import refit_reference as rr
import temporal_reference as tr
import test_gpu_motion as tgm

pytestmark = pytest.mark.gpu

F = np.float32
INVALID = _abi.GBL_ERR_INVALID
bits, as_gbl, fields, centre_records = tgm.bits, tgm.as_gbl, tgm.fields, tgm.centre_records


def by_position(fn, V):
    uniq, inv = np.unique(np.asarray(V, F), axis=0, return_inverse=True)
    return np.ascontiguousarray(fn(uniq)[np.asarray(inv).reshape(-1)], F)


def triangle_meshes(r):
    d = r.scene.desc
    return [m for m in range(d.num_meshes) if d.meshes[m].shape == 0 and d.meshes[m].tri_count > 0]


def faces(r, m):
    d = r.scene.desc
    gm = d.meshes[m]
    I = np.ctypeslib.as_array(d.indices, shape=(d.num_triangles * 3,)).reshape(-1, 3)
    return I[gm.tri_offset:gm.tri_offset + gm.tri_count].astype(np.int64)


def instance_mesh(r):
    d = r.scene.desc
    return tuple(int(d.instances[i].mesh) for i in range(d.num_instances))


def moved_camera(cam):
    c = dict(cam, position=(cam["position"][0] + 0.02, cam["position"][1] - 0.01, cam["position"][2] + 0.015),
             orientation=tgm.quat_mul(cam["orientation"], (float(np.cos(0.01)), 0.0, float(np.sin(0.01)), 0.0)))
    return tr.camera(**{k: c[k] for k in ("position", "orientation", "fov_degrees", "type", "film_width", "lens_radius", "focal_distance", "near_plane", "far_plane")})


# 1 ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mesh_dir():
    import tempfile
    d = tempfile.mkdtemp(prefix="gbl_deform_")
    meshes.write_meshes(d, meshes.ALL)
    return d


@functools.lru_cache(maxsize=None)
def mesh_tracer(name, size, bvh="host"):
    """tests/meshes.py's scene of one generated mesh (instance 1, mesh 1; 0 is the floor)."""
    doc = meshes.scene_doc(name, resolution=(size, size), spp=1, depth=2)
    return HipPathTracer(gs.load_scene_text(json.dumps(doc), mesh_dir()), 0, bvh=bvh)


@pytest.mark.parametrize("case", [("grid", 40, 40, ""), ("grid", 9, 9, ""), ("textured", 40, 40, ""), ("grid", 40, 40, "ortho"), ("deep_spiral", 24, 24, "")])
def test_no_mesh_deformed_is_render_motion_bit_for_bit(case):
    name, w, h, tag = case
    r = mesh_tracer(name, w) if name == "deep_spiral" else tgm.tracer(name, w, h, 1, 4, tag + "deform")
    if name == "deep_spiral":
        assert 3 * r.info.blas_depth + 2 > 64          # past the packet's stack: one ray per lane, lean
    if tag == "ortho":
        r.update_camera(type=_abi.GBL_CAMERA_ORTHOGRAPHIC, film_width=6.0)
    rec = centre_records(r)
    assert rec["hit"].sum() > 0.3 * rec["hit"].size
    cam = moved_camera(fields(r.camera()))
    before = r.instances()
    prevs = [None, before]
    if name == "grid":
        r.update_instances(0, tgm.grid_moves(r))          # ``before`` is now six moved instances' previous frame
        rec = centre_records(r)
    try:
        editable = triangle_meshes(r)[0] if name != "deep_spiral" else 1
        A = r.vertices(editable)
        for prev_instances in prevs:
            for normal in (None, rec["normal"]):
                want = r.motion(as_gbl(cam), prev_instances, normal=normal).cpu().numpy()
                assert want[0, ..., 3].sum() > 0
                held = {m: r.vertices(m) for m in triangle_meshes(r)}
                for what, pv in (("nothing listed", {}), ("the unedited positions", held), ("one mesh of them", {editable: A})):
                    got = r.motion(as_gbl(cam), prev_instances, normal=normal, prev_vertices=pv).cpu().numpy()
                    np.testing.assert_array_equal(bits(got), bits(want), err_msg="%s %s" % (case, what))
        # A -> B -> A: the context holds A's bits again, so A as the previous pose deforms nothing
        B = by_position(lambda V: rr.jitter(V, 0.05 * float(np.abs(A).max())), A)
        assert B.tobytes() != A.tobytes()
        r.update_vertices(editable, B)
        r.update_vertices(editable, A)
        for prev_instances in prevs:
            want = r.motion(as_gbl(cam), prev_instances, normal=rec["normal"]).cpu().numpy()
            got = r.motion(as_gbl(cam), prev_instances, normal=rec["normal"], prev_vertices={editable: A}).cpu().numpy()
            np.testing.assert_array_equal(bits(got), bits(want), err_msg="%s A -> B -> A" % (case,))
    finally:
        if name == "grid":
            r.update_instances(0, before[:6])
        if tag == "ortho":
            r.update_camera(type=_abi.GBL_CAMERA_PERSPECTIVE)


# 2 ------------------------------------------------------------------------------------------------------------------
def check_deform(r, rec, prev_camera, prev_instances, prev_vertices, normal, what, found):
    """Device planes against the restatement from the records.  Returns (gpu planes, the restatement's info)."""
    film = rec["normal"] if normal else None
    gpu = r.motion(as_gbl(prev_camera), prev_instances, normal=film, prev_vertices=prev_vertices).cpu().numpy()
    cur_camera, cur_instances = fields(r.camera()), r.instances()
    nrm = rec["normal"].cpu().numpy() if normal else None
    t = np.where(rec["hit"], rec["t"], F(0.0))
    inst = np.where(rec["hit"], rec["inst"], -1)
    np.testing.assert_array_equal(gpu[1, ..., 3].astype(np.int64) - 1, inst, err_msg="%s: M1.w - 1 against the records' instance" % (what,))
    ms = {m: (r.vertices(m), np.asarray(p, F), faces(r, m)) for m, p in prev_vertices.items()}
    info = {}
    args = (t, inst, cur_camera, prev_camera, cur_instances, prev_instances, nrm, instance_mesh(r), ms)
    ref32 = dr.deform_planes(*args, T=F, found=found)
    ref64 = dr.deform_planes(*args, T=np.float64, info=info, found=found)
    on = info["on"]
    # the restatement found every hit's triangle: its own hit distance is the record's, to float32 rounding of the device's t
    assert (info["t_miss"][on] <= 1e-4 * np.maximum(1.0, np.abs(t[on]))).all(), (what, float(info["t_miss"][on].max()))
    ok = ref64[0, ..., 3] != 0
    np.testing.assert_array_equal(gpu[0, ..., 3] != 0, ok, err_msg="%s: ok" % (what,))
    assert not gpu[0][~ok].any() and not ok[~rec["hit"]].any()
    if not normal:
        assert not gpu[1, ..., :3].any()
    extra = None
    for k, name in ((0, "M0"), (1, "M1")):
        tol = tr.bound(ref32[k], ref64[k])
        err = np.abs(gpu[k].astype(np.float64) - ref64[k]).max(-1)
        needed = bool((err > tol).any())
        if needed:      # |dP_prev / d(b1, b2)| times the barycentrics' float32 uncertainty, per pixel, by the restatement's own difference
            if extra is None:
                zero = np.zeros_like(info["eb1"])
                extra = [np.abs(dr.deform_planes(*args, T=np.float64, nudge=nd, found=found) - ref64) for nd in ((info["eb1"], zero), (zero, info["eb2"]))]
            allowed = tol + (extra[0][k] + extra[1][k]).max(-1)
        else:
            allowed = np.full(err.shape, tol)
        print("%s %s: largest difference from the float64 restatement %.3g (on the deformed mesh %.3g), bound %.3g, barycentric term %s; pixels on the "
              "deformed mesh %d of %d, largest barycentric uncertainty %.3g" %
              (what, name, err.max(), err[on].max() if on.any() else 0.0, tol, "NEEDED (largest %.3g)" % (allowed - tol).max() if needed else "not needed",
               on.sum(), on.size, max(info["eb1"][on].max(), info["eb2"][on].max()) if on.any() else 0.0))
        worst = np.unravel_index(np.argmax(err - allowed), err.shape)
        assert (err <= allowed).all(), (what, name, float(err[worst]), float(allowed[worst]), worst)
    return gpu, info


def moved_instance(trs):
    pos, quat, scale = trs
    return ((pos[0] + 0.03, pos[1] + 0.02, pos[2] - 0.025), tgm.quat_mul(quat, (float(np.cos(0.03)), float(np.sin(0.03)), 0.0, 0.0)), tuple(1.1 * s for s in scale))


CASES = [("few1", 20), ("few5", 44), ("flatgrid", 44), ("slivers", 44), ("deep_spiral", 24), ("textured", 44)]


@pytest.mark.parametrize("bvh", ["host", "device"])
@pytest.mark.parametrize("how", ["jitter", "stretch"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_deformed_planes_against_the_restatement(case, how, bvh):
    name, size = case
    if name == "textured":
        r = HipPathTracer(ar.scene("textured", (size, size), 1, 4), 0, bvh=bvh)
        mesh, inst, radius = instance_mesh(r)[2], 2, 0.5          # the cube under the globe
    else:
        r = mesh_tracer(name, size, bvh)
        mesh, inst, radius = 1, 1, meshes.MESHES[name][1]
    A = r.vertices(mesh)
    B = by_position((lambda V: rr.jitter(V, radius)) if how == "jitter" else (lambda V: rr.stretch(V, radius)), A)
    try:
        r.update_vertices(mesh, B)
        rec = centre_records(r)
        on = rec["hit"] & (rec["inst"] == inst)
        assert on.sum() >= 12, (case, how, int(on.sum()))
        cam = fields(r.camera())
        found = {}
        before = r.instances()
        for moved in (False, True):
            prev_camera = moved_camera(cam) if moved else cam
            prev_instances = [moved_instance(t) if i == inst else t for i, t in enumerate(before)] if moved else None
            for normal in (True, False):
                gpu, info = check_deform(r, rec, prev_camera, prev_instances, {mesh: A}, normal, (name, how, bvh, "moved" if moved else "unmoved", "normal" if normal else "no film"), found)
                np.testing.assert_array_equal(info["on"], on)
        # the deformation is seen: the planes differ from the ones that treat the mesh as static
        static = r.motion(as_gbl(cam), None, normal=rec["normal"]).cpu().numpy()
        aware = r.motion(as_gbl(cam), None, normal=rec["normal"], prev_vertices={mesh: A}).cpu().numpy()
        np.testing.assert_array_equal(bits(aware[:, ~on]), bits(static[:, ~on]))          # ... and only on the deformed mesh
        assert np.abs(aware[0] - static[0])[on].max() > 0.05
    finally:
        r.update_vertices(mesh, A)


def test_a_collapsed_previous_triangle_takes_the_normal_fallback():
    """few5's triangle under the image centre had no area in the previous pose (two of its own vertices coincided): the point
    is still followed, along the remaining edge, and the normal is carried by the instance's transforms alone."""
    r = mesh_tracer("few5", 44)
    A = r.vertices(1)
    rec = centre_records(r)
    on = rec["hit"] & (rec["inst"] == 1)
    found, info = {}, {}
    cam = fields(r.camera())
    prev = A.copy()
    f = faces(r, 1)[0]
    prev[f[1]] = prev[f[0]]
    gpu, info = check_deform(r, rec, moved_camera(cam), [moved_instance(t) if i == 1 else t for i, t in enumerate(r.instances())], {1: prev}, True, ("few5", "collapsed"), found)
    flat = info["on"] & (info["tri"] == 0)
    assert flat.sum() >= 12 and (info["on"] & (info["tri"] != 0)).any()
    # on the collapsed triangle n_b is what gbl_render_motion carries for the moved instance, bit for bit
    plain = r.motion(as_gbl(moved_camera(cam)), [moved_instance(t) if i == 1 else t for i, t in enumerate(r.instances())], normal=rec["normal"]).cpu().numpy()
    np.testing.assert_array_equal(bits(gpu[1][flat]), bits(plain[1][flat]))
    assert np.abs(gpu[0] - plain[0])[flat].max() > 0.05


# 3 ------------------------------------------------------------------------------------------------------------------
def rotate(q, v):
    return np.array(tr.quat_rotate([np.float64(c) for c in q], [np.float64(c) for c in v], np.float64))


@pytest.mark.parametrize("case", [("few5", (1,)), ("textured", (2,)), ("textured", (0, 4))], ids=["few5", "textured cube", "textured quad twice"])
def test_a_translated_pose_is_the_instance_edit(case):
    """The previous pose is the current one minus DELTA in object space; the same world motion as an instance edit moves every
    instance of the mesh by R S (-DELTA).  Both device results lie within ``bound`` of their own restatements; the restatements
    differ from each other by the float32 rounding of V - DELTA and of the edited positions, which is measured (in float64, from
    the same records) and allowed on top.  Nothing else is."""
    name, insts = case
    r = mesh_tracer(name, 44) if name != "textured" else tgm.tracer("textured", 44, 44, 1, 4, "rigid")
    mesh = instance_mesh(r)[insts[0]]
    assert [i for i, m in enumerate(instance_mesh(r)) if m == mesh] == list(insts)          # every instance of the mesh, and no other
    delta = np.array([0.25, -0.125, 0.0625], F) * F(0.25 if name == "few5" else 1.0)
    A = r.vertices(mesh)
    prev_vertices = (A - delta).astype(F)
    cur = r.instances()
    prev_instances = list(cur)
    for i in insts:
        pos, quat, scale = cur[i]
        shift = rotate(quat, np.array(scale, np.float64) * (-delta.astype(np.float64)))
        prev_instances[i] = (tuple(float(F(pos[k] + shift[k])) for k in range(3)), quat, scale)
    rec = centre_records(r)
    on = rec["hit"] & np.isin(rec["inst"], insts)
    assert on.sum() >= 30
    cam = fields(r.camera())
    prev_camera = moved_camera(cam)
    a = r.motion(as_gbl(prev_camera), None, normal=rec["normal"], prev_vertices={mesh: prev_vertices}).cpu().numpy()
    b = r.motion(as_gbl(prev_camera), prev_instances, normal=rec["normal"]).cpu().numpy()
    nrm = rec["normal"].cpu().numpy()
    t, inst = np.where(rec["hit"], rec["t"], F(0.0)), np.where(rec["hit"], rec["inst"], -1)
    ms = {mesh: (A, prev_vertices, faces(r, mesh))}
    found = {}
    ra = [dr.deform_planes(t, inst, cam, prev_camera, cur, None, nrm, instance_mesh(r), ms, T=T, found=found) for T in (F, np.float64)]
    rb = [mr.motion_planes(t, inst, cam, prev_camera, cur, prev_instances, nrm, T=T) for T in (F, np.float64)]
    np.testing.assert_array_equal(a[0, ..., 3], b[0, ..., 3])
    np.testing.assert_array_equal(bits(a[:, ~on]), bits(b[:, ~on]))
    for k, plane in ((0, "M0"), (1, "M1")):
        tol = tr.bound(ra[0][k], ra[1][k]) + tr.bound(rb[0][k], rb[1][k]) + float(np.abs(ra[1][k] - rb[1][k]).max())
        err = float(np.abs(a[k].astype(np.float64) - b[k]).max())
        print(case, plane, "deformed pose against instance edit: largest difference %.3g, allowed %.3g (of which the restatements' own difference %.3g)" %
              (err, tol, np.abs(ra[1][k] - rb[1][k]).max()))
        assert err <= tol, (case, plane, err, tol)
    assert np.abs(a[0, ..., :2] - r.motion(as_gbl(prev_camera), None).cpu().numpy()[0, ..., :2])[on].max() > 0.05        # the pose did move


# 4 ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    r = tgm.tracer("textured", 9, 9, 1, 4, "deform refusals")
    n = 9 * 9
    cam = r.camera()
    d = r.scene.desc
    sphere = next(m for m in range(d.num_meshes) if d.meshes[m].shape == 1)
    disk = next(m for m in range(d.num_meshes) if d.meshes[m].shape == 2)
    quad, cube = instance_mesh(r)[0], instance_mesh(r)[2]
    A0, A1 = r.vertices(quad), r.vertices(cube)
    P0, P1 = (A0 + F(0.125)).astype(F), (A1 * F(1.25)).astype(F)
    arena = torch.full((2 * n * 4,), -1.0, dtype=torch.float32, device=r.device)
    good = r.motion(cam, None, prev_vertices={quad: P0, cube: P1}).cpu().numpy()
    assert not np.array_equal(bits(good), bits(r.motion(cam, None).cpu().numpy()))
    nan, inf = P1.copy(), P0.copy()
    nan[3, 1], inf[-1, 2] = np.nan, np.inf

    def call(entries, null_list=False, count=None, params=True, motion_out=True, prev_type=None):
        p = _abi.gbl_motion_params()
        p.prev_camera = cam
        if prev_type is not None:
            p.prev_camera.type = prev_type
        p.stream = torch.cuda.current_stream(r.device).cuda_stream
        listed = (_abi.gbl_motion_mesh * max(len(entries), 1))()
        for k, (mesh, reserved, pos) in enumerate(entries):
            listed[k].mesh, listed[k].reserved, listed[k].positions = mesh, reserved, None if pos is None else pos.ctypes.data
        st = r.lib.gbl_render_motion_deform(r.handle, C.byref(p) if params else None, None if null_list else listed, len(entries) if count is None else count,
                                            arena.data_ptr() if motion_out else None)
        return st, r.lib.gbl_last_error(r.handle).decode()
    cases = [(dict(entries=[], params=False), "params"), (dict(entries=[], motion_out=False), "motion_out"), (dict(entries=[(quad, 0, P0)], prev_type=7), "prev_camera.type"),
             (dict(entries=[], null_list=True, count=2), "prev_meshes is NULL"), (dict(entries=[(cube, 0, None)]), "positions is NULL"),
             (dict(entries=[(quad, 0, P0), (d.num_meshes, 0, P1)]), "out of range"), (dict(entries=[(0xffffffff, 0, P1)]), "out of range"),
             (dict(entries=[(sphere, 0, P1)]), "sphere or a disk"), (dict(entries=[(disk, 0, P1)]), "sphere or a disk"),
             (dict(entries=[(quad, 0, P0), (cube, 0, P1), (quad, 0, A0)]), "listed twice"), (dict(entries=[(cube, 1, P1)]), "reserved"),
             (dict(entries=[(quad, 0, P0), (cube, 0, nan)]), "not finite"), (dict(entries=[(quad, 0, inf)]), "not finite")]
    for kw, text in cases:
        st, msg = call(**kw)
        print(text, "->", st, repr(msg))
        assert st == INVALID and text in msg and "gbl_render_motion_deform" in msg, (text, st, msg)
        torch.cuda.synchronize()
        assert (arena == -1).all(), text            # nothing was written
        np.testing.assert_array_equal(bits(r.motion(cam, None, prev_vertices={quad: P0, cube: P1}).cpu().numpy()), bits(good), err_msg=text)
    assert r.lib.gbl_render_motion_deform(None, None, None, 0, None) == INVALID
    st, msg = call([(cube, 0, P1), (quad, 0, P0)])            # the order of the list does not matter
    torch.cuda.synchronize()
    assert st == _abi.GBL_OK, msg
    np.testing.assert_array_equal(bits(arena.cpu().numpy().reshape(2, 9, 9, 4)), bits(good))
    # the Python layer checks shapes before the library sees a pointer
    for bad in ({quad: P0[:-1]}, {cube: P1.reshape(-1)}, {-1: P0}):
        with pytest.raises(ValueError):
            r.motion(cam, None, prev_vertices=bad)
    with pytest.raises(_abi.GoblinError) as e:
        r.motion(cam, None, prev_vertices={sphere: P0})
    assert e.value.status == INVALID
    np.testing.assert_array_equal(bits(r.motion(cam, None, prev_vertices={quad: P0, cube: P1}).cpu().numpy()), bits(good))


# 5 ------------------------------------------------------------------------------------------------------------------
FRAMES = 6
SHEAR_STEP = 0.125        # object units per frame at the quad's far edge: half a check of the floor's 8 x 8 checker (a check is 0.25 wide)


def test_end_to_end_a_shearing_floor():
    """Six frames of 4 spp of `textured` at 64 x 64 under a still camera while the quad mesh under the floor is sheared in its own
    plane: its far edge slides sideways by half a check per frame, the near edge stays.  The floor's checker is uv-mapped, so it
    travels with the surface, while the depth and the normal under every pixel stay what they were.  That is the ghost, not the
    loss of history (which test_end_to_end_a_moving_globe shows): without prev_vertices no test rejects a stale tap, so the static
    treatment keeps ALL its history and blends opposite checks, and the deformation-aware planes fetch the history from where the
    surface was.  Both orders are asserted on the floor's final pixels: the error against the last frame's own albedo is smaller
    with prev_vertices, and the static treatment's mean history length is at least the deformation-aware one's -- it is the
    history it should not have kept -- while the deformation-aware one is well above 1.  (A first version also raised the far
    edge: the depth test then rejected every stale tap, the static path restarted from the frame's own 4 spp everywhere, and
    against that frame's own albedo a path without history has no error to speak of.  Measured figures: DESIGN.md 4.8.)"""
    r = tgm.tracer("textured", 64, 64, 4, 4, "deforming")
    mesh = instance_mesh(r)[0]
    rest = r.vertices(mesh)
    cam = r.camera()

    def pose(i):        # the last frame is the scene's own
        V = rest.copy()
        far = (F(1.0) + rest[:, 2]) * F(0.5)            # 0 at the edge towards the camera (z = -1), 1 at the far one
        V[:, 0] = (rest[:, 0] + F(SHEAR_STEP * (i - (FRAMES - 1))) * far).astype(F)
        return V
    try:
        hist = {True: None, False: None}
        prev_verts = None
        for i in range(FRAMES):
            r.update_vertices(mesh, pose(i))
            aov = r.render_aov(seed=i)
            planes = {True: r.motion(cam, None, normal=aov["normal"], prev_vertices=prev_verts), False: r.motion(cam, None, normal=aov["normal"])}
            for aware in (True, False):
                acc = r.accumulate(aov["albedo"], aov["depth"], None, aov["normal"], hist[aware], cam, motion=planes[aware])
                hist[aware] = acc["history"]
            prev_verts = {mesh: r.vertices(mesh)}
        torch.cuda.synchronize()
        assert np.array_equal(r.vertices(mesh), rest)
        on_floor = planes[True][1, ..., 3].cpu().numpy() == 1
        assert on_floor.sum() >= 500
        last = aov["albedo"].normalized().cpu().numpy()
        err = {aware: float(((hist[aware][0, ..., :3].cpu().numpy() - last)[on_floor] ** 2).mean()) for aware in (True, False)}
        length = {aware: float(hist[aware][0, ..., 3].cpu().numpy()[on_floor].mean()) for aware in (True, False)}
        print("textured 64^2, %d x 4 spp, the floor's far edge sheared by %.3f per frame, %d pixels on the floor: albedo MSE against the last frame "
              "deformation-aware %.4g, static %.4g (ratio %.3f); mean history length there deformation-aware %.2f, static %.2f" %
              (FRAMES, SHEAR_STEP, on_floor.sum(), err[True], err[False], err[True] / err[False] if err[False] > 0 else float("inf"), length[True], length[False]))
        assert err[True] < err[False]
        assert length[False] >= length[True] > 1
        assert torch.isfinite(hist[True]).all()
    finally:
        r.update_vertices(mesh, rest)
