"""gbl_radiance_rays on the device (kernels/radiance.h): PathTracer::Li along caller rays.

The pin: a caller's ray is the reference's RayDifferential without differentials at vertex 0, so when the rays are a frame's own
camera rays (Oracle.camera_ray at the samples' image positions) the answers are that frame's per-sample Li -- the compiled
reference's logged Li under its own records (tests/golden/surface_<case>.npz), the oracle's Li and gbl_render's li_out under the
native law -- bit for bit (surface_chart.same_bits; tests/test_radiance_cpu.py holds that no reference value is a NaN, so nothing is
left out).  Then the call's own ground: splits, schedules, counts, invalid rays, depth, roulette, edits, refusals.

Which build ran follows api_radiance.hip's rule as the render's follows api_render.hip's: records -> the replay builds, a scene for
which surface_chart.is_lean fails or a `+ext` twin -> the EXT builds, exact_ties on a lean scene -> the lean native build with the
tie rule, else the lean native build.
"""
import ctypes as C

import numpy as np
import pytest

import helpers
import oracle_binding as ob
import query_cases as qc
import radiance_cases as rc
import surface_chart as sc
from goblin_amd import _abi

pytestmark = pytest.mark.gpu

SEED = rc.SEED


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def tracer(scene, bvh="host"):
    from goblin_amd.renderer import HipPathTracer
    return HipPathTracer(scene, 0, bvh=bvh)


def dev(torch, a):
    return torch.as_tensor(np.array(a, np.float32, order="C"), device="cuda:0")


def host(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def assert_li(case, what, got, ref, samples=None, w=1.0):
    same = sc.same_bits(got[:, :3], ref[:, :3])
    if not same and samples is not None:
        print(sc.sample_report(case, what, got, ref, samples))
    assert same, (case, what)
    assert np.array_equal(got[:, 3], np.full(got.shape[0], w, np.float32)), (case, what)


def with_depth(scene, depth):
    s = _abi.gbl_render_setting.from_buffer_copy(scene.desc.setting)
    s.max_ray_depth = depth
    return s


_native = {}


def native(case):
    """(samples, rays, oracle li) of the native law's camera samples of a chart, computed once and shared read-only."""
    if case not in _native:
        o = ob.Oracle(sc.scene(case))
        samples = o.native_samples(SEED)
        li, _ = o.li_replay(samples, threads=4)
        rays = rc.camera_rays(o, samples)
        for a in (samples, li, rays):
            a.setflags(write=False)
        _native[case] = (samples, rays, li)
    return _native[case]


def check_native(torch, case, bvh="host", exact_ties=False):
    samples, rays, li_ref = native(case)
    spp = sc.doc(case)["render_setting"]["sample_per_pixel"]
    r = tracer(sc.scene(case), bvh)
    d_rays = dev(torch, rays)
    for ties in ([False, True] if exact_ties else [False]):
        got = host(torch, r.radiance(d_rays, seed=SEED, samples_per_group=spp, first_group=0, exact_ties=ties))
        assert_li(case, "native exact_ties=%s against the oracle" % ties, got, li_ref, samples)
        li = host(torch, r.render(seed=SEED, want_li=True, schedule="megakernel", exact_ties=ties)["li"])
        assert_li(case, "native exact_ties=%s against gbl_render" % ties, got, li, samples)


# ---------------------------------------------------------------------------
# 1. the reference's Li
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.CHARTS)
def test_replay_is_the_reference_li(torch, case):
    g = sc.golden(case)
    o = ob.Oracle(sc.scene(case))
    res = o.render(threads=1, want_samples=True)
    assert np.array_equal(res["samples"][:, :4], g["samples"])
    idx = helpers.tile_order_index(o.window(), 1)
    samples, li_ref = np.ascontiguousarray(res["samples"][idx]), g["li"][idx]
    rays = rc.camera_rays(o, samples)
    got = host(torch, tracer(sc.scene(case)).radiance(dev(torch, rays), records=dev(torch, samples)))
    assert_li(case, "replay", got, li_ref, samples)


# ---------------------------------------------------------------------------
# 2. the native law
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.CHARTS)
def test_native_is_the_oracle_and_the_render(torch, case):
    check_native(torch, case, exact_ties=sc.is_lean(case))


@pytest.mark.parametrize("case", rc.SUMMED)
def test_native_groups_of_four_are_pixels_of_four_samples(torch, case):
    """4 spp: ray i is pixel i // 4, sample i % 4."""
    check_native(torch, case, exact_ties=sc.is_lean(case))


@pytest.mark.parametrize("case", rc.TWINS)
def test_twin_takes_the_ext_build_to_the_lean_bits(torch, case):
    check_native(torch, case)
    assert sc.same_bits(native(case)[2], native(case[:-4])[2])


@pytest.mark.parametrize("case", rc.BASES)
def test_native_over_the_device_built_bvh(torch, case):
    check_native(torch, case, bvh="device")


# ---------------------------------------------------------------------------
# 3. split and schedule independence
# ---------------------------------------------------------------------------
def test_split_calls_and_one_workgroup_draw_what_one_call_draws(torch):
    samples, rays, li_ref = native("deep")
    r = tracer(sc.scene("deep"))
    d_rays = dev(torch, rays)
    whole = host(torch, r.radiance(d_rays, seed=SEED))
    assert_li("deep", "whole", whole, li_ref, samples)
    a = host(torch, r.radiance(d_rays[:100].contiguous(), seed=SEED, first_group=0))
    b = host(torch, r.radiance(d_rays[100:].contiguous(), seed=SEED, first_group=100))
    assert np.array_equal(np.concatenate([a, b]).view(np.uint32), whole.view(np.uint32))
    one = host(torch, r.radiance(d_rays, seed=SEED, _max_workgroups=1))
    assert np.array_equal(one.view(np.uint32), whole.view(np.uint32))


def test_incoherent_rays_give_the_same_bits_whatever_the_schedule(torch):
    scene = sc.scene("deep")
    bound = qc.scene_bound(scene, skip_floor=False)
    rays = rc.unit_rays(np.concatenate([qc.sphere_rays(bound, 1000), qc.chord_rays(bound, 1000)]))
    d = rays[:, 4:7].astype(np.float64)
    assert np.abs((d * d).sum(axis=1) - 1.0).max() <= rc.UNIT_HEADROOM
    r = tracer(scene)
    d_rays = dev(torch, rays)
    first = host(torch, r.radiance(d_rays, seed=SEED))
    again = host(torch, r.radiance(d_rays, seed=SEED))
    one = host(torch, r.radiance(d_rays, seed=SEED, _max_workgroups=1))
    assert np.array_equal(first[:, 3], np.ones(len(rays), np.float32))
    assert (first[:, :3] > 0).any(), "no ray of the population gathered light"
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32))
    assert np.array_equal(first.view(np.uint32), one.view(np.uint32))


# ---------------------------------------------------------------------------
# 4. counts
# ---------------------------------------------------------------------------
def test_every_prefix_is_the_prefix_of_the_full_answer(torch):
    samples, rays, li_ref = native("deep")
    r = tracer(sc.scene("deep"))
    d_rays = dev(torch, rays)
    for n in rc.COUNTS:
        got = host(torch, r.radiance(d_rays[:n].contiguous(), seed=SEED, _max_workgroups=1))
        assert got.shape == (n, 4)
        assert_li("deep", "n=%d" % n, got, li_ref[:n])


# ---------------------------------------------------------------------------
# 5. invalid rays
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["deep", "lean"])
def test_invalid_rays_answer_zeros_and_the_others_keep_their_bits(torch, case):
    samples, rays, li_ref = native(case)
    mixed, ok = rc.mixed_rays(rays)
    assert (~ok).sum() >= 4 * len(rc.INVALID_RAYS)
    r = tracer(sc.scene(case))
    for wgs in (None, 1):
        out = dev(torch, np.full((len(mixed), 4), 7.0, np.float32))
        got = host(torch, r.radiance(dev(torch, mixed), seed=SEED, out=out, _max_workgroups=wgs))
        assert np.array_equal(got[~ok].view(np.uint32), np.zeros(((~ok).sum(), 4), np.uint32)), wgs
        assert_li(case, "valid among invalid", got[ok], li_ref[ok])


# ---------------------------------------------------------------------------
# 6. depth and roulette
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case,depth", [("quad", 1), ("ibl", 1), ("emitter_front", 1), ("lean", 2), ("deep", 2), ("lean", 6), ("deep", 6), ("ibl", 6)])
def test_depth_is_the_path_tracers_max_ray_depth(torch, case, depth):
    scene = sc.scene(case)
    o = ob.Oracle(scene)
    s = with_depth(scene, depth)
    samples = o.native_samples(SEED, setting=s)
    li_ref, _ = o.li_replay(samples, setting=s, threads=4)
    rays = rc.camera_rays(o, samples)
    r = tracer(scene)
    got = host(torch, r.radiance(dev(torch, rays), depth=depth, seed=SEED))
    assert_li(case, "depth %d native" % depth, got, li_ref, samples)
    got = host(torch, r.radiance(dev(torch, rays), depth=depth, records=dev(torch, samples)))
    assert_li(case, "depth %d replay" % depth, got, li_ref, samples)
    if depth == 1 and case != "quad":   # (the quad faces down: no camera ray sees its lit side, and depth 1 is Black everywhere)
        assert (li_ref[:, :3] > 0).any(), "emission / environment only, and some ray sees it"


def test_roulette_is_the_oracles_restatement(torch):
    samples, rays, li_plain = native("deep")
    li_ref = ob.Oracle(sc.scene("deep")).li_native(SEED, rr=True)
    assert not sc.same_bits(li_ref[:, :3], li_plain[:, :3]), "the roulette ends no path of this chart"
    got = host(torch, tracer(sc.scene("deep")).radiance(dev(torch, rays), seed=SEED, rr=True))
    assert_li("deep", "roulette", got, li_ref, samples)


# ---------------------------------------------------------------------------
# 7. edits seen
# ---------------------------------------------------------------------------
def material_row(m):
    return list(m.color) + list(m.color2) + list(m.color3) + [m.index, m.k, m.exponent]


@pytest.mark.parametrize("case", ["lean", "deep"])
def test_edits_queued_on_the_stream_are_seen_without_a_synchronise(torch, case):
    samples, rays, li_ref = native(case)
    scene = sc.scene(case)
    r = tracer(scene)
    d_rays = dev(torch, rays)
    before = host(torch, r.radiance(d_rays, seed=SEED))
    assert_li(case, "before", before, li_ref, samples)
    # the floor's material: the first instance's
    material = int(scene.desc.instances[0].material)
    row = material_row(r.materials()[material])
    row[0:3] = [0.15, 0.6, 0.3]
    d_row = dev(torch, np.array([row], np.float32))
    torch.cuda.synchronize()
    r.update_lights(0, color=(11.0, 23.0, 5.0))
    r.update_materials(material, d_row)
    got = r.radiance(d_rays, seed=SEED)   # (no synchronise between the edits and the query: one stream orders them)
    got = host(torch, got)
    li = host(torch, r.render(seed=SEED, want_li=True, schedule="megakernel")["li"])
    assert_li(case, "after the edits", got, li, samples)
    assert not sc.same_bits(got[:, :3], before[:, :3])
    # ... and each edit alone moved the answer
    r.update_lights(0, color=tuple(scene.desc.lights[0].color))
    only_material = host(torch, r.radiance(d_rays, seed=SEED))
    assert not sc.same_bits(only_material[:, :3], before[:, :3]) and not sc.same_bits(only_material[:, :3], got[:, :3])


# ---------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------
def params(depth=2, S=1, first_group=0, flags=0, seed=0, records=None, stride=0, reserved=0):
    p = _abi.gbl_radiance_params()
    p.max_ray_depth, p.samples_per_group, p.first_group, p.flags, p.seed = depth, S, first_group, flags, seed
    p.d_records, p.record_stride, p.reserved = records, stride, reserved
    return p


def test_every_refusal_by_status_and_text(torch):
    samples, rays, _ = native("lean")
    scene = sc.scene("lean")
    r = tracer(scene)
    n = 64
    d_rays = dev(torch, rays[:n])
    d_out = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    dims = samples.shape[1]
    d_rec = dev(torch, samples[:n])
    h_rays = np.ascontiguousarray(rays[:n])
    INV, UNS = _abi.GBL_ERR_INVALID, _abi.GBL_ERR_UNSUPPORTED
    rp, op, cp = d_rays.data_ptr(), d_out.data_ptr(), d_rec.data_ptr()
    # allocations of their own, 4 bytes short (a tensor's block in torch's caching allocator is larger than the tensor): checked by the
    # refusal, never launched into
    with open("/proc/self/maps") as f:   # the HIP runtime this process already runs on, not a second copy of it
        hip = C.CDLL(next(line.split()[-1] for line in f if "libamdhip64" in line))
    short_out, short_rec = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(short_out), C.c_size_t(16 * n - 4)) == 0
    assert hip.hipMalloc(C.byref(short_rec), C.c_size_t(4 * dims * n - 4)) == 0
    both = torch.zeros((2 * n, 8), dtype=torch.float32, device="cuda:0")
    table = [
        ("null params", (rp, n, None, op), INV, "params"),
        ("reserved", (rp, n, params(reserved=1), op), INV, "reserved"),
        ("flags", (rp, n, params(flags=4), op), INV, "flags"),
        ("depth 0", (rp, n, params(depth=0), op), INV, "max_ray_depth"),
        ("depth 16385", (rp, n, params(depth=16385), op), INV, "max_ray_depth"),
        ("S 0", (rp, n, params(S=0), op), INV, "perfect square"),
        ("S 2", (rp, n, params(S=2), op), INV, "perfect square"),
        ("n % S", (rp, n, params(S=9), op), INV, "multiple"),
        ("groups past 2^32", (rp, n, params(first_group=2 ** 32 - n + 1), op), INV, "2^32"),
        ("n >= 2^32", (rp, 2 ** 32, params(), op), UNS, "2^32 rays"),
        ("roulette with records", (rp, n, params(flags=_abi.GBL_RADIANCE_RUSSIAN_ROULETTE, records=cp, stride=dims), op), INV, "ROULETTE"),
        ("record_stride", (rp, n, params(records=cp, stride=dims - 1), op), INV, "record_stride"),
        ("null rays", (None, n, params(), op), INV, "null pointer"),
        ("null out", (rp, n, params(), None), INV, "null pointer"),
        ("host rays", (h_rays.ctypes.data, n, params(), op), INV, "d_rays"),
        ("short out", (rp, n, params(), short_out.value), INV, "d_out"),
        ("short records", (rp, n, params(records=short_rec.value, stride=dims), op), INV, "d_records"),
        ("out overlaps rays", (both.data_ptr(), n, params(), both.data_ptr() + 16), INV, "overlaps"),
        ("out overlaps records", (rp, n, params(records=cp, stride=dims), cp), INV, "overlaps"),
    ]
    torch.cuda.synchronize()
    for name, (a_rays, a_n, a_p, a_out), status, word in table:
        for fn, extra in ((r.lib.gbl_radiance_rays, ()), (r.lib.gbl_selftest_radiance, (1,))):
            st = fn(r.handle, a_rays, a_n, C.byref(a_p) if a_p is not None else None, a_out, *extra)
            text = r.lib.gbl_last_error(r.handle).decode()
            assert st == status, (name, st, text)
            assert word in text, (name, text)
    torch.cuda.synchronize()
    assert hip.hipFree(short_out) == 0 and hip.hipFree(short_rec) == 0
    assert not d_out.any(), "a refused call wrote"
    # accepted without a launch: n == 0, whatever the pointers
    assert r.lib.gbl_radiance_rays(r.handle, None, 0, C.byref(params()), None) == _abi.GBL_OK
    assert r.radiance(d_rays[:0].contiguous()).shape == (0, 4)
    # the Python face checks its tensors as trace() does
    with pytest.raises(ValueError):
        r.radiance(d_rays[:, :7])
    with pytest.raises(ValueError):
        r.radiance(d_rays.double())
    with pytest.raises(ValueError):
        r.radiance(d_rays, out=d_out[:n - 1])
    with pytest.raises(ValueError):
        r.radiance(d_rays, records=d_rec[:n - 1])
    with pytest.raises(_abi.GoblinError) as e:
        r.radiance(d_rays, samples_per_group=3)
    assert e.value.status == INV


@pytest.mark.parametrize("which", ["medium", "subsurface"])
def test_a_medium_or_a_subsurface_material_is_unsupported(torch, which):
    if which == "medium":
        import medium_chart as chart
        scene = chart.scene("hom")
    else:
        import sss_chart as chart
        scene = chart.scene("pt")
    r = tracer(scene)
    rays = dev(torch, rc.camera_rays(ob.Oracle(scene), np.array([[12.5, 8.5], [3.5, 4.5]], np.float32)))
    with pytest.raises(_abi.GoblinError) as e:
        r.radiance(rays)
    assert e.value.status == _abi.GBL_ERR_UNSUPPORTED and which in str(e.value)


def test_no_lights_answers_black_with_weight_one(torch):
    samples, rays, li_ref = native("lights_none")
    assert not li_ref[:, :3].any()
    mixed, ok = rc.mixed_rays(rays)
    got = host(torch, tracer(sc.scene("lights_none")).radiance(dev(torch, mixed), seed=SEED))
    assert not got[:, :3].any()
    assert np.array_equal(got[:, 3], ok.astype(np.float32))
