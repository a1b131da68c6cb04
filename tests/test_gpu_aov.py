"""gbl_render_aov on the device: first-hit records against the oracle sample by sample (bit for bit, the project's LI_FLIP_TOL = 0
standard; the albedo too, which Oracle.first_hit looks up as the bounce-0 BSDF does), the three films against the oracle's splat of the expected values, and every layer above the kernel -- replay, windows,
shards, accumulation, chunking, refusals, another stream, the command-line tool.  Expected values: tests/aov_reference.py."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from goblin_amd import _abi
from goblin_amd import scene as gs
from goblin_amd.renderer import HipPathTracer
import aov_reference as ar
import helpers
import integration_helpers as ih
import meshes
import oracle_binding as ob
import texture_chart as tc

pytestmark = pytest.mark.gpu

SEED = ar.SEED
FILM_RELL2_TOL = 2.5e-5     # summation order (tests/test_gpu_parity.py)
CLI = os.path.join(ih.REPO, "goblin_amd", "lib", "g_ray_hip")
RECORD_SCENES = ["cornell", "shapes", "bumpy", "grid", "masked", "volume"]
TEXTURED_SCENES = ["textured", "imagetex", "bumpy", "masked", "subsurface", "ibl"]   # first colour slots that are texture graphs, masks, Kr of a subsurface material
BUILDERS = ["host", "device"]
CHART = "chart_5x3"        # tests/texture_chart.py: every hit textured (the other charts: tests/test_gpu_texture_chart.py)


def scene_of(name, shape=None):
    return tc.scene(name[len("chart_"):]) if name.startswith("chart_") else ar.scene(name, **dict(shape or ()))


def reference_of(name):
    return tc.reference(name[len("chart_"):]) if name.startswith("chart_") else ar.reference(name)


@functools.lru_cache(maxsize=None)
def tracer(name, bvh="host", shape=None):
    return HipPathTracer(scene_of(name, shape), 0, bvh=bvh)


class Records:
    """The (n, 12) record rows of a call, split into the struct's fields."""

    def __init__(self, out):
        torch.cuda.synchronize()
        rows = out["samples"].cpu().numpy()
        ints = out["samples_i32"].cpu().numpy()
        self.albedo, self.t, self.normal, self.position = rows[:, 0:3], rows[:, 3], rows[:, 4:7], rows[:, 8:11]
        self.instance, self.hit = ints[:, 7], ints[:, 11].view(np.uint32)
        self.rows = ints


@functools.lru_cache(maxsize=None)
def device_records(name, bvh="host", exact=True, shape=None):
    return Records(tracer(name, bvh, shape).render_aov(albedo=False, normal=False, depth=False, want_samples=True, seed=SEED, exact_ties=exact))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_records_equal_oracle(rec, ref, what, geometry=True):
    """hit, instance, t, position, normal, albedo: zero tolerance."""
    assert rec.hit.shape == ref.hit.shape, what
    np.testing.assert_array_equal(rec.hit, ref.hit, err_msg=str(what))
    np.testing.assert_array_equal(bits(rec.t), bits(ref.t), err_msg=str(what))
    if geometry:
        np.testing.assert_array_equal(rec.instance, ref.instance, err_msg=str(what))
        np.testing.assert_array_equal(bits(rec.position), bits(ref.position), err_msg=str(what))
        np.testing.assert_array_equal(bits(rec.normal), bits(ref.normal), err_msg=str(what))
        np.testing.assert_array_equal(bits(rec.albedo), bits(ref.oracle_albedo), err_msg=str(what))


# 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", BUILDERS)
@pytest.mark.parametrize("name", RECORD_SCENES)
def test_records_equal_the_oracle_bit_for_bit(name, bvh):
    ref = ar.reference(name)
    rec = device_records(name, bvh)
    assert ref.hit.sum() > 0 and (ref.hit == 0).sum() > 0, name
    assert_records_equal_oracle(rec, ref, (name, bvh))
    miss = ref.hit == 0
    assert not rec.albedo[miss].any() and not rec.position[miss].any() and not rec.normal[miss].any()


@pytest.mark.parametrize("mode", ["native", "replay"])
@pytest.mark.parametrize("name", TEXTURED_SCENES)
def test_textured_records_equal_the_oracle_bit_for_bit(name, mode):
    """The whole record rows, albedo included, where the first colour slot is looked up: filtered checkerboards, image textures, a
    mask's wrapped material, a subsurface material's Kr, under bump and normal maps."""
    ref = ar.reference(name)
    if mode == "native":
        rec = device_records(name)
    else:
        rec = Records(tracer(name).render_aov(albedo=False, normal=False, depth=False, want_samples=True, replay_samples=ref.samples.copy()))
    assert ref.hit.sum() > 0
    assert_records_equal_oracle(rec, ref, (name, mode))
    np.testing.assert_array_equal(rec.rows, ref.rows)


# 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RECORD_SCENES)
def test_hit_and_t_do_not_depend_on_the_tie_rule(name):
    assert_records_equal_oracle(device_records(name, "host", exact=False), ar.reference(name), name, geometry=False)


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("name", ["cornell", "grid"])
def test_packets_and_single_rays_write_the_same_records(name, exact, monkeypatch):
    """The lean scenes take the packet kernel under the native sampler; GBL_AOV_PACKET=0 puts one ray on each lane."""
    monkeypatch.setenv("GBL_AOV_PACKET", "0")
    single = Records(tracer(name).render_aov(want_samples=True, seed=SEED, exact_ties=exact))
    np.testing.assert_array_equal(single.rows, device_records(name, "host", exact).rows)


# 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "shapes", "grid", "masked", "volume"])
def test_constant_albedo_is_the_description_colour(name):
    ref, rec = ar.reference(name), device_records(name)
    hit = ref.hit == 1
    covered = (ref.albedo_known & hit).sum() / hit.sum()
    print(name, "constant-slot fraction of the hits", covered)
    assert covered >= 0.99
    known = ref.albedo_known
    np.testing.assert_array_equal(bits(rec.albedo[known]), bits(ref.albedo[known]))
    if name == "masked":   # some hit lands on a mask, whose albedo is the wrapped material's
        desc = ref.scene.desc
        on_mask = np.array([i >= 0 and desc.materials[desc.instances[i].material].type == _abi.GBL_MAT_MASK for i in ref.instance])
        assert on_mask.sum() > 0


def test_textured_albedo():
    ref, rec = ar.reference("textured"), device_records("textured")
    assert_records_equal_oracle(rec, ref, "textured")
    f32 = np.float32
    # instance 1: an unfiltered checkerboard of red / white scaled by the float 0.5
    ball = ref.instance == 1
    products = [np.array([0.7, 0.1, 0.08], f32) * f32(0.5), np.array([0.8, 0.8, 0.8], f32) * f32(0.5)]
    is_a = (bits(rec.albedo[ball]) == bits(products[0])).all(axis=1)
    is_b = (bits(rec.albedo[ball]) == bits(products[1])).all(axis=1)
    print("textured: samples on the ball", int(ball.sum()), "red", int(is_a.sum()), "white", int(is_b.sum()))
    assert ball.sum() > 0 and (is_a | is_b).all() and is_a.any() and is_b.any()
    # instances 0 and 2: filtered checkerboards, between their two constants
    for inst, c1, c2 in ((0, [0.8, 0.8, 0.8], [0.08, 0.08, 0.1]), (2, [0.1, 0.2, 0.7], [0.9, 0.7, 0.3])):
        on = ref.instance == inst
        lo, hi = np.minimum(np.array(c1, f32), np.array(c2, f32)), np.maximum(np.array(c1, f32), np.array(c2, f32))
        a = rec.albedo[on]
        print("textured: instance", inst, "samples", int(on.sum()), "albedo range", a.min(axis=0), a.max(axis=0))
        assert on.sum() > 0 and (a >= lo).all() and (a <= hi).all()
    np.testing.assert_array_equal(bits(rec.albedo), bits(ref.oracle_albedo))


def test_image_texture_albedo_is_finite_and_in_range():
    ref, rec = ar.reference("imagetex"), device_records("imagetex")
    assert_records_equal_oracle(rec, ref, "imagetex")
    hit = ref.hit == 1
    assert hit.sum() > 0 and (~ref.albedo_known).sum() > 0
    assert np.isfinite(rec.albedo).all() and rec.albedo[hit].min() >= 0.0 and rec.albedo[hit].max() <= 1.0
    np.testing.assert_array_equal(bits(rec.albedo), bits(ref.oracle_albedo))
    textured = hit & ~ref.albedo_known
    assert len(np.unique(ref.oracle_albedo[textured], axis=0)) > 100      # (the lookups vary: not one colour per instance)


# 4 ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_films(name, shard=None):
    r = tracer(name)
    out = r.render_aov(seed=SEED, exact_ties=True, shard=shard)
    depth, coverage = r.resolve_depth(out["depth"])
    torch.cuda.synchronize()
    return {"albedo": out["albedo"].numpy(), "normal": out["normal"].numpy(), "depth": out["depth"].numpy(),
            "albedo_n": out["albedo"].normalized().cpu().numpy(), "normal_n": out["normal"].normalized().cpu().numpy(),
            "resolved": (depth.cpu().numpy(), coverage.cpu().numpy())}


@pytest.mark.parametrize("name", ["cornell", "shapes", "textured", "imagetex", CHART])
def test_films_equal_the_oracles_splat(name):
    want = reference_of(name).films()
    assert np.abs(want["albedo"][..., :3]).sum() > 0
    got = device_films(name)
    rels = {"albedo": helpers.rel_l2(got["albedo_n"], ob.normalize_film(want["albedo"])),
            "normal": helpers.rel_l2(got["normal_n"], ob.normalize_film(want["normal"]))}
    d_got, c_got = ar.depth_and_coverage(got["depth"])
    d_want, c_want = ar.depth_and_coverage(want["depth"])
    rels["depth"] = helpers.rel_l2(d_got, d_want)
    rels["coverage"] = helpers.rel_l2(c_got, c_want)
    rels["weight"] = helpers.rel_l2(got["depth"][..., 3], want["depth"][..., 3])
    print(name, "film relL2", rels)
    assert max(rels.values()) <= FILM_RELL2_TOL
    assert not got["depth"][..., 2].any()
    # resolve_depth is the float32 divide, exactly
    np.testing.assert_array_equal(bits(got["resolved"][0]), bits(d_got))
    np.testing.assert_array_equal(bits(got["resolved"][1]), bits(c_got))


def test_resolve_depth_is_zero_where_the_denominator_is():
    r = tracer("cornell")
    a = np.zeros((16, 16, 4), np.float32)
    a[0, 0] = (3.0, 0.0, 0.0, 2.0)      # covered by samples that all missed
    a[0, 1] = (0.0, 0.0, 0.0, 0.0)      # no sample at all
    a[0, 2] = (1.0, 3.0, 0.0, 7.0)
    depth, coverage = r.resolve_depth(torch.from_numpy(a).cuda())
    torch.cuda.synchronize()
    depth, coverage = depth.cpu().numpy(), coverage.cpu().numpy()
    assert depth[0, 0] == 0 and coverage[0, 0] == 0 and depth[0, 1] == 0 and coverage[0, 1] == 0
    assert depth[0, 2] == np.float32(1.0) / np.float32(3.0) and coverage[0, 2] == np.float32(3.0) / np.float32(7.0)


# 5 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "textured"])
def test_replayed_records_equal_the_native_call(name):
    ref = ar.reference(name)
    replayed = Records(tracer(name).render_aov(want_samples=True, replay_samples=ref.samples.copy()))
    np.testing.assert_array_equal(replayed.rows, device_records(name).rows)


# 6 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,misses,emitter", [("cornell", 454, 14), ("shapes", 560, 21)])
def test_same_camera_samples_as_the_beauty_pass(name, misses, emitter):
    rec = device_records(name)
    li = tracer(name).render(seed=SEED, want_li=True, exact_ties=True)["li"].cpu().numpy()
    miss = rec.hit == 0
    desc = ar.scene(name).desc
    on_light = np.array([i >= 0 and desc.instances[i].area_light >= 0 for i in rec.instance])
    assert (int(miss.sum()), int(on_light.sum())) == (misses, emitter)
    assert not li[miss, :3].any()
    assert (li[on_light, :3] > 0).all()


# 7 ------------------------------------------------------------------------------------------------------------------
def test_more_than_one_wave_per_pixel():
    shape = (("resolution", (8, 8)), ("spp", 81), ("depth", 2))
    ref = ar.reference("cornell", **dict(shape))
    assert ref.n == 12 * 12 * 81
    assert_records_equal_oracle(device_records("cornell", "host", True, shape), ref, "81 spp")


# 8 ------------------------------------------------------------------------------------------------------------------
def test_deep_tree(tmp_path):
    """The deep spiral's device-built tree needs more than 64 stack entries: no packets, per-lane LDS stacks past 64 KB."""
    meshes.write_meshes(tmp_path, [meshes.DEEP])
    scene = gs.load_scene_text(json.dumps(meshes.scene_doc(meshes.DEEP, resolution=(24, 24))), str(tmp_path))
    r = HipPathTracer(scene, 0, bvh="device")
    assert 3 * r.info.blas_depth + 2 > 64
    ref = ar.Reference(scene)
    assert ref.hit.sum() > 0
    for exact in (True, False):
        rec = Records(r.render_aov(want_samples=True, seed=SEED, exact_ties=exact))
        assert_records_equal_oracle(rec, ref, ("deep", exact), geometry=exact)


# 9 ------------------------------------------------------------------------------------------------------------------
def test_sub_window_is_a_slice_of_the_full_call():
    full = device_records("cornell")
    x0f, x1f, y0f, y1f = tracer("cornell").window
    win = (3, 14, -1, 9)
    sub = Records(tracer("cornell").render_aov(want_samples=True, seed=SEED, exact_ties=True, window=win))
    ys, xs = np.mgrid[win[2]:win[3], win[0]:win[1]]
    pixels = ((ys - y0f) * (x1f - x0f) + (xs - x0f)).reshape(-1)
    index = (pixels[:, None] * 4 + np.arange(4)[None, :]).reshape(-1)
    np.testing.assert_array_equal(sub.rows, full.rows[index])


def test_shards_sum_to_the_whole_and_calls_accumulate():
    whole = device_films("cornell")
    a, b = device_films("cornell", (0, 2)), device_films("cornell", (1, 2))
    r = tracer("cornell")
    once = r.render_aov(seed=SEED, exact_ties=True)
    twice = r.render_aov(seed=SEED, exact_ties=True, films=once)
    assert twice["albedo"] is once["albedo"]
    for f in ("albedo", "normal", "depth"):
        rel = helpers.rel_l2(a[f] + b[f], whole[f])
        rel2 = helpers.rel_l2(twice[f].numpy(), 2.0 * whole[f])
        print(f, "shards relL2", rel, "two calls relL2", rel2)
        assert rel <= FILM_RELL2_TOL and rel2 <= FILM_RELL2_TOL
        assert np.abs(a[f]).sum() > 0 and np.abs(b[f]).sum() > 0


# 10 -----------------------------------------------------------------------------------------------------------------
def test_chunked_call_equals_the_unchunked(monkeypatch):
    """9 samples per pixel in chunks of 4, 4 and 1 (GBL_AOV_PASS_SPP caps what the per-sample budget allows)."""
    shape = (("resolution", (16, 16)), ("spp", 9), ("depth", 2))
    r = tracer("cornell", "host", shape)
    whole = r.render_aov(want_samples=True, seed=SEED, exact_ties=True)
    monkeypatch.setenv("GBL_AOV_PASS_SPP", "4")
    parts = r.render_aov(want_samples=True, seed=SEED, exact_ties=True)
    np.testing.assert_array_equal(Records(parts).rows, Records(whole).rows)
    assert_records_equal_oracle(Records(parts), ar.reference("cornell", **dict(shape)), "chunked")
    for f in ("albedo", "normal", "depth"):
        rel = helpers.rel_l2(parts[f].numpy(), whole[f].numpy())
        print(f, "chunked relL2", rel)
        assert rel <= FILM_RELL2_TOL and np.abs(whole[f].numpy()).sum() > 0


# 11 -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    r = tracer("cornell")
    with pytest.raises(_abi.GoblinError) as e:
        r.render_aov(sampler="stream")
    assert e.value.status == _abi.GBL_ERR_UNSUPPORTED
    with pytest.raises(_abi.GoblinError) as e:
        r.render_aov(albedo=False, normal=False, depth=False, want_samples=False)
    assert e.value.status == _abi.GBL_ERR_INVALID
    with pytest.raises(_abi.GoblinError) as e:
        r.render_aov(sampler="replay")
    assert e.value.status == _abi.GBL_ERR_INVALID
    for bad in (dict(window=(-3, 18, -2, 18)), dict(shard=(2, 2))):
        with pytest.raises(_abi.GoblinError) as e:
            r.render_aov(**bad)
        assert e.value.status == _abi.GBL_ERR_INVALID
    again = Records(r.render_aov(want_samples=True, seed=SEED, exact_ties=True))
    np.testing.assert_array_equal(again.rows, device_records("cornell").rows)
    film = r.render(seed=SEED)["film"].numpy()
    assert np.isfinite(film).all() and film[..., :3].max() > 0


def test_stats():
    r = tracer("cornell")
    plain = r.render_aov(seed=SEED, stats=True)["stats"]
    assert plain["paths"] == plain["extension_rays"] == 1600 and plain["kernel_ms"] > 0 and plain["shadow_rays"] == 0
    half = r.render_aov(seed=SEED, stats=True, shard=(0, 2))["stats"]
    other = r.render_aov(seed=SEED, stats=True, shard=(1, 2))["stats"]
    assert half["paths"] + other["paths"] == 1600 and 0 < half["paths"] < 1600


# 12 -----------------------------------------------------------------------------------------------------------------
def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline() == b"PF\n"
        w, h = (int(v) for v in f.readline().split())
        assert float(f.readline()) < 0      # little endian
        data = np.frombuffer(f.read(), "<f4")
    assert data.size == w * h * 3
    return data.reshape(h, w, 3)[::-1]     # rows are stored bottom to top


def test_command_line_tool_writes_the_feature_films(tmp_path):
    js, out = str(tmp_path / "cornell.json"), str(tmp_path / "cornell.pfm")
    ih.write_scene("cornell", gs.config_overrides(**ar.SHAPE), js, film_file=out)
    p = subprocess.run([CLI, js], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "Render Complete" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    assert sorted(os.listdir(tmp_path)) == ["cornell.json", "cornell.pfm"]
    beauty = read_pfm(out).copy()
    p = subprocess.run([CLI, js, "--aov"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "Render Complete" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    assert sorted(os.listdir(tmp_path)) == ["cornell.albedo.pfm", "cornell.depth.pfm", "cornell.json", "cornell.normal.pfm", "cornell.pfm"]
    assert helpers.rel_l2(read_pfm(out), beauty) <= FILM_RELL2_TOL      # the image itself does not change (two renders: summation order)
    r = tracer("cornell")
    want = r.render_aov(seed=0)
    depth, coverage = r.resolve_depth(want["depth"])
    torch.cuda.synchronize()
    depth_file = read_pfm(str(tmp_path / "cornell.depth.pfm"))
    rels = {"albedo": helpers.rel_l2(read_pfm(str(tmp_path / "cornell.albedo.pfm")), want["albedo"].normalized().cpu().numpy()),
            "normal": helpers.rel_l2(read_pfm(str(tmp_path / "cornell.normal.pfm")), want["normal"].normalized().cpu().numpy()),
            "depth": helpers.rel_l2(depth_file[..., 0], depth.cpu().numpy()),
            "coverage": helpers.rel_l2(depth_file[..., 1], coverage.cpu().numpy())}
    print("g_ray_hip --aov against the Python face, relL2", rels)
    assert max(rels.values()) <= FILM_RELL2_TOL and not depth_file[..., 2].any() and depth_file[..., 0].max() > 0


# 13 -----------------------------------------------------------------------------------------------------------------
def test_on_another_stream():
    r = tracer("cornell")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = r.render_aov(want_samples=True, seed=SEED, exact_ties=True)
        depth, coverage = r.resolve_depth(out["depth"])
    s.synchronize()
    np.testing.assert_array_equal(Records(out).rows, device_records("cornell").rows)
    want = device_films("cornell")
    for f in ("albedo", "normal", "depth"):
        assert helpers.rel_l2(out[f].numpy(), want[f]) <= FILM_RELL2_TOL
    d, c = ar.depth_and_coverage(out["depth"].numpy())
    np.testing.assert_array_equal(bits(depth.cpu().numpy()), bits(d))
    np.testing.assert_array_equal(bits(coverage.cpu().numpy()), bits(c))
