"""gbl_trace_rays_filtered on the device: the isOpaque / notOpaque filters and the transmittance of a shadow segment, ray by ray.

Scenes and rays: tests/query_filtered_cases.py -- the pane stack with its lattices (514 rays), the bundled masked.json under camera
rays, rays from a sphere and chords (2 784 rays), the bundled cornell for a scene without masks.  The oracle has no filter of its
own: a filtered query of the full scene is compared with the unfiltered one of a scene that holds one side of the filter only
(tests/test_query_filtered_cpu.py shows that no ray meets two instances at one t, where that stand-in could not decide).

1. filter = removal: OPAQUE / MASK on the full scene against gbl_trace_rays on the sub-scene, all 32 bytes of every record with
   the instance mapped, both builders, lean and exact, with and without normals, any-hit; in exact mode also the sub-scene's oracle;
2. transmittance on the pane stack equals query_filtered_cases.chain bit for bit, lean and exact -- but on the 18 rays through the two
   image alphas, where `crossed` is equal and tr lies within query_filtered_cases.IMAGE_TOLERANCE (11 x 2^-24 x tint, derived there:
   the reference's `nearest` is a bilinear sum of four taps, whose roundings a restatement without the hit's uv cannot follow);
3. transmittance on masked.json: bit equality where only constant alphas are met, one of the checkerboards' alternatives elsewhere;
4. a scene without masks;  5. material and instance edits are seen in stream order;  6. refill and phases under one workgroup;
7. every refusal.

Measured on an MI355X: the 11 tests take 2.8 s.  Filtered and sub-scene records differ on no ray (514 and 2 784 rays, two builders,
lean and exact); the pane stack's transmittance equals the chain bit for bit on 496 rays and on 16 of the 18 image-alpha rays, the
other two within 0.09 of their bound; a material edit changes 117 of the 153 rays through P1 (the rest were Black already), the
instance edit all 171 through P0.

Bounds: bit equality everywhere but for the image alphas of 2; in 3, membership in the finite set of products the two alphas of each checkerboard allow.
"""
import ctypes as C

import numpy as np
import pytest

import query_cases as qc
import query_filtered_cases as fc
from goblin_amd import _abi
from goblin_amd import scene as gs

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = _abi.GBL_ERR_INVALID, _abi.GBL_ERR_UNSUPPORTED
CLOSEST, ANY, TRANSMIT = _abi.GBL_QUERY_CLOSEST, _abi.GBL_QUERY_ANY, _abi.GBL_QUERY_TRANSMITTANCE
NONE, OPAQUE, MASK = _abi.GBL_QUERY_FILTER_NONE, _abi.GBL_QUERY_FILTER_OPAQUE, _abi.GBL_QUERY_FILTER_MASK
TIES, NORMAL = _abi.GBL_QUERY_EXACT_TIES, _abi.GBL_QUERY_SHADING_NORMAL
F32 = np.float32
REC = np.dtype([("t", "<f4"), ("b1", "<f4"), ("b2", "<f4"), ("instance", "<i4"), ("primitive", "<u4"), ("n", "<f4", 3)])
TREC = np.dtype([("tr", "<f4", 3), ("crossed", "<u4")])
_shared = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def tracer(scene, bvh="host"):
    from goblin_amd.renderer import HipPathTracer
    return HipPathTracer(scene, 0, bvh=bvh)


def dev(torch, a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to("cuda:0")   # (a copy: the shared arrays are read-only)


def closest(torch, r, rays, **kw):
    out = r.trace(rays, **kw)["records"]
    torch.cuda.synchronize()
    return np.ascontiguousarray(out.cpu().numpy(), F32).view(REC).reshape(-1)


def occluded(torch, r, rays, **kw):
    out = r.trace(rays, kind="any", **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def transmittance(torch, r, rays, **kw):
    out = r.trace(rays, kind="transmittance", **kw)["records"]
    torch.cuda.synchronize()
    return np.ascontiguousarray(out.cpu().numpy(), F32).view(TREC).reshape(-1)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def shared(name):
    """Per scene, computed once and left unchanged: the case, its rays, the sub-scenes' oracle answers and the chain."""
    if name not in _shared:
        case = fc.pane_stack() if name == "pane_stack" else fc.masked()
        rays = fc.pane_rays()[0] if name == "pane_stack" else fc.masked_rays(case)
        s = dict(case=case, rays=rays, ref={side: fc.sub_answers(case, side, rays) for side in ("opaque", "mask")})
        s["tr"], s["crossed"], s["met"], s["two"] = fc.chains(case, rays)
        s["bound"] = fc.image_bound(case, s["met"]) if name == "pane_stack" else None
        for v in [s["tr"], s["crossed"]] + [a for ref in s["ref"].values() for a in ref.values()]:
            v.setflags(write=False)
        _shared[name] = s
    return _shared[name]


def mapped(records, to_full):
    out = records.copy()
    hit = out["instance"] >= 0
    out["instance"][hit] = to_full[out["instance"][hit]]
    return out


# ---------------------------------------------------------------------------
# 1. a filter removes one side of the scene
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", ["host", "device"])
@pytest.mark.parametrize("name", ["pane_stack", "masked"])
def test_a_filtered_query_is_the_query_of_the_scene_without_the_other_side(torch, name, bvh):
    s = shared(name)
    case, rays = s["case"], dev(torch, s["rays"])
    full = tracer(case.full, bvh)
    for side in ("opaque", "mask"):
        sub, to_full, ref = tracer(case.sub[side], bvh), case.to_full[side], s["ref"][side]
        for ties in (False, True):
            for normals in (False, True):
                got = closest(torch, full, rays, filter=side, exact_ties=ties, normals=normals)
                want = mapped(closest(torch, sub, rays, exact_ties=ties, normals=normals), to_full)
                differ = (got.view(np.uint32).reshape(-1, 8) != want.view(np.uint32).reshape(-1, 8)).any(axis=1)
                assert not differ.any(), (side, ties, normals, np.flatnonzero(differ)[:8])
                assert normals or not got["n"].any()
                if ties:
                    assert np.array_equal(got["instance"], ref["instance"]) and np.array_equal(bits(got["t"]), bits(ref["t"])), side
                    if normals:
                        assert np.array_equal(bits(got["n"]), bits(ref["normal"])), side
            occ = occluded(torch, full, rays, filter=side, exact_ties=ties)
            assert np.array_equal(occ, occluded(torch, sub, rays, exact_ties=ties)), (side, ties)
            if ties:
                assert np.array_equal(occ, ref["occluded"]), side
        hits = int((ref["instance"] >= 0).sum())
        print(name, bvh, side, "hits", hits, "of", len(s["rays"]), "occluded", int(ref["occluded"].sum()))
        assert 4 * hits >= len(s["rays"])
    # the two sides differ from the unfiltered scene and from each other: the filter did something
    none = closest(torch, full, rays, exact_ties=True)
    assert (none["instance"] != s["ref"]["opaque"]["instance"]).any() and (none["instance"] != s["ref"]["mask"]["instance"]).any()
    # filter="none" through the filtered entry: gbl_trace_rays' bytes
    out = torch.zeros((len(s["rays"]), 8), dtype=torch.float32, device="cuda:0")
    assert full.lib.gbl_trace_rays_filtered(full.handle, CLOSEST, NONE, rays.data_ptr(), len(s["rays"]), out.data_ptr(), TIES, None) == _abi.GBL_OK
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == none.tobytes()


# ---------------------------------------------------------------------------
# 2. transmittance on the pane stack
# ---------------------------------------------------------------------------
def assert_equals_chain(got, tr, crossed, where=None, what="", bound=None):
    """Bit for bit; where `bound` (n, 3) is not zero -- a ray through an image alpha, query_filtered_cases.IMAGE_TOLERANCE -- tr
    within it and crossed equal."""
    k = np.arange(len(got)) if where is None else np.flatnonzero(where)
    bad = (bits(got["tr"][k]) != bits(tr[k])).any(axis=1)
    if bound is not None:
        loose = bound[k].any(axis=1)
        err = np.abs(got["tr"][k].astype(np.float64) - tr[k].astype(np.float64))
        if loose.any():
            print(what, "image-alpha rays", int(loose.sum()), "not bit-equal", int((bad & loose).sum()), "largest error / bound %.3g" % float((err[loose] / bound[k][loose]).max()))
        bad = np.where(loose, (err > bound[k]).any(axis=1), bad)
    bad = bad | (got["crossed"][k] != crossed[k])
    assert not bad.any(), (what, k[bad][:8], got[k[bad][:4]], tr[k[bad][:4]], crossed[k[bad][:4]])


@pytest.mark.parametrize("bvh", ["host", "device"])
def test_transmittance_on_the_pane_stack_equals_the_chain(torch, bvh):
    s = shared("pane_stack")
    r = tracer(s["case"].full, bvh)
    rays = dev(torch, s["rays"])
    for ties in (False, True):
        got = transmittance(torch, r, rays, exact_ties=ties)
        assert_equals_chain(got, s["tr"], s["crossed"], what=(bvh, ties), bound=s["bound"])
    counts = np.bincount(s["crossed"][s["crossed"] < fc.OCCLUDED_BIT], minlength=5)
    print("crossed 0..4:", counts[:5], "occluded:", int((s["crossed"] == fc.OCCLUDED_BIT).sum()))
    assert (counts[:5] > 0).all()
    # the Python face's views
    d = r.trace(rays, kind="transmittance", exact_ties=True)
    torch.cuda.synchronize()
    assert np.array_equal(bits(d["tr"].cpu().numpy()), bits(got["tr"]))
    assert np.array_equal(d["crossed"].cpu().numpy(), (s["crossed"] & 0x7fffffff).astype(np.int32))
    assert np.array_equal(d["occluded"].cpu().numpy(), s["crossed"] == fc.OCCLUDED_BIT)


# ---------------------------------------------------------------------------
# 3. transmittance on masked.json
# ---------------------------------------------------------------------------
def test_transmittance_on_the_masked_scene(torch):
    s = shared("masked")
    case, rays = s["case"], s["rays"]
    r = tracer(case.full)
    d_rays = dev(torch, rays)
    got = transmittance(torch, r, d_rays, exact_ties=True)
    constant = s["two"] == 0                       # the chain met pane and ghost only (or nothing, or an occluder)
    crossed_some = constant & (s["crossed"] > 0) & (s["crossed"] < fc.OCCLUDED_BIT)
    print("rays", len(rays), "constant-alpha chains", int(constant.sum()), "of which cross a mask", int(crossed_some.sum()), "checkerboard chains",
          int((~constant).sum()))
    assert crossed_some.sum() >= 50 and (~constant).sum() >= 50
    assert_equals_chain(got, s["tr"], s["crossed"], constant, "constant alphas")
    # the occluder bit is the OPAQUE any-hit answer, on every ray
    occ = occluded(torch, r, d_rays, filter="opaque", exact_ties=True)
    assert np.array_equal(got["crossed"] == fc.OCCLUDED_BIT, occ != 0)
    assert not (got["crossed"][occ == 0] & fc.OCCLUDED_BIT).any()
    # a chain through checkerboards: one of the products its surfaces' alternatives allow
    for i in np.flatnonzero(~constant):
        allowed = fc.chain_alternatives(case, rays[i])
        assert (bits(got["tr"][i]).tobytes(), int(got["crossed"][i])) in allowed, (i, got[i], s["met"][i])
    lean = transmittance(torch, r, d_rays)
    same = (lean.view(np.uint32).reshape(-1, 4) == got.view(np.uint32).reshape(-1, 4)).all(axis=1)
    print("lean records that differ from exact:", int((~same).sum()))
    # (lean: the occlusion query's own invariant -- never unoccluded where the exact query is occluded)
    assert ((lean["crossed"] == fc.OCCLUDED_BIT) >= (got["crossed"] == fc.OCCLUDED_BIT)).all()


# ---------------------------------------------------------------------------
# 4. a scene without masks
# ---------------------------------------------------------------------------
def test_a_scene_without_masks(torch):
    import oracle_binding as ob
    scene = gs.load_scene("cornell")
    bound = qc.scene_bound(scene, skip_floor=False)
    rays = np.concatenate([qc.camera_rays(ob.Oracle(scene)), qc.sphere_rays(bound, 600), qc.chord_rays(bound, 600), qc.INVALID_RAYS])
    r = tracer(scene)
    d_rays = dev(torch, rays)
    for ties in (False, True):
        for normals in (False, True):
            plain = closest(torch, r, d_rays, exact_ties=ties, normals=normals)
            assert closest(torch, r, d_rays, filter="opaque", exact_ties=ties, normals=normals).tobytes() == plain.tobytes()
            miss = closest(torch, r, d_rays, filter="mask", exact_ties=ties, normals=normals)
            assert (miss["t"] == -1.0).all() and (miss["instance"] == -1).all()
            assert not miss["b1"].any() and not miss["b2"].any() and not miss["primitive"].any() and not miss["n"].any()
        occ = occluded(torch, r, d_rays, exact_ties=ties)
        assert 0 < occ.sum() < len(occ) and (plain["instance"] >= 0).sum() > len(rays) // 4
        assert np.array_equal(occluded(torch, r, d_rays, filter="opaque", exact_ties=ties), occ)
        assert not occluded(torch, r, d_rays, filter="mask", exact_ties=ties).any()
        tr = transmittance(torch, r, d_rays, exact_ties=ties)
        assert (tr["tr"] == np.where(occ[:, None] != 0, F32(0.0), F32(1.0))).all()
        assert np.array_equal(tr["crossed"], np.where(occ != 0, fc.OCCLUDED_BIT, 0).astype(np.uint32))
        # ... under the capped grid of the self-test hook as well
        assert transmittance(torch, r, d_rays, exact_ties=ties, _max_workgroups=1).tobytes() == tr.tobytes()


# ---------------------------------------------------------------------------
# 5. edits are seen, in stream order
# ---------------------------------------------------------------------------
def test_a_material_edit_and_an_instance_edit_are_seen_in_stream_order(torch):
    s = shared("pane_stack")
    case = s["case"]
    rays, d_rays = s["rays"], dev(torch, s["rays"])
    p1 = 1   # P1 among the mask-only instances
    through_p1 = np.array([p1 in m for m in s["met"]])
    r = tracer(case.full)
    before = transmittance(torch, r, d_rays, exact_ties=True)
    assert_equals_chain(before, s["tr"], s["crossed"], bound=s["bound"])
    # P1's alpha: the edit queued, then the query behind it, then one synchronise to read
    material = int(case.full.desc.instances[int(case.to_full["mask"][p1])].material)
    edited = fc.pane_case(p1_alpha=0.125)
    tr, crossed, _, _ = fc.chains(edited, rays)
    r.update_materials(material, exponent=0.125)
    got = r.trace(d_rays, kind="transmittance", exact_ties=True)["records"]
    torch.cuda.synchronize()
    got = np.ascontiguousarray(got.cpu().numpy(), F32).view(TREC).reshape(-1)
    assert_equals_chain(got, tr, crossed, what="P1's alpha", bound=s["bound"])
    changed = (got.view(np.uint32).reshape(-1, 4) != before.view(np.uint32).reshape(-1, 4)).any(axis=1)
    expect = (bits(tr) != bits(s["tr"])).any(axis=1) | (crossed != s["crossed"])
    print("rays through P1:", int(through_p1.sum()), "changed by its alpha:", int(changed.sum()))
    assert np.array_equal(changed, expect) and changed.sum() > 0 and not (changed & ~through_p1).any()
    # ... every ray through P1 whose product was not Black already
    assert np.array_equal(changed, through_p1 & s["tr"].any(axis=1))
    # P0 moved out of its columns, from a device tensor
    p0 = 0
    through_p0 = np.array([p0 in m for m in s["met"]])
    moved = fc.pane_case(p1_alpha=0.125, p0_offset=(0.0, 10.0, 0.0))
    tr2, crossed2, met2, _ = fc.chains(moved, rays)
    assert not any(p0 in m for m in met2)
    pos, quat, scale = fc.world_trs(fc.pane_instances(p0_offset=(0.0, 10.0, 0.0))[1])
    rows = dev(torch, np.array([list(pos) + list(quat) + list(scale)], F32))
    r.update_instances(int(case.to_full["mask"][p0]), rows)
    got2 = r.trace(d_rays, kind="transmittance", exact_ties=True)["records"]
    torch.cuda.synchronize()
    got2 = np.ascontiguousarray(got2.cpu().numpy(), F32).view(TREC).reshape(-1)
    assert_equals_chain(got2, tr2, crossed2, what="P0 moved", bound=s["bound"])
    changed2 = (got2.view(np.uint32).reshape(-1, 4) != got.view(np.uint32).reshape(-1, 4)).any(axis=1)
    print("rays through P0:", int(through_p0.sum()), "changed by its move:", int(changed2.sum()))
    assert changed2.sum() > 0 and not (changed2 & ~through_p0).any()
    assert np.array_equal(changed2, (bits(tr2) != bits(tr)).any(axis=1) | (crossed2 != crossed))


# ---------------------------------------------------------------------------
# 6. refill and phases: one workgroup
# ---------------------------------------------------------------------------
REFILL_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129)


def test_refill_and_phases_under_one_workgroup(torch):
    s = shared("pane_stack")
    order = np.random.default_rng(7101).permutation(np.tile(np.arange(len(s["rays"])), 4))[:2000]
    rays = dev(torch, s["rays"][order])
    r = tracer(s["case"].full)
    for ties in (False, True):
        whole = transmittance(torch, r, rays, exact_ties=ties)
        assert_equals_chain(whole, s["tr"][order], s["crossed"][order], what=("mixed", ties), bound=s["bound"][order])
        assert transmittance(torch, r, rays, exact_ties=ties, _max_workgroups=1).tobytes() == whole.tobytes()
        kinds = np.stack([whole["crossed"][a:a + 64] for a in range(0, 1984, 64)])
        # lanes of one wave's first 64 rays end occluded, clear and after one to four surfaces: the phases are mixed
        assert ((kinds == fc.OCCLUDED_BIT).any(axis=1) & (kinds == 0).any(axis=1) & ((kinds > 1) & (kinds < 5)).any(axis=1)).all()
        for n in REFILL_COUNTS:
            part = rays[:n].contiguous()
            assert transmittance(torch, r, part, exact_ties=ties, _max_workgroups=1).tobytes() == whole[:n].tobytes(), n
            assert transmittance(torch, r, part, exact_ties=ties).tobytes() == whole[:n].tobytes(), n
        for side in ("opaque", "mask"):
            for normals in (False, True):
                hits = closest(torch, r, rays, filter=side, exact_ties=ties, normals=normals)
                assert closest(torch, r, rays, filter=side, exact_ties=ties, normals=normals, _max_workgroups=1).tobytes() == hits.tobytes()
            occ = occluded(torch, r, rays, filter=side, exact_ties=ties)
            assert np.array_equal(occluded(torch, r, rays, filter=side, exact_ties=ties, _max_workgroups=1), occ)
            hits = closest(torch, r, rays, filter=side, exact_ties=ties)
            for n in REFILL_COUNTS:
                part = rays[:n].contiguous()
                assert closest(torch, r, part, filter=side, exact_ties=ties, _max_workgroups=1).tobytes() == hits[:n].tobytes()
                assert np.array_equal(occluded(torch, r, part, filter=side, exact_ties=ties, _max_workgroups=1), occ[:n])
    assert r.trace(rays[:0], kind="transmittance")["records"].shape == (0, 4)


# ---------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------
def test_refusals(torch):
    s = shared("pane_stack")
    r = tracer(s["case"].full)
    lib, h = r.lib, r.handle
    n = 64
    rays = dev(torch, s["rays"][:n])
    out = torch.full((n, 8), 7.0, dtype=torch.float32, device="cuda:0")

    def refused(status, needle, kind, filt, d_rays, count, d_out, flags):
        for call in (lambda: lib.gbl_trace_rays_filtered(h, kind, filt, d_rays, count, d_out, flags, None),
                     lambda: lib.gbl_selftest_query_filtered(h, kind, filt, d_rays, count, d_out, flags, 0)):
            assert call() == status, needle
            assert needle in lib.gbl_last_error(h).decode(), (needle, lib.gbl_last_error(h).decode())

    assert lib.gbl_trace_rays_filtered(None, CLOSEST, OPAQUE, rays.data_ptr(), n, out.data_ptr(), 0, None) == INVALID
    assert lib.gbl_selftest_query_filtered(None, CLOSEST, OPAQUE, rays.data_ptr(), n, out.data_ptr(), 0, 0) == INVALID
    for kind, filt in ((CLOSEST, OPAQUE), (ANY, MASK), (TRANSMIT, NONE)):
        refused(INVALID, "null pointer", kind, filt, None, n, out.data_ptr(), 0)
        refused(INVALID, "null pointer", kind, filt, rays.data_ptr(), n, None, 0)
        refused(INVALID, "flags", kind, filt, rays.data_ptr(), n, out.data_ptr(), 4)
        refused(INVALID, "flags", kind, filt, rays.data_ptr(), n, out.data_ptr(), 0x80000001)
        refused(UNSUPPORTED, "2^32", kind, filt, rays.data_ptr(), 1 << 32, out.data_ptr(), 0)
    refused(INVALID, "unknown kind", 3, NONE, rays.data_ptr(), n, out.data_ptr(), 0)
    refused(INVALID, "unknown filter", CLOSEST, 3, rays.data_ptr(), n, out.data_ptr(), 0)
    refused(INVALID, "unknown filter", ANY, 0x80000001, rays.data_ptr(), n, out.data_ptr(), 0)
    refused(INVALID, "GBL_QUERY_SHADING_NORMAL", ANY, OPAQUE, rays.data_ptr(), n, out.data_ptr(), NORMAL)
    refused(INVALID, "GBL_QUERY_SHADING_NORMAL", TRANSMIT, NONE, rays.data_ptr(), n, out.data_ptr(), NORMAL)
    refused(INVALID, "GBL_QUERY_TRANSMITTANCE takes GBL_QUERY_FILTER_NONE", TRANSMIT, OPAQUE, rays.data_ptr(), n, out.data_ptr(), 0)
    refused(INVALID, "GBL_QUERY_TRANSMITTANCE takes GBL_QUERY_FILTER_NONE", TRANSMIT, MASK, rays.data_ptr(), n, out.data_ptr(), TIES)
    host_rays, host_out = np.ascontiguousarray(s["rays"][:n]), np.zeros((n, 8), F32)
    refused(INVALID, "d_rays is not device memory", TRANSMIT, NONE, host_rays.ctypes.data, n, out.data_ptr(), 0)   # refused before anything reads it
    refused(INVALID, "d_out is not device memory", CLOSEST, MASK, rays.data_ptr(), n, host_out.ctypes.data, 0)
    both = torch.zeros((2 * n, 8), dtype=torch.float32, device="cuda:0")
    both[:n] = rays
    refused(INVALID, "overlaps", CLOSEST, OPAQUE, both.data_ptr(), n, both.data_ptr() + 32 * (n - 1), 0)
    refused(INVALID, "overlaps", TRANSMIT, NONE, both.data_ptr(), n, both.data_ptr() + 32 * n - 1, 0)
    with open("/proc/self/maps") as f:   # the HIP runtime this process already runs on, not a second copy of it
        hip = C.CDLL(next(line.split()[-1] for line in f if "libamdhip64" in line))
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(16 * n - 4)) == 0   # 4 bytes short of n transmittance records; never launched
    try:
        refused(INVALID, "d_out: its allocation ends", TRANSMIT, NONE, rays.data_ptr(), n, short.value, 0)
        refused(INVALID, "d_out: its allocation ends", CLOSEST, OPAQUE, rays.data_ptr(), n, short.value, 0)
        assert lib.gbl_trace_rays_filtered(h, ANY, OPAQUE, rays.data_ptr(), n, short.value, 0, None) == _abi.GBL_OK   # ... which n bytes fit
    finally:
        torch.cuda.synchronize()
        assert hip.hipFree(short) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()   # nothing was launched
    # n == 0: GBL_OK whatever the pointers
    assert lib.gbl_trace_rays_filtered(h, TRANSMIT, NONE, None, 0, None, 0, None) == _abi.GBL_OK
    assert lib.gbl_trace_rays_filtered(h, ANY, MASK, rays.data_ptr(), 0, out.data_ptr(), TIES, None) == _abi.GBL_OK
    # gbl_trace_rays itself accepts none of the new values
    for call in (lambda *a: lib.gbl_trace_rays(h, *a, None), lambda *a: lib.gbl_selftest_query(h, *a, 0)):
        assert call(CLOSEST, rays.data_ptr(), n, out.data_ptr(), 4) == INVALID and "flags" in lib.gbl_last_error(h).decode()
        assert call(ANY, rays.data_ptr(), n, out.data_ptr(), 0x80000001) == INVALID and "flags" in lib.gbl_last_error(h).decode()
        assert call(TRANSMIT, rays.data_ptr(), n, out.data_ptr(), 0) == INVALID and "unknown kind" in lib.gbl_last_error(h).decode()
    # the Python face's own checks
    with pytest.raises(ValueError):
        r.trace(rays, kind="transmittance", normals=True)
    with pytest.raises(ValueError):
        r.trace(rays, kind="transmittance", filter="opaque")
    with pytest.raises(ValueError):
        r.trace(rays, filter="translucent")
    with pytest.raises(ValueError):
        r.trace(rays, kind="any", filter="mask", normals=True)
    # the context still answers
    got = transmittance(torch, r, dev(torch, s["rays"]), exact_ties=True)
    assert_equals_chain(got, s["tr"], s["crossed"], bound=s["bound"])
