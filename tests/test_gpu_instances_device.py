"""gbl_update_instances_device, gbl_get_instances_device and gbl_selftest_instances on the device.

The frame and helpers are tests/test_gpu_refit.py's (48 x 48, 4 spp, depth 5, SEED 31337, both builders), the scenes
tests/meshes.instances_doc(n) -- the floor is instance 0, the line's instance k is instance k + 1 -- moved by
meshes.moved_transforms, and every tolerance is zero:

- flags == 0: a context edited from a tensor and a twin edited from the same floats as a list hold the same bytes -- the DevInstance
  and DevInstanceBound records of the new hook, the five geometry tables (as tests/test_gpu_vertices_device.py compares them),
  instances(), the TLAS root, stack_entries and gbl_info;
- GBL_INSTANCES_DEVICE_TLAS: the TLAS read back is a valid tree -- every instance reached once, no reference outside the used
  records, every child slot's dequantised box around the exact bounds beneath it, node count and levels as gbl_info says, and
  stack_entries at least the exact rule's 1 + need + 1, restated here over the records read back;
- in both modes the context renders, bit for bit, what a fresh context of the edited scene renders and what the oracle says;
- the host mirror, the raw table behind instances(device=True), and the order of vertex and instance edits;
- every refusal leaves every table's bytes alone.

Measured on an MI355X: the 33 tests take 3.2 s, the slowest 0.25 s; every radiance comparison printed flips 0.00000, relL2 0.00e+00
and 0 differing lean samples.  The 300-instance line, all moved: the device TLAS has 133 nodes in 16 levels, stack_entries 51 (52
over device-built BLASes); the host TLAS 133 nodes in 13 levels, stack_entries 41 (42).
"""
import ctypes as C

import numpy as np
import pytest

import meshes
import refit_reference as rr
import test_gpu_refit as base
import test_gpu_vertices_device as vd
from test_gpu_refit import dirs, torch   # noqa: F401  (module fixtures)
from goblin_amd import _abi
from goblin_amd import scene as gs

pytestmark = pytest.mark.gpu
SEED, BUILDERS, SCHEDULES = base.SEED, base.BUILDERS, base.SCHEDULES
INVALID, UNSUPPORTED = _abi.GBL_ERR_INVALID, _abi.GBL_ERR_UNSUPPORTED
SIZES = (2, 5, 65, 300)
REF_NONE = 0x7ffffffd
load, li_of, tracer = base.load, base.li_of, vd.tracer
F32 = np.float32


def rows(transforms):
    """(position, orientation, scale) tuples as the (n, 10) float32 rows of gbl_trs."""
    return np.array([list(p) + list(q) + list(s) for p, q, s in transforms], F32).reshape(-1, 10)


def on_device(torch, T, offset=0):
    """The rows as a tensor on the device; with `offset`, one that does not start at its storage's start."""
    T = np.ascontiguousarray(T, F32)
    buf = torch.zeros((len(T) + offset, 10), dtype=torch.float32, device="cuda:0")
    buf[offset:] = torch.from_numpy(T)
    t = buf[offset:]
    assert t.storage_offset() == 10 * offset and t.is_contiguous()
    return t


def as_tuples(T):
    return [(tuple(float(x) for x in r[:3]), tuple(float(x) for x in r[3:7]), tuple(float(x) for x in r[7:])) for r in np.asarray(T, F32)]


def instance_bytes(r):
    raw = r._instances_raw()
    assert raw["total"] == int(r.info.instances) == len(raw["records"]) == len(raw["bounds"])
    return raw["records"].tobytes(), raw["bounds"].tobytes(), raw["tlas_root"], raw["stack_entries"]


def assert_twins(a, b, bvh, what, whole=True):
    """vd.assert_twins and the new hook's records.  whole=False, for a context that has held a device-built TLAS: the records
    something refers to, not the whole node array -- a device tree uses more of the TLAS's reserved records than the host tree
    that replaces it, and the ones left over keep their bytes, unreferenced."""
    if whole:
        vd.assert_twins(a, b, bvh, what)
    else:
        ta, tb = vd.all_tables(a), vd.all_tables(b)
        for t in ("tris", "tri_bounds", "tri_order", "mesh_root"):
            assert ta[t].tobytes() == tb[t].tobytes(), (what, t)
        assert vd.used_nodes(a, ta, bvh) == vd.used_nodes(b, tb, bvh), (what, "nodes")
        assert a.instances() == b.instances(), what
        for f, _ in _abi.gbl_info._fields_:
            if f not in ("build_ms", "window"):
                assert getattr(a.info, f) == getattr(b.info, f), (what, f)
    ia, ib = instance_bytes(a), instance_bytes(b)
    for k, name in enumerate(("DevInstance records", "DevInstanceBound records", "tlas_root", "stack_entries")):
        assert ia[k] == ib[k], (what, name)


def snapshot(r, bvh):
    """Every byte a refusal must leave alone."""
    t = vd.all_tables(r)
    return ({k: v.tobytes() for k, v in t.items() if k != "nodes"}, vd.used_nodes(r, t, bvh), instance_bytes(r), r.instances(),
            r.instances(device=True).cpu().numpy().tobytes(), [getattr(r.info, f) for f, _ in _abi.gbl_info._fields_ if f not in ("build_ms", "window")])


def scene(dirs, n, moved=0, **kw):
    return load(meshes.instances_doc(n, moved=moved, **kw), dirs["a"])


# ---------------------------------------------------------------------------
# twins, flags == 0
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", BUILDERS)
@pytest.mark.parametrize("n", SIZES)
def test_a_tensor_edit_leaves_the_list_edits_bytes(torch, dirs, n, bvh):
    sc = scene(dirs, n)
    a, b = tracer(sc, bvh), tracer(sc, bvh)
    before = instance_bytes(a)
    T = rows(meshes.moved_transforms(n))
    a.update_instances(1, on_device(torch, T))
    b.update_instances(1, as_tuples(T))
    assert_twins(a, b, bvh, (n, bvh))
    assert instance_bytes(a)[0] != before[0] and instance_bytes(a)[1] != before[1]
    assert a.instances()[1:] == as_tuples(T)
    assert torch.equal(a.instances(device=True)[1:].cpu(), torch.from_numpy(T))
    # count == 0 with a valid pointer changes nothing
    a.update_instances(1, on_device(torch, T[:0]))
    assert_twins(a, b, bvh, (n, bvh, "empty edit"))


@pytest.mark.parametrize("bvh", BUILDERS)
def test_ranges_around_the_wave_and_workgroup_edges(torch, dirs, bvh):
    """n = 300: ranges whose compose launch ends at lane 63 / 64 / 65 and 255 / 256 / 257, ranges that start at those instances, and
    a tensor with a storage offset; the same pair of contexts takes them all, alternating between two sets of transforms."""
    n = 300
    sc = scene(dirs, n)
    a, b = tracer(sc, bvh), tracer(sc, bvh)
    sets = (rows(meshes.moved_transforms(n)), rows(meshes.line_transforms(n)))
    ranges = [(1, c) for c in (64, 65, 66, 256, 257, 258)] + [(f, n + 1 - f) for f in (63, 64, 65, 255, 256, 257)] + [(64, 1), (256, 2), (300, 1)]
    for step, (first, count) in enumerate(ranges):
        T = sets[step % 2][first - 1:first - 1 + count]
        assert len(T) == count
        a.update_instances(first, on_device(torch, T, offset=step % 3))
        b.update_instances(first, as_tuples(T))
        assert_twins(a, b, bvh, (bvh, first, count))


@pytest.mark.parametrize("bvh", BUILDERS)
def test_edge_transforms_on_the_device(torch, dirs, bvh):
    """The valid edge transforms of tests/instances_compose.cpp, composed by the kernel: non-uniform and negative scales, an
    unnormalised quaternion, -0.0 components, translations of 1e6, a uniform scale just above the determinant's threshold."""
    b0 = [0.3, -1.7, 2.9, 0.9238795, 0.0, 0.3826834, 0.0, 0.6, 0.6, 0.6]

    def with_(**ch):
        t = list(b0)
        for k, v in ch.items():
            t[int(k[1:])] = v
        return t
    T = np.array([with_(s7=0.2, s8=1.5, s9=3.0), with_(s7=-0.6), with_(s7=-0.6, s8=-1.1, s9=-0.4), with_(s3=1.7, s4=-0.4, s5=2.2, s6=0.9),
                  with_(s0=-0.0, s1=-0.0, s2=-0.0), with_(s4=-0.0, s6=-0.0), with_(s0=1e6, s1=-1e6, s2=1e6), with_(s7=0.0217, s8=0.0217, s9=0.0217),
                  with_(s3=1.0, s4=0.0, s5=0.0, s6=0.0, s7=1.0, s8=1.0, s9=1.0)], F32)
    sc = scene(dirs, 65)
    a, b = tracer(sc, bvh), tracer(sc, bvh)
    a.update_instances(3, on_device(torch, T, offset=1))
    b.update_instances(3, as_tuples(T))
    assert_twins(a, b, bvh, ("edge transforms", bvh))
    assert np.signbit(np.array(a.instances()[7][0])).all()      # the -0.0 position came through as it is


# ---------------------------------------------------------------------------
# the device TLAS is a valid tree
# ---------------------------------------------------------------------------
def blas_needs(nodes, roots):
    """Per mesh the exact traversal stack need of its BLAS (scene_prep.cpp node_stack_need), over refit_reference.plan_walk's records."""
    out = []
    for root in roots:
        recs, _ = rr.plan_walk(nodes, root)
        need = np.zeros(len(recs), np.int64)
        for i in range(len(recs) - 1, -1, -1):   # breadth first: children come after their parent
            child = nodes["child"][recs["node"][i]]
            k = int((child != REF_NONE).sum())
            deepest = max([0] + [int(need[p]) for p in recs["child_plan"][i] if p >= 0])
            need[i] = (k - 1 + deepest) if k > 0 else 0
        out.append(int(need[0]) if len(recs) else 0)
    return out


def check_device_tlas(r, bvh):
    """Walks the TLAS from tlas_root; returns (nodes used, levels, exact stack need of the scene)."""
    nodes = r._geometry("nodes")
    raw = r._instances_raw()
    where = base.tlas_slice(r, bvh)
    n_inst, tlas_base, used = raw["total"], where.start, int(r.info.tlas_nodes)
    assert used <= where.stop - where.start and raw["tlas_root"] == tlas_base
    mesh_need = blas_needs(nodes, r._geometry("mesh_root"))
    lo, hi = raw["bounds"]["lo"], raw["bounds"]["hi"]
    reached = np.zeros(n_inst, np.int64)
    visited = set()

    def walk(ref, level):
        """(levels below and including, stack need, bound lo, bound hi of the instances beneath)"""
        assert ref != REF_NONE
        if ref < 0:
            v = (~ref) & 0xffffffff
            assert v & 3 == 0 and (v >> 2) < n_inst, ref
            i = v >> 2
            reached[i] += 1
            rec = raw["records"][i]
            return 0, 1 + (mesh_need[rec["mesh"]] if rec["shape"] == 0 else 0), lo[i], hi[i]
        assert tlas_base <= ref < tlas_base + used and ref not in visited, ref
        visited.add(ref)
        nd = nodes[ref]
        levels, deepest, k = 0, 0, 0
        blo, bhi = np.full(3, np.inf, F32), np.full(3, -np.inf, F32)
        for c in range(4):
            child = int(nd["child"][c])
            if child == REF_NONE:
                assert all(((int(nd["qlo"][a]) >> (8 * c)) & 255) == 255 and ((int(nd["qhi"][a]) >> (8 * c)) & 255) == 0 for a in range(3))
                continue
            k += 1
            cl, need, clo, chi = walk(child, level + 1)
            qlo = np.array([(int(nd["qlo"][a]) >> (8 * c)) & 255 for a in range(3)], F32)
            qhi = np.array([(int(nd["qhi"][a]) >> (8 * c)) & 255 for a in range(3)], F32)
            slot_lo, slot_hi = nd["o"] + qlo * nd["scale"], nd["o"] + qhi * nd["scale"]      # float32, as the kernels dequantise
            assert (slot_lo <= clo).all() and (slot_hi >= chi).all(), (ref, c, slot_lo, clo, slot_hi, chi)
            levels, deepest = max(levels, cl), max(deepest, need)
            blo, bhi = np.minimum(blo, clo), np.maximum(bhi, chi)
        assert k >= 2
        return 1 + levels, k - 1 + deepest, blo, bhi
    levels, need, _, _ = walk(raw["tlas_root"], 1)
    assert (reached == 1).all(), np.nonzero(reached != 1)[0][:8]
    assert len(visited) == used == int(r.info.tlas_nodes)
    assert levels == int(r.info.tlas_depth)
    assert raw["stack_entries"] >= 1 + need + 1, (raw["stack_entries"], need)
    return used, levels, need, raw["stack_entries"]


@pytest.mark.parametrize("bvh", BUILDERS)
@pytest.mark.parametrize("n", SIZES)
def test_the_device_tlas_is_a_valid_tree(torch, dirs, n, bvh):
    r, twin = tracer(scene(dirs, n), bvh), tracer(scene(dirs, n), bvh)
    T = rows(meshes.moved_transforms(n))
    r.update_instances(1, on_device(torch, T), device_tlas=True)
    twin.update_instances(1, on_device(torch, T))
    used, levels, need, entries = check_device_tlas(r, bvh)
    print("n = %d, %s: device TLAS %d nodes, %d levels, exact need %d, stack_entries %d (host-built TLAS: %d nodes, %d levels, stack_entries %d)" %
          (n, bvh, used, levels, need, entries, twin.info.tlas_nodes, twin.info.tlas_depth, twin._instances_raw()["stack_entries"]))
    # everything but the tree is the flags == 0 edit's
    ra, rb = r._instances_raw(), twin._instances_raw()
    assert ra["records"].tobytes() == rb["records"].tobytes() and ra["bounds"].tobytes() == rb["bounds"].tobytes()
    assert r.instances() == twin.instances()
    # a host-tail edit puts the host's tree back
    r.update_instances(1, as_tuples(T[:1]))
    assert_twins(r, twin, bvh, (n, bvh, "host tail after a device TLAS"), whole=False)


@pytest.mark.parametrize("bvh", BUILDERS)
def test_device_tlas_over_awkward_boxes(torch, dirs, bvh):
    n = 64
    # 64 instances at one and the same transform: one Morton code, ordered by index
    r = tracer(scene(dirs, n), bvh)
    same = np.repeat(rows(meshes.moved_transforms(1)), n, axis=0)
    r.update_instances(1, on_device(torch, same), device_tlas=True)
    check_device_tlas(r, bvh)
    # a list goes the same way once uploaded
    r.update_instances(1, as_tuples(same), device_tlas=True)
    check_device_tlas(r, bvh)
    # an edit of a sub-range only: the untouched instances keep their records
    r = tracer(scene(dirs, n), bvh)
    before = r._instances_raw()
    T = rows(meshes.moved_transforms(n))
    r.update_instances(20, on_device(torch, T[19:40]), device_tlas=True)
    after = r._instances_raw()
    keep = np.ones(n + 1, bool)
    keep[20:41] = False
    for k in ("records", "bounds"):
        assert after[k][keep].tobytes() == before[k][keep].tobytes() and after[k][~keep].tobytes() != before[k][~keep].tobytes(), k
    check_device_tlas(r, bvh)
    # one instance 2^10 times the size of the others
    big = rows(meshes.line_transforms(n))
    big[31, 7:] *= F32(1024.0)
    r.update_instances(1, on_device(torch, big), device_tlas=True)
    check_device_tlas(r, bvh)


# ---------------------------------------------------------------------------
# renders
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n, moved", [(6, 2), (65, 65)])
def test_edited_contexts_render_what_a_fresh_one_and_the_oracle_do(torch, dirs, n, moved):
    base_scene, moved_scene = scene(dirs, n), scene(dirs, n, moved=moved)
    li_ref = base.oracle_li(moved_scene)
    T = rows(meshes.moved_transforms(moved))
    for bvh in BUILDERS:
        fresh = tracer(moved_scene, bvh)
        want = {s: li_of(fresh, schedule=s, exact_ties=True) for s in SCHEDULES}
        lean = {s: li_of(fresh, schedule=s) for s in SCHEDULES}
        for device_tlas in (False, True):
            r = tracer(base_scene, bvh)
            before = li_of(r, exact_ties=True)
            r.update_instances(1, on_device(torch, T), device_tlas=device_tlas)
            if n == 6 and bvh == "device" and not device_tlas:   # (the host's tree, no hot prefix: the fresh context's figures)
                assert base.tlas_facts(r) == base.tlas_facts(fresh), (base.tlas_facts(r), base.tlas_facts(fresh))
            for s in SCHEDULES:
                li = li_of(r, schedule=s, exact_ties=True)
                assert torch.equal(li, want[s]), (n, bvh, device_tlas, s)
                base.assert_equals_oracle(li, li_ref, (n, bvh, "device TLAS" if device_tlas else "host TLAS", s, "exact_ties"))
                # lean kernels break exact ties by the tree's order; on these tilted instances nothing ties exactly
                got = li_of(r, schedule=s)
                differing = int((got != lean[s]).any(dim=1).sum())
                print(n, bvh, device_tlas, s, "lean samples that differ from the fresh context's:", differing)
                assert differing == 0, (n, bvh, device_tlas, s, "lean")
            assert not torch.equal(li_of(r, exact_ties=True), before)


@pytest.mark.parametrize("bvh", BUILDERS)
def test_other_kernels_on_the_device_tlas(torch, dirs, bvh):
    """render_aov, motion() with prev_instances = instances() as it was, AO and Whitted: the device-built TLAS gives the host-built one's results."""
    n, moved = 65, 65
    T = on_device(torch, rows(meshes.moved_transforms(moved)))
    for method, ao in ((None, None), ("ao", 9), ("whitted", None)):
        doc = meshes.instances_doc(n)
        if method:
            doc["render_setting"]["render_method"] = method
        if ao:
            doc["render_setting"]["ao_sample_num"] = ao
        sc = load(doc, dirs["a"])
        dev, host = tracer(sc, bvh), tracer(sc, bvh)
        prev = dev.instances()
        before = li_of(dev)
        dev.update_instances(1, T, device_tlas=True)
        host.update_instances(1, T)
        li = li_of(dev)
        assert torch.equal(li, li_of(host)) and not torch.equal(li, before), (method, bvh)
        if method is None:
            for exact in (False, True):
                got, want = dev.render_aov(want_samples=True, seed=SEED, exact_ties=exact), host.render_aov(want_samples=True, seed=SEED, exact_ties=exact)
                assert torch.equal(got["samples_i32"], want["samples_i32"]), (bvh, exact, "aov records")
            cam = dev.camera()
            assert dev.instances() == host.instances() and dev.instances() != prev
            got, want = dev.motion(cam, prev), host.motion(cam, prev)
            assert torch.equal(got, want), (bvh, "motion planes")
            assert not torch.equal(got, dev.motion(cam, None))            # the moved instances are followed


# ---------------------------------------------------------------------------
# order and mirror
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", BUILDERS)
def test_vertex_and_instance_edits_commute_as_the_host_forms_do(torch, dirs, bvh):
    n, moved = 6, 2
    base_a, base_b = scene(dirs, n), load(meshes.instances_doc(n), dirs["jitter"])
    moved_b = load(meshes.instances_doc(n, moved=moved), dirs["jitter"])
    base.same_topology(base_a, base_b)
    PB = base.mesh_positions(base_b)[1]
    T = rows(meshes.moved_transforms(moved))
    want = li_of(tracer(moved_b, bvh), exact_ties=True)
    host = tracer(base_a, bvh)                      # the host forms: vertices, then instances
    host.update_vertices(1, PB)
    host.update_instances(1, as_tuples(T))
    for device_tlas in (False, True):
        r = tracer(base_a, bvh)                     # vertices, then instances from the device: the bound the vertex edit computed is used
        r.update_vertices(1, PB)
        r.update_instances(1, on_device(torch, T), device_tlas=device_tlas)
        other = tracer(base_a, bvh)                 # instances from the device, then vertices: the edit's TLAS tail reads the mirror
        other.update_instances(1, on_device(torch, T), device_tlas=device_tlas)
        other.update_vertices(1, PB)
        for ctx, what in ((r, "vertices then instances"), (other, "instances then vertices")):
            assert torch.equal(li_of(ctx, exact_ties=True), want), (bvh, device_tlas, what)
        assert_twins(other, host, bvh, (bvh, device_tlas, "instances then vertices"), whole=not device_tlas)      # (a vertex edit's tail is the host's tree)
        if not device_tlas:
            assert_twins(r, host, bvh, (bvh, "vertices then instances"))
        else:
            ra, rb = r._instances_raw(), host._instances_raw()
            assert ra["records"].tobytes() == rb["records"].tobytes() and ra["bounds"].tobytes() == rb["bounds"].tobytes()
            check_device_tlas(r, bvh)
        # a device vertex edit and a rebuild move the mesh bound too
        r.update_vertices(1, torch.from_numpy(np.ascontiguousarray(PB * F32(1.25))).cuda())
        r.rebuild_mesh(1)
        r.update_instances(1, on_device(torch, T), device_tlas=device_tlas)
        twin = tracer(base_a, bvh)
        twin.update_vertices(1, np.ascontiguousarray(PB * F32(1.25)))
        twin.rebuild_mesh(1)
        twin.update_instances(1, as_tuples(T))
        ra, rb = r._instances_raw(), twin._instances_raw()
        assert ra["records"].tobytes() == rb["records"].tobytes() and ra["bounds"].tobytes() == rb["bounds"].tobytes(), (bvh, device_tlas, "after a rebuild")
        assert torch.equal(li_of(r, exact_ties=True), li_of(twin, exact_ties=True))


@pytest.mark.parametrize("bvh", BUILDERS)
def test_the_mirror_and_the_raw_table(torch, dirs, bvh):
    n = 65
    sc = scene(dirs, n)
    r = tracer(sc, bvh)
    first_li = li_of(r, exact_ties=True)
    start = r.instances()
    S = rows(start)
    # before any edit the device form returns the scene's floats
    assert torch.equal(r.instances(device=True).cpu(), torch.from_numpy(S))
    T = rows(meshes.moved_transforms(n))
    r.update_instances(1, on_device(torch, T, offset=2), device_tlas=(bvh == "device"))
    # instances() after a device edit returns the tensor's floats bit for bit
    got = rows(r.instances())
    assert got[1:].tobytes() == T.tobytes() and got[:1].tobytes() == S[:1].tobytes()
    assert r.instances(device=True).cpu().numpy().tobytes() == got.tobytes()
    # a host edit after a device edit, then the device form: the host edit's floats
    H = rows(meshes.line_transforms(n))[10:20]
    r.update_instances(11, as_tuples(H))
    want = got.copy()
    want[11:21] = H
    assert r.instances(device=True).cpu().numpy().tobytes() == want.tobytes() and rows(r.instances()).tobytes() == want.tobytes()
    # a partial device edit leaves a partial stale range; the C entry reads a sub-range through it
    r.update_instances(30, on_device(torch, T[:5]))
    want[30:35] = T[:5]
    out = (_abi.gbl_trs * 3)()
    assert r.lib.gbl_get_instances(r.handle, 31, 3, out) == _abi.GBL_OK
    assert np.frombuffer(out, F32).reshape(3, 10).tobytes() == want[31:34].tobytes()
    assert rows(r.instances()).tobytes() == want.tobytes()
    # there and back returns the first render's bits
    r.update_instances(0, on_device(torch, S), device_tlas=True)
    assert torch.equal(li_of(r, exact_ties=True), first_li)
    r.update_instances(0, on_device(torch, S))
    assert torch.equal(li_of(r, exact_ties=True), first_li)
    twin = tracer(sc, bvh)
    twin.update_instances(0, start)
    assert_twins(r, twin, bvh, (bvh, "there and back"), whole=False)
    # the layouts update_instances turns away
    for bad in (torch.zeros((4, 10)), torch.zeros((4, 10), dtype=torch.float64, device="cuda:0"), torch.zeros((4, 3), dtype=torch.float32, device="cuda:0"),
                torch.zeros((4, 20), dtype=torch.float32, device="cuda:0")[:, ::2]):
        with pytest.raises(ValueError):
            r.update_instances(1, bad)


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def refused(r, status, needle, first, count, transforms, flags=0, host=None):
    """The device entry refuses with `status` and a message holding `needle`; `host` (rows) is what the host entry is given for the
    same call, whose status and message must then be the same."""
    ptr = None if transforms is None else transforms if isinstance(transforms, int) else transforms.data_ptr() if hasattr(transforms, "data_ptr") else transforms.ctypes.data
    st = r.lib.gbl_update_instances_device(r.handle, first, count, ptr, flags)
    msg = r.lib.gbl_last_error(r.handle).decode()
    assert st == status and needle in msg, (st, msg)
    if host is not None:
        arr = np.ascontiguousarray(host, F32)
        assert r.lib.gbl_update_instances(r.handle, first, count, C.cast(arr.ctypes.data, C.POINTER(_abi.gbl_trs))) == status
        assert r.lib.gbl_last_error(r.handle).decode() == msg


@pytest.mark.parametrize("bvh", BUILDERS)
def test_refusals_leave_every_table_alone(torch, dirs, bvh):
    n = 65
    r = tracer(scene(dirs, n), bvh)
    r.update_instances(1, on_device(torch, rows(meshes.moved_transforms(n))[:7]))      # (the raw table and the mirror are in play)
    before, li_before = snapshot(r, bvh), li_of(r)
    good_h = rows(meshes.line_transforms(n))
    good = on_device(torch, good_h)
    assert r.lib.gbl_update_instances_device(None, 1, 4, good.data_ptr(), 0) == INVALID
    refused(r, INVALID, "d_to_world is NULL", 1, 4, None)
    refused(r, INVALID, "flags", 1, 4, good, flags=2)
    refused(r, INVALID, "flags", 1, 4, good, flags=0x80000001)
    refused(r, INVALID, "instance range out of bounds", n - 2, 4, good, host=good_h)
    refused(r, INVALID, "instance range out of bounds", 0xffffffff, 4, good, host=good_h)
    refused(r, INVALID, "not device memory", 1, 4, good_h)                              # a host pointer, refused before anything reads it
    with open("/proc/self/maps") as f:   # the HIP runtime this process already runs on, not a second copy of it
        hip = C.CDLL(next(line.split()[-1] for line in f if "libamdhip64" in line))
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(156)) == 0                          # 4 bytes short of four records
    try:
        refused(r, INVALID, "allocation ends", 1, 4, short.value)
        refused(r, INVALID, "allocation ends", 1, 3, short.value + 40)
        out = r.lib.gbl_get_instances_device(r.handle, 0, 4, short.value)
        assert out == INVALID and "allocation ends" in r.lib.gbl_last_error(r.handle).decode()
    finally:
        assert hip.hipFree(short) == 0
    assert r.lib.gbl_get_instances_device(r.handle, 0, 4, None) == INVALID
    assert r.lib.gbl_get_instances_device(r.handle, n, 4, good.data_ptr()) == INVALID
    # met by the kernel: a float that is not finite, then the determinant; at index 0, in the middle, last, and two at once
    count = n                                                                           # instances 1 .. n
    for flags in (0, _abi.GBL_INSTANCES_DEVICE_TLAS):
        for where in ((0,), (count // 2,), (count - 1,), (count - 1, 17), (40, 3)):
            for bad, slot in ((np.nan, 0), (np.inf, 4), (-np.inf, 9)):
                t = good_h.copy()
                for w in where:
                    t[w, slot] = bad
                refused(r, INVALID, "the transform of instance %d is not finite" % (1 + min(where)), 1, count, on_device(torch, t), flags=flags)
            t = good_h.copy()
            for w in where:
                t[w, 7:] = 0.0215                                                       # |det| just below 1e-5
            refused(r, INVALID, "instance %d: |det(toWorld)| < 1e-5" % (1 + min(where)), 1, count, on_device(torch, t), flags=flags, host=t)
        # non-finite is tested before the determinant, whatever their indices
        t = good_h.copy()
        t[2, 7:] = 0.0
        t[50, 5] = np.nan
        refused(r, INVALID, "the transform of instance 51 is not finite", 1, count, on_device(torch, t), flags=flags)
    # a world bound that overflows a float cannot go into a device TLAS
    t = good_h.copy()
    t[9, :3] = 3.4e38                                                                  # (max float is 3.4028e38: a corner 1e36 further out is beyond it)
    t[9, 7:] = 1e36
    refused(r, INVALID, "the world bound of instance 10 is not finite", 1, count, on_device(torch, t), flags=_abi.GBL_INSTANCES_DEVICE_TLAS)
    with pytest.raises(_abi.GoblinError) as e:
        r.update_instances(n - 2, good[:4])
    assert e.value.status == INVALID
    after = snapshot(r, bvh)
    for k, (x, y) in enumerate(zip(before, after)):
        assert x == y, ("table group", k)
    assert torch.equal(li_of(r), li_before)


def test_light_refusals_are_the_host_entrys(torch, dirs):
    ov = gs.config_overrides(resolution=(16, 16), spp=1, depth=2)
    # cornell.json: an instance carries the area light
    r = tracer(gs.load_scene("cornell", ov))
    lit = next(i for i in range(r.scene.desc.num_instances) if r.scene.desc.instances[i].area_light >= 0)
    S = rows(r.instances())
    before, raw_before = li_of(r), instance_bytes(r)
    refused(r, UNSUPPORTED, "carries an area light", lit, 1, on_device(torch, S[lit:lit + 1]), host=S[lit:lit + 1])
    refused(r, UNSUPPORTED, "instance %d carries an area light" % lit, 0, len(S), on_device(torch, S), flags=_abi.GBL_INSTANCES_DEVICE_TLAS, host=S)
    assert instance_bytes(r) == raw_before and torch.equal(li_of(r), before) and rows(r.instances()).tobytes() == S.tobytes()
    # ibl.json: an image based light is sized by the scene bound
    r = tracer(gs.load_scene("ibl", ov))
    S = rows(r.instances())
    before, raw_before = li_of(r), instance_bytes(r)
    refused(r, UNSUPPORTED, "scene bound", 0, 1, on_device(torch, S[:1]), host=S[:1])
    with pytest.raises(_abi.GoblinError) as e:
        r.update_instances(0, on_device(torch, S[:1]), device_tlas=True)
    assert e.value.status == UNSUPPORTED
    assert instance_bytes(r) == raw_before and torch.equal(li_of(r), before)
    assert torch.equal(r.instances(device=True).cpu(), torch.from_numpy(S))
    # a directional light
    doc = meshes.instances_doc(5)
    doc["lights"].append({"name": "sun", "type": "directional", "radiance": [1, 1, 1], "direction": [0, -1, 0]})
    r = tracer(load(doc, dirs["a"]))
    S = rows(r.instances())
    refused(r, UNSUPPORTED, "directional", 1, 2, on_device(torch, S[1:3]), host=S[1:3])
