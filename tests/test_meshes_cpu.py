"""The adversarial meshes of tests/meshes.py without a GPU: the shape restatement checks itself, and the oracle is pinned to
the compiled reference (oracle/_ref/ref_harness) on every one of the scenes tests/test_gpu_meshes.py renders -- so that the
device's bar there (equal to the oracle bit for bit) is the reference's."""
import json
import os
import subprocess

import numpy as np
import pytest

import meshes
import oracle_binding as ob
from goblin_amd import scene as gs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(REPO, "oracle", "_ref", "ref_harness")
needs_harness = pytest.mark.skipif(not os.path.exists(HARNESS), reason="oracle/_ref/ref_harness not built (the reference sources are not here)")


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", meshes.ALL)
def test_restated_tree_is_a_partition_into_small_leaves(name):
    V, F = meshes.mesh(name)
    s = meshes.lbvh_shape(V, F)
    T = len(F)
    assert sorted(int(x) for x in s["order"]) == list(range(T))
    # every triangle in exactly one leaf of 1 .. 4 contiguous sorted triangles
    covered = np.zeros(T, np.int64)
    for first, count in s["leaves"]:
        assert 1 <= count <= 4 and 0 <= first and first + count <= T
        covered[first:first + count] += 1
    assert (covered == 1).all()
    # nodes / depth / leaves are those reachable from the root
    seen_nodes, seen_leaves, depth = 0, [], 0
    level = [0] if s["tree"] else []
    while level:
        depth += 1
        nxt = []
        for n in level:
            seen_nodes += 1
            assert 2 <= len(s["tree"][n]) <= 4
            for c in s["tree"][n]:
                if isinstance(c, tuple):
                    seen_leaves.append(c)
                else:
                    nxt.append(c)
        level = nxt
    assert seen_nodes == s["nodes"] == len(s["tree"]) and depth == s["depth"]
    if T <= 4:
        assert s["nodes"] == 0 and s["depth"] == 0 and s["leaves"] == [(0, T)]
    else:
        assert sorted(seen_leaves) == s["leaves"] and s["nodes"] >= 1 and s["nodes"] <= T - 1
    # a pure function of its input
    again = meshes.lbvh_shape(*meshes.MESHES[name][0]())
    assert again["nodes"] == s["nodes"] and again["depth"] == s["depth"] and again["leaves"] == s["leaves"]
    assert np.array_equal(again["order"], s["order"]) and again["tree"] == s["tree"]


def test_restated_tree_with_single_triangle_leaves():
    """max_leaf is the only knob: single-triangle leaves make a tree over every triangle."""
    V, F = meshes.mesh("few9")
    s = meshes.lbvh_shape(V, F, max_leaf=1)
    assert all(count == 1 for _, count in s["leaves"]) and len(s["leaves"]) == 9


def test_the_meshes_are_what_they_claim_to_be():
    # the deep spiral crosses the 64-entry line of the traversal stacks (3 entries per 4-wide level + TLAS + 2)
    deep = meshes.lbvh_shape(*meshes.mesh(meshes.DEEP))
    assert 3 * deep["depth"] + 2 > 64, deep["depth"]
    assert len(meshes.mesh(meshes.DEEP)[1]) == 2048 and len(meshes.mesh("spiral")[1]) == 400
    # ... with its smallest triangles at the face indices 0, 1, 2, 4, 8, ...
    V, F = meshes.mesh(meshes.DEEP)
    V0, F0 = meshes.spiral(2048, 0.993, 0.3)
    for j, slot in enumerate([0] + [1 << b for b in range(11)]):
        assert np.array_equal(V[F[slot]], V0[F0[2047 - j]])
    assert sorted(map(tuple, V[F].reshape(-1, 9))) == sorted(map(tuple, V0[F0].reshape(-1, 9)))
    # urchin: one Morton code, boxes centred exactly on the origin
    V, F = meshes.mesh("urchin")
    keys, lo, hi = meshes.morton_keys(V, F)
    assert len(F) == 64 and len(set(int(k) >> 32 for k in keys)) == 1
    assert (lo + hi == 0).all() and np.array_equal(V * 32, np.round(V * 32))
    # flatgrid: zero extent on y, 1152 triangles, every key's y bits zero
    V, F = meshes.mesh("flatgrid")
    keys, _, _ = meshes.morton_keys(V, F)
    assert len(F) == 1152 and (V[:, 1] == 0).all() and all((int(k) >> 32) & 0x12492492 == 0 for k in keys)
    # many triangles per Morton cell in the spirals (the bunny never has more than a handful)
    keys, _, _ = meshes.morton_keys(*meshes.mesh(meshes.DEEP))
    assert np.unique(keys >> np.uint64(32), return_counts=True)[1].max() > 100
    # slivers: 2 long, 0.004 wide
    V, F = meshes.mesh("slivers")
    t = V[F].astype(np.float64)
    assert len(F) == 96 and np.allclose(np.linalg.norm(t[:, 1] - t[:, 0], axis=1), 0.004, rtol=1e-3)
    assert np.allclose(np.linalg.norm(t[:, 2] - 0.5 * (t[:, 0] + t[:, 1]), axis=1), 2.0, rtol=1e-3)
    # tiny: the spiral's coordinates x 2^-10, exactly
    assert np.array_equal(meshes.mesh("tiny")[0] * np.float32(1024.0), meshes.mesh("spiral")[0])
    # degenerate: four zero-area triangles after few(8)
    V, F = meshes.mesh("degenerate")
    t = V[F].astype(np.float64)
    area = np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
    assert len(F) == 12 and (area[:8] > 0.1).all() and (area[8:] < 1e-7).all()
    for n in (1, 3, 4, 5, 8, 9):
        assert len(meshes.mesh("few%d" % n)[1]) == n


def test_written_obj_loads_back_bit_for_bit(tmp_path):
    """%.9g round-trips float32 through the scene loader, so the restatement sees the arrays the device is given."""
    names = ["deep_spiral", "tiny", "flatgrid", "degenerate"]
    meshes.write_meshes(tmp_path, names)
    scene = gs.load_scene_text(json.dumps(meshes.scene_doc(names)), str(tmp_path))
    got = meshes.scene_meshes(scene)
    assert len(got) == 1 + len(names)
    for (P, I), name in zip(got[1:], names):
        V, F = meshes.mesh(name)
        assert np.array_equal(P[I], V[F])
        assert meshes.lbvh_shape(P, I)["leaves"] == meshes.lbvh_shape(V, F)["leaves"]


# ---------------------------------------------------------------------------
# oracle against the compiled reference
# ---------------------------------------------------------------------------
def reference_and_oracle(tmp, names, method=None, ao_samples=None):
    meshes.write_meshes(tmp, names)
    doc = meshes.scene_doc(names, method=method, ao_samples=ao_samples)
    ref_doc = json.loads(json.dumps(doc))
    for g in ref_doc["geometries"]:
        g["file"] = os.path.join(str(tmp), g["file"])
    jp = os.path.join(str(tmp), "s.json")
    with open(jp, "w") as f:
        json.dump(ref_doc, f)
    prefix = os.path.join(str(tmp), "o")
    try:
        meta = json.loads(subprocess.check_output([HARNESS, "li", jp, prefix, "1", "100000"], stderr=subprocess.DEVNULL, timeout=300).decode())
    except (OSError, subprocess.SubprocessError) as e:   # a harness built for another machine
        pytest.skip("ref_harness did not run here: %s" % e)
    samples = np.fromfile(prefix + ".samples.f32", np.float32).reshape(-1, meta["dims"])
    li_ref = np.fromfile(prefix + ".li.f32", np.float32).reshape(-1, 4)
    film_ref = np.fromfile(prefix + ".film.f32", np.float32).reshape(meta["yres"], meta["xres"], 4)
    scene = gs.load_scene_text(json.dumps(doc), str(tmp))
    o = ob.Oracle(scene)
    assert o.dims() == meta["dims"] and o.window() == tuple(meta["window"])
    li, _ = o.li_replay(samples, threads=4)
    film = o.render(threads=1)["film"]
    return doc, o, li, li_ref, film, film_ref


def first_hit_instances(doc, o):
    """Instance index of the first hit of the camera ray through every pixel centre (-1: none)."""
    xres, yres = doc["camera"]["film"]["resolution"]
    out = np.full((yres, xres), -1, np.int64)
    for y in range(yres):
        for x in range(xres):
            r = o.camera_ray(x + 0.5, y + 0.5)
            h = o.intersect(r[:3], r[3:6], r[6], -1.0)
            if h is not None:
                out[y, x] = int(h[11])
    return out


@needs_harness
@pytest.mark.parametrize("name", meshes.ALL)
def test_oracle_equals_reference_on_each_mesh(name, tmp_path):
    doc, o, li, li_ref, film, film_ref = reference_and_oracle(tmp_path, [name])
    on_mesh = float((first_hit_instances(doc, o) == 1).mean())
    print(name, "records", len(li), "camera rays on the mesh %.3f" % on_mesh, "li exact", np.array_equal(li, li_ref),
          "film exact", np.array_equal(film, film_ref))
    assert np.isfinite(li).all() and np.isfinite(film).all()
    assert li[:, :3].max() > 0
    np.testing.assert_array_equal(li, li_ref)
    np.testing.assert_array_equal(film, film_ref)
    assert on_mesh >= 0.25, on_mesh   # a mesh out of frame proves nothing


@needs_harness
@pytest.mark.parametrize("method", ["path_tracing", "ao", "whitted"])
def test_oracle_equals_reference_on_all_meshes_together(method, tmp_path):
    doc, o, li, li_ref, film, film_ref = reference_and_oracle(tmp_path, meshes.ALL, method=method, ao_samples=9 if method == "ao" else None)
    inst = first_hit_instances(doc, o)
    per_mesh = [int((inst == 1 + i).sum()) for i in range(len(meshes.ALL))]
    print(method, "records", len(li), "camera rays per mesh", per_mesh, "li exact", np.array_equal(li, li_ref), "film exact", np.array_equal(film, film_ref))
    assert np.isfinite(li).all() and np.isfinite(film).all()
    np.testing.assert_array_equal(li, li_ref)
    np.testing.assert_array_equal(film, film_ref)
    assert min(per_mesh) >= 1 and sum(per_mesh) >= 0.25 * inst.size, per_mesh
