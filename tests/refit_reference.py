"""A numpy restatement of vertex edits (test infrastructure): the plan walk of goblin_amd/csrc/scene_refit.cpp and the two
kernels of goblin_amd/csrc/kernels/refit.h, over the device tables as numpy structured arrays.

Everything is float32 where the kernels are float32 and float64 only where they are double (the quantiser's floor and ceil), so
the restatement's tables must equal the device's BYTE FOR BYTE.  The library is compiled with -ffp-contract=off: a float32
numpy expression rounds after every operation just as the kernels do.
"""
import numpy as np

F32 = np.float32
REF_NONE = 0x7ffffffd

NODE = np.dtype([("o", "<f4", 3), ("scale", "<f4", 3), ("qlo", "<u4", 3), ("qhi", "<u4", 3), ("child", "<i4", 4)])
TRI = np.dtype([("p0", "<f4", 3), ("shade", "<u4"), ("e1", "<f4", 3), ("flags", "<u4"), ("e2", "<f4", 3), ("pad1", "<f4")])
BOUND = np.dtype([("lo", "<f4", 3), ("hi", "<f4", 3), ("pad", "<f4", 2)])
SHADE = np.dtype([("v", "<u4", 3), ("flags", "<u4")])
ORDER = np.dtype([("path", "<u4"), ("axes_lo", "<u4"), ("axes_hi", "<u4"), ("depth_rank", "<u4")])
RECORD = np.dtype([("node", "<i4"), ("level", "<i4"), ("child_plan", "<i4", 4)])
assert (NODE.itemsize, TRI.itemsize, BOUND.itemsize, SHADE.itemsize, ORDER.itemsize, RECORD.itemsize) == (64, 48, 32, 16, 16, 24)


def leaf_range(ref):
    """(first, count) of a leaf reference."""
    bits = (~int(ref)) & 0xffffffff
    return bits >> 2, (bits & 3) + 1


def plan_walk(nodes, root):
    """(records, level_first): the interior nodes reached BY REFERENCE from `root`, breadth first and so sorted by level.
    A root that is a leaf reference gives no record and no level."""
    root = int(root)
    if root < 0:
        return np.zeros(0, RECORD), []
    assert root != REF_NONE and root < len(nodes)
    recs, level_first, seen = [[root, 0, -1, -1, -1, -1]], [0], {root}
    begin, level = 0, 0
    while begin < len(recs):
        end = len(recs)
        for r in range(begin, end):
            child = nodes["child"][recs[r][0]]
            for c in range(4):
                ref = int(child[c])
                if ref == REF_NONE or ref < 0:
                    continue
                assert ref < len(nodes) and ref not in seen, ref
                seen.add(ref)
                recs[r][2 + c] = len(recs)
                recs.append([ref, level + 1, -1, -1, -1, -1])
        level_first.append(end)
        begin, level = end, level + 1
    out = np.zeros(len(recs), RECORD)
    a = np.array(recs, np.int32)
    out["node"], out["level"], out["child_plan"] = a[:, 0], a[:, 1], a[:, 2:]
    return out, level_first


def _min(a, b):
    """std::min(a, b): the first of two equal values (+0 and -0 are equal)."""
    return np.where(b < a, b, a)


def _max(a, b):
    return np.where(a < b, b, a)


def refit_tris(tris, bounds, tri_shade, positions, first, count):
    """refit_tris over records [first, first + count), in place.  positions: float32 [V, 3], every vertex of the scene."""
    k = slice(first, first + count)
    P = np.asarray(positions, F32)[tri_shade["v"][tris["shade"][k]]]      # [count, 3 vertices, 3 axes]
    x0, x1, x2 = P[:, 0], P[:, 1], P[:, 2]
    tris["p0"][k] = x0
    tris["e1"][k] = x1 - x0
    tris["e2"][k] = x2 - x0
    bounds["lo"][k] = _min(_min(x0, x1), x2)
    bounds["hi"][k] = _max(_max(x0, x1), x2)


def _nudge_down(v):
    return ((v - np.abs(v) * F32(4e-7)).astype(F32) - F32(1e-30)).astype(F32)


def _nudge_up(v):
    return ((v + np.abs(v) * F32(4e-7)).astype(F32) + F32(1e-30)).astype(F32)


def refit_level(nodes, bounds, records, node_box_lo, node_box_hi, begin, end):
    """refit_level over plan records [begin, end) -- one level --, in place; node_box_* are float32 [records, 3]."""
    if end <= begin:
        return
    rec = records[begin:end]
    idx = rec["node"]
    ref = nodes["child"][idx].astype(np.int64)                            # [n, 4]
    n = len(rec)
    used = ref != REF_NONE
    leaf = used & (ref < 0)
    inner = used & (ref >= 0)
    lo = np.full((n, 4, 3), np.inf, F32)
    hi = np.full((n, 4, 3), -np.inf, F32)
    bits = (~ref) & 0xffffffff
    first, count = np.where(leaf, bits >> 2, 0), np.where(leaf, (bits & 3) + 1, 0)
    for t in range(4):
        m = leaf & (t < count)
        at = np.where(m, first + t, 0)
        lo = np.where(m[..., None], np.minimum(lo, bounds["lo"][at]), lo)
        hi = np.where(m[..., None], np.maximum(hi, bounds["hi"][at]), hi)
    plan = np.where(inner, rec["child_plan"], 0)
    assert (rec["child_plan"][inner] > np.arange(begin, end)[:, None].repeat(4, 1)[inner]).all()   # children sit behind their parent
    lo = np.where(inner[..., None], node_box_lo[plan], lo)
    hi = np.where(inner[..., None], node_box_hi[plan], hi)
    node_box_lo[begin:end] = lo.min(axis=1)                               # unused slots hold +inf / -inf
    node_box_hi[begin:end] = hi.max(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        cl = np.where(used[..., None], _nudge_down(lo), F32(np.inf)).astype(F32)
        ch = np.where(used[..., None], _nudge_up(hi), F32(-np.inf)).astype(F32)
        o = cl.min(axis=1)                                                # [n, 3]
        top = ch.max(axis=1)
        extent = ((top - o).astype(F32) * F32(1.0001)).astype(F32) + F32(1e-30)
        _, e = np.frexp((extent / F32(255.0)).astype(F32))
        biased = np.minimum(254, np.maximum(1, e.astype(np.int64) + 127))
        step = np.ldexp(F32(1.0), (biased - 127).astype(np.int32)).astype(F32)
        O, S = o[:, None, :], step[:, None, :]
        fl = np.floor((cl.astype(np.float64) - O.astype(np.float64)) / S.astype(np.float64))
        fh = np.ceil((ch.astype(np.float64) - O.astype(np.float64)) / S.astype(np.float64))
        fl = np.where(used[..., None], fl, 0.0)
        fh = np.where(used[..., None], fh, 0.0)

        def at_q(q):   # lo + float(q) * step, in float32
            return (O + (q.astype(F32) * S).astype(F32)).astype(F32)
        while True:
            m = used[..., None] & (fl > 0) & (at_q(fl) > cl)
            if not m.any():
                break
            fl = np.where(m, fl - 1, fl)
        while True:
            m = used[..., None] & (fh < 255) & (at_q(fh) < ch)
            if not m.any():
                break
            fh = np.where(m, fh + 1, fh)
    ql = np.where(used[..., None], np.minimum(255.0, np.maximum(0.0, fl)), 255.0).astype(np.uint32)
    qh = np.where(used[..., None], np.minimum(255.0, np.maximum(0.0, fh)), 0.0).astype(np.uint32)
    shift = (8 * np.arange(4, dtype=np.uint32))[None, :, None]
    nodes["o"][idx] = o
    nodes["scale"][idx] = step
    nodes["qlo"][idx] = np.bitwise_or.reduce(ql << shift, axis=1)
    nodes["qhi"][idx] = np.bitwise_or.reduce(qh << shift, axis=1)


def refit_mesh(nodes, tris, bounds, tri_shade, positions, root, tri_first, tri_count, plan=None):
    """What gbl_update_vertices does to the three tables for one mesh, in place: refit_tris, then refit_level from the deepest
    level to the root.  Returns the plan (records, level_first) it walked (or was given)."""
    records, level_first = plan if plan is not None else plan_walk(nodes, root)
    refit_tris(tris, bounds, tri_shade, positions, tri_first, tri_count)
    box_lo = np.zeros((len(records), 3), F32)
    box_hi = np.zeros((len(records), 3), F32)
    for l in range(len(level_first) - 1, 0, -1):
        refit_level(nodes, bounds, records, box_lo, box_hi, level_first[l - 1], level_first[l])
    return records, level_first


def child_boxes(nodes, idx):
    """[len(idx), 4, 3] float32 lows and highs of the child boxes of nodes idx: o + q * scale, in float32."""
    nd = nodes[idx]
    shift = (8 * np.arange(4, dtype=np.uint32))[None, :, None]
    ql = ((nd["qlo"][:, None, :] >> shift) & 0xff).astype(F32)
    qh = ((nd["qhi"][:, None, :] >> shift) & 0xff).astype(F32)
    o, s = nd["o"][:, None, :], nd["scale"][:, None, :]
    return (o + (ql * s).astype(F32)).astype(F32), (o + (qh * s).astype(F32)).astype(F32)


# ---------------------------------------------------------------------------
# the deformations the tests edit meshes with (tests/meshes.py names; V float32 [n, 3] in any vertex order)
# ---------------------------------------------------------------------------
def jitter(V, radius, seed=7):
    """Every coordinate moved by up to a tenth of the mesh's radius of interest."""
    a = 0.1 * float(radius)
    rng = np.random.default_rng(seed)
    return (np.asarray(V, F32) + rng.uniform(-a, a, np.shape(V)).astype(F32)).astype(F32)


def stretch(V, radius):
    """Scaled by (1, 1.6, 0.7), the odd vertices pushed out by 0.3 radii: the mesh bound leaves its old box."""
    W = (np.asarray(V, F32) * np.array([1.0, 1.6, 0.7], F32)).astype(F32)
    W[1::2] = (W[1::2] + F32(0.3 * float(radius))).astype(F32)
    return W
