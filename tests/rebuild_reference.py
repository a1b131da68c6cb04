"""A numpy restatement of gbl_mesh_tree_stats (test infrastructure): goblin_amd/csrc/kernels/treestats.h over the node table as
a numpy structured array, built on refit_reference's plan walk and child boxes.

A slot's corners are float32 (o + float(q) * scale, as traversal forms them), its area is dx * dy + dy * dz + dz * dx in double
with the differences formed in double; the library is compiled with -ffp-contract=off, so every TERM here has the device's bits.
The sums are math.fsum's -- exact to the last bit --, so the whole distance between a device sum and the restatement's is the
device's own: at most N * 2^-52 relative for N non-negative terms added in any order.  `terms` carries the two N.

`same_tree` compares two trees up to where their nodes are stored: lbvh_collapse numbers nodes through an atomic counter, so two
builds of one tree differ in node indices and in nothing else.
"""
import math

import numpy as np

import refit_reference as rr

F64 = np.float64


def _area(lo, hi):
    d = hi.astype(F64) - lo.astype(F64)
    return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]


def tree_stats(nodes, root):
    """What gbl_mesh_tree_stats reports for the tree below `root`: nodes, levels, leaves, root_area, node_area, tri_area; and
    `terms` = (interior slots, leaf slots), `leaf_ranges` = [(first, count)] of every leaf slot (the root's own if it is a leaf)."""
    records, level_first = rr.plan_walk(nodes, root)
    if len(records) == 0:
        return {"nodes": 0, "levels": 0, "leaves": 1, "root_area": 0.0, "node_area": 0.0, "tri_area": 0.0, "terms": (0, 0),
                "leaf_ranges": [rr.leaf_range(root)]}
    idx = records["node"]
    lo, hi = rr.child_boxes(nodes, idx)                       # [n, 4, 3] float32
    ref = nodes["child"][idx].astype(np.int64)
    used = ref != rr.REF_NONE
    leaf, inner = used & (ref < 0), used & (ref >= 0)
    area = _area(lo, hi)                                      # [n, 4]
    count = (((~ref) & 3) + 1).astype(F64)
    u = used[0]
    root_area = float(_area(lo[0][u].min(axis=0), hi[0][u].max(axis=0))) if u.any() else 0.0
    bits = (~ref[leaf]) & 0xffffffff
    return {"nodes": len(records), "levels": len(level_first) - 1, "leaves": int(leaf.sum()), "root_area": root_area,
            "node_area": math.fsum(area[inner]), "tri_area": math.fsum((count * area)[leaf]),
            "terms": (int(inner.sum()), int(leaf.sum())), "leaf_ranges": [(int(b >> 2), int(b & 3) + 1) for b in bits]}


def costs(stats):
    """(node_cost, tri_cost) as HipPathTracer.tree_stats adds them."""
    a = stats["root_area"]
    return (1.0 + stats["node_area"] / a, stats["tri_area"] / a) if a > 0 else (0.0, 0.0)


def same_tree(nodes_a, root_a, nodes_b, root_b):
    """The two trees are equal slot by slot up to node numbering: o, scale, qlo, qhi, leaf references, and which slots are
    interior, recursively.  Returns the number of nodes compared."""
    stack, seen = [(int(root_a), int(root_b))], 0
    while stack:
        a, b = stack.pop()
        if a < 0 or b < 0 or a == rr.REF_NONE or b == rr.REF_NONE:
            assert a == b, ("leaf or empty slot", a, b)
            continue
        na, nb = nodes_a[a], nodes_b[b]
        for f in ("o", "scale", "qlo", "qhi"):
            assert na[f].tobytes() == nb[f].tobytes(), (f, a, b, na[f], nb[f])
        seen += 1
        stack += [(int(x), int(y)) for x, y in zip(na["child"], nb["child"])]
    return seen
