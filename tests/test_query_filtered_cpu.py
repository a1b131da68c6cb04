"""gbl_trace_rays_filtered without a GPU: the ABI's new names, and the inputs and the restatement of the device suite.

1. gbl_trace_rays_filtered, gbl_selftest_query_filtered, gbl_ray_transmittance and the filter / kind constants are declared in the
   header, mirrored in goblin_amd/_abi.py and exported by libgoblin_hip.so; a compiled C snippet prints the size and constants.
2. query_filtered_cases.chain -- evalAttenuation restated over the oracle -- against products written out here in float32, column
   by column of the pane stack.
3. What the populations cover, asserted on chain's output: every count from 0 to 4, Black by alpha 1, by an occluder and by the
   subsurface material, both texels of the 2 x 1 image, segments clipped between panes, and closest-hit populations under either
   filter that hit on at least a quarter of their rays.
4. The oracle's `nearest` lookup inside one texel's span stays within the tolerance the device suite gives the image alphas.
5. No ray of the pane stack or of masked.json meets two instances at exactly the same t (each instance intersected alone by the
   oracle): the device suite's sub-scene comparison decides every ray.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import query_filtered_cases as fc
from goblin_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "goblin_hip.h")
F32 = np.float32
NAMES = ("gbl_trace_rays_filtered", "gbl_selftest_query_filtered")


def test_the_new_names_are_declared_mirrored_and_exported():
    text = open(HEADER).read()
    for name in NAMES:
        assert "gbl_status %s(" % name in text, name
        assert name in _abi.HIP_SYMBOLS, name
    assert "} gbl_ray_transmittance;" in text
    assert C.sizeof(_abi.gbl_ray_transmittance) == 16
    assert [n for n, _ in _abi.gbl_ray_transmittance._fields_] == ["tr", "crossed"] and _abi.gbl_ray_transmittance.crossed.offset == 12
    assert (_abi.GBL_QUERY_FILTER_NONE, _abi.GBL_QUERY_FILTER_OPAQUE, _abi.GBL_QUERY_FILTER_MASK, _abi.GBL_QUERY_TRANSMITTANCE) == (0, 1, 2, 2)
    assert _abi.GBL_ABI_VERSION == 14
    lib = os.path.join(_abi.LIB_DIR, "libgoblin_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert " T %s\n" % name in exported, name


def test_a_c_program_sees_the_record_and_constants(tmp_path):
    src = tmp_path / "q.c"
    # (the two prototypes again: a redeclaration that did not match the header's would not compile)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "goblin_hip.h"\n'
                   'gbl_status gbl_trace_rays_filtered(gbl_ctx*, uint32_t, uint32_t, const gbl_ray*, uint64_t, void*, uint32_t, void*);\n'
                   'gbl_status gbl_selftest_query_filtered(gbl_ctx*, uint32_t, uint32_t, const gbl_ray*, uint64_t, void*, uint32_t, uint32_t);\n'
                   'int main(void) {\n'
                   '  printf("%zu %zu %u %u %u %u %d\\n", sizeof(gbl_ray_transmittance), offsetof(gbl_ray_transmittance, crossed),\n'
                   '         GBL_QUERY_FILTER_NONE, GBL_QUERY_FILTER_OPAQUE, GBL_QUERY_FILTER_MASK, GBL_QUERY_TRANSMITTANCE, GBL_ABI_VERSION);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "q"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["16", "12", "0", "1", "2", "2", "14"], out


@pytest.fixture(scope="module")
def pane():
    case = fc.pane_stack()
    rays, column, variant = fc.pane_rays()
    tr, crossed, met, _ = fc.chains(case, rays)
    return dict(case=case, rays=rays, column=column, variant=variant, tr=tr, crossed=crossed, met=met)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_the_restatement_equals_products_written_out_by_hand(pane):
    one = F32(1.0)
    f0 = [F32(F32(one - F32(0.25)) * F32(c)) for c in (1.0, 1.0, 1.0)]      # P0: alpha 0.25, white
    f1 = [F32(F32(one - F32(0.5)) * F32(c)) for c in (1.0, 0.75, 0.3)]      # P1: alpha 0.5, (1, 0.75, 0.3)
    f2 = [F32(F32(one - F32(0.0)) * F32(c)) for c in (0.9, 0.8, 0.7)]       # P2: alpha 0
    f3 = [F32(F32(one - F32(1.0)) * F32(c)) for c in (1.0, 1.0, 1.0)]       # P3: alpha 1

    def product(*fs):
        thr = [one, one, one]
        for f in fs:
            thr = [F32(thr[k] * f[k]) for k in range(3)]
        return np.array(thr, F32)
    want = {0: (product(), 0), 1: (product(f0), 1), 2: (product(f0, f1), 2), 3: (product(f0, f1, f2), 3), 4: (product(f0, f1, f2, f3), 4)}
    assert not want[4][0].any() and want[3][0].all()
    for name in ("short_of_wall", "scaled_3", "scaled_quarter"):
        for c in range(5):
            k = np.flatnonzero((pane["column"] == c) & (pane["variant"] == name))
            assert len(k) == len(fc.LATTICE)
            assert (bits(pane["tr"][k]) == bits(want[c][0])[None, :]).all(), (name, c, pane["tr"][k[0]], want[c][0])
            assert (pane["crossed"][k] == want[c][1]).all(), (name, c)
    # back to front from between P3 and the wall: the same surfaces in the other order; P3 first where it stands
    back = {0: (product(), 0), 1: (product(f0), 1), 2: (product(f1, f0), 2), 3: (product(f2, f1, f0), 3), 4: (product(f3), 1)}
    for c in range(5):
        k = np.flatnonzero((pane["column"] == c) & (pane["variant"] == "reversed_inside"))
        assert (bits(pane["tr"][k]) == bits(back[c][0])[None, :]).all() and (pane["crossed"][k] == back[c][1]).all(), c
    # the extras: a sphere crossed twice, a disk, the 1 x 1 image, the 2 x 1 image's two texels, the subsurface quad
    ball = [F32(F32(one - F32(0.5)) * F32(c)) for c in (0.5, 1.0, 0.25)]
    plate = [F32(F32(one - F32(0.75)) * F32(c)) for c in (1.0, 1.0, 1.0)]
    img1 = [F32(F32(one - F32(7.0 / 32.0)) * F32(c)) for c in (1.0, 1.0, 1.0)]
    img2 = [[F32(F32(one - F32(a)) * F32(c)) for c in (1.0, 0.5, 0.25)] for a in (7.0 / 32.0, 25.0 / 32.0)]
    extras = {5: [(product(ball, ball), 2)], 6: [(product(plate), 1)], 7: [(product(img1), 1)], 8: [(product(f), 1) for f in img2],
              9: [(np.zeros(3, F32), 0)]}
    for c, options in extras.items():
        k = np.flatnonzero((pane["column"] == c) & (pane["variant"] == "short_of_wall"))
        seen = set()
        for i in k:
            match = [j for j, (tr, n) in enumerate(options) if np.array_equal(bits(pane["tr"][i]), bits(tr)) and pane["crossed"][i] == n]
            assert match, (c, pane["tr"][i], pane["crossed"][i])
            seen.add(match[0])
        assert seen == set(range(len(options))), (c, seen)   # (both texels of the 2 x 1 image occur)
    assert fc.TEXEL_1X1 == 7.0 / 32.0 and fc.TEXELS_2X1 == (7.0 / 32.0, 25.0 / 32.0)


def test_what_the_populations_cover(pane):
    tr, crossed, column, variant, case = pane["tr"], pane["crossed"], pane["column"], pane["variant"], pane["case"]
    black = ~tr.any(axis=1)
    assert set(range(5)) <= set(int(c) for c in crossed[crossed < fc.OCCLUDED_BIT])
    assert (black & (crossed == 4)).any()                                   # Black by alpha 1, the count stopping there
    assert (black & (crossed == fc.OCCLUDED_BIT)).any()                     # Black by an occluder
    assert (black & (crossed == 0) & (column == 9)).any()                   # Black by the subsurface material: no factor counted
    assert not (black & (crossed == 0) & (column != 9)).any()
    full = crossed[(column == 4) & (variant == "short_of_wall")]
    assert (crossed[(column == 4) & (variant == "maxt_between")] < full).all()   # clipped between panes: fewer surfaces
    assert (crossed[(column == 4) & (variant == "mint_between")] < full).all()
    invalid = column == -1
    assert invalid.sum() == len(fc.qc.INVALID_RAYS) and (tr[invalid] == 1.0).all() and not crossed[invalid].any()
    for side in ("opaque", "mask"):
        ref = fc.sub_answers(case, side, pane["rays"])
        hits = int((ref["instance"] >= 0).sum())
        print(side, "closest-hit rays that hit:", hits, "of", len(pane["rays"]))
        assert 4 * hits >= len(pane["rays"]), side
    masked = fc.masked()
    rays = fc.masked_rays(masked)
    for side in ("opaque", "mask"):
        ref = fc.sub_answers(masked, side, rays)
        hits = int((ref["instance"] >= 0).sum())
        print("masked.json", side, "closest-hit rays that hit:", hits, "of", len(rays))
        assert 4 * hits >= len(rays), side


@pytest.mark.parametrize("name", ["pane_stack", "masked"])
def test_no_ray_meets_two_instances_at_the_same_t(name):
    case = fc.pane_stack() if name == "pane_stack" else fc.masked()
    rays = fc.pane_rays()[0] if name == "pane_stack" else fc.masked_rays(case)
    t = fc.first_hits_alone(fc.alone(name), rays)
    for side in ("opaque", "mask"):
        mine = t[:, case.to_full[side]]
        ordered = np.sort(mine, axis=1)                                    # (NaN, a miss, sorts last)
        tied = (ordered[:, 1:] == ordered[:, :-1]).any(axis=1)
        assert not tied.any(), (name, side, np.flatnonzero(tied)[:8])
        # ... and the sub-scene's own closest hit is the nearest of them
        ref = fc.sub_answers(case, side, rays)
        with np.errstate(invalid="ignore"):
            nearest = np.where(np.isnan(mine).all(axis=1), F32(-1.0), np.nanmin(np.where(np.isnan(mine), np.inf, mine), axis=1)).astype(F32)
        assert np.array_equal(bits(nearest), bits(ref["t"])), (name, side)


def test_a_nearest_lookup_inside_one_texels_span_stays_within_the_image_tolerance():
    """The bound the device suite gives the two image alphas (query_filtered_cases.IMAGE_TOLERANCE: |alpha - v| <= 9 x 2^-24 x v of
    its 11), on the oracle's MIPMap::lookup: `nearest` under `clamp`, 20 000 uniform (s, t) per texel span."""
    import oracle_binding as ob
    oracle = ob.Oracle(fc.pane_stack().full)
    rng = np.random.default_rng(7102)
    spans = [(0, 0.02, 0.98, fc.TEXEL_1X1), (1, 0.02, 0.25, fc.TEXELS_2X1[0]), (1, 0.75, 0.98, fc.TEXELS_2X1[1])]
    for image, lo, hi, v in spans:
        q = np.zeros((20000, 6), F32)
        q[:, 0], q[:, 1] = rng.uniform(lo, hi, len(q)), rng.uniform(0.02, 0.98, len(q))
        alpha = oracle.mip_lookup(image, q, _abi.GBL_IMAGE_FILTER_NONE, _abi.GBL_ADDRESS_CLAMP, is_float=True)[:, 0].astype(np.float64)
        worst = np.abs(alpha - v).max() / (2.0 ** -24 * v)
        print("image", image, "texel", v, "not exact:", int((alpha != v).sum()), "of", len(q), "largest |alpha - v| / (2^-24 v): %.2f" % worst)
        assert worst <= 9.0
    # at the 2 x 1 image's quarter points the taps straddle both texels: one ulp of u moves alpha by more than the bound
    q = np.zeros((2, 6), F32)
    q[:, 0], q[:, 1] = [np.nextafter(F32(0.75), F32(0)), 0.75], 0.5
    at = oracle.mip_lookup(1, q, _abi.GBL_IMAGE_FILTER_NONE, _abi.GBL_ADDRESS_CLAMP, is_float=True)[:, 0]
    assert at[1] == F32(fc.TEXELS_2X1[1]) and at[0] != at[1]
