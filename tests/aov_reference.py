"""TEST INFRASTRUCTURE: what gbl_render_aov must produce, from the oracle binding alone.

native_samples -> first_hit gives the per-sample records, the albedo (the oracle's lookup of the material's first colour slot)
included; splat(samples, values) the three films.  expected_albedo is the same colour from the scene description alone, where
that slot is a constant.  Computed once per (scene, shape) and shared read-only by tests/test_aov_cpu.py, tests/test_gpu_aov.py
and tests/test_gpu_texture_chart.py.
"""
import functools

import numpy as np

from goblin_amd import _abi
from goblin_amd import scene as gs
import oracle_binding as ob

SEED = 7
SHAPE = dict(resolution=(16, 16), spp=4, depth=2)   # a 20x20 sample window: 3x3 tiles of 8x8, the last row and column partial


class Reference:
    """Per-sample first-hit records of the native sampler's camera samples, li order (pixel-major over the window): the rows of
    Oracle.first_hit.  oracle_albedo is the oracle's lookup of the first colour slot, known at every hit; albedo / albedo_known
    are what the scene description alone says (expected_albedo)."""

    def __init__(self, scene, seed=SEED, window=None, oracle=None):
        self.scene = scene
        self.oracle = oracle or ob.Oracle(scene)
        self.window = tuple(window or self.oracle.window())
        self.samples = self.oracle.native_samples(seed, window=self.window)
        self.n = self.samples.shape[0]
        self.records = self.oracle.first_hit(self.samples)
        ints = self.records.view(np.int32)
        self.rows = ints
        self.oracle_albedo, self.t, self.normal, self.position = self.records[:, 0:3], self.records[:, 3], self.records[:, 4:7], self.records[:, 8:11]
        self.instance, self.hit = ints[:, 7], ints[:, 11].view(np.uint32)
        self.albedo, self.albedo_known = expected_albedo(scene.desc, self.instance)
        for a in (self.samples, self.records, self.albedo, self.albedo_known):
            a.setflags(write=False)

    @functools.cached_property
    def rays(self):
        """(o, d) of the camera rays, by the per-sample probe (pinhole and orthographic cameras: orc_camera_ray draws no lens sample)."""
        o, d = np.zeros((self.n, 3), np.float32), np.zeros((self.n, 3), np.float32)
        for i in range(self.n):
            ray = self.oracle.camera_ray(float(self.samples[i, 0]), float(self.samples[i, 1]))
            o[i], d[i] = ray[0:3], ray[3:6]
        return o, d

    o = property(lambda self: self.rays[0])
    d = property(lambda self: self.rays[1])

    def emitter_hits(self):
        inst = self.scene.desc.instances
        return np.array([i >= 0 and inst[i].area_light >= 0 for i in self.instance])

    def depth_values(self):
        h = self.hit.astype(np.float32)
        return np.stack([np.where(self.hit == 1, self.t, np.float32(0.0)) * h, h, np.zeros_like(h), np.zeros_like(h)], axis=1).astype(np.float32)

    def films(self):
        """The three accumulators the oracle's splat makes of the records."""
        pad = np.zeros((self.n, 1), np.float32)
        return {"albedo": self.oracle.splat(self.samples, np.concatenate([self.oracle_albedo, pad], axis=1)),
                "normal": self.oracle.splat(self.samples, np.concatenate([self.normal, pad], axis=1)),
                "depth": self.oracle.splat(self.samples, self.depth_values())}


def loop_records(oracle, samples):
    """The records one probe call at a time (camera_ray + intersect per sample; no lens sample, so pinhole and orthographic cameras):
    what Reference did before Oracle.first_hit, kept to pin first_hit's geometry to the probes the other tests use."""
    n = samples.shape[0]
    hit, t, instance = np.zeros(n, np.uint32), np.full(n, -1.0, np.float32), np.full(n, -1, np.int32)
    position, normal = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    for i in range(n):
        ray = oracle.camera_ray(float(samples[i, 0]), float(samples[i, 1]))
        h = oracle.intersect(ray[0:3], ray[3:6], mint=float(ray[6]))
        if h is not None:
            hit[i], t[i], position[i], normal[i], instance[i] = 1, h[0], h[2:5], h[5:8], int(h[11])
    return hit, t, instance, position, normal


def albedo_slot(desc, material):
    """(colour, tex) of the material's first colour slot: Kd / Kg / Kr in color, a subsurface material's Kr in color3, a mask's
    wrapped material's."""
    m = desc.materials[material]
    if m.type == _abi.GBL_MAT_MASK:
        m = desc.materials[m.masked_material]
    if m.type == _abi.GBL_MAT_SUBSURFACE:
        return np.array(m.color3[:], np.float32), m.tex_color3
    return np.array(m.color[:], np.float32), m.tex_color


def expected_albedo(desc, instance):
    """Per sample: the slot's constant (zeros for a miss) and whether it is known, i.e. a miss or a constant slot."""
    albedo = np.zeros((len(instance), 3), np.float32)
    known = np.ones(len(instance), bool)
    slots = {}
    for i, inst in enumerate(instance):
        if inst < 0:
            continue
        if inst not in slots:
            slots[inst] = albedo_slot(desc, desc.instances[inst].material)
        color, tex = slots[inst]
        if tex == -1:
            albedo[i] = color
        else:
            known[i] = False
    return albedo, known


def depth_and_coverage(accum):
    """depth = x / y and coverage = y / w of a depth accumulator in float32, 0 where the denominator is 0."""
    x, y, w = accum[..., 0], accum[..., 1], accum[..., 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.where(y != 0, x / y, np.float32(0.0)).astype(np.float32)
        coverage = np.where(w != 0, y / w, np.float32(0.0)).astype(np.float32)
    return depth, coverage


@functools.lru_cache(maxsize=None)
def scene(name, resolution=SHAPE["resolution"], spp=SHAPE["spp"], depth=SHAPE["depth"]):
    return gs.load_scene(name, gs.config_overrides(resolution=resolution, spp=spp, depth=depth))


@functools.lru_cache(maxsize=None)
def reference(name, resolution=SHAPE["resolution"], spp=SHAPE["spp"], depth=SHAPE["depth"]):
    return Reference(scene(name, resolution, spp, depth))
