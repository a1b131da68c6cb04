"""TEST INFRASTRUCTURE: ctypes face of oracle/liboracle.so (the CPU restatement).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import
this module.  Nothing under goblin_amd/ does.
"""
import ctypes as C
import os
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(REPO, "oracle")
ORACLE_SO = os.path.join(ORACLE_DIR, "liboracle.so")
REF_HARNESS = os.path.join(ORACLE_DIR, "_ref", "ref_harness")


class orc_counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("paths", "closest_queries", "anyhit_queries", "filtered_queries", "nodes",
                                          "tris", "splats", "dims")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


_lib = None


def build_oracle():
    """Compile liboracle.so if it is missing or stale (g++, a few seconds)."""
    src = os.path.join(ORACLE_DIR, "goblin_oracle.cpp")
    hdr = os.path.join(os.path.dirname(ORACLE_DIR), "include", "goblin_hip.h")   # the ABI structs (and version) it is compiled against
    if (not os.path.exists(ORACLE_SO)) or os.path.getmtime(ORACLE_SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "oracle"], stdout=subprocess.DEVNULL)


def lib():
    global _lib
    if _lib is None:
        build_oracle()
        from goblin_amd import _abi
        L = C.CDLL(ORACLE_SO)
        L.orc_create.argtypes = [C.POINTER(_abi.gbl_scene_desc)]
        L.orc_create.restype = C.c_void_p
        L.orc_destroy.argtypes = [C.c_void_p]
        L.orc_destroy.restype = None
        L.orc_sample_window.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.orc_sample_window.restype = None
        L.orc_sample_dimension.argtypes = [C.POINTER(_abi.gbl_render_setting)]
        L.orc_sample_dimension_scene.argtypes = [C.c_void_p, C.POINTER(_abi.gbl_render_setting)]
        L.orc_pt_offsets.argtypes = [C.POINTER(_abi.gbl_render_setting), C.POINTER(C.c_int32)]
        L.orc_pt_offsets.restype = None
        L.orc_glibc_rand.argtypes = [C.POINTER(C.c_int32), C.c_int32]
        L.orc_glibc_rand.restype = None
        L.orc_filter_table.argtypes = [C.c_void_p, C.c_void_p]
        L.orc_filter_table.restype = None
        L.orc_camera_ray.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_void_p]
        L.orc_camera_ray.restype = None
        L.orc_light_power.argtypes = [C.c_void_p, C.c_void_p]
        L.orc_intersect.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p]
        L.orc_first_hit.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]
        L.orc_first_hit.restype = C.c_int32
        L.orc_occluded.argtypes =[C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float]
        L.orc_li_replay.argtypes = [C.c_void_p, C.POINTER(_abi.gbl_render_setting), C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_int32, C.POINTER(orc_counters)]
        L.orc_splat.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        L.orc_native_samples.argtypes = [C.c_void_p, C.POINTER(_abi.gbl_render_setting), C.c_uint64,
                                         C.POINTER(C.c_int32), C.c_void_p]
        L.orc_li_native.argtypes = [C.c_void_p, C.POINTER(_abi.gbl_render_setting), C.c_uint64, C.POINTER(C.c_int32), C.c_int32,
                                    C.c_void_p, C.c_int32]
        L.orc_render.argtypes = [C.c_void_p, C.POINTER(_abi.gbl_render_setting), C.c_int32, C.c_int32, C.c_int32,
                                 C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double),
                                 C.POINTER(orc_counters)]
        L.orc_medium.argtypes = [C.c_void_p, C.POINTER(_abi.gbl_render_setting), C.c_void_p, C.c_int64, C.c_void_p]
        L.orc_medium.restype = C.c_int32
        L.orc_render_medium.argtypes = [C.c_void_p, C.POINTER(_abi.gbl_render_setting), C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
        L.orc_render_medium.restype = C.c_int32
        L.orc_subsurface.argtypes = [C.c_void_p, C.POINTER(_abi.gbl_render_setting), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.orc_subsurface.restype = C.c_int32
        L.orc_sss_offsets.argtypes = [C.c_void_p, C.POINTER(_abi.gbl_render_setting), C.POINTER(C.c_int32)]
        L.orc_sss_offsets.restype = None
        L.orc_surface.argtypes = [C.c_void_p, C.POINTER(_abi.gbl_render_setting), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.orc_surface.restype = C.c_int32
        L.orc_hardware_threads.restype = C.c_int32
        L.orc_mip_lookup.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p]
        L.orc_mip_lookup.restype = C.c_int32
        _lib = L
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Oracle:
    """The CPU restatement bound to one loaded scene (goblin_amd.scene.Scene)."""

    def __init__(self, scene):
        self.scene = scene  # keeps the host arrays alive
        self.h = lib().orc_create(scene.desc_ptr)
        if not self.h:
            raise RuntimeError("orc_create failed")

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            lib().orc_destroy(h)

    # -- facts ---------------------------------------------------------------
    def window(self):
        w = (C.c_int32 * 4)()
        lib().orc_sample_window(self.h, w)
        return tuple(w)

    def dims(self, setting=None):
        return lib().orc_sample_dimension_scene(self.h, C.byref(setting or self.scene.desc.setting))

    def pt_offsets(self, setting=None):
        s = setting or self.scene.desc.setting
        out = (C.c_int32 * (5 * max(1, s.max_ray_depth)))()
        lib().orc_pt_offsets(C.byref(s), out)
        return np.array(out, dtype=np.int32).reshape(-1, 5)

    # -- known-answer probes -------------------------------------------------
    def filter_table(self):
        out = np.zeros(256, np.float32)
        lib().orc_filter_table(self.h, _ptr(out))
        return out

    def camera_ray(self, x, y):
        out = np.zeros(8, np.float32)
        lib().orc_camera_ray(self.h, x, y, _ptr(out))
        return out

    def mip_lookup(self, image, queries, filter, mode, max_aniso=10.0, is_float=False):
        """MIPMap<T>::lookup of the scene's image `image` for n x {s, t, dsdx, dtdx, dsdy, dtdy} -> n x rgba."""
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, 6)
        out = np.zeros((q.shape[0], 4), np.float32)
        if lib().orc_mip_lookup(self.h, image, int(is_float), _ptr(q), q.shape[0], filter, mode, max_aniso, _ptr(out)) != 0:
            raise RuntimeError("orc_mip_lookup failed")
        return out

    def light_power(self):
        out = np.zeros(4 * max(1, self.scene.desc.num_lights), np.float32)
        n = lib().orc_light_power(self.h, _ptr(out))
        return out[:4 * n].reshape(n, 4)

    def intersect(self, o, d, mint=1e-3, maxt=-1.0):
        o = np.asarray(o, np.float32)
        d = np.asarray(d, np.float32)
        out = np.zeros(12, np.float32)
        hit = lib().orc_intersect(self.h, _ptr(o), _ptr(d), mint, maxt, _ptr(out))
        return out if hit else None

    def first_hit(self, samples):
        """The (n, 12) float32 first-hit records (gbl_aov_sample rows) of n camera samples {image_x, image_y, lens_u1, lens_u2, ...}:
        albedo(3), t, normal(3), instance, position(3), hit; words 7 and 11 are integers (view the rows as int32 / uint32)."""
        samples = np.ascontiguousarray(samples, np.float32)
        assert samples.ndim == 2 and samples.shape[1] >= 4, samples.shape
        out = np.zeros((samples.shape[0], 12), np.float32)
        if lib().orc_first_hit(self.h, _ptr(samples), samples.shape[1], samples.shape[0], _ptr(out)) != 0:
            raise RuntimeError("orc_first_hit failed")
        return out

    def occluded(self, o, d, mint=1e-3, maxt=-1.0):
        o = np.asarray(o, np.float32)
        d = np.asarray(d, np.float32)
        return bool(lib().orc_occluded(self.h, _ptr(o), _ptr(d), mint, maxt))

    # -- integrator ----------------------------------------------------------
    def li_replay(self, samples, setting=None, threads=1):
        s = setting or self.scene.desc.setting
        samples = np.ascontiguousarray(samples, np.float32)
        n = samples.shape[0]
        assert samples.shape[1] == self.dims(s), (samples.shape, self.dims(s))
        li = np.zeros((n, 4), np.float32)
        cnt = orc_counters()
        lib().orc_li_replay(self.h, C.byref(s), _ptr(samples), n, _ptr(li), threads, C.byref(cnt))
        return li, cnt.as_dict()

    # the medium probe's flags (word 7 of a record, an integer)
    MEDIUM_CROSSES, MEDIUM_THIN, MEDIUM_CLIPPED, MEDIUM_ENDS_INSIDE, MEDIUM_OCCLUDED, MEDIUM_UNOCCLUDED, MEDIUM_LIGHT0 = 1, 2, 4, 8, 16, 32, 256

    def medium(self, samples, setting=None):
        """The medium's part of li_replay, per record (n, 8): {tr rgb, Lv rgb, number of medium draws, flags} under the hashed draws
        of the replay and native samplers.  li_replay's output is float32(tr * L + Lv) with L the same replay without the medium."""
        s = setting or self.scene.desc.setting
        samples = np.ascontiguousarray(samples, np.float32)
        assert samples.shape[1] == self.dims(s), (samples.shape, self.dims(s))
        out = np.zeros((samples.shape[0], 8), np.float32)
        if lib().orc_medium(self.h, C.byref(s), _ptr(samples), samples.shape[0], _ptr(out)) != 0:
            raise RuntimeError("orc_medium failed (no medium in the scene?)")
        return out

    def render_medium(self, setting=None, sampler=0, seed=0):
        """render(threads=1) with the probe along: dict(film, samples, li, medium) in tile-then-pixel order, where `li` is Li itself
        (what the compiled reference's probes log) and `medium` the probe's records under this render's own draws."""
        s = setting or self.scene.desc.setting
        d = self.scene.desc
        film = np.zeros((d.film.yres, d.film.xres, 4), np.float32)
        w = self.window()
        n = (w[1] - w[0]) * (w[3] - w[2]) * int(np.ceil(np.sqrt(np.float32(s.sample_per_pixel)))) ** 2
        samples, li, medium = np.zeros((n, self.dims(s)), np.float32), np.zeros((n, 4), np.float32), np.zeros((n, 8), np.float32)
        if lib().orc_render_medium(self.h, C.byref(s), sampler, seed, _ptr(film), _ptr(samples), _ptr(li), _ptr(medium)) != 0:
            raise RuntimeError("orc_render_medium failed (no medium in the scene?)")
        return {"film": film, "samples": samples, "li": li, "medium": medium}

    # the subsurface probe's words (columns of a record)
    SSS_SINGLE, SSS_MULTI, SSS_CALLS, SSS_CALLS_DEEP = slice(0, 3), slice(3, 6), 6, 7
    SSS_AXIS_N, SSS_AXIS_U, SSS_AXIS_V, SSS_PROBE_MISS, SSS_PROBE_OTHER, SSS_PROBE_BLACK, SSS_PROBE_OCCLUDED, SSS_PROBE_ACCEPTED = range(8, 16)
    SSS_SINGLE_BLACK, SSS_SINGLE_MISS, SSS_SINGLE_OTHER, SSS_SINGLE_OCCLUDED, SSS_SINGLE_ACCEPTED, SSS_LIGHTS, SSS_NAN, SSS_FIRST_LEVEL = range(16, 24)
    SSS_MI_DIFFERS, SSS_MP_DIFFERS, SSS_MAX_LEVEL, SSS_WORDS = 24, 25, 26, 28

    def sss_offsets(self, setting=None):
        """Where a Sample record keeps its BSSRDF block: dict of the columns of slot 0's {ls_comp, ls_geo, pick_light, pick_axis,
        disc, single} (slot i: + i, or + 2 i for the two 2D patterns ls_geo and disc) and `n`, the number of slots."""
        out = (C.c_int32 * 7)()
        lib().orc_sss_offsets(self.h, C.byref(setting or self.scene.desc.setting), out)
        return dict(zip(("ls_comp", "ls_geo", "pick_light", "pick_axis", "disc", "single", "n"), (int(v) for v in out)))

    def subsurface(self, samples, setting=None):
        """What Lsubsurface did in li_replay, per record (n, 28): {single rgb, multi rgb} of the sample's first evaluation, the number
        of evaluations (and of those at a recursion level > 0), and counters over their slots -- probe axis N / U / V; probe ray
        missed / hit another material / hit the same one with a black light sample, an occluded one, an accepted one; single
        scatter's light sample black, its exit missed / on another material / occluded / accepted; a bit mask of the lights picked;
        1 | 2 for a NaN single | multi term; the first evaluation's level; slots whose single-scatter exit / probe fragment resolved
        other coefficients than the shaded fragment; the deepest evaluation's level.  Returns (records, li) with li what li_replay gives."""
        s = setting or self.scene.desc.setting
        samples = np.ascontiguousarray(samples, np.float32)
        assert samples.shape[1] == self.dims(s), (samples.shape, self.dims(s))
        out, li = np.zeros((samples.shape[0], self.SSS_WORDS), np.float32), np.zeros((samples.shape[0], 4), np.float32)
        if lib().orc_subsurface(self.h, C.byref(s), _ptr(samples), samples.shape[0], _ptr(out), _ptr(li)) != 0:
            raise RuntimeError("orc_subsurface failed")
        return out, li

    # the surface probe's events (a bit of word SURF_FIRST, a counter at SURF_COUNTS + event) and words
    SURF_EVENTS = ("ENTERING", "LEAVING", "TOTAL_REFLECTION", "REFLECT", "REFRACT", "PUNCHED", "BSDF_BLACK", "SAMPLE_BLACK", "SAMPLE_PDF_ZERO",
                   "LIGHT_BLACK", "LIGHT_PDF_ZERO", "OCCLUDED", "UNOCCLUDED", "ATTENUATED", "SPOT_OUTSIDE", "SPOT_FALLOFF", "SPOT_FULL",
                   "EMITTER_BACK", "SPHERE_INSIDE", "END_PICKED", "END_OTHER", "END_SURFACE", "END_ESCAPED", "ENV_ADDED")
    SURF_MATERIAL, SURF_REFLECT_CHANCE, SURF_MASKED_PROB, SURF_LIGHT, SURF_FIRST, SURF_VERTICES, SURF_NAN, SURF_EARLY_ESCAPE, SURF_LATE_ESCAPE, SURF_INSIDE_EPSILON, SURF_COUNTS = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
    SURF_WORDS = SURF_COUNTS + len(SURF_EVENTS)

    def surface(self, samples, setting=None):
        """What the materials, the lights and the integrator did in li_replay, per record (n, 34): the first vertex's material type
        + 1 (+ 16 under a mask; 0 where the camera ray escaped), the first transparent vertex's reflectChance, the first masked
        vertex's maskedProb, the light picked at the first vertex + 1, the first vertex's events as a bit mask (bit i: SURF_EVENTS[i]),
        the number of vertices, 1 for a NaN in li, the number of punched-through paths that escaped where the `firstBounce` rule adds the
        environment and where it adds none, the number of light samples nearer than the fragment's epsilon (a negative shadow maxt), and per event the number of times any vertex noted it.  Returns (records, li)
        with li what li_replay gives."""
        s = setting or self.scene.desc.setting
        samples = np.ascontiguousarray(samples, np.float32)
        assert samples.shape[1] == self.dims(s), (samples.shape, self.dims(s))
        out, li = np.zeros((samples.shape[0], self.SURF_WORDS), np.float32), np.zeros((samples.shape[0], 4), np.float32)
        if lib().orc_surface(self.h, C.byref(s), _ptr(samples), samples.shape[0], _ptr(out), _ptr(li)) != 0:
            raise RuntimeError("orc_surface failed")
        return out, li

    def splat(self, samples, li, film=None):
        d = self.scene.desc
        if film is None:
            film = np.zeros((d.film.yres, d.film.xres, 4), np.float32)
        samples = np.ascontiguousarray(samples, np.float32)
        li = np.ascontiguousarray(li, np.float32)
        lib().orc_splat(self.h, _ptr(samples), samples.shape[1], _ptr(li), samples.shape[0], _ptr(film))
        return film

    def native_samples(self, seed, window=None, setting=None):
        s = setting or self.scene.desc.setting
        w = window or self.window()
        spp = int(np.ceil(np.sqrt(np.float32(s.sample_per_pixel)))) ** 2
        n = (w[1] - w[0]) * (w[3] - w[2]) * spp
        out = np.zeros((n, self.dims(s)), np.float32)
        lib().orc_native_samples(self.h, C.byref(s), seed, (C.c_int32 * 4)(*w), _ptr(out))
        return out

    def li_native(self, seed, rr=False, window=None, setting=None, threads=4):
        """Li of the native sampler's records for a window, pixel-major (the device's li order); rr: with the device's Russian
        roulette extension restated (same counter-based kill draw, same 1 / q placement)."""
        s = setting or self.scene.desc.setting
        w = window or self.window()
        spp = int(np.ceil(np.sqrt(np.float32(s.sample_per_pixel)))) ** 2
        li = np.zeros(((w[1] - w[0]) * (w[3] - w[2]) * spp, 4), np.float32)
        lib().orc_li_native(self.h, C.byref(s), seed, (C.c_int32 * 4)(*w), 1 if rr else 0, _ptr(li), threads)
        return li

    def render(self, setting=None, threads=1, ref_faithful=0, sampler=0, seed=0, want_samples=False):
        """The reference's whole render loop.  Returns dict(film, seconds, counters[, samples, li])."""
        s = setting or self.scene.desc.setting
        d = self.scene.desc
        film = np.zeros((d.film.yres, d.film.xres, 4), np.float32)
        w = self.window()
        spp = int(np.ceil(np.sqrt(np.float32(s.sample_per_pixel)))) ** 2
        n = (w[1] - w[0]) * (w[3] - w[2]) * spp
        samples = np.zeros((n, self.dims(s)), np.float32) if want_samples else None
        li = np.zeros((n, 4), np.float32) if want_samples else None
        sec = C.c_double()
        cnt = orc_counters()
        lib().orc_render(self.h, C.byref(s), threads, ref_faithful, sampler, seed, _ptr(film), _ptr(samples), _ptr(li),
                         C.byref(sec), C.byref(cnt))
        out = {"film": film, "seconds": sec.value, "counters": cnt.as_dict()}
        if want_samples:
            out["samples"] = samples
            out["li"] = li
        return out


def hardware_threads():
    return lib().orc_hardware_threads()


def normalize_film(film):
    """Film::writeImage's rgb/weight (GoblinFilm.cpp:164-172); weight-0 pixels -> 0."""
    w = film[..., 3:4]
    with np.errstate(divide="ignore", invalid="ignore"):
        rgb = film[..., :3] * (np.float32(1.0) / w)
    return np.where(w > 0, rgb, 0).astype(np.float32)
