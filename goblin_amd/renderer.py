"""HipPathTracer: the Python face of the device integrator.

Mirrors the shape of the reference's ``Renderer`` (/root/reference/src/
GoblinRenderer.h:53-60): construct from the render settings, ``render(scene)``
fills the Film.  All computation happens in libgoblin_hip.so through the C ABI
(include/goblin_hip.h); PyTorch only supplies device memory and streams.  There
is no CPU fallback: without the HIP library or a GPU this raises.
"""
import ctypes as C

import numpy as np

from . import _abi


def _torch():
    import torch
    return torch


class Film:
    """Accumulators {sum w*L.rgb, sum w} as a (yres, xres, 4) float32 CUDA tensor
    (the reference's Pixel array, GoblinFilm.h:16-23)."""

    def __init__(self, xres, yres, device):
        torch = _torch()
        self.xres, self.yres = xres, yres
        self.accum = torch.zeros((yres, xres, 4), dtype=torch.float32, device=device)

    def zero_(self):
        self.accum.zero_()

    def normalized(self):
        """Film::writeImage's rgb / weight (GoblinFilm.cpp:164-172) as a tensor."""
        torch = _torch()
        w = self.accum[..., 3:4]
        rgb = self.accum[..., :3] * (1.0 / w)
        return torch.where(w > 0, rgb, torch.zeros_like(rgb))

    def numpy(self):
        return self.accum.detach().cpu().numpy()


class HipPathTracer:
    """Device path tracer / AO renderer bound to one scene on one GPU."""

    def __init__(self, scene, device=0, bvh="host"):
        """bvh: "host" (binned SAH, the default) or "device" (Morton-sorted linear BVH built on the GPU)."""
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError("HipPathTracer needs a HIP device: torch.cuda.is_available() is False and there is no "
                               "CPU fallback on the product path")
        self.lib = _abi.hip_lib()
        self.scene = scene
        self.device_index = device if isinstance(device, int) else torch.device(device).index or 0
        self.device = torch.device("cuda", self.device_index)
        handle = C.c_void_p()
        if bvh not in ("host", "device"):
            raise ValueError("bvh must be 'host' or 'device'")
        if bvh == "device":
            st = self.lib.gbl_create_ex(scene.desc_ptr, self.device_index, _abi.GBL_CREATE_DEVICE_BVH, C.byref(handle))
        else:
            st = self.lib.gbl_create(scene.desc_ptr, self.device_index, C.byref(handle))
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(None).decode())
        self.handle = handle
        info = _abi.gbl_info()
        self.lib.gbl_get_info(self.handle, C.byref(info))
        self.info = info
        self.window = tuple(info.window)

    def _device_transforms(self, t):
        """The data pointer of ``t``, a contiguous float32 (n, 10) tensor on the tracer's device (its storage offset included);
        ValueError for anything else.  An empty tensor has no pointer of its own and borrows one."""
        torch = _torch()
        if t.dtype != torch.float32 or t.device != self.device or t.dim() != 2 or t.shape[1] != 10 or not t.is_contiguous():
            raise ValueError("transforms must be a contiguous float32 (n, 10) tensor on %s, got %s %s on %s%s" %
                             (self.device, t.dtype, tuple(t.shape), t.device, "" if t.is_contiguous() else ", not contiguous"))
        if t.shape[0] == 0:
            self._one_transform = getattr(self, "_one_transform", None)
            if self._one_transform is None:
                self._one_transform = torch.zeros((1, 10), dtype=torch.float32, device=self.device)
            return self._one_transform.data_ptr()
        return t.data_ptr()

    def update_instances(self, first, transforms, device_tlas=False):
        """Move instances first.. to new (position, orientation wxyz, scale) transforms and rebuild the TLAS in place.

        A contiguous float32 (n, 10) torch tensor on the tracer's device -- columns position, orientation wxyz, scale, which is
        gbl_trs' layout -- is read where it lies (gbl_update_instances_device; a slice with a storage offset is fine); any
        other tensor is a ValueError.  ``device_tlas``: build the TLAS on the device too (GBL_INSTANCES_DEVICE_TLAS: faster
        to build for many instances, slower to trace); a list is uploaded to a tensor first then."""
        if hasattr(transforms, "data_ptr") or device_tlas:
            torch = _torch()
            if not hasattr(transforms, "data_ptr"):
                rows = np.array([list(pos) + list(quat) + list(scale) for pos, quat, scale in transforms], np.float32).reshape(-1, 10)
                transforms = torch.from_numpy(rows).to(self.device)
            ptr = self._device_transforms(transforms)
            st = self.lib.gbl_update_instances_device(self.handle, int(first), transforms.shape[0], ptr,
                                                      _abi.GBL_INSTANCES_DEVICE_TLAS if device_tlas else 0)
            if st != _abi.GBL_OK:
                raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
            self.lib.gbl_get_info(self.handle, C.byref(self.info))
            return
        arr = (_abi.gbl_trs * len(transforms))()
        for i, (pos, quat, scale) in enumerate(transforms):
            arr[i].position[:] = pos
            arr[i].orientation[:] = quat
            arr[i].scale[:] = scale
        st = self.lib.gbl_update_instances(self.handle, first, len(transforms), arr)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        self.lib.gbl_get_info(self.handle, C.byref(self.info))

    def instances(self, device=False):
        """The transforms the context holds now (gbl_get_instances): a list of (position, orientation wxyz, scale) tuples, one per
        instance -- the scene's at first, the edited ones after ``update_instances``.  What ``motion`` takes as ``prev_instances``.
        ``device=True``: an (n, 10) float32 tensor on the tracer's device, copied device to device (gbl_get_instances_device)."""
        n = int(self.info.instances)
        if device:
            torch = _torch()
            out = torch.empty((max(n, 1), 10), dtype=torch.float32, device=self.device)
            st = self.lib.gbl_get_instances_device(self.handle, 0, n, out.data_ptr())
            if st != _abi.GBL_OK:
                raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
            return out[:n]
        arr = (_abi.gbl_trs * max(n, 1))()
        st = self.lib.gbl_get_instances(self.handle, 0, n, arr)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, "gbl_get_instances")
        return [(tuple(arr[i].position), tuple(arr[i].orientation), tuple(arr[i].scale)) for i in range(n)]

    def _device_vertices(self, what, t, shape=None):
        """The data pointer of ``t``, a contiguous float32 (n, 3) tensor on the tracer's device (its storage offset included);
        ValueError for anything else.  An empty tensor has no pointer of its own and borrows one."""
        torch = _torch()
        if t.dtype != torch.float32 or t.device != self.device or t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float32 (n, 3) tensor on %s, got %s %s on %s%s" %
                             (what, self.device, t.dtype, tuple(t.shape), t.device, "" if t.is_contiguous() else ", not contiguous"))
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError("%s must have shape %s, got %s" % (what, tuple(shape), tuple(t.shape)))
        if t.shape[0] == 0:
            self._one_vertex = getattr(self, "_one_vertex", None)
            if self._one_vertex is None:
                self._one_vertex = torch.zeros((1, 3), dtype=torch.float32, device=self.device)
            return self._one_vertex.data_ptr()
        return t.data_ptr()

    def update_vertices(self, mesh, positions, normals=None, first=0, defer_order=False):
        """Give vertices first.. of triangle mesh ``mesh`` (its index in the scene's meshes) new object-space positions -- an (n, 3)
        float32 array -- and, with ``normals``, new vertex normals; the mesh's BLAS is refitted on the device in place
        (gbl_update_vertices).  The topology stays; without ``normals`` the vertex normals stay as they were.

        A contiguous float32 (n, 3) torch tensor on the tracer's device is read where it lies (gbl_update_vertices_device; a
        slice with a storage offset is fine); any other tensor is a ValueError.  ``defer_order``: leave the mesh's tie order --
        7.6 ms on the host for the bunny, read only by exact_ties, replay, stream, instrumented and Whitted renders and by
        scenes beyond the headline feature set -- to the first call that needs it (``order_pending``); arrays are uploaded to
        a tensor first then."""
        is_tensor = [hasattr(x, "data_ptr") for x in (positions, normals) if x is not None]
        if any(is_tensor) or defer_order:
            torch = _torch()
            if any(is_tensor) and not all(is_tensor):
                raise ValueError("positions and normals must both be tensors or both be arrays")
            if not is_tensor[0]:
                pos = np.ascontiguousarray(positions, np.float32)
                if pos.ndim != 2 or pos.shape[1] != 3:
                    raise ValueError("positions must have shape (n, 3), got %s" % (pos.shape,))
                positions = torch.from_numpy(pos).to(self.device)
                if normals is not None:
                    normals = torch.from_numpy(np.ascontiguousarray(normals, np.float32)).to(self.device)
            p_ptr = self._device_vertices("positions", positions)
            n_ptr = self._device_vertices("normals", normals, positions.shape) if normals is not None else None
            st = self.lib.gbl_update_vertices_device(self.handle, int(mesh), int(first), positions.shape[0], p_ptr, n_ptr,
                                                     _abi.GBL_VERTICES_DEFER_ORDER if defer_order else 0)
            if st != _abi.GBL_OK:
                raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
            self.lib.gbl_get_info(self.handle, C.byref(self.info))
            return
        pos = np.ascontiguousarray(positions, np.float32)
        if pos.ndim != 2 or pos.shape[1] != 3:
            raise ValueError("positions must have shape (n, 3), got %s" % (pos.shape,))
        nrm = None
        if normals is not None:
            nrm = np.ascontiguousarray(normals, np.float32)
            if nrm.shape != pos.shape:
                raise ValueError("normals must have the positions' shape %s, got %s" % (pos.shape, nrm.shape))
        st = self.lib.gbl_update_vertices(self.handle, int(mesh), int(first), pos.shape[0], pos.ctypes.data, nrm.ctypes.data if nrm is not None else None)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        self.lib.gbl_get_info(self.handle, C.byref(self.info))

    def vertices(self, mesh, device=False):
        """The positions the context holds now for triangle mesh ``mesh`` (gbl_get_vertices): (vertex_count, 3) float32 -- the
        scene's at first, the edited ones after ``update_vertices``.  ``device=True``: a tensor on the tracer's device, copied
        device to device (gbl_get_vertices_device) -- what ``motion`` takes as ``prev_vertices`` without a trip to the host."""
        n = int(self.scene.desc.meshes[int(mesh)].vertex_count) if 0 <= int(mesh) < self.scene.desc.num_meshes else 0
        if device:
            torch = _torch()
            out = torch.empty((max(n, 1), 3), dtype=torch.float32, device=self.device)
            st = self.lib.gbl_get_vertices_device(self.handle, int(mesh), 0, n, out.data_ptr())
            if st != _abi.GBL_OK:
                raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
            return out[:n]
        out = np.empty((n, 3), np.float32)
        st = self.lib.gbl_get_vertices(self.handle, int(mesh), 0, n, out.ctypes.data)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, "gbl_get_vertices")
        return out

    def order_pending(self, mesh):
        """1 while the tie order of ``mesh`` waits for its first reader after ``update_vertices(..., defer_order=True)``, else 0
        (gbl_order_pending)."""
        pending = C.c_uint32()
        st = self.lib.gbl_order_pending(self.handle, int(mesh), C.byref(pending))
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, "gbl_order_pending")
        return int(pending.value)

    def rebuild_mesh(self, mesh):
        """Build the BLAS of triangle mesh ``mesh`` again on the device, in place, over the positions the context holds now
        (gbl_rebuild_mesh): afterwards the mesh's triangles, bounds and tree are what a ``bvh="device"`` tracer of the deformed
        scene holds, whichever builder made this one.  For a pose that is rendered many times after a large deformation
        (``tree_stats`` tells when); a deferred tie order stays deferred."""
        st = self.lib.gbl_rebuild_mesh(self.handle, int(mesh), 0)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        self.lib.gbl_get_info(self.handle, C.byref(self.info))

    def tree_stats(self, mesh):
        """Size and expected traversal cost of the BLAS of triangle mesh ``mesh`` as it is now (gbl_mesh_tree_stats): a dict of
        nodes, levels, leaves; root_area, node_area, tri_area (sums over the quantised child boxes); and the two ratios
        node_cost = 1 + node_area / root_area -- the expected number of nodes a ray that enters the root visits -- and
        tri_cost = tri_area / root_area, the expected number of triangles it tests (both 0.0 when root_area is 0)."""
        ts = _abi.gbl_tree_stats()
        st = self.lib.gbl_mesh_tree_stats(self.handle, int(mesh), C.byref(ts))
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        out = {name: getattr(ts, name) for name in ("nodes", "levels", "leaves", "root_area", "node_area", "tri_area")}
        out["node_cost"] = 1.0 + ts.node_area / ts.root_area if ts.root_area > 0 else 0.0
        out["tri_cost"] = ts.tri_area / ts.root_area if ts.root_area > 0 else 0.0
        return out

    _GEOMETRY = (np.dtype([("o", "<f4", 3), ("scale", "<f4", 3), ("qlo", "<u4", 3), ("qhi", "<u4", 3), ("child", "<i4", 4)]),
                 np.dtype([("p0", "<f4", 3), ("shade", "<u4"), ("e1", "<f4", 3), ("flags", "<u4"), ("e2", "<f4", 3), ("pad1", "<f4")]),
                 np.dtype([("lo", "<f4", 3), ("hi", "<f4", 3), ("pad", "<f4", 2)]),
                 np.dtype([("path", "<u4"), ("axes_lo", "<u4"), ("axes_hi", "<u4"), ("depth_rank", "<u4")]), np.dtype("<i4"))

    def _geometry(self, table):
        """A device geometry table read back (gbl_selftest_geometry) as a numpy structured array: 0 or "nodes", 1 or "tris",
        2 or "tri_bounds", 3 or "tri_order"; 4 or "mesh_root": the BLAS root reference per mesh, as int32.  For tests."""
        t = {"nodes": 0, "tris": 1, "tri_bounds": 2, "tri_order": 3, "mesh_root": 4}.get(table, table)
        total = C.c_uint64()
        st = self.lib.gbl_selftest_geometry(self.handle, t, 0, 0, None, C.byref(total))
        if st == _abi.GBL_OK:
            out = np.zeros(total.value, self._GEOMETRY[t])
            st = self.lib.gbl_selftest_geometry(self.handle, t, 0, total.value, out.ctypes.data, None)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        return out

    _INSTANCE = np.dtype([("m", "<f4", 12), ("inv", "<f4", 12), ("root", "<i4"), ("material", "<i4"), ("area_light", "<i4"), ("mesh", "<i4"),
                          ("shape", "<u4"), ("radius", "<f4"), ("is_mask", "<u4"), ("pad", "<i4")])
    _INSTANCE_BOUND = np.dtype([("lo", "<f4", 3), ("hi", "<f4", 3)])

    def _instances_raw(self, first=0, count=None):
        """The device's instance records and instance bounds of [first, first + count) read back (gbl_selftest_instances) as
        numpy structured arrays, with the TLAS root and the traversal stack entries the context holds now: a dict of records,
        bounds, total, tlas_root, stack_entries.  For tests."""
        total, root, entries = C.c_uint64(), C.c_int32(), C.c_int32()
        st = self.lib.gbl_selftest_instances(self.handle, 0, 0, None, None, C.byref(total), C.byref(root), C.byref(entries))
        if st == _abi.GBL_OK:
            count = total.value - first if count is None else count
            records, bounds = np.zeros(max(count, 0), self._INSTANCE), np.zeros(max(count, 0), self._INSTANCE_BOUND)
            st = self.lib.gbl_selftest_instances(self.handle, first, count, records.ctypes.data, bounds.ctypes.data, None, None, None)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        return {"records": records, "bounds": bounds, "total": total.value, "tlas_root": root.value, "stack_entries": entries.value}

    def camera(self):
        """The camera description last set (gbl_get_camera): a gbl_camera, the scene's at first."""
        cam = _abi.gbl_camera()
        st = self.lib.gbl_get_camera(self.handle, C.byref(cam))
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        return cam

    def update_camera(self, position=None, orientation=None, **fields):
        """Give the context a new camera (gbl_update_camera): position (3), orientation (w, x, y, z) and any other gbl_camera
        field by name (fov_degrees, lens_radius, focal_distance, type, film_width, ...); what is not given keeps its value.
        Host work only: nothing is rebuilt or uploaded, and renders already queued keep the camera they were launched with."""
        cam = self.camera()
        if position is not None:
            cam.position[:] = [float(v) for v in position]
        if orientation is not None:
            cam.orientation[:] = [float(v) for v in orientation]
        names = {name for name, _ in _abi.gbl_camera._fields_} - {"position", "orientation"}
        for name, value in fields.items():
            if name not in names:
                raise TypeError("gbl_camera has no field %r" % name)
            setattr(cam, name, value)
        st = self.lib.gbl_update_camera(self.handle, C.byref(cam))
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())

    _LIGHT = np.dtype([("type", "<u4"), ("color", "<f4", 3), ("pos", "<f4", 3), ("cos_max", "<f4"), ("axis", "<f4", 3), ("cos_falloff", "<f4"),
                       ("m", "<f4", 12), ("inv", "<f4", 12), ("tri_first", "<u4"), ("tri_count", "<u4"), ("sum_area", "<f4"), ("shape", "<u4"),
                       ("radius", "<f4"), ("wh_n", "<u4"), ("wh_prefix", "<u4"), ("image", "<i4"), ("dist_offset", "<u4"), ("dist_w", "<u4"),
                       ("dist_h", "<u4"), ("pad", "<f4")])

    def lights(self):
        """The light records the context holds now (gbl_get_lights): a list of gbl_light, the scene's at first, the edited ones
        after ``update_lights``."""
        n = int(self.scene.desc.num_lights)
        arr = (_abi.gbl_light * max(n, 1))()
        st = self.lib.gbl_get_lights(self.handle, 0, n, arr)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, "gbl_get_lights")
        return [arr[i] for i in range(n)]

    def update_lights(self, first, lights=None, stream=None, **fields):
        """Edit lights (gbl_update_lights).  ``lights``: gbl_light records for lights first..; without it, light ``first`` takes
        the named gbl_light fields -- color, position, direction (3 floats each), cos_theta_max, cos_falloff_start, to_world (a
        (position, orientation wxyz, scale) tuple or a gbl_trs) -- and what is not given keeps its value.  type, mesh, sample_num
        and image cannot change.  Queued on ``stream`` (a torch stream; the current one by default) without a synchronisation,
        unless an area light moves: its instances move with it, which synchronises the device as ``update_instances`` does."""
        torch = _torch()
        if lights is None:
            light = self.lights()[first] if fields else None
            names = {name for name, _ in _abi.gbl_light._fields_}
            for name, value in fields.items():
                if name not in names:
                    raise TypeError("gbl_light has no field %r" % name)
                if name == "to_world" and not isinstance(value, _abi.gbl_trs):
                    for part, values in zip(("position", "orientation", "scale"), value):
                        getattr(light.to_world, part)[:] = [float(v) for v in values]
                elif isinstance(getattr(light, name), C.Array):
                    getattr(light, name)[:] = [float(v) for v in value]
                else:
                    setattr(light, name, value)
            lights = [light] if fields else []
        arr = (_abi.gbl_light * max(len(lights), 1))(*lights)
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        st = self.lib.gbl_update_lights(self.handle, int(first), len(lights), arr, s.cuda_stream)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        self.lib.gbl_get_info(self.handle, C.byref(self.info))   # (a moved area light rebuilds the TLAS)

    def _lights_raw(self):
        """The device's light records, light_cdf and light_pick_pdf read back (gbl_selftest_lights): a dict of records (a numpy
        structured array), cdf, pick_pdf and total.  For tests."""
        total = C.c_uint64()
        st = self.lib.gbl_selftest_lights(self.handle, None, None, None, C.byref(total))
        if st == _abi.GBL_OK:
            n = total.value
            records, cdf, pick = np.zeros(n, self._LIGHT), np.zeros(n + 1, np.float32), np.zeros(max(n, 1), np.float32)
            st = self.lib.gbl_selftest_lights(self.handle, records.ctypes.data, cdf.ctypes.data, pick.ctypes.data, None)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        return {"records": records, "cdf": cdf, "pick_pdf": pick, "total": n}

    _MATERIAL = np.dtype([("type", "<u4"), ("color", "<f4", 3), ("color2", "<f4", 3), ("index", "<f4"), ("k", "<f4"), ("exponent", "<f4"),
                          ("tex_color", "<i4"), ("tex_color2", "<i4"), ("tex_exponent", "<i4"), ("has_tex", "<u4"), ("masked", "<i4"),
                          ("color3", "<f4", 3), ("tex_color3", "<i4"), ("tex_bump", "<i4"), ("tex_normal", "<i4"), ("pad", "<f4")])
    _TEXTURE = np.dtype([("type", "<u4"), ("is_float", "<u4"), ("value", "<f4", 3), ("child", "<i4", 2), ("mapping", "<u4"), ("filter", "<u4"),
                         ("uv_scale", "<f4", 2), ("uv_offset", "<f4", 2), ("to_tex", "<f4", 12), ("image", "<i4"), ("address", "<u4"),
                         ("max_aniso", "<f4"), ("pad", "<f4", 2)])
    MATERIAL_ROW = 12   # floats of a device row: color[3], color2[3], color3[3], index, k, exponent
    TEXTURE_ROW = 7     # value[3], uv_scale[2], uv_offset[2]

    def _get_records(self, name, record, n):
        arr = (record * max(n, 1))()
        st = getattr(self.lib, name)(self.handle, 0, n, arr)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode() or name)
        return [arr[i] for i in range(n)]

    def materials(self):
        """The material records the context holds now (gbl_get_materials): a list of gbl_material, the scene's at first, the
        edited ones after ``update_materials``.  The first call after an edit from a tensor downloads what that edit wrote."""
        return self._get_records("gbl_get_materials", _abi.gbl_material, int(self.scene.desc.num_materials))

    def textures(self):
        """The texture records the context holds now (gbl_get_textures), as ``materials``."""
        return self._get_records("gbl_get_textures", _abi.gbl_texture, int(self.scene.desc.num_textures))

    def _update_records(self, what, first, records, stream, fields, record, row, total, current, host_fn, device_fn):
        torch = _torch()
        first = int(first)
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if isinstance(records, torch.Tensor):
            if fields:
                raise TypeError("%s: give a tensor of rows or keyword fields, not both" % what)
            t = records
            if t.dtype != torch.float32 or t.device != self.device or t.dim() != 2 or t.shape[1] != row or not t.is_contiguous():
                raise ValueError("%s rows must be a contiguous float32 (n, %d) tensor on %s, got %s %s on %s%s" %
                                 (what, row, self.device, t.dtype, tuple(t.shape), t.device, "" if t.is_contiguous() else ", not contiguous"))
            if first < 0 or first + t.shape[0] > total:
                raise ValueError("%s %d .. %d out of range: the scene holds %d" % (what, first, first + t.shape[0], total))
            if t.shape[0] == 0:
                return
            st = getattr(self.lib, device_fn)(self.handle, first, t.shape[0], t.data_ptr(), s.cuda_stream)
        else:
            if records is not None and fields:
                raise TypeError("%s: give records or keyword fields, not both" % what)
            if records is None:
                names = {name for name, _ in record._fields_}
                for name in fields:
                    if name not in names:
                        raise TypeError("%s has no field %r" % (record.__name__, name))
                if not 0 <= first < total and fields:
                    raise ValueError("%s %d out of range: the scene holds %d" % (what, first, total))
                rec = current()[first] if fields else None
                for name, value in fields.items():
                    if name == "to_tex" and not isinstance(value, _abi.gbl_trs):
                        for part, values in zip(("position", "orientation", "scale"), value):
                            getattr(rec.to_tex, part)[:] = [float(v) for v in values]
                    elif isinstance(getattr(rec, name), C.Array):
                        getattr(rec, name)[:] = [float(v) for v in value]
                    else:
                        setattr(rec, name, value)
                records = [rec] if fields else []
            records = list(records)
            for r in records:
                if not isinstance(r, record):
                    raise TypeError("%s records must be %s, got %s" % (what, record.__name__, type(r).__name__))
            if first < 0 or first + len(records) > total:
                raise ValueError("%s %d .. %d out of range: the scene holds %d" % (what, first, first + len(records), total))
            arr = (record * max(len(records), 1))(*records)
            st = getattr(self.lib, host_fn)(self.handle, first, len(records), arr, s.cuda_stream)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())

    def update_materials(self, first, materials=None, stream=None, **fields):
        """Edit materials (gbl_update_materials).  ``materials``: gbl_material records for materials first..; without it, material
        ``first`` takes the named gbl_material fields -- color, color2, color3 (3 floats each), index, k, exponent, and the texture
        index of an occupied slot -- and what is not given keeps its value.  type, masked_material and whether a slot is occupied
        cannot change.  A contiguous float32 (n, 12) torch tensor on the tracer's device -- rows of color, color2, color3, index,
        k, exponent -- is read where it lies by a kernel (gbl_update_materials_device; a slice with a storage offset is fine,
        and its values are not inspected); any other tensor is a ValueError.  Queued on ``stream`` (a torch stream; the current
        one by default) without a synchronisation."""
        self._update_records("material", first, materials, stream, fields, _abi.gbl_material, self.MATERIAL_ROW, int(self.scene.desc.num_materials),
                             self.materials, "gbl_update_materials", "gbl_update_materials_device")

    def update_textures(self, first, textures=None, stream=None, **fields):
        """Edit nodes of the texture graph (gbl_update_textures).  ``textures``: gbl_texture records for textures first..; without
        it, texture ``first`` takes the named fields -- value (3 floats), uv_scale, uv_offset (2 each), to_tex (a (position,
        orientation wxyz, scale) tuple or a gbl_trs), max_anisotropy.  Every other field cannot change.  A contiguous float32
        (n, 7) torch tensor on the tracer's device -- rows of value, uv_scale, uv_offset -- takes the device form
        (gbl_update_textures_device), as in ``update_materials``."""
        self._update_records("texture", first, textures, stream, fields, _abi.gbl_texture, self.TEXTURE_ROW, int(self.scene.desc.num_textures),
                             self.textures, "gbl_update_textures", "gbl_update_textures_device")

    def _materials_raw(self):
        """The device's material and texture records read back (gbl_selftest_materials): a dict of two numpy structured arrays.
        For tests."""
        nm, nt = C.c_uint64(), C.c_uint64()
        st = self.lib.gbl_selftest_materials(self.handle, None, None, C.byref(nm), C.byref(nt))
        if st == _abi.GBL_OK:
            materials, textures = np.zeros(nm.value, self._MATERIAL), np.zeros(nt.value, self._TEXTURE)
            st = self.lib.gbl_selftest_materials(self.handle, materials.ctypes.data, textures.ctypes.data, None, None)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        return {"materials": materials, "textures": textures}

    def _image_record(self, image):
        d = self.scene.desc
        if not 0 <= int(image) < d.num_images:
            raise ValueError("image %r out of range: the scene holds %d" % (image, d.num_images))
        return d.images[int(image)]

    def update_image(self, image, texels, stream=None):
        """Give image ``image`` (its index in the scene's images) a new level 0 and build the MIP levels above it on the device
        (gbl_update_image_device / gbl_update_image).  ``texels``: (height, width, channels) float32 in the layout the context
        holds -- already converted, sides powers of two, 4 channels for a colour image; (height, width) also for a float image.

        A contiguous float32 torch tensor on the tracer's device is read where it lies; a numpy array goes through the host
        form; anything else is a ValueError.  Queued on ``stream`` (a torch stream; the current one by default) without a
        synchronisation.  Width, height and channels cannot change, and an image an image based light reads is refused:
        ``update_environment`` is the edit for it."""
        im = self._image_record(image)
        shapes = [(im.height, im.width, im.channels)] + ([(im.height, im.width)] if im.channels == 1 else [])
        torch = _torch()
        if isinstance(texels, torch.Tensor):
            if texels.dtype != torch.float32 or texels.device != self.device or not texels.is_contiguous():
                raise ValueError("texels must be a contiguous float32 tensor on %s, got %s on %s%s" %
                                 (self.device, texels.dtype, texels.device, "" if texels.is_contiguous() else ", not contiguous"))
            on_device, keep = True, texels
        elif isinstance(texels, np.ndarray):
            on_device, keep = False, np.ascontiguousarray(texels, np.float32)
        else:
            raise ValueError("texels must be a torch tensor on %s or a numpy array, got %s" % (self.device, type(texels).__name__))
        if tuple(keep.shape) not in shapes:
            raise ValueError("texels of image %d must have shape %s, got %s" % (image, " or ".join(map(str, shapes)), tuple(keep.shape)))
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if on_device:
            st = self.lib.gbl_update_image_device(self.handle, int(image), keep.data_ptr(), s.cuda_stream)
        else:
            st = self.lib.gbl_update_image(self.handle, int(image), keep.ctypes.data, s.cuda_stream)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())

    def _environment_light(self, light):
        d = self.scene.desc
        if not 0 <= int(light) < d.num_lights:
            raise ValueError("light %r out of range: the scene holds %d" % (light, d.num_lights))
        if d.lights[int(light)].type != _abi.GBL_LIGHT_IBL:
            raise ValueError("light %d is not an image based light (type %d)" % (light, d.lights[int(light)].type))
        return d.lights[int(light)]

    def update_environment(self, light, texels, stream=None):
        """Give the image of image based light ``light`` (its index in the scene's lights) a new level 0 and make again, on the
        device, all that the context derives from it: the image's MIP pyramid, the light's sampling distribution, its power and
        the pick distribution over the lights (gbl_update_environment_device / gbl_update_environment).  ``texels``: (height,
        width, 4) float32 in the layout the context holds -- sides powers of two, the light's filter colour multiplied in.

        A contiguous float32 torch tensor on the tracer's device is read where it lies; a numpy array goes through the host
        form; anything else is a ValueError.  Queued on ``stream`` (a torch stream; the current one by default) without a
        synchronisation; the next ``update_lights`` waits until the edit has run, for the light's new power."""
        im = self._image_record(self._environment_light(light).image)
        shape = (im.height, im.width, 4)
        torch = _torch()
        if isinstance(texels, torch.Tensor):
            if texels.dtype != torch.float32 or texels.device != self.device or not texels.is_contiguous():
                raise ValueError("texels must be a contiguous float32 tensor on %s, got %s on %s%s" %
                                 (self.device, texels.dtype, texels.device, "" if texels.is_contiguous() else ", not contiguous"))
            on_device, keep = True, texels
        elif isinstance(texels, np.ndarray):
            if texels.dtype != np.float32:
                raise ValueError("texels must be float32, got %s" % texels.dtype)
            on_device, keep = False, np.ascontiguousarray(texels)
        else:
            raise ValueError("texels must be a torch tensor on %s or a numpy array, got %s" % (self.device, type(texels).__name__))
        if tuple(keep.shape) != shape:
            raise ValueError("texels of light %d must have shape %s, got %s" % (light, shape, tuple(keep.shape)))
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if on_device:
            st = self.lib.gbl_update_environment_device(self.handle, int(light), keep.data_ptr(), s.cuda_stream)
        else:
            st = self.lib.gbl_update_environment(self.handle, int(light), keep.ctypes.data, s.cuda_stream)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())

    def _environment_raw(self, light):
        """The light's block of the device's distribution table read back (gbl_selftest_environment): a dict of dist (flat
        float32: the marginal block, then the rows'), level, dist_w and dist_h.  For tests."""
        floats, dims = C.c_uint64(), (C.c_uint32 * 3)()
        st = self.lib.gbl_selftest_environment(self.handle, int(light), None, C.byref(floats), C.byref(dims))
        if st == _abi.GBL_OK:
            dist = np.zeros(floats.value, np.float32)
            st = self.lib.gbl_selftest_environment(self.handle, int(light), dist.ctypes.data, None, None)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        return {"dist": dist, "level": int(dims[0]), "dist_w": int(dims[1]), "dist_h": int(dims[2])}

    def image(self, image):
        """The image as the context holds it now (gbl_get_image): its gbl_image record (texel_offset 0) and one
        (height_l, width_l, channels) float32 array per level, level 0 first.  Synchronises the device."""
        im = self._image_record(image)
        sizes = [(max(1, im.height >> l), max(1, im.width >> l), im.channels) for l in range(im.levels)]
        pool = np.empty(sum(h * w * c for h, w, c in sizes), np.float32)
        record = _abi.gbl_image()
        st = self.lib.gbl_get_image(self.handle, int(image), C.byref(record), pool.ctypes.data)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        levels, at = [], 0
        for h, w, c in sizes:
            levels.append(pool[at:at + h * w * c].reshape(h, w, c))
            at += h * w * c
        return record, levels

    _QUERY_KINDS = {"closest": _abi.GBL_QUERY_CLOSEST, "any": _abi.GBL_QUERY_ANY, "transmittance": _abi.GBL_QUERY_TRANSMITTANCE}
    _QUERY_FILTERS = {"none": _abi.GBL_QUERY_FILTER_NONE, "opaque": _abi.GBL_QUERY_FILTER_OPAQUE, "mask": _abi.GBL_QUERY_FILTER_MASK}

    def _query_flags(self, kind, exact_ties, normals, filter="none"):
        if kind not in self._QUERY_KINDS:
            raise ValueError("kind must be 'closest', 'any' or 'transmittance', got %r" % (kind,))
        if filter not in self._QUERY_FILTERS:
            raise ValueError("filter must be 'none', 'opaque' or 'mask', got %r" % (filter,))
        if normals and kind != "closest":
            raise ValueError("normals need kind='closest': an any-hit or a transmittance query has no hit to shade")
        if kind == "transmittance" and filter != "none":
            raise ValueError("kind='transmittance' takes filter='none': it filters by itself")
        return (self._QUERY_KINDS[kind],
                (_abi.GBL_QUERY_EXACT_TIES if exact_ties else 0) | (_abi.GBL_QUERY_SHADING_NORMAL if normals else 0))

    def trace(self, rays, kind="closest", exact_ties=False, normals=False, out=None, stream=None, _max_workgroups=None, filter="none"):
        """Scene queries for a batch of rays (gbl_trace_rays, gbl_trace_rays_filtered) against the scene as edited so far.

        ``rays``: a contiguous float32 (n, 8) tensor on the tracer's device -- columns origin, mint, direction, maxt, which is
        gbl_ray's layout -- read where it lies.  The direction need not be normalised; t is in its units.

        kind="closest": a dict of views over one (n, 8) float32 output tensor (``out``, or a new one; the dict's "records"):
        t (-1: miss), b1, b2, instance (int32, -1: miss), primitive (int32: the triangle's number within its mesh), normal
        ((n, 3): the world-space shading normal with ``normals``, zeros without).  kind="any": an (n,) uint8 tensor, 1 occluded.
        ``filter``: "opaque" leaves out every instance whose material is a mask, as the integrator's shadow rays do; "mask"
        keeps only those.  kind="transmittance": what the path tracer multiplies a light sample by along the segment -- a dict
        over one (n, 4) float32 tensor ("records"): tr ((n, 3) view), crossed (int32: the mask surfaces multiplied in),
        occluded (bool: an opaque surface blocks the segment; tr is then zero).
        ``exact_ties``: the reference's answer bit for bit.  Queued on ``stream`` (a torch stream; the current one by
        default); does not synchronise.  With the defaults of ``filter`` and a kind other than "transmittance" the call is
        gbl_trace_rays."""
        torch = _torch()
        k, flags = self._query_flags(kind, exact_ties, normals, filter)
        filtered = kind == "transmittance" or filter != "none"
        if rays.dtype != torch.float32 or rays.device != self.device or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_contiguous():
            raise ValueError("rays must be a contiguous float32 (n, 8) tensor on %s, got %s %s on %s%s" %
                             (self.device, rays.dtype, tuple(rays.shape), rays.device, "" if rays.is_contiguous() else ", not contiguous"))
        n = rays.shape[0]
        want = {"any": (n,), "closest": (n, 8), "transmittance": (n, 4)}[kind]
        dtype = torch.uint8 if kind == "any" else torch.float32
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if out is None:
            with torch.cuda.stream(s):   # (the caching allocator ties the block to the stream that uses it)
                out = torch.empty(want, dtype=dtype, device=self.device)
        elif out.dtype != dtype or out.device != self.device or tuple(out.shape) != want or not out.is_contiguous():
            raise ValueError("out must be a contiguous %s %s tensor on %s" % (dtype, want, self.device))
        if n > 0:
            if filtered:
                f = self._QUERY_FILTERS[filter]
                if _max_workgroups is None:
                    st = self.lib.gbl_trace_rays_filtered(self.handle, k, f, rays.data_ptr(), n, out.data_ptr(), flags, s.cuda_stream)
                else:
                    st = self.lib.gbl_selftest_query_filtered(self.handle, k, f, rays.data_ptr(), n, out.data_ptr(), flags, int(_max_workgroups))
            elif _max_workgroups is None:
                st = self.lib.gbl_trace_rays(self.handle, k, rays.data_ptr(), n, out.data_ptr(), flags, s.cuda_stream)
            else:
                st = self.lib.gbl_selftest_query(self.handle, k, rays.data_ptr(), n, out.data_ptr(), flags, int(_max_workgroups))
            if st != _abi.GBL_OK:
                raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        if kind == "any":
            return out
        ints = out.view(torch.int32)
        if kind == "transmittance":
            with torch.cuda.stream(s):   # (the two derived tensors are made behind the query, on its stream)
                return {"records": out, "tr": out[:, 0:3], "crossed": ints[:, 3] & 0x7fffffff, "occluded": ints[:, 3] < 0}
        return {"records": out, "t": out[:, 0], "b1": out[:, 1], "b2": out[:, 2], "instance": ints[:, 3], "primitive": ints[:, 4],
                "normal": out[:, 5:8]}

    def radiance(self, rays, depth=None, seed=0, samples_per_group=1, first_group=0, records=None, exact_ties=False, rr=False,
                 out=None, stream=None, _max_workgroups=None):
        """Path-traced radiance along a batch of rays (gbl_radiance_rays) against the scene as edited so far: PathTracer::Li.

        ``rays``: as ``trace`` takes them, a contiguous float32 (n, 8) tensor on the tracer's device, but the direction MUST be a
        unit vector.  Returns an (n, 4) float32 tensor (``out``, or a new one): {r, g, b, 1} per ray, {0, 0, 0, 0} for an invalid
        ray; a NaN component is stored as it is.  ``depth``: the path tracer's max_ray_depth (None: the scene's; 1 = emission and
        environment only).
        Native draws: ray i is sample i % samples_per_group of group first_group + i // samples_per_group -- a group is to this
        call what a pixel is to ``render``, its samples stratified against each other (a probe is a group of directions, a
        lightmap texel a group of positions); ``seed``, ``rr`` and ``exact_ties`` are ``render``'s.  ``records``: a contiguous
        float32 (n, dims) tensor on the device of replay records in ``render``'s layout at this depth instead (their first
        four floats are not read).  Queued on ``stream`` (a torch stream; the current one by default); does not synchronise.
        The mean of a group: ``out.view(-1, samples_per_group, 4).mean(1)``."""
        torch = _torch()
        if rays.dtype != torch.float32 or rays.device != self.device or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_contiguous():
            raise ValueError("rays must be a contiguous float32 (n, 8) tensor on %s, got %s %s on %s%s" %
                             (self.device, rays.dtype, tuple(rays.shape), rays.device, "" if rays.is_contiguous() else ", not contiguous"))
        n = rays.shape[0]
        p = _abi.gbl_radiance_params()
        p.max_ray_depth = self.scene.desc.setting.max_ray_depth if depth is None else int(depth)
        p.samples_per_group = int(samples_per_group)
        p.first_group = int(first_group)
        p.flags = (_abi.GBL_RADIANCE_EXACT_TIES if exact_ties else 0) | (_abi.GBL_RADIANCE_RUSSIAN_ROULETTE if rr else 0)
        p.seed = int(seed)
        if records is not None:
            if records.dtype != torch.float32 or records.device != self.device or records.dim() != 2 or records.shape[0] != n or not records.is_contiguous():
                raise ValueError("records must be a contiguous float32 (%d, dims) tensor on %s" % (n, self.device))
            p.d_records = records.data_ptr()
            p.record_stride = records.shape[1]
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        p.stream = s.cuda_stream
        if out is None:
            with torch.cuda.stream(s):   # (the caching allocator ties the block to the stream that uses it)
                out = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or out.device != self.device or tuple(out.shape) != (n, 4) or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 (%d, 4) tensor on %s" % (n, self.device))
        if _max_workgroups is None:
            st = self.lib.gbl_radiance_rays(self.handle, rays.data_ptr(), n, C.byref(p), out.data_ptr())
        else:
            st = self.lib.gbl_selftest_radiance(self.handle, rays.data_ptr(), n, C.byref(p), out.data_ptr(), int(_max_workgroups))
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        return out

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            try:
                self.lib.gbl_destroy(h)
            except Exception:
                pass

    def timings(self, n=1):
        """Device times (ms) of the last n render() calls, most recent first: list of (main_kernel_ms, total_ms)."""
        buf = (_abi.gbl_timing * n)()
        got = self.lib.gbl_get_timings(self.handle, n, buf)
        return [(buf[i].main_kernel_ms, buf[i].total_ms) for i in range(got)]

    def valu_issue(self, op, waves_per_simd, iters=4096):
        """gbl_selftest_valu_issue: {ms, wave_instructions, ticks_per_wave, ticks_per_instruction, realtime_ticks_per_wave, clock_ghz}
        of one launch made after two seconds of the same launch back to back."""
        out = (C.c_double * 8)()
        st = self.lib.gbl_selftest_valu_issue(self.handle, int(op), int(waves_per_simd), int(iters), out)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        return {"ms": out[0], "wave_instructions": out[1], "ticks_per_wave": out[2], "ticks_per_instruction": out[3],
                "realtime_ticks_per_wave": out[4], "clock_ghz": out[5],
                "longest_span_us": out[6] * 0.01, "shortest_span_us": out[7] * 0.01}

    def new_film(self):
        return Film(self.info.xres, self.info.yres, self.device)

    def develop(self, film, bloom_radius=None, bloom_weight=None, tone_mapping=None, want_rgb8=False):
        """Film::writeImage's tail on the device (gbl_film_develop): normalise, bloom, tone map and, with want_rgb8, the
        .ppm writer's 8-bit quantisation, on the current stream.  ``film`` is a Film or its (yres, xres, 4) accumulator
        tensor; None for a setting means the scene's ``film`` block.
        Returns {"rgb": (yres, xres, 3) float32 tensor, "rgb8": (yres, xres, 3) uint8 tensor or None}."""
        torch = _torch()
        accum = film.accum if isinstance(film, Film) else film
        h, w = self.info.yres, self.info.xres
        if tuple(accum.shape) != (h, w, 4) or accum.dtype != torch.float32 or accum.device != self.device or not accum.is_contiguous():
            raise ValueError("film must be a contiguous (%d, %d, 4) float32 tensor on %s" % (h, w, self.device))
        f = self.scene.desc.film
        p = _abi.gbl_develop_params()
        p.bloom_radius = f.bloom_radius if bloom_radius is None else float(bloom_radius)
        p.bloom_weight = f.bloom_weight if bloom_weight is None else float(bloom_weight)
        p.tone_mapping = f.tone_mapping if tone_mapping is None else (1 if tone_mapping else 0)
        p.stream = torch.cuda.current_stream(self.device).cuda_stream
        rgb = torch.empty((h, w, 3), dtype=torch.float32, device=self.device)
        rgb8 = torch.empty((h, w, 3), dtype=torch.uint8, device=self.device) if want_rgb8 else None
        st = self.lib.gbl_film_develop(self.handle, accum.data_ptr(), C.byref(p), rgb.data_ptr(), rgb8.data_ptr() if want_rgb8 else None)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        return {"rgb": rgb, "rgb8": rgb8}

    def _params(self, setting=None, window=None, seed=0, replay=None, li_out=None, stats=False, rr=False, shard=None,
                schedule=0, sampler="native", exact_ties=False):
        s = setting or self.scene.desc.setting
        p = _abi.gbl_render_params()
        p.integrator = s.integrator
        p.sample_per_pixel = s.sample_per_pixel
        p.max_ray_depth = s.max_ray_depth
        p.ao_sample_num = s.ao_sample_num
        p.bssrdf_sample_num = s.bssrdf_sample_num
        w = window or (0, 0, 0, 0)
        for i in range(4):
            p.window[i] = int(w[i])
        if shard is not None:
            p.tile_shard_index, p.tile_shard_count = int(shard[0]), int(shard[1])
        p.sample_mode = _abi.GBL_SAMPLES_REPLAY if replay is not None else (
            _abi.GBL_SAMPLES_STREAM if sampler == "stream" else _abi.GBL_SAMPLES_NATIVE)
        p.seed = int(seed)
        p.replay_samples = replay.data_ptr() if replay is not None else None
        p.li_out = li_out.data_ptr() if li_out is not None else None
        p.russian_roulette = 1 if rr else 0
        p.collect_stats = 1 if stats else 0
        p.schedule = {"auto": 0, "megakernel": 1, "wavefront": 2}.get(schedule, schedule)
        p.exact_ties = 1 if exact_ties else 0
        torch = _torch()
        p.stream = torch.cuda.current_stream(self.device).cuda_stream
        return p

    def render(self, film=None, setting=None, window=None, seed=0, replay_samples=None, want_li=False, stats=False,
               timed=False, rr=False, shard=None, schedule="auto", sampler="native", exact_ties=False):
        """Accumulate one pass into ``film`` (created if None).

        replay_samples: (n, dims) float32 tensor/array of Sample records for the
        window, pixel-major (GBL_SAMPLES_REPLAY); otherwise the native sampler.
        sampler: "native" (counter-based law) or "stream" (the reference's own mt19937 stream, GBL_SAMPLES_STREAM).
        shard: (index, count) renders only every count-th 8x8 sample tile (multi-GPU).
        exact_ties: native sampler on lean scenes -- keep the reference's exact-t tie rule (gbl_render_params.exact_ties).
        Returns dict(film=..., li=..., stats=...).
        """
        torch = _torch()
        if film is None:
            film = self.new_film()
        replay = None
        if replay_samples is not None:
            replay = torch.as_tensor(np.ascontiguousarray(replay_samples, np.float32) if isinstance(
                replay_samples, np.ndarray) else replay_samples, dtype=torch.float32, device=self.device).contiguous()
        s = setting or self.scene.desc.setting
        w = window or self.window
        spp = _abi.host_lib().gbl_host_round_to_square(s.sample_per_pixel)
        npaths = (w[1] - w[0]) * (w[3] - w[2]) * spp
        if replay is not None:
            dims = _abi.host_lib().gbl_host_sample_dimension_scene(C.byref(self.scene.desc), C.byref(s))
            if tuple(replay.shape) != (npaths, dims):
                raise ValueError("replay_samples must have shape (%d, %d), got %s" % (npaths, dims, tuple(replay.shape)))
        li = torch.zeros((npaths, 4), dtype=torch.float32, device=self.device) if want_li else None
        p = self._params(s, window, seed, replay, li, stats, rr, shard, schedule, sampler, exact_ties)
        st_out = _abi.gbl_stats() if (stats or timed) else None
        st = self.lib.gbl_render(self.handle, C.byref(p), film.accum.data_ptr(), C.byref(st_out) if st_out else None)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        return {"film": film, "li": li, "stats": st_out.as_dict() if st_out else None, "paths": npaths}

    def render_aov(self, albedo=True, normal=True, depth=True, want_samples=False, films=None, setting=None, window=None,
                   seed=0, replay_samples=None, shard=None, exact_ties=False, stats=False, sampler="native", timed=False):
        """First-hit feature films of the camera samples ``render`` draws for the same arguments (gbl_render_aov).

        albedo / normal / depth: which films to produce; ``films`` may carry existing ones ({"albedo": Film, ...}), which are
        accumulated into.  want_samples: also the per-sample records, an (n, 12) float32 tensor in ``render``'s li order --
        {albedo(3), t, normal(3), instance, position(3), hit}; words 7 and 11 are integers, ``samples_i32`` is the int32 view.
        The depth film holds {sum w*t*hit, sum w*hit, 0, sum w}: see ``resolve_depth``.
        stats: gbl_stats with the node / triangle counters (the instrumented kernels); timed: gbl_stats for its kernel_ms only.
        Returns dict(albedo=, normal=, depth= Film or None, samples=, samples_i32=, stats=, paths=).
        """
        torch = _torch()
        films = dict(films or {})
        out = {}
        for name, want in (("albedo", albedo), ("normal", normal), ("depth", depth)):
            f = films.get(name)
            out[name] = f if f is not None else (self.new_film() if want else None)
        replay = None
        if replay_samples is not None:
            replay = torch.as_tensor(np.ascontiguousarray(replay_samples, np.float32) if isinstance(
                replay_samples, np.ndarray) else replay_samples, dtype=torch.float32, device=self.device).contiguous()
        s = setting or self.scene.desc.setting
        w = window or self.window
        spp = _abi.host_lib().gbl_host_round_to_square(s.sample_per_pixel)
        npaths = (w[1] - w[0]) * (w[3] - w[2]) * spp
        if replay is not None:
            dims = _abi.host_lib().gbl_host_sample_dimension_scene(C.byref(self.scene.desc), C.byref(s))
            if tuple(replay.shape) != (npaths, dims):
                raise ValueError("replay_samples must have shape (%d, %d), got %s" % (npaths, dims, tuple(replay.shape)))
        samples = torch.zeros((npaths, 12), dtype=torch.float32, device=self.device) if want_samples else None
        p = self._params(s, window, seed, replay, None, stats, False, shard, 0, sampler, exact_ties)
        if sampler == "replay" and replay is None:
            p.sample_mode = _abi.GBL_SAMPLES_REPLAY
        tg = _abi.gbl_aov_targets()
        tg.albedo_accum = out["albedo"].accum.data_ptr() if out["albedo"] is not None else None
        tg.normal_accum = out["normal"].accum.data_ptr() if out["normal"] is not None else None
        tg.depth_accum = out["depth"].accum.data_ptr() if out["depth"] is not None else None
        tg.samples_out = samples.data_ptr() if samples is not None else None
        st_out = _abi.gbl_stats() if (stats or timed) else None
        st = self.lib.gbl_render_aov(self.handle, C.byref(p), C.byref(tg), C.byref(st_out) if st_out else None)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        out.update(samples=samples, samples_i32=samples.view(torch.int32) if samples is not None else None,
                   stats=st_out.as_dict() if st_out else None, paths=npaths)
        return out

    def resolve_depth(self, film):
        """(depth, coverage) of a depth film (gbl_aov_resolve_depth) on the current stream: two (yres, xres) float32 tensors,
        depth = x / y and coverage = y / w of the accumulator, 0 where the denominator is 0."""
        torch = _torch()
        accum = film.accum if isinstance(film, Film) else film
        h, w = self.info.yres, self.info.xres
        if tuple(accum.shape) != (h, w, 4) or accum.dtype != torch.float32 or accum.device != self.device or not accum.is_contiguous():
            raise ValueError("film must be a contiguous (%d, %d, 4) float32 tensor on %s" % (h, w, self.device))
        depth = torch.empty((h, w), dtype=torch.float32, device=self.device)
        coverage = torch.empty((h, w), dtype=torch.float32, device=self.device)
        st = self.lib.gbl_aov_resolve_depth(self.handle, accum.data_ptr(), depth.data_ptr(), coverage.data_ptr(),
                                            torch.cuda.current_stream(self.device).cuda_stream)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        return depth, coverage

    def variance(self, li, window=None, setting=None):
        """Variance of the pixel mean (gbl_film_variance) from the per-sample radiance ``render(want_li=True)`` returns for the
        same window and setting: a (yres, xres) float32 tensor, 0 outside the window and where fewer than two finite
        samples fell.  On the current stream."""
        torch = _torch()
        s = setting or self.scene.desc.setting
        w = window or self.window
        spp = _abi.host_lib().gbl_host_round_to_square(s.sample_per_pixel)
        n = (w[1] - w[0]) * (w[3] - w[2]) * spp
        if tuple(li.shape) != (n, 4) or li.dtype != torch.float32 or li.device != self.device or not li.is_contiguous():
            raise ValueError("li must be a contiguous (%d, 4) float32 tensor on %s" % (n, self.device))
        out = torch.zeros((self.info.yres, self.info.xres), dtype=torch.float32, device=self.device)
        st = self.lib.gbl_film_variance(self.handle, li.data_ptr(), (C.c_int32 * 4)(*[int(v) for v in w]), s.sample_per_pixel,
                                        out.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        return out

    def denoise(self, film, variance=None, albedo=None, normal=None, depth=None, iterations=5, sigma_luminance=4.0,
                sigma_normal=0.5, sigma_albedo=0.1, sigma_depth=0.1, demodulate=True):
        """Edge-avoiding a-trous filter of a film (gbl_film_denoise) on the current stream.  ``film`` and the guides
        ``albedo`` / ``normal`` / ``depth`` (render_aov's) are Films or their (yres, xres, 4) accumulator tensors, ``variance``
        the (yres, xres) plane of ``variance()``; a guide left None drops out of the filter.  demodulate divides by the albedo
        before filtering and multiplies back after; it is ignored without an albedo film.
        Returns a new Film {rgb, 1} ({0, 0, 0, 0} for a pixel of weight 0 or with a non-finite input): ``normalized()`` and
        ``develop()`` take it as they take a rendered one."""
        torch = _torch()
        h, w = self.info.yres, self.info.xres

        def plane(t, shape, what):
            if t is None:
                return None
            t = t.accum if isinstance(t, Film) else t
            if tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
                raise ValueError("%s must be a contiguous %s float32 tensor on %s" % (what, shape, self.device))
            return t
        accum = plane(film, (h, w, 4), "film")
        var = plane(variance, (h, w), "variance")
        guides = [plane(albedo, (h, w, 4), "albedo"), plane(normal, (h, w, 4), "normal"), plane(depth, (h, w, 4), "depth")]
        p = _abi.gbl_denoise_params()
        p.iterations = int(iterations)
        p.sigma_luminance, p.sigma_normal = float(sigma_luminance), float(sigma_normal)
        p.sigma_albedo, p.sigma_depth = float(sigma_albedo), float(sigma_depth)
        p.demodulate = 1 if (demodulate and guides[0] is not None) else 0
        p.stream = torch.cuda.current_stream(self.device).cuda_stream
        out = Film(w, h, self.device)
        st = self.lib.gbl_film_denoise(self.handle, accum.data_ptr(), var.data_ptr() if var is not None else None,
                                       *[g.data_ptr() if g is not None else None for g in guides], C.byref(p), out.accum.data_ptr())
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        return out

    def new_history(self):
        """A history for ``accumulate``: (3, yres, xres, 4) float32 zeros on the device -- the planes {c.rgb, N}, {m1, m2, v, z} and
        {n.xyz, surf}.  N = 0 everywhere: no pixel has history yet."""
        torch = _torch()
        return torch.zeros((3, self.info.yres, self.info.xres, 4), dtype=torch.float32, device=self.device)

    def motion(self, prev_camera, prev_instances=None, normal=None, prev_vertices=None):
        """Motion planes of the current frame (gbl_render_motion) on the current stream: a (2, yres, xres, 4) float32 tensor --
        [0] = {image_x, image_y, z_exp, ok}, where the surface under each pixel's centre lay under ``prev_camera`` (a gbl_camera)
        and, for an instance that moved since, under its transform in ``prev_instances`` (``instances()`` as it was when the
        previous frame was rendered; None: no instance moved); [1] = {the current normal carried into the previous frame, instance
        + 1 or 0}, the normal taken from ``normal`` (render_aov's film; zeros without one).  ``accumulate(motion=...)`` reads it.
        ``prev_vertices``: {mesh: (vertex_count, 3) float32 array}, ``vertices(mesh)`` as it was when the previous frame was
        rendered, for every mesh ``update_vertices`` edited since (gbl_render_motion_deform): a surface that deformed is followed
        through its triangle's previous pose.  A mesh whose positions are the context's own counts as not deformed.  Tensors on
        the tracer's device (``vertices(mesh, device=True)``) are read where they lie (gbl_render_motion_deform_device); a dict
        that mixes tensors and arrays is a ValueError."""
        torch = _torch()
        h, w = self.info.yres, self.info.xres
        p = _abi.gbl_motion_params()
        p.prev_camera = prev_camera
        arr = None
        if prev_instances is not None:
            if len(prev_instances) != int(self.info.instances):
                raise ValueError("prev_instances must hold one transform per instance (%d)" % int(self.info.instances))
            arr = (_abi.gbl_trs * max(len(prev_instances), 1))()
            for i, (pos, quat, scale) in enumerate(prev_instances):
                arr[i].position[:] = pos
                arr[i].orientation[:] = quat
                arr[i].scale[:] = scale
            p.prev_to_world = arr
        if normal is not None:
            normal = normal.accum if isinstance(normal, Film) else normal
            if tuple(normal.shape) != (h, w, 4) or normal.dtype != torch.float32 or normal.device != self.device or not normal.is_contiguous():
                raise ValueError("normal must be a contiguous (%d, %d, 4) float32 tensor on %s" % (h, w, self.device))
            p.normal_accum = normal.data_ptr()
        p.stream = torch.cuda.current_stream(self.device).cuda_stream
        out = torch.empty((2, h, w, 4), dtype=torch.float32, device=self.device)
        if prev_vertices is None:
            st = self.lib.gbl_render_motion(self.handle, C.byref(p), out.data_ptr())
        else:
            keep = []       # the arrays the list points into, alive across the call
            listed = (_abi.gbl_motion_mesh * max(len(prev_vertices), 1))()
            on_device = [hasattr(v, "data_ptr") for v in prev_vertices.values()]
            if any(on_device) and not all(on_device):
                raise ValueError("prev_vertices must hold tensors only or arrays only")
            for k, (mesh, positions) in enumerate(prev_vertices.items()):
                mesh = int(mesh)
                known = 0 <= mesh < self.scene.desc.num_meshes and self.scene.desc.meshes[mesh].shape == 0
                count = int(self.scene.desc.meshes[mesh].vertex_count) if known else None
                if mesh < 0:
                    raise ValueError("prev_vertices: mesh %d is out of range" % mesh)
                if all(on_device):
                    ptr = self._device_vertices("prev_vertices[%d]" % mesh, positions, (count, 3) if known else None)
                    keep.append(positions)
                else:
                    pos = np.ascontiguousarray(positions, np.float32)
                    if known and pos.shape != (count, 3):
                        raise ValueError("prev_vertices[%d] must have shape (%d, 3), got %s" % (mesh, count, pos.shape))
                    keep.append(pos)
                    ptr = pos.ctypes.data
                listed[k].mesh, listed[k].reserved, listed[k].positions = mesh, 0, ptr
            entry = self.lib.gbl_render_motion_deform_device if prev_vertices and all(on_device) else self.lib.gbl_render_motion_deform
            st = entry(self.handle, C.byref(p), listed, len(prev_vertices), out.data_ptr())
            del keep
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        return out

    def accumulate(self, film, depth, variance=None, normal=None, history=None, prev_camera=None, alpha_min=0.1, max_history=64.0,
                   sigma_depth=0.05, cos_normal=0.9, motion=None):
        """Reprojected temporal accumulation (gbl_film_accumulate) on the current stream: blends the frame ``film`` (rendered
        under the tracer's current camera) into ``history``, the "history" a previous call returned, fetched from where each
        pixel's surface lay under ``prev_camera`` (a gbl_camera: ``camera()`` as it was when that frame was rendered).
        ``depth`` and ``normal`` are render_aov's films, ``variance`` the plane of ``variance()``; without it the variance is
        estimated from the accumulated luminance moments and the current frame's neighbourhood.  history=None starts a
        sequence.  ``motion``: the planes ``motion()`` returned for this frame -- the history is then fetched from where they say
        (gbl_film_accumulate_motion), which carries moved instances along, and ``prev_camera`` is not needed.  Returns {"film": Film {rgb, 1} (``denoise``, ``normalized`` and ``develop`` take it as a rendered one),
        "variance": (yres, xres) variance of the accumulated pixel, "history": the new history (the input one is not touched)}."""
        torch = _torch()
        h, w = self.info.yres, self.info.xres

        def plane(t, shape, what):
            if t is None:
                return None
            t = t.accum if isinstance(t, Film) else t
            if tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
                raise ValueError("%s must be a contiguous %s float32 tensor on %s" % (what, shape, self.device))
            return t
        accum, dep = plane(film, (h, w, 4), "film"), plane(depth, (h, w, 4), "depth")
        if accum is None or dep is None:
            raise ValueError("accumulate needs a film and a depth film")
        var, nrm = plane(variance, (h, w), "variance"), plane(normal, (h, w, 4), "normal")
        hist = plane(history, (3, h, w, 4), "history")
        mo = plane(motion, (2, h, w, 4), "motion")
        if hist is not None and prev_camera is None and mo is None:
            raise ValueError("a history needs the camera it was accumulated under (prev_camera)")
        p = _abi.gbl_temporal_params()
        if prev_camera is not None:
            p.prev_camera = prev_camera
        p.alpha_min, p.max_history = float(alpha_min), float(max_history)
        p.sigma_depth, p.cos_normal = float(sigma_depth), float(cos_normal)
        p.stream = torch.cuda.current_stream(self.device).cuda_stream
        out = Film(w, h, self.device)
        var_out = torch.empty((h, w), dtype=torch.float32, device=self.device)
        hist_out = torch.empty((3, h, w, 4), dtype=torch.float32, device=self.device)

        def ptr(t):
            return t.data_ptr() if t is not None else None
        if mo is not None:
            st = self.lib.gbl_film_accumulate_motion(self.handle, accum.data_ptr(), ptr(var), ptr(nrm), dep.data_ptr(), ptr(hist), hist_out.data_ptr(),
                                                     mo.data_ptr(), C.byref(p), out.accum.data_ptr(), var_out.data_ptr())
        else:
            st = self.lib.gbl_film_accumulate(self.handle, accum.data_ptr(), ptr(var), ptr(nrm), dep.data_ptr(), ptr(hist), hist_out.data_ptr(),
                                              C.byref(p), out.accum.data_ptr(), var_out.data_ptr())
        if st != _abi.GBL_OK:
            raise _abi.GoblinError(st, self.lib.gbl_last_error(self.handle).decode())
        return {"film": out, "variance": var_out, "history": hist_out}
