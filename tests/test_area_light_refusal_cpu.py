"""validate_desc refuses an instance whose `area_light` names a light that is not an area light (no GPU: gbl_create packs the
description before it looks for a device).  The lean path kernels rest on it: a vertex that picked a spot, point or directional
light can never pass the MIS test `instances[hit].area_light == picked light`, so the capped vertex traces no ray under such a
light (kernels/render_kernels.h).  The loader only ever writes an area light's index there; this is for hand-made descriptions."""
import ctypes as C

from goblin_amd import _abi
from goblin_amd import scene as gs


def _create(desc):
    h = C.c_void_p()
    got = _abi.hip_lib().gbl_create(C.byref(desc), 0, C.byref(h))
    return got, _abi.hip_lib().gbl_last_error(None).decode(), h


def test_an_emissive_instance_must_name_an_area_light():
    scene = gs.load_scene("grid", gs.config_overrides(resolution=(16, 16), spp=1, depth=2))   # a spot and a point light
    desc = _abi.gbl_scene_desc.from_buffer_copy(scene.desc)
    assert desc.num_lights == 2 and all(desc.lights[i].type != _abi.GBL_LIGHT_AREA for i in range(2))
    instances = (_abi.gbl_instance * desc.num_instances)()
    C.memmove(instances, desc.instances, desc.num_instances * C.sizeof(_abi.gbl_instance))
    instances[1].area_light = 1
    desc.instances = C.cast(instances, type(desc.instances))
    got, text, h = _create(desc)
    assert got == _abi.GBL_ERR_INVALID and "instance 1: area_light names a light that is not an area light" in text, (got, text)
    assert not h
