"""gbl_radiance_rays without a GPU: the ABI's new names and the struct's layout, the headroom of the call's unit-direction bound over
the rays it is pinned on, that the bit comparisons of tests/test_gpu_radiance.py leave no sample out, and the five kernels in the
cross-compiled library."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob
import radiance_cases as rc
import surface_chart as sc
from goblin_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "goblin_hip.h")
NAMES = ("gbl_radiance_rays", "gbl_selftest_radiance")


def test_new_names_are_declared_exported_and_listed():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _abi.hip_lib()   # dlopen only
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _abi.HIP_SYMBOLS, name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+GBL_RADIANCE_EXACT_TIES\s+1u", text) and _abi.GBL_RADIANCE_EXACT_TIES == 1
    assert re.search(r"#define\s+GBL_RADIANCE_RUSSIAN_ROULETTE\s+2u", text) and _abi.GBL_RADIANCE_RUSSIAN_ROULETTE == 2
    assert re.search(r"#define\s+GBL_ABI_VERSION\s+14\b", text) and _abi.GBL_ABI_VERSION == 14
    from goblin_amd.renderer import HipPathTracer
    assert callable(HipPathTracer.radiance)


def test_params_struct_has_the_c_layout(tmp_path):
    src = tmp_path / "sizes.c"
    fields = [f[0] for f in _abi.gbl_radiance_params._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "goblin_hip.h"\nint main(void){\n'
                   'printf("size %zu\\n", sizeof(gbl_radiance_params));\n' +
                   "".join('printf("%s %%zu\\n", offsetof(gbl_radiance_params, %s));\n' % (f, f) for f in fields) + "return 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])   # plain C
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert C.sizeof(_abi.gbl_radiance_params) == int(out["size"])
    assert _abi.gbl_radiance_params.seed.offset == int(out["seed"])
    for f in fields:
        assert getattr(_abi.gbl_radiance_params, f).offset == int(out[f]), f


def test_the_charts_are_the_path_traced_ones_but_the_thin_lens():
    assert len(rc.CHARTS) == 68 and "thinlens" not in rc.CHARTS and all(sc.is_path(c) for c in rc.CHARTS)
    assert len(rc.TWINS) == 8 and len(rc.SUMMED) >= 3 and set(rc.BASES) == {"lean", "ext", "deep"}


@pytest.fixture(scope="module")
def chart_rays():
    """Per chart: (native samples, their camera rays, the oracle's li of those samples), computed once."""
    out = {}
    for case in rc.CHARTS:
        o = ob.Oracle(sc.scene(case))
        samples = o.native_samples(rc.SEED)
        li, _ = o.li_replay(samples, threads=4)
        out[case] = (samples, rc.camera_rays(o, samples), li)
    return out


def test_camera_rays_are_unit_well_inside_the_validity_bound(chart_rays):
    """The call refuses |d.d - 1| > 1e-4; the reference's own normalise must leave an order of magnitude less on every pinned ray."""
    worst = 0.0
    for case, (samples, rays, _) in chart_rays.items():
        assert rays.shape == (425, 8), (case, rays.shape)
        d = rays[:, 4:7].astype(np.float64)
        worst = max(worst, float(np.abs((d * d).sum(axis=1) - 1.0).max()))
    print("max |d.d - 1| over %d charts: %.3g" % (len(chart_rays), worst))
    assert worst <= rc.UNIT_HEADROOM < rc.UNIT_TOL


def test_no_oracle_li_on_the_charts_is_nan(chart_rays):
    """same_bits treats NaN positions as equal: with none, the GPU comparisons leave nothing out."""
    total = sum(li.shape[0] for _, _, li in chart_rays.values())
    nans = sum(int(np.isnan(li[:, :3]).any(axis=1).sum()) for _, _, li in chart_rays.values())
    print("NaN li: %d of %d" % (nans, total))
    assert nans == 0 and total == 425 * len(rc.CHARTS)


def test_invalid_table_is_invalid_by_the_stated_rule():
    r = rc.INVALID_RAYS
    d = r[:, 4:7].astype(np.float64)
    dd = (d * d).sum(axis=1)
    with np.errstate(invalid="ignore"):
        bad = (~np.isfinite(r[:, [0, 1, 2, 4, 5, 6]]).all(axis=1) | np.isnan(r).any(axis=1) | (dd == 0) | ~(r[:, 3] <= r[:, 7]) | ~(np.abs(dd - 1.0) <= rc.UNIT_TOL))
    assert bad.all()
    assert abs(np.sqrt(dd[-2]) - 1.01) < 1e-6 and abs(np.sqrt(dd[-1]) - 0.5) < 1e-6


def test_library_holds_exactly_five_radiance_kernels():
    lib = os.path.join(REPO, "goblin_amd", "lib", "libgoblin_hip.so")
    assert os.path.exists(lib), "build the HIP library first (__graft_entry__.build())"
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--json", lib], capture_output=True, text=True, check=True).stdout
    names = sorted(r["name"].split("(")[0] for r in json.loads(out) if "radiance_trace<" in r["name"])
    want = sorted("void radiance_trace<%s>" % t for t in ("false, false, false", "false, false, true", "true, false, true", "false, true, true", "true, true, true"))
    assert names == want, names
