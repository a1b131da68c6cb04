#!/usr/bin/env python3
"""Generate surface_<case>.npz from the REAL reference for the cases of tests/surface_chart.py.

Runs only where oracle/_ref/ref_harness exists (the reference compiled by oracle/Makefile, `make -C oracle ref`).  For every
case the harness renders with one thread (`ref_harness li`, every Li call logged) and the fixture keeps what its programs wrote:

    film      (16, 24, 4)  the Film's accumulators {r, g, b, weight}
    samples   (n, 4)       every camera sample's {imageX, imageY, lensU1, lensU2}, in the order Li was called (tile, then pixel)
    li        (n, 4)       what Li returned for it

(The rest of a Sample record is not kept: the oracle regenerates the whole stream, tests/test_surface_chart_cpu.py.)  The archives are
written with fixed member timestamps, so that a second run gives the same bytes.

    python tests/golden/make_surface_golden.py [case ...]
"""
import io
import json
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import surface_chart as sc  # noqa: E402

HARNESS = os.path.join(REPO, "oracle", "_ref", "ref_harness")


def run_case(case, tmp):
    """The harness on one case -> dict(film, samples, li)."""
    jp, prefix = os.path.join(tmp, case + ".json"), os.path.join(tmp, case)
    with open(jp, "w") as f:
        json.dump(sc.harness_doc(case, sc.scene_dir()), f)
    meta = json.loads(subprocess.check_output([HARNESS, "li", jp, prefix, "1", str(1 << 30)]).decode())
    film = np.fromfile(prefix + ".film.f32", np.float32).reshape(meta["yres"], meta["xres"], 4)
    samples = np.fromfile(prefix + ".samples.f32", np.float32).reshape(-1, meta["dims"])
    li = np.fromfile(prefix + ".li.f32", np.float32).reshape(-1, 4)
    assert samples.shape[0] == li.shape[0] == meta["records"] == meta["paths"], meta
    return {"film": film, "samples": np.ascontiguousarray(samples[:, :4]), "li": li}


def save(path, arrays):
    """np.savez_compressed's layout with every member dated 1980-01-01: the same arrays give the same file."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in ("film", "samples", "li"):
            buf = io.BytesIO()
            np.save(buf, np.ascontiguousarray(arrays[name]))
            z.writestr(zipfile.ZipInfo(name + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    if not os.path.exists(HARNESS):
        sys.exit("oracle/_ref/ref_harness is missing: run `make -C oracle ref` (needs the reference's sources)")
    only = set(sys.argv[1:])
    with tempfile.TemporaryDirectory() as tmp:
        for case in sc.ALL_CASES:
            if only and case not in only:
                continue
            arrays = run_case(case, tmp)
            save(os.path.join(HERE, "surface_" + case + ".npz"), arrays)
            print(case, arrays["li"].shape[0], "samples, film", arrays["film"].shape)


if __name__ == "__main__":
    main()
