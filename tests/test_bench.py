"""bench.py's plain run and --dump-outputs: the line a plain run prints, and the film it writes, which must be the film the timed
path computes (the same frame rendered in this process, up to the film's float summation order)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_dump_outputs_writes_the_whole_film_when_it_fits(tmp_path):
    film = np.random.default_rng(1).random((24, 40, 4), dtype=np.float32)
    files = bench.dump_outputs(str(tmp_path / "out"), film)
    assert [os.path.basename(f) for f in files] == ["film.npy"]
    got = np.load(files[0])
    assert got.dtype == np.float32 and np.array_equal(got, film)


def test_dump_outputs_samples_a_larger_film_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 40000)
    film = np.random.default_rng(2).random((100, 120, 4), dtype=np.float32)   # 192 000 bytes
    a = bench.dump_outputs(str(tmp_path / "a"), film)
    b = bench.dump_outputs(str(tmp_path / "b"), film)
    assert [os.path.basename(f) for f in a] == ["film_sample.npy", "film_sample_index.npy"]
    assert sum(os.path.getsize(f) for f in a) <= 40000
    sample, index = np.load(a[0]), np.load(a[1])
    assert sample.dtype == np.float32 and index.dtype == np.float64
    assert sample.shape == (index.shape[0], 4) and index.shape[0] > 1000
    assert (np.diff(index) > 0).all()
    assert np.array_equal(sample, film.reshape(-1, 4)[index.astype(np.int64)])
    assert all(np.array_equal(np.load(x), np.load(y)) for x, y in zip(a, b))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_timed_film(tmp_path):
    import torch
    from goblin_amd import scene as gs
    from goblin_amd.renderer import HipPathTracer
    assert torch.cuda.is_available()
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--resolution", "128", "128", "--spp", "16", "--dump-outputs", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "Mpaths/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["metric"].startswith("Mpaths/sec at 128x128x16spp")
    assert line["ms_per_step"] > 0 and line["value"] > 0
    paths = line["config"]["paths_per_step"]
    assert paths == 132 * 132 * 16                       # the sample window: 128 + 2 x 2 halo pixels a side
    assert abs(paths / (line["ms_per_step"] * 1e3) - line["value"]) <= 1e-3 * line["value"] + 1e-3
    # what moved behind --full stays out of a plain run
    for key in ("roofline", "value_tie_exact", "reference_stream_sampler", "other_configs", "feature_scenes", "cpu_baseline"):
        assert key not in line, key
    assert sorted(os.listdir(out)) == ["film.npy"]
    film_bench = np.load(out / "film.npy")
    scene = gs.load_scene("bunny", gs.config_overrides(resolution=(128, 128), spp=16, depth=8))
    film = HipPathTracer(scene, 0).render(seed=20261003)["film"].numpy()
    assert film_bench.dtype == np.float32 and film_bench.shape == film.shape
    np.testing.assert_allclose(film_bench[..., 3], film[..., 3], rtol=1e-5, atol=1e-6)
    rel = float(np.linalg.norm(film_bench[..., :3].astype(np.float64) - film[..., :3]) / np.linalg.norm(film[..., :3].astype(np.float64)))
    assert rel <= 1e-5, rel
