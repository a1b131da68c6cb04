"""The participating medium on generated charts (tests/medium_chart.py), device side: kernels/medium.h, kernels/volume.h and
stream_medium_phase against the oracle (per sample, native sampler) and against the compiled reference's own Films (stream sampler,
tests/golden/medium_<case>.npz).

Every spp-1 case is bit-identical: a Film pixel of these charts is one sample's w * (tr * L + Lv) (asserted on the host,
tests/test_medium_chart_cpu.py::test_a_film_pixel_is_one_sample), so the device's Film under the stream sampler must BE the
reference's, in whatever order its atomics land.  The four summed cases are held to the bar of the other stream + medium tests
(tests/test_gpu_parity.py::test_stream_mode_medium_*): relL2 of the normalised Film <= 1e-5, weight plane rtol 1e-5.
"""
import numpy as np
import pytest

import helpers
import medium_chart as mc
import oracle_binding as ob

pytestmark = pytest.mark.gpu

SEED = 0x5EEDC0FFEE


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def tracer(case, bvh="host"):
    from goblin_amd.renderer import HipPathTracer
    return HipPathTracer(mc.scene(case), 0, bvh=bvh)


def check_native(case, r, schedules):
    """Per sample: the device's li is the oracle's replay of the native sampler's records, bit for bit, NaN positions equal; and the
    device's Film has weight 0 exactly where the oracle's splat dropped every sample."""
    o = ob.Oracle(mc.scene(case))
    samples = o.native_samples(SEED)
    li_ref, _ = o.li_replay(samples, threads=4)
    dropped = o.splat(samples, li_ref)[..., 3] == 0
    for schedule in schedules:
        out = r.render(seed=SEED, want_li=True, schedule=schedule)
        li = out["li"].cpu().numpy()
        assert li.shape[0] == li_ref.shape[0]
        same = mc.same_bits(li[:, :3], li_ref[:, :3])
        if not same:
            bad = np.flatnonzero((li[:, :3].view(np.uint32) != li_ref[:, :3].view(np.uint32)).any(axis=1) & ~(np.isnan(li[:, :3]) & np.isnan(li_ref[:, :3])).all(axis=1))
            print(case, schedule, "%d of %d samples differ; first:" % (len(bad), li.shape[0]),
                  [(int(i), samples[i, :2].tolist(), li[i, :3].tolist(), li_ref[i, :3].tolist()) for i in bad[:5]])
        assert same, (case, schedule)
        film = out["film"].numpy()
        assert not np.isnan(film).any()
        assert np.array_equal(film[..., 3] == 0, dropped), (case, schedule)


@pytest.mark.parametrize("case", mc.ALL_CASES)
def test_native_sampler_is_the_oracle_per_sample(torch, case):
    """The megakernel on every case, the wavefront schedule too under the path tracer."""
    check_native(case, tracer(case), ["megakernel", "wavefront"] if case in mc.PATH_CASES else ["auto"])


@pytest.mark.parametrize("case", ["hom", "het"])
def test_native_sampler_over_the_device_built_bvh(torch, case):
    check_native(case, tracer(case, bvh="device"), ["megakernel", "wavefront"])


@pytest.mark.parametrize("case", list(mc.CASES))
def test_stream_film_is_the_reference_film(torch, case):
    """The device's Film under the stream sampler against the compiled reference's: all four planes, bit for bit."""
    ref = mc.golden(case)["film"]
    film = tracer(case).render(sampler="stream")["film"].numpy()
    same = np.array_equal(film.view(np.uint32), ref.view(np.uint32))
    if not same:
        print(mc.pixel_report(case, film, ref))
    assert same, case


def summed_bar(case, what, film, ref):
    rel = helpers.rel_l2(ob.normalize_film(film), ob.normalize_film(ref))
    print(case, what, "film relL2 %.3g, max weight rel diff %.3g" % (rel, float(np.abs(film[..., 3] / ref[..., 3] - 1).max())))
    np.testing.assert_allclose(film[..., 3], ref[..., 3], rtol=1e-5, atol=1e-6)
    assert rel <= 1e-5, (case, what, rel)


@pytest.mark.parametrize("case", list(mc.SUMMED))
def test_stream_summed_film(torch, case):
    summed_bar(case, "stream", tracer(case).render(sampler="stream")["film"].numpy(), mc.golden(case)["film"])


@pytest.mark.parametrize("case", list(mc.SUMMED))
def test_stream_chunked_walk(torch, case, monkeypatch):
    """GBL_STREAM_TAIL=1: the least scratch the phase can work with, so a pixel's four samples are walked in more than one chunk,
    the generator's state saved and restored in between.  Homogeneous: room for 4 x 19 words where a crossing sample brings 18
    and its Li's discarded draws.  Heterogeneous (its own cap arithmetic): a quarter of one sample's budget each, 4 x 187 words less
    the 640 set aside for the generator's state = 108, where a crossing sample brings up to 42 and its Li's discarded draws (18
    under the path tracer, 84 under Whitted).  Same samples either way: the per-sample radiance is identical, the Film
    differs by the order of its additions."""
    whole = tracer(case).render(sampler="stream", want_li=True)
    monkeypatch.setenv("GBL_STREAM_TAIL", "1")
    chunked = tracer(case).render(sampler="stream", want_li=True)
    assert mc.same_bits(chunked["li"].cpu().numpy(), whole["li"].cpu().numpy()), case
    whole, chunked = whole["film"].numpy(), chunked["film"].numpy()
    print(case, "chunked vs one chunk: max abs diff %.3g" % float(np.abs(chunked - whole).max()))
    np.testing.assert_allclose(chunked, whole, rtol=1e-6, atol=1e-7)
    summed_bar(case, "chunked", chunked, mc.golden(case)["film"])
