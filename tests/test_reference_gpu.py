"""The device against the reference renderer's recorded outputs, directly.

tests/golden/reference/ holds what the reference's own code computed for the cases of
tests/reference_cases.py (oracle/ref/make_reference_fixtures.py wrote it from
oracle/_ref/ref_driver; tests/test_reference_cpu.py holds the oracle to the same files).
Here the same cases go through the C ABI and miro on the GPU and are compared with those
files, not with the oracle: bits for the exact tier and for the deep tier (every chain level,
path and eye ray, the reference run on the logged draws: float frame and 8-bit pixels), the
three statistical assertions for the statistical tier.  Nothing here needs the reference or
its driver.
"""
import numpy as np
import pytest

import miro
import reference_cases as RC
from helpers import bits, camera, scene_pair, tuned

pytestmark = pytest.mark.gpu

DET = RC.deterministic_cases()
REPLAY = RC.replay_cases()
STAT = RC.statistical_cases()
DEEP = RC.deep_cases()


def product(case):
    cfg, kw = RC.pair_args(case)
    P, _, _ = scene_pair(cfg, **kw)
    return P


def device_frame(case, size=None):
    w, h = size or RC.case_size(case)
    img = miro.Image(); img.resize(w, h)
    product(case).raytraceImage(camera(RC.case_camera(case)), img)
    return img.rgb


@pytest.mark.parametrize("name", ["deterministic." + n for n in sorted(DET)] + ["replay." + n for n in sorted(REPLAY)])
def test_frame_matches_the_recorded_reference(name):
    """raytraceImage at one sample per pixel: the deterministic frames, and the stochastic ones the
    reference rendered on the draws the device's counter RNG makes (seed 0)."""
    tier, key = name.split(".", 1)
    ref = RC.fixture("frames.npz")[name]
    got = device_frame((DET if tier == "deterministic" else REPLAY)[key])
    assert got.shape == ref.shape and np.array_equal(bits(got), bits(ref))


@pytest.mark.parametrize("name", ["rect_8_transparent", "depth_of_field", "motion_blur_cannonball"])
def test_sample_rays_matches_the_recorded_reference(name):
    """mrt_sample_rays on mrt_camera_rays' rays (lens points and time samples included)."""
    case = REPLAY[name]
    w, h = RC.case_size(case)
    o, d, t = camera(RC.case_camera(case)).rays(w, h)
    rgb = product(case).sampleRays(o, d, t)
    assert np.array_equal(bits(rgb), bits(RC.fixture("frames.npz")["replay." + name]))


@pytest.mark.parametrize("model", RC.TRACE_MODELS)
def test_trace_matches_the_recorded_reference(model):
    fx = RC.fixture("trace_%s.npz" % model)
    P, _, _ = scene_pair(dict(RC.C1, material=dict(kind="lambert", kd=(1, 1, 1))), meshes=[RC.trace_mesh(model)])
    assert set(fx["cls"]) == set(range(len(RC.RAY_CLASSES))) and len(fx["o"]) >= 10000
    h = P.traceBatch(fx["o"], fx["d"], fx["tmin"], fx["tmax"])
    assert np.array_equal(h["prim"], fx["prim"])
    for k in ("t", "a", "b"):
        assert np.array_equal(bits(h[k]), bits(fx[k])), k
    # any-hit mode: prim 1 = occluded, -1 = clear; the reference's shadow query hits the same rays
    occ = P.traceBatch(fx["o"], fx["d"], fx["tmin"], fx["tmax"], any_hit=True)
    assert np.array_equal(occ["prim"] >= 0, fx["shadow_hit"] != 0)


@pytest.mark.parametrize("name", sorted(STAT))
def test_distribution_matches_the_recorded_reference(name):
    fx, meta = RC.fixture("statistical.npz"), RC.fixture_json()["statistical"][name]
    m, s, K = fx[name + ".m"], fx[name + ".s"], meta["K"]
    held = RC.statistics(fx[name + ".held_out"], m, s, K)
    ours = RC.statistics(device_frame(STAT[name], RC.STAT_SIZE), m, s, K)
    print(name, "held-out", held, "device", ours)
    RC.assert_statistics(held, "the reference's held-out replica")
    RC.assert_statistics(ours, "the device")


# ------------------------------------------------------------------ deep tier
_products = {}


def deep_product(name):
    if name not in _products:
        _products[name] = product(DEEP[name])
    return _products[name]


def assert_deep_frame(name):
    fx = RC.fixture("deep.npz")
    case = DEEP[name]
    w, h = RC.case_size(case)
    img = miro.Image(); img.resize(w, h)
    P = deep_product(name)
    P.raytraceImage(camera(RC.case_camera(case)), img)
    ref = fx[name + ".rgb"]
    bad = (bits(img.rgb) != bits(ref)).any(2)
    assert img.rgb.shape == ref.shape and not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:1].tolist())
    assert np.array_equal(img.pixels, fx[name + ".rgb8"])
    return P


@pytest.mark.parametrize("name", sorted(DEEP))
def test_deep_frame_matches_the_recorded_reference(name):
    """raytraceImage's float frame and img.pixels against what Scene::adaptiveSampleScene and
    Image::setPixel made of the same draws at every chain level."""
    assert_deep_frame(name)


@pytest.mark.parametrize("name", sorted(DEEP))
def test_deep_frame_in_chunks_matches_the_recorded_reference(name):
    """The same under worst-case level capacities in a 1-MB scratch budget: the chunked route."""
    with tuned(chain_mb=1, chain_est=0):
        P = assert_deep_frame(name)
    assert P.last_stats["chain_chunks"] > 1 and P.last_stats["secondary_rays"] > 0, P.last_stats


@pytest.mark.parametrize("name", sorted(n for n in DEEP if "subdivs" not in DEEP[n]))
def test_deep_sample_rays_matches_the_recorded_reference(name):
    """One eye ray per pixel: mrt_sample_rays on mrt_camera_rays' rays is the same frame."""
    case = DEEP[name]
    w, h = RC.case_size(case)
    o, d, t = camera(RC.case_camera(case)).rays(w, h)
    rgb = deep_product(name).sampleRays(o, d, t)
    assert np.array_equal(bits(rgb), bits(RC.fixture("deep.npz")[name + ".rgb"]))
