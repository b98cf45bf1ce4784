"""Scene::sampleScene for caller rays (mrt_sample_rays / mrt_sample_rays_async /
mrt_camera_rays; miro.Scene.sampleRays, miro.Camera.rays).

The defining property: shading the rays of mrt_camera_rays(cam, W, H, seed) gives the
float frame and the hit records of mrt_render(cam, W x H, seed) bit for bit, on every
dispatch path of the engine -- ray index y * W + x is the RNG's pixel key.  CPU tests
cover the argument checks and the host camera rays; GPU tests the identity per path, the
independence of the coherence hint, rays no camera can make and the async entry.
Frames are 37 x 29: neither 8, 64 nor the row width divides evenly."""
import ctypes as C

import numpy as np
import pytest

import miro
from helpers import bits, camera, fixture_mesh, scene_pair, tuned
from miro import scenes

W, H = 37, 29
CAM = dict(eye=(2.75, 2.75, 5.0), lookAt=(2.75, 2.75, 0.0), up=(0, 1, 0), fov=55.0)


def need_gpu():
    if miro.device_count() < 1:
        pytest.fail("no HIP device visible (GPU tests must run on the MI355X box)")


# ------------------------------------------------------------------ CPU: argument checks
def built_scene():
    P, _, _ = scene_pair(dict(scenes.CONFIGS["C1"]), meshes=[fixture_mesh("cornell_box")])
    return P


def last_error():
    return miro.lib().mrt_last_error().decode()


@pytest.mark.parametrize("entry", ["mrt_sample_rays", "mrt_sample_rays_async"])
def test_argument_checks_come_before_any_device_call(entry):
    """Both entries reject bad arguments with the error code and mrt_last_error set, before
    touching a device (this runs on a host without one); n == 0 is MRT_OK."""
    L = miro.lib()
    P = built_scene()
    buf = np.zeros(12, np.float32)
    p = buf.ctypes.data
    tail = (None,) if entry.endswith("async") else ()

    def call(scene, o, d, t, n, row_width, rgb):
        return getattr(L, entry)(scene, o, d, t, n, row_width, 0, 0, rgb, None, *tail)

    assert call(None, p, p, None, 1, 0, p) == -1 and "null scene" in last_error()
    for o, d, rgb in ((None, p, p), (p, None, p), (p, p, None)):
        assert call(P.handle, o, d, None, 1, 0, rgb) == -1 and "null" in last_error()
    assert call(P.handle, p, p, None, 1, -1, p) == -1 and "row_width" in last_error()
    assert call(P.handle, p, p, None, (1 << 28) + 1, 0, p) == -1 and "2^28" in last_error()
    assert call(P.handle, None, None, None, 0, 0, None) == 0
    assert call(P.handle, p, p, None, 0, 5, p) == 0
    raw = L.mrt_scene_create()   # no BVH yet
    try:
        assert call(raw, p, p, None, 1, 0, p) == -5 and "not built" in last_error()
    finally:
        L.mrt_scene_destroy(raw)


def test_camera_rays_rejects_null_outputs_and_bad_sizes():
    L = miro.lib()
    c = camera(CAM)._c()
    o, d, t = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), np.zeros(4, np.float32)
    po, pd, pt = o.ctypes.data, d.ctypes.data, t.ctypes.data
    assert L.mrt_camera_rays(C.byref(c), 2, 2, 0, po, pd, pt) == 0
    assert L.mrt_camera_rays(None, 2, 2, 0, po, pd, pt) == -1 and last_error()
    for a in ((None, pd, pt), (po, None, pt), (po, pd, None)):
        assert L.mrt_camera_rays(C.byref(c), 2, 2, 0, *a) == -1
    for w, h in ((0, 2), (2, 0), (-1, 2), (2, -3)):
        assert L.mrt_camera_rays(C.byref(c), w, h, 0, po, pd, pt) == -1
    with pytest.raises(miro.MRTError):
        camera(CAM).rays(0, 4)


def test_pinhole_rays_start_at_the_eye_with_times_in_the_shutter_interval():
    shutter = 0.25
    o, d, t = camera(dict(CAM, shutterSpeed=shutter)).rays(W, H, seed=3)
    assert o.shape == (H, W, 3) and d.shape == (H, W, 3) and t.shape == (H, W)
    assert np.array_equal(bits(o), bits(np.broadcast_to(np.asarray(CAM["eye"], np.float32), o.shape)))
    assert t.min() >= 1.0 - shutter and t.max() <= 1.0 and t.std() > 0
    assert np.allclose(np.linalg.norm(d, axis=-1), 1.0, atol=1e-6)
    assert np.all(d[..., 2] < 0)   # looking down -z
    # the centre column looks straight ahead in x; rows are bottom to top
    assert d[0, W // 2, 1] < 0 < d[H - 1, W // 2, 1] and abs(d[H // 2, W // 2, 0]) < 1e-6


def test_lens_rays_start_within_the_aperture_and_follow_the_seed():
    ap = 0.3
    cam = camera(dict(CAM, aperture=ap, focusPlane=7.0))
    o, d, t = cam.rays(W, H, seed=7)
    off = o - np.asarray(CAM["eye"], np.float32)
    # u = +x, v = +y, w = +z for this camera: the lens lies in the u/v plane
    assert np.abs(off[..., 2]).max() == 0
    r = np.hypot(off[..., 0], off[..., 1])
    assert 0 < r.max() <= ap * (1 + 1e-6) and r.std() > 0
    o2, d2, t2 = cam.rays(W, H, seed=7)
    assert np.array_equal(bits(o), bits(o2)) and np.array_equal(bits(d), bits(d2)) and np.array_equal(bits(t), bits(t2))
    o3, _, _ = cam.rays(W, H, seed=8)
    assert not np.array_equal(bits(o), bits(o3))
    # every lens ray passes through its pixel's focal point: the pinhole ray at the focus distance
    _, dp, _ = camera(CAM).rays(W, H, seed=7)
    focal = np.asarray(CAM["eye"], np.float32) + 7.0 * dp
    to = focal - o
    assert np.allclose(to / np.linalg.norm(to, axis=-1, keepdims=True), d, atol=1e-5)


# ------------------------------------------------------------------ GPU: scenes, one per dispatch path
BLINN = dict(kind="blinn", kd=(0.8, 0.5, 0.25), specExp=10.0, specAmt=0.4)
MIXED = dict(kind="blinn", kd=(0.6, 0.5, 0.4), ks=(0.9, 0.8, 0.7), reflectAmt=0.6, refractAmt=0.7, ior=1.33,
             specExp=12.0, specAmt=0.2)
PRISM = dict(kind="blinn", kd=(0.2, 0.3, 0.3), reflectAmt=1.0, refractAmt=1.0, specExp=30.0,
             disperse=True, ior3=(1.57, 1.60, 1.62))
RECT = dict(type="rect", v1=(3.0, 5.4, -2.5), v2=(3.0, 5.4, -3.0), v3=(2.5, 5.4, -2.5), power=15.0, samples=3,
            noise=0.001)
POINT = dict(type="point", pos=(2.75, 2.0, -2.75), power=20.0)


def quad(z=1.0, lo=0.5, hi=5.0):
    v = np.array([[lo, lo, z], [hi, lo, z], [hi, hi, z], [lo, hi, z]], np.float32)
    n = np.tile(np.array([[0, 0, 1]], np.float32), (4, 1))
    idx = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    return v, n, idx, idx.copy()


def cornell(material=None, cam=CAM, **kw):
    cfg = dict(scenes.CONFIGS["C1"])
    if material:
        cfg["material"] = material
    P, _, _ = scene_pair(cfg, meshes=[fixture_mesh("cornell_box")], **kw)
    return P, cam


def point_light_scene():
    """One point light, Blinn (specExp != 1) walls and a Lambert sheet: the two-kernel path."""
    return cornell(BLINN, extra=[(quad(z=-3.0, lo=1.5, hi=4.0), dict(kind="lambert", kd=(0.3, 0.6, 0.8)))])


def dome_scene():
    """Dome light + environment map, seen from far enough that rays pass the box and miss."""
    cfg = dict(scenes.CONFIGS["C1"], material=BLINN, env=dict(sky=(64, 32), exposure=1.5),
               lights=[dict(type="dome", sky=(64, 32), power=0.15, samples=3, noise=0.001)])
    P, _, _ = scene_pair(cfg, meshes=[fixture_mesh("cornell_box")])
    return P, dict(CAM, eye=(2.75, 2.75, 16.0))


def instanced_scene():
    from test_instancing import CAM as ICAM, instanced_pair
    return instanced_pair("blinn", spec=(8.0, 0.3))[0], ICAM


def alpha_scene():
    from test_textures import leaves_scene
    return leaves_scene()[0], CAM


def motion_scene(walls=None, ball_mat=None):
    from test_motion_blur import BALL, moved, sphere
    ball = sphere()
    P, _ = cornell(walls, moving=[(ball, moved(ball), ball_mat or BALL)])
    return P, dict(CAM, shutterSpeed=1.0)


CASES = {
    "point_light": point_light_scene,
    "rect_paths": lambda: cornell(BLINN, lights=[RECT, POINT], num_paths=3),
    "dome_env": dome_scene,
    "instanced": instanced_scene,
    "alpha_map": alpha_scene,
    "motion_blur": motion_scene,
    "depth_of_field": lambda: cornell(BLINN, cam=dict(CAM, aperture=0.3, focusPlane=7.0), lights=[RECT]),
    "reflect_refract": lambda: cornell(MIXED, lights=[RECT, POINT], num_paths=2),
    "path_trace": lambda: cornell(dict(kind="blinn", kd=(0.7, 0.6, 0.5)), lights=[POINT], path_trace=(3, False),
                                  num_paths=2),
    "dispersion": lambda: cornell(None, extra=[(quad(), PRISM)]),
    # a moving ball between reflecting / refracting walls: the chain engine's rays below the
    # caller's ray inherit its time
    "motion_blur_chain": lambda: motion_scene(MIXED, dict(kind="blinn", kd=(0.2, 0.3, 0.3), reflectAmt=1.0, ior=1.8)),
}
CHAIN_CASES = ("reflect_refract", "path_trace", "dispersion", "motion_blur_chain")
RAY_COUNTS = ("primary_rays", "shadow_rays", "secondary_rays", "primary_hits")


def frame(P, cam, w, h, seed):
    img = miro.Image()
    img.resize(w, h)
    hits = P.raytraceImage(camera(cam), img, want_hits=True, seed=seed)
    return img.rgb.copy(), hits, dict(P.last_stats)


def assert_same_hits(a, b):
    for k in ("t", "a", "b"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert np.array_equal(a["prim"], b["prim"]) and np.array_equal(a["inst"], b["inst"])


def assert_rays_equal_frame(P, cam, seed, chain=None, **kw):
    rgb, hits, st = frame(P, cam, W, H, seed)
    out, rh = P.sampleRays(*camera(cam).rays(W, H, seed), seed=seed, want_hits=True, **kw)
    rs = dict(P.last_stats)
    assert out.shape == (H, W, 3) and rh.shape == (H, W)
    assert np.array_equal(bits(out), bits(rgb)), "float RGB differs from the frame"
    assert_same_hits(rh, hits)
    for k in RAY_COUNTS:
        assert rs[k] == st[k], (k, rs[k], st[k])
    assert rs["primary_rays"] == W * H and rs["fused"] == 0
    assert rs["chain"] == st["chain"]
    if chain is not None:
        assert rs["chain"] == chain
    return rgb, hits, rs


@pytest.mark.gpu
def test_camera_rays_are_the_eye_rays_by_an_independent_route():
    """mrt_trace and the oracle's trace on Camera.rays() of a static scene agree bit for
    bit, and both equal the oracle render's primary hit records."""
    need_gpu()
    P, Osc, cam = scene_pair(dict(scenes.CONFIGS["C1"], material=BLINN), meshes=[fixture_mesh("cornell_box")],
                             extra=[(quad(z=-3.0, lo=1.5, hi=4.0), dict(kind="lambert", kd=(0.3, 0.6, 0.8)))])
    cam = dict(CAM, eye=(2.75, 2.75, 16.0))   # some rays miss
    o, d, _ = camera(cam).rays(W, H)
    got = P.traceBatch(o, d, 0.001, 1e12)
    ref = Osc.trace(o, d, 0.001, 1e12)[0]
    ren = Osc.render(cam, W, H)["hits"].reshape(-1)
    assert np.array_equal(got["prim"], ref["prim"]) and np.array_equal(got["prim"], ren["prim"])
    hit = got["prim"] >= 0
    assert 0 < hit.sum() < hit.size
    for k in ("t", "a", "b"):
        assert np.array_equal(bits(got[k][hit]), bits(ref[k][hit])), k
        assert np.array_equal(bits(got[k][hit]), bits(ren[k][hit])), k


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_camera_rays_shade_to_the_frame(case):
    """sampleRays on the camera's own rays = raytraceImage, rgb / hits / ray counts, on
    every dispatch path; the chain cases also with a scratch budget that forces chunks."""
    need_gpu()
    P, cam = CASES[case]()
    chain = 1 if case in CHAIN_CASES else None
    _, hits, st = assert_rays_equal_frame(P, cam, 11, chain=chain)
    if case == "dome_env":
        assert 0 < (hits["prim"] < 0).sum() < hits.size
    if case == "instanced":
        assert (hits["inst"] >= 0).sum() > 20
    if case in ("rect_paths", "reflect_refract", "path_trace"):
        assert st["shadow_rays"] > W * H
    if chain:
        assert st["secondary_rays"] > 0
        with tuned(chain_mb=1, chain_est=0):   # worst-case level capacities in a 1-MB budget: several chunks
            _, _, many = assert_rays_equal_frame(P, cam, 11, chain=1)
        assert many["chain_chunks"] > 1


@pytest.mark.gpu
def test_fused_chain_shading_and_the_chunk_fallback_shade_rays_too():
    """The engine's other routes for secondary rays: the fused chain kernel (tuning chain 0)
    and the fallback of a chunk that outgrew its estimated capacity."""
    need_gpu()
    P, cam = CASES["reflect_refract"]()
    ref, _, _ = assert_rays_equal_frame(P, cam, 5, chain=1)
    with tuned(chain=0):
        fused, _, _ = assert_rays_equal_frame(P, cam, 5, chain=0)
    assert np.array_equal(bits(fused), bits(ref))
    o, d, t = camera(cam).rays(W, H, 5)
    with tuned(chain_est=1):
        P.sampleRays(o, d, t, seed=5)   # seeds this stream's estimates
        P.sampleRays(o, d, t, seed=5)
        with tuned(chain_est_pct=1):
            fb = P.sampleRays(o, d, t, seed=5)
            assert P.last_stats["chain_fallbacks"] >= 1
    assert np.array_equal(bits(fb), bits(ref))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["point_light", "path_trace"])
def test_results_do_not_depend_on_the_layout(case):
    """row_width 0 / 37 / 64 / 5 and a flat (n, 3) array give the same bits; so do the
    n = 1 and n = 63 prefixes: ray i keys the RNG by i, whatever the batch around it."""
    need_gpu()
    P, cam = CASES[case]()
    o, d, t = camera(cam).rays(W, H, 9)
    ref, rhits = P.sampleRays(o, d, t, seed=9, want_hits=True)
    fo, fd, ft = o.reshape(-1, 3), d.reshape(-1, 3), t.reshape(-1)
    for rw in (0, 37, 64, 5):
        out, hits = P.sampleRays(o, d, t, seed=9, want_hits=True, row_width=rw)
        assert np.array_equal(bits(out), bits(ref)), rw
        assert_same_hits(hits, rhits)
        out = P.sampleRays(fo, fd, ft, seed=9, row_width=rw)
        assert out.shape == (W * H, 3) and np.array_equal(bits(out), bits(ref.reshape(-1, 3))), rw
    out = P.sampleRays(fo, fd, ft, seed=9)   # a flat array: row_width 0
    assert np.array_equal(bits(out), bits(ref.reshape(-1, 3)))
    for n in (1, 63):
        out, hits = P.sampleRays(fo[:n], fd[:n], ft[:n], seed=9, want_hits=True)
        assert out.shape == (n, 3) and np.array_equal(bits(out), bits(ref.reshape(-1, 3)[:n])), n
        assert_same_hits(hits, rhits.reshape(-1)[:n])
        assert P.last_stats["primary_rays"] == n


THREE_CAMS = [CAM, dict(CAM, eye=(1.0, 4.0, 4.0), lookAt=(3.5, 2.0, -3.0)),
              dict(CAM, eye=(4.5, 1.0, 3.0), lookAt=(1.5, 3.0, -4.0))]
# Blinn::shade's Russian roulette reads the RNG whenever 0 < Rs * reflectAmt < 1.  With this
# reflectAmt both of its tests are decided without the draw: rrWeight = 1 - Rs * reflectAmt < 0
# and reflectAmt * Rs > 1 for every Rs >= 1e-8 -- and Rs >= 0.04 from air into ior 1.5 -- so
# every hit of it reflects and no result depends on a ray's RNG key.
ALWAYS_MIRROR = dict(kind="blinn", kd=(0.6, 0.5, 0.4), specExp=10.0, specAmt=0.4, reflectAmt=1e9, ior=1.5)
SHEET = quad(z=-3.0, lo=1.5, hi=4.0)


@pytest.mark.gpu
@pytest.mark.parametrize("sheet,chain", [(dict(kind="lambert", kd=(0.3, 0.6, 0.8)), 0), (ALWAYS_MIRROR, 1)])
def test_rays_no_camera_can_make(sheet, chain):
    """The rays of three cameras, concatenated and permuted, on deterministic scenes (one
    point light; Blinn walls around a Lambert sheet, or around a Blinn sheet with a
    reflection every hit takes, no gloss): the shading reads no RNG key that matters, so
    each output is the matching pixel of that camera's own frame."""
    need_gpu()
    P, _ = cornell(BLINN, extra=[(SHEET, sheet)])
    n = 16
    frames = [frame(P, c, n, n, 0) for c in THREE_CAMS]
    rays = [camera(c).rays(n, n) for c in THREE_CAMS]
    o = np.concatenate([r[0].reshape(-1, 3) for r in rays])
    d = np.concatenate([r[1].reshape(-1, 3) for r in rays])
    t = np.concatenate([r[2].reshape(-1) for r in rays])
    want = np.concatenate([f[0].reshape(-1, 3) for f in frames])
    whits = np.concatenate([f[1].reshape(-1) for f in frames])
    perm = np.random.default_rng(4).permutation(len(o))
    out, hits = P.sampleRays(o[perm], d[perm], t[perm], want_hits=True)
    assert P.last_stats["chain"] == chain and (P.last_stats["secondary_rays"] > 0) == bool(chain)
    assert len(np.unique(bits(want), axis=0)) > 100   # not a flat image
    assert np.array_equal(bits(out), bits(want[perm]))
    assert_same_hits(hits, whits[perm])


@pytest.mark.gpu
def test_rays_of_mixed_cameras_keep_their_index_keys():
    """Stochastic shading too: ray i of the batch is pixel i of one of three cameras, picked
    per ray.  Its RNG key is its index either way, so it shades to that camera's pixel i
    (rectangle light, reflection / refraction roulette, two paths)."""
    need_gpu()
    P, _ = CASES["reflect_refract"]()
    n = 16
    frames = [frame(P, c, n, n, 13) for c in THREE_CAMS]
    rays = [camera(c).rays(n, n, 13) for c in THREE_CAMS]
    pick = np.random.default_rng(8).integers(0, 3, n * n)
    idx = np.arange(n * n)
    o = np.stack([r[0].reshape(-1, 3) for r in rays])[pick, idx]
    d = np.stack([r[1].reshape(-1, 3) for r in rays])[pick, idx]
    t = np.stack([r[2].reshape(-1) for r in rays])[pick, idx]
    want = np.stack([f[0].reshape(-1, 3) for f in frames])[pick, idx]
    whits = np.stack([f[1].reshape(-1) for f in frames])[pick, idx]
    out, hits = P.sampleRays(o, d, t, seed=13, want_hits=True)
    assert len(set(pick)) == 3 and P.last_stats["chain"] == 1
    assert np.array_equal(bits(out), bits(want))
    assert_same_hits(hits, whits)


@pytest.mark.gpu
def test_no_time_array_is_time_zero():
    need_gpu()
    P, cam = CASES["motion_blur"]()
    o, d, t = camera(cam).rays(W, H, 2)
    a, ha = P.sampleRays(o, d, None, seed=2, want_hits=True)
    b, hb = P.sampleRays(o, d, np.zeros_like(t), seed=2, want_hits=True)
    c, hc = P.sampleRays(o, d, t, seed=2, want_hits=True)
    assert np.array_equal(bits(a), bits(b))
    assert_same_hits(ha, hb)
    assert not np.array_equal(ha["prim"], hc["prim"])   # the ball is elsewhere at the camera's times


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rect_paths", "instanced"])
def test_device_tensors_on_a_side_stream_equal_the_host_call(case):
    """torch device tensors go through mrt_sample_rays_async on the current stream."""
    need_gpu()
    import torch
    P, cam = CASES[case]()
    o, d, t = camera(cam).rays(W, H, 6)
    ref, rhits = P.sampleRays(o, d, t, seed=6, want_hits=True)
    dev = torch.device("cuda", P.device)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        to, td, tt = (torch.from_numpy(x).to(dev) for x in (o, d, t))
        rgb, hits = P.sampleRays(to, td, tt, seed=6, want_hits=True)
        flat = P.sampleRays(to.reshape(-1, 3), td.reshape(-1, 3), None, seed=6)
    side.synchronize()
    assert rgb.shape == (H, W, 3) and np.array_equal(bits(rgb.cpu().numpy()), bits(ref))
    h = hits.cpu().numpy()
    fr = rhits.reshape(-1)
    for i, k in enumerate(("t", "a", "b")):
        assert np.array_equal(h[:, i].view(np.uint32), bits(fr[k]))
    assert np.array_equal(h[:, 3], fr["prim"]) and np.array_equal(h[:, 4], fr["inst"])
    assert flat.shape == (W * H, 3)
    assert P.stats()["primary_rays"] == W * H
