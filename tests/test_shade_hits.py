"""Shade caller-supplied hits (mrt_shade_hits), the timed trace (mrt_trace_rays) and their
argument / record checks; miro.Scene.traceRays / shadeHits.  The surface query has its own
file, tests/test_hit_surfaces.py.

The defining property: for the rays of mrt_camera_rays, the closest hits of
mrt_trace_rays(o, d, time, tmin = 0.001, tmax = 1e12) are the hit records of mrt_sample_rays
byte for byte, and mrt_shade_hits on them is its float RGB bit for bit, with the same ray
counts -- on every dispatch path of the engine, the scene list of tests/test_sample_rays.py.
CPU tests cover the argument checks of all six entries, those the older mrt_trace pair keeps,
and the host validation of hit records.  Frames are 37 x 29: neither 8, 64 nor a row width
divides evenly.  One GPU test holds every synchronous entry against its async twin."""
import ctypes as C

import numpy as np
import pytest

import miro
from helpers import bits, camera, fixture_mesh, scene_pair, tuned
from miro import scenes
from test_sample_rays import CAM, CASES, CHAIN_CASES, H, W

COUNTS = ("primary_rays", "shadow_rays", "secondary_rays", "primary_hits")
INT32_MAX = 2 ** 31 - 1


def need_gpu():
    if miro.device_count() < 1:
        pytest.fail("no HIP device visible (GPU tests must run on the MI355X box)")


def last_error():
    return miro.lib().mrt_last_error().decode()


# ------------------------------------------------------------------ CPU: argument checks
def built_scene():
    P, _, _ = scene_pair(dict(scenes.CONFIGS["C1"]), meshes=[fixture_mesh("cornell_box")])
    return P


def entry_call(entry):
    """call(scene, o, d, hits / bounds / out pointers..., n, row_width): the entry with every
    other argument at a harmless value.  The four array slots (o, d, third, out) are what
    the null checks cover; `third` is the hit array, or tmin and tmax for the trace."""
    L = miro.lib()
    f = getattr(L, entry)
    tail = (None,) if entry.endswith("async") else ()
    if entry.startswith("mrt_trace_rays"):
        return lambda s, o, d, third, out, n, rw=0: f(s, o, d, None, third, third, n, 0, out, *tail)
    if entry.startswith("mrt_shade_hits"):
        return lambda s, o, d, third, out, n, rw=0: f(s, o, d, None, third, n, rw, 0, 0, out, *tail)
    return lambda s, o, d, third, out, n, rw=0: f(s, o, d, third, n, out, *tail)


ENTRIES = ["mrt_trace_rays", "mrt_trace_rays_async", "mrt_shade_hits", "mrt_shade_hits_async", "mrt_hit_surfaces",
           "mrt_hit_surfaces_async"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_checks_come_before_any_device_call(entry):
    """All six entries reject bad arguments with the error code and mrt_last_error set, before
    touching a device (this runs on a host without one); n == 0 is MRT_OK."""
    L = miro.lib()
    P = built_scene()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    call = entry_call(entry)
    assert call(None, p, p, p, p, 1) == -1 and "null scene" in last_error()
    for a in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert call(P.handle, *a, 1) == -1 and "null" in last_error(), a
    if "shade_hits" in entry:
        assert call(P.handle, p, p, p, p, 1, -1) == -1 and "row_width" in last_error()
    assert call(P.handle, p, p, p, p, (1 << 28) + 1) == -1 and "2^28" in last_error()
    assert call(P.handle, None, None, None, None, 0) == 0
    assert call(P.handle, p, p, p, p, 0, 5) == 0
    raw = L.mrt_scene_create()   # no BVH yet
    try:
        assert call(raw, p, p, p, p, 1) == -5 and "not built" in last_error()
    finally:
        L.mrt_scene_destroy(raw)


@pytest.mark.parametrize("entry", ["mrt_trace", "mrt_trace_async"])
def test_untimed_trace_keeps_its_own_argument_checks(entry):
    """mrt_trace / mrt_trace_async, the older pair: "bad argument" for a null scene or array, no
    2^28 cap (such a batch passes the checks and, on a host without a device, stops at the
    upload), and n == 0 still asks for the replica first: "not built" on an unbuilt scene."""
    L = miro.lib()
    P = built_scene()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    f = getattr(L, entry)
    tail = (None,) if entry.endswith("async") else ()

    def call(s, o, d, tmin, tmax, out, n):
        if not tail:   # mrt_trace declares its four inputs float*
            o, d, tmin, tmax = (x and C.cast(x, C.POINTER(C.c_float)) for x in (o, d, tmin, tmax))
        return f(s, o, d, tmin, tmax, n, 0, out, *tail)

    assert call(None, p, p, p, p, p, 1) == -1 and last_error() == "bad argument"
    for k in range(5):
        a = [p] * 5
        a[k] = None
        L.mrt_scene_upload(None, 0)   # another text in between: "null scene"
        assert call(P.handle, *a, 1) == -1 and last_error() == "bad argument", k
    raw = L.mrt_scene_create()   # no BVH yet
    try:
        for n in (0, 1):
            assert call(raw, p, p, p, p, p, n) == -5 and "not built" in last_error(), n
        assert call(raw, None, None, None, None, None, 0) == -5 and "not built" in last_error()
    finally:
        L.mrt_scene_destroy(raw)
    if miro.device_count() < 1:   # past the checks: the next stop is the device
        assert call(P.handle, p, p, p, p, p, (1 << 28) + 1) == -7 and "no HIP device" in last_error()
        assert call(P.handle, None, None, None, None, None, 0) == -7


# ------------------------------------------------------------------ CPU: the host validation of hit records
def instanced_world():
    """(scene, hit-id count, the ProxyObject's own world slot): a floor triangle (world
    object 0), then one instance of the teapot (world slot 1, BLAS objects from id 2)."""
    from test_instancing import instanced_pair, rot_y
    P, _ = instanced_pair(transforms=[rot_y(0, 1.0, (0, 0, 0))])
    n_world = P.bvh_info["prims"]
    assert n_world == 2 and P.primObject(1)[2] == 0 and P.primObject(0)[2] == -1
    n_blas = len(fixture_mesh("teapot")[2])
    assert P.primObject(n_world + n_blas - 1)[2] == 0
    with pytest.raises(miro.MRTError):
        P.primObject(n_world + n_blas)
    return P, n_world + n_blas, 1


def record(t=1.0, a=0.25, b=0.25, prim=0, inst=-1):
    h = np.zeros(1, miro.HIT_DTYPE)
    h[0] = (t, a, b, prim, inst)
    return h


@pytest.mark.parametrize("entry", ["mrt_shade_hits", "mrt_hit_surfaces"])
def test_synchronous_entries_refuse_bad_hit_records_on_the_host(entry):
    """prim = -2, the hit-id count, INT32_MAX, an instance's own proxy slot, NaN t and infinite
    a: MRT_ERR_INVALID with the record's index in mrt_last_error, before any device call (this
    runs without a device: a valid batch goes on to the device and fails there instead)."""
    L = miro.lib()
    P, n_ids, proxy_slot = instanced_world()
    good = [record(prim=0), record(prim=-1, t=np.nan), record(prim=n_ids - 1), record(prim=2, inst=77)]
    bad = {"prim = -2": record(prim=-2), "prim = the hit-id count": record(prim=n_ids),
           "prim = INT32_MAX": record(prim=INT32_MAX), "the proxy's own slot": record(prim=proxy_slot),
           "NaN t": record(t=np.nan), "infinite a": record(a=np.inf), "-infinite b": record(b=-np.inf),
           "NaN b": record(b=np.nan), "a past 2^24": record(a=2.0 ** 25)}
    o = np.zeros((8, 3), np.float32)
    out = np.zeros(8 * 21, np.float32)

    def call(h):
        n = len(h)
        if entry == "mrt_shade_hits":
            return L.mrt_shade_hits(P.handle, o.ctypes.data, o.ctypes.data, None, h.ctypes.data, n, 0, 0, 0,
                                    out.ctypes.data)
        return L.mrt_hit_surfaces(P.handle, o.ctypes.data, o.ctypes.data, h.ctypes.data, n, out.ctypes.data)

    for what, rec in bad.items():
        for at in (0, 3):   # alone, and behind valid records: the first bad index is named
            h = np.concatenate(good[:at] + [rec])
            assert call(h) == -1, what
            assert "hit record %d:" % at in last_error(), (what, last_error())
    if miro.device_count() < 1:   # valid records pass the host check: the next stop is the device
        assert call(np.concatenate(good)) == -7


def test_python_wrappers_check_shapes_and_hit_arrays():
    P = built_scene()
    o = np.zeros((4, 3), np.float32)
    with pytest.raises(miro.MRTError):
        P.traceRays(o, o[:3])
    with pytest.raises(miro.MRTError):
        P.shadeHits(o, o, np.zeros(3, miro.HIT_DTYPE))
    with pytest.raises(miro.MRTError):
        P.shadeHits(o, o, np.zeros((4, 5), np.int32))
    with pytest.raises(miro.MRTError):
        P.hitSurfaces(o, o, np.zeros(5, miro.HIT_DTYPE))
    with pytest.raises(miro.MRTError):
        P.shadeHits(o, o, np.zeros(4, miro.HIT_DTYPE), time=np.zeros(3, np.float32))
    assert miro.SURFACE_DTYPE.itemsize == C.sizeof(miro._lib.mrt_surface) == 84


# ------------------------------------------------------------------ GPU: the defining identity
def reference(P, cam, seed, **kw):
    """(rays, rgb, hit records, statistics) of mrt_sample_rays on the camera's rays."""
    o, d, t = camera(cam).rays(W, H, seed)
    rgb, hits = P.sampleRays(o, d, t, seed=seed, want_hits=True, **kw)
    return (o, d, t), rgb, hits, dict(P.last_stats)


def assert_trace_then_shade_is_sample_rays(P, cam, seed, row_widths=(None, 0, 5), chain=None):
    (o, d, t), rgb, rhits, rs = reference(P, cam, seed)
    hits = P.traceRays(o, d, t)   # tmin 0.001, tmax 1e12, closest hit
    assert hits.shape == (H, W) and hits.tobytes() == rhits.tobytes(), "traced hits differ from the sampled records"
    for rw in row_widths:   # None: the rays' row width, 37
        out = P.shadeHits(o, d, hits, t, seed=seed, row_width=rw)
        st = dict(P.last_stats)
        assert out.shape == (H, W, 3) and np.array_equal(bits(out), bits(rgb)), ("float RGB differs", rw)
        for k in COUNTS:
            assert st[k] == rs[k], (k, rw, st[k], rs[k])
        assert st["fused"] == 0 and st["chain"] == rs["chain"]
        if rw is None:   # the same work items: the same chunks
            assert st["chain_chunks"] == rs["chain_chunks"]
        if chain is not None:
            assert st["chain"] == chain
    return rgb, rhits, rs


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_trace_then_shade_equals_sample_rays(case):
    """One scene per dispatch path, at row_width 37 / 0 / 5."""
    need_gpu()
    P, cam = CASES[case]()
    chain = 1 if case in CHAIN_CASES else None
    _, hits, st = assert_trace_then_shade_is_sample_rays(P, cam, 11, chain=chain)
    if case == "dome_env":
        assert 0 < (hits["prim"] < 0).sum() < hits.size
    if case == "instanced":
        assert (hits["inst"] >= 0).sum() > 20
    if chain:
        assert st["secondary_rays"] > 0
    assert st["primary_hits"] == (hits["prim"] >= 0).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CHAIN_CASES)
@pytest.mark.parametrize("route", ["chunks", "fused"])
def test_chain_cases_in_chunks_and_through_the_fused_chain_kernel(case, route):
    need_gpu()
    P, cam = CASES[case]()
    ref, _, _ = assert_trace_then_shade_is_sample_rays(P, cam, 11, row_widths=(None,), chain=1)
    if route == "chunks":   # worst-case level capacities in a 1-MB budget: several chunks
        with tuned(chain_mb=1, chain_est=0):
            got, _, st = assert_trace_then_shade_is_sample_rays(P, cam, 11, row_widths=(None, 0), chain=1)
            assert st["chain_chunks"] > 1   # (of the rays' own row width, which shadeHits matched)
    else:
        with tuned(chain=0):
            got, _, _ = assert_trace_then_shade_is_sample_rays(P, cam, 11, row_widths=(None, 0), chain=0)
    assert np.array_equal(bits(got), bits(ref))


@pytest.mark.gpu
def test_chunk_fallback_shades_supplied_hits_too():
    """A chunk that outgrows its estimated level capacity is rendered by the fallback."""
    need_gpu()
    P, cam = CASES["reflect_refract"]()
    (o, d, t), ref, hits, _ = reference(P, cam, 5)
    with tuned(chain_est=1):
        P.shadeHits(o, d, hits, t, seed=5)   # seeds this stream's estimates
        P.shadeHits(o, d, hits, t, seed=5)
        with tuned(chain_est_pct=1):
            fb = P.shadeHits(o, d, hits, t, seed=5)
            assert P.last_stats["chain_fallbacks"] >= 1
    assert np.array_equal(bits(fb), bits(ref))


# ------------------------------------------------------------------ GPU: the timed trace
@pytest.mark.gpu
def test_timed_trace_finds_the_moving_cannonball_where_sample_rays_does():
    """The reference's own MBObject pair (tests/golden/cannonball_mb.npz) under a full shutter:
    with the camera's times the trace equals the sampled hit records; without a time array it
    is mrt_trace, and the ball is elsewhere for some rays."""
    need_gpu()
    from test_motion_blur import BALL_CAM, N_GROUND, cannonball
    P, _, _ = cannonball()
    cam = dict(BALL_CAM, shutterSpeed=1.0)   # times over [0, 1]: the ball's whole path
    (o, d, t), _, rhits, _ = reference(P, cam, 3)
    timed = P.traceRays(o, d, t)
    assert timed.tobytes() == rhits.tobytes()
    assert (timed["prim"] >= N_GROUND).sum() > 20   # the ball is in view
    static = P.traceRays(o, d, None)
    plain = P.traceBatch(o, d, 0.001, 1e12).reshape(H, W)
    assert static.tobytes() == plain.tobytes()
    differ = (static["prim"] != timed["prim"]) | (bits(static["t"]) != bits(timed["t"]))
    assert differ.sum() >= 1
    # any-hit with a time: the occlusion flag of the same rays
    occl = P.traceRays(o, d, t, any_hit=True)
    assert np.array_equal(occl["prim"] == 1, timed["prim"] >= 0) and set(np.unique(occl["prim"])) <= {-1, 1}


# ------------------------------------------------------------------ GPU: hits the library did not make
def background_scene():
    """A background colour and no environment map, seen from where rays pass the box."""
    cfg = dict(scenes.CONFIGS["C1"], bg=(0.25, 0.5, 0.75))
    P, _, _ = scene_pair(cfg, meshes=[fixture_mesh("cornell_box")])
    return P, dict(CAM, eye=(2.75, 2.75, 16.0))


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["dome_env", "background"])
def test_a_miss_record_takes_the_colour_of_its_rays_direction(scene):
    """Slots of rays that hit are given a miss record and the direction of a ray that misses:
    they return that ray's mrt_sample_rays colour (the environment lookup of the direction,
    or the background), whatever the rest of the batch holds."""
    need_gpu()
    P, cam = CASES["dome_env"]() if scene == "dome_env" else background_scene()
    (o, d, t), ref, hits, _ = reference(P, cam, 7)
    fo, fd, ft, fh, fr = o.reshape(-1, 3), d.reshape(-1, 3), t.reshape(-1), hits.reshape(-1).copy(), ref.reshape(-1, 3)
    miss, hit = np.flatnonzero(fh["prim"] < 0), np.flatnonzero(fh["prim"] >= 0)
    assert len(miss) > 20 and len(hit) > 20
    take = hit[:: max(1, len(hit) // 16)]
    src = miss[np.arange(len(take)) * 7 % len(miss)]
    d2, want = fd.copy(), fr.copy()
    d2[take] = fd[src]
    fh["prim"][take] = -1
    fh["t"][take] = np.nan   # a miss record's t, a, b are not read
    want[take] = fr[src]
    out = P.shadeHits(fo, d2, fh, ft, seed=7)
    assert np.array_equal(bits(out), bits(want))
    if scene == "background":
        assert np.array_equal(out[take], np.broadcast_to(np.float32([0.25, 0.5, 0.75]), (len(take), 3)))
    else:   # the environment's colour along the borrowed directions, not the shaded hits'
        assert not np.any(np.all(bits(out[take]) == bits(fr[take]), axis=-1))
    assert P.last_stats["primary_hits"] == len(hit) - len(take)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["point_light", "path_trace"])
def test_prefixes_return_the_prefix_of_the_full_result(case):
    need_gpu()
    P, cam = CASES[case]()
    (o, d, t), ref, hits, _ = reference(P, cam, 9)
    fo, fd, ft, fh, fr = o.reshape(-1, 3), d.reshape(-1, 3), t.reshape(-1), hits.reshape(-1), ref.reshape(-1, 3)
    for n in (1, 63):
        out = P.shadeHits(fo[:n], fd[:n], fh[:n], ft[:n], seed=9)
        assert out.shape == (n, 3) and np.array_equal(bits(out), bits(fr[:n])), n
        assert P.last_stats["primary_rays"] == n
        assert P.last_stats["primary_hits"] == (fh[:n]["prim"] >= 0).sum()


# ------------------------------------------------------------------ GPU: the async entries
def hit_tensor(hits, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(hits).reshape(-1).view(np.int32).reshape(-1, 5)).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rect_paths", "instanced"])
def test_device_tensors_on_a_side_stream_equal_the_host_calls(case):
    """traceRays, shadeHits and hitSurfaces from torch tensors on a side stream."""
    need_gpu()
    import torch
    P, cam = CASES[case]()
    (o, d, t), ref, rhits, _ = reference(P, cam, 6)
    surf = P.hitSurfaces(o, d, rhits)
    dev = torch.device("cuda", P.device)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        to, td, tt = (torch.from_numpy(x).to(dev) for x in (o, d, t))
        th = P.traceRays(to, td, tt)
        rgb = P.shadeHits(to, td, th, tt, seed=6)
        ts = P.hitSurfaces(to, td, th)
    side.synchronize()
    assert th.cpu().numpy().tobytes() == rhits.tobytes()
    assert rgb.shape == (H, W, 3) and np.array_equal(bits(rgb.cpu().numpy()), bits(ref))
    assert ts.shape == (W * H, 21) and ts.cpu().numpy().tobytes() == surf.tobytes()


@pytest.mark.gpu
def test_async_bad_ids_are_shaded_as_misses_and_reported_by_last_stats():
    """Two bad ids in an otherwise valid batch: mrt_scene_last_stats returns MRT_ERR_INVALID,
    their slots hold the miss colour, every other slot is unchanged.  (Validation by
    comparison: the bad ids -- INT32_MAX and a negative one -- are never used as an index.)"""
    need_gpu()
    import torch
    P, cam = background_scene()
    (o, d, t), ref, hits, _ = reference(P, cam, 4)
    fh = hits.reshape(-1).copy()
    hit = np.flatnonzero(fh["prim"] >= 0)
    bad = hit[[3, len(hit) // 2]]
    fh["prim"][bad[0]] = INT32_MAX
    fh["prim"][bad[1]] = -7
    dev = torch.device("cuda", P.device)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        to, td, tt = (torch.from_numpy(x.reshape(-1, *x.shape[2:])).to(dev) for x in (o, d, t))
        rgb = P.shadeHits(to, td, hit_tensor(fh, dev), tt, seed=4)
    side.synchronize()
    st = miro._lib.mrt_stats()
    assert miro.lib().mrt_scene_last_stats(P.handle, C.byref(st)) == -1 and "2 invalid hit record" in last_error()
    assert st.primary_hits == len(hit) - 2
    want = ref.reshape(-1, 3).copy()
    want[bad] = np.float32([0.25, 0.5, 0.75])
    assert np.array_equal(bits(rgb.cpu().numpy()), bits(want))
    # the surface query reports the same way and writes its miss rows
    with torch.cuda.stream(side):
        ts = P.hitSurfaces(to, td, hit_tensor(fh, dev))
    side.synchronize()
    assert miro.lib().mrt_scene_last_stats(P.handle, C.byref(st)) == -1 and "2 invalid hit record" in last_error()
    s = ts.cpu().numpy().view(miro.SURFACE_DTYPE).reshape(-1)
    good = P.hitSurfaces(o, d, hits).reshape(-1)
    keep = np.ones(len(s), bool)
    keep[bad] = False
    assert s[keep].tobytes() == good[keep].tobytes()
    assert np.all(s[bad]["mesh"] == -1) and not np.any(s[bad]["p"]) and np.all(s[bad]["material"] == -1)
    # a valid batch afterwards is MRT_OK again
    with torch.cuda.stream(side):
        P.shadeHits(to, td, hit_tensor(hits, dev), tt, seed=4)
    side.synchronize()
    assert miro.lib().mrt_scene_last_stats(P.handle, C.byref(st)) == 0


@pytest.mark.gpu
def test_every_synchronous_entry_equals_its_async_twin():
    """The five host-array entries against their device-array twins, bit for bit, with and
    without a time array, at n = 1 and n = 65: one ray more than a 64-ray work item, an odd
    tail of the 256-thread record kernels."""
    need_gpu()
    import torch
    L = miro.lib()
    P = built_scene()
    dev = torch.device("cuda", P.device)
    ro, rd, rt = (x.reshape(-1, *x.shape[2:]) for x in camera(dict(CAM, shutterSpeed=0.25)).rays(W, H, 9))
    for n in (1, 65):
        o, d = np.ascontiguousarray(ro[:n]), np.ascontiguousarray(rd[:n])
        to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        # mrt_trace has no tensor wrapper: its twin through the C ABI, on the current stream
        lo, hi = torch.full((n,), 0.001, device=dev), torch.full((n,), 1e12, device=dev)
        out = torch.empty((n, 5), dtype=torch.int32, device=dev)
        assert L.mrt_trace_async(P.handle, to.data_ptr(), td.data_ptr(), lo.data_ptr(), hi.data_ptr(), n, 0,
                                 out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream) == 0
        plain = P.traceBatch(o, d)
        assert out.cpu().numpy().tobytes() == plain.tobytes(), n
        for t in (None, np.ascontiguousarray(rt[:n])):
            tt = None if t is None else torch.from_numpy(t).to(dev)
            what = (n, t is not None)
            hits = P.traceRays(o, d, t)
            th = P.traceRays(to, td, tt)
            assert th.cpu().numpy().tobytes() == hits.tobytes(), what
            if t is None:
                assert hits.tobytes() == plain.tobytes(), n
            rgb, shits = P.sampleRays(o, d, t, seed=9, want_hits=True)
            assert P.stats()["primary_rays"] == n, what
            trgb, tshits = P.sampleRays(to, td, tt, seed=9, want_hits=True)
            assert np.array_equal(bits(trgb.cpu().numpy()), bits(rgb)), what
            assert tshits.cpu().numpy().tobytes() == shits.tobytes() == hits.tobytes(), what
            assert P.stats()["primary_rays"] == n, what
            shaded = P.shadeHits(o, d, hits, t, seed=9)
            assert P.stats()["primary_rays"] == n and np.array_equal(bits(shaded), bits(rgb)), what
            tshaded = P.shadeHits(to, td, th, tt, seed=9)
            assert np.array_equal(bits(tshaded.cpu().numpy()), bits(shaded)), what
            assert P.stats()["primary_rays"] == n, what
        surf = P.hitSurfaces(o, d, plain)
        tsurf = P.hitSurfaces(to, td, hit_tensor(plain, dev))
        assert surf.shape == (n,) and tsurf.cpu().numpy().tobytes() == surf.tobytes(), n
