"""The samples behind Light::sampleLight at caller points (mrt_light_samples /
mrt_light_samples_async, mrt_scene_light_sample_cap; miro.Scene.lightSamples / lightSampleCap).

The yardsticks are the existing query, mrt_sample_lights (pinned to mrt_shade_hits, the oracle
and the reference by tests/test_sample_lights.py), and mrt_trace_rays' any-hit bit.  The scenes,
the 37 x 29 points (the mrt_hit_surfaces records of the camera's own rays) and their cache are
that file's.  All value comparisons are on float bits.  CPU tests cover the exports, the
argument checks, the three refusals, the sample caps and the wrapper's shape checks."""
import ctypes

import numpy as np
import pytest

import miro
from helpers import bits, tuned
from test_sample_lights import (BLOCKS_PER_CU, H, KWG, POINT, RECT, W, WHITE, blinn_frame, cornell, dot, last_error,
                                need_gpu, point_light_by_hand, scene, surfaces, whitened)
from test_sample_rays import dome_scene

F = np.float32
REC = miro.LIGHT_SAMPLE_DTYPE
NAN_WORD = 0x7FC12345   # a quiet NaN no kernel writes: the prefill of rows that must survive
# a rectangle light whose noise threshold cuts the loop short inside the box: E / k < 0.1 after
# k samples at distances above 6.9 (k = 1) and 4.9 (k = 2); RECT's own 0.001 never cuts there
RECT_CUT = dict(RECT, noise=0.1)
_extra = {}


def scene2(name):
    """test_sample_lights' scenes, and "rect_cut" ([RECT_CUT, POINT] over the same box)."""
    if name != "rect_cut":
        return scene(name)
    if name not in _extra:
        _extra[name] = cornell(WHITE, lights=[RECT_CUT, POINT])
    return _extra[name]


def points(name, seed=11):
    """(p, n, rvec, t, hit mask) of the scene's camera rays, flat."""
    (o, d, t), _, surf, hit = surfaces("rect_point" if name == "rect_cut" else name, seed)
    n, rvec = blinn_frame(d, surf["n"], surf["geo_n"])
    flat = lambda x: np.ascontiguousarray(x.reshape(-1, 3))
    return flat(surf["p"]), flat(n), flat(rvec), np.ascontiguousarray(t.reshape(-1)), hit.reshape(-1)


def words(rec):
    """A record array as uint32 words, (..., 8)."""
    return np.ascontiguousarray(rec).view(np.uint32).reshape(rec.shape + (8,))


def same(a, b):
    """Two lightSamples results: the same keys, every array equal on its bits."""
    assert a.keys() == b.keys()
    for k in a:
        x, y = (words(v[k]) if v[k].dtype == REC else np.ascontiguousarray(v[k]).view(np.uint32) for v in (a, b))
        if not np.array_equal(x, y):
            return False
    return True


def light_kinds(P):
    return [type(l).__name__ for l in P._lights]


# ------------------------------------------------------------------ CPU: exports, checks, refusals, caps
def test_the_three_symbols_are_exported_and_wrapped():
    L = miro.lib()
    for name in ("mrt_light_samples", "mrt_light_samples_async", "mrt_scene_light_sample_cap"):
        assert name in miro._lib.EXPORTS and hasattr(L, name)
        assert getattr(L, name).argtypes is not None
    assert len(L.mrt_light_samples_async.argtypes) == len(L.mrt_light_samples.argtypes) + 1 == 15
    assert L.mrt_abi_version() == 10
    assert callable(miro.Scene.lightSamples) and callable(miro.Scene.lightSampleCap)
    assert REC.itemsize == 32 and REC.names == ("dir", "dist", "e", "vis")


def transparent_box():
    return cornell(WHITE, lights=[dict(RECT, fast_shadows=False)])[0]


@pytest.mark.parametrize("entry", ["mrt_light_samples", "mrt_light_samples_async"])
def test_argument_checks_and_refusals_come_before_any_device_call(entry):
    """Bad arguments and the three refusals give MRT_ERR_INVALID with their own mrt_last_error
    text before a device is touched (this runs on a host without one); n == 0 is MRT_OK and
    writes nothing."""
    L = miro.lib()
    P, _ = cornell(WHITE, lights=[RECT, POINT])
    buf = np.full(64, 7.0, F)
    p = buf.ctypes.data
    tail = (None,) if entry.endswith("async") else ()

    def call(handle, frm, nrm, outs, n):
        return getattr(L, entry)(handle, frm, nrm, None, None, n, 0, 0, 0, 0, *outs, *tail)

    every = (p, p, p, p)
    assert call(None, p, p, every, 1) == -1 and "null scene" in last_error()
    for frm, nrm in ((None, p), (p, None)):
        assert call(P.handle, frm, nrm, every, 1) == -1 and "null" in last_error()
    assert call(P.handle, p, p, (None, None, None, None), 1) == -1 and "null output" in last_error()
    assert call(P.handle, p, p, every, (1 << 28) + 1) == -1 and "2^28" in last_error()
    assert call(P.handle, None, None, (None, None, None, None), 0) == 0
    assert call(P.handle, p, p, every, 0) == 0 and np.all(buf == 7.0)
    raw = L.mrt_scene_create()   # no BVH yet
    try:
        assert call(raw, p, p, every, 1) == -5 and "not built" in last_error()
    finally:
        L.mrt_scene_destroy(raw)
    # the refusals: a transparent-shadow light, M = 65, n * M = 2^32
    for single in ((p, None, None, None), (None, p, None, None), (None, None, p, None), (None, None, None, p), every):
        assert call(transparent_box().handle, p, p, single, 1) == -1 and "transparent" in last_error()
    many, _ = cornell(WHITE, lights=[dict(RECT, samples=64), POINT])
    assert many.lightSampleCap()[1] == 65
    assert call(many.handle, p, p, every, 1) == -1 and "64" in last_error()
    sixteen, _ = cornell(WHITE, lights=[dict(RECT, samples=16)])
    assert call(sixteen.handle, p, p, every, 1 << 28) == -1 and "2^32" in last_error()
    assert np.all(buf == 7.0)


def test_light_sample_cap_per_light_and_in_total():
    L = miro.lib()
    P, _ = cornell(WHITE, lights=[RECT, POINT])
    for secondary in (False, True):   # a rectangle light does not look at isSecondary
        per, total = P.lightSampleCap(secondary)
        assert per.dtype == np.int32 and per.tolist() == [3, 1] and total == 4
    D, _ = dome_scene()
    assert D.lightSampleCap()[0].tolist() == [3] and D.lightSampleCap()[1] == 3
    assert D.lightSampleCap(secondary=True)[0].tolist() == [1] and D.lightSampleCap(True)[1] == 1
    none, _ = cornell(WHITE, lights=[])
    assert none.lightSampleCap()[1] == 0
    zero, _ = cornell(WHITE, lights=[dict(RECT, samples=0)])   # the do-while takes one sample
    assert zero.lightSampleCap()[0].tolist() == [1]
    # either output alone; a null scene and an unbuilt one
    total = ctypes.c_int32(-1)
    assert L.mrt_scene_light_sample_cap(P.handle, 0, None, ctypes.byref(total)) == 0 and total.value == 4
    assert L.mrt_scene_light_sample_cap(P.handle, 0, None, None) == 0
    assert L.mrt_scene_light_sample_cap(None, 0, None, ctypes.byref(total)) == -1 and "null scene" in last_error()
    raw = L.mrt_scene_create()
    try:
        assert L.mrt_scene_light_sample_cap(raw, 0, None, ctypes.byref(total)) == -5
    finally:
        L.mrt_scene_destroy(raw)


def test_wrapper_refuses_bad_shapes_and_sample_arrays():
    import torch
    P, _ = cornell(WHITE, lights=[RECT, POINT])
    a = np.zeros((4, 3), F)
    bad = (((a, a[:3]), {}), ((a, np.zeros((4, 2), F)), {}), ((a, a), dict(rvec=a[:3])),
           ((a, a), dict(time=np.zeros(3, F))), ((a, a), dict(rvec=torch.zeros(4, 3))),
           ((a, a), dict(samples=False, counts=False)),                      # nothing asked for
           ((a, a), dict(samples=np.zeros((4, 3), REC))),                     # M is 4
           ((a, a), dict(samples=np.zeros((4, 4, 8), F))),                    # not the record type
           ((a, a), dict(samples=np.zeros((4, 8), REC)[:, ::2])),             # strided
           ((torch.zeros(4, 3), torch.zeros(4, 3)), {}))                      # host tensors
    for args, kw in bad:
        with pytest.raises(miro.MRTError):
            P.lightSamples(*args, **kw)


# ------------------------------------------------------------------ GPU 1: the numbers of the existing query
@pytest.mark.gpu
@pytest.mark.parametrize("seed", [11, 5])
@pytest.mark.parametrize("name", ["point", "rect_point", "dome", "instanced", "alpha_map", "motion_blur"])
def test_e_per_light_and_shadow_rays_equal_sample_lights(name, seed):
    need_gpu()
    P, _ = scene(name)
    p, n, rvec, t, hit = points(name, seed)
    for first_draw in (0, 1):
        e, per = P.sampleLights(p, n, rvec, time=t, seed=seed, first_draw=first_draw, per_light=True)
        want = dict(P.last_stats)
        got = P.lightSamples(p, n, rvec, time=t, seed=seed, first_draw=first_draw, e=True, per_light=True)
        st = dict(P.last_stats)
        assert np.array_equal(bits(got["e"]), bits(e)), (name, first_draw)
        assert np.array_equal(bits(got["per_light"]), bits(per)), (name, first_draw)
        assert st["shadow_rays"] == want["shadow_rays"] > 0
        assert st["primary_rays"] == 0 and st["kernel_ms"] > 0
        assert np.any(e[hit] > 0) and np.any(per[hit][..., 3] != 0)


@pytest.mark.gpu
def test_secondary_equals_sample_lights_on_the_dome_scene():
    need_gpu()
    P, _ = scene("dome")
    p, n, rvec, t, hit = points("dome")
    e, per = P.sampleLights(p, n, rvec, time=t, seed=8, secondary=True, per_light=True)
    want = P.last_stats["shadow_rays"]
    got = P.lightSamples(p, n, rvec, time=t, seed=8, secondary=True, e=True, per_light=True)
    assert P.last_stats["shadow_rays"] == want > 0
    assert np.array_equal(bits(got["e"]), bits(e)) and np.array_equal(bits(got["per_light"]), bits(per))
    assert got["samples"].shape == (W * H, 1) and got["counts"].max() == 1


# ------------------------------------------------------------------ GPU 2: the records add up
def sums_of_records(rec, counts, caps):
    """Per point and light, in float32: acc = 0; acc += e_j * vis_j in order; times
    float32(1) / float32(count) -- count 0 gives zeros, a point light's one sample e_0 * vis_0."""
    n, nl = counts.shape
    out = np.zeros((n, nl, 3), F)
    start = np.cumsum(counts, 1) - counts
    rows = np.arange(n)
    for l in range(nl):
        acc = np.zeros((n, 3), F)
        for j in range(caps[l]):
            on = j < counts[:, l]
            r = rec[rows, np.minimum(start[:, l] + j, rec.shape[1] - 1)]
            term = (r["e"] * r["vis"][:, None]).astype(F)
            acc = np.where(on[:, None], (acc + term).astype(F), acc)
        recip = (F(1) / np.maximum(counts[:, l], 1).astype(F)).astype(F)
        out[:, l] = (acc * recip[:, None]).astype(F)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rect_point", "rect_cut", "dome", "instanced"])
def test_the_records_of_a_light_sum_to_its_e(name):
    """rect_point's noise threshold (0.001) cannot cut a loop inside the box -- E / 3 is above
    0.02 at every point of it -- so the case "fewer samples than the cap" is asserted on
    rect_cut, the same scene with the threshold at 0.1, which gets every check rect_point
    gets; the rejected sample (dist = 0) is asserted on both."""
    need_gpu()
    P, _ = scene2(name)
    p, n, rvec, t, hit = points(name)
    caps, m = P.lightSampleCap()
    got = P.lightSamples(p, n, rvec, time=t, seed=3, e=True, per_light=True)
    rec, counts = got["samples"], got["counts"]
    assert rec.shape == (W * H, m) and counts.shape == (W * H, len(caps))
    assert np.all(counts >= 0) and np.all(counts <= caps[None, :])
    want = sums_of_records(rec, counts, caps)
    assert np.array_equal(bits(want), bits(got["per_light"][..., :3]))
    assert np.any(want > 0)
    if name in ("rect_point", "rect_cut"):
        total = counts.sum(1)
        live = np.arange(m)[None, :] < total[:, None]
        assert np.any(live & (rec["dist"] == 0)), "no rejected rectangle sample"
        assert np.all(rec["vis"][live & (rec["dist"] == 0)] == 0)
        fewer = int((counts[:, 0] < caps[0]).sum())
        print(name, "points with fewer rectangle samples than the cap:", fewer)
        if name == "rect_cut":
            assert fewer > 20 and np.all(counts[:, 0] >= 1)
            # and the existing query agrees on that scene too
            e, per = P.sampleLights(p, n, rvec, time=t, seed=3, per_light=True)
            assert np.array_equal(bits(per), bits(got["per_light"])) and np.array_equal(bits(e), bits(got["e"]))
    if name == "dome":
        assert np.all(rec["dist"][np.arange(m)[None, :] < counts.sum(1)[:, None]] == F(1e12))


# ------------------------------------------------------------------ GPU 3: the records are the rays
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rect_point", "dome", "instanced", "alpha_map", "motion_blur"])
def test_vis_is_the_any_hit_answer_of_the_recorded_ray(name):
    """Every sample with dist > 0 (every light of these scenes casts shadows): vis = 1 - the
    any-hit bit of the ray (p, dir, time) over [0.001, tmax], tmax = dist for a point light,
    float32(dist) - float32(0.001) for a rectangle light, 1e12 for a dome light."""
    need_gpu()
    P, _ = scene(name)
    assert all(l.castShadows for l in P._lights)
    p, n, rvec, t, hit = points(name)
    caps, m = P.lightSampleCap()
    got = P.lightSamples(p, n, rvec, time=t, seed=11)
    rec, counts = got["samples"], got["counts"]
    # the light of every row: light l's rows of point i are [start, start + counts)
    light = np.full((W * H, m), -1, np.int32)
    start = np.cumsum(counts, 1) - counts
    for l in range(len(caps)):
        for j in range(caps[l]):
            on = j < counts[:, l]
            light[np.arange(W * H)[on], start[on, l] + j] = l
    pick = (light >= 0) & (rec["dist"] > 0)
    assert pick.sum() > 200
    i, _ = np.nonzero(pick)
    r, l = rec[pick], light[pick]
    kinds = np.array(light_kinds(P))[l]
    tmax = np.where(kinds == "PointLight", r["dist"], np.where(kinds == "RectangleLight", r["dist"] - F(0.001), F(1e12))).astype(F)
    occl = P.traceRays(p[i], np.ascontiguousarray(r["dir"]), t[i], tmin=0.001, tmax=tmax, any_hit=True)["prim"] == 1
    assert np.array_equal(r["vis"], np.where(occl, F(0), F(1)))
    assert occl.sum() > 20 and (~occl).sum() > 20
    assert P.lightSamples(p, n, rvec, time=t, seed=11, samples=False)["counts"].shape == counts.shape
    assert P.last_stats["shadow_rays"] == pick.sum()
    assert set(np.unique(rec["vis"][light >= 0])) <= {F(0), F(1)}


@pytest.mark.gpu
def test_the_point_lights_record_equals_its_restatement():
    """dir, dist and e of a point light's one sample against src/PointLight.cpp:18-36 in float32
    (point_light_by_hand without shadows gives A * nDotL; L and distance restated beside it)."""
    need_gpu()
    light = dict(POINT)
    P, _ = scene("point")
    p, n, rvec, t, hit = points("point")
    n = n.copy()
    n[::3] = -n[::3]   # a third of the points face away from where they did
    E, spec, lit = point_light_by_hand(P, light, p, n, rvec, cast_shadows=False)
    L = (np.asarray(light["pos"], F) - p).astype(F)
    safe = np.where(lit, dot(L, L), F(1))
    dr = np.array([miro.rsqrt_nr(float(x)) for x in safe], F)
    dist = np.array([miro.rcp_nr(float(x)) for x in dr], F)
    L = (L * dr[:, None]).astype(F)
    got = P.lightSamples(p, n, rvec, time=t, per_light=True)
    rec, counts = got["samples"][:, 0], got["counts"][:, 0]
    assert (~lit).sum() > 50 and lit.sum() > 200
    assert np.array_equal(counts, lit.astype(np.int32))
    assert np.array_equal(bits(rec["dir"][lit]), bits(L[lit])) and np.array_equal(bits(rec["dist"][lit]), bits(dist[lit]))
    assert np.array_equal(bits(rec["e"][lit]), bits(np.repeat(E[lit, None], 3, 1)))
    assert not np.any(words(rec)[~lit])   # (the wrapper's zeros: no row was written)
    # and with the answers, the light's E and outSpec
    Es, specs, _ = point_light_by_hand(P, light, p, n, rvec, cast_shadows=True)
    assert np.array_equal(bits(got["per_light"][:, 0, 0]), bits(Es)) and np.array_equal(bits(got["per_light"][:, 0, 3]), bits(specs))
    assert np.array_equal(rec["vis"][lit] == 0, (Es[lit] == 0))


# ------------------------------------------------------------------ GPU 4: layout
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rect_cut", "rect_point"])
def test_rows_past_a_points_count_are_not_written(name):
    """`samples` prefilled with a NaN pattern: the rows past a point's count keep it, the rows
    before it hold no NaN.  A quarter of the points get a zero normal, where the point light
    takes nothing (and the rectangle light's samples are all rejected, yet counted)."""
    need_gpu()
    P, _ = scene2(name)
    p, n, rvec, t, hit = points(name)
    m = P.lightSampleCap()[1]
    mine = np.zeros((W * H, m), REC)
    words_of_mine = mine.view(np.uint32).reshape(W * H, m, 8)
    words_of_mine[...] = NAN_WORD
    zero_n = n.copy()
    zero_n[1::4] = 0
    got = P.lightSamples(p, zero_n, rvec, time=t, seed=9, samples=mine)
    assert got["samples"] is mine
    total = got["counts"].sum(1)
    live = np.arange(m)[None, :] < total[:, None]
    assert (~live).sum() > 50 and live.sum() > 200
    assert np.all(words_of_mine[~live] == NAN_WORD)
    assert not np.any(np.isnan(words_of_mine[live].view(F)))
    fresh = P.lightSamples(p, zero_n, rvec, time=t, seed=9)
    assert np.array_equal(words(fresh["samples"])[live], words_of_mine[live])
    assert not np.any(words(fresh["samples"])[~live])


@pytest.mark.gpu
def test_a_point_light_without_shadows_is_visible_and_traces_nothing():
    need_gpu()
    P, _ = cornell(WHITE, lights=[dict(POINT, cast_shadows=False)])
    p, n, rvec, t, hit = points("point")
    got = P.lightSamples(p, n, rvec, time=t, e=True)
    assert P.last_stats["shadow_rays"] == 0
    took = got["counts"][:, 0] == 1
    assert took.sum() > 200 and np.all(got["samples"]["vis"][took, 0] == 1)
    assert np.array_equal(bits(got["e"]), bits(P.sampleLights(p, n, rvec, time=t)))


# ------------------------------------------------------------------ GPU 5: schedules and batch sizes
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dome", "instanced"])
def test_bins_and_shadow_schedules_change_no_bit(name):
    need_gpu()
    P, _ = scene(name)
    p, n, rvec, t, hit = points(name)
    ref = rays = None
    for binned in (0, 1):
        for sched in (0, 1, 2):
            with tuned(bin=binned, shadow_sched=sched):
                got = P.lightSamples(p, n, rvec, time=t, seed=7, e=True, per_light=True)
                st = P.last_stats["shadow_rays"]
            if ref is None:
                ref, rays = got, st
            assert same(got, ref) and st == rays > 0, (binned, sched)
    assert np.any(ref["e"] > 0)


@pytest.mark.gpu
def test_every_batch_is_a_prefix_of_the_longest():
    """n = 1, 63, 64, 65, kWG - 1, kWG, kWG + 1 and grid x kWG + 77 points (the 37 x 29 points,
    tiled): a chunk's last lanes, a band's cut chunk, fewer workgroups than the bands need (the
    grid-stride launch), more than the grid holds.  A point's results depend on its index alone."""
    need_gpu()
    import torch
    P, _ = scene("rect_point")
    p0, n0, rvec0, t0, hit = points("rect_point")
    cus = torch.cuda.get_device_properties(P.device).multi_processor_count
    longest = cus * BLOCKS_PER_CU * KWG + 77
    reps = -(-longest // (W * H))
    p, n, rvec = (np.ascontiguousarray(np.tile(x, (reps, 1))[:longest]) for x in (p0, n0, rvec0))
    full = P.lightSamples(p, n, rvec, seed=2, e=True, per_light=True)
    rays = P.last_stats["shadow_rays"]
    assert full["e"].shape == (longest, 3) and full["samples"].shape == (longest, 4)
    e, per = P.sampleLights(p, n, rvec, seed=2, per_light=True)
    assert P.last_stats["shadow_rays"] == rays
    assert np.array_equal(bits(e), bits(full["e"])) and np.array_equal(bits(per), bits(full["per_light"]))
    # (the rectangle light draws: a tile does not repeat the first)
    assert not np.array_equal(bits(full["e"][:W * H]), bits(full["e"][W * H:2 * W * H]))
    for k in (1, 63, 64, 65, KWG - 1, KWG, KWG + 1, 3 * KWG + 65):
        got = P.lightSamples(p[:k], n[:k], rvec[:k], seed=2, e=True, per_light=True)
        assert same(got, {key: v[:k] for key, v in full.items()}), k


# ------------------------------------------------------------------ GPU 6: inputs and modes
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rect_point", "instanced"])
def test_device_tensors_on_a_side_stream_equal_the_host_call(name):
    need_gpu()
    import torch
    P, _ = scene(name)
    p, n, rvec, t, hit = points(name)
    m = P.lightSampleCap()[1]
    ref = P.lightSamples(p, n, rvec, time=t, seed=6, first_draw=1, e=True, per_light=True)
    ref_rays = P.last_stats["shadow_rays"]
    dev = torch.device("cuda", P.device)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        tp, tn, tr, tt = (torch.from_numpy(x).to(dev) for x in (p, n, rvec, t))
        got = P.lightSamples(tp, tn, tr, time=tt, seed=6, first_draw=1, e=True, per_light=True)
    side.synchronize()
    assert P.stats()["shadow_rays"] == ref_rays and P.stats()["primary_rays"] == 0
    assert got["samples"].shape == (W * H, m, 8) and got["samples"].dtype == torch.float32
    assert got["counts"].shape == (W * H, len(P._lights)) and got["counts"].dtype == torch.int32
    assert np.array_equal(got["samples"].cpu().numpy().view(np.uint32), words(ref["samples"]))
    assert np.array_equal(got["counts"].cpu().numpy(), ref["counts"])
    assert np.array_equal(bits(got["e"].cpu().numpy()), bits(ref["e"]))
    assert np.array_equal(bits(got["per_light"].cpu().numpy()), bits(ref["per_light"]))
    with pytest.raises(miro.MRTError):   # a strided view is refused, not copied
        P.lightSamples(tp[:, ::2], tn[:, ::2])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rect_point", "dome"])
def test_any_single_output_equals_that_output_of_the_full_call(name):
    need_gpu()
    P, _ = scene(name)
    p, n, rvec, t, hit = points(name)
    full = P.lightSamples(p, n, rvec, time=t, seed=4, e=True, per_light=True)
    for key in ("samples", "counts", "e", "per_light"):
        only = dict(samples=False, counts=False, e=False, per_light=False)
        only[key] = True
        got = P.lightSamples(p, n, rvec, time=t, seed=4, **only)
        assert list(got) == [key] and same(got, {key: full[key]}), key


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rect_point", "instanced"])
def test_count_mode_gives_the_same_bits_and_fills_the_visit_counters(name):
    need_gpu()
    P, _ = scene(name)
    p, n, rvec, t, hit = points(name)
    ref = P.lightSamples(p, n, rvec, time=t, seed=4, e=True, per_light=True)
    plain = dict(P.last_stats)
    got = P.lightSamples(p, n, rvec, time=t, seed=4, e=True, per_light=True, count_visits=True)
    st = dict(P.last_stats)
    assert same(got, ref)
    assert st["shadow_rays"] == plain["shadow_rays"] > 0
    assert st["node_visits"] > 0 and st["leaf_visits"] > 0
    assert plain["node_visits"] == 0 and plain["leaf_visits"] == 0


@pytest.mark.gpu
def test_a_scene_without_lights_writes_a_zero_e():
    need_gpu()
    P, _ = cornell(WHITE, lights=[])
    p, n, rvec, t, hit = points("point")
    got = P.lightSamples(p, n, rvec, time=t, e=True, per_light=True)
    assert got["samples"].shape == (W * H, 0) and got["counts"].shape == (W * H, 0)
    assert got["per_light"].shape == (W * H, 0, 4) and got["e"].shape == (W * H, 3)
    e = np.full((W * H, 3), 7.0, F)   # through the C ABI: the zeros are written, not the wrapper's
    L = miro.lib()
    assert L.mrt_light_samples(P.handle, p.ctypes.data, n.ctypes.data, None, None, len(p), 0, 0, 0, 0, None, None,
                               e.ctypes.data, None) == 0
    assert not np.any(bits(e)) and not np.any(bits(got["e"]))
    assert P.stats()["shadow_rays"] == 0
