"""Light::sampleLight at caller points (mrt_sample_lights / mrt_sample_lights_async;
miro.Scene.sampleLights).

The yardstick is mrt_shade_hits, which is pinned to the oracle and the reference: on the
points and normals mrt_hit_surfaces gives for a camera's rays, `e` is the float RGB a white
Lambert surface (kd = 1, ka = 0) gets there, and sum_l E_l * spec_l is what a Blinn surface
of ks = 1, specAmt = 1, specExp = 1 gets, bit for bit.  The scenes are those of
tests/test_sample_rays.py with every material replaced (rematerial: the geometry, the
lights and the alpha maps -- what casts shadows -- stay).  Frames are 37 x 29.  CPU tests
cover the exports, the argument checks and the wrapper's shape checks."""
import numpy as np
import pytest

import miro
from helpers import bits, camera
from test_sample_rays import H, POINT, RECT, W, alpha_scene, cornell, dome_scene, instanced_scene, motion_scene, quad

F = np.float32
KWG = 256            # csrc/mrt_kernels.h kWG: threads per workgroup
BLOCKS_PER_CU = 8    # csrc/mrt_shader.h kMaxBlocksPerCU: the launch grid's upper bound per CU
WHITE = dict(kind="lambert", kd=(1, 1, 1))


def need_gpu():
    if miro.device_count() < 1:
        pytest.fail("no HIP device visible (GPU tests must run on the MI355X box)")


def last_error():
    return miro.lib().mrt_last_error().decode()


# ------------------------------------------------------------------ CPU: exports, argument checks, shapes
def test_both_symbols_are_exported_and_wrapped():
    L = miro.lib()
    for name in ("mrt_sample_lights", "mrt_sample_lights_async"):
        assert name in miro._lib.EXPORTS and hasattr(L, name)
        assert getattr(L, name).argtypes is not None
    assert len(L.mrt_sample_lights_async.argtypes) == len(L.mrt_sample_lights.argtypes) + 1 == 13
    assert L.mrt_abi_version() == 10
    assert callable(miro.Scene.sampleLights)


@pytest.mark.parametrize("entry", ["mrt_sample_lights", "mrt_sample_lights_async"])
def test_argument_checks_come_before_any_device_call(entry):
    """Bad arguments give the error code with mrt_last_error set before a device is touched
    (this runs on a host without one); n == 0 is MRT_OK and writes nothing."""
    L = miro.lib()
    P, _ = cornell()
    buf = np.full(64, 7.0, F)
    p = buf.ctypes.data
    tail = (None,) if entry.endswith("async") else ()

    def call(scene, frm, nrm, e, per, n):
        return getattr(L, entry)(scene, frm, nrm, None, None, n, 0, 0, 0, 0, e, per, *tail)

    assert call(None, p, p, p, p, 1) == -1 and "null scene" in last_error()
    for frm, nrm in ((None, p), (p, None)):
        assert call(P.handle, frm, nrm, p, p, 1) == -1 and "null" in last_error()
    assert call(P.handle, p, p, None, None, 1) == -1 and "null" in last_error()
    assert call(P.handle, p, p, p, p, (1 << 28) + 1) == -1 and "2^28" in last_error()
    assert call(P.handle, None, None, None, None, 0) == 0
    assert call(P.handle, p, p, p, p, 0) == 0 and np.all(buf == 7.0)
    raw = L.mrt_scene_create()   # no BVH yet
    try:
        assert call(raw, p, p, p, p, 1) == -5 and "not built" in last_error()
    finally:
        L.mrt_scene_destroy(raw)


def test_wrapper_refuses_mismatched_shapes_and_tensors_that_are_not_float32():
    import torch
    P, _ = cornell()
    a = np.zeros((4, 3), F)
    for args, kw in (((a, a[:3]), {}), ((a, np.zeros((4, 2), F)), {}), ((a, a), dict(rvec=a[:3])),
                     ((a, a), dict(time=np.zeros(3, F))), ((a, a), dict(rvec=torch.zeros(4, 3)))):
        with pytest.raises(miro.MRTError):
            P.sampleLights(*args, **kw)
    t = torch.zeros((4, 3), dtype=torch.float64)   # (a host tensor is refused the same way)
    with pytest.raises(miro.MRTError):
        P.sampleLights(t, t)
    with pytest.raises(miro.MRTError):
        P.sampleLights(torch.zeros(4, 3), torch.zeros(4, 3))


# ------------------------------------------------------------------ scenes
def rematerial(P, make):
    """Every material of the built scene P replaced by make(old) (one new material per old
    one), the hierarchy rebuilt: the same geometry and lights."""
    new = {}

    def swap(m):
        if id(m) not in new:
            new[id(m)] = make(m)
        return new[id(m)]
    seen = set()
    for k, ent in enumerate(P._meshes):
        if ent[1] is None:   # a ProxyObject: its shared Objects list, once
            objs = ent[0].objects
            if id(objs) not in seen:
                seen.add(id(objs))
                objs[:] = [(mesh, swap(m)) for mesh, m in objs]
        else:
            P._meshes[k] = (ent[0], swap(ent[1])) + tuple(ent[2:])
    P.preCalc()
    return P


def white(old):
    """Lambert kd = 1, ka = 0; an alpha map stays (it decides what the surface occludes)."""
    m = miro.Lambert(miro.Vector3(1))
    if getattr(old, "alphaMap", None) is not None:
        m.setAlphaMap(old.alphaMap)
    return m


def mirror(old):
    """Blinn kd = ka = 0, ks = 1, specAmt = 1, specExp = 1, no optics: rgb = sum_l E_l * spec_l."""
    return miro.Blinn(miro.Vector3(0), ka=miro.Vector3(0), ks=miro.Vector3(1), specExp=1.0, specAmt=1.0)


GLASS = dict(kind="blinn", kd=(0.3, 0.4, 0.5), refractAmt=0.6, ior=1.3)


def transparent_scene():
    """A rectangle light with transparent shadows over a white Cornell box, and a Blinn sheet of
    refractAmt 0.6 (z = -2, facing the camera) between the light and the front of the floor."""
    return cornell(WHITE, lights=[dict(RECT, fast_shadows=False)], extra=[(quad(z=-2.0, lo=0.5, hi=5.0), GLASS)])


def whitened(build):
    P, cam = build()
    return rematerial(P, white), cam


SCENES = {
    "point": lambda: cornell(WHITE, lights=[POINT]),
    "rect_point": lambda: cornell(WHITE, lights=[RECT, POINT]),
    "dome": lambda: whitened(dome_scene),
    "instanced": lambda: whitened(instanced_scene),
    "alpha_map": lambda: whitened(alpha_scene),
    "motion_blur": lambda: whitened(motion_scene),
    "transparent": transparent_scene,
}
_built = {}


def scene(name):
    """One scene per name for the whole module (they are never changed after the build)."""
    if name not in _built:
        _built[name] = SCENES[name]()
    return _built[name]


_surfaces = {}


def surfaces(name, seed):
    """((o, d, t), hits, surface records, hit mask) of the camera's own rays, computed once."""
    if (name, seed) not in _surfaces:
        P, cam = scene(name)
        o, d, t = camera(cam).rays(W, H, seed)
        hits = P.traceRays(o, d, t)
        _surfaces[name, seed] = ((o, d, t), hits, P.hitSurfaces(o, d, hits), hits["prim"] >= 0)
    return _surfaces[name, seed]


# ------------------------------------------------------------------ GPU 1: the Lambert identity
@pytest.mark.gpu
@pytest.mark.parametrize("seed", [11, 5])
@pytest.mark.parametrize("name", list(SCENES))
def test_e_is_the_white_lambert_shading_of_the_same_points(name, seed):
    """e = shadeHits' rgb at every hit row, bit for bit, and the same shadow_rays.  All W * H
    points are passed, so point i keeps ray i's RNG stream; a miss row's point and normal are
    the zeros mrt_hit_surfaces writes, and they take part in no comparison of values.
    shadow_rays: a zero normal makes a point or rectangle light trace nothing (nDotL is not
    positive), so the counts are equal; a dome light does not look at the point before it
    samples -- a zero normal rejects no direction -- so each miss row there traces its 1 to
    `samples` rays, which shadeHits does not: the count lies in that range above shadeHits',
    and the dome scene is shaded once more with a hit row's surface lent to every miss row,
    so that no row misses and the counts are equal."""
    need_gpu()
    P, cam = scene(name)
    (o, d, t), hits, surf, hit = surfaces(name, seed)
    rgb = P.shadeHits(o, d, hits, time=t, seed=seed)
    want = P.last_stats["shadow_rays"]
    e = P.sampleLights(surf["p"], surf["n"], time=t, seed=seed)
    got = dict(P.last_stats)
    assert e.shape == (H, W, 3) and hit.sum() > 50
    rows = hit
    if name == "transparent":   # the sheet's own rows are Blinn: compare the white Lambert's
        rows = hit & (surf["material"] == 0)   # (the configuration's material is the scene's first)
        assert 0 < (hit & ~rows).sum() and rows.sum() > 50
        assert got["shadow_rays"] > 0
    assert np.array_equal(bits(e[rows]), bits(rgb[rows])), "e differs from the Lambert shading"
    assert np.any(e[rows] > 0)
    assert got["primary_rays"] == 0 and got["kernel_ms"] > 0
    n_miss = int((~hit).sum())
    if name == "dome":
        samples = 3
        assert n_miss > 20 and want + n_miss <= got["shadow_rays"] <= want + samples * n_miss
        # every miss row given the ray, time and hit record of one hit row (its own index, so
        # its own draws): no row misses, and the counts are equal under the dome light too
        donor = tuple(np.argwhere(hit)[len(np.argwhere(hit)) // 2])
        o2, d2, t2, h2 = o.copy(), d.copy(), t.copy(), hits.copy()
        o2[~hit], d2[~hit], t2[~hit], h2[~hit] = o[donor], d[donor], t[donor], hits[donor]
        surf2 = P.hitSurfaces(o2, d2, h2)
        rgb2 = P.shadeHits(o2, d2, h2, time=t2, seed=seed)
        want2 = P.last_stats["shadow_rays"]
        e2 = P.sampleLights(surf2["p"], surf2["n"], time=t2, seed=seed)
        assert np.array_equal(bits(e2), bits(rgb2)) and P.last_stats["shadow_rays"] == want2 >= W * H
    elif name != "transparent":
        assert got["shadow_rays"] == want, (got["shadow_rays"], want)
    if name == "instanced":
        assert (hits["inst"] >= 0).sum() > 20
    if name == "motion_blur":
        assert t.std() > 0


@pytest.mark.gpu
def test_transparent_shadows_attenuate_and_count_as_in_the_frame():
    """The transparency walk runs (shadows of 0.6 on the floor in front of the sheet), and with
    only the white Lambert's rows lit the ray count equals shadeHits' on the same rows."""
    need_gpu()
    P, _ = scene("transparent")
    (o, d, t), hits, surf, hit = surfaces("transparent", 11)
    rows = hit & (surf["material"] == 0)
    # every other row: a miss for shadeHits, a zero normal (no ray) for sampleLights
    h2 = hits.copy()
    h2["prim"][~rows] = -1
    n2 = surf["n"].copy()
    n2[~rows] = 0
    rgb = P.shadeHits(o, d, h2, time=t, seed=11)
    want = P.last_stats["shadow_rays"]
    e, per = P.sampleLights(surf["p"], n2, time=t, seed=11, per_light=True)
    assert P.last_stats["shadow_rays"] == want > rows.sum()
    assert np.array_equal(bits(e[rows]), bits(rgb[rows]))
    # the same light with fast shadows: the sheet is opaque, so some rows are darker
    Q, _ = cornell(WHITE, lights=[RECT], extra=[(quad(z=-2.0, lo=0.5, hi=5.0), GLASS)])
    eq = Q.sampleLights(surf["p"], n2, time=t, seed=11)
    assert np.all(eq[rows] <= e[rows]) and (eq[rows] < e[rows]).sum() > 20


# ------------------------------------------------------------------ GPU 2: the specular term and first_draw
def dot(a, b):
    """mrt_math.h dot: (x x' + y y') + (z z' + 0), float32."""
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + (a[..., 2] * b[..., 2] + F(0))).astype(F)


def blinn_frame(d, N, geoN):
    """n and rVec of Blinn::shade (src/Blinn.cpp:91-113) in the operation order of
    mrt_shader.h: the normal that agrees with the view side, flipped to face it, and
    rayD + n * (2 * vDotN)."""
    view = -d
    vn, vg = dot(view, N), dot(view, geoN)
    same = (vn * vg) >= 0
    n = np.where(same[..., None], N, geoN)
    vn = np.where(same, vn, vg)
    flip = vn < 0
    vn = np.where(flip, -vn, vn).astype(F)
    n = np.where(flip[..., None], -n, n).astype(F)
    return n, (d + n * (F(2) * vn)[..., None]).astype(F)


def respec(build):
    P, cam = build()
    return rematerial(P, mirror), cam


SPEC_SCENES = {
    "point": lambda: respec(lambda: cornell(None, lights=[POINT])),
    "rect_point": lambda: respec(lambda: cornell(None, lights=[RECT, POINT])),
    "dome": lambda: respec(dome_scene),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SPEC_SCENES))
def test_specular_terms_from_draw_one_sum_to_the_blinn_shading(name):
    need_gpu()
    P, cam = SPEC_SCENES[name]()
    seed = 11
    o, d, t = camera(cam).rays(W, H, seed)
    hits = P.traceRays(o, d, t)
    surf = P.hitSurfaces(o, d, hits)
    hit = hits["prim"] >= 0
    rgb = P.shadeHits(o, d, hits, time=t, seed=seed)
    n, rvec = blinn_frame(d, surf["n"], surf["geo_n"])
    e, per = P.sampleLights(surf["p"], n, rvec, time=t, seed=seed, first_draw=1, per_light=True)
    assert per.shape == (H, W, len(P._lights), 4)
    ls = np.zeros((H, W, 3), F)
    for l in range(per.shape[2]):
        ls = (ls + per[:, :, l, :3] * per[:, :, l, 3:4]).astype(F)
    assert hit.sum() > 50 and np.any(ls[hit] > 0)
    assert np.array_equal(bits(ls[hit]), bits(rgb[hit]))
    if name != "point":   # a sampled light's draws moved by one: other samples, another result
        e0 = P.sampleLights(surf["p"], n, rvec, time=t, seed=seed, first_draw=0)
        assert not np.array_equal(bits(e0[hit]), bits(e[hit]))


# ------------------------------------------------------------------ GPU 3: the point light by hand
def point_light_by_hand(P, light, frm, nrm, rvec, cast_shadows=True):
    """src/PointLight.cpp:8-81 in float32: (E, outSpec) per point."""
    frm, nrm, rvec = (np.ascontiguousarray(x, F).reshape(-1, 3) for x in (frm, nrm, rvec))
    L = (np.asarray(light["pos"], F) - frm).astype(F)
    ndl = dot(nrm, L)
    lit = ndl > 0
    fall = dot(L, L)
    safe = np.where(lit, fall, F(1))
    dr = np.array([miro.rsqrt_nr(float(x)) for x in safe], F)
    fall = np.array([miro.rcp_nr(float(x)) for x in safe], F)
    dist = np.array([miro.rcp_nr(float(x)) for x in dr], F)
    L = (L * dr[:, None]).astype(F)
    ndl = (ndl * dr).astype(F)
    A = ((F(light["power"]) * fall) * (F(0.25) / F(3.1415926))).astype(F)
    rdl = np.maximum(F(0), dot(rvec, L))
    att = np.ones(len(frm), F)
    if cast_shadows:
        occl = P.traceBatch(frm, L, 0.001, dist, any_hit=True)["prim"] == 1
        att[occl] = 0
    att = (att * ndl).astype(F)
    E, spec = (A * att).astype(F), (rdl * att).astype(F)
    E[~lit] = 0
    spec[~lit] = 0
    return E, spec, lit


@pytest.mark.gpu
@pytest.mark.parametrize("cast_shadows", [True, False])
def test_one_point_light_equals_its_restatement(cast_shadows):
    need_gpu()
    light = dict(POINT, cast_shadows=cast_shadows)
    P, cam = cornell(WHITE, lights=[light])
    (o, d, t), hits, surf, hit = surfaces("point", 11)   # the same geometry and camera
    p, n = surf["p"].reshape(-1, 3), surf["n"].reshape(-1, 3).copy()
    n[::3] = -n[::3]   # a third of the points face away from where they did
    rvec = blinn_frame(d.reshape(-1, 3), n, n)[1]
    E, spec, lit = point_light_by_hand(P, light, p, n, rvec, cast_shadows)
    e, per = P.sampleLights(p, n, rvec, per_light=True)
    assert per.shape == (W * H, 1, 4)
    assert (~lit).sum() > 50 and lit.sum() > 200 and np.any(spec > 0)
    assert not np.any(per[~lit]) and not np.any(e[~lit])
    assert np.array_equal(bits(per[:, 0, :3]), bits(np.repeat(E[:, None], 3, 1)))
    assert np.array_equal(bits(per[:, 0, 3]), bits(spec))
    shadowed = lit & (E == 0)
    assert (shadowed.sum() > 0) == cast_shadows
    assert P.last_stats["shadow_rays"] == (lit.sum() if cast_shadows else 0)


# ------------------------------------------------------------------ GPU 4: e and per_light agree
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rect_point", "dome"])
def test_e_is_the_float_sum_of_per_light_and_either_output_may_be_left_out(name):
    need_gpu()
    L = miro.lib()
    P, _ = scene(name)
    _, _, surf, hit = surfaces(name, 11)
    p, n = np.ascontiguousarray(surf["p"].reshape(-1, 3)), np.ascontiguousarray(surf["n"].reshape(-1, 3))
    e, per = P.sampleLights(p, n, seed=3, per_light=True)
    acc = np.zeros_like(e)
    for l in range(per.shape[1]):
        acc = (acc + per[:, l, :3]).astype(F)
    assert np.array_equal(bits(acc), bits(e)) and np.any(e > 0)
    assert np.array_equal(bits(P.sampleLights(p, n, seed=3)), bits(e))
    alone = np.zeros_like(per)   # per_light alone: through the C ABI
    assert L.mrt_sample_lights(P.handle, p.ctypes.data, n.ctypes.data, None, None, len(p), 3, 0, 0, 0, None,
                               alone.ctypes.data) == 0
    assert np.array_equal(bits(alone), bits(per))


@pytest.mark.gpu
def test_a_scene_without_lights_writes_zeros():
    need_gpu()
    P, _ = cornell(WHITE, lights=[])
    _, _, surf, _ = surfaces("point", 11)
    p, n = surf["p"].reshape(-1, 3), surf["n"].reshape(-1, 3)
    e, per = P.sampleLights(p, n, per_light=True)
    assert per.shape == (W * H, 0, 4) and e.shape == (W * H, 3) and not np.any(bits(e))
    assert P.last_stats["shadow_rays"] == 0


# ------------------------------------------------------------------ GPU 5: secondary
@pytest.mark.gpu
def test_secondary_takes_one_dome_sample():
    need_gpu()
    P, _ = scene("dome")
    _, _, surf, hit = surfaces("dome", 11)
    four, _ = whitened(dome_scene)
    four._lights[0].setSamples(4)
    four.preCalc()
    one, _ = whitened(dome_scene)
    one._lights[0].setSamples(1)
    one.preCalc()
    p, n = surf["p"], surf["n"]
    a = four.sampleLights(p, n, seed=8, secondary=True, per_light=True)
    ra = four.last_stats["shadow_rays"]
    b = one.sampleLights(p, n, seed=8, per_light=True)
    assert ra == one.last_stats["shadow_rays"] > 0
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    c = four.sampleLights(p, n, seed=8)
    assert four.last_stats["shadow_rays"] > ra and not np.array_equal(bits(c[hit]), bits(a[0][hit]))


# ------------------------------------------------------------------ GPU 6: sizes where the indexing can go wrong
@pytest.mark.gpu
def test_every_batch_is_a_prefix_of_the_longest():
    """n = 1, 63, 64, 65, kWG - 1, kWG, kWG + 1 and one batch longer than a full pass of the
    launch grid (grid x kWG + 77 points; the 37 x 29 points, tiled): a chunk's last lanes, a
    band's cut chunk, more workgroups than the grid holds.  The results depend on the point's
    index alone."""
    need_gpu()
    import torch
    P, _ = scene("point")
    _, _, surf, hit = surfaces("point", 11)
    cus = torch.cuda.get_device_properties(P.device).multi_processor_count
    longest = cus * BLOCKS_PER_CU * KWG + 77
    reps = -(-longest // (W * H))
    p = np.ascontiguousarray(np.tile(surf["p"].reshape(-1, 3), (reps, 1))[:longest])
    n = np.ascontiguousarray(np.tile(surf["n"].reshape(-1, 3), (reps, 1))[:longest])
    full, full_per = P.sampleLights(p, n, seed=2, per_light=True)
    assert full.shape == (longest, 3)
    # one point light draws nothing: every tile repeats the first
    first = full[:W * H]
    assert np.any(first > 0) and np.array_equal(bits(full[-W * H:]), bits(np.roll(first, -(longest % (W * H)), 0)))
    for k in (1, 63, 64, 65, KWG - 1, KWG, KWG + 1):
        e, per = P.sampleLights(p[:k], n[:k], seed=2, per_light=True)
        assert np.array_equal(bits(e), bits(full[:k])) and np.array_equal(bits(per), bits(full_per[:k])), k
    # with draws (the rectangle light): a prefix keeps its points' streams
    R, _ = scene("rect_point")
    m = 3 * KWG + 65
    ref = R.sampleLights(p[:m], n[:m], seed=2)
    for k in (1, 65, KWG + 1):
        assert np.array_equal(bits(R.sampleLights(p[:k], n[:k], seed=2)), bits(ref[:k])), k


# ------------------------------------------------------------------ GPU 7: sync and async agree
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rect_point", "instanced"])
def test_device_tensors_on_a_side_stream_equal_the_host_call(name):
    """Contiguous float32 device tensors go through mrt_sample_lights_async on the current
    stream; the results are read after that stream is synchronised, not before."""
    need_gpu()
    import torch
    P, _ = scene(name)
    (o, d, t), _, surf, hit = surfaces(name, 11)
    n, rvec = blinn_frame(d, surf["n"], surf["geo_n"])
    ref, ref_per = P.sampleLights(surf["p"], n, rvec, time=t, seed=6, first_draw=1, per_light=True)
    ref_rays = P.last_stats["shadow_rays"]
    dev = torch.device("cuda", P.device)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        tp, tn, tr, tt = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (surf["p"], n, rvec, t))
        e, per = P.sampleLights(tp, tn, tr, time=tt, seed=6, first_draw=1, per_light=True)
        flat = P.sampleLights(tp.reshape(-1, 3), tn.reshape(-1, 3), seed=6)
    side.synchronize()
    assert e.shape == (H, W, 3) and per.shape == (H, W, len(P._lights), 4) and flat.shape == (W * H, 3)
    assert np.array_equal(bits(e.cpu().numpy()), bits(ref)) and np.array_equal(bits(per.cpu().numpy()), bits(ref_per))
    assert np.array_equal(bits(flat.cpu().numpy()), bits(P.sampleLights(surf["p"], surf["n"], seed=6).reshape(-1, 3)))
    with torch.cuda.stream(side):
        P.sampleLights(tp, tn, tr, time=tt, seed=6, first_draw=1)
    side.synchronize()
    assert P.stats()["shadow_rays"] == ref_rays and P.stats()["primary_rays"] == 0
    with pytest.raises(miro.MRTError):   # a strided view is refused, not copied
        P.sampleLights(tp[:, ::2], tn[:, ::2])


# ------------------------------------------------------------------ GPU 8: count mode
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rect_point", "instanced"])
def test_count_mode_gives_the_same_bits_and_fills_the_visit_counters(name):
    need_gpu()
    P, _ = scene(name)
    (o, d, t), _, surf, hit = surfaces(name, 11)
    e = P.sampleLights(surf["p"], surf["n"], time=t, seed=4)
    plain = dict(P.last_stats)
    c = P.sampleLights(surf["p"], surf["n"], time=t, seed=4, count_visits=True)
    st = dict(P.last_stats)
    assert np.array_equal(bits(c), bits(e))
    assert st["shadow_rays"] == plain["shadow_rays"] > 0
    assert st["node_visits"] > 0 and st["leaf_visits"] > 0
    assert plain["node_visits"] == 0 and plain["leaf_visits"] == 0
