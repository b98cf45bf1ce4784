"""Every kernel family on a tree that mrt_scene_rebuild_bvh made on the device, and the sequences
around a rebuild that tests/test_rebuild.py does not run.

A rebuilt replica differs from an uploaded one in more than a refitted one does: node numbers
(the world's nodes past the built count live in a tail behind the BLAS nodes), packet order,
child-word bits made on the device, a reallocated node array, and the LDS top-node walk off.
test_rebuild.py's scenes are Lambert under one point light, so only frame1_kernel, the ray entries
and sampleLights have walked such a tree.  Here: the shade kernels with the wavefront shadow
passes (rectangle, dome, transparent shadows), the binned dome shadow rays over instances, the
chain engine (reflection, path tracing, binned levels, the fused rec kernels, the chunk fallback),
adaptive supersampling, lightSamples, alpha lanes in the world and inside an instance, a
motion-blurred mesh over the open shutter, and the walk_exit x walk_latch x scalar_nodes forms.

Scene A renders a frame (the upload), is rebuilt on the device, and its export must equal
rebuild_arrays (test_rebuild.py) of its export from before.  The twin T is the same scene that
imports those restated arrays: uploaded as any build is, its world nodes in one range, no tail,
the LDS walk available.  Where a scene of the suite does not hand out its triangles, T is that
scene rebuilt on the host before its upload (the host rule is held to the restatement by the CPU
tests of test_rebuild.py and test_rebuild_shapes.py) and A's export must equal T's.  Frames
(float and 8-bit), hit records, ray counts and count-mode visit counts are compared bit for bit,
and each test reads last_stats to show that the family it is about ran.

Two scenes are tail fixtures, with line_tris(1028) among their meshes (asserted on the CPU):
`plain` (test_refit's stand-in, the line and a floor) and Kinds(line=1028) (instances, an
alpha-mapped quad, a motion-blurred sphere)."""
import functools
import itertools

import numpy as np
import pytest

import miro
from miro import _lib
from helpers import bits, camera, tuned
from test_refit import (CAM, F32, assert_arrays, assert_frames, floor_mesh, frame, import_bvh, point_light, prim_verts_of,
                        rect_light, refit_of, standin, tri_mesh)
from test_refit_shapes import chain_case, same_words
from test_rebuild import Kinds, assert_counted, assert_tree, counted, line_tris, rebuild_arrays

W = H = 64
# Kinds' three instances (191 pixels of 64 x 64), its alpha-mapped quad (185) and its motion-blurred sphere (33) in view
KCAM = dict(eye=(0.5, 4.5, 9.5), lookAt=(0, 2.8, 0), up=(0, 1, 0), fov=65)
SHUTTER = dict(KCAM, shutterSpeed=1.0)
TUNINGS = [dict(walk_exit=we, walk_latch=wl, scalar_nodes=sn) for we, wl, sn in itertools.product((0, 1), (0, 1), (0, 7))]
N_LINE = 1028


# ---------------------------------------------------------------- scenes
@functools.lru_cache(maxsize=None)
def plain_meshes():
    """The stand-in, the 1028 triangles of line_tris on a line of length 8 beside it, the floor."""
    V, N, F = standin()
    lV, lN, lF = line_tris(N_LINE)
    lV = np.asarray(lV * F32(0.125) + np.array([-12.0, 0.5, 2.0], F32), F32)
    fl = floor_mesh()
    out = ((V, N, F), (lV, lN, lF), (fl.verts.copy(), fl.normals.copy(), fl.vidx.copy()))
    for m in out:
        for a in m:
            a.setflags(write=False)
    return out


def plain_scene(light=point_light, material=None, num_paths=1, path_trace=None, subdivs=None):
    """test_refit.scene_a with the line between the stand-in and the floor."""
    (V, N, F), (lV, lN, lF), _ = plain_meshes()
    P = miro.Scene()
    miro.makeMeshObjs(P, tri_mesh(V, N, F), material or miro.Lambert((0.8, 0.7, 0.6)))
    miro.makeMeshObjs(P, tri_mesh(lV, lN, lF), miro.Lambert((0.5, 0.8, 0.6)))
    miro.makeMeshObjs(P, floor_mesh(), miro.Lambert((0.6, 0.6, 0.6)))
    P.addLight(light())
    P.setBGColor((0.1, 0.1, 0.3))
    P.setNumPaths(num_paths)
    if path_trace is not None:
        P.setPathTrace(True)
        P.setMaxBounces(path_trace)
    if subdivs is not None:
        P.setMinSubdivs(subdivs[0])
        P.setMaxSubdivs(subdivs[1])
        P.setNoise(subdivs[2])
    P.preCalc()
    return P


def plain_pv():
    return prim_verts_of(*((m[0], m[2]) for m in plain_meshes()))


def sky(seed, w=32, h=16):
    return np.random.default_rng(seed).uniform(0.05, 4.0, (h, w, 3)).astype(np.float32)


def dome_light(rgb, power=0.4, samples=3):
    dl = miro.DomeLight()
    dl.setTexture(miro.Texture(miro.RawImage(rgb.shape[1], rgb.shape[0], rgb)))
    dl.setPower(power)
    dl.setSamples(samples)
    dl.setNoiseThreshold(0.001)
    return dl


def kinds(**kw):
    return Kinds(line=N_LINE, **kw)


class Restated:
    """The export of a built scene, its node count, rebuild_arrays of it: read-only."""

    def __init__(self, P, pv, fixed):
        self.ex0, self.built, self.pv, self.fixed = P.bvh_export(), P.bvh_info["nodes"], pv, fixed
        self.n = P.bvh_info["prims"]
        self.want = rebuild_arrays(*self.ex0, pv, fixed)
        for a in self.ex0 + self.want:
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def plain_restated():
    return Restated(plain_scene(), plain_pv(), {})


@functools.lru_cache(maxsize=None)
def kinds_restated():
    S = kinds()
    return Restated(S.P, S.pv(), S.fixed())


# ---------------------------------------------------------------- what is compared
def shown(P, cam):
    """A 64 x 64 frame with its hit records and stats, and the same frame in count mode."""
    f = frame(P, W, H, cam)
    return f, dict(P.last_stats), counted(P, cam, W, H)


def assert_shown(a, b):
    assert_frames(a[0], b[0])
    assert a[0]["secondary_rays"] == b[0]["secondary_rays"]
    for k in ("fused", "chain", "primary_rays"):
        assert a[1][k] == b[1][k], k
    assert_counted(a[2], b[2])
    assert a[2]["secondary_rays"] == b[2]["secondary_rays"]


def rebuilt_pair(make, R, cam):
    """(A, T): A = make() after a frame and a device rebuild, its export the restatement R.want;
    T = make() with R.want imported."""
    A = make()
    assert_arrays(A.bvh_export(), R.ex0)
    frame(A, W, H, cam)   # uploaded
    assert A.rebuildBVH() > 0.0
    assert_arrays(A.bvh_export(), R.want)
    T = make()
    import_bvh(T, R.want)
    return A, T


def instance_hits(f, R):
    return int((f["hits"]["prim"] >= R.n).sum())   # hit ids past the world's prims are a BLAS's triangles


# ---------------------------------------------------------------- CPU tests: the premises
def test_both_scenes_are_tail_fixtures():
    """M of the rebuilt tree passes the node count of the built one in the plain scene and in the
    instanced one, whose node array continues with the BLAS's nodes; the rebuilt trees are trees;
    the twin's tree is large enough for the LDS top-node walk."""
    for R in (plain_restated(), kinds_restated()):
        M, P = len(R.want[1]), len(R.want[3])
        print(f"prims {R.n}, P {P}, M {M}, built {R.built}")
        assert M > R.built and M >= 64 and P > 256
        assert_tree(R.want, R.n, R.pv, R.fixed)
    S = kinds()
    assert S.P.instance_count() == 3 and S.P.blas_export(0)[1].shape[0] > 0


def test_host_rebuild_of_the_family_scenes_is_the_restatement():
    """The twins of the suite's own scenes are rebuilt on the host: that path on this file's two
    scenes, and with the alpha-mapped BLAS (the lanes are the same: materials are no input)."""
    for make, R in ((plain_scene, plain_restated()), (lambda: kinds(cutout=True).P, kinds_restated())):
        P = make()
        assert_arrays(P.bvh_export(), R.ex0)
        assert P.rebuildBVH() == 0.0
        assert_arrays(P.bvh_export(), R.want)


# ---------------------------------------------------------------- GPU 1-3: the shade kernels, wavefront shadow passes
@pytest.mark.gpu
def test_rectangle_light_with_blinn_wavefront_and_not():
    """1. a rectangle light of two samples on a Blinn stand-in: the shade kernels with the
    shadow rays inline (wavefront 0) and in their own passes (wavefront 1)."""
    R = plain_restated()
    make = lambda: plain_scene(light=rect_light, material=miro.Blinn((0.7, 0.7, 0.7), specExp=8.0, specAmt=0.25))
    A, T = rebuilt_pair(make, R, CAM)
    for wf in (0, 1):
        with tuned(wavefront=wf):
            a, t = shown(A, CAM), shown(T, CAM)
        assert_shown(a, t)
        assert a[1]["fused"] == 0 and a[1]["shadow_rays"] > 0 and a[1]["chain"] == 0
        assert (a[0]["hits"]["prim"] >= 0).mean() > 0.3


@pytest.mark.gpu
def test_dome_light_over_instances_binned_and_not():
    """2. a dome light over the instanced tail fixture: the shadow rays unbinned and binned, the
    instance binning off and at 2, the dome replay off and on."""
    R = kinds_restated()
    rgb = sky(1)
    A, T = rebuilt_pair(lambda: kinds(lights=[dome_light(rgb)]).P, R, KCAM)
    seen = []
    for b, bi, dr in itertools.product((0, 6), (0, 2), (0, 1)):
        with tuned(bin=b, bin_inst=bi, dome_replay=dr):
            a, t = shown(A, KCAM), shown(T, KCAM)
        assert_shown(a, t)
        assert a[1]["fused"] == 0 and a[1]["shadow_rays"] > 0
        seen.append(a)
    assert instance_hits(seen[0][0], R) > 50
    for a in seen[1:]:   # and no setting changes a bit
        assert_frames(a[0], seen[0][0])


@pytest.mark.gpu
def test_transparent_shadows_through_the_glass_sheet():
    """3. test_sample_lights' transparent scene: a rectangle light with transparent shadows over a
    Cornell box and a refracting sheet.  The scene does not hand out its triangles: the twin is
    rebuilt on the host before its upload."""
    from test_sample_lights import SCENES
    A, cam = SCENES["transparent"]()
    T, _ = SCENES["transparent"]()
    assert T.rebuildBVH() == 0.0
    frame(A, W, H, cam)   # uploaded
    assert A.rebuildBVH() > 0.0
    assert_arrays(A.bvh_export(), T.bvh_export())
    a, t = shown(A, cam), shown(T, cam)
    assert_shown(a, t)
    assert a[1]["fused"] == 0 and a[1]["shadow_rays"] > 0 and a[1]["secondary_rays"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rect_point", "dome", "instanced", "alpha_map", "motion_blur"])
def test_the_sample_lights_scenes_after_a_rebuild(name):
    """The other scenes of test_sample_lights.py (two lights, a dome light with an environment
    map, instances, alpha-mapped leaves, a motion-blurred ball over the open shutter), against
    their host-rebuilt twins: the frame and sampleLights at the camera rays' hit points."""
    from test_sample_lights import SCENES
    A, cam = SCENES[name]()
    T, _ = SCENES[name]()
    assert T.rebuildBVH() == 0.0
    frame(A, W, H, cam)   # uploaded
    assert A.rebuildBVH() > 0.0
    assert_arrays(A.bvh_export(), T.bvh_export())
    a, t = shown(A, cam), shown(T, cam)
    assert_shown(a, t)
    assert a[1]["shadow_rays"] > 0 and (a[0]["hits"]["prim"] >= 0).sum() > 50
    o, d, tm = camera(cam).rays(W, H, 11)
    ha, ht = A.traceRays(o, d, tm), T.traceRays(o, d, tm)
    assert same_words(ha, ht)
    sa, st = A.hitSurfaces(o, d, ha), T.hitSurfaces(o, d, ht)
    assert sa.tobytes() == st.tobytes()
    ea, et = (P.sampleLights(sa["p"], sa["n"], time=tm, seed=11, per_light=True) for P in (A, T))
    assert np.array_equal(bits(ea[0]), bits(et[0])) and np.array_equal(bits(ea[1]), bits(et[1])) and np.any(ea[0] > 0)


# ---------------------------------------------------------------- GPU 4: the chain engine
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mirror", "rect_paths4"])
def test_chain_engine_binned_levels_and_the_fused_rec_kernels(kind):
    """4. reflection (an always-mirror stand-in, a point light) and path tracing (a rectangle
    light, four paths): the chain engine with its levels unbinned and binned, and the fused
    recursive kernels (chain 0).  The three render the same frame."""
    R = plain_restated()
    kw, cam = chain_case(kind, 0.0)
    A, T = rebuilt_pair(lambda: plain_scene(**kw), R, cam)
    out = []
    for knobs, chain in ((dict(bin=0), 1), (dict(bin=6), 1), (dict(chain=0), 0)):
        with tuned(**knobs):
            a, t = shown(A, cam), shown(T, cam)
        assert_shown(a, t)
        assert a[1]["chain"] == chain and a[1]["secondary_rays"] > 0 and a[1]["shadow_rays"] > 0, knobs
        out.append(a)
    assert (out[0][0]["hits"]["prim"] >= 0).mean() > 0.3
    for a in out[1:]:
        assert_frames(a[0], out[0][0])
        assert a[0]["secondary_rays"] == out[0][0]["secondary_rays"]


@pytest.mark.gpu
def test_chain_chunk_fallback():
    """4. the path-traced scene with the level capacities cut to 1 % of the estimate: every chunk
    outgrows a level and is shaded by the fused chain kernels over the chunk's units."""
    R = plain_restated()
    kw, cam = chain_case("rect_paths4", 0.0)
    A, T = rebuilt_pair(lambda: plain_scene(**kw), R, cam)
    with tuned(chain_est=1):
        want = shown(A, cam)   # seeds the estimates
        shown(T, cam)
        with tuned(chain_est_pct=1):
            a, t = shown(A, cam), shown(T, cam)
    assert a[1]["chain_fallbacks"] > 0 and t[1]["chain_fallbacks"] > 0
    assert a[1]["chain"] == 1 and a[1]["secondary_rays"] > 0 and a[1]["shadow_rays"] > 0
    assert_shown(a, t)
    assert_frames(a[0], want[0])


# ---------------------------------------------------------------- GPU 5: adaptive supersampling
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lambert_point", "mirror"])
def test_adaptive_supersampling(kind):
    """5. subdivs (1, 2, 0.01): the adaptive kernel, and its passes over the chain engine."""
    R = plain_restated()
    kw, cam = ({}, CAM) if kind == "lambert_point" else chain_case("mirror", 0.0)
    A, T = rebuilt_pair(lambda: plain_scene(subdivs=(1, 2, 0.01), **kw), R, cam)
    a, t = shown(A, cam), shown(T, cam)
    assert_shown(a, t)
    assert a[1]["primary_rays"] > W * H and a[1]["shadow_rays"] > 0
    assert a[1]["chain"] == (1 if kind == "mirror" else 0)


# ---------------------------------------------------------------- GPU 6: alpha lanes, the open shutter
@pytest.mark.gpu
def test_alpha_lanes_in_the_world_and_in_an_instance_and_the_open_shutter():
    """6. Kinds with the alpha map on the instanced sphere too, shutterSpeed 1: the checked lanes
    of the world (the quad, the motion-blurred sphere) and of the BLAS, in camera and shadow rays."""
    R = kinds_restated()
    S = kinds(cutout=True)
    A, T = rebuilt_pair(lambda: kinds(cutout=True).P, R, SHUTTER)
    a, t = shown(A, SHUTTER), shown(T, SHUTTER)
    assert_shown(a, t)
    assert a[1]["shadow_rays"] > 0
    prim = a[0]["hits"]["prim"]
    n_plain = len(S.F)
    assert instance_hits(a[0], R) > 20
    assert ((prim >= n_plain) & (prim < S.inst0)).sum() > 20, "the alpha-mapped quad is in view"
    assert ((prim >= S.mb0) & (prim < S.mb0 + len(S.bF))).sum() > 0, "the motion-blurred sphere is in view"
    # the alpha channel cuts squares out of the quad and of the instanced sphere: where the scene
    # with the opaque map shows them, some pixels show what lies behind
    opaque = frame(kinds().P, W, H, SHUTTER)["hits"]["prim"]
    for on in (opaque >= R.n, (opaque >= n_plain) & (opaque < S.inst0)):
        assert on.sum() > 50 and (prim[on] != opaque[on]).sum() > 5


# ---------------------------------------------------------------- GPU 7: lightSamples, sampleLights
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dome_over_instances", "rectangle"])
def test_light_samples_and_sample_lights_at_the_hit_points(name):
    """7. the wavefront passes of lightSamples (samples, counts, e, per_light) and
    sampleLights(per_light=True) at the hit points of the camera rays."""
    from test_light_samples import same
    if name == "rectangle":
        R, make = plain_restated(), lambda: plain_scene(light=rect_light)
    else:
        rgb = sky(2)
        R, make = kinds_restated(), lambda: kinds(lights=[dome_light(rgb)]).P
    cam = CAM if name == "rectangle" else KCAM
    A, T = rebuilt_pair(make, R, cam)
    o, d, tm = camera(cam).rays(W, H, 5)
    o, d, tm = o.reshape(-1, 3), d.reshape(-1, 3), tm.reshape(-1)
    ha, ht = A.traceRays(o, d, tm), T.traceRays(o, d, tm)
    assert same_words(ha, ht) and (ha["prim"] >= 0).mean() > 0.3
    sa, st = A.hitSurfaces(o, d, ha), T.hitSurfaces(o, d, ht)
    assert sa.tobytes() == st.tobytes()
    p, n = np.ascontiguousarray(sa["p"], F32), np.ascontiguousarray(sa["n"], F32)
    la = A.lightSamples(p, n, time=tm, seed=7, e=True, per_light=True)
    rays_a = A.last_stats["shadow_rays"]
    lt = T.lightSamples(p, n, time=tm, seed=7, e=True, per_light=True)
    assert set(la) >= {"samples", "counts", "e", "per_light"} and same(la, lt)
    assert rays_a == T.last_stats["shadow_rays"] > 0 and np.any(la["e"] > 0) and la["counts"].sum() > 0
    ea = A.sampleLights(p, n, time=tm, seed=7, per_light=True)
    rays_a = A.last_stats["shadow_rays"]
    et = T.sampleLights(p, n, time=tm, seed=7, per_light=True)
    assert np.array_equal(bits(ea[0]), bits(et[0])) and np.array_equal(bits(ea[1]), bits(et[1]))
    assert rays_a == T.last_stats["shadow_rays"] > 0
    assert np.array_equal(bits(ea[0]), bits(la["e"]))   # the two entries agree on e
    if name == "dome_over_instances":
        assert (ha["inst"] >= 0).sum() > 50


# ---------------------------------------------------------------- GPU 8: the walk forms of the one-light frame
@pytest.mark.gpu
def test_one_light_frame_under_every_walk_form():
    """8. frame1_kernel under walk_exit x walk_latch x scalar_nodes with the LDS top-node walk
    asked for: the rebuilt replica cannot take it (its first 64 node numbers are not the tree's
    breadth-first head) and walks the form the tuning names; the twin takes it."""
    R = plain_restated()
    assert len(R.want[1]) >= 64
    A, T = rebuilt_pair(plain_scene, R, CAM)
    first = None
    for knobs in TUNINGS:
        with tuned(lds_nodes=1, **knobs):
            a, t = shown(A, CAM), shown(T, CAM)
            frame(A, W, H, CAM)   # walk_info: of the last one-light frame
            frame(T, W, H, CAM)
            wa, wt = A.walk_info(), T.walk_info()
        assert_shown(a, t)
        assert a[1]["fused"] == 1 and a[1]["shadow_rays"] > 0, knobs
        assert wa["lds_nodes"] == 0 and wt["lds_nodes"] == 1, knobs
        assert wa["walk_exits"] == (2 if knobs["walk_exit"] == 0 else 1), knobs
        first = first or a
        assert_frames(a[0], first[0])
    assert (first[0]["hits"]["prim"] >= 0).mean() > 0.3


# ---------------------------------------------------------------- GPU D: sequences
@pytest.mark.gpu
def test_rebuild_reupload_rebuild():
    """Rebuild, a re-upload (mrt_scene_set_material_gloss marks the replica stale), a rebuild of
    the second replica: it has P packets of capacity, M world nodes and a tail of its own."""
    L = miro.lib()
    live0 = L.mrt_debug_live_resources()
    R = kinds_restated()
    want2 = rebuild_arrays(*R.want, R.pv, R.fixed)
    assert len(want2[1]) > 0 and len(R.want[3]) - 1 > len(R.want[1])   # P - 1 passes M: the second replica grows too
    A, T = rebuilt_pair(lambda: kinds().P, R, KCAM)
    _lib.check(L.mrt_scene_set_material_gloss(A.handle, 0, 1.0), "gloss")
    up = A.uploadCount()
    a, t = shown(A, KCAM), shown(T, KCAM)
    assert A.uploadCount() == up + 1
    assert_shown(a, t)
    assert_arrays(A.bvh_export(), R.want)
    assert A.rebuildBVH() > 0.0
    assert_arrays(A.bvh_export(), want2)
    assert A.uploadCount() == up + 1
    T2 = kinds().P
    import_bvh(T2, want2)
    a2 = shown(A, KCAM)
    assert_shown(a2, shown(T2, KCAM))
    assert instance_hits(a2[0], R) > 50
    for P in (A, T, T2):
        L.mrt_scene_destroy(P._h)
        P._h = None
    assert L.mrt_debug_live_resources() == live0


@pytest.mark.gpu
def test_rebuild_blas_deform_rebuild():
    """Rebuild, deformMesh of the BLAS mesh (each instance's box and the world refit on the
    rebuilt topology), rebuild again (the keys come from the new fixed boxes)."""
    from test_deform_mesh import blas_displaced, blas_refit
    R = kinds_restated()
    S = kinds()
    A = S.P
    blas0 = A.blas_export(0)
    frame(A, W, H, KCAM)   # uploaded
    assert A.rebuildBVH() > 0.0
    assert_arrays(A.bvh_export(), R.want)
    bV1, bN1 = blas_displaced(S.bV * F32(1.25), S.bF, 3)
    assert A.deformMesh(S.ids["blas"], bV1, bN1) > 0.0
    bw = blas_refit(blas0, bV1, S.bF)
    fixed1 = S.fixed(root=bw[0][0])
    moved = [i for i in range(3) if not np.array_equal(fixed1[S.inst0 + i][0], R.fixed[S.inst0 + i][0])]
    assert moved == [0, 1, 2]
    assert_arrays(A.blas_export(0), bw)
    refitted = refit_of(R.want, R.pv, fixed1)
    assert_arrays(A.bvh_export(), refitted)
    assert A.rebuildBVH() > 0.0
    want = rebuild_arrays(*refitted, R.pv, fixed1)
    assert_arrays(A.bvh_export(), want)
    assert_tree(want, R.n, R.pv, fixed1)
    # a twin deformed on the host before its upload, with the restated world arrays
    T = kinds()
    T.P.deformMesh(T.ids["blas"], bV1, bN1)
    assert_arrays(T.P.blas_export(0), bw)
    import_bvh(T.P, want)
    a = shown(A, KCAM)
    assert_shown(a, shown(T.P, KCAM))
    assert instance_hits(a[0], R) > 50


@pytest.mark.gpu
def test_rebuild_then_a_relight():
    """Rebuild, then updateLights with a moved point light and updateTexture of the dome's sky:
    the frame equals that of a fresh scene with those lights that imports the same tree."""
    R = kinds_restated()
    sky0, sky1 = sky(3), sky(4)
    at0, at1 = (5, 12, 8), (-6, 9, 7)

    def lights(pos, rgb):
        pl = point_light()
        pl.setPosition(pos)
        return [pl, dome_light(rgb)]

    S = kinds(lights=lights(at0, sky0))
    A = S.P
    before = frame(A, W, H, KCAM)   # uploaded
    assert A.rebuildBVH() > 0.0
    assert_arrays(A.bvh_export(), R.want)
    up = A.uploadCount()
    A._lights[0].setPosition(at1)
    A.updateLights()
    A.updateTexture(A._lights[1].texture, sky1)
    a = shown(A, KCAM)
    assert A.uploadCount() == up
    T = kinds(lights=lights(at1, sky1)).P
    import_bvh(T, R.want)
    assert_shown(a, shown(T, KCAM))
    assert a[1]["shadow_rays"] > 0 and not np.array_equal(bits(a[0]["rgb"]), bits(before["rgb"]))
    assert_arrays(A.bvh_export(), R.want)
