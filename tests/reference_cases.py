"""The cases pinned to the reference renderer's own code, in one table.

Three readers share it, so that all three mean the same scenes:
  tests/test_reference_cpu.py   oracle vs the reference driver (oracle/_ref/ref_driver) and
                                oracle vs the recorded fixtures;
  tests/test_reference_gpu.py   device vs the recorded fixtures (tests/golden/reference/);
  oracle/ref/make_reference_fixtures.py   writes those fixtures from the driver.

A case is what helpers.scene_pair takes (a config dict and keyword arguments), a camera,
a frame size and the driver command that renders it.  build_scenes() has scene_pair make its
oracle calls on an OracleScene and a RefScene (oracle/refdriver.py) at once.
Nothing here needs the reference tree or its driver.
"""
import os

import numpy as np

import oracle as O
from conftest import GOLDEN, ref_hdr_images, ref_model
from helpers import ROOT, fixture_mesh
from miro import scenes

REF_DIR = os.path.join(GOLDEN, "reference")
LEAF_TGA = os.path.join(ROOT, "assets", "Tree_03_Leaves.tga")
LEAF_OBJ = os.path.join(GOLDEN, "leaf_test.obj")
C1 = scenes.CONFIGS["C1"]
CAM = C1["camera"]
TEX_RGB, TEX_GRAY = 3, 1          # oracle.TEX_CHANNELS keys (miro.TEX_RGB / TEX_GRAY)
W, H = 40, 36                     # two buckets each way, not square
HDRS = ("Arches_E_PineTree.hdr", "Arches_E_PineTree_Env.hdr", "Topanga_Forest_B_light.hdr", "sky.hdr",
        "hdrvfx_nyany_1_n2_v101_Ref.hdr")


# ------------------------------------------------------------------ geometry
def quads(n=6, seed=5, y=(1.0, 4.5)):
    """n textured quads (two triangles each) floating in the Cornell box at seeded places,
    tilted about y; (verts, normals, vidx, nidx, uv, tidx)."""
    rng = np.random.default_rng(seed)
    V, N, F, UV = [], [], [], []
    for _ in range(n):
        c = np.array([rng.uniform(1.0, 4.5), rng.uniform(*y), rng.uniform(-4.5, -1.0)], np.float32)
        s = np.float32(rng.uniform(0.6, 1.3))
        tilt = rng.uniform(-0.5, 0.5)
        ex = np.array([np.cos(tilt), 0, np.sin(tilt)], np.float32) * s
        ey = np.array([0, 1, 0], np.float32) * s
        nrm = np.cross(ex, ey); nrm /= np.linalg.norm(nrm)
        b = len(V)
        V += [c - ex - ey, c + ex - ey, c + ex + ey, c - ex + ey]
        N += [nrm] * 4
        UV += [(0, 0), (1, 0), (1, 1), (0, 1)]
        F += [(b, b + 1, b + 2), (b, b + 2, b + 3)]
    F = np.array(F, np.uint32)
    return np.array(V, np.float32), np.array(N, np.float32), F, F.copy(), np.array(UV, np.float32), F.copy()


def canopy():
    """Two refractive quads lying flat just under the ceiling light, above what FLOOR_CAM sees:
    they shade no camera ray and stand in every shadow ray's way."""
    V = np.array([(1.0, 5.0, -4.5), (4.5, 5.0, -4.5), (4.5, 5.0, -1.0), (1.0, 5.0, -1.0)], np.float32)
    N = np.array([(0, -1, 0)], np.float32)
    F = np.array([(0, 1, 2), (0, 2, 3)], np.uint32)
    return V, N, F, np.zeros_like(F)


def wall_uv(arrs, scale_=5.5):
    """Planar texture coordinates for the Cornell mesh, skewed so that no wall, floor or ceiling
    triangle maps to a line: where a triangle's uv edges are parallel the reference's
    TriangleMesh::preCalc leaves that triangle's tangents unwritten in memory it never
    cleared (src/TriangleMesh.cpp:111-150), and a normal map then shades from garbage."""
    v = arrs[0]
    uv = np.stack([v[:, 0] / scale_ + v[:, 2] / (2 * scale_), v[:, 1] / scale_ + v[:, 2] / 7.0], 1).astype(np.float32)
    return tuple(arrs) + (uv, arrs[2].copy())


def synthetic_maps(seed=9, w=64, h=48):
    rng = np.random.default_rng(seed)
    color = rng.uniform(0.1, 0.9, (h, w, 3)).astype(np.float32)
    normal = np.concatenate([rng.uniform(-0.3, 0.3, (h, w, 2)), rng.uniform(0.8, 1.0, (h, w, 1))], 2).astype(np.float32)
    spec = rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)
    return dict(color=(color, TEX_RGB), normal=(normal, TEX_RGB), specular=(spec, TEX_GRAY))


_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def leaf_image():
    return _once("leaf", lambda: O.image_load(LEAF_TGA))


def hdr(name):
    return _once(name, lambda: O.hdr_load(ref_hdr_images()[name]))


def placements(n=5, seed=11):
    """Instance matrices: rotation about a seeded axis times a non-uniform scale, then a place in the box."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        a = rng.uniform(0, 2 * np.pi)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
        M = np.eye(4)
        M[:3, :3] = R @ np.diag(rng.uniform(0.5, 1.8, 3))
        M[:3, 3] = (rng.uniform(1.0, 4.5), rng.uniform(1.0, 4.0), rng.uniform(-4.5, -1.0))
        out.append(M.astype(np.float32))
    return out


def cannonball_parts():
    f = np.load(os.path.join(GOLDEN, "cannonball_mb.npz"))
    return ((f["ground_verts"], f["ground_normals"], f["ground_vidx"], f["ground_nidx"]),
            (f["verts"], f["normals"], f["vidx"], f["nidx"]), f["verts2"])


# ------------------------------------------------------------------ the cases
LAMBERT = dict(kind="lambert", kd=(0.8, 0.8, 0.8))
POINT = C1["lights"]
RECT = dict(type="rect", v1=(2.2, 5.4, -2.0), v2=(3.3, 5.4, -2.0), v3=(2.2, 5.4, -3.0), power=60.0)
FLOOR_CAM = dict(eye=(2.75, 3.2, 1.0), lookAt=(2.75, 0.0, -2.75), up=(0, 1, 0), fov=40.0)
BALL_CAM = dict(eye=(0.75, 0.62, 0.38), lookAt=(0.0, 0.5, 0.38), up=(0, 1, 0), fov=60.0)
BALL_CFG = dict(C1, material=dict(kind="lambert", kd=(0.5, 0.45, 0.4)),
                lights=[dict(type="point", pos=(2.0, 3.0, 2.0), power=60.0)])
# cameras in the open (the env-map cases hold a few quads only): straight at each pole and at
# the +-pi seam of the longitude, the centre pixel of an odd frame exactly on it
ENV_CAMS = {"up": dict(eye=(2.75, 2.75, -2.0), lookAt=(2.75, 9.0, -2.0), up=(0, 0, -1), fov=70.0),
            "down": dict(eye=(2.75, 2.75, -2.0), lookAt=(2.75, -9.0, -2.0), up=(0, 0, 1), fov=70.0),
            "seam": dict(eye=(2.75, 2.75, -2.0), lookAt=(-9.0, 2.75, -2.0), up=(0, 1, 0), fov=70.0)}


def _box(material=LAMBERT, **kw):
    return dict(cfg=dict(C1, material=material, **kw), meshes=[fixture_mesh("cornell_box")])


def _glass(reflect, refract, **more):
    return dict(kind="blinn", kd=(0.7, 0.8, 0.9), specExp=20.0, specAmt=0.3, reflectAmt=reflect, refractAmt=refract,
                ior=1.5, **more)


def deterministic_cases():
    """name -> case, each rendered by Scene::adaptiveSampleScene with nothing random in the result."""
    c = {}
    c["lambert_point"] = _box(dict(kind="lambert", kd=(1, 1, 1)))
    for e in (1.0, 7.5, 30.0, 200.0):
        c["blinn_specexp_%g" % e] = _box(dict(kind="blinn", kd=(0.7, 0.6, 0.5), specExp=e, specAmt=0.6))
    c["lambert_no_cast_shadows"] = dict(_box(), extra=[(quads()[:4], LAMBERT)],
                                        lights=[dict(POINT[0], cast_shadows=False)])
    c["point_transparent_shadows"] = dict(_box(), extra=[(quads()[:4], LAMBERT)], lights=[dict(POINT[0], fast_shadows=False)])
    for name in HDRS:
        for cam in ENV_CAMS:
            c["scene_env_%s_%s" % (name[:-4], cam)] = dict(
                cfg=dict(C1, material=LAMBERT, env=dict(sky=name, exposure=1.3)), extra=[(quads()[:4], LAMBERT)],
                camera=ENV_CAMS[cam], size=(33, 33))
    maps = synthetic_maps()
    c["colour_specular_normal_maps"] = dict(
        cfg=dict(C1, material=LAMBERT),
        extra=[(wall_uv(fixture_mesh("cornell_box")), dict(kind="blinn", kd=(1, 1, 1), specExp=12.0, specAmt=0.5, maps=maps))])
    # a loaded mesh whose normals are shared between triangles (every slot's tangent frame is the last
    # writer's, src/TriangleMesh.cpp:132-147) and whose uv has no degenerate triangle
    c["normal_map_shared_normals"] = dict(
        cfg=dict(C1, material=LAMBERT), lights=[dict(type="point", pos=(3.0, 6.0, 4.0), power=150.0)],
        camera=dict(eye=(0.0, 2.5, 5.0), lookAt=(0.0, 1.4, 0.0), up=(0, 1, 0), fov=45.0),
        extra=[(ref_model("sphere2.obj"), dict(kind="blinn", kd=(1, 1, 1), specExp=12.0, specAmt=0.5,
                                               maps=dict(color=maps["color"], normal=maps["normal"])))])
    img, typ = leaf_image()
    leaf = dict(kind="blinn", kd=(1, 1, 1), specExp=6.0, specAmt=0.2, maps=dict(color=(img, typ), alpha=(img, typ)))
    c["alpha_map_any_hit"] = dict(_box(), extra=[(quads(), leaf)])
    inst = ([LEAF_OBJ], [(0, M) for M in placements()])
    c["alpha_map_inside_instances"] = dict(cfg=dict(C1, material=leaf), instances=inst,
                                           extra=[(fixture_mesh("cornell_box"), LAMBERT)])
    c["instances_scaled_rotated"] = dict(cfg=dict(C1, material=dict(kind="blinn", kd=(0.9, 0.5, 0.3), specExp=15.0, specAmt=0.4)),
                                         instances=inst, extra=[(fixture_mesh("cornell_box"), LAMBERT)])
    c["blinn_reflect_0_refract_0"] = dict(_box(), extra=[(quads()[:4], _glass(0.0, 0.0))])
    return c


def replay_cases():
    """name -> case, one sample per pixel, the reference fed the oracle's draws (ref_driver replay)."""
    c = {}
    glass = _glass(0.0, 1.0)
    # every material a shadow ray can meet is a Blinn here: the transparent walk multiplies by the hit
    # material's m_refractAmt (src/RectangleLight.cpp:105), which Lambert's constructor never sets
    matte = dict(kind="blinn", kd=(0.8, 0.8, 0.8))
    for n in (1, 8, 16):
        for fast in (True, False):
            # noise 0.05 against the default 0.001: some pixels stop after the first batch of samples
            light = dict(RECT, samples=n, noise=0.05 if n > 1 else 0.001, fast_shadows=fast)
            extra = [(quads(4, y=(0.5, 2.0))[:4], matte)] + ([] if fast else [(canopy(), glass)])
            c["rect_%d_%s" % (n, "fast" if fast else "transparent")] = dict(
                _box(matte), lights=[light], camera=FLOOR_CAM, extra=extra)
    inst = ([LEAF_OBJ], [(0, M) for M in placements()])
    dome = dict(type="dome", sky="Arches_E_PineTree.hdr", power=0.15, samples=6)
    c["dome_6_over_instances"] = dict(cfg=dict(C1, material=LAMBERT), instances=inst, lights=[dome],
                                      extra=[(quads(3, seed=2)[:4], LAMBERT)], camera=ENV_CAMS["down"])
    c["depth_of_field"] = dict(_box(), extra=[(quads()[:4], LAMBERT)], camera=dict(CAM, aperture=0.3, focusPlane=7.0))
    ground, ball, v2 = cannonball_parts()
    c["motion_blur_cannonball"] = dict(cfg=BALL_CFG, meshes=[ground], moving=[(ball, v2, dict(kind="lambert", kd=(0.3, 0.3, 0.35)))],
                                       camera=dict(BALL_CAM, shutterSpeed=0.6))
    # Blinn's roulette (src/Blinn.cpp:195-246) reads its draw whatever the amounts are: direct light
    # if draw <= 1 - Rs * reflectAmt - Ts * refractAmt, so amounts of exactly 0 and 1 decide it only
    # together with the draw.  Replayed, both sides read the same draw at level 0; the secondary ray
    # then lands on a Lambert wall under a point light (or leaves the box), where nothing is drawn.
    for refl, refr in ((1.0, 0.0), (0.0, 1.0), (1.0, 1.0)):
        c["blinn_reflect_%g_refract_%g" % (refl, refr)] = dict(_box(), extra=[(quads(4, seed=8)[:4], _glass(refl, refr))])
    for name in HDRS:
        c["material_env_%s" % name[:-4]] = dict(
            cfg=dict(C1, material=LAMBERT), size=(33, 33),
            extra=[(quads(4, seed=8)[:4], dict(_glass(1.0, 1.0), env=dict(sky=name, exposure=0.8)))])
    c4, c5 = scenes.CONFIGS["C4"], scenes.CONFIGS["C5"]
    c["c4_blinn_rect_light"] = dict(_box(c4["material"]), lights=[dict(RECT, samples=1)], extra=[(quads()[:4], c4["material"])])
    c["c5_dome_instances"] = dict(cfg=dict(C1, material=c5["material"]), instances=inst,
                                  lights=[dict(dome, samples=c5["lights"][0].get("samples", 1))],
                                  extra=[(quads(3, seed=2)[:4], c5["material"])], camera=ENV_CAMS["down"])
    return c


def sphere(radius, centre):
    """sphere2.obj (closed, 960 triangles, shared normals) as mesh arrays, scaled about its own
    centre to `radius` and moved to `centre`."""
    def load():
        s = O.OracleScene()
        return s.mesh_arrays(s.add_obj(ref_model("sphere2.obj"), s.add_material("lambert")))
    v, n, vi, ni = _once("sphere2", load)
    c = (v.min(0) + v.max(0)) * np.float32(0.5)
    r = np.float32((v.max(0) - v.min(0)).max() * 0.5)
    return ((v - c) * (np.float32(radius) / r) + np.asarray(centre, np.float32)).astype(np.float32), n, vi, ni


def room(lo=(0.0, 0.0, -5.5), hi=(5.5, 5.5, 0.0)):
    """A closed box of six quads, every normal pointing inwards; (verts, normals, vidx, nidx)."""
    V, N, F, NI = [], [], [], []
    for axis in range(3):
        for side in (0, 1):
            a, b = (axis + 1) % 3, (axis + 2) % 3
            q = []
            for da, db in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = [0.0, 0.0, 0.0]
                p[axis] = (lo, hi)[side][axis]; p[a] = (lo, hi)[da][a]; p[b] = (lo, hi)[db][b]
                q.append(p)
            n = [0.0, 0.0, 0.0]
            n[axis] = -1.0 if side else 1.0
            k = len(V)
            V += q; N.append(n)
            F += [(k, k + 2, k + 1), (k, k + 3, k + 2)] if side else [(k, k + 1, k + 2), (k, k + 2, k + 3)]   # wound to face inwards too
            NI += [(len(N) - 1,) * 3] * 2
    return np.array(V, np.float32), np.array(N, np.float32), np.array(F, np.uint32), np.array(NI, np.uint32)


def corner():
    """Three large quads in the open: a floor and two walls meeting in a corner; (verts, normals, vidx, nidx)."""
    V = np.array([(0, 0, 0), (6, 0, 0), (6, 0, -6), (0, 0, -6),          # floor, +y
                  (0, 0, -6), (6, 0, -6), (6, 5, -6), (0, 5, -6),        # back wall, +z
                  (0, 0, 0), (0, 0, -6), (0, 5, -6), (0, 5, 0)], np.float32)   # left wall, +x
    N = np.array([(0, 1, 0), (0, 0, 1), (1, 0, 0)], np.float32)
    F = np.array([(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7), (8, 9, 10), (8, 10, 11)], np.uint32)
    return V, N, F, np.repeat(np.arange(3, dtype=np.uint32), 2)[:, None].repeat(3, 1)


# A Blinn whose Fresnel term is large at every angle (ior 50: Rs = 0.92 head-on), so that reflectAmt
# decides how often a reflection ray goes out, and chains last.  The roulette draws twice (leave direct
# light, then take the reflection), so that is with probability (reflectAmt * Rs) squared.
MIRROR = dict(kind="blinn", kd=(0.7, 0.7, 0.7), specExp=20.0, specAmt=0.3, reflectAmt=0.9, refractAmt=0.0, ior=50.0)
GLASS = _glass(0.3, 0.9)
DEEP_CAM = dict(eye=(2.75, 2.75, 6.0), lookAt=(2.75, 2.75, 0.0), up=(0, 1, 0), fov=32.0)
SPHERE_ROW = [((2.75, 2.75, 2.2), 1.0), ((2.75, 2.75, -0.6), 1.2), ((2.75, 2.75, -3.6), 1.4)]


def deep_cases():
    """name -> case whose chains go past level 0: the reference runs Scene::adaptiveSampleScene on
    the oracle's logged draws (ref_driver replaylog), every level, path and eye ray.  Each puts one
    piece of Blinn::shade at level >= 1 (tests/test_reference_cpu.py asserts, from the oracle's
    log alone, that it gets there).  Lambert never recurses, so what carries a chain is a Blinn.
    The cases keep to DESIGN.md section 7's traps: every light here casts fast shadows, so no
    transparent shadow walk meets a Lambert; no case uses a normal map; emitters are set through
    the setters; and a wall that must reflect faces the ray (mirror_box)."""
    c = {}
    rect1 = dict(RECT, samples=1)
    # a closed room whose six walls all face inwards (a wall seen from behind pops the ray's IOR history
    # and the Fresnel term falls to nothing): no reflection leaves it, and every hit reflects alike
    walls = dict(MIRROR, reflectAmt=0.6, ior=1000.0)
    c["mirror_box"] = dict(cfg=dict(C1, material=walls), meshes=[room()],
                           camera=dict(eye=(2.6, 2.9, -0.3), lookAt=(2.2, 2.4, -5.5), up=(0, 1, 0), fov=70.0))
    # three spheres in a row along the view axis: in, out, in, out, in, out is level 5
    row = [(sphere(r, p), GLASS) for p, r in SPHERE_ROW]
    c["glass_sphere"] = dict(_box(), lights=[rect1], extra=row, camera=DEEP_CAM)
    c["glass_in_glass"] = dict(_box(), lights=[rect1], camera=DEEP_CAM,
                               extra=[(sphere(1.7, (2.75, 2.75, 0.5)), GLASS),
                                      (sphere(0.9, (2.75, 2.75, 0.5)), dict(GLASS, ior=1.8))])
    glossy = dict(MIRROR, specGloss=0.8)
    c["glossy_rect"] = dict(_box(glossy), lights=[dict(RECT, samples=4, noise=0.05)])
    c["dispersion_sphere"] = dict(_box(), lights=[rect1], camera=DEEP_CAM,
                                  extra=[(sphere(1.5, (2.75, 2.75, 1.0)), _glass(0.3, 0.9, disperse=True, ior3=(1.45, 1.5, 1.6)))])
    img, typ = leaf_image()
    c["translucent_behind_mirror"] = dict(
        _box(MIRROR), lights=[dict(RECT, samples=2)], camera=FLOOR_CAM,
        extra=[(quads(), dict(kind="blinn", kd=(1, 1, 1), translucency=0.4, maps=dict(color=(img, typ))))])
    maps = synthetic_maps()
    grey = lambda seed: (np.random.default_rng(seed).uniform(0.2, 1.0, (48, 64)).astype(np.float32), TEX_GRAY)  # noqa: E731
    c["reflect_refract_maps"] = dict(
        _box(MIRROR), lights=[rect1],
        extra=[(quads(), dict(_glass(0.9, 0.9), maps=dict(color=maps["color"], reflect=grey(21), refract=grey(22))))])
    matte = dict(kind="blinn", kd=(0.8, 0.8, 0.8))
    emitter = dict(kind="blinn", kd=(1, 1, 1), emitted=2.0, le=(1.0, 0.9, 0.7))
    c["path_trace_3"] = dict(_box(matte), path_trace=(3, False), lights=[dict(RECT, samples=2)],
                             extra=[(quads()[:4], emitter)])
    c["path_trace_env"] = dict(cfg=dict(C1, material=matte, env=dict(sky="Arches_E_PineTree.hdr", exposure=1.3)),
                               meshes=[corner()], path_trace=(3, True), lights=[rect1],
                               extra=[(quads(3, seed=2)[:4], matte)],
                               camera=dict(eye=(5.5, 4.0, 0.5), lookAt=(1.5, 0.5, -4.0), up=(0, 1, 0), fov=50.0))
    # the eye inside the first sphere: every camera ray meets a back face at level 0, where Blinn::shade
    # pops the camera ray's own IOR history, and the four paths share that ray (src/Scene.cpp:228-231)
    c["num_paths_4"] = dict(c["glass_sphere"], num_paths=4, camera=dict(DEEP_CAM, eye=(2.75, 2.75, 2.2), fov=60.0))
    c["supersampled_dof"] = dict(c["glossy_rect"], subdivs=(1, 3, 0.01),
                                 camera=dict(eye=(2.75, 2.75, 9.0), lookAt=(2.75, 2.75, 0.0), up=(0, 1, 0), fov=55.0,
                                             aperture=0.3, focusPlane=11.0))
    ground, ball, v2 = cannonball_parts()
    # a mirror ceiling over the ground: the two reflect each other, and the moving ball, for as long as a chain lasts
    lid = (np.array([(-3, 1.0, -3), (3, 1.0, -3), (3, 1.0, 3), (-3, 1.0, 3)], np.float32), np.array([(0, -1, 0)], np.float32),
           np.array([(0, 1, 2), (0, 2, 3)], np.uint32), np.zeros((2, 3), np.uint32))
    c["motion_blur_mirror"] = dict(cfg=dict(BALL_CFG, material=MIRROR), meshes=[ground], moving=[(ball, v2, MIRROR)],
                                   extra=[(lid, MIRROR)], lights=[dict(type="point", pos=(1.0, 0.8, 1.0), power=8.0)],
                                   camera=dict(BALL_CAM, shutterSpeed=0.6))
    c["instanced_glass"] = dict(cfg=dict(C1, material=GLASS), lights=[rect1],
                                instances=([ref_model("sphere2.obj")], [(0, M) for M in placements()]),
                                extra=[(fixture_mesh("cornell_box"), LAMBERT)], camera=dict(CAM, fov=40.0))
    return c


def decode_key(keys):
    """A draw log's (skey, dim) pairs as columns (sample, path, level, branch, k); camera draws are level -1."""
    keys = np.asarray(keys, np.uint32).reshape(-1, 2).astype(np.int64)
    skey, dim = keys[:, 0], keys[:, 1]
    return np.stack([skey // 1024, skey % 1024, (dim >> 24) - 1, (dim >> 16) & 0xFF, dim & 0xFFFF], 1)


# images whose decoding the reference's own loader is asked for (RawImage::loadImage)
def decode_images():
    from miro import final_scene
    out = {name: ref_hdr_images()[name] for name in HDRS}
    out["Tree_03_Leaves.tga"] = LEAF_TGA
    for name in ("bw2.tga", "petal-pink-02.tga"):
        out[name] = final_scene.asset(name)
    return out


def oracle_decode(path):
    return O.hdr_load(path) if path.lower().endswith(".hdr") else O.image_load(path)[0]


def map_inputs():
    """The floats Map() is compared on: 0, the smallest normal, k / 32768 for a seeded sample of
    512 k with one ulp either side, 1, 1 + ulp, 4 and 1e30.  No negative and no NaN inputs: the
    reference's cast is undefined there and the oracle documents its deviation."""
    k = np.sort(np.random.default_rng(168).choice(np.arange(1, 32768), 512, replace=False))
    x = (k / 32768.0).astype(np.float32)
    one = np.float32(1.0)
    return np.concatenate([np.array([0.0, np.finfo(np.float32).tiny], np.float32), _ulp(x, -1), x, _ulp(x, 1),
                           np.array([one, np.nextafter(one, np.float32(2.0)), 4.0, 1e30], np.float32)]).astype(np.float32)


STAT_K = 64
STAT_SIZE = (32, 32)


def statistical_cases():
    """name -> case whose frame spans chain levels: compared with the reference's own
    distribution over STAT_K replicas.  Settings chosen so that a held-out replica of the
    reference passes the test's three assertions (recorded in reference.json)."""
    c = {}
    c["glossy_roulette"] = dict(_box(), extra=[(quads()[:4], _glass(0.5, 0.5, specGloss=0.8))], num_paths=128,
                                lights=[dict(RECT, samples=1)])
    c["dispersion"] = dict(_box(), num_paths=32, lights=[dict(RECT, samples=2)],
                           extra=[(quads()[:4], _glass(0.5, 0.5, disperse=True, ior3=(1.57, 1.60, 1.62)))])
    img, typ = leaf_image()
    c["translucency"] = dict(_box(), num_paths=8, lights=[dict(RECT, samples=4)],
                             extra=[(quads(), dict(kind="blinn", kd=(1, 1, 1), translucency=0.4, maps=dict(color=(img, typ))))])
    c["path_trace_emissive"] = dict(_box(dict(kind="blinn", kd=(0.8, 0.8, 0.8))), num_paths=64, path_trace=(3, False),
                                    extra=[(quads()[:4], dict(kind="blinn", kd=(1, 1, 1), emitted=2.0, le=(1.0, 0.9, 0.7)))])
    # no hard silhouettes inside the box: a jittered eye ray that seldom crosses one is an event too
    # rare for 64 replicas to have seen, whatever the sample count
    c["adaptive_subdivs"] = dict(_box(), lights=[dict(RECT, samples=1)], subdivs=(1, 3, 0.01))
    return c


def case_camera(case):
    return case.get("camera", case["cfg"]["camera"])


def case_size(case):
    return case.get("size", (W, H))


def pair_args(case):
    """(cfg, kwargs) for helpers.scene_pair; sky names resolved to images."""
    kw = {k: v for k, v in case.items() if k not in ("cfg", "camera", "size")}
    cfg = dict(case["cfg"])
    if cfg.get("env"):
        cfg["env"] = dict(cfg["env"], sky=_sky(cfg["env"]["sky"]))
    lights = kw.get("lights", cfg["lights"])
    kw["lights"] = [dict(l, sky=_sky(l["sky"])) if l["type"] == "dome" else l for l in lights]
    kw["extra"] = [(a, dict(m, env=dict(m["env"], sky=_sky(m["env"]["sky"]))) if m.get("env") else m)
                   for a, m in kw.get("extra", [])]
    return cfg, kw


def _sky(spec):
    return hdr(spec) if isinstance(spec, str) else spec


# ------------------------------------------------------------------ oracle + reference scenes
class _Both:
    """An OracleScene and a RefScene taking the same calls: what helpers.scene_pair tells the
    oracle, it tells both, and both must answer with the same ids."""

    def __init__(self, Os, Rs):
        self.Os, self.Rs = Os, Rs

    def add_obj(self, path, material):
        mid = self.Os.add_obj(path, material)       # the driver's hit ids need the triangle count
        assert self.Rs.add_obj(path, material, len(self.Os.mesh_arrays(mid)[2])) == mid
        return mid

    def __getattr__(self, name):
        fo, fr = getattr(self.Os, name), getattr(self.Rs, name)

        def call(*a, **kw):
            r = fo(*a, **kw)
            assert fr(*a, **kw) == r, name
            return r
        return call


def build_scenes(case, want_ref):
    """(OracleScene, RefScene or None) of a case, built by helpers.scene_pair itself: the one
    builder the GPU tests use for the product, so the three cannot drift apart."""
    from helpers import scene_pair
    cfg, kw = pair_args(case)
    Os = O.OracleScene()
    Rs = None
    if want_ref:
        import refdriver
        Rs = refdriver.RefScene()
    scene_pair(cfg, oracle=Os if Rs is None else _Both(Os, Rs), **kw)
    return Os, Rs


# ------------------------------------------------------------------ traversal: models and ray sets
TRACE_MODELS = ("cornell_box", "teapot", "explosion01")
N_RANDOM = 6000


def trace_mesh(model):
    return fixture_mesh(model)


def _ulp(x, k):
    return (np.ascontiguousarray(x, np.float32).view(np.int32) + np.int32(k)).view(np.float32)


def ray_set(model, hits_of):
    """The rays of one model, by class: (o (n, 3), d (n, 3), tmin (n,), tmax (n,), class (n,) names).
    hits_of(o, d) -> the full-ray hit distances of some tracer (for the tMax classes: the oracle's,
    so the set is the same with or without the reference)."""
    V, _, F, _ = trace_mesh(model)
    V = np.asarray(V, np.float32); F = np.asarray(F, np.int64)
    rng = np.random.default_rng(sum(map(ord, model)))
    lo, hi = V.min(0), V.max(0)
    ext = float((hi - lo).max())
    ctr = (lo + hi) / 2
    O_, D_, C_ = [], [], []

    def add(o, d, name):
        o = np.asarray(o, np.float32).reshape(-1, 3); d = np.asarray(d, np.float32).reshape(-1, 3)
        O_.append(o); D_.append(d); C_.extend([name] * len(o))

    def unit(n):
        d = rng.normal(size=(n, 3))
        return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)

    def outside(n):
        return (ctr + unit(n) * ext * rng.uniform(0.8, 1.6, (n, 1))).astype(np.float32)

    # random: from outside towards a point of the box, and from inside in any direction
    o = outside(N_RANDOM // 2)
    tgt = rng.uniform(lo, hi, (len(o), 3)).astype(np.float32)
    add(o, (tgt - o) / np.linalg.norm(tgt - o, axis=1, keepdims=True), "random")
    add(rng.uniform(lo, hi, (N_RANDOM // 2, 3)), unit(N_RANDOM // 2), "random")
    # one and two direction components exactly +0 / -0
    for zero in (0.0, -0.0):
        for axes in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):
            n = 120
            d = unit(n)
            d[:, axes] = np.float32(zero)
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            d[:, axes] = np.float32(zero)
            add(rng.uniform(lo - 0.1 * ext, hi + 0.1 * ext, (n, 3)), d, "zero_component")
    tri = F[rng.integers(0, len(F), 400)]
    A, B, C = V[tri[:, 0]], V[tri[:, 1]], V[tri[:, 2]]
    # rays lying in a triangle's plane: along its edge AB from outside, both ways (in the plane up to
    # float rounding of the direction), and, where a triangle is axis-aligned (cornell_box), exactly
    # in it along an axis through a vertex
    nrm = np.cross(B - A, C - A)
    e = B - A
    e /= np.maximum(np.linalg.norm(e, axis=1, keepdims=True), np.float32(1e-30))
    add(A[:200] - e[:200] * np.float32(0.5 * ext), e[:200], "in_plane")
    add(B[:200] + e[:200] * np.float32(0.5 * ext), -e[:200], "in_plane")
    for k in np.nonzero((np.abs(nrm) > 0).sum(1) == 1)[0][:200]:
        free = [a for a in range(3) if nrm[k, a] == 0]
        d = np.zeros(3, np.float32); d[free[0]] = 1.0
        add(A[k] - d * np.float32(0.5 * ext), d, "in_plane")
        add(A[k] + d * np.float32(0.5 * ext), -d, "in_plane")
    # exactly at shared vertices and at edge midpoints, from outside
    o = outside(len(tri))
    add(o, A - o, "at_vertex")
    o = outside(len(tri))
    add(o, (A + B) * np.float32(0.5) - o, "at_edge")
    # origins on a surface: a point of a triangle, any direction
    w = rng.dirichlet((1, 1, 1), len(tri)).astype(np.float32)
    add(A * w[:, :1] + B * w[:, 1:2] + C * w[:, 2:], unit(len(tri)), "on_surface")
    o, d = np.concatenate(O_), np.concatenate(D_)
    cls = np.array(C_)
    tmin = np.full(len(o), 0.001, np.float32)
    tmax = np.full(len(o), 1e12, np.float32)
    # tMax at a full-ray hit's t, one ulp below it and one above
    t = np.asarray(hits_of(o, d), np.float32)
    pick = np.nonzero(t < np.float32(1e11))[0][:700]
    for k, name in ((0, "tmax_at_t"), (-1, "tmax_below_t"), (1, "tmax_above_t")):
        o, d = np.concatenate([o, o[pick]]), np.concatenate([d, d[pick]])
        tmin = np.concatenate([tmin, tmin[pick]])
        tmax = np.concatenate([tmax, _ulp(t[pick], k)])
        cls = np.concatenate([cls, np.array([name] * len(pick))])
    return o, d, tmin, tmax, cls


RAY_CLASSES = ("random", "zero_component", "in_plane", "at_vertex", "at_edge", "on_surface", "tmax_at_t",
               "tmax_below_t", "tmax_above_t")


def fixture_subset(cls):
    """Indices of the rays the fixtures record: all of them (the files stay well under the size limit)."""
    return np.arange(len(cls))


def trace_scene(model, want_ref):
    case = dict(cfg=dict(C1, material=dict(kind="lambert", kd=(1, 1, 1))), meshes=[trace_mesh(model)])
    return build_scenes(case, want_ref)


def oracle_ray_set(model, Os):
    return ray_set(model, lambda o, d: Os.trace(o, d, 0.001, 1e12)[0]["t"])


LOADER_MODELS = ("cornell_box.obj", "teapot.obj", "sphere2.obj", "leaf_test.obj", "Final/explosion01.obj",
                 "Final/cannonBallT1.obj", "Final/cannonBallT2.obj", "Final/flower01Petals.obj")


def loader_path(model):
    return LEAF_OBJ if model == "leaf_test.obj" else ref_model(model)


# ------------------------------------------------------------------ the statistical tier
def t_two_sided_tail(x, df):
    """P(|t_df| > x), by the regularised incomplete beta function (continued fraction)."""
    from math import exp, lgamma, log
    a, b, z = df / 2.0, 0.5, df / (df + x * x)
    front = exp(lgamma(a + b) - lgamma(a) - lgamma(b) + a * log(z) + b * log(1 - z)) / a
    f, c, d = 1.0, 1.0, 0.0
    for i in range(400):
        m = i // 2
        if i == 0:
            num = 1.0
        elif i % 2 == 0:
            num = m * (b - m) * z / ((a + 2 * m - 1) * (a + 2 * m))
        else:
            num = -(a + m) * (a + b + m) * z / ((a + 2 * m) * (a + 2 * m + 1))
        d = 1.0 + num * d
        d = 1.0 / (d if abs(d) > 1e-300 else 1e-300)
        c = 1.0 + num / (c if abs(c) > 1e-300 else 1e-300)
        f *= c * d
        if abs(1.0 - c * d) < 1e-14:
            break
    return front * (f - 1.0)


def z_bound(n, df):
    """The |z| at which n * P(|t_df| > bound) = 1e-3."""
    lo_, hi_ = 2.0, 60.0
    for _ in range(80):
        mid = 0.5 * (lo_ + hi_)
        if n * t_two_sided_tail(mid, df) > 1e-3:
            lo_ = mid
        else:
            hi_ = mid
    return hi_


def statistics(frame, m, s, K):
    """The three figures of the statistical tier for one frame against the reference's per-value
    mean m and sample standard deviation s over K replicas (where s == 0 every replica is m).
    Returns dict(exact_mismatches, bias, max_z, bound, n, varying)."""
    f32 = np.ascontiguousarray(frame, np.float32).reshape(-1)
    frame = f32.astype(np.float64)
    m = np.asarray(m, np.float64).reshape(-1); s = np.asarray(s, np.float64).reshape(-1)
    var = s > 0
    n = int(var.sum())
    z = (frame[var] - m[var]) / (s[var] * np.sqrt(1.0 + 1.0 / K))
    exact = f32[~var].view(np.uint32) != m.astype(np.float32)[~var].view(np.uint32)
    return dict(exact_mismatches=int(exact.sum()), bias=float(abs(z.sum()) / np.sqrt(max(n, 1))),
                max_z=float(np.abs(z).max()) if n else 0.0, bound=z_bound(max(n, 1), K - 1), n=n,
                varying=n / frame.size)


def assert_statistics(st, who):
    assert st["varying"] >= 0.5, (who, st)
    assert st["exact_mismatches"] == 0, (who, st)
    assert st["bias"] < 5, (who, st)
    assert st["max_z"] < st["bound"], (who, st)


# ------------------------------------------------------------------ fixture files
def save_npz(path, arrays):
    """A compressed .npz whose bytes depend on the arrays alone (fixed member order and dates)."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def fixture(name):
    return _once("fx:" + name, lambda: dict(np.load(os.path.join(REF_DIR, name))))


def fixture_json():
    import json
    return _once("fx:json", lambda: json.load(open(os.path.join(REF_DIR, "reference.json"))))


def sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def oracle_loader_arrays(model):
    """The oracle's arrays of one OBJ: verts, normals, vidx, nidx and, with texture coordinates,
    uv, tidx and the tangent frames per normal slot (tangents, bitangents)."""
    Os = O.OracleScene()
    mid = Os.add_obj(loader_path(model), Os.add_material("lambert"))
    v, n, vi, ni = Os.mesh_arrays(mid)
    out = dict(verts=v, normals=n, vidx=vi, nidx=ni)
    uv, ti = Os.texcoords(mid)
    if len(uv):
        t, b = Os.tangents(mid)
        out.update(uv=uv, tidx=ti, tangents=t, bitangents=b)
    return out


def written_tangent_slots(m):
    """The normal slots whose tangent frame some triangle writes (src/TriangleMesh.cpp:124-148: those
    of a triangle whose uv edges have a non-zero cross product, in float as there), from a mesh's
    arrays.  The reference never initialises the others."""
    uv, ti = m["uv"], m["tidx"].astype(np.int64)
    e1, e2 = uv[ti[:, 1]] - uv[ti[:, 0]], uv[ti[:, 2]] - uv[ti[:, 0]]
    cp = e1[:, 1] * e2[:, 0] - e1[:, 0] * e2[:, 1]
    w = np.zeros(len(m["normals"]), bool)
    w[m["nidx"].astype(np.int64)[cp != 0].ravel()] = True
    return w


def reference_loader_arrays(model):
    """The reference's arrays of one OBJ (needs the driver); unwritten tangent slots zeroed, as
    the oracle holds them."""
    import refdriver
    m = refdriver.load_obj(loader_path(model))
    if "tangents" in m:
        w = written_tangent_slots(m)
        m["tangents"][~w] = 0
        m["bitangents"][~w] = 0
    return m
