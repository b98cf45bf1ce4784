"""mrt_scene_deform_mesh: new vertices for any mesh of a built scene -- a mesh of a BLAS (the
BLAS refitted, the boxes of its instances recomputed, the world tree refitted) and a
motion-blurred world mesh (both vertex sets, the MBObject boxes recomputed, the world tree
refitted); a plain world mesh goes the way of mrt_scene_update_mesh.

The yardstick is test_refit.py's numpy restatement, not the library:
  BLAS    refit_of(blas_export0, V[F[::-1]])  (a BLAS's objects: its meshes in order, each
          mesh's triangles last to first)
  boxes   instance_box(restated BLAS root, M) per instance of that BLAS
  world   refit_of(world export0, prim_verts, fixed) with those boxes (and, for MBObject
          lanes, the union of box3 at time 0 and box3 at time 1) as the fixed lanes
Scaling a mesh by a power of two leaves the build's topology as it is, so a deform to 2 V0 or
V0 / 2 is also compared with a fresh build (and the oracle) at those vertices, bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import miro
from miro import _lib, scenes
from helpers import bits, camera, tuned
from test_refit import (CAM, EMPTY, F32, INVALID, NOT_BUILT, PLACED, agreeing, assert_arrays, assert_frames, blas_mesh, box3,
                        displaced, floor_mesh, frame, import_bvh, instance_box, point_light, prim_verts_of,
                        refit_of, smax, smin, standin, tri_mesh, update_rc)
from test_refit_shapes import LANES_PER_WG, NODES_PER_WG, assert_encloses, heights, refit_arrays_by_height, same_words
from test_instance_update import (FRAME_CASES, NEW, OTHER, assert_infos, async_frame, dev, infos, mirror_blinn,
                                  scene_kw)


# ---------------------------------------------------------------- shapes
@functools.lru_cache(maxsize=None)
def big_blas_mesh():
    """The smallest even nu whose BLAS has two heights of more than 64 nodes (premise test)."""
    V, F, N = scenes.bunny_standin(46, 23, radius=0.6)
    return np.asarray(V, F32), np.asarray(N, F32), np.asarray(F, np.uint32)


BLAS_MESHES = {"small": blas_mesh, "big": big_blas_mesh}


def blas_displaced(V, F, seed, amp=0.06):
    """test_refit.displaced scaled to the BLAS sphere (radius 0.6 about (0, 0.65, 0)): a smooth
    seeded displacement of ~10 % of the radius with recomputed smooth normals."""
    rng = np.random.default_rng(seed)
    d = V - np.array([0.0, 0.65, 0.0])
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-6)
    s = sum(np.sin(V @ rng.uniform(1.5, 6.0, 3) + rng.uniform(0, 6.28)) for _ in range(3)) / 3.0
    V1 = np.asarray(V + amp * s[:, None] * d, F32)
    return V1, np.asarray(scenes._smooth_normals(V1.astype(np.float64), F.astype(np.int64)), F32)


def scaled(V, k):
    return np.asarray(V * F32(k), F32)   # a power of two: exact


def mb_sets(bV, k=1.0, shift=(0.0, 0.0, 0.0)):
    """mixed_scene's motion-blurred sphere: its time-0 and time-1 vertices (k, shift: moved)."""
    mV = np.asarray(bV * F32(0.7 * k) + np.array([0.0, 6.4, 2.0], F32) + np.array(shift, F32), F32)
    mV2 = np.asarray(mV + np.array([0.35, 0.1, 0.0], F32) * F32(k), F32)
    return mV, mV2


class Case:
    """mixed_scene with a BLAS mesh, matrices, a world mesh (or none: a world tree below 64
    nodes) and a motion-blurred mesh of choice.  World prims: the world mesh's triangles, the
    proxies, the motion-blurred triangles, the floor."""

    def __init__(self, bm, mats=PLACED, world=True, moving=True, mb=None, light=point_light, num_paths=1,
                 blas_material=None):
        self.bV, self.bN, self.bF = bm
        self.mats, self.moving = list(mats), moving
        P = self.P = miro.Scene()
        entries, self.ids, nmesh = [], {}, 0
        self.n0 = 0
        if world:
            V, N, F = standin()
            miro.makeMeshObjs(P, tri_mesh(V, N, F), miro.Lambert((0.8, 0.7, 0.6)))
            entries.append((V, F))
            self.n0 = len(F)
            self.ids["world"], nmesh = nmesh, nmesh + 1
        objs, bvh = miro.Objects(), miro.BVH()
        miro.ProxyObject.setupProxy(tri_mesh(self.bV, self.bN, self.bF), blas_material or miro.Lambert((0.3, 0.8, 0.4)), objs, bvh)
        for M in self.mats:
            P.addObject(miro.ProxyObject(objs, bvh, miro.Matrix4x4(M)))
        entries.append(len(self.mats))
        self.ids["blas"], nmesh = nmesh, nmesh + 1
        sV, sN, sF = blas_mesh()
        self.mF = sF
        if moving:
            self.mV, self.mV2 = mb if mb is not None else mb_sets(sV)
            miro.makeMBMeshObjs(P, tri_mesh(self.mV, sN, sF), tri_mesh(self.mV2, sN, sF), miro.Lambert((0.9, 0.4, 0.3)))
            entries.append((self.mV, sF))
            self.ids["mb"], nmesh = nmesh, nmesh + 1
        fl = floor_mesh()
        miro.makeMeshObjs(P, fl, miro.Lambert((0.6, 0.6, 0.6)))
        entries.append((fl.verts, fl.vidx))
        self.ids["floor"] = nmesh
        P.addLight(light())
        P.setBGColor((0.1, 0.1, 0.3))
        P.setNumPaths(num_paths)
        P.preCalc()
        self.pv = prim_verts_of(*entries)
        self.mb0 = self.n0 + len(self.mats)   # first motion-blurred prim

    def fixed(self, root, mats=None, mb=None):
        """The fixed lanes: each proxy at instance_box(root, M), each MBObject lane at the union
        of its boxes at both times."""
        out = {self.n0 + i: instance_box(root, M) for i, M in enumerate(mats or self.mats)}
        if self.moving:
            mV, mV2 = mb if mb is not None else (self.mV, self.mV2)
            for t, f in enumerate(self.mF):
                lo, hi = box3(*mV[f])
                lo2, hi2 = box3(*mV2[f])
                out[self.mb0 + t] = (smin(lo, lo2), smax(hi, hi2))
        return out

    def pv_with(self, mV=None, world=None):
        pv = self.pv.copy()
        if world is not None:
            pv[:self.n0] = world[standin()[2]]
        if mV is not None:
            pv[self.mb0:self.mb0 + len(self.mF)] = mV[self.mF]
        return pv


def refit(export, prim_verts, fixed=None):
    return refit_of(export, prim_verts, fixed, arrays=refit_arrays_by_height)


def blas_refit(blas_export0, V, F):
    """The BLAS restated at vertices V: its objects are the triangles last to first."""
    return refit(blas_export0, np.asarray(V, F32)[np.asarray(F)[::-1]])


def expected(S, blas0, ex0, bV1, mats=None, mb=None, world=None):
    """(BLAS arrays, fixed lanes, world arrays) after a deform of the BLAS mesh to bV1 (and the
    instances at mats, the motion-blurred mesh at mb = (V, V2), the world mesh at `world`)."""
    bw = blas_refit(blas0, bV1, S.bF)
    fx = S.fixed(bw[0][0], mats, mb)
    return bw, fx, refit(ex0, S.pv_with(mb[0] if mb is not None else None, world), fx)


def assert_state(P, n0, want_blas, fixed, want_world, blas=0):
    assert_arrays(P.blas_export(blas), want_blas)
    for i, inf in enumerate(infos(P)):
        if inf["blas"] != blas:
            continue
        lo, hi = fixed[n0 + i]
        assert np.array_equal(bits(inf["box"][0]), bits(lo)) and np.array_equal(bits(inf["box"][1]), bits(hi)), f"instance {i} box"
    assert_arrays(P.bvh_export(), want_world)


def deform_rc(P, mesh, verts, verts2=None, normals=None):
    a = [np.ascontiguousarray(x, F32) if x is not None else None for x in (verts, verts2, normals)]
    L = miro.lib()
    rc = L.mrt_scene_deform_mesh(P._h, mesh, *[x.ctypes.data if x is not None else None for x in a], None)
    return rc, L.mrt_last_error().decode()


# the scene of the power-of-two twins: the PLACED instances and the floor (a world mesh beside
# them would change the fresh build's world topology as the instance boxes double)
TWIN = dict(world=False, moving=False)


# ---------------------------------------------------------------- CPU tests: the premises
def test_symbols_and_wrapper():
    L = miro.lib()
    assert hasattr(L, "mrt_scene_deform_mesh") and hasattr(L, "mrt_scene_deform_mesh_async")
    assert {"mrt_scene_deform_mesh", "mrt_scene_deform_mesh_async"} <= set(_lib.EXPORTS)
    assert callable(miro.Scene.deformMesh) and L.mrt_abi_version() == 10


def test_blas_objects_are_the_triangles_last_to_first():
    """1. refit_of(blas_export, V[F[::-1]]) reproduces the export of blas_mesh()."""
    S = Case(blas_mesh())
    b0 = S.P.blas_export(0)
    assert len(S.bF) == 64 and len(b0[0]) == 5 and len(b0[2]) == 16
    h = heights(b0[1])
    assert np.bincount(h).tolist() == [4, 1]
    assert_arrays(blas_refit(b0, S.bV, S.bF), b0)
    assert_arrays(refit_of(b0, S.bV[S.bF[::-1]]), b0)   # the recursive restatement too
    with pytest.raises(AssertionError):
        assert_arrays(refit_of(b0, S.bV[S.bF]), b0)      # first to last is another BLAS


def _blas_facts(nu):
    V, F, N = scenes.bunny_standin(nu, nu // 2, radius=0.6)
    P = miro.Scene()
    objs, bvh = miro.Objects(), miro.BVH()
    miro.ProxyObject.setupProxy(tri_mesh(np.asarray(V, F32), np.asarray(N, F32), np.asarray(F, np.uint32)), miro.Lambert(), objs, bvh)
    P.addObject(miro.ProxyObject(objs, bvh, miro.Matrix4x4(PLACED[0])))
    P.preCalc()
    b = P.blas_export(0)
    return np.bincount(heights(b[1])).tolist(), len(b[2]), len(F)


def test_the_big_blas_is_the_smallest_with_several_workgroups_per_height():
    """1. two heights of more than 64 nodes, ragged, and a ragged lane count."""
    counts, leaves, tris = _blas_facts(46)
    assert (tris, leaves, counts) == (2024, 548, [172, 73, 20, 7, 3, 1, 1])
    wide = [c for c in counts if c > NODES_PER_WG]
    assert len(wide) == 2 and all(c % NODES_PER_WG for c in wide) and (4 * leaves) % LANES_PER_WG != 0
    for nu in range(8, 46, 2):
        assert sum(c > NODES_PER_WG for c in _blas_facts(nu)[0]) < 2, nu
    V, N, F = big_blas_mesh()
    assert len(F) == 2024


@pytest.mark.parametrize("size", ["small", "big"])
@pytest.mark.parametrize("k", [2.0, 0.5])
def test_a_power_of_two_keeps_the_topology(size, k):
    """1. the fresh build at k V0: same topology, the restated arrays, the restated boxes."""
    bm = BLAS_MESHES[size]()
    S0 = Case(bm, **TWIN)
    S1 = Case((scaled(bm[0], k), bm[1], bm[2]), **TWIN)
    b0, b1 = S0.P.blas_export(0), S1.P.blas_export(0)
    assert np.array_equal(b0[1], b1[1]) and np.array_equal(b0[3], b1[3])
    assert_arrays(b1, blas_refit(b0, scaled(bm[0], k), bm[2]))
    e0, e1 = S0.P.bvh_export(), S1.P.bvh_export()
    assert np.array_equal(e0[1], e1[1]) and np.array_equal(e0[3], e1[3])
    for i, M in enumerate(PLACED):
        lo, hi = instance_box(b1[0][0], M)
        assert np.array_equal(bits(S1.P.instance_info(i)["box"]), bits(np.stack([lo, hi])))


# ---------------------------------------------------------------- CPU tests: the host path
@pytest.mark.parametrize("size", ["small", "big"])
def test_host_deform_of_a_blas_mesh(size):
    """2. a never-uploaded scene: the BLAS, the instance boxes, the world tree; and back."""
    bm = BLAS_MESHES[size]()
    S = Case(bm)
    P = S.P
    blas0, ex0, inf0 = P.blas_export(0), P.bvh_export(), infos(P)
    bV1, bN1 = blas_displaced(bm[0], bm[2], 3)
    assert P.deformMesh(S.ids["blas"], bV1, bN1) == 0.0
    bw, fx, ww = expected(S, blas0, ex0, bV1)
    assert_state(P, S.n0, bw, fx, ww)
    assert not np.array_equal(bw[0], blas0[0]) and not np.array_equal(ww[0], ex0[0])
    assert_infos(infos(P), inf0, keys=("m", "inv", "inv_t"))       # the matrices stay
    assert not np.array_equal(infos(P)[0]["box"], inf0[0]["box"])
    v, n, _, _ = P.mesh_arrays(S.ids["blas"])
    assert np.array_equal(v, bV1) and np.array_equal(n, bN1)
    assert_encloses(P.blas_export(0), bV1[bm[2][::-1]])
    assert_encloses(P.bvh_export(), S.pv, fx)
    assert P.deformMesh(S.ids["blas"], bm[0], bm[1]) == 0.0        # boxes shrink as well as grow
    assert_arrays(P.blas_export(0), blas0)
    assert_arrays(P.bvh_export(), ex0)
    assert_infos(infos(P), inf0)


@pytest.mark.parametrize("k", [2.0, 0.5])
def test_host_deform_to_a_power_of_two_is_a_fresh_build(k):
    """3. exports and instance infos equal a fresh scene's."""
    bm = blas_mesh()
    S = Case(bm, **TWIN)
    S.P.deformMesh(S.ids["blas"], scaled(bm[0], k))
    T = Case((scaled(bm[0], k), bm[1], bm[2]), **TWIN)
    assert_arrays(S.P.blas_export(0), T.P.blas_export(0))
    assert_arrays(S.P.bvh_export(), T.P.bvh_export())
    assert_infos(infos(S.P), infos(T.P))


def two_mesh_blas(second=None):
    """A BLAS of two meshes (setupMultiProxy): the small sphere and a copy beside it."""
    bV, bN, bF = blas_mesh()
    V2 = np.asarray(bV + np.array([1.5, 0.0, 0.0], F32), F32) if second is None else second
    P = miro.Scene()
    objs, bvh = miro.Objects(), miro.BVH()
    miro.ProxyObject.setupMultiProxy([tri_mesh(bV, bN, bF), tri_mesh(V2, bN, bF)], 2,
                                     [miro.Lambert((0.3, 0.8, 0.4)), miro.Lambert((0.8, 0.3, 0.4))], objs, bvh)
    for M in PLACED:
        P.addObject(miro.ProxyObject(objs, bvh, miro.Matrix4x4(M)))
    fl = floor_mesh()
    miro.makeMeshObjs(P, fl, miro.Lambert((0.6, 0.6, 0.6)))
    P.addLight(point_light())
    P.preCalc()
    return P, V2, prim_verts_of(len(PLACED), (fl.verts, fl.vidx))


def test_the_second_mesh_of_a_two_mesh_blas():
    """4. the first mesh's lanes keep their bits."""
    bV, bN, bF = blas_mesh()
    P, V2, pv = two_mesh_blas()
    blas0, ex0 = P.blas_export(0), P.bvh_export()
    objs0 = np.concatenate([bV[bF[::-1]], V2[bF[::-1]]])   # meshes in order, each last to first
    assert_arrays(refit(blas0, objs0), blas0)
    V2n, N2n = blas_displaced(bV, bF, 5)
    V2n = np.asarray(V2n + np.array([1.5, 0.0, 0.0], F32), F32)
    P.deformMesh(1, V2n, N2n)
    want = refit(blas0, np.concatenate([bV[bF[::-1]], V2n[bF[::-1]]]))
    got = P.blas_export(0)
    assert_arrays(got, want)
    first = (blas0[3] >= 0) & (blas0[3] < len(bF))          # lanes of mesh 0
    lt0, lt1 = blas0[2].reshape(-1, 9, 4), got[2].reshape(-1, 9, 4)
    assert first.sum() == len(bF) and np.array_equal(bits(lt0.transpose(0, 2, 1)[first]), bits(lt1.transpose(0, 2, 1)[first]))
    assert not np.array_equal(lt0, lt1)
    fx = {i: instance_box(want[0][0], M) for i, M in enumerate(PLACED)}
    assert_arrays(P.bvh_export(), refit(ex0, pv, fx))
    assert np.array_equal(P.mesh_arrays(0)[0], bV)


def two_blas_scene():
    """Two BLASes (the small sphere, a tetrahedron-like coarse sphere), two instances of each."""
    bV, bN, bF = blas_mesh()
    cV, cF, cN = scenes.bunny_standin(6, 4, radius=0.5)
    cV, cN, cF = np.asarray(cV, F32), np.asarray(cN, F32), np.asarray(cF, np.uint32)
    mats = [PLACED[0], NEW[1], PLACED[1], OTHER[0]]
    P = miro.Scene()
    pairs = []
    for V, N, F in ((bV, bN, bF), (cV, cN, cF)):
        objs, bvh = miro.Objects(), miro.BVH()
        miro.ProxyObject.setupProxy(tri_mesh(V, N, F), miro.Lambert((0.3, 0.8, 0.4)), objs, bvh)
        pairs.append((objs, bvh))
    for i, M in enumerate(mats):   # instances 0, 2 of BLAS 0; 1, 3 of BLAS 1
        P.addObject(miro.ProxyObject(*pairs[i % 2], miro.Matrix4x4(M)))
    fl = floor_mesh()
    miro.makeMeshObjs(P, fl, miro.Lambert((0.6, 0.6, 0.6)))
    P.addLight(point_light())
    P.setBGColor((0.1, 0.1, 0.3))
    P.preCalc()
    return P, mats, prim_verts_of(len(mats), (fl.verts, fl.vidx))


def test_the_other_blas_keeps_its_bits():
    """5. BLAS 1's export and its instances' boxes after a deform of BLAS 0."""
    bV, bN, bF = blas_mesh()
    P, mats, pv = two_blas_scene()
    assert [i["blas"] for i in infos(P)] == [0, 1, 0, 1]
    b0, b1, ex0, inf0 = P.blas_export(0), P.blas_export(1), P.bvh_export(), infos(P)
    bV1, bN1 = blas_displaced(bV, bF, 7)
    P.deformMesh(0, bV1, bN1)
    want = blas_refit(b0, bV1, bF)
    assert_arrays(P.blas_export(0), want)
    assert_arrays(P.blas_export(1), b1)
    got = infos(P)
    assert_infos([got[1], got[3]], [inf0[1], inf0[3]])
    fx = {i: (instance_box(want[0][0], mats[i]) if i % 2 == 0 else (inf0[i]["box"][0], inf0[i]["box"][1])) for i in range(4)}
    for i in (0, 2):
        assert np.array_equal(bits(got[i]["box"]), bits(np.stack(fx[i]))) and not np.array_equal(got[i]["box"], inf0[i]["box"])
    assert_arrays(P.bvh_export(), refit(ex0, pv, fx))


def test_host_deform_of_a_motion_blurred_mesh_and_of_a_plain_one():
    """6. the union boxes of the new vertex sets; a plain world mesh equals updateMesh."""
    S = Case(blas_mesh())
    P = S.P
    ex0, blas0, inf0 = P.bvh_export(), P.blas_export(0), infos(P)
    mb1 = mb_sets(blas_mesh()[0], k=1.25, shift=(0.4, -0.3, 0.2))
    assert P.deformMesh(S.ids["mb"], mb1[0], verts2=mb1[1]) == 0.0
    fx = S.fixed(blas0[0][0], mb=mb1)
    want = refit(ex0, S.pv_with(mb1[0]), fx)
    assert_arrays(P.bvh_export(), want)
    assert not np.array_equal(want[0], ex0[0])
    lanes = np.isin(ex0[3], np.arange(S.mb0, S.mb0 + len(S.mF)))   # the lanes' triangle data stays zero
    assert lanes.sum() == len(S.mF) and not P.bvh_export()[2].reshape(-1, 9, 4).transpose(0, 2, 1)[lanes].any()
    assert_arrays(P.blas_export(0), blas0)
    assert_infos(infos(P), inf0)
    assert np.array_equal(P.mesh_arrays(S.ids["mb"])[0], mb1[0])
    # time 1 alone moves: the boxes follow the second set too
    mb2 = (mb1[0], np.asarray(mb1[1] + np.array([0.0, 0.5, 0.0], F32), F32))
    P.deformMesh(S.ids["mb"], mb2[0], verts2=mb2[1])
    assert_arrays(P.bvh_export(), refit(ex0, S.pv_with(mb2[0]), S.fixed(blas0[0][0], mb=mb2)))
    # a plain world mesh through the new entry: updateMesh's result
    V, N, F = standin()
    V1, N1 = displaced(V, F, 1)
    A, B = Case(blas_mesh()), Case(blas_mesh())
    assert A.P.deformMesh(0, V1, N1) == 0.0
    B.P.updateMesh(0, V1, N1)
    assert_arrays(A.P.bvh_export(), B.P.bvh_export())
    assert np.array_equal(A.P.mesh_arrays(0)[0], V1) and np.array_equal(A.P.mesh_arrays(0)[1], N1)


def test_refusals():
    """7. every code and message, all before any change; update_mesh still refuses both kinds."""
    S = Case(blas_mesh())
    P, L = S.P, miro.lib()
    V, N, F = standin()
    bV, bN, bF = blas_mesh()
    ex0, blas0, inf0 = P.bvh_export(), P.blas_export(0), infos(P)
    meshes0 = [P.mesh_arrays(m) for m in range(4)]
    v = np.ascontiguousarray(bV, F32)
    assert L.mrt_scene_deform_mesh(None, 1, v.ctypes.data, None, None, None) == INVALID
    assert L.mrt_scene_deform_mesh(P._h, 1, None, None, None, None) == INVALID and b"null vertices" in L.mrt_last_error()
    for bad in (-1, 4, 1000):
        rc, msg = deform_rc(P, bad, bV)
        assert rc == INVALID and "bad mesh id" in msg
    rc, msg = deform_rc(P, S.ids["blas"], bV, verts2=bV)
    assert rc == INVALID and "BLAS" in msg and "inert" in msg
    rc, msg = deform_rc(P, S.ids["world"], V, verts2=V)
    assert rc == INVALID and "without" in msg
    rc, msg = deform_rc(P, S.ids["mb"], S.mV)
    assert rc == INVALID and "motion vertices" in msg and "both" in msg
    for val in (np.nan, np.inf, -np.inf):
        bad = bV.copy(); bad[17, 1] = val
        rc, msg = deform_rc(P, S.ids["blas"], bad)
        assert rc == INVALID and "vertex 17 " in msg and "finite" in msg
        badn = bN.copy(); badn[9, 2] = val
        rc, msg = deform_rc(P, S.ids["blas"], bV, normals=badn)
        assert rc == INVALID and "normal 9 " in msg
        bad2 = S.mV2.copy(); bad2[5, 0] = val
        rc, msg = deform_rc(P, S.ids["mb"], S.mV, verts2=bad2)
        assert rc == INVALID and "motion vertex 5 " in msg
        bad0 = S.mV.copy(); bad0[6, 0] = val
        rc, msg = deform_rc(P, S.ids["mb"], bad0, verts2=S.mV2)
        assert rc == INVALID and "vertex 6 " in msg and "motion vertex" not in msg
    # the async form: ids and kinds, and a scene that is not on a device (the pointers are never read)
    fake = C.c_void_p(v.ctypes.data)
    assert L.mrt_scene_deform_mesh_async(None, 1, fake, None, None, None) == INVALID
    assert L.mrt_scene_deform_mesh_async(P._h, 1, None, None, None, None) == INVALID
    assert L.mrt_scene_deform_mesh_async(P._h, 7, fake, None, None, None) == INVALID and b"bad mesh id" in L.mrt_last_error()
    assert L.mrt_scene_deform_mesh_async(P._h, S.ids["blas"], fake, fake, None, None) == INVALID and b"inert" in L.mrt_last_error()
    assert L.mrt_scene_deform_mesh_async(P._h, S.ids["mb"], fake, None, None, None) == INVALID and b"both" in L.mrt_last_error()
    for m, v2 in ((S.ids["blas"], None), (S.ids["mb"], fake), (S.ids["world"], None)):
        assert L.mrt_scene_deform_mesh_async(P._h, m, fake, v2, None, None) == INVALID
        assert b"exactly one device" in L.mrt_last_error()
    # mrt_scene_update_mesh still refuses both kinds
    rc, msg = update_rc(P, S.ids["blas"], bV)
    assert rc == INVALID and "BLAS" in msg
    rc, msg = update_rc(P, S.ids["mb"], S.mV)
    assert rc == INVALID and "motion" in msg
    # nothing above changed the scene
    assert_arrays(P.bvh_export(), ex0)
    assert_arrays(P.blas_export(0), blas0)
    assert_infos(infos(P), inf0)
    for m in range(4):
        for a, b in zip(P.mesh_arrays(m), meshes0[m]):
            assert np.array_equal(a, b)
    # an imported hierarchy may share nodes between parents
    import_bvh(P, ex0)
    rc, msg = deform_rc(P, S.ids["blas"], bV)
    assert rc == INVALID and "import" in msg
    assert L.mrt_scene_deform_mesh_async(P._h, S.ids["blas"], fake, None, None, None) == INVALID and b"import" in L.mrt_last_error()
    # an unbuilt scene
    h = L.mrt_scene_create()
    try:
        assert L.mrt_scene_deform_mesh(h, 0, v.ctypes.data, None, None, None) == NOT_BUILT and b"not built" in L.mrt_last_error()
        assert L.mrt_scene_deform_mesh_async(h, 0, fake, None, None, None) == NOT_BUILT
    finally:
        L.mrt_scene_destroy(h)
    # the wrapper checks the counts
    with pytest.raises(miro.MRTError, match="verts2"):
        Case(blas_mesh()).P.deformMesh(2, S.mV, verts2=S.mV2[:-1])


def test_a_textured_blas_mesh_is_refused_by_the_async_form_alone():
    """7. texture coordinates: the synchronous form recomputes the tangents on the host."""
    bV, bN, bF = blas_mesh()
    P = miro.Scene()
    tm = tri_mesh(bV, bN, bF)
    uv = np.asarray(np.stack([np.arctan2(bV[:, 2], bV[:, 0]) / 6.2832 + 0.5, bV[:, 1] / 1.3], -1), F32)
    tm.setTexCoords(uv, bF)
    objs, bvh = miro.Objects(), miro.BVH()
    miro.ProxyObject.setupProxy(tm, miro.Lambert((0.3, 0.8, 0.4)), objs, bvh)
    P.addObject(miro.ProxyObject(objs, bvh, miro.Matrix4x4(PLACED[0])))
    P.addLight(point_light())
    P.preCalc()
    L = miro.lib()
    v = np.ascontiguousarray(bV, F32)
    assert L.mrt_scene_deform_mesh_async(P._h, 0, C.c_void_p(v.ctypes.data), None, None, None) == INVALID
    assert b"texture coordinates" in L.mrt_last_error()
    b0 = P.blas_export(0)
    bV1, bN1 = blas_displaced(bV, bF, 2)
    assert P.deformMesh(0, bV1, bN1) == 0.0
    assert_arrays(P.blas_export(0), blas_refit(b0, bV1, bF))


def test_interactions_on_the_host():
    """8. deform, then updateInstances: boxes from the refitted root; deform, then updateMesh on
    a world mesh: proxy and MBObject lanes keep their new boxes."""
    bm = blas_mesh()
    S = Case(bm)
    P = S.P
    blas0, ex0 = P.blas_export(0), P.bvh_export()
    bV1, bN1 = blas_displaced(bm[0], bm[2], 3)
    mb1 = mb_sets(bm[0], k=1.25, shift=(0.4, -0.3, 0.2))
    P.deformMesh(S.ids["blas"], bV1, bN1)
    P.deformMesh(S.ids["mb"], mb1[0], verts2=mb1[1])
    P.updateInstances(NEW)
    bw, fx, ww = expected(S, blas0, ex0, bV1, mats=NEW, mb=mb1)
    assert_state(P, S.n0, bw, fx, ww)
    V, N, F = standin()
    V1, N1 = displaced(V, F, 1)
    P.updateMesh(S.ids["world"], V1, N1)
    bw, fx, ww = expected(S, blas0, ex0, bV1, mats=NEW, mb=mb1, world=V1)
    assert_state(P, S.n0, bw, fx, ww)
    P.updateInstances(OTHER[1:], ids=[1])
    bw, fx, ww = expected(S, blas0, ex0, bV1, mats=[NEW[0], OTHER[1]], mb=mb1, world=V1)
    assert_state(P, S.n0, bw, fx, ww)


# ---------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("size,world", [("small", True), ("big", True), ("big", False)])
def test_arrays_after_a_device_deform(size, world):
    """9. blas_export, instance infos and bvh_export after a synchronous deform of an uploaded
    scene: both BLAS sizes, a world tree of >= 64 nodes (renumbered for the LDS walk) and one
    below; then the enclosure (12)."""
    bm = BLAS_MESHES[size]()
    S = Case(bm, world=world)
    P = S.P
    assert (P.bvh_info["nodes"] >= 64) == world
    blas0, ex0, inf0 = P.blas_export(0), P.bvh_export(), infos(P)
    frame(P, 64, 64)   # uploaded
    bV1, bN1 = blas_displaced(bm[0], bm[2], 3)
    assert P.deformMesh(S.ids["blas"], bV1, bN1) > 0.0
    bw, fx, ww = expected(S, blas0, ex0, bV1)
    assert_state(P, S.n0, bw, fx, ww)
    assert_infos(infos(P), inf0, keys=("m", "inv", "inv_t"))
    assert_encloses(P.blas_export(0), bV1[bm[2][::-1]])
    assert_encloses(P.bvh_export(), S.pv, fx)
    v, n, _, _ = P.mesh_arrays(S.ids["blas"])
    assert np.array_equal(v, bV1) and np.array_equal(n, bN1)
    assert P.deformMesh(S.ids["blas"], bm[0], bm[1]) > 0.0   # and back
    assert_arrays(P.blas_export(0), blas0)
    assert_arrays(P.bvh_export(), ex0)
    assert_infos(infos(P), inf0)


def case_kw(kw):
    kw = scene_kw(kw)
    return {k: kw[k] for k in ("light", "num_paths", "blas_material") if k in kw}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(FRAME_CASES))
def test_frames_after_a_device_deform(case):
    """10. the device-deformed scene against a twin deformed on the host before its first
    upload: the same topology, so every frame product is equal bit for bit."""
    knobs, kw = FRAME_CASES[case]
    bm = big_blas_mesh()
    bV1, bN1 = blas_displaced(bm[0], bm[2], 3)
    with tuned(**knobs):
        A = Case(bm, **case_kw(kw))
        f0 = frame(A.P)
        A.P.deformMesh(A.ids["blas"], bV1, bN1)
        fa = frame(A.P)
        B = Case(bm, **case_kw(kw))
        B.P.deformMesh(B.ids["blas"], bV1, bN1)
        fb = frame(B.P)
        if case == "rect_paths4":
            assert fa["shadow_rays"] > 96 * 96
        if case.startswith("chain"):
            assert fa["secondary_rays"] == fb["secondary_rays"] and fa["secondary_rays"] > 0
    assert_frames(fa, fb)
    assert not np.array_equal(bits(fa["rgb"]), bits(f0["rgb"]))
    assert (fa["hits"]["prim"] >= A.P.bvh_info["prims"]).sum() > 50   # instances are in view
    assert_arrays(A.P.blas_export(0), B.P.blas_export(0))
    assert_arrays(A.P.bvh_export(), B.P.bvh_export())


def oracle_twin(bm, mats):
    """Case(bm, mats, **TWIN) in the oracle: the same arrays in the same order."""
    import oracle as O
    Os = O.OracleScene()
    blas = Os.make_blas([Os.add_mesh(bm[0], bm[1], bm[2], bm[2], Os.add_material("lambert", kd=(0.3, 0.8, 0.4)))])
    for M in mats:
        Os.add_instance(blas, M)
    fl = floor_mesh()
    Os.add_mesh(fl.verts, fl.normals, fl.vidx, fl.nidx, Os.add_material("lambert", kd=(0.6, 0.6, 0.6)))
    Os.add_point_light((5, 12, 8), 800)
    Os.set_bg((0.1, 0.1, 0.3))
    Os.build()
    return Os


def counted_frame(P, W=96, H=96):
    img = miro.Image()
    img.resize(W, H)
    hits = P.raytraceImage(camera(CAM), img, want_hits=True, count_visits=True)
    st = P.last_stats
    return dict(rgb=img.rgb.copy(), rgb8=img.pixels.copy(), hits=hits.copy(), shadow_rays=st["shadow_rays"],
                visits=(st["primary_node_visits"], st["primary_leaf_visits"], st["node_visits"], st["leaf_visits"]))


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["small", "big"])
def test_a_power_of_two_against_a_fresh_scene_and_the_oracle(size):
    """10. deform to 2 V0: a fresh scene and the oracle at 2 V0, visit counts included."""
    bm = BLAS_MESHES[size]()
    bm2 = (scaled(bm[0], 2.0), bm[1], bm[2])
    A = Case(bm, **TWIN)
    counted_frame(A.P)   # uploaded
    A.P.deformMesh(A.ids["blas"], bm2[0])
    fa = counted_frame(A.P)
    T = Case(bm2, **TWIN)
    ft = counted_frame(T.P)
    assert_frames(fa, ft)
    assert fa["visits"] == ft["visits"]
    assert_arrays(A.P.blas_export(0), T.P.blas_export(0))
    assert_arrays(A.P.bvh_export(), T.P.bvh_export())
    assert_infos(infos(A.P), infos(T.P))
    ref = oracle_twin(bm2, PLACED).render(CAM, 96, 96, threads=8)
    assert np.array_equal(bits(fa["rgb"]), bits(ref["rgb"])) and np.array_equal(fa["rgb8"], ref["rgb8"])
    assert np.array_equal(fa["hits"]["prim"], ref["hits"]["prim"])
    assert fa["visits"][0] == ref["primary_node_visits"] and fa["visits"][1] == ref["primary_leaf_visits"]
    assert (fa["hits"]["prim"] >= A.P.bvh_info["prims"]).sum() > 50


@pytest.mark.gpu
def test_a_general_displacement_against_a_fresh_scene():
    """11. where both find the same prim and t bits, every other hit field and the pixel are
    equal; the agreeing share is at least 0.99, established first on a pair that runs no new
    kernel (the host-deformed twin and the fresh scene)."""
    bm = big_blas_mesh()
    bV1, bN1 = blas_displaced(bm[0], bm[2], 3)
    B = Case(bm, moving=False)
    B.P.deformMesh(B.ids["blas"], bV1, bN1)   # on the host, before its first upload
    fresh = Case((bV1, bN1, bm[2]), moving=False)
    fb, ff = frame(B.P), frame(fresh.P)
    share = agreeing(fb["hits"], ff["hits"]).mean()
    print("agreeing share, host-deformed twin against a fresh scene:", share)
    assert share >= 0.99
    A = Case(bm, moving=False)
    frame(A.P)
    A.P.deformMesh(A.ids["blas"], bV1, bN1)
    fa = frame(A.P)
    same = agreeing(fa["hits"], ff["hits"])
    print("agreeing share, device-deformed scene against a fresh scene:", same.mean())
    assert same.mean() >= 0.99
    assert np.array_equal(fa["hits"].view(np.uint32).reshape(96, 96, -1)[same], ff["hits"].view(np.uint32).reshape(96, 96, -1)[same])
    assert np.array_equal(bits(fa["rgb"])[same], bits(ff["rgb"])[same])
    assert np.array_equal(fa["rgb8"][same], ff["rgb8"][same])
    assert (fa["hits"]["prim"][same] >= A.P.bvh_info["prims"]).sum() > 50


@pytest.mark.gpu
def test_every_entry_after_a_deform():
    """13. the timed trace, the any-hit trace, sampleRays, shadeHits and hitSurfaces after a
    deform equal the twin's; instance hits shade with the new normals."""
    bm = big_blas_mesh()
    bV1, bN1 = blas_displaced(bm[0], bm[2], 3)
    o, d, t = camera(CAM).rays(64, 64)
    rng = np.random.default_rng(23)   # and 1024 rays from the eye at the two instances
    aim = np.array([[-4.5, 0.85, 1.5], [4.5, 0.65, 2.0]])[rng.integers(0, 2, 1024)] + rng.uniform(-0.5, 0.5, (1024, 3))
    rd = aim - np.array(CAM["eye"])
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    o = np.concatenate([o.reshape(-1, 3), np.tile(np.array(CAM["eye"]), (1024, 1))]).astype(F32)
    d = np.concatenate([d.reshape(-1, 3), rd]).astype(F32)
    t = np.concatenate([t.reshape(-1), rng.uniform(0, 1, 1024)]).astype(F32)
    A, B, Cn = Case(bm), Case(bm), Case(bm)
    before = A.P.traceRays(o, d, t)   # uploaded
    A.P.deformMesh(A.ids["blas"], bV1, bN1)
    B.P.deformMesh(B.ids["blas"], bV1, bN1)
    Cn.P.deformMesh(Cn.ids["blas"], bV1)     # the old normals
    ha, hb = A.P.traceRays(o, d, t), B.P.traceRays(o, d, t)
    assert same_words(ha, hb) and not same_words(ha, before)
    inst = ha["prim"] >= A.P.bvh_info["prims"]
    assert inst.sum() > 50
    assert same_words(A.P.traceBatch(o, d, any_hit=True), B.P.traceBatch(o, d, any_hit=True))
    (ra, sa), (rb, sb) = (P.sampleRays(o, d, t, seed=5, want_hits=True) for P in (A.P, B.P))
    assert same_words(sa, sb) and np.array_equal(bits(ra), bits(rb))
    rc, _ = Cn.P.sampleRays(o, d, t, seed=5, want_hits=True)
    assert not np.array_equal(bits(ra)[inst], bits(rc)[inst])
    assert np.array_equal(bits(A.P.shadeHits(o, d, sa, t, seed=5)), bits(B.P.shadeHits(o, d, sb, t, seed=5)))
    fa, fb = A.P.hitSurfaces(o, d, ha), B.P.hitSurfaces(o, d, hb)
    assert fa.tobytes() == fb.tobytes()
    assert not np.array_equal(bits(fa["n"])[inst], bits(Cn.P.hitSurfaces(o, d, ha)["n"])[inst])


def tensor(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, F32)).cuda().contiguous()


@pytest.mark.gpu
def test_async_deform_from_device_tensors():
    """14. torch tensors on a non-default stream, a frame on that stream, then the read-backs;
    the motion-blurred mesh with both tensors."""
    import torch
    bm = big_blas_mesh()
    bV1, bN1 = blas_displaced(bm[0], bm[2], 3)
    mb1 = mb_sets(blas_mesh()[0], k=1.25, shift=(0.4, -0.3, 0.2))
    W = H = 96
    A, B = Case(bm), Case(bm)
    blas0, ex0, inf0 = A.P.blas_export(0), A.P.bvh_export(), infos(A.P)
    frame(A.P, W, H)   # uploaded
    st = torch.cuda.Stream()
    tv, tn, m0, m1 = tensor(bV1), tensor(bN1), tensor(mb1[0]), tensor(mb1[1])
    torch.cuda.synchronize()
    assert A.P.deformMesh(A.ids["blas"], tv, tn, stream=st) is None
    rgb, rgb8 = async_frame(A.P, st, W, H)
    B.P.deformMesh(B.ids["blas"], bV1, bN1)
    frame(B.P, W, H)             # B uploaded at the deformed state, then deformed in place again
    B.P.deformMesh(B.ids["blas"], bV1, bN1)
    fb = frame(B.P, W, H)
    assert np.array_equal(bits(rgb), bits(fb["rgb"])) and np.array_equal(rgb8, fb["rgb8"])
    bw, fx, ww = expected(A, blas0, ex0, bV1)
    assert_state(A.P, A.n0, bw, fx, ww)   # blas_export, instance_info and bvh_export read the device back
    assert_infos(infos(A.P), inf0, keys=("m", "inv", "inv_t"))
    v, n, _, _ = A.P.mesh_arrays(A.ids["blas"])
    assert np.array_equal(v, bV1) and np.array_equal(n, bN1)
    # the motion-blurred mesh, both tensors; then updateInstances reads the refitted root
    assert A.P.deformMesh(A.ids["mb"], m0, verts2=m1, stream=st) is None
    rgb, rgb8 = async_frame(A.P, st, W, H)
    B.P.deformMesh(B.ids["mb"], mb1[0], verts2=mb1[1])
    fb = frame(B.P, W, H)
    assert np.array_equal(bits(rgb), bits(fb["rgb"])) and np.array_equal(rgb8, fb["rgb8"])
    bw, fx, ww = expected(A, blas0, ex0, bV1, mb=mb1)
    assert_state(A.P, A.n0, bw, fx, ww)
    assert np.array_equal(A.P.mesh_arrays(A.ids["mb"])[0], mb1[0])
    # an async deform, then a synchronous updateInstances: its boxes come from the device's root
    assert A.P.deformMesh(A.ids["blas"], tensor(bm[0]), tensor(bm[1]), stream=st) is None
    assert A.P.updateInstances(NEW) > 0.0
    bw, fx, ww = expected(A, blas0, ex0, bm[0], mats=NEW, mb=mb1)
    assert_state(A.P, A.n0, bw, fx, ww)
    # the host copy of the time-1 set came back: a host refit of a scene due for a re-upload
    # computes the MBObject boxes from it
    assert A.P.deformMesh(A.ids["mb"], m0, verts2=m1, stream=st) is None
    _lib.check(miro.lib().mrt_scene_set_material_gloss(A.P.handle, 0, 1.0), "gloss")   # marks the replicas stale
    assert A.P.deformMesh(A.ids["blas"], bV1, bN1) == 0.0
    bw, fx, ww = expected(A, blas0, ex0, bV1, mats=NEW, mb=mb1)
    assert_state(A.P, A.n0, bw, fx, ww)
    with pytest.raises(miro.MRTError, match="inert"):
        A.P.deformMesh(A.ids["blas"], tv, verts2=tv, stream=st)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [True, False])
def test_motion_blurred_mesh_on_the_device(world):
    """15. arrays against the restatement; frames against a fresh scene at the new vertex sets
    given the restated arrays (the import takes motion and proxy lanes: exact under one seed)."""
    bm = blas_mesh()
    mb1 = mb_sets(bm[0], k=1.25, shift=(0.4, -0.3, 0.2))
    A = Case(bm, world=world)
    ex0, blas0 = A.P.bvh_export(), A.P.blas_export(0)
    cam = dict(CAM, shutterSpeed=1.0)   # ray times over [0, 1]: both vertex sets are read
    f0 = frame(A.P, cam=cam)
    assert A.P.deformMesh(A.ids["mb"], mb1[0], verts2=mb1[1]) > 0.0
    want = refit(ex0, A.pv_with(mb1[0]), A.fixed(blas0[0][0], mb=mb1))
    assert_arrays(A.P.bvh_export(), want)
    assert_encloses(A.P.bvh_export(), A.pv_with(mb1[0]), A.fixed(blas0[0][0], mb=mb1))
    B = Case(bm, world=world, mb=mb1)
    import_bvh(B.P, want)
    fa, fb = frame(A.P, cam=cam), frame(B.P, cam=cam)
    assert_frames(fa, fb)
    assert not np.array_equal(bits(fa["rgb"]), bits(f0["rgb"]))
    mbp = (fa["hits"]["prim"] >= A.mb0) & (fa["hits"]["prim"] < A.mb0 + len(A.mF))
    assert mbp.sum() > 20   # the motion-blurred mesh is in view


@pytest.mark.gpu
def test_round_trips_on_the_device():
    """16. deform the BLAS, updateInstances (sync and async), deform again, updateMesh on a
    world mesh; the motion-blurred mesh, then updateMesh: its lanes keep the new boxes."""
    bm = big_blas_mesh()
    V, N, F = standin()
    V1, N1 = displaced(V, F, 1)
    bV1, bN1 = blas_displaced(bm[0], bm[2], 3)
    bV2, bN2 = blas_displaced(bm[0], bm[2], 4)
    mb1 = mb_sets(blas_mesh()[0], k=1.25, shift=(0.4, -0.3, 0.2))
    S = Case(bm)
    P = S.P
    blas0, ex0 = P.blas_export(0), P.bvh_export()
    f0 = frame(P)
    P.deformMesh(S.ids["blas"], bV1, bN1)
    assert_state(P, S.n0, *expected(S, blas0, ex0, bV1))
    P.updateInstances(NEW)
    assert_state(P, S.n0, *expected(S, blas0, ex0, bV1, mats=NEW))
    P.updateInstances(dev(OTHER))
    assert_state(P, S.n0, *expected(S, blas0, ex0, bV1, mats=OTHER))
    P.deformMesh(S.ids["blas"], bV2, bN2)
    assert_state(P, S.n0, *expected(S, blas0, ex0, bV2, mats=OTHER))
    P.updateMesh(S.ids["world"], V1, N1)
    assert_state(P, S.n0, *expected(S, blas0, ex0, bV2, mats=OTHER, world=V1))
    P.deformMesh(S.ids["mb"], mb1[0], verts2=mb1[1])
    P.updateMesh(S.ids["world"], V, N)
    assert_state(P, S.n0, *expected(S, blas0, ex0, bV2, mats=OTHER, mb=mb1))
    f1 = frame(P)
    assert not np.array_equal(bits(f1["rgb"]), bits(f0["rgb"]))
    # everything back: the first frame
    P.deformMesh(S.ids["mb"], S.mV, verts2=S.mV2)
    P.deformMesh(S.ids["blas"], bm[0], bm[1])
    P.updateInstances(PLACED)
    assert_arrays(P.blas_export(0), blas0)
    assert_arrays(P.bvh_export(), ex0)
    assert_frames(frame(P), f0)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["sync", "async"])
def test_a_deform_takes_the_instances_out_of_the_binning_box(entry):
    """17. the BLAS moves up by twice the height of the root box the replica was uploaded with;
    no result depends on the binning box: the chain-engine frame, unbinned and binned, equals
    the host-deformed twin's."""
    bm = blas_mesh()
    W = H = 64
    frames = {}
    for b in (0, 7):
        with tuned(bin=b, bin_inst=1 if b else 0):
            A = Case(bm, blas_material=mirror_blinn())
            ex0 = A.P.bvh_export()
            used = ex0[1][0] != EMPTY
            lo, hi = ex0[0][0].reshape(6, 4)[:3, used].min(1), ex0[0][0].reshape(6, 4)[3:, used].max(1)
            dy = F32(2) * F32(hi[1] - lo[1])
            up = np.asarray(bm[0] + np.array([0, dy, 0], F32), F32)
            # the instances end up near y = dy + 0.85 and 1.2 (dy + 0.65): both in this view
            cam = dict(CAM, eye=(0.0, float(dy) + 2.3, 11.0), lookAt=(0, float(dy) + 2.3, 1.75), fov=60)
            frame(A.P, W, H, cam)   # uploaded
            if entry == "sync":
                A.P.deformMesh(A.ids["blas"], up)
            else:
                A.P.deformMesh(A.ids["blas"], tensor(up))
            fa = frame(A.P, W, H, cam)
            B = Case(bm, blas_material=mirror_blinn())
            B.P.deformMesh(B.ids["blas"], up)
            for i in (0, 1):
                assert B.P.instance_info(i)["box"][0, 1] > hi[1]
            fb = frame(B.P, W, H, cam)
            assert_frames(fa, fb)
            assert fa["secondary_rays"] == fb["secondary_rays"] and fa["secondary_rays"] > 0
            assert (fa["hits"]["prim"] >= A.P.bvh_info["prims"]).sum() > 50   # instances are in view
            assert_arrays(A.P.bvh_export(), B.P.bvh_export())
            assert_arrays(A.P.blas_export(0), B.P.blas_export(0))
            frames[b] = fa
    assert_frames(frames[0], frames[7])
