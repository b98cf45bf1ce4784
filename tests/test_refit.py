"""mrt_scene_update_mesh: new vertices for a world mesh, the hierarchy refitted in place.

The contract is `refit_arrays` below, a numpy restatement on the canonical export that does
not call the library: leaf triangles A, B - A, C - A from the vertices; a packet's box the
merge of its lanes in lane order from the empty box (+-1e12); a slot that is an inner node
the merge of that child's non-empty slots in slot order; empty slots keep their zero box;
ProxyObject / MBObject lanes keep the box the build gave them.  Floats are compared by value
(np.array_equal: +0 == -0, no NaN anywhere), integers exactly."""
import ctypes as C
import functools

import numpy as np
import pytest

import miro
from miro import _lib, scenes
from helpers import bits, camera, config_scene, fixture_mesh, tuned

F32 = np.float32
EMPTY = -2 ** 31
INVALID, NOT_BUILT = -1, -5


# ---------------------------------------------------------------- the yardstick
def smin(a, b):   # std::min(a, b) = b < a ? b : a
    return np.where(b < a, b, a).astype(F32)


def smax(a, b):   # std::max(a, b) = a < b ? b : a
    return np.where(a < b, b, a).astype(F32)


def box3(A, B, C):
    return smin(A, smin(B, C)), smax(A, smax(B, C))


def refit_arrays(node_boxes, node_child, leaf_tris, leaf_prims, prim_verts, fixed_boxes=None):
    """(node_boxes, leaf_tris) of the hierarchy (node_child, leaf_prims) refitted to
    prim_verts[(prim, corner, xyz)]; fixed_boxes: {prim: (lo, hi)} of ProxyObject / MBObject
    lanes (their triangle data stays as exported)."""
    nb, lt = np.array(node_boxes, F32), np.array(leaf_tris, F32)
    fixed_boxes = fixed_boxes or {}
    lbox = []
    for li in range(len(lt)):
        lo, hi = np.full(3, 1e12, F32), np.full(3, -1e12, F32)
        for k in range(4):
            p = int(leaf_prims[li, k])
            if p < 0:
                continue
            if p in fixed_boxes:
                blo, bhi = fixed_boxes[p]
            else:
                A, B, Cc = (np.asarray(prim_verts[p, j], F32) for j in range(3))
                lt[li, 0 + k], lt[li, 4 + k], lt[li, 8 + k] = A
                lt[li, 12 + k], lt[li, 16 + k], lt[li, 20 + k] = B - A
                lt[li, 24 + k], lt[li, 28 + k], lt[li, 32 + k] = Cc - A
                blo, bhi = box3(A, B, Cc)
            lo, hi = smin(lo, np.asarray(blo, F32)), smax(hi, np.asarray(bhi, F32))
        lbox.append((lo, hi))

    def fill(i):   # bottom-up by recursion from the root
        for k in range(4):
            c = int(node_child[i, k])
            if c == EMPTY:
                continue
            if c < 0:
                lo, hi = lbox[~c]
            else:
                fill(c)
                lo, hi = np.full(3, 1e12, F32), np.full(3, -1e12, F32)
                for j in range(4):
                    if int(node_child[c, j]) != EMPTY:
                        lo, hi = smin(lo, nb[c, [j, 4 + j, 8 + j]]), smax(hi, nb[c, [12 + j, 16 + j, 20 + j]])
            nb[i, [k, 4 + k, 8 + k]] = lo
            nb[i, [12 + k, 16 + k, 20 + k]] = hi

    fill(0)
    return nb, lt


def assert_arrays(got, want):
    for g, w, name in zip(got, want, ("node_boxes", "node_child", "leaf_tris", "leaf_prims")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if g.dtype == np.float32:
            assert not np.isnan(g).any(), name
        assert np.array_equal(g, w), f"{name} differ in {int((g != w).sum())} values"


def refit_of(export, prim_verts, fixed_boxes=None, arrays=None):
    """arrays: another form of refit_arrays (test_refit_shapes.py has one vectorised per height)."""
    nb, nc, lt, lp = export
    rb, rt = (arrays or refit_arrays)(nb, nc, lt, lp, prim_verts, fixed_boxes)
    return rb, nc, rt, lp


def prim_verts_of(*entries):
    """World prims in scene order: (verts, vidx) per world mesh, an int n for n slots without
    a triangle of their own (ProxyObjects)."""
    out = []
    for e in entries:
        if isinstance(e, int):
            out.append(np.zeros((e, 3, 3), F32))
        else:
            out.append(np.asarray(e[0], F32)[np.asarray(e[1]).reshape(-1, 3)])
    return np.concatenate(out)


# ---------------------------------------------------------------- scenes
def tri_mesh(V, N, F):
    tm = miro.TriangleMesh()
    tm.setArrays(V, N, F, F)
    return tm


def floor_mesh(verts=None):
    fl = miro.TriangleMesh()
    fl.createSingleTriangle()
    fl.setV1((-100, 0, -100)); fl.setV2((0, 0, 100)); fl.setV3((100, 0, -100))
    if verts is not None:
        fl.verts[:] = verts
    fl.setN1((0, 1, 0)); fl.setN2((0, 1, 0)); fl.setN3((0, 1, 0))
    return fl


def point_light():
    pl = miro.PointLight()
    pl.setPosition((5, 12, 8))
    pl.setPower(800)
    return pl


def rect_light():
    rl = miro.RectangleLight()
    rl.setVertices((-2, 11, 4), (2, 11, 4), (-2, 11, 8))
    rl.setPower(700)
    rl.setSamples(2)
    return rl


CAM = dict(eye=(0.5, 5.0, 11.0), lookAt=(0, 3, 0), up=(0, 1, 0), fov=45)


@functools.lru_cache(maxsize=None)
def _standin_nodes(nu):
    V, F, N = scenes.bunny_standin(nu, nu // 2)
    P = miro.Scene()
    miro.makeMeshObjs(P, tri_mesh(V, N, F), miro.Lambert())
    return P.preCalc()["nodes"]


@functools.lru_cache(maxsize=None)
def standin():
    """scenes.bunny_standin at the smallest (nu, nv = nu // 2), nu even, whose tree has >= 64
    nodes (the LDS top-node walk renumbers such a tree): verts0, normals0, faces."""
    nu = 6
    while _standin_nodes(nu) < 64:
        nu += 2
    assert _standin_nodes(nu) >= 64 and _standin_nodes(nu - 2) < 64
    V, F, N = scenes.bunny_standin(nu, nu // 2)
    return np.asarray(V, F32), np.asarray(N, F32), np.asarray(F, np.uint32)


def displaced(V, F, seed, amp=0.3):
    """V + a smooth seeded displacement of amplitude ~10% of the stand-in's radius (3), with
    recomputed smooth normals."""
    rng = np.random.default_rng(seed)
    c = np.array([0.0, 3.05, 0.0])
    d = V - c
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-6)
    s = sum(np.sin(V @ rng.uniform(0.3, 1.2, 3) + rng.uniform(0, 6.28)) for _ in range(3)) / 3.0
    V1 = np.asarray(V + amp * s[:, None] * d, F32)
    return V1, np.asarray(scenes._smooth_normals(V1.astype(np.float64), F.astype(np.int64)), F32)


def scene_a(V, N, F, light=point_light, num_paths=1, material=None, uv=None, floor=None, path_trace=None):
    """The stand-in (mesh 0), a floor (mesh 1; floor: its three vertices) and a light.
    path_trace: max bounces, turns Scene::m_pathTrace on."""
    P = miro.Scene()
    mat = material or miro.Lambert((0.8, 0.7, 0.6))
    tm = tri_mesh(V, N, F)
    if uv is not None:
        tm.setTexCoords(uv, F)
    miro.makeMeshObjs(P, tm, mat)
    miro.makeMeshObjs(P, floor_mesh(floor), miro.Lambert((0.6, 0.6, 0.6)))
    P.addLight(light())
    P.setBGColor((0.1, 0.1, 0.3))
    P.setNumPaths(num_paths)
    if path_trace is not None:
        P.setPathTrace(True)
        P.setMaxBounces(path_trace)
    P.preCalc()
    return P


def a_prim_verts(V, F, floor=None):
    fl = floor_mesh(floor)
    return prim_verts_of((V, F), (fl.verts, fl.vidx))


def import_bvh(P, arrays):
    nb, nc, lt, lp = (np.ascontiguousarray(a) for a in arrays)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    _lib.check(miro.lib().mrt_scene_bvh_import(P.handle, len(nb), len(lt), nb.ctypes.data_as(fp), nc.ctypes.data_as(ip),
                                               lt.ctypes.data_as(fp), lp.ctypes.data_as(ip)), "bvh_import")
    info = _lib.mrt_bvh_info()   # a later P.bvh_export() sizes its arrays by these counts
    _lib.check(miro.lib().mrt_scene_bvh_info(P.handle, C.byref(info)), "bvh_info")
    P.bvh_info = {k: getattr(info, k) for k, _ in info._fields_}


def update_rc(P, mesh, verts, normals=None):
    v = np.ascontiguousarray(verts, F32)
    n = np.ascontiguousarray(normals, F32) if normals is not None else None
    L = miro.lib()
    rc = L.mrt_scene_update_mesh(P._h, mesh, v.ctypes.data, n.ctypes.data if n is not None else None, None)
    return rc, L.mrt_last_error().decode()


def frame(P, W=96, H=96, cam=CAM):
    img = miro.Image()
    img.resize(W, H)
    hits = P.raytraceImage(camera(cam), img, want_hits=True)
    return dict(rgb=img.rgb.copy(), rgb8=img.pixels.copy(), hits=hits.copy(), shadow_rays=P.last_stats["shadow_rays"],
                secondary_rays=P.last_stats["secondary_rays"])


def assert_frames(a, b):
    assert np.array_equal(bits(a["rgb"]), bits(b["rgb"])), "float frame differs"
    assert np.array_equal(a["rgb8"], b["rgb8"]), "8-bit frame differs"
    assert np.array_equal(a["hits"].view(np.uint32), b["hits"].view(np.uint32)), "hit records differ"
    assert a["shadow_rays"] == b["shadow_rays"], "shadow ray counts differ"


# instances: a small sphere BLAS placed twice
def blas_mesh():
    V, F, N = scenes.bunny_standin(8, 5, radius=0.6)
    return np.asarray(V, F32), np.asarray(N, F32), np.asarray(F, np.uint32)


PLACED = [np.array([[1, 0, 0, -4.5], [0, 1, 0, 0.2], [0, 0, 1, 1.5], [0, 0, 0, 1]], F32),
          np.array([[0.8, 0, 0.6, 4.5], [0, 1.2, 0, 0.0], [-0.6, 0, 0.8, 2.0], [0, 0, 0, 1]], F32)]


def instance_box(root_boxes, M):
    """ProxyObject::getAABB restated: the BLAS root's four slot boxes (unused ones included as
    zero boxes) merged, its corners through multiplyAndDivideByW, grown in order."""
    lo, hi = np.full(3, 1e12, F32), np.full(3, -1e12, F32)
    for k in range(4):
        lo, hi = smin(lo, root_boxes[[k, 4 + k, 8 + k]]), smax(hi, root_boxes[[12 + k, 16 + k, 20 + k]])
    P = [(lo[0], lo[1], hi[2]), (lo[0], hi[1], lo[2]), (hi[0], lo[1], lo[2]), (lo[0], hi[1], hi[2]),
         (hi[0], hi[1], lo[2]), (hi[0], lo[1], hi[2]), (lo[0], lo[1], lo[2]), (hi[0], hi[1], hi[2])]

    def dp4(row, u):
        p = [F32(row[i]) * F32(u[i]) for i in range(4)]
        return F32(F32(p[0] + p[1]) + F32(p[2] + p[3]))
    nlo, nhi = np.full(3, 1e12, F32), np.full(3, -1e12, F32)
    for p in P:
        u = (p[0], p[1], p[2], F32(1))
        w = F32(miro.rcp_nr(float(dp4(M[3], u))))
        q = np.array([w * dp4(M[r], u) for r in range(3)], F32)
        nlo, nhi = smin(nlo, q), smax(nhi, q)
    return nlo, nhi


def mixed_scene(V, N, F, moving=True, later=None):
    """The stand-in (mesh 0), two instances of a small sphere (mesh 1), a small motion-blurred
    sphere (mesh 2; moving only), a static mesh after it (later: its (V, N, F)) and a floor.
    Returns (scene, prim_verts, fixed_boxes)."""
    P = miro.Scene()
    miro.makeMeshObjs(P, tri_mesh(V, N, F), miro.Lambert((0.8, 0.7, 0.6)))
    bV, bN, bF = blas_mesh()
    objs, bvh = miro.Objects(), miro.BVH()
    miro.ProxyObject.setupProxy(tri_mesh(bV, bN, bF), miro.Lambert((0.3, 0.8, 0.4)), objs, bvh)
    for M in PLACED:
        P.addObject(miro.ProxyObject(objs, bvh, miro.Matrix4x4(M)))
    entries = [(V, F), len(PLACED)]
    if moving:
        mV = np.asarray(bV * F32(0.7) + np.array([0.0, 6.4, 2.0], F32), F32)
        mV2 = np.asarray(mV + np.array([0.35, 0.1, 0.0], F32), F32)
        miro.makeMBMeshObjs(P, tri_mesh(mV, bN, bF), tri_mesh(mV2, bN, bF), miro.Lambert((0.9, 0.4, 0.3)))
        entries.append((mV, bF))
    if later is not None:
        miro.makeMeshObjs(P, tri_mesh(*later), miro.Lambert((0.4, 0.5, 0.9)))
        entries.append((later[0], later[2]))
    fl = floor_mesh()
    miro.makeMeshObjs(P, fl, miro.Lambert((0.6, 0.6, 0.6)))
    entries.append((fl.verts, fl.vidx))
    P.addLight(point_light())
    P.setBGColor((0.1, 0.1, 0.3))
    P.preCalc()
    root = P.blas_export(0)[0][0]
    n0 = len(F)
    fixed = {n0 + i: instance_box(root, M) for i, M in enumerate(PLACED)}
    if moving:
        for t, f in enumerate(bF):
            lo, hi = box3(*mV[f])
            lo2, hi2 = box3(*mV2[f])
            fixed[n0 + len(PLACED) + t] = (smin(lo, lo2), smax(hi, hi2))
    return P, prim_verts_of(*entries), fixed


# ---------------------------------------------------------------- CPU tests (host export only)
def _identity_scenes():
    one = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32), np.array([[0, 0, 1]] * 3, F32), np.array([[0, 1, 2]], np.uint32))
    rng = np.random.default_rng(5)
    fiveV = rng.uniform(-2, 2, (15, 3)).astype(F32)
    five = (fiveV, np.tile(np.array([[0, 0, 1]], F32), (15, 1)), np.arange(15, dtype=np.uint32).reshape(5, 3))
    cb = fixture_mesh("cornell_box")
    return {"one_triangle": lambda: one, "five_triangles": lambda: five,
            "cornell_box": lambda: (np.asarray(cb[0], F32), np.asarray(cb[1], F32), np.asarray(cb[2], np.uint32)),
            "standin": standin}


@pytest.mark.parametrize("name", ["one_triangle", "five_triangles", "cornell_box", "standin"])
def test_identity_refit_of_the_build_is_the_build(name):
    """1. union-of-children equals the build's boxes: refit_arrays(export, same vertices) == export."""
    V, N, F = _identity_scenes()[name]()
    P = miro.Scene()
    miro.makeMeshObjs(P, tri_mesh(V, N, F), miro.Lambert())
    info = P.preCalc()
    if name == "one_triangle":
        assert info["nodes"] == 1 and info["leaves"] == 1   # the root is a leaf
    if name == "standin":
        assert info["nodes"] >= 64
    if name == "cornell_box":
        assert info["prims"] == 36
    ex = P.bvh_export()
    assert_arrays(refit_of(ex, prim_verts_of((V, F))), ex)


def test_identity_refit_with_instances_and_motion_lanes():
    """1. (two instances and a world mesh; and with MBObject lanes): proxy / MB lanes take the
    box the build gave them, restated in numpy."""
    V, N, F = standin()
    for moving in (False, True):
        P, pv, fixed = mixed_scene(V, N, F, moving=moving)
        ex = P.bvh_export()
        assert_arrays(refit_of(ex, pv, fixed), ex)


def test_host_refit_of_a_scene_never_uploaded():
    """2. mrt_scene_update_mesh on a built, never-uploaded scene, then export."""
    V0, N0, F = standin()
    V1, N1 = displaced(V0, F, 1)
    P = scene_a(V0, N0, F)
    ex0 = P.bvh_export()
    assert P.updateMesh(0, V1, N1) == 0.0
    want = refit_of(ex0, a_prim_verts(V1, F))
    assert_arrays(P.bvh_export(), want)
    assert not np.array_equal(want[0], ex0[0]) and not np.array_equal(want[2], ex0[2])
    v, n, _, _ = P.mesh_arrays(0)
    assert np.array_equal(bits(v), bits(V1)) and np.array_equal(bits(n), bits(N1))
    # back again: boxes shrink as well as grow
    P.updateMesh(0, V0, N0)
    assert_arrays(P.bvh_export(), ex0)


def test_refusals():
    """3. codes and messages, all before any device call."""
    V, N, F = standin()
    P, _, _ = mixed_scene(V, N, F)
    bV = blas_mesh()[0]
    rc, msg = update_rc(P, 1, bV)
    assert rc == INVALID and "BLAS" in msg
    rc, msg = update_rc(P, 2, bV)
    assert rc == INVALID and "motion" in msg
    for bad in (-1, 4, 1000):
        rc, msg = update_rc(P, bad, V)
        assert rc == INVALID and "bad mesh id" in msg
    bad = V.copy()
    bad[7, 1] = np.nan
    rc, msg = update_rc(P, 0, bad)
    assert rc == INVALID and "vertex 7 " in msg and "finite" in msg
    badn = N.copy()
    badn[3, 0] = np.inf
    rc, msg = update_rc(P, 0, V, badn)
    assert rc == INVALID and "normal 3 " in msg
    assert miro.lib().mrt_scene_update_mesh(P._h, 0, None, None, None) == INVALID
    assert miro.lib().mrt_scene_update_mesh(None, 0, None, None, None) == INVALID
    ex = P.bvh_export()   # nothing above changed the scene
    rc, msg = update_rc(P, 0, V)
    assert rc == 0, msg
    assert_arrays(P.bvh_export(), ex)
    # an imported hierarchy may share nodes between parents
    Q = scene_a(V, N, F)
    import_bvh(Q, Q.bvh_export())
    rc, msg = update_rc(Q, 0, V)
    assert rc == INVALID and "import" in msg
    # an unbuilt scene
    L = miro.lib()
    h = L.mrt_scene_create()
    try:
        lam = miro.Lambert()._c()
        mid = L.mrt_scene_add_material(h, C.byref(lam))
        vi = np.ascontiguousarray(F)
        mm = _lib.mrt_mesh(V.ctypes.data_as(C.POINTER(C.c_float)), N.ctypes.data_as(C.POINTER(C.c_float)),
                           vi.ctypes.data_as(C.POINTER(C.c_uint32)), vi.ctypes.data_as(C.POINTER(C.c_uint32)),
                           len(V), len(N), len(F), 3, 3)
        assert L.mrt_scene_add_mesh(h, C.byref(mm), mid) == 0
        assert L.mrt_scene_update_mesh(h, 0, V.ctypes.data, None, None) == NOT_BUILT
        assert b"not built" in L.mrt_last_error()
    finally:
        L.mrt_scene_destroy(h)


# ---------------------------------------------------------------- GPU tests
@pytest.fixture(scope="module")
def shapes():
    V0, N0, F = standin()
    V1, N1 = displaced(V0, F, 1)
    V2, N2 = displaced(V0, F, 2, amp=0.2)
    return dict(F=F, V0=V0, N0=N0, V1=V1, N1=N1, V2=V2, N2=N2)


def scene_b(s, export0, **kw):
    """Built fresh from verts1 / normals1, then given the refit of A's original export."""
    B = scene_a(s["V1"], s["N1"], s["F"], **kw)
    import_bvh(B, refit_of(export0, a_prim_verts(s["V1"], s["F"])))
    return B


@pytest.mark.gpu
def test_arrays_after_a_device_refit(shapes):
    """4. the export after an update of an uploaded scene is what the device holds."""
    s = shapes
    A = scene_a(s["V0"], s["N0"], s["F"])
    ex0 = A.bvh_export()
    frame(A, 64, 64)   # uploaded
    ms = A.updateMesh(0, s["V1"], s["N1"])
    assert ms > 0.0
    assert_arrays(A.bvh_export(), refit_of(ex0, a_prim_verts(s["V1"], s["F"])))
    v, n, vi, _ = A.mesh_arrays(0)
    assert np.array_equal(bits(v), bits(s["V1"])) and np.array_equal(bits(n), bits(s["N1"]))
    assert np.array_equal(vi, s["F"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["default", "lds_nodes", "unfused", "rect_paths4"])
def test_frames_after_a_device_refit(shapes, case):
    """5. float frame, 8-bit frame, hit records and shadow-ray count of A after the refit equal
    those of B, a fresh build at the new vertices given the refitted arrays."""
    s = shapes
    knobs = {"lds_nodes": dict(lds_nodes=1), "unfused": dict(fused=0)}.get(case, {})
    kw = dict(light=rect_light, num_paths=4) if case == "rect_paths4" else {}
    with tuned(**knobs):
        A = scene_a(s["V0"], s["N0"], s["F"], **kw)
        ex0 = A.bvh_export()
        f0 = frame(A)
        A.updateMesh(0, s["V1"], s["N1"])
        fa = frame(A)
        if case == "lds_nodes":   # the permuted numbering reached LDS
            assert A.walk_info()["lds_nodes"] == 1
        B = scene_b(s, ex0, **kw)
        fb = frame(B)
        if case == "lds_nodes":
            assert B.walk_info()["lds_nodes"] == 1
        if case == "rect_paths4":
            assert fa["shadow_rays"] > 96 * 96
    assert_frames(fa, fb)
    assert not np.array_equal(bits(fa["rgb"]), bits(f0["rgb"]))


@pytest.mark.gpu
def test_identity_update_on_the_device_keeps_the_oracle_frame():
    """6. updateMesh(verts0, normals0) on an uploaded config scene (cornell)."""
    P, Osc, cam = config_scene("C1")
    W = H = 64
    V, N, _, _ = fixture_mesh("cornell_box")
    ex0 = P.bvh_export()
    f0 = frame(P, W, H, cam)
    P.updateMesh(0, V, N)
    f1 = frame(P, W, H, cam)
    ref = Osc.render(cam, W, H, threads=8)
    assert np.array_equal(bits(f1["rgb"]), bits(ref["rgb"])) and np.array_equal(f1["rgb8"], ref["rgb8"])
    assert np.array_equal(f1["hits"]["prim"], ref["hits"]["prim"])
    assert f1["shadow_rays"] == ref["shadow_rays"]
    assert_frames(f1, f0)
    assert_arrays(P.bvh_export(), ex0)


@pytest.mark.gpu
def test_repeated_updates_return_to_the_first_frame(shapes):
    """7. verts0 -> verts1 -> verts2 -> verts0: boxes that only ever grow would show."""
    s = shapes
    A = scene_a(s["V0"], s["N0"], s["F"])
    ex0 = A.bvh_export()
    f0 = frame(A)
    for k in ("1", "2", "0"):
        A.updateMesh(0, s["V" + k], s["N" + k])
    assert_frames(frame(A), f0)
    assert_arrays(A.bvh_export(), ex0)


def agreeing(ha, hb):
    return (ha["prim"] == hb["prim"]) & (bits(ha["t"]) == bits(hb["t"]))


@pytest.mark.gpu
def test_mixed_lanes_keep_their_build_boxes(shapes):
    """8. two instances + a world mesh + a motion-blurred mesh; the world mesh is updated."""
    s = shapes
    W = H = 96
    # the condition this test relies on, checked on existing code paths: the refitted tree and
    # a fresh build at verts1 find the same hits on at least 99% of the camera rays
    o, d, _ = camera(CAM).rays(W, H)
    A0 = scene_a(s["V0"], s["N0"], s["F"])
    fresh = scene_a(s["V1"], s["N1"], s["F"])
    hb = scene_b(s, A0.bvh_export()).traceBatch(o.reshape(-1, 3), d.reshape(-1, 3))
    hf = fresh.traceBatch(o.reshape(-1, 3), d.reshape(-1, 3))
    assert agreeing(hb, hf).mean() >= 0.99

    M, pv0, fixed = mixed_scene(s["V0"], s["N0"], s["F"])
    ex0 = M.bvh_export()
    blas0 = M.blas_export(0)
    frame(M, W, H)
    M.updateMesh(0, s["V1"], s["N1"])
    fm = frame(M, W, H)
    pv1 = pv0.copy()
    pv1[:len(s["F"])] = s["V1"][s["F"]]
    assert_arrays(M.bvh_export(), refit_of(ex0, pv1, fixed))
    assert_arrays(M.blas_export(0), blas0)
    Mf, _, _ = mixed_scene(s["V1"], s["N1"], s["F"])
    ff = frame(Mf, W, H)
    same = agreeing(fm["hits"], ff["hits"])
    assert same.mean() >= 0.99
    assert np.array_equal(bits(fm["rgb"])[same], bits(ff["rgb"])[same])
    assert np.array_equal(fm["rgb8"][same], ff["rgb8"][same])


@pytest.mark.gpu
def test_async_update_from_device_tensors(shapes):
    """9. torch device tensors on a non-default stream, then mrt_render_frame_async on it."""
    import torch
    s = shapes
    W = H = 96
    L = miro.lib()
    A = scene_a(s["V0"], s["N0"], s["F"])
    ex0 = A.bvh_export()
    frame(A, W, H)   # uploaded
    st = torch.cuda.Stream()
    v = torch.from_numpy(s["V1"]).cuda().contiguous()
    n = torch.from_numpy(s["N1"]).cuda().contiguous()
    rgb = torch.empty(H * W * 3, dtype=torch.float32, device="cuda")
    rgb8 = torch.empty(H * W * 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert A.updateMesh(0, v, n, stream=st) is None
    opts = _lib.mrt_render_opts(W, H, 0, 0, 1, 0, 0)
    cc = camera(CAM)._c()
    _lib.check(L.mrt_render_frame_async(A.handle, C.byref(cc), C.byref(opts), rgb.data_ptr(), rgb8.data_ptr(),
                                        st.cuda_stream), "render_frame_async")
    st.synchronize()
    fb = frame(scene_b(s, ex0), W, H)
    assert np.array_equal(bits(rgb.cpu().numpy().reshape(H, W, 3)), bits(fb["rgb"]))
    assert np.array_equal(rgb8.cpu().numpy().reshape(H, W, 3), fb["rgb8"])
    # the export reads the device state back
    assert_arrays(A.bvh_export(), refit_of(ex0, a_prim_verts(s["V1"], s["F"])))
    vv, nn, _, _ = A.mesh_arrays(0)
    assert np.array_equal(bits(vv), bits(s["V1"])) and np.array_equal(bits(nn), bits(s["N1"]))
    # a mesh with texture coordinates stays with the synchronous entry
    T = scene_a(s["V0"], s["N0"], s["F"], uv=sphere_uv(s["V0"]))
    frame(T, 64, 64)
    rc = L.mrt_scene_update_mesh_async(T.handle, 0, v.data_ptr(), n.data_ptr(), st.cuda_stream)
    assert rc == INVALID and b"texture coordinates" in L.mrt_last_error()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_reupload_after_an_async_update_reads_the_device_back(shapes):
    """9b. a scene change after an async update drops the replica: the re-upload must come from
    the device's state, read back into the host copy first."""
    import torch
    s = shapes
    L = miro.lib()
    A = scene_a(s["V0"], s["N0"], s["F"])
    ex0 = A.bvh_export()
    f0 = frame(A)
    A.updateMesh(0, torch.from_numpy(s["V1"]).cuda(), torch.from_numpy(s["N1"]).cuda())
    _lib.check(L.mrt_scene_set_material_gloss(A.handle, 0, 1.0), "gloss")   # marks the replicas stale
    fa = frame(A)
    assert_frames(fa, frame(scene_b(s, ex0)))
    assert_arrays(A.bvh_export(), refit_of(ex0, a_prim_verts(s["V1"], s["F"])))
    A.updateMesh(0, s["V0"], s["N0"])   # and the synchronous form on the new replica
    assert_frames(frame(A), f0)
    assert_arrays(A.bvh_export(), ex0)


def sphere_uv(V):
    d = V - np.array([0.0, 3.05, 0.0])
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-6)
    return np.stack([np.arctan2(d[:, 2], d[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(d[:, 1], -1, 1)) / np.pi],
                    -1).astype(F32)


def mapped_material():
    rng = np.random.default_rng(11)
    col = rng.uniform(0.2, 1.0, (16, 16, 3)).astype(F32)
    nrm = np.asarray(np.array([0.5, 0.5, 1.0]) + rng.uniform(-0.25, 0.25, (16, 16, 3)) * [1, 1, 0], F32)
    m = miro.Blinn((0.8, 0.8, 0.8), specExp=20.0, specAmt=0.3)
    m.setColorMap(miro.Texture(miro.RawImage(16, 16, col, miro.TEX_RGB)))
    m.setNormalMap(miro.Texture(miro.RawImage(16, 16, nrm, miro.TEX_RGB)))
    return m


@pytest.mark.gpu
def test_sync_update_of_a_textured_mesh(shapes):
    """10. a colour map and a normal map: the tangent frames are recomputed and re-uploaded."""
    s = shapes
    uv = sphere_uv(s["V0"])
    A = scene_a(s["V0"], s["N0"], s["F"], material=mapped_material(), uv=uv)
    ex0 = A.bvh_export()
    f0 = frame(A)
    A.updateMesh(0, s["V1"], s["N1"])
    fa = frame(A)
    fb = frame(scene_b(s, ex0, material=mapped_material(), uv=uv))
    assert_frames(fa, fb)
    assert not np.array_equal(bits(fa["rgb"]), bits(f0["rgb"]))
    # normals alone moving the tangent frames: vertices kept, normals of verts2
    A.updateMesh(0, s["V1"], s["N2"])
    B2 = scene_a(s["V1"], s["N2"], s["F"], material=mapped_material(), uv=uv)
    import_bvh(B2, refit_of(ex0, a_prim_verts(s["V1"], s["F"])))
    assert_frames(frame(A), frame(B2))
