"""mrt_scene_update_instances: new matrices for ProxyObject instances of a built scene, the
world hierarchy refitted in place.

The contract for the world tree is test_refit.py's numpy restatement, refit_of(export0,
prim_verts, fixed) with fixed[proxy slot] = instance_box(BLAS root, M_new); for the instance
itself (m, inv, inv_t, box) it is a fresh scene built with the new matrices, bit for bit; for
frames it is B, such a fresh scene given the restated arrays through mrt_scene_bvh_import.
The matrices: NEW[0] a rotation about three axes with a non-uniform scale and a translation (so
every entry of the 3x3 is used and inv_t differs from inv), NEW[1] a shear with a translation
and the last row (0, 0, 0, 2) (so multiplyAndDivideByW's rcp_nr is not of 1)."""
import ctypes as C
import functools

import numpy as np
import pytest

import miro
from miro import _lib
from helpers import bits, camera, tuned
from test_refit import (CAM, F32, INVALID, NOT_BUILT, PLACED, agreeing, assert_arrays, assert_frames, blas_mesh, box3,
                        displaced, floor_mesh, frame, import_bvh, instance_box, mixed_scene, point_light, prim_verts_of,
                        rect_light, refit_of, smax, smin, standin, tri_mesh)
from test_sample_rays import ALWAYS_MIRROR


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def affine(A, t, w=1.0):
    M = np.zeros((4, 4))
    M[:3, :3], M[:3, 3], M[3, 3] = np.asarray(A) * w, np.asarray(t) * w, w
    return M.astype(F32)


NEW = [affine(rot((0, 1, 0), 0.7) @ rot((1, 0, 0), 0.3) @ rot((0, 0, 1), 0.2) @ np.diag([1.3, 0.7, 1.1]), (-3.2, 0.9, 0.5)),
       affine([[1, 0.4, 0], [0, 1, 0.25], [0.3, 0, 1]], (3.4, 0.6, 2.5), w=2.0)]
OTHER = [affine(rot((1, 1, 0), -0.5) @ np.diag([0.8, 1.2, 0.9]), (-2.0, 1.5, 3.0)),
         affine(rot((0, 0, 1), 0.4) @ np.array([[1, 0, 0.3], [0.2, 1, 0], [0, 0, 1.0]]), (2.2, 1.1, 3.5))]


def mixed_at(mats, V, N, F, moving=True, light=point_light, num_paths=1, blas_material=None, path_trace=None):
    """test_refit.mixed_scene with the instances at `mats` (and a light, path count and BLAS
    material of choice): (scene, prim_verts, fixed_boxes)."""
    P = miro.Scene()
    miro.makeMeshObjs(P, tri_mesh(V, N, F), miro.Lambert((0.8, 0.7, 0.6)))
    bV, bN, bF = blas_mesh()
    objs, bvh = miro.Objects(), miro.BVH()
    miro.ProxyObject.setupProxy(tri_mesh(bV, bN, bF), blas_material or miro.Lambert((0.3, 0.8, 0.4)), objs, bvh)
    for M in mats:
        P.addObject(miro.ProxyObject(objs, bvh, miro.Matrix4x4(M)))
    entries = [(V, F), len(mats)]
    if moving:
        mV = np.asarray(bV * F32(0.7) + np.array([0.0, 6.4, 2.0], F32), F32)
        mV2 = np.asarray(mV + np.array([0.35, 0.1, 0.0], F32), F32)
        miro.makeMBMeshObjs(P, tri_mesh(mV, bN, bF), tri_mesh(mV2, bN, bF), miro.Lambert((0.9, 0.4, 0.3)))
        entries.append((mV, bF))
    fl = floor_mesh()
    miro.makeMeshObjs(P, fl, miro.Lambert((0.6, 0.6, 0.6)))
    entries.append((fl.verts, fl.vidx))
    P.addLight(light())
    P.setBGColor((0.1, 0.1, 0.3))
    P.setNumPaths(num_paths)
    if path_trace is not None:
        P.setPathTrace(True)
        P.setMaxBounces(path_trace)
    P.preCalc()
    root = P.blas_export(0)[0][0]
    n0 = len(F)
    fixed = {n0 + i: instance_box(root, M) for i, M in enumerate(mats)}
    if moving:
        for t, f in enumerate(bF):
            lo, hi = box3(*mV[f])
            lo2, hi2 = box3(*mV2[f])
            fixed[n0 + len(mats) + t] = (smin(lo, lo2), smax(hi, hi2))
    return P, prim_verts_of(*entries), fixed


def with_boxes(P, fixed, n0, mats, ids=None):
    """fixed with the proxy slots of `ids` (default 0 ..) at instance_box(BLAS root, M)."""
    root = P.blas_export(0)[0][0]
    out = dict(fixed)
    for k, M in enumerate(mats):
        out[n0 + (k if ids is None else ids[k])] = instance_box(root, M)
    return out


def infos(P):
    return [P.instance_info(i) for i in range(P.instance_count())]


def assert_infos(got, want, keys=("m", "inv", "inv_t", "box")):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["blas"] == w["blas"]
        for k in keys:
            assert not np.isnan(g[k]).any(), (i, k)
            assert np.array_equal(bits(g[k]), bits(w[k])), f"instance {i}: {k} differs"


def assert_boxes(P, fixed, n0):
    for i, inf in enumerate(infos(P)):
        lo, hi = fixed[n0 + i]
        assert np.array_equal(bits(inf["box"][0]), bits(lo)) and np.array_equal(bits(inf["box"][1]), bits(hi)), i


def update_rc(P, mats, ids=None, n=None):
    m = np.ascontiguousarray(mats, F32)
    idv = np.ascontiguousarray(ids, np.int32) if ids is not None else None
    L = miro.lib()
    rc = L.mrt_scene_update_instances(P._h, idv.ctypes.data if idv is not None else None, len(m) if n is None else n,
                                      m.ctypes.data, None)
    return rc, L.mrt_last_error().decode()


@functools.lru_cache(maxsize=None)
def fresh_infos(key):
    """instance_info of a fresh mixed scene built at NEW / OTHER / PLACED."""
    V, N, F = standin()
    P, _, _ = mixed_at({"new": NEW, "other": OTHER, "placed": PLACED}[key], V, N, F)
    return infos(P)


# ---------------------------------------------------------------- CPU tests (host path)
def test_matrices_exercise_every_term():
    for M in NEW + OTHER:
        assert np.isfinite(M).all() and abs(np.linalg.det(M.astype(np.float64))) > 0.1
    assert np.count_nonzero(NEW[0][:3]) == 12   # every entry of the 3x4 in use
    inf = fresh_infos("new")
    assert not np.array_equal(inf[0]["inv"], inf[0]["inv_t"])
    assert tuple(NEW[1][3]) == (0, 0, 0, 2) and inf[1]["inv"][3, 3] == F32(0.5)
    assert NEW[1][0, 1] != 0 and NEW[1][1, 0] == 0   # a shear


def test_mixed_at_placed_is_mixed_scene():
    V, N, F = standin()
    P, pv, fixed = mixed_scene(V, N, F)
    Q, pv2, fixed2 = mixed_at(PLACED, V, N, F)
    assert_arrays(Q.bvh_export(), P.bvh_export())
    assert np.array_equal(pv, pv2) and fixed.keys() == fixed2.keys()
    assert_infos(infos(Q), infos(P))
    assert P.instance_count() == 2 and infos(P)[1]["blas"] == 0
    assert np.array_equal(infos(P)[1]["m"], PLACED[1])


def test_identity_update_changes_nothing():
    """1. the matrices the scene already has."""
    V, N, F = standin()
    P, _, _ = mixed_scene(V, N, F)
    ex0, inf0, blas0 = P.bvh_export(), infos(P), P.blas_export(0)
    assert P.updateInstances(PLACED) == 0.0
    assert_arrays(P.bvh_export(), ex0)
    assert_infos(infos(P), inf0)
    assert P.updateInstances([miro.Matrix4x4(M) for M in PLACED], ids=[0, 1]) == 0.0   # Matrix4x4 objects, ids
    assert_arrays(P.bvh_export(), ex0)
    assert_infos(infos(P), inf0)
    assert_arrays(P.blas_export(0), blas0)


def test_host_update_of_a_scene_never_uploaded():
    """2. both instances of a never-uploaded mixed_scene."""
    V, N, F = standin()
    P, pv, fixed = mixed_scene(V, N, F)
    n0 = len(F)
    ex0, blas0 = P.bvh_export(), P.blas_export(0)
    assert P.updateInstances(NEW) == 0.0
    fixed1 = with_boxes(P, fixed, n0, NEW)
    want = refit_of(ex0, pv, fixed1)
    assert_arrays(P.bvh_export(), want)
    assert not np.array_equal(want[0], ex0[0])
    assert_boxes(P, fixed1, n0)
    assert_infos(infos(P), fresh_infos("new"))
    assert P.updateInstances(PLACED) == 0.0   # back again: boxes shrink as well as grow
    assert_arrays(P.bvh_export(), ex0)
    assert_infos(infos(P), fresh_infos("placed"))
    assert_arrays(P.blas_export(0), blas0)


def test_host_update_of_a_subset():
    """3. instance 1 alone, by id and by `first`."""
    V, N, F = standin()
    for how in (dict(ids=[1]), dict(first=1)):
        P, pv, fixed = mixed_scene(V, N, F)
        n0 = len(F)
        ex0, inf0 = P.bvh_export(), infos(P)
        P.updateInstances(NEW[1:], **how)
        got = infos(P)
        assert_infos(got[:1], inf0[:1])
        assert_infos(got[1:], fresh_infos("new")[1:])
        assert_arrays(P.bvh_export(), refit_of(ex0, pv, with_boxes(P, fixed, n0, NEW[1:], ids=[1])))
    # ids in another order than the instances
    P, pv, fixed = mixed_scene(V, N, F)
    ex0 = P.bvh_export()
    P.updateInstances([NEW[1], NEW[0]], ids=[1, 0])
    assert_infos(infos(P), fresh_infos("new"))
    assert_arrays(P.bvh_export(), refit_of(ex0, pv, with_boxes(P, fixed, len(F), NEW)))


def test_refusals():
    """4. every code and message, all before any change."""
    V, N, F = standin()
    P, _, _ = mixed_scene(V, N, F)
    L = miro.lib()
    ex0, inf0, blas0 = P.bvh_export(), infos(P), P.blas_export(0)
    m = np.ascontiguousarray(NEW, F32)
    assert L.mrt_scene_update_instances(None, None, 2, m.ctypes.data, None) == INVALID
    assert L.mrt_scene_update_instances(P._h, None, 2, None, None) == INVALID
    assert b"null matrices" in L.mrt_last_error()
    for bad in (-1, 2, 1000):
        rc, msg = update_rc(P, NEW, ids=[0, bad])
        assert rc == INVALID and f"instance id {bad} " in msg and "out of range" in msg
    rc, msg = update_rc(P, NEW + NEW[:1])   # ids == NULL: 0 .. n - 1
    assert rc == INVALID and "instance id 2 " in msg and "out of range" in msg
    rc, msg = update_rc(P, NEW, ids=[1, 1])
    assert rc == INVALID and "instance id 1 " in msg and "repeated" in msg
    rc, msg = update_rc(P, NEW, n=-1)
    assert rc == INVALID
    for v in (np.nan, np.inf):
        bad = np.array(NEW)
        bad[1, 2, 1] = v
        rc, msg = update_rc(P, bad)
        assert rc == INVALID and "matrix 1 " in msg and "finite" in msg
    sing = np.array(NEW)
    sing[1, 2] = sing[1, 0]   # two equal rows: det == 0, 1 / det = inf
    rc, msg = update_rc(P, sing)
    assert rc == INVALID and "matrix 1 " in msg and "singular" in msg
    rc, msg = update_rc(P, [np.zeros((4, 4), F32)], ids=[1])
    assert rc == INVALID and "matrix 0 " in msg and "instance 1" in msg and "singular" in msg
    rc, msg = update_rc(P, NEW, n=0)
    assert rc == 0, msg
    # the async form: its range, and a scene that is not on a device (the pointer is never read)
    fake = C.c_void_p(m.ctypes.data)
    assert L.mrt_scene_update_instances_async(None, 0, 2, fake, None) == INVALID
    assert L.mrt_scene_update_instances_async(P._h, 0, 2, None, None) == INVALID
    for first, n in ((1, 2), (-1, 1), (2, 1)):
        assert L.mrt_scene_update_instances_async(P._h, first, n, fake, None) == INVALID
        assert b"out of range" in L.mrt_last_error()
    assert L.mrt_scene_update_instances_async(P._h, 0, 2, fake, None) == INVALID
    assert b"exactly one device" in L.mrt_last_error()
    # nothing above changed the scene (the good first matrix of a refused batch included)
    assert_arrays(P.bvh_export(), ex0)
    assert_infos(infos(P), inf0)
    assert_arrays(P.blas_export(0), blas0)
    assert L.mrt_scene_instance_info(P._h, 2, None, None, None, None, None) == INVALID
    assert L.mrt_scene_instance_info(None, 0, None, None, None, None, None) == INVALID
    assert L.mrt_scene_instance_count(None) == INVALID
    # an imported hierarchy may share nodes between parents
    import_bvh(P, ex0)
    rc, msg = update_rc(P, NEW)
    assert rc == INVALID and "import" in msg
    assert L.mrt_scene_update_instances_async(P._h, 0, 2, fake, None) == INVALID and b"import" in L.mrt_last_error()
    # an unbuilt scene
    h = L.mrt_scene_create()
    try:
        assert L.mrt_scene_update_instances(h, None, 1, m.ctypes.data, None) == NOT_BUILT
        assert b"not built" in L.mrt_last_error()
        assert L.mrt_scene_update_instances_async(h, 0, 1, fake, None) == NOT_BUILT
        assert L.mrt_scene_instance_count(h) == 0
    finally:
        L.mrt_scene_destroy(h)


# ---------------------------------------------------------------- GPU tests
def scene_b(mats, ex0, pv, fixed, n0, V, N, F, **kw):
    """Built fresh with the instances at `mats`, then given the restated refit of A's export."""
    B, _, _ = mixed_at(mats, V, N, F, **kw)
    want = refit_of(ex0, pv, with_boxes(B, fixed, n0, mats))
    import_bvh(B, want)
    return B, want


@pytest.mark.gpu
def test_arrays_after_a_device_update():
    """5. the export and the infos after an update of an uploaded scene."""
    V, N, F = standin()
    A, pv, fixed = mixed_scene(V, N, F)
    n0 = len(F)
    ex0, blas0 = A.bvh_export(), A.blas_export(0)
    frame(A, 64, 64)   # uploaded
    ms = A.updateInstances(NEW)
    assert ms > 0.0
    fixed1 = with_boxes(A, fixed, n0, NEW)
    assert_arrays(A.bvh_export(), refit_of(ex0, pv, fixed1))
    assert_boxes(A, fixed1, n0)
    assert_infos(infos(A), fresh_infos("new"))
    assert_arrays(A.blas_export(0), blas0)
    # a subset by id on the device: instance 0 keeps NEW[0]
    assert A.updateInstances(OTHER[1:], ids=[1]) > 0.0
    assert_infos(infos(A), [fresh_infos("new")[0], fresh_infos("other")[1]])
    assert_arrays(A.bvh_export(), refit_of(ex0, pv, with_boxes(A, fixed1, n0, OTHER[1:], ids=[1])))


def mirror_blinn():
    m = ALWAYS_MIRROR
    return miro.Blinn(m["kd"], specExp=m["specExp"], specAmt=m["specAmt"], reflectAmt=m["reflectAmt"], ior=m["ior"])


FRAME_CASES = {
    "default": ({}, {}),
    "unfused": (dict(fused=0, wavefront=0), {}),
    "rect_paths4": ({}, dict(light=rect_light, num_paths=4)),
    "chain_bin0": (dict(bin=0), dict(blas_material=mirror_blinn)),
    "chain_bin7_inst": (dict(bin=7, bin_inst=1), dict(blas_material=mirror_blinn)),
}


def scene_kw(kw):
    return dict(kw, blas_material=kw["blas_material"]()) if "blas_material" in kw else kw


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(FRAME_CASES))
def test_frames_after_a_device_update(case):
    """6. float frame, 8-bit frame, hit records and shadow-ray count of A after the update equal
    those of B."""
    V, N, F = standin()
    knobs, kw = FRAME_CASES[case]
    n0 = len(F)
    with tuned(**knobs):
        A, pv, fixed = mixed_at(PLACED, V, N, F, **scene_kw(kw))
        ex0 = A.bvh_export()
        f0 = frame(A)
        A.updateInstances(NEW)
        fa = frame(A)
        B, want = scene_b(NEW, ex0, pv, fixed, n0, V, N, F, **scene_kw(kw))
        fb = frame(B)
        if case == "rect_paths4":
            assert fa["shadow_rays"] > 96 * 96
        if case.startswith("chain"):
            assert fa["secondary_rays"] == fb["secondary_rays"] and fa["secondary_rays"] > 0
    assert_frames(fa, fb)
    assert not np.array_equal(bits(fa["rgb"]), bits(f0["rgb"]))
    assert_arrays(A.bvh_export(), want)


def oracle_twin(mats, V, N, F):
    """mixed_at(mats, moving=False) in the oracle: the same arrays in the same order."""
    import oracle as O
    Os = O.OracleScene()
    Os.add_mesh(V, N, F, F, Os.add_material("lambert", kd=(0.8, 0.7, 0.6)))
    bV, bN, bF = blas_mesh()
    blas = Os.make_blas([Os.add_mesh(bV, bN, bF, bF, Os.add_material("lambert", kd=(0.3, 0.8, 0.4)))])
    for M in mats:
        Os.add_instance(blas, M)
    fl = floor_mesh()
    Os.add_mesh(fl.verts, fl.normals, fl.vidx, fl.nidx, Os.add_material("lambert", kd=(0.6, 0.6, 0.6)))
    Os.add_point_light((5, 12, 8), 800)
    Os.set_bg((0.1, 0.1, 0.3))
    Os.build()
    return Os


@pytest.mark.gpu
def test_against_the_oracle():
    """7. the oracle renders a fresh scene at the new matrices; where A's hit agrees with the
    oracle's (prim and the bits of t; trees of different topology differ on exact ties only),
    A's float and 8-bit RGB are the oracle's."""
    V, N, F = standin()
    W = H = 96
    n0 = len(F)
    # the condition first, on existing code paths: B's hits against a fresh build's
    A, pv, fixed = mixed_at(PLACED, V, N, F, moving=False)
    ex0 = A.bvh_export()
    B, _ = scene_b(NEW, ex0, pv, fixed, n0, V, N, F, moving=False)
    fresh, _, _ = mixed_at(NEW, V, N, F, moving=False)
    o, d, _ = camera(CAM).rays(W, H)
    hb = B.traceBatch(o.reshape(-1, 3), d.reshape(-1, 3))
    hf = fresh.traceBatch(o.reshape(-1, 3), d.reshape(-1, 3))
    assert agreeing(hb, hf).mean() >= 0.99
    frame(A, W, H)
    A.updateInstances(NEW)
    fa = frame(A, W, H)
    ref = oracle_twin(NEW, V, N, F).render(CAM, W, H, threads=8)
    same = agreeing(fa["hits"], ref["hits"])
    assert same.mean() >= 0.99
    assert (fa["hits"]["prim"][same] >= A.bvh_info["prims"]).sum() > 50   # instances are in view
    assert np.array_equal(bits(fa["rgb"])[same], bits(ref["rgb"])[same])
    assert np.array_equal(fa["rgb8"][same], ref["rgb8"][same])


def async_frame(A, st, W, H, cam=CAM):
    import torch
    rgb = torch.empty(H * W * 3, dtype=torch.float32, device="cuda")
    rgb8 = torch.empty(H * W * 3, dtype=torch.uint8, device="cuda")
    opts = _lib.mrt_render_opts(W, H, 0, 0, 1, 0, 0)
    cc = camera(cam)._c()
    _lib.check(miro.lib().mrt_render_frame_async(A.handle, C.byref(cc), C.byref(opts), rgb.data_ptr(), rgb8.data_ptr(),
                                                 st.cuda_stream), "render_frame_async")
    st.synchronize()
    return rgb.cpu().numpy().reshape(H, W, 3), rgb8.cpu().numpy().reshape(H, W, 3)


def dev(mats):
    import torch
    return torch.from_numpy(np.ascontiguousarray(mats, F32)).cuda().contiguous()


@pytest.mark.gpu
def test_async_update_from_device_tensors():
    """8. torch device tensors on a non-default stream, then mrt_render_frame_async on it."""
    import torch
    V, N, F = standin()
    V1, N1 = displaced(V, F, 1)
    W = H = 96
    n0 = len(F)
    L = miro.lib()
    A, pv, fixed = mixed_scene(V, N, F)
    ex0 = A.bvh_export()
    frame(A, W, H)   # uploaded
    st = torch.cuda.Stream()
    t_new, t_other = dev(NEW), dev(OTHER)
    torch.cuda.synchronize()
    assert A.updateInstances(t_new, stream=st) is None
    rgb, rgb8 = async_frame(A, st, W, H)
    B, want = scene_b(NEW, ex0, pv, fixed, n0, V, N, F)
    fb = frame(B, W, H)
    assert np.array_equal(bits(rgb), bits(fb["rgb"])) and np.array_equal(rgb8, fb["rgb8"])
    # instance_info and the export read the device state back (m: the replica's copy)
    assert_infos(infos(A), fresh_infos("new"))
    assert_arrays(A.bvh_export(), want)
    # a range: first = 1, n = 1 moves instance 1 only
    assert A.updateInstances(t_other[1:], first=1, stream=st) is None
    st.synchronize()
    mixed = [NEW[0], OTHER[1]]
    fixed2 = with_boxes(A, fixed, n0, mixed)
    assert_infos(infos(A), [fresh_infos("new")[0], fresh_infos("other")[1]])
    assert_arrays(A.bvh_export(), refit_of(ex0, pv, fixed2))
    with pytest.raises(miro.MRTError):
        A.updateInstances(t_new, ids=[0, 1])
    with pytest.raises(miro.MRTError, match="out of range"):
        A.updateInstances(t_new, first=1)
    # a later synchronous updateMesh of the world mesh uses the instance boxes the device holds
    assert A.updateInstances(t_other, stream=st) is None
    st.synchronize()
    pv1 = pv.copy()
    pv1[:n0] = V1[F]
    fixed3 = with_boxes(A, fixed, n0, OTHER)
    assert A.updateMesh(0, V1, N1) > 0.0
    assert_arrays(A.bvh_export(), refit_of(ex0, pv1, fixed3))
    # and so does a host refit of a scene due for a re-upload, after the device is read back
    assert A.updateInstances(t_new, stream=st) is None
    st.synchronize()
    _lib.check(L.mrt_scene_set_material_gloss(A.handle, 0, 1.0), "gloss")   # marks the replicas stale
    assert A.updateMesh(0, V, N) == 0.0
    assert_infos(infos(A), fresh_infos("new"))
    assert_arrays(A.bvh_export(), want)
    assert_frames(frame(A, W, H), fb)   # the re-upload carries the new instances
    torch.cuda.synchronize()


# 300 instances of a 4-triangle BLAS on a grid over a floor: more than one 256-thread
# workgroup of the instance kernel, the last one ragged and no multiple of a wave
GRID_N = 300
GRID_CAM = dict(eye=(0.0, 15.0, 17.0), lookAt=(0, 0, 0), up=(0, 1, 0), fov=45)


def tetra():
    V = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], F32) * F32(0.35)
    N = np.asarray(V / np.linalg.norm(V, axis=1, keepdims=True), F32)
    return V, N, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.uint32)


def grid_mats(seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(GRID_N):
        A = rot(rng.normal(size=3), rng.uniform(0, 6.28)) @ np.diag(rng.uniform(0.6, 1.4, 3))
        t = ((i % 20 - 9.5) * 1.2 + rng.uniform(-0.2, 0.2), rng.uniform(0.5, 1.2), (i // 20 - 7) * 1.2 + rng.uniform(-0.2, 0.2))
        out.append(affine(A, t))
    return out


def grid_scene(mats):
    """A floor (prim 0), then GRID_N instances (prims 1 ..): (scene, prim_verts, fixed_boxes)."""
    P = miro.Scene()
    fl = floor_mesh()
    miro.makeMeshObjs(P, fl, miro.Lambert((0.6, 0.6, 0.6)))
    objs, bvh = miro.Objects(), miro.BVH()
    miro.ProxyObject.setupProxy(tri_mesh(*tetra()), miro.Lambert((0.3, 0.8, 0.4)), objs, bvh)
    for M in mats:
        P.addObject(miro.ProxyObject(objs, bvh, miro.Matrix4x4(M)))
    P.addLight(point_light())
    P.setBGColor((0.1, 0.1, 0.3))
    P.preCalc()
    root = P.blas_export(0)[0][0]
    return P, prim_verts_of((fl.verts, fl.vidx), len(mats)), {1 + i: instance_box(root, M) for i, M in enumerate(mats)}


@pytest.mark.gpu
def test_more_than_one_workgroup_ragged():
    """9. all 300, then a scattered list of 37 ids."""
    M0, M1 = grid_mats(0), grid_mats(1)
    W = H = 64
    A, pv, fixed0 = grid_scene(M0)
    assert A.instance_count() == GRID_N and GRID_N > 256 and GRID_N % 64
    blas0 = A.blas_export(0)
    assert len(blas0[3]) == 1 and (blas0[3] >= 0).sum() == 4   # a 4-triangle BLAS: its root is a leaf
    ex0 = A.bvh_export()
    f0 = frame(A, W, H, GRID_CAM)
    assert A.updateInstances(M1) > 0.0
    B, _, fixed1 = grid_scene(M1)
    want = refit_of(ex0, pv, fixed1)
    assert_arrays(A.bvh_export(), want)
    assert_infos(infos(A), infos(B))
    assert_boxes(A, fixed1, 1)
    import_bvh(B, want)
    fa = frame(A, W, H, GRID_CAM)
    assert_frames(fa, frame(B, W, H, GRID_CAM))
    assert not np.array_equal(bits(fa["rgb"]), bits(f0["rgb"]))
    assert (fa["hits"]["prim"] >= 1 + GRID_N).mean() > 0.05   # instances are in view
    # 37 scattered ids back to their first matrices; the other 263 keep their bits
    ids = np.random.default_rng(2).permutation(GRID_N)[:37]
    assert len(set(ids.tolist())) == 37 and ids.max() >= 256
    before = infos(A)
    assert A.updateInstances([M0[i] for i in ids], ids=ids) > 0.0
    M2 = list(M1)
    for i in ids:
        M2[i] = M0[i]
    B2, _, fixed2 = grid_scene(M2)
    got = infos(A)
    keep = [i for i in range(GRID_N) if i not in set(ids.tolist())]
    assert len(keep) == 263
    assert_infos([got[i] for i in keep], [before[i] for i in keep])
    assert_infos(got, infos(B2))
    want2 = refit_of(ex0, pv, fixed2)
    assert_arrays(A.bvh_export(), want2)
    import_bvh(B2, want2)
    assert_frames(frame(A, W, H, GRID_CAM), frame(B2, W, H, GRID_CAM))
    assert_arrays(A.blas_export(0), blas0)


@pytest.mark.gpu
def test_round_trip_with_mesh_updates():
    """10. instances, the world mesh, the instances back, the mesh back: the first frame."""
    V, N, F = standin()
    V1, N1 = displaced(V, F, 1)
    n0 = len(F)
    A, pv, fixed = mixed_scene(V, N, F)
    ex0 = A.bvh_export()
    f0 = frame(A)
    A.updateInstances(NEW)
    A.updateMesh(0, V1, N1)
    pv1 = pv.copy()
    pv1[:n0] = V1[F]
    assert_arrays(A.bvh_export(), refit_of(ex0, pv1, with_boxes(A, fixed, n0, NEW)))
    f1 = frame(A)
    assert not np.array_equal(bits(f1["rgb"]), bits(f0["rgb"]))
    A.updateInstances(PLACED)
    A.updateMesh(0, V, N)
    assert_frames(frame(A), f0)
    assert_arrays(A.bvh_export(), ex0)
    assert_infos(infos(A), fresh_infos("placed"))


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["sync", "async"])
def test_instances_leave_the_binning_box(entry):
    """11. the instances move up by twice the height of the root box the replica was uploaded
    with: every ray that starts on them has its origin outside that box, its origin cell
    clamped.  The synchronous entry refreshes the binning box, the async one leaves it stale,
    and no result depends on it: the chain-engine frame, unbinned and binned, equals B's."""
    V, N, F = standin()
    n0 = len(F)
    W = H = 64
    frames = {}
    for b in (0, 7):
        with tuned(bin=b, bin_inst=1 if b else 0):
            A, pv, fixed = mixed_at(PLACED, V, N, F, blas_material=mirror_blinn())
            ex0 = A.bvh_export()
            used = ex0[1][0] != -2 ** 31
            lo, hi = ex0[0][0].reshape(6, 4)[:3, used].min(1), ex0[0][0].reshape(6, 4)[3:, used].max(1)
            dy = F32(2) * F32(hi[1] - lo[1])
            up = [affine(np.eye(3), (0, dy, 0)) @ M for M in NEW]
            cam = dict(CAM, eye=(0.5, 5.0 + float(dy), 11.0), lookAt=(0, float(dy) + 1.0, 0))
            frame(A, W, H, cam)   # uploaded
            if entry == "sync":
                A.updateInstances(up)
            else:
                A.updateInstances(dev(up))
            fa = frame(A, W, H, cam)
            B, want = scene_b(up, ex0, pv, fixed, n0, V, N, F, blas_material=mirror_blinn())
            for i in (0, 1):
                assert want[0][0].reshape(6, 4)[4, used].max() > hi[1] and B.instance_info(i)["box"][0, 1] > hi[1]
            fb = frame(B, W, H, cam)
            assert_frames(fa, fb)
            assert fa["secondary_rays"] == fb["secondary_rays"] and fa["secondary_rays"] > 0
            assert (fa["hits"]["prim"] >= A.bvh_info["prims"]).sum() > 50   # instances are in view
            assert_arrays(A.bvh_export(), want)
            frames[b] = fa
    assert_frames(frames[0], frames[7])
