"""mrt_scene_update_mesh at the shapes tests/test_refit.py does not reach: meshes after the
first (non-zero vertex and normal bases, the two different), heights of more than one
workgroup of nodes, updates without normals, the two entries mixed, every entry after a
refit, the chain engine and its binned levels on a stale binning box, an alpha-mapped mesh,
a static mesh behind a motion-blurred one, and edge values.

The yardstick is test_refit.py's: the numpy restatement on the canonical export, which never
calls the library (here also in a form vectorised per height, asserted equal to the recursive
one), and for frames and ray batches scene B, a fresh build at the new vertices given the
numpy-refitted arrays.  Everything is compared bit for bit; box and triangle arrays by value
with no NaN (assert_arrays).  assert_encloses checks what the contract is for."""
import functools

import numpy as np
import pytest

import miro
from miro import scenes
from helpers import bits, camera, fixture_mesh, tuned
from test_refit import (CAM, EMPTY, F32, PLACED, a_prim_verts, assert_arrays, assert_frames, blas_mesh, box3, displaced,
                        floor_mesh, frame, import_bvh, mixed_scene, point_light, prim_verts_of, refit_of, scene_a, smax,
                        smin, standin, tri_mesh)
from test_hit_surfaces import restated_surfaces
from test_sample_rays import ALWAYS_MIRROR
from test_textures import leaf_image, leaf_quads

NODES_PER_WG = 64   # refit_node_kernel: one lane per slot, kRefitWG = 256 lanes = 64 nodes
LANES_PER_WG = 256  # refit_leaf_kernel: one lane per packet lane, kRefitWG = 256


# ---------------------------------------------------------------- the yardstick, per height
def heights(node_child):
    """The height of every node as prepare() in mrt_refit.hip has it: 0 for a node whose slots
    are all leaves or empty, else 1 + the largest height among its inner children."""
    nc = np.asarray(node_child)
    h = np.zeros(len(nc), np.int64)
    for i in range(len(nc) - 1, -1, -1):   # every child has a larger number than its parent
        c = nc[i][nc[i] >= 0]
        assert (c > i).all() and (c < len(nc)).all()
        if len(c):
            h[i] = h[c].max() + 1
    return h


def _xyz(k):
    return [k, 4 + k, 8 + k], [12 + k, 16 + k, 20 + k]


def refit_arrays_by_height(node_boxes, node_child, leaf_tris, leaf_prims, prim_verts, fixed_boxes=None):
    """refit_arrays with every packet at once and every node of a height at once: the same
    merges in the same order (lane order, slot order, from the empty box)."""
    nb, lt = np.array(node_boxes, F32), np.array(leaf_tris, F32)
    nc, lp = np.asarray(node_child), np.asarray(leaf_prims)
    pv = np.asarray(prim_verts, F32)
    A, B, Cc = pv[:, 0], pv[:, 1], pv[:, 2]
    plo, phi = box3(A, B, Cc)
    e1, e2 = B - A, Cc - A
    fx = np.zeros(len(pv), bool)
    for p, (blo, bhi) in (fixed_boxes or {}).items():
        fx[p], plo[p], phi[p] = True, blo, bhi
    lo, hi = np.full((len(lt), 3), 1e12, F32), np.full((len(lt), 3), -1e12, F32)
    for k in range(4):
        used = lp[:, k] >= 0
        p = np.where(used, lp[:, k], 0)
        plain = used & ~fx[p]
        for a in range(3):
            lt[plain, 4 * a + k] = A[p[plain], a]
            lt[plain, 12 + 4 * a + k] = e1[p[plain], a]
            lt[plain, 24 + 4 * a + k] = e2[p[plain], a]
        lo = np.where(used[:, None], smin(lo, plo[p]), lo)
        hi = np.where(used[:, None], smax(hi, phi[p]), hi)
    h = heights(nc)
    for level in range(int(h.max()) + 1):
        idx = np.flatnonzero(h == level)
        for k in range(4):
            c = nc[idx, k]
            klo, khi = _xyz(k)
            leaf = (c < 0) & (c != EMPTY)
            nb[idx[leaf][:, None], klo] = lo[~c[leaf]]
            nb[idx[leaf][:, None], khi] = hi[~c[leaf]]
            ch = c[c >= 0]
            blo, bhi = np.full((len(ch), 3), 1e12, F32), np.full((len(ch), 3), -1e12, F32)
            for j in range(4):
                u = (nc[ch, j] != EMPTY)[:, None]
                jlo, jhi = _xyz(j)
                blo = np.where(u, smin(blo, nb[ch][:, jlo]), blo)
                bhi = np.where(u, smax(bhi, nb[ch][:, jhi]), bhi)
            nb[idx[c >= 0][:, None], klo] = blo
            nb[idx[c >= 0][:, None], khi] = bhi
    return nb, lt


def refit(export, prim_verts, fixed_boxes=None):
    return refit_of(export, prim_verts, fixed_boxes, arrays=refit_arrays_by_height)


def assert_encloses(export, prim_verts, fixed_boxes=None):
    """What the contract is for: every plain lane's three vertices (and every fixed lane's box)
    lie inside the slot box of its packet; every used slot box of a child lies inside the
    parent's slot box for that child; every used slot box has lo <= hi on each axis (what
    boxes_ordered and box_test_oct rest on)."""
    nb, nc, lt, lp = export
    pv = np.asarray(prim_verts, F32)
    seen = np.zeros(len(lp), bool)
    for k in range(4):
        klo, khi = _xyz(k)
        c = nc[:, k]
        used = c != EMPTY
        assert (nb[used][:, klo] <= nb[used][:, khi]).all(), "a used slot box has lo > hi"
        leaf = used & (c < 0)
        li = ~c[leaf]
        seen[li] = True
        slo, shi = nb[leaf][:, klo], nb[leaf][:, khi]
        for lane in range(4):
            p = lp[li, lane]
            m = p >= 0
            plo, phi = box3(*(pv[p[m], j] for j in range(3)))
            for q, (blo, bhi) in (fixed_boxes or {}).items():
                plo[p[m] == q], phi[p[m] == q] = blo, bhi
            assert (slo[m] <= plo).all() and (phi <= shi[m]).all(), "a lane lies outside its packet's box"
        inner = c >= 0
        ch = c[inner]
        for j in range(4):
            jlo, jhi = _xyz(j)
            u = nc[ch, j] != EMPTY
            assert (nb[inner][u][:, klo] <= nb[ch][u][:, jlo]).all() and (nb[ch][u][:, jhi] <= nb[inner][u][:, khi]).all(), \
                "a child's slot box lies outside its parent's"
    assert seen.all()   # every packet hangs in the tree


# ---------------------------------------------------------------- shapes
def flat_normals(V, F):
    """One normal per face and the normal index array that gives it to the face's corners."""
    V64 = np.asarray(V, np.float64)
    n = np.cross(V64[F[:, 1]] - V64[F[:, 0]], V64[F[:, 2]] - V64[F[:, 0]])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
    return np.asarray(n, F32), np.repeat(np.arange(len(F), dtype=np.uint32)[:, None], 3, 1)


BESIDE = np.array([6.5, 0.0, 0.0], F32)   # mesh 1's place
CAM3 = dict(eye=(3.25, 5.0, 17.0), lookAt=(3.25, 3.0, 0.0), up=(0, 1, 0), fov=45)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def three_mesh_scene(m0, m1, m2):
    """Three world meshes, each (verts, normals, vidx, nidx), and one point light."""
    P = miro.Scene()
    for (V, N, F, NF), kd in zip((m0, m1, m2), ((0.8, 0.7, 0.6), (0.5, 0.8, 0.6), (0.6, 0.6, 0.6))):
        tm = miro.TriangleMesh()
        tm.setArrays(V, N, F, NF)
        miro.makeMeshObjs(P, tm, miro.Lambert(kd))
    P.addLight(point_light())
    P.setBGColor((0.1, 0.1, 0.3))
    P.preCalc()
    return P


def three_meshes_with(nu):
    """Mesh 0: the small stand-in with flat per-face normals through its own normal index
    array (more normals than vertices, so nbase[1] != vbase[1]); mesh 1: bunny_standin(nu,
    nu // 2) beside it; mesh 2: the floor triangle."""
    V0, _, F0 = standin()
    N0, NF0 = flat_normals(V0, F0)
    V, F, N = scenes.bunny_standin(nu, nu // 2)
    V1, N1, F1 = np.asarray(V, F32) + BESIDE, np.asarray(N, F32), np.asarray(F, np.uint32)
    fl = floor_mesh()
    return [frozen(V0.copy(), N0, F0.copy(), NF0), frozen(V1, N1, F1, F1.copy()),
            frozen(fl.verts.copy(), fl.normals.copy(), fl.vidx.copy(), fl.nidx.copy())]


def pv_of(meshes):
    return prim_verts_of(*((m[0], m[2]) for m in meshes))


@functools.lru_cache(maxsize=None)
def shape_facts(nu):
    """(nodes per height, leaves) of the three-mesh scene's world tree with mesh 1 at nu."""
    _, nc, lt, _ = three_mesh_scene(*three_meshes_with(nu)).bvh_export()
    return tuple(np.bincount(heights(nc)).tolist()), len(lt)


def is_big(nu):
    counts, leaves = shape_facts(nu)
    wide = [c for c in counts if c > NODES_PER_WG]   # more than one workgroup of refit_node_kernel
    return len(wide) >= 2 and any(c % NODES_PER_WG for c in wide) and (4 * leaves) % LANES_PER_WG != 0


@functools.lru_cache(maxsize=None)
def big():
    """The smallest nu, even, at which the world tree of the three-mesh scene has at least two
    heights of more than 64 nodes, one of those counts no multiple of 64, and 4 x leaves no
    multiple of 256."""
    nu = 8
    while not is_big(nu):
        nu += 2
    return nu


@functools.lru_cache(maxsize=None)
def three_meshes():
    return three_meshes_with(big())


def updates():
    """Mesh 1, then the floor with a lifted corner, then mesh 0: (mesh, verts, normals)."""
    m0, m1, m2 = three_meshes()
    V1, N1 = displaced(m1[0] - BESIDE, m1[2], 3)
    V0, _ = displaced(m0[0], m0[2], 4)
    fl = m2[0].copy()
    fl[0, 1] = 1.5
    return [(1, np.asarray(V1 + BESIDE, F32), N1), (2, fl, m2[1].copy()), (0, V0, flat_normals(V0, m0[2])[0])]


def given(meshes, m, V, N=None):
    out = list(meshes)
    out[m] = (V, out[m][1] if N is None else N) + tuple(out[m][2:])
    return out


def assert_meshes(P, meshes):
    for m, (V, N, F, NF) in enumerate(meshes):
        v, n, vi, ni = P.mesh_arrays(m)
        assert np.array_equal(bits(v), bits(V)), f"mesh {m}: vertices"
        assert np.array_equal(bits(n), bits(N)), f"mesh {m}: normals"
        assert np.array_equal(vi, F) and np.array_equal(ni, NF), f"mesh {m}: indices"


def each_mesh_in_turn(A, after):
    """Test 4's sequence on scene A; after(meshes as last given, refit of the first export)
    runs behind every update.  Then back to the originals."""
    ex0 = A.bvh_export()
    cur = three_meshes()
    for m, V, N in updates():
        A.updateMesh(m, V, N)
        cur = given(cur, m, V, N)
        want = refit(ex0, pv_of(cur))
        got = A.bvh_export()
        assert_arrays(got, want)
        assert_meshes(A, cur)
        assert_encloses(got, pv_of(cur))
        after(cur, want)
    for m, (V, N, _, _) in enumerate(three_meshes()):
        A.updateMesh(m, V, N)
    assert_arrays(A.bvh_export(), ex0)
    assert_meshes(A, three_meshes())


# edge values: 12 unshared triangles
def edge_mesh():
    """(benign vertices the scene is built at, the edge vertices, normals, faces)."""
    rng = np.random.default_rng(17)
    T = 12
    V0 = rng.uniform(-2, 2, (3 * T, 3)).astype(F32)
    tiny, nz = F32(1e-39), F32(-0.0)
    a38, b38 = F32(1.0000001e-38), F32(1.0e-38)
    big1, big3 = F32(1e12), F32(3e12)
    tris = [
        [(0.0, nz, 1.0), (nz, 0.0, 2.0), (0.0, 1.0, nz)],                       # both zeros
        [(nz, nz, nz), (0.0, 0.0, 0.0), (nz, 0.0, nz)],                         # nothing but zeros
        [(tiny, -tiny, 0.5), (2 * tiny, tiny, 0.5), (tiny, 3 * tiny, 0.25)],    # subnormal coordinates
        [(a38, 1.0, a38), (b38, 2.0, -b38), (b38, a38, b38)],                   # B - A subnormal
        [(1.0, 1.0, 1.0), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0)],                    # three equal corners
        [(-1.0, 0.5, 2.0), (-1.0, 0.5, 2.0), (1.5, 0.5, -1.0)],                 # two equal corners
        [(big1, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)],                   # at the empty box
        [(0.0, -big1, 0.0), (1.0, -big1, 0.0), (0.0, -big1, 1.0)],              # on its other side
        [(big3, 1.0, 1.0), (big3, 2.0, 1.0), (big3, 1.0, 2.0)],                 # beyond it: lo stays 1e12
        [(1.0, 1.0, -big3), (2.0, 1.0, -big3), (1.0, 2.0, -big3)],              # hi stays -1e12
        [(big3, -big3, 0.0), (0.0, 1.0, 0.0), (-big3, big3, 1.0)],              # across it
    ]
    V1 = V0.copy()
    V1[:3 * len(tris)] = np.array(tris, F32).reshape(-1, 3)
    N = np.tile(np.array([[0, 0, 1]], F32), (3 * T, 1))
    return V0, V1, N, np.arange(3 * T, dtype=np.uint32).reshape(T, 3)


def assert_edge_premises(V1):
    """numpy keeps subnormals here (a flush-to-zero mode in this process would void the case)."""
    assert V1[6, 0] != 0 and abs(V1[6, 0]) < np.finfo(F32).tiny
    d = V1[10, 0] - V1[9, 0]
    assert d != 0 and abs(d) < np.finfo(F32).tiny and d.dtype == F32
    assert np.signbit(V1[0, 1]) and not np.signbit(V1[0, 0])
    assert V1[18, 0] == F32(1e12) and V1[24, 0] > F32(1e12)


def edge_scene(V, N, F):
    P = miro.Scene()
    miro.makeMeshObjs(P, floor_mesh(), miro.Lambert((0.6, 0.6, 0.6)))   # the edge mesh is mesh 1
    miro.makeMeshObjs(P, tri_mesh(V, N, F), miro.Lambert())
    P.addLight(point_light())
    P.preCalc()
    fl = floor_mesh()
    return P, lambda verts: prim_verts_of((fl.verts, fl.vidx), (verts, F))


# ---------------------------------------------------------------- CPU tests
def test_heights_of_small_trees():
    """1. heights() on trees written by hand."""
    E = EMPTY
    assert heights(np.array([[-1, E, E, E]], np.int32)).tolist() == [0]
    nc = np.array([[1, 2, -1, E], [-2, -3, E, E], [3, -4, E, E], [-5, -6, -7, -8]], np.int32)
    assert heights(nc).tolist() == [2, 0, 1, 0]


def test_the_big_mesh_is_the_smallest_with_several_workgroups_per_height():
    """2. the premise of the GPU tests, checked without a GPU."""
    nu = big()
    counts, leaves = shape_facts(nu)
    wide = [c for c in counts if c > NODES_PER_WG]
    assert len(wide) >= 2 and any(c % NODES_PER_WG for c in wide) and (4 * leaves) % LANES_PER_WG != 0
    assert nu % 2 == 0 and not any(is_big(n) for n in range(8, nu, 2))
    m0, m1, m2 = three_meshes()
    assert len(m0[1]) != len(m0[0])           # nbase[1] != vbase[1]
    assert 1000 < len(m1[2]) < 6000, len(m1[2])
    assert sum(counts) == three_mesh_scene(m0, m1, m2).bvh_info["nodes"]


def test_refit_by_height_equals_the_recursive_restatement():
    """2. the vectorised form on the small stand-in, with and without fixed lanes, moved."""
    V0, N0, F = standin()
    V1, _ = displaced(V0, F, 1)
    ex = scene_a(V0, N0, F).bvh_export()
    pv = a_prim_verts(V1, F)
    assert_arrays(refit(ex, pv), refit_of(ex, pv))
    P, pv0, fixed = mixed_scene(V0, N0, F)
    pv1 = pv0.copy()
    pv1[:len(F)] = V1[F]
    ex = P.bvh_export()
    assert_arrays(refit(ex, pv1, fixed), refit_of(ex, pv1, fixed))
    assert_arrays(refit(ex, pv0, fixed), ex)
    assert_encloses(ex, pv0, fixed)


def test_host_refit_of_each_mesh_in_turn():
    """4, 5. later meshes on the host: export, all three meshes' arrays, enclosure."""
    A = three_mesh_scene(*three_meshes())
    ex0 = A.bvh_export()
    assert_arrays(refit(ex0, pv_of(three_meshes())), ex0)
    assert_encloses(ex0, pv_of(three_meshes()))
    moved = []
    each_mesh_in_turn(A, lambda cur, want: moved.append(not np.array_equal(want[0], ex0[0])))
    assert moved == [True] * 3


def test_enclosure_check_sees_a_box_that_is_too_small():
    """5. assert_encloses is not vacuous: the old boxes do not enclose the moved vertices."""
    A = three_mesh_scene(*three_meshes())
    m, V, N = updates()[0]
    with pytest.raises(AssertionError):
        assert_encloses(A.bvh_export(), pv_of(given(three_meshes(), m, V, N)))


def test_edge_values_on_the_host():
    """6. both zeros, subnormals, subnormal differences, degenerate triangles, +-1e12 and beyond."""
    V0, V1, N, F = edge_mesh()
    assert_edge_premises(V1)
    P, pv = edge_scene(V0, N, F)
    ex0 = P.bvh_export()
    P.updateMesh(1, V1, N)
    got = P.bvh_export()
    want = refit_of(ex0, pv(V1))
    assert_arrays(got, want)
    assert_arrays(refit(ex0, pv(V1)), want)
    assert_encloses(got, pv(V1))
    assert np.array_equal(bits(P.mesh_arrays(1)[0]), bits(V1))
    # the bits too where the sign of a zero or a flushed subnormal would hide from ==
    assert np.array_equal(bits(got[2]), bits(want[2]))
    sub = (want[2] != 0) & (np.abs(want[2]) < np.finfo(F32).tiny)
    assert sub.sum() >= 8
    # a build at the edge vertices is its own refit
    Q, _ = edge_scene(V1, N, F)
    exq = Q.bvh_export()
    assert_arrays(refit_of(exq, pv(V1)), exq)
    P.updateMesh(1, V0, N)
    assert_arrays(P.bvh_export(), ex0)


# ---------------------------------------------------------------- GPU tests
def b_three(cur, want):
    B = three_mesh_scene(*cur)
    import_bvh(B, want)
    return B


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["default", "lds_nodes"])
def test_later_meshes_on_the_device(case):
    """7. test 4's sequence on an uploaded scene through the synchronous entry: non-zero vertex
    and normal bases (and the two different), node launches of several workgroups."""
    with tuned(**(dict(lds_nodes=1) if case == "lds_nodes" else {})):
        A = three_mesh_scene(*three_meshes())
        f0 = frame(A, cam=CAM3)   # uploaded
        seen = [f0]

        def after(cur, want):
            fa = frame(A, cam=CAM3)
            B = b_three(cur, want)
            assert_frames(fa, frame(B, cam=CAM3))
            assert not np.array_equal(bits(fa["rgb"]), bits(seen[-1]["rgb"]))
            seen.append(fa)
            if case == "lds_nodes":   # the permuted numbering reached LDS
                assert A.walk_info()["lds_nodes"] == 1 and B.walk_info()["lds_nodes"] == 1

        each_mesh_in_turn(A, after)
        assert len(seen) == 4
        assert_frames(frame(A, cam=CAM3), f0)


@pytest.mark.gpu
def test_async_updates_then_a_synchronous_one():
    """8. mesh 1 from device tensors on a side stream with normals, mesh 0 without normals,
    then mesh 2 through the synchronous entry while both are still ahead of the host."""
    import torch
    (_, V1, N1), (_, V2, N2), (_, V0, _) = updates()
    A = three_mesh_scene(*three_meshes())
    ex0 = A.bvh_export()
    frame(A, cam=CAM3)   # uploaded
    st = torch.cuda.Stream()
    tv1, tn1, tv0 = (torch.from_numpy(x).cuda().contiguous() for x in (V1, N1, V0))
    torch.cuda.synchronize()
    assert A.updateMesh(1, tv1, tn1, stream=st) is None
    assert A.updateMesh(0, tv0, None, stream=st) is None
    assert A.updateMesh(2, V2, N2) > 0.0
    cur = given(given(given(three_meshes(), 1, V1, N1), 0, V0), 2, V2, N2)
    want = refit(ex0, pv_of(cur))
    fa = frame(A, cam=CAM3)
    assert_frames(fa, frame(b_three(cur, want), cam=CAM3))
    got = A.bvh_export()
    assert_arrays(got, want)
    assert_encloses(got, pv_of(cur))
    assert_meshes(A, cur)
    assert np.array_equal(bits(A.mesh_arrays(0)[1]), bits(three_meshes()[0][1]))   # mesh 0 kept its normals
    assert_frames(frame(A, cam=CAM3), fa)   # and the read-back changed nothing on the device
    del tv1, tn1, tv0


@pytest.mark.gpu
def test_vertices_without_normals_on_an_uploaded_scene():
    """9. normals=None through the synchronous entry: the vertices change, the normals stay."""
    V0, N0, F = standin()
    V1, _ = displaced(V0, F, 1)
    A = scene_a(V0, N0, F)
    ex0 = A.bvh_export()
    f0 = frame(A)
    assert A.updateMesh(0, V1) > 0.0
    fa = frame(A)
    B = scene_a(V1, N0, F)
    want = refit(ex0, a_prim_verts(V1, F))
    import_bvh(B, want)
    assert_frames(fa, frame(B))
    assert not np.array_equal(bits(fa["rgb"]), bits(f0["rgb"]))
    assert_arrays(A.bvh_export(), want)
    v, n, _, _ = A.mesh_arrays(0)
    assert np.array_equal(bits(v), bits(V1)) and np.array_equal(bits(n), bits(N0))


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["sync", "async"])
def test_edge_values_on_the_device(entry):
    """10. test 6's vertices on an uploaded scene: neither the kernels nor the read-back flush a
    subnormal, and the empty box does to +-1e12 and beyond what the restatement says."""
    V0, V1, N, F = edge_mesh()
    assert_edge_premises(V1)
    P, pv = edge_scene(V0, N, F)
    ex0 = P.bvh_export()
    frame(P, 32, 32)   # uploaded
    if entry == "sync":
        assert P.updateMesh(1, V1, N) > 0.0
    else:
        import torch
        tv, tn = torch.from_numpy(V1).cuda(), torch.from_numpy(N).cuda()
        assert P.updateMesh(1, tv, tn) is None
    got = P.bvh_export()
    want = refit_of(ex0, pv(V1))
    assert_arrays(got, want)
    assert np.array_equal(bits(got[2]), bits(want[2]))
    assert_encloses(got, pv(V1))
    assert np.array_equal(bits(P.mesh_arrays(1)[0]), bits(V1))
    P.updateMesh(1, V0, N)
    assert_arrays(P.bvh_export(), ex0)


class Given:
    """What restated_surfaces asks of a scene, with the meshes' arrays as the test gave them
    (the topology, which no update changes, from the scene)."""

    def __init__(self, P, meshes):
        self.P, self.meshes, self.handle = P, meshes, P.handle

    def primObject(self, prim):
        return self.P.primObject(prim)

    def mesh_arrays(self, m):
        return self.meshes[m]


def same_words(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
def test_every_entry_after_a_refit():
    """11. the timed trace, the any-hit trace, sampleRays, shadeHits and hitSurfaces read the
    same verts / normals / leaves: A after an update of its later meshes against B, and the
    surfaces against test_hit_surfaces.py's restatement at the new vertices and normals."""
    o, d, t = camera(CAM3).rays(64, 64)
    rng = np.random.default_rng(23)
    ro = np.asarray(rng.uniform(-1, 1, (1024, 3)) * [12, 4, 12] + [3.25, 6, 0], F32)
    rd = np.asarray(rng.uniform(-1, 1, (1024, 3)) * [9, 3, 3] + [3.25, 3, 0] - ro, F32)
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    o = np.concatenate([o.reshape(-1, 3), ro]).astype(F32)
    d = np.concatenate([d.reshape(-1, 3), rd]).astype(F32)
    t = np.concatenate([t.reshape(-1), rng.uniform(0, 1, 1024)]).astype(F32)
    A = three_mesh_scene(*three_meshes())
    ex0 = A.bvh_export()
    before = A.traceRays(o, d, t)   # uploaded
    cur = three_meshes()
    for m, V, N in updates()[:2] + [updates()[2][:2] + (None,)]:   # mesh 0 keeps its normals
        A.updateMesh(m, V, N)
        cur = given(cur, m, V, N)
    B = b_three(cur, refit(ex0, pv_of(cur)))
    ha, hb = A.traceRays(o, d, t), B.traceRays(o, d, t)
    assert same_words(ha, hb)
    assert not same_words(ha, before)
    meshes_hit = {A.primObject(int(p))[0] for p in np.unique(ha["prim"][ha["prim"] >= 0])}
    assert meshes_hit == {0, 1, 2} and (ha["prim"] < 0).any()
    assert same_words(A.traceBatch(o, d, any_hit=True), B.traceBatch(o, d, any_hit=True))
    (ra, sa), (rb, sb) = (P.sampleRays(o, d, t, seed=5, want_hits=True) for P in (A, B))
    assert same_words(sa, sb)
    assert np.array_equal(bits(ra), bits(rb)) and len(np.unique(bits(ra), axis=0)) > 100
    assert np.array_equal(bits(A.shadeHits(o, d, sa, t, seed=5)), bits(B.shadeHits(o, d, sb, t, seed=5)))
    fa, fb = A.hitSurfaces(o, d, ha), B.hitSurfaces(o, d, hb)
    assert fa.tobytes() == fb.tobytes()
    want = restated_surfaces(Given(A, cur), o, d, ha)
    for k in ("mesh", "tri", "inst"):
        assert np.array_equal(fa[k], want[k]), k
    for k in ("p", "geo_n", "n"):
        assert np.array_equal(bits(fa[k]), bits(want[k])), k
    assert_meshes(A, cur)


def up(v, dy):
    return tuple(np.asarray(v, np.float64) + [0, dy, 0])


def chain_case(kind, dy):
    """(scene_a keywords, camera) with the light and the camera dy higher."""
    def light():
        if kind == "mirror":
            pl = miro.PointLight()
            pl.setPosition(up((5, 12, 8), dy))
            pl.setPower(800)
            return pl
        rl = miro.RectangleLight()
        rl.setVertices(up((-2, 11, 4), dy), up((2, 11, 4), dy), up((-2, 11, 8), dy))
        rl.setPower(700)
        rl.setSamples(2)
        return rl
    m = ALWAYS_MIRROR
    mat = miro.Blinn(m["kd"], specExp=m["specExp"], specAmt=m["specAmt"], reflectAmt=m["reflectAmt"], ior=m["ior"])
    if kind != "mirror":   # the Blinn of test_chain.py's pt_rect_panel: Lambert surfaces end a path
        mat = miro.Blinn((0.7, 0.7, 0.7), specExp=8.0, specAmt=0.25, reflectAmt=0.3)
    kw = dict(light=light, material=mat) if kind == "mirror" else dict(light=light, material=mat, num_paths=4, path_trace=3)
    return kw, dict(CAM, eye=up(CAM["eye"], dy), lookAt=up(CAM["lookAt"], dy))


def assert_chain_frames(a, b):
    assert_frames(a, b)
    assert a["secondary_rays"] == b["secondary_rays"] and a["secondary_rays"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["sync", "async"])
@pytest.mark.parametrize("kind", ["mirror", "rect_paths4"])
def test_chain_engine_and_binned_levels_after_a_refit(kind, entry):
    """12. reflection (an always-mirror stand-in over a Lambert floor, a point light) and path
    tracing (a rectangle light, four paths), unbinned and binned.  Both meshes move up by twice
    the height of the root box the replica was uploaded with (the axis on which the scene is
    thin, so that the light and the camera can stand where they light and see it): every ray
    origin of the deeper levels lies outside that box, its origin cell clamped.  The
    synchronous entry refreshes the binning box, the async one leaves it stale, and no result
    depends on it."""
    V0, N0, F = standin()
    fl0 = floor_mesh()
    lo = np.minimum(V0.min(0), fl0.verts.min(0))
    hi = np.maximum(V0.max(0), fl0.verts.max(0))
    dy = F32(2) * F32(hi[1] - lo[1])
    V1 = np.asarray(V0 + [0, dy, 0], F32)
    fl1 = np.asarray(fl0.verts + [0, dy, 0], F32)
    assert V1[:, 1].min() > hi[1] and fl1[:, 1].min() > hi[1]
    kw, cam = chain_case(kind, dy)
    W = H = 48
    frames = {}
    for b in (0, 6):
        with tuned(bin=b):
            A = scene_a(V0, N0, F, **kw)
            ex0 = A.bvh_export()
            root = ex0[0][0].reshape(6, 4)[:, ex0[1][0] != EMPTY]   # the uploaded root box is the one assumed
            assert np.array_equal(root[:3].min(1), lo) and np.array_equal(root[3:].max(1), hi)
            frame(A, W, H, cam)   # uploaded
            if entry == "sync":
                A.updateMesh(0, V1, N0)
                A.updateMesh(1, fl1, fl0.normals)
            else:
                import torch
                tv, tn, tf = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (V1, N0, fl1))
                A.updateMesh(0, tv, tn)
                A.updateMesh(1, tf)
            fa = frame(A, W, H, cam)
            B = scene_a(V1, N0, F, floor=fl1, **kw)
            want = refit(ex0, a_prim_verts(V1, F, fl1))
            import_bvh(B, want)
            assert_chain_frames(fa, frame(B, W, H, cam))
            assert (fa["hits"]["prim"] >= 0).mean() > 0.3
            got = A.bvh_export()
            assert_arrays(got, want)
            assert_encloses(got, a_prim_verts(V1, F, fl1))
            frames[b] = fa
    assert_chain_frames(frames[0], frames[6])


def alpha_scene(V):
    """The Cornell fixture (mesh 0) and the textured leaf quads (mesh 1) with an alpha map and
    a normal map, so that the tangent frames at the mesh's normal base are read."""
    _, N, F, NF, UV, T = leaf_quads()
    img, typ = leaf_image()
    tex = miro.Texture(miro.RawImage(img.shape[1], img.shape[0], img, typ))
    rng = np.random.default_rng(11)
    nrm = np.asarray(np.array([0.5, 0.5, 1.0]) + rng.uniform(-0.25, 0.25, (16, 16, 3)) * [1, 1, 0], F32)
    leaf = miro.Blinn((1, 1, 1))
    leaf.setColorMap(tex)
    leaf.setAlphaMap(tex)
    leaf.setNormalMap(miro.Texture(miro.RawImage(16, 16, nrm, miro.TEX_RGB)))
    cfg = scenes.CONFIGS["C1"]
    P = miro.Scene()
    cb = fixture_mesh("cornell_box")
    tm = miro.TriangleMesh()
    tm.setArrays(*cb)
    miro.makeMeshObjs(P, tm, miro.Lambert((0.8, 0.8, 0.8)))
    tm = miro.TriangleMesh()
    tm.setArrays(V, N, F, NF)
    tm.setTexCoords(UV, T)
    miro.makeMeshObjs(P, tm, leaf)
    pl = miro.PointLight()
    pl.setPosition((2.75, 4.5, 2.0))   # on the camera's side: the leaves face it, so their shading normals count
    pl.setPower(150.0)
    P.addLight(pl)
    P.setBGColor(cfg["bg"])
    P.preCalc()
    return P, prim_verts_of((cb[0], cb[2]), (V, F)), N


@pytest.mark.gpu
def test_sync_update_of_an_alpha_mapped_mesh():
    """13. the any-hit and closest-hit walks read the texture coordinates of a lane whose
    triangle moved, and the shading the tangent frames recomputed at nbase[1]: leaves pushed
    about inside the box (each quad as a whole) and bent (each corner a little)."""
    V0 = leaf_quads()[0]
    rng = np.random.default_rng(3)
    V1 = np.asarray(V0 + np.repeat(rng.uniform(-0.4, 0.4, (len(V0) // 4, 3)), 4, 0) + rng.uniform(-0.15, 0.15, V0.shape), F32)
    cam = scenes.CONFIGS["C1"]["camera"]
    A, _, N = alpha_scene(V0)
    ex0 = A.bvh_export()
    f0 = frame(A, cam=cam)
    assert A.updateMesh(1, V1, N) > 0.0
    fa = frame(A, cam=cam)
    B, pv1, _ = alpha_scene(V1)
    want = refit(ex0, pv1)
    import_bvh(B, want)
    assert_frames(fa, frame(B, cam=cam))
    assert not np.array_equal(fa["hits"]["prim"], f0["hits"]["prim"])
    n_cb = len(fixture_mesh("cornell_box")[2])
    leaf = fa["hits"]["prim"] >= n_cb
    assert leaf.sum() > 300 and (fa["rgb"][leaf].sum(-1) > 0).mean() > 0.5   # leaves are seen, and lit
    got = A.bvh_export()
    assert_arrays(got, want)
    assert_encloses(got, pv1)


def later_mesh(seed=None):
    """A small sphere placed behind the motion-blurred one in scene order."""
    bV, bN, bF = blas_mesh()
    V = np.asarray(bV * F32(1.5) + np.array([3.6, 0.4, 3.0], F32), F32)
    if seed is None:
        return V, bN, bF
    rng = np.random.default_rng(seed)
    s = np.sin(V @ rng.uniform(0.5, 2.0, 3) + rng.uniform(0, 6.28))
    c = V.mean(0)
    V1 = np.asarray(V + 0.15 * s[:, None] * (V - c), F32)
    return V1, np.asarray(scenes._smooth_normals(V1.astype(np.float64), bF.astype(np.int64)), F32), bF


@pytest.mark.gpu
def test_static_mesh_behind_a_motion_blurred_one():
    """14. two instances, a motion-blurred mesh and, after it, the static mesh that is updated:
    the verts2 slice at a non-zero base, mbslot / fixed at real prim offsets."""
    V, N, F = standin()
    W = H = 96
    M, pv0, fixed = mixed_scene(V, N, F, later=later_mesh())
    L1 = later_mesh(seed=9)
    at = len(F) + len(PLACED) + len(blas_mesh()[2])   # the later mesh's first prim
    pv1 = pv0.copy()
    pv1[at:at + len(L1[2])] = L1[0][L1[2]]
    assert not np.array_equal(pv1, pv0) and np.array_equal(pv1[at + len(L1[2]):], pv0[at + len(L1[2]):])
    ex0 = M.bvh_export()
    blas0 = M.blas_export(0)
    f0 = frame(M, W, H)
    assert M.updateMesh(3, L1[0], L1[1]) > 0.0
    fm = frame(M, W, H)
    want = refit(ex0, pv1, fixed)
    got = M.bvh_export()
    assert_arrays(got, want)
    assert_encloses(got, pv1, fixed)
    assert_arrays(M.blas_export(0), blas0)
    v, n, _, _ = M.mesh_arrays(3)
    assert np.array_equal(bits(v), bits(L1[0])) and np.array_equal(bits(n), bits(L1[1]))
    assert np.array_equal(bits(M.mesh_arrays(2)[0]), bits(mixed_scene(V, N, F, later=later_mesh())[0].mesh_arrays(2)[0]))
    B, _, _ = mixed_scene(V, N, F, later=L1)
    import_bvh(B, want)   # the import takes instance and motion lanes as it takes plain ones
    assert_frames(fm, frame(B, W, H))
    assert not np.array_equal(bits(fm["rgb"]), bits(f0["rgb"]))
