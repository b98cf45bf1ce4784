"""mrt_scene_rebuild_bvh: a new topology for the world hierarchy from the lanes its packets
hold, on the device (and by the same rule on the host for a scene not uploaded).

The contract is `rebuild_arrays` below, a numpy restatement of DESIGN.md §6i on the canonical
export that does not call the library.  Input: every lane with prim >= 0; its box is box3 of
its triangle's vertices, or its fixed box (ProxyObject / MBObject lanes, passed as refit_arrays
takes them).  Key: per axis c = 0.5f * (lo + hi), e = R.hi - R.lo, t = (c - R.lo) / e * 1024.0f
in single precision, q = 0 when !(e > 0) or !(t >= 0), else min(int(t), 1023); a 30-bit Morton
code (x, y, z per triple, most significant first) << 32 | 4 * packet + lane.  Sorted lanes
fill packets four at a time (data moved, not recomputed); a packet's box merges its lanes in
lane order from the empty box and its key is its first lane's.  The binary radix tree over the
packet keys splits a range where the highest differing bit changes (delta = clz64(first ^
last)); digit = delta >> 1; a binary node roots a 4-wide node iff it is the root or its
parent's digit is smaller; its children are its two binary children in key order, one that is
internal with the same digit replaced by its own two.  A slot's box is the union of the packet
boxes of its range.  Nodes are numbered breadth first, slots in order; a leaf child is ~p.
Integers are compared exactly, floats by value (np.array_equal, no NaN)."""
import ctypes as C
import functools

import numpy as np
import pytest

import miro
from miro import _lib, scenes
from helpers import bits, camera, fixture_mesh, tuned
from test_refit import (CAM, EMPTY, F32, INVALID, NOT_BUILT, PLACED, agreeing, assert_arrays, assert_frames, blas_mesh, box3,
                        floor_mesh, import_bvh, instance_box, point_light, prim_verts_of, refit_of, smax, smin, tri_mesh)
from test_refit_shapes import assert_encloses, same_words

U64 = (1 << 64) - 1
# three instances: test_refit's two and a third in front of the stand-in
PLACED3 = PLACED + [np.array([[0.9, 0, 0, 0.5], [0, 0.9, 0, 0.3], [0, 0, 0.9, 5.0], [0, 0, 0, 1]], F32)]
MOVED3 = [PLACED3[1], PLACED3[2], PLACED3[0]]


# ---------------------------------------------------------------- the yardstick
def quant(lo, hi, rlo, rhi):
    lo, hi, rlo, rhi = F32(lo), F32(hi), F32(rlo), F32(rhi)
    with np.errstate(all="ignore"):
        c = F32(F32(0.5) * F32(lo + hi))
        e = F32(rhi - rlo)
        t = F32(F32(F32(c - rlo) / e) * F32(1024.0))
    if not (e > 0) or not (t >= 0):
        return 0
    return int(t) if t < 1023 else 1023


def morton(qx, qy, qz):
    m = 0
    for b in range(9, -1, -1):
        m = (m << 3) | (((qx >> b) & 1) << 2) | (((qy >> b) & 1) << 1) | ((qz >> b) & 1)
    return m


def clz64(x):
    assert 0 < x <= U64
    return 64 - x.bit_length()


def root_box(node_boxes, node_child):
    used = node_child[0] != EMPTY
    b = node_boxes[0].reshape(6, 4)[:, used]
    return b[:3].min(1).astype(F32), b[3:].max(1).astype(F32)


def lane_boxes(leaf_prims, prim_verts, fixed_boxes):
    """{position 4 * packet + lane: (lo, hi)} of every lane with a prim."""
    out = {}
    for li in range(len(leaf_prims)):
        for k in range(4):
            p = int(leaf_prims[li, k])
            if p < 0:
                continue
            if p in fixed_boxes:
                lo, hi = (np.asarray(x, F32) for x in fixed_boxes[p])
            else:
                lo, hi = box3(*(np.asarray(prim_verts[p, j], F32) for j in range(3)))
            out[4 * li + k] = (lo, hi)
    return out


def rebuild_arrays(node_boxes, node_child, leaf_tris, leaf_prims, prim_verts, fixed_boxes=None):
    """The canonical arrays (node_boxes, node_child, leaf_tris, leaf_prims) after a rebuild."""
    rlo, rhi = root_box(node_boxes, node_child)
    boxes = lane_boxes(leaf_prims, prim_verts, fixed_boxes or {})
    keys = sorted((morton(*(quant(lo[a], hi[a], rlo[a], rhi[a]) for a in range(3))) << 32) | pos
                  for pos, (lo, hi) in boxes.items())
    n = len(keys)
    P = (n + 3) // 4
    lt, lp = np.zeros((P, 36), F32), np.full((P, 4), -1, np.int32)
    plo, phi = np.full((P, 3), 1e12, F32), np.full((P, 3), -1e12, F32)
    for i, key in enumerate(keys):
        src = key & 0xFFFFFFFF
        p, k = i >> 2, i & 3
        lt[p, k::4] = leaf_tris[src >> 2, (src & 3)::4]
        lp[p, k] = leaf_prims[src >> 2, src & 3]
        plo[p], phi[p] = smin(plo[p], boxes[src][0]), smax(phi[p], boxes[src][1])
    pkey = keys[0::4]

    def binary(first, last):   # ("leaf", p) or ("node", first, last, digit, left, right)
        if first == last:
            return ("leaf", first)
        delta = clz64(pkey[first] ^ pkey[last])
        bit = 63 - delta
        g = max(i for i in range(first, last) if not (pkey[i] >> bit) & 1)   # the last key with that bit clear
        return ("node", first, last, delta >> 1, binary(first, g), binary(g + 1, last))

    def children(b):
        out = []
        for c in b[4:]:
            if c[0] == "node" and c[3] == b[3]:
                out += list(c[4:])
            else:
                out.append(c)
        assert 2 <= len(out) <= 4
        return out

    nodes = [binary(0, P - 1)]
    nb, nc = [], []
    q = 0
    while q < len(nodes):
        b = nodes[q]
        q += 1
        box, ch = np.zeros(24, F32), np.full(4, EMPTY, np.int32)
        kids = [b] if b[0] == "leaf" else children(b)   # P == 1: the root holds the packet
        for k, c in enumerate(kids):
            if c[0] == "leaf":
                ch[k] = ~c[1]
                first = last = c[1]
            else:
                ch[k] = len(nodes)
                nodes.append(c)
                first, last = c[1], c[2]
            box[[k, 4 + k, 8 + k]] = plo[first:last + 1].min(0)
            box[[12 + k, 16 + k, 20 + k]] = phi[first:last + 1].max(0)
        nb.append(box)
        nc.append(ch)
    return np.array(nb, F32), np.array(nc, np.int32), lt, lp


def cost_of(export):
    """mrt_scene_bvh_cost in numpy: double, every used slot, a leaf slot once per lane."""
    nb, nc, lt, lp = export
    b = nb.astype(np.float64).reshape(-1, 6, 4)

    def area(lo, hi):
        d = hi - lo
        return 2.0 * (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0])
    used0 = nc[0] != EMPTY
    ra = area(b[0, :3][:, used0].min(1), b[0, 3:][:, used0].max(1))
    if not ra > 0:
        return 0.0
    total = 0.0
    for i in range(len(nc)):
        for k in range(4):
            c = int(nc[i, k])
            if c == EMPTY:
                continue
            w = 1.0 if c >= 0 else float((lp[~c] >= 0).sum())
            total += w * (area(b[i, :3, k], b[i, 3:, k]) / ra)
    return total


# ---------------------------------------------------------------- scenes
def lambert_scene(*meshes, light=True):
    """World meshes (V, N, F) in order, one Lambert each, a point light."""
    P = miro.Scene()
    for i, (V, N, F) in enumerate(meshes):
        miro.makeMeshObjs(P, tri_mesh(V, N, F), miro.Lambert((0.8, 0.7 - 0.1 * i, 0.6)))
    if light:
        P.addLight(point_light())
    P.setBGColor((0.1, 0.1, 0.3))
    P.preCalc()
    return P


def soup(tris):
    """(V, N, F) of separate triangles tris[(t, corner, xyz)]."""
    V = np.asarray(tris, F32).reshape(-1, 3)
    return V, np.tile(np.array([[0, 0, 1]], F32), (len(V), 1)), np.arange(len(V), dtype=np.uint32).reshape(-1, 3)


def line_tris(n=256):
    """n small triangles on a line along x, four Morton cells apart: every packet key differs
    from the next in an x bit alone, and no two bit levels of x share a digit."""
    base = np.array([[0, 0, 0], [0.05, 0, 0], [0, 0.05, 0.01]], F32)
    x = (np.arange(n, dtype=F32) * F32(0.0625)).astype(F32)
    return soup(base[None] + np.stack([x, np.zeros(n, F32), np.zeros(n, F32)], 1)[:, None, :])


def flat_mesh():
    """A 6 x 5 grid of quads in the plane y = 1.5: the root box has no extent in y."""
    gx, gz = np.meshgrid(np.arange(7, dtype=F32), np.arange(6, dtype=F32))
    V = np.stack([gx.ravel() * F32(0.75) - F32(2), np.full(42, 1.5, F32), gz.ravel() * F32(0.5)], 1).astype(F32)
    F = []
    for j in range(5):
        for i in range(6):
            a = 7 * j + i
            F += [[a, a + 1, a + 8], [a, a + 8, a + 7]]
    return V, np.tile(np.array([[0, 1, 0]], F32), (42, 1)), np.array(F, np.uint32)


@functools.lru_cache(maxsize=None)
def teapot():
    v, n, vi, ni = fixture_mesh("teapot")
    return np.asarray(v, F32), np.asarray(n, F32), np.asarray(vi, np.uint32).reshape(-1, 3), np.asarray(ni, np.uint32).reshape(-1, 3)


def teapot_scene():
    v, n, vi, ni = teapot()
    P = miro.Scene()
    tm = miro.TriangleMesh()
    tm.setArrays(v, n, vi, ni)
    miro.makeMeshObjs(P, tm, miro.Lambert((0.8, 0.7, 0.6)))
    P.addLight(point_light())
    P.setBGColor((0.1, 0.1, 0.3))
    P.preCalc()
    return P, prim_verts_of((v, vi)), {}


TEAPOT_CAM = dict(eye=(0.2, 2.2, 4.6), lookAt=(0.1, 0.9, 0), up=(0, 1, 0), fov=45)   # the teapot fills the view


class Kinds:
    """All four lane kinds at once: a plain mesh (a small stand-in sphere, mesh 0), an
    alpha-mapped mesh (mesh 1), the three instances PLACED3 of a small sphere (mesh 2), a motion-blurred
    sphere (mesh 3) and a floor (mesh 4).  line: the triangles of line_tris as mesh 0 instead
    (True: 256 of them, or their number), whose rebuilt tree needs more nodes than the built one
    has.  lights: the scene's lights in place of the point light.  cutout: the alpha map is an
    RGBA checkerboard of 2 x 2 texels whose alpha channel cuts every other square out, and the
    instanced sphere has that material too (alpha lanes inside an instance)."""

    def __init__(self, mats=PLACED3, line=False, mb=None, plain=None, lights=None, cutout=False):
        P = self.P = miro.Scene()
        if line:
            V, N, F = line_tris(256 if line is True else int(line))
            V = np.asarray(V * F32(0.5) + np.array([-4.0, 2.0, 0.0], F32), F32)
        else:
            V, F, N = scenes.bunny_standin(10, 5)
            V, N, F = np.asarray(V, F32), np.asarray(N, F32), np.asarray(F, np.uint32)
        if plain is not None:
            V = plain
        self.V, self.N, self.F = V, N, F
        miro.makeMeshObjs(P, tri_mesh(V, N, F), miro.Lambert((0.8, 0.7, 0.6)))
        # a quad with an alpha map: its lanes set the check bit of their packets
        aV = np.array([[-3, 0.5, 3], [-1, 0.5, 3], [-1, 2.5, 3], [-3, 2.5, 3]], F32)
        aF = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
        am = tri_mesh(aV, np.tile(np.array([[0, 0, 1]], F32), (4, 1)), aF)
        am.setTexCoords(np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F32), aF)
        alpha = miro.Lambert((0.9, 0.9, 0.2))
        tex = np.asarray((np.indices((8, 8)).sum(0) % 2)[..., None], F32)   # a checkerboard, one channel
        if cutout:
            rgba = np.ones((8, 8, 4), F32)
            rgba[..., 3] = (np.indices((8, 8)) // 2).sum(0) % 2
            alpha.setAlphaMap(miro.Texture(miro.RawImage(8, 8, rgba, miro.TEX_RGBA)))
        else:
            alpha.setAlphaMap(miro.Texture(miro.RawImage(8, 8, tex, miro.TEX_GRAY)))
        miro.makeMeshObjs(P, am, alpha)
        self.bV, self.bN, self.bF = blas_mesh()
        objs, bvh = miro.Objects(), miro.BVH()
        bm = tri_mesh(self.bV, self.bN, self.bF)
        if cutout:   # the checkerboard once across the sphere (x in [-0.6, 0.6], y in [0.05, 1.25])
            bm.setTexCoords(np.asarray((self.bV[:, :2] + F32(0.6)) / F32(1.25), F32), self.bF)
        miro.ProxyObject.setupProxy(bm, alpha if cutout else miro.Lambert((0.3, 0.8, 0.4)), objs, bvh)
        self.mats = list(mats)
        for M in self.mats:
            P.addObject(miro.ProxyObject(objs, bvh, miro.Matrix4x4(M)))
        self.mV = np.asarray(self.bV * F32(0.7) + np.array([0.0, 6.4, 2.0], F32), F32) if mb is None else mb[0]
        self.mV2 = np.asarray(self.mV + np.array([0.35, 0.1, 0.0], F32), F32) if mb is None else mb[1]
        miro.makeMBMeshObjs(P, tri_mesh(self.mV, self.bN, self.bF), tri_mesh(self.mV2, self.bN, self.bF), miro.Lambert((0.9, 0.4, 0.3)))
        fl = floor_mesh()
        miro.makeMeshObjs(P, fl, miro.Lambert((0.6, 0.6, 0.6)))
        for l in ([point_light()] if lights is None else lights):
            P.addLight(l)
        P.setBGColor((0.1, 0.1, 0.3))
        P.preCalc()
        self.inst0 = len(F) + len(aF)           # the proxies' world prims
        self.mb0 = self.inst0 + len(self.mats)   # the motion-blurred triangles'
        self.entries = [(V, F), (aV, aF), len(self.mats), (self.mV, self.bF), (fl.verts, fl.vidx)]
        self.ids = dict(plain=0, alpha=1, blas=2, mb=3, floor=4)

    def pv(self, plain=None, mV=None):
        e = list(self.entries)
        if plain is not None:
            e[0] = (plain, self.F)
        if mV is not None:
            e[3] = (mV, self.bF)
        return prim_verts_of(*e)

    def fixed(self, mats=None, mb=None, root=None):
        root = self.P.blas_export(0)[0][0] if root is None else root
        out = {self.inst0 + i: instance_box(root, M) for i, M in enumerate(mats or self.mats)}
        mV, mV2 = mb if mb is not None else (self.mV, self.mV2)
        for t, f in enumerate(self.bF):
            lo, hi = box3(*mV[f])
            lo2, hi2 = box3(*mV2[f])
            out[self.mb0 + t] = (smin(lo, lo2), smax(hi, hi2))
        return out


def _one():
    V, N, F = soup([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
    return lambert_scene((V, N, F)), prim_verts_of((V, F)), {}


def _five():
    rng = np.random.default_rng(5)
    V, N, F = soup(rng.uniform(-2, 2, (5, 3, 3)))
    return lambert_scene((V, N, F)), prim_verts_of((V, F)), {}


def _identical():
    V, N, F = soup(np.tile(np.array([[[0, 0, 0], [1, 0, 0.5], [0, 1, 0.25]]], F32), (70, 1, 1)))
    return lambert_scene((V, N, F)), prim_verts_of((V, F)), {}


def _line():
    V, N, F = line_tris()
    return lambert_scene((V, N, F)), prim_verts_of((V, F)), {}


def _flat():
    V, N, F = flat_mesh()
    return lambert_scene((V, N, F)), prim_verts_of((V, F)), {}


def _kinds():
    S = Kinds()
    return S.P, S.pv(), S.fixed()


def _line_kinds():
    S = Kinds(line=True)
    return S.P, S.pv(), S.fixed()


def _line_1028_kinds():
    """The tail fixture with a BLAS at more than one workgroup of packets: P = 275, and the BLAS's
    nodes lie between the world's node range and the tail the rebuild adds."""
    S = Kinds(line=1028)
    return S.P, S.pv(), S.fixed()


FIXTURES = {"one_triangle": _one, "five_triangles": _five, "teapot": teapot_scene, "identical_70": _identical,
            "line_256": _line, "flat": _flat, "four_kinds": _kinds, "line_1028_and_instances": _line_1028_kinds}
GPU_FIXTURES = dict(FIXTURES, line_and_instances=_line_kinds)
TAIL_FIXTURES = ("line_256", "line_and_instances", "line_1028_and_instances")   # M passes the built tree's node count


def assert_tree(export, n_prims, pv, fixed):
    """What any rebuilt tree must be: every world prim once, compact packets, a tree in breadth-
    first order, at least two used slots per node (a lone root aside), the enclosure."""
    nb, nc, lt, lp = export
    prims = lp[lp >= 0]
    assert sorted(prims.tolist()) == list(range(n_prims)), "every world prim once"
    P = (n_prims + 3) // 4
    assert len(lp) == P and (lp[:-1] >= 0).all(), "full packets before the last"
    last = lp[-1] >= 0
    assert last[0] and (last[:-1] | ~last[1:]).all(), "the last packet's lanes are its first"
    assert (lt[-1].reshape(9, 4)[:, ~last] == 0).all()
    inner = nc[(nc >= 0)]
    assert sorted(inner.tolist()) == list(range(1, len(nc))), "every node but the root has one parent"
    for i in range(len(nc)):
        used = nc[i] != EMPTY
        assert (used[:-1] | ~used[1:]).all(), "used slots first"
        assert used.sum() >= (1 if len(nc) == 1 and P == 1 else 2)
        assert all(c > i for c in nc[i][nc[i] >= 0]), "children after their parent"
        assert (nb[i].reshape(6, 4)[:, ~used] == 0).all(), "empty slots keep a zero box"
    leaves = nc[(nc < 0) & (nc != EMPTY)]
    assert sorted((~leaves).tolist()) == list(range(P)), "every packet in one slot"
    assert_encloses(export, pv, fixed)


# ---------------------------------------------------------------- CPU tests: the host path
def test_symbols_and_wrapper():
    L = miro.lib()
    for name in ("mrt_scene_rebuild_bvh", "mrt_scene_rebuild_bvh_async", "mrt_scene_bvh_cost"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert callable(miro.Scene.rebuildBVH) and callable(miro.Scene.bvhCost)
    assert L.mrt_abi_version() == 10


@pytest.mark.parametrize("name", list(FIXTURES))
def test_host_rebuild_is_the_restatement(name):
    """A scene that is built and not uploaded: the export after rebuildBVH() equals
    rebuild_arrays of the export before it; the tree's properties; an identity refit changes
    nothing; bvhCost is the numpy sum; a second rebuild against the state before it."""
    P, pv, fixed = FIXTURES[name]()
    n = P.bvh_info["prims"]
    ex0 = P.bvh_export()
    built_nodes = P.bvh_info["nodes"]
    assert P.bvhCost() == pytest.approx(cost_of(ex0), rel=1e-12)
    assert P.rebuildBVH() == 0.0
    want = rebuild_arrays(*ex0, pv, fixed)
    ex1 = P.bvh_export()
    assert_arrays(ex1, want)
    assert P.bvh_info["nodes"] == len(want[1]) and P.bvh_info["leaves"] == len(want[3]) == (n + 3) // 4
    assert P.bvh_info["prims"] == n
    assert_tree(ex1, n, pv, fixed)
    assert_arrays(refit_of(ex1, pv, fixed), ex1)
    assert P.bvhCost() == pytest.approx(cost_of(ex1), rel=1e-12)
    if name == "one_triangle":
        assert len(ex1[1]) == 1 and ex1[1][0].tolist() == [~0, EMPTY, EMPTY, EMPTY]
    if name == "line_256":   # every node is binary, and the tree outgrows the built one's node range
        assert len(ex1[1]) == 63 == len(ex1[3]) - 1 and ((ex1[1] != EMPTY).sum(1) == 2).all()
        assert len(ex1[1]) > built_nodes
    if name == "line_1028_and_instances":   # the premise: more than one workgroup of packets, a tail, a BLAS before it
        assert (n, len(ex1[3]), len(ex1[1]), built_nodes) == (1098, 275, 272, 179)
        assert P.instance_count() == 3 and P.blas_export(0)[1].shape[0] > 0
    if name == "identical_70":   # equal codes: the order is the positions'
        order = [4 * li + k for li in range(len(ex0[3])) for k in range(4) if ex0[3][li, k] >= 0]
        assert ex1[3].ravel()[:70].tolist() == [int(ex0[3].ravel()[p]) for p in sorted(order)]
    if name == "flat":
        lo, hi = root_box(ex0[0], ex0[1])
        assert lo[1] == hi[1]
    # again: the same lanes from other positions (equal-code lanes may change places)
    assert P.rebuildBVH() == 0.0
    ex2 = P.bvh_export()
    assert_arrays(ex2, rebuild_arrays(*ex1, pv, fixed))
    assert_tree(ex2, n, pv, fixed)


def test_the_four_kinds_scene_has_all_four_after_a_rebuild():
    """The fixture's premise and that a rebuild keeps it: three proxies, the motion-blurred and the
    alpha-mapped triangles each in one lane, before and after."""
    S = Kinds()
    assert S.P.instance_count() == 3
    assert S.P.bvh_info["prims"] == S.mb0 + len(S.bF) + 1
    before = np.sort(S.P.bvh_export()[3][S.P.bvh_export()[3] >= 0])
    assert S.P.rebuildBVH() == 0.0
    lp = S.P.bvh_export()[3]
    assert np.array_equal(np.sort(lp[lp >= 0]), before) and lp.max() == S.mb0 + len(S.bF)
    assert S.P.instance_count() == 3


def test_the_line_scene_outgrows_its_node_range():
    """The premise of the grown node array: M of the rebuilt line scene passes the node count of
    the built tree, whose node array continues with the BLAS's nodes."""
    S = Kinds(line=True)
    built = S.P.bvh_info["nodes"]
    want = rebuild_arrays(*S.P.bvh_export(), S.pv(), S.fixed())
    assert len(want[1]) > built
    assert S.P.blas_export(0)[1].shape[0] > 0
    assert S.P.rebuildBVH() == 0.0
    assert S.P.bvh_info["nodes"] == len(want[1]) > built
    assert_arrays(S.P.bvh_export(), want)


def test_a_host_rebuild_after_host_refits():
    """Refits on the host, then the rebuild: the lanes' boxes are those of the vertices,
    matrices and vertex sets of now."""
    S = Kinds()
    V1 = np.asarray(S.V * F32(1.5) + np.array([1.0, 0.0, -2.0], F32), F32)
    S.P.updateMesh(S.ids["plain"], V1)
    mats = MOVED3
    S.P.updateInstances(mats)
    mb = (np.asarray(S.mV + np.array([0.0, -3.0, 0.0], F32), F32), np.asarray(S.mV2 + np.array([0.5, -3.0, 0.0], F32), F32))
    S.P.deformMesh(S.ids["mb"], mb[0], verts2=mb[1])
    ex0 = S.P.bvh_export()
    pv, fixed = S.pv(plain=V1, mV=mb[0]), S.fixed(mats, mb)
    assert S.P.rebuildBVH() == 0.0
    ex1 = S.P.bvh_export()
    assert_arrays(ex1, rebuild_arrays(*ex0, pv, fixed))
    assert_tree(ex1, S.P.bvh_info["prims"], pv, fixed)
    # and a host refit on the rebuilt topology
    S.P.updateMesh(S.ids["plain"], S.V)
    assert_arrays(S.P.bvh_export(), refit_of(ex1, S.pv(mV=mb[0]), fixed))


def test_error_codes():
    L = miro.lib()
    cost = C.c_double(-1.0)
    assert L.mrt_scene_rebuild_bvh(None, None) == INVALID and b"null" in L.mrt_last_error()
    assert L.mrt_scene_rebuild_bvh_async(None, None) == INVALID
    assert L.mrt_scene_bvh_cost(None, C.byref(cost)) == INVALID
    h = L.mrt_scene_create()
    try:
        assert L.mrt_scene_rebuild_bvh(h, None) == NOT_BUILT and b"not built" in L.mrt_last_error()
        assert L.mrt_scene_rebuild_bvh_async(h, None) == NOT_BUILT
        assert L.mrt_scene_bvh_cost(h, C.byref(cost)) == NOT_BUILT
    finally:
        L.mrt_scene_destroy(h)
    P, pv, fixed = _five()
    assert L.mrt_scene_bvh_cost(P.handle, None) == INVALID
    ex = P.bvh_export()
    import_bvh(P, ex)
    assert L.mrt_scene_rebuild_bvh(P.handle, None) == INVALID and b"import" in L.mrt_last_error()
    assert L.mrt_scene_rebuild_bvh_async(P.handle, None) == INVALID and b"import" in L.mrt_last_error()
    assert_arrays(P.bvh_export(), ex)   # nothing changed
    Q, _, _ = _five()   # the async form needs a replica
    assert L.mrt_scene_rebuild_bvh_async(Q.handle, None) == INVALID and b"uploaded" in L.mrt_last_error()
    assert L.mrt_scene_bvh_cost(Q.handle, C.byref(cost)) == 0 and cost.value == pytest.approx(cost_of(ex), rel=1e-12)


def test_cost_of_a_degenerate_root_is_zero():
    V, N, F = soup([[[1, 2, 3], [1, 2, 3], [1, 2, 3]]])
    P = lambert_scene((V, N, F))
    assert P.bvhCost() == 0.0
    P.rebuildBVH()
    assert P.bvhCost() == 0.0


# ---------------------------------------------------------------- GPU tests
def counted(P, cam, W=64, H=64):
    img = miro.Image()
    img.resize(W, H)
    hits = P.raytraceImage(camera(cam), img, want_hits=True, count_visits=True)
    st = P.last_stats
    return dict(rgb=img.rgb.copy(), rgb8=img.pixels.copy(), hits=hits.copy(), shadow_rays=st["shadow_rays"],
                secondary_rays=st["secondary_rays"], primary_rays=st["primary_rays"],
                visits=(st["primary_node_visits"], st["primary_leaf_visits"], st["node_visits"], st["leaf_visits"]))


def assert_counted(a, b):
    assert_frames(a, b)
    assert a["primary_rays"] == b["primary_rays"] and a["visits"] == b["visits"]


def cam_of(name):
    if name == "teapot":
        return TEAPOT_CAM
    if name == "four_kinds":
        return CAM
    if name in ("line_and_instances", "line_1028_and_instances"):   # the first instance fills a third of the view
        return dict(eye=(-4.5, 1.2, 5.0), lookAt=(-4.5, 0.8, 1.5), up=(0, 1, 0), fov=45)
    if name in ("line_256",):
        return dict(eye=(8.0, 0.02, 1.5), lookAt=(8, 0.02, 0), up=(0, 1, 0), fov=60)   # a pixel is half a triangle wide
    return dict(eye=(0.5, 1.0, 7.0), lookAt=(0.5, 0.8, 0), up=(0, 1, 0), fov=60)


def queries(P, cam):
    """Every ray entry on the 64 x 64 camera rays: closest and any-hit traces, sampleRays,
    shadeHits, hitSurfaces and sampleLights at the hit points."""
    o, d, t = camera(cam).rays(64, 64)
    o, d, t = o.reshape(-1, 3).astype(F32), d.reshape(-1, 3).astype(F32), t.reshape(-1).astype(F32)
    h = P.traceRays(o, d, t)
    rad, sh = P.sampleRays(o, d, t, seed=5, want_hits=True)
    surf = P.hitSurfaces(o, d, h)
    return dict(closest=h, anyhit=P.traceBatch(o, d, any_hit=True), rad=rad, sample_hits=sh,
                shaded=P.shadeHits(o, d, sh, t, seed=5), surf=surf,
                lights=P.sampleLights(np.ascontiguousarray(surf["p"], F32), np.ascontiguousarray(surf["n"], F32), seed=7))


def assert_queries(a, b):
    for k in ("closest", "anyhit", "sample_hits"):
        assert same_words(a[k], b[k]), k
    for k in ("rad", "shaded", "lights"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert a["surf"].tobytes() == b["surf"].tobytes()


def tensor(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, F32)).cuda().contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GPU_FIXTURES))
def test_device_rebuild_is_the_restatement(name):
    """The synchronous form on an uploaded scene: the export equals the restatement; against a
    twin B that imports the restated arrays every frame product and every ray entry is equal bit
    for bit; a second rebuild; a re-upload renders the same frame; the resources return."""
    L = miro.lib()
    live0 = L.mrt_debug_live_resources()
    cam = cam_of(name)
    A, pv, fixed = GPU_FIXTURES[name]()
    n = A.bvh_info["prims"]
    ex0 = A.bvh_export()
    built = A.bvh_info["nodes"]
    f0 = counted(A, cam)   # uploaded
    assert A.rebuildBVH() > 0.0
    want = rebuild_arrays(*ex0, pv, fixed)
    ex1 = A.bvh_export()
    assert_arrays(ex1, want)
    assert A.bvh_info["nodes"] == len(want[1]) and A.bvh_info["leaves"] == len(want[3])
    assert_tree(ex1, n, pv, fixed)
    if name in TAIL_FIXTURES:
        assert len(want[1]) > built   # the grown node array
    assert A.bvhCost() == pytest.approx(cost_of(want), rel=1e-12)
    B, _, _ = GPU_FIXTURES[name]()
    import_bvh(B, want)
    fa, fb = counted(A, cam), counted(B, cam)
    assert_counted(fa, fb)
    assert (fa["hits"]["prim"] >= 0).sum() > 20   # the scene is in view
    if name in ("line_and_instances", "line_1028_and_instances"):
        assert (fa["hits"]["prim"] >= n).sum() > 50   # and so are its instances, as before
        assert np.array_equal(fa["hits"]["prim"] >= n, f0["hits"]["prim"] >= n)
    assert_queries(queries(A, cam), queries(B, cam))
    # again on the device, from the rebuilt state
    assert A.rebuildBVH() > 0.0
    ex2 = A.bvh_export()
    assert_arrays(ex2, rebuild_arrays(*ex1, pv, fixed))
    # a re-upload after a rebuild: the same frame
    f2 = counted(A, cam)
    _lib.check(L.mrt_scene_set_material_gloss(A.handle, 0, 1.0), "gloss")   # marks the replica stale
    up = A.uploadCount()
    f3 = counted(A, cam)
    assert A.uploadCount() == up + 1
    assert_counted(f2, f3)
    assert_arrays(A.bvh_export(), ex2)
    for P in (A, B):
        L.mrt_scene_destroy(P._h)
        P._h = None
    assert L.mrt_debug_live_resources() == live0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GPU_FIXTURES))
def test_async_rebuild_is_the_restatement(name):
    """The async form as the first rebuild of a replica (it allocates; P == 1 and the grown node
    array among the fixtures), twice in a row on a torch stream, a frame on that stream, then the
    read-backs: the export equals the restatement applied twice, the frame a twin's."""
    import torch
    from test_instance_update import async_frame
    cam = cam_of(name)
    A, pv, fixed = GPU_FIXTURES[name]()
    ex0 = A.bvh_export()
    counted(A, cam)   # uploaded
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert A.rebuildBVH(stream=st) is None
    assert A.rebuildBVH(stream=st) is None
    rgb, rgb8 = async_frame(A, st, 64, 64, cam)
    want = rebuild_arrays(*rebuild_arrays(*ex0, pv, fixed), pv, fixed)
    B, _, _ = GPU_FIXTURES[name]()
    import_bvh(B, want)
    fb = counted(B, cam)
    assert np.array_equal(bits(rgb), bits(fb["rgb"])) and np.array_equal(rgb8, fb["rgb8"])
    assert_arrays(A.bvh_export(), want)
    assert A.bvh_info["nodes"] == len(want[1]) and A.bvh_info["leaves"] == len(want[3])
    assert_counted(counted(A, cam), fb)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("line", [False, True])
def test_async_rebuild_after_an_async_deform(line):
    """The async form on a torch stream after an async deform of the plain mesh: a frame on that
    stream, then the read-backs (info, export, cost) against the restatement and a twin."""
    import torch
    from test_instance_update import async_frame
    S = Kinds(line=line)
    A = S.P
    V1 = np.asarray(S.V + np.array([0.5, 0.25, -0.5], F32), F32)
    ex0 = A.bvh_export()
    counted(A, CAM)   # uploaded
    st = torch.cuda.Stream()
    tv = tensor(V1)
    torch.cuda.synchronize()
    assert A.updateMesh(S.ids["plain"], tv, stream=st) is None
    assert A.rebuildBVH(stream=st) is None
    rgb, rgb8 = async_frame(A, st, 64, 64)
    pv, fixed = S.pv(plain=V1), S.fixed()
    refitted = refit_of(ex0, pv, fixed)
    want = rebuild_arrays(*refitted, pv, fixed)
    T = Kinds(line=line, plain=V1)
    import_bvh(T.P, want)
    fb = counted(T.P, CAM)
    assert np.array_equal(bits(rgb), bits(fb["rgb"])) and np.array_equal(rgb8, fb["rgb8"])
    info = _lib.mrt_bvh_info()
    _lib.check(miro.lib().mrt_scene_bvh_info(A.handle, C.byref(info)), "bvh_info")   # reads the counts back
    assert info.nodes == len(want[1]) and info.leaves == len(want[3])
    assert_arrays(A.bvh_export(), want)
    assert A.bvhCost() == pytest.approx(cost_of(want), rel=1e-12)
    # a second async rebuild straight after the first, then an async refit: the schedule is made again
    assert A.rebuildBVH(stream=st) is None
    assert A.rebuildBVH(stream=st) is None
    assert A.updateMesh(S.ids["plain"], tensor(S.V), stream=st) is None
    st.synchronize()
    w2 = rebuild_arrays(*rebuild_arrays(*want, pv, fixed), pv, fixed)
    assert_arrays(A.bvh_export(), refit_of(w2, S.pv(), fixed))
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_refits_after_a_rebuild():
    """updateMesh, updateInstances and deformMesh of the motion-blurred mesh after a rebuild equal
    refit_arrays on the rebuilt topology: the height schedule is made again."""
    S = Kinds()
    A = S.P
    ex0 = A.bvh_export()
    counted(A, CAM)   # uploaded
    A.updateMesh(S.ids["plain"], S.V)   # the first refit's schedule, of the built topology
    assert A.rebuildBVH() > 0.0
    ex1 = A.bvh_export()
    assert_arrays(ex1, rebuild_arrays(*ex0, S.pv(), S.fixed()))
    V1 = np.asarray(S.V * F32(0.75) + np.array([0.5, 0.25, -0.5], F32), F32)
    assert A.updateMesh(S.ids["plain"], V1) > 0.0
    assert_arrays(A.bvh_export(), refit_of(ex1, S.pv(plain=V1), S.fixed()))
    mats = MOVED3
    assert A.updateInstances(mats) > 0.0
    assert_arrays(A.bvh_export(), refit_of(ex1, S.pv(plain=V1), S.fixed(mats)))
    mb = (np.asarray(S.mV + np.array([0.0, -3.0, 0.0], F32), F32), np.asarray(S.mV2 + np.array([0.5, -3.0, 0.0], F32), F32))
    assert A.deformMesh(S.ids["mb"], mb[0], verts2=mb[1]) > 0.0
    pv, fixed = S.pv(plain=V1, mV=mb[0]), S.fixed(mats, mb)
    ex2 = A.bvh_export()
    assert_arrays(ex2, refit_of(ex1, pv, fixed))
    # and the rebuild of the moved scene, against a twin built there with the restated arrays
    assert A.rebuildBVH() > 0.0
    want = rebuild_arrays(*ex2, pv, fixed)
    assert_arrays(A.bvh_export(), want)
    T = Kinds(mats=mats, mb=mb, plain=V1)
    import_bvh(T.P, want)
    cam = dict(CAM, shutterSpeed=1.0)
    assert_counted(counted(A, cam), counted(T.P, cam))


@pytest.mark.gpu
def test_the_rebuilt_teapot_against_its_host_built_twin():
    """Two trees over the same triangles may differ on ties and grazing box tests: the rebuilt
    scene's hit records equal its host-built twin's on at least 99.9 % of the 64 x 64 rays."""
    A, _, _ = teapot_scene()
    T, _, _ = teapot_scene()
    o, d, _ = camera(TEAPOT_CAM).rays(64, 64)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    ht = T.traceBatch(o, d)
    A.traceBatch(o, d)   # uploaded
    assert A.rebuildBVH() > 0.0
    ha = A.traceBatch(o, d)
    same = (ha.view(np.uint32).reshape(len(o), -1) == ht.view(np.uint32).reshape(len(o), -1)).all(1)
    print("rays with equal hit records:", same.mean(), "hits:", (ht["prim"] >= 0).mean())
    assert (ht["prim"] >= 0).mean() > 0.2
    assert same.mean() >= 0.999
