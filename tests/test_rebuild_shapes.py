"""mrt_scene_rebuild_bvh at the sizes and key values tests/test_rebuild.py does not reach.

Sizes.  The teapot (P = 144 packets) is that file's largest fixture, so every launch there is one
workgroup of 256 and rebuild_seg_kernel (a launch per segment-tree level at and below node 256,
P > 256 only) never ran.  Here: line_tris(n), whose rebuilt tree is all binary nodes (M = P - 1,
past the built tree's node count: the whole tail is in use) at P = 257, 258, 513 and 1025, and
cloud(n, seed), small triangles uniform in a cube (3- and 4-child nodes), at P = 3, 5, 256 (the
last packet one lane, and full), 257, 513 and 1025.

Key cell edges.  `cells`: one triangle spans the root box R, and point triangles sit on, and one
and two floats to either side of, the edges of cells 0, 1, 2, 3, 511 .. 513, 1022 .. 1024 of
each axis, the other two coordinates in the middle of R: t = (c - R.lo) / e * 1024 decides there,
on one axis at a time.  `cells_far`: the same at R.lo = (1000, -2000, 0.5) with extents
(0.37, 3, 1e-3), where c - R.lo loses bits.

The yardstick is test_rebuild.py's rebuild_arrays, imported; integers exactly, floats by value;
frames and ray entries bit for bit against a twin that imports the restated arrays.  The
restatement of a fixture is computed once per process and never written to."""
import functools

import numpy as np
import pytest

from helpers import bits, camera
from test_refit import EMPTY, F32, assert_arrays, import_bvh, prim_verts_of, refit_of
from test_refit_shapes import same_words
from test_rebuild import (assert_counted, assert_tree, cost_of, counted, lambert_scene, line_tris, quant, rebuild_arrays,
                          root_box, soup)

KS = (0, 1, 2, 3, 511, 512, 513, 1022, 1023, 1024)   # the cell edges probed, per axis


# ---------------------------------------------------------------- generators
def cloud(n, seed):
    """n small triangles: centres uniform in [-3, 3]^3, corners within +-0.05 of them."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-3, 3, (n, 1, 3))
    return soup(np.asarray(c + rng.uniform(-0.05, 0.05, (n, 3, 3)), F32))


def cell_probes(rlo, rhi):
    """(triangles (t, corner, xyz), the probes as (axis, k, value) in triangle order from 1).
    Triangle 0 spans [rlo, rhi]; then per axis a and k of KS the float32 nearest
    rlo[a] + e k / 1024 and its two float32 neighbours on each side, clamped into the box, each
    a point triangle with the other two coordinates at the box's middle."""
    rlo, rhi = np.asarray(rlo, F32), np.asarray(rhi, F32)
    lo64, hi64 = rlo.astype(np.float64), rhi.astype(np.float64)
    mid = ((lo64 + hi64) / 2).astype(F32)
    tris = [[rlo, rhi, np.array([rlo[0], rhi[1], rlo[2]], F32)]]
    probes = []
    for a in range(3):
        for k in KS:
            v = F32(lo64[a] + (hi64[a] - lo64[a]) * k / 1024)
            down1 = np.nextafter(v, F32(-np.inf))
            up1 = np.nextafter(v, F32(np.inf))
            five = [np.nextafter(down1, F32(-np.inf)), down1, v, up1, np.nextafter(up1, F32(np.inf))]
            for x in five:
                p = mid.copy()
                p[a] = min(max(F32(x), rlo[a]), rhi[a])
                tris.append([p, p, p])
                probes.append((a, k, p[a]))
    return np.asarray(tris, F32), probes


CELLS = dict(cells=((-1.0, 10.0, -0.3), (2.0, 10.7, 0.9)),
             cells_far=((1000.0, -2000.0, 0.5), tuple(np.array([1000.0, -2000.0, 0.5], F32) + np.array([0.37, 3.0, 1e-3], F32))))


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    """(V, N, F) of a fixture, read-only."""
    kind, _, arg = name.partition("_")
    if name in CELLS:
        m = soup(cell_probes(*CELLS[name])[0])
    elif kind == "line":
        m = line_tris(int(arg))
    else:
        m = cloud(int(arg), seed=int(arg))
    for a in m:
        a.setflags(write=False)
    return m


def build(name):
    """(scene, prim_verts, fixed boxes), as test_rebuild.py's fixtures give them."""
    V, N, F = mesh_of(name)
    return lambert_scene((V, N, F)), prim_verts_of((V, F)), {}


#        name: (P, per-level segment launches)
LINES = {"line_1028": (257, 1), "line_1032": (258, 1), "line_2052": (513, 2), "line_4100": (1025, 3)}
CLOUDS = {"cloud_9": (3, 0), "cloud_17": (5, 0), "cloud_1021": (256, 0), "cloud_1024": (256, 0), "cloud_1025": (257, 1),
          "cloud_2049": (513, 2), "cloud_4097": (1025, 3)}
SIZES = dict(LINES, **CLOUDS)


def seg_launches(P):
    """The per-level launches enqueue() (mrt_rebuild.hip) makes for P packets: one per level of
    the segment tree from node P - 1's up to level 8, the levels under node 256 being one launch
    of one workgroup."""
    k = 0
    while (2 << k) < P:
        k += 1
    return max(0, k - 7)


@functools.lru_cache(maxsize=None)
def restated(name):
    """(export of the build, its node count, rebuild_arrays of it, rebuild_arrays of that), once."""
    P, pv, fixed = build(name)
    ex0 = P.bvh_export()
    want = rebuild_arrays(*ex0, pv, fixed)
    want2 = rebuild_arrays(*want, pv, fixed)
    for a in ex0 + want + want2:
        a.setflags(write=False)
    return ex0, P.bvh_info["nodes"], want, want2


# ---------------------------------------------------------------- cameras
def cams_of(name):
    """Cameras that see more than 20 of the fixture's triangles' pixels each (asserted)."""
    V, _, F = mesh_of(name)
    if name in CELLS:   # the spanning triangle, from in front of its middle
        lo, hi = (np.asarray(x, np.float64) for x in CELLS[name])
        mid, d = (lo + hi) / 2, float(np.max(hi - lo))
        return [dict(eye=tuple(mid + [0, 0, 1.5 * d + (hi[2] - lo[2])]), lookAt=tuple(mid), up=(0, 1, 0), fov=60)]
    if name.startswith("line"):   # a triangle is five pixels wide: the first packets and the last
        last = float(V[:, 0].max())
        return [dict(eye=(x, 0.02, 0.5), lookAt=(x, 0.02, 0), up=(0, 1, 0), fov=60) for x in (0.3, last - 0.3)]
    T = np.asarray(V, np.float64)[F]
    e1, e2 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    t = int(np.argmax(np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])))   # the largest seen along z
    c = T[t].mean(0)
    near = dict(eye=tuple(c + [0, 0, 0.3]), lookAt=tuple(c), up=(0, 1, 0), fov=45)
    if len(F) < 1000:
        return [near]
    return [near, dict(eye=(0.0, 0.0, 9.0), lookAt=(0, 0, 0), up=(0, 1, 0), fov=45)]   # and the whole cube


def rays_of(cam):
    o, d, _ = camera(cam).rays(64, 64)
    return o.reshape(-1, 3).astype(F32), d.reshape(-1, 3).astype(F32)


def seen(P, name):
    """Per camera: the counted 64 x 64 frame, the closest-hit and the any-hit records of its rays."""
    out = []
    for cam in cams_of(name):
        o, d = rays_of(cam)
        out.append((counted(P, cam), P.traceRays(o, d), P.traceBatch(o, d, any_hit=True)))
    return out


def assert_seen(a, b):
    for (fa, ca, aa), (fb, cb, ab) in zip(a, b):
        assert_counted(fa, fb)
        assert (fa["hits"]["prim"] >= 0).sum() > 20, "the camera sees too little"
        assert same_words(ca, cb), "closest hits differ"
        assert same_words(aa, ab), "any-hit records differ"
        assert (ca["prim"] >= 0).sum() > 20


_twins = {}


def twin(name):
    """What a scene that imports the restated arrays shows: uploaded as any build is, its world
    nodes in one range and no tail: (the scene, seen() of it), made once and only read."""
    if name not in _twins:
        B, _, _ = build(name)
        import_bvh(B, restated(name)[2])
        _twins[name] = (B, seen(B, name))
    return _twins[name]


# ---------------------------------------------------------------- CPU tests
def test_cloud_and_probe_generators():
    V, N, F = cloud(17, 3)
    assert V.shape == (51, 3) and F.shape == (17, 3) and V.dtype == F32
    c = V.reshape(17, 3, 3).mean(1)
    assert (np.abs(c) <= 3.05).all() and (np.abs(V.reshape(17, 3, 3) - c[:, None]) <= 0.1).all()
    tris, probes = cell_probes(*CELLS["cells"])
    assert tris.shape == (151, 3, 3) and len(probes) == 150
    assert (tris[1:, 0] == tris[1:, 1]).all() and (tris[1:, 0] == tris[1:, 2]).all()
    assert (tris.reshape(-1, 3).min(0) == tris[0].min(0)).all() and (tris.reshape(-1, 3).max(0) == tris[0].max(0)).all()


@pytest.mark.parametrize("name", list(SIZES) + list(CELLS))
def test_host_rebuild_is_the_restatement(name):
    """The host path on a scene built and not uploaded equals the restatement, is a tree, and a
    second rebuild equals the restatement applied twice; the premise the fixture exists for."""
    ex0, built, want, want2 = restated(name)
    A, pv, fixed = build(name)
    n = A.bvh_info["prims"]
    assert_arrays(A.bvh_export(), ex0)
    assert A.rebuildBVH() == 0.0
    ex1 = A.bvh_export()
    assert_arrays(ex1, want)
    assert A.bvh_info["nodes"] == len(want[1]) and A.bvh_info["leaves"] == len(want[3])
    assert_tree(ex1, n, pv, fixed)
    assert_arrays(refit_of(ex1, pv, fixed), ex1)
    assert A.bvhCost() == pytest.approx(cost_of(want), rel=1e-12)
    assert A.rebuildBVH() == 0.0
    assert_arrays(A.bvh_export(), want2)
    assert_tree(want2, n, pv, fixed)


@pytest.mark.parametrize("name", list(SIZES))
def test_size_premises(name):
    """P, the per-level launches that P reaches, the workgroups of 256 of the per-node launches;
    a line fixture fills the tail: M = P - 1 binary nodes, more than the built tree had."""
    ex0, built, want, _ = restated(name)
    P_want, launches = SIZES[name]
    n = len(mesh_of(name)[2])
    P, M = len(want[3]), len(want[1])
    assert P == P_want == (n + 3) // 4
    assert seg_launches(P) == launches == max(0, (P - 1).bit_length() - 1 - 7)
    used = (want[1] != EMPTY).sum(1)
    if name in LINES:
        assert M == P - 1 > built and (used == 2).all()
        assert -(-M // 256) == {257: 1, 258: 2, 513: 2, 1025: 4}[P] and (P != 257 or M == 256)
    elif P >= 8:   # the 3- and 4-child nodes the line fixtures do not have
        assert M < P - 1 and (used == 3).any() and (used == 4).any()
    if name == "cloud_1021":
        assert (want[3][-1] >= 0).sum() == 1   # the last packet holds one lane
    if name in ("cloud_17", "cloud_1025", "cloud_2049", "cloud_4097"):
        assert P % 2 == 1   # segment-tree nodes that mix a packet and an inner node
    print(f"{name}: n {n}, P {P}, M {M}, built {built}, launches {launches}, tail {'yes' if M > built else 'no'}")


def t_of(c, rlo, rhi):
    """t of the key rule in single precision, before it is truncated and clamped."""
    c, rlo, rhi = F32(c), F32(rlo), F32(rhi)
    return F32(F32(F32(c - rlo) / F32(rhi - rlo)) * F32(1024.0))


@pytest.mark.parametrize("name", list(CELLS))
def test_cell_premises(name):
    """With the numpy quant alone: cells 0 and 1023 occur on every axis, a centre equal to R.hi
    clamps from t = 1024, and on every axis at least five of the ten edges have two adjacent
    floats in different cells.  The root box the library keys with is the anchor's."""
    tris, probes = cell_probes(*CELLS[name])
    rlo, rhi = tris[0].min(0), tris[0].max(0)
    ex0, built, want, _ = restated(name)
    lo, hi = root_box(ex0[0], ex0[1])
    assert np.array_equal(lo, rlo) and np.array_equal(hi, rhi)
    assert len(tris) == 151 and len(want[3]) == 38
    for a in range(3):
        mine = [(k, v) for (b, k, v) in probes if b == a]
        q = [quant(v, v, rlo[a], rhi[a]) for _, v in mine]
        assert 0 in q and 1023 in q
        top = [v for _, v in mine if v == rhi[a]]
        assert top and t_of(top[0], rlo[a], rhi[a]) == 1024.0 and quant(top[0], top[0], rlo[a], rhi[a]) == 1023
        split = 0
        for k in KS:
            qk = [quant(v, v, rlo[a], rhi[a]) for kk, v in mine if kk == k]   # ascending floats
            split += any(x != y for x, y in zip(qk, qk[1:]))
        print(f"{name} axis {a}: {split} of {len(KS)} edges split two adjacent floats; cells {sorted(set(q))}")
        assert split >= 5
    # each axis carries the deciding bit somewhere: probes of one axis differ in that axis' cell alone
    codes = {a: {(quant(v, v, rlo[a], rhi[a])) for (b, _, v) in probes if b == a} for a in range(3)}
    assert all(len(c) >= 8 for c in codes.values())


# ---------------------------------------------------------------- GPU tests
def check_export(A, name, pv, fixed, want):
    ex = A.bvh_export()
    assert_arrays(ex, want)
    assert A.bvh_info["nodes"] == len(want[1]) and A.bvh_info["leaves"] == len(want[3])
    assert_tree(ex, A.bvh_info["prims"], pv, fixed)
    assert A.bvhCost() == pytest.approx(cost_of(want), rel=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SIZES) + list(CELLS))
def test_device_rebuild_is_the_restatement(name):
    """The synchronous form on an uploaded scene: the export, the tree, the cost; the counted
    frame, the closest and the any-hit trace against the twin; a second rebuild."""
    ex0, built, want, want2 = restated(name)
    A, pv, fixed = build(name)
    assert_arrays(A.bvh_export(), ex0)
    counted(A, cams_of(name)[0])   # uploaded
    assert A.rebuildBVH() > 0.0
    check_export(A, name, pv, fixed, want)
    assert_seen(seen(A, name), twin(name)[1])
    assert A.rebuildBVH() > 0.0
    assert_arrays(A.bvh_export(), want2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SIZES) + list(CELLS))
def test_async_rebuild_is_the_restatement(name):
    """The async form as the replica's first rebuild (it allocates, and grows the node array of a
    line fixture) on a torch stream, a frame on that stream, then the read-backs; a second
    rebuild on the stream."""
    import torch
    from test_instance_update import async_frame
    ex0, built, want, want2 = restated(name)
    cam = cams_of(name)[0]
    A, pv, fixed = build(name)
    counted(A, cam)   # uploaded
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert A.rebuildBVH(stream=st) is None
    rgb, rgb8 = async_frame(A, st, 64, 64, cam)
    fb = twin(name)[1][0][0]
    assert np.array_equal(bits(rgb), bits(fb["rgb"])) and np.array_equal(rgb8, fb["rgb8"])
    check_export(A, name, pv, fixed, want)
    assert_seen(seen(A, name), twin(name)[1])
    assert A.rebuildBVH(stream=st) is None
    st.synchronize()
    assert_arrays(A.bvh_export(), want2)
    torch.cuda.synchronize()
