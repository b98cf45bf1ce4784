"""mrt_hit_surfaces (miro.Scene.hitSurfaces): Ray::getPoint + HitInfo::getAllInfos, batched,
against a float32 numpy restatement of the reference's src/Ray.cpp:5-49 written here.

Every operation is a separately rounded IEEE single operation in the reference's order
(numpy float32 arrays round each elementwise operation once); dot products and normalized()
are src/Vector3.h's as DESIGN.md section 2 states them -- dot = (x*x' + y*y') + (z*z' + 0),
normalized = v * rsqrt_nr(dot(v, v)) -- and the reciprocal square root is the oracle's
rsqrt_nr.  Mesh arrays come from mrt_scene_mesh_export / mrt_scene_mesh_texcoords, the
object of a hit id from mrt_scene_prim_object, the tangent frames from the oracle's
mesh_tangents.  Every output is restated bit for bit: none needs the float64 fallback.
Frames are 37 x 29."""
import ctypes as C

import numpy as np
import pytest

import miro
import oracle as O
from helpers import bits, camera, fixture_mesh, scene_pair
from miro import scenes
from test_sample_rays import CAM, H, W

F = np.float32


def need_gpu():
    if miro.device_count() < 1:
        pytest.fail("no HIP device visible (GPU tests must run on the MI355X box)")


# ------------------------------------------------------------------ src/Vector3.h in float32
def rsqrt(x):
    return np.array([O.rsqrt_nr(float(v)) for v in x], F)


def dot(a, b):
    p = a * b
    return (p[:, 0] + p[:, 1]) + (p[:, 2] + F(0))


def normalized(a):
    return a * rsqrt(dot(a, a))[:, None]


def cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def blend(x0, x1, x2, a, b, c):
    """x0 * c + x1 * a + x2 * b, left to right (Vector3 operators; src/Ray.cpp:24,35-40)."""
    if x0.ndim == 2:
        a, b, c = a[:, None], b[:, None], c[:, None]
    return (x0 * c + x1 * a) + x2 * b


def mat3(T, v):
    """operator*(Matrix4x4, Vector3) (src/Matrix4x4.h:693-704): rows 0-2, left to right."""
    return np.stack([(T[r, 0] * v[:, 0] + T[r, 1] * v[:, 1]) + T[r, 2] * v[:, 2] for r in range(3)], axis=1)


def texcoords(P, mesh):
    L = miro.lib()
    n = C.c_int32()
    assert L.mrt_scene_mesh_texcoords(P.handle, mesh, C.byref(n), None, None) == 0
    if n.value == 0:
        return None
    nt = len(P.mesh_arrays(mesh)[2])
    uv, ti = np.zeros((n.value, 2), F), np.zeros((nt, 3), np.uint32)
    assert L.mrt_scene_mesh_texcoords(P.handle, mesh, C.byref(n), uv.ctypes.data_as(C.POINTER(C.c_float)),
                                      ti.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    return uv, ti


def restated_surfaces(P, o, d, hits, inv_t=None, tangents=None):
    """HitInfo::getAllInfos + Ray::getPoint per (ray, hit) pair in float32 numpy.
    inv_t: per instance, m_invTranspose (4 x 4); tangents: per mesh, the oracle's
    (tangents, bitangents) per normal slot."""
    o, d, hits = o.reshape(-1, 3).astype(F), d.reshape(-1, 3).astype(F), hits.reshape(-1)
    out = np.zeros(len(hits), miro.SURFACE_DTYPE)
    for k in ("material", "mesh", "tri", "inst"):
        out[k] = -1
    idx = np.flatnonzero(hits["prim"] >= 0)
    obj = np.array([P.primObject(int(p)) for p in hits["prim"][idx]], np.int32).reshape(-1, 3)
    out["mesh"][idx], out["tri"][idx], out["inst"][idx] = obj[:, 0], obj[:, 1], obj[:, 2]
    out["p"][idx] = o[idx] + hits["t"][idx][:, None] * d[idx]   # Ray::getPoint
    for mesh in np.unique(obj[:, 0]):
        sel = idx[obj[:, 0] == mesh]
        tri, inst = out["tri"][sel], out["inst"][sel]
        V, N, vi, ni = P.mesh_arrays(int(mesh))
        a, b = hits["a"][sel], hits["b"][sel]
        c = F(1.0) - a - b
        v0, v1, v2 = (V[vi[tri, k]] for k in range(3))
        geo = normalized(cross(v1 - v0, v2 - v0))
        n = normalized(blend(*(N[ni[tri, k]] for k in range(3)), a, b, c))
        for i in np.unique(inst[inst >= 0]):   # m_proxy: through the inverse transpose
            m = inst == i
            geo[m] = normalized(mat3(inv_t[i], geo[m]))
            n[m] = normalized(mat3(inv_t[i], n[m]))
        out["geo_n"][sel], out["n"][sel] = geo, n
        tc = texcoords(P, int(mesh))
        if tc is None:
            out["u"][sel], out["v"][sel] = a, b
        else:
            uv, ti = tc
            out["u"][sel] = blend(*(uv[ti[tri, k], 0] for k in range(3)), a, b, c)
            out["v"][sel] = blend(*(uv[ti[tri, k], 1] for k in range(3)), a, b, c)
            tn, bt = tangents[int(mesh)]
            out["tan"][sel] = normalized(blend(*(tn[ni[tri, k]] for k in range(3)), a, b, c))
            out["bitan"][sel] = normalized(blend(*(bt[ni[tri, k]] for k in range(3)), a, b, c))
    return out


def assert_surfaces_equal(got, want):
    got, want = got.reshape(-1), want.reshape(-1)
    for k in ("material", "mesh", "tri", "inst"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("p", "n", "geo_n", "u", "v", "tan", "bitan"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    miss = want["mesh"] < 0
    zero = np.zeros(1, miro.SURFACE_DTYPE)
    for k in ("material", "mesh", "tri", "inst"):
        zero[k] = -1
    assert all(r.tobytes() == zero.tobytes() for r in got[miss])   # all zeros and -1


# ------------------------------------------------------------------ the scenes
@pytest.mark.gpu
def test_cornell_surfaces_match_the_restatement():
    """The Cornell fixture from far enough that some rays miss: no texture coordinates, so
    (u, v) = (a, b) and the tangent frame is zero; miss rows are zeros and -1."""
    need_gpu()
    P, _, _ = scene_pair(dict(scenes.CONFIGS["C1"]), meshes=[fixture_mesh("cornell_box")])
    o, d, t = camera(dict(CAM, eye=(2.75, 2.75, 10.0))).rays(W, H)
    hits = P.traceRays(o, d, t)
    n_hit = (hits["prim"] >= 0).sum()
    assert 100 < n_hit < hits.size - 100
    got = P.hitSurfaces(o, d, hits)
    assert got.shape == (H, W)
    want = restated_surfaces(P, o, d, hits)
    want["material"][want["mesh"] >= 0] = 0   # one material
    assert_surfaces_equal(got, want)
    hit = got["mesh"] >= 0
    assert not np.any(got["tan"]) and not np.any(got["bitan"])
    assert np.array_equal(bits(got["u"][hit]), bits(hits["a"][hit])) and np.array_equal(bits(got["v"][hit]), bits(hits["b"][hit]))
    assert np.allclose(np.linalg.norm(got["n"][hit], axis=-1), 1.0, atol=1e-5)


@pytest.mark.gpu
def test_instance_surfaces_go_through_the_inverse_transpose():
    """A teapot instance under a quarter turn about y and the scales (1, 1/2, 2), over a world
    floor.  Every entry of the transform, its inverse and the inverse transpose is 0 or a
    signed power of two (checked below), so the float64 inverse taken here, rounded to float,
    is ProxyMatrix's m_invTranspose whatever route its inversion takes.  A normal that skipped
    the inverse transpose, or took the transform itself, is wrong by the scales."""
    need_gpu()
    from test_instancing import instanced_pair
    M = np.array([[0, 0, 2, 0.5], [0, 0.5, 0, 1.0], [-1, 0, 0, -0.25], [0, 0, 0, 1]], F)   # Ry(90) * S(1, .5, 2) + t
    inv = np.linalg.inv(M.astype(np.float64))
    assert np.array_equal(inv.astype(F).astype(np.float64), inv) and np.array_equal(inv @ M.astype(np.float64), np.eye(4))
    inv_t = inv.T.astype(F)
    P, _ = instanced_pair("blinn", transforms=[M], spec=(8.0, 0.3))
    cam = dict(eye=(0.0, 3.0, 9.0), lookAt=(0.5, 1.0, 0.0), up=(0, 1, 0), fov=45.0)
    o, d, t = camera(cam).rays(W, H)
    hits = P.traceRays(o, d, t)
    on_inst = hits["inst"] >= 0
    assert on_inst.sum() > 50 and ((hits["prim"] >= 0) & ~on_inst).sum() > 20   # the teapot and the floor
    got = P.hitSurfaces(o, d, hits)
    want = restated_surfaces(P, o, d, hits, inv_t={0: inv_t})
    # material ids in the order miro.Scene.preCalc meets them: the floor's, then the teapot's
    want["material"][(want["mesh"] >= 0) & (want["inst"] < 0)] = 0
    want["material"][want["inst"] >= 0] = 1
    assert_surfaces_equal(got, want)
    assert np.array_equal(got["inst"][on_inst], np.zeros(on_inst.sum(), np.int32))
    # the transform matters: object-space normals differ from the world-space ones
    plain = restated_surfaces(P, o, d, hits, inv_t={0: np.eye(4, dtype=F)})
    assert not np.array_equal(bits(plain["n"].reshape(H, W, 3)[on_inst]), bits(got["n"][on_inst]))


def textured_quad():
    """Two triangles with four different normals and texture coordinates outside [0, 1]."""
    v = np.array([[0.5, 0.5, -1.0], [5.0, 0.5, -1.5], [5.0, 5.0, -1.0], [0.5, 5.0, -2.0]], F)
    n = np.array([[0.1, 0.0, 1.0], [-0.2, 0.1, 0.9], [0.0, -0.3, 1.1], [0.2, 0.2, 0.8]], F)
    idx = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    uv = np.array([[0.1, 0.2], [1.3, 0.1], [1.2, 0.9], [-0.2, 1.1]], F)
    return v, n, idx, idx.copy(), uv, idx.copy()


@pytest.mark.gpu
def test_texture_coordinates_and_tangent_frame_match_the_oracle():
    """A quad with vt in front of the Cornell box (which has none): (u, v) interpolate the
    texture coordinates and tan / bitan the oracle's mesh_tangents over the normal indices --
    with no normal map bound, as getAllInfos computes them whenever the mesh has texture
    coordinates; the box's hits in the same batch keep (u, v) = (a, b) and a zero frame."""
    need_gpu()
    P, Osc, _ = scene_pair(dict(scenes.CONFIGS["C1"]), meshes=[fixture_mesh("cornell_box")],
                           extra=[(textured_quad(), dict(kind="lambert", kd=(0.3, 0.6, 0.8)))])
    o, d, t = camera(CAM).rays(W, H)
    hits = P.traceRays(o, d, t)
    got = P.hitSurfaces(o, d, hits)
    tangents = {1: Osc.tangents(1)}
    assert tangents[1] is not None and Osc.tangents(0) is None
    want = restated_surfaces(P, o, d, hits, tangents=tangents)
    want["material"][want["mesh"] >= 0] = want["mesh"][want["mesh"] >= 0]   # mesh k was added with material k
    assert_surfaces_equal(got, want)
    quad, box = got["mesh"] == 1, got["mesh"] == 0
    assert quad.sum() > 100 and box.sum() > 100
    assert np.all(np.abs(np.linalg.norm(got["tan"][quad], axis=-1) - 1) < 1e-5) and not np.any(got["tan"][box])
    assert got["u"][quad].min() < 0 and got["u"][quad].max() > 1   # the coordinates are not wrapped here
    assert not np.array_equal(bits(got["u"][quad]), bits(hits["a"][quad]))
