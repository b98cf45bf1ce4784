"""Who owns a replica's device memory: every allocation, pinned buffer, event and stream of a
scene's replica, its stream contexts and the entries' staging copies is made and freed by one
owner type (DevOwner, csrc/mrt_device.h), counted by mrt_debug_live_resources.  One scene
reaches every allocation path at its smallest; after mrt_scene_destroy the count is back
where it was, cycle after cycle, and the frames of the cycles are equal bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import miro
from miro import _lib
from helpers import bits, camera, fixture_mesh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAM = dict(eye=(0.0, 3.0, 9.0), lookAt=(0.0, 1.0, 0.0), up=(0, 1, 0), fov=50.0)
TEAPOT, QUAD, BALL, BLAS = 0, 1, 2, 3   # mesh ids, in add order
F32 = np.float32


def tri_mesh(V, N, vidx, nidx):
    tm = miro.TriangleMesh()
    tm.setArrays(V, N, vidx, nidx)
    return tm


def moved(x, y=0.0, z=0.0):
    M = np.eye(4, dtype=F32)
    M[:3, 3] = (x, y, z)
    return M


def build_scene():
    """The teapot as a world mesh, a texture-mapped quad with an alpha map, the cannonball
    motion-blur pair, one BLAS (the Cornell box, scaled down) with two instances; a point, a
    rectangle and a dome light; a reflective Blinn material (chain shading)."""
    P = miro.Scene()
    tv, tn, tvi, tni = fixture_mesh("teapot")
    mirror = miro.Blinn(kd=(0.6, 0.5, 0.4), ks=(1, 1, 1))
    mirror.setReflectAmt(0.4)
    miro.makeMeshObjs(P, tri_mesh(tv, tn, tvi, tni), mirror)
    quad = tri_mesh(np.array([(-3, 0, -3), (3, 0, -3), (3, 4, -3), (-3, 4, -3)], F32), np.array([(0, 0, 1)], F32),
                    np.array([(0, 1, 2), (0, 2, 3)], np.uint32), np.zeros((2, 3), np.uint32))
    quad.setTexCoords(np.array([(0, 0), (1, 0), (1, 1), (0, 1)], F32), np.array([(0, 1, 2), (0, 2, 3)], np.uint32))
    rng = np.random.default_rng(11)
    mapped = miro.Lambert((0.8, 0.8, 0.8))
    mapped.setColorMap(miro.Texture(miro.RawImage(8, 8, rng.uniform(0, 1, (8, 8, 3)), miro.TEX_RGB)))
    mapped.setAlphaMap(miro.Texture(miro.RawImage(8, 8, (rng.uniform(0, 1, (8, 8, 1)) > 0.3), miro.TEX_GRAY)))
    miro.makeMeshObjs(P, quad, mapped)
    f = np.load(os.path.join(GOLDEN, "cannonball_mb.npz"))
    ball = (f["verts"] + np.array([2.0, 1.0, 1.0], F32), f["normals"], f["vidx"], f["nidx"])
    miro.makeMBMeshObjs(P, tri_mesh(*ball), tri_mesh(ball[0] + np.array([0.3, 0.0, 0.0], F32), *ball[1:]),
                        miro.Lambert((0.3, 0.3, 0.35)))
    cv, cn, cvi, cni = fixture_mesh("cornell_box")
    cv = np.asarray(cv * F32(0.125), F32)
    objs, bvh = miro.Objects(), miro.BVH()
    miro.ProxyObject.setupProxy(tri_mesh(cv, cn, cvi, cni), miro.Lambert((0.3, 0.8, 0.4)), objs, bvh)
    for x in (-3.0, 3.0):
        P.addObject(miro.ProxyObject(objs, bvh, miro.Matrix4x4(moved(x, 0.0, 1.0))))
    pl = miro.PointLight()
    pl.setPosition((5, 12, 8)); pl.setPower(500)
    P.addLight(pl)
    rl = miro.RectangleLight()
    rl.setVertices((-1, 8, -1), (1, 8, -1), (-1, 8, 1)); rl.setPower(200); rl.setSamples(2)
    P.addLight(rl)
    hdr = miro.RawImage()
    hdr.loadHDR(os.path.join(GOLDEN, "Arches_E_PineTree_Env.hdr"))
    dl = miro.DomeLight()
    dl.setTexture(miro.Texture(hdr)); dl.setSamples(2)
    P.addLight(dl)
    P.setBGColor((0.1, 0.1, 0.3))
    P.preCalc()
    return P, dict(teapot=(tv, tn), ball=ball, box=cv)


def render(P, W, H, **kw):
    img = miro.Image()
    img.resize(W, H)
    P.raytraceImage(camera(CAM), img, **kw)
    return img.rgb.copy()


def cycle():
    """One scene through every entry that allocates; returns (live count while it lives, the
    48 x 48 null-stream frame)."""
    import torch
    L = miro.lib()
    P, m = build_scene()
    first = render(P, 48, 48)
    st = torch.cuda.Stream()   # a second stream: a second context
    rgb = torch.empty(48 * 48 * 3, dtype=torch.float32, device="cuda")
    rgb8 = torch.empty(48 * 48 * 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    opts = _lib.mrt_render_opts(48, 48, 0, 0, 1, 0, 0)
    cc = camera(CAM)._c()
    _lib.check(L.mrt_render_frame_async(P.handle, C.byref(cc), C.byref(opts), rgb.data_ptr(), rgb8.data_ptr(), st.cuda_stream),
               "render_frame_async")
    st.synchronize()
    assert np.array_equal(bits(rgb.cpu().numpy().reshape(48, 48, 3)), bits(first))
    shared = render(P, 48, 48, devices=[0, 0])   # share and gather buffers
    assert np.array_equal(bits(shared), bits(first))
    _lib.check(L.mrt_scene_set_subdivs(P.handle, 1, 2, 0.01), "subdivs")   # the adaptive scratch
    render(P, 48, 48)
    _lib.check(L.mrt_scene_set_subdivs(P.handle, 1, 1, 0.01), "subdivs")
    rng = np.random.default_rng(5)
    o = np.tile(np.array(CAM["eye"], F32), (65, 1))
    d = np.asarray(np.array([0.0, -0.2, -1.0]) + rng.uniform(-0.3, 0.3, (65, 3)), F32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    P.sampleRays(o, d)
    hits = P.traceRays(o, d)
    P.shadeHits(o, d, hits)
    P.hitSurfaces(o, d, hits)
    tv, tn = m["teapot"]
    P.updateMesh(TEAPOT, np.asarray(tv * F32(1.0625), F32), tn)
    P.deformMesh(BLAS, np.asarray(m["box"] * F32(1.125), F32))
    bv = m["ball"][0]
    P.deformMesh(BALL, np.asarray(bv + F32(0.125), F32), verts2=np.asarray(bv + F32(0.375), F32))
    P.updateInstances(np.stack([moved(-3.5, 0.0, 1.0), moved(3.5, 0.5, 1.0)]))
    render(P, 80, 80)   # every grown buffer grows once more
    live = L.mrt_debug_live_resources()
    L.mrt_scene_destroy(P._h)
    P._h = None
    return live, first


@pytest.mark.gpu
def test_destroy_returns_every_resource_over_three_cycles():
    import torch
    if miro.device_count() < 1:
        pytest.skip("no HIP device")
    L = miro.lib()
    torch.cuda.synchronize()
    frames, free = [], []
    for k in range(3):
        before = L.mrt_debug_live_resources()
        live, first = cycle()
        after = L.mrt_debug_live_resources()
        free.append(torch.cuda.mem_get_info()[0])
        print("cycle %d: live before %d, with the scene %d, after destroy %d; device memory free %d" % (
            k, before, live, after, free[-1]))
        assert after == before, "cycle %d: %d resources before create, %d after destroy" % (k, before, after)
        assert live - before > 40, "cycle %d: only %d resources counted while the scene lived" % (k, live - before)
        frames.append(first)
    assert np.array_equal(bits(frames[0]), bits(frames[1])) and np.array_equal(bits(frames[0]), bits(frames[2]))
