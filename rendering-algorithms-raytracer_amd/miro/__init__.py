"""miro -- host-side mirror of the reference's scene API over libmrt.so.

Names, argument meaning and call order follow the reference scene scripts
(reference src/assignment2.h, src/Scene.h, src/Camera.h, src/Light.h):

    scene = Scene(); cam = Camera(); img = Image(); img.resize(512, 512)
    scene.setBGColor(Vector3(0, 0, 0.2))
    cam.setEye(Vector3(8, 1.5, 1)); cam.setLookAt(Vector3(0, 2.5, -1))
    cam.setUp(Vector3(0, 1, 0)); cam.setFOV(55)
    light = PointLight(); light.setPosition(Vector3(0, 10, 0)); light.setPower(200)
    scene.addLight(light)
    mesh = TriangleMesh(); mesh.load("sponza.obj"); makeMeshObjs(scene, mesh, Blinn(Vector3(1)))
    scene.preCalc()                    # BVH::build
    scene.raytraceImage(cam, img)      # 1 spp primary + shadow rays on the GPU

Everything that computes runs in libmrt.so (HIP kernels for gfx950); this
module only marshals data.  Missing library -> MRTError, no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import time
from typing import List, Optional

import numpy as np

from . import _lib
from ._lib import MRTError, check, f3

__all__ = ["Vector3", "Matrix4x4", "TriangleMesh", "Lambert", "Blinn", "PointLight", "RectangleLight",
           "DomeLight", "RawImage", "Texture", "Objects", "BVH", "ProxyObject",
           "Camera", "Image", "Scene", "Ray", "HitInfo", "makeMeshObjs", "MRTError", "lib", "device_count",
           "rcp_nr", "rsqrt_nr"]

lib = _lib.load


def device_count() -> int:
    return int(lib().mrt_device_count())


def rcp_nr(x: float) -> float:
    return float(lib().mrt_rcp_nr(float(x)))


def rsqrt_nr(x: float) -> float:
    return float(lib().mrt_rsqrt_nr(float(x)))


def debug_libm(fn: str, x, y=None):
    """The device's acosf(x) ("acos") / atan2f(y, x) ("atan2") / sinf(x) ("sin") / cosf(x)
    ("cos") / powf(x, y) ("pow") / rcp_nr(x) ("rcp_nr") (numerics probe)."""
    import numpy as np
    x = np.ascontiguousarray(x, np.float32)
    y = np.ascontiguousarray(np.zeros_like(x) if y is None else y, np.float32)
    out = np.empty_like(x)
    _lib.check(lib().mrt_debug_libm({"acos": 0, "atan2": 1, "rcp_nr": 2, "sin": 3, "cos": 4, "pow": 5}[fn], x.ctypes.data, y.ctypes.data, len(x),
                                    out.ctypes.data), "mrt_debug_libm")
    return out


def bin_rays(o, d, *, n_dev=None, mul1=1, sub=0, cap1=0xFFFFFFFF, mul2=1, nrays=None, m=1, lo=(0, 0, 0), inv=(1, 1, 1),
             dbits=2, obits=2, grid=1, hits=None, hit_base=None, inst_class=None, n_world=0, inst_cell=None,
             inst_inv=None, keys_fill=0xABCD, perm_fill=0xDEADBEEF):
    """The ray-binning launches (csrc/mrt_bin.hip) on host arrays (mrt_debug_bin_rays, include/mrt.h):
    o, d (n, 4) floats; the count, validity, key and instance-table fields as the C entry takes them.
    Returns {"keys": (n,) uint16, "hist": (2^bits + 1,) uint32, "perm": (n,) uint32, "bits"}; keys and
    perm enter the launches filled with keys_fill / perm_fill, so words left alone keep them."""
    o = np.ascontiguousarray(o, np.float32).reshape(-1, 4)
    d = np.ascontiguousarray(d, np.float32).reshape(-1, 4)
    n = len(o)
    assert len(d) == n
    keep = [o, d]   # the arrays the probe points into

    def arr(a, dtype, count=None):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype).reshape(-1)
        assert count is None or m < 1 or a.size == count, (a.size, count)   # (m < 1: the entry refuses it)
        keep.append(a)
        return a.ctypes.data

    px = (n + m - 1) // m if m >= 1 else 0
    n_inst = 0 if hit_base is None else int(np.size(hit_base))
    P = _lib.mrt_bin_probe()
    P.o, P.d, P.n = o.ctypes.data, d.ctypes.data, n
    P.has_n_dev, P.n_dev = int(n_dev is not None), int(n_dev or 0)
    P.mul1, P.sub, P.cap1, P.mul2 = int(mul1), int(sub), int(cap1), int(mul2)
    P.nrays, P.m = arr(nrays, np.uint8, px), int(m)
    P.lo, P.inv = f3(lo), f3(inv)
    P.dbits, P.obits, P.grid = int(dbits), int(obits), int(grid)
    P.hits = arr(hits, np.float32, 4 * px)
    P.hit_base, P.inst_class = arr(hit_base, np.int32), arr(inst_class, np.uint16, n_inst if hit_base is not None else None)
    P.n_inst, P.n_world = n_inst, int(n_world)
    P.inst_cell, P.inst_inv = arr(inst_cell, np.float32, 8 * n_inst), arr(inst_inv, np.float32, 12 * n_inst)
    keys = np.full(max(n, 1), keys_fill, np.uint16)
    perm = np.full(max(n, 1), perm_fill, np.uint32)
    hist = np.full(4097, 0xFFFFFFFF, np.uint32)
    P.keys, P.hist, P.perm = keys.ctypes.data, hist.ctypes.data, perm.ctypes.data
    check(lib().mrt_debug_bin_rays(C.byref(P)), "mrt_debug_bin_rays")
    bits = 12 if hits is not None else 2 * int(dbits) + 3 * int(obits)
    return {"keys": keys[:n], "hist": hist[:(1 << bits) + 1], "perm": perm[:n], "bits": bits}


class Vector3(tuple):
    """Plain 3-tuple with the reference's constructors: Vector3(s) or Vector3(x, y, z)."""

    def __new__(cls, *a):
        if len(a) == 1 and np.ndim(a[0]) == 0:
            a = (a[0], a[0], a[0])
        elif len(a) == 1:
            a = tuple(a[0])
        if len(a) != 3:
            raise ValueError("Vector3 needs 1 or 3 components")
        return super().__new__(cls, (float(a[0]), float(a[1]), float(a[2])))

    x = property(lambda s: s[0])
    y = property(lambda s: s[1])
    z = property(lambda s: s[2])


class Matrix4x4:
    """Row-major 4x4 (m11..m44), src/Matrix4x4.h.  Only used as a load-time ctm."""

    def __init__(self, m=None):
        self.m = np.eye(4, dtype=np.float32) if m is None else np.asarray(m, np.float32).reshape(4, 4).copy()

    def setIdentity(self):
        self.m = np.eye(4, dtype=np.float32)

    def translate(self, x, y, z):  # setColumn4(Vector4(x,y,z,0) + column4), src/Matrix4x4.h:751-754
        self.m[0, 3] = np.float32(x) + self.m[0, 3]
        self.m[1, 3] = np.float32(y) + self.m[1, 3]
        self.m[2, 3] = np.float32(z) + self.m[2, 3]

    def scale(self, x, y, z):  # src/Matrix4x4.h:757-762
        self.m[0, 0] *= np.float32(x)
        self.m[1, 1] *= np.float32(y)
        self.m[2, 2] *= np.float32(z)


class TriangleMesh:
    """TriangleMesh (src/TriangleMesh.h).  load() keeps the path; the OBJ is parsed
    by libmrt's loader (src/TriangleMeshLoad.cpp semantics) at Scene.preCalc()."""

    def __init__(self):
        self.path: Optional[str] = None
        self.ctm: Optional[np.ndarray] = None
        self.verts = self.normals = self.vidx = self.nidx = None

    def load(self, file, ctm: Optional[Matrix4x4] = None) -> bool:
        self.path = str(file)
        self.ctm = None if ctm is None else np.ascontiguousarray(ctm.m, np.float32)
        return True

    def createSingleTriangle(self):  # src/TriangleMesh.cpp:11-42
        self.verts = np.zeros((3, 3), np.float32)
        self.normals = np.zeros((3, 3), np.float32)
        self.vidx = np.array([[0, 1, 2]], np.uint32)
        self.nidx = np.array([[0, 1, 2]], np.uint32)

    def setArrays(self, verts, normals, vidx, nidx):
        self.verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        self.normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        self.vidx = np.ascontiguousarray(vidx, np.uint32).reshape(-1, 3)
        self.nidx = np.ascontiguousarray(nidx, np.uint32).reshape(-1, 3)

    def setTexCoords(self, uv, tidx):
        """m_texCoords ((u, v) per texture coordinate) / m_texCoordIndices (3 per triangle)."""
        self.uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        self.tidx = np.ascontiguousarray(tidx, np.uint32).reshape(-1, 3)

    uv = tidx = None

    def setV1(self, v): self.verts[0] = v
    def setV2(self, v): self.verts[1] = v
    def setV3(self, v): self.verts[2] = v
    def setN1(self, n): self.normals[0] = n
    def setN2(self, n): self.normals[1] = n
    def setN3(self, n): self.normals[2] = n


class _Maps:
    """Material::setColorMap / setAlphaMap / setNormalMap / setSpecularMap /
    setReflectMap / setRefractMap (src/Material.h:20-25): Texture objects."""
    colorMap = normalMap = specularMap = reflectMap = refractMap = alphaMap = None

    def setColorMap(self, t): self.colorMap = t
    def setNormalMap(self, t): self.normalMap = t
    def setSpecularMap(self, t): self.specularMap = t
    def setReflectMap(self, t): self.reflectMap = t
    def setRefractMap(self, t): self.refractMap = t
    def setAlphaMap(self, t): self.alphaMap = t

    def _maps(self):
        return (self.colorMap, self.normalMap, self.specularMap, self.reflectMap, self.refractMap, self.alphaMap)

    # Material::setEnvMap / m_envExposure (src/Material.h:19,41-42): the map a missed
    # reflection / refraction / GI ray of a Blinn material takes (getEnvironmentColor,
    # src/Material.cpp:44-64); None = the scene's
    envMap = None
    envExposure = 1.0

    def setEnvMap(self, t): self.envMap = t
    def setEnvExposure(self, x): self.envExposure = float(x)


class Lambert(_Maps):
    """Lambert(kd = Vector3(1), ka = Vector3(0)), src/Lambert.h:11-13."""

    def __init__(self, kd=Vector3(1), ka=Vector3(0)):
        self.kd, self.ka = Vector3(kd), Vector3(ka)

    def setKd(self, kd): self.kd = Vector3(kd)
    def setKa(self, ka): self.ka = Vector3(ka)

    def setSampleEnv(self, b): self.sampleEnv = bool(b)          # Material::setSampleEnv (src/Material.h:27)

    sampleEnv = True

    def _c(self):
        return _lib.mrt_material(0, f3(self.kd), f3(self.ka), f3((1, 1, 1)), 1.0, 0.0, f3((0, 0, 0)), 0.0)


class Blinn(_Maps):
    """Blinn(kd, ka, ks, kt, ior, specExp, specAmt, reflectAmt, refractAmt) defaults of
    src/Blinn.h:11-22: direct lighting plus Fresnel-weighted reflection / refraction
    rays (src/Blinn.cpp:91-335), glossy reflection vectors, translucency, emission
    (setLightEmittedIntensity / setLightEmittedColor), path tracing (Scene.setPathTrace)
    texture maps (colour, normal, specular, reflect, refract, alpha) and dispersion
    (m_disperse with m_ior[0..2]: one refraction ray per colour channel).  As in the
    reference, setIor(ior, i) sets m_ior[i] and the non-dispersive refraction reads
    m_ior[1] (src/Blinn.cpp:183), so setIor(x) alone changes only dispersion."""

    def __init__(self, kd=Vector3(1), ka=Vector3(0), ks=Vector3(1), kt=Vector3(0), ior=1.5,
                 specExp=1.0, specAmt=0.0, reflectAmt=0.0, refractAmt=0.0, specGloss=1.0):
        self.kd, self.ka, self.ks, self.kt = Vector3(kd), Vector3(ka), Vector3(ks), Vector3(kt)
        self.m_ior = [float(ior)] * 3      # src/Blinn.cpp:25-27
        self.m_disperse = False            # Material::m_disperse (src/Material.cpp:6)
        self.specExp, self.specAmt = float(specExp), float(specAmt)
        self.reflectAmt, self.refractAmt = float(reflectAmt), float(refractAmt)
        self.specGloss = float(specGloss)
        self.translucency = 0.0
        self.lightEmitted = 0.0          # the Blinn ctor forces 0 (src/Blinn.cpp:28-29)
        self.Le = Vector3(0)
        self.sampleEnv = True            # Material::m_sampleEnv (src/Material.cpp:6)

    def setLightEmittedIntensity(self, le): self.lightEmitted = float(le)   # src/Blinn.h:44
    def setLightEmittedColor(self, c): self.Le = Vector3(c)                 # src/Blinn.h:45
    def setSampleEnv(self, b): self.sampleEnv = bool(b)                     # src/Material.h:27

    def setTranslucency(self, t): self.translucency = float(t)   # src/Material.h:30

    def setReflectGloss(self, g): self.specGloss = float(g)    # src/Blinn.h:42

    def setReflectAmt(self, a): self.reflectAmt = float(a)     # src/Blinn.h:41
    def setRefractAmt(self, a): self.refractAmt = float(a)     # src/Material.h:32
    def setIor(self, ior, i=0):                                # src/Blinn.h:38
        self.m_ior[i] = float(ior)

    @property
    def ior(self):                                             # the refraction IOR: m_ior[1] (src/Blinn.cpp:183)
        return self.m_ior[1]

    def setKd(self, v): self.kd = Vector3(v)
    def setKa(self, v): self.ka = Vector3(v)
    def setKs(self, v): self.ks = Vector3(v)
    def setSpecExp(self, e): self.specExp = float(e)
    def setSpecAmt(self, a): self.specAmt = float(a)

    def _c(self):
        return _lib.mrt_material(1, f3(self.kd), f3(self.ka), f3(self.ks), self.specExp, self.specAmt, f3(self.Le),
                                 self.lightEmitted)


class _Light:
    def __init__(self):  # Light::Light, src/Light.h:15-19
        self.color = Vector3(0)
        self.power = 0.0
        self.samples = 1
        self.castShadows = True
        self.fastShadows = True           # src/Light.h:16; False: a point light casts no shadow (its walk never traces), rect / dome lights walk through refractive hits
        self.noiseThreshold = 0.001

    def setColor(self, c): self.color = Vector3(c)
    def setPower(self, p): self.power = float(p)
    def setSamples(self, n): self.samples = int(n)
    def setCastShadows(self, c): self.castShadows = bool(c)
    def setFastShadows(self, c): self.fastShadows = bool(c)
    def setNoiseThreshold(self, t): self.noiseThreshold = float(t)


class PointLight(_Light):
    def __init__(self):
        super().__init__()
        self.position = Vector3(0)

    def setPosition(self, v): self.position = Vector3(v)

    def _c(self, texture=-1):
        return _lib.mrt_light(0, f3(self.position), f3((0, 0, 0)), f3((0, 0, 0)), f3((0, 0, 0)), self.power,
                              self.samples, self.noiseThreshold, int(self.castShadows), -1, int(not self.fastShadows))


class RectangleLight(_Light):
    def __init__(self):
        super().__init__()
        self.v1 = self.v2 = self.v3 = Vector3(0)

    def setVertices(self, v1, v2, v3):
        self.v1, self.v2, self.v3 = Vector3(v1), Vector3(v2), Vector3(v3)

    def _c(self, texture=-1):
        return _lib.mrt_light(1, f3((0, 0, 0)), f3(self.v1), f3(self.v2), f3(self.v3), self.power,
                              self.samples, self.noiseThreshold, int(self.castShadows), -1, int(not self.fastShadows))


TEX_HDR, TEX_GRAY, TEX_RGB, TEX_RGBA = 0, 1, 3, 4   # RawImage ImageType (floats per texel 3, 1, 3, 4)
_CHANNELS = {TEX_HDR: 3, TEX_GRAY: 1, TEX_RGB: 3, TEX_RGBA: 4}


class RawImage:
    """RawImage (src/RawImage.h:9-30): float texels in m_rawData order (row 0 =
    the top row for .hdr; TGA rows flipped as loadTGA does).  RawImage(w, h, data,
    type) wraps an array; loadImage decodes .tga / .ppm / .hdr in libmrt."""

    def __init__(self, w=0, h=0, data=None, imageType=TEX_HDR):
        self.m_width, self.m_height, self.m_imageType = int(w), int(h), int(imageType)
        self.m_rawData = None if data is None else np.ascontiguousarray(data, np.float32).reshape(
            self.m_height, self.m_width, _CHANNELS[self.m_imageType])

    def loadImage(self, filename):  # src/RawImage.cpp:16-26 (by extension)
        ext = str(filename).rsplit(".", 1)[-1]
        if ext in ("hdr", "HDR"):
            return self.loadHDR(filename)
        L = lib()
        w, h, t = C.c_int32(), C.c_int32(), C.c_int32()
        check(L.mrt_image_info(str(filename).encode(), C.byref(w), C.byref(h), C.byref(t)), f"image {filename}")
        data = np.zeros((h.value, w.value, _CHANNELS[t.value]), np.float32)
        check(L.mrt_image_load(str(filename).encode(), data.ctypes.data_as(C.POINTER(C.c_float)), w.value, h.value),
              f"image {filename}")
        self.m_width, self.m_height, self.m_imageType, self.m_rawData = w.value, h.value, t.value, data
        return True

    def loadHDR(self, filename):  # src/RawImage.cpp:29-32 -> HDRLoader::load
        L = lib()
        w, h = C.c_int32(), C.c_int32()
        check(L.mrt_hdr_info(str(filename).encode(), C.byref(w), C.byref(h)), f"HDR {filename}")
        data = np.zeros((h.value, w.value, 3), np.float32)
        check(L.mrt_hdr_load(str(filename).encode(), data.ctypes.data_as(C.POINTER(C.c_float)), w.value, h.value),
              f"HDR {filename}")
        self.m_width, self.m_height, self.m_rawData = w.value, h.value, data
        return True


class Texture:
    """Texture(RawImage) (src/Texture.h:9-28): a material map, or a lat-long map
    for DomeLight and Scene.setEnvMap."""

    def __init__(self, image: RawImage):
        self.m_image = image

    def getWidth(self): return self.m_image.m_width
    def getHeight(self): return self.m_image.m_height


class DomeLight(_Light):
    """DomeLight (src/DomeLight.h:44-62): setTexture, setPower (= m_Gain, default
    1), setSamples, setNoiseThreshold.  Importance-sampled from the texture."""

    def __init__(self):
        super().__init__()
        self.power = 1.0
        self.texture = None

    def setTexture(self, t): self.texture = t

    def _c(self, texture=-1):
        return _lib.mrt_light(2, f3((0, 0, 0)), f3((0, 0, 0)), f3((0, 0, 0)), f3((0, 0, 0)), self.power,
                              self.samples, self.noiseThreshold, int(self.castShadows), int(texture),
                              int(not self.fastShadows))


class Camera:
    """Camera setters of src/Camera.h:26-45 (fov in degrees, like setFOV), with the
    lens of eyeRayAdaptive: setAperture / setFocusPlane (depth of field,
    src/Camera.cpp:153-174) and setShutterSpeed (getTimeSample, src/Camera.h:44-46)."""

    def __init__(self):
        self.eye, self.lookAt, self.up, self.fov = Vector3(0), Vector3(0, 0, -1), Vector3(0, 1, 0), 45.0
        self.aperture, self.focusPlane, self.shutterSpeed = 0.0, 1.0, 0.001   # src/Camera.cpp:21-23

    def setEye(self, v): self.eye = Vector3(v)
    def setLookAt(self, v): self.lookAt = Vector3(v)
    def setUp(self, v): self.up = Vector3(v)
    def setFOV(self, f): self.fov = float(f)
    def setAperture(self, a): self.aperture = float(a)
    def setFocusPlane(self, f): self.focusPlane = float(f)
    def setShutterSpeed(self, s): self.shutterSpeed = float(s)

    def _c(self):
        return _lib.mrt_camera(f3(self.eye), f3(self.lookAt), f3(self.up), self.fov, self.aperture, self.focusPlane,
                               self.shutterSpeed)

    def rays(self, width, height, seed=0):
        """Camera::eyeRayAdaptive(x, y, .5, .5, .5, .5) of every pixel (mrt_camera_rays, on the
        host): (o, d, time) of shapes (H, W, 3), (H, W, 3), (H, W) -- the rays raytraceImage
        traces for a width x height frame with this seed (Scene.sampleRays shades them)."""
        W, H = int(width), int(height)
        if W <= 0 or H <= 0:
            raise MRTError("Camera.rays: the frame size must be positive")
        o, d = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
        t = np.zeros((H, W), np.float32)
        c = self._c()
        check(lib().mrt_camera_rays(C.byref(c), W, H, int(seed), o.ctypes.data, d.ctypes.data, t.ctypes.data),
              "camera_rays")
        return o, d, t


class Image:
    """Image (src/Image.h): 8-bit RGB, row 0 = bottom, plus the float RGB frame
    before Image::Map (`rgb`) for parity checks."""

    def __init__(self):
        self.resize(1, 1)

    def resize(self, w, h):
        self.m_width, self.m_height = int(w), int(h)
        self.rgb = np.zeros((self.m_height, self.m_width, 3), np.float32)
        self.pixels = np.zeros((self.m_height, self.m_width, 3), np.uint8)

    def width(self): return self.m_width
    def height(self): return self.m_height

    def writePPM(self, path):  # src/Image.cpp:137-154 (rows flipped)
        with open(path, "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (self.m_width, self.m_height))
            f.write(np.ascontiguousarray(self.pixels[::-1]).tobytes())


class Ray:
    def __init__(self, o, d):
        self.o, self.d = Vector3(o), Vector3(d)


class HitInfo:
    """HitInfo (src/Ray.h:185-200); obj is the global triangle id (-1 = none)."""

    def __init__(self, t=1e12, a=0.0, b=0.0, obj=-1):
        self.t, self.a, self.b, self.obj = float(t), float(a), float(b), int(obj)


HIT_DTYPE = np.dtype([("t", "<f4"), ("a", "<f4"), ("b", "<f4"), ("prim", "<i4"), ("inst", "<i4")])
# mrt_surface (Scene.hitSurfaces): Ray::getPoint + HitInfo::getAllInfos of a hit
SURFACE_DTYPE = np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("geo_n", "<f4", 3), ("tan", "<f4", 3), ("bitan", "<f4", 3),
                          ("u", "<f4"), ("v", "<f4"), ("material", "<i4"), ("mesh", "<i4"), ("tri", "<i4"),
                          ("inst", "<i4")])
# mrt_light_sample (Scene.lightSamples): one sample a light took at a point
LIGHT_SAMPLE_DTYPE = np.dtype([("dir", "<f4", 3), ("dist", "<f4"), ("e", "<f4", 3), ("vis", "<f4")])


def makeMeshObjs(scene: "Scene", mesh: TriangleMesh, material):
    """One Object per triangle, in mesh order (the reference's missing helper)."""
    scene.addMesh(mesh, material)


def _mesh_vertices(mesh: TriangleMesh) -> np.ndarray:
    """The vertices of a TriangleMesh: its arrays, or its OBJ parsed by libmrt's
    loader (through a scratch scene)."""
    if mesh.path is None:
        return mesh.verts
    L = lib()
    h = L.mrt_scene_create()
    try:
        ctm = mesh.ctm.ctypes.data_as(C.POINTER(C.c_float)) if mesh.ctm is not None else None
        mid = check(L.mrt_scene_add_material(h, C.byref(Lambert()._c())), "add_material")
        mesh_id = check(L.mrt_scene_add_obj(h, mesh.path.encode(), ctm, mid), f"load {mesh.path}")
        nv, nn, nt = C.c_int32(), C.c_int32(), C.c_int32()
        check(L.mrt_scene_mesh_info(h, mesh_id, C.byref(nv), C.byref(nn), C.byref(nt)), "mesh_info")
        v = np.zeros((nv.value, 3), np.float32)
        n = np.zeros((nn.value, 3), np.float32)
        vi = np.zeros((nt.value, 3), np.uint32)
        ni = np.zeros((nt.value, 3), np.uint32)
        check(L.mrt_scene_mesh_export(h, mesh_id, v.ctypes.data_as(C.POINTER(C.c_float)),
                                      n.ctypes.data_as(C.POINTER(C.c_float)), vi.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      ni.ctypes.data_as(C.POINTER(C.c_uint32))), "mesh_export")
        return v
    finally:
        L.mrt_scene_destroy(h)


def makeMBMeshObjs(scene: "Scene", mesh: TriangleMesh, mesh2: TriangleMesh, material):
    """makeMBMeshObjs (src/main.cpp:23, :202): one MBObject(material, mesh, mesh2, i)
    per triangle (src/MBObject.cpp:7-11) -- mesh at time 0, mesh2 (same topology)
    at time 1; a ray of time t meets the blend t * mesh2 + (1 - t) * mesh."""
    # mesh2 rides on this entry only: other entries of the same TriangleMesh
    # (makeMeshObjs) stay static, as their Objects are plain Objects
    scene._meshes.append((mesh, material, mesh2))


class Objects(list):
    """Objects (std::vector<Object*>) of a proxy: (mesh, material) pairs here."""


class BVH:
    """A ProxyObject's BVH (src/BVH.h:113-154); built in libmrt at Scene.preCalc()."""

    def __init__(self):
        self.objects = None


class ProxyObject:
    """ProxyObject(objects, bvh, Matrix4x4) (src/ProxyObject.h, src/ProxyObject.cpp:5-12):
    one instance of a shared BVH under a transform.  setupProxy / setupMultiProxy
    fill the Objects and BVH as the reference's static helpers do
    (src/ProxyObject.cpp:131-167); Scene.addObject adds the instance."""

    def __init__(self, objects, bvh, t=None):
        self.objects, self.bvh = objects, bvh
        self.matrix = (t if t is not None else Matrix4x4()).m.copy()

    @staticmethod
    def setupProxy(mesh, mat, objects, bvh):
        objects.append((mesh, mat))
        bvh.objects = objects

    @staticmethod
    def setupMultiProxy(meshes, numObjs, mats, objects, bvh):
        for j in range(numObjs):
            objects.append((meshes[j], mats[j]))
        bvh.objects = objects


def _ptr(x):
    """The address of a numpy array or a torch tensor; None stays None."""
    if x is None:
        return None
    return x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data


class _RayQuery:
    """What Scene's ray queries share: the checks of Scene._pairs, the scene on its device, and
    the marshalling -- numpy arrays (made contiguous float32) go through the synchronous entry,
    checked torch tensors through its _async twin on the current stream.  o, d, time, hits
    are the inputs' addresses (None where there is none)."""

    def __init__(self, scene, what, o, d, time=None, hits=None):
        self.scene, self.what = scene, what
        self.shape, self.n, self.tensors = scene._pairs(what, o, d, time, hits)
        check(lib().mrt_scene_upload(scene.handle, scene.device), "upload")
        if self.tensors:
            import torch
            self._device = o.device
            self._stream = torch.cuda.current_stream(o.device).cuda_stream
        else:
            o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
            time = np.ascontiguousarray(time, np.float32) if time is not None else None
            hits = np.ascontiguousarray(hits) if hits is not None else None
        self._inputs = (o, d, time, hits)   # (the contiguous copies live as long as their addresses)
        self.o, self.d, self.time, self.hits = map(_ptr, self._inputs)

    def row_width(self, row_width):
        """The coherence hint's default: W for an (H, W, 3) input, else 0."""
        if row_width is None:
            return self.shape[1] if len(self.shape) == 3 else 0
        return int(row_width)

    def new(self, dtype=None, words=None):
        """An output: float rgb in the rays' shape, or one record per ray -- a `dtype` array of the
        rays' shape, for tensors (n, words) int32."""
        if self.tensors:
            import torch
            if dtype is None:
                return torch.empty(self.shape, dtype=torch.float32, device=self._device)
            return torch.empty((self.n, words), dtype=torch.int32, device=self._device)
        return np.zeros(self.shape, np.float32) if dtype is None else np.zeros(self.shape[:-1], dtype)

    def call(self, entry, *args, stats=False):
        """entry(scene, *args), or entry_async(scene, *args, stream); stats: the synchronous
        entry has read the counters, so Scene.last_stats follows."""
        if self.tensors:
            check(getattr(lib(), entry + "_async")(self.scene.handle, *args, self._stream), self.what)
            return
        check(getattr(lib(), entry)(self.scene.handle, *args), self.what)
        if stats:
            self.scene.last_stats = self.scene.stats()


class Scene:
    """Scene (src/Scene.h).  Objects are whole meshes here; object ids inside a
    HitInfo are global triangle indices in insertion order."""

    def __init__(self, device: int = 0):
        self._meshes: List[tuple] = []   # (mesh, material) / (mesh, material, time-1 mesh) / (ProxyObject, None)
        self._lights: List[_Light] = []
        self.bg = Vector3(0)
        self.m_numPaths = 1
        self.m_pathTrace = False         # src/Scene.cpp:17-19
        self.m_maxBounces = 10
        self.m_sampleLightFromEnv = False   # never initialised by the reference's Scene ctor
        self.m_minSubdivs = 1            # src/Scene.cpp:20-22
        self.m_maxSubdivs = 1
        self.m_noiseThreshold = 0.01
        self.m_envMap = None
        self.m_envExposure = 1.0
        self.device = int(device)
        self._h = None
        self.bvh_info = None

    # -- construction (src/Scene.h:17-28)
    def addMesh(self, mesh, material): self._meshes.append((mesh, material))
    def addObject(self, proxy): self._meshes.append((proxy, None))   # Scene::addObject (a ProxyObject)
    def addLight(self, light): self._lights.append(light)
    def setBGColor(self, c): self.bg = Vector3(c)
    def setNumPaths(self, p): self.m_numPaths = int(p)
    def setPathTrace(self, pt): self.m_pathTrace = bool(pt)        # src/Scene.h:40
    def setMaxBounces(self, mb): self.m_maxBounces = int(mb)       # src/Scene.h:48
    def maxBounces(self): return self.m_maxBounces
    def setSampleEnv(self, b): self.m_sampleLightFromEnv = bool(b)  # src/Scene.h:57
    # adaptive supersampling, Scene::adaptiveSampleScene (src/Scene.h:42-55, src/Scene.cpp:252-293)
    def setMinSubdivs(self, r): self.m_minSubdivs = int(r)
    def minSubdivs(self): return self.m_minSubdivs
    def setMaxSubdivs(self, r): self.m_maxSubdivs = int(r)
    def maxSubdivs(self): return self.m_maxSubdivs
    def setNoise(self, n): self.m_noiseThreshold = float(n)
    def noise(self): return self.m_noiseThreshold
    def setEnvMap(self, t): self.m_envMap = t                    # src/Scene.h:23
    def setEnvExposure(self, e): self.m_envExposure = float(e)   # src/Scene.h:24

    def __del__(self):
        try:
            if self._h:
                lib().mrt_scene_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def handle(self):
        if self._h is None:
            raise MRTError("call preCalc() first")
        return self._h

    def preCalc(self):
        """Scene::preCalc -> BVH::build (host side of libmrt)."""
        L = lib()
        if self._h:
            L.mrt_scene_destroy(self._h)
        self._h = L.mrt_scene_create()
        mats = {}
        mat_objs = {}

        def add_mesh(mesh, mat):
            if id(mat) not in mats:
                mat_objs[id(mat)] = mat
                m = mat._c()
                mats[id(mat)] = check(L.mrt_scene_add_material(self._h, C.byref(m)), "add_material")
                if isinstance(mat, Blinn):
                    check(L.mrt_scene_set_material_optics(self._h, mats[id(mat)], mat.reflectAmt, mat.refractAmt,
                                                          mat.ior), "material optics")
                    check(L.mrt_scene_set_material_gloss(self._h, mats[id(mat)], mat.specGloss), "material gloss")
                    if mat.m_disperse:
                        i3 = (C.c_float * 3)(*mat.m_ior)
                        check(L.mrt_scene_set_material_dispersion(self._h, mats[id(mat)], 1, i3), "dispersion")
                    check(L.mrt_scene_set_material_translucency(self._h, mats[id(mat)], mat.translucency),
                          "material translucency")
                check(L.mrt_scene_set_material_sample_env(self._h, mats[id(mat)], int(mat.sampleEnv)), "sampleEnv")
            mid = mats[id(mat)]
            if mesh.path is not None:
                ctm = mesh.ctm.ctypes.data_as(C.POINTER(C.c_float)) if mesh.ctm is not None else None
                return check(L.mrt_scene_add_obj(self._h, mesh.path.encode(), ctm, mid), f"load {mesh.path}")
            v, n, vi, ni = mesh.verts, mesh.normals, mesh.vidx, mesh.nidx
            mm = _lib.mrt_mesh(v.ctypes.data_as(C.POINTER(C.c_float)), n.ctypes.data_as(C.POINTER(C.c_float)),
                               vi.ctypes.data_as(C.POINTER(C.c_uint32)), ni.ctypes.data_as(C.POINTER(C.c_uint32)),
                               len(v), len(n), len(vi), v.shape[1] if v.ndim == 2 else 3, n.shape[1] if n.ndim == 2 else 3)
            mesh_id = check(L.mrt_scene_add_mesh(self._h, C.byref(mm), mid), "add_mesh")
            if mesh.uv is not None:
                check(L.mrt_scene_mesh_set_texcoords(self._h, mesh_id, mesh.uv.ctypes.data_as(C.POINTER(C.c_float)),
                                                     len(mesh.uv), mesh.tidx.ctypes.data_as(C.POINTER(C.c_uint32))),
                      "texcoords")
            return mesh_id

        def set_motion(mesh_id, mesh2):
            v2 = np.ascontiguousarray(_mesh_vertices(mesh2), np.float32).reshape(-1, 3)
            nv = C.c_int32()
            check(L.mrt_scene_mesh_info(self._h, mesh_id, C.byref(nv), C.byref(C.c_int32()), C.byref(C.c_int32())),
                  "mesh_info")
            if len(v2) != nv.value:
                raise MRTError(f"motion mesh has {len(v2)} vertices, the time-0 mesh {nv.value}")
            check(L.mrt_scene_set_mesh_motion(self._h, mesh_id, v2.ctypes.data_as(C.POINTER(C.c_float))), "mesh motion")

        blas = {}   # BVH object -> BLAS id (built once, shared by its instances)
        self.blas_build_ms = 0.0
        self.blas_prims = 0
        self.blas_ids = blas
        for entry in self._meshes:
            item, mat = entry[0], entry[1]
            if not isinstance(item, ProxyObject):
                mesh_id = add_mesh(item, mat)
                if len(entry) > 2:   # makeMBMeshObjs: MBObjects of this entry only
                    set_motion(mesh_id, entry[2])
                continue
            key = id(item.bvh)
            if key not in blas:
                ids = (C.c_int32 * len(item.bvh.objects))(*[add_mesh(m, mt) for m, mt in item.bvh.objects])
                t0 = time.perf_counter()
                blas[key] = check(L.mrt_scene_make_blas(self._h, ids, len(ids)), "BLAS build")
                self.blas_build_ms += (time.perf_counter() - t0) * 1e3
                n, lv, p = C.c_int32(), C.c_int32(), C.c_int32()
                check(L.mrt_scene_blas_info(self._h, blas[key], C.byref(n), C.byref(lv), C.byref(p)), "blas_info")
                self.blas_prims += p.value
            m16 = np.ascontiguousarray(item.matrix, np.float32).reshape(16)
            check(L.mrt_scene_add_instance(self._h, blas[key], m16.ctypes.data_as(C.POINTER(C.c_float))), "instance")
        tex_ids = {}
        tex_shapes = {}   # texture id -> (H, W, channels): what updateTexture accepts

        def tex_id(t):
            if t is None:
                return -1
            if id(t) not in tex_ids:
                img = t.m_image
                if img.m_rawData is None:
                    raise MRTError("texture image has no data (loadImage first)")
                a = np.ascontiguousarray(img.m_rawData, np.float32)
                tex_ids[id(t)] = check(L.mrt_scene_add_texture_typed(self._h, a.ctypes.data_as(C.POINTER(C.c_float)),
                                                                     img.m_width, img.m_height,
                                                                     getattr(img, "m_imageType", TEX_HDR)), "add_texture")
                tex_shapes[tex_ids[id(t)]] = (img.m_height, img.m_width, _CHANNELS[getattr(img, "m_imageType", TEX_HDR)])
            return tex_ids[id(t)]

        for key, mid in mats.items():   # Material::set*Map
            mat = mat_objs[key]
            maps = mat._maps() if isinstance(mat, _Maps) else (None,) * 6
            if any(m is not None for m in maps):
                arr = (C.c_int32 * 6)(*[tex_id(m) for m in maps])
                check(L.mrt_scene_set_material_maps(self._h, mid, arr), "material maps")
            if getattr(mat, "envMap", None) is not None:
                check(L.mrt_scene_set_material_env_map(self._h, mid, tex_id(mat.envMap), mat.envExposure),
                      "material env map")

        self._mat_ids, self._mat_objs, self._tex_ids, self._tex_shapes = mats, mat_objs, tex_ids, tex_shapes
        for light in self._lights:
            tex_id(getattr(light, "texture", None))   # DomeLight::setTexture: the texture joins the scene
            lc = self._light_c(light)
            check(L.mrt_scene_add_light(self._h, C.byref(lc)), "add_light")
        if self.m_envMap is not None:
            check(L.mrt_scene_set_env_map(self._h, tex_id(self.m_envMap), self.m_envExposure), "env map")
        check(L.mrt_scene_set_background(self._h, f3(self.bg)), "bg")
        check(L.mrt_scene_set_num_paths(self._h, self.m_numPaths), "num_paths")
        check(L.mrt_scene_set_path_trace(self._h, int(self.m_pathTrace), self.m_maxBounces,
                                         int(self.m_sampleLightFromEnv)), "path trace")
        check(L.mrt_scene_set_subdivs(self._h, self.m_minSubdivs, self.m_maxSubdivs, self.m_noiseThreshold), "subdivs")
        t0 = time.perf_counter()
        check(L.mrt_scene_build_bvh(self._h), "BVH build")
        self.bvh_build_ms = (time.perf_counter() - t0) * 1e3   # host BVH::build wall time
        info = _lib.mrt_bvh_info()
        check(L.mrt_scene_bvh_info(self._h, C.byref(info)), "bvh_info")
        self.bvh_info = {k: getattr(info, k) for k, _ in info._fields_}
        return self.bvh_info

    def _light_c(self, light):
        """A Light object as mrt_light: the conversion preCalc and updateLights share (a dome
        light's texture as the id preCalc gave it)."""
        t = getattr(light, "texture", None)
        return light._c(-1 if t is None else self._tex_ids[id(t)])

    def mesh_arrays(self, mesh_id: int):
        L = lib()
        nv, nn, nt = C.c_int32(), C.c_int32(), C.c_int32()
        check(L.mrt_scene_mesh_info(self.handle, mesh_id, C.byref(nv), C.byref(nn), C.byref(nt)), "mesh_info")
        v = np.zeros((nv.value, 3), np.float32)
        n = np.zeros((nn.value, 3), np.float32)
        vi = np.zeros((nt.value, 3), np.uint32)
        ni = np.zeros((nt.value, 3), np.uint32)
        check(L.mrt_scene_mesh_export(self.handle, mesh_id, v.ctypes.data_as(C.POINTER(C.c_float)),
                                      n.ctypes.data_as(C.POINTER(C.c_float)), vi.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      ni.ctypes.data_as(C.POINTER(C.c_uint32))), "mesh_export")
        return v, n, vi, ni

    def dome_tables(self, light: int):
        """DomeLight::setTexture tables of light `light` (host arrays of libmrt)."""
        L = lib()
        nu, nv = C.c_int32(), C.c_int32()
        check(L.mrt_scene_dome_info(self.handle, int(light), C.byref(nu), C.byref(nv)), "dome_info")
        nu, nv = nu.value, nv.value
        shapes = {"cdf_u": (nu + 1,), "func_u": (nu,), "cdf_v": (nu, nv + 1), "func_v": (nu, nv),
                  "func_int": (nu + 1,), "cos_u": (nu + 1,), "sin_u": (nu + 1,), "cos_v": (nv + 1,),
                  "sin_v": (nv + 1,)}
        out = {k: np.zeros(s, np.float32) for k, s in shapes.items()}
        check(L.mrt_scene_dome_export(self.handle, int(light),
                                      *[out[k].ctypes.data_as(C.POINTER(C.c_float)) for k in shapes]), "dome_export")
        return out

    def blas_export(self, blas: int):
        L = lib()
        n, l, p = C.c_int32(), C.c_int32(), C.c_int32()
        check(L.mrt_scene_blas_info(self.handle, int(blas), C.byref(n), C.byref(l), C.byref(p)), "blas_info")
        nb = np.zeros((n.value, 24), np.float32)
        nc = np.zeros((n.value, 4), np.int32)
        lt = np.zeros((l.value, 36), np.float32)
        lp = np.zeros((l.value, 4), np.int32)
        check(L.mrt_scene_blas_export(self.handle, int(blas), nb.ctypes.data_as(C.POINTER(C.c_float)),
                                      nc.ctypes.data_as(C.POINTER(C.c_int32)), lt.ctypes.data_as(C.POINTER(C.c_float)),
                                      lp.ctypes.data_as(C.POINTER(C.c_int32))), "blas_export")
        return nb, nc, lt, lp

    def _refresh_bvh_info(self):
        info = _lib.mrt_bvh_info()
        check(lib().mrt_scene_bvh_info(self.handle, C.byref(info)), "bvh_info")
        self.bvh_info = {k: getattr(info, k) for k, _ in info._fields_}
        return self.bvh_info

    def bvh_export(self):
        info = self._refresh_bvh_info()   # a rebuild changes the counts
        nb = np.zeros((info["nodes"], 24), np.float32)
        nc = np.zeros((info["nodes"], 4), np.int32)
        lt = np.zeros((info["leaves"], 36), np.float32)
        lp = np.zeros((info["leaves"], 4), np.int32)
        check(lib().mrt_scene_bvh_export(self.handle, nb.ctypes.data_as(C.POINTER(C.c_float)),
                                         nc.ctypes.data_as(C.POINTER(C.c_int32)),
                                         lt.ctypes.data_as(C.POINTER(C.c_float)),
                                         lp.ctypes.data_as(C.POINTER(C.c_int32))), "bvh_export")
        return nb, nc, lt, lp

    def domeTablesDerived(self, light: int):
        """The derived tables of dome light `light` dome_tables leaves out: rad ((nv + 1, nu + 1, 4)),
        guide_u (nu + 1), guide_v ((nu, nv + 1)) (mrt_scene_dome_export_derived)."""
        L = lib()
        nu, nv = C.c_int32(), C.c_int32()
        check(L.mrt_scene_dome_info(self.handle, int(light), C.byref(nu), C.byref(nv)), "dome_info")
        nu, nv = nu.value, nv.value
        out = {"rad": np.zeros((nv + 1, nu + 1, 4), np.float32), "guide_u": np.zeros(nu + 1, np.int32),
               "guide_v": np.zeros((nu, nv + 1), np.int32)}
        check(L.mrt_scene_dome_export_derived(self.handle, int(light), out["rad"].ctypes.data_as(C.POINTER(C.c_float)),
                                              out["guide_u"].ctypes.data_as(C.POINTER(C.c_int32)),
                                              out["guide_v"].ctypes.data_as(C.POINTER(C.c_int32))), "dome_export_derived")
        return out

    def uploadCount(self):
        """How many times the built scene has been uploaded to a device (mrt_scene_upload_count)."""
        return check(lib().mrt_scene_upload_count(self.handle), "uploadCount")

    # -- lights, materials and texels that change between frames (no reference counterpart: its
    #    setters act on live objects; here the replica is updated in place, without a re-upload)
    def _stream_arg(self, stream):
        import torch
        return (stream if stream is not None else torch.cuda.current_stream(torch.device("cuda", self.device))).cuda_stream

    def updateLights(self, stream=None, asynchronous=False):
        """The current fields of the Light objects the scene was built from, in place
        (mrt_scene_update_lights): position, vertices, power, samples, noise threshold and
        castShadows may have changed; type, texture and fastShadows may not.  asynchronous=True
        (or a `stream`): mrt_scene_update_lights_async on `stream` (a torch stream; default: the
        current one), without a synchronisation; the scene is uploaded first if it is not."""
        L = lib()
        n = len(self._lights)
        arr = (_lib.mrt_light * max(n, 1))(*[self._light_c(l) for l in self._lights])
        if asynchronous or stream is not None:
            check(L.mrt_scene_upload(self.handle, self.device), "upload")
            check(L.mrt_scene_update_lights_async(self.handle, arr, n, self._stream_arg(stream)), "updateLights")
        else:
            check(L.mrt_scene_update_lights(self.handle, arr, n), "updateLights")

    def updateMaterial(self, material, stream=None, asynchronous=False):
        """The current kd, ka, ks, specExp, specAmt, Le and lightEmitted of `material` (a material
        object the scene was built with), in place (mrt_scene_update_material); everything its
        other setters cover stays.  asynchronous / stream: as updateLights."""
        L = lib()
        if id(material) not in getattr(self, "_mat_ids", {}):
            raise MRTError("updateMaterial: not a material of this scene (preCalc() assigns the ids)")
        mid, m = self._mat_ids[id(material)], material._c()
        if asynchronous or stream is not None:
            check(L.mrt_scene_upload(self.handle, self.device), "upload")
            check(L.mrt_scene_update_material_async(self.handle, mid, C.byref(m), self._stream_arg(stream)), "updateMaterial")
        else:
            check(L.mrt_scene_update_material(self.handle, mid, C.byref(m)), "updateMaterial")

    def textureId(self, texture):
        """The id preCalc gave a Texture object (an int passes through)."""
        if isinstance(texture, (int, np.integer)):
            return int(texture)
        if id(texture) not in getattr(self, "_tex_ids", {}):
            raise MRTError("not a texture of this scene (preCalc() assigns the ids)")
        return self._tex_ids[id(texture)]

    def updateTexture(self, texture, data, stream=None):
        """New texels for `texture` (a Texture of the scene, or its id), same width, height and
        type (mrt_scene_update_texture).  Environment maps and material maps read them at once;
        for a dome light of this texture DomeLight::setTexture runs again on the device.  A numpy
        array ((H, W, channels) float32) goes through the synchronous entry, which returns the
        device time in ms (0.0 for a scene not uploaded: the host rebuilds) and raises for a
        dome texture without positive radiance, everything staying as it was.  A float32 torch
        tensor on the scene's device goes through mrt_scene_update_texture_async on `stream`
        (default: the current one) and returns None; textureUpdateStatus() reports refusals."""
        L = lib()
        tid = self.textureId(texture)
        shape = getattr(self, "_tex_shapes", {}).get(tid)
        if shape is None:
            raise MRTError(f"updateTexture: bad texture id {tid}")
        if tuple(data.shape) != shape:
            raise MRTError(f"updateTexture: texels must have shape {shape} (height, width, channels), not {tuple(data.shape)}")
        if hasattr(data, "data_ptr"):
            import torch
            if not (data.is_cuda and data.dtype == torch.float32 and data.is_contiguous() and data.device.index == self.device):
                raise MRTError("updateTexture: tensors must be contiguous float32 on the scene's device")
            check(L.mrt_scene_upload(self.handle, self.device), "upload")
            check(L.mrt_scene_update_texture_async(self.handle, tid, data.data_ptr(), self._stream_arg(stream)), "updateTexture")
            return None
        if np.asarray(data).dtype != np.float32:
            raise MRTError("updateTexture: texels must be float32")
        a = np.ascontiguousarray(data, np.float32)
        ms = C.c_float(0.0)
        check(L.mrt_scene_update_texture(self.handle, tid, a.ctypes.data, C.byref(ms)), "updateTexture")
        return float(ms.value)

    def textureUpdateStatus(self):
        """Async texture updates refused since the last call (mrt_scene_texture_update_status; the
        caller has synchronised the streams it used)."""
        n = C.c_int32(0)
        check(lib().mrt_scene_texture_update_status(self.handle, C.byref(n)), "textureUpdateStatus")
        return int(n.value)

    # -- geometry that moves between frames (no reference counterpart: it rebuilds)
    def updateMesh(self, mesh_id: int, verts, normals=None, stream=None):
        """New vertices (and normals) for world mesh `mesh_id`, same counts and topology, and
        the hierarchy refitted in place (mrt_scene_update_mesh): the tree keeps its topology,
        so its quality degrades under large deformation and preCalc() remains the remedy.
        numpy arrays ((nv, 3) / (nn, 3)) go through the synchronous entry, which returns the
        device time of the refit kernels in ms (0.0 for a scene not yet uploaded: the host
        refits).  torch device tensors (contiguous float32 on the scene's device) go through
        mrt_scene_update_mesh_async on `stream` (a torch stream; default: the current one)
        without a host copy or a synchronisation (once the scene is on its device: a scene
        not yet uploaded is uploaded first), and return None; the mesh must have no texture
        coordinates."""
        L = lib()
        nv, nn, nt = C.c_int32(), C.c_int32(), C.c_int32()
        check(L.mrt_scene_mesh_info(self.handle, int(mesh_id), C.byref(nv), C.byref(nn), C.byref(nt)), "updateMesh")
        for x, n, what in ((verts, nv.value, "verts"), (normals, nn.value, "normals")):
            if x is not None and int(np.prod(tuple(x.shape))) != 3 * n:
                raise MRTError(f"updateMesh: {what} must hold {n} x 3 floats (the mesh's own count)")
        if hasattr(verts, "data_ptr"):
            import torch
            for x in (verts, normals):
                if x is not None and not (hasattr(x, "data_ptr") and x.is_cuda and x.dtype == torch.float32
                                          and x.is_contiguous() and x.device.index == self.device):
                    raise MRTError("updateMesh: tensors must be contiguous float32 on the scene's device")
            check(L.mrt_scene_upload(self.handle, self.device), "upload")
            st = (stream if stream is not None else torch.cuda.current_stream(verts.device)).cuda_stream
            check(L.mrt_scene_update_mesh_async(self.handle, int(mesh_id), verts.data_ptr(),
                                                normals.data_ptr() if normals is not None else None, st), "updateMesh")
            return None
        v = np.ascontiguousarray(verts, np.float32)
        n = np.ascontiguousarray(normals, np.float32) if normals is not None else None
        ms = C.c_float(0.0)
        check(L.mrt_scene_update_mesh(self.handle, int(mesh_id), v.ctypes.data, n.ctypes.data if n is not None else None,
                                      C.byref(ms)), "updateMesh")
        return float(ms.value)

    def deformMesh(self, mesh_id: int, verts, normals=None, verts2=None, stream=None):
        """New vertices (and normals) for any mesh `mesh_id`, same counts and topology
        (mrt_scene_deform_mesh).  A plain world mesh: what updateMesh does.  A mesh of a BLAS
        (setupProxy / setupMultiProxy): that BLAS refitted in place, the box of each of its
        instances recomputed from the new root, the world hierarchy refitted.  A motion-blurred
        world mesh (makeMBMeshObjs): `verts` at time 0 and `verts2` at time 1, both required; its
        MBObject boxes are recomputed, the world hierarchy refitted.  verts2 is refused elsewhere.
        numpy arrays go through the synchronous entry, which returns the device time of the
        kernels in ms (0.0 for a scene not yet uploaded: the host refits).  torch device tensors
        (contiguous float32 on the scene's device) go through mrt_scene_deform_mesh_async on
        `stream` (a torch stream; default: the current one) without a host copy or a
        synchronisation, and return None; the mesh must have no texture coordinates."""
        L = lib()
        nv, nn, nt = C.c_int32(), C.c_int32(), C.c_int32()
        check(L.mrt_scene_mesh_info(self.handle, int(mesh_id), C.byref(nv), C.byref(nn), C.byref(nt)), "deformMesh")
        for x, n, what in ((verts, nv.value, "verts"), (verts2, nv.value, "verts2"), (normals, nn.value, "normals")):
            if x is not None and int(np.prod(tuple(x.shape))) != 3 * n:
                raise MRTError(f"deformMesh: {what} must hold {n} x 3 floats (the mesh's own count)")
        if hasattr(verts, "data_ptr"):
            import torch
            for x in (verts, verts2, normals):
                if x is not None and not (hasattr(x, "data_ptr") and x.is_cuda and x.dtype == torch.float32
                                          and x.is_contiguous() and x.device.index == self.device):
                    raise MRTError("deformMesh: tensors must be contiguous float32 on the scene's device")
            check(L.mrt_scene_upload(self.handle, self.device), "upload")
            st = (stream if stream is not None else torch.cuda.current_stream(verts.device)).cuda_stream
            check(L.mrt_scene_deform_mesh_async(self.handle, int(mesh_id), verts.data_ptr(),
                                                verts2.data_ptr() if verts2 is not None else None,
                                                normals.data_ptr() if normals is not None else None, st), "deformMesh")
            return None
        v = np.ascontiguousarray(verts, np.float32)
        v2 = np.ascontiguousarray(verts2, np.float32) if verts2 is not None else None
        n = np.ascontiguousarray(normals, np.float32) if normals is not None else None
        ms = C.c_float(0.0)
        check(L.mrt_scene_deform_mesh(self.handle, int(mesh_id), v.ctypes.data, v2.ctypes.data if v2 is not None else None,
                                      n.ctypes.data if n is not None else None, C.byref(ms)), "deformMesh")
        return float(ms.value)

    def updateInstances(self, matrices, ids=None, first=0, stream=None):
        """New m_transform matrices for ProxyObject instances of the built scene
        (ProxyMatrix::set, then a refit where the reference rebuilds; mrt_scene_update_instances):
        inverse, inverse transpose and box per instance as addObject computes them, the BLAS and
        every hit id untouched, the world hierarchy refitted in place.
        numpy input ((n, 4, 4) or (n, 16)) or a sequence of Matrix4x4 goes through the
        synchronous entry for the instances `ids` (None: first .. first + n - 1) and returns the
        device time of the kernels in ms (0.0 for a scene not yet uploaded: the host refits).
        A contiguous float32 torch tensor (n, 4, 4) on the scene's device goes through
        mrt_scene_update_instances_async on `stream` (a torch stream; default: the current
        one) for the range first .. first + n - 1, without a host copy or a synchronisation,
        and returns None; `ids` must be None and the matrices finite and invertible (they are
        not checked).  The ProxyObjects given to addObject keep the matrices they had."""
        L = lib()
        if hasattr(matrices, "data_ptr"):
            import torch
            m = matrices
            if not (m.is_cuda and m.dtype == torch.float32 and m.is_contiguous() and m.device.index == self.device
                    and m.dim() == 3 and tuple(m.shape[1:]) == (4, 4)):
                raise MRTError("updateInstances: the tensor must be contiguous float32 (n, 4, 4) on the scene's device")
            if ids is not None:
                raise MRTError("updateInstances: device tensors take a range (first), not ids")
            check(L.mrt_scene_upload(self.handle, self.device), "upload")
            st = (stream if stream is not None else torch.cuda.current_stream(m.device)).cuda_stream
            check(L.mrt_scene_update_instances_async(self.handle, int(first), int(m.shape[0]), m.data_ptr(), st),
                  "updateInstances")
            return None
        if not isinstance(matrices, np.ndarray):
            matrices = [x.m if isinstance(x, Matrix4x4) else x for x in matrices]
        m = np.ascontiguousarray(matrices, np.float32)
        if m.size % 16 or (m.ndim == 3 and m.shape[1:] != (4, 4)):
            raise MRTError("updateInstances: matrices must be (n, 4, 4)")
        n = m.size // 16
        if ids is None:
            idv = np.arange(int(first), int(first) + n, dtype=np.int32) if first else None
        else:
            idv = np.ascontiguousarray(ids, np.int32).reshape(-1)
            if first or len(idv) != n:
                raise MRTError("updateInstances: one id per matrix, and no `first` beside ids")
        ms = C.c_float(0.0)
        check(L.mrt_scene_update_instances(self.handle, idv.ctypes.data if idv is not None else None, n, m.ctypes.data,
                                           C.byref(ms)), "updateInstances")
        return float(ms.value)

    def rebuildBVH(self, stream=None):
        """A new topology for the world hierarchy from the lanes its packets hold now, on the
        device and without a re-upload (mrt_scene_rebuild_bvh): where Scene::preCalc builds again
        after geometry has moved.  The tree is a Morton tree: measured faster than a refitted tree
        where instances have changed places, slower where one mesh of large triangles deforms
        (DESIGN.md 6i); bvhCost() and a timed frame decide.  Without a
        `stream` the synchronous entry acts on every replica and returns the device time in ms
        (0.0 for a scene not yet uploaded: the host rebuilds by the same rule); with a torch
        stream, mrt_scene_rebuild_bvh_async on it and None: no synchronisation, except that the
        first rebuild of a replica allocates and waits for the device once if its node array grows."""
        L = lib()
        if stream is not None:
            check(L.mrt_scene_upload(self.handle, self.device), "upload")
            check(L.mrt_scene_rebuild_bvh_async(self.handle, self._stream_arg(stream)), "rebuildBVH")
            return None
        ms = C.c_float(0.0)
        check(L.mrt_scene_rebuild_bvh(self.handle, C.byref(ms)), "rebuildBVH")
        self._refresh_bvh_info()
        return float(ms.value)

    def bvhCost(self):
        """The surface-area measure of the world hierarchy (mrt_scene_bvh_cost): every used slot's
        box area over the root box's, a leaf slot once per lane of its packet."""
        cost = C.c_double(0.0)
        check(lib().mrt_scene_bvh_cost(self.handle, C.byref(cost)), "bvhCost")
        return float(cost.value)

    def instance_count(self):
        return check(lib().mrt_scene_instance_count(self.handle), "instance_count")

    def instance_info(self, i: int):
        """What instance i holds now (mrt_scene_instance_info): blas, m, inv, inv_t ((4, 4)
        float32 each) and box ((2, 3): min, max).  Reads the device back after an async update."""
        blas = C.c_int32()
        m, inv, inv_t = (np.zeros((4, 4), np.float32) for _ in range(3))
        box = np.zeros((2, 3), np.float32)
        fp = C.POINTER(C.c_float)
        check(lib().mrt_scene_instance_info(self.handle, int(i), C.byref(blas), m.ctypes.data_as(fp), inv.ctypes.data_as(fp),
                                            inv_t.ctypes.data_as(fp), box.ctypes.data_as(fp)), "instance_info")
        return dict(blas=blas.value, m=m, inv=inv, inv_t=inv_t, box=box)

    # -- rendering (src/Scene.cpp:85-217)
    def raytraceImage(self, cam: Camera, img: Image, count_visits=False, want_hits=False, seed=0, devices=None):
        """devices: HIP device ordinals to deal the 32x32 buckets over (bucket b ->
        devices[b % n], mrt_render_opts.devices; one device may repeat)."""
        W, H = img.width(), img.height()
        opts = _lib.mrt_render_opts(W, H, self.device, int(count_visits), 1, int(want_hits), seed)
        if devices:
            dev_arr = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            opts.devices, opts.n_devices = dev_arr, len(devices)
        hits = np.zeros((H, W), HIT_DTYPE) if want_hits else None
        c = cam._c()
        check(lib().mrt_render(self.handle, C.byref(c), C.byref(opts), img.rgb.ctypes.data_as(C.POINTER(C.c_float)),
                               img.pixels.ctypes.data_as(C.POINTER(C.c_uint8)),
                               hits.ctypes.data if hits is not None else None), "raytraceImage")
        self.last_stats = self.stats()
        return hits

    def walk_info(self):
        """The walk of this scene's last one-light frame: {"lds_nodes": 1 (LDS top-node walk),
        0 (plain), -1 (none yet); "walk_exits": 1 or 2 (the walk loop's form: one exit unless
        tuning "walk_exit" 0 asks for the two-exit loop)}."""
        ln, wx = C.c_int32(-1), C.c_int32(-1)
        check(lib().mrt_scene_walk_info(self.handle, C.byref(ln), C.byref(wx)), "walk_info")
        return {"lds_nodes": int(ln.value), "walk_exits": int(wx.value)}

    def stats(self):
        st = _lib.mrt_stats()
        check(lib().mrt_scene_last_stats(self.handle, C.byref(st)), "stats")
        return {k: getattr(st, k) for k, _ in st._fields_}

    def wave_log(self, launch: int):
        """Per-wave records of the last count-mode render (diagnostics):
        array (waves, 60): start, end (device wall-clock ticks), tiles, node
        visits, then per tile (first 28) tile id << 40 | start tick & (2^40 - 1),
        then per tile its dequeue time in ticks;
        for launch 0 (primary) or 1 (shade); plus the clock rate (kHz)."""
        L = lib()
        out = np.zeros((1 << 16, 60), np.uint64)
        n = check(L.mrt_debug_wave_log(self.handle, int(launch), out.ctypes.data, len(out)), "wave_log")
        return out[:n].copy(), int(L.mrt_device_wall_clock_khz(self.handle))

    # -- ray queries (src/Scene.cpp:295-298)
    def traceBatch(self, o, d, tmin=0.001, tmax=1e12, any_hit=False):
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        n = len(o)
        tmin = np.ascontiguousarray(np.broadcast_to(np.asarray(tmin, np.float32), (n,)))
        tmax = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float32), (n,)))
        out = np.zeros(n, HIT_DTYPE)
        fp = C.POINTER(C.c_float)
        check(lib().mrt_trace(self.handle, o.ctypes.data_as(fp), d.ctypes.data_as(fp), tmin.ctypes.data_as(fp),
                              tmax.ctypes.data_as(fp), n, int(any_hit), out.ctypes.data), "trace")
        return out

    # -- Scene::sampleScene for caller rays (src/Scene.cpp:219-243)
    def sampleRays(self, o, d, time=None, seed=0, want_hits=False, count_visits=False, row_width=None):
        """Radiance along caller rays (mrt_sample_rays): closest hit, m_numPaths shade() calls
        averaged, environment / background on a miss.  o, d: (n, 3) or (H, W, 3); time: (n,) /
        (H, W) or None (0).  numpy arrays go through the synchronous entry; torch device tensors
        through mrt_sample_rays_async on the current stream, with no host copy (float32,
        contiguous, on the scene's device).  row_width (coherence hint, never changes a result):
        default W for an (H, W, 3) input, else 0.  Returns rgb in the input's shape -- and the
        primary hit records (HIT_DTYPE; an (n, 5) int32 device tensor of t, a, b bits, prim,
        inst for tensors) when want_hits.  Ray i draws from RNG stream i of `seed`."""
        q = _RayQuery(self, "sampleRays", o, d, time)
        rgb, hits = q.new(), q.new(HIT_DTYPE, 5) if want_hits else None
        q.call("mrt_sample_rays", q.o, q.d, q.time, q.n, q.row_width(row_width), int(seed), int(count_visits), _ptr(rgb),
               _ptr(hits), stats=True)
        return (rgb, hits) if want_hits else rgb

    # -- assemble sampleScene yourself: trace (with ray times), edit or filter the hits, shade them
    def _pairs(self, what, o, d, time=None, hits=None):
        """Shape checks shared by the ray queries: (shape, n, tensors?)."""
        shape = tuple(o.shape)
        if len(shape) not in (2, 3) or shape[-1] != 3 or tuple(d.shape) != shape:
            raise MRTError(f"{what}: o and d must both be (n, 3) or (H, W, 3)")
        n = int(np.prod(shape[:-1]))
        if time is not None and int(np.prod(tuple(time.shape))) != n:
            raise MRTError(f"{what}: time must hold one value per ray")
        tensors = hasattr(o, "data_ptr")
        if tensors:
            import torch
            for x in [o, d] + ([time] if time is not None else []):
                if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.device.index == self.device):
                    raise MRTError(f"{what}: tensors must be contiguous float32 on the scene's device")
        if hits is not None:
            if tensors:
                import torch
                if not (hasattr(hits, "data_ptr") and hits.is_cuda and hits.dtype == torch.int32 and hits.is_contiguous()
                        and tuple(hits.shape) == (n, 5) and hits.device.index == self.device):
                    raise MRTError(f"{what}: hits must be a contiguous (n, 5) int32 tensor on the scene's device")
            elif getattr(hits, "dtype", None) != HIT_DTYPE or int(np.prod(hits.shape)) != n:
                raise MRTError(f"{what}: hits must be a HIT_DTYPE array with one record per ray")
        return shape, n, tensors

    def traceRays(self, o, d, time=None, tmin=0.001, tmax=1e12, any_hit=False):
        """Scene::trace for rays with a time (mrt_trace_rays): o, d (n, 3) or (H, W, 3), time
        (n,) / (H, W) or None (= traceBatch), tmin / tmax scalars or one per ray (defaults: the
        reference's epsilon and MIRO_TMAX, the bounds of a camera ray).  numpy in: a HIT_DTYPE
        array of the rays' shape; torch device tensors: mrt_trace_rays_async on the current
        stream, an (n, 5) int32 tensor (t, a, b bits, prim, inst)."""
        q = _RayQuery(self, "traceRays", o, d, time)
        n = q.n
        if q.tensors:
            import torch

            def bound(x):
                if hasattr(x, "data_ptr"):
                    return x.to(device=o.device, dtype=torch.float32).reshape(-1).contiguous()
                return torch.full((n,), float(x), dtype=torch.float32, device=o.device)
            lo, hi = bound(tmin), bound(tmax)
            if lo.numel() != n or hi.numel() != n:
                raise MRTError("traceRays: tmin / tmax must be scalars or hold one value per ray")
        else:
            lo = np.ascontiguousarray(np.broadcast_to(np.asarray(tmin, np.float32).reshape(-1), (n,)))
            hi = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float32).reshape(-1), (n,)))
        out = q.new(HIT_DTYPE, 5)
        q.call("mrt_trace_rays", q.o, q.d, q.time, _ptr(lo), _ptr(hi), n, int(any_hit), _ptr(out))
        return out   # (tensors lo / hi were made on this stream: the allocator frees them in its order)

    def shadeHits(self, o, d, hits, time=None, seed=0, count_visits=False, row_width=None):
        """The hit / miss branch of Scene::sampleScene for caller (ray, hit) pairs
        (mrt_shade_hits): sampleRays with its primary rays replaced by `hits` -- closest-hit
        records as traceRays / sampleRays(want_hits=True) give them (not any-hit results), prim
        -1 = a miss.  numpy: a HIT_DTYPE array, checked on the host (MRTError names the first
        bad record); torch: an (n, 5) int32 device tensor on the current stream, bad records
        shaded as misses and reported by stats() as MRT_ERR_INVALID.  Returns rgb in the
        rays' shape."""
        q = _RayQuery(self, "shadeHits", o, d, time, hits)
        rgb = q.new()
        q.call("mrt_shade_hits", q.o, q.d, q.time, q.hits, q.n, q.row_width(row_width), int(seed), int(count_visits),
               _ptr(rgb), stats=True)
        return rgb

    def hitSurfaces(self, o, d, hits):
        """Ray::getPoint + HitInfo::getAllInfos per (ray, hit) pair (mrt_hit_surfaces): a
        SURFACE_DTYPE array of the rays' shape -- p, n, geo_n, tan, bitan, u, v, material,
        mesh, tri, inst; zeros and -1 for a miss.  torch device tensors: the current stream,
        an (n, 21) int32 tensor of the same words (floats as bits;
        x.cpu().numpy().view(SURFACE_DTYPE) names them)."""
        q = _RayQuery(self, "hitSurfaces", o, d, None, hits)
        out = q.new(SURFACE_DTYPE, 21)
        q.call("mrt_hit_surfaces", q.o, q.d, q.hits, q.n, _ptr(out))
        return out

    # -- Light::sampleLight at caller points (src/Light.h:35)
    def _light_query(self, what, p, n, rvec, time):
        """The checked inputs of sampleLights / lightSamples: the _RayQuery of (p, n, time) and
        rvec as an array of the points' kind and shape (None stays None)."""
        if rvec is not None:
            if hasattr(rvec, "data_ptr") != hasattr(p, "data_ptr") or tuple(rvec.shape) != tuple(p.shape):
                raise MRTError(f"{what}: rvec must be an array of the points' kind and shape")
        q = _RayQuery(self, what, p, n, time)
        if rvec is not None:
            if q.tensors:
                import torch
                if not (rvec.is_cuda and rvec.dtype == torch.float32 and rvec.is_contiguous() and rvec.device.index == self.device):
                    raise MRTError(f"{what}: tensors must be contiguous float32 on the scene's device")
            else:
                rvec = np.ascontiguousarray(rvec, np.float32)
        return q, rvec

    def lightSampleCap(self, secondary=False):
        """(per_light, total) of mrt_scene_light_sample_cap: the most samples each light can take
        at a point -- 1 for a point light, max(1, samples) for a rectangle or dome light, 1 for
        a dome light with `secondary` -- as an int32 array, and their sum M.  No device call."""
        per = np.zeros(len(self._lights), np.int32)
        total = C.c_int32()
        check(lib().mrt_scene_light_sample_cap(self.handle, int(bool(secondary)), per.ctypes.data, C.byref(total)),
              "lightSampleCap")
        return per, total.value

    def lightSamples(self, p, n, rvec=None, time=None, seed=0, first_draw=0, secondary=False, samples=True, counts=True,
                     e=False, per_light=False, count_visits=False):
        """sampleLights with the per-sample records (mrt_light_samples): the same points, draws
        and bits, through wavefront passes (gen / bin / trace / resolve).  Returns a dict of the
        outputs asked for (at least one): "samples", per point M = lightSampleCap()[1] rows of
        LIGHT_SAMPLE_DTYPE (dir, dist, e, vis), in light order then sample order, compact -- rows
        past the sum of the point's counts are zero here, or keep what they held when `samples`
        is the caller's own array of that shape, which is then written in place; "counts"
        (..., n_lights) int32, the samples each light took; "e" and "per_light" as sampleLights
        returns them.  For device tensors "samples" is (n, M, 8) float32 and "counts" (n,
        n_lights) int32, on the current stream (mrt_light_samples_async).  A scene with a
        transparent-shadow light, or with M above 64, is refused."""
        what = "lightSamples"
        own = not isinstance(samples, (bool, np.bool_))   # the caller's array, written in place
        if not (own or samples or counts or e or per_light):
            raise MRTError(f"{what}: at least one of samples, counts, e, per_light")
        shape, count, tensors = self._pairs(what, p, n, time, None)
        nl, m = len(self._lights), self.lightSampleCap(secondary)[1]
        lead = shape[:-1]
        if own:   # (checked before the scene goes to its device)
            if tensors:
                import torch
                ok = (hasattr(samples, "data_ptr") and samples.is_cuda and samples.dtype == torch.float32 and
                      samples.is_contiguous() and samples.device == p.device and tuple(samples.shape) == (count, m, 8))
                want = f"a contiguous float32 ({count}, {m}, 8) tensor on the points' device"
            else:
                ok = (isinstance(samples, np.ndarray) and samples.dtype == LIGHT_SAMPLE_DTYPE and
                      samples.flags.c_contiguous and samples.shape == lead + (m,))
                want = f"a C-contiguous LIGHT_SAMPLE_DTYPE array of shape {lead + (m,)}"
            if not ok:
                raise MRTError(f"{what}: samples must be {want}")
        q, rvec = self._light_query(what, p, n, rvec, time)
        out = {}
        if tensors:
            import torch

            def new(shape, dtype=torch.float32):
                return torch.zeros(shape, dtype=dtype, device=p.device)
            rec_shape, rec_type, cnt_shape, i32 = (count, m, 8), torch.float32, (count, nl), torch.int32
        else:
            def new(shape, dtype=np.float32):
                return np.zeros(shape, dtype)
            rec_shape, rec_type, cnt_shape, i32 = lead + (m,), LIGHT_SAMPLE_DTYPE, lead + (nl,), np.int32
        if own or samples:
            out["samples"] = samples if own else new(rec_shape, rec_type)
        if counts:
            out["counts"] = new(cnt_shape, i32)
        if e:
            out["e"] = new(q.shape)
        if per_light:
            out["per_light"] = new(lead + (nl, 4))
        q.call("mrt_light_samples", q.o, q.d, _ptr(rvec), q.time, q.n, int(seed), int(first_draw), int(secondary),
               int(count_visits), *(_ptr(out.get(k)) for k in ("samples", "counts", "e", "per_light")), stats=True)
        return out

    def sampleLights(self, p, n, rvec=None, time=None, seed=0, first_draw=0, secondary=False, per_light=False,
                     count_visits=False):
        """What the scene's lights deliver at caller points (mrt_sample_lights): p, n (points
        and normals, used as given) and rvec (the specular term's reflection vector; None: zero)
        are (n, 3) or (H, W, 3); time (n,) / (H, W) or None (0) is the shadow rays' time.
        Returns e, the sum of E over the lights in the points' shape -- Lambert::shade with kd =
        1, ka = 0 -- or (e, per) with per_light, per (..., n_lights, 4) holding E.r, E.g, E.b,
        outSpec of every light.  Point i draws from RNG stream i of `seed`, from draw
        first_draw of chain level 0 (0: Lambert::shade's light loop, 1: Blinn::shade's);
        secondary is isSecondary (a dome light takes one sample).  numpy arrays go through the
        synchronous entry; contiguous float32 torch tensors on the scene's device through
        mrt_sample_lights_async on the current stream."""
        q, rvec = self._light_query("sampleLights", p, n, rvec, time)
        shape = q.shape[:-1] + (len(self._lights), 4)
        if q.tensors:
            import torch
            per = torch.empty(shape, dtype=torch.float32, device=p.device) if per_light else None
        else:
            per = np.zeros(shape, np.float32) if per_light else None
        e = q.new()
        q.call("mrt_sample_lights", q.o, q.d, _ptr(rvec), q.time, q.n, int(seed), int(first_draw), int(secondary),
               int(count_visits), _ptr(e), _ptr(per), stats=True)
        return (e, per) if per_light else e

    def primObject(self, prim: int):
        """HitInfo::obj / m_proxy of a hit id: (mesh id, triangle index, instance or -1)."""
        m, t, i = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().mrt_scene_prim_object(self.handle, int(prim), C.byref(m), C.byref(t), C.byref(i)), "prim_object")
        return m.value, t.value, i.value

    def trace(self, hitInfo: HitInfo, ray: Ray, tMin=0.001) -> bool:
        """Scene::trace(threadID, HitInfo&, const Ray&, tMin): hitInfo.t is tMax in, t out."""
        r = self.traceBatch([ray.o], [ray.d], tMin, hitInfo.t)[0]
        if r["prim"] < 0:
            return False
        hitInfo.t, hitInfo.a, hitInfo.b, hitInfo.obj = float(r["t"]), float(r["a"]), float(r["b"]), int(r["prim"])
        return True
