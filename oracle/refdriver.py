"""Wrapper for oracle/_ref/ref_driver: the reference renderer's own code, run on a scene
described by the calls OracleScene takes (oracle/oracle.py), in the same order.

TEST INFRASTRUCTURE ONLY: tests/test_reference_cpu.py and oracle/ref/make_reference_fixtures.py.
The driver exists only where the reference's sources were at hand when oracle/ref/Makefile ran
(available()); nothing that runs on a GPU machine may import this module's driver side.
Every run is single-threaded (OMP_NUM_THREADS=1): the reference's random-number pool and its
counters are per thread, and thread 0's are the ones the driver reads.
"""
from __future__ import annotations

import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(_HERE, "_ref", "ref_driver")
MAKE_DIR = os.path.join(_HERE, "ref")

TRACE_DTYPE = np.dtype([("hit", "<i4"), ("t", "<f4"), ("a", "<f4"), ("b", "<f4"), ("obj", "<i4"), ("proxy", "<i4"),
                        ("nodes", "<u4"), ("leaves", "<u4")])
TEX_CHANNELS = {0: 3, 1: 1, 3: 3, 4: 4}   # oracle.TEX_CHANNELS: HDR, GRAYSCALE, RGB, RGBA


def reference_root():
    return os.environ.get("MRT_REFERENCE", "/root/reference")


def reference_present():
    return os.path.isdir(os.path.join(reference_root(), "src"))


def available():
    return os.path.exists(DRIVER)


def toolchain():
    """What decides the reference's float results here: compiler, flags, C library, FMA."""
    import platform
    flags = subprocess.run(["make", "-s", "-C", MAKE_DIR, "flags"], stdout=subprocess.PIPE, text=True).stdout.strip()
    cxx = subprocess.run(["g++", "--version"], stdout=subprocess.PIPE, text=True).stdout.splitlines()[0]
    try:
        fma = " fma " in (" " + open("/proc/cpuinfo").read().split("flags", 1)[1].split("\n", 1)[0] + " ")
    except (OSError, IndexError):
        fma = None
    return {"compiler": cxx, "flags": flags, "libc": " ".join(platform.libc_ver()), "host_cpu_fma": fma}


_current = None


def _ensure_current():
    """The driver must be the one oracle/ref's sources build: it prints the digest it was built
    from (ref_driver version), the Makefile prints the sources' (make sum).  A driver left over
    from other sources is rebuilt where the reference is at hand; one that still differs is an
    error, never a driver to take answers from."""
    global _current
    if _current:
        return

    def digests():
        want = subprocess.run(["make", "-s", "-C", MAKE_DIR, "sum"], stdout=subprocess.PIPE, text=True).stdout.strip()
        r = subprocess.run([DRIVER, "version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        return want, (r.stdout.strip() if r.returncode == 0 else "none (%s)" % r.stdout.strip()[-200:])
    want, have = digests()
    if want != have and reference_present():
        r = subprocess.run(["make", "-s", "-C", MAKE_DIR, "MRT_REFERENCE=" + reference_root()], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        built = r.stdout[-2000:]
        want, have = digests()
    else:
        built = ""
    if want != have:
        raise RuntimeError("oracle/_ref/ref_driver was built from other sources (digest %s, oracle/ref has %s) and "
                           "make -C oracle/ref did not replace it: %s" % (have, want, built))
    _current = want


def _run(args):
    _ensure_current()
    env = dict(os.environ, OMP_NUM_THREADS="1")
    r = subprocess.run([DRIVER] + [str(a) for a in args], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("ref_driver %s failed (%d): %s" % (args[0], r.returncode, r.stdout.decode(errors="replace")[-2000:]))


def _f(x):
    return struct.pack("<f", float(x))[::-1].hex()


def _v(x):
    x = [float(v) for v in (np.asarray(x, np.float32).reshape(-1))]
    if len(x) == 1:
        x = x * 3
    assert len(x) == 3
    return " ".join(_f(v) for v in x)


def load_obj(path):
    """TriangleMesh::load(path) and preCalc: dict of verts (nv, 3), normals (nn, 3), vidx, nidx
    (nt, 3); with texture coordinates also uv (ntc, 2), tidx (nt, 3) and tangents, bitangents
    (nn, 3), one per normal slot.  The driver counts nv, nn and ntc from the file itself.  Slots of
    the tangent arrays that no triangle writes hold whatever the allocation held."""
    d = tempfile.mkdtemp(prefix="refdrv_")
    try:
        out = os.path.join(d, "mesh.bin")
        _run(["load", path, out])
        raw = open(out, "rb").read()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    nt, has_tc, nv, nn, ntc, has_tan = struct.unpack_from("<6I", raw, 0)
    off = 24

    def take(n, dt, w):
        nonlocal off
        a = np.frombuffer(raw, dt, n * w, off).reshape(n, w).copy()
        off += a.nbytes
        return a
    m = {"verts": take(nv, "<f4", 3), "normals": take(nn, "<f4", 3), "vidx": take(nt, "<u4", 3), "nidx": take(nt, "<u4", 3)}
    if has_tc:
        m["uv"] = take(ntc, "<f4", 2)
        m["tidx"] = take(nt, "<u4", 3)
    if has_tan:
        m["tangents"] = take(nn, "<f4", 3)
        m["bitangents"] = take(nn, "<f4", 3)
    assert off == len(raw)
    return m


def _one_shot(args_of):
    d = tempfile.mkdtemp(prefix="refdrv_")
    try:
        out = os.path.join(d, "out.bin")
        _run(args_of(d, out))
        return open(out, "rb").read()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def gamma_tables():
    """(Image::linear_to_gamma (32769,) uint8, Image::linear_to_gammaF (32769,) float32)."""
    raw = _one_shot(lambda d, out: ["gamma", out])
    assert len(raw) == 32769 * 5
    return np.frombuffer(raw, np.uint8, 32769).copy(), np.frombuffer(raw[32769:], "<f4").copy()


def map_values(x):
    """Map() of each float (src/Image.cpp:71-76), through Image::setPixel on a 1-row image: uint8."""
    x = np.ascontiguousarray(x, "<f4").reshape(-1)

    def args(d, out):
        x.tofile(os.path.join(d, "in.bin"))
        return ["map", os.path.join(d, "in.bin"), len(x), out]
    raw = _one_shot(args)
    px = np.frombuffer(raw, np.uint8).reshape(len(x), 3)
    assert (px[:, 0] == px[:, 1]).all() and (px[:, 0] == px[:, 2]).all()
    return px[:, 0].copy()


def decode(path):
    """RawImage::loadImage(path): (H, W, channels) float32."""
    assert " " not in path
    raw = _one_shot(lambda d, out: ["decode", path, out])
    w, h, ch = struct.unpack_from("<3i", raw, 0)
    return np.frombuffer(raw, "<f4", w * h * ch, 12).reshape(h, w, ch).copy()


class RefScene:
    """The OracleScene calls, recorded as a scene file for the driver.  Methods return the
    same ids OracleScene's do (materials, meshes, textures, lights, BLASes count from 0)."""

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="refdrv_")
        self.lines = []
        self.n = {"material": 0, "mesh": 0, "texture": 0, "light": 0, "blas": 0, "blob": 0}
        self.world = []          # ("mesh", id) / ("inst", blas): the world's objects, in add order
        self.mesh_tris = []
        self.mesh_nv = []
        self.blas_meshes = []
        self.in_blas = set()

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def __del__(self):
        self.close()

    def _id(self, kind):
        self.n[kind] += 1
        return self.n[kind] - 1

    def _blob(self, *arrays):
        p = os.path.join(self.dir, "a%d.bin" % self._id("blob"))
        with open(p, "wb") as f:
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
        return p

    # -- the OracleScene calls ------------------------------------------------------
    def add_material(self, kind="lambert", kd=(1, 1, 1), ka=(0, 0, 0), ks=(1, 1, 1), specExp=1.0, specAmt=0.0,
                     reflectAmt=0.0, refractAmt=0.0, ior=1.5, specGloss=1.0, translucency=0.0, le=(0, 0, 0),
                     emitted=0.0, sampleEnv=True, disperse=False, ior3=None):
        i3 = (ior, ior, ior) if ior3 is None else tuple(ior3)
        self.lines.append(" ".join(["material", "0" if kind == "lambert" else "1", _v(kd), _v(ka), _v(ks), _f(specExp),
                                    _f(specAmt), _f(reflectAmt), _f(refractAmt), _f(ior), _f(specGloss), _f(translucency),
                                    _v(le), _f(emitted), str(int(bool(sampleEnv))), str(int(bool(disperse))),
                                    _f(i3[0]), _f(i3[1]), _f(i3[2])]))
        return self._id("material")

    def add_mesh(self, verts, normals, vidx, nidx, material):
        v = np.ascontiguousarray(verts, "<f4").reshape(-1, 3)
        n = np.ascontiguousarray(normals, "<f4").reshape(-1, 3)
        vi = np.ascontiguousarray(vidx, "<u4").reshape(-1, 3)
        ni = np.ascontiguousarray(nidx, "<u4").reshape(-1, 3)
        self.lines.append("mesh %d %d %d %d %s" % (len(v), len(n), len(vi), material, self._blob(v, n, vi, ni)))
        mid = self._id("mesh")
        self.world.append(("mesh", mid)); self.mesh_tris.append(len(vi)); self.mesh_nv.append(len(v))
        return mid

    def add_obj(self, path, material, ntris):
        """ntris: the triangles the file loads to (hit ids need it; the oracle knows)."""
        assert " " not in path
        self.lines.append("obj %d %s" % (material, path))
        mid = self._id("mesh")
        self.world.append(("mesh", mid)); self.mesh_tris.append(int(ntris)); self.mesh_nv.append(None)
        return mid

    def set_texcoords(self, mesh, uv, tidx):
        uv = np.ascontiguousarray(uv, "<f4").reshape(-1, 2)
        ti = np.ascontiguousarray(tidx, "<u4").reshape(-1, 3)
        assert len(ti) == self.mesh_tris[mesh]
        self.lines.append("texcoords %d %d %s" % (mesh, len(uv), self._blob(uv, ti)))

    def set_motion(self, mesh, verts2):
        v = np.ascontiguousarray(verts2, "<f4").reshape(-1, 3)
        assert len(v) == self.mesh_nv[mesh]
        self.lines.append("motion %d %d %s" % (mesh, len(v), self._blob(v)))

    def add_texture_typed(self, data, type_):
        a = np.ascontiguousarray(data, "<f4")
        ch = TEX_CHANNELS[int(type_)]
        assert a.size == a.shape[0] * a.shape[1] * ch
        self.lines.append("texture %d %d %d %d %s" % (a.shape[1], a.shape[0], int(type_), ch, self._blob(a)))
        return self._id("texture")

    def add_texture(self, rgb):
        return self.add_texture_typed(rgb, 0)

    def set_material_maps(self, material, color=-1, normal=-1, specular=-1, reflect=-1, refract=-1, alpha=-1):
        self.lines.append("maps %d %d %d %d %d %d %d" % (material, color, normal, specular, reflect, refract, alpha))

    def _light(self, head, samples, noise, cast, fast):
        self.lines.append("light %s %d %s %d %d" % (head, samples, _f(noise), int(bool(cast)), int(bool(fast))))
        return self._id("light")

    def add_point_light(self, pos, power, cast_shadows=True, fast_shadows=True):
        """fast_shadows False is Light::setFastShadows(false); the oracle's scene then gets
        cast_shadows False (tests/helpers.py says why)."""
        return self._light("point %s %s" % (_v(pos), _f(power)), 1, 0.001, cast_shadows, fast_shadows)

    def add_rect_light(self, v1, v2, v3, power, samples=1, noise=0.001, cast_shadows=True, fast_shadows=True):
        return self._light("rect %s %s %s %s" % (_v(v1), _v(v2), _v(v3), _f(power)), samples, noise, cast_shadows, fast_shadows)

    def add_dome_light(self, texture, power, samples=1, noise=0.001, fast_shadows=True):
        return self._light("dome %d %s" % (texture, _f(power)), samples, noise, True, fast_shadows)

    def make_blas(self, meshes):
        self.lines.append("blas %d %s" % (len(meshes), " ".join(str(int(m)) for m in meshes)))
        self.in_blas.update(int(m) for m in meshes)
        self.blas_meshes.append([int(m) for m in meshes])
        return self._id("blas")

    def add_instance(self, blas, m):
        m16 = np.asarray(m, np.float32).reshape(16)
        self.lines.append("instance %d %s" % (blas, " ".join(_f(x) for x in m16)))
        self.world.append(("inst", int(blas)))
        return sum(1 for k, _ in self.world if k == "inst") - 1

    def set_env_map(self, texture, exposure=1.0):
        self.lines.append("envmap %d %s" % (texture, _f(exposure)))

    def set_material_env_map(self, material, texture, exposure=1.0):
        self.lines.append("matenv %d %d %s" % (material, texture, _f(exposure)))

    def set_bg(self, rgb):
        self.lines.append("bg " + _v(rgb))

    def set_num_paths(self, n):
        self.lines.append("numpaths %d" % n)

    def set_path_trace(self, enable=True, max_bounces=10, sample_env=False):
        self.lines.append("pathtrace %d %d %d" % (int(bool(enable)), max_bounces, int(bool(sample_env))))

    def set_subdivs(self, min_subdivs, max_subdivs, noise=0.01):
        self.lines.append("subdivs %d %d %s" % (min_subdivs, max_subdivs, _f(noise)))

    def build(self):
        pass    # the driver runs Scene::preCalc when it has read the file

    # -- running ---------------------------------------------------------------------
    def _scene_file(self, cam=None, W=1, H=1):
        lines = list(self.lines)
        if cam is not None:
            lines.append(" ".join(["camera", _v(cam["eye"]), _v(cam.get("up", (0, 1, 0))), _v(cam["lookAt"]), _f(cam["fov"]),
                                   _f(cam.get("aperture", 0.0)), _f(cam.get("focusPlane", 1.0)),
                                   _f(cam.get("shutterSpeed", 0.001))]))
        lines.append("size %d %d" % (W, H))
        p = os.path.join(self.dir, "scene%d.txt" % self._id("blob"))
        open(p, "w").write("\n".join(lines) + "\n")
        return p

    def _out(self):
        return os.path.join(self.dir, "out%d.bin" % self._id("blob"))

    def bvh_counts(self):
        """(QBVH nodes, QBVH leaves) of the world's tree."""
        out = self._out()
        _run(["bvh", self._scene_file(), out])
        n = np.fromfile(out, "<i4")
        return int(n[0]), int(n[1])

    def hit_ids(self, rec):
        """The oracle's hit id (oro_hit.prim) of each driver record: world objects in add
        order, then every instance's own objects, instance by instance; -1 on a miss."""
        n_world, inst_pos = 0, []
        for kind, i in self.world:
            if kind == "mesh":
                n_world += 0 if i in self.in_blas else self.mesh_tris[i]
            else:
                inst_pos.append((n_world, i))
                n_world += 1
        base, acc = {}, 0
        for pos, b in inst_pos:
            base[pos] = n_world + acc
            acc += sum(self.mesh_tris[m] for m in self.blas_meshes[b])
        ids = np.where(rec["hit"] != 0, rec["obj"], -1).astype(np.int64)
        for k in np.nonzero((rec["hit"] != 0) & (rec["proxy"] >= 0))[0]:
            ids[k] = base[int(rec["proxy"][k])] + int(rec["obj"][k])
        return ids.astype(np.int32)

    def trace(self, o, d, tmin, tmax, shadow=False):
        """Scene::trace per ray -> TRACE_DTYPE records (nodes / leaves: this ray's increments of
        BVH::rayBoxIntersections / Ray::rayTriangleIntersections).  shadow: IS_SHADOW_RAY rays,
        for which the reference records t alone."""
        o = np.ascontiguousarray(o, "<f4").reshape(-1, 3)
        d = np.ascontiguousarray(d, "<f4").reshape(-1, 3)
        n = len(o)
        rays = np.empty((n, 8), "<f4")
        rays[:, 0:3], rays[:, 3:6] = o, d
        rays[:, 6], rays[:, 7] = np.float32(tmin) if np.ndim(tmin) == 0 else tmin, np.float32(tmax) if np.ndim(tmax) == 0 else tmax
        out = self._out()
        _run(["trace", self._scene_file(), self._blob(rays), n, int(bool(shadow)), out])
        return np.fromfile(out, TRACE_DTYPE)

    def _frames(self, cmd, cam, W, H, extra=()):
        out = self._out()
        _run([cmd, self._scene_file(cam, W, H)] + list(extra) + [out])
        return np.fromfile(out, "<f4")

    def render(self, cam, W, H):
        """adaptiveSampleScene per pixel in the reference's bucket order, its own RNG: (H, W, 3)."""
        return self._frames("render", cam, W, H).reshape(H, W, 3)

    def replay(self, cam, W, H):
        """One sample per pixel on the oracle's draws (ref_driver.cpp: replay_frame): (H, W, 3)."""
        return self._frames("replay", cam, W, H).reshape(H, W, 3)

    def replay_log(self, cam, W, H, log):
        """Scene::adaptiveSampleScene per pixel with the pool laid out from the oracle's draw log
        (OracleScene.render(..., draw_log=True); ref_driver.cpp: replay_log_frame), every chain
        level, path and eye ray: dict of rgb (H, W, 3) float32, rgb8 (H, W, 3) uint8 as
        Image::setPixel stored it, consumed (H, W) uint32 draws the reference took."""
        off, keys = np.asarray(log["draw_offsets"], np.int64), np.ascontiguousarray(log["draw_keys"], "<u4")
        assert len(off) == W * H + 1 and keys.shape == (int(off[-1]), 2)
        out = self._out()
        _run(["replaylog", self._scene_file(cam, W, H), self._blob(np.diff(off).astype("<u4"), keys), out])
        raw = open(out, "rb").read()
        n = W * H
        assert len(raw) == n * 12 + n * 3 + n * 4
        return {"rgb": np.frombuffer(raw, "<f4", n * 3).reshape(H, W, 3).copy(),
                "rgb8": np.frombuffer(raw, np.uint8, n * 3, n * 12).reshape(H, W, 3).copy(),
                "consumed": np.frombuffer(raw, "<u4", n, n * 15).reshape(H, W).copy()}

    def repeat(self, cam, W, H, K):
        """K renders in one process, the RNG stream running on: (K, H, W, 3) independent replicas."""
        return self._frames("repeat", cam, W, H, [int(K)]).reshape(K, H, W, 3)
