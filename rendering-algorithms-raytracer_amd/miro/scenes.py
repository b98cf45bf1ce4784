"""Deterministic synthetic stand-ins for the BASELINE scenes whose assets are
missing from the reference snapshot (.MISSING_LARGE_BLOBS: sponza.obj,
bunny.obj, dragon_2.obj, buddha_smooth.obj), plus the config presets C1..C3
(SURVEY.md §8(d)).  Camera and light parameters are the reference scripts':
  C1 Cornell   : src/assignment2.h:457-460 (camera), PointLight (2.75, 5, -2.75)
  C2 bunny     : src/assignment2.h:89-118  (eye (0,5,15), PointLight (10,20,10) 1000)
  C3 Sponza    : src/assignment2.h:354-373 (eye (8,1.5,1) -> (0,2.5,-1), fov 55,
                 PointLight (0,10,0) 200, Blinn kd = 1)
Meshes are written as OBJ text (v / vn / f lines < 80 chars) and go through
libmrt's OBJ loader like real assets would.  Every vertex carries a small
seeded jitter so no >=128-triangle group shares a centroid coordinate (the
reference's binning divides by the centroid extent, src/BVH.cpp:714).
"""
from __future__ import annotations

import hashlib
import os

import numpy as np

SCENE_VERSION = 1

# Reference data files the configs use as they are (copied from the reference's
# Images/ and Models/; data, not code): the dome / environment map of config 5
# and the Sponza path-tracing light panel of makeSponzaScenePathTrace.
ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "assets")
ARCHES_HDR = os.path.join(ASSETS, "Arches_E_PineTree.hdr")      # Images/Arches_E_PineTree.hdr, 1000 x 500
SPONZA_LIGHT_OBJ = os.path.join(ASSETS, "sponza-light.obj")      # Models/sponza-light.obj
SKIES = {"arches": ARCHES_HDR}


DEFAULT_CACHE = os.path.join("/tmp", "mrt_scenes")


def _cache_dir():
    """$MRT_SCENE_CACHE, or the shared default -- unless that one exists and belongs to
    another user (files cannot be added to it): then this user's own beside it."""
    d = os.environ.get("MRT_SCENE_CACHE")
    if d is None:
        d = DEFAULT_CACHE
        if os.path.isdir(d) and not os.access(d, os.W_OK | os.X_OK):
            d += "-%d" % os.getuid()
    os.makedirs(d, exist_ok=True)
    return d


def write_obj(path, verts, faces, normals=None):
    """faces: (n,3) 0-based.  With normals: one normal per vertex (f a//a ...)."""
    verts = np.asarray(verts, np.float64)
    faces = np.asarray(faces, np.int64) + 1
    lines = ["# synthetic scene (rendering-algorithms-raytracer_amd/miro/scenes.py)"]
    lines += ["v %.6f %.6f %.6f" % tuple(v) for v in verts]
    if normals is not None:
        lines += ["vn %.6f %.6f %.6f" % tuple(n) for n in np.asarray(normals, np.float64)]
        lines += ["f %d//%d %d//%d %d//%d" % (a, a, b, b, c, c) for a, b, c in faces]
    else:
        lines += ["f %d %d %d" % tuple(f) for f in faces]
    tmp = path + ".tmp%d" % os.getpid()
    with open(tmp, "w") as f:
        f.write("\n".join(lines) + "\n")
    os.replace(tmp, path)
    return path


class _Mesh:
    def __init__(self):
        self.v, self.f = [], []
        self.nv = 0

    def add(self, verts, faces):
        verts = np.asarray(verts, np.float64).reshape(-1, 3)
        self.v.append(verts)
        self.f.append(np.asarray(faces, np.int64).reshape(-1, 3) + self.nv)
        self.nv += len(verts)

    def grid(self, origin, du, dv, nu, nv_):
        """Quad grid spanning origin + s*du + t*dv, s,t in [0,1]; 2*nu*nv tris."""
        s = np.linspace(0, 1, nu + 1)
        t = np.linspace(0, 1, nv_ + 1)
        S, T = np.meshgrid(s, t, indexing="ij")
        P = np.asarray(origin) + S[..., None] * np.asarray(du) + T[..., None] * np.asarray(dv)
        idx = np.arange((nu + 1) * (nv_ + 1)).reshape(nu + 1, nv_ + 1)
        a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
        f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
        self.add(P.reshape(-1, 3), f)

    def box(self, lo, hi, n=(1, 1, 1)):
        lo, hi = np.asarray(lo, float), np.asarray(hi, float)
        ex = hi - lo
        X, Y, Z = np.eye(3) * ex
        nx, ny, nz = n
        self.grid(lo, X, Z, nx, nz)                 # bottom
        self.grid(lo + Y, Z, X, nz, nx)             # top
        self.grid(lo, Y, X, ny, nx)                 # front (z = lo)
        self.grid(lo + Z, X, Y, nx, ny)             # back
        self.grid(lo, Z, Y, nz, ny)                 # left
        self.grid(lo + X, Y, Z, ny, nz)             # right

    def cylinder(self, center, r, y0, y1, seg, rings):
        th = np.linspace(0, 2 * np.pi, seg, endpoint=False)
        ys = np.linspace(y0, y1, rings + 1)
        P = np.stack([center[0] + r * np.cos(th)[None, :].repeat(rings + 1, 0),
                      ys[:, None].repeat(seg, 1),
                      center[1] + r * np.sin(th)[None, :].repeat(rings + 1, 0)], -1).reshape(-1, 3)
        idx = np.arange((rings + 1) * seg).reshape(rings + 1, seg)
        a, b = idx[:-1], np.roll(idx[:-1], -1, axis=1)
        c, d = np.roll(idx[1:], -1, axis=1), idx[1:]
        f = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([a, d, c], -1).reshape(-1, 3)])
        self.add(P, f)

    def arch(self, x0, x1, y_base, z0, z1, thick, seg):
        """Semicircular arch band between x0 and x1 (extruded along z)."""
        cx, R = 0.5 * (x0 + x1), 0.5 * (x1 - x0)
        th = np.linspace(np.pi, 0, seg + 1)
        ring = []
        for rad in (R, R + thick):
            for z in (z0, z1):
                ring.append(np.stack([cx + rad * np.cos(th), y_base + rad * np.sin(th), np.full_like(th, z)], -1))
        # ring order: inner-z0, inner-z1, outer-z0, outer-z1
        base = self.nv
        P = np.concatenate(ring)
        n = seg + 1
        f = []
        for (p, q) in ((0, 1), (3, 2), (2, 0), (1, 3)):   # inner, outer, face z0, face z1
            i = np.arange(seg)
            a, b = p * n + i, p * n + i + 1
            c, d = q * n + i + 1, q * n + i
            f.append(np.stack([a, b, c], -1))
            f.append(np.stack([a, c, d], -1))
        self.v.append(P)
        self.f.append(np.concatenate(f) + base)
        self.nv += len(P)

    def arrays(self):
        return np.concatenate(self.v), np.concatenate(self.f)


def _jitter(verts, seed, amp):
    rng = np.random.default_rng(seed)
    return verts + rng.uniform(-amp, amp, size=verts.shape)


def sponza_standin(detail=1.0):
    """Closed-wall atrium with two storeys of colonnades, arches, gallery slabs and
    hanging banners (~66 k triangles at detail=1).  Units and extent follow the
    Sponza camera of src/assignment2.h:357-368."""
    m = _Mesh()
    k = lambda n: max(1, int(round(n * detail)))
    # floor and outer walls
    m.grid((-15, 0, -7), (30, 0, 0), (0, 0, 14), k(118), k(56))
    m.grid((-15, 0, -7), (0, 13, 0), (30, 0, 0), k(26), k(60))
    m.grid((-15, 0, 7), (30, 0, 0), (0, 13, 0), k(60), k(26))
    m.grid((-15, 0, -7), (0, 0, 14), (0, 13, 0), k(28), k(26))
    m.grid((15, 0, -7), (0, 13, 0), (0, 0, 14), k(26), k(28))
    for side in (-1, 1):
        zc = 4.0 * side
        # ground-floor colonnade + arches
        xs = -12.5 + 2.5 * np.arange(11)
        for x in xs:
            m.cylinder((x, zc), 0.32, 0.35, 4.2, k(20), k(12))
            m.box((x - 0.45, 0.0, zc - 0.45), (x + 0.45, 0.35, zc + 0.45))
            m.box((x - 0.45, 4.2, zc - 0.45), (x + 0.45, 4.5, zc + 0.45))
        for x0, x1 in zip(xs[:-1], xs[1:]):
            m.arch(x0 + 0.3, x1 - 0.3, 4.5, zc - 0.3, zc + 0.3, 0.3, k(24))
        # gallery slab over the aisle
        zlo, zhi = (4.3, 7.0) if side > 0 else (-7.0, -4.3)
        m.box((-15, 5.6, zlo), (15, 5.9, zhi), (k(60), 1, k(6)))
        # upper colonnade + arches
        xs2 = -13.0 + 2.0 * np.arange(14)
        for x in xs2:
            m.cylinder((x, zc), 0.22, 5.9, 9.2, k(16), k(12))
        for x0, x1 in zip(xs2[:-1], xs2[1:]):
            m.arch(x0 + 0.2, x1 - 0.2, 9.2, zc - 0.2, zc + 0.2, 0.25, k(20))
        # banners hanging from the gallery edge (wavy sheets)
        for j, x in enumerate((-9.0, -3.0, 3.0, 9.0)):
            nu, nvv = k(20), k(40)
            s = np.linspace(0, 1, nu + 1)
            t = np.linspace(0, 1, nvv + 1)
            S, T = np.meshgrid(s, t, indexing="ij")
            X = x - 0.8 + 1.6 * S
            Y = 9.0 - 6.5 * T
            Z = zc - 0.5 * side + 0.25 * np.sin(6.0 * S + 3.0 * T + j) * T
            P = np.stack([X, Y, Z], -1).reshape(-1, 3)
            idx = np.arange((nu + 1) * (nvv + 1)).reshape(nu + 1, nvv + 1)
            a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
            f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
            m.add(P, f)
    v, f = m.arrays()
    v = _jitter(v, 20110601, 1e-3)
    return v, f


def bunny_standin(nu=250, nv=140, radius=3.0):
    """Seeded displaced sphere standing in for bunny.obj (~69.5 k tris, smooth normals)."""
    th = np.linspace(0, np.pi, nv + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, nu, endpoint=False)
    T, Ph = np.meshgrid(th, ph, indexing="ij")
    dirs = np.stack([np.sin(T) * np.cos(Ph), np.cos(T), np.sin(T) * np.sin(Ph)], -1)
    rng = np.random.default_rng(1994)
    freq = rng.uniform(1.5, 5.0, (6, 3))
    phase = rng.uniform(0, 2 * np.pi, 6)
    disp = sum(0.035 * np.sin(dirs @ freq[i] * 2.0 + phase[i]) for i in range(6))
    Rr = radius * (1.0 + disp)
    P = dirs * Rr[..., None] + np.array([0.0, radius + 0.05, 0.0])
    P = P.reshape(-1, 3)
    top = np.array([[0.0, 2 * radius + 0.05, 0.0]])
    bot = np.array([[0.0, 0.05, 0.0]])
    V = np.concatenate([P, top, bot])
    ring = lambda r: r * nu + np.arange(nu)
    f = []
    for r in range(nv - 2):
        a, b = ring(r), ring(r) + 1 - nu * ((np.arange(nu) + 1) // nu)
        c, d = ring(r + 1) + 1 - nu * ((np.arange(nu) + 1) // nu), ring(r + 1)
        f.append(np.stack([a, b, c], -1))
        f.append(np.stack([a, c, d], -1))
    it, ib = len(P), len(P) + 1
    r0 = ring(0)
    f.append(np.stack([np.full(nu, it), r0 - nu * 0 + 0, np.roll(r0, -1)], -1)[:, [0, 2, 1]])
    rl = ring(nv - 2)
    f.append(np.stack([np.full(nu, ib), rl, np.roll(rl, -1)], -1))
    F = np.concatenate(f)
    # smooth normals: area-weighted vertex normals
    e1 = V[F[:, 1]] - V[F[:, 0]]
    e2 = V[F[:, 2]] - V[F[:, 0]]
    fn = np.cross(e1, e2)
    N = np.zeros_like(V)
    for k in range(3):
        np.add.at(N, F[:, k], fn)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    V = _jitter(V, 1994, 1e-4)
    return V, F, N


def _smooth_normals(V, F):
    e1 = V[F[:, 1]] - V[F[:, 0]]
    e2 = V[F[:, 2]] - V[F[:, 0]]
    fn = np.cross(e1, e2)
    N = np.zeros_like(V)
    for k in range(3):
        np.add.at(N, F[:, k], fn)
    return N / np.linalg.norm(N, axis=1, keepdims=True)


def _tube(center, radius, n_ring):
    """Closed tube around a closed polyline `center` (n, 3) with per-sample radius."""
    n = len(center)
    t = np.roll(center, -1, 0) - np.roll(center, 1, 0)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    a = np.cross(t, np.array([0.0, 1.0, 0.3]))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = np.cross(t, a)
    ang = np.linspace(0, 2 * np.pi, n_ring, endpoint=False)
    V = (center[:, None, :] + radius[..., None] * (np.cos(ang)[None, :, None] * a[:, None, :] +
                                                   np.sin(ang)[None, :, None] * b[:, None, :])).reshape(-1, 3)
    i = np.arange(n)[:, None]
    j = np.arange(n_ring)[None, :]
    v00, v01 = i * n_ring + j, i * n_ring + (j + 1) % n_ring
    v10, v11 = ((i + 1) % n) * n_ring + j, ((i + 1) % n) * n_ring + (j + 1) % n_ring
    F = np.concatenate([np.stack([v00, v10, v11], -1).reshape(-1, 3), np.stack([v00, v11, v01], -1).reshape(-1, 3)])
    return V, F


def dragon_standin(n_len=800, n_ring=64):
    """Seeded (2,3) torus-knot tube with a bumpy, tapering radius standing in for
    dragon_2.obj (~102 k tris, smooth normals), about 2 units across, resting on y = 0."""
    u = np.linspace(0, 2 * np.pi, n_len, endpoint=False)
    r = 0.6 + 0.25 * np.cos(3 * u)
    c = np.stack([r * np.cos(2 * u), 0.25 * np.sin(3 * u), r * np.sin(2 * u)], -1) * 1.2
    rng = np.random.default_rng(2002)
    k = rng.uniform(3, 9, 4)
    ph = rng.uniform(0, 2 * np.pi, 4)
    rad = 0.16 + 0.05 * np.sin(u * 2 + 0.5) + sum(0.012 * np.sin(k[i] * u * 3 + ph[i]) for i in range(4))
    rad = np.broadcast_to(rad[:, None], (n_len, n_ring))
    V, F = _tube(c, rad, n_ring)
    V[:, 1] -= V[:, 1].min() - 0.01
    N = _smooth_normals(V, F)
    return _jitter(V, 2002, 1e-4), F, N


def buddha_standin(nu=500, nv=250):
    """Seeded seated-figure stand-in for buddha_smooth.obj: a displaced,
    vertically stretched sphere with a narrower upper half (~248 k tris,
    smooth normals), about 1.6 units wide and 2.4 tall, resting on y = 0."""
    V, F, _ = bunny_standin(nu, nv, radius=1.0)
    y = V[:, 1] / V[:, 1].max()
    squeeze = 0.8 - 0.25 * np.clip(y - 0.45, 0.0, 1.0) + 0.1 * np.exp(-((y - 0.85) / 0.08) ** 2)
    V = V * np.stack([squeeze, np.full_like(y, 1.2), squeeze], -1)
    V[:, 1] -= V[:, 1].min() - 0.01
    N = _smooth_normals(V, F)
    return _jitter(V, 1993, 1e-4), F, N


def buddha_full_standin():
    """buddha_standin at the size of buddha_smooth.obj (1,087,716 tris): 1,090,980
    triangles -- the host-build throughput case."""
    return buddha_standin(nu=1045, nv=523)


def instance_transforms(n=64, grid=8, spacing=3.2, seed=64):
    """Row-major 4x4 ProxyObject transforms of config C5: an n = grid x grid
    layout, seeded rotation about y, uniform scale 0.8-1.2 and jitter."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        gx, gz = i % grid, i // grid
        a = rng.uniform(0, 2 * np.pi)
        s = rng.uniform(0.8, 1.2)
        tx = (gx - (grid - 1) / 2) * spacing + rng.uniform(-0.4, 0.4)
        tz = -(gz - (grid - 1) / 2) * spacing + rng.uniform(-0.4, 0.4)
        c, sn = np.cos(a), np.sin(a)
        out.append(np.array([[c * s, 0, sn * s, tx], [0, s, 0, 0], [-sn * s, 0, c * s, tz], [0, 0, 0, 1]], np.float32))
    return out


def _cached(name, builder):
    key = hashlib.sha1(f"{name}-{SCENE_VERSION}".encode()).hexdigest()[:10]
    path = os.path.join(_cache_dir(), f"{name}-{key}.obj")
    if not os.path.exists(path):
        out = builder()
        if len(out) == 3:
            write_obj(path, out[0], out[1], out[2])
        else:
            write_obj(path, out[0], out[1])
    return path


def sponza_obj():
    return _cached("sponza_standin", sponza_standin)


def sponza_large_obj():
    """The 262 k-triangle Sponza variant (Crytek Sponza is 262,267
    triangles): the same atrium at detail 2.03, 261,788 triangles, a ~16 MB hierarchy
    -- beyond one XCD's 4 MB L2."""
    return _cached("sponza_large_standin", lambda: sponza_standin(2.03))


def bunny_obj():
    return _cached("bunny_standin", bunny_standin)


def dragon_obj():
    return _cached("dragon_standin", dragon_standin)


def buddha_obj():
    return _cached("buddha_standin", buddha_standin)


def buddha_full_obj():
    return _cached("buddha_full_standin", buddha_full_standin)


def mesh_obj(cfg):
    """OBJ path of a single-mesh config (sponza, sponza_large, bunny)."""
    return {"sponza": sponza_obj, "sponza_large": sponza_large_obj, "bunny": bunny_obj}[cfg["mesh"]]()


def proto_objs(cfg):
    """The two ProxyObject meshes of an instanced config: the dragon stand-in and the
    buddha stand-in, at buddha_smooth.obj's size (1,087,716 triangles) when the config
    says buddha="full"."""
    return dragon_obj(), (buddha_full_obj() if cfg.get("buddha") == "full" else buddha_obj())


def sky_rgb(W=512, H=256):
    """Deterministic lat-long sky for the dome-light / environment-map configs
    (the reference's Images/*.hdr do not travel to the GPU box).  Same mapping
    as Texture::getLookupXYZ3 (src/Texture.cpp:80-98): row 0 = +y (zenith),
    column u = (atan2(z, x) + pi) / 2pi.  A blue sky brightening towards the
    horizon, a warm sun disc with a glow, and a darker ground; float32 (H, W, 3)."""
    v = (np.arange(H, dtype=np.float64) + 0.5) / H
    u = (np.arange(W, dtype=np.float64) + 0.5) / W
    phi = v * np.pi                                   # polar angle from +y
    theta = u * 2.0 * np.pi - np.pi                   # atan2(z, x)
    y = np.broadcast_to(np.cos(phi)[:, None], (H, W))
    s = np.sin(phi)[:, None]
    x = s * np.cos(theta)[None, :]
    z = s * np.sin(theta)[None, :]
    up = np.clip(y, 0.0, 1.0)[..., None]
    sky = np.array([0.35, 0.55, 1.0]) * (0.35 + 0.65 * (1.0 - up)) + np.array([0.25, 0.3, 0.45]) * up
    ground = np.broadcast_to(np.array([0.16, 0.14, 0.11]), (H, W, 3))
    rgb = np.where((y >= 0.0)[..., None], sky, ground)
    sun = np.array([0.45, 0.75, 0.48])
    sun /= np.linalg.norm(sun)
    c = x * sun[0] + y * sun[1] + z * sun[2]
    glow = 40.0 * (c > np.cos(np.radians(2.5))) + 3.0 * np.clip(c, 0.0, 1.0) ** 64
    rgb = rgb + glow[..., None] * np.array([1.0, 0.9, 0.72])
    return np.ascontiguousarray(rgb, np.float32)


def env_image(spec, hdr_loader=None):
    """(H, W, 3) float32 lat-long image of a config's sky spec: a name in SKIES
    (a Radiance .hdr decoded by `hdr_loader(path)`, default libmrt's
    HDRLoader::load restatement) or a (W, H) tuple (the procedural sky_rgb)."""
    if isinstance(spec, str):
        path = SKIES[spec]
        if hdr_loader is None:
            import miro
            img = miro.RawImage()
            img.loadHDR(path)
            return img.m_rawData
        return hdr_loader(path)
    return sky_rgb(*spec)


# ---------------------------------------------------------------- presets
CONFIGS = {
    # C1: cornell_box.obj 256x256, 1 spp, Lambert + 1 PointLight (plumbing)
    "C1": dict(name="cornell_box.obj 256x256 Lambert+PointLight", W=256, H=256,
               camera=dict(eye=(2.75, 2.75, 5.0), lookAt=(2.75, 2.75, 0.0), up=(0, 1, 0), fov=55.0),
               lights=[dict(type="point", pos=(2.75, 5.0, -2.75), power=40.0)],
               material=dict(kind="lambert", kd=(1, 1, 1)), bg=(0.0, 0.0, 0.2), mesh="cornell"),
    # C2: bunny stand-in 1024x1024, Blinn kd=1, PointLight (10,20,10) 1000, floor triangle
    "C2": dict(name="bunny stand-in (69.5k tris) 1024x1024 Blinn+PointLight", W=1024, H=1024,
               camera=dict(eye=(0.0, 5.0, 15.0), lookAt=(0.0, 0.0, 0.0), up=(0, 1, 0), fov=45.0),
               lights=[dict(type="point", pos=(10.0, 20.0, 10.0), power=1000.0)],
               material=dict(kind="blinn", kd=(1, 1, 1)), bg=(0.0, 0.0, 0.2), mesh="bunny",
               # bench.py frames in flight (one HIP stream and hardware queue each): the frame's latency is set by
               # a few heavy top-row tiles, so 4 in flight cap the step at latency / 4 (walk exit)
               inflight=8,
               # the frame kernel at 6 waves per SIMD: 6% faster here than the default 7 (C3 / C3L: 7 faster by
               # 1-2%; profiles/r06_walk_latch_ab.txt)
               tune={"frame1_waves": 6}),
    # C3: Sponza stand-in 1920x1080, Blinn kd=1, PointLight (0,10,0) 200
    "C3": dict(name="sponza stand-in (~66k tris) 1920x1080 Blinn+PointLight", W=1920, H=1080,
               camera=dict(eye=(8.0, 1.5, 1.0), lookAt=(0.0, 2.5, -1.0), up=(0, 1, 0), fov=55.0),
               lights=[dict(type="point", pos=(0.0, 10.0, 0.0), power=200.0)],
               material=dict(kind="blinn", kd=(1, 1, 1)), bg=(0.0, 0.0, 0.2), mesh="sponza",
               # the frame kernel's camera-ray walk with nested latches: 1.5% faster here than one
               # latch, which the other scenes run (C2 -11%, C3L -4.4%; DESIGN.md §4, walk latches)
               tune={"walk_latch": 0}),
    # C3L: C3 on the 262 k-triangle Sponza variant ("also a 262 k
    # variant"; Crytek Sponza's size): its ~16 MB hierarchy does not fit one XCD's L2
    "C3L": dict(name="sponza stand-in, 262k variant (261,788 tris) 1920x1080 Blinn+PointLight", W=1920, H=1080,
                camera=dict(eye=(8.0, 1.5, 1.0), lookAt=(0.0, 2.5, -1.0), up=(0, 1, 0), fov=55.0),
                lights=[dict(type="point", pos=(0.0, 10.0, 0.0), power=200.0)],
                material=dict(kind="blinn", kd=(1, 1, 1)), bg=(0.0, 0.0, 0.2), mesh="sponza_large"),
    # A3: C3 with adaptive supersampling as the Assignment 3 scenes set it
    # (m_minSubdivs = 1, m_maxSubdivs = 4, src/Assignment3.h:31-32; noise 0.01,
    # src/Scene.cpp:20): Scene::adaptiveSampleScene, 5 to 30 eye rays per pixel
    "A3": dict(name="sponza stand-in (~66k tris) 1920x1080 Blinn+PointLight, adaptive supersampling 1..4 subdivs",
               W=1920, H=1080,
               camera=dict(eye=(8.0, 1.5, 1.0), lookAt=(0.0, 2.5, -1.0), up=(0, 1, 0), fov=55.0),
               lights=[dict(type="point", pos=(0.0, 10.0, 0.0), power=200.0)],
               material=dict(kind="blinn", kd=(1, 1, 1)), bg=(0.0, 0.0, 0.2), mesh="sponza",
               subdivs=(1, 4, 0.01)),
    # R3: C3 with Whitted-style secondary rays: a Blinn material that reflects
    # (reflectAmt 0.5) and refracts (refractAmt 0.5, ior 1.5), Blinn::shade's
    # Fresnel-weighted roulette between direct light and one secondary ray per
    # level, up to 5 bounces (src/Blinn.cpp:180-330)
    "R3": dict(name="sponza stand-in (~66k tris) 1920x1080 Blinn reflect+refract (Fresnel roulette, 5 bounces)+PointLight",
               W=1920, H=1080,
               camera=dict(eye=(8.0, 1.5, 1.0), lookAt=(0.0, 2.5, -1.0), up=(0, 1, 0), fov=55.0),
               lights=[dict(type="point", pos=(0.0, 10.0, 0.0), power=200.0)],
               material=dict(kind="blinn", kd=(1, 1, 1), reflectAmt=0.5, refractAmt=0.5, ior=1.5),
               bg=(0.0, 0.0, 0.2), mesh="sponza"),
    # G3: R3's Fresnel glass made dispersive with the Assignment 3 prism IORs
    # (src/Assignment3.h:169-177: m_disperse, m_ior 1.57 / 1.60 / 1.62) under adaptive
    # supersampling 1..3 (the reference's final scene supersamples its dispersive glass,
    # src/main.cpp:143-174): the fused tree walk (dispersion splits) in adaptive_kernel
    "G3": dict(name="sponza stand-in (~66k tris) 1920x1080 dispersive Blinn glass (m_ior 1.57/1.60/1.62) "
                    "+ adaptive supersampling 1..3 + PointLight",
               W=1920, H=1080,
               camera=dict(eye=(8.0, 1.5, 1.0), lookAt=(0.0, 2.5, -1.0), up=(0, 1, 0), fov=55.0),
               lights=[dict(type="point", pos=(0.0, 10.0, 0.0), power=200.0)],
               material=dict(kind="blinn", kd=(1, 1, 1), reflectAmt=0.5, refractAmt=0.5, ior=1.60,
                             disperse=True, ior3=(1.57, 1.60, 1.62)),
               bg=(0.0, 0.0, 0.2), mesh="sponza", subdivs=(1, 3, 0.01)),
    # C4: Sponza stand-in, RectangleLight (8,10,2)/(8,10,-2)/(-8,10,2) power 1.5 and
    # Scene::m_numPaths = 16 (makeSponzaScenePathTrace, src/assignment2.h:663-708, direct
    # lighting only): 16 shade() calls per hit, one area-light shadow ray each;
    # Blinn with a specular lobe (specAmt > 0)
    "C4": dict(name="sponza stand-in (~66k tris) 1920x1080 Blinn+RectangleLight, 16 paths", W=1920, H=1080,
               camera=dict(eye=(8.0, 1.5, 1.0), lookAt=(0.0, 2.5, -1.0), up=(0, 1, 0), fov=55.0),
               lights=[dict(type="rect", v1=(8.0, 10.0, 2.0), v2=(8.0, 10.0, -2.0), v3=(-8.0, 10.0, 2.0),
                            power=1.5, samples=1, noise=0.001)],
               material=dict(kind="blinn", kd=(1, 1, 1), specExp=8.0, specAmt=0.25), bg=(0.0, 0.0, 0.2),
               mesh="sponza", num_paths=16, inflight=8),   # 8 frames in flight: -3.5% per step (r06 hwq2)
    # C5: dragon + buddha stand-ins instanced 64x via ProxyObject (two BLASes,
    # alternating, seeded transforms) on a floor triangle, 3840x2160, DomeLight (power
    # 0.15, 6 samples, src/main.cpp:157-165) over Images/Arches_E_PineTree.hdr, the same
    # map as environment on missed rays; Blinn with a specular lobe
    "C5": dict(name="dragon (102k tris) + buddha (1.09M tris) stand-ins instanced 64x (ProxyObject) 3840x2160, DomeLight "
                    "(Arches_E_PineTree.hdr) 6 samples + env map",
               W=3840, H=2160, camera=dict(eye=(0.0, 10.0, 27.0), lookAt=(0.0, 0.5, 0.0), up=(0, 1, 0), fov=45.0),
               lights=[dict(type="dome", sky="arches", power=0.15, samples=6, noise=0.001)],
               env=dict(sky="arches", exposure=1.0),
               material=dict(kind="blinn", kd=(0.8, 0.8, 0.8), specExp=20.0, specAmt=0.3), bg=(0.0, 0.0, 0.2),
               mesh="instances", instances=dict(n=64, grid=8, spacing=3.2, seed=64), buddha="full"),
    # D1: image-based lighting on the C2 bunny stand-in + floor: DomeLight (power
    # 0.15, 6 samples, as src/main.cpp:157-165) over Images/Arches_E_PineTree.hdr, the
    # same map as environment on missed primary rays; Blinn with a specular lobe
    "D1": dict(name="bunny stand-in + floor 1024x1024 Blinn+DomeLight (Arches_E_PineTree.hdr, 6 samples) + env map",
               W=1024, H=1024,
               camera=dict(eye=(0.0, 5.0, 15.0), lookAt=(0.0, 0.0, 0.0), up=(0, 1, 0), fov=45.0),
               lights=[dict(type="dome", sky="arches", power=0.15, samples=6, noise=0.001)],
               env=dict(sky="arches", exposure=1.0),
               material=dict(kind="blinn", kd=(0.8, 0.8, 0.8), specExp=20.0, specAmt=0.3), bg=(0.0, 0.0, 0.2),
               mesh="bunny"),
    # P4: makeSponzaScenePathTrace (src/assignment2.h:663-710) as written: 512x512,
    # Scene::m_pathTrace with m_numPaths = 16 and m_maxBounces = 10, RectangleLight
    # (8,10,2)/(8,10,-2)/(-8,10,2) power 1.5, Models/sponza-light.obj as an emissive
    # Blinn (setLightEmittedIntensity 1.5, colour 1), Blinn kd = 1 on the Sponza stand-in
    "P4": dict(name="sponza stand-in (~66k tris) 512x512 path tracing (16 paths, 10 bounces) + RectangleLight "
                    "+ emissive sponza-light.obj", W=512, H=512,
               camera=dict(eye=(8.0, 1.5, 1.0), lookAt=(0.0, 2.5, -1.0), up=(0, 1, 0), fov=55.0),
               lights=[dict(type="rect", v1=(8.0, 10.0, 2.0), v2=(8.0, 10.0, -2.0), v3=(-8.0, 10.0, 2.0),
                            power=1.5, samples=1, noise=0.001)],
               extra=[("sponza_light", dict(kind="blinn", kd=(1, 1, 1), emitted=1.5, le=(1, 1, 1)))],
               material=dict(kind="blinn", kd=(1, 1, 1)), bg=(0.0, 0.0, 0.2), mesh="sponza", num_paths=16,
               path_trace=(10, False)),
    # FS: the reference's own final scene (makeFinalScene, src/main.cpp:132-670; miro/final_scene.py):
    # dispersive MB glass, MB cannonball, DOF, dome light + env map, alpha-mapped translucent
    # leaves in proxies, flowers, 40,401 grass proxies, adaptive supersampling 3..5.  The
    # published render ("20 minutes on an i7 quadcore", webpage/aguzman_jschwarzhaupt.html:147)
    # is 1904 x 1042.
    "FS": dict(name="makeFinalScene (src/main.cpp:132-670) 1904x1042: dispersive MB glass, DOF, dome + env, "
                    "alpha leaves in proxies, 42k instances, adaptive 3..5",
               W=1904, H=1042, mesh="final",
               camera=dict(eye=(-1.277, 0.158, 2.139), lookAt=(0.294, 0.511, 0.503), up=(0, 1, 0), fov=39.0,
                           aperture=0.0018, focusPlane=2.0, shutterSpeed=0.1),
               lights=[dict(type="dome", sky="final_sky", power=0.15, samples=6)],
               material=dict(kind="blinn", kd=(0.9, 0.9, 0.9), specExp=30.0, reflectAmt=1.0, refractAmt=1.0,
                             ior3=(1.56, 1.5, 1.5), disperse=True),
               bg=(0.0, 0.0, 0.0), subdivs=(3, 5, 0.01)),
}


def camera_path(cam, n, step_deg=2.5):
    """n cameras panning from `cam` (a config camera dict): frame f turns the
    view direction by f * step_deg degrees about the up (y) axis around the
    fixed eye.  Frame 0 is `cam` itself.  Used for frame batches (bench.py at
    N > 1 renders N frames per step)."""
    eye = np.asarray(cam["eye"], np.float64)
    d = np.asarray(cam["lookAt"], np.float64) - eye
    out = []
    for f in range(n):
        a = np.deg2rad(step_deg * f)
        c, s = np.cos(a), np.sin(a)
        dd = np.array([c * d[0] + s * d[2], d[1], -s * d[0] + c * d[2]])
        out.append(dict(cam, lookAt=tuple(float(x) for x in (eye + dd)) if f else tuple(cam["lookAt"])))
    return out


EXTRA_OBJS = {"sponza_light": SPONZA_LIGHT_OBJ}


def sky_key(spec):
    return spec if isinstance(spec, str) else tuple(spec)


def make_material(mat):
    """miro material of a config's material dict (all of its Blinn settings)."""
    import miro
    if mat["kind"] == "lambert":
        return miro.Lambert(mat["kd"])
    m = miro.Blinn(mat["kd"], specExp=mat.get("specExp", 1.0), specAmt=mat.get("specAmt", 0.0),
                   reflectAmt=mat.get("reflectAmt", 0.0), refractAmt=mat.get("refractAmt", 0.0), ior=mat.get("ior", 1.5),
                   specGloss=mat.get("specGloss", 1.0))
    m.setTranslucency(mat.get("translucency", 0.0))
    m.setLightEmittedIntensity(mat.get("emitted", 0.0))
    m.setLightEmittedColor(mat.get("le", (0, 0, 0)))
    m.setSampleEnv(mat.get("sampleEnv", True))
    for i, v in enumerate(mat.get("ior3", ())):   # Blinn::setIor(ior, i), src/Blinn.h:38
        m.setIor(v, i)
    m.m_disperse = bool(mat.get("disperse", False))
    return m


def chain_level(cfg):
    """Which shading path libmrt takes for a config (Shader REC): 2 path tracing,
    1 reflection / refraction / gloss / translucency chains, 0 direct lighting."""
    if cfg.get("path_trace"):
        return 2
    for m in [cfg["material"]] + [e[1] for e in cfg.get("extra", ())]:
        if m["kind"] == "blinn" and (m.get("reflectAmt", 0) > 0 or m.get("refractAmt", 0) > 0
                                     or m.get("specGloss", 1.0) < 1.0 or m.get("translucency", 0) > 0.01):
            return 1
    return 0


def build_config(key, device=0):
    """Product-side scene for a config preset -> (miro.Scene, miro.Camera, cfg).
    C1 needs the Cornell mesh fixture path in MRT_CORNELL_NPZ (or tests/golden)."""
    import miro

    cfg = CONFIGS[key]
    if cfg["mesh"] == "final":   # the reference's final scene, from its own description
        from . import final_scene
        scene, cam = final_scene.build_product(final_scene.spec(), device=device)
        return scene, cam, cfg
    scene = miro.Scene(device=device)
    material = make_material(cfg["material"])
    mesh = miro.TriangleMesh()
    if cfg["mesh"] == "cornell":
        root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        npz = os.environ.get("MRT_CORNELL_NPZ", os.path.join(root, "tests", "golden", "cornell_box_mesh.npz"))
        f = np.load(npz)
        mesh.setArrays(f["verts"], f["normals"], f["vidx"], f["nidx"])
    elif cfg["mesh"] in ("sponza", "sponza_large", "bunny"):
        mesh.load(mesh_obj(cfg))
    if cfg["mesh"] != "instances":
        miro.makeMeshObjs(scene, mesh, material)
    else:  # two ProxyObject BVHs, 64 instances alternating (src/main.cpp proxy scenes)
        protos = []
        for path in proto_objs(cfg):
            tm = miro.TriangleMesh()
            tm.load(path)
            objs, bvh = miro.Objects(), miro.BVH()
            miro.ProxyObject.setupProxy(tm, material, objs, bvh)
            protos.append((objs, bvh))
        for i, M in enumerate(instance_transforms(**cfg["instances"])):
            objs, bvh = protos[i % 2]
            scene.addObject(miro.ProxyObject(objs, bvh, miro.Matrix4x4(M)))
    for name, emat in cfg.get("extra", ()):   # e.g. the emissive light panel of P4
        tm = miro.TriangleMesh()
        tm.load(EXTRA_OBJS[name])
        miro.makeMeshObjs(scene, tm, make_material(emat))
    if cfg["mesh"] in ("bunny", "instances"):  # floor triangle, src/assignment2.h:110-124
        fl = miro.TriangleMesh()
        fl.createSingleTriangle()
        fl.setV1((-100, 0, -100)); fl.setV2((0, 0, 100)); fl.setV3((100, 0, -100))
        fl.setN1((0, 1, 0)); fl.setN2((0, 1, 0)); fl.setN3((0, 1, 0))
        miro.makeMeshObjs(scene, fl, material)
    skies = {}

    def sky_texture(spec):
        if spec not in skies:
            rgb = env_image(spec)
            skies[spec] = miro.Texture(miro.RawImage(rgb.shape[1], rgb.shape[0], rgb))
        return skies[spec]

    for l in cfg["lights"]:
        if l["type"] == "point":
            pl = miro.PointLight()
            pl.setPosition(l["pos"])
        elif l["type"] == "dome":
            pl = miro.DomeLight()
            pl.setTexture(sky_texture(sky_key(l["sky"])))
            pl.setSamples(l.get("samples", 1))
            pl.setNoiseThreshold(l.get("noise", 0.001))
        else:
            pl = miro.RectangleLight()
            pl.setVertices(l["v1"], l["v2"], l["v3"])
            pl.setSamples(l.get("samples", 1))
            pl.setNoiseThreshold(l.get("noise", 0.001))
        pl.setPower(l["power"])
        scene.addLight(pl)
    scene.setBGColor(cfg["bg"])
    if cfg.get("env"):
        scene.setEnvMap(sky_texture(sky_key(cfg["env"]["sky"])))
        scene.setEnvExposure(cfg["env"]["exposure"])
    scene.setNumPaths(cfg.get("num_paths", 1))
    if cfg.get("path_trace"):
        scene.setPathTrace(True)
        scene.setMaxBounces(cfg["path_trace"][0])
        scene.setSampleEnv(cfg["path_trace"][1])
    if cfg.get("subdivs"):
        lo, hi, noise = cfg["subdivs"]
        scene.setMinSubdivs(lo); scene.setMaxSubdivs(hi); scene.setNoise(noise)
    scene.preCalc()
    cam = miro.Camera()
    c = cfg["camera"]
    cam.setEye(c["eye"]); cam.setLookAt(c["lookAt"]); cam.setUp(c["up"]); cam.setFOV(c["fov"])
    return scene, cam, cfg
